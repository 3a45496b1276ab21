"""Float64 NumPy restatement of the online overdetermined AuxIVA of csrc/overiva.hip (include/misonet.h, "online OverIVA";
INTEGRATION.md 4w), vectorised over the items and the bins, with explicit loops for the eliminations.  The project's own
definition in the OverIVA family (Scheibler & Ono, WASPAA 2019) in frame-recursive form; pyroomacoustics and torchiva were not
available and were not compared.  The helpers (``_sum``, ``_matvec``, ``_matmul``, ``solve``, ``pieces``, ``rel``) and the bar
rule are those of tests/oiva_ref.py.

K sources at M microphones, 2 <= M <= 8, 1 <= K <= M - 1.  State per (item b, bin f): Ws [K, M] (row k = w_k^H, y = Ws x),
J [M - K, K], V [K, M, M] (one Hermitian matrix per source), C [M, M] (Hermitian, the recursive mixture covariance), n, fail.
The full demixing matrix is W = [Ws ; J, -I].  ``reset``: Ws = [I 0], J = 0, V_k = init I, C = init I, n = 0, fail = 0.  Per new
frame, x_f the M samples of bin f:

    0. a bin whose frame holds a non-finite sample: fail |= 1, x_f = 0 in 1-2, step 3 skipped, its outputs of this frame 0
    1. yt_k[f] = sum_m Ws_f[k, m] x_f[m], m ascending, Ws as it stood before this frame
    2. r_k = sum_f |yt_k[f]|^2;  gauss phi_k = 1 / max(r_k / F, floor),  laplace phi_k = 1 / max(2 sqrt(r_k), floor)
    3. per bin:  C <- alpha C + (1 - alpha) x x^H           (lower triangle computed, the upper its mirror, the diagonal real)
       then for k = 0 .. K - 1 in order:
         V_k <- alpha V_k + (1 - alpha) phi_k x x^H          (the same rule)
         (W V_k) u = e_k                                     (the full M x M W as it stands; the elimination of oiva_ref.solve)
         d = Re(u^H V_k u)
         a pivot 0 or non-finite, d not finite or not > 0: row k stays, fail |= 2;  otherwise row k of Ws <- conj(u) / sqrt(d)
         J re-solved, after every k:  P = C Ws^H [M, K], P1 its first K rows, P2 its last M - K;  J P1 = P2 solved as
         P1^T J^T = P2^T by the same elimination;  a pivot 0 or non-finite: J stays, fail |= 8
    4. y = Ws x with the new Ws;  S = Ws[:, :K] + Ws[:, K:] J;  A_top = S^-1 by the same elimination (right-hand side I_K),
       A_bot = J A_top, A = [A_top; A_bot] (the first K columns of W^-1);  est[k] = A[ref_ch, k] y_k, images[k, m] = A[m, k] y_k,
       each rounded once to complex64;  S singular: fail |= 4, the outputs of this (f, t) are 0
    5. n <- min(n + 1, 2^31 - 1)

By construction [J, -I] C Ws^H = 0, Re(w_k^H V_k w_k) = 1 and W A = [I_K; 0].  sum_k images = x does NOT hold: the background is
what is left.

The device tests compare against this file; ``FAULTS`` are the planted mistakes that tests/test_overiva.py shows the device
tests' bars reject.
"""
import numpy as np

from oiva_ref import (BAR_CAP, MODELS, N_MAX, OUT_BAR, STATE_FLOOR, _matmul, _matvec, _real, _sum, best_image_sdr, hermitian,
                      pieces, rel, solve, to_stream)

FAULTS = ("j_once_per_frame", "j_from_v0", "c_weighted_by_phi", "identity_padding", "a_bot_dropped", "proj_mic0", "float32_d")
PARTS = ("Ws", "J", "V", "C")


class State:
    """the state of B x F bins"""

    def __init__(self, B, M, K, F, alpha=0.98, model="gauss", floor=1e-10, init=1.0, ref_ch=0, dtype=np.complex128):
        if not (2 <= M <= 8 and 1 <= K <= M - 1):
            raise ValueError(f"2 <= M <= 8 and 1 <= K <= M - 1, got M {M}, K {K}")
        self.B, self.M, self.K, self.F = B, M, K, F
        self.alpha, self.model, self.floor, self.init, self.ref_ch, self.dtype = alpha, model, floor, init, ref_ch, dtype
        self.reset()

    def reset(self):
        B, M, K, F = self.B, self.M, self.K, self.F
        i, k = np.arange(M), np.arange(K)
        self.Ws = np.zeros((B, F, K, M), self.dtype)
        self.Ws[:, :, k, k] = 1.0
        self.J = np.zeros((B, F, M - K, K), self.dtype)
        self.V = np.zeros((B, F, K, M, M), self.dtype)
        self.V[:, :, :, i, i] = self.init
        self.C = np.zeros((B, F, M, M), self.dtype)
        self.C[:, :, i, i] = self.init
        self.n = np.zeros((B, F), np.int32)
        self.fail = np.zeros((B, F), np.int32)

    def copy(self):
        s = State.__new__(State)
        s.__dict__.update(self.__dict__)
        for k in PARTS + ("n", "fail"):
            setattr(s, k, getattr(self, k).copy())
        return s

    def full(self):
        """W = [Ws ; J, -I] [B, F, M, M]"""
        return full_w(self.Ws, self.J)


def full_w(Ws, J):
    K, M = Ws.shape[-2:]
    bottom = np.concatenate([J, np.broadcast_to(-np.eye(M - K, dtype=Ws.dtype), J.shape[:-2] + (M - K, M - K))], axis=-1)
    return np.concatenate([Ws, bottom], axis=-2)


def _hermitian_update(old, g, outer, alpha):
    di = np.arange(old.shape[-1])
    new = alpha * old + g[..., None, None] * outer
    new = np.tril(new) + np.conj(np.swapaxes(np.tril(new, -1), -1, -2))
    new[..., di, di] = new[..., di, di].real
    return new


def _solve_j(Cm, Ws, reverse):
    """J of J P1 = P2 with P = Cm Ws^H -> (J [..., M - K, K], bad [...])"""
    K = Ws.shape[-2]
    P = _matmul(Cm, np.conj(np.swapaxes(Ws, -1, -2)), reverse)                     # [.., M, K]
    Jt, bad = solve(np.swapaxes(P[..., :K, :], -1, -2), np.swapaxes(P[..., K:, :], -1, -2))
    return np.swapaxes(Jt, -1, -2), bad


def demix_inverse(Ws, J, reverse=False):
    """the first K columns of W^-1 -> (A [..., M, K], bad [...])"""
    K = Ws.shape[-2]
    Sm = Ws[..., :, :K] + _matmul(Ws[..., :, K:], J, reverse)
    top, bad = solve(Sm, np.broadcast_to(np.eye(K, dtype=Ws.dtype), Sm.shape))
    return np.concatenate([top, _matmul(J, top, reverse)], axis=-2), bad


def step(st, x, fault=None, reverse=False):
    """One frame.  x complex64 [B, M, F] -> (est [B, K, F], images [B, K, M, F]) in the State's dtype"""
    M, K, F, cdt = st.M, st.K, st.F, st.dtype
    rdt = _real(cdt)
    one = rdt.type(1.0)
    alpha, oma, floor = rdt.type(st.alpha), one - rdt.type(st.alpha), rdt.type(st.floor)
    x32 = np.asarray(x).astype(np.complex64)
    xv = np.moveaxis(x32, 1, 2).astype(cdt)                                        # [B, F, M]
    badin = ~(np.isfinite(xv.real) & np.isfinite(xv.imag)).all(-1)                 # [B, F]
    xv = np.where(badin[..., None], 0, xv)
    keep2 = badin[..., None, None]
    with np.errstate(all="ignore"):
        yt = _matvec(st.Ws, xv, reverse)                                           # [B, F, K]
        r = _sum(yt.real ** 2 + yt.imag ** 2, reverse, axis=1)[:, None, :]         # [B, 1, K]
        den = r / rdt.type(F) if st.model == "gauss" else rdt.type(2.0) * np.sqrt(r)
        phi = np.broadcast_to(one / np.maximum(den, floor), yt.shape)
        outer = xv[..., :, None] * np.conj(xv[..., None, :])
        gc = oma * phi[..., 0] if fault == "c_weighted_by_phi" else np.broadcast_to(oma, badin.shape)
        Cn = _hermitian_update(st.C, gc, outer, alpha)
        st.C = np.where(keep2, st.C, Cn)
        eye = np.eye(M, dtype=cdt)
        for k in range(K):
            Vn = _hermitian_update(st.V[:, :, k], oma * phi[..., k], outer, alpha)
            if fault == "identity_padding":
                Wf = full_w(st.Ws, np.zeros_like(st.J))
            else:
                Wf = st.full()
            u, sbad = solve(_matmul(Wf, Vn, reverse), np.broadcast_to(eye[:, k:k + 1], Vn.shape[:-1] + (1,)))
            u = u[..., 0]
            q = _matvec(Vn, u, reverse)
            d = _sum(u.real * q.real + u.imag * q.imag, reverse)
            if fault == "float32_d":
                d = d.astype(np.float32).astype(rdt)
            ok = ~sbad & np.isfinite(d) & (d > 0) & ~badin
            row = np.conj(u) / np.sqrt(d)[..., None]
            st.Ws[:, :, k] = np.where(ok[..., None], row, st.Ws[:, :, k])
            st.V[:, :, k] = np.where(keep2, st.V[:, :, k], Vn)
            st.fail |= np.where(~ok & ~badin, 2, 0).astype(np.int32)
            if fault == "j_once_per_frame" and k < K - 1:
                continue
            Jn, jbad = _solve_j(st.V[:, :, 0] if fault == "j_from_v0" else Cn, st.Ws, reverse)
            st.J = np.where((jbad | badin)[..., None, None], st.J, Jn)
            st.fail |= np.where(jbad & ~badin, 8, 0).astype(np.int32)
        y = _matvec(st.Ws, xv, reverse)
        A, abad = demix_inverse(st.Ws, st.J, reverse)                              # [B, F, M, K]
        if fault == "a_bot_dropped":
            A = A.copy()
            A[..., K:, :] = 0
        ref = 0 if fault == "proj_mic0" else st.ref_ch
        est = A[..., ref, :] * y                                                   # [B, F, K]
        img = np.swapaxes(A, -1, -2) * y[..., :, None]                             # [B, F, K, M]
    zero = badin | abad
    st.fail |= np.where(badin, 1, 0).astype(np.int32) | np.where(abad & ~badin, 4, 0).astype(np.int32)
    est = np.where(zero[..., None], 0, est)
    img = np.where(zero[..., None, None], 0, img)
    st.n = np.minimum(st.n.astype(np.int64) + 1, N_MAX).astype(np.int32)
    return np.moveaxis(est, 1, 2), np.moveaxis(img, 1, 3)


def process(st, block, fault=None, reverse=False):
    """block complex64 [B, M, T, F] -> (est complex64 [B, K, T, F], images complex64 [B, K, M, T, F])"""
    block = np.asarray(block)
    B, M, T, F = block.shape
    est = np.zeros((B, st.K, T, F), np.complex64)
    img = np.zeros((B, st.K, M, T, F), np.complex64)
    for t in range(T):
        e, i = step(st, block[:, :, t], fault, reverse)
        est[:, :, t] = e.astype(np.complex64)
        img[:, :, :, t] = i.astype(np.complex64)
    return est, img


def overiva(mix, num_src, alpha=0.98, model="gauss", floor=1e-10, init=1.0, ref_ch=0, cuts=None, fault=None, reverse=False,
            dtype=np.complex128):
    """The one-shot call: reset, then the stream in one piece or in the pieces ``cuts`` (lengths; the rest follows).  mix complex64
    [B, M, T, F] -> (est, images, State)"""
    mix = np.asarray(mix)
    B, M, T, F = mix.shape
    st = State(B, M, num_src, F, alpha, model, floor, init, ref_ch, dtype)
    est = np.zeros((B, num_src, T, F), np.complex64)
    img = np.zeros((B, num_src, M, T, F), np.complex64)
    for t0, t1 in pieces(T, cuts):
        est[:, :, t0:t1], img[:, :, :, t0:t1] = process(st, mix[:, :, t0:t1], fault, reverse)
    return est, img, st


def figures(mix, num_src, **kw):
    """The reference of one case and its bar: dict(est, images, st, ext, bar, own).  Ws, J, V and C are measured against the
    clongdouble run (``ext``); bar = max(100 x own, STATE_FLOOR), own = the larger of the rel-L2 distances float64 - clongdouble
    and float64 - reversed summation order over Ws, J, V and C: the rule of oiva_ref.figures."""
    est, img, st = overiva(mix, num_src, **kw)
    _, _, ext = overiva(mix, num_src, dtype=np.clongdouble, **kw)
    _, _, rev = overiva(mix, num_src, reverse=True, **kw)
    own = max(rel(getattr(st, p), getattr(o, p)) for p in PARTS for o in (ext, rev))
    return dict(est=est, images=img, st=st, ext=ext, bar=max(100.0 * own, STATE_FLOOR), own=own)


def orthogonality_error(Ws, J, Cm):
    """max |[J, -I] C Ws^H| over every entry of every bin"""
    P = np.asarray(Cm, np.complex128) @ np.conj(np.swapaxes(np.asarray(Ws, np.complex128), -1, -2))   # [.., M, K]
    K = Ws.shape[-2]
    return float(np.max(np.abs(np.asarray(J, np.complex128) @ P[..., :K, :] - P[..., K:, :])))


def unit_norm_error(Ws, V):
    """max over (b, f, k) of |Re(w_k^H V_k w_k) - 1| with w_k^H = row k of Ws"""
    w = np.conj(Ws)
    q = np.einsum("bfki,bfkij,bfkj->bfk", np.conj(w), V, w)
    return float(np.max(np.abs(q.real - 1.0)))


def inverse_error(Ws, J):
    """max |W A - [I_K; 0]| with A = the first K columns of W^-1 as step 4 forms them"""
    Ws, J = np.asarray(Ws, np.complex128), np.asarray(J, np.complex128)
    K, M = Ws.shape[-2:]
    A, _ = demix_inverse(Ws, J)
    want = np.zeros((M, K))
    want[np.arange(K), np.arange(K)] = 1.0
    return float(np.max(np.abs(full_w(Ws, J) @ A - want)))


def rejected(cand, ref):
    """what the device tests assert, as one predicate: True when a candidate dict(est, images, Ws, J, V, C, fail, n) misses any
    bar of the reference ``figures`` dict"""
    st, ext, bar = ref["st"], ref["ext"], ref["bar"]
    if not (np.array_equal(cand["fail"], st.fail) and np.array_equal(cand["n"], st.n)):
        return True
    if not (hermitian(cand["V"]) and hermitian(cand["C"])):
        return True
    return (rel(cand["est"], ref["est"]) > OUT_BAR or rel(cand["images"], ref["images"]) > OUT_BAR
            or any(rel(cand[p], getattr(ext, p)) > bar for p in PARTS))


def as_candidate(est, img, st):
    d = dict(est=est, images=img, fail=st.fail, n=st.n)
    d.update({p: getattr(st, p).astype(np.complex128) for p in PARTS})
    return d


# ---- the device cases: tests/test_gpu_overiva.py runs them, tests/test_overiva.py checks their bars on the CPU ------------------
PAIRS = [(M, K) for M in range(2, 9) for K in range(1, M)]                         # all 28
# (model, alpha, images, ref_ch at the last microphone (>= K) or at 0): both models, both alphas, with and without images
VARIANTS = [("gauss", 0.98, True, False), ("laplace", 0.96, False, True), ("gauss", 0.96, False, False),
            ("laplace", 0.98, True, True)]
# (B, M, K, T, F) -> the variants it runs with.  Every pair once at (1, 30, 2), the variants in turn; the other shapes with all
# (the long stream with the two that have images)
CASES = [((1, M, K, 30, 2), (VARIANTS[i % 4],)) for i, (M, K) in enumerate(PAIRS)]
CASES += [((2, 6, 2, 40, 5), tuple(VARIANTS)), ((1, 6, 2, 1, 1), tuple(VARIANTS)), ((1, 6, 2, 300, 5), (VARIANTS[0], VARIANTS[3]))]
NOISE = {}                                                                         # shape -> the generator's noise where 0.01 is not it


def edge_cases(P):
    """F = P - 1, P, P + 1 and 2 P + 1 at T = 6 for (M, K) = (2, 1) and (6, 2), P(M, K) = the bins one workgroup covers at once"""
    out = []
    for i, (M, K) in enumerate(((2, 1), (6, 2))):
        p = P(M, K)
        out += [((1, M, K, 6, F), (VARIANTS[(2 * i + n) % 4],)) for n, F in enumerate((p - 1, p, p + 1, 2 * p + 1))]
    return out


def ref_ch_of(shape, variant):
    return shape[1] - 1 if variant[3] else 0


def case_inputs(shape):
    return inputs(*shape, noise=NOISE.get(tuple(shape), 0.01))


def inputs(B, M, K, T, F, noise=0.01):
    """the device cases' input: K sources at M microphones in the stream layout [B, M, T, F]"""
    import iva_ref
    return to_stream(iva_ref.sparse_mixture(B, K, M, T, F, seed=B + M + K + T + F, noise=noise)[0])


def image_sdr_m0(images, truth_img, lo):
    """mean over the sources of the SDR of images [K, M, T, F] at microphone 0 against the true images
    (``sparse_mixture``'s [N, F, M, T] of one item) over the frames lo .., under the best assignment; dB"""
    truth = np.transpose(truth_img[:, :, 0, :], (0, 2, 1))[:, lo:]
    return float(np.mean(best_image_sdr(images[:, 0, lo:], truth)))
