"""Float64 NumPy restatement of the online AuxIVA of csrc/oiva.hip (include/misonet.h, "online AuxIVA"),
vectorised over the items and the bins, with explicit loops for the elimination.  The project's own definition in the
online-AuxIVA family (Taniguchi, Ono, Kawamura & Sagayama 2014); pyroomacoustics and torchiva were not available and were not
compared.

Determined case, K = M, 2 <= M <= 8.  State per (item b, bin f): W [M, M] (row k = w_k^H, y = W x), V [M, M, M] (one Hermitian
matrix per source), n, fail.  ``reset``: W = I, V_k = init I, n = 0, fail = 0.  Per new frame, x_f the M samples of bin f:

    0. a bin whose frame holds a non-finite sample: fail |= 1, x_f = 0 in 1-2, step 3 skipped, its outputs of this frame 0
    1. yt_k[f] = sum_m W_f[k, m] x_f[m], m ascending, W as it stood before this frame
    2. r_k = sum_f |yt_k[f]|^2;  gauss phi_k = 1 / max(r_k / F, floor),  laplace phi_k = 1 / max(2 sqrt(r_k), floor)
    3. per bin, k = 0 .. M - 1 in order:
         V_k <- alpha V_k + (1 - alpha) phi_k x x^H        (lower triangle computed, the upper its mirror, the diagonal real)
         (W V_k) u = e_k                                    (W with the rows already replaced in this frame; Gaussian elimination
                                                             with partial pivoting: the pivot is the largest |re| + |im| of the
                                                             column, a non-finite one counting as the largest, ties to the lower
                                                             row; then back substitution)
         d = Re(u^H V_k u)
         a pivot 0 or non-finite, d not finite or not > 0: row k stays, fail |= 2;  otherwise row k of W <- conj(u) / sqrt(d)
    4. y = W x with the new W;  A = W^-1 by the same elimination (right-hand side I);  est[k] = A[ref_ch, k] y_k,
       images[k, m] = A[m, k] y_k, each rounded once to complex64;  W singular: fail |= 4, the outputs of this (f, t) are 0
    5. n <- min(n + 1, 2^31 - 1)

The device tests compare against this file; ``FAULTS`` are the planted mistakes that tests/test_oiva.py shows the device tests'
bars reject.
"""
import numpy as np

OUT_BAR = 2.4e-7            # 4 x 2^-24: one complex64 rounding of a float64 result (the bar of test_gpu_wpe.py)
STATE_FLOOR = 1e-12         # W and V: 100 x the restatement's own rounding figure on the case, never below this ...
BAR_CAP = 1e-6              # ... and a case whose bar would be above this is not a case
MODELS = ("gauss", "laplace")
FAULTS = ("phi_per_bin", "yt_new_w", "v_without_1_minus_alpha", "norm_uhu", "jacobi", "proj_mic0", "a_is_wh", "float32_d")
N_MAX = 0x7FFFFFFF


def _real(dtype):
    return np.empty(0, dtype).real.dtype


class State:
    """the state of B x F bins"""

    def __init__(self, B, M, F, alpha=0.98, model="gauss", floor=1e-10, init=1.0, ref_ch=0, dtype=np.complex128):
        self.B, self.M, self.F = B, M, F
        self.alpha, self.model, self.floor, self.init, self.ref_ch, self.dtype = alpha, model, floor, init, ref_ch, dtype
        self.reset()

    def reset(self):
        B, M, F = self.B, self.M, self.F
        i = np.arange(M)
        self.W = np.zeros((B, F, M, M), self.dtype)
        self.W[:, :, i, i] = 1.0
        self.V = np.zeros((B, F, M, M, M), self.dtype)
        self.V[:, :, :, i, i] = self.init
        self.n = np.zeros((B, F), np.int32)
        self.fail = np.zeros((B, F), np.int32)

    def copy(self):
        s = State.__new__(State)
        s.__dict__.update(self.__dict__)
        s.W, s.V, s.n, s.fail = self.W.copy(), self.V.copy(), self.n.copy(), self.fail.copy()
        return s


def _sum(terms, reverse, axis=-1):
    """plain partial sums along ``axis``, ascending (or descending) index"""
    terms = np.moveaxis(terms, axis, 0)
    acc = np.zeros(terms.shape[1:], terms.dtype)
    for i in (range(terms.shape[0] - 1, -1, -1) if reverse else range(terms.shape[0])):
        acc = acc + terms[i]
    return acc


def _matvec(A, v, reverse):
    """sum_m A[..., i, m] v[..., m]"""
    return _sum(A * v[..., None, :], reverse)


def _matmul(A, Bm, reverse):
    """sum_m A[..., i, m] B[..., m, c]"""
    return _sum(A[..., :, :, None] * Bm[..., None, :, :], reverse, axis=-2)


def solve(A, rhs):
    """Gaussian elimination with partial pivoting and back substitution, explicit loops.  A [..., M, M], rhs [..., M, R] ->
    (X [..., M, R], bad [...]): bad where a pivot was 0 or non-finite"""
    A, rhs = np.array(A), np.array(rhs)
    M = A.shape[-1]
    lead = A.shape[:-2]
    A, rhs = A.reshape((-1, M, M)), rhs.reshape((-1, M, rhs.shape[-1]))
    every = np.arange(A.shape[0])
    bad = np.zeros(A.shape[0], bool)
    with np.errstate(all="ignore"):
        for c in range(M):
            mag = np.abs(A[:, c:, c].real) + np.abs(A[:, c:, c].imag)
            mag = np.where(np.isfinite(mag), mag, np.inf)
            p = np.argmax(mag, axis=-1) + c                            # the first of equal ones: the lower row
            for Z in (A, rhs):
                rc, rp = Z[every, c].copy(), Z[every, p].copy()
                Z[every, c], Z[every, p] = rp, rc
            piv = A[:, c, c]
            pm = np.abs(piv.real) + np.abs(piv.imag)
            bad |= ~np.isfinite(pm) | (pm == 0)
            for i in range(c + 1, M):
                l = A[:, i, c] / piv
                A[:, i, c + 1:] -= l[:, None] * A[:, c, c + 1:]
                rhs[:, i] -= l[:, None] * rhs[:, c]
        X = np.zeros_like(rhs)
        for c in range(M - 1, -1, -1):
            X[:, c] = rhs[:, c] / A[:, c, c, None]
            for i in range(c):
                rhs[:, i] -= A[:, i, c, None] * X[:, c]
    return X.reshape(lead + X.shape[1:]), bad.reshape(lead)


def step(st, x, fault=None, reverse=False):
    """One frame.  x complex64 [B, M, F] -> (est [B, M, F], images [B, M(k), M, F]) in the State's dtype"""
    M, F, cdt = st.M, st.F, st.dtype
    rdt = _real(cdt)
    alpha, oma, floor = rdt.type(st.alpha), rdt.type(1.0) - rdt.type(st.alpha), rdt.type(st.floor)
    x32 = np.asarray(x).astype(np.complex64)
    xv = np.moveaxis(x32, 1, 2).astype(cdt)                                        # [B, F, M]
    badin = ~(np.isfinite(xv.real) & np.isfinite(xv.imag)).all(-1)                 # [B, F]
    xv = np.where(badin[..., None], 0, xv)
    W0 = st.W.copy()
    Wp = W0
    if fault == "yt_new_w":                                                        # the weights from this frame's own result
        trial = st.copy()
        step(trial, x, None, reverse)
        Wp = trial.W
    with np.errstate(all="ignore"):
        yt = _matvec(Wp, xv, reverse)                                              # [B, F, K]
        p = yt.real ** 2 + yt.imag ** 2
        if fault == "phi_per_bin":
            r, Fn = p, 1
        else:
            r, Fn = _sum(p, reverse, axis=1)[:, None, :], F                        # [B, 1, K]
        den = r / rdt.type(Fn) if st.model == "gauss" else rdt.type(2.0) * np.sqrt(r)
        phi = rdt.type(1.0) / np.maximum(den, floor)
        outer = xv[..., :, None] * np.conj(xv[..., None, :])
        eye = np.eye(M, dtype=cdt)
        di = np.arange(M)
        for k in range(M):
            g = (rdt.type(1.0) if fault == "v_without_1_minus_alpha" else oma) * phi[..., k]
            Vn = alpha * st.V[:, :, k] + g[..., None, None] * outer
            Vn = np.tril(Vn) + np.conj(np.swapaxes(np.tril(Vn, -1), -1, -2))
            Vn[..., di, di] = Vn[..., di, di].real
            Wc = W0 if fault == "jacobi" else st.W
            u, sbad = solve(_matmul(Wc, Vn, reverse), np.broadcast_to(eye[:, k:k + 1], Vn.shape[:-1] + (1,)))
            u = u[..., 0]
            if fault == "norm_uhu":
                d = _sum(u.real ** 2 + u.imag ** 2, reverse)
            else:
                q = _matvec(Vn, u, reverse)
                d = _sum(u.real * q.real + u.imag * q.imag, reverse)
            if fault == "float32_d":
                d = d.astype(np.float32).astype(rdt)
            ok = ~sbad & np.isfinite(d) & (d > 0) & ~badin
            row = np.conj(u) / np.sqrt(d)[..., None]
            st.W[:, :, k] = np.where(ok[..., None], row, st.W[:, :, k])
            st.V[:, :, k] = np.where(badin[..., None, None], st.V[:, :, k], Vn)
            st.fail |= np.where(~ok & ~badin, 2, 0).astype(np.int32)
        y = _matvec(st.W, xv, reverse)
        if fault == "a_is_wh":
            A, abad = np.conj(np.swapaxes(st.W, -1, -2)), np.zeros(badin.shape, bool)
        else:
            A, abad = solve(st.W, np.broadcast_to(eye, st.W.shape))
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
    """block complex64 [B, M, T, F] -> (est complex64 [B, M, T, F], images complex64 [B, M, M, T, F])"""
    block = np.asarray(block)
    B, M, T, F = block.shape
    est = np.zeros((B, M, T, F), np.complex64)
    img = np.zeros((B, M, M, T, F), np.complex64)
    for t in range(T):
        e, i = step(st, block[:, :, t], fault, reverse)
        est[:, :, t] = e.astype(np.complex64)
        img[:, :, :, t] = i.astype(np.complex64)
    return est, img


def pieces(T, cuts):
    """the (start, end) of every call when a stream of T frames is cut into calls of the lengths ``cuts`` and then the rest"""
    edges, t = [], 0
    for c in (cuts or []):
        if t >= T:
            break
        c = min(int(c), T - t)
        if c > 0:
            edges.append((t, t + c))
            t += c
    if t < T:
        edges.append((t, T))
    return edges


def oiva(mix, alpha=0.98, model="gauss", floor=1e-10, init=1.0, ref_ch=0, cuts=None, fault=None, reverse=False,
         dtype=np.complex128):
    """The one-shot call: reset, then the stream in one piece or in the pieces ``cuts`` (lengths; the rest follows).  mix complex64
    [B, M, T, F] -> (est, images, State)"""
    mix = np.asarray(mix)
    B, M, T, F = mix.shape
    st = State(B, M, F, alpha, model, floor, init, ref_ch, dtype)
    est = np.zeros((B, M, T, F), np.complex64)
    img = np.zeros((B, M, M, T, F), np.complex64)
    for t0, t1 in pieces(T, cuts):
        est[:, :, t0:t1], img[:, :, :, t0:t1] = process(st, mix[:, :, t0:t1], fault, reverse)
    return est, img, st


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = float(np.linalg.norm(b.ravel()))
    return float(np.linalg.norm((a - b).ravel())) / (den if den > 0 else 1.0)


def figures(mix, **kw):
    """The reference of one case and its bar: dict(est, images, st, bar, own).  W and V are measured against the clongdouble run
    (``ext``); bar = max(100 x own, STATE_FLOOR), own = the larger of the rel-L2 distances float64 - clongdouble and float64 -
    reversed summation order on W and V: the rule of owpe_ref and iva_ref.figures."""
    est, img, st = oiva(mix, **kw)
    _, _, ext = oiva(mix, dtype=np.clongdouble, **kw)
    _, _, rev = oiva(mix, reverse=True, **kw)
    own = max(rel(st.W, ext.W), rel(st.V, ext.V), rel(st.W, rev.W), rel(st.V, rev.V))
    return dict(est=est, images=img, st=st, ext=ext, bar=max(100.0 * own, STATE_FLOOR), own=own)


def hermitian(V):
    return bool(np.array_equal(V, np.conj(np.swapaxes(V, -1, -2))))


def unit_norm_error(W, V):
    """max over (b, f, k) of |Re(w_k^H V_k w_k) - 1| with w_k^H = row k of W"""
    w = np.conj(W)                                                                 # w[..., k, :] = w_k
    q = np.einsum("bfki,bfkij,bfkj->bfk", np.conj(w), V, w)
    return float(np.max(np.abs(q.real - 1.0)))


def image_sum_error(images, mix, fail):
    """rel-L2 of sum_k images[k, m] against the input on the bins without a flag.  images [B, K, M, T, F], mix [B, M, T, F]"""
    keep = (np.asarray(fail) == 0)[:, None, None, :]
    s = images.astype(np.complex128).sum(axis=1)
    return rel(np.where(keep, s, 0), np.where(keep, mix, 0))


def rejected(cand, ref):
    """what the device tests assert, as one predicate: True when a candidate dict(est, images, W, V, fail, n) misses any bar of
    the reference ``figures`` dict"""
    st, ext, bar = ref["st"], ref["ext"], ref["bar"]
    if not (np.array_equal(cand["fail"], st.fail) and np.array_equal(cand["n"], st.n)):
        return True
    if not hermitian(cand["V"]):
        return True
    return (rel(cand["est"], ref["est"]) > OUT_BAR or rel(cand["images"], ref["images"]) > OUT_BAR
            or rel(cand["W"], ext.W) > bar or rel(cand["V"], ext.V) > bar)


def as_candidate(est, img, st):
    return dict(est=est, images=img, W=st.W.astype(np.complex128), V=st.V.astype(np.complex128), fail=st.fail, n=st.n)


def to_stream(mix_bfmt):
    """[B, F, M, T] (the layout of iva_ref.sparse_mixture) -> [B, M, T, F]"""
    return np.ascontiguousarray(np.transpose(mix_bfmt, (0, 2, 3, 1)))


def best_image_sdr(images_m0, truth_m0):
    """images_m0 [K, T, F] against truth_m0 [N, T, F] (N <= K): the SDR of every true source under the best assignment, dB"""
    import itertools
    K, N = images_m0.shape[0], truth_m0.shape[0]

    def sdr(a, b):
        return 10.0 * np.log10(np.sum(np.abs(b) ** 2) / np.sum(np.abs(a - b) ** 2))
    best = max(itertools.permutations(range(K), N), key=lambda p: np.mean([sdr(images_m0[p[s]], truth_m0[s]) for s in range(N)]))
    return [float(sdr(images_m0[best[s]], truth_m0[s])) for s in range(N)]
