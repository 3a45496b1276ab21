"""Float64 NumPy restatement of the guided cACGMM of csrc/cacgmm.hip (include/misonet.h, "cACGMM (ABI 560)").

Per (item b, bin f), K = S + 1 classes, Y = mix[b, f] [M, T], gamma0 [K, T] the initial masks (float32 values):

    z[t] = y[t] / |y[t]|; a frame with |y[t]|^2 == 0 is EMPTY: it enters no sum, its output mask is its initial mask
    sweep 0 (M-step only, gamma = gamma0, q = 1):
        n_k = sum_t gamma[k, t],  B_k = M / n_k sum_t gamma[k, t] / q[k, t] z z^H,  B_k += diag_load tr(B_k) / M I,
        B_k = L_k L_k^H,  logdet_k = 2 sum_i log L_k[i, i]
        prior "bin": pi[k] = n_k / sum_k n_k;  "guided": pi[k, t] = max(gamma0[k, t], prior_floor), fixed
    iteration 1 .. I (E-step, then the M-step; the last one the E-step only):
        q[k, t] = |L_k^-1 z|^2,  l[k, t] = log pi - logdet_k - M log q[k, t],  gamma[., t] = softmax_k l[., t]
    log-likelihood = sum_t logsumexp_k l[k, t] of the last E-step;  I = 0 returns the initial masks

A bin is UNSOLVED (initial masks, fail = 1, B = pi = ll = 0) when an n_k is not > 0 or not finite, a Cholesky pivot is not
finite or not > 0, or the log-likelihood of an E-step is not finite.  The tests compare the device against this file; it also
holds the input generators of those tests and the planted faults their bars have to reject (``fault=``).
"""
import numpy as np

from wpd_ref import OUT_BAR, rel, wpd_inputs          # noqa: F401  (the image bar and rel-L2 are WPD's)
from wpe_ref import _pivots_ok

TILE = 64                   # frames per LDS tile of the kernel
# every wrong evaluation cacgmm_bin can plant
FAULTS = ("q_prev", "no_M", "no_scale_M", "logdet", "empty", "tile_last", "pi", "f32gram")
MASK_BAR = 2.4e-7           # 4 x 2^-24, max-abs: masks lie in [0, 1], one float32 rounding is <= 2^-25


def cacgmm_bin(Y, g0, iterations=10, prior="bin", diag_load=1e-8, prior_floor=1e-6, frame_order=None, solver="chol",
               fault=None):
    """One bin.  Y [M, T] complex, g0 [K, T] real.  Returns a dict: masks float64 [K, T], B complex128 [K, M, M], pi float64
    [K], ll, fail, lls (the log-likelihood of every E-step).  ``frame_order``: a permutation of range(T), the order in which
    the frames are summed.  ``solver``: "chol" (L^-1 z by a triangular solve) or "inv" (z^H B^-1 z through the inverse).
    ``fault``: one of FAULTS."""
    Y = np.asarray(Y).astype(np.complex128)
    g0 = np.asarray(g0).astype(np.float64)
    M, T = Y.shape
    K = g0.shape[0]
    order = np.arange(T) if frame_order is None else np.asarray(frame_order)
    nrm2 = (Y.real ** 2 + Y.imag ** 2).sum(axis=0)
    live = nrm2 > 0
    Z = np.zeros_like(Y)
    Z[:, live] = Y[:, live] / np.sqrt(nrm2[live])
    unsolved = dict(masks=g0.copy(), B=np.zeros((K, M, M), np.complex128), pi=np.zeros(K), ll=0.0, fail=1, lls=[])
    if iterations == 0:
        return dict(unsolved, fail=0)
    counted = np.ones(T, bool) if fault == "empty" else live        # the frames that enter n_k
    gram = live.copy()                                              # the frames that enter the Gram sums
    if fault == "tile_last":
        gram[TILE - 1 if T >= TILE else T - 1] = False
    zo, co, go = Z[:, order], counted[order], gram[order]
    log_prior_t = np.log(np.maximum(g0, prior_floor)) if prior == "guided" else None

    def m_step(gam, q):
        with np.errstate(all="ignore"):
            n = (gam[:, order] * co[None, :]).sum(axis=1)
            if not (np.all(np.isfinite(n)) and np.all(n > 0)):
                return None
            w = np.where(go[None, :], gam[:, order] / q[:, order], 0.0)
            Bs, Ls = [], []
            for k in range(K):
                if fault == "f32gram":
                    G = ((zo * w[k][None, :]).astype(np.complex64) @ zo.conj().T.astype(np.complex64)).astype(np.complex128)
                else:
                    G = (zo * w[k][None, :]) @ zo.conj().T
                Bk = (1.0 if fault == "no_scale_M" else M) / n[k] * G
                Bk = Bk + diag_load * np.real(np.trace(Bk)) / M * np.eye(M)
                if not _pivots_ok(Bk):
                    return None
                Bs.append(Bk)
                Ls.append(np.linalg.cholesky(Bk))
        logdet = np.array([2.0 * np.sum(np.log(np.real(np.diagonal(L)))) for L in Ls])
        return np.array(Bs), Ls, logdet, n / n.sum()

    def e_step(Bs, Ls, logdet, pi):
        with np.errstate(all="ignore"):
            q = np.ones((K, T))
            for k in range(K):
                if solver == "chol":
                    x = np.linalg.solve(Ls[k], Z[:, live])
                    q[k, live] = (x.real ** 2 + x.imag ** 2).sum(axis=0)
                else:
                    q[k, live] = np.real(np.sum(Z[:, live].conj() * (np.linalg.inv(Bs[k]) @ Z[:, live]), axis=0))
            lp = log_prior_t if prior == "guided" else np.log(pi)[:, None]
            ell = lp - (0.0 if fault == "logdet" else logdet[:, None]) - (1 if fault == "no_M" else M) * np.log(q)
            mx = ell.max(axis=0)
            ex = np.exp(ell - mx[None, :])
            sm = ex.sum(axis=0)
            gam = np.where(live[None, :], ex / sm[None, :], g0)
            ll = float(((mx + np.log(sm))[order] * live[order]).sum()) if live.any() else 0.0
        return gam, q, ll

    gam, q = g0, np.ones((K, T))
    q_before = q
    st = m_step(gam, q)
    if st is None:
        return unsolved
    pi0 = st[3]
    lls = []
    ll = 0.0
    for it in range(1, iterations + 1):
        gam, q_new, ll = e_step(*st)
        lls.append(ll)
        if not np.isfinite(ll):
            return unsolved
        if it == iterations:
            break
        st = m_step(gam, q_before if fault == "q_prev" else q_new)
        q_before = q_new
        if st is None:
            return unsolved
        if fault == "pi":
            st = st[:3] + (pi0,)
    return dict(masks=gam, B=st[0], pi=st[3], ll=ll, fail=0, lls=lls)


def cacgmm(mix, init, iterations=10, prior="bin", diag_load=1e-8, prior_floor=1e-6, frame_order=None, solver="chol", fault=None):
    """mix [B, F, M, T] complex, init [B, K, F, T] -> dict: masks float64 [B, K, F, T], images complex128 [B, S, F, M, T],
    B complex128 [B, F, K, M, M], pi [B, F, K], ll [B, F], fail int32 [B, F]"""
    mix, init = np.asarray(mix), np.asarray(init)
    Bn, F, M, T = mix.shape
    K = init.shape[1]
    out = dict(masks=np.zeros((Bn, K, F, T)), B=np.zeros((Bn, F, K, M, M), np.complex128), pi=np.zeros((Bn, F, K)),
               ll=np.zeros((Bn, F)), fail=np.zeros((Bn, F), np.int32))
    for b in range(Bn):
        for f in range(F):
            r = cacgmm_bin(mix[b, f], init[b, :, f], iterations, prior, diag_load, prior_floor, frame_order, solver, fault)
            out["masks"][b, :, f] = r["masks"]
            out["B"][b, f], out["pi"][b, f], out["ll"][b, f], out["fail"][b, f] = r["B"], r["pi"], r["ll"], r["fail"]
    out["images"] = out["masks"][:, :K - 1, :, None, :] * mix.astype(np.complex128)[:, None]
    return out


def masks_from_estimates(est, mix):
    """est [B, S, F, M, T], mix [B, F, M, T] complex -> float32 [B, S + 1, F, T]: P_k / sum_k P_k, 1 / K where that sum is 0"""
    est = np.asarray(est).astype(np.complex128)
    mix = np.asarray(mix).astype(np.complex128)
    P = [(np.abs(est[:, s]) ** 2).sum(axis=2) for s in range(est.shape[1])]
    P.append((np.abs(mix - est.sum(axis=1)) ** 2).sum(axis=2))
    P = np.stack(P, axis=1)                                                   # [B, K, F, T]
    tot = P.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(tot > 0, P / tot, 1.0 / P.shape[1]).astype(np.float32)


def reverberant_inputs(B, M, T, F, seed=0):
    """The reverberant two-source generator of wpd_ref.wpd_inputs with the estimates of both sources: mix complex64
    [B, F, M, T], est complex64 [B, 2, F, M, T], init float32 [B, 3, F, T] = masks_from_estimates(est, mix)"""
    mix, e0 = wpd_inputs(B, M, T, F, seed=seed, which=0)
    mix1, e1 = wpd_inputs(B, M, T, F, seed=seed, which=1)
    assert np.array_equal(mix, mix1)
    est = np.ascontiguousarray(np.stack([e0, e1], axis=1))
    return mix, est, masks_from_estimates(est, mix)


def sparse_inputs(B, S, M, T, F, seed=0, noise=0.1):
    """Sparse rank-1 scenes: per frame one of {source 0 .. S - 1, noise only} is active, with random steering vectors and noise
    at ``noise``.  mix complex64 [B, F, M, T], truth float64 [B, S + 1, F, T] (one-hot), init float32 = 0.4 truth + 0.2"""
    rng = np.random.default_rng(1000 + seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    K = S + 1
    act = rng.integers(0, K, size=(B, F, T))
    truth = np.stack([(act == k) for k in range(K)], axis=1).astype(np.float64)              # [B, K, F, T]
    steer = cn(B, S, F, M)
    sig = cn(B, S, F, T)
    mix = noise * cn(B, F, M, T)
    for s in range(S):
        mix = mix + steer[:, s][..., None] * (sig[:, s] * truth[:, s])[:, :, None, :]
    return mix.astype(np.complex64), truth, (0.4 * truth + 0.2).astype(np.float32)


# the shapes (B, S, M, T, F) of the device tests: below one tile, two items; the smallest K and M; odd M, one tile plus a tail;
# exactly one tile; one tile plus one frame; the product's M, several tiles; the largest K and M
SHAPES = [(2, 2, 4, 60, 9), (1, 1, 2, 40, 5), (1, 2, 3, 70, 4), (1, 2, 6, 64, 3), (1, 2, 6, 65, 3), (1, 2, 6, 300, 17),
          (1, 4, 8, 200, 3)]


def case_inputs(shape):
    """(mix, init, est or None) of a device test shape: the reverberant generator for two speakers, the sparse one otherwise"""
    B, S, M, T, F = shape
    if S == 2:
        mix, est, init = reverberant_inputs(B, M, T, F)
        return mix, init, est
    mix, _, init = sparse_inputs(B, S, M, T, F)
    return mix, init, None


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def figures(got, want, perm):
    """The figures the device tests assert and their bars, {name: (figure, bar)}: got / want / perm = dicts as cacgmm()
    returns them (got: the evaluation under test, want: the restatement, perm: the restatement with the frames summed in a
    permuted order).  masks: max-abs <= MASK_BAR; images: rel-L2 <= OUT_BAR; B, pi, ll: rel-L2 <= 100 x the restatement's
    permuted-order difference on that case, never below 1e-12."""
    out = dict(masks=(max_abs(got["masks"], want["masks"]), MASK_BAR))
    if got.get("images") is not None:
        out["images"] = (rel(got["images"], want["images"]), OUT_BAR)
    for name in ("B", "pi", "ll"):
        out[name] = (rel(got[name], want[name]), max(100.0 * rel(perm[name], want[name]), 1e-12))
    return out


def missed(fig):
    return [name for name, (v, bar) in fig.items() if not v <= bar]
