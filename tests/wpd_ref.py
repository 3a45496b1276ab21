"""Float64 NumPy restatement of the WPD convolutional beamformer of csrc/wpd.hip (include/misonet.h, "WPD (ABI 530)").

Per (item b, bin f), Y = mix[b, f] [M, T] and S = src[b, f] [M, T], the source estimate at every microphone:

    Z[(k M + m), t] = Y[m, t - delay - k]      (k = 0 .. taps - 1; zero before the start: wpe_ref.stack)
    ybar[t] = [Y[:, t]; Z[:, t]]               order K = M (taps + 1)
    p[t]    = mean_m |S[m, t]|^2,  w[t] = 1 / max(p[t], power_floor max_t p[t])
    R       = sum_t w ybar ybar^H,  R += diag_load tr(R) / K I
    Phi_s   = S S^H / T made Hermitian (0.5 (Phi + Phi^H), as beamform_ref.covariance); Phibar = Phi_s in the top-left block
    A       = R^-1 Phibar,  wbar = A[:, ref_ch] / tr(A),  out[t] = wbar^H ybar[t]

A bin FAILS (wbar = 0, out = 0, fail = 1) when a Cholesky pivot of R is not finite or not > 0, or tr(A) is not finite or is 0.
The tests compare the device against this file; it is also the only place the input generator of those tests is defined, and
the place where the faults are planted that the bars of the device tests have to reject (``fault=``).
"""
import numpy as np

from wpe_ref import _pivots_ok, stack, stack_hist

# every fault wpd_bin can plant; "floor" shows only where the floor binds (power_floor large enough), the TILE_FAULTS only where
# T reaches past one tile of the kernel
FAULTS = ("delay", "floor", "ref_ch", "conj", "seam", "block", "tail", "hist")
TILE_FAULTS = ("tail", "hist")
TILE = 64           # frames per LDS tile of the kernel: where a stale frame would sit


def wpd_bin(Y, S, taps=5, delay=3, diag_load=0.0, power_floor=1e-10, ref_ch=0, solver="lu", fault=None):
    """One bin.  Y, S [M, T] complex.  Returns (out complex128 [T], wbar complex128 [K] in the order [y; z], fail, cond(R)).
    ``solver``: "lu" (np.linalg.solve) or "chol".  ``fault``: one of FAULTS, a wrong evaluation."""
    Y = np.asarray(Y).astype(np.complex128)
    S = np.asarray(S).astype(np.complex128)
    M, T = Y.shape
    K = M * (taps + 1)
    if fault == "hist":                                               # z reads 0 wherever its frame lies in an earlier tile
        ybar = np.concatenate([Y, stack_hist(Y, taps, delay)], axis=0)
    else:
        ybar = np.concatenate([Y, stack(Y, taps, delay + (1 if fault == "delay" else 0))], axis=0)
    p = np.mean(np.abs(S) ** 2, axis=0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = 1.0 / np.maximum(p, (0.0 if fault == "floor" else power_floor) * np.max(p))
        if fault == "tail":                                           # the frames past the last whole tile carry no weight in R
            w = np.where(np.arange(T) < T // TILE * TILE, w, 0.0)
        lhs = ybar.copy()
        if fault == "seam":                                       # the first frame of a tile (the last frame where there is
            ts = TILE if T > TILE else T - 1                      # one tile only) is the one before it
            lhs[:, ts] = lhs[:, ts - 1]
        R = (lhs * w[None, :]) @ lhs.conj().T
        R = R + diag_load * np.real(np.trace(R)) / K * np.eye(K)
    phi = S @ S.conj().T / T
    phi = 0.5 * (phi + phi.conj().T)
    pb = np.zeros((K, K), dtype=np.complex128)
    if fault == "block":
        pb[K - M:, K - M:] = phi
    else:
        pb[:M, :M] = phi
    bad = (np.zeros(T, np.complex128), np.zeros(K, np.complex128), 1, np.inf)
    if not _pivots_ok(R):
        return bad
    if solver == "lu":
        A = np.linalg.solve(R, pb)
    else:
        L = np.linalg.cholesky(R)
        A = np.linalg.solve(L.conj().T, np.linalg.solve(L, pb))
    tr = np.trace(A)
    if not np.isfinite(tr) or tr == 0:
        return bad
    wbar = A[:, (ref_ch + 1) % M if fault == "ref_ch" else ref_ch] / tr
    out = (wbar if fault == "conj" else wbar.conj()) @ ybar
    return out, wbar, 0, float(np.linalg.cond(R))


def wpd(src, mix, taps=5, delay=3, diag_load=0.0, power_floor=1e-10, ref_ch=0, solver="lu", fault=None):
    """src, mix [B, F, M, T] complex (the layouts of misonet_beamform) -> (out complex128 [B, T, F], wbar complex128 [B, F, K],
    fail int32 [B, F], the largest cond(R) of a bin that did not fail)"""
    src, mix = np.asarray(src), np.asarray(mix)
    B, F, M, T = mix.shape
    out = np.zeros((B, T, F), dtype=np.complex128)
    wb = np.zeros((B, F, M * (taps + 1)), dtype=np.complex128)
    fail = np.zeros((B, F), dtype=np.int32)
    cond = 0.0
    for b in range(B):
        for f in range(F):
            o, w, bad, c = wpd_bin(mix[b, f], src[b, f], taps, delay, diag_load, power_floor, ref_ch, solver, fault)
            out[b, :, f] = o
            wb[b, f] = w
            fail[b, f] = bad
            if not bad:
                cond = max(cond, c)
    return out, wb, fail, cond


def wpe_then_souden_bin(Y, S, taps, delay, power_floor=1e-10, ref_ch=0):
    """wbar of one bin by another route (diag_load = 0): G = the WPE filter under the weights of S (wpe_ref.wpe_bin with
    power = p, one iteration), x = Y - G^H Z, q = the Souden weight of (sum_t w x x^H, Phi_s); then wbar = [q; -G q]"""
    from wpe_ref import wpe_bin
    Y = np.asarray(Y).astype(np.complex128)
    S = np.asarray(S).astype(np.complex128)
    M, T = Y.shape
    p = np.mean(np.abs(S) ** 2, axis=0)
    X, G, bad = wpe_bin(Y, p, taps, delay, 1, 0.0, power_floor)
    assert not bad
    w = 1.0 / np.maximum(p, power_floor * np.max(p))
    Rx = (X * w[None, :]) @ X.conj().T
    phi = S @ S.conj().T / T
    phi = 0.5 * (phi + phi.conj().T)
    A = np.linalg.solve(Rx, phi)
    q = A[:, ref_ch] / np.trace(A)
    return np.concatenate([q, -G @ q])


def wpd_inputs(B, M, T, F, seed=0, rev=12, noise=0.3, early=3, src_noise=0.2, which=0):
    """Two enveloped sources through exponentially decaying random filters, plus noise: mix complex64 [B, F, M, T]; and the
    estimate of source ``which`` at every microphone: its early part (the first ``early`` taps of its filters) plus
    ``src_noise`` times the rms of that part of noise: src complex64 [B, F, M, T]"""
    rng = np.random.default_rng(seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    t = np.arange(T + rev)[None, :, None]
    f = np.arange(F)[None, None, :]
    mix = np.zeros((B, M, T, F), dtype=np.complex128)
    src = np.zeros((B, M, T, F), dtype=np.complex128)
    for s in range(2):
        sig = cn(B, T + rev, F) * (np.abs(np.sin(0.05 * (s + 1) * t + f)) + 0.05)
        h = cn(B, M, rev, F) * np.exp(-0.35 * np.arange(rev))[None, None, :, None]
        for l in range(rev):
            img = h[:, :, l][:, :, None, :] * sig[:, None, rev - l:rev - l + T, :]
            mix += img
            if s == which and l < early:
                src += img
    mix += noise * cn(B, M, T, F)
    src += src_noise * np.sqrt(np.mean(np.abs(src) ** 2)) * cn(B, M, T, F)
    to = lambda x: np.ascontiguousarray((0.05 * x).transpose(0, 3, 1, 2)).astype(np.complex64)
    return to(mix), to(src)


# the shapes (B, M, T, F, taps, delay) of the device tests: T below one tile; the smallest order; odd M, one tile + 6; T no
# multiple of a tile; the largest order (K = 88)
SHAPES = [(2, 4, 60, 9, 3, 2), (1, 2, 40, 5, 2, 1), (1, 3, 70, 4, 3, 1), (1, 6, 300, 17, 5, 3), (1, 8, 200, 3, 10, 3)]
OUT_BAR = 2.4e-7            # 4 x 2^-24: one complex64 rounding of a float64 result


def rel(a, b):
    return float(np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel()))
