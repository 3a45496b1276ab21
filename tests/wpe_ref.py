"""Float64 NumPy restatement of the WPE dereverberation of csrc/wpe.hip (include/misonet.h, "WPE dereverberation").

Per (item b, bin f), Y = mix[b, :, :, f] [M, T]:

    Z[(k M + m), t] = Y[m, t - delay - k]      (k = 0 .. taps - 1; zero for t - delay - k < 0)
    X <- Y; repeat `iterations` times:
        p[t] = mean_m |X[m, t]|^2              (first iteration: power[b, t, f] when given)
        w[t] = 1 / max(p[t], power_floor max_t p[t])
        R = sum_t w Z Z^H,  P = sum_t w Z Y^H,  R += diag_load tr(R) / N I
        G = R^-1 P,  X = Y - G^H Z

A bin is passed through (X = Y, G = 0, fail = 1) when a Cholesky pivot of R is not finite or not > 0.  With the defaults this
is nara_wpe's wpe_v8 with psd_context = 0.  The tests compare the device against this file; it is also the only place the input
generator of those tests is defined, and the place where the faults are planted that the bars of the device tests have to reject
(``fault=``).
"""
import numpy as np

# every fault wpe_bin can plant; "floor" shows only where the floor binds (power_floor large enough), "tap_order" shows in G only
# (X is invariant under a permutation of the rows of Z) and is no fault at all where M = 1 or taps = 1; the TILE_FAULTS show only
# where T reaches past one tile of the kernel
FAULTS = ("delay", "tap_order", "conj", "floor", "stale_power", "seam", "tail", "hist", "inplace")
TILE_FAULTS = ("seam", "tail", "hist", "inplace")
TILE = 64           # frames per LDS tile of the kernel


def stack(Y, taps, delay):
    """Y [M, T] -> Z [M taps, T], row k M + m = Y[m] delayed by delay + k frames"""
    M, T = Y.shape
    Z = np.zeros((taps * M, T), dtype=Y.dtype)
    for k in range(taps):
        d = delay + k
        if d < T:
            Z[k * M:(k + 1) * M, d:] = Y[:, :T - d]
    return Z


def stack_hist(Y, taps, delay):
    """the fault "hist": stack(), but Z[., t] reads 0 wherever t - delay - k lies in an earlier tile than t"""
    Z = stack(Y, taps, delay)
    M, T = Y.shape
    t = np.arange(T)
    for k in range(taps):
        Z[k * M:(k + 1) * M, (t - delay - k) // TILE < t // TILE] = 0
    return Z


def _pivots_ok(R):
    """the failure rule: every pivot of the Cholesky factorisation finite and > 0"""
    if not np.all(np.isfinite(R)):
        return False
    try:
        L = np.linalg.cholesky(R)
    except np.linalg.LinAlgError:
        return False
    d = np.real(np.diagonal(L))
    return bool(np.all(np.isfinite(d)) and np.all(d > 0))


def wpe_bin(Y, power=None, taps=10, delay=3, iterations=3, diag_load=0.0, power_floor=1e-10, solver="lu", block=None,
            fault=None):
    """One bin.  Y [M, T] complex; power [T] or None.  Returns (X complex128 [M, T], G complex128 [M taps, M], fail).
    ``solver``: "lu" (np.linalg.solve) or "chol"; ``block``: add the correlations in blocks of that many frames (another
    summation order); ``fault``: one of FAULTS, a wrong evaluation."""
    Y = np.asarray(Y).astype(np.complex128)
    M, T = Y.shape
    N = M * taps
    if fault == "hist":
        Z = stack_hist(Y, taps, delay)
    else:
        Z = stack(Y, taps, delay + (1 if fault == "delay" else 0))
    if fault == "tap_order":                                          # row m taps + k holds what row k M + m should
        Z = Z.reshape(taps, M, T).transpose(1, 0, 2).reshape(N, T)
    apply = (lambda G: Y - G.T @ Z) if fault == "conj" else (lambda G: Y - G.conj().T @ Z)
    X = Y
    G = np.zeros((N, M), dtype=np.complex128)
    for it in range(iterations):
        if it == 0 and power is not None:
            p = np.asarray(power, dtype=np.float64)
        else:
            p = np.mean(np.abs(Y if fault == "stale_power" else X) ** 2, axis=0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            w = 1.0 / np.maximum(p, (0.0 if fault == "floor" else power_floor) * np.max(p))
            if fault == "tail":                                       # the frames past the last whole tile carry no weight
                w = np.where(np.arange(T) < T // TILE * TILE, w, 0.0)
            Zw = Z * w[None, :]
            if fault == "seam":                                       # the first frame of the second tile (the last frame where
                ts = TILE if T > TILE else T - 1                      # there is one tile only) is the one before it
                Zw[:, ts] = Zw[:, ts - 1]
            if block is None:
                R = Zw @ Z.conj().T
                P = Zw @ Y.conj().T
            else:
                R = np.zeros((N, N), dtype=np.complex128)
                P = np.zeros((N, M), dtype=np.complex128)
                for t0 in range(0, T, block):
                    R += Zw[:, t0:t0 + block] @ Z[:, t0:t0 + block].conj().T
                    P += Zw[:, t0:t0 + block] @ Y[:, t0:t0 + block].conj().T
            R = R + diag_load * np.real(np.trace(R)) / N * np.eye(N)
        if not _pivots_ok(R):
            return Y.copy(), np.zeros((N, M), dtype=np.complex128), 1
        if solver == "lu":
            G = np.linalg.solve(R, P)
        else:
            L = np.linalg.cholesky(R)
            G = np.linalg.solve(L.conj().T, np.linalg.solve(L, P))
        X = apply(G)
    if fault == "inplace":                                            # the output lands tile by tile in ascending order, over
        X = Y.copy()                                                  # the frames that the later tiles read as history
        for t0 in range(0, T, TILE):
            X[:, t0:t0 + TILE] = Y[:, t0:t0 + TILE] - G.conj().T @ stack(X, taps, delay)[:, t0:t0 + TILE]
    return X, G, 0


def wpe(mix, power=None, taps=10, delay=3, iterations=3, diag_load=0.0, power_floor=1e-10, solver="lu", block=None,
        fault=None):
    """mix [B, M, T, F] complex, power [B, T, F] or None -> (X complex128 [B, M, T, F], G complex128 [B, F, M taps, M],
    fail int32 [B, F])"""
    mix = np.asarray(mix)
    B, M, T, F = mix.shape
    X = np.zeros((B, M, T, F), dtype=np.complex128)
    G = np.zeros((B, F, M * taps, M), dtype=np.complex128)
    fail = np.zeros((B, F), dtype=np.int32)
    for b in range(B):
        for f in range(F):
            pw = None if power is None else np.asarray(power)[b, :, f]
            x, g, bad = wpe_bin(mix[b, :, :, f], pw, taps, delay, iterations, diag_load, power_floor, solver, block, fault)
            X[b, :, :, f] = x
            G[b, f] = g
            fail[b, f] = bad
    return X, G, fail


def reverb_inputs(B, M, T, F, seed=0, rev=12, noise=0.3):
    """Two enveloped sources through exponentially decaying random filters, plus noise: complex64 [B, M, T, F]"""
    rng = np.random.default_rng(seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    t = np.arange(T + rev)[None, :, None]
    f = np.arange(F)[None, None, :]
    out = np.zeros((B, M, T, F), dtype=np.complex128)
    for s in range(2):
        src = cn(B, T + rev, F) * (np.abs(np.sin(0.05 * (s + 1) * t + f)) + 0.05)
        h = cn(B, M, rev, F) * np.exp(-0.35 * np.arange(rev))[None, None, :, None]
        for l in range(rev):
            out += h[:, :, l][:, :, None, :] * src[:, None, rev - l:rev - l + T, :]
    out += noise * cn(B, M, T, F)
    return (0.05 * out).astype(np.complex64)
