"""NumPy restatement of continuous separation ("Long recordings without clean references"), independent of
misonet_amd.css: the window plan, the pairwise distances of the shared frames, the local pick, the chain and the
cross-fade stitch."""
import itertools
import math

import numpy as np

HOP = 64


def plan(L, W, H):
    """(starts, K, padded length) of a recording of L samples; ValueError on a bad window / hop"""
    if W <= 0 or H <= 0 or W % HOP or H % HOP or not (W // 2 <= H <= W - 256) or 2 * H < W:
        raise ValueError("bad window / hop")
    K = 1 if L <= W else 1 + math.ceil((L - W) / H)
    return [k * H for k in range(K)], K, (K - 1) * H + W


def windows(wav, W, H):
    """wav [L, M] -> [K, W, M] (zero-padded past L)"""
    _, K, Lp = plan(wav.shape[0], W, H)
    p = np.zeros((Lp,) + wav.shape[1:], dtype=wav.dtype)
    p[: wav.shape[0]] = wav
    return np.stack([p[k * H: k * H + W] for k in range(K)])


def ramp(ov):
    """(c, r) float32 [ov]: cos^2 and sin^2 of pi (j + 1/2) / (2 ov), evaluated in float64 and rounded"""
    x = np.pi * (np.arange(ov, dtype=np.float64) + 0.5) / (2 * ov)
    return (np.cos(x) ** 2).astype(np.float32), (np.sin(x) ** 2).astype(np.float32)


def _mag(z):
    z = np.asarray(z, dtype=np.complex64)
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    return np.sqrt(re * re + im * im)                    # float32 sqrtf(re^2 + im^2), not hypot


def distances(X, d):
    """X complex [K, S, T, F], d = hop in frames -> D float64 [K-1, S, S]"""
    X = np.asarray(X)
    K, S, T, F = X.shape
    D = np.zeros((max(0, K - 1), S, S), dtype=np.float64)
    for k in range(1, K):
        a = _mag(X[k - 1, :, d:])                        # [S, T-d, F]
        b = _mag(X[k, :, : T - d])
        for i in range(S):
            for j in range(S):
                D[k - 1, i, j] = np.abs(a[i] - b[j]).astype(np.float64).sum()
    return D


def pick(Dk):
    """the cheapest permutation of a distance matrix (itertools order, first minimum)"""
    S = Dk.shape[0]
    best, cbest = None, None
    for p in itertools.permutations(range(S)):
        c = 0.0
        for i in range(S):
            c += float(Dk[i, p[i]])
        if cbest is None or c < cbest:
            best, cbest = p, c
    return np.array(best, dtype=np.int32)


def margins(Dk):
    """(best cost, runner-up cost) over the permutations"""
    S = Dk.shape[0]
    costs = sorted(sum(float(Dk[i, p[i]]) for i in range(S)) for p in itertools.permutations(range(S)))
    return costs[0], (costs[1] if len(costs) > 1 else float("inf"))


def chain(D, S, perm0=None):
    """P [K, S]: P_0 = perm0 or identity, P_k[s] = L_k[P_{k-1}[s]]"""
    K = D.shape[0] + 1
    P = np.zeros((K, S), dtype=np.int32)
    P[0] = np.arange(S) if perm0 is None else perm0
    for k in range(1, K):
        Lk = pick(D[k - 1])
        P[k] = Lk[P[k - 1]]
    return P


def stitch(y, P, H, L):
    """y float32 [K, S, W], P [K, S] -> (float32 [S, L], int16 [S, L])"""
    y = np.asarray(y, dtype=np.float32)
    K, S, W = y.shape
    ov = W - H
    c, r = ramp(ov)
    out = np.zeros((S, L), dtype=np.float32)
    for s in range(S):
        for k in range(K):
            lo = k * H
            hi = L if k == K - 1 else min(L, (k + 1) * H)
            if lo >= hi:
                continue
            seg = y[k, P[k, s], : hi - lo].copy()
            if k >= 1:
                n = min(ov, hi - lo)
                a = y[k - 1, P[k - 1, s], H: H + n]
                seg[:n] = c[:n] * a + r[:n] * seg[:n]
            out[s, lo:hi] = seg
    i16 = (out * np.float32(32767.0)).astype(np.int32).astype(np.int16)
    return out, i16


def continuous(X, y, H, L):
    """steps 3-6 on the windows' outputs: X complex [K, S, T, F], y float32 [K, S, W] -> (P, D, float32, int16)"""
    D = distances(X, H // HOP)
    P = chain(D, X.shape[1])
    f32, i16 = stitch(y, P, H, L)
    return P, D, f32, i16
