"""Float64 NumPy restatement of the joint multi-speaker beamformers of csrc/jbf.hip (include/misonet.h, "LCMV, SDW-MWF, rank-1 MWF
(ABI 570)").

Per (item b, bin f), Y = mix[b, f] [M, T] and X_s = src[b, s, f] [M, T], complex64 as loaded, float64 from there on:

    V     = Y - sum_s X_s
    Phi_s = X_s X_s^H / T,  Phi_v = V V^H / T (noise "mix": Y Y^H / T); the lower triangle computed and mirrored, a real diagonal
    R     = Phi_v + diag_load tr(Phi_v) / M I,  N_s = sum_{j != s} Phi_j + R
    lcmv  : R = L L^H;  rtf "cw": C_s = L^-1 Phi_s L^-H, q_s = its principal eigenvector, a_s = L q_s;  rtf "eig": a_s = the
            principal eigenvector of Phi_s;  d_s = a_s / a_s[ref_ch], D = [d_0 .. d_{S-1}];  W = R^-1 D (D^H R^-1 D)^-1
    mwf   : w_s = (Phi_s + mu N_s)^-1 Phi_s e_ref
    r1mwf : A_s = N_s^-1 Phi_s,  w_s = A_s e_ref / (mu + tr A_s)
    out_s[t] = w_s^H y[t]

by two routes: "a" np.linalg.eigh and LU solves (np.linalg.solve); "b" a cyclic complex Jacobi with the device's stopping rule,
a column-by-column Cholesky and triangular solves (W = L^-H Z G^-1 with Z = L^-1 D, G = Z^H Z = K K^H, as the kernel).  The
difference between the two is the yardstick of the weight bars of tests/test_gpu_jbf.py.

lcmv FAILS as a whole bin (a pivot of R or G not finite or not > 0, a tr Phi_s that is 0 or not finite, an a_s[ref_ch] that is 0
or not finite); mwf / r1mwf fail per speaker (a pivot; r1mwf: mu + tr A_s 0 or not finite): w = 0, out = 0, fail = 1.  The pivots
are those of the column-by-column Cholesky in either route, so that the flags do not depend on the route.

This file is also the only place where the input generator of those tests is defined, and where the faults are planted that
their bars have to reject (``fault=``).  Everything is batched over the bins.
"""
import functools

import numpy as np

KINDS = ("lcmv", "mwf", "r1mwf")
# every fault jbf() can plant: the other speaker's relative transfer function (lcmv, S > 1), the upper triangle not mirrored, the
# diagonal loading dropped (shows with diag_load > 0), w instead of conj(w) on the output, N_s including Phi_s (mwf, r1mwf)
FAULTS = ("other_rtf", "mirror", "load", "conj", "ns")
OUT_BAR = 2.4e-7            # 4 x 2^-24: the one complex64 rounding of a float64 result (as tests/wpd_ref.py has it)
W_FLOOR = 1e-12             # the weight bar is max(100 x the route (a) - (b) difference of the case, this)

# (B, S, M, T, F) of the device tests: T below a tile, one class plus noise, the smallest M; exactly one tile, S = M; one frame
# past a tile, odd M; a ragged tail, odd M and S; the product's M and S; all 16 tile rows and five waves busy; S = M = 4
SHAPES = [(2, 1, 2, 40, 5), (2, 2, 2, 64, 5), (2, 2, 3, 65, 7), (1, 3, 5, 150, 5), (2, 2, 6, 129, 9), (1, 4, 8, 200, 5),
          (1, 4, 4, 70, 5)]


def rel(a, b):
    return float(np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel()))


def jbf_inputs(B, S, M, T, F, seed=7):
    """src complex64 [B, S, F, M, T], mix complex64 [B, F, M, T]: X_s = d_s (x) (c (0.2 + U[0, 1)))_t + 0.1 c with d_s = c(M),
    Y = sum_s X_s + 0.3 c; c = complex normal of unit variance"""
    rng = np.random.default_rng(seed)

    def c(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    d = c(B, S, F, M)
    sig = c(B, S, F, T) * (0.2 + rng.random((B, S, F, T)))
    X = d[..., None] * sig[:, :, :, None, :] + 0.1 * c(B, S, F, M, T)
    Y = X.sum(axis=1) + 0.3 * c(B, F, M, T)
    return X.astype(np.complex64), Y.astype(np.complex64)


def _H(A):
    return np.conj(np.swapaxes(A, -1, -2))


def _finite(x):
    return np.isfinite(x.real) & np.isfinite(x.imag)


def _chol(A):
    """column-by-column Cholesky of A [N, n, n] from its lower triangle: (L, ok [N]); ok is False from the first pivot that is
    not finite or not > 0 (what follows in that matrix is not meant to be used)"""
    N, n, _ = A.shape
    L = np.zeros_like(A)
    ok = np.ones(N, dtype=bool)
    for j in range(n):
        piv = A[:, j, j].real - np.sum(np.abs(L[:, j, :j]) ** 2, axis=1)
        ok &= np.isfinite(piv) & (piv > 0)
        dj = np.sqrt(np.where(ok, piv, 1.0))
        L[:, j, j] = dj
        for i in range(j + 1, n):
            L[:, i, j] = (A[:, i, j] - np.sum(L[:, i, :j] * np.conj(L[:, j, :j]), axis=1)) / dj
    return L, ok


def _fwd(L, Bm):
    """L X = Bm, L [N, n, n] lower, Bm [N, n, r]"""
    X = np.array(Bm, dtype=np.complex128)
    for i in range(L.shape[1]):
        X[:, i] = (X[:, i] - np.einsum("nk,nkr->nr", L[:, i, :i], X[:, :i])) / L[:, i, i][:, None]
    return X


def _bwd(L, Bm):
    """L^H X = Bm"""
    X = np.array(Bm, dtype=np.complex128)
    n = L.shape[1]
    for i in range(n - 1, -1, -1):
        X[:, i] = (X[:, i] - np.einsum("nk,nkr->nr", np.conj(L[:, i + 1:, i]), X[:, i + 1:])) / L[:, i, i][:, None]
    return X


def jacobi(A):
    """cyclic complex Jacobi on the Hermitian A [N, n, n] with the device's rotation and stopping rule (a matrix stops when the
    squared off-diagonal norm is <= 1e-28 (sum_i |a_ii|)^2 or 0, at most 16 sweeps): (eigenvalues [N, n] as they stand on the
    diagonal, eigenvectors in the columns [N, n, n])"""
    A = np.array(A, dtype=np.complex128)
    N, n, _ = A.shape
    V = np.broadcast_to(np.eye(n, dtype=np.complex128), A.shape).copy()
    scale = np.sum(np.abs(np.real(np.einsum("nii->ni", A))), axis=1)
    iu = np.triu_indices(n, 1)
    for _ in range(16):
        off = np.sum(np.abs(A[:, iu[0], iu[1]]) ** 2, axis=1)
        live = ~((off <= 1e-28 * scale * scale) | (off == 0.0))
        if not live.any():
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = A[:, p, q]
                g = np.abs(apq)
                act = live & (g > 1e-300)
                gs = np.where(act, g, 1.0)
                tau = (A[:, q, q].real - A[:, p, p].real) / (2.0 * gs)
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = t * cs
                ph = apq / gs
                one, zero = np.ones(N), np.zeros(N)
                Rpp = np.where(act, cs, one).astype(np.complex128)
                Rpq = np.where(act, sn, zero).astype(np.complex128)
                Rqp = np.where(act, -sn * np.conj(ph), zero)
                Rqq = np.where(act, cs * np.conj(ph), one)
                for Mx in (A, V):                                     # columns p, q: X <- X R
                    xp, xq = Mx[:, :, p].copy(), Mx[:, :, q].copy()
                    Mx[:, :, p] = xp * Rpp[:, None] + xq * Rqp[:, None]
                    Mx[:, :, q] = xp * Rpq[:, None] + xq * Rqq[:, None]
                ap, aq = A[:, p, :].copy(), A[:, q, :].copy()         # rows p, q: A <- R^H A
                A[:, p, :] = np.conj(Rpp)[:, None] * ap + np.conj(Rqp)[:, None] * aq
                A[:, q, :] = np.conj(Rpq)[:, None] * ap + np.conj(Rqq)[:, None] * aq
                A[act, p, q] = 0.0
                A[act, q, p] = 0.0
                A[act, p, p] = A[act, p, p].real
                A[act, q, q] = A[act, q, q].real
    return np.real(np.einsum("nii->ni", A)).copy(), V


def _principal(C, route):
    """(eigenvector of the largest eigenvalue [N, n], largest / second eigenvalue [N]) of the Hermitian C [N, n, n]"""
    if route == "a":
        lam, vec = np.linalg.eigh(C)
        q = vec[:, :, -1]
        srt = lam
    else:
        lam, vec = jacobi(C)
        best = np.argmax(lam, axis=1)                                 # the first maximum, as the device
        q = np.take_along_axis(vec, best[:, None, None], axis=2)[:, :, 0]
        srt = np.sort(lam, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = srt[:, -1] / srt[:, -2] if C.shape[1] > 1 else np.full(C.shape[0], np.inf)
    return q, gap


def _cov(A, T, fault):
    P = A @ _H(A) / T
    low = np.tril(P, -1)
    dg = np.real(np.einsum("...ii->...i", P))
    out = low + np.einsum("...i,ij->...ij", dg, np.eye(P.shape[-1]))
    return out if fault == "mirror" else out + _H(low)


def _safe(A, bad):
    """A with the identity in the matrices flagged bad (so that LAPACK is never handed a matrix it cannot take)"""
    return np.where(bad[:, None, None], np.eye(A.shape[-1], dtype=np.complex128), A)


def jbf(src, mix, kind="lcmv", noise="residual", rtf="cw", mu=1.0, diag_load=0.0, ref_ch=0, route="a", fault=None):
    """src [B, S, F, M, T], mix [B, F, M, T] complex -> dict: out complex128 [B, S, T, F], w complex128 [B, S, F, M], rtf
    complex128 [B, S, F, M] (lcmv; else None), fail int32 [B, S, F], and over the bins that did not fail: cond = the largest
    cond(R), gap = the smallest ratio of the two leading eigenvalues behind an a_s (lcmv; else inf), resid = the largest
    |w_s^H d_j - delta_sj| (lcmv; else 0)"""
    assert kind in KINDS and route in ("a", "b") and (fault is None or fault in FAULTS)
    X = np.asarray(src).astype(np.complex128)
    Y = np.asarray(mix).astype(np.complex128)
    B, S, F, M, T = X.shape
    N = B * F
    X = X.transpose(0, 2, 1, 3, 4).reshape(N, S, M, T)
    Y = Y.reshape(N, M, T)
    eyeM = np.eye(M, dtype=np.complex128)
    with np.errstate(all="ignore"):
        V = Y if noise == "mix" else Y - X.sum(axis=1)
        Phi = np.stack([_cov(X[:, s], T, fault) for s in range(S)], axis=1)            # [N, S, M, M]
        Pv = _cov(V, T, fault)
        dl = 0.0 if fault == "load" else diag_load
        R = Pv + dl * np.real(np.einsum("nii->n", Pv))[:, None, None] / M * eyeM
        w = np.zeros((N, S, M), dtype=np.complex128)
        d = np.zeros((N, S, M), dtype=np.complex128) if kind == "lcmv" else None
        bad = np.zeros((N, S), dtype=bool)
        gap = np.full(N, np.inf)
        resid = np.zeros(N)
        if kind == "lcmv":
            Lb, ok = _chol(R)
            tr = np.real(np.einsum("nsii->ns", Phi))
            fb = ~ok | np.any((tr == 0.0) | ~np.isfinite(tr), axis=1)
            Rs = _safe(R, fb)
            L = np.linalg.cholesky(Rs) if route == "a" else _safe(Lb, fb)
            a = np.zeros((N, S, M), dtype=np.complex128)
            for s in range(S):
                Ps = _safe(Phi[:, s], fb)
                if rtf == "cw":
                    if route == "a":
                        Xw = np.linalg.solve(L, Ps)
                        C = _H(np.linalg.solve(L, _H(Xw)))
                    else:
                        C = _H(_fwd(L, _H(_fwd(L, Ps))))
                    C = 0.5 * (C + _H(C))
                    q, g = _principal(C, route)
                    a[:, s] = np.einsum("nij,nj->ni", L, q)
                else:
                    a[:, s], g = _principal(Ps, route)
                gap = np.minimum(gap, g)
            ar = a[:, :, ref_ch]
            fb |= np.any((ar == 0) | ~_finite(ar), axis=1)
            dd = a / np.where(fb[:, None], 1.0, ar)[:, :, None]
            D = np.swapaxes(np.roll(dd, 1, axis=1) if fault == "other_rtf" else dd, 1, 2)      # [N, M, S]
            D = np.where(fb[:, None, None], np.eye(M, S, dtype=np.complex128), D)
            if route == "a":
                RiD = np.linalg.solve(Rs, D)
                G = _H(D) @ RiD
            else:
                Z = _fwd(L, D)
                G = _H(Z) @ Z
            G = 0.5 * (G + _H(G))
            K, okG = _chol(G)
            fb |= ~okG
            Gs = _safe(G, fb)
            if route == "a":
                W = _H(np.linalg.solve(_H(Gs), _H(RiD)))
            else:
                Ks = _safe(K, fb)
                E = _bwd(Ks, _fwd(Ks, np.broadcast_to(np.eye(S, dtype=np.complex128), Gs.shape)))
                W = _bwd(L, Z @ E)
            w = np.swapaxes(W, 1, 2)
            d = dd
            bad = np.repeat(fb[:, None], S, axis=1)
            resid = np.max(np.abs(np.einsum("nsm,njm->nsj", np.conj(w), dd) - np.eye(S)), axis=(1, 2))
        else:
            for s in range(S):
                Ns = R + sum(Phi[:, j] for j in range(S) if j != s or fault == "ns")
                A = Phi[:, s] + mu * Ns if kind == "mwf" else Ns
                Lb, ok = _chol(A)
                fb = ~ok
                As = _safe(A, fb)
                rhs = Phi[:, s, :, ref_ch][:, :, None] if kind == "mwf" else Phi[:, s]
                if route == "a":
                    sol = np.linalg.solve(As, rhs)
                else:
                    Ls = _safe(Lb, fb)
                    sol = _bwd(Ls, _fwd(Ls, rhs))
                if kind == "mwf":
                    w[:, s] = sol[:, :, 0]
                else:
                    den = mu + np.einsum("nii->n", sol)
                    fb = fb | (den == 0) | ~_finite(den)
                    w[:, s] = sol[:, :, ref_ch] / np.where(fb, 1.0, den)[:, None]
                bad[:, s] = fb
        w = np.where(bad[:, :, None], 0.0, w)
        if d is not None:
            d = np.where(bad[:, :, None], 0.0, d)
        out = np.einsum("nsm,nmt->nst", w if fault == "conj" else np.conj(w), np.where(_finite(Y), Y, 0.0))
        out = np.where(bad[:, :, None], 0.0, out)
        good = ~np.any(bad, axis=1)
        cond = float(np.max(np.linalg.cond(R[good]))) if good.any() else 0.0
    shape = lambda x: x.reshape((B, F) + x.shape[1:]).swapaxes(1, 2)                   # [N, S, ...] -> [B, S, F, ...]
    return dict(out=np.ascontiguousarray(shape(out).swapaxes(2, 3)), w=np.ascontiguousarray(shape(w)),
                rtf=np.ascontiguousarray(shape(d)) if d is not None else None,
                fail=np.ascontiguousarray(shape(bad.astype(np.int32))), cond=cond,
                gap=float(np.min(gap[good])) if good.any() else np.inf, resid=float(np.max(resid[good])) if good.any() else 0.0)


def options(shape):
    """every option set the device tests run on a shape: (kind, dict of the keywords of jbf())"""
    M = shape[2]
    out = []
    for ref_ch in (0, M - 1):
        for dl in (0.0, 1e-6):
            for r in ("cw", "eig"):
                for nz in ("residual", "mix"):
                    out.append(("lcmv", dict(noise=nz, rtf=r, diag_load=dl, ref_ch=ref_ch)))
            for mu in (1.0, 4.0):
                out.append(("mwf", dict(mu=mu, diag_load=dl, ref_ch=ref_ch)))
            for mu in (0.0, 1.0):
                out.append(("r1mwf", dict(mu=mu, diag_load=dl, ref_ch=ref_ch)))
    return out


def case_id(shape, kind, kw):
    return "-".join(str(v) for v in shape) + "-" + kind + "-" + "-".join(f"{k}={v}" for k, v in sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def inputs(shape):
    B, S, M, T, F = shape
    return jbf_inputs(B, S, M, T, F)


@functools.lru_cache(maxsize=None)
def _case(shape, kind, kw_items, route):
    src, mix = inputs(shape)
    return jbf(src, mix, kind=kind, route=route, **dict(kw_items))


def case(shape, kind, kw, route="a"):
    """the restatement on the inputs of a shape, computed once and shared (leave the arrays unchanged)"""
    return _case(tuple(shape), kind, tuple(sorted(kw.items())), route)


def bars(shape, kind, kw):
    """(route (a) - (b) difference of the weights and RTFs of the case, the weight bar that follows from it)"""
    a, b = case(shape, kind, kw, "a"), case(shape, kind, kw, "b")
    diff = rel(b["w"], a["w"])
    if a["rtf"] is not None:
        diff = max(diff, rel(b["rtf"], a["rtf"]))
    return diff, max(100.0 * diff, W_FLOOR)
