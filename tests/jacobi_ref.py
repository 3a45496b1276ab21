"""Float64 NumPy restatement of the shared eigen-solver (csrc/jacobi.hpp, ``jacobi_hermitian<M>``: the round-robin complex
Jacobi behind iva_pca_k, doa_cov_k, mvdr_scm_eig, bf_solve / gev and jbf_bin_k / lcmv), the degenerate inputs the device tests
face it with, and the figures and bars they are judged by.

``jacobi(R)``: the circle-method pairing with the dummy player for odd M; per round every pair's rotation from the untouched
matrix (tau, tt, cs, sn and the phase apq / g), the column update of A and V, the row update of A, the pivot pair zeroed and
the diagonal made real; stop at off <= 1e-28 scale^2 or off == 0, 16 sweeps at the most.  It returns (the diagonal, V, the
sweeps it ran); the order of the eigenpairs is the call sites' business (``order``: descending, equal ones the lower index
first).  ``fault=`` plants one of FAULTS.

Cases (``cases(M)``, M = 2 .. 8): complex64 X [M, T = 16] whose covariance R = X X^H / T is EXACT in float64 in any summation
order, with or without fused multiply-adds: every entry is a Gaussian integer of magnitude <= 2^11 times one power of two per
row, T is a power of two and shorter cases are padded with zero frames (that scales R by a power of two and changes no
eigenvector).  Host R and device R agree to the bit, so what the figures compare is the solver and not the covariance sum.

Figures, all invariant to the basis chosen inside a degenerate subspace:
    backward  ||R V - V diag(lam)||_F / ||R||_F   (lam: the device's, or the Rayleigh quotients v_k^H R v_k where it exports none)
    orth      ||V^H V - I||_F over the live columns
    eigs      max |sorted lam - eigvalsh(R)| / max eigvalsh(R)
    proj(S)   ||P_noise - P_noise(eigh)||_F for the split after the S leading eigenvalues
Bars:
    backward, eigs   sqrt(2) 1e-14 tr(R) / ||R||_F  +  max(100 x LAPACK's own backward on the case, 1e-15).  The first term is
                     what the stopping rule admits: off counts the upper triangle, so the off-diagonal norm it tolerates is
                     sqrt(2 off) <= sqrt(2) 1e-14 scale, and scale = tr(R) for a covariance.
    orth             max(100 x the restatement's own orth on the case, 1e-14)
    proj(S)          backward bar / relative gap + orth bar (Davis-Kahan), asserted only where the relative gap
                     (lam_{S-1} - lam_S) / lam_0 is >= GAP_MIN = 0.03; BAR_CAP where that sum is larger
    BAR_CAP = 1e-12  above every bar, asserted wherever a bar is used
tests/test_eig_cases.py holds the restatement to these bars and to 8 sweeps on every case and shows that every planted fault
misses a bar, the tie rule or the sweep cap (``no_zeroing``: inside every bar, but linear convergence on a null space of
dimension >= 3).
"""
import functools

import numpy as np

BAR_CAP = 1e-12
GAP_MIN = 0.03
RANK_TOL = 1e-12             # IVA_RANK_TOL, DOA_RANK_TOL: an eigenvalue not above this times the largest counts as 0
MAX_SWEEPS = 16
T = 16
MS = (2, 3, 4, 5, 6, 7, 8)
# every wrong evaluation jacobi() / order() can plant
FAULTS = ("no_dummy", "phase_sign", "no_zeroing", "one_sweep", "serial_read", "tie_high", "tol_1e-6")
# no fault: the second pair of a round takes its rotation from the matrix the first pair has updated completely, which is the
# serial cyclic Jacobi.  jacobi() accepts it so that tests/test_eig_cases.py can show that no bar rejects a correct method.
NOT_A_FAULT = "serial_order"


# ---- the solver ---------------------------------------------------------------------------------------------------------------
def round_pairs(M, rd, fault=None):
    """the pivot pairs (p < q) of round rd, slot by slot; None where the dummy player sits a pair out"""
    ME = (M + 1) & ~1
    out = []
    for pj in range(ME // 2):
        if pj == 0:
            p, q = rd, ME - 1
        else:
            p, q = (rd + pj) % (ME - 1), (rd - pj + (ME - 1)) % (ME - 1)
        if p > q:
            p, q = q, p
        if q >= M:                                                   # the dummy player
            if fault == "no_dummy" and p != M - 1:
                q = M - 1                                            # rotated with row M - 1 instead: no longer disjoint
            else:
                out.append(None)
                continue
        out.append((p, q))
    return out


def _rotation(A, p, q, fault=None):
    """R restricted to (p, q) as (Rpp, Rpq, Rqp, Rqq), or None where the pivot is already 0"""
    apq = A[p, q]
    g = np.sqrt(apq.real * apq.real + apq.imag * apq.imag)
    if not g > 1e-300:
        return None
    app, aqq = A[p, p].real, A[q, q].real
    tau = (aqq - app) / (2.0 * g)
    tt = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
    cs = 1.0 / np.sqrt(1.0 + tt * tt)
    sn = tt * cs
    pr, pi = apq.real / g, apq.imag / g                              # e^{i phi}
    rqp = complex(-sn * pr, -sn * pi) if fault == "phase_sign" else complex(-sn * pr, sn * pi)
    return complex(cs, 0.0), complex(sn, 0.0), rqp, complex(cs * pr, -cs * pi)


def _cols(A, V, p, q, r, rows):
    """A <- A R, V <- V R on the columns (p, q), the rows ``rows``"""
    rpp, rpq, rqp, rqq = r
    for k in rows:
        akp, akq = A[k, p], A[k, q]
        A[k, p], A[k, q] = akp * rpp + akq * rqp, akp * rpq + akq * rqq
        vkp, vkq = V[k, p], V[k, q]
        V[k, p], V[k, q] = vkp * rpp + vkq * rqp, vkp * rpq + vkq * rqq


def _rows(A, p, q, r):
    """A <- R^H A on the rows (p, q)"""
    rpp, rpq, rqp, rqq = r
    for k in range(A.shape[0]):
        apk, aqk = A[p, k], A[q, k]
        A[p, k] = np.conj(rpp) * apk + np.conj(rqp) * aqk
        A[q, k] = np.conj(rpq) * apk + np.conj(rqq) * aqk


def jacobi(R, fault=None):
    """(the diagonal float64 [M], V complex128 [M, M], sweeps) of the Hermitian R as jacobi_hermitian<M> leaves them.
    Faults: ``no_dummy`` the dummy player's pair is rotated with row M - 1 for odd M; ``phase_sign`` Rqp is not conjugated;
    ``no_zeroing``; ``one_sweep``; ``tol_1e-6`` for the 1e-28 of the stopping rule; ``serial_read`` a missing barrier between
    the column and the row update: the second pair of a round reads, for its row update, the matrix the first pair has already
    updated in row p and not yet in row q.  ``fault=NOT_A_FAULT`` is the serial order, see above."""
    A = np.array(R, dtype=np.complex128)
    M = A.shape[0]
    V = np.eye(M, dtype=np.complex128)
    ME = (M + 1) & ~1
    scale = 0.0
    for i in range(M):
        scale += abs(A[i, i].real)
    tol = 1e-6 if fault == "tol_1e-6" else 1e-28
    sweeps = 0
    for _ in range(1 if fault == "one_sweep" else MAX_SWEEPS):
        off = 0.0
        for p in range(M):
            for q in range(p + 1, M):
                off += A[p, q].real * A[p, q].real + A[p, q].imag * A[p, q].imag
        if off <= tol * scale * scale or off == 0.0:
            break
        sweeps += 1
        for rd in range(ME - 1):
            pairs = [pq for pq in round_pairs(M, rd, fault) if pq is not None]
            if fault == NOT_A_FAULT:
                act = []
                for p, q in pairs:
                    r = _rotation(A, p, q)
                    if r is not None:
                        _cols(A, V, p, q, r, range(M))
                        _rows(A, p, q, r)
                        act.append((p, q, r))
            else:
                act = [(p, q, r) for (p, q), r in ((pq, _rotation(A, *pq, fault)) for pq in pairs) if r is not None]
                if fault == "serial_read" and len(act) >= 2:
                    (p0, q0, r0), (p1, q1, r1) = act[0], act[1]
                    _cols(A, V, p0, q0, r0, [k for k in range(M) if k != q1])
                    for p, q, r in act[1:]:
                        _cols(A, V, p, q, r, range(M))
                    _rows(A, p1, q1, r1)
                    _cols(A, V, p0, q0, r0, [q1])
                    for p, q, r in act[:1] + act[2:]:
                        _rows(A, p, q, r)
                else:
                    for p, q, r in act:
                        _cols(A, V, p, q, r, range(M))
                    for p, q, r in act:
                        _rows(A, p, q, r)
            if fault != "no_zeroing":
                for p, q, _r in act:
                    A[p, q] = A[q, p] = 0.0
                    A[p, p] = A[p, p].real
                    A[q, q] = A[q, q].real
    return A.diagonal().real.copy(), V, sweeps


def order(lam, fault=None):
    """the call sites' order: descending, equal values the lower index first (``tie_high``: the higher)"""
    sign = -1 if fault == "tie_high" else 1
    return np.array(sorted(range(len(lam)), key=lambda i: (-lam[i], sign * i)), dtype=np.int64)


def eigen(R, fault=None):
    """(lam descending [M], V [M, M] in that order, sweeps) by the restatement"""
    lam, V, sweeps = jacobi(R, fault)
    idx = order(lam, fault)
    return lam[idx], V[:, idx], sweeps


# ---- the cases ----------------------------------------------------------------------------------------------------------------
FAMILIES = ("floor+1", "floor+2eq", "floor+2near", "rank1", "rank2eq", "rank2", "rankM-1", "twin", "dead", "graded", "sub-tol",
            "diag", "scalar", "generic", "rank3")
LEADING_GAP = ("floor+1", "rank1", "graded", "twin", "generic")     # the beamformers' cases: one leader apart from the rest
HADAMARD8 = np.array([[1 - 2 * (bin(i & j).count("1") & 1) for j in range(8)] for i in range(8)], dtype=np.int64)
DIAG_AMPS = (3, 3, 2, 2, 2, 1, 1, 1)


def _gauss(rng, *shape, lim=1400):
    """Gaussian integers with |re|, |im| <= lim: magnitude <= sqrt(2) lim < 2^11 for the default"""
    return rng.integers(-lim, lim + 1, shape) + 1j * rng.integers(-lim, lim + 1, shape)


def _uv(M):
    """u = (1, i, 1, i, ...), v = (1, -i, 1, -i, ...), the last entry 0 for odd M: orthogonal, of equal norm"""
    u = np.array([1.0 if k % 2 == 0 else 1j for k in range(M)])
    if M % 2:
        u[-1] = 0.0
    return u, np.conj(u)


def _pad(frames, M):
    """frames: a list of [M] columns -> complex128 [M, T]"""
    X = np.zeros((M, T), np.complex128)
    for t, c in enumerate(frames):
        X[:, t] = c
    return X


def frames(family, M):
    """(X complex128 [M, n] of the case's n <= T non-zero frames before padding, the designed rank)"""
    rng = np.random.default_rng(7000 + 100 * FAMILIES.index(family) + M)
    eye = np.eye(M)
    u, v = _uv(M)
    gen = _gauss(rng, M, T)                                          # every family draws the same amount: one stream per case
    small = _gauss(rng, M, lim=15)
    small[small == 0] = 1 + 2j
    if family == "floor+1":
        cols, rank = [64 * eye[:, i] for i in range(M)] + [32 * small], M
    elif family in ("floor+2eq", "floor+2near"):
        cv = 1024 if family == "floor+2eq" else 1025
        cols, rank = [256 * eye[:, i] for i in range(M)] + [1024 * u, cv * v], M
    elif family == "rank1":
        cols, rank = [gen[:, 0]], 1
    elif family == "rank2eq":
        cols, rank = [1024 * u, 1024 * v], 2
    elif family == "rank2":
        cols, rank = [gen[:, 0], gen[:, 1]], min(2, M)
    elif family == "rank3":
        cols, rank = [gen[:, t] for t in range(min(3, M - 1))], min(3, M - 1)
    elif family == "rankM-1":
        cols, rank = [gen[:, t] for t in range(M - 1)], M - 1
    elif family == "twin":
        gen[1] = gen[0]
        cols, rank = list(gen.T), M - 1
    elif family == "dead":
        gen[M - 1] = 0
        cols, rank = list(gen.T), M - 1
    elif family == "graded":
        cols, rank = list((gen * (2.0 ** (-2.0 * np.arange(M)))[:, None]).T), M
    elif family == "sub-tol":
        gen[M // 2] *= 2.0 ** -30
        cols, rank = list(gen.T), M - 1
    elif family in ("diag", "scalar"):
        amps = np.array(DIAG_AMPS[:M] if family == "diag" else (2,) * M)
        cols, rank = list((amps[:, None] * HADAMARD8[:M]).T), M
    elif family == "generic":
        cols, rank = list(gen.T), M
    else:
        raise ValueError(family)
    return np.stack(cols, axis=1).astype(np.complex128), rank


@functools.lru_cache(maxsize=None)
def case(family, M):
    """dict(name, M, X complex64 [M, T] read-only, rank = the designed number of live eigenvalues)"""
    Xn, rank = frames(family, M)
    X = _pad(list(Xn.T), M).astype(np.complex64)
    assert np.array_equal(X.astype(np.complex128), _pad(list(Xn.T), M))          # the float32 holds it exactly
    X.setflags(write=False)
    return dict(name=family, M=M, X=X, rank=rank)


def null_space_draw(M, rank, seed):
    """complex128 [M, T]: ``rank`` generic Gaussian-integer frames, the rest zero -- a null space of dimension M - rank whose block
    of R becomes rounding noise once the live part has converged.  Exact as the cases are."""
    rng = np.random.default_rng(7800 + 100 * M + 10 * rank + 1000 * seed)
    X = np.zeros((M, T), np.complex128)
    X[:, :rank] = _gauss(rng, M, rank)
    return X


def cases(M, families=FAMILIES):
    return [case(f, M) for f in families]


def cov(X, frames_=None):
    """R = X X^H / T in float64 (T = the frame count of X unless given); exact for the cases of this module"""
    X = np.asarray(X).astype(np.complex128)
    return X @ X.conj().T / float(X.shape[1] if frames_ is None else frames_)


def cov_longdouble(X):
    """(Re R, Im R) as np.longdouble, summed frame by frame"""
    xr, xi = np.asarray(X).real.astype(np.longdouble), np.asarray(X).imag.astype(np.longdouble)
    rr = np.zeros((X.shape[0],) * 2, np.longdouble)
    ri = np.zeros((X.shape[0],) * 2, np.longdouble)
    for t in range(X.shape[1]):
        rr += np.outer(xr[:, t], xr[:, t]) + np.outer(xi[:, t], xi[:, t])
        ri += np.outer(xi[:, t], xr[:, t]) - np.outer(xr[:, t], xi[:, t])
    return rr / np.longdouble(X.shape[1]), ri / np.longdouble(X.shape[1])


# ---- figures and bars -----------------------------------------------------------------------------------------------------------
def fro(a):
    return float(np.sqrt((np.abs(np.asarray(a)) ** 2).sum()))


def backward(R, lam, V):
    return fro(R @ V - V * np.asarray(lam)[None, :]) / fro(R)


def rayleigh(R, V):
    """v_k^H R v_k for every column (0 for a zero column)"""
    return np.einsum("mk,mn,nk->k", V.conj(), R, V).real


def orth(V):
    V = np.asarray(V)
    return fro(V.conj().T @ V - np.eye(V.shape[1]))


def eigs(R, lam):
    w = np.linalg.eigvalsh(R)[::-1]
    return float(np.max(np.abs(np.sort(np.asarray(lam))[::-1] - w)) / w[0])


def noise_projector(V, S):
    """sum_{r >= S} v_r v_r^H of the columns of V, taken in their order"""
    N = np.asarray(V)[:, S:]
    return N @ N.conj().T


_REFS = {}


def reference(R):
    """what a case's figures are judged against, computed once per matrix: dict(R, w / E = eigh descending, lam / V / sweeps =
    the restatement in the call sites' order, live, bar_backward, bar_eigs, bar_orth)"""
    R = np.ascontiguousarray(R, np.complex128)
    key = R.tobytes()
    if key in _REFS:
        return _REFS[key]
    w, E = np.linalg.eigh(R)
    w, E = w[::-1].copy(), E[:, ::-1].copy()
    lam, V, sweeps = eigen(R)
    live = lam > RANK_TOL * lam[0]
    stop = np.sqrt(2.0) * 1e-14 * float(np.trace(R).real) / fro(R)
    b = stop + max(100.0 * backward(R, w, E), 1e-15)
    o = max(100.0 * orth(V[:, live]), 1e-14)
    _REFS[key] = dict(R=R, w=w, E=E, lam=lam, V=V, sweeps=sweeps, live=live, bar_backward=b, bar_eigs=b, bar_orth=o)
    return _REFS[key]


def gap(ref, S):
    """the relative gap (lam_{S-1} - lam_S) / lam_0 of eigh's eigenvalues"""
    return float((ref["w"][S - 1] - ref["w"][S]) / ref["w"][0])


def bar_proj(ref, S):
    """the Davis-Kahan bar of proj(S), or None where the gap does not qualify.  A backward bar near 1e-13 over a gap near
    GAP_MIN admits 3e-12: where Davis-Kahan admits more than BAR_CAP the bar is BAR_CAP, the tighter of the two (the
    restatement's worst proj on these cases is 1.5e-13, tests/test_eig_cases.py)"""
    g = gap(ref, S)
    return None if g < GAP_MIN else min(ref["bar_backward"] / g + ref["bar_orth"], BAR_CAP)


def proj(ref, P, S):
    """||P - P_noise(eigh)||_F for the split after the S leading eigenvalues"""
    return fro(np.asarray(P) - noise_projector(ref["E"], S))


def figures(R, lam, V, live=None, splits=()):
    """{name: (figure, bar)} of a solver's result on R: ``lam`` [M] and ``V`` [M, M] in descending order, ``live`` the columns
    that count (default: by the rank rule on lam).  proj(S) for every S of ``splits`` whose gap qualifies."""
    ref = reference(R)
    lam, V = np.asarray(lam, np.float64), np.asarray(V)
    live = lam > RANK_TOL * lam[0] if live is None else np.asarray(live)
    out = dict(backward=(backward(R, lam, V), ref["bar_backward"]), orth=(orth(V[:, live]), ref["bar_orth"]),
               eigs=(eigs(R, lam), ref["bar_eigs"]))
    for S in splits:
        bar = bar_proj(ref, S)
        if bar is not None:
            out[f"proj({S})"] = (proj(ref, noise_projector(V, S), S), bar)
    return out


def missed(fig):
    return [name for name, (v, bar) in fig.items() if not v <= bar]


def bits(x):
    """the bit patterns of a float or complex array"""
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[x.dtype.itemsize])


def tie_rule_holds(name, V):
    """``diag`` and ``scalar``: R is exactly diagonal and descending along the diagonal, so no rotation happens and the tie rule
    (equal ones: the lower index first) is decidable: the eigenvectors in the call sites' order are the identity, bit for bit"""
    V = np.asarray(V, np.complex128)
    return name not in ("diag", "scalar") or np.array_equal(bits(V), bits(np.eye(V.shape[0], dtype=np.complex128)))


def capped(fig):
    """every bar of ``fig`` is under BAR_CAP"""
    return all(bar <= BAR_CAP for _, bar in fig.values())


def show(fig):
    return "  ".join(f"{k} {v:.2e} (bar {b:.2e})" for k, (v, b) in fig.items())


def bar_span(ref, X):
    """the bar of ``A Y = X on the live span`` (AuxIVA's projection back, rel-L2 against ||X||) on the case X: 1e-12 wherever
    the restatement's own figure stays under 1e-12.  Where it does not (``graded`` at M = 7 alone: 3.3e-11, LAPACK's
    eigenvectors 6.5e-16), what the stopping rule admits: an off-diagonal remainder of eps = the backward bar leaves eps of the
    leading eigenvector e_0 in the computed e_k; A_k = X y_k^H / |y_k|^2 = e_k + eps (lam_0 / lam_k) e_0 then, and A_k y_k is
    wrong by that times |y_k| / ||X|| <= sqrt(lam_k / lam_0): eps sqrt(lam_0 / lam_k) for the smallest live eigenvalue, 9.6e-11
    there.  BAR_CAP does not apply to that one case."""
    ours = span_figure(X, ref["V"] * ref["live"][None, :])
    if ours <= 1e-12:
        return 1e-12
    w = ref["w"]
    live = w[w > RANK_TOL * w[0]]
    return max(1e-12, ref["bar_backward"] * float(np.sqrt(w[0] / live[-1])))


def span_figure(X, V, Y=None, A=None):
    """||A Y - E E^H X||_F / ||X||_F over the non-zero columns E of V; Y = V^H X and A = X Y^H / |y_k|^2 unless given"""
    X, V = np.asarray(X, np.complex128), np.asarray(V)
    Y = V.conj().T @ X if Y is None else np.asarray(Y)
    if A is None:
        den = (np.abs(Y) ** 2).sum(axis=1)
        A = (X @ Y.conj().T) / np.where(den != 0, den, 1.0)[None, :] * (den != 0)[None, :]
    E = V[:, V.any(axis=0)]
    return fro(A @ Y - E @ (E.conj().T @ X)) / fro(X)


def splits(M):
    """the source counts MUSIC is run with"""
    return sorted({S for S in (1, 2, min(3, M - 1)) if 1 <= S <= M - 1})


# ---- the beamformers' inputs ------------------------------------------------------------------------------------------------
def noise_frames(M, n, lim):
    """N complex128 [M, T - 1]: the frames n e_i and T - 1 - M generic Gaussian-integer frames, so that Phi_n = N N^H / T is
    n^2 / T I plus a generic integer part: positive definite.  The last frame stays free for a source."""
    rng = np.random.default_rng(7900 + M)
    return np.concatenate([n * np.eye(M, dtype=np.complex128), _gauss(rng, M, T - 1 - M, lim=lim)], axis=1)


def leading_gap_inputs(M):
    """(src complex64 [F, M, T], mix complex64 [F, M, T], the cases): Phi_s of bin f is the R of the f-th LEADING_GAP case and
    the residual mix - src is noise_frames(M) in every bin"""
    cs = cases(M, LEADING_GAP)
    src = np.stack([c["X"] for c in cs])
    mix = src.astype(np.complex128)
    mix[:, :, :T - 1] += noise_frames(M, n=256, lim=200)[None]
    return src, mix.astype(np.complex64), cs


def cluster_inputs(M, F=4):
    """(src, mix complex64 [F, M, T]): Phi_s = (k^2 u u^H + N N^H) / T and Phi_n = N N^H / T = L L^H, so that C = L^-1 Phi_s L^-H
    is the identity plus a rank-1 term: an (M - 1)-fold cluster that is degenerate only up to the rounding of L, under a leader
    of 15 ... 60.  u: a Gaussian-integer vector per bin, k = 64."""
    rng = np.random.default_rng(7950 + M)
    N = noise_frames(M, n=256, lim=100)
    src = np.zeros((F, M, T), np.complex128)
    src[:, :, :T - 1] = N[None]
    u = _gauss(rng, F, M, lim=15)
    u[u == 0] = 1 + 2j
    src[:, :, T - 1] = 64 * u
    mix = src.copy()
    mix[:, :, :T - 1] += N[None]
    return src.astype(np.complex64), mix.astype(np.complex64)
