"""BSS-eval SDR / SIR / SAR (Vincent, Gribonval, Fevotte 2006; mir_eval.separation.bss_eval_sources) restated in NumPy / SciPy,
in two independent forms, plus the test signals of tests/test_bss.py and tests/test_gpu_bss.py.

  * :func:`explicit` -- the oracle.  The way mir_eval does it: correlations by FFT, the filters from ``np.linalg.solve``
    (LU), the projections as explicit convolutions, and the figures from the energies of the SIGNALS s_target, e_interf,
    e_artif.
  * :func:`energies` / :func:`figures` -- the energy form the device computes: correlations as direct float64 sums, Cholesky
    factors, and the figures from T_ij = d^T G_jj^-1 d, A_i = D^T G^-1 D and Eee_i alone (the projections are orthogonal, so
    |s_target|^2 = T, |e_interf|^2 = A - T, |e_artif|^2 = Eee - A).

  * :func:`solve_energies` / :func:`solve_bound` / :func:`blocked` -- the solver on its own input: the energy form from GIVEN
    correlations with the condition numbers that bound its forward error, and the panel scheme of the device restated in
    NumPy, which takes planted faults (``SOLVE_SHAPES``: every panel width the device admits).

float64 throughout; every signal is zero outside [0, n); an int16 estimate stands for q / 32767.
"""
import itertools

import numpy as np
import scipy.linalg
import scipy.signal

PIVOT_RATIO = 2.0 ** -40


def as_f64(est):
    est = np.asarray(est)
    return est.astype(np.float64) / 32767.0 if est.dtype == np.int16 else est.astype(np.float64)


# ---- the explicit (mir_eval) form -------------------------------------------------------------------------------------
def _fft_corr(x, y, Q, nfft):
    """c[a] = sum_t x[t] y[t + a] for a in (-Q, Q): returns (c[0..Q-1], c[0], c[-1], ..., c[-(Q-1)])"""
    c = np.fft.irfft(np.conj(np.fft.rfft(x, nfft)) * np.fft.rfft(y, nfft), nfft)
    return c[:Q], np.concatenate((c[:1], c[:-Q:-1]))


def _project(refs, e, Q):
    """least-squares projection of e on the span of the references delayed by 0 .. Q - 1: the projected signal [L + Q - 1]"""
    R, L = refs.shape
    nfft = int(2 ** np.ceil(np.log2(L + Q)))
    G = np.zeros((R * Q, R * Q))
    for j in range(R):
        for k in range(R):
            pos, neg = _fft_corr(refs[j], refs[k], Q, nfft)         # G[(j,a),(k,b)] = c_jk[a - b]
            G[j * Q:(j + 1) * Q, k * Q:(k + 1) * Q] = scipy.linalg.toeplitz(pos, neg)
    D = np.concatenate([_fft_corr(refs[j], e, Q, nfft)[0] for j in range(R)])
    C = np.linalg.solve(G, D).reshape(R, Q)
    out = np.zeros(L + Q - 1)
    for j in range(R):
        out += np.convolve(refs[j], C[j])
    return out


def explicit(est, refs, Q=512):
    """est [E, L] (int16 or float), refs [R, L] -> (SDR [E, R], SIR [E, R], SAR [E]) in dB, from the signals"""
    est, refs = as_f64(est), np.asarray(refs, dtype=np.float64)
    E, L = est.shape
    R = refs.shape[0]
    sdr, sir, sar = np.zeros((E, R)), np.zeros((E, R)), np.zeros(E)
    for i in range(E):
        e = np.concatenate((est[i], np.zeros(Q - 1)))
        p_all = _project(refs, est[i], Q)
        e_artif = e - p_all
        for j in range(R):
            s_target = _project(refs[j:j + 1], est[i], Q)
            e_interf = p_all - s_target
            sdr[i, j] = 10 * np.log10(np.sum(s_target ** 2) / np.sum((e_interf + e_artif) ** 2))
            with np.errstate(divide="ignore"):                       # one reference: no interference, SIR = +inf
                sir[i, j] = 10 * np.log10(np.sum(s_target ** 2) / np.sum(e_interf ** 2))
        sar[i] = 10 * np.log10(np.sum(p_all ** 2) / np.sum(e_artif ** 2))
    return sdr, sir, sar


# ---- the energy form ----------------------------------------------------------------------------------------------------
def corr(x, y, Q):
    """c[a] = sum_t x[t] y[t + a], a in [0, Q), as float64 dot products"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    L = x.shape[0]
    return np.array([np.dot(x[:L - a], y[a:]) if a < L else 0.0 for a in range(Q)])


def corr_abs(x, y, Q):
    """sum_t |x[t]| |y[t + a]|: the scale of the rounding error of corr"""
    return corr(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(y, dtype=np.float64)), Q)


def correlations(est, refs, Q):
    """-> Rrr [R, R, Q], Rre [R, E, Q], Eee [E]"""
    est, refs = as_f64(est), np.asarray(refs, dtype=np.float64)
    R, E = refs.shape[0], est.shape[0]
    Rrr = np.array([[corr(refs[j], refs[k], Q) for k in range(R)] for j in range(R)])
    Rre = np.array([[corr(refs[j], est[i], Q) for i in range(E)] for j in range(R)])
    return Rrr, Rre, np.array([np.dot(est[i], est[i]) for i in range(E)])


def gram(Rrr, silent=None):
    R, _, Q = Rrr.shape
    G = np.zeros((R * Q, R * Q))
    for j in range(R):
        for k in range(R):
            if silent is not None and (silent[j] or silent[k]):
                blk = np.eye(Q) if j == k else np.zeros((Q, Q))
            else:
                blk = scipy.linalg.toeplitz(Rrr[j, k], Rrr[k, j])     # first column Rrr[j][k], first row Rrr[k][j]
            G[j * Q:(j + 1) * Q, k * Q:(k + 1) * Q] = blk
    return G


def cholesky_info(G):
    """(L, info): Cholesky with the pivot rule of the device: info = -1, or the first row whose
    pivot is <= 2^-40 of the diagonal entry of G or not finite (L is None then)"""
    n = G.shape[0]
    d0 = np.diag(G).copy()
    try:
        Lf = np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        Lf = None
    if Lf is not None:
        piv = np.diag(Lf) ** 2
        bad = np.nonzero(~(piv > d0 * PIVOT_RATIO) | ~np.isfinite(piv))[0]
        if bad.size == 0:
            return Lf, -1
    # locate the first failing pivot column by column
    A = np.array(G, dtype=np.float64)
    for c in range(n):
        piv = A[c, c]
        if not (piv > d0[c] * PIVOT_RATIO) or not np.isfinite(piv):
            return None, c
        A[c:, c] /= np.sqrt(piv)
        A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], A[c + 1:, c])
    return np.tril(A), -1


def energies(est, refs, Q=512):
    """-> (T [E, R], A [E], Eee [E], valid [R], info): the energy form with NumPy / SciPy Cholesky"""
    Rrr, Rre, Eee = correlations(est, refs, Q)
    R, E = Rrr.shape[0], Rre.shape[1]
    silent = np.array([Rrr[j, j, 0] == 0 for j in range(R)])
    Lf, info = cholesky_info(gram(Rrr, silent))
    T, A = np.full((E, R), np.nan), np.full(E, np.nan)
    if info < 0:
        for i in range(E):
            D = np.concatenate([np.zeros(Q) if silent[j] else Rre[j, i] for j in range(R)])
            y = scipy.linalg.solve_triangular(Lf, D, lower=True)
            A[i] = np.dot(y, y)
            for j in range(R):
                if silent[j]:
                    T[i, j] = 0.0
                    continue
                Lj = np.linalg.cholesky(scipy.linalg.toeplitz(Rrr[j, j]))
                yj = scipy.linalg.solve_triangular(Lj, Rre[j, i], lower=True)
                T[i, j] = np.dot(yj, yj)
    return T, A, Eee, ~silent, info


def _db(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(num / np.maximum(den, 0.0))


def figures(T, A, Eee, valid=None, ok=True, T_mix=None, Eee_mix=None):
    """The rules of the issue, restated: -> dict of sdr, sir, sar, valid, ok, perm_best, *_best, sdr_mix, sdri"""
    T, A, Eee = np.asarray(T, np.float64), np.asarray(A, np.float64), np.asarray(Eee, np.float64)
    S = T.shape[0]
    valid = np.ones(S, bool) if valid is None else np.asarray(valid, bool)
    sdr_m, sir_m, sar = np.empty((S, S)), np.empty((S, S)), np.empty(S)
    for i in range(S):
        sar[i] = _db(A[i], Eee[i] - A[i]) if ok else np.nan
        for j in range(S):
            good = ok and valid[j]
            sdr_m[i, j] = _db(T[i, j], Eee[i] - T[i, j]) if good else np.nan
            sir_m[i, j] = _db(T[i, j], A[i] - T[i, j]) if good else np.nan
    best, vbest = None, None
    for p in itertools.permutations(range(S)):                       # mir_eval's rule: mean SIR, first optimum
        terms = [sir_m[p[j], j] for j in range(S)]
        v = float(sum(terms)) if all(np.isfinite(t) for t in terms) else -np.inf
        if best is None or v > vbest:
            best, vbest = list(p), v
    out = dict(sdr=np.diag(sdr_m).copy(), sir=np.diag(sir_m).copy(), sar=sar, valid=valid, ok=bool(ok), perm_best=best,
               sdr_best=np.array([sdr_m[best[j], j] for j in range(S)]),
               sir_best=np.array([sir_m[best[j], j] for j in range(S)]),
               sar_best=np.array([sar[best[j]] for j in range(S)]), sdr_mix=None, sdri=None, sdr_matrix=sdr_m,
               sir_matrix=sir_m)
    if T_mix is not None:
        tm = np.asarray(T_mix, np.float64)
        out["sdr_mix"] = np.array([_db(tm[j], Eee_mix - tm[j]) if ok and valid[j] else np.nan for j in range(S)])
        out["sdri"] = out["sdr"] - out["sdr_mix"]
    return out


# ---- the test signals -----------------------------------------------------------------------------------------------------
KINDS = ("white", "ar2", "lp50", "lp25")
LENGTHS = (5000, 16000, 64000)
FILT_LENS = (64, 512)
SPEAKERS = (1, 2, 3)


# The low-pass sources carry a white floor 84 dB under the signal.  A Butterworth stop band alone falls to the float32
# rounding of the samples, and what is left up there is the leakage of the two cut edges, a few shapes shared by all
# references: with three references G is singular to working precision (cond 1e13 at 5000 samples and 64 lags; at 512 lags
# NumPy's Cholesky raises).  The floor puts cond(G) where the ceilings of the tests (1e-7 dB between the two CPU forms, 1e-6 dB
# device against oracle) were derived, 1e9 .. 1e10: the largest of all cases is 7e9 (quarter band, S = 3, L = 5000, Q = 512),
# the smallest pivot ratio 5e-5.
LP_FLOOR = 10.0 ** (-84.0 / 20.0)


def sources(kind, S, L, seed):
    """float32 [S, L]: white noise, AR(2)-coloured noise, Butterworth low-pass at 0.5 (order 6) / 0.25 (order 8) of Nyquist"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((S, L + 512))
    if kind == "white":
        x = w
    elif kind == "ar2":
        x = scipy.signal.lfilter([1.0], [1.0, -1.2, 0.6], w, axis=1)
    elif kind == "lp50":
        x = scipy.signal.lfilter(*scipy.signal.butter(6, 0.5), w, axis=1)
    elif kind == "lp25":
        x = scipy.signal.lfilter(*scipy.signal.butter(8, 0.25), w, axis=1)
    else:
        raise ValueError(kind)
    x = x[:, 512:]
    x = x / np.sqrt(np.mean(x ** 2, axis=1, keepdims=True))
    if kind in ("lp50", "lp25"):
        x = x + LP_FLOOR * rng.standard_normal((S, L))
    return (0.1 * x).astype(np.float32)


def estimates(refs, seed, noise=0.02):
    """int16 [S, L]: every estimate = its source through a 40-tap filter + 0.15 of every other source through another one +
    white noise, quantised as the pipeline's output is"""
    rng = np.random.default_rng(seed + 1000)
    S, L = refs.shape
    out = np.zeros((S, L))
    for i in range(S):
        for j in range(S):
            h = rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0)
            h[0] += 2.0
            h /= np.sqrt(np.sum(h ** 2))
            out[i] += (1.0 if i == j else 0.15) * np.convolve(refs[j].astype(np.float64), h)[:L]
        out[i] += noise * 0.1 * rng.standard_normal(L)
    return np.clip(np.rint(out * 32767.0), -32768, 32767).astype(np.int16)


def case(kind, S, L, seed=0):
    refs = sources(kind, S, L, seed + 17 * S + L)
    return estimates(refs, seed + 17 * S + L), refs


def all_cases():
    return [(k, S, L, Q) for k in KINDS for S in SPEAKERS for L in LENGTHS for Q in FILT_LENS]


# ---- the solver on its own input --------------------------------------------------------------------------------------------
# The estimates above pass every source through 40 taps, so a right-hand side carries its energy in the first 40 lags of each
# block and the late columns of the forward substitution hold 1e-6 of A: a wrong element there is invisible.  The estimates
# below pass every source through Q taps; the last 16 columns of L^-1 D then hold 1e-3 of A and more.
def long_estimates(refs, Q, seed, E=None, noise=0.05):
    """int16 [E, L]: estimate i = sum_j g_ij (refs[j] * h_ij)[:L] + noise * 0.1 * white noise, g_ij = 1 where i % R == j and
    0.3 elsewhere, h_ij = Q Gaussian taps of unit norm (every lag carries energy), quantised as :func:`estimates` does"""
    rng = np.random.default_rng(seed + 2000)
    R, L = refs.shape
    E = R if E is None else E
    out = np.zeros((E, L))
    for i in range(E):
        for j in range(R):
            h = rng.standard_normal(Q)
            h /= np.sqrt(np.sum(h ** 2))
            out[i] += (1.0 if i % R == j else 0.3) * np.convolve(refs[j].astype(np.float64), h)[:L]
        out[i] += noise * 0.1 * rng.standard_normal(L)
    return np.clip(np.rint(out * 32767.0), -32768, 32767).astype(np.int16)


def long_case(kind, R, E, Q, L, seed=0):
    refs = sources(kind, R, L, seed + 17 * R + L)
    return long_estimates(refs, Q, seed + 17 * R + L, E), refs


# (R, E, Q, L): what each shape reaches in the panel scheme of the device (panels of 64 columns)
SOLVE_SHAPES = (
    (1, 1, 16, 2000),        # one panel of width 16, systems 0 and 1 of the same order
    (3, 2, 16, 2000),        # N = 48: a single narrow panel, one row block, E != R
    (2, 2, 48, 4000),        # the order-Q systems end narrow in panel 0 while system 0 goes on; its last panel is 32 wide
    (1, 4, 48, 4000),        # four extra rows behind a 48-wide panel
    (4, 4, 80, 8000),        # N = 320 is whole panels, the order-Q systems end 16 wide at column 64; R = E = 4
    (4, 1, 80, 8000),        # the mixture-row shape at R = 4
    (3, 3, 272, 16000),      # N = 816 = 12 * 64 + 48, Q = 4 * 64 + 16
    (1, 1, 1008, 16000),     # 15 full panels and one of 48
    (4, 4, 64, 8000),        # R = 4 at a friendly order (separates "R = 4" from "narrow panel")
    (2, 2, 1024, 32000),     # the largest Q
    (4, 4, 1024, 64000),     # the admitted maximum N = 4096: white only
)
SOLVE_KINDS = ("white", "ar2")
FULL_SIZE = (4, 4, 1024, 64000)


def solve_cases():
    return [(k,) + s for s in SOLVE_SHAPES for k in SOLVE_KINDS if s != FULL_SIZE or k == "white"]


def _silent(Rrr):
    return np.array([Rrr[j, j, 0] == 0 for j in range(Rrr.shape[0])])


def solve_energies(Rrr, Rre, solver="chol", cond=True):
    """Rrr [R, R, Q], Rre [R, E, Q] -> (T [E, R], A [E], info, cond): the energies from GIVEN correlations, with the silent
    rule and the pivot rule of :func:`energies`.  ``solver="chol"``: Cholesky factor and triangular solve; ``"lu"``:
    D^T solve(G, D).  cond = [cond_2(G), cond_2(G_00), ...] (None with ``cond=False``)."""
    Rrr, Rre = np.asarray(Rrr, np.float64), np.asarray(Rre, np.float64)
    R, E, Q = Rre.shape
    silent = _silent(Rrr)
    G = gram(Rrr, silent)
    Lf, info = cholesky_info(G)
    blocks = [np.eye(Q) if silent[j] else scipy.linalg.toeplitz(Rrr[j, j]) for j in range(R)]
    conds = [float(np.linalg.cond(M)) for M in [G] + blocks] if cond else None
    T, A = np.full((E, R), np.nan), np.full(E, np.nan)
    if info < 0:
        for i in range(E):
            D = np.concatenate([np.zeros(Q) if silent[j] else Rre[j, i] for j in range(R)])
            if solver == "chol":
                y = scipy.linalg.solve_triangular(Lf, D, lower=True)
                A[i] = np.dot(y, y)
            else:
                A[i] = np.dot(D, np.linalg.solve(G, D))
            for j in range(R):
                if silent[j]:
                    T[i, j] = 0.0
                elif solver == "chol":
                    yj = scipy.linalg.solve_triangular(np.linalg.cholesky(blocks[j]), Rre[j, i], lower=True)
                    T[i, j] = np.dot(yj, yj)
                else:
                    T[i, j] = np.dot(Rre[j, i], np.linalg.solve(blocks[j], Rre[j, i]))
    return T, A, info, conds


def solve_bound(N, cond):
    """relative: the first-order forward error of one Cholesky factorisation, one triangular solve and one dot product of
    order N is about 3 N u cond, rounded up to 4.  For A: N = R Q and cond(G); for T[., j]: N = Q and cond(G_jj)."""
    return 4.0 * N * 2.0 ** -53 * cond


FAULTS = ("last_group", "tail_tile", "extra_row", "short_system", "pad_pivot")


def blocked(Rrr, Rre, nb=64, fault=None, hit=None):
    """-> (T [E, R], A [E], info): the scheme of the device restated in NumPy float64 (the scheme, not its code).  Per item
    1 + R systems -- system 0 = G of order N = R Q over D, system 1 + j = G_jj of order Q over d_.j -- each held as its lower
    triangle with the E right-hand sides as extra ROWS under it.  One loop over panels of ``nb`` columns advances every system
    that still has the panel: the diagonal block (a narrow last panel padded by the identity) is factored column by column
    with the pivot rule on system 0, the rows under it are solved against it in groups of 16 columns, then the trailing
    lower triangle and the extra rows take C -= P_i P_j^T column tile by column tile.  After the last panel the extra rows
    hold (L^-1 D)^T; T and A are their squared norms.

    ``fault`` plants one mistake of the kind the narrow panels and the early end of a short system invite (``hit``, a list,
    receives the fault's name when the shape reaches the place):
      last_group    the last 16-column group of a narrow last panel is left unsolved
      tail_tile     the partial last column tile is skipped by the trailing update of panel 0
      extra_row     the last extra row is missed by the trailing update of panel 0
      short_system  an order-Q system takes system 0's panel width in its narrow last panel: its extra rows, which start at
                    column-panel width w of its OWN order, are not among the rows solved
      pad_pivot     the pivot rule also looks at the padded rows.  No diagonal entry of G matches such a row, what is read
                    for it is arbitrary: the restatement takes the worst case, an entry the pivot 1 does not pass"""
    Rrr, Rre = np.asarray(Rrr, np.float64), np.asarray(Rre, np.float64)
    R, E, Q = Rre.shape
    N = R * Q
    silent = _silent(Rrr)
    note = (lambda: hit.append(fault)) if hit is not None else (lambda: None)
    D = np.array([np.concatenate([np.zeros(Q) if silent[j] else Rre[j, i] for j in range(R)]) for i in range(E)])
    systems = [np.vstack([np.tril(gram(Rrr, silent)), D])]
    for j in range(R):
        Gj = np.eye(Q) if silent[j] else scipy.linalg.toeplitz(Rrr[j, j])
        systems.append(np.vstack([np.tril(Gj), D[:, j * Q:(j + 1) * Q]]))
    gd = np.repeat([1.0 if silent[j] else Rrr[j, j, 0] for j in range(R)], Q)
    T, A = np.full((E, R), np.nan), np.full(E, np.nan)
    for pc in range(0, N, nb):
        for s, M in enumerate(systems):
            n = M.shape[1]
            if pc >= n:
                continue
            w = min(nb, n - pc)
            Lb = np.eye(nb)
            Lb[:w, :w] = np.tril(M[pc:pc + w, pc:pc + w])
            for c in range(nb):
                piv = Lb[c, c]
                if s == 0 and (c < w or fault == "pad_pivot"):
                    if c >= w:
                        note()
                    g = gd[pc + c] if c < w else np.inf
                    if not (piv > g * PIVOT_RATIO) or not np.isfinite(piv):
                        return T, A, pc + c
                Lb[c, c] = np.sqrt(piv)
                Lb[c + 1:, c] /= Lb[c, c]
                Lb[c + 1:, c + 1:] -= np.tril(np.outer(Lb[c + 1:, c], Lb[c + 1:, c]))
            rows = M[pc + w:]                                        # w < nb only in a last panel: the extra rows follow
            if fault == "short_system" and s > 0 and w < nb and min(nb, N - pc) > w:
                note()
                rows = rows[:0]
            groups = list(range(0, w, 16))
            if fault == "last_group" and w < nb:
                note()
                groups = groups[:-1]
            for cb in groups:
                X = rows[:, pc + cb:pc + cb + 16] - rows[:, pc:pc + cb] @ Lb[cb:cb + 16, :cb].T
                rows[:, pc + cb:pc + cb + 16] = scipy.linalg.solve_triangular(Lb[cb:cb + 16, cb:cb + 16], X.T, lower=True).T
        for s, M in enumerate(systems):                              # C -= P_i P_j^T behind the panel
            n = M.shape[1]
            P = M[:, pc:pc + nb]
            for j0 in range(pc + nb, n, nb):                         # (nothing where pc + nb >= n)
                j1 = min(j0 + nb, n)
                if fault == "tail_tile" and pc == 0 and j1 - j0 < nb:
                    note()
                    continue
                i1 = n + E
                if fault == "extra_row" and pc == 0:
                    note()
                    i1 -= 1
                for i0 in range(j0, i1, nb):                         # nb x nb tiles, the last of a strip partial
                    M[i0:min(i0 + nb, i1), j0:j1] -= P[i0:min(i0 + nb, i1)] @ P[j0:j1].T
    for i in range(E):
        A[i] = np.dot(systems[0][N + i], systems[0][N + i])
        for j in range(R):
            T[i, j] = np.dot(systems[1 + j][Q + i], systems[1 + j][Q + i])
    return T, A, -1
