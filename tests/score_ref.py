"""NumPy restatement (float64) of the scores of misonet_amd.score, independent of it: the wave statistics, SI-SDR / SNR from
statistics, the best permutation, and the spectral training criterion of the reference (criterion.py loss_uPIT /
loss_Enhance).  It is the definition the device code is held to."""
import itertools

import numpy as np

C16 = 1.0 / 32767.0          # what one unit of an int16 estimate stands for


def wave_stats(est, ref, n_valid=None):
    """est [E, n] (int16: sums over the raw values, scaled once at the end; or float), ref [R, n] -> float64 [E, R, 5] =
    (S e_i, S r_j, S e_i^2, S r_j^2, S e_i r_j) over samples [0, n_valid)"""
    est, ref = np.asarray(est), np.asarray(ref)
    n = est.shape[1] if n_valid is None else int(n_valid)
    c = C16 if est.dtype == np.int16 else 1.0
    e = est[:, :n].astype(np.float64)
    r = ref[:, :n].astype(np.float64)
    out = np.zeros((e.shape[0], r.shape[0], 5), dtype=np.float64)
    for i in range(e.shape[0]):
        for j in range(r.shape[0]):
            out[i, j] = (e[i].sum() * c, r[j].sum(), (e[i] * e[i]).sum() * (c * c), (r[j] * r[j]).sum(),
                         (e[i] * r[j]).sum() * c)
    return out


def combine(stats_list, n_list):
    """a recording of K chunks: the sum of its K stat blocks and of their valid counts"""
    total = np.zeros_like(np.asarray(stats_list[0], dtype=np.float64))
    for s in stats_list:
        total = total + np.asarray(s, dtype=np.float64)
    return total, int(sum(n_list))


def _one(st, n):
    se, sr, see, srr, ser = (float(v) for v in st)
    n = float(n)
    return see - se * se / n, srr - sr * sr / n, ser - se * sr / n


def si_sdr_one(st, n):
    """one block of 5 sums -> SI-SDR in dB (zero-mean form of Le Roux et al. 2019)"""
    cee, crr, cer = _one(st, n)
    if not crr > 0:
        return float("nan")
    target = cer * cer / crr
    noise = max(cee - target, 0.0)
    if noise == 0.0:
        return float("inf") if target > 0 else float("nan")
    if target == 0.0:
        return float("-inf")
    return 10.0 * np.log10(target / noise)


def snr_one(st, n):
    cee, crr, cer = _one(st, n)
    if not crr > 0:
        return float("nan")
    err = max(crr - 2.0 * cer + cee, 0.0)
    if err == 0.0:
        return float("inf")
    return 10.0 * np.log10(crr / err)


def si_sdr(stats, n):
    st = np.asarray(stats, dtype=np.float64)
    out = np.empty(st.shape[:-1], dtype=np.float64)
    for idx in np.ndindex(*st.shape[:-1]):
        out[idx] = si_sdr_one(st[idx], n)
    return out


def snr(stats, n):
    st = np.asarray(stats, dtype=np.float64)
    out = np.empty(st.shape[:-1], dtype=np.float64)
    for idx in np.ndindex(*st.shape[:-1]):
        out[idx] = snr_one(st[idx], n)
    return out


def valid(stats, n):
    """[R] bool: reference j is not silent (Crr > 0)"""
    st = np.asarray(stats, dtype=np.float64)
    return np.array([_one(st[0, j], n)[1] > 0 for j in range(st.shape[1])])


def best_perm(M):
    """M [S, S] (estimate, reference) -> p, p[j] = the estimate of reference j: the first permutation in itertools order that
    maximises sum_j M[p[j], j]; a permutation with a non-finite term loses"""
    M = np.asarray(M, dtype=np.float64)
    S = M.shape[0]
    best, vbest = None, None
    for p in itertools.permutations(range(S)):
        v = 0.0
        for j in range(S):
            t = M[p[j], j]
            v = v + t if np.isfinite(t) and np.isfinite(v) else -np.inf
        if best is None or v > vbest:
            best, vbest = list(p), v
    return best


def score(est, ref, mix=None, n_valid=None):
    """est [S, n], ref [S, n], mix [n] or None -> dict of the figures misonet_amd.score.Score holds"""
    est, ref = np.asarray(est), np.asarray(ref)
    n = est.shape[1] if n_valid is None else int(n_valid)
    st = wave_stats(est, ref, n)
    return score_from_stats(st, n, wave_stats(np.asarray(mix)[None], ref, n) if mix is not None else None)


def score_from_stats(st, n, st_mix=None):
    S = st.shape[0]
    M = si_sdr(st, n)
    p = best_perm(M)
    out = dict(si_sdr=np.array([M[j, j] for j in range(S)]), snr=np.array([snr_one(st[j, j], n) for j in range(S)]),
               valid=valid(st, n), perm_best=p, si_sdr_best=np.array([M[p[j], j] for j in range(S)]), n_samples=n,
               si_sdr_mix=None, si_sdri=None)
    if st_mix is not None:
        out["si_sdr_mix"] = si_sdr(np.asarray(st_mix).reshape(S, 5), n)
        out["si_sdri"] = out["si_sdr"] - out["si_sdr_mix"]
    return out


def spec_pair(e, r):
    """e, r complex [T, F] -> sum |Re e - Re r| + |Im e - Im r| + | sqrt(Re e^2 + Im e^2 + 1e-8) - |r| |: each term in float32
    as the reference forms it (criterion.py:36-39, 131-135), summed in float64"""
    e = np.asarray(e, dtype=np.complex64)
    r = np.asarray(r, dtype=np.complex64)
    er, ei = e.real.astype(np.float32), e.imag.astype(np.float32)
    rr, ri = r.real.astype(np.float32), r.imag.astype(np.float32)
    t1 = np.abs(er - rr)
    t2 = np.abs(ei - ri)
    mag = np.sqrt(er * er + ei * ei + np.float32(1e-8))
    t3 = np.abs(mag - np.abs(r).astype(np.float32))
    return float(t1.astype(np.float64).sum() + t2.astype(np.float64).sum() + t3.astype(np.float64).sum())


def spec_pairs(est, ref):
    """est complex [E, T, F], ref complex [R, T, F] -> float64 [E, R]"""
    return np.array([[spec_pair(e, r) for r in ref] for e in est], dtype=np.float64)


def upit(pair):
    """pair [S, S] -> (min over the permutations of sum_i pair[i][p(i)], p): itertools order, first minimum"""
    pair = np.asarray(pair, dtype=np.float64)
    S = pair.shape[0]
    best, vbest = None, None
    for p in itertools.permutations(range(S)):
        v = 0.0
        for i in range(S):
            v += pair[i, p[i]]
        if best is None or v < vbest:
            best, vbest = list(p), v
    return vbest, best


def loss_enhance(est, ref):
    """aligned output: est, ref [S, T, F] -> [S], pair[j][j]"""
    return np.array([spec_pair(est[j], ref[j]) for j in range(len(est))])
