"""Scores of separated output against clean references: SI-SDR and its improvement over the mixture, SNR, the best
permutation, and the reference's training criterion (criterion.py ``loss_uPIT`` / ``loss_Enhance``).  The sums run on the
device (csrc/score.hip, C ABI ``misonet_score_wave`` / ``misonet_score_spec``); the handful of doubles they leave is turned
into dB on the host.  tests/score_ref.py restates every definition in NumPy.  BSS-eval SDR, SIR and SAR (Vincent et al. 2006,
the figures SMS-WSJ tabulates) come from the energies of two projections (csrc/bss.hip, C ABI ``misonet_bss_corr`` /
``misonet_bss_solve``; :class:`BssEval`, INTEGRATION.md 4e, restated in tests/bss_ref.py).  STOI and ESTOI, the intelligibility
figures, are computed whole on the device (csrc/stoi.hip, C ABI ``misonet_stoi_resample`` / ``misonet_stoi_measure``;
:class:`Stoi`, INTEGRATION.md 4f, restated in tests/stoi_ref.py).  Cepstral distance, log-likelihood ratio and
frequency-weighted segmental SNR, the figures dereverberation is judged by, likewise (csrc/reverb.hip, C ABI
``misonet_reverb_measure``; :class:`Reverb`, INTEGRATION.md 4j, restated in tests/reverb_ref.py).  SRMR, the one figure that
takes no clean reference, is at the end (csrc/srmr.hip, ``misonet_srmr_measure``; :class:`Srmr`, INTEGRATION.md 4k,
tests/srmr_ref.py).

Definitions:
  * stats[i][j] = (S e_i, S r_j, S e_i^2, S r_j^2, S e_i r_j) over the valid samples; additive over the chunks of a recording;
    an int16 estimate stands for q / 32767 (sums over q, scaled once);
  * Cee = S e^2 - (S e)^2 / n, Crr, Cer likewise; target = Cer^2 / Crr, noise = max(Cee - target, 0);
    SI-SDR = 10 log10(target / noise) (Le Roux et al. 2019, zero-mean); SNR = 10 log10(Crr / max(Crr - 2 Cer + Cee, 0));
    Crr == 0 (a silent reference): NaN, ``valid = False``;
  * best permutation: the first of the S! (itertools order) that maximises sum_j SI-SDR(e_p(j), r_j); a non-finite term
    makes a permutation lose;
  * spectral criterion per pair: sum_{t,f} |Re e - Re r| + |Im e - Im r| + | sqrt(Re e^2 + Im e^2 + 1e-8) - |r| |.
"""
from __future__ import annotations

import dataclasses
import itertools
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

PIECE = 1 << 20      # samples per device call of score_waves: memory does not grow with the length of the recording


# ---- host side: float64 NumPy, no GPU ----------------------------------------------------------------------------------
def combine(stats_list: Sequence[np.ndarray], n_list: Sequence[int]) -> Tuple[np.ndarray, int]:
    """The statistics of a recording from those of its chunks: (sum of the blocks in list order, sum of the counts)."""
    if len(stats_list) == 0 or len(stats_list) != len(n_list):
        raise ValueError("stats_list and n_list must be non-empty and of equal length")
    total = np.array(stats_list[0], dtype=np.float64, copy=True)
    for s in stats_list[1:]:
        total = total + np.asarray(s, dtype=np.float64)
    return total, int(sum(int(n) for n in n_list))


def _centred(stats, n):
    st = np.asarray(stats, dtype=np.float64)
    if st.shape[-1] != 5:
        raise ValueError("stats must end in the 5 sums (S e, S r, S e^2, S r^2, S e r)")
    if int(n) < 1:
        raise ValueError(f"n must be positive (got {n})")
    n = float(int(n))
    se, sr, see, srr, ser = (st[..., k] for k in range(5))
    return see - se * se / n, srr - sr * sr / n, ser - se * sr / n


def si_sdr(stats, n) -> np.ndarray:
    """stats [..., 5], n valid samples -> SI-SDR in dB [...] (NaN where the reference is silent, +inf where noise == 0)"""
    cee, crr, cer = _centred(stats, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        target = np.where(crr > 0, cer * cer / np.where(crr > 0, crr, 1.0), np.nan)
        noise = np.maximum(cee - target, 0.0)
        return 10.0 * np.log10(target / noise)


def snr(stats, n) -> np.ndarray:
    """stats [..., 5] -> SNR in dB [...]: 10 log10(Crr / max(Crr - 2 Cer + Cee, 0)), NaN where the reference is silent"""
    cee, crr, cer = _centred(stats, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.maximum(crr - 2.0 * cer + cee, 0.0)
        return np.where(crr > 0, 10.0 * np.log10(np.where(crr > 0, crr, 1.0) / err), np.nan)


def best_perm(si_sdr_matrix) -> List[int]:
    """si_sdr_matrix [S estimates, S references] -> p with p[j] = the estimate that goes with reference j: the first
    permutation (itertools order) with the largest sum_j M[p[j], j]; a non-finite term makes a permutation lose."""
    M = np.asarray(si_sdr_matrix, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("si_sdr_matrix must be square")
    S = M.shape[0]
    best, vbest = None, None
    for p in itertools.permutations(range(S)):
        terms = [M[p[j], j] for j in range(S)]
        v = float(sum(terms)) if all(np.isfinite(t) for t in terms) else -np.inf
        if best is None or v > vbest:
            best, vbest = list(p), v
    return best


def upit(pair) -> Tuple[float, List[int]]:
    """pair [S, S] -> (the least sum_i pair[i][p(i)] over the permutations, p): itertools order, first minimum"""
    P = np.asarray(pair, dtype=np.float64)
    S = P.shape[0]
    best, vbest = None, None
    for p in itertools.permutations(range(S)):
        v = 0.0
        for i in range(S):
            v += P[i, p[i]]
        if best is None or v < vbest:
            best, vbest = list(p), v
    return float(vbest), best


def _lst(x):
    return None if x is None else [float(v) for v in np.asarray(x, dtype=np.float64)]


@dataclasses.dataclass
class Score:
    """The scores of one recording, speaker j = reference j.  ``perm_best != identity`` means that the magnitude alignment
    of the pass and the SI-SDR disagree about who is who: it is reported, nothing acts on it."""
    si_sdr: np.ndarray                    # [S] SI-SDR(e_j, r_j), dB
    si_sdr_mix: Optional[np.ndarray]      # [S] SI-SDR(mixture at ref_ch, r_j), or None without a mixture
    si_sdri: Optional[np.ndarray]         # [S] si_sdr - si_sdr_mix
    snr: np.ndarray                       # [S] SNR(e_j, r_j), dB
    valid: np.ndarray                     # [S] bool: reference j is not silent
    perm_best: List[int]                  # p[j] = the estimate with the best SI-SDR assignment to reference j
    si_sdr_best: np.ndarray               # [S] SI-SDR(e_p[j], r_j)
    n_samples: int
    loss_miso1: Optional[float] = None    # uPIT value of the MISO1 estimate at ref_ch (criterion.py loss_uPIT), per item
    loss_enhance: Optional[np.ndarray] = None   # [S] criterion.py loss_Enhance of output j against reference j

    def as_dict(self) -> dict:
        return dict(si_sdr=_lst(self.si_sdr), si_sdr_mix=_lst(self.si_sdr_mix), si_sdri=_lst(self.si_sdri), snr=_lst(self.snr),
                    valid=[bool(v) for v in self.valid], perm_best=[int(p) for p in self.perm_best],
                    si_sdr_best=_lst(self.si_sdr_best), n_samples=int(self.n_samples),
                    loss_miso1=None if self.loss_miso1 is None else float(self.loss_miso1),
                    loss_enhance=_lst(self.loss_enhance))


def from_stats(stats_est, n, stats_mix=None, loss_miso1=None, loss_enhance=None) -> Score:
    """stats_est float64 [S, S, 5] (estimates x references), stats_mix [1, S, 5] or [S, 5] or None, n valid samples"""
    st = np.asarray(stats_est, dtype=np.float64)
    if st.ndim != 3 or st.shape[0] != st.shape[1]:
        raise ValueError("stats_est must be [S, S, 5]")
    S = st.shape[0]
    M = si_sdr(st, n)
    own = np.array([M[j, j] for j in range(S)])
    _, crr, _ = _centred(st[0], n)
    p = best_perm(M)
    mix_v = sdri = None
    if stats_mix is not None:
        mix_v = si_sdr(np.asarray(stats_mix, dtype=np.float64).reshape(S, 5), n)
        sdri = own - mix_v
    return Score(si_sdr=own, si_sdr_mix=mix_v, si_sdri=sdri, snr=np.array([snr(st[j, j], n) for j in range(S)]),
                 valid=crr > 0, perm_best=p, si_sdr_best=np.array([M[p[j], j] for j in range(S)]), n_samples=int(n),
                 loss_miso1=loss_miso1, loss_enhance=None if loss_enhance is None else np.asarray(loss_enhance, np.float64))


def _mean_valid(items, keys) -> dict:
    """{key: the mean of item.key[j] over the items that have the figure and their valid speakers j where it is finite, or
    None}: what every ``*_mean_of`` starts from"""
    out = {}
    for key in keys:
        vals = [float(getattr(e, key)[j]) for e in items if getattr(e, key) is not None
                for j in range(len(e.valid)) if e.valid[j] and np.isfinite(getattr(e, key)[j])]
        out[key] = float(np.mean(vals)) if vals else None
    return out


def mean_of(scores: Sequence[Score]) -> dict:
    """The ``"mean"`` entry of scores.json: the dB figures averaged over the valid speakers of every recording, the
    criterion values over the recordings that have them."""
    out = _mean_valid(scores, ("si_sdr", "si_sdr_mix", "si_sdri", "snr", "si_sdr_best"))
    l1 = [float(s.loss_miso1) for s in scores if s.loss_miso1 is not None]
    le = [float(v) for s in scores if s.loss_enhance is not None for v in s.loss_enhance]
    out["loss_miso1"] = float(np.mean(l1)) if l1 else None
    out["loss_enhance"] = float(np.mean(le)) if le else None
    out["n_recordings"] = len(scores)
    out["n_speakers_valid"] = int(sum(int(np.sum(s.valid)) for s in scores))
    return out


# ---- device side ---------------------------------------------------------------------------------------------------------
def scratch_bytes(B: int, E: int, R: int, n_or_F: int) -> int:
    """bytes of scratch for :func:`wave_stats` (n samples) or :func:`spec_pairs` (F bins):
    8 B max(ceil(x / 4096) (2E + 2R + E R), min(x, 1024) E R)"""
    return int(_lib.lib().misonet_score_scratch_bytes(int(B), int(E), int(R), int(n_or_F)))


def _wave_view(x, name, dtypes):
    import torch
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or not x.is_cuda or x.dtype not in dtypes:
        raise ValueError(f"{name} must be a device tensor [B, sources, n] of {' or '.join(str(d) for d in dtypes)} "
                         "(any strides: a transposed view of a time-major array is read in place)")
    if any(s < 0 for s in x.stride()) or x.stride(2) < 1:
        raise ValueError(f"{name}: negative or zero strides are not supported")
    return x


def _check_counts(n_valid, B, dev, name="n_valid"):
    import torch
    if n_valid is not None and (not isinstance(n_valid, torch.Tensor) or n_valid.dtype != torch.int32 or n_valid.device != dev
                                or n_valid.numel() != B or not n_valid.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous int32 device tensor of {B} entries")


def _check_views(est, ref, mix, n_valid, what="est", most=4096):
    """What the device steps of BSS-eval, STOI, the reverb figures and SRMR ask of their input: ``est`` (named ``what``) int16 or
    float32 [B, E, n], ref float32 [B, R, n] or None (SRMR), mix float32 [B, 1, n] or None, all views on one device; 1 <= E, R
    <= 4, n <= 2^24, 1 <= B <= ``most`` (None: any); n_valid a contiguous int32 device tensor of B entries or None.
    Returns (B, E, R or None, n, device)."""
    import torch
    est = _wave_view(est, what, (torch.int16, torch.float32))
    B, E, n = est.shape
    dev, R = est.device, None
    if ref is not None:
        ref = _wave_view(ref, "ref", (torch.float32,))
        if ref.shape[0] != B or ref.shape[2] != n or ref.device != dev:
            raise ValueError("est and ref must agree in B, n and device")
        R = ref.shape[1]
        if not (1 <= E <= 4 and 1 <= R <= 4):
            raise ValueError(f"1 <= estimates, references <= 4 (got {E}, {R})")
    _signal_limits(E, n)
    if B < 1 or (most is not None and B > most):
        raise ValueError("at least one item" if most is None else f"1 <= B <= {most} items")
    if mix is not None:
        mix = _wave_view(mix, "mix", (torch.float32,))
        if tuple(mix.shape) != (B, 1, n) or mix.device != dev:
            raise ValueError(f"mix must be [B, 1, n] on the device of {what}")
    _check_counts(n_valid, B, dev)
    return B, E, R, n, dev


def _ptr(x):
    return x.data_ptr() if x is not None else None


def _view_args(est, ref=None):
    """the leading arguments of the C entry points: the estimates (pointer, int16 flag, three strides) and, unless None, the
    references (pointer, three strides)"""
    import torch
    a = (est.data_ptr(), int(est.dtype == torch.int16)) + tuple(est.stride())
    return a if ref is None else a + (ref.data_ptr(),) + tuple(ref.stride())


def _mix_args(mix):
    """the mixture [B, 1, n] or None as the C entry points take it: pointer, item stride, sample stride"""
    return (mix.data_ptr(), mix.stride(0), mix.stride(2)) if mix is not None else (None, 0, 1)


def _call(fn, dev, *args):
    """one C entry point, queued on the current stream of ``dev``"""
    import torch
    with torch.cuda.device(dev):
        _lib.check(fn(*args, _lib.stream_ptr(dev)))


def _scratch(nb, dev):
    import torch
    return torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)


def _limits(S, L, what="speakers"):
    if not (1 <= S <= 4):
        raise ValueError(f"1 <= S <= 4 {what} (got {S})")
    if not (1 <= L <= 1 << 24):
        raise ValueError(f"1 <= L <= 2^24 samples (got {L})")


def _signal_limits(S, L):
    _limits(S, L, "signals")


def _check_fs(fs, rates, what):
    if int(fs) != fs or int(fs) not in rates:
        raise ValueError(f"{what} defined here for fs = {', '.join(str(r) for r in rates[:-1])} or {rates[-1]} Hz (got {fs})")
    return int(fs)


def _groups(B, per_item, cap, most=None):
    """[(lo, hi)]: B items in runs whose scratch of ``per_item`` bytes each stays under ``cap``, of at most ``most`` items"""
    g = max(1, min(B, cap // max(1, per_item), most or B))
    return [(lo, min(B, lo + g)) for lo in range(0, B, g)]


def _block_rows(groups, est, ref, mix, n_valid, measure):
    """``measure(est, ref, mix, n_valid)`` -> tensors [b, ...] over every group of items; each item's flattened as float64 side
    by side, the groups one under the other: the device block [B, W] of ``stoi_block`` and ``reverb_block``"""
    import torch
    rows = []
    for lo, hi in groups:
        got = measure(est[lo:hi], ref[lo:hi], mix[lo:hi] if mix is not None else None,
                      n_valid[lo:hi] if n_valid is not None else None)
        rows.append(torch.cat([t.to(torch.float64).reshape(hi - lo, -1) for t in got], dim=1))
    return rows[0] if len(rows) == 1 else torch.cat(rows, dim=0)


def wave_stats(est, ref, n_valid=None):
    """est int16 or float32 [B, E, n], ref float32 [B, R, n] (device; strided views are read in place, e.g.
    ``clean_wav.transpose(1, 2)`` of a time-major [B, n, S]); n_valid int32 [B] (device) or None = n.  Returns float64
    [B, E, R, 5] = (S e_i, S r_j, S e_i^2, S r_j^2, S e_i r_j) over samples [0, n_valid).  Asynchronous on the current stream."""
    import torch
    est = _wave_view(est, "est", (torch.int16, torch.float32))
    ref = _wave_view(ref, "ref", (torch.float32,))
    B, E, n = est.shape
    if ref.shape[0] != B or ref.shape[2] != n or ref.device != est.device:
        raise ValueError("est and ref must agree in B, n and device")
    R = ref.shape[1]
    dev = est.device
    _check_counts(n_valid, B, dev)
    out = torch.empty((B, E, R, 5), dtype=torch.float64, device=dev)
    L = _lib.lib()
    scratch = _scratch(int(L.misonet_score_scratch_bytes(B, max(E, 1), max(R, 1), n)) if B > 0 and n > 0 else 0, dev)
    _call(L.misonet_score_wave, dev, *_view_args(est, ref), B, E, R, n, _ptr(n_valid), out.data_ptr(), scratch.data_ptr(),
          scratch.numel())
    return out


def spec_pairs(est, ref, return_value=False):
    """est complex64 [B, E, T, F], ref complex64 [B, R, T, F] (device; bins contiguous, any other strides).  Returns
    (pair float64 [B, E, R], perm int32 [B, R] or None): the spectral criterion of every pair and, where E == R, the uPIT
    pick (estimate i goes with reference perm[i]).  ``return_value``: a third entry, float64 [B] = the value of the pick
    (sum_i pair[i][perm[i]]; None where E != R).  Asynchronous on the current stream."""
    import torch
    for x, name in ((est, "est"), (ref, "ref")):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.complex64 or not x.is_cuda:
            raise ValueError(f"{name} must be a complex64 device tensor [B, sources, T, F]")
        if x.stride(3) != 1 or any(s < 0 for s in x.stride()) or x.stride(2) < 1:
            raise ValueError(f"{name}: the bins must be contiguous and no stride negative")
    B, E, T, F = est.shape
    if ref.shape[0] != B or tuple(ref.shape[2:]) != (T, F) or ref.device != est.device:
        raise ValueError("est and ref must agree in B, T, F and device")
    R = ref.shape[1]
    dev = est.device
    pick = E == R
    pair = torch.empty((B, E, R), dtype=torch.float64, device=dev)
    perm = torch.empty((B, R), dtype=torch.int32, device=dev) if pick else None
    val = torch.empty((B,), dtype=torch.float64, device=dev) if pick else None
    L = _lib.lib()
    scratch = _scratch(int(L.misonet_score_scratch_bytes(B, max(E, 1), max(R, 1), F)) if B > 0 and F > 0 else 0, dev)
    _call(L.misonet_score_spec, dev, est.data_ptr(), *est.stride()[:3], ref.data_ptr(), *ref.stride()[:3], B, E, R, T, F,
          pair.data_ptr(), _ptr(perm), _ptr(val), scratch.data_ptr(), scratch.numel())
    return (pair, perm, val) if return_value else (pair, perm)


def score_waves(est, clean, mix=None, fs: int = 16000, device=None) -> Score:
    """est int16 or float32 [S, L], clean float32 [S, L], mix float32 [L] or None (ndarrays or tensors, host or device) ->
    :class:`Score`.  Any L: the sums are taken on the device in pieces of 2^20 samples and added on the host in float64.
    The entry point for the output of ``enhance_continuous`` and for files read back from disk (``fs`` is carried for
    callers that report durations; the scores do not depend on it)."""
    import torch
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    est = torch.as_tensor(est)
    clean = torch.as_tensor(clean)
    if est.dim() != 2 or clean.dim() != 2 or est.shape != clean.shape:
        raise ValueError("est and clean must both be [S, L]")
    if est.dtype != torch.int16:
        est = est.to(torch.float32)
    clean = clean.to(torch.float32)
    S, Ltot = est.shape
    if S < 1 or S > 4 or Ltot < 1:
        raise ValueError("1 <= S <= 4 speakers and at least one sample")
    if mix is not None:
        mix = torch.as_tensor(mix).to(torch.float32).reshape(-1)
        if mix.numel() != Ltot:
            raise ValueError("mix must hold L samples")
    blocks_e, blocks_m, ns = [], [], []
    with torch.cuda.device(dev):
        for lo in range(0, Ltot, PIECE):
            hi = min(Ltot, lo + PIECE)
            e = est[:, lo:hi].to(dev).contiguous()[None]
            r = clean[:, lo:hi].to(dev).contiguous()[None]
            blocks_e.append(wave_stats(e, r)[0].cpu().numpy())
            if mix is not None:
                m = mix[lo:hi].to(dev).contiguous()[None, None]
                blocks_m.append(wave_stats(m, r)[0].cpu().numpy())
            ns.append(hi - lo)
    st, n = combine(blocks_e, ns)
    sm = combine(blocks_m, ns)[0] if mix is not None else None
    return from_stats(st, n, sm)


# ---- BSS-eval SDR / SIR / SAR ------------------------------------------------------------------------
# float64 throughout, every signal zero outside [0, n); references r_j, estimates e_i, filter length Q:
#   Rrr[j][k][a] = S_t r_j[t] r_k[t + a], Rre[j][i][a] = S_t r_j[t] e_i[t + a], a in [0, Q), Eee[i] = S_t e_i[t]^2;
#   G [R Q, R Q]: G[(j,a),(k,b)] = S_t r_j[t - a] r_k[t - b]; D_i = the Rre[.][i][.] stacked;
#   A_i = D_i^T G^-1 D_i (projection on all references), T_ij = d_ij^T G_jj^-1 d_ij (on reference j alone);
#   SDR_ij = 10 log10(T_ij / max(Eee_i - T_ij, 0)), SIR_ij = 10 log10(T_ij / max(A_i - T_ij, 0)),
#   SAR_i = 10 log10(A_i / max(Eee_i - A_i, 0)): mir_eval's figures, the projections being orthogonal.
BSS_SCRATCH_CAP = 1 << 30    # bytes of device scratch per call of bss_solve / bss_corr: larger batches go in groups


@dataclasses.dataclass
class BssEval:
    """BSS-eval figures of one recording, speaker j = reference j, dB.  ``ok = False``: the factorisation met a pivot
    <= 2^-40 of its diagonal entry (linearly dependent references) and every figure is NaN."""
    sdr: np.ndarray                       # [S] SDR(e_j, r_j)
    sir: np.ndarray                       # [S] SIR(e_j, r_j)
    sar: np.ndarray                       # [S] SAR(e_j)
    valid: np.ndarray                     # [S] bool: reference j is not silent (a silent one leaves the span; NaN SDR / SIR)
    ok: bool
    perm_best: List[int]                  # p[j] = the estimate of reference j in the assignment with the largest mean SIR
    sdr_best: np.ndarray                  # [S] SDR(e_p[j], r_j)
    sir_best: np.ndarray                  # [S] SIR(e_p[j], r_j)
    sar_best: np.ndarray                  # [S] SAR(e_p[j])
    sdr_mix: Optional[np.ndarray]         # [S] SDR(mixture, r_j), or None without a mixture
    sdri: Optional[np.ndarray]            # [S] sdr - sdr_mix
    filt_len: int
    n_samples: int

    def as_dict(self) -> dict:
        return dict(sdr=_lst(self.sdr), sir=_lst(self.sir), sar=_lst(self.sar), valid=[bool(v) for v in self.valid],
                    ok=bool(self.ok), perm_best=[int(p) for p in self.perm_best], sdr_best=_lst(self.sdr_best),
                    sir_best=_lst(self.sir_best), sar_best=_lst(self.sar_best), sdr_mix=_lst(self.sdr_mix), sdri=_lst(self.sdri),
                    filt_len=int(self.filt_len), n_samples=int(self.n_samples))


def _db_ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(num / np.maximum(den, 0.0))


def bss_from_energies(T, A, Eee, valid=None, ok: bool = True, T_mix=None, Eee_mix=None, filt_len: int = 512,
                      n_samples: int = 0) -> BssEval:
    """T float64 [S estimates, S references], A [S], Eee [S] (:func:`bss_solve` / :func:`bss_corr` of one recording) ->
    :class:`BssEval`.  ``valid`` bool [S] (None: all): reference j is not silent; ``ok``: the factorisation succeeded;
    ``T_mix`` [S] and ``Eee_mix`` (scalar): the energies of the mixture scored as a single estimate.  Host, float64, no GPU."""
    T = np.asarray(T, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != T.shape[1]:
        raise ValueError("T must be [S, S] (estimates x references)")
    S = T.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1)
    Eee = np.asarray(Eee, dtype=np.float64).reshape(-1)
    if A.shape != (S,) or Eee.shape != (S,):
        raise ValueError("A and Eee must hold one entry per estimate")
    valid = np.ones(S, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).reshape(-1)
    if valid.shape != (S,):
        raise ValueError("valid must hold one entry per reference")
    if (T_mix is None) != (Eee_mix is None):
        raise ValueError("T_mix and Eee_mix go together")
    sdr_m = np.where(valid[None, :], _db_ratio(T, Eee[:, None] - T), np.nan)
    sir_m = np.where(valid[None, :], _db_ratio(T, A[:, None] - T), np.nan)
    sar_v = _db_ratio(A, Eee - A)
    mix_v = None
    if T_mix is not None:
        tm = np.asarray(T_mix, dtype=np.float64).reshape(-1)
        if tm.shape != (S,):
            raise ValueError("T_mix must hold one entry per reference")
        mix_v = np.where(valid, _db_ratio(tm, float(Eee_mix) - tm), np.nan)
    if not ok:
        sdr_m, sir_m, sar_v = np.full((S, S), np.nan), np.full((S, S), np.nan), np.full(S, np.nan)
        mix_v = None if mix_v is None else np.full(S, np.nan)
    p = best_perm(sir_m)
    idx = np.arange(S)
    sdr = sdr_m[idx, idx]
    return BssEval(sdr=sdr, sir=sir_m[idx, idx], sar=sar_v.copy(), valid=valid, ok=bool(ok), perm_best=p,
                   sdr_best=np.array([sdr_m[p[j], j] for j in range(S)]), sir_best=np.array([sir_m[p[j], j] for j in range(S)]),
                   sar_best=np.array([sar_v[p[j]] for j in range(S)]), sdr_mix=mix_v,
                   sdri=None if mix_v is None else sdr - mix_v, filt_len=int(filt_len), n_samples=int(n_samples))


def bss_mean_of(evals: Sequence[BssEval]) -> dict:
    """The ``"bss"`` part of the ``"mean"`` entry of scores.json: every figure averaged over the valid speakers of the
    recordings whose factorisation succeeded."""
    out = _mean_valid([e for e in evals if e.ok], ("sdr", "sir", "sar", "sdr_best", "sir_best", "sar_best", "sdr_mix", "sdri"))
    out["n_recordings"] = len(evals)
    out["n_failed"] = int(sum(1 for e in evals if not e.ok))
    return out


def bss_scratch_bytes(B: int, E: int, R: int, n: int, filt_len: int = 512) -> int:
    """bytes of scratch for :func:`bss_corr` (n samples) and :func:`bss_solve` (n = 1):
    8 B max(ceil((n + 15) / 4096) (R R + R E + E) Q, (R Q + 4) R Q + R (Q + 4) Q); negative outside the limits"""
    return int(_lib.lib().misonet_bss_scratch_bytes(int(B), int(E), int(R), int(n), int(filt_len)))


def _check_filt_len(filt_len):
    Q = int(filt_len)
    if not (16 <= Q <= 1024) or Q % 16:
        raise ValueError(f"filt_len must be a multiple of 16 in [16, 1024] (got {Q})")
    return Q


def bss_corr(est, ref, n_valid=None, filt_len: int = 512):
    """est int16 or float32 [B, E, n], ref float32 [B, R, n] (device views as :func:`wave_stats` takes them), n_valid int32
    [B] (device) or None.  Returns float64 (Rrr [B, R, R, Q], Rre [B, R, E, Q], Eee [B, E]).  Asynchronous on the current
    stream; an item's block does not depend on the batch."""
    import torch
    B, E, R, n, dev = _check_views(est, ref, None, n_valid, most=None)
    Q = _check_filt_len(filt_len)
    Rrr = torch.empty((B, R, R, Q), dtype=torch.float64, device=dev)
    Rre = torch.empty((B, R, E, Q), dtype=torch.float64, device=dev)
    Eee = torch.empty((B, E), dtype=torch.float64, device=dev)
    L = _lib.lib()
    groups = _groups(B, int(L.misonet_bss_scratch_bytes(1, E, R, n, Q)), BSS_SCRATCH_CAP, 4096)
    scratch = _scratch(int(L.misonet_bss_scratch_bytes(groups[0][1] - groups[0][0], E, R, n, Q)), dev)
    for lo, hi in groups:
        _call(L.misonet_bss_corr, dev, *_view_args(est[lo:hi], ref[lo:hi]), hi - lo, E, R, n,
              _ptr(n_valid[lo:hi] if n_valid is not None else None), Q, Rrr[lo:hi].data_ptr(), Rre[lo:hi].data_ptr(),
              Eee[lo:hi].data_ptr(), scratch.data_ptr(), scratch.numel())
    return Rrr, Rre, Eee


def bss_solve(Rrr, Rre, Eee):
    """Rrr float64 [B, R, R, Q], Rre [B, R, E, Q], Eee [B, E] (device, contiguous) -> (T float64 [B, E, R], A [B, E], info
    int32 [B]): the energies of the projections of estimate i on reference j alone and on all references, by a blocked
    Cholesky factorisation per item; info = -1, or the first row of G whose pivot failed (then T and A of the item are NaN).
    Asynchronous on the current stream; batches whose systems exceed 1 GiB of scratch run in groups."""
    import torch
    for x, name, nd in ((Rrr, "Rrr", 4), (Rre, "Rre", 4), (Eee, "Eee", 2)):
        if not isinstance(x, torch.Tensor) or x.dim() != nd or x.dtype != torch.float64 or not x.is_cuda \
                or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float64 device tensor of {nd} dimensions")
    B, R, R2, Q = Rrr.shape
    E = Rre.shape[2]
    if R2 != R or tuple(Rre.shape) != (B, R, E, Q) or tuple(Eee.shape) != (B, E) or Rre.device != Rrr.device \
            or Eee.device != Rrr.device:
        raise ValueError("Rrr [B, R, R, Q], Rre [B, R, E, Q] and Eee [B, E] must agree")
    if not (1 <= E <= 4 and 1 <= R <= 4):
        raise ValueError(f"1 <= estimates, references <= 4 (got {E}, {R})")
    _check_filt_len(Q)
    if B < 1:
        raise ValueError("at least one item")
    dev = Rrr.device
    T = torch.empty((B, E, R), dtype=torch.float64, device=dev)
    A = torch.empty((B, E), dtype=torch.float64, device=dev)
    info = torch.empty((B,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    groups = _groups(B, int(L.misonet_bss_scratch_bytes(1, E, R, 1, Q)), BSS_SCRATCH_CAP, 4096)
    scratch = _scratch(int(L.misonet_bss_scratch_bytes(groups[0][1] - groups[0][0], E, R, 1, Q)), dev)
    for lo, hi in groups:
        _call(L.misonet_bss_solve, dev, Rrr[lo:hi].data_ptr(), Rre[lo:hi].data_ptr(), Eee[lo:hi].data_ptr(), hi - lo, E, R, Q,
              T[lo:hi].data_ptr(), A[lo:hi].data_ptr(), info[lo:hi].data_ptr(), scratch.data_ptr(), scratch.numel())
    return T, A, info


def bss_energies(est, ref, mix=None, n_valid=None, filt_len: int = 512):
    """est int16 / float32 [B, S, n], ref float32 [B, S, n], mix float32 [B, 1, n] or None (device views), n_valid int32 [B] or
    None -> a device float64 block [B, W]: per item T [S, S], A [S], Eee [S], Rrr[j][j][0] [S] (0: reference j is silent),
    info and, with a mixture, T_mix [S] and Eee_mix (the mixture scored as a one-estimate call): what :func:`bss_unpack`
    reads.  Everything is queued on the current stream; nothing synchronises."""
    import torch
    Rrr, Rre, Eee = bss_corr(est, ref, n_valid, filt_len)
    T, A, info = bss_solve(Rrr, Rre, Eee)
    B = est.shape[0]
    if est.shape[1] != ref.shape[1]:
        raise ValueError("as many estimates as references")
    idx = torch.arange(ref.shape[1], device=est.device)
    cols = [T.reshape(B, -1), A, Eee, Rrr[:, idx, idx, 0], info.to(torch.float64)[:, None]]
    if mix is not None:
        _, Rrm, Emm = bss_corr(mix, ref, n_valid, filt_len)
        Tm, _, _ = bss_solve(Rrr, Rrm, Emm)
        cols += [Tm.reshape(B, -1), Emm]
    return torch.cat(cols, dim=1)


def bss_unpack(row, S: int, filt_len: int, n_samples: int) -> BssEval:
    """one host row of :func:`bss_energies` -> :class:`BssEval`"""
    row = np.asarray(row, dtype=np.float64)
    o = S * S
    T, A, Eee, rr0, info = row[:o].reshape(S, S), row[o:o + S], row[o + S:o + 2 * S], row[o + 2 * S:o + 3 * S], row[o + 3 * S]
    o += 3 * S + 1
    tm = em = None
    if row.shape[0] > o:
        tm, em = row[o:o + S], row[o + S]
    return bss_from_energies(T, A, Eee, valid=rr0 != 0, ok=not info >= 0, T_mix=tm, Eee_mix=em, filt_len=filt_len,
                             n_samples=n_samples)


def _wave_batch(items, dev, pinned, limits):
    """items: a list of (est int16 or float32 [S, L], clean float32 [S, L] -- or None in every item: SRMR's signals have no clean
    sources --, mix float32 [L] or None) -> the device tensors (est [G, S, n], clean [G, S, n] or None, mix [G, 1, n] or None,
    n_valid int32 [G] or None for a single recording), zero-padded to the longest; ``limits(S, L)`` raises for what the caller
    does not take.  Must run under ``torch.cuda.device(dev)``."""
    import torch
    recs = []
    for est, clean, mix in items:
        est = torch.as_tensor(est)
        if clean is not None:
            clean = torch.as_tensor(clean)
            if est.dim() != 2 or clean.dim() != 2 or est.shape != clean.shape:
                raise ValueError("est and clean must both be [S, L]")
            clean = clean.to(torch.float32)
        elif est.dim() != 2:
            raise ValueError("signals must be [S, L]")
        if est.dtype != torch.int16:
            est = est.to(torch.float32)
        if mix is not None:
            mix = torch.as_tensor(mix).to(torch.float32).reshape(1, -1)
            if mix.numel() != est.shape[1]:
                raise ValueError("mix must hold L samples")
        recs.append((est, clean, mix))
    if not recs:
        raise ValueError("at least one recording")
    S = recs[0][0].shape[0]
    if any(r[0].shape[0] != S or (r[1] is None) != (recs[0][1] is None) or (r[2] is None) != (recs[0][2] is None) for r in recs):
        raise ValueError("every recording must have the same number of speakers, and all or none a mixture")
    for r in recs:
        limits(S, r[0].shape[1])
    if any(r[0].dtype != recs[0][0].dtype for r in recs):
        raise ValueError("int16 and float32 estimates cannot share a batch")
    cols, nv = _pad_batch(recs, dev, pinned)
    return cols[0], cols[1], cols[2], nv


def _pad_batch(recs, dev, pinned):
    """recs: per recording a tuple of 2-D tensors [rows_k, L] (or None, alike in every recording) -> (per entry the device
    tensor [G, rows_k, n], zero-padded to the longest recording, or None; n_valid int32 [G], or None for a single recording,
    which goes up as it is)"""
    import torch

    def up(x):
        if x.device.type == "cpu" and pinned:
            return x.contiguous().pin_memory().to(dev, non_blocking=True)
        return x.to(dev).contiguous()

    G = len(recs)
    if G == 1:
        return [up(x)[None] if x is not None else None for x in recs[0]], None
    lens = [int(r[0].shape[1]) for r in recs]
    n = max(lens)
    nv = torch.tensor(lens, dtype=torch.int32)
    nv = (nv.pin_memory() if pinned else nv).to(dev, non_blocking=pinned)
    cols = []
    for k, first in enumerate(recs[0]):
        if first is None:
            cols.append(None)
            continue
        buf = torch.zeros((G, first.shape[0], n), dtype=first.dtype, pin_memory=pinned)
        for g, r in enumerate(recs):
            buf[g, :, :lens[g]].copy_(r[k])
        cols.append(buf.to(dev, non_blocking=pinned))
    return cols, nv


def _side_blocks(items, dev, pinned, params):
    """:func:`side_queue` by name: ``params`` = {name of a figure of SIDE_FIGURES: its parameter (the filter length of "bss",
    the rate of the others), or None} -> {name: device block} of the figures asked for, all from one batch"""
    import torch
    figs = [(f, f.check(params[f.name])) for f in SIDE_FIGURES if params.get(f.name) is not None]

    def limits(S, L):
        for f, _ in figs:
            f.limits(S, L)

    with torch.cuda.device(dev):
        est, clean, mix, nv = _wave_batch(items, dev, pinned, limits)
        return {f.name: f.block(est, clean, mix, nv, par) if f.needs_clean else f.block(est, mix, nv, par) for f, par in figs}


def side_queue(items, dev, pinned: bool = False, bss_filt_len: Optional[int] = None, stoi_fs: Optional[int] = None,
               reverb_fs: Optional[int] = None, srmr_fs: Optional[int] = None):
    """items: a list of (est int16 or float32 [S, L], clean float32 [S, L], mix float32 [L] or None) (ndarrays or tensors; the
    same S and all or none with a mixture; any lengths) -> (the device block [len(items), W] of :func:`bss_energies` for
    filters of ``bss_filt_len`` taps, that of :func:`stoi_block` at rate ``stoi_fs``), either None where its argument is
    None, queued on the current stream of ``dev``.  Several recordings go as one batch, zero-padded to the longest with
    ``n_valid`` set, and the batch is built and copied once for both: a row is bit for bit what the recording gives
    alone.  ``pinned``: host inputs go through pinned memory and asynchronous copies, so that the caller is not held up.
    ``reverb_fs`` (not None): a third entry, the block of :func:`reverb_block` at that rate, from the same batch; without it
    the pair is returned as it always was.  ``srmr_fs`` (not None): four entries, (bss, stoi, reverb or None, the block of
    :func:`srmr_block` of the estimates and the mixture at that rate), again from the same batch."""
    got = _side_blocks(items, dev, pinned, dict(bss=bss_filt_len, stoi=stoi_fs, reverb=reverb_fs, srmr=srmr_fs))
    return tuple(got.get(f.name) for f in SIDE_FIGURES)[:4 if srmr_fs is not None else 3 if reverb_fs is not None else 2]


def _one_recording(est, limits, device, queue, unpack):
    """What every ``*_waves`` does with its first argument [S, L] once the rate is checked: ``limits(S, L)`` before a device is
    touched, the device, ``queue(est, device)`` -> a block of one row, ``unpack(row, S, L)``"""
    import torch
    est = torch.as_tensor(est)
    if est.dim() == 2:
        limits(int(est.shape[0]), int(est.shape[1]))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    row = queue(est, dev)[0].cpu().numpy()
    return unpack(row, int(est.shape[0]), int(est.shape[1]))


def bss_queue(items, filt_len: int, dev, pinned: bool = False):
    """:func:`side_queue` for BSS-eval alone: the device block [len(items), W] of :func:`bss_energies`"""
    return side_queue(items, dev, pinned, bss_filt_len=filt_len)[0]


def bss_eval_waves(est, clean, mix=None, filt_len: int = 512, device=None) -> BssEval:
    """est int16 or float32 [S, L], clean float32 [S, L], mix float32 [L] or None (ndarrays or tensors, host or device) ->
    :class:`BssEval` (1 <= S <= 4, L <= 2^24): the counterpart of :func:`score_waves` for BSS-eval SDR, SIR and SAR, for the
    output of ``enhance_continuous`` and for files read back from disk."""
    return _one_recording(est, _limits, device, lambda e, dev: bss_queue([(e, clean, mix)], filt_len, dev),
                          lambda row, S, L: bss_unpack(row, S, int(filt_len), L))


# ---- STOI and ESTOI ----------------------------------------------------------------------------------
# x the clean reference, y the estimate, float64 throughout: both to 10 kHz (polyphase, Kaiser window), the frames of 256 whose
# energy is more than 40 dB under the loudest frame of x dropped from both, the kept frames overlap-added and framed again,
# 512-point transform, 15 third-octave bands, segments of 30 frames; STOI = the mean clipped band-wise correlation, ESTOI =
# the mean correlation of the row- and column-normalised segments.
STOI_RATES = (8000, 10000, 16000)
STOI_SEG = 30                 # frames per segment: fewer kept frames give 1e-5 and ``valid = False``
STOI_SCRATCH_CAP = 1 << 30    # bytes of device memory per group of stoi_block: larger batches go in groups


@dataclasses.dataclass
class Stoi:
    """STOI and ESTOI of one recording, speaker j = reference j.  ``valid[j] = False``: reference j is silent (NaN) or keeps
    fewer than 30 frames (1e-5, as pystoi answers)."""
    stoi: np.ndarray                      # [S] STOI(e_j, r_j)
    estoi: np.ndarray                     # [S] ESTOI(e_j, r_j)
    valid: np.ndarray                     # [S] bool
    perm_best: List[int]                  # p[j] = the estimate of reference j in the assignment with the largest summed STOI
    stoi_best: np.ndarray                 # [S] STOI(e_p[j], r_j)
    estoi_best: np.ndarray                # [S] ESTOI(e_p[j], r_j)
    stoi_mix: Optional[np.ndarray]        # [S] STOI(mixture, r_j), or None without a mixture
    estoi_mix: Optional[np.ndarray]       # [S]
    stoi_i: Optional[np.ndarray]          # [S] stoi - stoi_mix
    estoi_i: Optional[np.ndarray]         # [S] estoi - estoi_mix
    frames: np.ndarray                    # [S] int: frames of reference j at 10 kHz
    frames_kept: np.ndarray               # [S] int: those within 40 dB of its loudest frame
    fs: int
    n_samples: int

    def as_dict(self) -> dict:
        return dict(stoi=_lst(self.stoi), estoi=_lst(self.estoi), valid=[bool(v) for v in self.valid],
                    perm_best=[int(p) for p in self.perm_best], stoi_best=_lst(self.stoi_best), estoi_best=_lst(self.estoi_best),
                    stoi_mix=_lst(self.stoi_mix), estoi_mix=_lst(self.estoi_mix), stoi_i=_lst(self.stoi_i),
                    estoi_i=_lst(self.estoi_i), frames=[int(v) for v in self.frames],
                    frames_kept=[int(v) for v in self.frames_kept], fs=int(self.fs), n_samples=int(self.n_samples))


def stoi_from_matrices(stoi_m, estoi_m, frames, frames_kept, nonsilent, stoi_mix=None, estoi_mix=None, fs: int = 16000,
                       n_samples: int = 0) -> Stoi:
    """stoi_m / estoi_m float64 [S estimates, S references] as the device leaves them, frames / frames_kept int [S], nonsilent
    bool [S] (reference j has a sample that is not zero), stoi_mix / estoi_mix [S] or None -> :class:`Stoi`.  The rules of the
    edges are applied here: a silent reference gives NaN, fewer than 30 kept frames 1e-5, neither is valid.  The definition
    calls a reference silent when sum x^2 == 0 over the input; ``nonsilent`` as the device reports it says that a sample of
    the reference at 10 kHz differs from zero.  The two agree unless a non-zero input resamples to exact zeros everywhere,
    which the filter's non-zero taps rule out for float32 input short of cancellation to the last bit.  Host, no GPU."""
    sm, em = np.array(stoi_m, dtype=np.float64), np.array(estoi_m, dtype=np.float64)
    if sm.ndim != 2 or sm.shape[0] != sm.shape[1] or em.shape != sm.shape:
        raise ValueError("stoi_m and estoi_m must both be [S, S] (estimates x references)")
    S = sm.shape[0]
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    kept = np.asarray(frames_kept, dtype=np.int64).reshape(-1)
    ns = np.asarray(nonsilent, dtype=bool).reshape(-1)
    if frames.shape != (S,) or kept.shape != (S,) or ns.shape != (S,):
        raise ValueError("frames, frames_kept and nonsilent must hold one entry per reference")
    if (stoi_mix is None) != (estoi_mix is None):
        raise ValueError("stoi_mix and estoi_mix go together")
    short = kept < STOI_SEG
    sm = np.where(ns[None, :], np.where(short[None, :], 1e-5, sm), np.nan)
    em = np.where(ns[None, :], np.where(short[None, :], 1e-5, em), np.nan)
    mix_s = mix_e = None
    if stoi_mix is not None:
        mix_s, mix_e = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (stoi_mix, estoi_mix))
        if mix_s.shape != (S,) or mix_e.shape != (S,):
            raise ValueError("stoi_mix and estoi_mix must hold one entry per reference")
        mix_s = np.where(ns, np.where(short, 1e-5, mix_s), np.nan)
        mix_e = np.where(ns, np.where(short, 1e-5, mix_e), np.nan)
    p = best_perm(sm)
    idx = np.arange(S)
    own_s, own_e = sm[idx, idx], em[idx, idx]
    return Stoi(stoi=own_s, estoi=own_e, valid=ns & ~short, perm_best=p, stoi_best=np.array([sm[p[j], j] for j in range(S)]),
                estoi_best=np.array([em[p[j], j] for j in range(S)]), stoi_mix=mix_s, estoi_mix=mix_e,
                stoi_i=None if mix_s is None else own_s - mix_s, estoi_i=None if mix_e is None else own_e - mix_e,
                frames=frames, frames_kept=kept, fs=int(fs), n_samples=int(n_samples))


def stoi_mean_of(items: Sequence[Stoi]) -> dict:
    """The ``"stoi"`` part of the ``"mean"`` entry of scores.json: every figure averaged over the valid speakers"""
    out = _mean_valid(items, ("stoi", "estoi", "stoi_best", "estoi_best", "stoi_mix", "estoi_mix", "stoi_i", "estoi_i"))
    out["n_recordings"] = len(items)
    out["n_speakers_valid"] = int(sum(int(np.sum(e.valid)) for e in items))
    return out


def check_stoi_fs(fs):
    return _check_fs(fs, STOI_RATES, "STOI is")


def stoi_resampled_len(n: int, fs: int) -> int:
    """ceil(n p / q), p / q = 10000 / fs: the length at 10 kHz; negative outside the limits (n <= 2^24, the three rates)"""
    return int(_lib.lib().misonet_stoi_resampled_len(int(n), int(fs)))


def stoi_taps(fs: int) -> np.ndarray:
    """the polyphase taps g[k] = p h[k - Lh] / sum h of rate fs as the library builds them (host, no GPU): 581 for 16 kHz,
    365 for 8 kHz, the single 1.0 for 10 kHz"""
    import ctypes as C
    L = _lib.lib()
    n = int(L.misonet_stoi_taps(check_stoi_fs(fs), None))
    buf = (C.c_double * n)()
    L.misonet_stoi_taps(int(fs), buf)
    return np.array(buf, dtype=np.float64)


def stoi_scratch_bytes(B: int, NS: int, R: int, n10: int) -> int:
    """bytes of scratch for :func:`stoi_measure` over NS signals per item (R references first) of n10 samples at 10 kHz:
    8 B (R f + 15 R (NS - R + 1) f + 2 R (NS - R) max(f - 29, 1) + R ceil(f / 2)), f = max(frames, 1); negative outside the
    limits"""
    return int(_lib.lib().misonet_stoi_scratch_bytes(int(B), int(NS), int(R), int(n10)))


def stoi_resample(est, ref, mix=None, n_valid=None, fs: int = 16000):
    """est int16 or float32 [B, E, n], ref float32 [B, R, n] (device views as :func:`wave_stats` takes them), mix float32
    [B, 1, n] or None, n_valid int32 [B] (device) or None.  Returns (x10 float64 [B, R + E (+ 1), n10]: the references, the
    estimates and the mixture at 10 kHz, zero past an item's own length; len10 int32 [B] = ceil(n_valid p / q)).
    Asynchronous on the current stream; an item's rows do not depend on the batch."""
    import torch
    fs = check_stoi_fs(fs)
    B, E, R, n, dev = _check_views(est, ref, mix, n_valid)
    L = _lib.lib()
    n10 = int(L.misonet_stoi_resampled_len(n, fs))
    x10 = torch.empty((B, R + E + (1 if mix is not None else 0), n10), dtype=torch.float64, device=dev)
    len10 = torch.empty((B,), dtype=torch.int32, device=dev)
    _call(L.misonet_stoi_resample, dev, *_view_args(est, ref), *_mix_args(mix), B, E, R, n, _ptr(n_valid), fs, x10.data_ptr(),
          len10.data_ptr())
    return x10, len10


def stoi_measure(x10, len10, R: int):
    """x10 float64 [B, NS, n10] (device, contiguous; the first R signals of an item are its references, the others are
    measured against each of them), len10 int32 [B] (device) or None -> (out float64 [B, NS - R, R, 2] = (STOI, ESTOI) of
    estimate i against reference j, 1e-5 where fewer than 30 frames are kept; frames int32 [B, R, 3] = (frames, kept frames,
    1 if the reference has a sample that is not zero)).  Asynchronous on the current stream: the number of kept frames
    stays on the device."""
    import torch
    if not isinstance(x10, torch.Tensor) or x10.dim() != 3 or x10.dtype != torch.float64 or not x10.is_cuda \
            or not x10.is_contiguous():
        raise ValueError("x10 must be a contiguous float64 device tensor [B, signals, n10]")
    B, NS, n10 = x10.shape
    R = int(R)
    dev = x10.device
    _check_counts(len10, B, dev, "len10")
    L = _lib.lib()
    nb = int(L.misonet_stoi_scratch_bytes(B, NS, R, n10))
    if nb < 0:
        raise ValueError(f"1 <= B <= 4096, 1 <= R <= 4, 1 <= NS - R <= 5, 1 <= n10 <= 5 * 2^22 (got {B}, {R}, {NS - R}, {n10})")
    out = torch.empty((B, NS - R, R, 2), dtype=torch.float64, device=dev)
    frames = torch.empty((B, R, 3), dtype=torch.int32, device=dev)
    scratch = _scratch(nb, dev)
    _call(L.misonet_stoi_measure, dev, x10.data_ptr(), _ptr(len10), B, NS, R, n10, out.data_ptr(), frames.data_ptr(),
          scratch.data_ptr(), scratch.numel())
    return out, frames


def stoi_block(est, ref, mix=None, n_valid=None, fs: int = 16000):
    """est int16 / float32 [B, S, n], ref float32 [B, S, n], mix float32 [B, 1, n] or None (device views), n_valid int32 [B] or
    None -> a device float64 block [B, W]: per item the (STOI, ESTOI) of every (estimate, reference) pair ([S (+ 1), S, 2], the
    mixture as the last estimate) and (frames, kept, not silent) per reference: what :func:`stoi_unpack` reads.  Everything
    is queued on the current stream; nothing synchronises.  Batches beyond 1 GiB of device memory run in groups."""
    B, E, n = est.shape
    R = ref.shape[1]
    NS = R + E + (1 if mix is not None else 0)
    n10 = stoi_resampled_len(n, check_stoi_fs(fs))
    per = 8 * NS * max(n10, 1) + max(stoi_scratch_bytes(1, NS, R, max(n10, 1)), 0)
    return _block_rows(_groups(B, per, STOI_SCRATCH_CAP), est, ref, mix, n_valid,
                       lambda e, r, m, nv: stoi_measure(*stoi_resample(e, r, m, nv, fs), R))


def stoi_unpack(row, S: int, fs: int, n_samples: int) -> Stoi:
    """one host row of :func:`stoi_block` -> :class:`Stoi`"""
    row = np.asarray(row, dtype=np.float64)
    E = (row.shape[0] - 3 * S) // (2 * S)
    if E not in (S, S + 1) or row.shape[0] != 2 * S * E + 3 * S:
        raise ValueError("not a row of stoi_block for this number of speakers")
    fig = row[:2 * S * E].reshape(E, S, 2)
    meta = row[2 * S * E:].reshape(S, 3)
    mix = fig[S] if E > S else None
    return stoi_from_matrices(fig[:S, :, 0], fig[:S, :, 1], meta[:, 0], meta[:, 1], meta[:, 2] != 0,
                              None if mix is None else mix[:, 0], None if mix is None else mix[:, 1], fs=fs,
                              n_samples=n_samples)


def stoi_queue(items, fs: int, dev, pinned: bool = False):
    """:func:`side_queue` for STOI / ESTOI alone: the device block [len(items), W] of :func:`stoi_block`"""
    return side_queue(items, dev, pinned, stoi_fs=fs)[1]


def stoi_waves(est, clean, mix=None, fs: int = 16000, device=None) -> Stoi:
    """est int16 or float32 [S, L], clean float32 [S, L], mix float32 [L] or None (ndarrays or tensors, host or device) ->
    :class:`Stoi` (1 <= S <= 4, L <= 2^24, fs 8000, 10000 or 16000): the counterpart of :func:`score_waves` for STOI and
    ESTOI, for the output of ``enhance_continuous`` and for files read back from disk."""
    fs = check_stoi_fs(fs)
    return _one_recording(est, _limits, device, lambda e, dev: stoi_queue([(e, clean, mix)], fs, dev),
                          lambda row, S, L: stoi_unpack(row, S, fs, L))


# ---- cepstral distance, LLR and fwSegSNR -------------------------------------------------------------
# x the clean reference, y the estimate, float64 throughout: frames of 25 ms every 10 ms under MATLAB's hanning, per frame the
# real cepstrum (25 coefficients), 23 mel band sums, the autocorrelation and the LPC of order 12; CD = the mean-normalised
# cepstral distance in dB (cap 10), LLR = ln(a_y' R_x a_y / a_x' R_x a_x) in [0, 2], fwSegSNR = the band-weighted segmental SNR
# in [-10, 35] dB of the signals at unit power; mean and median over the frames whose reference is not digital silence.  The
# parameters are the REVERB challenge's as published; the figures have not been compared against its MATLAB tools.
REVERB_RATES = (8000, 16000)
REVERB_SCRATCH_CAP = 1 << 30    # bytes of device scratch per group of reverb_block: larger batches go in groups
REVERB_FIGURES = ("cd", "cd_median", "llr", "llr_median", "fwsegsnr", "fwsegsnr_median")


@dataclasses.dataclass
class Reverb:
    """Cepstral distance (dB), log-likelihood ratio (nats) and frequency-weighted segmental SNR (dB) of one recording, speaker
    j = reference j: the mean and the median over the counted frames.  Smaller is better for CD and LLR, larger for fwSegSNR,
    so an improvement ``*_i`` (best assignment minus mixture, a plain difference) is good when NEGATIVE for CD and LLR and when
    POSITIVE for fwSegSNR.  ``valid[j] = False``: reference j has no frame that is not digital silence; every figure is NaN."""
    cd: np.ndarray                        # [S] mean CD(e_j, r_j)
    cd_median: np.ndarray
    llr: np.ndarray
    llr_median: np.ndarray
    fwsegsnr: np.ndarray
    fwsegsnr_median: np.ndarray
    perm_best: List[int]                  # p[j] = the estimate of reference j in the assignment with the least summed mean CD
    cd_best: np.ndarray                   # [S] the figures of (e_p[j], r_j)
    cd_median_best: np.ndarray
    llr_best: np.ndarray
    llr_median_best: np.ndarray
    fwsegsnr_best: np.ndarray
    fwsegsnr_median_best: np.ndarray
    cd_mix: Optional[np.ndarray]          # [S] the figures of (mixture, r_j), or None without a mixture
    cd_median_mix: Optional[np.ndarray]
    llr_mix: Optional[np.ndarray]
    llr_median_mix: Optional[np.ndarray]
    fwsegsnr_mix: Optional[np.ndarray]
    fwsegsnr_median_mix: Optional[np.ndarray]
    cd_i: Optional[np.ndarray]            # [S] cd_best - cd_mix (negative is better), ...
    cd_median_i: Optional[np.ndarray]
    llr_i: Optional[np.ndarray]
    llr_median_i: Optional[np.ndarray]
    fwsegsnr_i: Optional[np.ndarray]      # ... fwsegsnr_best - fwsegsnr_mix (positive is better)
    fwsegsnr_median_i: Optional[np.ndarray]
    frames: np.ndarray                    # [S] int: frames of the recording
    frames_used: np.ndarray               # [S] int: K, those where reference j is not digital silence
    frames_llr: np.ndarray                # [S] int: K_llr of (e_j, r_j)
    valid: np.ndarray                     # [S] bool
    fs: int
    n_samples: int

    def as_dict(self) -> dict:
        out = {}
        for key in REVERB_FIGURES:
            for suffix in ("", "_best", "_mix", "_i"):
                out[key + suffix] = _lst(getattr(self, key + suffix))
        out.update(perm_best=[int(p) for p in self.perm_best], frames=[int(v) for v in self.frames],
                   frames_used=[int(v) for v in self.frames_used], frames_llr=[int(v) for v in self.frames_llr],
                   valid=[bool(v) for v in self.valid], fs=int(self.fs), n_samples=int(self.n_samples))
        return out


def reverb_from_matrices(figures, counts, fs: int = 16000, n_samples: int = 0) -> Reverb:
    """figures float64 [S (+ 1) estimates, S references, 6] and counts int [S (+ 1), S, 3] = (frames, K, K_llr) as the device
    leaves them (the mixture as the last estimate, where there is one) -> :class:`Reverb`.  Host, no GPU."""
    fig = np.array(figures, dtype=np.float64)
    cnt = np.asarray(counts, dtype=np.int64)
    if fig.ndim != 3 or fig.shape[2] != 6 or fig.shape[0] not in (fig.shape[1], fig.shape[1] + 1) \
            or cnt.shape != fig.shape[:2] + (3,):
        raise ValueError("figures must be [S (+ 1), S, 6] (estimates x references) and counts [S (+ 1), S, 3]")
    S = fig.shape[1]
    idx = np.arange(S)
    p = best_perm(-fig[:S, :, 0])
    f = {}
    for k, key in enumerate(REVERB_FIGURES):
        f[key] = fig[idx, idx, k]
        f[key + "_best"] = np.array([fig[p[j], j, k] for j in range(S)])
        f[key + "_mix"] = fig[S, :, k].copy() if fig.shape[0] > S else None
        f[key + "_i"] = f[key + "_best"] - f[key + "_mix"] if fig.shape[0] > S else None
    return Reverb(perm_best=p, frames=cnt[idx, idx, 0], frames_used=cnt[idx, idx, 1], frames_llr=cnt[idx, idx, 2],
                  valid=cnt[idx, idx, 1] >= 1, fs=int(fs), n_samples=int(n_samples), **f)


def reverb_mean_of(items: Sequence[Reverb]) -> dict:
    """The ``"reverb"`` part of the ``"mean"`` entry of scores.json: every figure averaged over the valid speakers"""
    out = _mean_valid(items, [key + suffix for key in REVERB_FIGURES for suffix in ("", "_best", "_mix", "_i")])
    out["n_recordings"] = len(items)
    out["n_speakers_valid"] = int(sum(int(np.sum(e.valid)) for e in items))
    return out


def check_reverb_fs(fs):
    return _check_fs(fs, REVERB_RATES, "CD, LLR and fwSegSNR are")


def reverb_frames(n: int, fs: int) -> int:
    """(n - N) // H + 1 frames of N = fs / 40 samples every H = fs / 100, 0 for n < N; negative outside the limits (n <= 2^24,
    the two rates)"""
    return int(_lib.lib().misonet_reverb_frames(int(n), int(fs)))


def reverb_scratch_bytes(B: int, NS: int, R: int, n: int, fs: int) -> int:
    """bytes of scratch for :func:`reverb_measure` over NS signals per item (R references, the estimates, the mixture) of n
    samples: 8 B (NS + 75 NS f + 3 (NS - R) R f), f = max(frames, 1); negative outside the limits"""
    return int(_lib.lib().misonet_reverb_scratch_bytes(int(B), int(NS), int(R), int(n), int(fs)))


def reverb_measure(est, ref, mix=None, n_valid=None, fs: int = 16000, frame_values: bool = False):
    """est int16 or float32 [B, E, n], ref float32 [B, R, n] (device views as :func:`wave_stats` takes them), mix float32
    [B, 1, n] or None (measured as one more estimate, the last), n_valid int32 [B] (device) or None.  Returns (out float64
    [B, E (+ 1), R, 6] = (CD mean, CD median, LLR mean, LLR median, fwSegSNR mean, fwSegSNR median), count int32
    [B, E (+ 1), R, 3] = (frames, K, K_llr), frame float64 [B, E (+ 1), R, 3, frames of n] or None: the CD, LLR and fwSegSNR of
    every frame, NaN where it is not counted).  Asynchronous on the current stream; an item's rows do not depend on the batch."""
    import torch
    fs = check_reverb_fs(fs)
    B, E, R, n, dev = _check_views(est, ref, mix, n_valid)
    L = _lib.lib()
    NE = E + (1 if mix is not None else 0)
    nb = int(L.misonet_reverb_scratch_bytes(B, R + NE, R, n, fs))
    out = torch.empty((B, NE, R, 6), dtype=torch.float64, device=dev)
    count = torch.empty((B, NE, R, 3), dtype=torch.int32, device=dev)
    frame = None
    if frame_values:
        frame = torch.full((B, NE, R, 3, int(L.misonet_reverb_frames(n, fs))), float("nan"), dtype=torch.float64, device=dev)
    scratch = _scratch(nb, dev)
    _call(L.misonet_reverb_measure, dev, *_view_args(est, ref), *_mix_args(mix), B, E, R, n, _ptr(n_valid), fs, out.data_ptr(),
          count.data_ptr(), frame.data_ptr() if frame is not None and frame.numel() else None, scratch.data_ptr(),
          scratch.numel())
    return out, count, frame


def reverb_frame_values(est, ref, fs: int = 16000, mix=None, n_valid=None):
    """the values of every frame behind the figures, for tests and plots: est / ref / mix / n_valid as :func:`reverb_measure`
    takes them -> float64 [B, E (+ 1), R, 3, frames of n] = the CD, LLR and fwSegSNR of frame t of estimate i against reference
    j, NaN where the frame is not counted"""
    return reverb_measure(est, ref, mix, n_valid, fs, frame_values=True)[2]


def reverb_block(est, ref, mix=None, n_valid=None, fs: int = 16000):
    """est int16 / float32 [B, S, n], ref float32 [B, S, n], mix float32 [B, 1, n] or None (device views), n_valid int32 [B] or
    None -> a device float64 block [B, W]: per item the six figures of every (estimate, reference) pair ([S (+ 1), S, 6], the
    mixture as the last estimate) and (frames, K, K_llr) per pair ([S (+ 1), S, 3]): what :func:`reverb_unpack` reads.
    Everything is queued on the current stream; nothing synchronises.  Batches beyond 1 GiB of scratch run in groups."""
    B, E, n = est.shape
    R = ref.shape[1]
    NS = R + E + (1 if mix is not None else 0)
    per = reverb_scratch_bytes(1, NS, R, max(n, 1), check_reverb_fs(fs))
    return _block_rows(_groups(B, per, REVERB_SCRATCH_CAP), est, ref, mix, n_valid,
                       lambda e, r, m, nv: reverb_measure(e, r, m, nv, fs)[:2])


def reverb_unpack(row, S: int, fs: int, n_samples: int) -> Reverb:
    """one host row of :func:`reverb_block` -> :class:`Reverb`"""
    row = np.asarray(row, dtype=np.float64)
    E = row.shape[0] // (9 * S)
    if E not in (S, S + 1) or row.shape[0] != 9 * S * E:
        raise ValueError("not a row of reverb_block for this number of speakers")
    return reverb_from_matrices(row[:6 * S * E].reshape(E, S, 6), row[6 * S * E:].reshape(E, S, 3), fs=fs, n_samples=n_samples)


def reverb_queue(items, fs: int, dev, pinned: bool = False):
    """:func:`side_queue` for CD / LLR / fwSegSNR alone: the device block [len(items), W] of :func:`reverb_block`"""
    return side_queue(items, dev, pinned, reverb_fs=fs)[2]


def reverb_waves(est, clean, mix=None, fs: int = 16000, device=None) -> Reverb:
    """est int16 or float32 [S, L], clean float32 [S, L], mix float32 [L] or None (ndarrays or tensors, host or device) ->
    :class:`Reverb` (1 <= S <= 4, L <= 2^24, fs 8000 or 16000): the counterpart of :func:`score_waves` for cepstral distance,
    LLR and fwSegSNR, for the output of ``enhance_continuous`` and for files read back from disk."""
    fs = check_reverb_fs(fs)
    return _one_recording(est, _limits, device, lambda e, dev: reverb_queue([(e, clean, mix)], fs, dev),
                          lambda row, S, L: reverb_unpack(row, S, fs, L))


# ---- SRMR: the figure that needs no clean reference ------------------------------------------------------------------------------
# Definition (restated in tests/srmr_ref.py): 23 gammatone channels (Slaney's ERB filters, 125 Hz .. fs / 2),
# the magnitude of the analytic signal of every channel over the whole recording, eight second-order modulation filters (4 .. 128
# Hz, Q = 2), the energy of every 256 ms frame (64 ms hop, Hamming) averaged over the frames; SRMR = the energy in the four
# lowest modulation bands over that in bands 4 .. K* - 1, K* following the bandwidth of the channel that completes 90 % of the
# energy from the top.  The figure has not been compared against the SRMRToolbox or srmrpy: neither was available.
SRMR_RATES = (8000, 16000)
SRMR_CHANNELS, SRMR_MODULATIONS = 23, 8


@dataclasses.dataclass
class Srmr:
    """The speech-to-reverberation modulation energy ratio of the S signals of one recording; larger is better, and nothing is
    paired with anything, so there is no permutation.  ``srmr_i = srmr - srmr_mix`` is an improvement when POSITIVE.
    ``valid[j] = False``: signal j is shorter than one 256 ms frame or has no energy; its figures are NaN and ``k_star`` 0."""
    srmr: np.ndarray                      # [S]
    k_star: np.ndarray                    # [S] int: modulation bands 4 .. k_star - 1 form the denominator (5 .. 8)
    bw90: np.ndarray                      # [S] Hz: ERB of the channel that completes 90 % of the energy from the top
    frames: np.ndarray                    # [S] int
    valid: np.ndarray                     # [S] bool
    srmr_mix: Optional[float]             # the figure of the mixture, or None without one
    srmr_i: Optional[np.ndarray]          # [S] srmr - srmr_mix (positive is better)
    energy: Optional[np.ndarray]          # [S, 23, 8] the mean modulation energies, channels ascending, or None
    fs: int
    n_samples: int

    def as_dict(self) -> dict:
        return dict(srmr=_lst(self.srmr), k_star=[int(v) for v in self.k_star], bw90=_lst(self.bw90),
                    frames=[int(v) for v in self.frames], valid=[bool(v) for v in self.valid],
                    srmr_mix=None if self.srmr_mix is None else float(self.srmr_mix), srmr_i=_lst(self.srmr_i),
                    fs=int(self.fs), n_samples=int(self.n_samples))


def check_srmr_fs(fs):
    return _check_fs(fs, SRMR_RATES, "SRMR is")


def srmr_frames(n: int, fs: int) -> int:
    """1 + (n - N_w) // H_w frames of N_w = ceil(0.256 fs) samples every H_w = ceil(0.064 fs), 0 for n < N_w; negative outside
    the limits (0 <= n <= 2^24, the two rates)"""
    return int(_lib.lib().misonet_srmr_frames(int(n), int(fs)))


def srmr_chunk() -> int:
    """the samples of a chunk of the scan that runs the recurrences in parallel along time"""
    return int(_lib.lib().misonet_srmr_chunk())


def srmr_scratch_bytes(B: int, NS: int, n: int, fs: int) -> int:
    """bytes of scratch for :func:`srmr_measure` over NS signals per item of n samples: the 184 means of every signal and as many
    slots of one (signal, channel) as fit 1 GiB, at least one -- bounded whatever B; negative outside the limits"""
    return int(_lib.lib().misonet_srmr_scratch_bytes(int(B), int(NS), int(n), int(fs)))


def srmr_measure(sig, mix=None, n_valid=None, fs: int = 16000, energy: bool = False, scratch=None):
    """sig int16 or float32 [B, S, n] (a device view as :func:`wave_stats` takes its estimates), mix float32 [B, 1, n] or None
    (measured as one more signal, the last), n_valid int32 [B] (device) or None.  Returns (out float64 [B, S (+ 1), 3] = (SRMR,
    K*, BW), count int32 [B, S (+ 1)] = the frames, energy float64 [B, S (+ 1), 23, 8] or None).  Asynchronous on the current
    stream; an item's rows do not depend on the batch.  ``scratch``: a uint8 device tensor of at least
    :func:`srmr_scratch_bytes` bytes to work in (its contents do not matter); by default one is allocated."""
    import torch
    fs = check_srmr_fs(fs)
    B, S, _, n, dev = _check_views(sig, None, mix, n_valid, what="sig")
    L = _lib.lib()
    NS = S + (1 if mix is not None else 0)
    nb = int(L.misonet_srmr_scratch_bytes(B, NS, n, fs))
    out = torch.empty((B, NS, 3), dtype=torch.float64, device=dev)
    count = torch.empty((B, NS), dtype=torch.int32, device=dev)
    en = torch.empty((B, NS, SRMR_CHANNELS, SRMR_MODULATIONS), dtype=torch.float64, device=dev) if energy else None
    if scratch is None:
        scratch = _scratch(nb, dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.uint8 or scratch.device != dev \
            or not scratch.is_contiguous() or scratch.numel() < nb or scratch.data_ptr() % 16:
        raise ValueError(f"scratch must be a contiguous uint8 device tensor of at least {nb} bytes, 16-byte aligned")
    _call(L.misonet_srmr_measure, dev, *_view_args(sig), *_mix_args(mix), B, S, n, _ptr(n_valid), fs, out.data_ptr(),
          count.data_ptr(), _ptr(en), scratch.data_ptr(), scratch.numel())
    return out, count, en


def srmr_block(sig, mix=None, n_valid=None, fs: int = 16000):
    """sig int16 / float32 [B, S, n], mix float32 [B, 1, n] or None (device views), n_valid int32 [B] or None -> a device float64
    block [B, W]: per item (SRMR, K*, BW) of every signal ([S (+ 1), 3], the mixture last) and the frames ([S (+ 1)]): what
    :func:`srmr_unpack` reads.  Everything is queued on the current stream; nothing synchronises.  The scratch is bounded by the
    library itself (the channels run in groups), so a batch is one call."""
    import torch
    out, count, _ = srmr_measure(sig, mix, n_valid, fs)
    B = out.shape[0]
    return torch.cat([out.reshape(B, -1), count.to(torch.float64).reshape(B, -1)], dim=1)


def srmr_from_rows(figures, frames, fs: int = 16000, n_samples: int = 0, S: Optional[int] = None, energy=None) -> Srmr:
    """figures float64 [S (+ 1), 3] = (SRMR, K*, BW) and frames int [S (+ 1)] as the device leaves them (the mixture last, where
    there is one: S tells) -> :class:`Srmr`.  Host, no GPU."""
    fig = np.array(figures, dtype=np.float64)
    fr = np.asarray(frames, dtype=np.int64)
    if fig.ndim != 2 or fig.shape[1] != 3 or fr.shape != fig.shape[:1]:
        raise ValueError("figures must be [S (+ 1), 3] and frames [S (+ 1)]")
    S = fig.shape[0] if S is None else int(S)
    if fig.shape[0] not in (S, S + 1) or S < 1:
        raise ValueError("figures must hold S signals, or S and the mixture")
    with_mix = fig.shape[0] == S + 1
    srmr = fig[:S, 0].copy()
    mixv = float(fig[S, 0]) if with_mix else None
    return Srmr(srmr=srmr, k_star=fig[:S, 1].astype(np.int64), bw90=fig[:S, 2].copy(), frames=fr[:S].copy(),
                valid=np.isfinite(srmr) & (fr[:S] >= 1), srmr_mix=mixv, srmr_i=srmr - mixv if with_mix else None,
                energy=None if energy is None else np.array(energy, dtype=np.float64)[:S], fs=int(fs), n_samples=int(n_samples))


def srmr_unpack(row, S: int, fs: int, n_samples: int) -> Srmr:
    """one host row of :func:`srmr_block` -> :class:`Srmr`"""
    row = np.asarray(row, dtype=np.float64)
    NS = row.shape[0] // 4
    if NS not in (S, S + 1) or row.shape[0] != 4 * NS:
        raise ValueError("not a row of srmr_block for this number of signals")
    return srmr_from_rows(row[:3 * NS].reshape(NS, 3), row[3 * NS:], fs=fs, n_samples=n_samples, S=S)


def srmr_mean_of(items: Sequence[Srmr]) -> dict:
    """The ``"srmr"`` part of the ``"mean"`` entry of scores.json: the figures averaged over the valid signals"""
    out = _mean_valid(items, ("srmr", "srmr_i"))
    mixes = [float(e.srmr_mix) for e in items if e.srmr_mix is not None and np.isfinite(e.srmr_mix)]
    out["srmr_mix"] = float(np.mean(mixes)) if mixes else None
    out["n_recordings"] = len(items)
    out["n_signals_valid"] = int(sum(int(np.sum(e.valid)) for e in items))
    return out


def srmr_queue(items, fs: int, dev, pinned: bool = False):
    """items: a list of (signals int16 or float32 [S, L], mix float32 [L] or None) (ndarrays or tensors; the same S and all or
    none with a mixture; any lengths) -> the device block [len(items), W] of :func:`srmr_block`, queued on the current stream
    of ``dev``: one padded batch with ``n_valid`` set, a row bit for bit what the recording gives alone"""
    import torch
    fs = check_srmr_fs(fs)
    with torch.cuda.device(dev):
        sig, _, mix, nv = _wave_batch([(sig, None, mix) for sig, mix in items], dev, pinned, _signal_limits)
        return srmr_block(sig, mix, nv, fs)


def srmr_waves(waves, mix=None, fs: int = 16000, device=None) -> Srmr:
    """waves int16 or float32 [S, L], mix float32 [L] or None (ndarrays or tensors, host or device) -> :class:`Srmr`
    (1 <= S <= 4, L <= 2^24, fs 8000 or 16000): the figure for the output of ``enhance_continuous``, ``dereverb_wav`` and for
    files read back from disk, none of which has a clean reference."""
    import torch
    fs = check_srmr_fs(fs)
    waves = torch.as_tensor(waves)
    if waves.dim() != 2:
        raise ValueError("waves must be [S, L]")
    return _one_recording(waves, _signal_limits, device, lambda w, dev: srmr_queue([(w, mix)], fs, dev),
                          lambda row, S, L: srmr_unpack(row, S, fs, L))


# ---- the figures beside the scores: one table for side_queue and for the recording paths of pipeline.py ------------------
@dataclasses.dataclass(frozen=True)
class SideFigure:
    """A figure computed from the stitched result of a recording.  ``name`` is the flag of ``Enhancer.enhance_recording`` /
    ``enhance_recordings``; its parameter is the filter length for "bss" and the rate ``fs`` for the others."""
    name: str
    rates: Optional[Tuple[int, ...]]      # the rates it is defined for, None: any
    check: object                         # parameter -> the parameter as the calls below take it, or ValueError
    limits: object                        # (S, L): ValueError for a recording the figure does not take
    block: object                         # (est, clean, mix, n_valid, parameter) -> device block [B, W]; SRMR: without clean
    unpack: object                        # (host row, S, parameter, n_samples) -> the dataclass
    waves: object                         # (est [S, L], clean, mix, parameter, device) -> the dataclass of one recording
    needs_clean: bool                     # takes the clean sources, hence score=True


SIDE_FIGURES = (
    SideFigure("bss", None, _check_filt_len, _limits, bss_energies, bss_unpack, bss_eval_waves, True),
    SideFigure("stoi", STOI_RATES, check_stoi_fs, _limits, stoi_block, stoi_unpack, stoi_waves, True),
    SideFigure("reverb", REVERB_RATES, check_reverb_fs, _limits, reverb_block, reverb_unpack, reverb_waves, True),
    SideFigure("srmr", SRMR_RATES, check_srmr_fs, _signal_limits, srmr_block, srmr_unpack,
               lambda est, clean, mix, fs, device: srmr_waves(est, mix, fs, device), False),
)
