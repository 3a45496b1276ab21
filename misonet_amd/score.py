"""Scores of separated output against clean references: SI-SDR and its improvement over the mixture, SNR, the best
permutation, and the reference's training criterion (criterion.py ``loss_uPIT`` / ``loss_Enhance``).  The sums run on the
device (csrc/score.hip, C ABI ``misonet_score_wave`` / ``misonet_score_spec``); the handful of doubles they leave is turned
into dB on the host.  tests/score_ref.py restates every definition in NumPy.

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
        def lst(x):
            return None if x is None else [float(v) for v in np.asarray(x, dtype=np.float64)]
        return dict(si_sdr=lst(self.si_sdr), si_sdr_mix=lst(self.si_sdr_mix), si_sdri=lst(self.si_sdri), snr=lst(self.snr),
                    valid=[bool(v) for v in self.valid], perm_best=[int(p) for p in self.perm_best],
                    si_sdr_best=lst(self.si_sdr_best), n_samples=int(self.n_samples),
                    loss_miso1=None if self.loss_miso1 is None else float(self.loss_miso1),
                    loss_enhance=lst(self.loss_enhance))


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


def mean_of(scores: Sequence[Score]) -> dict:
    """The ``"mean"`` entry of scores.json: the dB figures averaged over the valid speakers of every recording, the
    criterion values over the recordings that have them."""
    out = {}
    for key in ("si_sdr", "si_sdr_mix", "si_sdri", "snr", "si_sdr_best"):
        vals = [float(getattr(s, key)[j]) for s in scores if getattr(s, key) is not None
                for j in range(len(s.valid)) if s.valid[j] and np.isfinite(getattr(s, key)[j])]
        out[key] = float(np.mean(vals)) if vals else None
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
    if n_valid is not None:
        if not isinstance(n_valid, torch.Tensor) or n_valid.dtype != torch.int32 or n_valid.device != dev \
                or n_valid.numel() != B or not n_valid.is_contiguous():
            raise ValueError(f"n_valid must be a contiguous int32 device tensor of {B} entries")
    out = torch.empty((B, E, R, 5), dtype=torch.float64, device=dev)
    L = _lib.lib()
    nb = max(8, int(L.misonet_score_scratch_bytes(B, max(E, 1), max(R, 1), n))) if B > 0 and n > 0 else 8
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.misonet_score_wave(est.data_ptr(), 1 if est.dtype == torch.int16 else 0, est.stride(0), est.stride(1),
                                        est.stride(2), ref.data_ptr(), ref.stride(0), ref.stride(1), ref.stride(2), B, E, R,
                                        n, n_valid.data_ptr() if n_valid is not None else None, out.data_ptr(),
                                        scratch.data_ptr(), scratch.numel(), _lib.stream_ptr(dev)))
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
    nb = max(8, int(L.misonet_score_scratch_bytes(B, max(E, 1), max(R, 1), F))) if B > 0 and F > 0 else 8
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.misonet_score_spec(est.data_ptr(), est.stride(0), est.stride(1), est.stride(2), ref.data_ptr(),
                                        ref.stride(0), ref.stride(1), ref.stride(2), B, E, R, T, F, pair.data_ptr(),
                                        perm.data_ptr() if pick else None, val.data_ptr() if pick else None,
                                        scratch.data_ptr(), scratch.numel(), _lib.stream_ptr(dev)))
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
