"""Continuous separation of long recordings without clean references: windows of ``W`` samples at a hop of ``H`` (the
reference trains on 4 s windows at a 2 s hop, dataloader/SMS_WSJ.py:225-227), each through the fused pass, the speaker
order of every window linked to the previous one through their shared frames, and a raised-cosine cross-fade over the
overlap (csrc/css.hip, C ABI ``misonet_css_align`` / ``misonet_css_stitch``).

Semantics ("Long recordings without clean references"):
  * windows: ``K = 1`` if ``L <= W`` else ``1 + ceil((L - W) / H)``; window k is ``wav[kH : kH + W]``, zero-padded past L;
  * D_k[i][j] = sum over the ``T - H/64`` shared frames and the bins of | |X_{k-1}[i, t + H/64]| - |X_k[j, t]| | (float64);
  * L_k = the cheapest permutation (itertools order, first minimum); P_0 = identity, P_k[s] = L_k[P_{k-1}[s]];
  * out[s][m] = y_k[P_k[s]][j] (k = min(K-1, m // H), j = m - kH), and for k >= 1, j < ov = W - H:
    c(j) y_{k-1}[P_{k-1}[s]][H + j] + r(j) y_k[P_k[s]][j], r = sin^2, c = cos^2 of pi (j + 1/2) / (2 ov).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib

HOP = 64            # STFT hop: window and hop must be whole frames
MIN_OVERLAP = 256   # four hops: at least five shared frames


def plan_windows(L: int, W: int = 64000, H: Optional[int] = None) -> Tuple[List[int], int, int]:
    """The window plan of a recording of ``L`` samples: (starts, K, padded length ``(K - 1) H + W``).  ``H = None``: W // 2.
    Raises ValueError unless 64 | W, 64 | H and W/2 <= H <= W - 256."""
    W = int(W)
    H = W // 2 if H is None else int(H)
    L = int(L)
    if L < 1:
        raise ValueError(f"the recording must hold at least one sample (got {L})")
    if W <= 0 or W % HOP or H <= 0 or H % HOP:
        raise ValueError(f"window ({W}) and hop ({H}) must be positive multiples of {HOP} samples")
    if 2 * H < W or H > W - MIN_OVERLAP:
        raise ValueError(f"hop {H} outside [W/2, W - {MIN_OVERLAP}] = [{W // 2}, {W - MIN_OVERLAP}] for window {W}")
    K = 1 if L <= W else 1 + -(-(L - W) // H)
    return [k * H for k in range(K)], K, (K - 1) * H + W


def scratch_bytes(K: int, S: int, F: int = 129) -> int:
    """bytes of the ``dist`` scratch of :func:`align` for K windows: (K - 1) S S (F + 1) doubles"""
    return int(_lib.lib().misonet_css_scratch_bytes(int(K), int(S), int(F)))


def align(est: torch.Tensor, hop_frames: int, perm0: Optional[torch.Tensor] = None, perm: Optional[torch.Tensor] = None,
          dist: Optional[torch.Tensor] = None):
    """est complex64 [K, S, T, 129] (device): K consecutive windows ``hop_frames`` frames apart.  ``perm0`` int32 [S] = the
    P of est[0] (None: identity, est[0] is the recording's first window).  Returns (perm int32 [K, S] with output speaker s
    of window k = est[k, perm[k, s]], D float64 [K - 1, S, S]).  ``perm`` (int32 [K, S]) and ``dist`` (uint8,
    :func:`scratch_bytes`) may be given to avoid the allocations.  Asynchronous on the current stream."""
    if not isinstance(est, torch.Tensor) or est.dim() != 4 or est.dtype != torch.complex64 or not est.is_cuda:
        raise ValueError("est must be a complex64 device tensor [K, S, T, F]")
    est = est.contiguous()
    K, S, T, F = est.shape
    dev = est.device
    if perm is None:
        perm = torch.empty((K, S), dtype=torch.int32, device=dev)
    if perm0 is not None:
        perm0 = perm0.to(device=dev, dtype=torch.int32).contiguous()
        if perm0.numel() != S:
            raise ValueError(f"perm0 must hold {S} entries")
    n = max(0, scratch_bytes(K, S, F))
    if dist is None:
        dist = torch.empty(max(n, 8), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        _lib.check(L.misonet_css_align(est.data_ptr(), K, S, T, F, int(hop_frames),
                                       perm0.data_ptr() if perm0 is not None else None, perm.data_ptr(), dist.data_ptr(),
                                       dist.numel() * dist.element_size(), _lib.stream_ptr(dev)))
    nd = max(0, K - 1) * S * S
    D = dist.view(torch.uint8)[: nd * 8].view(torch.float64).reshape(max(0, K - 1), S, S)
    return perm, D


def stitch(y: torch.Tensor, perms: torch.Tensor, hop: int, first: bool, n_out: int, dtype=torch.int16,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y float32 [K, S, W] (device): the iSTFT of K consecutive windows; perms int32 [K, S].  ``first``: y[0] is the
    recording's first window and its samples are written; otherwise y[0] is the window carried over from the previous call
    and only the samples of windows 1..K-1 are written.  Returns ``dtype`` (int16 or float32) [S, n_out] (``out``: a
    contiguous tensor of that shape and type to write into).  Asynchronous on the current stream."""
    if not isinstance(y, torch.Tensor) or y.dim() != 3 or y.dtype != torch.float32 or not y.is_cuda:
        raise ValueError("y must be a float32 device tensor [K, S, W]")
    if dtype not in (torch.int16, torch.float32):
        raise ValueError("dtype must be torch.int16 or torch.float32")
    y = y.contiguous()
    K, S, W = y.shape
    perms = perms.to(device=y.device, dtype=torch.int32).contiguous()
    if tuple(perms.shape) != (K, S):
        raise ValueError(f"perms must be [{K}, {S}]")
    n_out = int(n_out)
    if out is None:
        out = torch.empty((S, max(0, n_out)), dtype=dtype, device=y.device)
    elif out.dtype != dtype or tuple(out.shape) != (S, n_out) or not out.is_contiguous() or out.device != y.device:
        raise ValueError(f"out must be a contiguous {dtype} tensor [{S}, {n_out}] on {y.device}")
    L = _lib.lib()
    with torch.cuda.device(y.device):
        _lib.check(L.misonet_css_stitch(y.data_ptr(), perms.data_ptr(), K, S, W, int(hop), 1 if first else 0, n_out,
                                        out.data_ptr() if dtype == torch.int16 else None,
                                        out.data_ptr() if dtype == torch.float32 else None, _lib.stream_ptr(y.device)))
    return out
