"""Guided spatial clustering between the separation network and the beamformer (csrc/cacgmm.hip, C ABI ``misonet_cacgmm`` /
``misonet_masks_from_estimates`` in include/misonet.h).

The complex angular central Gaussian mixture model (cACGMM; Ito, Araki & Nakatani 2016) re-estimates the time-frequency masks
of S speakers and the noise from the observation itself, started from -- and, with ``prior="guided"``, held to -- the masks of
the network's estimate.  The refined source image ``gamma_s * Y`` has the shape and the meaning of the source estimate every
beamformer of :mod:`misonet_amd.beamform` consumes.  This is the project's own definition in the pb_bss / GSS family; nothing
here was compared against pb_bss.

``masks_from_estimates(est, mix)``        -- initial masks [B, S + 1, F, T] from the estimates [B, S, F, M, T] and the mixture
``cacgmm(mix, init_masks, ...)``          -- the EM; masks, optionally the images [B, S, F, M, T] and the diagnostics
``Refine``                                -- the options as plain data, for :class:`misonet_amd.pipeline.Enhancer`
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from ._online import _dev_c64, spec_of

PRIORS = ("bin", "guided")                   # the priors of misonet_cacgmm_opts, in its numbering
MAX_ITERATIONS = 1000


@dataclasses.dataclass(frozen=True)
class Refine:
    """One plain-data description of the clustering step (``misonet_cacgmm_opts`` of include/misonet.h).

    iterations   EM iterations (E-step, then M-step; the last one the E-step only); 0 returns the initial masks
    prior        "bin": one mixture weight per class and bin, re-estimated (pb_bss's default); "guided": the initial mask of
                 every frame, floored at ``prior_floor``, is that frame's prior in every iteration
    diag_load    B_k += diag_load tr(B_k) / M I
    prior_floor  the floor of the guided prior (> 0 there)
    """
    iterations: int = 10
    prior: str = "bin"
    diag_load: float = 1e-8
    prior_floor: float = 1e-6

    @classmethod
    def of(cls, spec) -> "Refine":
        """None or True (the defaults), a Refine, a prior name, or a dict of the fields above"""
        return spec_of(cls, spec, "refine", "refine must be None, True, a Refine, a prior name or a dict of its fields", "prior")

    def validate(self, num_mic=None, num_spks=None) -> "Refine":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        v = self.iterations
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= MAX_ITERATIONS:
            raise ValueError(f"refine iterations must be an integer in [0, {MAX_ITERATIONS}], got {v!r}")
        if self.prior not in PRIORS:
            raise ValueError(f"refine prior {self.prior!r}: one of {PRIORS}")
        for name in ("diag_load", "prior_floor"):
            v = getattr(self, name)
            if isinstance(v, bool) or not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f"refine {name} must be finite and >= 0, got {v!r}")
        if self.prior == "guided" and not self.prior_floor > 0:
            raise ValueError("refine prior_floor must be > 0 with the guided prior")
        if num_mic is not None and not 2 <= num_mic <= 8:
            raise ValueError(f"refine needs 2 <= M <= 8 microphones, got {num_mic}")
        if num_spks is not None and not 1 <= num_spks <= 4:
            raise ValueError(f"refine needs 1 <= S <= 4 speakers, got {num_spks}")
        return self

    def c_opts(self) -> "_lib.CacgmmOpts":
        return _lib.CacgmmOpts(int(self.iterations), PRIORS.index(self.prior), float(self.diag_load), float(self.prior_floor))


def masks_from_estimates(est, mix, device=None):
    """Initial masks from source estimates: est complex [B, S, F, M, T], mix complex [B, F, M, T] (ndarrays or tensors) ->
    float32 [B, S + 1, F, T] (speakers, then noise): P_s = sum_m |est_s|^2, P_n = sum_m |y - sum_s est_s|^2, each over their
    sum; 1 / (S + 1) where that sum is 0.  On the CPU when the inputs were ndarrays, on the device otherwise."""
    if np.ndim(est) != 5 or np.ndim(mix) != 4 or tuple(np.shape(est)[:1] + np.shape(est)[2:]) != tuple(np.shape(mix)):
        raise ValueError(f"est {tuple(np.shape(est))} must be [B, S, F, M, T] and mix {tuple(np.shape(mix))} [B, F, M, T]")
    B, S, F, M, T = np.shape(est)
    Refine().validate(M, S)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    e, np_in = _dev_c64(est, device)
    y, _ = _dev_c64(mix, e.device)
    out = torch.empty((B, S + 1, F, T), dtype=torch.float32, device=e.device)
    with torch.cuda.device(e.device):
        _lib.check(_lib.lib().misonet_masks_from_estimates(e.data_ptr(), y.data_ptr(), B, S, F, M, T, out.data_ptr(),
                                                           _lib.stream_ptr(e.device)))
    return out.cpu() if np_in else out


def cacgmm(mix, init_masks, iterations=10, prior="bin", diag_load=1e-8, prior_floor=1e-6, device=None, return_images=False,
           return_debug=False, *, refine=None):
    """The guided cACGMM.  mix complex [B, F, M, T] (the beamformer's layout), init_masks real [B, K, F, T], K = S + 1 classes
    (the speakers, then the noise) -> the masks float32 [B, K, F, T]; with ``return_images`` also the refined source images
    ``gamma_s * Y`` complex64 [B, S, F, M, T] (``images[:, s]`` is a ``source_stft`` of ``Apply_Beamforming``); with
    ``return_debug`` also a dict of device tensors: ``B`` complex128 [B, F, K, M, M] (the last M-step's, as factored), ``pi``
    float64 [B, F, K], ``ll`` float64 [B, F] (the log-likelihood of the last E-step) and ``fail`` int32 [B, F].  The results
    are on the CPU when ``mix`` was an ndarray, on the device otherwise.  The options are the fields of :class:`Refine`
    (``refine``: a whole Refine or dict, which wins).  A bin the EM cannot solve keeps its initial masks (``fail`` = 1)."""
    opt = (Refine(iterations=iterations, prior=prior, diag_load=diag_load, prior_floor=prior_floor) if refine is None
           else Refine.of(refine))
    if np.ndim(mix) != 4 or np.ndim(init_masks) != 4:
        raise ValueError(f"mix {tuple(np.shape(mix))} must be [B, F, M, T] and init_masks {tuple(np.shape(init_masks))} "
                         "[B, K, F, T]")
    B, F, M, T = np.shape(mix)
    K = np.shape(init_masks)[1]
    if tuple(np.shape(init_masks)) != (B, K, F, T):
        raise ValueError(f"init_masks {tuple(np.shape(init_masks))} must be [B, K, F, T] = [{B}, K, {F}, {T}]")
    opt.validate(M, K - 1)                                                   # before any copy or launch
    if T < 1 or B < 1 or F < 1:
        raise ValueError("B, F and T must be positive")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    y, np_in = _dev_c64(mix, device)
    g0 = torch.as_tensor(init_masks)
    if g0.is_complex():
        raise TypeError("init_masks must be real")
    g0 = g0.to(y.device).to(torch.float32).contiguous()
    S = K - 1
    L = _lib.lib()
    opts = opt.c_opts()
    nws = L.misonet_cacgmm_workspace_bytes(B, K, F, M)
    if nws < 0:
        _lib.check(_lib.EINVAL)
    ws = torch.empty(max(int(nws), 8), dtype=torch.uint8, device=y.device)
    masks = torch.empty((B, K, F, T), dtype=torch.float32, device=y.device)
    images = torch.empty((B, S, F, M, T), dtype=torch.complex64, device=y.device) if return_images else None
    dbg = None
    with torch.cuda.device(y.device):
        st = _lib.stream_ptr(y.device)
        _lib.check(L.misonet_cacgmm(y.data_ptr(), g0.data_ptr(), B, K, F, M, T, C.byref(opts), masks.data_ptr(),
                                    images.data_ptr() if return_images else None, ws.data_ptr(), ws.numel(), st))
        if return_debug:
            dbg = dict(B=torch.empty((B, F, K, M, M), dtype=torch.complex128, device=y.device),
                       pi=torch.empty((B, F, K), dtype=torch.float64, device=y.device),
                       ll=torch.empty((B, F), dtype=torch.float64, device=y.device),
                       fail=torch.empty((B, F), dtype=torch.int32, device=y.device))
            _lib.check(L.misonet_cacgmm_debug(ws.data_ptr(), B, K, F, M, dbg["B"].data_ptr(), dbg["pi"].data_ptr(),
                                              dbg["ll"].data_ptr(), dbg["fail"].data_ptr(), st))
    if np_in:
        masks = masks.cpu()
        images = images.cpu() if images is not None else None
    res = [masks] + ([images] if return_images else []) + ([dbg] if return_debug else [])
    return res[0] if len(res) == 1 else tuple(res)


def refined_images(est, mix, refine):
    """The composition the fused pass runs as its step 4b, on device tensors: est complex [B, S, F, M, T] (the aligned MISO1
    estimates), mix complex [B, F, M, T] -> the refined source images complex64 [B, S, F, M, T]"""
    return cacgmm(mix, masks_from_estimates(est, mix), return_images=True, refine=Refine.of(refine))[1]
