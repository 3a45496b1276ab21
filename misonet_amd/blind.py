"""Blind separation as a weight-free front end (csrc/iva.hip, C ABI ``misonet_auxiva`` in include/misonet.h).

Auxiliary-function independent vector analysis with iterative source steering (AuxIVA-ISS; Ono 2011, Scheibler & Ono 2020)
behind a per-bin PCA to ``channels`` channels, projected back to all microphones by least squares.  Its images have the shape and
the meaning of the source estimate that every block behind MISO1 consumes -- the beamformers of :mod:`misonet_amd.beamform`, the
guided cACGMM of :mod:`misonet_amd.refine`, the writers and the scores -- so that whole back half runs on real recordings
without a trained network.  This is the project's own definition in the pyroomacoustics / torchiva family; nothing here was
compared against those packages.

``auxiva(mix, num_spks, ...)``   -- the separation; images complex64 [B, S, F, M, T], optionally the chosen rows and the diagnostics
``AuxIVA``                       -- the options as plain data
``BlindSeparator``               -- the recording-level composition: AuxIVA -> (cACGMM) -> beamformer -> iSTFT -> files

Online AuxIVA (csrc/oiva.hip, C ABI ``misonet_oiva``): the frame-recursive form of the determined case
(K = M, no PCA; Taniguchi, Ono, Kawamura & Sagayama 2014), fed audio as it arrives in the stream layout [B, M, T, F] of
:class:`misonet_amd.dereverb.DereverbStream`.  It is not a better separator than :func:`auxiva`.

``SeparateStream``               -- the state of one stream; ``process(block)`` takes any T >= 1 new frames
``auxiva_online(mix, ...)``      -- the one-shot call: reset, then process
``OnlineAuxIVA``                 -- its options as plain data

With ``num_src`` = K below the number of microphones the same three run the overdetermined form (csrc/overiva.hip, C ABI
``misonet_overiva``; OverIVA, Scheibler & Ono 2019, frame-recursive): K rows out, the other M - K rows of the
demixing matrix fixed as [J, -I].  The project's own definition; nothing was compared against other packages.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import stft as S
from ._online import OnlineStream, _dev_c64, check_index, check_real, default_device, spec_of
from .beamform import Beamformer, JointBeamformer

MODELS = ("gauss", "laplace")                # the source models of misonet_iva_opts, in its numbering
MAX_ITERATIONS = 1000


@dataclasses.dataclass(frozen=True)
class AuxIVA:
    """One plain-data description of the separation (``misonet_iva_opts`` of include/misonet.h).

    iterations   sweeps over the sources (weights once, then every source steered once); 0 returns the PCA projection's images
    model        "gauss": time-varying Gaussian, phi = 1 / max(mean_f |y|^2, floor); "laplace": phi = 1 / max(2 sqrt(sum_f |y|^2),
                 floor), the textbook model
    channels     K, the channels kept by the per-bin PCA, S <= K <= M; None = the number of sources
    floor        the floor under the weights' denominators (> 0)
    ref_ch       the microphone the eigenvectors' phase and the sources' power are taken at
    """
    iterations: int = 20
    model: str = "gauss"
    channels: Optional[int] = None
    floor: float = 1e-10
    ref_ch: int = 0

    @classmethod
    def of(cls, spec) -> "AuxIVA":
        """None or True (the defaults), an AuxIVA, a model name, or a dict of the fields above"""
        return spec_of(cls, spec, "blind", "blind must be None, True, an AuxIVA, a model name or a dict of its fields", "model")

    def validate(self, num_mic=None, num_spks=None) -> "AuxIVA":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if not integer(self.iterations) or not 0 <= self.iterations <= MAX_ITERATIONS:
            raise ValueError(f"blind iterations must be an integer in [0, {MAX_ITERATIONS}], got {self.iterations!r}")
        if self.model not in MODELS:
            raise ValueError(f"blind model {self.model!r}: one of {MODELS}")
        v = self.floor
        if isinstance(v, bool) or not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0):
            raise ValueError(f"blind floor must be finite and > 0, got {v!r}")
        if self.channels is not None and (not integer(self.channels) or self.channels < 1):
            raise ValueError(f"blind channels must be None or a positive integer, got {self.channels!r}")
        check_index("blind", "ref_ch", self.ref_ch)
        if num_mic is not None:
            if not 2 <= num_mic <= 8:
                raise ValueError(f"blind separation needs 2 <= M <= 8 microphones, got {num_mic}")
            if self.ref_ch >= num_mic:
                raise ValueError(f"blind ref_ch {self.ref_ch} outside [0, {num_mic})")
        if num_spks is not None:
            if not 1 <= num_spks <= 4 or (num_mic is not None and num_spks > num_mic):
                raise ValueError(f"blind separation needs 1 <= S <= min(M, 4) sources, got {num_spks}")
            if self.channels is not None and not num_spks <= self.channels <= (8 if num_mic is None else num_mic):
                raise ValueError(f"blind channels must lie in [S, M], got {self.channels}")
        return self

    def num_channels(self, num_spks) -> int:
        return int(num_spks if self.channels is None else self.channels)

    def c_opts(self) -> "_lib.IvaOpts":
        return _lib.IvaOpts(int(self.iterations), MODELS.index(self.model), int(self.channels or 0), int(self.ref_ch),
                            float(self.floor))


@dataclasses.dataclass(frozen=True)
class OnlineAuxIVA:
    """One plain-data description of the online separation (``misonet_oiva_opts`` of include/misonet.h).

    alpha    forgetting factor of the weighted covariances, 0 < alpha < 1 (1 would freeze them)
    model    "gauss": phi = 1 / max(mean_f |y|^2, floor); "laplace": phi = 1 / max(2 sqrt(sum_f |y|^2), floor), per frame
    floor    the floor under the weights' denominators (> 0)
    init     V_k = init I at reset (> 0)
    ref_ch   the microphone ``est`` is projected to
    num_src  K, the sources the stream returns: None or the number of microphones -- the determined case, ``misonet_oiva``;
             1 <= K < M -- the overdetermined one, ``misonet_overiva``, K rows out

    ``num_src`` is a dimension and not a member of ``misonet_oiva_opts``: it is the last argument of the constructor, it is
    kept by ``dataclasses.replace`` and compared by ``==``, and ``dataclasses.astuple`` / ``asdict`` stay the five members of the
    C structure, as they were.  :meth:`as_kwargs` has all six.
    """
    alpha: float = 0.98
    model: str = "gauss"
    floor: float = 1e-10
    init: float = 1.0
    ref_ch: int = 0
    num_src: dataclasses.InitVar[Optional[int]] = None

    def __post_init__(self, num_src):
        object.__setattr__(self, "num_src", num_src)

    def __eq__(self, other):
        if other.__class__ is not self.__class__:
            return NotImplemented
        return self.as_kwargs() == other.as_kwargs()

    def __repr__(self):
        return f"OnlineAuxIVA({', '.join(f'{k}={v!r}' for k, v in self.as_kwargs().items())})"

    def as_kwargs(self) -> dict:
        """every argument of the constructor, ``num_src`` included"""
        return dict(dataclasses.asdict(self), num_src=self.num_src)

    def sources(self, num_mic: int) -> int:
        """K: the rows the stream returns at ``num_mic`` microphones"""
        return int(num_mic if self.num_src is None else self.num_src)

    @classmethod
    def of(cls, spec) -> "OnlineAuxIVA":
        """None or True (the defaults), an OnlineAuxIVA, a model name, or a dict of the fields above"""
        return spec_of(cls, spec, "online blind",
                       "online must be None, True, an OnlineAuxIVA, a model name or a dict of its fields", "model")

    def validate(self, num_mic: Optional[int] = None) -> "OnlineAuxIVA":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        if self.model not in MODELS:
            raise ValueError(f"online blind model {self.model!r}: one of {MODELS}")
        for name in ("alpha", "floor", "init"):
            check_real("online blind", name, getattr(self, name), positive=True)
        if not self.alpha < 1:
            raise ValueError(f"online blind alpha must be in (0, 1), got {self.alpha!r}")
        r = self.ref_ch
        check_index("online blind", "ref_ch", r)
        if num_mic is not None:
            if not 2 <= num_mic <= 8:
                raise ValueError(f"online blind separation needs 2 <= M <= 8 microphones, got {num_mic}")
            if r >= num_mic:
                raise ValueError(f"online blind ref_ch {r} outside [0, {num_mic})")
        k = self.num_src
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
                raise ValueError(f"online blind num_src must be None or a positive integer, got {k!r}")
            if num_mic is not None and k > num_mic:
                raise ValueError(f"online blind num_src {k} outside [1, {num_mic}]: no more sources than microphones")
        return self

    def c_opts(self) -> "_lib.OivaOpts":
        return _lib.OivaOpts(MODELS.index(self.model), int(self.ref_ch), float(self.alpha), float(self.floor), float(self.init))


def bins_per_pass(num_mic: int, num_src: Optional[int] = None) -> int:
    """the bins of an item that one workgroup of the online kernel covers at once (``misonet_oiva_bins_per_pass``; with
    ``num_src`` < ``num_mic``, ``misonet_overiva_bins_per_pass``)"""
    if num_src is None or int(num_src) == int(num_mic):
        return int(_lib.lib().misonet_oiva_bins_per_pass(int(num_mic)))
    return int(_lib.lib().misonet_overiva_bins_per_pass(int(num_mic), int(num_src)))


class SeparateStream(OnlineStream):
    """The state of one stream of online AuxIVA, on the device: ``batch`` recordings of ``num_mic`` microphones and
    ``num_bins`` bins.  ``opts``: the fields of :class:`OnlineAuxIVA`.  The state is allocated once; a call allocates only its
    outputs.

    ``num_src`` None or equal to ``num_mic``: the determined case (``misonet_oiva``); the stream returns all M rows, in no
    particular order of the sources.  ``num_src`` = K < M: the overdetermined case (``misonet_overiva``); the
    stream returns exactly K rows, est [B, K, T, F] and images [B, K, M, T, F], and the images no longer add up to the input: the
    background is what is left.  The project's own definition in the OverIVA family; nothing was compared against other
    packages."""

    def __init__(self, num_mic, num_bins=129, batch=1, *, device=None, **opts):
        self.opts = OnlineAuxIVA(**opts).validate(int(num_mic))
        self.num_mic, self.num_bins, self.batch = int(num_mic), int(num_bins), int(batch)
        self.num_src = self.opts.sources(self.num_mic)
        self._over = self.num_src < self.num_mic
        if not 1 <= self.num_bins <= 1025 or self.batch < 1:
            raise ValueError(f"num_bins must be in [1, 1025] and batch positive, got {num_bins}, {batch}")
        self._c = self.opts.c_opts()
        if self._over:
            nbytes = _lib.lib().misonet_overiva_state_bytes(self.batch, self.num_mic, self.num_src, self.num_bins)
        else:
            nbytes = _lib.lib().misonet_oiva_state_bytes(self.batch, self.num_mic, self.num_bins)
        self._alloc(nbytes, device)

    def _reset_call(self):
        """W = I (Ws = [I 0], J = 0), V_k = init I (and C = init I), no frame seen, no flag"""
        if self._over:
            return _lib.lib().misonet_overiva_reset(self.state.data_ptr(), self.batch, self.num_mic, self.num_src, self.num_bins,
                                                    C.byref(self._c), _lib.stream_ptr(self.device))
        return _lib.lib().misonet_oiva_reset(self.state.data_ptr(), self.batch, self.num_mic, self.num_bins, C.byref(self._c),
                                             _lib.stream_ptr(self.device))

    def process_into(self, block: torch.Tensor, est: torch.Tensor, images: Optional[torch.Tensor] = None):
        """block: complex64 [B, M, T, F], est: complex64 [B, K, T, F], images: complex64 [B, K, M, T, F] or None (K = M in the
        determined case), contiguous on the stream's device and not overlapping.  One launch, nothing allocated: the call a HIP
        graph captures."""
        B, M, T, F = block.shape
        self._same_geometry(block.shape)
        img_ptr = images.data_ptr() if images is not None else None
        with torch.cuda.device(self.device):
            if self._over:
                K = self.num_src
                if tuple(est.shape) != (B, K, T, F) or (images is not None and tuple(images.shape) != (B, K, M, T, F)):
                    raise ValueError(f"est must be [{B}, {K}, {T}, {F}] and images [{B}, {K}, {M}, {T}, {F}]")
                _lib.check(_lib.lib().misonet_overiva(block.data_ptr(), B, M, K, T, F, C.byref(self._c), est.data_ptr(), img_ptr,
                                                      self.state.data_ptr(), self.state.numel(), _lib.stream_ptr(self.device)))
            else:
                _lib.check(_lib.lib().misonet_oiva(block.data_ptr(), B, M, T, F, C.byref(self._c), est.data_ptr(), img_ptr,
                                                   self.state.data_ptr(), self.state.numel(), _lib.stream_ptr(self.device)))
        return est if images is None else (est, images)

    def process(self, block, images=False):
        """The next T >= 1 frames of the stream: complex [B, M, T, F] -> est complex64 [B, K, T, F] (row k at ``ref_ch``), with
        ``images=True`` also the images complex64 [B, K, M, T, F] (K = M in the determined case); on the device for device input
        and on the CPU for an ndarray.  The bits do not depend on how the stream is cut into calls."""
        shape = np.shape(block)
        self._check_block(shape)
        x, np_in = _dev_c64(block, self.device)
        K = self.num_src
        est = torch.empty((shape[0], K) + tuple(x.shape[2:]), dtype=torch.complex64, device=x.device) if self._over \
            else torch.empty_like(x)
        img = torch.empty((shape[0], K) + tuple(x.shape[1:]), dtype=torch.complex64, device=x.device) if images else None
        self.process_into(x, est, img)
        if np_in:
            est, img = est.cpu(), (img.cpu() if images else None)
        return (est, img) if images else est

    def _parts(self):
        B, M, K, F = self.batch, self.num_mic, self.num_src, self.num_bins
        if self._over:
            return dict(Ws=((B, F, K, M), torch.complex128), J=((B, F, M - K, K), torch.complex128),
                        V=((B, F, K, M, M), torch.complex128), C=((B, F, M, M), torch.complex128), fail=((B, F), torch.int32),
                        n=((B, F), torch.int32))
        return dict(W=((B, F, M, M), torch.complex128), V=((B, F, M, M, M), torch.complex128), fail=((B, F), torch.int32),
                    n=((B, F), torch.int32))

    def _debug_call(self, ptr):
        if self._over:
            return _lib.lib().misonet_overiva_debug(self.state.data_ptr(), self.batch, self.num_mic, self.num_src, self.num_bins,
                                                    ptr("Ws"), ptr("J"), ptr("V"), ptr("C"), ptr("fail"), ptr("n"),
                                                    _lib.stream_ptr(self.device))
        return _lib.lib().misonet_oiva_debug(self.state.data_ptr(), self.batch, self.num_mic, self.num_bins, ptr("W"), ptr("V"),
                                             ptr("fail"), ptr("n"), _lib.stream_ptr(self.device))

    def demixing(self):
        """the demixing matrices as they stand (row k = w_k^H), on the device: W complex128 [B, F, M, M], or with K < M sources
        Ws complex128 [B, F, K, M]"""
        return self._debug(("Ws",))["Ws"] if self._over else self._debug(("W",))["W"]

    def covariance(self):
        """the weighted covariances V complex128 [B, F, K, M, M] as they stand (K = M in the determined case), on the device"""
        return self._debug(("V",))["V"]

    def _only_over(self, what):
        if not self._over:
            raise ValueError(f"{what} belongs to the overdetermined stream: set num_src below the number of microphones")

    def background(self):
        """J complex128 [B, F, M - K, K] as it stands, on the device: the rows [J, -I] of the full demixing matrix, which keep
        the background uncorrelated with the sources under the mixture covariance (K < M only)"""
        self._only_over("background()")
        return self._debug(("J",))["J"]

    def mixture_covariance(self):
        """the recursive mixture covariance C complex128 [B, F, M, M] as it stands, on the device (K < M only)"""
        self._only_over("mixture_covariance()")
        return self._debug(("C",))["C"]

    fail = property(OnlineStream.fail.fget, doc="int32 [B, F] on the device: bit 0 a non-finite sample, bit 1 a row update that "
                                                "was dropped, bit 2 a singular W (with K < M: a singular Ws[:, :K] + Ws[:, K:] "
                                                "J), bit 3 (K < M only) a re-solve of J that was dropped")


def auxiva_online(mix, *, return_debug=False, images=False, device=None, **opts):
    """Online AuxIVA of a batch of spectrograms in one call: reset, then process.  mix complex [B, M, T, F], any T >= 1 -> est
    complex64 of the same shape (with ``images=True``: ``(est, images [B, M, M, T, F])``), on the device for device input and on
    the CPU for an ndarray.  ``opts``: the fields of :class:`OnlineAuxIVA`.  ``return_debug`` adds, on the device, ``W``, ``V``,
    ``fail`` and ``n`` of the final state.  Causal: frame t of the output depends on no later frame.  It does not separate better
    than :func:`auxiva`.  With ``num_src=K`` below M: est [B, K, T, F], images [B, K, M, T, F], and the debug parts ``Ws``,
    ``J``, ``V``, ``C``, ``fail`` and ``n`` (:class:`SeparateStream`)."""
    shape = np.shape(mix)
    o = OnlineAuxIVA(**opts).validate(shape[1] if len(shape) == 4 else None)
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f"mix {tuple(shape)} must be [B, M, T, F], all positive")
    st = SeparateStream(shape[1], shape[3], shape[0], device=default_device(mix, device), **o.as_kwargs())
    out = st.process(mix, images=images)
    if not return_debug:
        return out
    return (out + (st._debug(),)) if images else (out, st._debug())


def resident_frames(channels: int) -> int:
    """the largest T at which the steering kernel keeps a bin's Y in registers (``misonet_auxiva_resident_frames``)"""
    return int(_lib.lib().misonet_auxiva_resident_frames(int(channels)))


def auxiva(mix, num_spks, iterations=20, model="gauss", channels=None, floor=1e-10, ref_ch=0, device=None, return_order=False,
           return_debug=False, *, blind=None):
    """AuxIVA-ISS.  mix complex [B, F, M, T] (the beamformers' layout) -> the source images complex64 [B, S, F, M, T]:
    ``images[:, s]`` is a ``source_stft`` of ``Apply_Beamforming``, the whole tensor the ``est`` of ``Apply_Beamforming_Joint``
    and of ``masks_from_estimates``.  With ``return_order`` also the chosen rows int32 [B, S]; with ``return_debug`` also a dict
    of device tensors: ``Y`` complex128 [B, F, K, T], ``A`` and ``evec`` complex128 [B, F, M, K], ``power`` float64 [B, K] and
    ``fail`` int32 [B, F] (bit 0: a non-finite input sample, the bin was taken as zero; bit 1: a non-finite step was dropped).
    The results are on the CPU when ``mix`` was an ndarray, on the device otherwise.  The options are the fields of
    :class:`AuxIVA` (``blind``: a whole AuxIVA or dict, which wins)."""
    opt = (AuxIVA(iterations=iterations, model=model, channels=channels, floor=floor, ref_ch=ref_ch) if blind is None
           else AuxIVA.of(blind))
    if np.ndim(mix) != 4:
        raise ValueError(f"mix {tuple(np.shape(mix))} must be [B, F, M, T]")
    B, F, M, T = np.shape(mix)
    Sn = num_spks
    if isinstance(Sn, bool) or not isinstance(Sn, (int, np.integer)):
        raise ValueError(f"num_spks must be an integer, got {Sn!r}")
    Sn = int(Sn)
    opt.validate(M, Sn)                                                      # before any copy or launch
    if T < 1 or B < 1 or F < 1:
        raise ValueError("B, F and T must be positive")
    K = opt.num_channels(Sn)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    y, np_in = _dev_c64(mix, device)
    L = _lib.lib()
    opts = opt.c_opts()
    nws = L.misonet_auxiva_workspace_bytes(B, Sn, K, F, M, T)
    if nws < 0:
        _lib.check(_lib.EINVAL)
    ws = torch.empty(max(int(nws), 8), dtype=torch.uint8, device=y.device)
    images = torch.empty((B, Sn, F, M, T), dtype=torch.complex64, device=y.device)
    order = torch.empty((B, Sn), dtype=torch.int32, device=y.device) if return_order else None
    dbg = None
    with torch.cuda.device(y.device):
        st = _lib.stream_ptr(y.device)
        _lib.check(L.misonet_auxiva(y.data_ptr(), B, Sn, F, M, T, C.byref(opts), images.data_ptr(),
                                    order.data_ptr() if return_order else None, ws.data_ptr(), ws.numel(), st))
        if return_debug:
            dbg = dict(Y=torch.empty((B, F, K, T), dtype=torch.complex128, device=y.device),
                       A=torch.empty((B, F, M, K), dtype=torch.complex128, device=y.device),
                       evec=torch.empty((B, F, M, K), dtype=torch.complex128, device=y.device),
                       power=torch.empty((B, K), dtype=torch.float64, device=y.device),
                       fail=torch.empty((B, F), dtype=torch.int32, device=y.device))
            _lib.check(L.misonet_auxiva_debug(ws.data_ptr(), B, K, F, M, T, dbg["Y"].data_ptr(), dbg["A"].data_ptr(),
                                              dbg["evec"].data_ptr(), dbg["power"].data_ptr(), dbg["fail"].data_ptr(), st))
    if np_in:
        images = images.cpu()
        order = order.cpu() if order is not None else None
    res = [images] + ([order] if return_order else []) + ([dbg] if return_debug else [])
    return res[0] if len(res) == 1 else tuple(res)


class BlindSeparator:
    """The recording-level composition behind a blind front end: AuxIVA -> (guided cACGMM) -> beamformer -> iSTFT -> files.  It
    uses no networks and no pipeline handle; every stage is the drop-in entry point of its module.

    ``blind``: None (the defaults), an :class:`AuxIVA`, a model name or a dict of its fields (its ``ref_ch`` is replaced by this
    object's); ``beamformer``: None (the reference's MVDR), a :class:`misonet_amd.beamform.Beamformer`, a kind name or a dict of
    its fields, or a :class:`misonet_amd.beamform.JointBeamformer` instance; ``refine``: None (off), True, a
    :class:`misonet_amd.refine.Refine`, a prior name or a dict of its fields."""

    def __init__(self, num_spks: int = 2, num_ch: int = 6, ref_ch: int = 0, blind=None, beamformer=None, refine=None,
                 device=None):
        from .pipeline import Enhancer
        from .refine import Refine
        self.num_spks, self.num_ch, self.ref_ch = int(num_spks), int(num_ch), int(ref_ch)
        self.blind = dataclasses.replace(AuxIVA.of(blind), ref_ch=self.ref_ch).validate(self.num_ch, self.num_spks)
        if isinstance(beamformer, JointBeamformer):
            self.beamformer = beamformer.validate(self.num_ch, self.num_spks)
        else:
            self.beamformer = Beamformer.of(beamformer).validate(self.num_ch)
        self.refine = None if refine is None or refine is False else Refine.of(refine).validate(self.num_ch, self.num_spks)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # the microphone selection and the writers of the recording paths, as they are (pipeline.py): they read num_ch,
        # num_spks, ref_ch and device of the object they are called on and nothing else
        self._select_mics = Enhancer._select_mics.__get__(self)
        self._write_speakers = Enhancer._write_speakers.__get__(self)
        self._srmr_of = Enhancer._srmr_of.__get__(self)

    def _images(self, mix_bf):
        """mix complex64 [B, F, M, T] on the device -> images complex64 [B, S, F, M, T]"""
        return auxiva(mix_bf, self.num_spks, blind=self.blind)

    def _beamform(self, est, mix_bf):
        """est [B, S, F, M, T], mix [B, F, M, T] -> [B, S, T, F]: the optional clustering, then the beamformer"""
        from .beamform import Apply_Beamforming, Apply_Beamforming_Joint
        from .refine import refined_images
        if self.refine is not None:
            est = refined_images(est, mix_bf, self.refine)
        if isinstance(self.beamformer, JointBeamformer):                     # one joint solve for all speakers
            return Apply_Beamforming_Joint(est, mix_bf, self.beamformer)
        return torch.stack([Apply_Beamforming(est[:, s], mix_bf, beamformer=self.beamformer)
                            for s in range(self.num_spks)], dim=1)

    def _mix(self, mix):
        if not isinstance(mix, torch.Tensor) or mix.dim() != 4 or not mix.is_complex():
            raise ValueError("mix must be a 4-D complex tensor [B, M, T, F]")
        if mix.shape[1] != self.num_ch:
            raise ValueError(f"expected {self.num_ch} microphones, got {mix.shape[1]}")
        return mix.to(self.device).to(torch.complex64).permute(0, 3, 1, 2).contiguous()          # [B, F, M, T]

    def separate(self, mix: torch.Tensor) -> torch.Tensor:
        """mix complex [B, M, T, F] -> the source images complex64 [B, S, M, T, F], the layout of ``Enhancer.separate``"""
        return self._images(self._mix(mix)).permute(0, 1, 3, 4, 2)

    def beamform_chunks(self, mix: torch.Tensor) -> torch.Tensor:
        """mix complex [B, M, T, F] -> beamformer outputs complex64 [B, S, T, F]: the composition of
        ``Enhancer.beamform_chunks`` with AuxIVA in the place of MISO1 (every item of the batch separated on its own)"""
        mix_bf = self._mix(mix)
        return self._beamform(self._images(mix_bf), mix_bf)

    def _online_pick(self, est):
        """est [M, Tt, F] -> the indices of the num_spks rows of largest sum |est|^2, descending, ties to the lower index"""
        power = (est.real.double() ** 2 + est.imag.double() ** 2).sum(dim=(1, 2))                # [M]
        return torch.sort(power, descending=True, stable=True).indices[:self.num_spks]

    def _online_rows(self, spec, online, dereverb, beamform=None):
        """spec complex64 [1, M, Tt, F] on the device -> the num_spks strongest rows of the online separation [S, Tt, F]; with
        ``beamform`` (an OnlineBeamformer) the rows of the online beamformer at the same indices"""
        M = spec.shape[1]
        online.validate(M)
        K = online.sources(M)                                                # the rows the stream returns
        if beamform is not None:
            beamform.validate(M, K)
        if self.num_spks > K:
            raise ValueError(f"online separation returns {K} rows; {self.num_spks} speakers were asked for"
                             + ("" if online.num_src is None else f" (num_src must be >= num_spks)"))
        # num_src == num_spks: every row is a speaker and nothing is chosen; without num_src the rows are ordered as they always were
        pick = online.num_src is None or K > self.num_spks
        if dereverb is not None:
            from .dereverb import DereverbStream
            spec = DereverbStream(M, spec.shape[3], 1, device=self.device, **dataclasses.asdict(dereverb.validate(M))).process(spec)
        sep = SeparateStream(M, spec.shape[3], 1, device=self.device, **online.as_kwargs())
        if beamform is None:
            est = sep.process(spec)[0]
            return est[self._online_pick(est)].contiguous() if pick else est
        from .beamform import BeamformStream
        est, images = sep.process(spec, images=True)
        out = BeamformStream(M, K, spec.shape[3], 1, device=self.device, **dataclasses.asdict(beamform)).process(images, spec)
        return out[0][self._online_pick(est[0])].contiguous() if pick else out[0]

    def separate_recording(self, wav, num_ch_utilize: Optional[int] = None, save_path: Optional[str] = None, fs: int = 16000,
                           beamform: Optional[bool] = None, srmr: bool = False, fs_in=None, fs_out=None, online=None,
                           dereverb=None):
        """Recording in -> separated int16 waves out.  wav float32 [L, M_all] (time-major, as ``read_wav`` returns it) ->
        int16 [S, L] (an ndarray).  The microphone selection of ``Enhancer.enhance_recording`` (``[0:M:M // num_ch_utilize]``),
        ONE STFT over the recording zero-padded to whole hops, ONE AuxIVA over all its frames, then the optional clustering
        and the beamformer -- or, with ``beamform=False``, the image at ``ref_ch`` -- the iSTFT, x 32767 -> int16, trimmed to
        ``L``.  ``save_path`` = "<dir>/<name>" also writes ``<save_path>_{s}.wav`` as 24-bit PCM, the files
        ``tools/score_eval.py`` reads.  ``srmr=True`` returns ``(pcm, Srmr)``, as ``enhance_recording``.  ``fs_in`` / ``fs_out``: a
        recording at another rate than the separation's ``fs``, as ``enhance_recording`` takes them; both
        None adds nothing to the call.

        ``online``: None -- the offline path above, bit for bit; True, an :class:`OnlineAuxIVA`, a model name or
        a dict of its fields (its ``ref_ch`` is replaced by this object's) -- ONE STFT, optionally a
        :class:`misonet_amd.dereverb.DereverbStream` over the frames (``dereverb``: None, True, an
        :class:`misonet_amd.dereverb.OnlineDereverb` or a dict of its fields), a :class:`SeparateStream` over the frames with all
        the selected microphones as sources, then the ``num_spks`` rows of largest sum |est|^2 over the recording, descending, ties
        to the lower index, the iSTFT and the int16 waves as above.  That row selection is made on the device with torch after the
        whole recording has been seen: it is NOT causal -- the stream itself returns all M rows and leaves the choice to its
        caller.  ``beamform``: None is True on the offline path, as it always was, and False with ``online``; ``beamform=True`` with
        ``online`` is refused: the beamformers here are block algorithms.  ``beamform=`` a
        :class:`misonet_amd.beamform.OnlineBeamformer` instance (only an instance selects it, and its ``ref_ch``
        is replaced by this object's) adds the one beamformer that is not: the :class:`SeparateStream` also returns its images, a
        :class:`misonet_amd.beamform.BeamformStream` with M sources runs on those images and on the spectrum AuxIVA saw (behind
        ``dereverb``: the dereverberated one), the rows are chosen as above, by the power of ``est``, and the beamformed rows of
        those indices go to the iSTFT.  An ``OnlineBeamformer`` without ``online`` is refused; so is ``dereverb`` without
        ``online``.

        ``online`` with ``num_src`` = K set: K < M runs the overdetermined stream, which returns exactly K
        rows (the online beamformer behind it is a ``BeamformStream(M, K)``); K >= ``num_spks`` is required.  With K > ``num_spks``
        the strongest ``num_spks`` rows are chosen as above, after the fact.  With K == ``num_spks`` every row of the stream is a
        speaker and the path makes no choice after the whole recording has been seen: that is what makes it causal -- frame t of
        every wave depends on no later frame."""
        from .beamform import OnlineBeamformer
        online_bf = None
        if isinstance(beamform, OnlineBeamformer):
            if online is None or online is False:
                raise ValueError("beamform=OnlineBeamformer(...) belongs to the online path: set online= as well")
            online_bf, beamform = dataclasses.replace(beamform, ref_ch=self.ref_ch).validate(), None
        if online is None or online is False:
            if dereverb is not None:
                raise ValueError("dereverb= belongs to the online path: set online= as well, or dereverberate with dereverb_wav first")
            online = None
            beamform = True if beamform is None else beamform
        else:
            if beamform:
                raise ValueError("online= with beamform=True: the beamformers here are block algorithms; pass beamform=False")
            beamform = False
            online = dataclasses.replace(OnlineAuxIVA.of(online), ref_ch=self.ref_ch)
            if dereverb is not None:
                from .dereverb import OnlineDereverb
                dereverb = OnlineDereverb.of(dereverb)
        if fs_in is not None or fs_out is not None:
            from . import resample as RS
            RS.plan_rates(fs, fs_in, fs_out)                                 # a bad rate: before anything else
            if srmr:
                from . import score as SC
                SC.check_srmr_fs(fs)
            return RS.around(lambda w, _c, path: self.separate_recording(w, num_ch_utilize, path, fs,
                                                                         beamform if online_bf is None else online_bf, srmr,
                                                                         online=online, dereverb=dereverb),
                             wav, None, fs, fs_in, fs_out, save_path, self._write_speakers, self.device)
        if srmr:
            from . import score as SC
            SC.check_srmr_fs(fs)
        mics, obs = self._select_mics(wav, num_ch_utilize)
        L = obs.shape[0]
        sig = torch.from_numpy(np.ascontiguousarray(obs[:, mics])).to(self.device)               # [L, M]
        sig = torch.nn.functional.pad(sig, (0, 0, 0, (-L) % S.HOP))[None].contiguous()           # [1, Lp, M]
        if online is not None:
            out = self._online_rows(S.stft_hip(sig), online, dereverb, online_bf)                # [S, Tt, F]
            pcm = np.ascontiguousarray(S.istft_int16(out)[:, :L].cpu().numpy())
            if save_path is not None:
                self._write_speakers(pcm, save_path, fs)
            return (pcm, self._srmr_of(pcm, wav, num_ch_utilize, fs)) if srmr else pcm
        mix_bf = S.stft_hip(sig)[0].permute(2, 0, 1)[None].contiguous()                          # [1, F, M, Tt]
        est = self._images(mix_bf)                                                               # [1, S, F, M, Tt]
        if beamform:
            out = self._beamform(est, mix_bf)[0]                                                 # [S, Tt, F]
        else:
            out = est[0, :, :, self.ref_ch, :].permute(0, 2, 1)
        pcm = np.ascontiguousarray(S.istft_int16(out.contiguous())[:, :L].cpu().numpy())
        if save_path is not None:
            self._write_speakers(pcm, save_path, fs)
        return (pcm, self._srmr_of(pcm, wav, num_ch_utilize, fs)) if srmr else pcm
