"""Host-side mirror of the reference's array-processing calls on the inference path.

``Apply_Beamforming(source_stft, mix_stft, epsi)``  -- reference tester.py:1071-1136 (MVDR per frequency bin); keywords
                                                       select the other beamformers (:class:`Beamformer`), among them the
                                                       WPD convolutional beamformer (``beamformer="wpd"``: misonet_wpd)
``pit_select(anchor, cand)``                        -- reference tester.py:1043-1065 / 889-915 (PIT over all S! permutations)

``Apply_Beamforming_Joint(sources_stft, mix_stft)``  -- the joint multi-speaker beamformers (:class:`JointBeamformer`: LCMV,
                                                       SDW-MWF, rank-1 MWF): all speakers of a bin in one solve

``BeamformStream`` / ``beamform_online``             -- the online beamformer (:class:`OnlineBeamformer`: the frame-recursive Souden
                                                       MVDR / rank-1 MWF of INTEGRATION.md 4t, its state carried from call to
                                                       call; csrc/obf.hip, C ABI ``misonet_obf``)

All run as HIP kernels through the C ABI (misonet_beamform / misonet_beamform_joint / misonet_pit_select / misonet_obf in
include/misonet.h).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._online import OnlineStream, check_index, check_real, default_device, spec_of
from ._online import _dev_c64                   # also under this module's name: tests and tools import it from here


KINDS = ("mvdr", "souden", "gev")            # the kinds of misonet_bf_opts, in its numbering
WPD = "wpd"                                  # the convolutional beamformer has options and entry points of its own (ABI 530)
WPD_KMAX = 88                                # the largest order M (taps + 1) the kernel takes (include/misonet.h, "WPD")
NOISES = ("residual", "mix")
JOINT_KINDS = ("lcmv", "mwf", "r1mwf")       # the kinds of misonet_jbf_opts, in its numbering (ABI 570); "sdw_mwf" is "mwf"
RTFS = ("cw", "eig")


@dataclasses.dataclass(frozen=True)
class Beamformer:
    """One plain-data description of a beamformer (``misonet_bf_opts`` of include/misonet.h), used by every layer.

    kind             "mvdr" (the reference's live path, tester.py:1071-1136), "souden" (w = G[:, ref_ch] / tr G with
                     G = Phi_n'^-1 Phi_s) or "gev" (principal generalised eigenvector of (Phi_s, Phi_n'), w^H Phi_n' w = 1,
                     (Phi_n' w)[ref_ch] real and >= 0 per bin)
    noise            "residual": Phi_n from Y - S (tester.py:1095); "mix": from Y (tester.py:1096, MPDR / "MP-GEV")
    condition        gamma >= 0: Phi_n <- (Phi_n + gamma tr(Phi_n) / M I) / (1 + gamma), per bin
    trace_normalize  Phi_n <- Phi_n / tr(Phi_n) (tester.py:1099), after the conditioning
    epsi             Phi_n' = Phi_n + epsi I, last (tester.py:1221); None = the default of the call that uses the options
    ban              blind analytic normalisation of w (tester.py:1186-1208)
    ref_ch           reference microphone of "souden", "gev" and "wpd"

    kind "wpd" (``misonet_wpd_opts``): the WPD convolutional beamformer, one filter of order M (taps + 1) per bin over the
    current frame and ``taps`` frames that lie ``delay`` and more back, R weighted by the power of the source estimate, the
    Souden solve against the zero-padded Phi_s.  Its fields -- ignored by the other kinds:
    taps, delay      frames of the prediction part and its distance (>= 1 each; M (taps + 1) <= 88)
    diag_load        R += diag_load tr(R) / K I
    power_floor      w[t] = 1 / max(p[t], power_floor max_t p[t])
    It has no noise covariance: ``noise``, ``condition``, ``trace_normalize`` and ``ban`` must keep their defaults; ``epsi`` is
    ignored.
    """
    kind: str = "mvdr"
    noise: str = "residual"
    condition: float = 0.0
    trace_normalize: bool = False
    epsi: Optional[float] = None
    ban: bool = False
    ref_ch: int = 0
    taps: int = 5
    delay: int = 3
    diag_load: float = 0.0
    power_floor: float = 1e-10

    @classmethod
    def of(cls, spec) -> "Beamformer":
        """None (the defaults), a Beamformer, a kind name, or a dict of the fields above"""
        return spec_of(cls, spec, "beamformer", "beamformer must be None, a Beamformer, a kind name or a dict of its fields", "kind",
                       true_ok=False)

    def with_epsi(self, default: float) -> "Beamformer":
        return self if self.epsi is not None else dataclasses.replace(self, epsi=float(default))

    def validate(self, num_mic: Optional[int] = None) -> "Beamformer":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        if self.kind not in KINDS + (WPD,):
            hint = ""
            if self.kind in JOINT_KINDS + ("sdw_mwf",):
                hint = " (a joint kind: JointBeamformer / Apply_Beamforming_Joint take it)"
            raise ValueError(f"beamformer kind {self.kind!r}: one of {KINDS + (WPD,)}{hint}")
        if self.noise not in NOISES:
            raise ValueError(f"beamformer noise {self.noise!r}: one of {NOISES}")
        if not (isinstance(self.condition, (int, float)) and math.isfinite(self.condition) and self.condition >= 0):
            raise ValueError(f"beamformer condition (gamma) must be finite and >= 0, got {self.condition!r}")
        if self.epsi is not None and not (math.isfinite(self.epsi) and self.epsi >= 0):
            raise ValueError(f"beamformer epsi must be finite and >= 0, got {self.epsi!r}")
        if int(self.ref_ch) != self.ref_ch or self.ref_ch < 0 or (num_mic is not None and self.ref_ch >= num_mic):
            raise ValueError(f"beamformer ref_ch {self.ref_ch!r} outside [0, {num_mic if num_mic is not None else 'M'})")
        if self.kind == WPD:
            if self.noise != "residual" or self.condition != 0 or self.trace_normalize or self.ban:
                raise ValueError('beamformer kind "wpd" has no noise covariance: noise, condition, trace_normalize and ban '
                                 "must keep their defaults")
            for name in ("taps", "delay"):
                v = getattr(self, name)
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                    raise ValueError(f"wpd {name} must be an integer >= 1, got {v!r}")
            if num_mic is not None and not 2 <= num_mic <= 8:
                raise ValueError(f"wpd needs 2 <= M <= 8 microphones, got {num_mic}")
            if (num_mic if num_mic is not None else 2) * (self.taps + 1) > WPD_KMAX:
                raise ValueError(f"wpd order M (taps + 1) must be <= {WPD_KMAX}, got taps {self.taps}"
                                 + (f" with M {num_mic}" if num_mic is not None else ""))
            for name in ("diag_load", "power_floor"):
                v = getattr(self, name)
                if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                    raise ValueError(f"wpd {name} must be finite and >= 0, got {v!r}")
        return self

    def c_opts(self, epsi_default: float = 1e-6) -> "_lib.BfOpts":
        if self.kind == WPD:
            raise ValueError('kind "wpd" is not a misonet_bf_opts kind: use wpd_opts()')
        return _lib.BfOpts(KINDS.index(self.kind), NOISES.index(self.noise), float(self.condition),
                           int(bool(self.trace_normalize)), float(self.epsi if self.epsi is not None else epsi_default),
                           int(bool(self.ban)), int(self.ref_ch))

    def wpd_opts(self) -> "_lib.WpdOpts":
        """the fields of kind "wpd" as ``misonet_wpd_opts``"""
        return _lib.WpdOpts(int(self.taps), int(self.delay), float(self.diag_load), float(self.power_floor), int(self.ref_ch))


def _wpd_device(src, mix, bf, return_debug):
    """misonet_wpd on device tensors [B, F, M, T]: (out [B, T, F], None or dict(w [B, F, K], fail [B, F]))"""
    B, F, M, T = src.shape
    if T <= bf.delay + bf.taps - 1:
        raise ValueError(f"wpd needs T > delay + taps - 1 = {bf.delay + bf.taps - 1} frames, got {T}")
    opts = bf.wpd_opts()
    L = _lib.lib()
    nws = L.misonet_wpd_workspace_bytes(B, F, M, C.byref(opts))
    if nws < 0:
        _lib.check(_lib.EINVAL)
    ws = torch.empty(max(int(nws), 8), dtype=torch.uint8, device=src.device)
    out = torch.empty((B, T, F), dtype=torch.complex64, device=src.device)
    dbg = None
    with torch.cuda.device(src.device):
        st = _lib.stream_ptr(src.device)
        _lib.check(L.misonet_wpd(src.data_ptr(), mix.data_ptr(), B, F, M, T, C.byref(opts), out.data_ptr(), ws.data_ptr(),
                                 ws.numel(), st))
        if return_debug:
            w = torch.empty((B, F, M * (bf.taps + 1)), dtype=torch.complex128, device=src.device)
            bad = torch.empty((B, F), dtype=torch.int32, device=src.device)
            _lib.check(L.misonet_wpd_debug(ws.data_ptr(), B, F, M, C.byref(opts), w.data_ptr(), bad.data_ptr(), st))
            dbg = dict(w=w, fail=bad)
    return out, dbg


def Apply_Beamforming(source_stft, mix_stft, epsi=1e-6, device=None, return_debug=False, *, beamformer="mvdr",
                      noise="residual", condition=0.0, trace_normalize=False, ban=False, ref_ch=0, taps=5, delay=3,
                      diag_load=0.0, power_floor=1e-10):
    """Beamforming, same arguments and (with the keyword defaults) same result as Tester_Enhance.Apply_Beamforming
    (tester.py:1071-1136: residual-noise MVDR).

    source_stft, mix_stft: complex [B, F, Ch, T] (np.ndarray as in the reference, or torch tensors; permuted
    views are fine).  Returns a torch complex64 tensor [B, T, F]: on the CPU when the inputs were ndarrays (the
    reference returns torch.from_numpy(...)), on the device when they were device tensors.  Inputs are not modified.

    The keywords are the fields of :class:`Beamformer` (``beamformer`` = its ``kind``, or a whole Beamformer / dict, whose
    ``epsi``, when set, wins over the positional one).  ``return_debug`` adds what the kind has, complex128 / float64 on
    the device: "mvdr" ``steer1`` and ``w`` [B, F, Ch]; "souden" ``w``; "gev" ``w`` and ``lam`` [B, F] (lambda_max);
    "wpd" ``w`` [B, F, Ch (taps + 1)] (the weights on the current frame first) and ``fail`` int32 [B, F].
    ``beamformer="wpd"`` (``taps``, ``delay``, ``diag_load``, ``power_floor``, ``ref_ch``) is the WPD convolutional
    beamformer (``misonet_wpd``); it needs T > delay + taps - 1 frames.
    """
    if isinstance(beamformer, str):
        bf = Beamformer(kind=beamformer, noise=noise, condition=condition, trace_normalize=trace_normalize, epsi=epsi,
                        ban=ban, ref_ch=ref_ch, taps=taps, delay=delay, diag_load=diag_load, power_floor=power_floor)
    else:
        bf = Beamformer.of(beamformer).with_epsi(epsi)
    bf.validate(np.shape(source_stft)[2] if np.ndim(source_stft) == 4 else None)     # before any copy or launch
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    src, np_in = _dev_c64(source_stft, device)
    mix, _ = _dev_c64(mix_stft, device)
    if src.shape != mix.shape or src.dim() != 4:
        raise ValueError(f"source_stft {tuple(src.shape)} and mix_stft {tuple(mix.shape)} must both be [B, F, Ch, T]")
    B, F, M, T = src.shape
    if bf.kind == WPD:
        out, dbg = _wpd_device(src, mix, bf, return_debug)
        if np_in:
            out = out.cpu()
        return (out, dbg) if return_debug else out
    opts = bf.c_opts()
    L = _lib.lib()
    nws = L.misonet_beamform_workspace_bytes(B, F, M, C.byref(opts))
    if nws < 0:
        _lib.check(_lib.EINVAL)
    ws = torch.empty(max(int(nws), 8), dtype=torch.uint8, device=src.device)
    out = torch.empty((B, T, F), dtype=torch.complex64, device=src.device)
    with torch.cuda.device(src.device):
        st = _lib.stream_ptr(src.device)
        _lib.check(L.misonet_beamform(src.data_ptr(), mix.data_ptr(), B, F, M, T, C.byref(opts), out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), st))
        dbg = None
        if return_debug:
            w = torch.empty((B, F, M), dtype=torch.complex128, device=src.device)
            dbg = dict(w=w)
            if bf.kind == "mvdr":
                steer = torch.empty((B, F, M), dtype=torch.complex128, device=src.device)
                _lib.check(L.misonet_mvdr_debug(ws.data_ptr(), B, F, M, steer.data_ptr(), w.data_ptr(), st))
                dbg = dict(steer1=steer, w=w)
            else:
                lam = torch.empty((B, F), dtype=torch.float64, device=src.device) if bf.kind == "gev" else None
                _lib.check(L.misonet_beamform_debug(ws.data_ptr(), B, F, M, C.byref(opts), w.data_ptr(),
                                                    lam.data_ptr() if lam is not None else None, st))
                if lam is not None:
                    dbg["lam"] = lam
    if np_in:
        out = out.cpu()
    return (out, dbg) if return_debug else out


@dataclasses.dataclass(frozen=True)
class JointBeamformer:
    """The options of the joint multi-speaker beamformers (``misonet_jbf_opts`` of include/misonet.h): one
    solve per bin for ALL speakers, from their estimates and the mixture.  Deliberately not a :class:`Beamformer` kind: a kind
    name or a dict still means Beamformer everywhere; the joint kinds are selected with an instance of this class.

    kind       "lcmv" (unit gain on the target's relative transfer function, a null on every other speaker's), "mwf" (the
               speech-distortion-weighted multichannel Wiener filter; "sdw_mwf" is accepted as its name) or "r1mwf" (rank-1 MWF)
    noise      "residual": Phi_v from Y - sum_s X_s; "mix": from Y (lcmv only: power minimisation, "LCMP")
    rtf        "cw": relative transfer functions by covariance whitening; "eig": the principal eigenvector of Phi_s (lcmv only)
    mu         the speech-distortion weight: > 0 for "mwf" (1 = the MWF), >= 0 for "r1mwf" (0 = Souden MVDR on the sum-of-sources
               model); ignored by "lcmv"
    diag_load  R = Phi_v + diag_load tr(Phi_v) / M I
    ref_ch     reference microphone
    """
    kind: str = "lcmv"
    noise: str = "residual"
    rtf: str = "cw"
    mu: float = 1.0
    diag_load: float = 0.0
    ref_ch: int = 0

    def __post_init__(self):
        if self.kind == "sdw_mwf":
            object.__setattr__(self, "kind", "mwf")

    @classmethod
    def of(cls, spec) -> "JointBeamformer":
        """None (the defaults), a JointBeamformer, a kind name, or a dict of the fields above"""
        return spec_of(cls, spec, "joint beamformer",
                       "joint beamformer must be None, a JointBeamformer, a kind name or a dict of its fields", "kind", true_ok=False)

    def validate(self, num_mic: Optional[int] = None, num_spks: Optional[int] = None) -> "JointBeamformer":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        if self.kind not in JOINT_KINDS:
            raise ValueError(f"joint beamformer kind {self.kind!r}: one of {JOINT_KINDS}")
        if self.noise not in NOISES:
            raise ValueError(f"joint beamformer noise {self.noise!r}: one of {NOISES}")
        if self.rtf not in RTFS:
            raise ValueError(f"joint beamformer rtf {self.rtf!r}: one of {RTFS}")
        if self.kind != "lcmv" and (self.noise != "residual" or self.rtf != "cw"):
            raise ValueError(f'noise "mix" and rtf belong to kind "lcmv": they must keep their defaults for kind {self.kind!r}')
        for name in ("diag_load",) if self.kind == "lcmv" else ("mu", "diag_load"):      # mu is ignored by "lcmv"
            v = getattr(self, name)
            if isinstance(v, bool) or not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f"joint beamformer {name} must be finite and >= 0, got {v!r}")
        if self.kind == "mwf" and not self.mu > 0:
            raise ValueError(f'joint beamformer mu must be > 0 for kind "mwf", got {self.mu!r}')
        if int(self.ref_ch) != self.ref_ch or self.ref_ch < 0 or (num_mic is not None and self.ref_ch >= num_mic):
            raise ValueError(f"joint beamformer ref_ch {self.ref_ch!r} outside [0, {num_mic if num_mic is not None else 'M'})")
        if num_mic is not None and not 2 <= num_mic <= 8:
            raise ValueError(f"the joint beamformers need 2 <= M <= 8 microphones, got {num_mic}")
        if num_spks is not None and not 1 <= num_spks <= min(4, num_mic if num_mic is not None else 4):
            raise ValueError(f"the joint beamformers need 1 <= S <= 4 speakers and S <= M, got S {num_spks}"
                             + (f" with M {num_mic}" if num_mic is not None else ""))
        return self

    def c_opts(self) -> "_lib.JbfOpts":
        return _lib.JbfOpts(JOINT_KINDS.index(self.kind), NOISES.index(self.noise), RTFS.index(self.rtf), float(self.mu),
                            float(self.diag_load), int(self.ref_ch))


def Apply_Beamforming_Joint(sources_stft, mix_stft, beamformer="lcmv", *, noise="residual", rtf="cw", mu=1.0, diag_load=0.0,
                            ref_ch=0, device=None, return_debug=False):
    """The joint multi-speaker beamformers (``misonet_beamform_joint``): every speaker's filter of a bin from ONE solve that
    knows all of them.

    sources_stft complex [B, S, F, Ch, T] (the S source estimates at every microphone), mix_stft complex [B, F, Ch, T];
    np.ndarray or torch tensors, as :func:`Apply_Beamforming` takes them (permuted views are fine, nothing is modified).
    Returns a torch complex64 tensor [B, S, T, F]: on the CPU when the inputs were ndarrays, on the device when they were
    device tensors.  The keywords are the fields of :class:`JointBeamformer` (``beamformer`` = its ``kind``, or a whole
    JointBeamformer / dict).  ``return_debug`` adds, on the device, ``w`` complex128 [B, S, F, Ch], ``fail`` int32 [B, S, F]
    and, for "lcmv", ``rtf`` complex128 [B, S, F, Ch] (the relative transfer functions d_s)."""
    if isinstance(beamformer, str):
        bf = JointBeamformer(kind=beamformer, noise=noise, rtf=rtf, mu=mu, diag_load=diag_load, ref_ch=ref_ch)
    else:
        bf = JointBeamformer.of(beamformer)
    five = np.ndim(sources_stft) == 5
    bf.validate(np.shape(sources_stft)[3] if five else None, np.shape(sources_stft)[1] if five else None)   # before any copy
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    src, np_in = _dev_c64(sources_stft, device)
    mix, _ = _dev_c64(mix_stft, device)
    if src.dim() != 5 or mix.dim() != 4 or src.shape[:1] + src.shape[2:] != mix.shape:
        raise ValueError(f"sources_stft {tuple(src.shape)} must be [B, S, F, Ch, T] and mix_stft {tuple(mix.shape)} [B, F, Ch, T]")
    B, S, F, M, T = src.shape
    opts = bf.c_opts()
    L = _lib.lib()
    nws = L.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(opts))
    if nws < 0:
        _lib.check(_lib.EINVAL)
    ws = torch.empty(max(int(nws), 8), dtype=torch.uint8, device=src.device)
    out = torch.empty((B, S, T, F), dtype=torch.complex64, device=src.device)
    dbg = None
    with torch.cuda.device(src.device):
        st = _lib.stream_ptr(src.device)
        _lib.check(L.misonet_beamform_joint(src.data_ptr(), mix.data_ptr(), B, S, F, M, T, C.byref(opts), out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), st))
        if return_debug:
            w = torch.empty((B, S, F, M), dtype=torch.complex128, device=src.device)
            bad = torch.empty((B, S, F), dtype=torch.int32, device=src.device)
            d = torch.empty_like(w) if bf.kind == "lcmv" else None
            _lib.check(L.misonet_beamform_joint_debug(ws.data_ptr(), B, S, F, M, C.byref(opts), w.data_ptr(),
                                                      d.data_ptr() if d is not None else None, bad.data_ptr(), st))
            dbg = dict(w=w, fail=bad)
            if d is not None:
                dbg["rtf"] = d
    if np_in:
        out = out.cpu()
    return (out, dbg) if return_debug else out


@dataclasses.dataclass(frozen=True)
class OnlineBeamformer:
    """One plain-data description of the online beamformer (``misonet_obf_opts`` of include/misonet.h).

    noise      "residual": Phi_n from y - x; "mix": from y (MPDR).  0 and 1 are taken as well
    ref_ch     the reference microphone
    alpha      forgetting factor of Phi_s and Phi_n, 0 < alpha < 1 (1 would freeze them)
    mu         0: the Souden MVDR, w = G[:, ref_ch] / tr G; > 0: the rank-1 / speech-distortion-weighted MWF, / (mu + tr G)
    diag_load  R = Phi_n + (diag_load tr(Phi_n) / M + epsi) I
    epsi
    init       Phi_n = init I at reset
    The defaults are choices, not tuned values.
    """
    noise: object = "residual"
    ref_ch: int = 0
    alpha: float = 0.98
    mu: float = 0.0
    diag_load: float = 1e-3
    epsi: float = 1e-10
    init: float = 1.0

    @classmethod
    def of(cls, spec) -> "OnlineBeamformer":
        """None or True (the defaults), an OnlineBeamformer, a noise name, or a dict of the fields above"""
        return spec_of(cls, spec, "online beamformer",
                       "an online beamformer must be None, True, an OnlineBeamformer, a noise name or a dict of its fields", "noise")

    @property
    def noise_index(self) -> int:
        n = self.noise
        if isinstance(n, str) and n in NOISES:
            return NOISES.index(n)
        if not isinstance(n, bool) and isinstance(n, (int, np.integer)) and 0 <= n < len(NOISES):
            return int(n)
        raise ValueError(f"online beamformer noise {n!r}: one of {NOISES} (or 0, 1)")

    def validate(self, num_mic: Optional[int] = None, num_src: Optional[int] = None) -> "OnlineBeamformer":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        self.noise_index
        a = self.alpha
        if isinstance(a, bool) or not isinstance(a, (int, float, np.floating)) or not 0 < a < 1:
            raise ValueError(f"online beamformer alpha must be in (0, 1), got {a!r}")
        for name in ("mu", "diag_load", "epsi", "init"):
            check_real("online beamformer", name, getattr(self, name), positive=False)
        r = self.ref_ch
        check_index("online beamformer", "ref_ch", r)
        if num_mic is not None:
            if not 2 <= num_mic <= 8:
                raise ValueError(f"the online beamformer needs 2 <= M <= 8 microphones, got {num_mic}")
            if r >= num_mic:
                raise ValueError(f"online beamformer ref_ch {r} outside [0, {num_mic})")
        if num_src is not None and not 1 <= num_src <= 8:
            raise ValueError(f"the online beamformer takes 1 <= S <= 8 sources, got {num_src}")
        return self

    def c_opts(self) -> "_lib.ObfOpts":
        return _lib.ObfOpts(self.noise_index, int(self.ref_ch), float(self.alpha), float(self.mu), float(self.diag_load),
                            float(self.epsi), float(self.init))


def cells_per_block(num_mic: int) -> int:
    """the cells (item, source, bin) one workgroup of the online beamformer covers (``misonet_obf_cells_per_block``)"""
    return int(_lib.lib().misonet_obf_cells_per_block(int(num_mic)))


class BeamformStream(OnlineStream):
    """The state of one stream of the online beamformer, on the device: ``batch`` recordings of ``num_mic`` microphones,
    ``num_src`` sources and ``num_bins`` bins.  ``opts``: the fields of :class:`OnlineBeamformer`.  The state is allocated once; a
    call allocates only its output."""

    def __init__(self, num_mic, num_src, num_bins=129, batch=1, *, device=None, **opts):
        self.num_mic, self.num_src, self.num_bins, self.batch = int(num_mic), int(num_src), int(num_bins), int(batch)
        self.opts = OnlineBeamformer(**opts).validate(self.num_mic, self.num_src)
        if not 1 <= self.num_bins <= 1025 or self.batch < 1:
            raise ValueError(f"num_bins must be in [1, 1025] and batch positive, got {num_bins}, {batch}")
        self._c = self.opts.c_opts()
        self._alloc(_lib.lib().misonet_obf_state_bytes(self.batch, self.num_src, self.num_mic, self.num_bins), device)

    def _reset_call(self):
        """Phi_s = 0, Phi_n = init I, w = 0, no frame seen, no flag"""
        return _lib.lib().misonet_obf_reset(self.state.data_ptr(), self.batch, self.num_src, self.num_mic, self.num_bins,
                                            C.byref(self._c), _lib.stream_ptr(self.device))

    def _geometry(self, ishape, mshape):
        B, S, M, F = self.batch, self.num_src, self.num_mic, self.num_bins
        if len(ishape) != 5 or len(mshape) != 4 or ishape[3] < 1:
            raise ValueError(f"images {tuple(ishape)} must be [B, S, M, T, F] and mix {tuple(mshape)} [B, M, T, F] with T >= 1")
        T = ishape[3]
        if tuple(ishape) != (B, S, M, T, F) or tuple(mshape) != (B, M, T, F):
            raise ValueError(f"images {tuple(ishape)} must be [{B}, {S}, {M}, T, {F}] and mix {tuple(mshape)} [{B}, {M}, T, {F}]")
        return T

    def process_into(self, images: torch.Tensor, mix: torch.Tensor, out: torch.Tensor):
        """images complex64 [B, S, M, T, F], mix complex64 [B, M, T, F], out complex64 [B, S, T, F], contiguous on the stream's
        device and not overlapping.  One launch, nothing allocated: the call a HIP graph captures."""
        T = self._geometry(images.shape, mix.shape)
        B, S, M, F = self.batch, self.num_src, self.num_mic, self.num_bins
        if tuple(out.shape) != (B, S, T, F):
            raise ValueError(f"out {tuple(out.shape)} must be [{B}, {S}, {T}, {F}]")
        for name, t in (("images", images), ("mix", mix), ("out", out)):
            if t.dtype != torch.complex64 or not t.is_contiguous() or t.device != self.state.device:
                raise ValueError(f"{name} must be a contiguous complex64 tensor on {self.state.device}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().misonet_obf(mix.data_ptr(), images.data_ptr(), B, S, M, T, F, C.byref(self._c), out.data_ptr(),
                                              self.state.data_ptr(), self.state.numel(), _lib.stream_ptr(self.device)))
        return out

    def process(self, images, mix):
        """The next T >= 1 frames of the stream: images complex [B, S, M, T, F] (what ``SeparateStream.process(images=True)``
        returns, or ``mask * mix`` formed by the caller) and mix complex [B, M, T, F] -> out complex64 [B, S, T, F]; on the device
        for device input and on the CPU when ``images`` was an ndarray.  The bits do not depend on how the stream is cut into
        calls."""
        self._geometry(np.shape(images), np.shape(mix))
        x, np_in = _dev_c64(images, self.device)
        y, _ = _dev_c64(mix, self.device)
        out = torch.empty((x.shape[0], x.shape[1], x.shape[3], x.shape[4]), dtype=torch.complex64, device=x.device)
        self.process_into(x, y, out)
        return out.cpu() if np_in else out

    def _parts(self):
        B, S, M, F = self.batch, self.num_src, self.num_mic, self.num_bins
        return dict(phi_s=((B, S, F, M, M), torch.complex128), phi_n=((B, S, F, M, M), torch.complex128),
                    w=((B, S, F, M), torch.complex128), fail=((B, S, F), torch.int32), n=((B, S, F), torch.int32))

    def _debug_call(self, ptr):
        return _lib.lib().misonet_obf_debug(self.state.data_ptr(), self.batch, self.num_src, self.num_mic, self.num_bins,
                                            ptr("phi_s"), ptr("phi_n"), ptr("w"), ptr("fail"), ptr("n"), _lib.stream_ptr(self.device))

    def filters(self):
        """the filters w complex128 [B, S, F, M] of the last frame (out = w^H y), on the device"""
        return self._debug(("w",))["w"]

    def covariances(self):
        """(Phi_s, Phi_n), complex128 [B, S, F, M, M] each, as they stand, on the device"""
        d = self._debug(("phi_s", "phi_n"))
        return d["phi_s"], d["phi_n"]

    fail = property(OnlineStream.fail.fget, doc="int32 [B, S, F] on the device: bit 0 a non-finite sample, bit 1 a Cholesky pivot "
                                                "not > 0, bit 2 a non-finite mu + tr G")


def beamform_online(images, mix, *, return_debug=False, device=None, **opts):
    """The online beamformer over a batch of spectrograms in one call: reset, then process.  images complex [B, S, M, T, F], mix
    complex [B, M, T, F], any T >= 1 -> out complex64 [B, S, T, F], on the device for device input and on the CPU for an ndarray.
    ``opts``: the fields of :class:`OnlineBeamformer`.  ``return_debug`` adds, on the device, ``phi_s``, ``phi_n``, ``w``, ``fail``
    and ``n`` of the final state.  Causal: frame t of the output depends on no later frame."""
    ishape, mshape = np.shape(images), np.shape(mix)
    o = OnlineBeamformer(**opts).validate(ishape[2] if len(ishape) == 5 else None, ishape[1] if len(ishape) == 5 else None)
    if len(ishape) != 5 or len(mshape) != 4 or min(ishape) < 1 or tuple(mshape) != (ishape[0],) + tuple(ishape[2:]):
        raise ValueError(f"images {tuple(ishape)} must be [B, S, M, T, F], all positive, and mix {tuple(mshape)} [B, M, T, F]")
    st = BeamformStream(ishape[2], ishape[1], ishape[4], ishape[0], device=default_device(images, device), **dataclasses.asdict(o))
    out = st.process(images, mix)
    return (out, st._debug()) if return_debug else out


def pit_select(anchor, cand, return_dist=False):
    """Speaker alignment by the reference's PIT rule (tester.py:1053-1065, 902-915): all S! permutations in
    itertools.permutations order, first minimum of the summed magnitude distance (1 <= S <= 4).

    anchor, cand: complex [B, S, T, F] device tensors.  Returns int32 [B, S] ``sel`` with aligned speaker i =
    cand[:, sel[:, i]] (and the distance matrix float64 [B, S, S] if asked)."""
    a, _ = _dev_c64(anchor, None if isinstance(anchor, torch.Tensor) and anchor.is_cuda else torch.device("cuda"))
    c, _ = _dev_c64(cand, a.device)
    if a.shape != c.shape or a.dim() != 4:
        raise ValueError("anchor and cand must both be [B, S, T, F]")
    B, S, T, F = a.shape
    sel = torch.empty((B, S), dtype=torch.int32, device=a.device)
    L = _lib.lib()
    nd = L.misonet_pit_scratch_bytes(B, S, F) // 8                                    # result [B,S,S] + per-bin partials
    dist = torch.empty((nd // (S * S), S, S), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.misonet_pit_select(a.data_ptr(), c.data_ptr(), B, S, T, F, sel.data_ptr(), dist.data_ptr(),
                                        dist.numel() * 8, _lib.stream_ptr(a.device)))
    return (sel, dist[:B]) if return_dist else sel
