"""WPE dereverberation on the device (csrc/wpe.hip, C ABI ``misonet_wpe`` in include/misonet.h).

``dereverb(mix)``        complex [B, M, T, F] -> complex64 of the same shape: multichannel linear prediction per bin
                         (Nakatani et al. 2010; with the defaults nara_wpe's ``wpe_v8``), float64 on the matrix cores
``dereverb_wav(wav)``    float32 [L, M] -> float32 [L, M]: STFT of the whole recording -> WPE -> iSTFT, on the device
``Dereverb``             the options as one plain-data object, used by every layer (``Enhancer(dereverb=...)``)

Online WPE (csrc/owpe.hip, C ABI ``misonet_owpe``): the frame-recursive form, fed audio as it arrives.
``DereverbStream(M)``    owns the state of one stream: ``process(block)`` takes any T >= 1 new frames; the memory does not grow
``dereverb_online(mix)`` the one-shot call: reset, then process
``OnlineDereverb``       its options (``dereverb_wav(online=...)``, ``Enhancer(dereverb=OnlineDereverb(...))``)
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._online import OnlineStream, _dev_c64, check_real, default_device, make_callable, spec_of

HOP = 64


@dataclasses.dataclass(frozen=True)
class Dereverb:
    """One plain-data description of the dereverberation (``misonet_wpe_opts`` of include/misonet.h).

    taps         prediction filter length per microphone (M taps <= 80)
    delay        prediction delay in frames (>= 1): the direct sound and the early reflections are left alone
    iterations   alternations of power estimate and filter (1 .. 10)
    diag_load    R <- R + diag_load tr(R) / (M taps) I
    power_floor  w[t] = 1 / max(p[t], power_floor max_t p[t])
    """
    taps: int = 10
    delay: int = 3
    iterations: int = 3
    diag_load: float = 0.0
    power_floor: float = 1e-10

    @classmethod
    def of(cls, spec) -> "Dereverb":
        """None or True (the defaults), a Dereverb, or a dict of the fields above"""
        return spec_of(cls, spec, "dereverb", "dereverb must be None, True, a Dereverb or a dict of its fields")

    def validate(self, num_mic: Optional[int] = None) -> "Dereverb":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        for name in ("taps", "delay", "iterations"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"dereverb {name} must be an integer, got {v!r}")
        if num_mic is not None and not 1 <= num_mic <= 8:
            raise ValueError(f"dereverb takes 1 .. 8 microphones, got {num_mic}")
        if self.taps < 1 or self.taps * (num_mic if num_mic is not None else 1) > 80:
            raise ValueError(f"dereverb taps must be >= 1 with M * taps <= 80, got taps {self.taps}"
                             + (f" at M = {num_mic}" if num_mic is not None else ""))
        if self.delay < 1:
            raise ValueError(f"dereverb delay must be >= 1, got {self.delay}")
        if not 1 <= self.iterations <= 10:
            raise ValueError(f"dereverb iterations must be in [1, 10], got {self.iterations}")
        for name in ("diag_load", "power_floor"):
            check_real("dereverb", name, getattr(self, name), positive=False)
        return self

    def c_opts(self) -> "_lib.WpeOpts":
        return _lib.WpeOpts(int(self.taps), int(self.delay), int(self.iterations), float(self.diag_load),
                            float(self.power_floor))


@dataclasses.dataclass(frozen=True)
class OnlineDereverb:
    """One plain-data description of the online dereverberation (``misonet_owpe_opts`` of include/misonet.h).

    taps         prediction filter length per microphone (M taps <= 80)
    delay        prediction delay in frames (>= 1)
    context      earlier frames in the power estimate (0 .. 16)
    alpha        forgetting factor, 0 < alpha <= 1
    power_floor  lambda = max(mean of the latest powers, power_floor): absolute, > 0
    init         P = init I at reset, > 0
    """
    taps: int = 10
    delay: int = 3
    context: int = 0
    alpha: float = 0.999
    power_floor: float = 1e-10
    init: float = 1.0

    @classmethod
    def of(cls, spec) -> "OnlineDereverb":
        """None or True (the defaults), an OnlineDereverb, or a dict of the fields above"""
        return spec_of(cls, spec, "online dereverb",
                       "online dereverb must be None, True, an OnlineDereverb or a dict of its fields")

    def validate(self, num_mic: Optional[int] = None) -> "OnlineDereverb":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        for name in ("taps", "delay", "context"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"online dereverb {name} must be an integer, got {v!r}")
        if num_mic is not None and not 1 <= num_mic <= 8:
            raise ValueError(f"online dereverb takes 1 .. 8 microphones, got {num_mic}")
        if self.taps < 1 or self.taps * (num_mic if num_mic is not None else 1) > 80:
            raise ValueError(f"online dereverb taps must be >= 1 with M * taps <= 80, got taps {self.taps}"
                             + (f" at M = {num_mic}" if num_mic is not None else ""))
        if self.delay < 1:
            raise ValueError(f"online dereverb delay must be >= 1, got {self.delay}")
        if not 0 <= self.context <= 16:
            raise ValueError(f"online dereverb context must be in [0, 16], got {self.context}")
        for name in ("alpha", "power_floor", "init"):
            check_real("online dereverb", name, getattr(self, name), positive=True)
        if self.alpha > 1:
            raise ValueError(f"online dereverb alpha must be in (0, 1], got {self.alpha!r}")
        return self

    def c_opts(self) -> "_lib.OwpeOpts":
        return _lib.OwpeOpts(int(self.taps), int(self.delay), int(self.context), float(self.alpha), float(self.power_floor),
                             float(self.init))


class DereverbStream(OnlineStream):
    """The state of one stream of online WPE, on the device: ``batch`` recordings of ``num_mic`` microphones and ``num_bins``
    bins.  ``opts``: the fields of :class:`OnlineDereverb`.  The state is allocated once; a call allocates only its output."""

    def __init__(self, num_mic, num_bins=129, batch=1, *, device=None, **opts):
        self.opts = OnlineDereverb(**opts).validate(int(num_mic))
        self.num_mic, self.num_bins, self.batch = int(num_mic), int(num_bins), int(batch)
        if self.num_bins < 1 or self.batch < 1:
            raise ValueError(f"num_bins and batch must be positive, got {num_bins}, {batch}")
        self._c = self.opts.c_opts()
        self._alloc(_lib.lib().misonet_owpe_state_bytes(self.batch, self.num_mic, self.num_bins, C.byref(self._c)), device)

    def _reset_call(self):
        """P = init I, G = 0, the rings empty, no frame seen, no flag"""
        return _lib.lib().misonet_owpe_reset(self.state.data_ptr(), self.batch, self.num_mic, self.num_bins, C.byref(self._c),
                                             _lib.stream_ptr(self.device))

    def process_into(self, block: torch.Tensor, out: torch.Tensor):
        """block, out: complex64 [B, M, T, F] contiguous on the stream's device, not the same buffer.  One launch, nothing
        allocated: the call a HIP graph captures."""
        B, M, T, F = block.shape
        self._same_geometry(block.shape)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().misonet_owpe(block.data_ptr(), B, M, T, F, C.byref(self._c), out.data_ptr(),
                                               self.state.data_ptr(), self.state.numel(), _lib.stream_ptr(self.device)))
        return out

    def process(self, block):
        """The next T >= 1 frames of the stream: complex [B, M, T, F] -> complex64 of the same shape, on the device for device
        input and on the CPU for an ndarray.  The bits do not depend on how the stream is cut into calls."""
        self._check_block(np.shape(block))
        x, np_in = _dev_c64(block, self.device)
        out = self.process_into(x, torch.empty_like(x))
        return out.cpu() if np_in else out

    def _parts(self):
        B, M, F, N = self.batch, self.num_mic, self.num_bins, self.num_mic * self.opts.taps
        return dict(G=((B, F, N, M), torch.complex128), P=((B, F, N, N), torch.complex128), fail=((B, F), torch.int32),
                    n=((B, F), torch.int32))

    def _debug_call(self, ptr):
        return _lib.lib().misonet_owpe_debug(self.state.data_ptr(), self.batch, self.num_mic, self.num_bins, C.byref(self._c),
                                             ptr("G"), ptr("P"), ptr("fail"), ptr("n"), _lib.stream_ptr(self.device))

    def filters(self):
        """the prediction filter G complex128 [B, F, M taps, M] as it stands, on the device"""
        return self._debug(("G",))["G"]

    def covariance(self):
        """the inverse correlation matrix P complex128 [B, F, M taps, M taps] as it stands, on the device"""
        return self._debug(("P",))["P"]

    fail = property(OnlineStream.fail.fget, doc="int32 [B, F] on the device: bit 0 set once a frame of that bin was passed through")


def dereverb_online(mix, *, return_debug=False, device=None, **opts):
    """Online WPE of a batch of spectrograms in one call: reset, then process.  mix complex [B, M, T, F], any T >= 1 -> complex64
    of the same shape, on the device for device input and on the CPU for an ndarray.  ``opts``: the fields of
    :class:`OnlineDereverb`.  ``return_debug`` adds, on the device, ``G``, ``P``, ``fail`` and ``n`` of the final state.  Causal:
    frame t of the output depends on no later frame.  It does not dereverberate better than :func:`dereverb`."""
    shape = np.shape(mix)
    o = OnlineDereverb(**opts).validate(shape[1] if len(shape) == 4 else None)
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f"mix {tuple(shape)} must be [B, M, T, F], all positive")
    st = DereverbStream(shape[1], shape[3], shape[0], device=default_device(mix, device), **dataclasses.asdict(o))
    out = st.process(mix)
    return (out, st._debug()) if return_debug else out


def _wpe_device(mix: torch.Tensor, power: Optional[torch.Tensor], opts: "_lib.WpeOpts", return_debug: bool):
    """mix complex64 [B, M, T, F] contiguous on the device (power float32 [B, T, F] or None) -> out (and the debug dict)"""
    B, M, T, F = mix.shape
    L = _lib.lib()
    nws = L.misonet_wpe_workspace_bytes(B, M, T, F, C.byref(opts))
    if nws < 0:
        _lib.check(_lib.EINVAL)
    ws = torch.empty(int(nws), dtype=torch.uint8, device=mix.device)
    out = torch.empty_like(mix)
    dbg = None
    with torch.cuda.device(mix.device):
        st = _lib.stream_ptr(mix.device)
        _lib.check(L.misonet_wpe(mix.data_ptr(), power.data_ptr() if power is not None else None, B, M, T, F, C.byref(opts),
                                 out.data_ptr(), ws.data_ptr(), ws.numel(), st))
        if return_debug:
            g = torch.empty((B, F, M * opts.taps, M), dtype=torch.complex128, device=mix.device)
            bad = torch.empty((B, F), dtype=torch.int32, device=mix.device)
            _lib.check(L.misonet_wpe_debug(ws.data_ptr(), B, M, F, C.byref(opts), g.data_ptr(), bad.data_ptr(), st))
            dbg = dict(G=g, fail=bad)
    return out, dbg


def dereverb(mix, power=None, *, taps=10, delay=3, iterations=3, diag_load=0.0, power_floor=1e-10, return_debug=False,
             device=None):
    """WPE dereverberation of a batch of spectrograms.

    mix: complex [B, M, T, F] (np.ndarray or torch tensor): the layout of ``stft_hip`` and of the networks' input.  Returns
    complex64 of the same shape: on the CPU for ndarray input, on the device for device input.  ``power`` float [B, T, F]
    replaces the power estimate of the FIRST iteration (DNN-WPE: e.g. ``sum_s |MISO1 estimate|^2`` averaged over the
    microphones, with ``iterations=1``).  A bin whose correlation matrix cannot be factored (an all-zero bin) comes back
    unchanged.  ``return_debug`` adds, on the device, ``G`` complex128 [B, F, M taps, M] (the filter of the last
    iteration) and ``fail`` int32 [B, F]."""
    shape = np.shape(mix)
    opts = Dereverb(taps, delay, iterations, diag_load, power_floor).validate(shape[1] if len(shape) == 4 else None)
    if len(shape) != 4:
        raise ValueError(f"mix {tuple(shape)} must be [B, M, T, F]")
    if shape[2] < 2 or shape[0] < 1 or shape[3] < 1:
        raise ValueError(f"mix {tuple(shape)}: B and F must be positive and T >= 2")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    x, np_in = _dev_c64(mix, device)
    pw = None
    if power is not None:
        pw = torch.as_tensor(power)
        if tuple(pw.shape) != (shape[0], shape[2], shape[3]) or pw.is_complex():
            raise ValueError(f"power {tuple(pw.shape)} must be real [B, T, F] = {(shape[0], shape[2], shape[3])}")
        pw = pw.to(x.device).to(torch.float32).contiguous()
    out, dbg = _wpe_device(x, pw, opts.c_opts(), return_debug)
    if np_in:
        out = out.cpu()
    return (out, dbg) if return_debug else out


def dereverb_wav(wav, fs=16000, *, device=None, srmr=False, ref_ch=0, fs_in=None, fs_out=None, online=None, **opts):
    """Recording-wise dereverberation: wav float32 [L, M] (ndarray or tensor) -> float32 [L, M] of the same kind.

    The recording is zero-padded to whole hops, transformed in one piece (``misonet_stft``), dereverberated
    (``misonet_wpe``: the filters are estimated over the whole recording), transformed back (``misonet_istft``, float32)
    and trimmed to L: all on the device.  ``fs`` is accepted for symmetry with the other recording calls; the frame
    geometry is the networks' (256 / 64 samples).  ``opts``: the fields of :class:`Dereverb`.

    ``srmr=True``: returns ``(wav, Srmr)``: the speech-to-reverberation modulation energy ratio (the figure
    that needs no clean reference) of output channel ``ref_ch`` at rate ``fs`` (8000 or 16000), with input channel ``ref_ch``
    as the mixture, so that ``srmr_i`` is what the dereverberation gained.  Both are read on the device, in place, as
    time-major views; the waves are bit for bit those of ``srmr=False``.

    ``fs_in`` / ``fs_out``: ``fs`` is the rate the dereverberation runs at.  ``fs_in`` other than ``fs``: ``wav``
    is at ``fs_in`` and is taken to ``fs`` on the device first (:mod:`misonet_amd.resample`); ``fs_out`` (an integer rate or ``"in"``):
    the float32 result is taken to that rate on the device, and has the input's length L when that is the input's rate.  The SRMR
    is measured at ``fs``.  With both None not one launch is added.

    ``online``: None -- the offline filter above, every bit and every launch as before; True, an
    :class:`OnlineDereverb` or a dict of its fields -- the frame-recursive form between the same STFT and iSTFT
    (``misonet_owpe_reset``, one ``misonet_owpe`` over all frames); ``opts`` must then be empty."""
    if online is not None and online is not False:
        if opts:
            raise ValueError(f"with online= the options go into it, not beside it: {sorted(opts)}")
        online = OnlineDereverb.of(online)
    else:
        online = None
    if fs_in is not None or fs_out is not None:
        from . import resample as RS
        r_in, r_out, _ = RS.plan_rates(fs, fs_in, fs_out)                  # a bad rate: before anything else
        if srmr:
            from . import score as SC
            SC.check_srmr_fs(fs)
        Dereverb(**opts)                                                   # ... and an unknown option
        if online is not None:
            opts = dict(online=online)
        np_in = not isinstance(wav, torch.Tensor)
        w = torch.as_tensor(wav)
        if w.dim() != 2 or w.shape[0] <= w.shape[1]:
            raise ValueError("wav must be [n_samples, n_mics] with n_samples > n_mics")
        if device is None:
            device = w.device if w.is_cuda else torch.device("cuda", torch.cuda.current_device())
        L0, x = int(w.shape[0]), w.to(device=device, dtype=torch.float32)
        if r_in is not None:
            x = RS.resample(x, r_in, fs)
        res = dereverb_wav(x, fs, device=device, srmr=srmr, ref_ch=ref_ch, **opts)
        y = res[0] if srmr else res
        if r_out is not None:
            y = RS.resample(y, fs, r_out)
            if r_out == (fs if r_in is None else r_in) and y.shape[0] != L0:
                y = torch.nn.functional.pad(y[:L0], (0, 0, 0, max(0, L0 - y.shape[0])))
        y = y.cpu().numpy() if np_in else y
        return (y, res[1]) if srmr else y
    from . import stft as S
    if srmr:
        from . import score as SC
        SC.check_srmr_fs(fs)
    d = Dereverb(**opts) if online is None else online
    np_in = not isinstance(wav, torch.Tensor)
    w = torch.as_tensor(wav)
    if w.dim() != 2 or w.shape[0] <= w.shape[1]:
        raise ValueError("wav must be [n_samples, n_mics] with n_samples > n_mics")
    d.validate(int(w.shape[1]))
    if device is None:
        device = w.device if w.is_cuda else torch.device("cuda", torch.cuda.current_device())
    L, M = w.shape
    Lp = max(2 * HOP, -(-L // HOP) * HOP)
    padded = torch.zeros((1, Lp, M), dtype=torch.float32, device=device)
    padded[0, :L] = w.to(device=device, dtype=torch.float32)
    spec = S.stft_hip(padded)                                          # [1, M, Lp / 64 + 1, 129]
    if online is None:
        out, _ = _wpe_device(spec, None, d.c_opts(), False)
    else:
        out = DereverbStream(M, spec.shape[3], 1, device=device, **dataclasses.asdict(d)).process(spec)
    y = S._istft_hip(out, False)[0, :, :L].transpose(0, 1).contiguous()    # [L, M]
    if srmr:
        if not 0 <= int(ref_ch) < M:
            raise ValueError(f"ref_ch must be in [0, {M}) (got {ref_ch})")
        r = int(ref_ch)
        block = SC.srmr_block(y[:, r:r + 1].transpose(0, 1)[None], padded[:, :L, r:r + 1].transpose(1, 2), None, fs)
        sr = SC.srmr_unpack(block[0].cpu().numpy(), 1, int(fs), int(L))
        return (y.cpu().numpy() if np_in else y), sr
    return y.cpu().numpy() if np_in else y


# ``misonet_amd.dereverb`` names both this module and the function above: ``misonet_amd.dereverb(mix)`` works either way
make_callable(__name__)
