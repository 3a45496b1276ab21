"""Recordings at any sample rate: the polyphase resampler on the device (csrc/resample.hip, C ABI ``misonet_resample*`` in
include/misonet.h).

The definition is ``scipy.signal.resample_poly``'s (= librosa's ``res_type="polyphase"``; it is NOT librosa's default, ``soxr_hq``,
which was not available and was not compared): p / q = fs_out / fs_in in lowest terms, half-length Lh = 10 max(p, q), taps
g = p firwin(2 Lh + 1, 1 / max(p, q), window=("kaiser", 5.0)), y[m] = sum_j x[j] g[m q - j p + Lh] with j ascending, zeros outside
the signal, ceil(n p / q) output samples, every channel on its own.  The sum is float64 and is rounded once.

``resample(x, fs_in, fs_out)``     -- [L], [L, M] or [B, L, M], float32 or int16, ndarray or tensor -> the same kind of container
``resample_into(src, dst, n_valid, fs_in, fs_out)`` -- the same into a device buffer of the caller's (capturable in a HIP graph)
``resampled_len(n, fs_in, fs_out)`` and ``ratio(fs_in, fs_out)`` and ``taps(fs_in, fs_out)`` -- host only, no GPU
``load_wav(path, sr=None)``        -- the reference's loader line (``librosa.load(path, mono=False, sr=...)``, dataloader/data.py:613)
``tile()``                         -- the output samples one workgroup owns

The recording paths (``Enhancer.enhance_recording`` / ``enhance_recordings`` / ``enhance_continuous``,
``BlindSeparator.separate_recording``, ``dereverb_wav``) take ``fs_in`` and ``fs_out`` and go through :func:`plan_rates`,
:func:`to_rate` and :func:`pcm_to_rate` below.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._online import make_callable

MAX_RATE = 1024            # max(p, q)
MAX_N = 1 << 28            # samples per channel
MAX_CH = 16                # channels of one launch; wider inputs go in groups of this many
MAX_B = 65535


def _rate(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1 or int(v) > 0x7FFFFFFF:
        raise ValueError(f"{name} must be a positive integer sample rate, got {v!r}")
    return int(v)


def ratio(fs_in, fs_out):
    """(p, q) with p / q = fs_out / fs_in in lowest terms; ValueError for a rate < 1 or max(p, q) > 1024"""
    fs_in, fs_out = _rate(fs_in, "fs_in"), _rate(fs_out, "fs_out")
    p, q = C.c_int(), C.c_int()
    if _lib.lib().misonet_resample_ratio(fs_in, fs_out, C.byref(p), C.byref(q)) != _lib.OK:
        raise ValueError(f"{fs_in} -> {fs_out} Hz: max(p, q) of p / q = fs_out / fs_in must not exceed {MAX_RATE}")
    return p.value, q.value


def resampled_len(n, fs_in, fs_out) -> int:
    """ceil(n p / q): the length ``resample`` gives n samples (``misonet_resampled_len``)"""
    ratio(fs_in, fs_out)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_N:
        raise ValueError(f"n must be an integer in [1, 2^28], got {n!r}")
    return int(_lib.lib().misonet_resampled_len(int(n), int(fs_in), int(fs_out)))


def taps(fs_in, fs_out) -> np.ndarray:
    """g = p firwin(2 Lh + 1, 1 / max(p, q), window=("kaiser", 5.0)) as float64 [2 Lh + 1], built by the library on the host
    ([1.0] for p = q = 1)"""
    ratio(fs_in, fs_out)
    L = _lib.lib()
    n = L.misonet_resample_taps(int(fs_in), int(fs_out), None, 0)
    if n < 1:
        _lib.check(n)
    out = np.empty(n, dtype=np.float64)
    if L.misonet_resample_taps(int(fs_in), int(fs_out), out.ctypes.data_as(C.POINTER(C.c_double)), n) != n:
        _lib.check(_lib.EINVAL)
    return out


def tile() -> int:
    """the output samples one workgroup of the kernel owns (``misonet_resample_tile``)"""
    return int(_lib.lib().misonet_resample_tile())


def resample_into(src, dst, n_valid, fs_in, fs_out):
    """The call itself, into a buffer of the caller's (what a HIP graph captures: no allocation, no synchronisation once the
    taps of this ratio exist on the device).  src [B, n, M] and dst [B, ceil(n p / q), M]: device tensors, float32 or int16,
    any strides (dst without overlap); n_valid None or int32 [B] on the device.  One launch per group of 16 channels."""
    L = _lib.lib()
    p, q = ratio(fs_in, fs_out)
    if not (isinstance(src, torch.Tensor) and isinstance(dst, torch.Tensor) and src.is_cuda and dst.is_cuda and src.dim() == 3):
        raise ValueError("src and dst must be device tensors [B, n, M]")
    if src.dtype not in (torch.float32, torch.int16) or dst.dtype not in (torch.float32, torch.int16):
        raise TypeError("src and dst must be float32 or int16")
    B, n, M = src.shape
    if tuple(dst.shape) != (B, (n * p + q - 1) // q, M) or dst.device != src.device:
        raise ValueError(f"dst {tuple(dst.shape)} must be {(B, (n * p + q - 1) // q, M)} on the device of src")
    if n_valid is not None and (not isinstance(n_valid, torch.Tensor) or n_valid.device != src.device or
                                n_valid.dtype != torch.int32 or tuple(n_valid.shape) != (B,) or not n_valid.is_contiguous()):
        raise ValueError(f"n_valid must be None or a contiguous int32 [{B}] on the device of src")
    with torch.cuda.device(src.device):
        st = _lib.stream_ptr(src.device)
        for c0 in range(0, M, MAX_CH):
            s, d = src[:, :, c0:c0 + MAX_CH], dst[:, :, c0:c0 + MAX_CH]
            _lib.check(L.misonet_resample(s.data_ptr(), int(s.dtype == torch.int16), s.stride(0), s.stride(2), s.stride(1), B,
                                          s.shape[2], n, None if n_valid is None else n_valid.data_ptr(), fs_in, fs_out,
                                          d.data_ptr(), int(d.dtype == torch.int16), d.stride(0), d.stride(2), d.stride(1), st))


def resample(x, fs_in, fs_out, n_valid=None, out_int16=False, device=None):
    """x [L], [L, M] or [B, L, M], float32 or int16 (ndarray or tensor) at ``fs_in`` -> the same shape with ceil(L p / q) samples
    at ``fs_out``, float32 or (``out_int16``: x 32767, rounded to nearest, saturated) int16; an int16 input sample q stands for
    q / 32767.  An ndarray or CPU tensor comes back as one; a device tensor is read in place through its strides (a view such as
    every second microphone or a transposed [M, L] buffer costs no copy) and the result is on the device, channel-major in memory
    where the input was.  ``n_valid``: B lengths (a sequence, or an int32 device tensor), one per item; the outputs of item b past
    ceil(n_valid[b] p / q) are zeros.  Every argument is checked before anything is copied or launched."""
    fs_in, fs_out = _rate(fs_in, "fs_in"), _rate(fs_out, "fs_out")
    p, q = ratio(fs_in, fs_out)
    is_t = isinstance(x, torch.Tensor)
    if not is_t and not isinstance(x, np.ndarray):
        raise TypeError("x must be an ndarray or a tensor")
    if x.dtype not in ((torch.float32, torch.int16) if is_t else (np.dtype(np.float32), np.dtype(np.int16))):
        raise TypeError(f"x must be float32 or int16, got {x.dtype}")
    nd = x.dim() if is_t else x.ndim
    if nd not in (1, 2, 3):
        raise ValueError(f"x {tuple(x.shape)} must be [L], [L, M] or [B, L, M]")
    shape = tuple(x.shape)
    B, n, M = (1, shape[0], 1) if nd == 1 else ((1,) + shape if nd == 2 else shape)
    if not 1 <= n <= MAX_N:
        raise ValueError(f"the number of samples must be in [1, 2^28], got {n}")
    if M < 1 or not 1 <= B <= MAX_B:
        raise ValueError(f"x {shape}: needs at least one channel and 1 <= B <= {MAX_B}")
    nv_dev = isinstance(n_valid, torch.Tensor) and n_valid.is_cuda
    if n_valid is not None:
        if nv_dev:
            if n_valid.dtype != torch.int32 or tuple(n_valid.shape) != (B,) or not n_valid.is_contiguous():
                raise ValueError(f"a device n_valid must be contiguous int32 [{B}]")
        else:
            nv = np.asarray(n_valid)
            if nv.shape != (B,) or nv.dtype.kind not in "iu" or nv.min() < 0 or nv.max() > n:
                raise ValueError(f"n_valid must hold {B} integer lengths in [0, {n}]")
    on_dev = is_t and x.is_cuda
    if device is None:
        device = x.device if on_dev else torch.device("cuda", torch.cuda.current_device())
    n_out = (n * p + q - 1) // q
    src = x if is_t else torch.from_numpy(np.ascontiguousarray(x))
    src = src.reshape(B, n, M) if (not on_dev or nd != 2) else src[None]        # a device view keeps its strides
    src = src.to(device)
    odt = torch.int16 if out_int16 else torch.float32
    if on_dev and M > 1 and src.stride(2) > src.stride(1):                      # channel-major in memory: so is the result
        dst = torch.empty((B, M, n_out), dtype=odt, device=device).transpose(1, 2)
    else:
        dst = torch.empty((B, n_out, M), dtype=odt, device=device)
    if n_valid is not None and not nv_dev:
        n_valid = torch.from_numpy(np.asarray(n_valid).astype(np.int32)).to(device)
    resample_into(src, dst, n_valid, fs_in, fs_out)
    out = dst[0, :, 0] if nd == 1 else (dst[0] if nd == 2 else dst)
    if on_dev:
        return out
    return out.cpu() if is_t else out.cpu().numpy()


def load_wav(path, sr: Optional[int] = None, device=None):
    """The reference's loader line, ``librosa.load(path, mono=False, sr=sr)`` (dataloader/data.py:613), for PCM 16 / 24 wav files:
    -> (float32 [L, M] time-major, rate).  ``sr=None`` keeps the file's rate; another rate resamples on the device
    (``res_type="polyphase"``'s definition, see the module text).  The samples are the integers / 2^15 or / 2^23, as libsndfile
    reads them."""
    import wave
    from .stft import read_wav_pcm24
    if sr is not None:
        sr = _rate(sr, "sr")
    with wave.open(path, "rb") as w:
        width, ch, fs, n = w.getsampwidth(), w.getnchannels(), w.getframerate(), w.getnframes()
        raw = w.readframes(n) if width == 2 else None
    if width == 2:
        x = (np.frombuffer(raw, dtype="<i2").reshape(n, ch) / 32768.0).astype(np.float32)
    elif width == 3:
        x = (read_wav_pcm24(path)[0] / float(1 << 23)).astype(np.float32)
    else:
        raise ValueError(f"{path}: {8 * width}-bit PCM is not supported (16 or 24)")
    if sr is None or sr == fs:
        return x, int(fs)
    return resample(x, int(fs), sr, device=device), sr


# ---- what the recording paths share ----------------------------------------------------------------------------------------
def plan_rates(fs, fs_in, fs_out):
    """The ``fs_in`` / ``fs_out`` arguments of a recording path whose model runs at ``fs`` -> (rate to resample the input from or
    None, rate to resample the result to or None, the rate of the result).  ``fs_out="in"`` is the input's rate.  ValueError for
    anything else that is no admitted rate -- before anything is copied."""
    fs = _rate(fs, "fs")
    r_in = None if fs_in is None else _rate(fs_in, "fs_in")
    if fs_out is None:
        r_out = None
    elif isinstance(fs_out, str):
        if fs_out != "in":
            raise ValueError(f"fs_out must be None, an integer rate or \"in\", got {fs_out!r}")
        r_out = fs if r_in is None else r_in
    else:
        r_out = _rate(fs_out, "fs_out")
    if r_in is not None:
        ratio(r_in, fs)
    if r_out is not None:
        ratio(fs, r_out)
    return (None if r_in == fs else r_in), (None if r_out == fs else r_out), (fs if r_out is None else r_out)


def to_rate(wavs, fs_in, fs, device):
    """Host recordings float32 [L, M] of one shape (the observation and, with scores, its clean sources) -> the same at ``fs``,
    in ONE launch as the items of a batch, back on the host for the paths' chunking code (that one copy: INTEGRATION.md 4o)."""
    arrs = [np.asarray(w, dtype=np.float32) for w in wavs]
    if any(a.ndim != 2 or a.shape != arrs[0].shape for a in arrs):
        raise ValueError("the recordings resampled together must all be [n_samples, n_mics] of one shape")
    out = resample(torch.from_numpy(np.stack(arrs)).to(device), fs_in, fs).cpu().numpy()
    return [out[k] for k in range(len(arrs))]


def pcm_to_rate(pcm, fs, fs_out, length, device):
    """The separated waves int16 [S, L'] at ``fs`` -> int16 [S, L''] at ``fs_out`` on the device (read channel-major, in place);
    ``length`` not None: trimmed or zero-padded to it (the original length, when the result goes back to the input's rate)."""
    x = torch.from_numpy(np.ascontiguousarray(pcm)).to(device)                  # [S, L']
    y = resample(x.transpose(0, 1), fs, fs_out, out_int16=True).transpose(0, 1)      # [S, L''], contiguous
    out = y.cpu().numpy()
    if length is not None and out.shape[1] != length:
        fit = np.zeros((out.shape[0], length), dtype=np.int16)
        fit[:, :min(length, out.shape[1])] = out[:, :length]
        out = fit
    return np.ascontiguousarray(out)


def around(run, wav_observe, wav_clean, fs, fs_in, fs_out, save_path, write, device):
    """A recording path with ``fs_in`` / ``fs_out``: ``run(wav_observe, wav_clean, save_path)`` is the path at the model rate and
    returns int16 [S, L'] or a tuple that starts with it (scores and the like stay as they are: they are taken at the model
    rate); ``write(pcm, save_path, rate)`` writes the files."""
    r_in, r_out, rate = plan_rates(fs, fs_in, fs_out)
    L0 = int(np.shape(wav_observe)[0])
    if r_in is not None:
        got = to_rate([wav_observe] + list(wav_clean or []), r_in, fs, device)
        wav_observe, wav_clean = got[0], (got[1:] if wav_clean is not None else None)
    if r_out is None:
        return run(wav_observe, wav_clean, save_path)
    res = run(wav_observe, wav_clean, None)
    pcm = res[0] if isinstance(res, tuple) else res
    pcm = pcm_to_rate(pcm, fs, r_out, L0 if r_out == (fs if r_in is None else r_in) else None, device)
    if save_path is not None:
        write(pcm, save_path, rate)
    return (pcm,) + tuple(res[1:]) if isinstance(res, tuple) else pcm


# ---- the streaming form ----------------------------------------------------------------------------------------------------
class ResampleStream:
    """The resampler fed in blocks, on the device (csrc/resample_stream.hip, C ABI ``misonet_resample_stream``; INTEGRATION.md
    4v): ``batch`` recordings of ``channels`` channels at ``fs_in``, blocks of any length in, blocks at ``fs_out`` out.  The stream
    carries its last ``carry`` = floor(2 Lh / p) samples; after N samples it has emitted every output whose last input has arrived
    (``latency`` = Lh / p input samples behind), and after :meth:`flush` the ``ceil(N p / q)`` samples of :func:`resample` of the
    whole signal, bit for bit and however it was cut.  ``in_int16`` / ``out_int16``: the sample kinds, with the rules of
    :func:`resample`.  The state is allocated once; a call allocates only its output.  More than 16 channels go in groups of 16,
    each on its own slice of the state."""

    def __init__(self, channels, fs_in, fs_out, batch=1, in_int16=False, out_int16=False, device=None):
        self.fs_in, self.fs_out = _rate(fs_in, "fs_in"), _rate(fs_out, "fs_out")
        self.p, self.q = ratio(self.fs_in, self.fs_out)
        self.channels, self.batch = int(channels), int(batch)
        if self.channels < 1 or not 1 <= self.batch <= MAX_B:
            raise ValueError(f"channels must be >= 1 and batch in [1, {MAX_B}], got {channels}, {batch}")
        self.in_int16, self.out_int16 = bool(in_int16), bool(out_int16)
        L = _lib.lib()
        self.carry = int(L.misonet_resample_stream_carry(self.fs_in, self.fs_out))
        half = 0 if self.p == self.q == 1 else 10 * max(self.p, self.q)
        self.latency = half / self.p
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # (first channel, channels, first byte, bytes) of every group
        self._groups, at = [], 0
        for c0 in range(0, self.channels, MAX_CH):
            m = min(MAX_CH, self.channels - c0)
            nb = int(L.misonet_resample_stream_state_bytes(self.batch, m, self.fs_in, self.fs_out))
            self._groups.append((c0, m, at, nb))
            at += nb
        self.state = torch.empty(at, dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self):
        """no sample seen: the carried tail is zero"""
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for _c0, m, at, nb in self._groups:
                _lib.check(L.misonet_resample_stream_reset(self.state.data_ptr() + at if nb else None, self.batch, m, self.fs_in,
                                                           self.fs_out, _lib.stream_ptr(self.device)))
        self.samples_seen, self.samples_out, self._spent = 0, 0, False
        return self

    def outputs(self, n_new: int, flush: bool = False) -> int:
        """the samples the next call emits for ``n_new`` samples (``misonet_resample_stream_outputs``)"""
        n = int(_lib.lib().misonet_resample_stream_outputs(self.samples_seen, int(n_new), int(bool(flush)), self.fs_in,
                                                           self.fs_out))
        if n < 0:
            raise ValueError(f"a block must hold 1 .. 2^28 samples (0 with flush), got {n_new}")
        return n

    def _block(self, block):
        if self._spent:
            raise ValueError("the stream was flushed: reset() before the next block")
        want = torch.int16 if self.in_int16 else torch.float32
        if not isinstance(block, torch.Tensor) or block.device != self.state.device or block.dtype != want:
            raise ValueError(f"block must be a {want} tensor on {self.state.device}")
        if block.dim() == 2 and self.batch == 1:
            block = block[None]
        if block.dim() != 3 or (block.shape[0], block.shape[2]) != (self.batch, self.channels):
            raise ValueError(f"block {tuple(block.shape)} must be [{self.batch}, n, {self.channels}]")
        if block.shape[1] > 1 and block.stride(1) < 1:
            raise ValueError("block must advance in memory from sample to sample: a time axis made by expand() (stride 0) is "
                             "not a block of samples")
        return block

    def process_into(self, block: torch.Tensor, out, flush: bool = False):
        """block [B, n, M] and out [B, n_out, M] with ``n_out = outputs(n, flush)`` (None when n_out == 0): device tensors of the
        stream's sample kinds, any strides (out without overlap).  Two launches per group of 16 channels, nothing allocated: the
        call a HIP graph captures (once the stream emits, a launch depends on ``samples_seen`` only through the place of the first
        output against the block: replay it with blocks of that length, a multiple of q).  The counters ``samples_seen`` and
        ``samples_out`` live on the host and advance once per call of this method: a capture advances them with no device work
        behind it, and replays of the graph do not move them -- the owner of a graph keeps its own count."""
        L = _lib.lib()
        block = self._block(block)
        n = block.shape[1]
        n_out = self.outputs(n, flush)
        want = torch.int16 if self.out_int16 else torch.float32
        if n_out > 0 and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (self.batch, n_out, self.channels)
                          or out.dtype != want or out.device != self.state.device):
            raise ValueError(f"out must be a {want} tensor [{self.batch}, {n_out}, {self.channels}] on {self.state.device}")
        if n_out > 0 and any(size > 1 and stride < 1 for size, stride in zip(out.shape, out.stride())):
            raise ValueError("out must not overlap itself: a stride of 0 along an axis longer than 1")
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            for c0, m, at, nb in self._groups:
                s = block[:, :, c0:c0 + m]
                d = out[:, :, c0:c0 + m] if n_out else None
                _lib.check(L.misonet_resample_stream(
                    s.data_ptr() if n else None, int(self.in_int16), s.stride(0), s.stride(2), s.stride(1) if n > 1 else 1, self.batch, m,
                    n, self.samples_seen, int(bool(flush)), self.fs_in, self.fs_out, d.data_ptr() if n_out else None,
                    int(self.out_int16), d.stride(0) if n_out else 1, d.stride(2) if n_out else 1, d.stride(1) if n_out else 1,
                    self.state.data_ptr() + at if nb else None, nb, st))
        self.samples_seen += n
        self.samples_out += n_out
        self._spent = bool(flush)
        return out

    def process(self, block, flush: bool = False):
        """The next n >= 1 samples: [B, n, M] (or [n, M] when batch == 1) on the device, read in place through its strides ->
        [B, n_out, M], the outputs these samples complete; n_out may be 0, which gives an empty tensor."""
        block = self._block(block)
        out = torch.empty((self.batch, self.outputs(block.shape[1], flush), self.channels),
                          dtype=torch.int16 if self.out_int16 else torch.float32, device=self.device)
        self.process_into(block, out, flush)
        return out

    def flush(self, block=None):
        """The end of the stream, with or without a last block: the outputs still owed -- ``ceil(samples_seen p / q)`` in all.
        The stream is spent until :meth:`reset`."""
        if block is None:
            if self._spent:
                raise ValueError("the stream was flushed: reset() before the next block")
            block = torch.empty((self.batch, 0, self.channels), dtype=torch.int16 if self.in_int16 else torch.float32,
                                device=self.device)
        return self.process(block, flush=True)


# ``misonet_amd.resample`` names both this module and the function above: ``misonet_amd.resample(x, 48000, 16000)`` works either
# way
make_callable(__name__)
