"""STFT / iSTFT contract of the reference's test-time data path, on torch (device or CPU).

  * analysis  : dataloader/data.py:505-522,540-544 -- scipy.signal.stft(hann, 256, 192) / scale with
                scale = 1/sum(hann) = 1/128, i.e. the UN-normalised one-sided STFT, zero 'boundary' padding of
                nperseg/2 on both sides; chunking into 4 s pieces with a zero-padded tail and its ``gap``
                (data.py:555-595)
  * synthesis : tester.py:949-952, 979-990 -- istft(spec * scale) * 32767 -> int16 (truncation toward zero)

torch.stft/istft with center=True, zero padding and a periodic hann window compute the same transforms (checked
against SciPy in tests/test_stft.py).  On the device both directions are hand-written HIP (csrc/stft.hip: ``stft_hip``, and
since round 4 the iSTFT + int16 of :func:`istft` / :func:`istft_int16`); torch's versions remain for CPU tensors (tests, host
tools) -- the north_star allows PyTorch for "tensor containers and iSTFT".
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from ._online import default_device

NPERSEG, HOP = 256, 64
N_FREQ = NPERSEG // 2 + 1
MAX_INT16 = 32767


def _window(device, dtype=torch.float32):
    return torch.hann_window(NPERSEG, periodic=True, device=device, dtype=dtype)


def stft_hip(wav: torch.Tensor) -> torch.Tensor:
    """The hand-written HIP front-end (csrc/stft.hip, C ABI ``misonet_stft``): wav float32 [B, L, M] on the device
    (time-major, microphones interleaved -- the ``librosa.load(...).T`` array of dataloader/data.py:605-616) ->
    complex64 [B, M, T, 129], T = L // 64 + 1.  Same transform as :func:`stft` (DFT on the fp32 matrix cores)."""
    import ctypes as C
    from . import _lib
    if wav.dim() != 3 or not wav.is_cuda:
        raise ValueError("expected a device tensor [B, n_samples, n_mic]")
    w = wav.to(torch.float32).contiguous()
    B, L, M = w.shape
    lib = _lib.lib()
    T = lib.misonet_stft_frames(L)
    out = torch.empty((B, M, T, 129), dtype=torch.complex64, device=w.device)
    ws = torch.empty(lib.misonet_stft_workspace_bytes(B, M, L), dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.misonet_stft(w.data_ptr(), B, L, M, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_ptr(w.device)))
    return out


def stft(wav: torch.Tensor) -> torch.Tensor:
    """wav float [..., L] -> complex64 [..., T, F] with T = L // 64 + 1, F = 129 (un-normalised, as fed to MISO_1).
    Host tool and test reference (torch.stft).  On a DEVICE tensor this is rocFFT with run-time compiled kernels: fine in one
    process, but one of eight processes started together on one GPU got a wrong spectrogram in a quarter of the runs (round 5,
    LAB section 0) -- device code paths use :func:`stft_hip` (or the wav entry points of the pipeline)."""
    lead = wav.shape[:-1]
    x = wav.reshape(-1, wav.shape[-1]).float()
    z = torch.stft(x, n_fft=NPERSEG, hop_length=HOP, win_length=NPERSEG, window=_window(x.device), center=True,
                   pad_mode="constant", normalized=False, onesided=True, return_complex=True)      # [N, F, T]
    return z.transpose(1, 2).reshape(*lead, z.shape[2], z.shape[1]).to(torch.complex64)


def _istft_hip(spec: torch.Tensor, want_i16: bool) -> torch.Tensor:
    """The hand-written HIP iSTFT (csrc/stft.hip ``istft_k``, C ABI ``misonet_istft``): device complex [..., T, 129] ->
    float32 or int16 [..., 64 (T - 1)] (windowed inverse DFT on the fp32 matrix cores, overlap-add, envelope division and --
    for int16 -- ``x 32767`` and the truncating cast in one launch)."""
    from . import _lib
    lead = spec.shape[:-2]
    T, F = spec.shape[-2:]
    z = spec.reshape(-1, T, F).to(torch.complex64).contiguous()
    out = torch.empty((z.shape[0], (T - 1) * HOP), dtype=torch.int16 if want_i16 else torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        _lib.check(_lib.lib().misonet_istft(z.data_ptr(), z.shape[0], T, out.data_ptr() if want_i16 else None,
                                            None if want_i16 else out.data_ptr(), _lib.stream_ptr(z.device)))
    return out.reshape(*lead, (T - 1) * HOP)


def istft(spec: torch.Tensor, length: int = None) -> torch.Tensor:
    """complex [..., T, F] -> float32 [..., (T-1)*64]: inverse of :func:`stft` (== scipy istft(spec * scale)).  Device tensors
    of the network geometry run the HIP kernel; CPU tensors (tests, host tools) and other lengths go through torch."""
    lead = spec.shape[:-2]
    T, F = spec.shape[-2:]
    if spec.is_cuda and F == N_FREQ and T >= 2 and (length is None or length == (T - 1) * HOP) and spec.numel() > 0:
        return _istft_hip(spec, False)
    z = spec.reshape(-1, T, F).transpose(1, 2).to(torch.complex64)
    n = (T - 1) * HOP if length is None else length
    x = torch.istft(z, n_fft=NPERSEG, hop_length=HOP, win_length=NPERSEG, window=_window(z.device), center=True,
                    normalized=False, onesided=True, length=n, return_complex=False)
    return x.reshape(*lead, n)


def istft_int16(spec: torch.Tensor) -> torch.Tensor:
    """tester.py:950-952: time signal * 32767 -> int16 (C-style truncation, like ndarray.astype(np.int16))."""
    if spec.is_cuda and spec.shape[-1] == N_FREQ and spec.shape[-2] >= 2 and spec.numel() > 0:
        return _istft_hip(spec, True)
    return (istft(spec) * MAX_INT16).to(torch.int16)


class StftStream:
    """The analysis half of the streaming front end, on the device (csrc/stft.hip ``stft_stream_k``, C ABI
    ``misonet_stft_stream``): ``batch`` recordings of ``num_mic`` microphones, fed in blocks of any length.
    The stream carries its last 255 samples; after N samples it has emitted ``max(0, N // 64 - 1)`` frames, and after
    :meth:`flush` the ``N // 64 + 1`` frames of :func:`stft_hip` of the whole signal, bit for bit and however it was cut.  The
    state is allocated once; a call allocates only its output."""

    def __init__(self, num_mic, batch=1, device=None):
        self.num_mic, self.batch = int(num_mic), int(batch)
        from . import _lib
        n = _lib.lib().misonet_stft_stream_state_bytes(self.batch, self.num_mic)
        if n < 0:
            raise ValueError(f"num_mic must be in [1, 64] and batch in [1, 65535], got {num_mic}, {batch}")
        self.device = default_device(None, device)
        self.state = torch.empty(int(n), dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self):
        """no sample seen: the carried tail is zero"""
        from . import _lib
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().misonet_stft_stream_reset(self.state.data_ptr(), self.batch, self.num_mic,
                                                            _lib.stream_ptr(self.device)))
        self.samples_seen, self.frames_out, self._spent = 0, 0, False
        return self

    def frames(self, n_new: int, flush: bool = False) -> int:
        """the frames the next call emits for ``n_new`` samples (``misonet_stft_stream_frames``)"""
        from . import _lib
        t = int(_lib.lib().misonet_stft_stream_frames(self.samples_seen, int(n_new), int(bool(flush))))
        if t < 0:
            raise ValueError(f"a block must hold 1 .. 2^28 samples (0 with flush), got {n_new}")
        return t

    def _block(self, block):
        if self._spent:
            raise ValueError("the stream was flushed: reset() before the next block")
        if not isinstance(block, torch.Tensor) or block.device != self.state.device or block.dtype != torch.float32:
            raise ValueError(f"block must be a float32 tensor on {self.state.device}")
        if block.dim() == 2 and self.batch == 1:
            block = block[None]
        if block.dim() != 3 or (block.shape[0], block.shape[2]) != (self.batch, self.num_mic):
            raise ValueError(f"block {tuple(block.shape)} must be [{self.batch}, n, {self.num_mic}]")
        return block

    def process_into(self, block: torch.Tensor, out, flush: bool = False):
        """block float32 [B, n, M], out complex64 [B, M, Tn, 129] with ``Tn = frames(n, flush)`` (None when Tn == 0), contiguous
        on the stream's device.  Two launches, nothing allocated: the call a HIP graph captures (once the stream has seen 128
        samples a launch depends on ``samples_seen`` through ``samples_seen % 64`` alone: replay it with blocks of that length)."""
        from . import _lib
        block = self._block(block)
        n = block.shape[1]
        Tn = self.frames(n, flush)
        if not block.is_contiguous():
            raise ValueError("block must be contiguous")
        if Tn > 0 and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (self.batch, self.num_mic, Tn, N_FREQ)
                       or out.dtype != torch.complex64 or not out.is_contiguous() or out.device != self.state.device):
            raise ValueError(f"out must be a contiguous complex64 tensor [{self.batch}, {self.num_mic}, {Tn}, {N_FREQ}] on "
                             f"{self.state.device}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().misonet_stft_stream(block.data_ptr() if n else None, self.batch, n, self.num_mic,
                                                      self.samples_seen, int(bool(flush)), out.data_ptr() if Tn else None,
                                                      self.state.data_ptr(), self.state.numel(), _lib.stream_ptr(self.device)))
        self.samples_seen += n
        self.frames_out += Tn
        self._spent = bool(flush)
        return out

    def process(self, block, flush: bool = False):
        """The next n >= 1 samples: float32 [B, n, M] (or [n, M] when batch == 1) on the device -> complex64 [B, M, Tn, 129], the
        frames these samples complete; Tn may be 0, which gives an empty tensor."""
        block = self._block(block).contiguous()
        out = torch.empty((self.batch, self.num_mic, self.frames(block.shape[1], flush), N_FREQ), dtype=torch.complex64,
                          device=self.device)
        self.process_into(block, out, flush)
        return out

    def flush(self, block=None):
        """The end of the stream, with or without a last block: the frames still owed, everything beyond the last sample counted as
        zero -- ``samples_seen // 64 + 1`` frames in all.  The stream is spent until :meth:`reset`."""
        if block is None:
            if self._spent:
                raise ValueError("the stream was flushed: reset() before the next block")
            block = torch.empty((self.batch, 0, self.num_mic), dtype=torch.float32, device=self.device)
        return self.process(block, flush=True)


class IstftStream:
    """The synthesis half (csrc/stft.hip ``istft_stream_k``, C ABI ``misonet_istft_stream``): ``rows``
    spectrogram rows fed in blocks of frames.  The stream carries its last 3 frames; after Tc frames it has emitted
    ``max(0, Tc - 2)`` hops of 64 samples, and after :meth:`flush` the ``64 (Tc - 1)`` samples of :func:`istft` (``int16=True``:
    of :func:`istft_int16`) of all its frames, bit for bit and however they were cut."""

    def __init__(self, rows, int16=False, device=None):
        from . import _lib
        self.rows, self.int16 = int(rows), bool(int16)
        n = _lib.lib().misonet_istft_stream_state_bytes(self.rows)
        if n < 0:
            raise ValueError(f"rows must be in [1, 65535], got {rows}")
        self.device = default_device(None, device)
        self.state = torch.empty(int(n), dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self):
        """no frame seen"""
        from . import _lib
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().misonet_istft_stream_reset(self.state.data_ptr(), self.rows, _lib.stream_ptr(self.device)))
        self.frames_seen, self.samples_out, self._spent = 0, 0, False
        return self

    def hops(self, t_new: int, flush: bool = False) -> int:
        """the hops of 64 samples the next call emits for ``t_new`` frames (``misonet_istft_stream_hops``)"""
        from . import _lib
        h = int(_lib.lib().misonet_istft_stream_hops(self.frames_seen, int(t_new), int(bool(flush))))
        if h < 0:
            raise ValueError(f"a block must hold 1 .. 2^22 frames (0 with flush), got {t_new}")
        return h

    def _spec(self, spec):
        if self._spent:
            raise ValueError("the stream was flushed: reset() before the next block")
        if not isinstance(spec, torch.Tensor) or spec.device != self.state.device or spec.dtype != torch.complex64:
            raise ValueError(f"spec must be a complex64 tensor on {self.state.device}")
        if spec.dim() < 2 or spec.shape[-1] != N_FREQ or int(np.prod(spec.shape[:-2], dtype=np.int64)) != self.rows:
            raise ValueError(f"spec {tuple(spec.shape)} must be [..., Tn, {N_FREQ}] with {self.rows} rows in all")
        return spec

    def process_into(self, spec: torch.Tensor, out, flush: bool = False):
        """spec complex64 [..., Tn, 129], out [..., 64 H] with ``H = hops(Tn, flush)`` (None when H == 0) of the stream's sample
        type, contiguous on the stream's device.  Two launches, nothing allocated: the call a HIP graph captures (once the stream
        has seen 3 frames a launch does not depend on ``frames_seen``)."""
        from . import _lib
        spec = self._spec(spec)
        Tn = spec.shape[-2]
        H = self.hops(Tn, flush)
        if not spec.is_contiguous():
            raise ValueError("spec must be contiguous")
        want = torch.int16 if self.int16 else torch.float32
        if H > 0 and (not isinstance(out, torch.Tensor) or out.numel() != self.rows * HOP * H or out.shape[-1] != HOP * H
                      or out.dtype != want or not out.is_contiguous() or out.device != self.state.device):
            raise ValueError(f"out must be a contiguous {want} tensor [..., {HOP * H}] of {self.rows} rows on {self.state.device}")
        ptr = out.data_ptr() if H else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().misonet_istft_stream(spec.data_ptr() if Tn else None, self.rows, Tn, self.frames_seen,
                                                       int(bool(flush)), ptr if self.int16 else None,
                                                       None if self.int16 else ptr, self.state.data_ptr(), self.state.numel(),
                                                       _lib.stream_ptr(self.device)))
        self.frames_seen += Tn
        self.samples_out += HOP * H
        self._spent = bool(flush)
        return out

    def process(self, spec, flush: bool = False):
        """The next Tn >= 1 frames: complex64 [..., Tn, 129] on the device -> float32 (int16) [..., 64 H], the hops these frames
        complete; H may be 0, which gives an empty tensor."""
        spec = self._spec(spec).contiguous()
        out = torch.empty(tuple(spec.shape[:-2]) + (HOP * self.hops(spec.shape[-2], flush),),
                          dtype=torch.int16 if self.int16 else torch.float32, device=self.device)
        self.process_into(spec, out, flush)
        return out

    def flush(self, spec=None):
        """The end of the stream, with or without a last block of frames: the hops still owed, the last one divided by its partial
        envelope -- ``64 (frames_seen - 1)`` samples in all, none for fewer than 2 frames.  ``spec=None`` returns [rows, 64 H].
        The stream is spent until :meth:`reset`."""
        if spec is None:
            if self._spent:
                raise ValueError("the stream was flushed: reset() before the next block")
            spec = torch.empty((self.rows, 0, N_FREQ), dtype=torch.complex64, device=self.device)
        return self.process(spec, flush=True)


def split_chunks(wav: np.ndarray, chunk: int) -> Tuple[List[np.ndarray], int]:
    """data.py:555-595: wav [L, M] -> list of [chunk, M] pieces (last one zero-padded) and the pad length ``gap``.

    The reference leaves L == chunk unhandled (neither branch, data.py:558-565); here it is one chunk, gap 0."""
    L = wav.shape[0]
    out, start = [], 0
    while True:
        piece = wav[start:start + chunk]
        gap = chunk - piece.shape[0]
        if gap:
            piece = np.pad(piece, ((0, gap), (0, 0)))
        out.append(piece)
        start += chunk
        if start >= L:
            return out, gap


def stitch_int16(chunks: List[np.ndarray], gap: int) -> np.ndarray:
    """tester.py:960-969: drop the zero-padded tail of the last chunk and concatenate."""
    chunks = list(chunks)
    if gap:
        chunks[-1] = chunks[-1][: len(chunks[-1]) - gap]
    return np.concatenate(chunks)


def write_wav_pcm24(path: str, samples_int16: np.ndarray, fs: int) -> None:
    """tester.py:972-974: ``sf.write(path, int16_array.T, fs, 'PCM_24')``.  libsndfile widens int16 to 24-bit PCM by a
    left shift of 8 bits, so each sample is written as the 3 little-endian bytes of ``int16 << 8``, behind the plain
    44-byte RIFF/WAVE header it writes for PCM (fmt chunk of 16 bytes, format tag 1); a data chunk of odd length is
    followed by one zero pad byte that the RIFF size counts and the data size does not -- byte for byte the layout of
    the reference's own outputs (sample/MISO3/*.wav: 64059 mono samples -> data 192177, RIFF 192214, file 192222).
    samples_int16: [n_samples] (mono) or [n_samples, n_channels]."""
    import struct
    x = np.asarray(samples_int16)
    if x.dtype != np.int16:
        raise TypeError("expected int16 samples (tester.py:952 casts before writing)")
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    v = (x.astype(np.int32) << 8)
    b = np.empty(x.shape + (3,), dtype=np.uint8)
    b[..., 0] = v & 0xFF
    b[..., 1] = (v >> 8) & 0xFF
    b[..., 2] = (v >> 16) & 0xFF
    data = b.tobytes()
    pad = len(data) & 1
    hdr = (b"RIFF" + struct.pack("<I", 36 + len(data) + pad) + b"WAVE" +
           b"fmt " + struct.pack("<IHHIIHH", 16, 1, ch, int(fs), int(fs) * ch * 3, ch * 3, 24) +
           b"data" + struct.pack("<I", len(data)))
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(data)
        if pad:
            f.write(b"\x00")


def read_wav_pcm24(path: str):
    """Inverse of :func:`write_wav_pcm24` (tests): returns (int32 samples [n, ch] in 24-bit range, fs)."""
    import wave
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 3
        ch, fs, n = w.getnchannels(), w.getframerate(), w.getnframes()
        raw = np.frombuffer(w.readframes(n), dtype=np.uint8).reshape(n, ch, 3).astype(np.int32)
    v = raw[..., 0] | (raw[..., 1] << 8) | (raw[..., 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    return v, fs
