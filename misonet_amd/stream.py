"""The causal chain from waveform block to waveform block, on the device:

    StftStream -> DereverbStream (online WPE) -> SeparateStream (online AuxIVA) -> BeamformStream (online MVDR / MWF) -> IstftStream

Every link holds its state on the device and gives bits that do not depend on how the stream is cut into calls; the two transforms
at the ends give the bits of the offline kernels (``stft_hip`` / ``istft``).  So a recording pushed through
:class:`StreamSeparator` in blocks of any size, then flushed, yields exactly what the one-shot path yields:
``stft_hip`` -> ``DereverbStream.process`` -> ``SeparateStream.process`` -> ``BeamformStream.process`` -> ``istft_int16`` over
all its frames.  The transforms cost 255 samples of latency (output sample 64 h needs input sample 64 h + 255) plus the block;
the three recursions add none.

At any sample rate: with ``fs`` (the model's rate) and ``fs_in`` / ``fs_out`` a
:class:`misonet_amd.resample.ResampleStream` sits in front of ``StftStream`` and / or behind ``IstftStream``; both give the bits of
the offline ``resample``, so the guarantee above holds for the whole chain from capture rate to playback rate.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch

from . import stft as S

__all__ = ["StreamSeparator", "separate_stream"]


class StreamSeparator:
    """``batch`` recordings of ``num_mic`` microphones, fed in waveform blocks; separated waveform blocks come back.

    dereverb   None: no dereverberation; True, an :class:`misonet_amd.dereverb.OnlineDereverb` or a dict of its fields: online
               WPE in front of the separation
    separate   True, an :class:`misonet_amd.blind.OnlineAuxIVA`, a model name or a dict of its fields (its ``ref_ch`` is replaced
               by this object's): online AuxIVA with all microphones as sources; None leaves it out, and the rows are the
               (dereverberated) microphones.  With ``num_src`` = K below ``num_mic`` (``OnlineAuxIVA(num_src=K)`` or
               ``dict(num_src=K)``) it is the overdetermined stream: it has exactly K rows, and the online
               beamformer behind it is a ``BeamformStream(num_mic, K)`` on its K images and on the spectrum it saw
    beamform   None, or an :class:`misonet_amd.beamform.OnlineBeamformer` (True or a dict of its fields are taken as well; its
               ``ref_ch`` is replaced by this object's): the online beamformer on AuxIVA's images and on the spectrum AuxIVA saw;
               needs ``separate``
    rows       the rows that go to the iSTFT, a sequence of indices in [0, num_mic) -- in [0, K) with ``num_src`` = K; default:
               all of them, in order.  The choice stays with the caller: the strongest-rows pick of
               ``BlindSeparator.separate_recording`` needs the whole recording, is not causal and is NOT offered here
    int16      True: int16 waves, ``(short)(int)(y * 32767)`` as ``istft_int16``; False: float32
    fs, fs_in, fs_out   the model's rate, the rate of the blocks that come in and the rate of the waves that go out
               (:func:`misonet_amd.resample.plan_rates`; ``fs_out="in"``: the input's rate).  ``fs`` is required with either of
               the other two.  All None: the chain at the model's rate, not one launch added.  ``fs_in``: a ``ResampleStream``
               (float32) in front; a block that completes no sample at the model's rate skips the rest of the chain.
               ``fs_out``: another behind the iSTFT, on its waves in place (int16 -> int16 when ``int16``)
    """

    latency_samples = 255

    def __init__(self, num_mic, batch=1, dereverb=None, separate=True, beamform=None, rows: Optional[Sequence[int]] = None,
                 ref_ch=0, int16=True, device=None, fs=None, fs_in=None, fs_out=None):
        M, B = int(num_mic), int(batch)
        self.num_mic, self.batch, self.ref_ch = M, B, int(ref_ch)
        if not 0 <= self.ref_ch < max(M, 1):
            raise ValueError(f"ref_ch {ref_ch} outside [0, {M})")
        sep_opts = None
        if separate is not None and separate is not False:
            from .blind import OnlineAuxIVA
            sep_opts = dataclasses.replace(OnlineAuxIVA.of(separate), ref_ch=self.ref_ch).validate(M)
        K = M if sep_opts is None else sep_opts.sources(M)       # the rows of the stream: num_src of them where that is set
        self.num_src = K
        self.rows = list(range(K)) if rows is None else [int(r) for r in rows]
        if not self.rows or any(not 0 <= r < K for r in self.rows):
            raise ValueError(f"rows must be a non-empty sequence of indices in [0, {K}), got {rows!r}")
        if beamform is not None and beamform is not False and (separate is None or separate is False):
            raise ValueError("beamform= runs on the images of the online separation: it needs separate=")
        if fs is None and (fs_in is not None or fs_out is not None):
            raise ValueError("fs_in / fs_out need fs, the rate the chain itself runs at")
        r_in = r_out = None
        if fs is not None:
            from .resample import plan_rates
            r_in, r_out, _ = plan_rates(fs, fs_in, fs_out)
        self.fs, self.fs_in, self.fs_out = (None if fs is None else int(fs)), r_in, r_out
        self.stft = S.StftStream(M, B, device=device)
        self.device = self.stft.device
        self.resample_in = self.resample_out = None
        self._trimmed = 0                                    # samples of zero padding cut from the last hop by flush(pad=True)
        if r_in is not None:
            from .resample import ResampleStream
            self.resample_in = ResampleStream(M, r_in, self.fs, batch=B, device=self.device)
        if r_out is not None:
            from .resample import ResampleStream
            self.resample_out = ResampleStream(len(self.rows), self.fs, r_out, batch=B, in_int16=bool(int16),
                                               out_int16=bool(int16), device=self.device)
        self.dereverb = self.separate = self.beamform = None
        if dereverb is not None and dereverb is not False:
            from .dereverb import DereverbStream, OnlineDereverb
            o = OnlineDereverb.of(dereverb).validate(M)
            self.dereverb = DereverbStream(M, S.N_FREQ, B, device=self.device, **dataclasses.asdict(o))
        if separate is not None and separate is not False:
            from .blind import SeparateStream
            self.separate = SeparateStream(M, S.N_FREQ, B, device=self.device, **sep_opts.as_kwargs())
        if beamform is not None and beamform is not False:
            from .beamform import BeamformStream, OnlineBeamformer
            o = dataclasses.replace(OnlineBeamformer.of(beamform), ref_ch=self.ref_ch).validate(M, K)
            self.beamform = BeamformStream(M, K, S.N_FREQ, B, device=self.device, **dataclasses.asdict(o))
        self.istft = S.IstftStream(B * len(self.rows), int16=int16, device=self.device)
        self._pick = None if self.rows == list(range(K)) else torch.tensor(self.rows, dtype=torch.long, device=self.device)

    def reset(self):
        """every link back to its first state"""
        for st in (self.resample_in, self.stft, self.dereverb, self.separate, self.beamform, self.istft, self.resample_out):
            if st is not None:
                st.reset()
        self._trimmed = 0
        return self

    @property
    def samples_seen(self) -> int:
        return self.stft.samples_seen if self.resample_in is None else self.resample_in.samples_seen

    @property
    def samples_out(self) -> int:
        return self.istft.samples_out - self._trimmed if self.resample_out is None else self.resample_out.samples_out

    @property
    def latency_seconds(self) -> float:
        """the latency of the chain without the block: ``Lh_in / (p_in fs_in) + 255 / fs + Lh_out / (p_out fs)``, each resampler's
        term where that resampler is; needs ``fs``"""
        if self.fs is None:
            raise ValueError("latency_seconds needs fs, the rate the chain runs at")
        t = self.latency_samples / self.fs
        if self.resample_in is not None:
            t += self.resample_in.latency / self.fs_in
        if self.resample_out is not None:
            t += self.resample_out.latency / self.fs
        return t

    @property
    def fail(self) -> dict:
        """the flags of the recursions that are in the chain, by name: ``{"dereverb": ..., "separate": ..., "beamform": ...}``,
        int32 tensors on the device (all zero: no stage met a frame it could not use)"""
        return {k: st.fail for k, st in (("dereverb", self.dereverb), ("separate", self.separate), ("beamform", self.beamform))
                if st is not None}

    def _frames(self, spec):
        """spec complex64 [B, M, Tn, F], Tn >= 1 -> the rows for the iSTFT [B, R, Tn, F]"""
        if self.dereverb is not None:
            spec = self.dereverb.process(spec)
        out = spec
        if self.beamform is not None:
            _est, images = self.separate.process(spec, images=True)
            out = self.beamform.process(images, spec)
        elif self.separate is not None:
            out = self.separate.process(spec)
        return out if self._pick is None else out.index_select(1, self._pick)

    def _waves(self, spec, flush):
        B, R = self.batch, len(self.rows)
        if spec.shape[2] == 0:                               # no frame completed: the recursions are not called
            if not flush:
                return torch.empty((B, R, 0), dtype=torch.int16 if self.istft.int16 else torch.float32, device=self.device)
            return self.istft.flush().reshape(B, R, -1)
        return self.istft.process(self._frames(spec).contiguous(), flush=flush).reshape(B, R, -1)

    def _empty(self):
        return torch.empty((self.batch, len(self.rows), 0), dtype=torch.int16 if self.istft.int16 else torch.float32,
                           device=self.device)

    def _to_rate_out(self, waves, flush):
        """waves [B, R, n] at the model's rate, read in place as the channel-major view [B, n, R] -> [B, R, n_out] at fs_out"""
        rs = self.resample_out
        if rs is None:
            return waves
        n = waves.shape[2]
        if n == 0 and not flush:
            return self._empty()
        out = torch.empty((self.batch, len(self.rows), rs.outputs(n, flush)), dtype=waves.dtype, device=self.device)
        rs.process_into(waves.transpose(1, 2), out.transpose(1, 2), flush)
        return out

    def process(self, block):
        """The next n >= 1 samples: float32 [B, n, M] (or [n, M] when batch == 1) on the device -> waves [B, R, 64 H], the hops
        these samples complete.  When the block completes no frame the recursions are skipped and an empty block comes back.
        With ``fs_in`` the block is at that rate; with ``fs_out`` the waves are, in whatever number these samples complete."""
        if self.resample_in is None and self.resample_out is None:
            return self._waves(self.stft.process(block), False)
        if self.resample_in is not None:
            block = self.resample_in.process(block)
            if block.shape[1] == 0:
                return self._empty()
        return self._to_rate_out(self._waves(self.stft.process(block), False), False)

    def flush(self, block=None, pad=False):
        """The end of the stream, with or without a last block: everything still owed.  In all, N samples at the model's rate give
        ``64 (N // 64)`` samples out (feed whole hops, zero-padded, to lose none: :func:`separate_stream`).  ``pad=True`` does
        that here: the stream at the model's rate is completed to a whole hop with zeros before the STFT's flush, and the chain's
        output is cut to the N samples that went in before the output resampler's flush, if there is one."""
        if self.resample_in is None and self.resample_out is None and not pad:
            return self._waves(self.stft.flush(block), True)
        if self.resample_in is not None:
            block = self.resample_in.flush(block)
        if block is not None and block.dim() == 2:
            block = block[None]
        # the samples at the model's rate that this stream has been given in all: what the chain owes once flushed
        n_model = self.stft.samples_seen + (0 if block is None else block.shape[1])
        if pad and n_model % S.HOP:
            zeros = torch.zeros((self.batch, (-n_model) % S.HOP, self.num_mic), dtype=torch.float32, device=self.device)
            block = zeros if block is None else torch.cat([block, zeros], dim=1)
        if block is not None and block.shape[1] == 0:
            block = None
        done = self.istft.samples_out
        waves = self._waves(self.stft.flush(block), True)
        if pad:
            # the iSTFT has emitted `done` samples before this call and emits whole hops now; of these only n_model - done
            # answer samples that went in, the rest answers the zeros above.  samples_out leaves them out (_trimmed)
            self._trimmed = waves.shape[2] - max(0, min(waves.shape[2], n_model - done))
            waves = waves[:, :, :waves.shape[2] - self._trimmed]
        return self._to_rate_out(waves, True)


def separate_stream(wav, block: int = 1024, **kw):
    """A whole recording through a :class:`StreamSeparator` in blocks of ``block`` samples: wav float32 [L, M] (ndarray or
    tensor) -> waves [R, L], an ndarray for an ndarray and a device tensor for a tensor.  The recording is zero-padded to whole
    hops, as ``separate_recording`` does, and the result trimmed to ``L``.  ``kw``: the arguments of :class:`StreamSeparator`
    (``num_mic`` and ``batch`` follow from ``wav``).  With ``fs`` and ``fs_in`` / ``fs_out`` among them the blocks are at ``fs_in``,
    the stream ends with ``flush(pad=True)`` and the result equals, bit for bit, ``resample`` to ``fs``, this function at ``fs``
    and ``resample`` to ``fs_out`` one after the other; where the result is back at the rate the blocks came in at
    (``fs_out="in"``, or an ``fs_out`` equal to it) it is trimmed or zero-padded to ``L``, as ``pcm_to_rate`` does."""
    shape = np.shape(wav)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"wav {tuple(shape)} must be [L, M]")
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or block < 1:
        raise ValueError(f"block must be a positive number of samples, got {block!r}")
    L, M = shape
    sep = StreamSeparator(M, 1, **kw)
    np_in = not isinstance(wav, torch.Tensor)
    sig = (torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)) if np_in else wav.to(torch.float32)).to(sep.device)
    if sep.resample_in is not None or sep.resample_out is not None:
        sig = sig[None].contiguous()
        out = [sep.process(sig[:, a:a + block]) for a in range(0, L, block)]
        out.append(sep.flush(pad=True))
        y = torch.cat(out, dim=2)[0]
        if sep.fs_out is not None and sep.fs_out == (sep.fs if sep.fs_in is None else sep.fs_in) and y.shape[1] != L:
            y = torch.nn.functional.pad(y[:, :L], (0, max(0, L - y.shape[1])))
        return np.ascontiguousarray(y.cpu().numpy()) if np_in else y.contiguous()
    sig = torch.nn.functional.pad(sig, (0, 0, 0, (-L) % S.HOP))[None].contiguous()               # [1, Lp, M]
    out = [sep.process(sig[:, a:a + block].contiguous()) for a in range(0, sig.shape[1], block)]
    out.append(sep.flush())
    y = torch.cat(out, dim=2)[0, :, :L]
    return np.ascontiguousarray(y.cpu().numpy()) if np_in else y.contiguous()
