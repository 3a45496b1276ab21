"""The causal chain from waveform block to waveform block, on the device:

    StftStream -> DereverbStream (online WPE) -> SeparateStream (online AuxIVA) -> BeamformStream (online MVDR / MWF) -> IstftStream

Every link holds its state on the device and gives bits that do not depend on how the stream is cut into calls; the two transforms
at the ends give the bits of the offline kernels (``stft_hip`` / ``istft``).  So a recording pushed through
:class:`StreamSeparator` in blocks of any size, then flushed, yields exactly what the one-shot path yields:
``stft_hip`` -> ``DereverbStream.process`` -> ``SeparateStream.process`` -> ``BeamformStream.process`` -> ``istft_int16`` over
all its frames.  The transforms cost 255 samples of latency (output sample 64 h needs input sample 64 h + 255) plus the block;
the three recursions add none.
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
               (dereverberated) microphones
    beamform   None, or an :class:`misonet_amd.beamform.OnlineBeamformer` (True or a dict of its fields are taken as well; its
               ``ref_ch`` is replaced by this object's): the online beamformer on AuxIVA's images and on the spectrum AuxIVA saw;
               needs ``separate``
    rows       the rows that go to the iSTFT, a sequence of indices in [0, num_mic); default: all of them, in order.  The choice
               stays with the caller: the strongest-rows pick of ``BlindSeparator.separate_recording`` needs the whole recording,
               is not causal and is NOT offered here
    int16      True: int16 waves, ``(short)(int)(y * 32767)`` as ``istft_int16``; False: float32
    """

    latency_samples = 255

    def __init__(self, num_mic, batch=1, dereverb=None, separate=True, beamform=None, rows: Optional[Sequence[int]] = None,
                 ref_ch=0, int16=True, device=None):
        M, B = int(num_mic), int(batch)
        self.num_mic, self.batch, self.ref_ch = M, B, int(ref_ch)
        if not 0 <= self.ref_ch < max(M, 1):
            raise ValueError(f"ref_ch {ref_ch} outside [0, {M})")
        self.rows = list(range(M)) if rows is None else [int(r) for r in rows]
        if not self.rows or any(not 0 <= r < M for r in self.rows):
            raise ValueError(f"rows must be a non-empty sequence of indices in [0, {M}), got {rows!r}")
        if beamform is not None and beamform is not False and (separate is None or separate is False):
            raise ValueError("beamform= runs on the images of the online separation: it needs separate=")
        self.stft = S.StftStream(M, B, device=device)
        self.device = self.stft.device
        self.dereverb = self.separate = self.beamform = None
        if dereverb is not None and dereverb is not False:
            from .dereverb import DereverbStream, OnlineDereverb
            o = OnlineDereverb.of(dereverb).validate(M)
            self.dereverb = DereverbStream(M, S.N_FREQ, B, device=self.device, **dataclasses.asdict(o))
        if separate is not None and separate is not False:
            from .blind import OnlineAuxIVA, SeparateStream
            o = dataclasses.replace(OnlineAuxIVA.of(separate), ref_ch=self.ref_ch).validate(M)
            self.separate = SeparateStream(M, S.N_FREQ, B, device=self.device, **dataclasses.asdict(o))
        if beamform is not None and beamform is not False:
            from .beamform import BeamformStream, OnlineBeamformer
            o = dataclasses.replace(OnlineBeamformer.of(beamform), ref_ch=self.ref_ch).validate(M, M)
            self.beamform = BeamformStream(M, M, S.N_FREQ, B, device=self.device, **dataclasses.asdict(o))
        self.istft = S.IstftStream(B * len(self.rows), int16=int16, device=self.device)
        self._pick = None if self.rows == list(range(M)) else torch.tensor(self.rows, dtype=torch.long, device=self.device)

    def reset(self):
        """every link back to its first state"""
        for st in (self.stft, self.dereverb, self.separate, self.beamform, self.istft):
            if st is not None:
                st.reset()
        return self

    @property
    def samples_seen(self) -> int:
        return self.stft.samples_seen

    @property
    def samples_out(self) -> int:
        return self.istft.samples_out

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

    def process(self, block):
        """The next n >= 1 samples: float32 [B, n, M] (or [n, M] when batch == 1) on the device -> waves [B, R, 64 H], the hops
        these samples complete.  When the block completes no frame the recursions are skipped and an empty block comes back."""
        return self._waves(self.stft.process(block), False)

    def flush(self, block=None):
        """The end of the stream, with or without a last block: everything still owed.  In all, N samples in give
        ``64 (N // 64)`` samples out (feed whole hops, zero-padded, to lose none: :func:`separate_stream`)."""
        return self._waves(self.stft.flush(block), True)


def separate_stream(wav, block: int = 1024, **kw):
    """A whole recording through a :class:`StreamSeparator` in blocks of ``block`` samples: wav float32 [L, M] (ndarray or
    tensor) -> waves [R, L], an ndarray for an ndarray and a device tensor for a tensor.  The recording is zero-padded to whole
    hops, as ``separate_recording`` does, and the result trimmed to ``L``.  ``kw``: the arguments of :class:`StreamSeparator`
    (``num_mic`` and ``batch`` follow from ``wav``)."""
    shape = np.shape(wav)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"wav {tuple(shape)} must be [L, M]")
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or block < 1:
        raise ValueError(f"block must be a positive number of samples, got {block!r}")
    L, M = shape
    sep = StreamSeparator(M, 1, **kw)
    np_in = not isinstance(wav, torch.Tensor)
    sig = (torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)) if np_in else wav.to(torch.float32)).to(sep.device)
    sig = torch.nn.functional.pad(sig, (0, 0, 0, (-L) % S.HOP))[None].contiguous()               # [1, Lp, M]
    out = [sep.process(sig[:, a:a + block].contiguous()) for a in range(0, sig.shape[1], block)]
    out.append(sep.flush())
    y = torch.cat(out, dim=2)[0, :, :L]
    return np.ascontiguousarray(y.cpu().numpy()) if np_in else y.contiguous()
