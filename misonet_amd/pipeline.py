"""On-device MISO1 -> MVDR -> MISO3 pipeline: the body of the reference's Tester_Enhance.inference
(reference tester.py:846-975) with every stage kept in HBM, plus the utterance sharding used for multi-GPU runs.

``Enhancer`` mirrors the part of ``Tester_Enhance`` that does arithmetic:
    __init__(model_sep, model, num_spks, ref_ch, ...)   tester.py:799-825
    MISO1_Inference / alignment / Apply_Beamforming / MISO3_inference   tester.py:874-939  -> ``enhance``
    ISTFT + int16 + gap trim + chunk concat                               tester.py:949-969  -> ``to_wav_int16``
Unlike the reference it is correct for batch > 1 (the reference broadcasts the last batch row, tester.py:1065):
every utterance of the batch gets its own alignment, i.e. results equal the reference run utterance by utterance.

Multi-GPU: utterances are independent, so the batch is block-split over ranks with no collective on the data
path; ``gather_outputs`` is the optional all_gather of the results (RCCL on GPUs, gloo in the CPU tests).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import weakref
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import stft as S
from .beamform import Beamformer, JointBeamformer
from .dereverb import Dereverb, OnlineDereverb, dereverb_wav
from .model import MISO_1, MISO_3
from .refine import Refine, refined_images
from .weights import N_FREQ


def shard_range(n_items: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block split of ``n_items`` utterances: rank r owns [lo, hi).
    The first ``n_items % world`` ranks get one extra item."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError("bad rank/world")
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_outputs(local: torch.Tensor, n_items: int, group=None) -> torch.Tensor:
    """all_gather of per-rank results (first dim = utterances of this rank's shard) back into global order."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    sizes = [shard_range(n_items, r, world) for r in range(world)]
    cap = max(hi - lo for lo, hi in sizes)
    pad = torch.zeros((cap,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    if pad.is_complex():
        bufs = [torch.empty_like(torch.view_as_real(pad)) for _ in range(world)]
        dist.all_gather(bufs, torch.view_as_real(pad).contiguous(), group=group)
        bufs = [torch.view_as_complex(b) for b in bufs]
    else:
        bufs = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(bufs, pad, group=group)
    return torch.cat([b[: hi - lo] for b, (lo, hi) in zip(bufs, sizes)], dim=0)


def run_sharded(process: Callable[[int, int], torch.Tensor], n_items: int, rank: int, world: int, gather: bool,
                group=None):
    """Run ``process(lo, hi)`` on this rank's shard; optionally gather every rank's result in global order."""
    lo, hi = shard_range(n_items, rank, world)
    local = process(lo, hi)
    if gather and world > 1:
        return gather_outputs(local, n_items, group)
    return local


class CapturedPass:
    """One :meth:`Enhancer.enhance` pass captured in a HIP graph, together with everything the graph's kernels point at.

    The graph bakes raw device addresses (workspace, inputs, result), so this object OWNS references to all of them: the
    workspace stays alive for as long as the graph does, whatever other batch sizes / lengths / precision modes the
    Enhancer is used with in between (its own cache may drop and re-allocate workspaces freely).  ``replay()`` re-runs the
    pass; new inputs are copied INTO ``mix`` / ``clean`` first (``load``).  Unpacks as ``(graph, out)``."""

    def __init__(self, graph, out, ws, mix, clean, key, owner=None):
        self.graph, self.out, self.mix, self.clean = graph, out, mix, clean
        self._ws, self.key = ws, key
        # a STRONG reference: the graph's kernels read the Enhancer's pipeline handle and the nets' device weights, so they must
        # outlive the graph -- and check() must stay usable for as long as replay() is (the Enhancer keeps only a WeakSet of its
        # captured passes: no cycle)
        self._owner = owner

    def check(self):
        """Synchronise and raise FloatingPointError if the last replay produced a NaN (the pass's flag word lives in the
        workspace this object owns, not in the Enhancer's eager workspace)."""
        if self._owner is None:
            raise RuntimeError("this pass was captured without an owning Enhancer")
        self._owner.check(self.key[0], self.key[1], captured=self)

    def load(self, mix, clean=None):
        self.mix.copy_(mix)
        if self.clean is not None and clean is not None:
            self.clean.copy_(clean)

    def replay(self):
        self.graph.replay()
        return self.out

    def __iter__(self):                       # ``g, out = enh.capture_graph(...)``
        yield self
        yield self.out


class _Overlapped:
    """The stream and event discipline of :meth:`Enhancer.stream_wav`, for any pass: the H2D copies of a batch's inputs on a
    copy-in stream, the pass on the CURRENT stream, the D2H copy of its result and of the pipeline's NaN flag word on a
    copy-out stream, ``depth`` slots of device input / pinned output buffers (batch i uses slot i % depth).  The caller
    keeps at most ``depth`` batches in flight: :meth:`finish` of batch i - depth comes before :meth:`submit` of batch i."""

    def __init__(self, dev, depth: int):
        self.dev, self.depth = dev, max(1, int(depth))
        self.s_in, self.s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        self.slots = [dict() for _ in range(self.depth)]

    @staticmethod
    def _staged(sl, name, host, dtype):
        """pinned source for the H2D copy of `host` (itself if already pinned, or already on a device)"""
        host = host.to(dtype).contiguous() if host.dtype != dtype or not host.is_contiguous() else host
        if host.is_cuda or host.is_pinned():
            return host
        pin = sl.get("pin_" + name)
        if pin is None or pin.shape != host.shape:
            pin = sl["pin_" + name] = torch.empty(host.shape, dtype=dtype, pin_memory=True)
        elif "ev_in" in sl:
            sl["ev_in"].synchronize()                 # the previous H2D out of this staging buffer is done
        pin.copy_(host)
        return pin

    def submit(self, i: int, inputs, compute, dtype=torch.float32, to_host: bool = True):
        """Queue batch ``i``: ``inputs`` is a sequence of tensors (host, pinned or device) or None; ``compute(*device
        inputs)`` enqueues the pass on the current stream and returns ``(result, flag)`` (flag: the int32 NaN flag word,
        a device copy).  ``to_host``: the result (a device tensor) goes back through a pinned slot buffer; otherwise it
        stays on the device (any object).  Returns the record :meth:`finish` takes."""
        dev = self.dev
        s_in, s_out = self.s_in, self.s_out
        sl = self.slots[i % self.depth]
        cur = torch.cuda.current_stream(dev)          # the consumer may have changed streams between two next() calls
        srcs = [self._staged(sl, str(j), x, dtype) if x is not None else None for j, x in enumerate(inputs)]
        fresh = False
        for j, src in enumerate(srcs):
            if src is not None and (sl.get(f"d{j}") is None or sl[f"d{j}"].shape != src.shape):
                sl[f"d{j}"] = torch.empty(src.shape, dtype=dtype, device=dev)
                fresh = True
        if any(src is not None and src.is_cuda for src in srcs):
            s_in.wait_stream(cur)                     # a device-resident input: after its producer on the current stream
        if fresh:
            # a new slot buffer comes out of the CURRENT stream's allocator pool: its block may be one that work
            # already queued on the current stream still writes (e.g. the previous batch's spectrogram, freed on the
            # host the moment its iSTFT was enqueued).  The copy-in stream must not touch it before that work is
            # done.  (Found when the iSTFT became a HIP kernel: torch.istft synchronises the host, which had hidden it.)
            s_in.wait_stream(cur)
        with torch.cuda.stream(s_in):
            if "ev_free" in sl:
                s_in.wait_event(sl["ev_free"])        # the pass that read this slot's device buffers is done
            for j, src in enumerate(srcs):
                if src is not None:
                    sl[f"d{j}"].copy_(src, non_blocking=True)
            # device-resident inputs are read by the copy-in stream: the caching allocator must not hand their blocks out
            # on the current stream before that copy is done, whatever the caller does with them after next() returns
            for src in srcs:
                if src is not None and src.is_cuda:
                    src.record_stream(s_in)
            sl["ev_in"] = torch.cuda.Event()
            sl["ev_in"].record(s_in)
        cur.wait_event(sl["ev_in"])
        res, flag, *more = compute(*[sl[f"d{j}"] if src is not None else None for j, src in enumerate(srcs)])
        extra = more[0] if more else None             # a small device tensor that rides the result's D2H (the score sums)
        sl["ev_free"] = torch.cuda.Event()
        sl["ev_free"].record(cur)
        rec = {"pcm_h": sl.get("pcm_h") if to_host else None, "flag_h": sl.get("flag_h"), "res": None if to_host else res}
        if to_host and (rec["pcm_h"] is None or rec["pcm_h"].shape != res.shape or rec["pcm_h"].dtype != res.dtype):
            rec["pcm_h"] = sl["pcm_h"] = torch.empty(res.shape, dtype=res.dtype, pin_memory=True)
        if rec["flag_h"] is None:
            rec["flag_h"] = sl["flag_h"] = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        with torch.cuda.stream(s_out):
            s_out.wait_event(sl["ev_free"])
            if to_host:
                rec["pcm_h"].copy_(res, non_blocking=True)
                res.record_stream(s_out)
            rec["flag_h"].copy_(flag, non_blocking=True)
            flag.record_stream(s_out)
            if extra is not None:
                ex = sl.get("extra_h")
                if ex is None or ex.shape != extra.shape or ex.dtype != extra.dtype:
                    ex = sl["extra_h"] = torch.empty(extra.shape, dtype=extra.dtype, pin_memory=True)
                ex.copy_(extra, non_blocking=True)
                extra.record_stream(s_out)
                rec["extra_h"] = ex
            rec["ev_out"] = torch.cuda.Event()
            rec["ev_out"].record(s_out)
        return rec

    @staticmethod
    def finish(rec):
        """Wait for a batch's D2H; returns (result: an ndarray copy of the pinned buffer, or the device object; NaN flag)"""
        rec["ev_out"].synchronize()
        res = rec["pcm_h"].numpy().copy() if rec["pcm_h"] is not None else rec["res"]
        return res, int(rec["flag_h"][0]) != 0

    @staticmethod
    def extra(rec):
        """after :meth:`finish`: an ndarray copy of the extra block the batch's compute returned, or None"""
        return rec["extra_h"].numpy().copy() if rec.get("extra_h") is not None else None


class Enhancer:
    """Fused on-device MISO1 -> (alignment) -> beamformer (MVDR unless another is set) -> MISO3 for batches of 4 s chunks."""

    def __init__(self, model_sep: MISO_1, model: Optional[MISO_3], num_spks: int = 2, ref_ch: int = 0, epsi: float = 1e-6,
                 beamformer=None, dereverb=None, refine=None):
        """``model = None``: a separation-only Enhancer (:meth:`separate`, :meth:`beamform_utterance`,
        :meth:`beamform_chunks` -- what the reference's ``Tester_Beamforming`` needs: it has no MISO_3, tester.py:259-262).
        ``beamformer``: None (the reference's MVDR), a :class:`misonet_amd.beamform.Beamformer` or a dict of its fields, or a
        :class:`misonet_amd.beamform.JointBeamformer` instance (one joint solve for all speakers); it reaches the fused pass and
        every ``beamform_*`` method (:meth:`set_beamformer`).
        ``dereverb``: None (no dereverberation), True, a :class:`misonet_amd.dereverb.Dereverb` or a dict of its fields, or a
        :class:`misonet_amd.dereverb.OnlineDereverb` instance:
        the recording paths dereverberate the observation first (:meth:`set_dereverb`).
        ``refine``: None (off), True, a :class:`misonet_amd.refine.Refine` or a dict of its fields: guided spatial clustering
        between the separation and the beamformer (:meth:`set_refine`)."""
        if not isinstance(model_sep, MISO_1) or not (model is None or isinstance(model, MISO_3)):
            raise TypeError("Enhancer needs misonet_amd.MISO_1 and misonet_amd.MISO_3 (or None) instances")
        self.model_sep, self.model = model_sep, model
        self.num_spks, self.ref_ch, self.num_ch = int(num_spks), int(ref_ch), model_sep.num_ch
        if model_sep._device is None:
            model_sep.cuda()
        if model is not None and model._device is None:
            model.cuda(model_sep._device)
        self.device = model_sep._device
        if model is not None and model._device != self.device:
            raise RuntimeError(f"MISO_1 is on {self.device} but MISO_3 on {model._device}")
        model_sep._commit()
        if model is not None:
            model._commit()
        self._pipe = C.c_void_p()
        _lib.check(_lib.lib().misonet_pipeline_create(model_sep._net, model._net if model is not None else None, self.num_ch,
                                                      self.num_spks, self.ref_ch, float(epsi), C.byref(self._pipe)))
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._captured = weakref.WeakSet()     # live CapturedPass objects: check(B, T) must not silently look elsewhere
        self._epsi = float(epsi)
        self.beamformer = Beamformer()
        if beamformer is not None:
            self.set_beamformer(beamformer)
        self.dereverb = None
        if dereverb is not None:
            self.set_dereverb(dereverb)
        self.refine = None
        if refine is not None:
            self.set_refine(refine)

    def set_dereverb(self, dereverb=None):
        """WPE dereverberation in front of the recording paths (:meth:`enhance_recording`, :meth:`enhance_recordings`,
        :meth:`enhance_continuous`): None (off, the default: the existing path, no extra launch), True (the defaults), a
        :class:`misonet_amd.dereverb.Dereverb` or a dict of its fields, or a :class:`misonet_amd.dereverb.OnlineDereverb`
        INSTANCE (the frame-recursive form, ``dereverb_wav(online=...)``).  When set, the selected microphones of the whole
        recording go through :func:`misonet_amd.dereverb.dereverb_wav` on the device before they are cut into chunks or
        windows; everything downstream is untouched, and with ``score=True`` the mixture baseline (SI-SDRi, BSS-eval, STOI)
        stays the ORIGINAL observation at ``ref_ch``.  :meth:`enhance`, the ``beamform_*`` methods and the loader-driven
        :meth:`inference` receive ready spectrograms and are not changed: put ``dereverb(mix)`` in front of them.  Legal
        between passes; ValueError for a bad field."""
        if isinstance(dereverb, OnlineDereverb):
            self.dereverb = dereverb.validate(self.num_ch)
            return
        self.dereverb = None if dereverb is None or dereverb is False else Dereverb.of(dereverb).validate(self.num_ch)

    def _observe(self, obs):
        """the selected microphones of one recording, float32 [L, M], as the networks will see them"""
        if self.dereverb is None:
            return obs
        if isinstance(self.dereverb, OnlineDereverb):
            return dereverb_wav(np.ascontiguousarray(obs), device=self.device, online=self.dereverb)
        return dereverb_wav(np.ascontiguousarray(obs), device=self.device, **dataclasses.asdict(self.dereverb))

    def set_beamformer(self, beamformer=None):
        """Select the beamformer of the fused pass (:meth:`enhance` and everything built on it) and of
        :meth:`beamform_chunks` / :meth:`beamform_utterance`: None (back to the reference's MVDR), a Beamformer or a dict of
        its fields.  ``epsi`` left unset keeps each call's own default (the constructor's ``epsi`` in the fused pass).  Legal
        between passes; ValueError for a bad field.  A captured pass keeps the options it was captured with, so the change is
        refused while one is alive.  A :class:`JointBeamformer` INSTANCE selects a joint multi-speaker beamformer (LCMV, SDW-MWF,
        rank-1 MWF: one solve per bin for all speakers) as that step; a kind name or a dict always means Beamformer."""
        if isinstance(beamformer, JointBeamformer):
            bf = beamformer.validate(self.num_ch, self.num_spks)
        else:
            bf = Beamformer.of(beamformer).validate(self.num_ch)
        if bf == self.beamformer:
            return
        if len(self._captured):
            raise RuntimeError("set_beamformer: a captured pass of this Enhancer is alive and would go on replaying the old "
                               "beamformer; drop it and capture again after the change")
        L = _lib.lib()
        if isinstance(bf, JointBeamformer):    # the per-speaker options that are set stay behind it, for the way back
            jopts = bf.c_opts()
            _lib.check(L.misonet_pipeline_set_joint(self._pipe, C.byref(jopts)))
            self.beamformer = bf
            self._ws.clear()
            return
        _lib.check(L.misonet_pipeline_set_joint(self._pipe, None))
        if bf.kind == "wpd":                   # the convolutional beamformer has options and an entry point of its own
            wopts = bf.wpd_opts()
            _lib.check(L.misonet_pipeline_set_wpd(self._pipe, C.byref(wopts)))
        else:
            opts = bf.c_opts(self._epsi)
            _lib.check(L.misonet_pipeline_set_beamformer(self._pipe, C.byref(opts)))
            _lib.check(L.misonet_pipeline_set_wpd(self._pipe, None))
        self.beamformer = bf
        self._ws.clear()                       # the workspace size depends on the kind

    def set_refine(self, refine=None):
        """Guided spatial clustering (cACGMM, :mod:`misonet_amd.refine`) between the separation and the beamformer: None or
        False (off, the default: every path and the workspace as without it), True (the defaults), a Refine or a dict of its
        fields.  When set, the initial masks come from the aligned MISO1 estimates and the mixture, and the refined source
        images ``gamma_s * Y`` are the source estimate of whichever beamformer is set -- in the fused pass (:meth:`enhance`
        and everything built on it: the recording and continuous paths, captured graphs) and in :meth:`beamform_chunks` /
        :meth:`beamform_utterance` (there one clustering over the whole recording's frames).  MISO3's third input and the
        ``miso1`` output stay the raw MISO1 estimate.  Legal between passes; ValueError for a bad field; refused while a
        captured pass is alive, as :meth:`set_beamformer`."""
        rf = None if refine is None or refine is False else Refine.of(refine).validate(self.num_ch, self.num_spks)
        if rf == self.refine:
            return
        if len(self._captured):
            raise RuntimeError("set_refine: a captured pass of this Enhancer is alive and would go on replaying the old "
                               "options; drop it and capture again after the change")
        opts = rf.c_opts() if rf is not None else None
        _lib.check(_lib.lib().misonet_pipeline_set_refine(self._pipe, C.byref(opts) if opts is not None else None))
        self.refine = rf
        self._ws.clear()                       # the workspace grows while it is set

    def _bf(self, beamformer, epsi):
        """the options of one beamform_* call: its own ``beamformer`` (None: the Enhancer's) and ``epsi`` (None: the
        options', else the reference's 1e-6)"""
        if isinstance(beamformer, JointBeamformer):
            return beamformer.validate(self.num_ch, self.num_spks)
        bf = self.beamformer if beamformer is None else Beamformer.of(beamformer).validate(self.num_ch)
        if isinstance(bf, JointBeamformer):    # the joint kinds have no epsi
            return bf
        return bf if epsi is None else dataclasses.replace(bf, epsi=float(epsi))

    def __del__(self):
        try:
            if self._pipe:
                _lib.lib().misonet_pipeline_destroy(self._pipe)
                self._pipe = C.c_void_p()
        except Exception:
            pass

    def _ready(self):
        """Re-commit after a later ``load_state_dict`` / ``.cuda()`` on either model (a checkpoint loaded after the
        Enhancer was built clears the committed state) and follow a device move."""
        if self.model is not None and self.model_sep._device != self.model._device:
            raise RuntimeError(f"MISO_1 is on {self.model_sep._device} but MISO_3 on {self.model._device}")
        if self.model_sep._device != self.device:
            self.device = self.model_sep._device
            self._ws.clear()
        self.model_sep._commit()
        if self.model is not None:
            self.model._commit()

    def _check_c64(self, x, name, shape=None):
        """shared argument check of enhance / separate: complex tensor on this Enhancer's device, optional shape"""
        if not isinstance(x, torch.Tensor) or not x.is_complex():
            raise TypeError(f"{name} must be a complex torch tensor")
        if x.device != self.device:
            raise RuntimeError(f"Expected all tensors to be on the same device, but found {name} on {x.device} and the "
                               f"models on {self.device}")
        if shape is not None and tuple(x.shape) != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)}, got {list(x.shape)}")
        return x.to(torch.complex64).contiguous()

    def _ws_key(self, B, T):
        # the layout depends on the arithmetic modes and on whether buffers may share memory
        m3 = self.model
        return (B, T, self.model_sep.precision, m3.precision if m3 is not None else None, self.model_sep._keep,
                m3._keep if m3 is not None else None, self.beamformer.kind, self.refine is not None)

    def workspace(self, B, T):
        key = self._ws_key(B, T)
        ws = self._ws.get(key)
        if ws is None:
            self._ws.clear()
            n = _lib.lib().misonet_pipeline_workspace_bytes(self._pipe, B, T)
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            ws[:16].zero_()                    # the NaN flag word: check() on a workspace no pass has run in reads "clean"
            self._ws[key] = ws
        return ws

    def enhance(self, mix: torch.Tensor, clean: Optional[torch.Tensor] = None, want_bf=False, want_miso1=False,
                check_nan=True, out: Optional[torch.Tensor] = None):
        """mix complex [B,M,T,F] (device); clean complex [B,S,T,F] = clean sources at ref_ch (tester.py:889-891) or
        None to skip the clean-reference re-ordering.  Returns MISO3 output complex64 [B,S,T,F]
        (and a dict with 'bf' [B,S,T,F] / 'miso1' [B,S,M,T,F] when requested)."""
        self._ready()
        if self.model is None:
            raise RuntimeError("this Enhancer was built without MISO_3 (separation only): use separate() / beamform_*()")
        if not isinstance(mix, torch.Tensor) or mix.dim() != 4:
            raise ValueError("mix must be a 4-D complex tensor [B, M, T, F]")
        mix = self._check_c64(mix, "mix")
        B, M, T, F = mix.shape
        if M != self.num_ch:
            raise ValueError(f"expected {self.num_ch} microphones, got {M}")
        if F != N_FREQ:
            raise ValueError(f"the networks are defined for F = {N_FREQ} frequency bins, got {F}")
        if T < 2:                              # as the reference: InstanceNorm over one element (model.py:89, 413)
            raise ValueError(f"Expected more than 1 spatial element when training, got T = {T} frame(s)")
        if clean is not None:
            clean = self._check_c64(clean, "clean", (B, self.num_spks, T, F))
        ws = self.workspace(B, T)
        if out is None:
            out = torch.empty((B, self.num_spks, T, F), dtype=torch.complex64, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.complex64 or out.device != self.device
              or tuple(out.shape) != (B, self.num_spks, T, F) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous complex64 tensor [{B}, {self.num_spks}, {T}, {F}] on {self.device}")
        bf = torch.empty_like(out) if want_bf else None
        m1 = torch.empty((B, self.num_spks, M, T, F), dtype=torch.complex64, device=self.device) if want_miso1 else None
        L = _lib.lib()
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            _lib.check(L.misonet_pipeline_run(self._pipe, mix.data_ptr(), clean.data_ptr() if clean is not None else None,
                                              B, T, out.data_ptr(), bf.data_ptr() if want_bf else None,
                                              m1.data_ptr() if want_miso1 else None, ws.data_ptr(), ws.numel(), st))
            if check_nan:
                _lib.check(L.misonet_pipeline_check(self._pipe, ws.data_ptr(), st))
        if want_bf or want_miso1:
            return out, dict(bf=bf, miso1=m1)
        return out

    def capture_graph(self, mix: torch.Tensor, clean: Optional[torch.Tensor] = None) -> CapturedPass:
        """Capture one :meth:`enhance` pass over the given (static) input tensors into a HIP graph and return a
        :class:`CapturedPass` (unpacks as ``(graph, out)``): ``graph.replay()`` re-runs the ≈ 450 kernel launches of the
        pass with one host call and leaves the result in ``out``; new inputs are copied INTO ``mix`` / ``clean`` before a
        replay.  Every entry point of the C ABI is asynchronous on the caller's stream and allocates nothing, so the whole
        pass is capturable.  The graph holds raw addresses: ``mix`` / ``clean`` must ALREADY be contiguous complex64
        device tensors (a converted copy would be what the graph reads, not the caller's tensor), and the returned object
        keeps the workspace, the inputs and the result alive -- the Enhancer's own workspace cache may be re-used for other
        shapes / modes meanwhile.  NaN checking is the caller's (``misonet_pipeline_check`` synchronises, so it is not part
        of the graph): call ``captured.check()`` (or ``enh.check(B, T, captured=captured)``) after a replay -- the flag word
        lives in the workspace the CapturedPass owns; ``enh.check(B, T)`` without it refuses to answer while a captured pass
        of that shape is alive (it would read the eager workspace, which a replay never touches)."""
        self._ready()
        for name, x in (("mix", mix), ("clean", clean)):
            if x is None:
                continue
            if (not isinstance(x, torch.Tensor) or x.dtype != torch.complex64 or not x.is_contiguous()
                    or x.device != self.device):
                raise ValueError(f"capture_graph: {name} must be a contiguous complex64 tensor on {self.device} (the graph "
                                 "records its address)")
        B, M, T, F = mix.shape
        out = torch.empty((B, self.num_spks, T, F), dtype=torch.complex64, device=self.device)
        self.enhance(mix, clean, check_nan=False, out=out)               # warm-up: workspace allocation, lazy init
        torch.cuda.synchronize(self.device)
        key = self._ws_key(B, T)
        ws = self._ws[key]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.device(self.device), torch.cuda.graph(g):
            self.enhance(mix, clean, check_nan=False, out=out)
        if self._ws.get(key) is not ws:                                  # (cannot happen: same key as the warm-up)
            raise RuntimeError("workspace changed during capture")
        # from now on this workspace belongs to the graph: the cache hands out a fresh one for the same key, so an eager
        # pass between two replays cannot clobber activations a replay is about to read
        del self._ws[key]
        cp = CapturedPass(g, out, ws, mix, clean, key, owner=self)
        self._captured.add(cp)
        return cp

    def check(self, B: int, T: int, captured: Optional[CapturedPass] = None):
        """Synchronise and raise FloatingPointError if the last pass on the (B, T) workspace produced a NaN
        (``captured``: the workspace of that captured pass instead of the eager one)."""
        if captured is None:
            key = self._ws_key(B, T)
            live = [c for c in self._captured if c.key == key]
            if live and key not in self._ws:
                # after capture_graph the (B, T) workspace belongs to the graph; a fresh eager workspace always reads
                # clean, so `g.replay(); enh.check(B, T)` would silently check nothing
                raise RuntimeError(f"check({B}, {T}): a captured pass owns the workspace of this shape and no eager pass has run "
                                   "since; call captured.check() / check(B, T, captured=...) for the replay's NaN flag")
        ws = captured._ws if captured is not None else self.workspace(B, T)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().misonet_pipeline_check(self._pipe, ws.data_ptr(), _lib.stream_ptr(self.device)))

    def enhance_wav(self, wav: torch.Tensor, clean_wav: Optional[torch.Tensor] = None, want_bf=False, want_miso1=False,
                    check_nan=True):
        """Waveform entry: wav float32 [B, n_samples, M] on the device (one 4 s chunk per row,
        time-major as ``librosa.load(...).T``), clean_wav float32 [B, n_samples, S] = the clean sources at ref_ch, or
        None.  The STFT front-end runs as a HIP kernel straight into the network's layout; returns what
        :meth:`enhance` returns (T = n_samples // 64 + 1 frames)."""
        self._ready()
        if self.model is None:
            raise RuntimeError("this Enhancer was built without MISO_3 (separation only): use separate() / beamform_*()")
        if not isinstance(wav, torch.Tensor) or wav.dim() != 3 or wav.is_complex():
            raise ValueError("wav must be a real 3-D tensor [B, n_samples, M]")
        if wav.device != self.device:
            raise RuntimeError(f"Expected all tensors to be on the same device, but found wav on {wav.device} and the "
                               f"models on {self.device}")
        wav = wav.to(torch.float32).contiguous()
        B, Ls, M = wav.shape
        if M != self.num_ch:
            raise ValueError(f"expected {self.num_ch} microphones, got {M}")
        if clean_wav is not None:
            if not isinstance(clean_wav, torch.Tensor) or clean_wav.device != self.device:
                raise RuntimeError(f"clean_wav must be a tensor on {self.device}")
            clean_wav = clean_wav.to(torch.float32).contiguous()
            if tuple(clean_wav.shape) != (B, Ls, self.num_spks):
                raise ValueError("clean_wav must be [B, n_samples, num_spks]")
        L = _lib.lib()
        T = L.misonet_stft_frames(Ls)
        if T < 2:                              # n_samples < 64: one frame -- the reference's instance norms raise (model.py:89, 413)
            raise ValueError(f"Expected more than 1 spatial element when training, got T = {T} frame(s) ({Ls} samples)")
        ws = self.workspace(B, T)
        out = torch.empty((B, self.num_spks, T, 129), dtype=torch.complex64, device=self.device)
        bf = torch.empty_like(out) if want_bf else None
        m1 = torch.empty((B, self.num_spks, M, T, 129), dtype=torch.complex64, device=self.device) if want_miso1 else None
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            _lib.check(L.misonet_pipeline_run_wav(self._pipe, wav.data_ptr(),
                                                  clean_wav.data_ptr() if clean_wav is not None else None, B, Ls,
                                                  out.data_ptr(), bf.data_ptr() if want_bf else None,
                                                  m1.data_ptr() if want_miso1 else None, ws.data_ptr(), ws.numel(), st))
            if check_nan:
                _lib.check(L.misonet_pipeline_check(self._pipe, ws.data_ptr(), st))
        if want_bf or want_miso1:
            return out, dict(bf=bf, miso1=m1)
        return out

    def enhance_wav_int16(self, wav: torch.Tensor, clean_wav: Optional[torch.Tensor] = None, check_nan=True) -> torch.Tensor:
        """The reference's unit of work on the device: wav in -> int16 wav out (tester.py:865-867 H2D ... 949-952 iSTFT,
        x 32767, int16).  wav float32 [B, n_samples, M] (device) -> int16 [B, S, 64 * (n_samples // 64)] (device; = n_samples
        when that is a multiple of the hop, as the reference's 4 s chunks are): HIP STFT front-end,
        the fused pipeline, ONE ``istft_k`` launch over the B * S enhanced spectrograms incl. the truncating cast --
        nothing leaves the device and nothing synchronises (with ``check_nan=False``)."""
        return S.istft_int16(self.enhance_wav(wav, clean_wav, check_nan=check_nan))

    def stream_wav(self, batches, depth: int = 2, check_nan: bool = True, score: bool = False):
        """HOST-resident batches in, int16 waves out, copies overlapped with compute.

        ``score=True``: ``batches`` yields ``(wav, clean_wav, n_valid)`` (n_valid: B ints, the samples of each chunk that
        count; None = all; a fourth element, float32 [B, n_samples, 1], replaces the observation at ``ref_ch`` as the
        mixture of the baseline) and the generator yields ``(pcm, (stats float64 [B, S, S, 5], stats_mix float64 [B, S, 5]))``: the
        sums of :func:`score.wave_stats` of the int16 result (and of the observation at ``ref_ch``) against ``clean_wav``,
        launched on the compute stream right behind the iSTFT; the block travels with the result's D2H.

        ``batches`` yields ``wav`` or ``(wav, clean_wav)``: CPU float32 tensors [B, n_samples, M] / [B, n_samples, S] (pinned
        or not; un-pinned ones are staged through a pinned buffer of this generator).  For every batch, in order, yields
        int16 ndarray [B, S, n_samples].  Three streams: H2D copies of batch i + 1 (copy-in stream) and the D2H copy of
        batch i - 1's int16 result (copy-out stream) run beside the pipeline of batch i (current stream); ``depth`` device
        input / pinned output slots.  The host only blocks on the result of the OLDEST batch in flight, so the GPU always
        has the next batch queued.  A NaN in batch i raises FloatingPointError when that batch is handed out (the
        pipeline's flag word travels with the result instead of a synchronising check).

        Contracts: the compute stream is whatever stream is CURRENT when the generator resumes for a batch
        (re-read every iteration; the events that protect the slot buffers are recorded on and waited by that stream).  A
        PINNED input is the direct source of an asynchronous H2D copy: leave it untouched until the result of ITS batch has
        been yielded (un-pinned inputs are copied into the generator's own staging buffer before ``next()`` returns).  A
        CUDA-resident input is read on the copy-in stream after the work queued on the stream that was current when it
        was handed over."""
        import collections
        self._ready()
        dev = self.device
        depth = max(1, int(depth))
        with torch.cuda.device(dev):
            ov = _Overlapped(dev, depth)
            pending = collections.deque()

            def finish(rec):
                pcm, nan = ov.finish(rec)
                if check_nan and nan:
                    raise FloatingPointError("libmisonet_hip: NaN in pipeline output")
                if score:
                    return pcm, self._score_rows(ov.extra(rec), pcm.shape[0], False)
                return pcm

            for i, item in enumerate(batches):
                while len(pending) >= depth:                  # slot i % depth still belongs to batch i - depth
                    yield finish(pending.popleft())
                if score:
                    wav_h, clean_h, nv, *mix_ref = item          # mix_ref: the observation the baseline is taken from
                    if clean_h is None:
                        raise ValueError("score=True needs the clean sources of every batch")
                    nv = [wav_h.shape[1]] * wav_h.shape[0] if nv is None else nv
                    pending.append(ov.submit(i, (wav_h, clean_h, self._nv_bits(nv, torch.float32), *mix_ref),
                                             self._wav_pass_score))
                    continue
                wav_h, clean_h = item if isinstance(item, (tuple, list)) else (item, None)
                pending.append(ov.submit(i, (wav_h, clean_h), self._wav_pass))
            while pending:
                yield finish(pending.popleft())

    def _wav_pass(self, wav, clean_wav):
        """one stream_wav batch on the current stream: int16 waves and a copy of the pass's NaN flag word (ws[0])"""
        pcm = self.enhance_wav_int16(wav, clean_wav, check_nan=False)
        B, Ls, _ = wav.shape
        T = _lib.lib().misonet_stft_frames(Ls)
        return pcm, self.workspace(B, T)[:4].view(torch.int32).clone()

    # ---- scoring beside the pass (score.py, csrc/score.hip) ----------------------------------------------------------
    # The per-chunk valid counts reach the device as one more staged input of the batch: int32 bit patterns in a tensor of
    # the batch's dtype (one element per chunk), copied bit for bit by the H2D copies.
    @staticmethod
    def _nv_bits(n_valid, dtype):
        nv = np.asarray(n_valid, dtype=np.int32).reshape(-1, 1)
        if dtype == torch.complex64:
            nv = np.concatenate([nv, np.zeros_like(nv)], axis=1)
        return torch.from_numpy(np.ascontiguousarray(nv)).view(dtype).reshape(-1, 1)

    @staticmethod
    def _nv_dev(nv):
        """the staged bits [N, 1] back as contiguous int32 [N] on the device"""
        v = nv.view(torch.int32).reshape(nv.shape[0], -1)
        return v[:, 0].contiguous()

    def _score_rows(self, ex, N, spec):
        """the flat float64 block of a scored batch of N chunks -> per chunk (stats [S, S, 5], stats_mix [S, 5]) and, for
        ``spec``, also (pair of the output [S, S], pair of the MISO1 estimate at ref_ch [S, S], its uPIT value)"""
        Sp = self.num_spks
        a, b = N * Sp * Sp * 5, N * Sp * 5
        st, sm = ex[:a].reshape(N, Sp, Sp, 5), ex[a:a + b].reshape(N, Sp, 5)
        if not spec:
            return st, sm
        c = N * Sp * Sp
        o = a + b
        return st, sm, ex[o:o + c].reshape(N, Sp, Sp), ex[o + c:o + 2 * c].reshape(N, Sp, Sp), ex[o + 2 * c:o + 2 * c + N]

    def _wav_pass_score(self, wav, clean_wav, nv, mix_ref=None):
        """:meth:`_wav_pass` and, right behind its iSTFT on the same stream, the sums of the int16 waves and of the
        observation at ref_ch against the clean waves (read in place from the time-major inputs).  ``mix_ref`` [B, n, 1]:
        the observation at ref_ch when ``wav`` is not it (a dereverberated recording)"""
        from . import score as SC
        pcm, flag = self._wav_pass(wav, clean_wav)
        n = pcm.shape[2]
        nvd = self._nv_dev(nv)
        ref = clean_wav.transpose(1, 2)[:, :, :n]
        st = SC.wave_stats(pcm, ref, nvd)
        mix = wav[:, :n, self.ref_ch:self.ref_ch + 1] if mix_ref is None else mix_ref[:, :n]
        sm = SC.wave_stats(mix.transpose(1, 2), ref, nvd)
        return pcm, flag, torch.cat((st.reshape(-1), sm.reshape(-1)))

    def _spec_pass_score(self, mix, clean, nv):
        """:meth:`_spec_pass` with scores: the loader carries spectrograms, so the reference waves are the device iSTFT
        (float32) of the clean spectrograms and of the observation at ref_ch; the spectral criterion of the output
        (loss_Enhance) and of the MISO1 estimate at ref_ch (loss_uPIT) is taken from the spectrograms themselves"""
        from . import score as SC
        N, _, T, _ = mix.shape
        Sp = self.num_spks
        out, aux = self.enhance(mix, clean, want_miso1=True, check_nan=False)
        pcm = S.istft_int16(out)                                                             # [N, S, (T - 1) * 64]
        refw = S._istft_hip(torch.cat((clean, mix[:, self.ref_ch:self.ref_ch + 1]), dim=1), False)   # [N, S + 1, n]
        nvd = self._nv_dev(nv)
        st = SC.wave_stats(pcm, refw[:, :Sp], nvd)
        sm = SC.wave_stats(refw[:, Sp:], refw[:, :Sp], nvd)
        pair_o, _ = SC.spec_pairs(out, clean)
        pair_m, _, val = SC.spec_pairs(aux["miso1"][:, :, self.ref_ch], clean, return_value=True)
        extra = torch.cat((st.reshape(-1), sm.reshape(-1), pair_o.reshape(-1), pair_m.reshape(-1), val))
        return pcm, self.workspace(N, T)[:4].view(torch.int32).clone(), extra

    def _recording_score(self, rows, n_valid):
        """(stats, stats_mix[, pair_out, pair_miso1, upit]) of the chunks of one recording, in order -> :class:`score.Score`"""
        from . import score as SC
        st, n = SC.combine([r[0] for r in rows], n_valid)
        sm, _ = SC.combine([r[1] for r in rows], n_valid)
        if len(rows[0]) == 2:
            return SC.from_stats(st, n, sm)
        # the criterion is a sum over frames and bins: a recording's value is the sum over its chunks
        le = np.sum([np.diagonal(r[2]) for r in rows], axis=0)
        return SC.from_stats(st, n, sm, loss_miso1=float(np.sum([r[4] for r in rows])), loss_enhance=le)

    def _spec_pass(self, mix, clean):
        """one coalesced Tester_Enhance batch on the current stream: the pass, ONE iSTFT + int16 over its N * S
        spectrograms, and a copy of the pass's NaN flag word (ws[0])"""
        N, _, T, _ = mix.shape
        pcm = S.istft_int16(self.enhance(mix, clean, check_nan=False))                      # [N, S, (T - 1) * 64]
        return pcm, self.workspace(N, T)[:4].view(torch.int32).clone()

    def _coalesced(self, items, fill, compute, dtype, max_batch: int, depth: int, label, to_host: bool = True,
                   extra_rows=None):
        """The engine of the coalesced drop-ins: :func:`coalesce.coalesce` over :class:`_Overlapped`.

        ``items``: :class:`coalesce.Item` whose ``key`` is the tuple of the per-chunk input shapes (None: input absent);
        ``fill(chunk, rows)`` copies one chunk's inputs into its rows of the pinned staging buffers ([max_batch, *shape]
        per input, ``dtype``, one set per slot: batch i - depth, their last user, has been collected when batch i is
        staged); ``compute(*device inputs [N, ...])`` -> (result [N, ...], flag) on the current stream.  No per-batch host
        synchronisation: the host waits for the oldest batch in flight only.  Yields completed items in loader order with
        ``item.outputs[split][b]`` = the chunk's result row (ndarray; the device row(s) with ``to_host=False``).  A NaN in a
        batch raises FloatingPointError naming ``label(chunk)`` of its chunks.  ``extra_rows(block, n)``: ``compute`` returns
        a third value, a small device block that rides the result's D2H; the function cuts its host copy into per-chunk
        tuples and a chunk's output becomes ``(result row, *its tuple)``."""
        from .coalesce import coalesce
        depth = max(1, int(depth))
        ov = _Overlapped(self.device, depth)
        staging = [dict() for _ in range(depth)]

        def submit(i, chunks):
            st, n = staging[i % depth], len(chunks)
            bufs = []
            for j, shape in enumerate(chunks[0].item.key):
                if shape is None:
                    bufs.append(None)
                    continue
                pin = st.get(j)
                if pin is None or tuple(pin.shape[1:]) != tuple(shape) or pin.shape[0] < n:
                    pin = st[j] = torch.empty((max(n, int(max_batch)),) + tuple(shape), dtype=dtype, pin_memory=True)
                bufs.append(pin)
            for r, c in enumerate(chunks):
                fill(c, [b[r] if b is not None else None for b in bufs])
            rec = ov.submit(i, [b[:n] if b is not None else None for b in bufs], compute, dtype=dtype, to_host=to_host)
            return rec, chunks

        def collect(handle):
            rec, chunks = handle
            res, nan = ov.finish(rec)
            if nan:
                names = list(dict.fromkeys(label(c) for c in chunks))
                raise FloatingPointError(f"libmisonet_hip: NaN in pipeline output of the batch holding {', '.join(names)}")
            if extra_rows is not None:
                parts = extra_rows(ov.extra(rec), len(chunks))
                return [(res[r],) + tuple(q[r] for q in parts) for r in range(len(chunks))]
            return list(zip(*res)) if isinstance(res, tuple) else list(res)

        with torch.cuda.device(self.device):
            yield from coalesce(items, submit, collect, max_batch, depth)

    def separate(self, mix: torch.Tensor, clean: Optional[torch.Tensor] = None, check_nan=True) -> torch.Tensor:
        """Separation stage only: MISO1_Inference over the circular shifts + alignments (tester.py:1014-1068, 889-915).
        mix complex [B,M,T,F] -> aligned estimates complex64 [B,S,M,T,F] (speaker, microphone)."""
        self._ready()
        if not isinstance(mix, torch.Tensor) or mix.dim() != 4:
            raise ValueError("mix must be a 4-D complex tensor [B, M, T, F]")
        mix = self._check_c64(mix, "mix")
        B, M, T, F = mix.shape
        if M != self.num_ch:
            raise ValueError(f"expected {self.num_ch} microphones, got {M}")
        if F != N_FREQ:
            raise ValueError(f"the networks are defined for F = {N_FREQ} frequency bins, got {F}")
        if T < 2:                              # as the reference: InstanceNorm over one element (model.py:89, 413)
            raise ValueError(f"Expected more than 1 spatial element when training, got T = {T} frame(s)")
        if clean is not None:
            clean = self._check_c64(clean, "clean", (B, self.num_spks, T, F))
        ws = self.workspace(B, T)
        m1 = torch.empty((B, self.num_spks, M, T, F), dtype=torch.complex64, device=self.device)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            _lib.check(L.misonet_pipeline_run(self._pipe, mix.data_ptr(), clean.data_ptr() if clean is not None else None,
                                              B, T, None, None, m1.data_ptr(), ws.data_ptr(), ws.numel(), st))
            if check_nan:
                _lib.check(L.misonet_pipeline_check(self._pipe, ws.data_ptr(), st))
        return m1

    def beamform_utterance(self, obs_splits: List[torch.Tensor], clean_splits: List[torch.Tensor], gap: int,
                           epsi: Optional[float] = None, max_batch: int = 16, to_host: bool = True, beamformer=None):
        """Utterance-wise MVDR of the reference's Tester_Beamforming (tester.py:340-449, ``utterance_flag``) for ONE
        recording: its splits are separated as ONE batch (:meth:`separate`; the reference runs them one by one), all
        (speaker, mic) estimates and the observation go back to the time domain with one batched iSTFT, the splits are
        stitched (last one trimmed by ``gap``), the whole recording is re-analysed by the HIP STFT front-end and ONE MVDR per
        speaker is solved over all its frames (spatial covariances accumulated over the full utterance instead of per 4 s
        chunk).  obs_splits: list of complex [M,T,F]; clean_splits: list of complex [S,T,F].  Returns int16 [S, n] (an ndarray;
        ``to_host=False``: the device tensor, nothing synchronises).  ``beamformer``: None = the Enhancer's
        (:meth:`set_beamformer`); ``epsi``: None = the options' own, 1e-6 where they leave it unset."""
        K = len(obs_splits)
        if K < 1 or len(clean_splits) != K:
            raise ValueError("obs_splits / clean_splits must be non-empty lists of equal length")
        obs = torch.stack([torch.as_tensor(o) for o in obs_splits]).to(self.device, non_blocking=True)   # [K,M,T,F]
        cl = torch.stack([torch.as_tensor(c) for c in clean_splits]).to(self.device, non_blocking=True)  # [K,S,T,F]
        est = torch.cat([self.separate(obs[lo:lo + max_batch], cl[lo:lo + max_batch])          # [K,S,M,T,F], in groups of
                         for lo in range(0, K, max_batch)])                                   # <= max_batch splits (workspace)
        pcm = self._utterance_tail(est, obs, gap, epsi, beamformer)
        return pcm.cpu().numpy() if to_host else pcm

    def _utterance_tail(self, est: torch.Tensor, obs: torch.Tensor, gap: int, epsi: Optional[float] = None,
                        beamformer=None) -> torch.Tensor:
        """The per-recording tail of :meth:`beamform_utterance` (and of the coalesced utterance-wise Tester_Beamforming):
        est complex [K,S,M,T,F] = the separated splits, obs complex [K,M,T,F] (device) -> int16 [S, n] (device): one
        batched iSTFT, the splits stitched (last one trimmed by ``gap``), one long STFT, one MVDR per speaker, int16."""
        from .beamform import Apply_Beamforming, Apply_Beamforming_Joint
        bf_opts = self._bf(beamformer, epsi)
        K = est.shape[0]
        e = S.istft(est)                                                                      # [K,S,M,chunk]
        o = S.istft(obs)                                                                      # [K,M,chunk]
        n = e.shape[-1]
        keep = [n] * (K - 1) + [n - int(gap)]
        est_t = torch.cat([e[k, ..., : keep[k]] for k in range(K)], dim=-1)                   # [S,M,L]
        obs_t = torch.cat([o[k, ..., : keep[k]] for k in range(K)], dim=-1)                   # [M,L]
        Ls = obs_t.shape[-1]
        pad = (-Ls) % S.HOP                                                   # scipy's padded=True: whole hops
        sig = torch.cat([obs_t[None], est_t], dim=0)                          # [1+S, M, L]
        sig = torch.nn.functional.pad(sig, (0, pad)).permute(0, 2, 1).contiguous()      # [1+S, Lp, M]
        spec = S.stft_hip(sig)                                                # [1+S, M, Tt, F]
        mix_bf = spec[0].permute(2, 0, 1)[None]                               # [1,F,M,Tt]
        src = spec[1:].permute(0, 3, 1, 2)[None]                              # [1,S,F,M,Tt]
        if self.refine is not None:                                           # one clustering over the recording's frames
            src = refined_images(src, mix_bf, self.refine)
        if isinstance(bf_opts, JointBeamformer):                              # one joint solve for all speakers
            bf = Apply_Beamforming_Joint(src, mix_bf, bf_opts)[0]
        else:
            bf = torch.stack([Apply_Beamforming(src[:, s], mix_bf, beamformer=bf_opts)[0]
                              for s in range(self.num_spks)])                 # [S,Tt,F]
        return S.istft_int16(bf)

    def beamform_chunks(self, mix: torch.Tensor, clean: Optional[torch.Tensor] = None, epsi: Optional[float] = None,
                        check_nan: bool = True, beamformer=None) -> torch.Tensor:
        """Chunk-wise MVDR (BASELINE configs[2]: MISO1 -> MVDR; the ``utterance_flag = False`` branch of the reference's
        Tester_Beamforming, tester.py:452-535): separation of a batch of 4 s chunks, then one MVDR per (chunk, speaker) over
        the chunk's own frames.  mix complex [B,M,T,F], clean complex [B,S,T,F] or None -> beamformer outputs complex64
        [B,S,T,F].  (With MISO_3 attached, ``enhance(..., want_bf=True)`` returns the same tensor from the fused pass.)"""
        from .beamform import Apply_Beamforming, Apply_Beamforming_Joint
        bf_opts = self._bf(beamformer, epsi)
        est = self.separate(mix, clean, check_nan=check_nan)                                  # [B,S,M,T,F]
        mix_bf = self._check_c64(mix, "mix").permute(0, 3, 1, 2)                              # [B,F,M,T]
        if self.refine is not None:
            est = refined_images(est.permute(0, 1, 4, 2, 3), mix_bf, self.refine).permute(0, 1, 3, 4, 2)
        if isinstance(bf_opts, JointBeamformer):                                              # one joint solve for all speakers
            return Apply_Beamforming_Joint(est.permute(0, 1, 4, 2, 3), mix_bf, bf_opts)
        return torch.stack([Apply_Beamforming(est[:, s].permute(0, 3, 1, 2), mix_bf, beamformer=bf_opts)
                            for s in range(self.num_spks)], dim=1)                            # [B,S,T,F]

    def enhance_recording(self, wav_observe, wav_clean=None, num_ch_utilize: Optional[int] = None, chunk_size: int = 64000,
                          max_batch: int = 16, save_path: Optional[str] = None, fs: int = 16000, score: bool = False,
                          bss: bool = False, bss_filt_len: int = 512, stoi: bool = False, reverb: bool = False,
                          srmr: bool = False, fs_in=None, fs_out=None):
        """Recording in -> enhanced int16 waves out: the reference's loader item AND its tester body as one device-side
        object (``AudioDataset_Test.__getitem__``, dataloader/data.py:524-597, + ``Tester_Enhance.inference``,
        tester.py:846-975), without host STFT dicts.

        wav_observe: float32 [L, M_all] (ndarray or CPU tensor, time-major as ``read_wav`` returns it); wav_clean: the
        clean sources, a sequence of S arrays [L, M_all] (``<name>_0.wav``, ``<name>_1.wav``, data.py:527-528) or None.
        Steps, each as the reference does it: microphone sub-sampling ``[0:M:M // num_ch_utilize]`` (data.py:544; default:
        the network's microphone count), 4 s chunks with the last one zero-padded by ``gap`` (data.py:536-595;
        ``L == chunk_size``, which the reference leaves unhandled, is one chunk), the clean sources at ``ref_ch`` of the
        sub-sampled array (tester.py:889-890), per chunk STFT -> MISO1 x M -> alignments -> MVDR x S -> MISO3 x S -> iSTFT ->
        x 32767 -> int16 (HIP kernels end to end, the chunks of the recording as batches of <= ``max_batch`` through
        :meth:`stream_wav`: H2D of the next batch and D2H of the previous one beside the compute), chunks stitched with the
        padded tail dropped (tester.py:960-969).  Returns int16 [S, L]; ``save_path`` = "<dir>/<wav_name>" also writes
        ``<save_path>_{s}.wav`` as 24-bit PCM (tester.py:972-974).  With ``wav_clean=None`` the speaker order is that of
        each chunk on its own (MISO1 is PIT-trained): for one speaker per output across a long recording use
        :meth:`enhance_continuous`.

        ``score=True`` (needs ``wav_clean``): returns ``(pcm, Score)``: the int16 result, bit for bit what ``score=False``
        returns, and its :class:`score.Score` against the clean sources at ``ref_ch`` (SI-SDR, its improvement over the
        observation at ``ref_ch``, SNR, the best permutation).  The sums are taken on the device behind the iSTFT of every
        batch and come back with the int16 waves; the padded tail of the last chunk is left out; the chunks are added on
        the host in float64.  A chunk's sums do not depend on ``max_batch``.

        ``bss=True`` (needs ``score=True``): returns ``(pcm, Score, BssEval)``; ``pcm`` and ``Score`` are bit for bit those
        of ``bss=False``.  :class:`score.BssEval` holds BSS-eval SDR, SIR and SAR (the figures SMS-WSJ tabulates,
        INTEGRATION.md 4e) of the stitched int16 result against the clean sources at ``ref_ch`` with filters of
        ``bss_filt_len`` taps, the observation at ``ref_ch`` as the mixture: what
        ``score.bss_eval_waves(pcm, clean[:, :, ref_ch], mix)`` returns.

        ``stoi=True`` (needs ``score=True``): a :class:`score.Stoi` is appended as the last element of the returned tuple,
        ``(pcm, Score, Stoi)`` or ``(pcm, Score, BssEval, Stoi)``; everything before it keeps its bits.  It holds STOI and
        ESTOI of the stitched int16 result against the clean sources at ``ref_ch`` at rate ``fs`` (8000,
        10000 or 16000), the observation at ``ref_ch`` as the mixture: what
        ``score.stoi_waves(pcm, clean[:, :, ref_ch], mix, fs)`` returns.

        ``reverb=True`` (needs ``score=True``): a :class:`score.Reverb` is appended as the last element of the returned
        tuple, after ``BssEval`` and ``Stoi`` where those are asked for; everything before it keeps its bits.  It holds the
        cepstral distance, the log-likelihood ratio and the frequency-weighted segmental SNR, the figures
        dereverberation is judged by, of the stitched int16 result against the clean sources at ``ref_ch`` at rate ``fs``
        (8000 or 16000), the original observation at ``ref_ch`` as the mixture (also with ``dereverb=`` set): what
        ``score.reverb_waves(pcm, clean[:, :, ref_ch], mix, fs)`` returns.

        ``srmr=True`` (needs neither ``score=True`` nor the clean sources): a :class:`score.Srmr` is appended as the last
        element, ``(pcm, Srmr)`` on its own or after ``Reverb`` and the others; everything before it keeps its bits.  It
        holds the speech-to-reverberation modulation energy ratio, the one figure that takes no clean
        reference, of the stitched int16 result at rate ``fs`` (8000 or 16000), the original observation at ``ref_ch`` as the
        mixture: what ``score.srmr_waves(pcm, mix, fs)`` returns.  A recording shorter than one 256 ms frame gives an
        invalid ``Srmr``, not an error.

        ``fs_in`` / ``fs_out``: ``fs`` is the rate the networks run at.  ``fs_in`` other than ``fs``: the
        files are at ``fs_in``; the observation -- with its clean sources, as the items of one launch -- is taken to ``fs`` on the
        device (:mod:`misonet_amd.resample`) before anything else.  ``fs_out``: an integer rate or ``"in"`` (= ``fs_in``): the
        int16 result is taken to that rate on the device and written with that rate in the header; it has the input's length
        when ``fs_out`` is the input's rate.  Every score is computed at ``fs``.  With both None not one launch is added."""
        if fs_in is not None or fs_out is not None:
            from . import resample as RS
            RS.plan_rates(fs, fs_in, fs_out)                               # a bad rate: before anything else
            return RS.around(lambda w, c, path: self.enhance_recording(w, c, num_ch_utilize, chunk_size, max_batch, path, fs,
                                                                       score, bss, bss_filt_len, stoi, reverb, srmr),
                             wav_observe, wav_clean, fs, fs_in, fs_out, save_path, self._write_speakers, self.device)
        if srmr:
            from . import score as SC
            SC.check_srmr_fs(fs)
            res = self.enhance_recording(wav_observe, wav_clean, num_ch_utilize, chunk_size, max_batch, save_path, fs, score,
                                         bss, bss_filt_len, stoi, reverb)
            return (res if isinstance(res, tuple) else (res,)) + (self._srmr_of(res, wav_observe, num_ch_utilize, fs),)
        asked = self._side_asked(score, wav_clean is None, fs, bss_filt_len, bss=bss, stoi=stoi, reverb=reverb)
        self._ready()
        if self.model is None:
            raise RuntimeError("this Enhancer was built without MISO_3 (separation only): use separate() / beamform_*()")
        pieces, cpieces, gap, mpieces = self._recording_chunks(wav_observe, wav_clean, num_ch_utilize, chunk_size)
        K = len(pieces)
        if score:
            nv = [pieces[0].shape[0]] * (K - 1) + [pieces[0].shape[0] - gap]

            def scored_batches():
                for lo in range(0, K, max_batch):
                    b = (torch.from_numpy(np.stack(pieces[lo:lo + max_batch])),
                         torch.from_numpy(np.stack(cpieces[lo:lo + max_batch])), nv[lo:lo + max_batch])
                    yield b if mpieces is None else b + (torch.from_numpy(np.stack(mpieces[lo:lo + max_batch])),)

            got = list(self.stream_wav(scored_batches(), score=True))
            pcm = np.concatenate([g[0] for g in got], axis=0)
            rows = [(g[1][0][b], g[1][1][b]) for g in got for b in range(g[0].shape[0])]
            out, sc = self._finish_recording([pcm[k] for k in range(K)], gap, save_path, fs), self._recording_score(rows, nv)
            if not asked:
                return out, sc
            clean, mix = self._wave_refs(wav_observe, wav_clean, num_ch_utilize)
            return (out, sc) + tuple(f.waves(out, clean, mix, par, self.device) for f, par in asked)

        def batches():
            for lo in range(0, K, max_batch):
                w = torch.from_numpy(np.stack(pieces[lo:lo + max_batch]))
                yield (w, torch.from_numpy(np.stack(cpieces[lo:lo + max_batch]))) if cpieces is not None else w

        pcm = np.concatenate(list(self.stream_wav(batches())), axis=0)     # [K, S, chunk]
        return self._finish_recording([pcm[k] for k in range(K)], gap, save_path, fs)

    @staticmethod
    def _side_asked(score, clean_missing, fs, bss_filt_len, **flags):
        """the flags of the recording paths for the figures of ``score.SIDE_FIGURES`` that take the clean sources -> [(figure,
        its parameter)] of those asked for, in the order they are appended; ValueError for a flag without ``score=True``, for
        ``score=True`` without clean sources (``clean_missing``) and for a rate a figure is not defined at"""
        from . import score as SC
        figs = [f for f in SC.SIDE_FIGURES if f.needs_clean and flags[f.name]]
        if figs and not score:
            raise ValueError(f"{figs[0].name}=True needs score=True (and the clean sources)")
        if score and clean_missing:
            raise ValueError("score=True needs the clean sources (wav_clean)")
        return [(f, bss_filt_len if f.rates is None else f.check(fs)) for f in figs]

    def _srmr_of(self, res, wav_observe, num_ch_utilize, fs):
        """the :class:`score.Srmr` of a recording's result (int16 [S, L], or a tuple that starts with it) with the original
        observation at ref_ch of the sub-sampled array as the mixture"""
        from . import score as SC
        mics, obs = self._select_mics(wav_observe, num_ch_utilize)
        pcm = res[0] if isinstance(res, tuple) else res
        return SC.srmr_waves(pcm, np.ascontiguousarray(obs[:, mics[self.ref_ch]]), fs=fs, device=self.device)

    def _wave_refs(self, wav_observe, wav_clean, num_ch_utilize):
        """the references of BSS-eval, STOI and the reverb figures for one recording: (the clean sources at ref_ch of the sub-sampled array, float32
        [S, L]; the observation there, float32 [L])"""
        mics, obs = self._select_mics(wav_observe, num_ch_utilize)
        m = mics[self.ref_ch]
        return (np.stack([np.asarray(c, dtype=np.float32)[:, m] for c in wav_clean]), np.ascontiguousarray(obs[:, m]))

    def _select_mics(self, wav_observe, num_ch_utilize):
        """float32 [L, M_all] -> (the microphone indices [0:M:M // num_ch_utilize] (data.py:544), the recording as float32)"""
        obs = np.asarray(wav_observe, dtype=np.float32)
        if obs.ndim != 2 or obs.shape[0] <= obs.shape[1]:
            raise ValueError("wav_observe must be [n_samples, n_mics] with n_samples > n_mics (data.py:510)")
        M_all = obs.shape[1]
        n_use = self.num_ch if num_ch_utilize is None else int(num_ch_utilize)
        if n_use < 1 or n_use > M_all:
            raise ValueError(f"num_ch_utilize must be in [1, {M_all}]")
        mics = list(range(0, M_all, M_all // n_use))                       # data.py:544: [0:M:M // num_ch_utilize]
        if len(mics) != self.num_ch:
            raise ValueError(f"[0:{M_all}:{M_all // n_use}] selects {len(mics)} microphones, the networks take {self.num_ch}")
        return mics, obs

    def _recording_chunks(self, wav_observe, wav_clean, num_ch_utilize, chunk_size):
        """enhance_recording's loader side: microphone sub-sampling, the dereverberation when one is set, the clean sources at
        ref_ch, 4 s chunks -> (list of float32 [chunk, M], list of float32 [chunk, S] or None, gap, None or -- with a
        dereverberation -- the chunks of the original observation at ref_ch, float32 [chunk, 1])"""
        mics, obs = self._select_mics(wav_observe, num_ch_utilize)
        L, M_all = obs.shape
        if int(chunk_size) < 2 * S.HOP or int(chunk_size) % S.HOP:
            raise ValueError(f"chunk_size must be a multiple of the hop ({S.HOP}) and at least two hops")
        obs = obs[:, mics]
        raw = None
        if self.dereverb is not None:
            raw, obs = obs[:, self.ref_ch:self.ref_ch + 1], self._observe(obs)
        cl = None
        if wav_clean is not None:
            if len(wav_clean) != self.num_spks:
                raise ValueError(f"wav_clean must hold {self.num_spks} source recordings")
            srcs = []
            for c in wav_clean:
                c = np.asarray(c, dtype=np.float32)
                if c.shape != (L, M_all):
                    raise ValueError("every clean source must have the shape of wav_observe")
                srcs.append(c[:, mics][:, self.ref_ch])
            cl = np.stack(srcs, axis=1)                                    # [L, S]
        pieces, gap = S.split_chunks(obs, int(chunk_size))
        cpieces = S.split_chunks(cl, int(chunk_size))[0] if cl is not None else None
        mpieces = S.split_chunks(raw, int(chunk_size))[0] if raw is not None else None
        return pieces, cpieces, gap, mpieces

    def _finish_recording(self, pcm_chunks, gap, save_path, fs):
        """the K int16 chunks [S, chunk] of one recording -> stitched int16 [S, L]; ``save_path``: the PCM-24 files"""
        out = np.stack([S.stitch_int16([p[s] for p in pcm_chunks], gap) for s in range(self.num_spks)])
        if save_path is not None:
            self._write_speakers(out, save_path, fs)
        return out

    def _write_speakers(self, out, save_path, fs):
        """int16 [S, L] -> ``<save_path>_{s}.wav`` as 24-bit PCM (tester.py:972-974)"""
        import os
        os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
        for s in range(self.num_spks):
            S.write_wav_pcm24(f"{save_path}_{s}.wav", out[s], fs)

    def enhance_continuous(self, wav_observe, num_ch_utilize: Optional[int] = None, window: int = 64000,
                           hop: Optional[int] = None, max_batch: int = 16, save_path: Optional[str] = None,
                           fs: int = 16000, return_perms: bool = False, srmr: bool = False, fs_in=None, fs_out=None):
        """A long recording WITHOUT clean references -> one speaker per output from start to end (continuous separation).

        wav_observe float32 [L, M_all] (as :meth:`enhance_recording` takes it; same microphone sub-sampling).  The recording
        is cut into windows of ``window`` samples at a hop of ``hop`` (default window // 2; both multiples of 64,
        window/2 <= hop <= window - 256: :func:`css.plan_windows`), the last one zero-padded.  Every window goes through the
        fused pass without clean sources (STFT -> MISO1 x M -> shift alignment -> MVDR x S -> MISO3 x S, bit for bit what
        :meth:`enhance_wav` returns for it alone); the speaker order of window k is linked to window k-1 through their
        shared frames (``misonet_css_align``: the reference's alignment metric over the overlap, composed along the
        recording, so the output order is window 0's) and the windows' waveforms are joined by a raised-cosine cross-fade
        over the overlap (``misonet_css_stitch``).  Windows run in batches of at most ``max_batch`` plus the window carried
        over from the previous batch: device memory depends on ``max_batch``, not on the recording's length, the host waits
        only for the oldest of two batches in flight, and the result does not depend on ``max_batch``.

        Returns int16 [S, L] (ndarray) and, with ``return_perms``, P int32 [K, S] (output speaker s of window k = MISO3
        output P[k, s] of that window).  ``save_path`` also writes ``<save_path>_{s}.wav`` as 24-bit PCM.  A NaN raises
        FloatingPointError naming the first window that produced it.

        ``srmr=True``: a :class:`score.Srmr` is appended, ``(pcm, Srmr)`` or ``(pcm, P, Srmr)``: the speech-to-reverberation
        modulation energy ratio of the stitched int16 result at rate ``fs`` (8000 or 16000), the original
        observation at ``ref_ch`` as the mixture -- the figure to read when choosing ``taps``, ``delay`` or ``iterations``
        on recordings that have no references.  It is measured on the device from the int16 pieces the pass leaves there;
        the waves and P are bit for bit those of ``srmr=False``, and the figure is what
        ``score.srmr_waves(pcm, observation[:, ref_ch], fs)`` returns.

        ``fs_in`` / ``fs_out``: a recording at another rate than the networks' ``fs``, as :meth:`enhance_recording` takes them
        (INTEGRATION.md 4o); ``window`` and ``hop`` count samples at ``fs``.  With both None not one launch is added."""
        if fs_in is not None or fs_out is not None:
            from . import resample as RS
            RS.plan_rates(fs, fs_in, fs_out)                               # a bad rate: before anything else
            return RS.around(lambda w, _c, path: self.enhance_continuous(w, num_ch_utilize, window, hop, max_batch, path, fs,
                                                                         return_perms, srmr),
                             wav_observe, None, fs, fs_in, fs_out, save_path, self._write_speakers, self.device)
        import collections
        from . import css
        if srmr:
            from . import score as SC
            SC.check_srmr_fs(fs)
        self._ready()
        if self.model is None:
            raise RuntimeError("this Enhancer was built without MISO_3 (separation only): use separate() / beamform_*()")
        mics, obs = self._select_mics(wav_observe, num_ch_utilize)
        L = obs.shape[0]
        W = int(window)
        H = W // 2 if hop is None else int(hop)
        _, K, Lp = css.plan_windows(L, W, H)
        nb_max = max(1, int(max_batch))
        M, Sp, T, F = self.num_ch, self.num_spks, W // S.HOP + 1, N_FREQ
        padded = np.zeros((Lp, M), dtype=np.float32)
        padded[:L] = self._observe(obs[:, mics])
        dev, lib = self.device, _lib.lib()
        out = np.empty((Sp, L), dtype=np.int16)
        with torch.cuda.device(dev):
            # row 0 of est / y / perm: the window carried over from the previous batch (its spectrogram, waveform and P)
            est = torch.empty((nb_max + 1, Sp, T, F), dtype=torch.complex64, device=dev)
            y = torch.empty((nb_max + 1, Sp, W), dtype=torch.float32, device=dev)
            perm = torch.empty((nb_max + 1, Sp), dtype=torch.int32, device=dev)
            dist = torch.empty(max(8, css.scratch_bytes(nb_max + 1, Sp, F)), dtype=torch.uint8, device=dev)
            perms = torch.empty((K, Sp), dtype=torch.int32, device=dev)
            kept = torch.empty((1, Sp, L), dtype=torch.int16, device=dev) if srmr else None

            def compute_for(lo, hi):
                def compute(wav):
                    nb, c = hi - lo, (1 if lo else 0)         # c: row of window lo
                    n = c + nb
                    st = _lib.stream_ptr(dev)
                    ws = self.workspace(nb, T)
                    _lib.check(lib.misonet_pipeline_run_wav(self._pipe, wav.data_ptr(), None, nb, W, est[c].data_ptr(), None,
                                                            None, ws.data_ptr(), ws.numel(), st))
                    flag = ws[:4].view(torch.int32).clone()
                    css.align(est[:n], H // S.HOP, perm0=perm[0] if c else None, perm=perm[:n], dist=dist)
                    _lib.check(lib.misonet_istft(est[c].data_ptr(), nb * Sp, T, None, y[c].data_ptr(), st))
                    pcm = css.stitch(y[:n], perm[:n], H, c == 0, (L if hi == K else hi * H) - lo * H)
                    perms[lo:hi].copy_(perm[c:n])
                    if kept is not None:
                        kept[0, :, lo * H: lo * H + pcm.shape[1]].copy_(pcm)
                    if hi < K and n > 1:
                        est[0].copy_(est[n - 1])
                        y[0].copy_(y[n - 1])
                        perm[0].copy_(perm[n - 1])
                    return pcm, flag
                return compute

            ov = _Overlapped(dev, 2)
            pending = collections.deque()

            def finish(rec, lo, hi):
                pcm, nan = ov.finish(rec)
                if nan:
                    raise FloatingPointError(self._nan_window(padded, lo, hi, W, H))
                out[:, lo * H: lo * H + pcm.shape[1]] = pcm

            for i, lo in enumerate(range(0, K, nb_max)):
                hi = min(K, lo + nb_max)
                while len(pending) >= ov.depth:
                    finish(*pending.popleft())
                wav_h = torch.from_numpy(np.stack([padded[k * H: k * H + W] for k in range(lo, hi)]))
                pending.append((ov.submit(i, (wav_h,), compute_for(lo, hi)), lo, hi))
            while pending:
                finish(*pending.popleft())
            P = perms.cpu().numpy() if return_perms else None
            sr = None
            if srmr:
                torch.cuda.synchronize(dev)                   # the pieces were left by the streams of the batches
                mixd = torch.from_numpy(np.ascontiguousarray(obs[:, mics[self.ref_ch]])).to(dev)[None, None]
                sr = SC.srmr_unpack(SC.srmr_block(kept, mixd, None, fs)[0].cpu().numpy(), Sp, int(fs), L)
        if save_path is not None:
            self._write_speakers(out, save_path, fs)
        res = (out, P) if return_perms else out
        if srmr:
            return (res if return_perms else (res,)) + (sr,)
        return res

    def _nan_window(self, padded, lo, hi, W, H):
        """the message of a NaN in the batch of windows lo..hi-1: those windows again, one at a time, to name the first"""
        for k in range(lo, hi):
            try:
                self.enhance_wav(torch.from_numpy(padded[k * H: k * H + W][None].copy()).to(self.device), None)
            except FloatingPointError:
                return f"libmisonet_hip: NaN in pipeline output of window {k} (samples {k * H}..{k * H + W} of the recording)"
        return f"libmisonet_hip: NaN in pipeline output of windows {lo}..{hi - 1}"

    BSS_GROUP = 16      # recordings per BSS-eval / STOI batch of enhance_recordings: 0.53 ms each at 16 against 6.1 ms one by one

    def enhance_recordings(self, recordings, num_ch_utilize: Optional[int] = None, chunk_size: int = 64000,
                           max_batch: int = 16, save_path: Optional[str] = None, fs: int = 16000,
                           depth: int = 2, score: bool = False, bss: bool = False,
                           bss_filt_len: int = 512, stoi: bool = False, reverb: bool = False,
                           srmr: bool = False, fs_in=None, fs_out=None) -> Dict[str, np.ndarray]:
        """:meth:`enhance_recording` over many recordings, with every launch filled across them.

        ``recordings``: an iterable of ``(wav_observe, wav_clean or None, name)``, each as :meth:`enhance_recording` takes
        it (``num_ch_utilize`` and ``chunk_size`` apply to every one).  Every recording is cut into its 4 s chunks; the
        chunks go through the pipeline in batches of ``max_batch`` taken across recordings (:mod:`coalesce`; the HIP STFT
        front-end, the fused pass, one iSTFT + int16 per batch, copies overlapped as in :meth:`stream_wav`, at most
        ``depth`` batches in flight); the int16 chunks are scattered back and every recording stitched.  ``save_path``: a
        directory; recording ``name`` is written as ``<save_path>/<name>_{s}.wav``.  Returns {name: int16 [S, L]} in input
        order; each recording bit for bit what :meth:`enhance_recording` returns for it alone (results do not depend on the
        batch).  ``score=True`` (every recording needs its clean sources): {name: (int16 [S, L], Score)}, each
        pair bit for bit what :meth:`enhance_recording` returns with ``score=True``.  ``bss=True`` (needs ``score=True``):
        {name: (int16 [S, L], Score, BssEval)}.  The stitched recordings are queued for BSS-eval in groups of
        ``BSS_GROUP`` on a stream of their own (pinned copies, the correlation and factorisation kernels of csrc/bss.hip,
        one batch per group: a recording's figures do not depend on the group) and nothing waits for them until every
        recording has gone through: the pass is not stalled.  ``stoi=True`` (needs ``score=True``): a :class:`score.Stoi`
        (STOI and ESTOI at rate ``fs``, csrc/stoi.hip) is appended as the last element of every tuple, queued in the same
        groups on the same side stream; everything before it keeps its bits.  ``reverb=True`` (needs ``score=True``): a
        :class:`score.Reverb` (cepstral distance, LLR and fwSegSNR at rate ``fs``, csrc/reverb.hip) is appended after those,
        from the same padded, pinned batch on the same side stream.  ``srmr=True`` (needs neither ``score=True`` nor clean
        sources): a :class:`score.Srmr` (csrc/srmr.hip) is appended as the last element of every entry,
        ``(pcm, Srmr)`` on its own; the stitched recordings go in padded batches of ``BSS_GROUP`` with their observation at
        ``ref_ch`` as the mixture, and each figure is what :meth:`enhance_recording` gives for the recording alone.

        ``fs_in`` / ``fs_out``: as :meth:`enhance_recording` takes them, for every recording: each is taken
        to ``fs`` on the device as it is drawn from ``recordings`` (one launch for the observation and its clean sources), and
        each result to ``fs_out`` behind the pass; every entry is bit for bit what :meth:`enhance_recording` gives with the same
        rates.  With both None not one launch is added."""
        import os
        from .coalesce import Item
        if fs_in is not None or fs_out is not None:
            from . import resample as RS
            r_in, r_out, rate = RS.plan_rates(fs, fs_in, fs_out)           # a bad rate: before anything else
            lengths = {}

            def at_model_rate():
                for wav_observe, wav_clean, name in recordings:
                    lengths[name] = int(np.shape(wav_observe)[0])
                    if r_in is not None:
                        got = RS.to_rate([wav_observe] + list(wav_clean or []), r_in, fs, self.device)
                        wav_observe, wav_clean = got[0], (got[1:] if wav_clean is not None else None)
                    yield wav_observe, wav_clean, name

            res = self.enhance_recordings(at_model_rate(), num_ch_utilize, chunk_size, max_batch,
                                          None if r_out is not None else save_path, fs, depth, score, bss, bss_filt_len, stoi,
                                          reverb, srmr)
            if r_out is not None:
                back = r_out == (fs if r_in is None else r_in)
                for name, r in res.items():
                    pcm = RS.pcm_to_rate(r[0] if isinstance(r, tuple) else r, fs, r_out, lengths[name] if back else None,
                                         self.device)
                    if save_path is not None:
                        self._write_speakers(pcm, os.path.join(save_path, str(name)), rate)
                    res[name] = (pcm,) + tuple(r[1:]) if isinstance(r, tuple) else pcm
            return res
        if srmr:
            from . import score as SC
            SC.check_srmr_fs(fs)
            recordings = list(recordings)
            res = self.enhance_recordings(recordings, num_ch_utilize, chunk_size, max_batch, save_path, fs, depth, score, bss,
                                          bss_filt_len, stoi, reverb)
            names = list(res)
            mixes = {}
            for wav_observe, _, name in recordings:
                mics, obs = self._select_mics(wav_observe, num_ch_utilize)
                mixes[name] = np.ascontiguousarray(obs[:, mics[self.ref_ch]])
            for lo in range(0, len(names), self.BSS_GROUP):
                grp = names[lo:lo + self.BSS_GROUP]
                pcms = [res[k][0] if isinstance(res[k], tuple) else res[k] for k in grp]
                block = SC.srmr_queue([(p, mixes[k]) for p, k in zip(pcms, grp)], fs, self.device).cpu().numpy()
                for k, p, row in zip(grp, pcms, block):
                    res[k] = (res[k] if isinstance(res[k], tuple) else (res[k],)) + \
                        (SC.srmr_unpack(row, self.num_spks, int(fs), p.shape[1]),)
            return res
        asked = self._side_asked(score, False, fs, bss_filt_len, bss=bss, stoi=stoi, reverb=reverb)
        self._ready()
        if self.model is None:
            raise RuntimeError("this Enhancer was built without MISO_3 (separation only): use separate() / beamform_*()")

        def items():
            for i, (wav_observe, wav_clean, name) in enumerate(recordings):
                if score and wav_clean is None:
                    raise ValueError(f"score=True needs the clean sources (wav_clean) of every recording ({name} has none)")
                pieces, cpieces, gap, mpieces = self._recording_chunks(wav_observe, wav_clean, num_ch_utilize, chunk_size)
                key = (pieces[0].shape, cpieces[0].shape if cpieces is not None else None)
                if score:
                    key = key + ((1,),)                              # the chunk's valid count rides as a third input
                    if mpieces is not None:
                        key = key + (mpieces[0].shape,)              # and the original observation at ref_ch as a fourth
                if asked:
                    side_refs[i] = self._wave_refs(wav_observe, wav_clean, num_ch_utilize)
                yield Item(i, 1, len(pieces), key, (pieces, cpieces, gap, name, mpieces))

        def fill(c, rows):
            pieces, cpieces, gap, _, mpieces = c.item.payload
            rows[0].copy_(torch.from_numpy(pieces[c.split]))
            if rows[1] is not None:
                rows[1].copy_(torch.from_numpy(cpieces[c.split]))
            if score:
                n = pieces[0].shape[0]
                rows[2].copy_(self._nv_bits([n - gap if c.split == len(pieces) - 1 else n], torch.float32)[0])
                if mpieces is not None:
                    rows[3].copy_(torch.from_numpy(mpieces[c.split]))

        results = {}
        side_refs, side_wait, side_done = {}, [], []
        if asked:
            from . import score as SC
            side = torch.cuda.Stream(self.device)

            def side_flush():
                with torch.cuda.stream(side):
                    blocks = SC._side_blocks([w[1:] for w in side_wait], self.device, True,
                                             {f.name: par for f, par in asked})   # one padded, pinned batch serves all
                    side_done.append(([w[0] for w in side_wait], blocks))
                side_wait.clear()
        for it in self._coalesced(items(), fill, self._wav_pass_score if score else self._wav_pass, torch.float32, max_batch,
                                  depth, lambda c: str(c.item.payload[3]),
                                  extra_rows=(lambda ex, n: self._score_rows(ex, n, False)) if score else None):
            pieces, _, gap, name, _ = it.payload
            path = os.path.join(save_path, str(name)) if save_path is not None else None
            if score:
                n = pieces[0].shape[0]
                pcm = self._finish_recording([o[0][0] for o in it.outputs], gap, path, fs)
                results[name] = (pcm, self._recording_score([o[0][1:] for o in it.outputs], [n] * (len(pieces) - 1) + [n - gap]))
                if asked:
                    side_wait.append((name, pcm) + side_refs.pop(it.index))
                    if len(side_wait) >= self.BSS_GROUP:
                        side_flush()
            else:
                results[name] = self._finish_recording([o[0] for o in it.outputs], gap, path, fs)
        if asked:
            if side_wait:
                side_flush()
            side.synchronize()
            for names, blocks in side_done:
                for f, par in asked:
                    for name, row in zip(names, blocks[f.name].cpu().numpy()):
                        results[name] = results[name] + (f.unpack(row, self.num_spks, par, results[name][0].shape[1]),)
        return results

    def inference(self, data_loader, saveDir, fs=16000, write=True, max_batch=32, coalesce=True, depth=2, score=False):
        """Drop-in for ``Tester_Enhance.inference(data_loader, saveDir)`` (tester.py:846-975): the loader yields
        ``(split_observe_dict, split_clean_s0_dict, split_clean_s1_dict, gap, wav_name)`` with dict values complex
        ``[B, Ch, T, F]`` keyed '0', '1', ... (dataloader/data.py:524-597).  Every split runs through
        :meth:`enhance`; the int16 waves of the splits are stitched (last split trimmed by ``gap``) and written as
        ``<saveDir>/<wav_name>_{0,1}.wav`` (PCM-24).  Returns {wav_name: int16 [2, n_samples]}.

        ``coalesce=True``: every launch holds ``max_batch`` chunks taken across loader items (:mod:`coalesce`; a change of
        T and the end of the loader flush a shorter one), staged in pinned slots, with no host synchronisation per batch
        (at most ``depth`` batches in flight, the NaN flag word travels with each batch's D2H).  ``coalesce=False``: one
        item at a time, its splits in groups of at most ``max_batch``.  Both return and write the same bits (results do not
        depend on the batch).

        ``score=True``: the return value is unchanged and ``<saveDir>/scores.json`` is written: ``{wav_name:
        Score.as_dict()}`` plus a ``"mean"`` entry over the valid speakers.  The loader carries spectrograms, so the
        reference waves are the device iSTFT (float32) of the clean spectrograms at ``ref_ch`` and the mixture row that of
        the observation at ``ref_ch``; ``loss_enhance`` / ``loss_miso1`` are criterion.py's ``loss_Enhance`` of the output
        and ``loss_uPIT`` of the MISO1 estimate at ``ref_ch``, summed over the recording's chunks."""
        import os
        os.makedirs(saveDir, exist_ok=True)
        if score:
            scores = {}
            if coalesce:
                results = self._inference_coalesced(data_loader, saveDir, fs, write, max_batch, depth, scores)
            else:
                results = {}
                for item in data_loader:                         # one item at a time: its chunks never share a launch
                    results.update(self._inference_coalesced([item], saveDir, fs, write, max_batch, depth, scores))
            self._write_scores(saveDir, scores)
            return results
        if coalesce:
            return self._inference_coalesced(data_loader, saveDir, fs, write, max_batch, depth)
        results = {}
        dev = self.device

        def h2d(x):
            """one asynchronous copy per tensor (pinned staging), instead of a synchronous ``.to(device)`` per split"""
            x = torch.as_tensor(x)
            if x.device == dev:
                return x
            if x.device.type == "cpu" and not x.is_pinned():
                x = x.contiguous().pin_memory()
            return x.to(dev, non_blocking=True)

        def finalize(rec):
            """the previous loader item: wait for ITS D2H only, stitch, write"""
            rec["ev"].synchronize()
            pcm = rec["pcm_h"].numpy()                                                        # [n_split, B, S, n]
            for b in range(pcm.shape[1]):
                gp = rec["gap"]
                g = int(gp[b]) if hasattr(gp, "__len__") else int(gp)
                wav = np.stack([S.stitch_int16([pcm[k, b, s] for k in range(pcm.shape[0])], g)
                                for s in range(self.num_spks)])                               # [S, n_total]
                name = rec["name"][b] if not isinstance(rec["name"], str) else rec["name"]
                results[name] = wav
                if write:
                    for s in range(self.num_spks):
                        S.write_wav_pcm24(os.path.join(saveDir, f"{name}_{s}.wav"), wav[s], fs)

        with torch.cuda.device(dev):
            s_out = torch.cuda.Stream(dev)
            prev = None
            for (obs_d, s0_d, s1_d, gap, wav_name) in data_loader:
                n_split = len(obs_d)
                obs, cl = [], []
                for k in range(n_split):
                    obs.append(h2d(obs_d[str(k)]))
                    s0 = h2d(torch.as_tensor(s0_d[str(k)])[:, self.ref_ch])                   # tester.py:889-890
                    s1 = h2d(torch.as_tensor(s1_d[str(k)])[:, self.ref_ch])
                    cl.append(torch.stack((s0, s1), dim=1))
                # the 4 s splits of a loader item are independent chunks of equal length (dataloader/data.py:558-595): they run
                # as ONE batch of n_split * B utterances (the reference: one pass per split), in groups of at most
                # ``max_batch``.  Bit-identical to split-by-split (results do not depend on the batch).
                Bk = obs[0].shape[0]
                obs, cl = torch.cat(obs), torch.cat(cl)                                        # [n_split * B, ...]
                out = torch.empty((obs.shape[0], self.num_spks) + tuple(obs.shape[2:]), dtype=torch.complex64, device=dev)
                for lo in range(0, obs.shape[0], max_batch):
                    self.enhance(obs[lo:lo + max_batch], cl[lo:lo + max_batch], out=out[lo:lo + max_batch])
                outs = out.reshape((n_split, Bk) + tuple(out.shape[1:]))                       # [n_split,B,S,T,F]
                pcm = S.istft_int16(outs)                        # ONE batched iSTFT over n_split * B * S spectrograms
                ev_done = torch.cuda.Event()
                ev_done.record(torch.cuda.current_stream(dev))
                rec = {"pcm_h": torch.empty(pcm.shape, dtype=torch.int16, pin_memory=True), "gap": gap, "name": wav_name}
                with torch.cuda.stream(s_out):                   # ONE D2H per loader item, beside the next item's compute
                    s_out.wait_event(ev_done)
                    rec["pcm_h"].copy_(pcm, non_blocking=True)
                    pcm.record_stream(s_out)
                    rec["ev"] = torch.cuda.Event()
                    rec["ev"].record(s_out)
                if prev is not None:
                    finalize(prev)
                prev = rec
            if prev is not None:
                finalize(prev)
        return results

    def _loader_items(self, data_loader):
        """Loader tuples ``(split_observe_dict, split_clean_s0_dict, split_clean_s1_dict, gap, wav_name)`` ->
        :class:`coalesce.Item` (B utterances x n_split chunks, keyed by the chunk shapes [M,T,F] / [S,T,F]); the payload
        holds the splits, the clean sources, the per-utterance gaps and names"""
        from .coalesce import Item
        for i, (obs_d, s0_d, s1_d, gap, wav_name) in enumerate(data_loader):
            K = len(obs_d)
            obs = [torch.as_tensor(obs_d[str(k)]) for k in range(K)]
            s0 = [torch.as_tensor(s0_d[str(k)]) for k in range(K)]
            s1 = [torch.as_tensor(s1_d[str(k)]) for k in range(K)]
            B, M, T, F = obs[0].shape
            gaps = [int(gap[b]) if hasattr(gap, "__len__") else int(gap) for b in range(B)]
            names = [wav_name] * B if isinstance(wav_name, str) else list(wav_name)
            yield Item(i, B, K, ((M, T, F), (self.num_spks, T, F)), dict(obs=obs, s0=s0, s1=s1, gaps=gaps, names=names))

    def _tap_references(self, data_loader, refs):
        """Passes the loader's items through and leaves in ``refs[wav_name]`` the reference waves of every recording:
        float32 [S + 1, n] on the host, the iSTFT (device) of the clean spectrograms at ref_ch and, last row, of the
        observation at ref_ch, the chunks stitched with the padded tail dropped."""
        for item in data_loader:
            obs_d, s0_d, s1_d, gap, wav_name = item
            K = len(obs_d)
            with torch.cuda.device(self.device):
                spec = torch.stack([torch.stack([torch.as_tensor(s0_d[str(k)])[:, self.ref_ch],
                                                 torch.as_tensor(s1_d[str(k)])[:, self.ref_ch],
                                                 torch.as_tensor(obs_d[str(k)])[:, self.ref_ch]], dim=1)
                                    for k in range(K)], dim=1).to(self.device)               # [B, K, S + 1, T, F]
                w = S._istft_hip(spec, False).permute(0, 2, 1, 3)                              # [B, S + 1, K, n]
                w = w.reshape(w.shape[0], w.shape[1], -1).cpu().numpy()
            for b in range(w.shape[0]):
                g = int(gap[b]) if hasattr(gap, "__len__") else int(gap)
                name = wav_name if isinstance(wav_name, str) else wav_name[b]
                refs[name] = w[b, :, : w.shape[2] - g]
            yield item

    def _fill_spec(self, c, rows):
        """stage one loader chunk: the observation [M,T,F] and the clean sources at ref_ch [S,T,F] (tester.py:889-890)"""
        p = c.item.payload
        rows[0].copy_(p["obs"][c.split][c.b])
        rows[1][0].copy_(p["s0"][c.split][c.b, self.ref_ch])
        rows[1][1].copy_(p["s1"][c.split][c.b, self.ref_ch])

    @staticmethod
    def _write_scores(saveDir, scores):
        """``<saveDir>/scores.json``: {wav_name: Score.as_dict()} and the "mean" entry"""
        import json
        import os
        from . import score as SC
        doc = {str(name): sc.as_dict() for name, sc in scores.items()}
        doc["mean"] = SC.mean_of(list(scores.values()))
        with open(os.path.join(saveDir, "scores.json"), "w") as fh:
            json.dump(doc, fh, indent=1)

    def _inference_coalesced(self, data_loader, saveDir, fs, write, max_batch, depth, scores=None):
        import os
        results = {}
        items = self._loader_items(data_loader)
        if scores is None:
            batches = self._coalesced(items, self._fill_spec, self._spec_pass, torch.complex64, max_batch, depth,
                                      lambda c: str(c.item.payload["names"][c.b]))
        else:
            def keyed(src):
                for it in src:
                    it.key = tuple(it.key) + ((1,),)               # the chunk's valid count rides as a third input
                    yield it

            def fill(c, rows):
                self._fill_spec(c, rows)
                n = (c.item.key[0][1] - 1) * S.HOP
                last = c.split == c.item.n_split - 1
                rows[2].copy_(self._nv_bits([n - c.item.payload["gaps"][c.b] if last else n], torch.complex64)[0])

            batches = self._coalesced(keyed(items), fill, self._spec_pass_score, torch.complex64, max_batch, depth,
                                      lambda c: str(c.item.payload["names"][c.b]),
                                      extra_rows=lambda ex, n: self._score_rows(ex, n, True))
        for it in batches:
            p = it.payload
            if scores is not None:
                n = (it.key[0][1] - 1) * S.HOP
                for b in range(it.n_b):
                    nv = [n] * (it.n_split - 1) + [n - p["gaps"][b]]
                    scores[p["names"][b]] = self._recording_score([it.outputs[k][b][1:] for k in range(it.n_split)], nv)
                it.outputs = [[row[0] for row in split] for split in it.outputs]
            for b in range(it.n_b):
                wav = np.stack([S.stitch_int16([it.outputs[k][b][s] for k in range(it.n_split)], p["gaps"][b])
                                for s in range(self.num_spks)])                               # [S, n_total]
                name = p["names"][b]
                results[name] = wav
                if write:
                    for s in range(self.num_spks):
                        S.write_wav_pcm24(os.path.join(saveDir, f"{name}_{s}.wav"), wav[s], fs)
        return results

    def to_wav_int16(self, enhanced_chunks: List[torch.Tensor], gap: int) -> np.ndarray:
        """tester.py:949-969 for one recording: list over 4 s splits of complex [S,T,F] -> int16 [S, n_samples].
        One batched iSTFT over all (split, speaker) spectrograms and one device-to-host copy."""
        pcm = S.istft_int16(torch.stack([torch.as_tensor(ch) for ch in enhanced_chunks])).cpu().numpy()   # [n_split, S, n]
        return np.stack([S.stitch_int16([pcm[k, s] for k in range(pcm.shape[0])], gap) for s in range(self.num_spks)])
