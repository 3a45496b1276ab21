"""Source localisation on the device (csrc/doa.hip, C ABI ``misonet_doa`` in include/misonet.h).

Steered-response-power maps with and without the phase transform (SRP, SRP-PHAT; DiBiase 2000) and MUSIC (Schmidt 1986) of a
mixture over a table of candidate delays, and the peaks of every map.  The delay table is built on the host, so one kernel
serves far-field directions and near-field points; with cACGMM masks as ``weight`` every class gets a map of its own.  This is
the project's own definition in the SRP-PHAT / MUSIC family; pyroomacoustics was not available and nothing here was compared
against it.

``directions``, ``far_field_delays``, ``near_field_delays``  -- the candidates and their delay tables (host, NumPy)
``Localizer``                                                 -- the options as plain data
``localize(spec, tau, pts, fs, ...)``                         -- the maps and peaks of spectra [B, F, M, T] -> ``DoaResult``
``localize_wav(wav, tau, pts, fs, ...)``                      -- the same of a recording [L, M], through the device STFT
``angular_error``                                             -- degrees between found and true directions (host)
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import itertools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from ._online import make_callable, spec_of

KINDS = ("srp", "srp_phat", "music")         # the kinds of misonet_doa_opts, in its numbering
MAX_SRC, MAX_CLASSES, MAX_CANDIDATES = 4, 8, 65536


def directions(n_az, elevations=(0.0,)):
    """unit vectors float64 [D, 3], D = len(elevations) * n_az: for every elevation (radians above the x-y plane) in turn, n_az
    azimuths 2 pi i / n_az"""
    if isinstance(n_az, bool) or not isinstance(n_az, (int, np.integer)) or n_az < 1:
        raise ValueError(f"n_az must be a positive integer, got {n_az!r}")
    el = np.atleast_1d(np.asarray(elevations, np.float64))
    if el.ndim != 1 or el.size < 1 or not np.isfinite(el).all():
        raise ValueError("elevations must be a non-empty list of finite angles")
    az = 2.0 * np.pi * np.arange(int(n_az)) / int(n_az)
    return np.concatenate([np.stack([np.cos(e) * np.cos(az), np.cos(e) * np.sin(az), np.full(az.shape, np.sin(e))], axis=1)
                           for e in el], axis=0)


def _geometry(mic, cand, c, name):
    mic = np.asarray(mic, np.float64)
    cand = np.asarray(cand, np.float64)
    if mic.ndim != 2 or mic.shape[1] != 3 or mic.shape[0] < 1 or not np.isfinite(mic).all():
        raise ValueError(f"mic {mic.shape} must be finite [M, 3]")
    if cand.ndim != 2 or cand.shape[1] != 3 or cand.shape[0] < 1 or not np.isfinite(cand).all():
        raise ValueError(f"{name} {cand.shape} must be finite [D, 3]")
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or not c > 0:
        raise ValueError(f"c must be finite and > 0, got {c!r}")
    return mic, cand


def far_field_delays(mic, dirs, c=343.0):
    """tau[d, m] = -u_d . (p_m - mean p) / c, seconds, float64 [D, M]: a plane wave FROM direction u_d reaches a microphone
    that lies towards u_d earlier"""
    mic, dirs = _geometry(mic, dirs, c, "dirs")
    return -(dirs @ (mic - mic.mean(axis=0)).T) / float(c)


def near_field_delays(mic, points, c=343.0):
    """tau[d, m] = |x_d - p_m| / c minus its mean over m, seconds, float64 [D, M]"""
    mic, points = _geometry(mic, points, c, "points")
    t = np.sqrt(((points[:, None, :] - mic[None, :, :]) ** 2).sum(axis=2)) / float(c)
    return t - t.mean(axis=1, keepdims=True)


def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


@dataclasses.dataclass(frozen=True)
class Localizer:
    """One plain-data description of the localisation (``misonet_doa_opts`` of include/misonet.h).

    kind      "srp", "srp_phat" (the maximum of the map is a source) or "music" (the minimum of q is; ``DoaResult.map`` is 1 / q)
    num_src   S: the peaks taken from every map; for "music" also the dimension of the signal subspace (S <= M - 1)
    block     frames per map; 0 = one map over all frames
    hop       frames between maps; 0 = block
    band      (f_lo_hz, f_hi_hz): the bins whose centre lies inside, or None for all bins; ``bins`` = (f_lo, f_hi), inclusive bin
              indices, instead (not both)
    min_sep   peaks are kept at least this far apart, in the unit of ``pts`` (for unit vectors: the chord 2 sin(angle / 2))
    """
    kind: str = "srp_phat"
    num_src: int = 1
    block: int = 0
    hop: int = 0
    band: Optional[Tuple[float, float]] = None
    bins: Optional[Tuple[int, int]] = None
    min_sep: float = 0.0

    @classmethod
    def of(cls, spec) -> "Localizer":
        """None or True (the defaults), a Localizer, a kind name, or a dict of the fields above"""
        return spec_of(cls, spec, "localizer", "localizer must be None, True, a Localizer, a kind name or a dict of its fields",
                       "kind")

    def validate(self, num_mic=None, num_cand=None, num_frames=None) -> "Localizer":
        """ValueError for a bad field -- before anything is launched (the library checks again: MISONET_EINVAL)"""
        if self.kind not in KINDS:
            raise ValueError(f"localizer kind {self.kind!r}: one of {KINDS}")
        if not _integer(self.num_src) or not 1 <= self.num_src <= MAX_SRC:
            raise ValueError(f"localizer num_src must be an integer in [1, {MAX_SRC}], got {self.num_src!r}")
        if not _integer(self.block) or self.block < 0 or not _integer(self.hop) or self.hop < 0:
            raise ValueError(f"localizer block and hop must be integers >= 0, got {self.block!r}, {self.hop!r}")
        v = self.min_sep
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"localizer min_sep must be finite and >= 0, got {v!r}")
        if self.band is not None and self.bins is not None:
            raise ValueError("localizer takes band (Hz) or bins (indices), not both")
        if self.band is not None:
            if len(self.band) != 2 or not all(isinstance(h, (int, float)) and not isinstance(h, bool) and math.isfinite(h)
                                              for h in self.band) or not 0 <= self.band[0] <= self.band[1]:
                raise ValueError(f"localizer band must be (f_lo_hz, f_hi_hz) with 0 <= f_lo <= f_hi, got {self.band!r}")
        if self.bins is not None:
            if len(self.bins) != 2 or not all(_integer(i) for i in self.bins) or not 0 <= self.bins[0] <= self.bins[1]:
                raise ValueError(f"localizer bins must be (f_lo, f_hi) with 0 <= f_lo <= f_hi, got {self.bins!r}")
        if num_mic is not None:
            if not 2 <= num_mic <= 8:
                raise ValueError(f"localisation needs 2 <= M <= 8 microphones, got {num_mic}")
            if self.kind == "music" and self.num_src > num_mic - 1:
                raise ValueError(f"music needs num_src <= M - 1 = {num_mic - 1}, got {self.num_src}")
        if num_cand is not None:
            if not 1 <= num_cand <= MAX_CANDIDATES:
                raise ValueError(f"localisation takes 1 <= D <= {MAX_CANDIDATES} candidates, got {num_cand}")
            if self.num_src > num_cand:
                raise ValueError(f"num_src {self.num_src} exceeds the {num_cand} candidates")
        if num_frames is not None and self.block > num_frames:
            raise ValueError(f"localizer block {self.block} exceeds the {num_frames} frames")
        return self

    def bin_range(self, num_freq, fs) -> Tuple[int, int]:
        """(f_lo, f_hi), inclusive, among num_freq bins at sample rate fs; ValueError when no bin is left"""
        F = int(num_freq)
        if self.bins is not None:
            lo, hi = int(self.bins[0]), int(self.bins[1])
        elif self.band is not None:
            nfft = 2 * (F - 1) if F > 1 else 2
            lo = int(math.ceil(self.band[0] * nfft / fs - 1e-9))
            hi = min(int(math.floor(self.band[1] * nfft / fs + 1e-9)), F - 1)
        else:
            lo, hi = 0, F - 1
        if not 0 <= lo <= hi < F:
            raise ValueError(f"the band leaves no bin: bins [{lo}, {hi}] of {F}")
        return lo, hi

    def c_opts(self, num_freq, fs) -> "_lib.DoaOpts":
        lo, hi = self.bin_range(num_freq, fs)
        return _lib.DoaOpts(KINDS.index(self.kind), int(self.num_src), int(self.block), int(self.hop), lo, hi, float(self.min_sep))


def num_blocks(num_frames, block=0, hop=0) -> int:
    """N, the maps per recording (``misonet_doa_blocks``); ValueError for block > T"""
    n = int(_lib.lib().misonet_doa_blocks(int(num_frames), int(block), int(hop)))
    if n < 0:
        raise ValueError(f"block {block} / hop {hop} do not fit {num_frames} frames")
    return n


class DoaResult(NamedTuple):
    """q float64 [B, K, N, D] as the kernel defines it; map: q for the SRP kinds, 1 / max(q, 1e-12) for music (large at a source
    for every kind); peak int32 [B, K, N, S] (-1: no candidate left) and value float64, q at the peak; used int32 [B, K, N], the
    bins that entered the map; fail int32 [B, K, N]: bit 0 a bin with a non-finite sample or weight was skipped, bit 1 no bin
    was left (the map is 0).  With image input [B, S, F, M, T] every field has the leading axes [B, S, ...]."""
    q: object
    map: object
    peak: object
    value: object
    used: object
    fail: object


def _check_tables(tau, pts, B, M):
    tau = np.ascontiguousarray(np.asarray(tau, np.float64))
    pts = np.ascontiguousarray(np.asarray(pts, np.float64))
    if tau.ndim == 2:
        tau = tau[None]
    if tau.ndim != 3 or tau.shape[2] != M or tau.shape[0] not in (1, B):
        raise ValueError(f"tau {tau.shape} must be [D, M] or [Bg, D, M] with M = {M} and Bg in (1, {B})")
    D = tau.shape[1]
    if pts.shape != (D, 3):
        raise ValueError(f"pts {pts.shape} must be [D, 3] = [{D}, 3]")
    if not np.isfinite(tau).all() or not np.isfinite(pts).all():
        raise ValueError("tau and pts must be finite")
    return tau, pts, D


def localize(spec, tau, pts, fs, kind="srp_phat", num_src=1, block=0, hop=0, band=None, bins=None, min_sep=0.0, weight=None,
             device=None, return_debug=False, *, localizer=None):
    """The maps and peaks of ``spec`` complex [B, F, M, T] (the beamformers' layout) -- or of images [B, S, F, M, T], run as B S
    recordings -- over the candidates of ``tau`` float64 [D, M] or [Bg, D, M] (seconds; Bg 1 or the number of recordings) with
    the coordinates ``pts`` [D, 3].  ``weight`` float [B, K, F, T] (for instance the cACGMM masks): a map per class.  The options
    are the fields of :class:`Localizer` (``localizer``: a whole Localizer, kind name or dict, which wins).  Returns a
    :class:`DoaResult` -- on the CPU (NumPy) when ``spec`` was an ndarray, device tensors otherwise; with ``return_debug`` also C
    complex128 [B, K, N, F, M, M], the per-bin matrices that were steered."""
    import torch
    from ._online import _dev_c64
    opt = (Localizer(kind=kind, num_src=num_src, block=block, hop=hop, band=band, bins=bins, min_sep=min_sep)
           if localizer is None else Localizer.of(localizer))
    shape = tuple(np.shape(spec))
    if len(shape) not in (4, 5):
        raise ValueError(f"spec {shape} must be [B, F, M, T] or [B, S, F, M, T]")
    lead = shape[:-3]
    F, M, T = shape[-3:]
    B = int(np.prod(lead))
    if B < 1 or F < 1 or T < 1:
        raise ValueError("B, F and T must be positive")
    if isinstance(fs, bool) or not isinstance(fs, (int, float, np.integer, np.floating)) or not math.isfinite(fs) or not fs > 0:
        raise ValueError(f"fs must be finite and > 0, got {fs!r}")
    tau, pts, D = _check_tables(tau, pts, B, M)
    opt.validate(M, D, T)                                                    # before any copy or launch
    opt.bin_range(F, fs)
    K = 1
    if weight is not None:
        wshape = tuple(np.shape(weight))
        if len(wshape) != 4 or wshape[0] != B or wshape[2:] != (F, T) or not 1 <= wshape[1] <= MAX_CLASSES:
            raise ValueError(f"weight {wshape} must be [B, K, F, T] = [{B}, 1..{MAX_CLASSES}, {F}, {T}]")
        if len(lead) != 1:
            raise ValueError("weights go with spectra [B, F, M, T], not with images")
        K = wshape[1]
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    y, np_in = _dev_c64(spec, device)
    y = y.reshape(B, F, M, T)
    L = _lib.lib()
    opts = opt.c_opts(F, fs)
    N = L.misonet_doa_blocks(T, opts.block, opts.hop)
    nws = L.misonet_doa_workspace_bytes(B, K, F, M, T, D, C.byref(opts))
    if N < 0 or nws < 0:
        _lib.check(L.misonet_doa(None, None, None, tau.shape[0], None, B, K, F, M, T, D, float(fs), C.byref(opts), None, None,
                                 None, None, None, 0, None))                 # the message of the failed check
        _lib.check(_lib.EINVAL)
    Sn = int(opt.num_src)
    dev = y.device
    w = None
    if weight is not None:
        w = torch.as_tensor(weight).to(dev).to(torch.float32).contiguous()
    tau_d = torch.from_numpy(tau).to(dev)
    pts_d = torch.from_numpy(pts).to(dev)
    ws = torch.empty(max(int(nws), 16), dtype=torch.uint8, device=dev)
    q = torch.empty((B, K, N, D), dtype=torch.float64, device=dev)
    peak = torch.empty((B, K, N, Sn), dtype=torch.int32, device=dev)
    value = torch.empty((B, K, N, Sn), dtype=torch.float64, device=dev)
    fail = torch.empty((B, K, N), dtype=torch.int32, device=dev)
    used = torch.empty((B, K, N), dtype=torch.int32, device=dev)
    cmat = torch.empty((B, K, N, F, M, M), dtype=torch.complex128, device=dev) if return_debug else None
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        _lib.check(L.misonet_doa(y.data_ptr(), w.data_ptr() if w is not None else None, tau_d.data_ptr(), tau.shape[0],
                                 pts_d.data_ptr(), B, K, F, M, T, D, float(fs), C.byref(opts), q.data_ptr(), peak.data_ptr(),
                                 value.data_ptr(), fail.data_ptr(), ws.data_ptr(), ws.numel(), st))
        _lib.check(L.misonet_doa_debug(ws.data_ptr(), B, K, F, M, T, D, C.byref(opts),
                                       cmat.data_ptr() if return_debug else None, used.data_ptr(), None, st))
    mp = 1.0 / torch.clamp(q, min=1e-12) if opt.kind == "music" else q
    out = [q, mp, peak, value, used, fail]
    if len(lead) == 2:
        out = [t.reshape(lead + t.shape[1:]) for t in out]
        cmat = cmat.reshape(lead + cmat.shape[1:]) if cmat is not None else None
    if np_in:
        out = [t.cpu().numpy() for t in out]
        cmat = cmat.cpu().numpy() if cmat is not None else None
    res = DoaResult(*out)
    return (res, cmat) if return_debug else res


def localize_wav(wav, tau, pts, fs=16000, device=None, **kw):
    """A recording float [L, M] (time-major, as ``read_wav`` returns it) or [B, L, M] -> :class:`DoaResult` of its STFT (the
    device STFT of :mod:`misonet_amd.stft`: 256-point frames every 64 samples, 129 bins, the recording zero-padded to whole
    hops).  The keywords are those of :func:`localize`.  The result is on the CPU (NumPy)."""
    import torch
    from . import stft as S
    w = np.asarray(wav)
    if w.ndim == 2:
        w = w[None]
    if w.ndim != 3 or w.shape[1] < 1 or not 2 <= w.shape[2] <= 8:
        raise ValueError(f"wav {np.shape(wav)} must be [L, M] or [B, L, M] with 2 <= M <= 8")
    B, L, M = w.shape
    T = (L + (-L) % S.HOP) // S.HOP + 1
    tau_c, pts_c, D = _check_tables(tau, pts, B, M)
    opt = Localizer.of(kw["localizer"]) if kw.get("localizer") is not None else Localizer(
        **{k: v for k, v in kw.items() if k in {f.name for f in dataclasses.fields(Localizer)}})
    opt.validate(M, D, T)                                                    # before the STFT is launched
    opt.bin_range(S.N_FREQ, fs)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    sig = torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(device)
    sig = torch.nn.functional.pad(sig, (0, 0, 0, (-L) % S.HOP)).contiguous()                 # [B, Lp, M]
    spec = S.stft_hip(sig).permute(0, 3, 1, 2).contiguous()                                  # [B, F, M, T]
    res = localize(spec, tau_c, pts_c, fs, device=device, **kw)
    if kw.get("return_debug"):
        return DoaResult(*[t.cpu().numpy() for t in res[0]]), res[1].cpu().numpy()
    return DoaResult(*[t.cpu().numpy() for t in res])


def angular_error(dirs, peak, truth):
    """Degrees between the found and the true directions.  dirs [D, 3] (unit vectors); peak int [..., S] (indices into dirs,
    -1: none); truth [S, 3] unit vectors or int [S] indices.  The found peaks are matched to the truths by the permutation of
    the smallest total error; a missing peak counts 180.  Returns float64 [..., S], in the order of ``truth``."""
    dirs = np.asarray(dirs, np.float64)
    peak = np.asarray(peak)
    tr = np.asarray(truth)
    tr = dirs[tr] if tr.ndim == 1 and np.issubdtype(tr.dtype, np.integer) else np.asarray(tr, np.float64)
    S = peak.shape[-1]
    if tr.shape != (S, 3):
        raise ValueError(f"truth {tr.shape} must be [S, 3] or S indices, S = {S}")
    out = np.zeros(peak.shape, np.float64)
    for at in np.ndindex(*peak.shape[:-1]):
        p = peak[at]
        err = np.full((S, S), 180.0)                                         # [truth, found]
        for j in range(S):
            if p[j] >= 0:
                u = dirs[p[j]]
                cosv = (tr @ u) / np.maximum(np.linalg.norm(tr, axis=1) * np.linalg.norm(u), 1e-300)
                err[:, j] = np.degrees(np.arccos(np.clip(cosv, -1.0, 1.0)))
        best = min(itertools.permutations(range(S)), key=lambda pm: sum(err[i, pm[i]] for i in range(S)))
        out[at] = [err[i, best[i]] for i in range(S)]
    return out


# ``misonet_amd.localize`` names both this module and the function above: ``misonet_amd.localize(spec, tau, pts, fs)`` works
# either way
make_callable(__name__)
