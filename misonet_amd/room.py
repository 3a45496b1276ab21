"""Room simulator on the device (csrc/room.hip, C ABI ``misonet_room_*`` in include/misonet.h).

Image-source room impulse responses of a shoebox with one reflection coefficient per wall, and the scene mixer that convolves dry
sources with them: reverberant, noisy, multi-microphone scenes whose images, early parts and RIRs are known exactly -- the
material the array-processing chain and the scores of this package are measured and tuned on.  This is the project's own
definition in the Allen & Berkley (1979) family; nothing here was compared against pyroomacoustics, gpuRIR, rir_generator or
sms_wsj.

``beta_from_rt60(dim, rt60)``  -- Sabine's reflection coefficient of a nominal RT60 (nominal: ``beta`` is the contract)
``Room``                       -- the shoebox as plain data
``rir(room, src, mic, fs, length)``      -- float64 [S, M, Lh], or [B, S, M, Lh] for batched geometry
``direct_sample(room, src, mic, fs)``    -- floor of the smallest direct-path delay over the microphones, per source
``mix(sources, rirs, fs)``     -- (images, early, mixture)
``simulate(sources, room, src, mic, fs, rir_len, snr_db)``  -- a whole ``Scene``; ``Scene.wav`` is float32 [L, M], the layout
                                  ``enhance_recording``, ``separate_recording`` and ``dereverb_wav`` take
``schroeder_t30(h, fs)``       -- host: the decay time read off a RIR
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _lib

W = 80                        # support of the fractional-delay kernel in samples
MAX_B, MAX_S, MAX_M, MAX_LH, MAX_L = 4096, 4, 16, 1 << 16, 1 << 24
FAIL_GEOMETRY, FAIL_NEAR, FAIL_IMAGES = 1, 2, 4          # the bits of ``fail``


def beta_from_rt60(dim, rt60) -> float:
    """Sabine: beta = sqrt(1 - 0.161 V / (A rt60)) for the shoebox ``dim`` = (Lx, Ly, Lz), one value for all six walls.
    ValueError where that is outside [0, 1): the room cannot be that dry."""
    lx, ly, lz = (float(v) for v in dim)
    if not (min(lx, ly, lz) > 0 and math.isfinite(lx + ly + lz)):
        raise ValueError(f"room dim must be three finite edges > 0, got {dim!r}")
    if not (isinstance(rt60, (int, float)) and math.isfinite(rt60) and rt60 > 0):
        raise ValueError(f"rt60 must be finite and > 0, got {rt60!r}")
    vol, area = lx * ly * lz, 2.0 * (lx * ly + ly * lz + lx * lz)
    b2 = 1.0 - 0.161 * vol / (area * float(rt60))
    if not 0.0 <= b2 < 1.0:
        raise ValueError(f"rt60 {rt60} s needs beta^2 = {b2:.4f} in a room {lx} x {ly} x {lz} m: outside [0, 1)")
    return math.sqrt(b2)


@dataclasses.dataclass(frozen=True)
class Room:
    """A shoebox with one corner at the origin.

    dim    (Lx, Ly, Lz) in metres, each > 0
    beta   the reflection coefficients in [0, 1): one number for all walls, or six ordered x0, x1, y0, y1, z0, z1 ("0": the wall
           at coordinate 0, "1": the wall at L)
    rt60   instead of ``beta``: a NOMINAL reverberation time, turned into one beta by Sabine's formula; the decay time read off
           the RIR differs from it
    c      the speed of sound in m/s
    """
    dim: tuple
    beta: object = None
    rt60: Optional[float] = None
    c: float = 343.0

    def validate(self) -> "Room":
        """ValueError for a bad field -- before anything is launched"""
        d = np.asarray(self.dim, np.float64)
        if d.shape != (3,) or not np.isfinite(d).all() or not (d > 0).all():
            raise ValueError(f"room dim must be three finite edges > 0, got {self.dim!r}")
        if (self.beta is None) == (self.rt60 is None):
            raise ValueError("give exactly one of beta and rt60")
        if isinstance(self.c, bool) or not (isinstance(self.c, (int, float)) and math.isfinite(self.c) and self.c > 0):
            raise ValueError(f"c must be finite and > 0, got {self.c!r}")
        b = self.betas()
        if not ((b >= 0) & (b < 1)).all():
            raise ValueError(f"every beta must lie in [0, 1), got {self.beta!r}")
        return self

    def betas(self) -> np.ndarray:
        """float64 [6]"""
        if self.beta is None:
            return np.full(6, beta_from_rt60(self.dim, self.rt60))
        b = np.asarray(self.beta, np.float64)
        if b.shape == ():
            return np.full(6, float(b))
        if b.shape != (6,):
            raise ValueError(f"beta must be one number or six (x0, x1, y0, y1, z0, z1), got shape {b.shape}")
        return b.copy()


@dataclasses.dataclass
class Scene:
    """What ``simulate`` returns.  wav float32 [L, M] (mix + noise); images and early float32 [S, L, M]; mix and noise float32
    [L, M]; rir float64 [S, M, Lh]; fail int32 [S, M]; split int32 [S], the first late tap of each source."""
    wav: object
    images: object
    early: object
    mix: object
    noise: object
    rir: object
    fail: object
    split: object
    fs: int
    snr_db: Optional[float]


def _rooms(room):
    rooms = [room] if isinstance(room, Room) else list(room)
    if not rooms or not all(isinstance(r, Room) for r in rooms):
        raise TypeError("room must be a Room or a sequence of them")
    cs = {float(r.validate().c) for r in rooms}
    if len(cs) != 1:
        raise ValueError("the rooms of one call share one speed of sound")
    return rooms, isinstance(room, Room), cs.pop()


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _geometry(room, src, mic):
    """-> rooms, single, c, src float64 [B, S, 3], mic float64 [B, M, 3] on the host, whether the result is an ndarray"""
    rooms, single, c = _rooms(room)
    np_in = not (isinstance(src, torch.Tensor) or isinstance(mic, torch.Tensor))
    s, m = np.asarray(_host(src), np.float64), np.asarray(_host(mic), np.float64)
    if single:
        if s.ndim != 2 or m.ndim != 2:
            raise ValueError(f"src {s.shape} and mic {m.shape} must be [S, 3] and [M, 3] for one Room")
        s, m = s[None], m[None]
    if s.ndim != 3 or m.ndim != 3 or s.shape[2] != 3 or m.shape[2] != 3 or s.shape[0] != len(rooms) or m.shape[0] != len(rooms):
        raise ValueError(f"src {s.shape} and mic {m.shape} must be [B, S, 3] and [B, M, 3] for {len(rooms)} room(s)")
    B, S, M = len(rooms), s.shape[1], m.shape[1]
    if not (1 <= B <= MAX_B and 1 <= S <= MAX_S and 1 <= M <= MAX_M):
        raise ValueError(f"B, S, M = {B}, {S}, {M} outside [1, {MAX_B}], [1, {MAX_S}], [1, {MAX_M}]")
    return rooms, single, c, s, m, np_in


def _check_fs(fs):
    if isinstance(fs, bool) or not (isinstance(fs, (int, float, np.integer, np.floating)) and math.isfinite(fs) and fs > 0):
        raise ValueError(f"fs must be finite and > 0, got {fs!r}")
    return float(fs)


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def rir(room, src, mic, fs, length, max_order=None, return_fail=False, device=None):
    """Image-source RIRs.  room a :class:`Room` with src [S, 3] and mic [M, 3] -> float64 [S, M, Lh]; a sequence of B rooms
    with src [B, S, 3] and mic [B, M, 3] -> [B, S, M, Lh].  ``length`` = Lh taps at ``fs``; ``max_order``: None (no limit) or
    the largest reflection count kept.  With ``return_fail`` also int32 [.., S, M]: bit 0 bad geometry (a point outside the room,
    a non-finite coordinate; the RIR is zero), bit 1 an image closer than 1e-3 m was dropped, bit 2 more than 2^27 images or more
    than 255 image indices along an axis (the RIR is zero).  The results are ndarrays when src and mic were, device tensors
    otherwise."""
    rooms, single, c, s, m, np_in = _geometry(room, src, mic)
    fs = _check_fs(fs)
    if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or not 1 <= length <= MAX_LH:
        raise ValueError(f"length must be an integer in [1, {MAX_LH}], got {length!r}")
    if max_order is not None and (isinstance(max_order, bool) or not isinstance(max_order, (int, np.integer)) or max_order < 0):
        raise ValueError(f"max_order must be None or an integer >= 0, got {max_order!r}")
    dev = _device(device)
    B, S, M, Lh = len(rooms), s.shape[1], m.shape[1], int(length)
    geo = np.concatenate([np.stack([np.asarray(r.dim, np.float64) for r in rooms]).ravel(),
                          np.stack([r.betas() for r in rooms]).ravel(), s.ravel(), m.ravel()])
    g = torch.from_numpy(geo).to(dev)                                          # one copy: room | beta | src | mic
    o = np.cumsum([0, 3 * B, 6 * B, 3 * B * S]) * 8
    out = torch.empty((B, S, M, Lh), dtype=torch.float64, device=dev)
    fail = torch.empty((B, S, M), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        p = g.data_ptr()
        _lib.check(_lib.lib().misonet_room_rir(p + int(o[0]), p + int(o[1]), p + int(o[2]), p + int(o[3]), B, S, M, fs, c, Lh,
                                               -1 if max_order is None else int(max_order), out.data_ptr(), fail.data_ptr(),
                                               _lib.stream_ptr(dev)))
    if single:
        out, fail = out[0], fail[0]
    if np_in:
        out, fail = out.cpu().numpy(), fail.cpu().numpy()
    return (out, fail) if return_fail else out


def direct_sample(room, src, mic, fs):
    """floor of the smallest direct-path delay tau = d fs / c over the microphones, per source: int64 ndarray [S] (or [B, S]).
    Host arithmetic; nothing is launched."""
    rooms, single, c, s, m, _ = _geometry(room, src, mic)
    fs = _check_fs(fs)
    d = np.sqrt(((s[:, :, None, :] - m[:, None, :, :]) ** 2).sum(-1))         # [B, S, M]
    out = np.floor(d.min(-1) * fs / c).astype(np.int64)
    return out[0] if single else out


def _f32_dev(a, dev):
    if isinstance(a, torch.Tensor):
        return a.to(dev).to(torch.float32), False
    return torch.from_numpy(np.asarray(a, np.float32)).to(dev), True


def mix(sources, rirs, fs, early_ms=50.0, out_len=None, direct=None, device=None):
    """Scene mixing.  sources float32 [S, L] (any strides; read in place), rirs float64 [S, M, Lh] -> (images float32
    [S, M, Lo], early float32 [S, M, Lo], mixture float32 [M, Lo]); with a leading B on both, on all three.  images = the
    convolution, early = its part through the taps before ``split = direct + round(early_ms fs / 1000)``, mixture = the sum of
    the images.  ``direct`` int [S] (or [B, S]): the direct-path sample of each source, as :func:`direct_sample` gives it;
    None: the tap of the largest magnitude, the smallest over the microphones, found on the device.  ``out_len`` = Lo, None: L;
    at most L + Lh - 1.  ndarrays in, ndarrays out."""
    fs = _check_fs(fs)
    if isinstance(early_ms, bool) or not (isinstance(early_ms, (int, float)) and math.isfinite(early_ms) and early_ms >= 0):
        raise ValueError(f"early_ms must be finite and >= 0, got {early_ms!r}")
    if np.ndim(sources) not in (2, 3) or np.ndim(rirs) != np.ndim(sources) + 1:
        raise ValueError(f"sources {tuple(np.shape(sources))} must be [S, L] with rirs [S, M, Lh], or both with a leading B")
    single = np.ndim(sources) == 2
    shx, shh = ((1,) if single else ()) + tuple(np.shape(sources)), ((1,) if single else ()) + tuple(np.shape(rirs))
    (B, S, L), (M, Lh) = shx, shh[2:]
    if shh[:2] != (B, S):
        raise ValueError(f"sources {shx} and rirs {shh} disagree on B or S")
    if not (1 <= B <= MAX_B and 1 <= S <= MAX_S and 1 <= M <= MAX_M and 1 <= Lh <= MAX_LH and 1 <= L <= MAX_L):
        raise ValueError(f"B, S, M, Lh, L = {B}, {S}, {M}, {Lh}, {L} outside the limits of misonet_room_mix")
    Lo = L if out_len is None else out_len
    if isinstance(Lo, bool) or not isinstance(Lo, (int, np.integer)) or not 1 <= Lo <= L + Lh - 1:
        raise ValueError(f"out_len must be an integer in [1, L + Lh - 1] = [1, {L + Lh - 1}], got {out_len!r}")
    dev = _device(device if device is not None else
                  (sources.device if isinstance(sources, torch.Tensor) and sources.is_cuda else None))
    x, np_in = _f32_dev(sources, dev)
    np_in = np_in and not isinstance(rirs, torch.Tensor)
    h = (rirs if isinstance(rirs, torch.Tensor) else torch.from_numpy(np.asarray(rirs))).to(dev).to(torch.float64)
    if single:
        x, h = x[None], h[None]
    h = h.contiguous()
    if any(st < 0 for st in x.stride()) or x.stride(2) < 1:
        x = x.contiguous()
    ahead = int(round(float(early_ms) * fs / 1000.0))
    if direct is None:
        first = h.abs().argmax(dim=3).amin(dim=2)                              # [B, S], on the device: no synchronisation
    else:
        first = torch.from_numpy(np.asarray(_host(direct), np.int64).reshape(B, S)).to(dev)
    split = (first + ahead).clamp(0, Lh).to(torch.int32).contiguous()
    images = torch.empty((B, S, M, Lo), dtype=torch.float32, device=dev)
    early = torch.empty((B, S, M, Lo), dtype=torch.float32, device=dev)
    mixture = torch.empty((B, M, Lo), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().misonet_room_mix(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), h.data_ptr(), split.data_ptr(),
                                               B, S, M, L, Lh, int(Lo), images.data_ptr(), early.data_ptr(), mixture.data_ptr(),
                                               _lib.stream_ptr(dev)))
    res = [images, early, mixture]
    if single:
        res = [r[0] for r in res]
    if np_in:
        res = [r.cpu().numpy() for r in res]
    return tuple(res)


def simulate(sources, room, src, mic, fs, rir_len, snr_db=None, seed=0, early_ms=50.0, max_order=None, device=None):
    """One scene.  sources float32 [S, L] dry, ``room`` a :class:`Room`, src [S, 3], mic [M, 3] -> a :class:`Scene`: the RIRs
    of ``rir_len`` taps, the images and their early parts (``early_ms`` past each source's direct path), their sum, and -- with
    ``snr_db`` -- white sensor noise from ``torch.randn`` under a device generator seeded with ``seed``, scaled so that the
    float64 power of the clean mixture over all microphones stands ``snr_db`` above the noise's.  The noise samples are torch's:
    the same for one torch version and device kind, NOT pinned across torch versions.  ndarrays in, ndarrays out."""
    if not isinstance(room, Room):
        raise TypeError("simulate takes one Room")
    if np.ndim(sources) != 2:
        raise ValueError(f"sources {tuple(np.shape(sources))} must be [S, L]")
    if snr_db is not None and (isinstance(snr_db, bool) or not (isinstance(snr_db, (int, float)) and math.isfinite(snr_db))):
        raise ValueError(f"snr_db must be None or finite, got {snr_db!r}")
    np_in = not isinstance(sources, torch.Tensor)
    if np.shape(sources)[0] != np.shape(src)[0]:
        raise ValueError(f"{np.shape(sources)[0]} source signals for {np.shape(src)[0]} source positions")
    dev = _device(device)
    s_t = torch.as_tensor(_host(src), dtype=torch.float64)
    m_t = torch.as_tensor(_host(mic), dtype=torch.float64)
    h, fail = rir(room, s_t, m_t, fs, rir_len, max_order=max_order, return_fail=True, device=dev)
    direct = direct_sample(room, s_t, m_t, fs)
    x, _ = _f32_dev(sources, dev)
    images, early, clean = mix(x, h, fs, early_ms=early_ms, out_len=x.shape[1], direct=direct, device=dev)
    split = torch.from_numpy(np.minimum(direct + int(round(float(early_ms) * float(fs) / 1000.0)), int(rir_len)).astype(np.int32))
    clean_lm = clean.t().contiguous()                                          # [L, M]
    if snr_db is None:
        noise = torch.zeros_like(clean_lm)
        wav = clean_lm.clone()
    else:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        noise = torch.randn(clean_lm.shape, generator=gen, device=dev, dtype=torch.float32)
        p_mix = clean_lm.double().pow(2).sum()
        p_noise = noise.double().pow(2).sum()
        scale = torch.sqrt(p_mix / (p_noise * 10.0 ** (float(snr_db) / 10.0)))
        noise = (noise.double() * scale).float()
        wav = clean_lm + noise
    sc = Scene(wav=wav, images=images.permute(0, 2, 1).contiguous(), early=early.permute(0, 2, 1).contiguous(), mix=clean_lm,
               noise=noise, rir=h, fail=fail, split=split, fs=int(fs), snr_db=snr_db)
    if np_in:
        for f in ("wav", "images", "early", "mix", "noise", "rir", "fail", "split"):
            setattr(sc, f, getattr(sc, f).cpu().numpy())
    return sc


def schroeder_t30(h, fs) -> float:
    """Host: Schroeder's backward integration of h^2; the line fitted to the decay between -5 and -35 dB, extrapolated to
    60 dB.  NaN where the response does not fall 35 dB inside its length."""
    e = np.cumsum((np.asarray(_host(h), np.float64) ** 2)[::-1])[::-1]
    if e.ndim != 1 or not e[0] > 0:
        return float("nan")
    db = 10.0 * np.log10(np.maximum(e / e[0], 1e-300))
    if not (db <= -35.0).any():
        return float("nan")
    i0, i1 = int(np.argmax(db <= -5.0)), int(np.argmax(db <= -35.0))
    if i1 <= i0 + 1:
        return float("nan")
    return float(-60.0 / np.polyfit(np.arange(i0, i1) / float(fs), db[i0:i1], 1)[0])
