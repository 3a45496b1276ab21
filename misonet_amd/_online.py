"""What the option classes and the frame-recursive streams share.

``spec_of``, ``check_real``, ``check_index``  -- the one body behind every ``of()`` classmethod, and the two pasted field checks
``OnlineStream``                             -- the state block of :class:`misonet_amd.dereverb.DereverbStream`,
                                                :class:`misonet_amd.blind.SeparateStream` and
                                                :class:`misonet_amd.beamform.BeamformStream`: allocation, reset, the debug copies
``default_device``, ``_dev_c64``              -- where a call runs, and its input as complex64 on that device
``_CallableModule``                          -- a module that is also the function of its own name

Importing this module does not import torch: :mod:`misonet_amd.localize` imports it.
"""
from __future__ import annotations

import math
import sys
import types

import numpy as np

from . import _lib


def spec_of(cls, spec, label, type_error, shorthand=None, true_ok=True):
    """``cls.of(spec)``: None (and True, with ``true_ok``) are the defaults, an instance is itself, a string sets the field
    ``shorthand`` where the class has one, a dict holds fields.  ``label`` names the class in the unknown-field message;
    ``type_error`` is the message for anything else."""
    if spec is None or (true_ok and spec is True):
        return cls()
    if isinstance(spec, cls):
        return spec
    if shorthand is not None and isinstance(spec, str):
        return cls(**{shorthand: spec})
    if isinstance(spec, dict):
        unknown = set(spec) - set(cls.__dataclass_fields__)                   # the fields and the init-only arguments
        if unknown:
            raise ValueError(f"unknown {label} field(s) {sorted(unknown)}")
        return cls(**spec)
    raise TypeError(type_error)


def check_real(label, name, v, *, positive):
    """ValueError unless v is a finite real number (no bool), > 0 with ``positive`` and >= 0 without"""
    if (isinstance(v, bool) or not isinstance(v, (int, float, np.floating)) or not math.isfinite(v)
            or (not v > 0 if positive else v < 0)):
        raise ValueError(f"{label} {name} must be finite and {'> 0' if positive else '>= 0'}, got {v!r}")


def check_index(label, name, v):
    """ValueError unless v is an integer (no bool) >= 0"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError(f"{label} {name} must be a non-negative integer, got {v!r}")


def default_device(x, device):
    """``device`` where it is given; else the device of ``x`` where that is a tensor on a GPU; else the current GPU"""
    import torch
    if device is not None:
        return torch.device(device)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _dev_c64(x, device):
    import torch
    was_numpy = not isinstance(x, torch.Tensor)
    t = torch.as_tensor(x)
    if not t.is_complex():
        raise TypeError("expected a complex array")
    if t.device.type != "cuda":
        t = t.to(device)
    return t.to(torch.complex64).contiguous(), was_numpy


class OnlineStream:
    """The state block of one frame-recursive stream, on the device.  A subclass sets ``batch``, ``num_mic``, ``num_bins`` and its
    options, calls :meth:`_alloc` with the size the library names, and supplies

    ``_reset_call()``     the library's reset on ``self.state``; returns its code
    ``_parts()``          name -> (shape, dtype) of every part of the state that the library's debug call copies out
    ``_debug_call(ptr)``  that debug call; ``ptr(name)`` is the address to copy the part to, or None; returns its code
    """

    def _alloc(self, nbytes, device):
        import torch
        if nbytes < 0:
            _lib.check(_lib.EINVAL)
        self.device = default_device(None, device)
        self.state = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self):
        """the state as it is before the first frame: nothing seen, no flag"""
        import torch
        with torch.cuda.device(self.device):
            _lib.check(self._reset_call())
        return self

    def _same_geometry(self, shape):
        if (shape[0], shape[1], shape[3]) != (self.batch, self.num_mic, self.num_bins):
            raise ValueError(f"block {tuple(shape)} must be [{self.batch}, {self.num_mic}, T, {self.num_bins}]")

    def _check_block(self, shape):
        """a block [B, M, T, F] of this stream's geometry with T >= 1"""
        if len(shape) != 4 or shape[2] < 1:
            raise ValueError(f"block {tuple(shape)} must be [B, M, T, F] with T >= 1")
        self._same_geometry(shape)

    def _debug(self, want=None):
        """copies of the named parts of the state (None: all of them), on the device"""
        import torch
        parts = self._parts()
        d = {k: torch.empty(parts[k][0], dtype=parts[k][1], device=self.device) for k in (parts if want is None else want)}
        with torch.cuda.device(self.device):
            _lib.check(self._debug_call(lambda k: d[k].data_ptr() if k in d else None))
        return d

    @property
    def frames_seen(self) -> int:
        return int(self._debug(("n",))["n"].max().item())

    @property
    def fail(self):
        """int32 on the device: the fail word of every bin"""
        return self._debug(("fail",))["fail"]


class _CallableModule(types.ModuleType):
    """``misonet_amd.dereverb``, ``.localize`` and ``.resample`` each name a module and the function in it: once the module is
    imported the package attribute is the module, so the module itself is made callable -- ``misonet_amd.dereverb(mix)`` works
    either way."""

    def __call__(self, *args, **kwargs):
        return getattr(self, self.__name__.rpartition(".")[2])(*args, **kwargs)


def make_callable(module_name):
    """the module of that name calls its function of the same name from now on"""
    sys.modules[module_name].__class__ = _CallableModule
