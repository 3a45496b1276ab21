"""The option classes' ``of()`` and the online classes' ``validate()``: every result, exception type and message, as plain text.
One body (misonet_amd/_online.py) stands behind all of them; this file pins what each caller sees.  CPU only: nothing here loads
the library."""
import dataclasses
import pathlib
import re

import pytest

from misonet_amd.beamform import Beamformer, BeamformStream, JointBeamformer, OnlineBeamformer
from misonet_amd.blind import AuxIVA, OnlineAuxIVA, SeparateStream
from misonet_amd.dereverb import Dereverb, DereverbStream, OnlineDereverb
from misonet_amd.localize import Localizer
from misonet_amd.refine import Refine

# class, the label of its unknown-field message, its TypeError text, the field a bare string sets (and a value for it), whether
# True means the defaults
SPECS = [
    (Beamformer, "beamformer", "beamformer must be None, a Beamformer, a kind name or a dict of its fields", ("kind", "gev"), False),
    (JointBeamformer, "joint beamformer",
     "joint beamformer must be None, a JointBeamformer, a kind name or a dict of its fields", ("kind", "r1mwf"), False),
    (OnlineBeamformer, "online beamformer",
     "an online beamformer must be None, True, an OnlineBeamformer, a noise name or a dict of its fields", ("noise", "mix"), True),
    (AuxIVA, "blind", "blind must be None, True, an AuxIVA, a model name or a dict of its fields", ("model", "laplace"), True),
    (OnlineAuxIVA, "online blind", "online must be None, True, an OnlineAuxIVA, a model name or a dict of its fields",
     ("model", "laplace"), True),
    (Dereverb, "dereverb", "dereverb must be None, True, a Dereverb or a dict of its fields", None, True),
    (OnlineDereverb, "online dereverb", "online dereverb must be None, True, an OnlineDereverb or a dict of its fields", None, True),
    (Refine, "refine", "refine must be None, True, a Refine, a prior name or a dict of its fields", ("prior", "guided"), True),
    (Localizer, "localizer", "localizer must be None, True, a Localizer, a kind name or a dict of its fields", ("kind", "music"),
     True),
]
IDS = [s[0].__name__ for s in SPECS]


def _raises(exc, text, call):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and str(e.value) == text


@pytest.mark.parametrize("cls, label, type_error, shorthand, true_ok", SPECS, ids=IDS)
def test_of(cls, label, type_error, shorthand, true_ok):
    assert cls.of(None) == cls()
    if true_ok:
        assert cls.of(True) == cls()
    else:
        _raises(TypeError, type_error, lambda: cls.of(True))
    first = dataclasses.fields(cls)[0].name
    inst = dataclasses.replace(cls(), ref_ch=1) if hasattr(cls, "ref_ch") else cls()
    assert cls.of(inst) is inst
    if shorthand is not None:
        assert cls.of(shorthand[1]) == cls(**{shorthand[0]: shorthand[1]})
    else:
        _raises(TypeError, type_error, lambda: cls.of("name"))
    assert cls.of({first: getattr(cls(), first)}) == cls()
    _raises(ValueError, f"unknown {label} field(s) ['no_such_field']", lambda: cls.of({first: getattr(cls(), first), "no_such_field": 1}))
    _raises(ValueError, f"unknown {label} field(s) ['a', 'b']", lambda: cls.of({"b": 1, "a": 2}))
    _raises(TypeError, type_error, lambda: cls.of(3.5))
    _raises(TypeError, type_error, lambda: cls.of(False))


INF, NAN = float("inf"), float("nan")
BAD = [
    (OnlineDereverb, dict(taps=2.5), "online dereverb taps must be an integer, got 2.5"),
    (OnlineDereverb, dict(taps=True), "online dereverb taps must be an integer, got True"),
    (OnlineDereverb, dict(taps=0), "online dereverb taps must be >= 1 with M * taps <= 80, got taps 0"),
    (OnlineDereverb, dict(delay="3"), "online dereverb delay must be an integer, got '3'"),
    (OnlineDereverb, dict(delay=0), "online dereverb delay must be >= 1, got 0"),
    (OnlineDereverb, dict(context=1.0), "online dereverb context must be an integer, got 1.0"),
    (OnlineDereverb, dict(context=17), "online dereverb context must be in [0, 16], got 17"),
    (OnlineDereverb, dict(alpha=0.0), "online dereverb alpha must be finite and > 0, got 0.0"),
    (OnlineDereverb, dict(alpha=1.5), "online dereverb alpha must be in (0, 1], got 1.5"),
    (OnlineDereverb, dict(power_floor=0), "online dereverb power_floor must be finite and > 0, got 0"),
    (OnlineDereverb, dict(power_floor=NAN), "online dereverb power_floor must be finite and > 0, got nan"),
    (OnlineDereverb, dict(init=INF), "online dereverb init must be finite and > 0, got inf"),
    (OnlineDereverb, dict(init=True), "online dereverb init must be finite and > 0, got True"),
    (OnlineAuxIVA, dict(model="cauchy"), "online blind model 'cauchy': one of ('gauss', 'laplace')"),
    (OnlineAuxIVA, dict(alpha=-0.5), "online blind alpha must be finite and > 0, got -0.5"),
    (OnlineAuxIVA, dict(alpha=1.0), "online blind alpha must be in (0, 1), got 1.0"),
    (OnlineAuxIVA, dict(floor=0.0), "online blind floor must be finite and > 0, got 0.0"),
    (OnlineAuxIVA, dict(floor="1e-10"), "online blind floor must be finite and > 0, got '1e-10'"),
    (OnlineAuxIVA, dict(init=INF), "online blind init must be finite and > 0, got inf"),
    (OnlineAuxIVA, dict(ref_ch=-1), "online blind ref_ch must be a non-negative integer, got -1"),
    (OnlineAuxIVA, dict(ref_ch=1.0), "online blind ref_ch must be a non-negative integer, got 1.0"),
    (OnlineAuxIVA, dict(ref_ch=True), "online blind ref_ch must be a non-negative integer, got True"),
    (OnlineBeamformer, dict(noise="both"), "online beamformer noise 'both': one of ('residual', 'mix') (or 0, 1)"),
    (OnlineBeamformer, dict(noise=2), "online beamformer noise 2: one of ('residual', 'mix') (or 0, 1)"),
    (OnlineBeamformer, dict(alpha=1.0), "online beamformer alpha must be in (0, 1), got 1.0"),
    (OnlineBeamformer, dict(alpha=True), "online beamformer alpha must be in (0, 1), got True"),
    (OnlineBeamformer, dict(alpha=NAN), "online beamformer alpha must be in (0, 1), got nan"),
    (OnlineBeamformer, dict(mu=-1.0), "online beamformer mu must be finite and >= 0, got -1.0"),
    (OnlineBeamformer, dict(diag_load=NAN), "online beamformer diag_load must be finite and >= 0, got nan"),
    (OnlineBeamformer, dict(epsi=True), "online beamformer epsi must be finite and >= 0, got True"),
    (OnlineBeamformer, dict(init=INF), "online beamformer init must be finite and >= 0, got inf"),
    (OnlineBeamformer, dict(init="1"), "online beamformer init must be finite and >= 0, got '1'"),
    (OnlineBeamformer, dict(ref_ch=-1), "online beamformer ref_ch must be a non-negative integer, got -1"),
    (OnlineBeamformer, dict(ref_ch=0.0), "online beamformer ref_ch must be a non-negative integer, got 0.0"),
]


@pytest.mark.parametrize("cls, fields, text", BAD, ids=[f"{c.__name__}-{'-'.join(f)}-{i}" for i, (c, f, _) in enumerate(BAD)])
def test_validate_message(cls, fields, text):
    _raises(ValueError, text, lambda: cls(**fields).validate())


def test_validate_geometry_messages():
    _raises(ValueError, "online dereverb takes 1 .. 8 microphones, got 9", lambda: OnlineDereverb().validate(9))
    _raises(ValueError, "online dereverb taps must be >= 1 with M * taps <= 80, got taps 11 at M = 8",
            lambda: OnlineDereverb(taps=11).validate(8))
    _raises(ValueError, "online blind separation needs 2 <= M <= 8 microphones, got 1", lambda: OnlineAuxIVA().validate(1))
    _raises(ValueError, "online blind ref_ch 2 outside [0, 2)", lambda: OnlineAuxIVA(ref_ch=2).validate(2))
    _raises(ValueError, "the online beamformer needs 2 <= M <= 8 microphones, got 9", lambda: OnlineBeamformer().validate(9))
    _raises(ValueError, "online beamformer ref_ch 3 outside [0, 3)", lambda: OnlineBeamformer(ref_ch=3).validate(3))
    _raises(ValueError, "the online beamformer takes 1 <= S <= 8 sources, got 9", lambda: OnlineBeamformer().validate(2, 9))
    for cls in (OnlineDereverb, OnlineAuxIVA, OnlineBeamformer):
        o = cls()
        assert o.validate() is o and o.validate(2) is o


def test_one_stream_base():
    from misonet_amd._online import OnlineStream
    for cls in (DereverbStream, SeparateStream, BeamformStream):
        assert issubclass(cls, OnlineStream) and cls is not OnlineStream


def test_one_callable_module():
    pkg = pathlib.Path(__file__).resolve().parent.parent / "misonet_amd"
    defs = sorted(p.name for p in pkg.glob("*.py") if re.search(r"^class _CallableModule\b", p.read_text(), re.M))
    assert defs == ["_online.py"]
