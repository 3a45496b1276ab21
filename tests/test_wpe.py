"""CPU checks of the WPE dereverberation: the NumPy restatement (tests/wpe_ref.py) has the properties the device tests lean on,
and the host side of the C ABI (version, prototypes, defaults, validation) and of the Python options behaves.  No kernel is
launched here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import wpe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_stacking_order():
    Y = (np.arange(12).reshape(3, 4) + 1).astype(np.complex128)
    Z = wpe_ref.stack(Y, taps=2, delay=1)
    assert Z.shape == (6, 4)
    assert np.array_equal(Z[0], [0, 1, 2, 3]) and np.array_equal(Z[2], [0, 9, 10, 11])      # k = 0: delayed by 1
    assert np.array_equal(Z[3], [0, 0, 1, 2]) and np.array_equal(Z[5], [0, 0, 9, 10])       # k = 1: delayed by 2
    assert not wpe_ref.stack(Y, taps=2, delay=7).any()                                       # all before the first frame


def test_restatement_reduces_energy_and_is_insensitive():
    """three iterations remove energy; LU against Cholesky and another summation order move the float64 result far less than
    one complex64 rounding does"""
    mix = wpe_ref.reverb_inputs(1, 4, 120, 5)
    X, G, bad = wpe_ref.wpe(mix, None, 4, 2, 3)
    assert not bad.any() and G.shape == (1, 5, 16, 4)
    ratio = np.linalg.norm(X) ** 2 / np.linalg.norm(mix) ** 2
    assert 0.1 < ratio < 1.0, ratio
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert rel(wpe_ref.wpe(mix, None, 4, 2, 3, solver="chol")[0], X) < 1e-10
    assert rel(wpe_ref.wpe(mix, None, 4, 2, 3, block=16)[0], X) < 1e-10
    assert 1e-8 < rel(X.astype(np.complex64), X) < 2.0 ** -24
    # the filter is the minimiser of the weighted prediction error of its own iteration: one iteration, checked directly
    Y = mix[0, :, :, 2].astype(np.complex128)
    x1, g1, _ = wpe_ref.wpe_bin(Y, None, 4, 2, 1)
    Z = wpe_ref.stack(Y, 4, 2)
    p = np.mean(np.abs(Y) ** 2, axis=0)
    w = 1.0 / np.maximum(p, 1e-10 * p.max())
    assert np.abs((Z * w) @ x1.conj().T).max() < 1e-9 * np.abs((Z * w) @ Y.conj().T).max()  # the normal equations
    assert np.allclose(x1, Y - g1.conj().T @ Z)


def test_power_argument_is_the_first_iteration():
    mix = wpe_ref.reverb_inputs(2, 3, 50, 4)
    own = np.mean(np.abs(mix.astype(np.complex128)) ** 2, axis=1)                            # [B, T, F]
    a = wpe_ref.wpe(mix, own, 3, 2, 1)
    b = wpe_ref.wpe(mix, None, 3, 2, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = wpe_ref.wpe(mix, 2.0 * own + 1e-3, 3, 2, 1)
    assert not np.allclose(c[0], b[0])


def test_zero_bin_comes_back_unchanged_and_flagged():
    mix = wpe_ref.reverb_inputs(1, 3, 40, 4).copy()
    mix[0, :, :, 1] = 0
    X, G, bad = wpe_ref.wpe(mix, None, 3, 1, 3)
    assert bad.tolist() == [[0, 1, 0, 0]]
    assert np.array_equal(X[0, :, :, 1], mix[0, :, :, 1]) and not G[0, 1].any()
    assert np.isfinite(X).all() and np.linalg.norm(X[0, :, :, 0] - mix[0, :, :, 0]) > 0


def test_generator_is_fixed():
    a, b = wpe_ref.reverb_inputs(1, 2, 20, 3), wpe_ref.reverb_inputs(1, 2, 20, 3)
    assert a.dtype == np.complex64 and a.shape == (1, 2, 20, 3) and np.array_equal(a, b)
    assert not np.array_equal(a, wpe_ref.reverb_inputs(1, 2, 20, 3, seed=1))


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_wpe_opts_default", "misonet_wpe_workspace_bytes", "misonet_wpe", "misonet_wpe_debug"}


def test_abi_520():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 520
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    assert "misonet_wpe_opts;" in hdr
    for name in NEW:
        assert hasattr(lib, name), name
    o = L.WpeOpts(0, 0, 0, 1.0, 1.0)
    assert lib.misonet_wpe_opts_default(C.byref(o)) == L.OK
    assert (o.taps, o.delay, o.iterations, o.diag_load, o.power_floor) == (10, 3, 3, 0.0, 1e-10)
    assert lib.misonet_wpe_opts_default(None) == L.EINVAL


def _opts(**kw):
    L = _lib()
    o = L.WpeOpts()
    L.lib().misonet_wpe_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD_OPTS = [dict(taps=0), dict(taps=14), dict(delay=0), dict(delay=-1), dict(iterations=0), dict(iterations=11),
            dict(diag_load=-1e-9), dict(diag_load=math.nan), dict(diag_load=math.inf), dict(power_floor=-1.0),
            dict(power_floor=math.nan), dict(power_floor=math.inf)]


def test_workspace_size_and_invalid_fields():
    L = _lib()
    lib = L.lib()
    size = lambda B, M, T, F, o: lib.misonet_wpe_workspace_bytes(B, M, T, F, C.byref(o) if o is not None else None)
    n = size(16, 6, 1001, 129, _opts())
    assert n >= 16 * 129 * 6 * 1001 * 8 and n < 2 * 16 * 129 * 6 * 1001 * 8          # one transposed copy and small change
    assert size(1, 6, 15001, 129, _opts()) > 0                                          # a whole 60 s recording is one call
    assert size(1, 8, 200, 3, _opts()) > 0 and size(1, 1, 2, 1, _opts(taps=80)) > 0     # order 80 both ways
    for kw in BAD_OPTS:
        assert size(2, 6, 100, 129, _opts(**kw)) == -1, kw
        assert lib.misonet_last_error(), kw
    assert size(2, 6, 100, 129, None) == -1
    for B, M, T, F in [(0, 6, 100, 129), (2, 0, 100, 129), (2, 9, 100, 129), (2, 6, 1, 129), (2, 6, 100, 0)]:
        assert size(B, M, T, F, _opts()) == -1, (B, M, T, F)
    assert size(1, 8, 100, 129, _opts(taps=11)) == -1 and size(1, 8, 100, 129, _opts(taps=10)) > 0
    # the call itself refuses before any launch: null pointers (no device is touched here)
    o = _opts()
    assert lib.misonet_wpe(None, None, 1, 6, 100, 129, C.byref(o), None, None, 0, None) == L.EINVAL
    assert lib.misonet_wpe_debug(None, 1, 6, 129, C.byref(o), None, None, None) == L.EINVAL


# ---- the Python options -------------------------------------------------------------------------------------------------
def test_dereverb_options():
    import misonet_amd as mz
    from misonet_amd.dereverb import Dereverb
    assert mz.Dereverb is Dereverb and callable(mz.dereverb) and callable(mz.dereverb_wav)
    d = Dereverb()
    assert (d.taps, d.delay, d.iterations, d.diag_load, d.power_floor) == (10, 3, 3, 0.0, 1e-10)
    assert Dereverb.of(None) == d and Dereverb.of(True) == d and Dereverb.of(d) is d
    assert Dereverb.of(dict(taps=5, delay=2)) == Dereverb(taps=5, delay=2)
    with pytest.raises(ValueError):
        Dereverb.of(dict(tap=5))
    with pytest.raises(TypeError):
        Dereverb.of("wpe")
    with pytest.raises(dataclasses_error()):
        d.taps = 3
    assert d.validate(6) is d and d.validate(8) is d
    for kw in BAD_OPTS:
        with pytest.raises(ValueError):
            Dereverb(**kw).validate(6)
    for m in (0, 9):
        with pytest.raises(ValueError):
            d.validate(m)
    with pytest.raises(ValueError):
        Dereverb(taps=11).validate(8)
    with pytest.raises(ValueError):
        Dereverb(taps=2.5).validate(2)
    o = Dereverb(taps=4, delay=2, iterations=1, diag_load=1e-6, power_floor=1e-8).c_opts()
    assert (o.taps, o.delay, o.iterations, o.diag_load, o.power_floor) == (4, 2, 1, 1e-6, 1e-8)


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_dereverb_refuses_before_any_launch():
    """bad shapes and fields raise ValueError on the host: no device is needed to see them"""
    from misonet_amd.dereverb import dereverb, dereverb_wav
    mix = wpe_ref.reverb_inputs(1, 2, 20, 3)
    with pytest.raises(ValueError):
        dereverb(mix, taps=41)
    with pytest.raises(ValueError):
        dereverb(mix, delay=0)
    with pytest.raises(ValueError):
        dereverb(mix[0])
    with pytest.raises(ValueError):
        dereverb(mix[:, :, :1])
    with pytest.raises(ValueError):
        dereverb_wav(np.zeros((1000, 9), np.float32))
    with pytest.raises(ValueError):
        dereverb_wav(np.zeros((4, 1000), np.float32))
