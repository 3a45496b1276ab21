"""CPU checks of the online WPE: the NumPy restatement (tests/owpe_ref.py) has the properties the device tests lean on -- it is
the regularised weighted least-squares filter at alpha = 1, it dereverberates the fixed room, it does not depend on how the
stream is cut, and every planted mistake misses the device tests' bars -- and the host side of the C ABI (version, prototypes,
defaults, validation) and of the Python options behaves.  No kernel is launched here.

The fixed room (``owpe_ref.fixed_room``, seeds 1-3, T 1600, F 8, taps 8, delay 3, alpha 0.999; late over early energy in the
frames [T/4, T/2) and [3T/4, T), the late part of an output being what is left of it without the early part and the noise of the
input).  Measured with this file, float64:
    input 0.139 / 0.111 / 0.143; offline ``wpe_ref.wpe`` 0.0088 / 0.0097 / 0.0094;
    the recursion at context 1: 0.0123 .. 0.0138 (alpha 0.995: 0.0249 .. 0.0284; 0.99: 0.0543 .. 0.0587);
    the recursion at context 0: 0.0152 / 0.0143 / 0.0195, i.e. 1.72 / 1.48 / 2.08 x offline.
The table of the feature's issue (0.012 - 0.014, 0.025 - 0.028, 0.054 - 0.058) is the context-1 row to its printed digits, so the
condition "<= 1.5 x offline and <= 0.2 x the input" is asserted at context 1; the context-0 figures are printed beside it and
asserted against the input only."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

import owpe_ref as R
import wpe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = lambda delay: [1, 1, delay, 61]


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_alpha_one_is_regularised_weighted_least_squares():
    """with alpha = 1 the recursion is exact RLS: after T frames G = (I / init + sum z z^H / lambda)^-1 sum z y^H / lambda,
    and P is that inverse"""
    B, M, T, F, taps, delay = 1, 3, 50, 2, 4, 2
    mix = wpe_ref.reverb_inputs(B, M, T, F, seed=3)
    out, st = R.owpe(mix, taps, delay, 0, 1.0, init=2.0)
    for f in range(F):
        Y = mix[0, :, :, f].astype(np.complex128)
        Z = wpe_ref.stack(Y, taps, delay)
        lam = np.maximum(np.mean(np.abs(Y) ** 2, axis=0), 1e-10)
        Rm = np.eye(M * taps) / 2.0 + (Z / lam) @ Z.conj().T
        G = np.linalg.solve(Rm, (Z / lam) @ Y.conj().T)
        assert R.rel(st.G[0, f], G) < 1e-9 and R.rel(st.P[0, f], np.linalg.inv(Rm)) < 1e-9
    assert np.array_equal(st.P, np.conj(np.swapaxes(st.P, -1, -2)))
    assert st.n.tolist() == [[T] * F] and not st.fail.any()
    assert out.dtype == np.complex64 and np.array_equal(out[:, :, :delay], mix[:, :, :delay])     # nothing to predict from yet


def test_state_stays_finite_and_hermitian():
    mix = wpe_ref.reverb_inputs(1, 6, 400, 2, seed=3)
    for taps, alpha in [(10, 0.999), (5, 0.99), (13, 0.995)]:
        out, st = R.owpe(mix, taps, 3, 0, alpha)
        assert np.isfinite(out).all() and np.isfinite(st.P).all() and not st.fail.any()
        assert np.array_equal(st.P, np.conj(np.swapaxes(st.P, -1, -2)))


def _late(out, mix, early, late):
    noise = mix.astype(np.complex128) - early - late
    return R.late_over_early(early, out.astype(np.complex128) - early - noise)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fixed_room(seed):
    mix, early, late = R.fixed_room(seed)
    fig_in = R.late_over_early(early, late)
    off = _late(wpe_ref.wpe(mix, None, 8, 3)[0], mix, early, late)
    on1 = _late(R.owpe(mix, 8, 3, 1, 0.999)[0], mix, early, late)
    on0 = _late(R.owpe(mix, 8, 3, 0, 0.999)[0], mix, early, late)
    print(f"[owpe] fixed room seed {seed}: input {fig_in:.4f}  offline {off:.4f}  recursion context 1 {on1:.4f} "
          f"({on1 / off:.2f} x offline)  context 0 {on0:.4f} ({on0 / off:.2f} x offline)")
    assert 0.1 < fig_in < 0.15 and off < fig_in
    assert on1 <= 1.5 * off and on1 <= 0.2 * fig_in, (on1, off, fig_in)
    assert on0 <= 0.2 * fig_in, (on0, fig_in)
    assert on1 > off                                     # causal and forgetting: not a better filter than the offline one


def _same_state(a, b):
    return all(np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8))
               for k in ("P", "G", "ring", "pw", "n", "fail"))


def test_restatement_is_chunk_invariant():
    B, M, T, F, taps, delay = 2, 2, 80, 3, 3, 2
    mix = wpe_ref.reverb_inputs(B, M, T, F, seed=3)
    whole, st = R.owpe(mix, taps, delay, 5, 0.98)
    cut, sc = R.owpe(mix, taps, delay, 5, 0.98, cuts=CUTS(delay))
    assert R.pieces(T, CUTS(delay)) == [(0, 1), (1, 2), (2, 4), (4, 65), (65, 80)]
    assert np.array_equal(whole.view(np.uint64), cut.view(np.uint64)) and _same_state(st, sc)
    one, s1 = R.owpe(mix[:, :, :12], taps, delay, 5, 0.98, cuts=[1] * 12)
    w12, s12 = R.owpe(mix[:, :, :12], taps, delay, 5, 0.98)
    assert np.array_equal(one.view(np.uint64), w12.view(np.uint64)) and _same_state(s1, s12)
    assert R.pieces(3, [1, 1, 3, 61]) == [(0, 1), (1, 2), (2, 3)]       # a stream shorter than the cuts


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_miss_the_device_bars(fault):
    """each mistake a kernel could make, planted in the restatement, is rejected by what tests/test_gpu_owpe.py asserts
    (``owpe_ref.rejected``); the restatement itself, and its other summation order, are not"""
    B, M, T, F, taps, delay = 2, 2, 40, 5, 3, 1
    mix = wpe_ref.reverb_inputs(B, M, T, F, seed=3)
    kw = dict(taps=taps, delay=delay, context=5, alpha=0.999)
    out, st, bar, own = R.figures(mix, **kw)
    assert own < 1e-13 and bar == R.STATE_FLOOR
    assert not R.rejected(out, st, out, st, bar)
    ro, rs = R.owpe(mix, reverse=True, **kw)
    assert not R.rejected(ro, rs, out, st, bar)
    fo, fs = R.owpe(mix, fault=fault, **kw)
    print(f"[owpe] fault {fault}: out {R.rel(fo, out):.3e}  G {R.rel(fs.G, st.G):.3e}  P {R.rel(fs.P, st.P):.3e}  (bars "
          f"{R.OUT_BAR:g}, {bar:g})  Hermitian {np.array_equal(fs.P, np.conj(np.swapaxes(fs.P, -1, -2)))}")
    assert R.rejected(fo, fs, out, st, bar), fault


def test_failing_frames_and_silence():
    B, M, T, F, taps, delay = 1, 2, 30, 3, 3, 1
    mix = wpe_ref.reverb_inputs(B, M, T, F, seed=3).copy()
    clean, sc = R.owpe(mix, taps, delay, 2, 0.99)
    mix[0, 1, 10, 1] = np.nan
    mix[0, 0, 10, 1] = complex(0.0, np.inf)
    out, st = R.owpe(mix, taps, delay, 2, 0.99)
    assert st.fail.tolist() == [[0, 1, 0]] and st.n.tolist() == [[T] * F]
    assert np.array_equal(out[0, :, 10, 1].view(np.uint64), mix[0, :, 10, 1].view(np.uint64))
    keep = [0, 2]
    assert np.array_equal(out[..., keep].view(np.uint64), clean[..., keep].view(np.uint64))
    assert np.isfinite(out[0, :, 11:, 1]).all() and np.isfinite(st.P).all()
    mix = wpe_ref.reverb_inputs(B, M, T, F, seed=3).copy()
    mix[..., 2] = 0
    out, st = R.owpe(mix, taps, delay, 2, 0.99)
    assert not st.fail.any() and np.isfinite(out).all() and not out[..., 2].any()


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_owpe_opts_default", "misonet_owpe_state_bytes", "misonet_owpe_lds_bytes", "misonet_owpe_reset", "misonet_owpe",
       "misonet_owpe_debug"}


def test_abi_620():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 620
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    assert "misonet_owpe_opts;" in hdr
    for name in NEW:
        assert hasattr(lib, name), name
    o = L.OwpeOpts(0, 0, 9, 0.0, 0.0, 0.0)
    assert lib.misonet_owpe_opts_default(C.byref(o)) == L.OK
    assert (o.taps, o.delay, o.context, o.alpha, o.power_floor, o.init) == (10, 3, 0, 0.999, 1e-10, 1.0)
    assert lib.misonet_owpe_opts_default(None) == L.EINVAL


def _opts(**kw):
    L = _lib()
    o = L.OwpeOpts()
    L.lib().misonet_owpe_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD_OPTS = [dict(taps=0), dict(taps=14), dict(delay=0), dict(delay=-1), dict(context=-1), dict(context=17), dict(alpha=0.0),
            dict(alpha=-0.5), dict(alpha=1.0000001), dict(alpha=math.nan), dict(alpha=math.inf), dict(power_floor=0.0),
            dict(power_floor=-1.0), dict(power_floor=math.nan), dict(power_floor=math.inf), dict(init=0.0), dict(init=-1.0),
            dict(init=math.nan), dict(init=math.inf)]


def test_state_size_and_invalid_fields():
    L = _lib()
    lib = L.lib()
    size = lambda B, M, F, o: lib.misonet_owpe_state_bytes(B, M, F, C.byref(o) if o is not None else None)
    n = size(16, 6, 129, _opts())
    per_bin = 60 * 60 * 16 + 60 * 6 * 16 + 12 * 6 * 8 + 16 * 8 + 12
    assert 16 * 129 * per_bin <= n <= 16 * 129 * per_bin + 7 * 16                       # nothing in it grows with T
    assert size(1, 8, 3, _opts()) > 0 and size(1, 1, 1, _opts(taps=80)) > 0 and size(1, 1, 1, _opts(taps=1, delay=1)) > 0
    assert size(1, 6, 129, _opts(alpha=1.0, context=16)) > 0
    for kw in BAD_OPTS:
        assert size(2, 6, 129, _opts(**kw)) == -1, kw
        assert lib.misonet_last_error(), kw
        assert lib.misonet_owpe_lds_bytes(6, C.byref(_opts(**kw))) == -1, kw
    assert size(2, 6, 129, None) == -1 and lib.misonet_owpe_lds_bytes(6, None) == -1
    for B, M, F in [(0, 6, 129), (2, 0, 129), (2, 9, 129), (2, 6, 0), (1 << 16, 6, 1 << 15)]:
        assert size(B, M, F, _opts()) == -1, (B, M, F)
    assert size(1, 8, 129, _opts(taps=11)) == -1 and size(1, 8, 129, _opts(taps=10)) > 0
    # the frame ring must fit the LDS beside P: a delay of thousands of frames is refused, one of hundreds is not
    assert size(1, 8, 129, _opts(delay=5000)) == -1 and size(1, 8, 129, _opts(delay=300)) > 0
    # the calls themselves refuse before any launch: null pointers (no device is touched here)
    o = _opts()
    assert lib.misonet_owpe(None, 1, 6, 100, 129, C.byref(o), None, None, 0, None) == L.EINVAL
    assert lib.misonet_owpe_reset(None, 1, 6, 129, C.byref(o), None) == L.EINVAL
    assert lib.misonet_owpe_debug(None, 1, 6, 129, C.byref(o), None, None, None, None, None) == L.EINVAL


# ---- the Python options -------------------------------------------------------------------------------------------------
def test_online_dereverb_options():
    import misonet_amd as mz
    from misonet_amd.dereverb import Dereverb, OnlineDereverb
    assert mz.OnlineDereverb is OnlineDereverb and callable(mz.dereverb_online) and isinstance(mz.DereverbStream, type)
    d = OnlineDereverb()
    assert dataclasses.astuple(d) == (10, 3, 0, 0.999, 1e-10, 1.0)
    assert OnlineDereverb.of(None) == d and OnlineDereverb.of(True) == d and OnlineDereverb.of(d) is d
    assert OnlineDereverb.of(dict(taps=5, alpha=0.99)) == OnlineDereverb(taps=5, alpha=0.99)
    with pytest.raises(ValueError):
        OnlineDereverb.of(dict(iterations=3))
    with pytest.raises(TypeError):
        OnlineDereverb.of("rls")
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.taps = 3
    assert d.validate(6) is d and d.validate(8) is d and OnlineDereverb(alpha=1.0, context=16).validate(6)
    for kw in BAD_OPTS:
        with pytest.raises(ValueError):
            OnlineDereverb(**kw).validate(6)
    for m in (0, 9):
        with pytest.raises(ValueError):
            d.validate(m)
    with pytest.raises(ValueError):
        OnlineDereverb(taps=11).validate(8)
    with pytest.raises(ValueError):
        OnlineDereverb(context=2.0).validate(2)
    o = OnlineDereverb(taps=4, delay=2, context=3, alpha=0.98, power_floor=1e-8, init=5.0).c_opts()
    assert (o.taps, o.delay, o.context, o.alpha, o.power_floor, o.init) == (4, 2, 3, 0.98, 1e-8, 5.0)
    # what Dereverb.of accepts and raises is what it was: an OnlineDereverb is not one of its specs
    with pytest.raises(TypeError):
        Dereverb.of(d)
    assert Dereverb.of(True) == Dereverb()


def test_online_calls_refuse_before_any_launch():
    """bad shapes and fields raise ValueError on the host: no device is needed to see them"""
    from misonet_amd.dereverb import DereverbStream, dereverb_online, dereverb_wav
    mix = wpe_ref.reverb_inputs(1, 2, 20, 3)
    with pytest.raises(ValueError):
        dereverb_online(mix, taps=41)
    with pytest.raises(ValueError):
        dereverb_online(mix, alpha=0.0)
    with pytest.raises(ValueError):
        dereverb_online(mix[0])
    with pytest.raises(ValueError):
        dereverb_online(mix[:, :, :0])
    with pytest.raises(ValueError):
        DereverbStream(9)
    with pytest.raises(ValueError):
        DereverbStream(2, num_bins=0)
    with pytest.raises((TypeError, ValueError)):
        DereverbStream(2, iterations=3)
    with pytest.raises(ValueError):
        dereverb_wav(np.zeros((1000, 9), np.float32), online=True)
    with pytest.raises(ValueError):
        dereverb_wav(np.zeros((1000, 3), np.float32), online=True, taps=4)         # the options go into online=
    with pytest.raises(ValueError):
        dereverb_wav(np.zeros((1000, 3), np.float32), online=dict(tap=4))
