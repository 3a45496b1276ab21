"""CPU checks of the online AuxIVA: the NumPy restatement (tests/oiva_ref.py) has the properties the device tests lean on -- it
separates, it does not depend on how the stream is cut, every device case's bar stays under the cap, and every planted mistake
misses the device tests' bars on at least one device case -- and the host side of the C ABI (version, prototypes, defaults,
validation) and of the Python options behaves.  No kernel is launched here.

Quality, measured with this file, float64: ``sparse_mixture(1, 2, 2, 400, 16, seed=1)`` at alpha 0.96, init 1.0, the images at
microphone 0 over the frames 200 .. 399 against the true images: 32.7 / 28.4 dB; the mixture itself 4.0 / -4.0 dB (0.0 dB in
the mean)."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

import iva_ref
import oiva_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = [1, 1, 2, 17]
# the device cases that do not depend on misonet_oiva_bins_per_pass, (B, M, T, F): tests/test_gpu_oiva.py runs these and F around P
CASES = [(2, 2, 40, 5), (1, 2, 1, 1), (1, 3, 30, 3), (1, 4, 40, 2), (1, 5, 30, 2), (1, 6, 40, 3), (1, 7, 30, 2), (1, 8, 30, 2),
         (1, 2, 300, 5)]
VARIANTS = [("gauss", 0.98, 0), ("laplace", 0.96, 1), ("gauss", 0.96, 0), ("laplace", 0.98, 1)]


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _inputs(B, M, T, F):
    """as tests/test_gpu_oiva.py: M sources at M microphones"""
    return R.to_stream(iva_ref.sparse_mixture(B, M, M, T, F, seed=B + M + T + F)[0])


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_quality():
    mix, img = iva_ref.sparse_mixture(1, 2, 2, 400, 16, seed=1)
    x = R.to_stream(mix)
    est, images, st = R.oiva(x, alpha=0.96)
    truth = np.transpose(img[0, :, :, 0, :], (0, 2, 1))[:, 200:]                    # [N, T, F] at microphone 0
    got = R.best_image_sdr(images[0, :, 0, 200:], truth)
    base = R.best_image_sdr(np.stack([x[0, 0, 200:]] * 2), truth)
    print(f"[oiva] quality: images {got[0]:.1f} / {got[1]:.1f} dB, mixture {base[0]:.1f} / {base[1]:.1f} dB")
    assert min(got) >= 20.0 and np.mean(base) < 1.0 and not st.fail.any()
    assert np.array_equal(est, images[:, :, 0])                                    # est is the image at ref_ch
    assert R.unit_norm_error(st.W, st.V) <= 1e-9 and R.image_sum_error(images, x, st.fail) <= 1e-5 and R.hermitian(st.V)


def _same_state(a, b):
    return all(np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)) for k in ("W", "V", "n", "fail"))


def test_restatement_is_cut_invariant():
    mix = _inputs(2, 3, 40, 4)
    e0, i0, s0 = R.oiva(mix, alpha=0.96, model="laplace")
    e1, i1, s1 = R.oiva(mix, alpha=0.96, model="laplace", cuts=CUTS)
    assert R.pieces(40, CUTS) == [(0, 1), (1, 2), (2, 4), (4, 21), (21, 40)]
    assert np.array_equal(e0.view(np.uint64), e1.view(np.uint64)) and np.array_equal(i0.view(np.uint64), i1.view(np.uint64))
    assert _same_state(s0, s1)
    e2, i2, s2 = R.oiva(mix[:, :, :12], cuts=[1] * 12)
    e3, i3, s3 = R.oiva(mix[:, :, :12])
    assert np.array_equal(e2.view(np.uint64), e3.view(np.uint64)) and _same_state(s2, s3)
    assert R.pieces(3, CUTS) == [(0, 1), (1, 2), (2, 3)]                             # a stream shorter than the cuts


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_every_device_case_stays_under_the_cap(shape):
    for model, alpha, ref_ch in VARIANTS:
        ref = R.figures(_inputs(*shape), model=model, alpha=alpha, ref_ch=ref_ch)
        print(f"[oiva] case {shape} {model} alpha {alpha:g}: own {ref['own']:.3e}  bar {ref['bar']:.3e}")
        assert ref["bar"] <= R.BAR_CAP and not ref["st"].fail.any()
        assert not R.rejected(R.as_candidate(ref["est"], ref["images"], ref["st"]), ref)
        rev = R.oiva(_inputs(*shape), model=model, alpha=alpha, ref_ch=ref_ch, reverse=True)
        assert not R.rejected(R.as_candidate(*rev), ref)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_miss_the_device_bars(fault):
    """each mistake a kernel could make, planted in the restatement, is rejected by what tests/test_gpu_oiva.py asserts
    (``oiva_ref.rejected``) on a device case: (2, 2, 40, 5) at ref_ch 0 and (1, 3, 30, 3) at ref_ch 1"""
    hits = []
    for shape, ref_ch in (((2, 2, 40, 5), 0), ((1, 3, 30, 3), 1)):
        kw = dict(model="gauss", alpha=0.98, ref_ch=ref_ch)
        ref = R.figures(_inputs(*shape), **kw)
        fe, fi, fs = R.oiva(_inputs(*shape), fault=fault, **kw)
        print(f"[oiva] fault {fault} on {shape}: est {R.rel(fe, ref['est']):.3e}  W {R.rel(fs.W, ref['ext'].W):.3e}  "
              f"V {R.rel(fs.V, ref['ext'].V):.3e}  (bars {R.OUT_BAR:g}, {ref['bar']:g})")
        hits.append(R.rejected(R.as_candidate(fe, fi, fs), ref))
    assert any(hits), fault


def test_failing_frames_and_silence():
    mix = _inputs(1, 3, 30, 3).copy()
    e0, i0, s0 = R.oiva(mix[:, :, :10])
    mix[0, 1, 10, 1] = np.nan
    mix[0, 0, 10, 1] = complex(0.0, np.inf)
    e1, i1, s1 = R.oiva(mix[:, :, :11])
    assert s1.fail.tolist() == [[0, 1, 0]] and s1.n.tolist() == [[11] * 3]
    assert not e1[0, :, 10, 1].any() and not i1[0, :, :, 10, 1].any()
    assert np.array_equal(s1.W[0, 1], s0.W[0, 1]) and np.array_equal(s1.V[0, 1], s0.V[0, 1])
    e2, i2, s2 = R.oiva(mix)
    assert np.isfinite(e2).all() and np.isfinite(s2.W).all() and np.isfinite(s2.V).all()
    mix = _inputs(1, 3, 30, 3).copy()
    mix[..., 2] = 0
    e3, i3, s3 = R.oiva(mix)
    assert not (s3.fail & 1).any() and np.isfinite(e3).all() and not e3[..., 2].any()
    st = R.State(1, 2, 1)
    st.n[:] = R.N_MAX
    R.step(st, np.ones((1, 2, 1), np.complex64))
    assert st.n.tolist() == [[R.N_MAX]]


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_oiva_opts_default", "misonet_oiva_state_bytes", "misonet_oiva_bins_per_pass", "misonet_oiva_reset", "misonet_oiva",
       "misonet_oiva_debug"}


def test_abi_630():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 630
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    assert "misonet_oiva_opts;" in hdr
    for name in NEW:
        assert hasattr(lib, name), name
    o = L.OivaOpts(7, 7, 0.0, 0.0, 0.0)
    assert lib.misonet_oiva_opts_default(C.byref(o)) == L.OK
    assert (o.model, o.ref_ch, o.alpha, o.floor, o.init) == (0, 0, 0.98, 1e-10, 1.0)
    assert lib.misonet_oiva_opts_default(None) == L.EINVAL


def _opts(**kw):
    L = _lib()
    o = L.OivaOpts()
    L.lib().misonet_oiva_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD_OPTS = [dict(model=2), dict(model=-1), dict(ref_ch=-1), dict(ref_ch=6), dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.0),
            dict(alpha=1.5), dict(alpha=math.nan), dict(alpha=math.inf), dict(floor=0.0), dict(floor=-1.0), dict(floor=math.nan),
            dict(floor=math.inf), dict(init=0.0), dict(init=-1.0), dict(init=math.nan), dict(init=math.inf)]
BAD_GEOM = [(0, 6, 129), (-1, 6, 129), (2, 1, 129), (2, 9, 129), (2, 6, 0), (2, 6, 1026), (1 << 22, 6, 1 << 9)]


def test_sizes_and_invalid_arguments():
    L = _lib()
    lib = L.lib()
    n = lib.misonet_oiva_state_bytes(16, 6, 129)
    per_bin = 6 * 6 * 16 + 6 * 6 * 6 * 16 + 8
    assert 16 * 129 * per_bin <= n <= 16 * 129 * per_bin + 2 * 16 and n % 16 == 0        # nothing in it grows with T
    assert lib.misonet_oiva_state_bytes(1, 2, 1) > 0 and lib.misonet_oiva_state_bytes(1, 8, 1025) > 0
    for g in BAD_GEOM:
        assert lib.misonet_oiva_state_bytes(*g) == -1, g
        assert lib.misonet_last_error(), g
    P = [lib.misonet_oiva_bins_per_pass(M) for M in range(2, 9)]
    assert all(p >= 8 and p % 8 == 0 for p in P) and 2 * P[0] + 1 <= 1025, P
    assert lib.misonet_oiva_bins_per_pass(1) == -1 and lib.misonet_oiva_bins_per_pass(9) == -1
    # every limit is refused before any pointer is looked at: the pointers here are null or not addresses at all
    junk = C.c_void_p(8)
    for kw in BAD_OPTS:
        o = _opts(**kw)
        assert lib.misonet_oiva(junk, 2, 6, 10, 129, C.byref(o), junk, junk, junk, 1 << 40, None) == L.EINVAL, kw
        assert lib.misonet_last_error(), kw
        assert lib.misonet_oiva_reset(junk, 2, 6, 129, C.byref(o), None) == L.EINVAL, kw
    o = _opts()
    for B, M, F in BAD_GEOM:
        assert lib.misonet_oiva(junk, B, M, 10, F, C.byref(o), junk, junk, junk, 1 << 40, None) == L.EINVAL, (B, M, F)
        assert lib.misonet_oiva_reset(junk, B, M, F, C.byref(o), None) == L.EINVAL, (B, M, F)
        assert lib.misonet_oiva_debug(junk, B, M, F, None, None, None, None, None) == L.EINVAL, (B, M, F)
    for T in (0, -3):
        assert lib.misonet_oiva(junk, 2, 6, T, 129, C.byref(o), junk, junk, junk, 1 << 40, None) == L.EINVAL
    assert lib.misonet_oiva(junk, 2, 6, 10, 129, None, junk, junk, junk, 1 << 40, None) == L.EINVAL
    assert lib.misonet_oiva(None, 2, 6, 10, 129, C.byref(o), None, None, None, 0, None) == L.EINVAL
    assert lib.misonet_oiva_reset(None, 2, 6, 129, C.byref(o), None) == L.EINVAL
    assert lib.misonet_oiva_debug(None, 2, 6, 129, None, None, None, None, None) == L.EINVAL
    # mix and the outputs must not overlap; a short state is ENOMEM (addresses only: nothing is launched)
    a, b, c, s = C.c_void_p(1 << 30), C.c_void_p(2 << 30), C.c_void_p(3 << 30), C.c_void_p(4 << 30)
    need = lib.misonet_oiva_state_bytes(1, 2, 5)
    assert lib.misonet_oiva(a, 1, 2, 4, 5, C.byref(o), a, None, s, need, None) == L.EINVAL
    assert lib.misonet_oiva(a, 1, 2, 4, 5, C.byref(o), C.c_void_p((1 << 30) + 8), None, s, need, None) == L.EINVAL
    assert lib.misonet_oiva(a, 1, 2, 4, 5, C.byref(o), b, b, s, need, None) == L.EINVAL
    assert lib.misonet_oiva(a, 1, 2, 4, 5, C.byref(o), b, a, s, need, None) == L.EINVAL
    assert lib.misonet_oiva(a, 1, 2, 4, 5, C.byref(o), b, c, s, need - 1, None) == L.ENOMEM


# ---- the Python options -------------------------------------------------------------------------------------------------
def test_online_auxiva_options():
    import misonet_amd as mz
    from misonet_amd.blind import AuxIVA, OnlineAuxIVA
    assert mz.OnlineAuxIVA is OnlineAuxIVA and callable(mz.auxiva_online) and isinstance(mz.SeparateStream, type)
    d = OnlineAuxIVA()
    assert dataclasses.astuple(d) == (0.98, "gauss", 1e-10, 1.0, 0)
    assert OnlineAuxIVA.of(None) == d and OnlineAuxIVA.of(True) == d and OnlineAuxIVA.of(d) is d
    assert OnlineAuxIVA.of("laplace") == OnlineAuxIVA(model="laplace")
    assert OnlineAuxIVA.of(dict(alpha=0.96, ref_ch=1)) == OnlineAuxIVA(alpha=0.96, ref_ch=1)
    with pytest.raises(ValueError):
        OnlineAuxIVA.of(dict(iterations=3))
    with pytest.raises(TypeError):
        OnlineAuxIVA.of(3)
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.alpha = 0.5
    assert d.validate(2) is d and d.validate(8) is d and d.validate() is d
    for kw in BAD_OPTS:
        kw = dict(kw)
        if "model" in kw:
            kw["model"] = "student"
        with pytest.raises(ValueError):
            OnlineAuxIVA(**kw).validate(6)
    for m in (1, 9):
        with pytest.raises(ValueError):
            d.validate(m)
    with pytest.raises(ValueError):
        OnlineAuxIVA(ref_ch=1.0).validate(2)
    o = OnlineAuxIVA(alpha=0.9, model="laplace", floor=1e-8, init=5.0, ref_ch=2).c_opts()
    assert (o.model, o.ref_ch, o.alpha, o.floor, o.init) == (1, 2, 0.9, 1e-8, 5.0)
    assert AuxIVA.of(True) == AuxIVA()                                          # the offline options are what they were
    with pytest.raises(TypeError):
        AuxIVA.of(d)


def test_online_calls_refuse_before_any_launch():
    """bad shapes and fields raise on the host: no device is needed to see them"""
    from misonet_amd.blind import BlindSeparator, SeparateStream, auxiva_online
    mix = _inputs(1, 2, 20, 3)
    with pytest.raises(ValueError):
        auxiva_online(mix, alpha=1.0)
    with pytest.raises(ValueError):
        auxiva_online(mix, ref_ch=2)
    with pytest.raises(ValueError):
        auxiva_online(mix[0])
    with pytest.raises(ValueError):
        auxiva_online(mix[:, :, :0])
    with pytest.raises(ValueError):
        auxiva_online(mix[:, :1])
    with pytest.raises(ValueError):
        SeparateStream(9)
    with pytest.raises(ValueError):
        SeparateStream(2, num_bins=1026)
    with pytest.raises((TypeError, ValueError)):
        SeparateStream(2, iterations=3)
