"""CPU checks of the WPD convolutional beamformer: the NumPy restatement (tests/wpd_ref.py) is pinned by another route (the WPE
filter followed by a Souden solve), its inputs are as well conditioned as the device bars assume, the bars reject every planted
fault; and the host side of the C ABI (version 530, prototypes, defaults, validation) and of the Python options behaves.  No
kernel is launched here."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import wpd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


# ---- the restatement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(shape):
    B, M, T, F, taps, delay = shape
    mix, src = R.wpd_inputs(B, M, T, F)
    return mix, src, R.wpd(src, mix, taps, delay)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_is_wpe_then_souden(shape):
    """wbar = [q; -G q]: G the WPE filter under the weights of the source estimate, q the Souden weight on the WPE output"""
    B, M, T, F, taps, delay = shape
    mix, src, (out, wb, bad, cond) = _case(shape)
    assert not bad.any() and wb.shape == (B, F, M * (taps + 1)) and out.shape == (B, T, F)
    for ref_ch in (0, M - 1):
        w = wb if ref_ch == 0 else R.wpd(src, mix, taps, delay, ref_ch=ref_ch)[1]
        worst = max(R.rel(R.wpe_then_souden_bin(mix[b, f], src[b, f], taps, delay, ref_ch=ref_ch), w[b, f])
                    for b in range(B) for f in range(F))
        assert worst < 1e-11, (ref_ch, worst)
    # the filter is distortionless towards the source estimate in the sense of the Souden solve: tr-normalised column
    Y = mix[0, 0].astype(np.complex128)
    ybar = np.concatenate([Y, R.stack(Y, taps, delay)])
    assert np.allclose(wb[0, 0].conj() @ ybar, out[0, :, 0])


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inputs_are_well_conditioned(shape):
    """LU against Cholesky moves the float64 output by less than 1e-10 on every case of the device tests (measured: at most
    8.1e-14 at cond(R) <= 1.1e4), far below the one complex64 rounding the output bar allows"""
    B, M, T, F, taps, delay = shape
    mix, src, _ = _case(shape)
    for ref_ch in (0, M - 1):
        for diag_load in (0.0, 1e-6):
            out, wb, bad, cond = R.wpd(src, mix, taps, delay, diag_load, ref_ch=ref_ch)
            oc, wc, _, _ = R.wpd(src, mix, taps, delay, diag_load, ref_ch=ref_ch, solver="chol")
            assert not bad.any() and cond < 1e5
            assert R.rel(oc, out) < 1e-10 and R.rel(wc, wb) < 1e-10, (ref_ch, diag_load, R.rel(oc, out))
            assert 1e-9 < R.rel(out.astype(np.complex64), out) < 2.0 ** -24


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bars_reject_planted_faults(shape):
    """a second evaluation with one thing wrong misses a bar of tests/test_gpu_wpd.py: delay off by one, the wrong reference
    microphone, a missing conjugate in the apply, a stale frame at a tile seam, Phibar in the wrong block and, where T reaches past
    one tile, a dropped last tile and a history that reads zero across the seam"""
    B, M, T, F, taps, delay = shape
    mix, src, (out, wb, _, _) = _case(shape)
    wbar_bar = max(100.0 * R.rel(R.wpd(src, mix, taps, delay, solver="chol")[1], wb), 1e-12)
    for fault in R.FAULTS:
        if fault == "floor":
            continue                                      # the floor does not bind at 1e-10: its own case below
        if fault in R.TILE_FAULTS and T <= R.TILE:
            continue                                      # no second tile to lose: tests/test_sg_cases.py has their cases
        o, w, _, _ = R.wpd(src, mix, taps, delay, fault=fault)
        assert R.rel(o, out) > 100 * R.OUT_BAR, (fault, R.rel(o, out))
        if fault != "conj":                               # the weights themselves are right there
            assert R.rel(w, wb) > 100 * wbar_bar, (fault, R.rel(w, wb))


def test_bars_reject_a_dropped_floor():
    """with power_floor = 0.05 the floor binds (the case test_gpu_wpd.py runs for it): dropping it moves output and weights"""
    B, M, T, F, taps, delay = R.SHAPES[2]
    mix, src = R.wpd_inputs(B, M, T, F)
    out, wb, bad, _ = R.wpd(src, mix, taps, delay, power_floor=0.05)
    o, w, _, _ = R.wpd(src, mix, taps, delay, power_floor=0.05, fault="floor")
    assert not bad.any() and R.rel(o, out) > 100 * R.OUT_BAR and R.rel(w, wb) > 1e-6
    assert R.rel(R.wpd(src, mix, taps, delay, power_floor=0.05, solver="chol")[0], out) < 1e-10
    assert R.rel(R.wpd(src, mix, taps, delay)[0], out) > 100 * R.OUT_BAR             # and it is not the default's result


def test_failure_rule_and_generator():
    B, M, T, F, taps, delay = R.SHAPES[0]
    mix, src = R.wpd_inputs(B, M, T, F)
    a, b = R.wpd_inputs(B, M, T, F)
    assert mix.dtype == np.complex64 and mix.shape == (B, F, M, T) == src.shape and np.array_equal(a, mix) and np.array_equal(b, src)
    assert not np.array_equal(R.wpd_inputs(B, M, T, F, seed=1)[0], mix) and not np.array_equal(R.wpd_inputs(B, M, T, F, which=1)[1], src)
    mix, src = mix.copy(), src.copy()
    mix[1, 4] = 0                                          # an all-zero bin of the observation (and of the estimate)
    src[1, 4] = 0
    src[0, 2] = 0                                          # an all-zero source estimate under a live observation
    out, wb, bad, _ = R.wpd(src, mix, taps, delay)
    want = np.zeros((B, F), np.int32)
    want[1, 4] = want[0, 2] = 1
    assert np.array_equal(bad, want)
    assert not out[1, :, 4].any() and not out[0, :, 2].any() and not wb[1, 4].any() and not wb[0, 2].any()
    assert np.isfinite(out).all() and np.linalg.norm(out[0, :, 0]) > 0


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_wpd_opts_default", "misonet_wpd_workspace_bytes", "misonet_wpd", "misonet_wpd_debug", "misonet_pipeline_set_wpd"}


def test_abi_530():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 530
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    assert "misonet_wpd_opts;" in hdr and "WPD (ABI 530)" in hdr
    assert declared == set(L.SIGNATURES)                                     # header == bindings, the six new names included
    for name in NEW:
        assert hasattr(lib, name), name
    o = L.WpdOpts(0, 0, 1.0, 1.0, 3)
    assert lib.misonet_wpd_opts_default(C.byref(o)) == L.OK
    assert (o.taps, o.delay, o.diag_load, o.power_floor, o.ref_ch) == (5, 3, 0.0, 1e-10, 0)
    assert lib.misonet_wpd_opts_default(None) == L.EINVAL


def _opts(**kw):
    L = _lib()
    o = L.WpdOpts()
    L.lib().misonet_wpd_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# with M = 6: the order 6 (taps + 1) <= 88 allows 13 taps
BAD_OPTS = [dict(taps=0), dict(taps=-1), dict(taps=14), dict(delay=0), dict(delay=-2), dict(ref_ch=6), dict(ref_ch=-1),
            dict(diag_load=-1e-9), dict(diag_load=math.nan), dict(diag_load=math.inf), dict(power_floor=-1.0),
            dict(power_floor=math.nan), dict(power_floor=math.inf)]


def test_invalid_fields_report_einval_without_a_device():
    """the checks come before any launch and before any pointer is looked at"""
    L = _lib()
    lib = L.lib()
    p = C.c_void_p(256)
    B, F, M, T = 2, 129, 6, 50
    size = lambda B, F, M, o: lib.misonet_wpd_workspace_bytes(B, F, M, C.byref(o) if o is not None else None)
    n = size(B, F, M, _opts())
    assert B * F * (4 + 36 * 16) <= n <= B * F * (4 + 36 * 16) + 1024         # fail int32 and wbar complex128 [K] per bin
    assert size(1, 3, 8, _opts(taps=10)) > 0 and size(1, 3, 2, _opts(taps=43)) > 0           # the order 88 both ways
    assert size(1, 3, 8, _opts(taps=11)) == -1 and size(1, 3, 2, _opts(taps=44)) == -1
    for kw in BAD_OPTS:
        o = _opts(**kw)
        assert size(B, F, M, o) == -1, kw
        assert lib.misonet_last_error(), kw
        assert lib.misonet_wpd(p, p, B, F, M, T, C.byref(o), p, p, 1 << 40, None) == L.EINVAL, kw
        assert lib.misonet_wpd_debug(p, B, F, M, C.byref(o), p, None, None) == L.EINVAL, kw
        assert lib.misonet_pipeline_set_wpd(None, C.byref(o)) == L.EINVAL, kw
    for m in (1, 9):
        assert size(B, F, m, _opts(taps=1)) == -1
        assert lib.misonet_wpd(p, p, B, F, m, T, C.byref(_opts(taps=1)), p, p, 1 << 40, None) == L.EINVAL
        assert lib.misonet_wpd_debug(p, B, F, m, C.byref(_opts(taps=1)), p, None, None) == L.EINVAL
    assert size(B, F, M, None) == -1 and size(0, F, M, _opts()) == -1 and size(B, 0, M, _opts()) == -1
    assert lib.misonet_wpd(p, p, B, F, M, T, None, p, p, 1 << 40, None) == L.EINVAL
    # T <= delay + taps - 1 = 7
    assert lib.misonet_wpd(p, p, B, F, M, 7, C.byref(_opts()), p, p, 1 << 40, None) == L.EINVAL
    assert b"delay + taps" in lib.misonet_last_error()
    assert lib.misonet_wpd(None, p, B, F, M, T, C.byref(_opts()), p, p, 1 << 40, None) == L.EINVAL
    assert lib.misonet_wpd_debug(None, B, F, M, C.byref(_opts()), p, None, None) == L.EINVAL
    assert lib.misonet_pipeline_set_wpd(None, None) == L.EINVAL
    # a short workspace, still before any launch
    assert lib.misonet_wpd(p, p, B, F, M, T, C.byref(_opts()), p, p, n - 1, None) == L.ENOMEM
    assert lib.misonet_wpd(p, p, B, F, M, 8, C.byref(_opts()), p, p, 0, None) == L.ENOMEM


# ---- the Python options -------------------------------------------------------------------------------------------------
def test_python_options():
    from misonet_amd.beamform import Apply_Beamforming, Beamformer
    bf = Beamformer(kind="wpd")
    assert (bf.taps, bf.delay, bf.diag_load, bf.power_floor, bf.ref_ch) == (5, 3, 0.0, 1e-10, 0)
    assert Beamformer.of("wpd") == bf and Beamformer.of(dict(kind="wpd", taps=4)) == Beamformer(kind="wpd", taps=4)
    assert bf.validate(6) is bf and bf.validate() is bf and Beamformer(kind="wpd", epsi=1e-3).validate(6)
    o = Beamformer(kind="wpd", taps=4, delay=2, diag_load=1e-6, power_floor=1e-8, ref_ch=3).wpd_opts()
    assert (o.taps, o.delay, o.diag_load, o.power_floor, o.ref_ch) == (4, 2, 1e-6, 1e-8, 3)
    # the existing kinds ignore the new fields, and their options are what they were
    s = Beamformer(kind="souden", taps=0, delay=-1, diag_load=-1.0).validate(6).c_opts()
    assert (s.kind, s.noise, s.ref_ch) == (1, 0, 0)
    for bad in (dict(noise="mix"), dict(condition=1e-3), dict(trace_normalize=True), dict(ban=True), dict(taps=0),
                dict(taps=2.5), dict(delay=0), dict(taps=14), dict(ref_ch=6), dict(diag_load=-1.0), dict(diag_load=math.nan),
                dict(power_floor=math.inf), dict(power_floor=-1e-3)):
        with pytest.raises(ValueError):
            Beamformer(kind="wpd", **bad).validate(6)
    for m in (1, 9):
        with pytest.raises(ValueError):
            Beamformer(kind="wpd", taps=1).validate(m)
    with pytest.raises(ValueError):
        bf.c_opts()                                        # not a misonet_bf_opts kind
    # Apply_Beamforming refuses on the host: no device, no library call
    x = np.zeros((1, 5, 4, 20), np.complex64)
    for bad in (dict(taps=0), dict(delay=0), dict(ref_ch=4), dict(noise="mix"), dict(ban=True), dict(taps=22),
                dict(diag_load=-1.0)):
        with pytest.raises(ValueError):
            Apply_Beamforming(x, x, beamformer="wpd", **bad)
    with pytest.raises(ValueError):
        Apply_Beamforming(x, x, beamformer=dict(kind="wpd", tap=3))
