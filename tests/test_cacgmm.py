"""CPU checks of the guided cACGMM: the NumPy restatement (tests/cacgmm_ref.py) has the properties that define an EM of this
kind (a log-likelihood that never decreases, the identity at zero iterations, empty frames that pass through, masks that
sharpen on sparse scenes), its inputs are as benign as the device bars assume, the bars reject every planted fault; and the
host side of the C ABI (version 560, prototypes, defaults, validation) and of the Python options behaves.  No kernel is
launched here."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import cacgmm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS = ("bin", "guided")
IDS = lambda s: "x".join(map(str, s))


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return R.case_inputs(shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, prior, iterations=10):
    mix, init, _ = _inputs(shape)
    return R.cacgmm(mix, init, iterations, prior)


@functools.lru_cache(maxsize=None)
def _perm(shape, prior, iterations=10):
    mix, init, _ = _inputs(shape)
    order = np.random.default_rng(5).permutation(shape[3])
    return R.cacgmm(mix, init, iterations, prior, frame_order=order)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", PRIORS)
@pytest.mark.parametrize("shape", R.SHAPES[:5] + R.SHAPES[6:], ids=IDS)
def test_log_likelihood_never_decreases(shape, prior):
    """the EM property, per bin, with diag_load = 0 (the loading is outside the likelihood)"""
    mix, init, _ = _inputs(shape)
    for b in range(shape[0]):
        for f in range(shape[4]):
            r = R.cacgmm_bin(mix[b, f], init[b, :, f], 10, prior, diag_load=0.0)
            lls = np.array(r["lls"])
            assert not r["fail"] and len(lls) == 10
            assert np.all(np.diff(lls) >= -1e-9 * np.abs(lls[:-1])), (b, f, lls)


def test_zero_iterations_is_the_identity():
    mix, init, _ = _inputs(R.SHAPES[0])
    r = R.cacgmm(mix, init, 0)
    assert np.array_equal(r["masks"], init.astype(np.float64)) and not r["fail"].any() and not r["B"].any()


@pytest.mark.parametrize("prior", PRIORS)
def test_empty_frames_pass_through(prior):
    """a zero tail and isolated zero frames keep their initial masks and move no other frame's result"""
    B, S, M, T, F = R.SHAPES[2]
    mix, init, _ = (x.copy() if x is not None else None for x in _inputs(R.SHAPES[2]))
    empty = np.zeros(T, bool)
    empty[[5, 17, 18, 40]] = True
    empty[T - 7:] = True
    mix[:, :, :, empty] = 0
    full = R.cacgmm(mix, init, 10, prior)
    cut = R.cacgmm(mix[..., ~empty], init[..., ~empty], 10, prior)
    assert not full["fail"].any()
    assert np.array_equal(full["masks"][..., empty], init[..., empty].astype(np.float64))
    assert R.max_abs(full["masks"][..., ~empty], cut["masks"]) < 1e-12
    assert R.rel(full["B"], cut["B"]) < 1e-12 and R.rel(full["ll"], cut["ll"]) < 1e-12


@pytest.mark.parametrize("MT", [(2, 40), (3, 70), (4, 200), (6, 300), (8, 200)], ids=IDS)
def test_sharpens_sparse_scenes(MT):
    """on sparse rank-1 scenes ten iterations bring the blurred initial masks (0.4 truth + 0.2: mean distance 0.267) to at
    most 0.6 x that distance in every bin.  Seed 4 of the generator, checked here before it was committed: its worst ratios
    are 0.47 (M = 2, T = 40), 0.20, 0.12, 0.09 and 0.09.  This is a property of benign scenes, not of every scene: three
    classes in two dimensions on 40 frames is the hard end, and of the seeds 0 .. 11 five (0, 1, 8, 10, 11) end a bin of that
    case at 0.73 .. 1.09 (two classes trade places); every seed stays below 0.37 from M = 3 on."""
    M, T = MT
    mix, truth, init = R.sparse_inputs(1, 2, M, T, 4, seed=4)
    got = R.cacgmm(mix, init, 10)["masks"]
    assert not np.array_equal(got, init)
    for f in range(4):
        d0 = np.mean(np.abs(init[0, :, f] - truth[0, :, f]))
        d1 = np.mean(np.abs(got[0, :, f] - truth[0, :, f]))
        assert d1 <= 0.6 * d0, (MT, f, d0, d1)


# ---- sensitivity and bars ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", PRIORS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_float64_path_is_benign(shape, prior):
    """a permuted summation order and the inverse in place of the triangular solve move the masks by less than 1e-10 on every
    case of the device tests: far below the float32 rounding their bar allows"""
    mix, init, _ = _inputs(shape)
    want = _ref(shape, prior)
    assert not want["fail"].any()
    assert R.max_abs(_perm(shape, prior)["masks"], want["masks"]) < 1e-10
    assert R.max_abs(R.cacgmm(mix, init, 10, prior, solver="inv")["masks"], want["masks"]) < 1e-10
    assert 1e-9 < R.max_abs(want["masks"].astype(np.float32), want["masks"]) <= 2.0 ** -25


@pytest.mark.parametrize("prior", PRIORS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_bars_reject_planted_faults(shape, prior):
    """a second evaluation with one thing wrong misses a bar of tests/test_gpu_cacgmm.py (ten iterations)"""
    mix, init, _ = _inputs(shape)
    want, perm = _ref(shape, prior), _perm(shape, prior)
    assert not R.missed(R.figures(perm, want, perm))                         # and a right one does not
    for fault in R.FAULTS:
        if fault == "empty":
            continue                                                         # no empty frame here: its own case below
        got = R.cacgmm(mix, init, 10, prior, fault=fault)
        assert R.missed(R.figures(got, want, perm)), (fault, R.figures(got, want, perm))


@pytest.mark.parametrize("prior", PRIORS)
def test_bars_reject_a_counted_empty_frame(prior):
    B, S, M, T, F = R.SHAPES[2]
    mix, init, _ = (x.copy() if x is not None else None for x in _inputs(R.SHAPES[2]))
    mix[..., T - 7:] = 0
    want = R.cacgmm(mix, init, 10, prior)
    perm = R.cacgmm(mix, init, 10, prior, frame_order=np.random.default_rng(5).permutation(T))
    got = R.cacgmm(mix, init, 10, prior, fault="empty")
    assert not R.missed(R.figures(perm, want, perm)) and R.missed(R.figures(got, want, perm))


def test_failure_rule_generators_and_masks():
    B, S, M, T, F = R.SHAPES[0]
    mix, init, est = _inputs(R.SHAPES[0])
    assert mix.dtype == np.complex64 and init.dtype == np.float32 and init.shape == (B, S + 1, F, T)
    assert np.allclose(init.sum(axis=1), 1.0, atol=1e-6) and est.shape == (B, S, F, M, T)
    mix, init = mix.copy(), init.copy()
    mix[1, 4] = 0                                          # an all-zero bin: every frame empty, n_k = 0
    init[0, 1, 2] = 0                                      # a class with an all-zero initial mask
    r = R.cacgmm(mix, init, 10)
    want = np.zeros((B, F), np.int32)
    want[1, 4] = want[0, 2] = 1
    assert np.array_equal(r["fail"], want)
    assert np.array_equal(r["masks"][1, :, 4], init[1, :, 4]) and np.array_equal(r["masks"][0, :, 2], init[0, :, 2])
    assert not r["B"][1, 4].any() and not r["B"][0, 2].any() and np.isfinite(r["masks"]).all()
    # the masks of the estimates: a zero total gives 1 / K
    e = est.copy()
    e[0, :, 3, :, 7] = 0
    m = mix.copy()
    m[0, 3, :, 7] = 0
    g = R.masks_from_estimates(e, m)
    assert np.all(g[0, :, 3, 7] == np.float32(1.0 / 3)) and np.all(g >= 0)
    # the sparse generator
    mx, truth, g0 = R.sparse_inputs(1, 4, 8, 50, 3)
    assert mx.shape == (1, 3, 8, 50) and truth.shape == g0.shape == (1, 5, 3, 50) and np.all(truth.sum(axis=1) == 1)


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_cacgmm_opts_default", "misonet_cacgmm_workspace_bytes", "misonet_cacgmm", "misonet_cacgmm_debug",
       "misonet_masks_from_estimates", "misonet_pipeline_set_refine"}


def test_abi_560():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 560
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES) and declared == set(L.SIGNATURES)
    assert "misonet_cacgmm_opts;" in hdr and "cACGMM (ABI 560)" in hdr
    for name in NEW:
        assert hasattr(lib, name), name
    o = L.CacgmmOpts(0, 1, 1.0, 1.0)
    assert lib.misonet_cacgmm_opts_default(C.byref(o)) == L.OK
    assert (o.iterations, o.prior, o.diag_load, o.prior_floor) == (10, 0, 1e-8, 1e-6)
    assert lib.misonet_cacgmm_opts_default(None) == L.EINVAL


def _opts(**kw):
    L = _lib()
    o = L.CacgmmOpts()
    L.lib().misonet_cacgmm_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD_OPTS = [dict(iterations=-1), dict(prior=2), dict(prior=-1), dict(diag_load=-1e-9), dict(diag_load=math.nan),
            dict(diag_load=math.inf), dict(prior_floor=-1.0), dict(prior_floor=math.nan), dict(prior_floor=math.inf),
            dict(prior=1, prior_floor=0.0)]


def test_invalid_arguments_report_einval_without_a_device():
    """the checks come before any launch and before any pointer is looked at"""
    L = _lib()
    lib = L.lib()
    p, q = C.c_void_p(256), C.c_void_p(512)
    B, K, F, M, T = 2, 3, 129, 6, 50
    n = lib.misonet_cacgmm_workspace_bytes(B, K, F, M)
    per_bin = 4 + 8 + K * 8 + K * M * M * 16
    assert B * F * per_bin <= n <= B * F * per_bin + 4 * 256
    assert lib.misonet_cacgmm_workspace_bytes(B, K, F, M) == n          # no dependence on T: it is not an argument
    run = lambda o, B=B, K=K, F=F, M=M, T=T, a=p, b=q, ws=1 << 40: lib.misonet_cacgmm(
        p, a, B, K, F, M, T, C.byref(o) if o is not None else None, b, None, p, ws, None)
    for kw in BAD_OPTS:
        o = _opts(**kw)
        assert run(o) == L.EINVAL, kw
        assert lib.misonet_last_error(), kw
        assert lib.misonet_pipeline_set_refine(None, C.byref(o)) == L.EINVAL, kw
    for bad in (dict(M=1), dict(M=9), dict(K=1), dict(K=6), dict(B=0), dict(F=0), dict(T=0)):
        assert run(_opts(), **bad) == L.EINVAL, bad
        g = {**dict(B=B, K=K, F=F, M=M), **{k: v for k, v in bad.items() if k != "T"}}
        if "T" not in bad:
            assert lib.misonet_cacgmm_workspace_bytes(g["B"], g["K"], g["F"], g["M"]) == -1, bad
            assert lib.misonet_cacgmm_debug(p, g["B"], g["K"], g["F"], g["M"], p, None, None, None, None) == L.EINVAL, bad
    assert run(None) == L.EINVAL
    assert run(_opts(), a=p, b=p) == L.EINVAL and b"init_masks" in lib.misonet_last_error()      # in place
    assert run(_opts(), a=None) == L.EINVAL and run(_opts(), b=None) == L.EINVAL
    assert lib.misonet_cacgmm_debug(None, B, K, F, M, p, None, None, None, None) == L.EINVAL
    assert run(_opts(), ws=n - 1) == L.ENOMEM                            # a short workspace, still before any launch
    assert lib.misonet_pipeline_set_refine(None, None) == L.EINVAL
    mk = lambda S=2, M=M, T=T, e=p, o=q: lib.misonet_masks_from_estimates(e, p, B, S, F, M, T, o, None)
    for bad in (dict(S=0), dict(S=5), dict(M=1), dict(M=9), dict(T=0), dict(e=None), dict(o=None)):
        assert mk(**bad) == L.EINVAL, bad


# ---- the Python options -------------------------------------------------------------------------------------------------
def test_python_options():
    import misonet_amd as mz
    from misonet_amd.refine import Refine, cacgmm, masks_from_estimates
    assert mz.Refine is Refine and mz.cacgmm is cacgmm and mz.masks_from_estimates is masks_from_estimates
    rf = Refine()
    assert (rf.iterations, rf.prior, rf.diag_load, rf.prior_floor) == (10, "bin", 1e-8, 1e-6)
    assert Refine.of(None) == rf == Refine.of(True) and Refine.of("guided") == Refine(prior="guided")
    assert Refine.of(dict(iterations=3)) == Refine(iterations=3) and rf.validate(6, 2) is rf and rf.validate() is rf
    o = Refine(iterations=4, prior="guided", diag_load=1e-6, prior_floor=1e-3).c_opts()
    assert (o.iterations, o.prior, o.diag_load, o.prior_floor) == (4, 1, 1e-6, 1e-3)
    for bad in (dict(iterations=-1), dict(iterations=2.5), dict(iterations=True), dict(prior="frame"), dict(diag_load=-1.0),
                dict(diag_load=math.nan), dict(prior_floor=math.inf), dict(prior="guided", prior_floor=0.0)):
        with pytest.raises(ValueError):
            Refine(**bad).validate()
    for m, s in ((1, 2), (9, 2), (6, 0), (6, 5)):
        with pytest.raises(ValueError):
            rf.validate(m, s)
    with pytest.raises(ValueError):
        Refine.of(dict(iteration=3))
    with pytest.raises(TypeError):
        Refine.of(3)
    # the calls refuse on the host: no device, no library call
    y, g = np.zeros((1, 5, 4, 20), np.complex64), np.zeros((1, 3, 5, 20), np.float32)
    for bad in (dict(iterations=-1), dict(prior="x"), dict(diag_load=-1.0), dict(prior="guided", prior_floor=0.0)):
        with pytest.raises(ValueError):
            cacgmm(y, g, **bad)
    with pytest.raises(ValueError):
        cacgmm(y, g[:, :, :4])
    with pytest.raises(ValueError):
        cacgmm(y, np.zeros((1, 6, 5, 20), np.float32))
    with pytest.raises(ValueError):
        masks_from_estimates(np.zeros((1, 2, 5, 4, 19), np.complex64), y)
