"""GPU tests of the stacked-Gram bin solver (csrc/stacked_gram.hpp) behind wpe_bin_k and wpd_bin_k at every order and tile edge:
the cases of tests/sg_cases.py -- every NT = ceil(2K / 16) from 1 to 11, Re | Im split on and off a tile edge, every slots-per-wave
deal, every admitted M, the long filters at few microphones (a history window longer than the 64-frame tile), T at the edges of one
and of two tiles, delay around and past a tile, delay >= T -- against the float64 NumPy restatements of tests/wpe_ref.py and
tests/wpd_ref.py, through the runners of test_gpu_wpe.py and test_gpu_wpd.py.

Bars (the project's).  Output: rel-L2 <= 2.4e-7 = 4 x 2^-24, whole-array AND in the worst frame (norms over microphones and bins
for WPE, over bins for WPD), so that one wrong frame at a seam cannot hide in a 200-frame norm.  Filter G / weights wbar: rel-L2 <=
max(100 x the restatement's LU-versus-Cholesky difference on that case, 1e-12).  fail all zero.  tests/test_sg_cases.py shows on the
CPU that the restatement's own sensitivity on every case is two orders below the output bar and that these bars reject every
planted fault.  The module prints every figure (``[sg] ...``); LAB.md has the worst of each family."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sg_cases as S
import wpd_ref
import wpe_ref
from test_gpu_parity import _need_gpu
from test_gpu_wpd import _run as _run_wpd
from test_gpu_wpe import _run as _run_wpe

pytestmark = pytest.mark.gpu

ids = dict(ids=S.case_id)
rel = wpd_ref.rel
WPE_FRAME, WPD_FRAME = (1, 3), (2,)          # a frame of [B, M, T, F] and of [B, T, F]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({np.dtype(np.complex64): np.uint64, np.dtype(np.complex128): np.uint64}.get(x.dtype, np.uint8))


@functools.lru_cache(maxsize=None)
def _wpe_in(B, M, T, F):
    return wpe_ref.reverb_inputs(B, M, T, F)


@functools.lru_cache(maxsize=None)
def _wpd_in(B, M, T, F):
    return wpd_ref.wpd_inputs(B, M, T, F)


@functools.lru_cache(maxsize=None)
def _wpe_ref(case, iterations, diag_load, power_floor=1e-10):
    """(X, G, fail, LU-versus-Cholesky rel-L2 of G) of the restatement, computed once per case"""
    B, M, T, F, taps, delay = case
    mix = _wpe_in(B, M, T, F)
    X, G, bad = wpe_ref.wpe(mix, None, taps, delay, iterations, diag_load, power_floor)
    Gc = wpe_ref.wpe(mix, None, taps, delay, iterations, diag_load, power_floor, solver="chol")[1]
    return X, G, bad, rel(Gc, G)


@functools.lru_cache(maxsize=None)
def _wpd_ref(case, ref_ch, diag_load):
    B, M, T, F, taps, delay = case
    mix, src = _wpd_in(B, M, T, F)
    out, wb, bad, _ = wpd_ref.wpd(src, mix, taps, delay, diag_load, 1e-10, ref_ch)
    wc = wpd_ref.wpd(src, mix, taps, delay, diag_load, 1e-10, ref_ch, solver="chol")[1]
    return out, wb, bad, rel(wc, wb)


def _judge(tag, what, got, want, frame_axes, g, G, lu_chol, bad, fail):
    e_out, e_frame, e_g, bar_g = rel(got, want), S.per_frame(got, want, frame_axes), rel(g, G), max(100.0 * lu_chol, 1e-12)
    print(f"[sg] {tag}: out {e_out:.3e}  frame {e_frame:.3e} (bar {S.OUT_BAR:g})  {what} {e_g:.3e} (LU vs Cholesky {lu_chol:.3e}, "
          f"bar {bar_g:.3e})")
    assert got.dtype == np.complex64 and got.shape == want.shape and g.shape == G.shape
    assert not bad.any() and not fail.any(), (tag, fail)
    assert e_out <= S.OUT_BAR, (tag, e_out)
    assert e_frame <= S.OUT_BAR, (tag, e_frame)
    assert e_g <= bar_g, (tag, e_g, bar_g)


def _check_wpe(case, iterations=3, diag_load=0.0, power_floor=1e-10, family="wpe"):
    B, M, T, F, taps, delay = case
    X, G, bad, lu_chol = _wpe_ref(case, iterations, diag_load, power_floor)
    out, g, fail = _run_wpe(_wpe_in(B, M, T, F), taps=taps, delay=delay, iterations=iterations, diag_load=diag_load,
                            power_floor=power_floor)
    _judge(f"{family} {case} it {iterations} load {diag_load:g} floor {power_floor:g}", "G", out, X, WPE_FRAME, g, G, lu_chol, bad, fail)


def _check_wpd(case, ref_ch, diag_load=0.0, family="wpd"):
    B, M, T, F, taps, delay = case
    want, wb, bad, lu_chol = _wpd_ref(case, ref_ch, diag_load)
    mix, src = _wpd_in(B, M, T, F)
    out, w, fail = _run_wpd(src, mix, taps=taps, delay=delay, diag_load=diag_load, ref_ch=ref_ch)
    _judge(f"{family} {case} ref {ref_ch} load {diag_load:g}", "wbar", out, want, WPD_FRAME, w, wb, lu_chol, bad, fail)


# ---- every order -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ORDERS_WPE, **ids)
def test_wpe_orders(case):
    _need_gpu()
    _check_wpe(case, family="wpe order")


@pytest.mark.parametrize("last_ref", [False, True], ids=["ref0", "refM-1"])
@pytest.mark.parametrize("case", S.ORDERS_WPD, **ids)
def test_wpd_orders(case, last_ref):
    _need_gpu()
    _check_wpd(case, case[1] - 1 if last_ref else 0, family="wpd order")


# ---- T at the edges of one and of two tiles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations,diag_load", [(3, 0.0), (1, 1e-6)])
@pytest.mark.parametrize("case", S.T_EDGES, **ids)
def test_wpe_t_edges(case, iterations, diag_load):
    _need_gpu()
    _check_wpe(case, iterations, diag_load, family="wpe T edge")


@pytest.mark.parametrize("diag_load", [0.0, 1e-6])
@pytest.mark.parametrize("last_ref", [False, True], ids=["ref0", "refM-1"])
@pytest.mark.parametrize("case", S.T_EDGES, **ids)
def test_wpd_t_edges(case, last_ref, diag_load):
    _need_gpu()
    _check_wpd(case, case[1] - 1 if last_ref else 0, diag_load, family="wpd T edge")


# ---- delay around and past one tile ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.DELAY_EDGES, **ids)
def test_wpe_delay_edges(case):
    _need_gpu()
    _check_wpe(case, family="wpe delay edge")


@pytest.mark.parametrize("last_ref", [False, True], ids=["ref0", "refM-1"])
@pytest.mark.parametrize("case", S.DELAY_EDGES, **ids)
def test_wpd_delay_edges(case, last_ref):
    _need_gpu()
    _check_wpd(case, case[1] - 1 if last_ref else 0, family="wpd delay edge")


def test_wpe_floor_that_binds():
    """power_floor = 0.05 limits the weights of the quiet frames, with a second tile of one frame (tests/test_sg_cases.py: dropping
    the floor there misses the bars)"""
    _need_gpu()
    _check_wpe(S.FLOOR_WPE, power_floor=S.FLOOR, family="wpe floor")


# ---- delay >= T: the documented pass-through ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("diag_load", [0.0, 1e-6])
@pytest.mark.parametrize("case", S.WPE_PASS_THROUGH, **ids)
def test_wpe_pass_through(case, diag_load):
    """Z = 0, so R = 0 and no pivot is > 0: fail = 1 in every bin, G reads 0, the output is the input bit for bit; tr(R) = 0: the
    diagonal loading must not rescue the bin"""
    _need_gpu()
    B, M, T, F, taps, delay = case
    mix = _wpe_in(B, M, T, F)
    X, G, bad = wpe_ref.wpe(mix, None, taps, delay, 3, diag_load)
    assert bad.all() and not G.any()
    out, g, fail = _run_wpe(mix, taps=taps, delay=delay, iterations=3, diag_load=diag_load)
    print(f"[sg] wpe pass-through {case} load {diag_load:g}: fail {fail.tolist()}")
    assert np.array_equal(fail, np.ones((B, F), np.int32))
    assert g.shape == G.shape and not _bits(g).any()
    assert np.array_equal(_bits(out), _bits(mix))


# ---- the DNN power across the tile edges of the two transposes ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 65, 33), (1, 3, 64, 32)], ids=lambda s: "x".join(map(str, s)))
def test_wpe_dnn_power_across_transpose_tiles(shape):
    """power_dev with iterations = 1 where T and F reach past one 32 x 32 tile of wpe_in_k (and end on its edge), against the
    restatement with the same power"""
    _need_gpu()
    B, M, T, F = shape
    taps, delay = 2, 1
    mix = _wpe_in(B, M, T, F)
    rng = np.random.default_rng(5)
    power = (np.mean(np.abs(mix) ** 2, axis=1) * rng.uniform(0.5, 2.0, (B, T, F))).astype(np.float32)
    X, G, bad = wpe_ref.wpe(mix, power, taps, delay, 1)
    Gc = wpe_ref.wpe(mix, power, taps, delay, 1, solver="chol")[1]
    out, g, fail = _run_wpe(mix, power, taps=taps, delay=delay, iterations=1)
    _judge(f"wpe dnn power {shape}", "G", out, X, WPE_FRAME, g, G, rel(Gc, G), bad, fail)
    # and it is not the plain first iteration
    assert rel(out, wpe_ref.wpe(mix, None, taps, delay, 1)[0]) > 1e-4


# ---- what the kernel finds in its workspace and in its output changes nothing --------------------------------------------------------
def test_wpe_nan_workspace_changes_nothing():
    """the workspace holds pw and Yt, which wpe_bin_k reads back: every byte it reads it has written in this call"""
    _need_gpu()
    from misonet_amd import _lib
    B, M, T, F, taps, delay = 2, 4, 129, 9, 3, 2
    mix = torch.from_numpy(_wpe_in(B, M, T, F)).cuda()
    L = _lib.lib()
    o = _lib.WpeOpts(taps, delay, 3, 0.0, 1e-10)
    n = L.misonet_wpe_workspace_bytes(B, M, T, F, C.byref(o))
    assert n > 0
    st = _lib.stream_ptr(mix.device)
    got = []
    for fill in (0.0, float("nan")):
        ws = torch.full((n // 8 + 1,), fill, dtype=torch.float64, device="cuda")
        out = torch.full((B, M, T, F), fill, dtype=torch.complex64, device="cuda")
        g = torch.empty((B, F, M * taps, M), dtype=torch.complex128, device="cuda")
        bad = torch.empty((B, F), dtype=torch.int32, device="cuda")
        _lib.check(L.misonet_wpe(mix.data_ptr(), None, B, M, T, F, C.byref(o), out.data_ptr(), ws.data_ptr(), n, st))
        _lib.check(L.misonet_wpe_debug(ws.data_ptr(), B, M, F, C.byref(o), g.data_ptr(), bad.data_ptr(), st))
        got.append((out.cpu().numpy(), g.cpu().numpy(), bad.cpu().numpy()))
    assert np.isfinite(got[0][0]).all() and np.isfinite(got[0][1]).all() and not got[0][2].any()
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert np.array_equal(got[0][2], got[1][2])
    X = wpe_ref.wpe(_wpe_in(B, M, T, F), None, taps, delay, 3)[0]
    assert rel(got[1][0], X) <= S.OUT_BAR and S.per_frame(got[1][0], X, WPE_FRAME) <= S.OUT_BAR


# ---- the same bits twice, and in any batch, at a tile edge ---------------------------------------------------------------------------
def test_wpe_bit_reproducible_and_batch_independent_at_a_tile_edge():
    _need_gpu()
    B, M, T, F, taps, delay = 3, 3, 128, 3, 3, 2
    mix = _wpe_in(B, M, T, F)
    a = _run_wpe(mix, taps=taps, delay=delay)
    b = _run_wpe(mix, taps=taps, delay=delay)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert not a[2].any() and np.abs(a[0]).min() > 0
    for i in range(B):
        one = _run_wpe(np.ascontiguousarray(mix[i:i + 1]), taps=taps, delay=delay)
        assert np.array_equal(_bits(a[0][i]), _bits(one[0][0])), i
        assert np.array_equal(_bits(a[1][i]), _bits(one[1][0])), i


def test_wpd_bit_reproducible_and_batch_independent_at_a_tile_edge():
    _need_gpu()
    B, M, T, F, taps, delay = 3, 3, 128, 3, 3, 2
    mix, src = _wpd_in(B, M, T, F)
    a = _run_wpd(src, mix, taps=taps, delay=delay)
    b = _run_wpd(src, mix, taps=taps, delay=delay)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert not a[2].any() and np.abs(a[0]).min() > 0
    for i in range(B):
        one = _run_wpd(np.ascontiguousarray(src[i:i + 1]), np.ascontiguousarray(mix[i:i + 1]), taps=taps, delay=delay)
        assert np.array_equal(_bits(a[0][i]), _bits(one[0][0])), i
        assert np.array_equal(_bits(a[1][i]), _bits(one[1][0])), i
