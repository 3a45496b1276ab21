"""CPU checks of the cases of tests/sg_cases.py, which tests/test_gpu_sg_edges.py runs on the device: they reach every branch of the
stacked-Gram scheme (csrc/stacked_gram.hpp) that an integer of the caller selects; the library's host check admits each; the
float64 restatements (tests/wpe_ref.py, tests/wpd_ref.py) are insensitive enough on them that the output bar tests the kernel and
not the inputs; and the bars of the device tests reject every planted fault on the cases meant to show it.  No kernel is launched.

The conditioning is a condition on the inputs: LU against Cholesky (for WPE also another summation order, block = 64) must move
the restatement's output, whole-array and in its worst frame, by no more than OUT_BAR / 100 = 2.4e-9.  OUT_BAR = 4 x 2^-24 allows one
complex64 rounding plus the device's float64 deviation; the condition keeps the second term two orders below the bar.  Figures of
this module on the cases as they stand (seed 0; whole-array / worst frame): WPE orders but the two long filters <= 7.3e-12 /
2.2e-11, (2, 40) at T = 300 1.1e-10 / 9.0e-10, (1, 80) at T = 2000 5.2e-11 / 8.2e-10 (at T = 230, the rule of the other orders, it is
1.5e-8 whole-array and at T = 600 6.3e-9 in the worst frame: both refused); WPD orders <= 2.3e-14 / 3.5e-13; every T and delay edge
<= 3.7e-14 / 1.3e-13.  Every planted fault misses a bar by four orders or more on each of its cases."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import sg_cases as S
import wpd_ref
import wpe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENS_BAR = S.OUT_BAR / 100.0
MARGIN = 100.0                       # a planted fault misses a bar by this factor at least (the margin of tests/test_wpd.py)
FLOOR = S.FLOOR                      # the power_floor that binds (test_gpu_wpd.py runs WPD with it, test_gpu_sg_edges.py WPE)
FLOOR_WPE = S.FLOOR_WPE
FLOOR_WPD = wpd_ref.SHAPES[2]
ids = dict(ids=S.case_id)


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


# ---- the tile arithmetic -------------------------------------------------------------------------------------------------
def test_geometry_restates_the_header():
    hdr = open(os.path.join(ROOT, "misonet_amd", "csrc", "stacked_gram.hpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, hdr).group(1))
    assert (const("SG_TT"), const("SG_THREADS") // 64, const("SG_SLOTS")) == (S.TILE, S.WAVES, S.SLOTS)
    assert "(SG_TT + taps - 1) | 1" in hdr and "(2 * K + 15) / 16" in hdr and "NT * (NT + 1) / 2" in hdr
    g = S.geometry(8, 10)
    assert (g["K"], g["K2"], g["NT"], g["ntiles"], g["zl"]) == (88, 176, 11, 66, 73) and g["slots"] == (9, 9, 8, 8, 8, 8, 8, 8)
    assert S.geometry(1, 1) == dict(K=2, K2=4, NT=1, ntiles=1, slots=(1, 0, 0, 0, 0, 0, 0, 0), zl=64)
    for kernel in ("wpe", "wpd"):
        for M, taps in S.admitted(kernel):
            g = S.geometry(M, taps)
            deal = [0] * S.WAVES                                              # tile tau, counted row by row, goes to wave tau % 8
            for tau in range(sum(I + 1 for I in range(g["NT"]))):
                deal[tau % S.WAVES] += 1
            assert tuple(deal) == g["slots"] and max(deal) <= S.SLOTS and 16 * (g["NT"] - 1) < g["K2"] <= 16 * g["NT"], (M, taps)
    assert max(M * (t + 1) for M, t in S.admitted("wpe")) == max(M * (t + 1) for M, t in S.admitted("wpd")) == 88


# ---- coverage: asserted, not described -------------------------------------------------------------------------------------
def _cases(kernel):
    return (S.OLD_WPE + S.NEW_WPE) if kernel == "wpe" else (S.OLD_WPD + S.NEW_WPD)


def test_the_older_shapes_are_restated_right():
    import test_gpu_wpe
    assert S.OLD_WPE == test_gpu_wpe.SHAPES + [(1, 6, 1001, 129, 10, 3)] and S.OLD_WPD == wpd_ref.SHAPES
    assert S.OUT_BAR == test_gpu_wpe.OUT_BAR == wpd_ref.OUT_BAR and S.TILE == wpe_ref.TILE == wpd_ref.TILE


@pytest.mark.parametrize("kernel", ["wpe", "wpd"])
def test_cases_reach_every_branch(kernel):
    geo = [S.geometry(M, taps) for _, M, _, _, taps, _ in _cases(kernel)]
    assert {g["NT"] for g in geo} == set(range(1, 12))
    assert {0, 2} <= {g["K2"] % 16 for g in geo}                               # Re | Im split on a tile edge, and two rows past one
    assert {c[1] for c in _cases(kernel)} == set(range(1 if kernel == "wpe" else 2, 9))
    every = {S.geometry(M, taps)["slots"] for M, taps in S.admitted(kernel)}
    assert {g["slots"] for g in geo} == every and len(every) == 11
    # the staged z window longer than two tiles: taps - 1 > 64 is WPE's alone (M = 1); WPD's longest, 2 x 43 taps, is reached
    longest = max(S.geometry(M, taps)["zl"] for M, taps in S.admitted(kernel))
    assert max(g["zl"] for g in geo) == longest == (143 if kernel == "wpe" else 106)
    new = S.NEW_WPE if kernel == "wpe" else S.NEW_WPD
    # the frames: the last tile exactly full and holding one frame, at one and at two tiles; the delays around and past a tile
    assert {63, 64, 65, 127, 128, 129} <= {c[2] for c in new}
    assert {62, 63, 64, 65, 70, 130} <= {c[5] for c in new} and all(c[5] < c[2] for c in new)
    assert all(c[5] >= c[2] for c in S.WPE_PASS_THROUGH)
    assert len(set(new)) == len(new) and all(c[0] == 1 and c[3] in (2, 3) for c in new)
    orders = S.ORDERS_WPE if kernel == "wpe" else S.ORDERS_WPD
    for (_, M, T, _, taps, delay), mt in zip(orders, S.ORDERS_WPE_MT if kernel == "wpe" else S.ORDERS_WPD_MT):
        order = M * taps if kernel == "wpe" else M * (taps + 1)
        assert (M, taps) == mt and delay == 3 and T >= max(130, 2 * order + 70)
        assert T == max(130, 2 * order + 70) or (kernel == "wpe" and mt in S.LONG_T)


def test_the_library_admits_every_case():
    L = _lib()
    lib = L.lib()
    for B, M, T, F, taps, delay in S.NEW_WPE + S.WPE_PASS_THROUGH + [(2, 2, 65, 33, 2, 1), (1, 3, 64, 32, 2, 1), (2, 4, 129, 9, 3, 2)]:
        for iterations, diag_load in ((3, 0.0), (1, 1e-6)):
            o = L.WpeOpts(taps, delay, iterations, diag_load, 1e-10)
            assert lib.misonet_wpe_workspace_bytes(B, M, T, F, C.byref(o)) > 0, (B, M, T, F, taps, delay)
    p = C.c_void_p(256)
    for B, M, T, F, taps, delay in S.NEW_WPD:
        for ref_ch in (0, M - 1):
            o = L.WpdOpts(taps, delay, 1e-6, 1e-10, ref_ch)
            assert lib.misonet_wpd_workspace_bytes(B, F, M, C.byref(o)) > 0, (B, M, T, F, taps, delay)
            # T > delay + taps - 1: with a workspace of no bytes the call gets as far as the size check, past every field
            assert lib.misonet_wpd(p, p, B, F, M, T, C.byref(o), p, p, 0, None) == L.ENOMEM, (B, M, T, F, taps, delay)
    for B, M, T, F, taps, delay in S.WPE_PASS_THROUGH:                          # ... and WPD refuses these
        assert lib.misonet_wpd(p, p, B, F, M, T, C.byref(L.WpdOpts(taps, delay, 0.0, 1e-10, 0)), p, p, 1 << 40, None) == L.EINVAL


# ---- the restatements on the cases, each evaluation computed once -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wpe_in(B, M, T, F):
    return wpe_ref.reverb_inputs(B, M, T, F)


@functools.lru_cache(maxsize=None)
def _wpd_in(B, M, T, F):
    return wpd_ref.wpd_inputs(B, M, T, F)


@functools.lru_cache(maxsize=None)
def _wpe(case, iterations=3, diag_load=0.0, power_floor=1e-10, solver="lu", block=None, fault=None):
    B, M, T, F, taps, delay = case
    return wpe_ref.wpe(_wpe_in(B, M, T, F), None, taps, delay, iterations, diag_load, power_floor, solver, block, fault)


@functools.lru_cache(maxsize=None)
def _wpd(case, ref_ch=0, diag_load=0.0, power_floor=1e-10, solver="lu", fault=None):
    B, M, T, F, taps, delay = case
    mix, src = _wpd_in(B, M, T, F)
    return wpd_ref.wpd(src, mix, taps, delay, diag_load, power_floor, ref_ch, solver, fault)[:3]


WPE_FRAME = (1, 3)                   # a frame of the WPE output [B, M, T, F]: norms over microphones and bins
WPD_FRAME = (2,)                     # a frame of the WPD output [B, T, F]: norms over bins


def _wpe_sens(case, **kw):
    X, G, bad = _wpe(case, **kw)
    assert not bad.any(), case
    whole = frame = g = 0.0
    for other in (dict(solver="chol"), dict(block=S.TILE)):
        Xo, Go, bo = _wpe(case, **kw, **other)
        assert not bo.any(), (case, other)
        whole, frame = max(whole, wpd_ref.rel(Xo, X)), max(frame, S.per_frame(Xo, X, WPE_FRAME))
        if "solver" in other:
            g = wpd_ref.rel(Go, G)
    return whole, frame, g


def _wpd_sens(case, **kw):
    out, w, bad = _wpd(case, **kw)
    oc, wc, bc = _wpd(case, solver="chol", **kw)
    assert not bad.any() and not bc.any(), case
    return wpd_ref.rel(oc, out), S.per_frame(oc, out, WPD_FRAME), wpd_ref.rel(wc, w)


# ---- conditioning: a condition on the inputs, not a measurement of the kernel ---------------------------------------------------
@pytest.mark.parametrize("case", S.NEW_WPE, **ids)
def test_wpe_conditioning(case):
    """a case that misses this gets another T, never another bar"""
    variants = [dict()] + ([dict(iterations=1, diag_load=1e-6)] if case in S.T_EDGES else [])
    for kw in variants:
        whole, frame, _ = _wpe_sens(case, **kw)
        print(f"[sg] wpe conditioning {case} {kw}: whole {whole:.3e}  frame {frame:.3e}  (bar {SENS_BAR:.1e})")
        assert whole <= SENS_BAR and frame <= SENS_BAR, (case, kw, whole, frame)


@pytest.mark.parametrize("case", S.NEW_WPD, **ids)
def test_wpd_conditioning(case):
    variants = [dict(ref_ch=r) for r in (0, case[1] - 1)] + ([dict(diag_load=1e-6)] if case in S.T_EDGES else [])
    for kw in variants:
        whole, frame, _ = _wpd_sens(case, **kw)
        print(f"[sg] wpd conditioning {case} {kw}: whole {whole:.3e}  frame {frame:.3e}  (bar {SENS_BAR:.1e})")
        assert whole <= SENS_BAR and frame <= SENS_BAR, (case, kw, whole, frame)


def test_floor_cases_conditioning():
    for sens in (_wpe_sens(FLOOR_WPE, power_floor=FLOOR), _wpd_sens(FLOOR_WPD, power_floor=FLOOR)):
        assert sens[0] <= SENS_BAR and sens[1] <= SENS_BAR, sens


# ---- the bars reject every planted fault --------------------------------------------------------------------------------------
def _wpe_miss(case, fault, **kw):
    """by what factor the faulty restatement misses the bars of the device test: (output, worst frame, G); inf: a bin failed"""
    X, G, _ = _wpe(case, **kw)
    Xf, Gf, bad = _wpe(case, fault=fault, **kw)
    if bad.any():
        return (np.inf,) * 3
    bar_g = max(100.0 * _wpe_sens(case, **kw)[2], 1e-12)
    return wpd_ref.rel(Xf, X) / S.OUT_BAR, S.per_frame(Xf, X, WPE_FRAME) / S.OUT_BAR, wpd_ref.rel(Gf, G) / bar_g


def _wpd_miss(case, fault, **kw):
    out, w, _ = _wpd(case, **kw)
    of, wf, bad = _wpd(case, fault=fault, **kw)
    if bad.any():
        return (np.inf,) * 3
    bar_w = max(100.0 * _wpd_sens(case, **kw)[2], 1e-12)
    return wpd_ref.rel(of, out) / S.OUT_BAR, S.per_frame(of, out, WPD_FRAME) / S.OUT_BAR, wpd_ref.rel(wf, w) / bar_w


def test_every_fault_has_its_cases():
    assert set(wpe_ref.TILE_FAULTS) < set(wpe_ref.FAULTS) and set(wpd_ref.TILE_FAULTS) < set(wpd_ref.FAULTS)
    assert set(wpe_ref.FAULTS) == {"delay", "tap_order", "conj", "stale_power"} | {"floor"} | set(wpe_ref.TILE_FAULTS)
    assert set(wpd_ref.FAULTS) == {"delay", "ref_ch", "conj", "seam", "block"} | {"floor"} | set(wpd_ref.TILE_FAULTS)
    assert FLOOR_WPE in S.T_EDGES and FLOOR_WPD == (1, 3, 70, 4, 3, 1)


@pytest.mark.parametrize("case", S.ORDERS_WPE, **ids)
def test_wpe_bars_reject_faults_at_every_order(case):
    """delay off by one, the taps in the wrong order, no conjugate in the apply, the power never updated"""
    M, taps = case[1], case[4]
    for fault in ("delay", "tap_order", "conj", "stale_power"):
        out, frame, g = _wpe_miss(case, fault)
        print(f"[sg] wpe fault {fault} {case}: misses out x{out:.3g}  frame x{frame:.3g}  G x{g:.3g}")
        if fault == "tap_order":
            # X is invariant under the permutation: the G bar is what catches it -- where it is a permutation at all
            assert out < 1e-2
            assert g >= MARGIN if M > 1 and taps > 1 else g == 0.0, (fault, g)
        else:
            assert out >= MARGIN and frame >= MARGIN, (fault, out, frame)
            assert g >= MARGIN, (fault, g)


TILE_CASES = [c for c in S.T_EDGES if c[2] in (65, 127, 129)]


@pytest.mark.parametrize("case", TILE_CASES + [S.ORDERS_WPE[3]], **ids)
def test_wpe_bars_reject_tile_faults(case):
    """a stale frame at the seam, a dropped last tile, a history that reads zero across the seam, the output written over the
    history of the tiles behind it"""
    for fault in wpe_ref.TILE_FAULTS:
        out, frame, g = _wpe_miss(case, fault)
        print(f"[sg] wpe fault {fault} {case}: misses out x{out:.3g}  frame x{frame:.3g}  G x{g:.3g}")
        assert max(out, frame, g) >= MARGIN and frame >= MARGIN, (fault, out, frame, g)
        if fault != "inplace":                                                  # the filter itself is right there
            assert g >= MARGIN, (fault, g)


@pytest.mark.parametrize("case", [c for c in S.T_EDGES if c[2] <= 64], **ids)
def test_tile_faults_are_invisible_in_one_tile(case):
    """tail, hist and inplace are no faults where there is one tile: as they must be (tail at T = 64 only: below it the one tile
    is the dropped one)"""
    for fault in ("hist", "inplace") + (("tail",) if case[2] == 64 else ()):
        a, b = _wpe(case), _wpe(case, fault=fault)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), fault
    for fault in ("hist",) + (("tail",) if case[2] == 64 else ()):
        a, b = _wpd(case), _wpd(case, fault=fault)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), fault


@pytest.mark.parametrize("case", S.ORDERS_WPD, **ids)
def test_wpd_bars_reject_faults_at_every_order(case):
    for fault in ("delay", "ref_ch", "conj", "seam", "block"):
        out, frame, w = _wpd_miss(case, fault)
        print(f"[sg] wpd fault {fault} {case}: misses out x{out:.3g}  frame x{frame:.3g}  wbar x{w:.3g}")
        assert out >= MARGIN and frame >= MARGIN, (fault, out, frame)
        if fault != "conj":                                                     # the weights themselves are right there
            assert w >= MARGIN, (fault, w)


@pytest.mark.parametrize("case", TILE_CASES + [S.ORDERS_WPD[3]], **ids)
def test_wpd_bars_reject_tile_faults(case):
    for fault in ("seam",) + wpd_ref.TILE_FAULTS:
        out, frame, w = _wpd_miss(case, fault)
        print(f"[sg] wpd fault {fault} {case}: misses out x{out:.3g}  frame x{frame:.3g}  wbar x{w:.3g}")
        assert out >= MARGIN and frame >= MARGIN and w >= MARGIN, (fault, out, frame, w)


@pytest.mark.parametrize("case", S.DELAY_EDGES, **ids)
def test_bars_reject_a_lost_history_at_every_delay(case):
    """with delay >= 64 the history of a tile lies wholly in earlier tiles: the fault zeroes Z, and shows as fail = 1 in every
    bin -- as it does from delay + taps - 1 >= 64 on, where the row of the last tap is all zero; below that it would miss the bars"""
    taps, delay = case[4:]
    for miss, run in ((_wpe_miss, _wpe), (_wpd_miss, _wpd)):
        bad = run(case, fault="hist")[2]
        if delay + taps - 1 >= S.TILE:
            assert bad.all() and not run(case)[2].any()
            if delay >= S.TILE:
                B, M, T, F = case[:4]
                assert not wpe_ref.stack_hist(_wpe_in(B, M, T, F)[0, :, :, 0], taps, delay).any()
        else:
            m = miss(case, "hist")
            assert not bad.any() and min(m) >= MARGIN, m
        m = miss(case, "delay")
        assert min(m) >= MARGIN, m


def test_bars_reject_a_dropped_floor():
    """with power_floor = 0.05 the floor binds: dropping it moves output and filter; and it is not the default's result"""
    for miss, run, case in ((_wpe_miss, _wpe, FLOOR_WPE), (_wpd_miss, _wpd, FLOOR_WPD)):
        m = miss(case, "floor", power_floor=FLOOR)
        print(f"[sg] fault floor {case}: misses out x{m[0]:.3g}  frame x{m[1]:.3g}  filter x{m[2]:.3g}")
        assert min(m) >= MARGIN, (case, m)
        assert wpd_ref.rel(run(case)[0], run(case, power_floor=FLOOR)[0]) > MARGIN * S.OUT_BAR


# ---- pass-through ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.WPE_PASS_THROUGH, **ids)
def test_wpe_pass_through(case):
    """delay >= T: Z = 0, R = 0, no pivot: fail = 1 in every bin, G = 0, X = Y bit for bit -- and diag_load tr(R) / N = 0 does
    not rescue the bin"""
    B, M, T, F, taps, delay = case
    mix = _wpe_in(B, M, T, F)
    assert not wpe_ref.stack(mix[0, :, :, 0], taps, delay).any()
    for iterations, diag_load in ((3, 0.0), (1, 1e-6)):
        X, G, bad = _wpe(case, iterations, diag_load)
        assert bad.all() and not G.any() and G.shape == (B, F, M * taps, M)
        assert np.array_equal(X, mix.astype(np.complex128)) and np.array_equal(X.astype(np.complex64).view(np.uint64), mix.view(np.uint64))
