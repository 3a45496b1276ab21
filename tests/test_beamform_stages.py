"""CPU tests of the stage comparator of tests/beamform_ref.py: the comparator of the device tests (tests/test_gpu_beamform_stages.py)
must be able to fail.

* a healthy SECOND evaluation -- ``beamform_ref.device_order``: the kernels' summation order (64 lane partials in float32 with
  stride 64, reduced in float64; w rounded to float32; the sum over the microphones in float32) with LAPACK where the kernels have
  Jacobi and Gaussian elimination -- passes every stage at the K of the device tests.  Measured here on ``stage_inputs(2, 9, M, T)``,
  M in {2, 3, 5, 6, 7, 8}, T in {2 M, 65, 257}: yardstick 2.4e-8 ... 2.3e-7 (eig), 4.8e-8 ... 2.5e-7 (solve), 3.5e-8 ... 6.4e-8 (apply);
  device order / yardstick 0.02 ... 0.46 (eig), 0.02 ... 0.87 (solve), 1.00 (apply: NumPy's complex64 product sums the
  microphones in the same order), phase 0.006 ... 0.25 of its derived bound; souden / gev 0.05 ... 0.83, lambda_max <= 1.9;
* every injected fault is rejected by the stage it belongs to with at least 2 K to spare, on the item it touches and there only;
* a missing or doubled eps moves w by only 0.3 ... 9 yardsticks on those inputs; on ``eps_inputs`` (the residual in M - 2 frames
  only and small: Phi_n is singular without eps) it is decisive, while the healthy restatement stays under K;
* the PIT distances: the device's arithmetic restated passes, frames >= 256 dropped do not;
* the eigenvector property of the edge inputs: healthy under the bound, a lost frame over it.
"""
import numpy as np
import pytest

import beamform_ref as R

F = 9
HEALTHY = [(M, T) for M in (2, 3, 5, 6, 7, 8) for T in (2 * M, 65, 257)]
FAULT_AT = [(3, 65), (7, 257), (6, 257)]
# fault -> the stage that has to reject it
FAULT_STAGE = {"phis_last": "eig", "phin_last": "solve", "w16": "apply", "out_hole": "apply", "phase_prev": "phase",
               "item_swap": "eig", "stale_T": "eig", "argmax2": "eig", "conj_s": "eig", "conj_n": "solve"}
ALSO = {"item_swap": ("solve",), "stale_T": ("solve",)}                 # and these as well
WHOLE_ITEM = ("w16", "phase_prev", "item_swap")                         # not confined to one bin
EVERY_ITEM = ("w16", "phase_prev")                                      # nor to one item

_cache = {}


def _inputs(M, T):
    if (M, T) not in _cache:
        src, mix = R.stage_inputs(2, F, M, T, 100 * M + T)
        for a in (src, mix):
            a.setflags(write=False)
        _cache[(M, T)] = (src, mix)
    return _cache[(M, T)]


@pytest.mark.parametrize("M,T", HEALTHY)
def test_device_order_passes(M, T):
    src, mix = _inputs(M, T)
    res = R.stage_compare(src, mix, R.device_order(src, mix))
    assert sorted(res) == ["apply", "eig", "phase", "solve"]
    R.check_stages(res, "mvdr", M, T)
    for stage, lo, hi in (("eig", 2e-8, 3e-7), ("solve", 4e-8, 3e-7), ("apply", 3e-8, 8e-8)):
        for c in res[stage]:
            assert lo <= c["whole32"] <= hi, (stage, c)                 # float32 round-off and nothing else: K x it is not vacuous


@pytest.mark.parametrize("kind", ["souden", "gev"])
@pytest.mark.parametrize("noise", ["residual", "mix"])
@pytest.mark.parametrize("M", [3, 5, 7])
def test_device_order_passes_other_kinds(kind, noise, M):
    for T in (2 * M, 65):
        src, mix = _inputs(M, T)
        res = R.stage_compare(src, mix, R.device_order(src, mix, kind=kind, noise=noise), kind=kind, noise=noise)
        assert sorted(res) == (["apply", "lam", "solve"] if kind == "gev" else ["apply", "solve"])
        R.check_stages(res, kind, M, T)


@pytest.mark.parametrize("M", [3, 5, 7])
def test_device_order_passes_with_options(M):
    o = dict(condition=1e-3, trace_normalize=True, ban_=True)
    src, mix = _inputs(M, 65)
    R.check_stages(R.stage_compare(src, mix, R.device_order(src, mix, **o), **o), "mvdr+options", M, 65)
    o = dict(kind="souden", ref_ch=M - 1)
    R.check_stages(R.stage_compare(src, mix, R.device_order(src, mix, **o), **o), "souden+ref", M, 65)


@pytest.mark.parametrize("M,T", FAULT_AT)
@pytest.mark.parametrize("fault", sorted(FAULT_STAGE))
def test_fault_is_rejected(fault, M, T):
    src, mix = _inputs(M, T)
    res = R.stage_compare(src, mix, R.device_order(src, mix, fault=fault))
    for stage in (FAULT_STAGE[fault],) + ALSO.get(fault, ()):
        healthy, hit = res[stage][0], res[stage][R.FAULT_ITEM]
        r = R.ratios(hit)
        print(f"[fault-ratio] {fault} {stage} {M} {T} " + " ".join(f"{v:.3g}" for v in r))
        assert bool(R.failures(healthy)) == (fault in EVERY_ITEM), (fault, stage, healthy)      # item 0 is untouched
        assert R.failures(hit), f"fault {fault!r} ({R.FAULTS[fault]}) passed stage {stage} at K = {R.K:g}"
        assert min(r) >= 2 * R.K, (fault, stage, r)                     # whole tensor AND worst bin (AND worst frame)
        if fault not in WHOLE_ITEM:
            assert hit["f"] == F // 2, hit                              # the bin the fault sits in
        if fault == "out_hole":
            assert hit["t"] == T // 2, hit
        with pytest.raises(AssertionError) as ei:
            R.check(hit, f"stage {stage}, kind mvdr, M = {M}, T = {T}, item {R.FAULT_ITEM}")
        assert f"stage {stage}" in str(ei.value) and f"(K = {R.K:g})" in str(ei.value) and "worst bin f = " in str(ei.value)
    for stage, items in res.items():                                    # and no other stage blames itself for it
        if stage not in (FAULT_STAGE[fault],) + ALSO.get(fault, ()):
            assert not R.failures(items[0]) and not R.failures(items[R.FAULT_ITEM]), (fault, stage)


@pytest.mark.parametrize("M,T", FAULT_AT)
def test_stale_frame_of_the_padded_plane(M, T):
    """the ``Tp`` fault with what the padded planes really hold behind frame T - 1: the next bin's first frame"""
    src, mix = _inputs(M, T)
    stale = src[R.FAULT_ITEM, F // 2 + 1, :, 0]
    res = R.stage_compare(src, mix, R.device_order(src, mix, fault="stale_T", stale=stale))
    for stage in ("eig", "solve"):
        r = R.ratios(res[stage][R.FAULT_ITEM])
        print(f"[fault-ratio] stale_T(next bin) {stage} {M} {T} " + " ".join(f"{v:.3g}" for v in r))
        assert min(r) >= 2 * R.K, (stage, r)


@pytest.mark.parametrize("M,T", FAULT_AT)
def test_eps_is_not_decisive_on_the_rank1_inputs(M, T):
    """recorded, not wished for: on the inputs of the matrix a missing or doubled eps moves w by 2.8 ... 9 yardsticks as a whole tensor
    on item 0 and by 0.26 ... 0.9 on the louder item 1 (Phi_n nine times as large), so it is not rejected with 2 K to spare"""
    src, mix = _inputs(M, T)
    for fault in ("eps0", "eps2"):
        r = [R.ratios(c)[0] for c in R.stage_compare(src, mix, R.device_order(src, mix, fault=fault))["solve"]]
        print(f"[fault-ratio] {fault} solve {M} {T} " + " ".join(f"{v:.3g}" for v in r))
        assert min(r) < 2 * R.K and max(r) <= 12.0, r


@pytest.mark.parametrize("M,T", [(3, 65), (5, 65), (7, 257), (8, 64)])
def test_eps_is_decisive_on_a_rank_deficient_residual(M, T):
    src, mix = R.eps_inputs(2, F, M, T, 7 + M)
    n = (mix - src)[0, 0]
    assert np.linalg.matrix_rank(n @ n.conj().T) == M - 2                # Phi_n is singular without eps
    res = R.stage_compare(src, mix, R.device_order(src, mix))
    R.check_stages(res, "mvdr/eps", M, T)
    assert max(max(R.ratios(c)) for c in res["solve"]) <= R.K
    for fault in ("eps0", "eps2"):
        bad = R.stage_compare(src, mix, R.device_order(src, mix, fault=fault))["solve"]
        for c in bad:
            r = R.ratios(c)
            print(f"[fault-ratio] {fault} solve(eps input) {M} {T} " + " ".join(f"{v:.3g}" for v in r))
            assert R.failures(c) and min(r) >= 2 * R.K, (fault, r)


PIT_T = (63, 64, 65, 255, 256, 257, 600)


@pytest.mark.parametrize("S", [2, 3])
def test_pit_distances(S):
    for T in PIT_T:
        a, c = R.pit_inputs(3, S, T, F, 1000 * S + T)
        e, e32, _ = R.pit_compare(R.pit_dist(a, c, np.complex64, device_order_=True), a, c)
        print(f"[pit-ratio] S={S} T={T}: yardstick {e32:.2e} device order {e / e32:.3g}")
        assert 0 < e32 <= 3e-7 and e <= R.K * e32, (S, T, e, e32)
        if T > 256:                                                     # the second pass over T lost
            e, e32, where = R.pit_compare(R.pit_dist(a, c, np.complex64, device_order_=True, drop_from=256), a, c)
            print(f"[fault-ratio] pit_drop256 S={S} T={T}: {e / e32:.3g}")
            assert e >= 2 * R.K * e32, (S, T, e, e32, where)


@pytest.mark.parametrize("M", [5, 8])
@pytest.mark.parametrize("name", R.EDGES)
def test_eigenvector_property(name, M):
    src, mix = R.edge_inputs(name, 2, F, M, 40 + M)
    dev = R.device_order(src, mix)
    d, y32, lim = R.eig_property(dev["steer1"], src)
    print(f"[bf-eig] {name} M={M}: deficit {d.max():.2e} yardstick {y32.max():.2e} worst deficit / bound {np.max(d / lim):.3g}")
    assert np.isfinite(dev["out"]).all() and np.isfinite(dev["w"]).all()
    assert (d <= lim).all(), (name, M, d, lim)
    if name == "white":                                                 # the property can fail: one bin without its last frame
        d, _, lim = R.eig_property(R.device_order(src, mix, fault="phis_last")["steer1"], src)
        assert d[R.FAULT_ITEM, F // 2] >= 2 * lim[R.FAULT_ITEM, F // 2] and (d > lim).sum() == 1, (d, lim)
