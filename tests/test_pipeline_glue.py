"""CPU tests of tests/pipeline_glue_ref.py: the checker of the device test (tests/test_gpu_pipeline_glue.py) must be able to fail.

A toy "network" (a fixed complex mixing of the input channels, the speakers in an order that depends on which microphone comes first)
stands for MISO_1: its outputs over the circular shifts are permuted copies of one another plus an order-dependent residue, as the real
network's are.  ``pipeline_glue_ref.emulate`` runs the fused pass's glue on it in NumPy.  At S = 3, M = 4, B = 2 the healthy emulation
passes ``judge`` (what the device test asserts about the glue) and every fault of ``FAULTS`` is rejected; at S = 2 the two faults of
``BLIND_AT_S2`` (composition in the other order, gather with the inverse permutation) give the very same bits as the healthy pass --
every permutation of two elements is its own inverse and all of them commute -- which is why the device test runs at S >= 3.
``pipeline_glue_ref.read_est`` (the read path of steps 4b and 5, tests/test_gpu_pipeline_steps.py) gets the same treatment on synthetic
planes and hand-made selections."""
import numpy as np
import pytest

import pipeline_glue_ref as G

T, F = 5, 9


class ToyNet:
    """[N, M, T, F] complex -> [N, S, T, F] complex64: speaker s = (mean over the channels) * gain plane s + 0.05 * (a channel-order
    dependent mixture); the speakers come out in the order ``table[x[n, 0, 0, 0]]`` (keyed by the first channel: the shift)"""

    def __init__(self, S, M, table, seed):
        r = np.random.default_rng(seed)
        self.gain = (r.standard_normal((S, T, F)) + 1j * r.standard_normal((S, T, F))) * (1.0 + np.arange(S))[:, None, None]
        self.w = r.standard_normal((S, M)) + 1j * r.standard_normal((S, M))
        self.table = table

    def __call__(self, x):
        y = x.mean(1)[:, None] * self.gain[None] + 0.05 * np.einsum("sc,nctf->nstf", self.w, x)
        return np.stack([y[n][self.table[complex(x[n, 0, 0, 0])]] for n in range(x.shape[0])]).astype(np.complex64)


def _case(S, M, B, ref_ch, orders, c, seed):
    """orders[b][k]: the speaker order of the toy network when microphone k of item b comes first; c[b]: the forced clean order"""
    r = np.random.default_rng(seed)
    mix = (r.standard_normal((B, M, T, F)) + 1j * r.standard_normal((B, M, T, F))).astype(np.complex64)
    mix *= (1.0 + 2.0 * np.arange(B, dtype=np.float32))[:, None, None, None]
    net = ToyNet(S, M, {complex(mix[b, k, 0, 0]): np.array(orders[b][k]) for b in range(B) for k in range(M)}, seed + 1)
    raw = net(np.stack([np.roll(mix[b], -k, axis=0) for b in range(B) for k in range(M)]))          # the explicit roll
    clean = np.stack([raw[b * M + ref_ch][np.array(c[b])] for b in range(B)])
    rms = np.sqrt((np.abs(clean) ** 2).mean())
    clean = (clean + 0.05 * rms * (r.standard_normal(clean.shape) + 1j * r.standard_normal(clean.shape))).astype(np.complex64)
    for a in (mix, raw, clean):
        a.setflags(write=False)
    return dict(S=S, M=M, B=B, ref_ch=ref_ch, mix=mix, clean=clean, raw=raw, net=net, c=np.array(c))


@pytest.fixture(scope="module")
def case3():
    orders = [[(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)], [(2, 1, 0), (0, 1, 2), (1, 0, 2), (1, 2, 0)]]
    return _case(3, 4, 2, 2, orders, [(1, 0, 2), (1, 2, 0)], 50)


@pytest.fixture(scope="module")
def case2():
    return _case(2, 4, 2, 2, [[(0, 1), (1, 0), (0, 1), (1, 0)], [(1, 0), (1, 0), (0, 1), (0, 1)]], [(1, 0), (0, 1)], 60)


def _judge(k, got, what):
    return G.judge(k["mix"], k["clean"], k["raw"], got, k["M"], k["S"], k["ref_ch"], what)


def _emulate(k, fault=None):
    return G.emulate(k["net"], k["mix"], k["clean"], k["M"], k["S"], k["ref_ch"], fault)


def test_healthy_emulation_passes_with_full_coverage(case3):
    k = case3
    e, obs, res = _judge(k, _emulate(k), "healthy S=3")
    cov = G.coverage(e["sel_shift"], e["sel_clean"])
    print(G.coverage_line("toy S=3 M=4", cov, res))
    assert cov["non_involutive"] > 0 and cov["non_commuting"] > 0 and cov["clean_differs"], cov
    assert np.array_equal(e["sel_clean"], k["c"]) and np.array_equal(obs, e["sel_final"]) and not res["undecided"]
    assert all(list(e["sel_shift"][b, k["ref_ch"]]) == [0, 1, 2] for b in range(k["B"]))
    assert any(list(e["sel_shift"][b, 0]) != [0, 1, 2] for b in range(k["B"]))      # the anchor at shift 0 would be another one
    assert res["ratio_shift"] > 1e3 and res["ratio_clean"] > 1e3                      # decided by far: nothing here is marginal
    # without clean references: the identity, and the estimates at ref_ch are the raw ones
    e0, obs0, _ = G.judge(k["mix"], None, k["raw"], G.emulate(k["net"], k["mix"], None, k["M"], k["S"], k["ref_ch"]), k["M"], k["S"],
                          k["ref_ch"], "healthy S=3, no clean")
    assert np.array_equal(obs0, e0["sel_shift"]) and np.array_equal(obs0[:, k["ref_ch"]], np.tile(np.arange(3), (2, 1)))


def test_every_fault_is_rejected(case3):
    k, verdict = case3, {}
    for fault in G.FAULTS:
        try:
            _judge(k, _emulate(k, fault), fault)
            verdict[fault] = "passed"
        except AssertionError as err:
            verdict[fault] = "rejected"
            why = str(err).splitlines()[0][:150]
        print(f"[glue-fault] S=3 {fault}: {verdict[fault]}" + (f" ({why})" if verdict[fault] == "rejected" else ""))
    assert all(v == "rejected" for v in verdict.values()), verdict


def test_two_speakers_cannot_see_the_selection_rule(case2):
    """the reason for S >= 3 on the device"""
    k = case2
    healthy = _emulate(k)
    e, obs, _ = _judge(k, healthy, "healthy S=2")
    assert any(list(p) == [1, 0] for p in e["sel_shift"].reshape(-1, 2)) and [1, 0] in e["sel_clean"].tolist()   # not all identity
    cov = G.coverage(e["sel_shift"], e["sel_clean"])
    assert cov["non_involutive"] == 0 and cov["non_commuting"] == 0
    verdict = {}
    for fault in G.FAULTS:
        got = _emulate(k, fault)
        try:
            _judge(k, got, fault)
            verdict[fault] = "passed"
        except AssertionError:
            verdict[fault] = "rejected"
        print(f"[glue-fault] S=2 {fault}: {verdict[fault]}")
        if fault in G.BLIND_AT_S2:
            assert all(np.array_equal(got[key], healthy[key]) for key in healthy), fault      # the same bits: nothing could tell
    assert [f for f, v in verdict.items() if v == "passed"] == list(G.BLIND_AT_S2), verdict


def test_observed_sel_needs_exactly_one_bit_equal_plane(case3):
    k = case3
    got = _emulate(k)
    m1 = got["miso1"].copy()
    m1[1, 2, 3, T - 1, F - 1] = np.nextafter(m1[1, 2, 3, T - 1, F - 1].real, np.float32(9)) + 1j * m1[1, 2, 3, T - 1, F - 1].imag
    with pytest.raises(AssertionError, match="bit-equal to 0"):
        G.observed_sel(m1, k["raw"], k["M"])
    raw = k["raw"].copy()
    raw[5, 1] = raw[5, 0]                                             # two identical planes: the choice cannot be read off
    with pytest.raises(AssertionError, match="bit-equal to 2|bit-equal to 0"):
        G.observed_sel(G.gather(raw, got["sel"], k["M"]), raw, k["M"])
    m1 = got["miso1"].copy()
    m1[0, 1, 1] = m1[0, 0, 1]                                         # one plane twice: no permutation
    with pytest.raises(AssertionError, match="no permutation"):
        G.observed_sel(m1, k["raw"], k["M"])


def test_planted_read_faults_and_what_two_speakers_cannot_see():
    """``read_est`` (src_row in pipeline mode, the read path of steps 4b and 5) with one planted fault at a time, on synthetic raw
    planes and hand-made selections.  S = 3, M = 3, B = 2 with per-microphone and per-item different, non-involutive rows tells every
    variant apart by plain array inequality.  S = 2 cannot see the inverse permutation whatever its rows are, B = 1 cannot see the
    rows of item 0, S = 1 sees nothing; and the geometry the fused-pass tests of the step-5 features share -- S = 2, here with the
    same selection at every microphone and item, which nothing there rules out -- sees only the imaginary plane.  Hence the
    geometries of tests/test_gpu_pipeline_steps.py: S >= 3, B >= 2, and the variants checked on each case's own selection."""
    r = np.random.default_rng(80)

    def raw_of(B, M, S):
        return (r.standard_normal((B * M, S, T, F)) + 1j * r.standard_normal((B * M, S, T, F))).astype(np.complex64)

    def seen(raw, sel, M, S):
        healthy = G.read_est(raw, sel, M, S)
        assert np.array_equal(healthy, G.gather(raw, sel, M))                # the healthy read is the exported miso1
        return {f: not np.array_equal(G.read_est(raw, sel, M, S, f), healthy) for f in G.READ_FAULTS}

    sel3 = np.array([[(1, 2, 0), (0, 1, 2), (2, 0, 1)], [(0, 2, 1), (2, 0, 1), (1, 0, 2)]])
    assert seen(raw_of(2, 3, 3), sel3, 3, 3) == dict(mic0=True, item0=True, inverse=True, imag=True)
    assert all(G.READ_FAULT_NEEDS[f](3, 2) for f in G.READ_FAULTS)
    # two speakers: rows that differ per microphone and per item, and still no sight of the inverse
    sel2 = np.array([[(1, 0), (0, 1), (1, 0)], [(0, 1), (0, 1), (1, 0)]])
    got = seen(raw_of(2, 3, 2), sel2, 3, 2)
    assert got == dict(mic0=True, item0=True, inverse=False, imag=True), got
    assert [f for f in G.READ_FAULTS if not G.READ_FAULT_NEEDS[f](2, 2)] == ["inverse"]
    # two speakers, one swap everywhere (every shift agrees with ref_ch, both items given in the same clean order)
    got = seen(raw_of(2, 6, 2), np.tile(np.array([1, 0]), (2, 6, 1)), 6, 2)
    assert got == dict(mic0=False, item0=False, inverse=False, imag=True), got
    # ... and with the identity everywhere (no clean references, no re-ordered shift) nothing at all
    got = seen(raw_of(2, 6, 2), np.tile(np.array([0, 1]), (2, 6, 1)), 6, 2)
    assert not any(got.values()), got
    # one item; one speaker
    got = seen(raw_of(1, 3, 3), sel3[:1], 3, 3)
    assert got == dict(mic0=True, item0=False, inverse=True, imag=True) and not G.READ_FAULT_NEEDS["item0"](3, 1)
    got = seen(raw_of(2, 3, 1), np.zeros((2, 3, 1), np.int64), 3, 1)
    assert not any(got.values()) and not any(G.READ_FAULT_NEEDS[f](1, 2) for f in G.READ_FAULTS)
    with pytest.raises(AssertionError):
        G.read_est(raw_of(2, 3, 3), sel3, 3, 3, "no such fault")


def test_first_minimum_wins_and_undecided_items_are_bounded():
    r = np.random.default_rng(70)
    S, M, ref = 3, 3, 0
    raw = (r.standard_normal((M, S, T, F)) + 1j * r.standard_normal((M, S, T, F))).astype(np.complex64)
    raw[:, 1] *= 2
    raw[:, 2] *= 4
    raw[1, 1] = raw[1, 0]                                             # exact tie in item (0, 1): permutations 0 and 2 cost the same
    e = G.expected(raw, None, M, S, ref)
    assert e["margin_shift"][0, 1] == 0.0 and list(e["sel_shift"][0, 1]) == [0, 1, 2]     # itertools order: the first minimum
    assert e["margin_shift"][0, 2] > 2 * e["tol_shift"][0, 2] > 0
    # (bit-equal planes cannot be told apart by observed_sel, so the near tie is made of two planes one ulp apart)
    raw[1, 1] = (np.nextafter(raw[1, 0].real, np.float32(9)) + 1j * raw[1, 0].imag).astype(np.complex64)
    e = G.expected(raw, None, M, S, ref)
    assert 0 < e["margin_shift"][0, 1] <= 2 * e["tol_shift"][0, 1]
    for sel1, ok in (((0, 1, 2), True), ((1, 0, 2), True), ((0, 2, 1), False), ((2, 1, 0), False)):
        sel = e["sel_final"].copy()
        sel[0, 1] = sel1
        obs = G.observed_sel(G.gather(raw, sel, M), raw, M)
        if ok:
            assert G.check(e, obs, ref)["undecided"] == [(0, 1)]
        else:
            with pytest.raises(AssertionError, match="undecided shift item"):
                G.check(e, obs, ref)
    raw[2, 1] = (np.nextafter(raw[2, 0].real, np.float32(9)) + 1j * raw[2, 0].imag).astype(np.complex64)
    e = G.expected(raw, None, M, S, ref)
    with pytest.raises(AssertionError, match="another input seed"):
        G.check(e, G.observed_sel(G.gather(raw, e["sel_final"], M), raw, M), ref)


def test_tol_covers_float32_distances(case3):
    """the device's distances (float32 magnitudes and differences, float64 sums) are within tol / 4 * 3 of the float64 ones"""
    k = case3
    raw, M, S, ref = k["raw"], k["M"], k["S"], k["ref_ch"]
    e = G.expected(raw, k["clean"], M, S, ref)
    m32 = np.sqrt(raw.real * raw.real + raw.imag * raw.imag)          # float32
    assert m32.dtype == np.float32
    P = G.perms(S)
    for b in range(k["B"]):
        for m in range(M):
            A, Bc = m32[b * M + ref], m32[b * M + m]
            D = np.array([[np.abs(A[i] - Bc[j]).astype(np.float64).sum() for j in range(S)] for i in range(S)])
            cost = D[np.arange(S)[None, :], P].sum(1)
            assert np.abs(cost - e["cost_shift"][b, m]).max() <= 0.75 * e["tol_shift"][b, m]
