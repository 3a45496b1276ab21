"""Scoring on the CPU: the NumPy restatement (tests/score_ref.py) against closed forms and against the reference's own
criterion (tests/golden/g15_score.npz, written by tools/gen_golden_score.py from criterion.py), the host functions of
misonet_amd.score against the restatement, and the validation of the three C entry points (ABI 480), none of which
needs a device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import score_ref
from conftest import golden


def _signals(seed, n, target_db):
    """r, e = a r + d with d orthogonal to the centred r and scaled so that SI-SDR(e, r) = target_db exactly (in float64)"""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal(n)
    d = rng.standard_normal(n)
    rc = r - r.mean()
    d = d - d.mean()
    d = d - rc * (d @ rc) / (rc @ rc)
    a = 0.7
    d *= np.sqrt((a * a * (rc @ rc)) / (10.0 ** (target_db / 10.0)) / (d @ d))
    return r, a * r + d


def _st(e, r, n=None):
    """float64 statistics of float64 signals (score_ref.wave_stats keeps float64 inputs as they are)"""
    return score_ref.wave_stats(np.asarray(e)[None], np.asarray(r)[None], n)[0, 0]


def test_scaled_copy_is_perfect():
    r = np.random.default_rng(0).standard_normal(4096)
    r = np.round(r * 1024) / 1024                      # short mantissas: every sum below is exact
    assert score_ref.si_sdr_one(_st(0.5 * r, r), r.size) == float("inf")


@pytest.mark.parametrize("db", [-20.0, 0.0, 13.5, 40.0, 60.0])
def test_orthogonal_noise_gives_the_chosen_si_sdr(db):
    r, e = _signals(1, 64000, db)
    assert abs(score_ref.si_sdr_one(_st(e, r), r.size) - db) <= 1e-9


@pytest.mark.parametrize("db", [0.0, 30.0])
def test_offsets_change_nothing(db):
    r, e = _signals(2, 20000, db)
    base = score_ref.si_sdr_one(_st(e, r), r.size)
    assert abs(score_ref.si_sdr_one(_st(e + 0.25, r), r.size) - base) <= 1e-9
    assert abs(score_ref.si_sdr_one(_st(e, r - 0.125), r.size) - base) <= 1e-9
    assert abs(score_ref.si_sdr_one(_st(3.0 * e, r), r.size) - base) <= 1e-9      # scale-invariant


@pytest.mark.parametrize("db", [5.0, 50.0])
def test_chunked_sums_equal_one_piece(db):
    """a recording in chunks of 4096 with the zero-padded tail of the last one left out (n_valid = chunk - gap)"""
    L, chunk = 3 * 4096 + 1000, 4096
    r, e = _signals(3, L, db)
    gap = 4 * chunk - L
    ep, rp = np.concatenate([e, np.full(gap, 0.3)]), np.concatenate([r, np.zeros(gap)])    # the estimate is not silent there
    blocks, ns = [], []
    for k in range(4):
        nv = chunk - gap if k == 3 else chunk
        blocks.append(score_ref.wave_stats(ep[None, k * chunk:(k + 1) * chunk], rp[None, k * chunk:(k + 1) * chunk], nv))
        ns.append(nv)
    st, n = score_ref.combine(blocks, ns)
    assert n == L
    assert abs(score_ref.si_sdr_one(st[0, 0], n) - score_ref.si_sdr_one(_st(e, r), L)) <= 1e-9
    assert abs(score_ref.snr_one(st[0, 0], n) - score_ref.snr_one(_st(e, r), L)) <= 1e-9


def test_silent_reference_is_invalid():
    rng = np.random.default_rng(4)
    est = rng.standard_normal((2, 1000)).astype(np.float32)
    ref = np.stack([rng.standard_normal(1000).astype(np.float32), np.zeros(1000, np.float32)])
    s = score_ref.score(est, ref)
    assert list(s["valid"]) == [True, False]
    assert np.isfinite(s["si_sdr"][0]) and np.isnan(s["si_sdr"][1]) and np.isnan(s["snr"][1])
    const = np.stack([ref[0], np.full(1000, 0.5, np.float32)])         # a constant reference is silent once centred
    assert list(score_ref.score(est, const)["valid"]) == [True, False]


def test_int16_estimates_are_scaled_once():
    rng = np.random.default_rng(5)
    q = rng.integers(-32768, 32768, size=(2, 5000)).astype(np.int16)
    ref = rng.standard_normal((2, 5000)).astype(np.float32)
    a = score_ref.wave_stats(q, ref)
    b = score_ref.wave_stats(q.astype(np.float64) / 32767.0, ref)
    e = np.abs(q.astype(np.float64)) / 32767.0
    mag = np.stack([e.sum(1)[:, None] + 0 * ref.sum(1), 0 * e.sum(1)[:, None] + np.abs(ref).sum(1),
                    (e * e).sum(1)[:, None] + 0 * ref.sum(1), 0 * e.sum(1)[:, None] + (ref.astype(np.float64) ** 2).sum(1),
                    e @ np.abs(ref.astype(np.float64)).T], axis=-1)
    assert np.all(np.abs(a - b) <= 5000 * 2.0 ** -52 * mag)            # worst case of any order of 5000 rounded terms
    assert np.allclose(score_ref.si_sdr(a, 5000), score_ref.si_sdr(b, 5000), rtol=0, atol=1e-9)


@pytest.mark.parametrize("S", [2, 3])
def test_spectral_criterion_against_the_reference(S):
    """score_ref against criterion.py's own answers: relative 1e-6 and the same permutation"""
    g = golden("g15_score.npz")
    est, ref = g[f"est{S}"], g[f"ref{S}"]
    B = est.shape[0]
    perms = list(itertools.permutations(range(S)))
    vals, enh = [], np.zeros(S)
    for b in range(B):
        pair = score_ref.spec_pairs(est[b], ref[b])
        v, p = score_ref.upit(pair)
        vals.append(v)
        assert tuple(p) == perms[int(g[f"upit_idx{S}"][b])]
        assert tuple(p) != tuple(range(S))                              # the fixture's winner is not the identity ...
        others = [sum(pair[i, q[i]] for i in range(S)) for q in perms if tuple(q) != tuple(p)]
        assert min(others) > 2.0 * v                                    # ... and wins by a wide margin
        enh += score_ref.loss_enhance(est[b], ref[b])
    want = float(g[f"upit{S}"])
    print(f"S={S} uPIT ref {want!r} restated {np.mean(vals)!r} rel {abs(np.mean(vals) - want) / want:.3e}")
    assert abs(np.mean(vals) - want) <= 1e-6 * want                     # loss_uPIT: the batch mean of the minima
    rel = np.abs(enh / B - g[f"enh{S}"]) / g[f"enh{S}"]
    print(f"S={S} loss_Enhance rel {rel}")
    assert np.all(rel <= 1e-6)                                          # loss_Enhance: the batch sum over B


def test_host_functions_equal_the_restatement():
    from misonet_amd import score
    rng = np.random.default_rng(6)
    for trial in range(20):
        S, n = int(rng.integers(1, 5)), int(rng.integers(100, 5000))
        est = rng.standard_normal((S, n)).astype(np.float32)
        ref = (rng.standard_normal((S, n)) * rng.uniform(0.1, 2.0)).astype(np.float32) + (0.5 * est if trial % 2 else 0)
        ref = ref.astype(np.float32)
        if trial % 5 == 0:
            ref[-1] = 0
        mix = ref.sum(0)
        st, sm = score_ref.wave_stats(est, ref), score_ref.wave_stats(mix[None], ref)
        assert np.array_equal(score.si_sdr(st, n), score_ref.si_sdr(st, n), equal_nan=True)
        assert np.array_equal(score.snr(st, n), score_ref.snr(st, n), equal_nan=True)
        want = score_ref.score_from_stats(st, n, sm)
        got = score.from_stats(st, n, sm)
        for key in ("si_sdr", "si_sdr_mix", "si_sdri", "snr", "si_sdr_best"):
            assert np.array_equal(getattr(got, key), want[key], equal_nan=True), key
        assert list(got.valid) == list(want["valid"]) and got.perm_best == want["perm_best"] and got.n_samples == n
        d = got.as_dict()
        assert isinstance(d["si_sdr"], list) and isinstance(d["n_samples"], int) and d["loss_miso1"] is None
        halves = [score_ref.wave_stats(est[:, :n // 2], ref[:, :n // 2]), score_ref.wave_stats(est[:, n // 2:], ref[:, n // 2:])]
        a, na = score.combine(halves, [n // 2, n - n // 2])
        b, nb = score_ref.combine(halves, [n // 2, n - n // 2])
        assert np.array_equal(a, b) and na == nb == n
    pair = rng.uniform(1, 2, size=(3, 3))
    assert score.upit(pair) == score_ref.upit(pair)


def test_best_perm_takes_the_first_optimum():
    from misonet_amd import score
    for bp in (score.best_perm, score_ref.best_perm):
        assert bp(np.zeros((3, 3))) == [0, 1, 2]                               # every permutation ties: the first
        assert bp(np.array([[1.0, 5.0], [5.0, 1.0]])) == [1, 0]
        assert bp(np.array([[1.0, 1.0], [1.0, 1.0]])) == [0, 1]
        M = np.array([[0.0, 9.0, 0.0], [0.0, 0.0, 9.0], [9.0, 0.0, 0.0]])       # reference j goes with estimate p[j]
        assert bp(M) == [2, 0, 1]
        assert bp(np.array([[np.nan, 3.0], [3.0, 1.0]])) == [1, 0]             # a non-finite term makes the identity lose
        assert bp(np.array([[np.inf, 0.0], [0.0, 2.0]])) == [1, 0]             # +inf is not finite either
        assert bp(np.array([[np.inf, np.nan], [0.0, 2.0]])) == [0, 1]          # both lose: the first
        assert bp(np.array([[7.0]])) == [0]


def test_abi_480_validation_without_a_device():
    from misonet_amd import _lib
    lib, EINVAL, ENOMEM = _lib.lib(), _lib.EINVAL, _lib.ENOMEM
    assert lib.misonet_version() >= 480
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def wave(est=p, ref=p, B=2, E=2, R=2, n=1000, stats=p, scratch=p, nbytes=1 << 20, es=(2000, 1000, 1), rs=(2000, 1000, 1)):
        return lib.misonet_score_wave(est, 1, es[0], es[1], es[2], ref, rs[0], rs[1], rs[2], B, E, R, n, None, stats,
                                      scratch, nbytes, None)

    def spec(est=p, ref=p, B=2, E=2, R=2, T=10, F=129, pair=p, perm=None, scratch=p, nbytes=1 << 20, es=(2580, 1290, 129)):
        return lib.misonet_score_spec(est, es[0], es[1], es[2], ref, 2580, 1290, 129, B, E, R, T, F, pair, perm, None,
                                      scratch, nbytes, None)

    for kw in (dict(est=None), dict(ref=None), dict(stats=None), dict(scratch=None)):
        assert wave(**kw) == EINVAL and b"null" in lib.misonet_last_error()
    for kw in (dict(E=0), dict(E=6), dict(R=0), dict(R=5), dict(B=0), dict(n=0), dict(n=-5), dict(es=(2000, 1000, 0)),
               dict(rs=(-1, 1000, 1))):
        assert wave(**kw) == EINVAL and lib.misonet_last_error() != b"", kw
    assert wave(nbytes=8) == ENOMEM and b"scratch" in lib.misonet_last_error()
    assert wave(nbytes=lib.misonet_score_scratch_bytes(2, 2, 2, 1000) - 1) == ENOMEM
    for kw in (dict(est=None), dict(ref=None), dict(pair=None), dict(scratch=None)):
        assert spec(**kw) == EINVAL and b"null" in lib.misonet_last_error()
    for kw in (dict(E=0), dict(E=6), dict(R=0), dict(R=5), dict(B=0), dict(T=0), dict(F=0), dict(F=1025),
               dict(E=3, perm=p), dict(es=(2580, 1290, 0))):
        assert spec(**kw) == EINVAL and lib.misonet_last_error() != b"", kw
    assert spec(nbytes=8) == ENOMEM and b"scratch" in lib.misonet_last_error()
    assert spec(nbytes=2 * 129 * 4 * 8 - 1) == ENOMEM


def test_scratch_bytes_formula_and_monotone():
    from misonet_amd import _lib, score
    f = _lib.lib().misonet_score_scratch_bytes

    def want(B, E, R, x):
        return 8 * B * max(-(-x // 4096) * (2 * E + 2 * R + E * R), min(x, 1024) * E * R)

    xs = [1, 64, 129, 1024, 1025, 4095, 4096, 4097, 64000, 191936, 1 << 24]
    for B, E, R, x in itertools.product([1, 3, 16], [1, 3, 5], [1, 2, 4], xs):
        assert f(B, E, R, x) == want(B, E, R, x) == score.scratch_bytes(B, E, R, x)
    for E, R in itertools.product(range(1, 6), range(1, 5)):
        prev = 0
        for x in range(1, 20000, 7):
            cur = f(4, E, R, x)
            assert cur >= prev
            prev = cur
        for x in xs:
            assert f(5, E, R, x) >= f(4, E, R, x)
            if E < 5:
                assert f(4, E + 1, R, x) >= f(4, E, R, x)
            if R < 4:
                assert f(4, E, R + 1, x) >= f(4, E, R, x)
    assert f(0, 1, 1, 10) == -1 and f(1, 0, 1, 10) == -1 and f(1, 1, 0, 10) == -1 and f(1, 1, 1, 0) == -1
    # both entry points fit into what the function answers for their own argument
    assert f(16, 3, 2, 64000) >= 8 * 16 * 16 * (6 + 4 + 6) and f(16, 2, 2, 129) >= 8 * 16 * 129 * 4


def test_recording_score_needs_clean_input():
    """score=True without clean references is refused before anything touches a device"""
    from misonet_amd.pipeline import Enhancer
    enh = Enhancer.__new__(Enhancer)
    with pytest.raises(ValueError, match="clean"):
        Enhancer.enhance_recording(enh, np.zeros((1000, 6), np.float32), None, score=True)
