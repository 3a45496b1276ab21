"""BSS-eval on the CPU: the two NumPy / SciPy forms of tests/bss_ref.py against each other (the explicit mir_eval form is the
oracle of tests/test_gpu_bss.py), the host function ``score.bss_from_energies`` against the restated rules, and the host
side of the C ABI (version 490, the size function and its limits).  No device is needed."""
import itertools
import os
import re

import numpy as np
import pytest

import bss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS_TOL = 1e-7      # dB, set by the issue (measured there: <= 3.6e-9)


@pytest.mark.parametrize("S", bss_ref.SPEAKERS)
@pytest.mark.parametrize("kind", bss_ref.KINDS)
def test_the_two_forms_agree(kind, S):
    worst = 0.0
    for L in bss_ref.LENGTHS:
        est, refs = bss_ref.case(kind, S, L)
        for Q in bss_ref.FILT_LENS:
            sdr, sir, sar = bss_ref.explicit(est, refs, Q)
            T, A, Eee, valid, info = bss_ref.energies(est, refs, Q)
            assert info == -1 and valid.all()
            f = bss_ref.figures(T, A, Eee)
            d = max(np.abs(f["sdr_matrix"] - sdr).max(), np.abs(f["sar"] - sar).max())
            if S > 1:
                d = max(d, np.abs(f["sir_matrix"] - sir).max())
            print(f"[bss] {kind} S={S} L={L} Q={Q}: sdr {np.diag(sdr)} sir {np.diag(sir)} sar {sar}; forms differ by {d:.2e} dB")
            assert np.isfinite(sdr).all() and np.isfinite(sar).all()
            assert d <= FORMS_TOL, (kind, S, L, Q, d)
            worst = max(worst, d)
    print(f"[bss] {kind} S={S}: largest gap between the forms {worst:.2e} dB")


def _same(ev, want):
    for key in ("sdr", "sir", "sar", "sdr_best", "sir_best", "sar_best", "sdr_mix", "sdri"):
        got, ref = getattr(ev, key), want[key]
        if ref is None:
            assert got is None, key
        else:
            assert np.array_equal(np.asarray(got), np.asarray(ref), equal_nan=True), (key, got, ref)
    assert ev.perm_best == want["perm_best"] and list(ev.valid) == list(want["valid"]) and ev.ok == want["ok"]


def test_from_energies_equals_the_restatement():
    from misonet_amd import score
    rng = np.random.default_rng(3)
    for S in (1, 2, 3, 4):
        for trial in range(20):
            Eee = rng.uniform(1.0, 2.0, S)
            A = Eee * rng.uniform(0.5, 0.999, S)
            T = A[:, None] * rng.dirichlet(np.ones(S), S) * rng.uniform(0.8, 1.0, (S, 1))
            tm, em = rng.uniform(0.1, 0.5, S), 1.0
            valid = rng.uniform(size=S) > 0.25 if trial % 3 == 0 else None
            ok = trial % 7 != 6
            with_mix = trial % 2 == 0
            ev = score.bss_from_energies(T, A, Eee, valid=valid, ok=ok, T_mix=tm if with_mix else None,
                                         Eee_mix=em if with_mix else None, filt_len=64, n_samples=100)
            _same(ev, bss_ref.figures(T, A, Eee, valid, ok, tm if with_mix else None, em if with_mix else None))
            assert ev.filt_len == 64 and ev.n_samples == 100
            d = ev.as_dict()
            assert sorted(d) == sorted(["sdr", "sir", "sar", "valid", "ok", "perm_best", "sdr_best", "sir_best", "sar_best",
                                        "sdr_mix", "sdri", "filt_len", "n_samples"])


def test_from_energies_rules():
    from misonet_amd import score
    # swapped estimates: the permutation with the largest summed SIR
    T = np.array([[0.01, 0.9], [0.8, 0.02]])
    ev = score.bss_from_energies(T, [0.95, 0.85], [1.0, 1.0])
    assert ev.perm_best == [1, 0]
    assert ev.sdr_best[0] == 10 * np.log10(0.8 / (1.0 - 0.8)) and ev.sar_best[1] == 10 * np.log10(0.95 / (1.0 - 0.95))
    # ties: the first of the optima in itertools order
    ev = score.bss_from_energies(np.full((3, 3), 0.2), np.full(3, 0.7), np.ones(3))
    assert ev.perm_best == [0, 1, 2]
    # a silent reference: its SDR and SIR are NaN, every permutation loses, the identity is reported
    ev = score.bss_from_energies(T, [0.95, 0.85], [1.0, 1.0], valid=[True, False])
    assert np.isnan(ev.sdr[1]) and np.isnan(ev.sir[1]) and np.isfinite(ev.sdr[0]) and np.isfinite(ev.sar).all()
    assert ev.perm_best == [0, 1] and list(ev.valid) == [True, False]
    # a failed factorisation: everything NaN
    ev = score.bss_from_energies(T, [0.95, 0.85], [1.0, 1.0], ok=False, T_mix=[0.3, 0.3], Eee_mix=1.0)
    assert not ev.ok and all(np.isnan(getattr(ev, k)).all() for k in ("sdr", "sir", "sar", "sdr_best", "sdr_mix", "sdri"))
    # denominators are max(., 0): a projection that holds all the energy gives +inf, not NaN
    ev = score.bss_from_energies([[1.0]], [1.0], [1.0 - 1e-17])
    assert ev.sdr[0] == np.inf and ev.sar[0] == np.inf
    with pytest.raises(ValueError):
        score.bss_from_energies(np.ones((2, 3)), [1, 1], [1, 1])
    with pytest.raises(ValueError):
        score.bss_from_energies(T, [1.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        score.bss_from_energies(T, [1.0, 1.0], [1.0, 1.0], T_mix=[0.1, 0.1])


def test_identical_references_trip_the_pivot_rule_at_row_q():
    """two identical references: G = [[T, T], [T, T]], the Schur complement vanishes at row Q (NumPy's Cholesky raises)"""
    est, refs = bss_ref.case("ar2", 2, 5000)
    refs[1] = refs[0]
    Q = 64
    T, A, Eee, valid, info = bss_ref.energies(est, refs, Q)
    assert info == Q and np.isnan(T).all() and np.isnan(A).all() and valid.all()
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(bss_ref.gram(bss_ref.correlations(est, refs, Q)[0]))


def test_silent_reference_leaves_the_span():
    est, refs = bss_ref.case("white", 3, 5000)
    refs[1] = 0
    Q = 64
    T, A, Eee, valid, info = bss_ref.energies(est, refs, Q)
    assert info == -1 and list(valid) == [True, False, True]
    f = bss_ref.figures(T, A, Eee, valid)
    sdr, sir, sar = bss_ref.explicit(est, refs[[0, 2]], Q)
    assert np.abs(f["sdr_matrix"][:, [0, 2]] - sdr).max() <= FORMS_TOL and np.abs(f["sar"] - sar).max() <= FORMS_TOL
    assert np.abs(f["sir_matrix"][:, [0, 2]] - sir).max() <= FORMS_TOL and np.isnan(f["sdr_matrix"][:, 1]).all()


def test_abi_490_header_exports_and_signatures():
    from misonet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    new = {"misonet_bss_scratch_bytes", "misonet_bss_corr", "misonet_bss_solve"}
    assert new <= declared and declared == set(_lib.SIGNATURES)
    lib = _lib.lib()
    assert lib.misonet_version() >= 490
    for name in new:
        assert hasattr(lib, name)


def test_scratch_bytes_value_and_limits():
    from misonet_amd import score
    for B, E, R, n, Q in itertools.product((1, 16), (1, 2, 4), (1, 2, 4), (1, 5000, 192000, 1 << 24), (16, 64, 512, 1024)):
        corr = -(-(n + 15) // 4096) * (R * R + R * E + E) * Q
        systems = (R * Q + 4) * R * Q + R * (Q + 4) * Q
        assert score.bss_scratch_bytes(B, E, R, n, Q) == 8 * B * max(corr, systems), (B, E, R, n, Q)
    good = dict(B=1, E=2, R=2, n=1000, Q=512)
    for key, bad in (("B", (0, -1, 4097)), ("E", (0, 5)), ("R", (0, 5)), ("n", (0, -3, (1 << 24) + 1)),
                     ("Q", (0, 8, 24, 500, 1040, 2048))):
        for v in bad:
            a = dict(good, **{key: v})
            assert score.bss_scratch_bytes(a["B"], a["E"], a["R"], a["n"], a["Q"]) < 0, (key, v)


def test_entry_points_reject_bad_limits_without_a_device():
    """the range checks come before any launch: MISONET_EINVAL with a message"""
    import ctypes as C
    from misonet_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(256)             # never dereferenced: the checks fail first
    for E, R, n, Q in ((5, 2, 100, 512), (2, 5, 100, 512), (2, 2, (1 << 24) + 1, 512), (2, 2, 100, 500), (2, 2, 100, 2048)):
        rc = lib.misonet_bss_corr(p, 1, n * E, n, 1, p, n * R, n, 1, 1, E, R, n, None, Q, p, p, p, p, 1 << 40, None)
        assert rc == _lib.EINVAL and lib.misonet_last_error(), (E, R, n, Q)
    for E, R, Q in ((0, 2, 512), (2, 0, 512), (2, 2, 8), (2, 2, 1000)):
        assert lib.misonet_bss_solve(p, p, p, 1, E, R, Q, p, p, p, p, 1 << 40, None) == _lib.EINVAL
    assert lib.misonet_bss_solve(p, p, p, 1, 2, 2, 512, p, p, p, p, 1000, None) == _lib.ENOMEM
    assert lib.misonet_bss_solve(None, p, p, 1, 2, 2, 512, p, p, p, p, 1 << 40, None) == _lib.EINVAL
