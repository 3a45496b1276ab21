"""BSS-eval on the CPU: the two NumPy / SciPy forms of tests/bss_ref.py against each other (the explicit mir_eval form is the
oracle of tests/test_gpu_bss.py), the host function ``score.bss_from_energies`` against the restated rules, and the host
side of the C ABI (version 490, the size function and its limits).  No device is needed.

The solver on its own input (``bss_ref.SOLVE_SHAPES``: every panel width, the short systems that end early, R = 4, Q = 1024):
the two forms on those inputs, the reference by Cholesky against the one by LU within ``bss_ref.solve_bound``, and
``bss_ref.blocked`` -- the panel scheme of the device restated in NumPy -- within the same bound when it is clean and outside
it by a factor of 100 or more with every planted fault.  The full-size case (N = 4096) runs through all of it but the planted
faults: Q = 1024 is whole panels, the one fault it reaches is reached at (2, 2, 1024) already."""
import functools
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


@functools.lru_cache(maxsize=None)
def _solve_ref(kind, R, E, Q, L):
    """one SOLVE_SHAPES case: the signals, their float64 correlations and the Cholesky reference, computed once"""
    est, refs = bss_ref.long_case(kind, R, E, Q, L)
    Rrr, Rre, Eee = bss_ref.correlations(est, refs, Q)
    T, A, info, cond = bss_ref.solve_energies(Rrr, Rre)
    for x in (est, refs, Rrr, Rre, Eee, T, A):
        x.setflags(write=False)
    return dict(est=est, refs=refs, Rrr=Rrr, Rre=Rre, Eee=Eee, T=T, A=A, info=info, cond=cond)


def _miss(T, A, c, R, Q):
    """the largest error / solve_bound over T and A against the reference of case c"""
    bT = np.array([bss_ref.solve_bound(Q, k) for k in c["cond"][1:]])
    return max(float(np.max(np.abs(A - c["A"]) / (np.abs(c["A"]) * bss_ref.solve_bound(R * Q, c["cond"][0])))),
               float(np.max(np.abs(T - c["T"]) / (np.abs(c["T"]) * bT))))


_CASES = bss_ref.solve_cases()
_ids = lambda c: "-".join(str(v) for v in c)     # noqa: E731


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_the_two_forms_agree_on_the_solver_inputs(case):
    kind, R, E, Q, L = case
    c = _solve_ref(*case)
    sdr, sir, sar = bss_ref.explicit(c["est"], c["refs"], Q)
    T, A, Eee, valid, info = bss_ref.energies(c["est"], c["refs"], Q)
    assert info == -1 and valid.all()
    assert np.array_equal(T, c["T"]) and np.array_equal(A, c["A"])          # solve_energies is the same form
    d = max(np.abs(10 * np.log10(T / (Eee[:, None] - T)) - sdr).max(), np.abs(10 * np.log10(A / (Eee - A)) - sar).max())
    if R > 1:
        d = max(d, np.abs(10 * np.log10(T / (A[:, None] - T)) - sir).max())
    print(f"[bss] solver input {case}: cond {c['cond'][0]:.2e}; forms differ by {d:.2e} dB")
    assert d <= FORMS_TOL, (case, d)


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_the_reference_stays_inside_the_bound(case):
    kind, R, E, Q, L = case
    c = _solve_ref(*case)
    assert c["info"] == -1 and np.isfinite(c["cond"]).all()
    T, A, info, _ = bss_ref.solve_energies(c["Rrr"], c["Rre"], solver="lu", cond=False)
    m = _miss(T, A, c, R, Q)
    print(f"[bss] solver input {case}: cond {[f'{k:.2e}' for k in c['cond']]}; LU - Cholesky = {m:.2e} of the bound")
    assert info == -1 and m <= 1.0, (case, m)


_fault_miss = {}


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_the_restatement_is_clean_and_every_fault_is_caught(case):
    kind, R, E, Q, L = case
    c = _solve_ref(*case)
    T, A, info = bss_ref.blocked(c["Rrr"], c["Rre"])
    m = _miss(T, A, c, R, Q)
    print(f"[bss] solver input {case}: blocked - reference = {m:.2e} of the bound")
    assert info == -1 and m <= 1.0, (case, m)
    for fault in bss_ref.FAULTS if case[1:] != bss_ref.FULL_SIZE else ():
        hit = []
        T, A, info = bss_ref.blocked(c["Rrr"], c["Rre"], fault=fault, hit=hit)
        if not hit:
            continue                                                # the shape does not reach the place
        f = np.inf if info != -1 else _miss(T, A, c, R, Q)
        print(f"[bss] solver input {case}: fault {fault}: info {info}, {f:.2e} of the bound")
        _fault_miss[fault] = min(_fault_miss.get(fault, np.inf), f)
        assert f >= 100.0, (case, fault, f)


def test_every_fault_is_reached_by_a_shape():
    """a fault no shape exposes is a gap in SOLVE_SHAPES (the shapes up to N = 320 reach all five); after the table above
    this prints the smallest miss factor per fault over all shapes"""
    reached = set()
    for case in _CASES:
        kind, R, E, Q, L = case
        if kind == "white" and R * Q <= 320:
            c = _solve_ref(*case)
            for fault in bss_ref.FAULTS:
                hit = []
                bss_ref.blocked(c["Rrr"], c["Rre"], fault=fault, hit=hit)
                reached.update(hit)
    assert sorted(reached) == sorted(bss_ref.FAULTS)
    for fault, f in sorted(_fault_miss.items()):
        print(f"[bss] fault {fault}: smallest miss over the shapes {f:.2e} of the bound")


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


def test_the_pivot_rule_inside_a_narrow_panel():
    """three references, the third a copy of the first, Q = 16: the only panel is 48 wide and fails at row 32; two identical
    references at Q = 48 and 80 fail at row Q, in panel 0 (row 48 of 64) and in column 16 of panel 1.  The restatement of
    the device's scheme reports the same rows."""
    est, refs = bss_ref.long_case("ar2", 3, 3, 16, 2000)
    refs[2] = refs[0]
    T, A, Eee, valid, info = bss_ref.energies(est, refs, 16)
    assert info == 32 and np.isnan(T).all() and np.isnan(A).all() and valid.all()
    Rrr, Rre, _ = bss_ref.correlations(est, refs, 16)
    Tb, Ab, ib = bss_ref.blocked(Rrr, Rre)
    assert ib == 32 and np.isnan(Tb).all() and np.isnan(Ab).all()
    for Q in (48, 80):
        est, refs = bss_ref.long_case("ar2", 2, 2, Q, 4000)
        refs[1] = refs[0]
        assert bss_ref.energies(est, refs, Q)[4] == Q
        Rrr, Rre, _ = bss_ref.correlations(est, refs, Q)
        assert bss_ref.solve_energies(Rrr, Rre, cond=False)[2] == Q and bss_ref.blocked(Rrr, Rre)[2] == Q


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
    for B, E, R, n, Q in itertools.product((1, 16), (1, 2, 4), (1, 2, 4), (1, 5000, 192000, 1 << 24),
                                         (16, 48, 64, 80, 272, 512, 1008, 1024)):
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
