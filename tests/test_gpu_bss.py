"""GPU tests of BSS-eval SDR / SIR / SAR (csrc/bss.hip, misonet_amd/score.py): the lagged correlations against float64 NumPy
within the bound of their summation order, the dB figures against the explicit mir_eval form of tests/bss_ref.py on every
test input, bit-reproducibility and independence of the batch, the silent-reference and failed-pivot rules, the best
permutation, and the recording paths with ``bss=True``.

Measured on one MI355X: correlations within 2.7e-3 of their bound; largest deviation from the oracle over all 72 inputs
6.3e-8 dB (quarter-band sources; 3.9e-11 dB on white and AR(2) ones) against the ceiling of 1e-6 dB.  The
module prints both (``[bss] correlations ...``, ``[bss] all inputs ...``).

The solver on its own input (``bss_ref.SOLVE_SHAPES``, 21 inputs: every panel width from 16 to 64, order-Q systems that end
narrow while system 0 goes on, R = 4, E != R, Q = 1024, N = 4096; estimates whose filters span all Q lags): T and A against
``bss_ref.solve_energies`` on the device's own correlations within ``bss_ref.solve_bound`` = 4 N u cond, relative.  Measured
on one MI355X: largest error / bound 1.7e-2 (white, R = 3, E = 2, Q = 16), 3.4e-4 at N = 4096; largest deviation of the figures
from the explicit oracle on those inputs 1.1e-12 dB (``[bss] solver ...``).  Correlations at Q = 16 ... 1008 and
n = 15 ... 9000 within 4.7e-3 of their bound.  The same bits from a scratch of all ones and of all zero."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import bss_ref
from test_gpu_parity import nets, _need_gpu      # noqa: F401

pytestmark = pytest.mark.gpu

CORR_TOL = 1e-12      # x sum_t |x[t]| |y[t + a]|: <= 4143 sequential float64 additions of exact products (2^-53 each)
DB_CEIL = 1e-6        # dB against the explicit oracle, set by the issue: ~300 x the CPU gap of the two forms at cond(G) 1e10


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check_corr(got, est, refs, nv, Q, tag):
    """got = (Rrr, Rre, Eee) host arrays of one item against float64 NumPy over samples [0, nv)"""
    e, r = bss_ref.as_f64(est)[:, :nv], refs[:, :nv].astype(np.float64)
    R, E = r.shape[0], e.shape[0]
    worst = 0.0
    for j in range(R):
        for k in range(R):
            lim = CORR_TOL * bss_ref.corr_abs(r[j], r[k], Q)
            err = np.abs(got[0][j, k] - bss_ref.corr(r[j], r[k], Q))
            assert np.all(err <= lim), (tag, "Rrr", j, k, float(err.max()), float(lim.min()))
            worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        for i in range(E):
            lim = CORR_TOL * bss_ref.corr_abs(r[j], e[i], Q)
            err = np.abs(got[1][j, i] - bss_ref.corr(r[j], e[i], Q))
            assert np.all(err <= lim), (tag, "Rre", j, i, float(err.max()), float(lim.min()))
            worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
    for i in range(E):
        want = float(np.dot(e[i], e[i]))
        assert abs(got[2][i] - want) <= CORR_TOL * want, (tag, "Eee", i)
    return worst


@pytest.mark.parametrize("i16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("Q", [64, 512, 1024])
def test_correlations_against_numpy(Q, i16):
    """float32 and int16 estimates, contiguous and time-major views, B = 3 with different n_valid, lengths that are no
    multiple of 4096 and one shorter than Q"""
    _corr_sweep(Q, i16, ((300, 2, 2), (4096, 1, 1), (5000, 4, 4), (20001, 2, 3), (70000, 1, 2)))


@pytest.mark.parametrize("i16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("Q", [16, 48, 240, 256, 272, 768, 1008])
def test_correlations_at_the_other_lag_tilings(Q, i16):
    """a last wave with fewer than 256 lags (16, 48, 240, 272, 1008), exactly one and two waves (256, 272), three waves of
    four (768); n = 15 (one staging round, every lag past n), 4081 / 4082 (the last length of one segment and the first of
    two: row v of A reads x[k - v], so segment 1 starts with x[4081]), 4097 and 9000 (three segments)"""
    _corr_sweep(Q, i16, [(n, E, R) for n in (15, 4081, 4082, 4097, 9000) for E, R in ((1, 1), (2, 3))])


def test_segment_count_steps_at_4082():
    """ceil((n + 15) / 4096) segments.  The size function returns the larger of the correlation partials and the systems, and
    at every admitted shape the systems outweigh two segments, so the step shows where the partials lead: E = 4, R = 1,
    Q = 16 (9 pairs of 16 lags per segment against 640 doubles of systems) from five segments on, at n = 4 * 4096 + 4081
    and + 4082.  At 4081 and 4082 themselves the size is that of the systems."""
    from misonet_amd import score
    per_seg = 8 * (1 + 4 + 4) * 16
    assert score.bss_scratch_bytes(1, 4, 1, 4 * 4096 + 4081, 16) == 5 * per_seg
    assert score.bss_scratch_bytes(1, 4, 1, 4 * 4096 + 4082, 16) == 6 * per_seg
    assert score.bss_scratch_bytes(1, 4, 1, 4081, 16) == score.bss_scratch_bytes(1, 4, 1, 4082, 16) == 8 * 640


def _corr_sweep(Q, i16, shapes):
    _need_gpu()
    from misonet_amd import score
    rng = np.random.default_rng(Q + int(i16))
    worst = 0.0
    for n, E, R in shapes:
        refs = (0.1 * rng.standard_normal((3, R, n))).astype(np.float32)
        est = (0.1 * rng.standard_normal((3, E, n))).astype(np.float32)
        est[:, :min(E, R)] += np.float32(0.5) * refs[:, :min(E, R)]
        if i16:
            est = np.rint(est * 32767.0).clip(-32768, 32767).astype(np.int16)
        nvs = [n, max(1, n - 100), max(1, (2 * n) // 3)]
        nv_dev = torch.tensor(nvs, dtype=torch.int32, device="cuda")
        d_e = _dev(est)
        d_r = _dev(refs.transpose(0, 2, 1)).transpose(1, 2)                 # time-major [B, n, R], read in place
        assert d_r.stride(2) == R or R == 1
        for use_nv in (False, True):
            out = score.bss_corr(d_e, d_r, nv_dev if use_nv else None, Q)
            again = score.bss_corr(d_e, d_r, nv_dev if use_nv else None, Q)
            assert all(torch.equal(a, b) for a, b in zip(out, again))       # two calls: the same bits
            contig = score.bss_corr(d_e, _dev(refs), nv_dev if use_nv else None, Q)
            assert all(torch.equal(a, b) for a, b in zip(out, contig))      # the layout moves no bit
            got = [x.cpu().numpy() for x in out]
            assert got[0].shape == (3, R, R, Q) and got[1].shape == (3, R, E, Q) and got[2].shape == (3, E)
            for b in range(3):
                w = _check_corr([g[b] for g in got], est[b], refs[b], nvs[b] if use_nv else n, Q, (n, E, R, use_nv, b))
                worst = max(worst, w)
    print(f"[bss] correlations Q={Q} {'int16' if i16 else 'float32'}: worst error / bound = {worst:.3e}")


def _device_figures(est, refs, Q):
    from misonet_amd import score
    Rrr, Rre, Eee = score.bss_corr(_dev(est)[None], _dev(refs)[None], None, Q)
    T, A, info = score.bss_solve(Rrr, Rre, Eee)
    assert int(info[0]) == -1
    return bss_ref.figures(T[0].cpu().numpy(), A[0].cpu().numpy(), Eee[0].cpu().numpy())


@functools.lru_cache(maxsize=None)
def _solver_run(case):
    """one SOLVE_SHAPES case through bss_corr and bss_solve, and the float64 reference on the DEVICE's correlations: the
    error of the correlations is not part of what is measured.  Computed once, shared by the tests below."""
    from misonet_amd import score
    kind, R, E, Q, L = case
    est, refs = bss_ref.long_case(kind, R, E, Q, L)
    Rrr, Rre, Eee = score.bss_corr(_dev(est)[None], _dev(refs)[None], None, Q)
    T, A, info = score.bss_solve(Rrr, Rre, Eee)
    out = dict(est=est, refs=refs, Rrr=Rrr[0].cpu().numpy(), Rre=Rre[0].cpu().numpy(), Eee=Eee[0].cpu().numpy(),
               T=T[0].cpu().numpy(), A=A[0].cpu().numpy(), info=int(info[0]))
    out["T_ref"], out["A_ref"], out["info_ref"], out["cond"] = bss_ref.solve_energies(out["Rrr"], out["Rre"])
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


_CASES = bss_ref.solve_cases()
_ids = lambda c: "-".join(str(v) for v in c)     # noqa: E731
_ratios, _devs = {}, {}


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_solver_on_its_own_input(case):
    """every T[i, j] and A[i] within ``bss_ref.solve_bound`` (4 N u cond, relative) of the float64 reference on the device's
    own correlations, at every panel width the solver admits (bss_ref.SOLVE_SHAPES)"""
    _need_gpu()
    kind, R, E, Q, L = case
    c = _solver_run(case)
    assert c["T"].shape == (E, R) and c["A"].shape == (E,)
    bA = bss_ref.solve_bound(R * Q, c["cond"][0])
    bT = np.array([bss_ref.solve_bound(Q, k) for k in c["cond"][1:]])
    rA = np.abs(c["A"] - c["A_ref"]) / (np.abs(c["A_ref"]) * bA)
    rT = np.abs(c["T"] - c["T_ref"]) / (np.abs(c["T_ref"]) * bT)
    worst = float(max(rA.max(), rT.max()))                           # NaN where the device gave one: fails below
    _ratios[case] = worst
    print(f"[bss] solver {case}: info {c['info']} cond(G) {c['cond'][0]:.2e}; error / bound: A {rA.max():.3e} T {rT.max():.3e}")
    print(f"[bss] solver: worst error / bound so far {max(_ratios.values()):.3e} over {len(_ratios)} of {len(_CASES)} inputs")
    assert c["info"] == -1 and c["info_ref"] == -1
    assert np.all(rA <= 1.0) and np.all(rT <= 1.0), (case, rA, rT)


@pytest.mark.parametrize("case", _CASES, ids=_ids)
def test_solver_inputs_against_the_explicit_oracle(case):
    _need_gpu()
    kind, R, E, Q, L = case
    c = _solver_run(case)
    sdr, sir, sar = bss_ref.explicit(c["est"], c["refs"], Q)
    assert c["info"] == -1
    T, A, Eee = c["T"], c["A"], c["Eee"]
    # bss_ref.figures wants as many estimates as references: the three figures straight from their definitions
    d = max(np.abs(10 * np.log10(T / (Eee[:, None] - T)) - sdr).max(), np.abs(10 * np.log10(A / (Eee - A)) - sar).max())
    if R > 1:
        d = max(d, np.abs(10 * np.log10(T / (A[:, None] - T)) - sir).max())
    _devs[case] = float(d)
    print(f"[bss] solver input {case}: device - oracle {d:.3e} dB")
    print(f"[bss] solver inputs: largest deviation from the oracle so far {max(_devs.values()):.3e} dB (ceiling {DB_CEIL:.0e})")
    assert d <= DB_CEIL, (case, d)


def test_pivot_rule_inside_narrow_panels():
    """the first failing row lies inside a narrow panel: row 32 of the only panel (48 wide) with three references of which
    the third repeats the first at Q = 16; row Q with two identical references at Q = 48 (panel 0, 64 wide in system 0) and
    80 (column 16 of panel 1).  The item beside the failed one keeps the bits it has alone."""
    _need_gpu()
    from misonet_amd import score
    for R, Q, L, row in ((3, 16, 2000, 32), (2, 48, 4000, 48), (2, 80, 4000, 80)):
        est, refs = bss_ref.long_case("ar2", R, R, Q, L)
        refs[R - 1] = refs[0]
        Rrr, Rre, Eee = score.bss_corr(_dev(est)[None], _dev(refs)[None], None, Q)
        T, A, info = score.bss_solve(Rrr, Rre, Eee)
        assert int(info[0]) == row, (R, Q, int(info[0]))
        assert torch.isnan(T).all() and torch.isnan(A).all()
        e2, r2 = bss_ref.long_case("ar2", R, R, Q, L, seed=9)
        both = _block(np.stack([est, e2]), np.stack([refs, r2]), None, None, Q)
        alone = _block(e2[None], r2[None], None, None, Q)[0]
        assert np.array_equal(both[1], alone) and np.isfinite(alone).all() and alone[R * R + 3 * R] == -1.0
        assert both[0][R * R + 3 * R] == float(row) and np.isnan(both[0][:R * R + R]).all()


def test_silent_middle_reference_at_a_narrow_panel():
    """R = 3, Q = 48: N = 144 = two panels and one of 16; the identity block of the silent reference spans the seam of
    panels 0 and 1"""
    _need_gpu()
    from misonet_amd import score
    Q = 48
    est, refs = bss_ref.long_case("white", 3, 3, Q, 4000)
    refs[1] = 0
    Rrr, Rre, Eee = score.bss_corr(_dev(est)[None], _dev(refs)[None], None, Q)
    T, A, info = score.bss_solve(Rrr, Rre, Eee)
    assert int(info[0]) == -1 and torch.equal(T[0, :, 1], torch.zeros(3, dtype=torch.float64, device="cuda"))
    ev = score.bss_eval_waves(est, refs, filt_len=Q)
    assert ev.ok and list(ev.valid) == [True, False, True]
    assert np.isnan(ev.sdr[1]) and np.isnan(ev.sir[1]) and np.isfinite(ev.sar).all()
    sdr, sir, sar = bss_ref.explicit(est, refs[[0, 2]], Q)           # the oracle run without that reference
    for j, c in ((0, 0), (2, 1)):
        assert abs(ev.sdr[j] - sdr[j, c]) <= DB_CEIL and abs(ev.sir[j] - sir[j, c]) <= DB_CEIL
    assert np.abs(ev.sar - sar).max() <= DB_CEIL


@pytest.mark.parametrize("R,E,Q,L", [(2, 2, 48, 4000), (3, 3, 272, 16000)])
def test_result_does_not_depend_on_what_the_scratch_held(R, E, Q, L):
    """bss_assemble_k writes the lower triangle only and bss_update_k reads, adds to and stores the upper half of every
    diagonal tile: a caller-owned scratch of exactly misonet_bss_scratch_bytes bytes, all ones (NaN as float64) and all zero,
    must give the same bits"""
    _need_gpu()
    from misonet_amd import _lib, score
    est, refs = bss_ref.long_case("ar2", R, E, Q, L)
    Rrr, Rre, Eee = score.bss_corr(_dev(est)[None], _dev(refs)[None], None, Q)
    lib = _lib.lib()
    nbytes = int(lib.misonet_bss_scratch_bytes(1, E, R, 1, Q))
    assert nbytes == 8 * ((R * Q + 4) * R * Q + R * (Q + 4) * Q)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    got = []
    for fill in (0xFF, 0x00):
        scratch.fill_(fill)
        T = torch.full((1, E, R), -7.0, dtype=torch.float64, device="cuda")
        A = torch.full((1, E), -7.0, dtype=torch.float64, device="cuda")
        info = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        _lib.check(lib.misonet_bss_solve(Rrr.data_ptr(), Rre.data_ptr(), Eee.data_ptr(), 1, E, R, Q, T.data_ptr(), A.data_ptr(),
                                         info.data_ptr(), scratch.data_ptr(), nbytes, _lib.stream_ptr(scratch.device)))
        torch.cuda.synchronize()
        got.append((T.cpu().numpy(), A.cpu().numpy(), info.cpu().numpy()))
    for a, b in zip(*got):
        assert np.array_equal(a, b) and np.isfinite(a).all()
    assert int(got[0][2][0]) == -1
    T, A, info = score.bss_solve(Rrr, Rre, Eee)                      # and those of the call that allocates its own
    assert np.array_equal(T.cpu().numpy(), got[0][0]) and np.array_equal(A.cpu().numpy(), got[0][1])


_seen = {}


@pytest.mark.parametrize("kind", bss_ref.KINDS)
def test_figures_against_the_explicit_oracle(kind):
    _need_gpu()
    worst = 0.0
    for S in bss_ref.SPEAKERS:
        for L in bss_ref.LENGTHS:
            est, refs = bss_ref.case(kind, S, L)
            for Q in bss_ref.FILT_LENS:
                sdr, sir, sar = bss_ref.explicit(est, refs, Q)
                f = _device_figures(est, refs, Q)
                d = max(np.abs(f["sdr_matrix"] - sdr).max(), np.abs(f["sar"] - sar).max())
                if S > 1:
                    d = max(d, np.abs(f["sir_matrix"] - sir).max())
                print(f"[bss] {kind} S={S} L={L} Q={Q}: sdr {np.diag(sdr)} sar {sar}: device - oracle {d:.3e} dB")
                worst = max(worst, float(d))
                assert d <= DB_CEIL, (kind, S, L, Q, d)
    _seen[kind] = worst
    print(f"[bss] {kind}: largest deviation from the oracle {worst:.3e} dB")
    if len(_seen) == len(bss_ref.KINDS):
        print(f"[bss] all inputs: largest deviation from the oracle {max(_seen.values()):.3e} dB (ceiling {DB_CEIL:.0e})")


def _block(est, refs, mix, nv, Q):
    from misonet_amd import score
    nv_dev = torch.tensor(nv, dtype=torch.int32, device="cuda") if nv is not None else None
    return score.bss_energies(_dev(est), _dev(refs), _dev(mix) if mix is not None else None, nv_dev, Q).cpu().numpy()


@pytest.mark.parametrize("Q", [48, 64, 512])
def test_reproducible_and_independent_of_the_batch(Q):
    _need_gpu()
    lens = (20000, 64000, 33333)
    S = 2
    items = [bss_ref.case("ar2", S, L, seed=5) for L in lens]
    n = max(lens)
    est = np.zeros((3, S, n), np.int16)
    refs = np.zeros((3, S, n), np.float32)
    mix = np.zeros((3, 1, n), np.float32)
    junk = np.random.default_rng(1)
    for b, (e, r) in enumerate(items):
        est[b, :, :lens[b]], refs[b, :, :lens[b]] = e, r
        mix[b, 0, :lens[b]] = r.sum(0)
        est[b, :, lens[b]:] = 77                                    # what lies past n_valid must not matter
        refs[b, :, lens[b]:] = junk.standard_normal((S, n - lens[b]))
        mix[b, 0, lens[b]:] = 1.0
    batch = _block(est, refs, mix, list(lens), Q)
    assert np.array_equal(batch, _block(est, refs, mix, list(lens), Q))
    assert np.isfinite(batch).all()
    for b in range(3):
        alone = _block(items[b][0][None], items[b][1][None], items[b][1].sum(0)[None, None], None, Q)
        assert np.array_equal(alone[0], batch[b]), b
        for pos in range(3):                                        # the same recording as item 0, 1, 2 of another batch
            order = [(b + k - pos) % 3 for k in range(3)]
            moved = _block(est[order], refs[order], mix[order], [lens[o] for o in order], Q)
            assert order[pos] == b and np.array_equal(moved[pos], batch[b]), (b, pos)


def test_eval_waves_and_the_mixture_row():
    _need_gpu()
    from misonet_amd import score
    est, refs = bss_ref.case("ar2", 2, 16000)
    mix = refs.sum(0)
    ev = score.bss_eval_waves(est, refs, mix, filt_len=64)
    again = score.bss_eval_waves(torch.from_numpy(est), torch.from_numpy(refs).cuda(), mix, filt_len=64)
    assert json.dumps(ev.as_dict(), sort_keys=True) == json.dumps(again.as_dict(), sort_keys=True)
    sdr, sir, sar = bss_ref.explicit(est, refs, 64)
    mix_sdr = bss_ref.explicit(mix[None], refs, 64)[0][0]
    assert np.abs(ev.sdr - np.diag(sdr)).max() <= DB_CEIL and np.abs(ev.sir - np.diag(sir)).max() <= DB_CEIL
    assert np.abs(ev.sar - sar).max() <= DB_CEIL and np.abs(ev.sdr_mix - mix_sdr).max() <= DB_CEIL
    assert np.array_equal(ev.sdri, ev.sdr - ev.sdr_mix) and ev.ok and list(ev.valid) == [True, True]
    assert ev.perm_best == [0, 1] and ev.filt_len == 64 and ev.n_samples == 16000
    f32 = score.bss_eval_waves(bss_ref.as_f64(est).astype(np.float32), refs, filt_len=64)
    assert f32.sdr_mix is None and f32.sdri is None and np.abs(f32.sdr - ev.sdr).max() <= 1e-4   # q / 32767 rounded to float32
    with pytest.raises(ValueError):
        score.bss_eval_waves(est, refs[:1])
    with pytest.raises(ValueError):
        score.bss_eval_waves(est, refs, filt_len=100)
    with pytest.raises(ValueError):
        score.bss_eval_waves(est, refs, mix[:-1])


@pytest.mark.parametrize("Q", [64, 512])
def test_silent_reference(Q):
    _need_gpu()
    from misonet_amd import score
    est, refs = bss_ref.case("white", 3, 16000)
    refs[1] = 0
    ev = score.bss_eval_waves(est, refs, filt_len=Q)
    assert ev.ok and list(ev.valid) == [True, False, True]
    assert np.isnan(ev.sdr[1]) and np.isnan(ev.sir[1]) and np.isfinite(ev.sar).all()
    sdr, sir, sar = bss_ref.explicit(est, refs[[0, 2]], Q)           # the oracle run without that reference
    for j, c in ((0, 0), (2, 1)):
        assert abs(ev.sdr[j] - sdr[j, c]) <= DB_CEIL and abs(ev.sir[j] - sir[j, c]) <= DB_CEIL
    assert np.abs(ev.sar - sar).max() <= DB_CEIL


@pytest.mark.parametrize("Q", [64, 512])
def test_identical_references(Q):
    _need_gpu()
    from misonet_amd import score
    est, refs = bss_ref.case("ar2", 2, 16000)
    refs[1] = refs[0]
    Rrr, Rre, Eee = score.bss_corr(_dev(est)[None], _dev(refs)[None], None, Q)
    T, A, info = score.bss_solve(Rrr, Rre, Eee)
    torch.cuda.synchronize()                                        # the call returns
    assert int(info[0]) == Q and torch.isnan(T).all() and torch.isnan(A).all()
    ev = score.bss_eval_waves(est, refs, refs[0], filt_len=Q)
    assert not ev.ok
    for key in ("sdr", "sir", "sar", "sdr_best", "sir_best", "sar_best", "sdr_mix", "sdri"):
        assert np.isnan(getattr(ev, key)).all(), key
    # a healthy item beside it keeps its bits
    e2, r2 = bss_ref.case("ar2", 2, 16000, seed=9)
    both = _block(np.stack([est, e2]), np.stack([refs, r2]), None, None, Q)
    assert np.array_equal(both[1], _block(e2[None], r2[None], None, None, Q)[0]) and np.isfinite(both[1]).all()


def test_swapped_estimates():
    _need_gpu()
    from misonet_amd import score
    est, refs = bss_ref.case("ar2", 2, 16000)
    ev = score.bss_eval_waves(est, refs, filt_len=512)
    sw = score.bss_eval_waves(est[::-1].copy(), refs, filt_len=512)
    assert ev.perm_best == [0, 1] and sw.perm_best == [1, 0]
    assert np.array_equal(sw.sdr_best, ev.sdr) and np.array_equal(sw.sir_best, ev.sir) and np.array_equal(sw.sar_best, ev.sar)
    assert np.all(sw.sdr < ev.sdr - 10.0)


def _same(a, b):
    return json.dumps(a.as_dict(), sort_keys=True) == json.dumps(b.as_dict(), sort_keys=True)      # bit for bit


def test_recording_with_bss(nets):
    import misonet_amd as mz
    from misonet_amd import score
    from misonet_amd.weights import synthetic_utterance
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    L = 100000
    obs, s0, s1 = synthetic_utterance(40, L)
    pcm0, sc0 = enh.enhance_recording(obs, [s0, s1], max_batch=16, score=True)
    pcm, sc, ev = enh.enhance_recording(obs, [s0, s1], max_batch=16, score=True, bss=True)
    assert np.array_equal(pcm, pcm0) and _same(sc, sc0)                                  # bss moves no bit of pcm or Score
    want = score.bss_eval_waves(pcm, np.stack([s0[:, 0], s1[:, 0]]), obs[:, 0])
    assert _same(ev, want) and ev.n_samples == L and ev.filt_len == 512 and ev.ok
    print(f"[bss] recording: sdr {ev.sdr} sir {ev.sir} sar {ev.sar} sdr_mix {ev.sdr_mix}")
    ev64 = enh.enhance_recording(obs, [s0, s1], score=True, bss=True, bss_filt_len=64)[2]
    assert _same(ev64, score.bss_eval_waves(pcm, np.stack([s0[:, 0], s1[:, 0]]), obs[:, 0], filt_len=64))
    others = [synthetic_utterance(41 + i, n) for i, n in enumerate((70000, 64000, 130001))]
    recs = [(o[0], [o[1], o[2]], f"x{i}") for i, o in enumerate(others)]
    recs.insert(2, (obs, [s0, s1], "me"))
    plain = enh.enhance_recordings(recs, max_batch=4, score=True)
    seen = []
    for mb in (4, 16):
        out = enh.enhance_recordings(recs, max_batch=mb, score=True, bss=True)
        assert list(out) == ["x0", "x1", "me", "x2"]
        for name, (o, c, _) in zip(out, recs):
            p, s, e = out[name]
            assert np.array_equal(p, plain[name][0]) and _same(s, plain[name][1])
            assert _same(e, score.bss_eval_waves(p, np.stack([c[0][:, 0], c[1][:, 0]]), o[:, 0])), name
        assert _same(out["me"][2], ev)
        seen.append(out)
    assert all(_same(seen[0][k][2], seen[1][k][2]) for k in seen[0])
    with pytest.raises(ValueError):
        enh.enhance_recording(obs, [s0, s1], bss=True)
    with pytest.raises(ValueError):
        enh.enhance_recordings(recs, bss=True)
    with pytest.raises(ValueError):
        enh.enhance_recording(obs, None, score=True, bss=True)


def test_score_eval_command_line_with_bss(tmp_path):
    _need_gpu()
    import sys
    from misonet_amd import score, stft as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import score_eval
    rng = np.random.default_rng(9)
    est_dir, ref_dir = tmp_path / "est", tmp_path / "ref"
    est_dir.mkdir()
    ref_dir.mkdir()
    want, plain = {}, {}
    f = lambda q: ((q.astype(np.int32) << 8) / float(1 << 23)).astype(np.float32)   # noqa: E731  (what a wav reader returns)
    for name, L in (("u1", 30000), ("u2", 20000)):
        cq = (0.05 * 32767 * rng.standard_normal((2, L, 3))).astype(np.int16)
        eq = (0.6 * cq[:, :, 1] + 0.1 * cq[::-1, :, 1] + 40 * rng.standard_normal((2, L))).astype(np.int16)
        mq = (cq[0] + cq[1]).astype(np.int16)
        for s in range(2):
            S.write_wav_pcm24(str(est_dir / f"{name}_{s}.wav"), eq[s], 16000)
            S.write_wav_pcm24(str(ref_dir / f"{name}_{s}.wav"), cq[s], 16000)
        S.write_wav_pcm24(str(ref_dir / f"{name}.wav"), mq, 16000)
        want[name] = score.bss_eval_waves(eq, f(cq[:, :, 1]), f(mq[:, 1]), filt_len=64).as_dict()
        plain[name] = score.score_waves(eq, f(cq[:, :, 1]), f(mq[:, 1])).as_dict()
    out, out0 = tmp_path / "bss.json", tmp_path / "plain.json"
    score_eval.main([str(est_dir), str(ref_dir), "--ref-ch", "1", "--out", str(out), "--bss", "--filt-len", "64"])
    score_eval.main([str(est_dir), str(ref_dir), "--ref-ch", "1", "--out", str(out0)])
    with open(out) as fh:
        doc = json.load(fh)
    with open(out0) as fh:
        doc0 = json.load(fh)
    assert sorted(doc) == ["mean", "u1", "u2"]
    for name in want:
        assert doc[name]["bss"] == want[name] and doc[name]["bss"]["perm_best"] == [0, 1]
        assert {k: v for k, v in doc[name].items() if k != "bss"} == plain[name] == doc0[name]     # without the flag: unchanged
    assert "bss" not in doc0["mean"] and {k: v for k, v in doc["mean"].items() if k != "bss"} == doc0["mean"]
    vals = [v for n in want for v in want[n]["sdr"]]
    assert abs(doc["mean"]["bss"]["sdr"] - np.mean(vals)) <= 1e-9 and doc["mean"]["bss"]["n_failed"] == 0
