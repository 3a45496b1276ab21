"""CPU checks of the streaming polyphase resampler: the library's count functions equal the restatement's formulas
(tests/rstream_ref.py), the counts of any cutting add up to the offline length, the restatement's streamed output equals
``resample_ref.restate`` of the whole signal EXACTLY in float64 for any cut, the planted mistakes are rejected by that equality,
and the host side of the C ABI (version, prototypes, refusals) behaves.  No kernel is launched here.

Two of the planted faults show only where the definition lets them.  Where p divides 2 Lh (every p <= q with p = 1, every p > q)
the sample C back only ever meets the LAST tap, g[2 Lh], the sinc's zero crossing times the window (1e-18): a carry one sample
short changes a float64 sum there only by luck, so that fault is planted at 160 / 441 and 147 / 160, where the oldest sample meets
taps that count.  The e(N) one short where N p - 1 - Lh = 0 (mod q) is planted where a call starts and not where the call
before it ended -- two places in such code: the output at that boundary then comes twice."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resample_ref as R
import rstream_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = {"1/1024": (1024, 1), "1024/1": (1, 1024)}


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ---- the count functions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RATIOS) + list(EXTRA))
def test_library_counts_equal_the_restatement(name):
    lib = _lib().lib()
    fi, fo = {**R.RATIOS, **EXTRA}[name]
    p, q = R.pq(fi, fo)
    Cc = S.carry(p, q)
    assert lib.misonet_resample_stream_carry(fi, fo) == Cc
    assert lib.misonet_resample_stream_state_bytes(3, 5, fi, fo) == 3 * 5 * Cc * 4
    news = sorted({0, 1, max(q - 1, 0), q, q + 1, Cc, Cc + 1})
    for seen in list(range(0, 3 * (Cc + q) + 1)) + [(1 << 33) + 1, (1 << 33) + q, (1 << 40) + 12345]:
        for new in news:
            for flush in (0, 1):
                assert lib.misonet_resample_stream_outputs(int(seen), new, flush, fi, fo) == S.outputs(int(seen), new, flush, p, q), \
                    (seen, new, flush)


def test_the_carry_of_the_ratios_named_in_the_header():
    got = {k: S.carry(*R.pq(*v)) for k, v in {**R.RATIOS, **EXTRA}.items()}
    assert (got["1/3"], got["3/1"], got["160/441"], got["441/160"], got["1/1024"], got["1/1"]) == (60, 20, 55, 20, 20480, 0)
    assert S.latency(1, 3) == 30.0


@pytest.mark.parametrize("name", list(R.RATIOS))
def test_the_carry_is_enough_and_no_larger_than_needed(name):
    """for every N the next output's first input lies at most C back, and for some N exactly C back"""
    p, q = R.pq(*R.RATIOS[name])
    Lh, Cc = R.half_len(p, q), S.carry(p, q)
    need = 0
    for N in range(0, 4 * (Cc + q) + p):
        m = S.emitted(N, p, q)
        need = max(need, N - max(0, -((Lh - m * q) // p)))
    assert need == Cc


@pytest.mark.parametrize("name", list(R.RATIOS))
def test_counts_of_any_cutting_add_up_to_the_offline_length(name):
    p, q = R.pq(*R.RATIOS[name])
    Cc = S.carry(p, q)
    rng = np.random.default_rng(5)
    for n in (1, 2, q, Cc, Cc + 1, 3 * (Cc + q) + 7):
        for pieces in ([n], [1], [q], [max(Cc, 1)], rng.choice([1, max(q - 1, 1), q, q + 1, max(Cc, 1), Cc + 1], 50).tolist()):
            for with_block in (True, False):
                blocks, N, tot = S.cut(n, pieces), 0, 0
                for k, b in enumerate(blocks):
                    tot += S.outputs(N, b, int(with_block and k == len(blocks) - 1), p, q)
                    N += b
                if not with_block:
                    tot += S.outputs(N, 0, 1, p, q)
                assert tot == R.out_len(n, p, q), (n, pieces, with_block)
    assert S.outputs(0, 0, 1, p, q) == 0                            # flushing a stream that has seen nothing


# ---- the streamed restatement against the offline one -------------------------------------------------------------------------
def _cuttings(n, q, Cc, seed):
    rng = np.random.default_rng(seed)
    around = [1, max(q - 1, 1), q, q + 1, max(Cc - 1, 1), max(Cc, 1), Cc + 1]
    return [[n], [1], [q], [max(Cc, 1)], rng.choice(around, 64).tolist(), rng.choice(around, 64).tolist()]


@pytest.mark.parametrize("name", list(R.RATIOS))
def test_streamed_restatement_equals_offline_exactly(name):
    p, q = R.pq(*R.RATIOS[name])
    Cc = S.carry(p, q)
    g = R.firwin_taps(p, q)
    for n in (1, 2, Cc + q + 3, 2 * (Cc + q) + 7):
        x = np.random.default_rng(n + p).standard_normal((n, 2))
        ref = R.restate(x, p, q, g)
        for pieces in _cuttings(n, q, Cc, n):
            if pieces == [1] and n > 600:                            # run time: single samples up to C + q + 3 of every ratio
                continue                                             # (554 at 80 / 441), not at 2 (C + q) + 7 of the 441s
            for with_block in (True, False):
                assert _same(S.stream(x, p, q, pieces, g, flush_with_block=with_block), ref), (n, pieces, with_block)
    xi = np.rint(np.random.default_rng(3).standard_normal((Cc + q + 3, 2)) * 3000.0)
    ref = R.restate(xi, p, q, g) * (1.0 / 32767.0)
    assert _same(S.stream(xi, p, q, [q + 1], g, in_i16=True), ref)


# a short carry shows where p does not divide 2 Lh (module text)
PLANTED = [(n, f) for n in ("1/2", "1/3", "160/441", "147/160") for f in S.FAULTS
           if f != "carry_short" or n in ("160/441", "147/160")]


@pytest.mark.parametrize("name,fault", PLANTED)
def test_planted_faults_are_rejected(name, fault):
    p, q = R.pq(*R.RATIOS[name])
    Cc = S.carry(p, q)
    g = R.firwin_taps(p, q)
    n = 2 * (Cc + q) + 7 if q < 100 else Cc + q + 40
    i16 = fault == "i16_scale_per_term"
    x = np.rint(np.random.default_rng(11).standard_normal((n, 2)) * 3000.0) if i16 else \
        np.random.default_rng(11).standard_normal((n, 2))
    ref = R.restate(x, p, q, g) * (1.0 / 32767.0) if i16 else R.restate(x, p, q, g)
    assert _same(S.stream(x, p, q, [1], g, in_i16=i16), ref)
    assert not _same(S.stream(x, p, q, [1], g, fault=fault, in_i16=i16), ref)


def test_the_rotation_of_the_gpu_test_meets_every_length_with_every_cutting():
    """tests/test_gpu_resample_stream.py does not run lengths x cuttings x layouts in full: layout li and length ni take the
    cuttings li + 3 ni + {0, 5, 10} (mod 16).  The arithmetic: the 20 layouts bring all 16 cuttings to every length."""
    import itertools
    for ni in range(12):
        assert {(li + 3 * ni + 5 * k) % 16 for li in range(20) for k in range(3)} == set(range(16))
    assert len(list(itertools.product(R.CHANNELS, (1, 3), (False, True)))) == 20
    assert all(len(R.lengths(*R.pq(*v), 32)) <= 12 for v in R.RATIOS.values())


# ---- the C ABI, host side --------------------------------------------------------------------------------------------------
NEW = {"misonet_resample_stream_carry", "misonet_resample_stream_state_bytes", "misonet_resample_stream_outputs",
       "misonet_resample_stream_tile", "misonet_resample_stream_reset", "misonet_resample_stream"}


def test_abi_660():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 660
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name), name
    assert 1 <= lib.misonet_resample_stream_tile() <= lib.misonet_resample_tile()
    assert lib.misonet_resample_stream_state_bytes(3, 6, 48000, 16000) == 3 * 6 * 60 * 4
    assert lib.misonet_resample_stream_state_bytes(1, 16, 16000, 16000) == 0


def _call(lib, **kw):
    a = dict(src=None, si=0, ssb=0, ssc=1, sst=2, B=1, M=2, new=64, seen=0, flush=0, fi=48000, fo=16000, dst=None, di=0, dsb=0,
             dsc=1, dst_st=2, state=None, nb=1 << 40)
    a.update(kw)
    return lib.misonet_resample_stream(a["src"], a["si"], a["ssb"], a["ssc"], a["sst"], a["B"], a["M"], a["new"], a["seen"],
                                       a["flush"], a["fi"], a["fo"], a["dst"], a["di"], a["dsb"], a["dsc"], a["dst_st"],
                                       a["state"], a["nb"], None)


BAD_RATES = [(0, 16000), (16000, 0), (-1, 16000), (1025, 1), (1, 1025), (44101, 16000), (1 << 31, 16000)]


def test_every_refusal_comes_before_any_pointer_is_looked_at():
    L = _lib()
    lib = L.lib()
    for fi, fo in BAD_RATES:
        assert lib.misonet_resample_stream_carry(fi, fo) == -1, (fi, fo)
        assert lib.misonet_resample_stream_state_bytes(1, 2, fi, fo) == -1, (fi, fo)
        assert lib.misonet_resample_stream_outputs(0, 64, 0, fi, fo) == -1, (fi, fo)
        assert lib.misonet_resample_stream_reset(None, 1, 2, fi, fo, None) == L.EINVAL, (fi, fo)
        assert _call(lib, fi=fi, fo=fo) == L.EINVAL and lib.misonet_last_error(), (fi, fo)
    for B, M in [(0, 2), (-1, 2), (65536, 2), (1, 0), (1, -1), (1, 17)]:
        assert lib.misonet_resample_stream_state_bytes(B, M, 48000, 16000) == -1, (B, M)
        assert lib.misonet_resample_stream_reset(None, B, M, 48000, 16000, None) == L.EINVAL, (B, M)
        assert _call(lib, B=B, M=M) == L.EINVAL and lib.misonet_last_error(), (B, M)
    for seen, new, flush in [(-1, 64, 0), (-1, 64, 1), (0, 0, 0), (100, 0, 0), (0, -1, 0), (0, -1, 1), (0, (1 << 28) + 1, 0),
                             (0, (1 << 28) + 1, 1), ((1 << 50) + 1, 64, 0)]:
        assert lib.misonet_resample_stream_outputs(seen, new, flush, 48000, 16000) == -1, (seen, new, flush)
        assert _call(lib, seen=seen, new=new, flush=flush) == L.EINVAL and lib.misonet_last_error(), (seen, new, flush)
    for kw in (dict(si=2), dict(di=-1), dict(ssb=-1), dict(ssc=-1), dict(sst=0), dict(sst=-2), dict(dst_st=0), dict(dsc=-1),
               dict(dsc=0), dict(dsb=-1), dict(B=2, dsb=0)):
        assert _call(lib, **kw) == L.EINVAL and lib.misonet_last_error(), kw
    # legal arguments, null pointers: still refused, nothing launched
    assert _call(lib) == L.EINVAL
    assert lib.misonet_resample_stream_reset(None, 1, 2, 48000, 16000, None) == L.EINVAL
    # a short state is ENOMEM (addresses only: nothing is launched)
    a, b, s = C.c_void_p(1 << 30), C.c_void_p(2 << 30), C.c_void_p(3 << 30)
    nb = lib.misonet_resample_stream_state_bytes(1, 2, 48000, 16000)
    assert _call(lib, src=a, dst=b, state=s, nb=nb - 1) == L.ENOMEM
    # a call that emits nothing needs no output: the pointer check passes, the state's size is looked at next
    assert lib.misonet_resample_stream_outputs(0, 20, 0, 48000, 16000) == 0
    assert _call(lib, src=a, new=20, state=s, nb=0) == L.ENOMEM
