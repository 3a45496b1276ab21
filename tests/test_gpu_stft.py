"""GPU tests of the two kernels that open and close every recording path, ``stft_pack_k`` and ``istft_k`` (csrc/stft.hip, through
``misonet_amd.stft.stft_hip`` / ``istft`` / ``istft_int16`` and the C ABI ``misonet_stft`` / ``misonet_istft``), against the float64
restatement of tests/frontend_ref.py at every tile edge: the first, the last and the frame past each 64-frame tile of the STFT, the
61-hop workgroup seams of the iSTFT, tails of 0, 1 and 63 samples, 1 to 64 microphones, items of different loudness.

Bars.  For every case and every metric (whole tensor, worst frame, worst bin, worst microphone; whole signal, worst output hop, max
|diff| over the peak) the bar is 4 x the float32 statement's value of that metric on that very case -- the same tables, accumulated
in float32 in the kernel's K order; the factor leaves room for the order of additions inside an MFMA and nothing else
(tests/test_frontend.py shows on the CPU what these bars reject).  Exact checks carry no tolerance: an impulse through the forward
product must give the float32 table entry itself, one coefficient through the inverse the table entry over the envelope to 2^-21
(three float32 additions in the envelope, one division, one spare bit).  The int16 output must equal the float64 cast outside the
band |y 32767 - nearest integer| < delta, delta = 4 x the float32 statement's max abs error in LSB, and be within 1 LSB inside it; the
band may hold at most 5 % of the samples and the peak is 0.1 ... 0.5 of full scale (>= 3000 LSB).

Every case prints ``[stft] ...`` / ``[istft] ...`` lines with the device value, the float32 statement's value and their ratio.

Measured (MI355X, first device run of this module, recorded in LAB.md, "Front end on its own input"): device / float32 statement
between 0.93 and 1.18 on every STFT metric of the 23 cases, between 0.84 and 1.32 on every iSTFT metric of the 21 cases and the two
round trips; no int16 sample differs outside the band; single coefficients within 2.25 x 2^-24; 64 tests in 2 s."""
import functools

import numpy as np
import pytest
import torch

import frontend_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _line(tag, case, got, f32, keys):
    return f"[{tag}] {case}: " + "  ".join(f"{k} {got[k]:.3e} / {f32[k]:.3e} = {got[k] / f32[k] if f32[k] else float(got[k] != 0):.2f}"
                                          for k in keys)


# ----------------------------------------------------------------------------------------------------------------------
# STFT against float64
def _L(T, r):
    return 64 * (T - 1) + r


# (kind, B, L, M): T = 1 (L = 1, 63), 2 (L = 64), 3, 63, 64 | 65, 128 | 129, 193 = first, last and one past each 64-frame tile and one in
# the fourth; tails 0, 1, 63 at T = 65 and 129; M = 1 and 64 at T = 65, M = 7 at 129; the three characters at T = 65 and 129
STFT_CASES = ([("white", 3, L, 3) for L in (1, 63, 64, _L(3, 5), _L(63, 9), _L(64, 40), _L(128, 33), _L(193, 20))] +
              [("white", 3, _L(T, r), 3) for T in (65, 129) for r in (0, 1, 63)] +
              [("white", 1, _L(65, 63), 64), ("white", 1, _L(65, 1), 1), ("white", 3, _L(65, 0), 1), ("white", 3, _L(129, 1), 7),
               ("white", 1, _L(129, 63), 7)] +
              [(kind, 3, _L(T, 17), 3) for kind in ("coloured", "silent") for T in (65, 129)])


@functools.lru_cache(maxsize=None)
def _stft_ref(kind, B, L, M):
    """(wav, float64 STFT, metrics of the float32 statement), computed once per case"""
    wav = R.wave(kind, B, L, M, seed=5)
    ref = R.stft64(wav)
    wav.setflags(write=False)
    ref.setflags(write=False)
    return wav, ref, R.stft_metrics(R.stft32(wav), ref)


def _stft_dev(wav):
    from misonet_amd import stft as S
    return S.stft_hip(torch.from_numpy(np.array(wav)).cuda()).cpu().numpy()


@pytest.mark.parametrize("kind,B,L,M", STFT_CASES, ids=lambda v: str(v))
def test_stft_vs_float64(kind, B, L, M):
    _need_gpu()
    wav, ref, m32 = _stft_ref(kind, B, L, M)
    got = _stft_dev(wav)
    T = L // 64 + 1
    assert got.shape == (B, M, T, 129) and got.dtype == np.complex64
    m = R.stft_metrics(got, ref)
    print(_line("stft", f"{kind} B={B} L={L} (T={T}, tail {L - 64 * (T - 1)}) M={M}", m, m32, R.STFT_KEYS))
    assert np.isfinite(got.view(np.float32)).all()
    assert m32["zero_ok"] and m["zero_ok"], "a frame whose float64 reference is exactly 0 is not exactly 0"
    over = R.over_bar(m, m32, R.STFT_KEYS)
    assert all(v <= 1.0 for v in over.values()), (over, m["where"])


# ----------------------------------------------------------------------------------------------------------------------
# exact indexing
def _impulse_case(B, M):
    """impulses of 1.0 at least 320 samples apart per channel: 0, 63, 64, 127, 128, L - 1 and both sides of the first tile's edge
    (frame 64 starts at sample 64 * 64 - 128), spread over items and microphones"""
    L = 64 * 72 + 17
    e = 64 * 64
    groups = [[0, e - 129, L - 1], [63, e - 128], [64, e - 127], [127, e + 127], [128, e + 128], [1000, e - 1], [2000, e]]
    wav = np.zeros((B, L, M), np.float32)
    want = np.zeros((B, M, L // 64 + 1, 129), np.complex64)
    c, s = R.stft_tables()
    assert B * M >= len(groups)
    for g, pos in enumerate(groups):
        b, m = divmod(B * M - 1 if g == len(groups) - 1 else g * (B * M // len(groups)), M)      # one channel each, the last one included
        assert not wav[b, :, m].any() and all(abs(p - q) >= 320 for i, p in enumerate(pos) for q in pos[:i])
        for l in pos:
            wav[b, l, m] = 1.0
            for t in range(L // 64 + 1):
                j = l - 64 * t + 128
                if 0 <= j < 256:
                    want[b, m, t].real = c[j]
                    want[b, m, t].imag = s[j]
    return wav, want


@pytest.mark.parametrize("B,M", [(3, 3), (1, 7), (2, 64)])
def test_stft_impulses_give_the_table_entries(B, M):
    """one product and zeros through the matrix core is exact: every value equals the float32 table entry w[j] cos or -w[j] sin at
    j = l - 64 t + 128, and is 0 in every frame that does not cover the impulse (== : -0 equals 0)"""
    _need_gpu()
    wav, want = _impulse_case(B, M)
    assert (wav != 0).sum() >= 7 * 2
    got = _stft_dev(wav)
    bad = np.argwhere((got.real != want.real) | (got.imag != want.imag))
    assert bad.size == 0, f"{len(bad)} values differ, first (b, m, t, f) = {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


# ----------------------------------------------------------------------------------------------------------------------
# batch, repeat and memory
@pytest.mark.parametrize("T", [65, 129])
def test_stft_repeatable_and_batch_independent(T):
    _need_gpu()
    wav, _, _ = _stft_ref("white", 3, _L(T, 1), 3)
    a, b = _stft_dev(wav), _stft_dev(wav)
    assert np.array_equal(_bits(a), _bits(b))
    one = _stft_dev(wav[1:2])
    assert np.array_equal(_bits(a[1]), _bits(one[0]))


def _abi_stft(wav, ws_fill=0xFF, short=0, M_arg=None):
    from misonet_amd import _lib
    L = _lib.lib()
    x = torch.from_numpy(np.array(wav)).cuda()
    B, n, M = x.shape
    T = L.misonet_stft_frames(n)
    nb = L.misonet_stft_workspace_bytes(B, M, n)
    ws = torch.full((nb,), ws_fill, dtype=torch.uint8, device="cuda")
    out = torch.full((B, M, T, 129, 2), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.misonet_stft(x.data_ptr(), B, n, M if M_arg is None else M_arg, out.data_ptr(), ws.data_ptr(), nb - short,
                        _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().view(np.complex64)[..., 0]


@pytest.mark.parametrize("B,L,M", [(2, _L(65, 1), 3), (1, _L(3, 5), 7), (2, _L(129, 63), 2)])
def test_stft_abi_ignores_previous_memory(B, L, M):
    """Tp > T leaves pad columns in the planar workspace: with the workspace full of 0xFF bytes and the output full of NaN the
    result has the bits of stft_hip's (whose buffers come from the allocator) and is finite"""
    _need_gpu()
    from misonet_amd import _lib
    wav = R.wave("white", B, L, M, seed=6)
    rc, got = _abi_stft(wav)
    assert rc == _lib.OK
    assert np.isfinite(got.view(np.float32)).all()
    assert np.array_equal(_bits(got), _bits(_stft_dev(wav)))
    rc0, got0 = _abi_stft(wav, ws_fill=0)
    assert rc0 == _lib.OK and np.array_equal(_bits(got), _bits(got0))


def test_stft_abi_refuses_bad_arguments():
    _need_gpu()
    from misonet_amd import _lib
    wav = R.wave("white", 1, 300, 3, seed=6)
    assert _abi_stft(wav, short=1)[0] == _lib.ENOMEM
    assert _abi_stft(wav, M_arg=65)[0] == _lib.EINVAL


# ----------------------------------------------------------------------------------------------------------------------
# iSTFT against float64
ISTFT_CASES = ([("white", 3, H + 1) for H in (1, 2, 3, 4, 60, 61, 62, 63, 122, 123, 124, 183, 184)] +
               [("white", 1, H + 1) for H in (1, 61, 62, 123)] +
               [(kind, 3, H + 1) for kind in ("coloured", "silent") for H in (62, 123)])


@functools.lru_cache(maxsize=None)
def _istft_ref(kind, N, T):
    spec = R.spectrogram(kind, N, T, seed=8, amp=0.3)
    ref = R.istft64(spec)
    spec.setflags(write=False)
    ref.setflags(write=False)
    return spec, ref, R.istft_metrics(R.istft32(spec), ref)


def _istft_dev(spec, i16=False):
    from misonet_amd import stft as S
    z = torch.from_numpy(np.array(spec)).cuda()
    return (S.istft_int16(z) if i16 else S.istft(z)).cpu().numpy()


@pytest.mark.parametrize("kind,N,T", ISTFT_CASES, ids=lambda v: str(v))
def test_istft_vs_float64(kind, N, T):
    _need_gpu()
    spec, ref, m32 = _istft_ref(kind, N, T)
    got = _istft_dev(spec)
    assert got.shape == (N, 64 * (T - 1)) and got.dtype == np.float32
    m = R.istft_metrics(got, ref)
    print(_line("istft", f"{kind} N={N} hops={T - 1}", m, m32, R.ISTFT_KEYS))
    assert np.isfinite(got).all()
    assert np.all(got[ref == 0] == 0), "a sample whose float64 reference is exactly 0 is not exactly 0"
    over = R.over_bar(m, m32, R.ISTFT_KEYS)
    assert all(v <= 1.0 for v in over.values()), (over, m["where"])


@functools.lru_cache(maxsize=None)
def _int16_ref(kind, N, T):
    if kind == "near":
        spec = R.spec_of_wave(R.near_integer_wave(N, 64 * (T - 1), peak=0.12))
    else:
        spec = R.scaled_to_peak(R.spectrogram(kind, N, T, amp=1.0) / 3.0 ** np.arange(N)[:, None, None], 0.12)
    y64 = R.istft64(spec)
    y32 = R.istft32(spec)
    delta, band = R.int16_band(y64, y32)
    return spec, y64, y32, delta, band


@pytest.mark.parametrize("kind,N,T", [("white", 3, 124), ("coloured", 3, 124), ("silent", 3, 124), ("near", 2, 124), ("near", 3, 63),
                                      ("white", 1, 63)], ids=lambda v: str(v))
def test_istft_int16_vs_float64_cast(kind, N, T):
    """the truncating cast at a peak of 0.12 of full scale: equal to the float64 cast outside the near-integer band, within 1 LSB
    inside it.  'near' ends in a DC offset of +3 / -3 LSB with 0.4 LSB of noise: truncation toward zero, floor and rounding part
    there, on both sides of zero."""
    _need_gpu()
    spec, y64, y32, delta, band = _int16_ref(kind, N, T)
    peak = np.abs(y64).max()
    q = _istft_dev(spec, i16=True)
    assert q.dtype == np.int16 and q.shape == y64.shape
    out, inside, share = R.int16_verdict(q, y64, band)
    o32, i32, _ = R.int16_verdict(R.to_int16(y32), y64, band)
    print(f"[istft] int16 {kind} N={N} hops={T - 1}: peak {peak * 32767:.0f} LSB, delta {delta:.2e} LSB, band {100 * share:.2f} % of the "
          f"samples; device {out} mismatches outside, max {inside} LSB inside (float32 statement {o32}, {i32})")
    assert 0.1 <= peak <= 0.5 and peak * 32767 >= 3000
    assert share <= 0.05
    assert out == 0 and inside <= 1
    if kind == "near":
        h = y64.shape[1] // 2
        assert (q[0, h:] >= 2).all() and (q[0, h:] <= 3).all() and (q[1, h:] <= -2).all() and (q[1, h:] >= -3).all()
        assert {2, 3} == set(np.unique(q[0, h:])) and {-3, -2} == set(np.unique(q[1, h:]))


def _abi_istft(spec, want_i16, want_f32, sentinel=True):
    from misonet_amd import _lib
    L = _lib.lib()
    z = torch.from_numpy(np.array(spec)).cuda()
    N, T, _ = z.shape
    n = 64 * (T - 1)
    oi = torch.full((N, n), -12345, dtype=torch.int16, device="cuda")
    of = torch.full((N, n), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.misonet_istft(z.data_ptr(), N, T, oi.data_ptr() if want_i16 else None, of.data_ptr() if want_f32 else None,
                         _lib.stream_ptr(z.device))
    torch.cuda.synchronize()
    assert rc == _lib.OK
    return oi.cpu().numpy(), of.cpu().numpy()


@pytest.mark.parametrize("T", [63, 124])
def test_istft_both_outputs_in_one_call_and_sentinels(T):
    """out_f32 and out_i16 of one call = the two separate calls, bit for bit; outputs that held a sentinel are fully overwritten
    (62 hops: the second workgroup writes a single hop), and the output that was not asked for is left alone"""
    _need_gpu()
    spec, y64, _, _, _ = _int16_ref("white", 3 if T == 124 else 1, T)
    bi, bf = _abi_istft(spec, True, True)
    i_only, f_left = _abi_istft(spec, True, False)
    i_left, f_only = _abi_istft(spec, False, True)
    assert np.array_equal(bi, i_only) and np.array_equal(_bits(bf), _bits(f_only))
    assert np.isfinite(bf).all() and np.isnan(f_left).all() and (i_left == -12345).all()
    # no sample of this input casts to the sentinel, so a left-over would show
    want = R.to_int16(y64).astype(np.int32)
    assert np.abs(bi.astype(np.int32) - want).max() <= 1
    assert np.array_equal(_bits(bf), _bits(_istft_dev(spec))) and np.array_equal(bi, _istft_dev(spec, i16=True))
    # two runs, and an item alone
    assert np.array_equal(_bits(_istft_dev(spec)), _bits(bf))
    if spec.shape[0] > 1:
        assert np.array_equal(_bits(_istft_dev(spec[1:2])[0]), _bits(bf[1]))


# ----------------------------------------------------------------------------------------------------------------------
# one coefficient at a time
COEFFS = [("re", 0), ("re", 1), ("re", 127), ("re", 128), ("im", 1), ("im", 64), ("im", 128)]


def _single_coefficient_case(T=124):
    """items x frames: every coefficient kind in frames 0, 1, T - 2, T - 1 and 60 ... 63 (both sides of the workgroup seam), the
    frames of one item at least 4 apart so that no output sample sees two coefficients"""
    patterns = [[0, 60, T - 2], [1, 61, T - 1], [62], [63]]
    itw, _ = R.istft_tables()
    env = R.envelope(T)                                                  # float64 sum of the float32 w^2 entries
    n = 64 * (T - 1)
    items = [(p, c) for p in patterns for c in COEFFS]
    spec = np.zeros((len(items), T, 129), np.complex64)
    want = np.zeros((len(items), n), np.float64)
    table = np.zeros((len(items), n), np.float32)
    for i, (p, (part, f)) in enumerate(items):
        assert all(b - a >= 4 for a, b in zip(p, p[1:]))
        for t in p:
            spec[i, t, f] = 1.0 if part == "re" else 1j
            row = itw[f if part == "re" else 129 + f]
            for k in range(256):
                s = 64 * t - 128 + k
                if 0 <= s < n:
                    table[i, s] = row[k]
                    want[i, s] = float(row[k]) / env[s]
    return spec, want, table


def test_istft_single_coefficients_give_table_over_envelope():
    """each output sample is one table entry divided by the envelope: within 2^-21 relative of table32 / sum w^2_32 (the latter in
    float64), exactly 0 where the table entry is 0 and wherever no coefficient reaches"""
    _need_gpu()
    spec, want, table = _single_coefficient_case()
    got = _istft_dev(spec).astype(np.float64)
    zero = table == 0
    assert zero.any() and (~zero).any()
    bad0 = np.argwhere(zero & (got != 0))
    assert bad0.size == 0, f"{len(bad0)} samples are not 0, first (item, sample) = {bad0[0].tolist()}"
    err = np.abs(got - want)
    lim = 2.0 ** -21 * np.abs(want)
    # a quotient below the normal range of float32 is rounded on the subnormal grid (2^-149), not relatively
    lim = np.maximum(lim, np.where(np.abs(want) < 2.0 ** -126, 2.0 ** -149, 0.0))
    bad = np.argwhere(~zero & (err > lim))
    worst = float((err[~zero] / np.abs(want[~zero])).max())
    print(f"[istft] single coefficients: {spec.shape[0]} items, worst relative error {worst:.3e} = {worst * 2.0 ** 24:.2f} x 2^-24 "
          f"(allowed 8)")
    assert bad.size == 0, f"{len(bad)} samples off, first (item, sample) = {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


# ----------------------------------------------------------------------------------------------------------------------
# round trip
@functools.lru_cache(maxsize=None)
def _round_trip_ref(T):
    wav = R.wave("white", 2, 64 * (T - 1), 3, seed=9)
    x = np.ascontiguousarray(wav.transpose(0, 2, 1)).reshape(6, -1).astype(np.float64)
    back32 = R.istft32(R.stft32(wav).reshape(6, T, 129))
    return wav, x, R.istft_metrics(back32, x)


@pytest.mark.parametrize("T", [65, 129])
def test_round_trip(T):
    """istft(stft_hip(x)) against x, L = 64 (T - 1): the bar is 4 x the float32 statement's own round-trip error on the same x"""
    _need_gpu()
    from misonet_amd import stft as S
    wav, x, m32 = _round_trip_ref(T)
    spec = S.stft_hip(torch.from_numpy(np.array(wav)).cuda())
    back = S.istft(spec)[..., :wav.shape[1]].cpu().numpy().reshape(6, -1)
    m = R.istft_metrics(back, x)
    print(_line("istft", f"round trip T={T}", m, m32, R.ISTFT_KEYS))
    over = R.over_bar(m, m32, R.ISTFT_KEYS)
    assert all(v <= 1.0 for v in over.values()), (over, m["where"])
