"""CPU checks of the streaming STFT / iSTFT: the library's count functions equal the restatement's formulas (tests/stream_ref.py),
the restatement's streamed output equals its own one-shot output EXACTLY for any cut and equals torch's transforms within their
float32 rounding, the planted mistakes are rejected by that exact-equality check -- all but a tail that merely loses its oldest
sample, which no output can show because hann[0] = 0 multiplies that sample (the test says so and rejects the misaligned
254-sample tail instead) -- and the host side of the C ABI (version, prototypes, refusals) behaves.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import stream_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
# cuts (cycled): single samples and hops, every residue of the phase, blocks past one and two frames
CUTS = [[1], [64], [63, 1, 65, 127, 2, 129, 255, 256, 257, 128], [1000, 3, 61], [4097]]
FCUTS = [[1], [2, 1, 3], [4, 60, 1, 61, 62, 64, 65], [1000]]
LENGTHS = [1, 5, 63, 64, 65, 127, 128, 129, 191, 192, 200, 64 * 5, 64 * 7 + 17, 64 * 33 + 5]
FRAMES = [2, 3, 4, 5, 9, 40]


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _wave(L, M, seed=0):
    return np.random.default_rng(1000 * seed + L + M).standard_normal((L, M)) * 0.1


def _spec(Rr, T, seed=0):
    r = np.random.default_rng(7000 * seed + 10 * T + Rr)
    X = r.standard_normal((Rr, T, R.F)) + 1j * r.standard_normal((Rr, T, R.F))
    X[..., 0] = X[..., 0].real                  # a real signal's spectrum: DC and Nyquist are real
    X[..., -1] = X[..., -1].real
    return X


# ---- the count functions -----------------------------------------------------------------------------------------------------
def test_library_counts_equal_the_restatement():
    lib = _lib().lib()
    fr, hp = lib.misonet_stft_stream_frames, lib.misonet_istft_stream_hops
    for flush in (0, 1):
        for seen in range(0, 401):
            for new in range(0, 301):
                assert fr(seen, new, flush) == R.stft_frames(seen, new, flush), (seen, new, flush)
                assert hp(seen, new, flush) == R.istft_hops(seen, new, flush), (seen, new, flush)
    for seen, new in [(10 ** 12 + 37, 1 << 28), (1 << 40, 1), ((1 << 40) + 63, 64), (5, 1 << 22)]:
        for flush in (0, 1):
            assert fr(seen, new, flush) == R.stft_frames(seen, new, flush)
            if new <= R.MAX_T:
                assert hp(seen, new, flush) == R.istft_hops(seen, new, flush)


def test_count_formulas():
    # e(N), g(Tc), and the totals of a flushed stream: L // 64 + 1 frames, T - 1 hops (none for T <= 1)
    assert [R.emitted_frames(n) for n in (0, 63, 64, 127, 128, 191, 192)] == [0, 0, 0, 0, 1, 1, 2]
    assert [R.emitted_hops(t) for t in (0, 1, 2, 3, 4)] == [0, 0, 0, 1, 2]
    for L in LENGTHS:
        for cuts in CUTS:
            pc = R.pieces(L, cuts)
            tot = sum(R.stft_frames(a, b - a, i == len(pc) - 1) for i, (a, b) in enumerate(pc))
            assert tot == L // 64 + 1, (L, cuts)
            assert sum(R.stft_frames(a, b - a, 0) for a, b in pc) + R.stft_frames(L, 0, 1) == L // 64 + 1
    for T in (0, 1, 2, 3, 4, 70):
        for cuts in FCUTS:
            pc = R.pieces(T, cuts)
            assert sum(R.istft_hops(a, b - a, 0) for a, b in pc) + R.istft_hops(T, 0, 1) == max(0, T - 1), (T, cuts)
    # the tail is long enough: the first frame a call can owe starts no earlier than 255 samples before the stream's end
    assert all(64 * R.emitted_frames(N) - 128 >= N - 255 for N in range(128, 2000))
    assert all(R.emitted_hops(Tc) - 1 >= Tc - 3 for Tc in range(2, 200))


# ---- the restatement: cut-invariant to the bit, and the transform torch computes ------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_stft_restatement_streams_to_its_one_shot_bits(L):
    x = _wave(L, 2)
    ref = R.stft(x)
    assert ref.shape == (2, L // 64 + 1, R.F)
    for cuts in CUTS:
        for with_block in (True, False):
            assert _same(R.stft_stream(x, cuts, flush_with_block=with_block), ref), (L, cuts, with_block)


@pytest.mark.parametrize("T", FRAMES)
def test_istft_restatement_streams_to_its_one_shot_bits(T):
    X = _spec(3, T)
    ref = R.istft(X)
    assert ref.shape == (3, 64 * (T - 1))
    for cuts in FCUTS:
        for with_block in (True, False):
            assert _same(R.istft_stream(X, cuts, flush_with_block=with_block), ref), (T, cuts, with_block)


def test_a_stream_flushed_with_fewer_than_two_frames_emits_nothing():
    for T in (0, 1):
        st = R.IstftStream(2)
        out = st.process(_spec(2, T), flush=True)
        assert out.shape == (2, 0)


@pytest.mark.parametrize("L", [1, 40, 64, 127, 128, 129, 64 * 7 + 17])
def test_stft_restatement_is_torchs_transform(L):
    """float32 rounding of torch's FFT: a bin is a sum of 256 terms |x_j| w_j through log2(256) = 8 butterfly levels, each
    rounding to EPS32 relative: |error| <= 8 EPS32 sum_j |x_j| w_j <= 8 EPS32 128 max|x|; x2 for the input's own rounding and the
    float32 window.  No figure of the code under test enters the bound."""
    import torch
    from misonet_amd import stft as S
    x = _wave(L, 2)
    got = S.stft(torch.from_numpy(x.T.astype(np.float32).copy())).numpy().astype(np.complex128)         # [M, T, F]
    ref = R.stft(x.astype(np.float32))
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 2 * 8 * EPS32 * 128 * np.abs(x).max()


@pytest.mark.parametrize("T", [2, 3, 4, 9])
def test_istft_restatement_is_torchs_transform(T):
    """a segment sample is 1/256 of a sum of 256 spectral terms through 8 levels: |error| <= 8 EPS32 mean-bound; the overlap-add
    adds up to four of them and divides by an envelope >= 1 (1.25 at the edges of hop 0 and of the flush hop, 1.5 inside), and
    every step rounds once more: 4 (8 + 4) EPS32 max_t,k |irfft(X_t)[k]|-bound with |irfft| <= sum_f c_f |X_f| / 256."""
    import torch
    from misonet_amd import stft as S
    X = _spec(2, T)
    got = S.istft(torch.from_numpy(X.astype(np.complex64))).numpy().astype(np.float64)
    ref = R.istft(X.astype(np.complex64))
    assert got.shape == ref.shape == (2, 64 * (T - 1))
    zmax = (2 * np.abs(X).sum(axis=-1) / 256).max()
    assert np.abs(got - ref).max() <= 4 * 12 * EPS32 * zmax


# ---- planted faults: each one is rejected by exact equality --------------------------------------------------------------------
def test_planted_faults_are_rejected():
    x = _wave(64 * 9 + 17, 2, seed=1)
    X = _spec(2, 12, seed=1)
    sref, iref = R.stft(x), R.istft(X)
    scuts, fcuts = [127, 128, 65, 63, 1, 130], [1, 2, 4]
    assert _same(R.stft_stream(x, scuts), sref) and _same(R.istft_stream(X, fcuts), iref)
    for fault in ("tail_stuck", "tail_254_shifted", "phase_n_new"):
        got = R.stft_stream(x, scuts, fault=fault)
        assert got.shape == sref.shape and not _same(got, sref), fault
        assert _same(R.istft_stream(X, fcuts, fault=fault), iref)           # ... and touches nothing else
    for fault in ("missing_as_zero", "flush_full_envelope", "carry_2"):
        got = R.istft_stream(X, fcuts, fault=fault)
        assert got.shape == iref.shape and not _same(got, iref), fault
        assert _same(R.stft_stream(x, scuts, fault=fault), sref)
    # where each one bites: the edges only, or everything behind the first cut
    d = np.abs(R.istft_stream(X, fcuts, fault="missing_as_zero") - iref).max(axis=0).reshape(-1, 64).max(axis=1)
    assert d[0] > 0 and d[-1] > 0 and not d[1:-1].any()
    d = np.abs(R.istft_stream(X, fcuts, fault="flush_full_envelope") - iref).max(axis=0).reshape(-1, 64).max(axis=1)
    assert d[-1] > 0 and not d[:-1].any()
    # A tail that merely loses its oldest sample (254 kept, aligned to the end) cannot be rejected by ANY comparison of outputs:
    # the only frame that reads the sample 255 back starts with it, and hann[0] == 0 multiplies it.  The fault that a 254-sample
    # tail does make visible is the misalignment above ("tail_254_shifted").
    assert R.WIN[0] == 0.0
    for cuts in ([127, 128], scuts, [1]):                                   # n_seen = 255: frame 2 starts at the tail's first slot
        assert _same(R.stft_stream(x, cuts, fault="tail_254"), sref)


def test_int16_cast_truncates_toward_zero():
    y = np.array([0.99999, -0.99999, 0.5 / 32767, -0.5 / 32767, 1.5 / 32767, -1.5 / 32767, 0.1])
    assert R.to_int16(y).tolist() == [32766, -32766, 0, 0, 1, -1, 3276]


# ---- the C ABI, host side --------------------------------------------------------------------------------------------------
NEW = {"misonet_stft_stream_state_bytes", "misonet_stft_stream_reset", "misonet_stft_stream_frames", "misonet_stft_stream",
       "misonet_istft_stream_state_bytes", "misonet_istft_stream_reset", "misonet_istft_stream_hops", "misonet_istft_stream"}


def test_abi_650():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 650
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name), name
    # the state does not grow with the stream: the size functions take no length
    assert re.search(r"long long misonet_stft_stream_state_bytes\(([^)]*)\);", hdr).group(1).replace(" ", "") == "intB,intM"
    assert re.search(r"long long misonet_istft_stream_state_bytes\(([^)]*)\);", hdr).group(1).replace(" ", "") == "intR"
    assert lib.misonet_stft_stream_state_bytes(3, 6) == 3 * 6 * 256 * 4            # 255 samples and a zero, float32
    assert lib.misonet_istft_stream_state_bytes(5) == 5 * 3 * 129 * 8             # 3 frames, complex64


# (B, M)
BAD_BM = [(0, 2), (-1, 2), (65536, 2), (1, 0), (1, -1), (1, 65)]
BAD_R = [0, -1, 65536]
# (seen, new, flush)
BAD_N = [(-1, 64, 0), (-1, 64, 1), (0, 0, 0), (100, 0, 0), (0, -1, 0), (0, -1, 1), (0, (1 << 28) + 1, 0), (0, (1 << 28) + 1, 1)]
BAD_T = [(-1, 4, 0), (-1, 4, 1), (0, 0, 0), (7, 0, 0), (0, -1, 0), (0, -1, 1), (0, (1 << 22) + 1, 0), (0, (1 << 22) + 1, 1)]


def test_every_refusal_comes_before_any_pointer_is_looked_at():
    L = _lib()
    lib = L.lib()
    big = 1 << 40
    for B, M in BAD_BM:
        assert lib.misonet_stft_stream_state_bytes(B, M) == -1, (B, M)
        assert lib.misonet_stft_stream_reset(None, B, M, None) == L.EINVAL, (B, M)
        assert lib.misonet_last_error(), (B, M)
        assert lib.misonet_stft_stream(None, B, 64, M, 0, 0, None, None, big, None) == L.EINVAL, (B, M)
    for Rr in BAD_R:
        assert lib.misonet_istft_stream_state_bytes(Rr) == -1, Rr
        assert lib.misonet_istft_stream_reset(None, Rr, None) == L.EINVAL, Rr
        assert lib.misonet_istft_stream(None, Rr, 4, 0, 0, None, None, None, big, None) == L.EINVAL, Rr
    for seen, new, flush in BAD_N:
        assert lib.misonet_stft_stream_frames(seen, new, flush) == -1, (seen, new, flush)
        assert lib.misonet_stft_stream(None, 1, new, 2, seen, flush, None, None, big, None) == L.EINVAL, (seen, new, flush)
        assert lib.misonet_last_error(), (seen, new, flush)
    for seen, new, flush in BAD_T:
        assert lib.misonet_istft_stream_hops(seen, new, flush) == -1, (seen, new, flush)
        assert lib.misonet_istft_stream(None, 3, new, seen, flush, None, None, None, big, None) == L.EINVAL, (seen, new, flush)
        assert lib.misonet_last_error(), (seen, new, flush)
    # legal counts, null pointers: still refused, nothing launched
    assert lib.misonet_stft_stream(None, 1, 256, 2, 0, 0, None, None, big, None) == L.EINVAL
    assert lib.misonet_istft_stream(None, 3, 4, 4, 0, None, None, None, big, None) == L.EINVAL
    assert lib.misonet_stft_stream_reset(None, 1, 2, None) == L.EINVAL and lib.misonet_istft_stream_reset(None, 3, None) == L.EINVAL
    # a short state is ENOMEM (addresses only: nothing is launched)
    a, b, s = C.c_void_p(1 << 30), C.c_void_p(2 << 30), C.c_void_p(3 << 30)
    assert lib.misonet_stft_stream(a, 2, 256, 3, 0, 0, b, s, lib.misonet_stft_stream_state_bytes(2, 3) - 1, None) == L.ENOMEM
    assert lib.misonet_istft_stream(a, 3, 4, 4, 0, None, b, s, lib.misonet_istft_stream_state_bytes(3) - 1, None) == L.ENOMEM
    # a call that emits nothing needs no output: the pointer check passes, the state's size is looked at next
    assert lib.misonet_stft_stream(a, 2, 20, 3, 0, 0, None, s, 0, None) == L.ENOMEM
    assert lib.misonet_istft_stream(a, 3, 1, 0, 0, None, None, s, 0, None) == L.ENOMEM
