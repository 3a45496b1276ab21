"""GPU tests of the room simulator (csrc/room.hip, ``misonet_amd.room``) against the float64 NumPy restatement of
tests/room_ref.py: RIRs at every Lh around the tile, three batch geometries, three sets of beta, four values of max_order and a
source 2 cm from a wall; the mixer at every (L, Lh, Lo, split, strides) of room_ref's lists; bit-reproducibility, independence of
the batch, buffers full of NaN, a source on a microphone, a point outside the room, a captured HIP graph; and ``simulate`` end to
end into ``dereverb_wav`` and ``BlindSeparator.separate_recording``.

Bars.  RIR: rel-L2 and the worst tap error relative to the peak, each <= max(100 x the restatement's own permuted-order
difference on that case, 1e-12).  Mixer: images, early and mix within rel-L2 <= 1.2e-7 = 2 x 2^-24 of the float64 reference (one
float32 rounding of a float64 sum, plus a rare flipped rounding); ``early`` with split >= Lh bit-equal to ``images``.  The module
prints every figure (``[room] ...``); LAB.md has them."""
import functools
import os

import numpy as np
import pytest
import torch

import room_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
FS = R.FS


def _tile():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return int(_lib.lib().misonet_room_tile())


TILE = _tile()
CASES = R.rir_cases(TILE)
CASE_ID = lambda c: f"Lh{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-o{c[3]}" + ("-wall" if c[4] else "")


@functools.lru_cache(maxsize=None)
def _ref(case):
    """(inputs, the restatement, the restatement summed in a permuted order), computed once per case"""
    Lh, _, _, mo, _ = case
    inp = R.rir_case_inputs(case)
    return inp, R.rir(*inp, FS, Lh, max_order=mo), R.rir(*inp, FS, Lh, max_order=mo, image_order=5)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _raw_rir(room, beta, src, mic, Lh, max_order=None, fill=0.0, fs=FS, c=343.0):
    """misonet_room_rir itself on outputs that held ``fill`` -> (rir, fail) as numpy"""
    from misonet_amd import _lib
    B, S, M = src.shape[0], src.shape[1], mic.shape[1]
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda() for a in (room, beta, src, mic)]
    out = torch.full((B, S, M, Lh), fill, dtype=torch.float64, device="cuda")
    fail = torch.full((B, S, M), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().misonet_room_rir(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), B, S, M, float(fs),
                                           float(c), Lh, -1 if max_order is None else max_order, out.data_ptr(), fail.data_ptr(),
                                           _lib.stream_ptr(out.device)))
    return out.cpu().numpy(), fail.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=CASE_ID)
def test_rir_against_restatement(case):
    _need_gpu()
    from misonet_amd import room as RM
    Lh, (B, S, M), _, mo, wall = case
    (room, beta, src, mic), (want, wfail), (perm, _) = _ref(case)
    rooms = [RM.Room(tuple(room[b]), beta=tuple(beta[b])) for b in range(B)]
    got, fail = RM.rir(rooms, src, mic, FS, Lh, max_order=mo, return_fail=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (B, S, M, Lh)
    assert fail.dtype == np.int32 and fail.shape == (B, S, M) and not fail.any() and not wfail.any()
    assert np.isfinite(got).all() and (Lh < 100 or np.abs(want).max() > 0)
    for b in range(B):
        for s in range(S):
            for m in range(M):
                fig = R.figures(got[b, s, m], want[b, s, m], perm[b, s, m])
                print(f"[room] rir {CASE_ID(case)} pair {b}.{s}.{m}: " +
                      "  ".join(f"{k} {v:.3e} (bar {bar:.3e})" for k, (v, bar) in fig.items()))
                assert not R.missed(fig), (b, s, m, fig)
    if B == 1:                                             # the single-room call is the batched one without the axis
        one = RM.rir(rooms[0], src[0], mic[0], FS, Lh, max_order=mo)
        assert one.shape == (S, M, Lh) and np.array_equal(_bits(one), _bits(got[0]))


def test_max_order_none_is_a_large_order():
    _need_gpu()
    case = CASES[5]
    Lh = case[0]
    inp = R.rir_case_inputs(case)
    a, _ = _raw_rir(*inp, Lh, None)
    b, _ = _raw_rir(*inp, Lh, 10000)
    assert np.array_equal(_bits(a), _bits(b)) and np.abs(a).max() > 0


def _run_mix(x, h, split, Lo, strided, fill=0.0, with_early=True, with_mix=True):
    """misonet_room_mix itself -> (images, early, mix) as numpy float32"""
    from misonet_amd import _lib
    S, L = x.shape
    M, Lh = h.shape[1], h.shape[2]
    if strided:                                            # time-major [L][S] with a gap: sample stride 2 S, source stride 2
        buf = torch.zeros((L, S, 2), dtype=torch.float32, device="cuda")
        buf[:, :, 0] = torch.from_numpy(x.T.copy()).cuda()
        xv = buf[:, :, 0].t()
        assert xv.stride() == (2, 2 * S)
    else:
        xv = torch.from_numpy(x).cuda()
    hd = torch.from_numpy(h).cuda()
    sp = torch.from_numpy(np.ascontiguousarray(split, np.int32)).cuda() if split is not None else None
    images = torch.full((S, M, Lo), fill, dtype=torch.float32, device="cuda")
    early = torch.full((S, M, Lo), fill, dtype=torch.float32, device="cuda") if with_early else None
    mix = torch.full((M, Lo), fill, dtype=torch.float32, device="cuda") if with_mix else None
    _lib.check(_lib.lib().misonet_room_mix(xv.data_ptr(), 0, xv.stride(0), xv.stride(1), hd.data_ptr(),
                                           sp.data_ptr() if sp is not None else None, 1, S, M, L, Lh, Lo, images.data_ptr(),
                                           early.data_ptr() if with_early else None, mix.data_ptr() if with_mix else None,
                                           _lib.stream_ptr(images.device)))
    return tuple(None if t is None else t.cpu().numpy() for t in (images, early, mix))


@pytest.mark.parametrize("Lh", R.MIX_LH)
@pytest.mark.parametrize("L", R.MIX_L)
def test_mix_against_convolve(L, Lh):
    """every Lo in {L, L + Lh - 1}, split in {0, 40, past Lh}, contiguous and strided sources at this (L, Lh)"""
    _need_gpu()
    x, h = R.mix_case_inputs(L, Lh)
    worst = 0.0
    for Lo in sorted({L, L + Lh - 1}):
        for split in R.MIX_SPLITS:
            sp = R.mix_split(split, Lh)
            want = R.mix(x, h, sp, Lo)
            for strided in (False, True):
                got = _run_mix(x, h, sp, Lo, strided)
                for name, g, w in zip(("images", "early", "mix"), got, want):
                    assert g.dtype == np.float32 and g.shape == w.shape
                    if np.abs(w).max() == 0:
                        assert not g.any(), (name, Lo, split, strided)
                        continue
                    e = R.rel_l2(g, w)
                    worst = max(worst, e)
                    assert e <= R.MIX_BAR, (name, Lo, split, strided, e)
                if split is None:                          # both splits past the last tap: the same bits
                    assert np.array_equal(_bits(got[0]), _bits(got[1])), (Lo, strided)
                if split == 0:                             # source 0 has no early part at all
                    assert not got[1][0].any()
    print(f"[room] mix L {L} Lh {Lh}: worst rel-L2 {worst:.3e} (bar {R.MIX_BAR:.1e})")


@pytest.mark.parametrize("L,Lh,split", [(300, 513, 512), (700, 1100, 520), (130, 1025, 1024)])
def test_mix_past_one_chunk_of_taps(L, Lh, split):
    """more taps than the kernel stages at once (512): a split on a chunk's edge, inside the second chunk, on the last tap"""
    _need_gpu()
    x, h = R.mix_case_inputs(L, Lh)
    h = h * np.exp(np.arange(Lh) / 61.0)                   # nearly flat: the late chunks carry as much as the first
    sp = np.array([split, 0], np.int32)
    for Lo in (L, L + Lh - 1):
        want = R.mix(x, h, sp, Lo)
        got = _run_mix(x, h, sp, Lo, True)
        errs = [R.rel_l2(g[..., :], w) for g, w in zip(got, want)]
        print(f"[room] mix L {L} Lh {Lh} Lo {Lo} split {split}: rel-L2 " + " ".join(f"{e:.3e}" for e in errs))
        assert all(e <= R.MIX_BAR for e in errs) and not got[1][1].any()


def test_mix_null_outputs_and_null_split():
    _need_gpu()
    x, h = R.mix_case_inputs(257, 80)
    full = _run_mix(x, h, R.mix_split(40, 80), 300, False)
    only = _run_mix(x, h, R.mix_split(40, 80), 300, False, with_early=False, with_mix=False)
    assert only[1] is None and only[2] is None and np.array_equal(_bits(only[0]), _bits(full[0]))
    nosplit = _run_mix(x, h, None, 300, False)             # split NULL = Lh
    assert np.array_equal(_bits(nosplit[1]), _bits(nosplit[0])) and np.array_equal(_bits(nosplit[0]), _bits(full[0]))


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    from misonet_amd import room as RM
    Lh = TILE + 44
    room, src, mic = R.geometry(3, 2, 3, seed=11)
    beta = np.tile(np.array(R.BETAS["distinct"]), (3, 1)) * np.array([1.0, 0.9, 0.8])[:, None]
    a, fa = _raw_rir(room, beta, src, mic, Lh)
    b, fb = _raw_rir(room, beta, src, mic, Lh)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(fa, fb) and not fa.any() and np.isfinite(a).all()
    for i in range(3):
        one, _ = _raw_rir(room[i:i + 1], beta[i:i + 1], src[i:i + 1], mic[i:i + 1], Lh)
        assert np.array_equal(_bits(one[0]), _bits(a[i])), i
    x = np.random.default_rng(0).standard_normal((3, 2, 500)).astype(np.float32)
    h = torch.from_numpy(a).cuda()
    out = RM.mix(torch.from_numpy(x).cuda(), h, FS, early_ms=5.0, out_len=500 + Lh - 1)
    again = RM.mix(torch.from_numpy(x).cuda(), h, FS, early_ms=5.0, out_len=500 + Lh - 1)
    for i in range(3):
        one = RM.mix(torch.from_numpy(x[i]).cuda(), h[i], FS, early_ms=5.0, out_len=500 + Lh - 1)
        for t, u, v in zip(out, again, one):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(u.cpu().numpy()))
            assert np.array_equal(_bits(t[i].cpu().numpy()), _bits(v.cpu().numpy())), i


def test_nan_buffers_change_nothing():
    """outputs that held NaN before the call: the same bits as with zeros (neither call has scratch)"""
    _need_gpu()
    case = CASES[6]
    inp = R.rir_case_inputs(case)
    a, fa = _raw_rir(*inp, case[0], fill=0.0)
    b, fb = _raw_rir(*inp, case[0], fill=float("nan"))
    assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b)) and np.array_equal(fa, fb)
    x, h = R.mix_case_inputs(257, 300)
    sp = R.mix_split(40, 300)
    for u, v in zip(_run_mix(x, h, sp, 400, True, fill=0.0), _run_mix(x, h, sp, 400, True, fill=float("nan"))):
        assert np.isfinite(u).all() and np.array_equal(_bits(u), _bits(v))


def test_source_on_a_microphone_and_a_point_outside():
    """argument handling, not faults: flag bit 1 with a finite RIR that lacks only the dropped image; flag bit 0 (a point
    outside, a NaN coordinate, a beta of 1, an edge of 0) and bit 2 (too many images) with a zero RIR -- and the neighbouring
    pairs of the same call untouched"""
    _need_gpu()
    Lh = 300
    room, src, mic = R.geometry(1, 2, 2, seed=4)
    beta = np.array([R.BETAS["distinct"]])
    good, gf = _raw_rir(room, beta, src, mic, Lh)
    assert not gf.any()
    on = mic.copy()
    on[0, 1] = src[0, 0]                                   # microphone 1 on source 0
    h, f = _raw_rir(room, beta, src, on, Lh)
    want, wf = R.rir(room, beta, src, on, FS, Lh)
    assert f[0, 0, 1] == 2 and wf[0, 0, 1] == 2 and f[0, 0, 0] == 0 and f[0, 1, 0] == 0
    assert np.isfinite(h).all() and R.rel_l2(h, want) <= 1e-12
    assert np.array_equal(_bits(h[0, :, 0]), _bits(good[0, :, 0]))
    for what in ("outside", "nan", "beta", "edge", "many"):
        r2, b2, s2, fs = room.copy(), beta.copy(), src.copy(), FS
        if what == "outside":
            s2[0, 1, 2] = r2[0, 2] + 0.01
        elif what == "nan":
            s2[0, 1, 0] = np.nan
        elif what == "beta":
            b2[0, 3] = 1.0
        elif what == "edge":
            r2[0, 1] = 0.0
        else:
            r2[0, 0] = 0.004                               # N_x far above 255
            s2[0, :, 0] = 0.002
        mm = mic.copy()
        if what == "many":
            mm[0, :, 0] = 0.002
        h, f = _raw_rir(r2, b2, s2, mm, Lh, fill=float("nan"), fs=fs)
        _, wf = R.rir(r2, b2, s2, mm, fs, Lh)
        assert np.array_equal(f, wf), (what, f, wf)
        bit = 4 if what == "many" else 1
        whole = what in ("beta", "edge", "many")           # these spoil every pair of the item
        assert f[0, 1, 0] == bit and f[0, 1, 1] == bit and (f[0, 0] == (bit if whole else 0)).all(), (what, f)
        assert not h[0, 1].any() and np.isfinite(h).all(), what
        if not whole:
            assert np.array_equal(_bits(h[0, 0]), _bits(good[0, 0])), what


def test_mix_wrapper_split_and_lengths():
    """``room.mix``: split = direct + round(early_ms fs / 1000) clamped to Lh; without ``direct`` the tap of the largest magnitude,
    the smallest over the microphones; out_len None is L; tensors in, device tensors out"""
    _need_gpu()
    from misonet_amd import room as RM
    x, h = R.mix_case_inputs(257, 300)
    h[:, :, 0] = 0.1
    h[0, np.arange(3), [17, 12, 25]] = 9.0                  # source 0 peaks at taps 17, 12, 25 of its three microphones
    h[1, :, 280] = 9.0
    for direct, first in ((None, (12, 280)), ([3, 5], (3, 5))):
        got = RM.mix(x, h, 1000, early_ms=30.0, direct=direct)
        want = R.mix(x, h, np.minimum(np.array(first) + 30, 300), 257)
        assert all(isinstance(g, np.ndarray) and g.shape == w.shape for g, w in zip(got, want))
        assert all(R.rel_l2(g, w) <= R.MIX_BAR for g, w in zip(got, want)), direct
    dev = RM.mix(torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda(), 1000, early_ms=30.0, direct=[3, 5], out_len=556)
    assert all(t.is_cuda for t in dev) and dev[0].shape == (2, 3, 556) and dev[2].shape == (3, 556)
    assert np.array_equal(_bits(dev[1][..., :257].cpu().numpy()), _bits(got[1]))


def test_hip_graph():
    """misonet_room_rir and misonet_room_mix captured once, replayed with new geometry and new sources copied in: the bits of
    the eager calls"""
    _need_gpu()
    from misonet_amd import _lib
    L = _lib.lib()
    B, S, M, Lh, Ls = 1, 2, 3, TILE + 10, 400
    Lo = Ls + Lh - 1
    geos, eager = [], []
    beta = np.array([R.BETAS["distinct"]])
    for i in range(3):
        room, src, mic = R.geometry(B, S, M, seed=60 + i)
        x = np.random.default_rng(i).standard_normal((S, Ls)).astype(np.float32)
        sp = R.direct_sample(src[0], mic[0], FS).astype(np.int32) + 40
        h, _ = _raw_rir(room, beta, src, mic, Lh)
        geos.append((room, src, mic, x, sp))
        eager.append((h, _run_mix(x, h[0], sp, Lo, False)))
    assert not np.array_equal(eager[1][0], eager[2][0])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    room_d, beta_d, src_d, mic_d = (dev(a, np.float64) for a in (geos[0][0], beta, geos[0][1], geos[0][2]))
    x_d, sp_d = dev(geos[0][3], np.float32), dev(geos[0][4], np.int32)
    h_d = torch.zeros((B, S, M, Lh), dtype=torch.float64, device="cuda")
    fail = torch.zeros((B, S, M), dtype=torch.int32, device="cuda")
    img, early = (torch.zeros((B, S, M, Lo), dtype=torch.float32, device="cuda") for _ in range(2))
    mixd = torch.zeros((B, M, Lo), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st = _lib.stream_ptr(h_d.device)
            _lib.check(L.misonet_room_rir(room_d.data_ptr(), beta_d.data_ptr(), src_d.data_ptr(), mic_d.data_ptr(), B, S, M,
                                          float(FS), 343.0, Lh, -1, h_d.data_ptr(), fail.data_ptr(), st))
            _lib.check(L.misonet_room_mix(x_d.data_ptr(), S * Ls, Ls, 1, h_d.data_ptr(), sp_d.data_ptr(), B, S, M, Ls, Lh, Lo,
                                          img.data_ptr(), early.data_ptr(), mixd.data_ptr(), st))
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2):
        room, src, mic, x, sp = geos[i]
        room_d.copy_(dev(room, np.float64)); src_d.copy_(dev(src, np.float64)); mic_d.copy_(dev(mic, np.float64))
        x_d.copy_(dev(x, np.float32)); sp_d.copy_(dev(sp, np.int32))
        for t in (h_d, img, early, mixd):
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(h_d.cpu().numpy()), _bits(eager[i][0])), i
        for t, w in zip((img, early, mixd), eager[i][1]):
            assert np.array_equal(_bits(t[0].cpu().numpy()), _bits(w)), i
        assert not fail.cpu().numpy().any()


def test_simulate_end_to_end():
    _need_gpu()
    from misonet_amd import room as RM
    from misonet_amd.blind import BlindSeparator
    from misonet_amd.dereverb import dereverb_wav
    clean = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_stoi.npz"))["clean"][:, 8000:24000]
    S, L = clean.shape
    M, Lh, snr = 6, 1024, 20.0
    room = RM.Room((3.2, 2.6, 2.1), beta=0.6)
    ang = 2 * np.pi * np.arange(M) / M
    mic = np.stack([1.5 + 0.05 * np.cos(ang), 1.2 + 0.05 * np.sin(ang), np.full(M, 1.0)], 1)
    src = np.array([[2.6, 1.9, 1.3], [0.6, 0.5, 1.1]])
    sc = RM.simulate(clean, room, src, mic, FS, Lh, snr_db=snr, seed=3)
    assert isinstance(sc.wav, np.ndarray) and sc.wav.dtype == np.float32 and sc.wav.shape == (L, M)
    assert sc.images.dtype == sc.early.dtype == np.float32 and sc.images.shape == sc.early.shape == (S, L, M)
    assert sc.rir.dtype == np.float64 and sc.rir.shape == (S, M, Lh) and sc.fail.shape == (S, M) and not sc.fail.any()
    assert np.isfinite(sc.wav).all() and sc.noise.shape == sc.mix.shape == (L, M)
    got_snr = 10 * np.log10((sc.mix.astype(np.float64) ** 2).sum() / (sc.noise.astype(np.float64) ** 2).sum())
    print(f"[room] simulate: realised SNR {got_snr:.5f} dB for {snr} dB")
    assert abs(got_snr - snr) <= 0.01
    # wav - noise is the clean mixture (one float32 rounding of the sum) and that is the sum of the images: the mixture is the
    # float64 sum of the unrounded image sums rounded once, the images are those sums rounded, so each sample differs by at most
    # half an ulp of every image and half an ulp of the mixture
    u = 2.0 ** -24
    w64, n64, m64, i64 = (a.astype(np.float64) for a in (sc.wav, sc.noise, sc.mix, sc.images))
    assert (np.abs((w64 - n64) - m64) <= u * (np.abs(w64) + np.abs(n64)) + 1e-45).all()
    assert (np.abs(m64 - i64.sum(0)) <= u * (np.abs(i64).sum(0) + np.abs(m64)) + 1e-45).all()
    assert np.array_equal(sc.split, np.minimum(R.direct_sample(src, mic, FS) + 400, Lh))
    want = R.mix(clean, sc.rir, sc.split, L)
    assert R.rel_l2(sc.images, want[0].transpose(0, 2, 1)) <= R.MIX_BAR
    assert R.rel_l2(sc.early, want[1].transpose(0, 2, 1)) <= R.MIX_BAR
    same = RM.simulate(clean, room, src, mic, FS, Lh, snr_db=snr, seed=3)
    assert np.array_equal(_bits(same.wav), _bits(sc.wav))
    other = RM.simulate(clean, room, src, mic, FS, Lh, snr_db=snr, seed=4)
    assert not np.array_equal(other.noise, sc.noise) and np.array_equal(_bits(other.mix), _bits(sc.mix))
    quiet = RM.simulate(clean, room, src, mic, FS, Lh)
    assert not quiet.noise.any() and np.array_equal(_bits(quiet.wav), _bits(sc.mix))
    # the layout the recording paths take
    dry = dereverb_wav(sc.wav, fs=FS)
    assert dry.dtype == np.float32 and dry.shape == (L, M) and np.isfinite(dry).all()
    pcm = BlindSeparator(num_spks=S, num_ch=M).separate_recording(sc.wav, fs=FS)
    assert pcm.dtype == np.int16 and pcm.shape == (S, L) and pcm.any()
    pcm2 = BlindSeparator(num_spks=S, num_ch=M).separate_recording(dry, fs=FS)
    assert pcm2.dtype == np.int16 and pcm2.shape == (S, L) and pcm2.any()
