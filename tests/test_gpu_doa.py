"""GPU tests of the source localisation (csrc/doa.hip, ``misonet_amd.localize``) against the float64 NumPy restatement of
tests/doa_ref.py: ``misonet_doa`` itself, on outputs and a workspace that held NaN, at every case of ``doa_ref.gpu_cases`` -- D
around the steering tile, bands around the bin chunk, one-bin bands at F 1, 2 and 129, M 2 .. 8, every S music admits at M 3 and
6, T around the frame chunk, four block / hop pairs, B, K and Bg 1 and 3, weights absent, random and zero on one class -- for all
three kinds; the behaviour at NaN, silence, rank-1 bins and equal candidates; bit-reproducibility, independence of the batch, a
captured HIP graph, absent weights against ones; and ``room.simulate`` end to end into ``localize_wav`` and AuxIVA images.

Bars.  q: rel-L2 and the worst candidate's error relative to max q - min q, each <= max(100 x the restatement's own difference
under a permuted frame order on that case, 1e-12).  used and fail equal; peak equal wherever the restatement's margin to the next
candidate exceeds 1e-9 of the range, and every case has that margin (a flat map ties to the lower index on both sides).  The
module prints every figure (``[doa] ...``); LAB.md has them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import doa_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
FS = 16000.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _consts():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return int(_lib.lib().misonet_doa_tile()), int(_lib.lib().misonet_doa_bin_chunk())


TILE, CHUNK = _consts()
CASES = R.gpu_cases(TILE, CHUNK)
CASE_ID = lambda c: c["tag"]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _nan_like(shape, dtype):
    """a device tensor whose every byte is 0xff: NaN as float64, -1 as int32"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((max(n, 1),), 255, dtype=torch.uint8, device="cuda")[:n].view(dtype).reshape(shape)


class _Call:
    """the device buffers of one ``misonet_doa`` call; ``run`` launches it on the current stream, ``host`` reads everything"""

    def __init__(self, mix, weight, tau, pts, kind, S, block=0, hop=0, f_lo=0, f_hi=-1, min_sep=0.0, fs=FS):
        from misonet_amd import _lib
        self.L = _lib
        B, F, M, T = mix.shape
        tau = np.asarray(tau, np.float64)
        tau = tau[None] if tau.ndim == 2 else tau
        self.dims = (B, 1 if weight is None else weight.shape[1], F, M, T, tau.shape[1])
        B, K, F, M, T, D = self.dims
        self.Bg, self.fs, self.S = tau.shape[0], float(fs), S
        self.opts = _lib.DoaOpts(R.KINDS.index(kind), S, block, hop, f_lo, f_hi, float(min_sep))
        lib = _lib.lib()
        self.N = lib.misonet_doa_blocks(T, block, hop)
        nws = lib.misonet_doa_workspace_bytes(B, K, F, M, T, D, C.byref(self.opts))
        assert self.N >= 1 and nws > 0, (self.N, nws)
        self.mix = torch.from_numpy(np.ascontiguousarray(mix, np.complex64)).cuda()
        self.w = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight, np.float32)).cuda()
        self.tau = torch.from_numpy(np.ascontiguousarray(tau)).cuda()
        self.pts = torch.from_numpy(np.ascontiguousarray(pts, np.float64)).cuda()
        self.ws = _nan_like((nws,), torch.uint8)
        self.q = _nan_like((B, K, self.N, D), torch.float64)
        self.peak = _nan_like((B, K, self.N, S), torch.int32) - 6
        self.value = _nan_like((B, K, self.N, S), torch.float64)
        self.fail = _nan_like((B, K, self.N), torch.int32) - 6
        self.used = _nan_like((B, K, self.N), torch.int32) - 6
        self.c = _nan_like((B, K, self.N, F, M, M), torch.complex128)

    def run(self):
        B, K, F, M, T, D = self.dims
        lib = self.L.lib()
        st = self.L.stream_ptr(self.q.device)
        self.L.check(lib.misonet_doa(self.mix.data_ptr(), None if self.w is None else self.w.data_ptr(), self.tau.data_ptr(),
                                     self.Bg, self.pts.data_ptr(), B, K, F, M, T, D, self.fs, C.byref(self.opts), self.q.data_ptr(),
                                     self.peak.data_ptr(), self.value.data_ptr(), self.fail.data_ptr(), self.ws.data_ptr(),
                                     self.ws.numel(), st))
        self.L.check(lib.misonet_doa_debug(self.ws.data_ptr(), B, K, F, M, T, D, C.byref(self.opts), self.c.data_ptr(),
                                           self.used.data_ptr(), None, st))
        return self

    def host(self):
        return dict(q=self.q.cpu().numpy(), peak=self.peak.cpu().numpy(), value=self.value.cpu().numpy(),
                    fail=self.fail.cpu().numpy(), used=self.used.cpu().numpy(), C=self.c.cpu().numpy())


def _raw(*a, **kw):
    return _Call(*a, **kw).run().host()


@functools.lru_cache(maxsize=None)
def _inputs(idx):
    return R.case_inputs(CASES[idx])


@functools.lru_cache(maxsize=None)
def _ref(idx, kind):
    """(the restatement, its q under a permuted frame order), computed once per case and kind"""
    c = CASES[idx]
    mix, w, tau, pts = _inputs(idx)
    kw = dict(S=R.case_kind_S(c, kind), block=c["block"], hop=c["hop"], f_lo=c["f_lo"], f_hi=c["f_hi"], min_sep=c["min_sep"],
              weight=w)
    want = R.localize(mix, tau, pts, FS, kind, **kw)
    return want, R.cov_steer(mix, tau, FS, kind, frame_order=5, **{k: v for k, v in kw.items() if k != "min_sep"})


def _hold(tag, got, want, perm_q):
    """the bars of the module's docstring on one result"""
    assert got["q"].shape == want["q"].shape and np.isfinite(got["q"]).all() and np.isfinite(got["value"]).all()
    fig = R.figures(got["q"], want["q"], perm_q)
    margin = float(want["margin"].min())
    print(f"[doa] {tag}: " + "  ".join(f"{k} {v:.3e} (bar {bar:.3e})" for k, (v, bar) in fig.items()) +
          f"  margin {margin:.2e}  used {int(want['used'].min())}..{int(want['used'].max())}")
    assert not R.missed(fig), fig
    assert np.array_equal(got["used"], want["used"]) and np.array_equal(got["fail"], want["fail"])
    assert margin > R.PEAK_MARGIN, margin
    assert np.array_equal(got["peak"], want["peak"]), (got["peak"], want["peak"])
    sel = want["peak"] >= 0
    picked = np.take_along_axis(got["q"], np.maximum(got["peak"], 0).astype(np.int64), axis=-1)
    assert np.array_equal(_bits(got["value"][sel]), _bits(picked[sel])) and not got["value"][~sel].any()
    on = want["state"] == 0
    assert not got["C"][~on].any()                                      # skipped and out-of-band bins hold zeros
    if on.any():
        cerr = np.abs(got["C"][on] - want["C"][on]).max() / np.abs(want["C"][on]).max()
        print(f"[doa] {tag}: C worst element {cerr:.3e}")
        assert cerr <= 1e-10, cerr                                      # the map's bars judge; this catches a wrong matrix early


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[CASE_ID(c) for c in CASES])
def test_against_restatement(idx, kind):
    _need_gpu()
    c = CASES[idx]
    mix, w, tau, pts = _inputs(idx)
    want, perm_q = _ref(idx, kind)
    got = _raw(mix, w, tau, pts, kind, R.case_kind_S(c, kind), c["block"], c["hop"], c["f_lo"], c["f_hi"], c["min_sep"])
    _hold(f"{c['tag']} {kind}", got, want, perm_q)


# ---- behaviour --------------------------------------------------------------------------------------------------------------------
def _small(seed=3, B=1, F=17, M=4, T=20, D=37):
    return R.case_inputs(dict(B=B, K=1, Bg=1, F=F, M=M, T=T, D=D, weights="none", seed=seed))


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_bin_of_nan_is_skipped_and_flagged(kind):
    _need_gpu()
    mix, _, tau, pts = _small()
    mix = mix.copy()
    mix[0, 5, 2, 7] = np.nan
    mix[0, 9, 0, 19] = np.inf + 0j
    w = np.ones((1, 2, 17, 20), np.float32)
    w[0, 1, 11, 3] = np.nan                                             # a weight of class 1 only
    kw = dict(block=10, hop=10, f_lo=1, f_hi=15, min_sep=0.3)
    got = _raw(mix, w, tau, pts, kind, 1, **kw)
    want = R.localize(mix, tau, pts, FS, kind, 1, weight=w, **kw)
    assert want["used"].tolist() == [[[14, 14], [13, 14]]] and want["fail"].tolist() == [[[1, 1], [1, 1]]]
    _hold(f"nan {kind}", got, want, R.cov_steer(mix, tau, FS, kind, S=1, weight=w, frame_order=5, block=10, hop=10, f_lo=1, f_hi=15))


@pytest.mark.parametrize("kind", R.KINDS)
def test_silence_gives_fail_2_and_a_zero_map(kind):
    _need_gpu()
    mix, _, tau, pts = _small(B=2)
    mix = mix.copy()
    mix[1] = 0
    got = _raw(mix, None, tau, pts, kind, 2, min_sep=0.3)
    assert got["fail"].ravel().tolist() == [0, 2] and got["used"].ravel().tolist() == [17, 0]
    assert not got["q"][1].any() and got["q"][0].any() and got["peak"][1].ravel().tolist() == [0, 2]    # candidate 1 is within 0.3


def test_a_rank_one_bin_is_skipped_by_music_with_two_sources():
    _need_gpu()
    mix, _, tau, pts = _small(T=12)
    mix = mix.copy()
    mix[0, 4] = np.outer(mix[0, 4, :, 0], np.exp(1j * np.arange(12))).astype(np.complex64)           # one direction in every frame
    got = _raw(mix, None, tau, pts, "music", 2, min_sep=0.3)
    want = R.localize(mix, tau, pts, FS, "music", 2, min_sep=0.3)
    assert want["state"][0, 0, 0, 4] == 2 and want["used"].item() == 16 and got["used"].item() == 16 and got["fail"].item() == 0
    assert not got["C"][0, 0, 0, 4].any()
    one = _raw(mix, None, tau, pts, "music", 1, min_sep=0.3)
    assert one["used"].item() == 17 and one["C"][0, 0, 0, 4].any()


@pytest.mark.parametrize("kind", R.KINDS)
def test_of_two_identical_candidates_the_lower_index_wins(kind):
    _need_gpu()
    mix, _, tau, pts = _small()
    best = int(R.localize(mix, tau, pts, FS, kind, 1)["peak"].item())
    twin = (best + 11) % 37
    tau, pts = tau.copy(), pts.copy()
    tau[0, twin], pts[twin] = tau[0, best], pts[best]
    got = _raw(mix, None, tau, pts, kind, 2, min_sep=0.0)
    assert got["peak"].ravel().tolist() == sorted([best, twin]), (got["peak"], best, twin)
    assert _bits(got["value"]).ravel()[0] == _bits(got["value"]).ravel()[1]
    far = _raw(mix, None, tau, pts, kind, 2, min_sep=0.2)                # with a separation the twin is retired with its peak
    assert far["peak"].ravel()[0] == min(best, twin) and far["peak"].ravel()[1] not in (best, twin)


@pytest.mark.parametrize("kind", R.KINDS)
def test_bit_reproducible_batch_invariant_graph_and_unit_weights(kind):
    _need_gpu()
    c = dict(B=3, K=1, Bg=3, F=33, M=5, T=70, D=TILE + 5, weights="none", seed=11)
    mix, _, tau, pts = R.case_inputs(c)
    kw = dict(block=32, hop=16, f_lo=2, f_hi=2 + CHUNK, min_sep=0.3)
    S = 2
    a = _raw(mix, None, tau, pts, kind, S, **kw)
    b = _raw(mix, None, tau, pts, kind, S, **kw)
    for k in ("q", "value", "C"):
        assert np.array_equal(_bits(a[k].view(np.float64) if k == "C" else a[k]), _bits(b[k].view(np.float64) if k == "C" else b[k])), k
    assert np.array_equal(a["peak"], b["peak"]) and np.array_equal(a["used"], b["used"]) and np.array_equal(a["fail"], b["fail"])
    for i in range(3):                                                   # a recording alone = the same recording in the batch
        one = _raw(mix[i:i + 1], None, tau[i:i + 1], pts, kind, S, **kw)
        assert np.array_equal(_bits(one["q"][0]), _bits(a["q"][i])) and np.array_equal(one["peak"][0], a["peak"][i]), i
        assert np.array_equal(_bits(one["value"][0]), _bits(a["value"][i]))
    ones = _raw(mix, np.ones((3, 1, 33, 70), np.float32), tau, pts, kind, S, **kw)
    assert np.array_equal(_bits(ones["q"]), _bits(a["q"])) and np.array_equal(ones["peak"], a["peak"])
    call = _Call(mix, None, tau, pts, kind, S, **kw)                     # a captured graph's replay = the eager call
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call.run()                                                       # warm-up on the side stream
        stream.synchronize()
        call.q.fill_(float("nan"))
        call.peak.fill_(-9)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            call.run()
        call.q.fill_(float("nan"))
        call.peak.fill_(-9)
        graph.replay()
        stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    g = call.host()
    assert np.array_equal(_bits(g["q"]), _bits(a["q"])) and np.array_equal(g["peak"], a["peak"])
    assert np.array_equal(_bits(g["value"]), _bits(a["value"])) and np.array_equal(g["fail"], a["fail"])


def test_python_surface_matches_the_raw_call():
    _need_gpu()
    from misonet_amd import localize as LZ
    c = dict(B=2, K=2, Bg=1, F=33, M=4, T=24, D=37, weights="random", seed=5)
    mix, w, tau, pts = R.case_inputs(c)
    raw = _raw(mix, w, tau, pts, "music", 2, 8, 4, 2, 30, 0.3)
    res, cm = LZ.localize(mix, tau[0], pts, FS, kind="music", num_src=2, block=8, hop=4, bins=(2, 30), min_sep=0.3, weight=w,
                          return_debug=True)
    assert isinstance(res.q, np.ndarray) and res.q.shape == (2, 2, 5, 37) and res.peak.dtype == np.int32
    for k in ("q", "value"):
        assert np.array_equal(_bits(getattr(res, k)), _bits(raw[k])), k
    assert np.array_equal(res.peak, raw["peak"]) and np.array_equal(res.used, raw["used"]) and np.array_equal(res.fail, raw["fail"])
    assert np.array_equal(cm, raw["C"]) and np.array_equal(res.map, 1.0 / np.maximum(res.q, 1e-12))
    dev = LZ.localize(torch.from_numpy(mix).cuda(), tau, pts, FS, localizer=dict(kind="srp", band=(500.0, 7500.0)))
    assert isinstance(dev.q, torch.Tensor) and dev.q.is_cuda and dev.map is dev.q and dev.q.shape == (2, 1, 1, 37)
    img = np.stack([mix, mix[::-1]], axis=1)                             # images [B, S, F, M, T] run as B S recordings
    r5 = LZ.localize(img, tau, pts, FS, kind="srp_phat")
    r4 = LZ.localize(mix, tau, pts, FS, kind="srp_phat")
    assert r5.q.shape == (2, 2, 1, 1, 37) and np.array_equal(_bits(r5.q[:, 0]), _bits(r4.q))
    assert np.array_equal(_bits(r5.q[:, 1]), _bits(r4.q[::-1]))
    with pytest.raises(ValueError):
        LZ.localize(mix, tau, pts, FS, num_src=0)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
E2E_FS, E2E_SEED, E2E_D = 8000, 0, 72


def _e2e_scene(seed):
    """an anechoic room (beta = 0), six microphones on a 5 cm circle, two sources 1.5 m away on grid azimuths at least 30
    degrees apart, 2 s of the golden dry speech, 25 dB SNR"""
    from misonet_amd import room as RM
    rng = np.random.default_rng(seed)
    dry = np.load(os.path.join(ROOT, "tests", "golden", "g16_stoi.npz"))["clean"].astype(np.float32)[:, 8000:24000]
    centre = np.array([3.0, 2.5, 1.2])
    while True:
        idx = np.sort(rng.choice(E2E_D, 2, replace=False))
        if R.grid_distance(idx[0], idx[1], E2E_D) >= 6:
            break
    dirs = R.azimuths(E2E_D)
    src = centre + 1.5 * dirs[idx]
    mic = centre + R.circle(6)
    sc = RM.simulate(dry, RM.Room((6.0, 5.0, 2.8), beta=(0.0,) * 6), src, mic, E2E_FS, 512, snr_db=25.0, seed=seed)
    return sc, mic, dirs, idx


def _stft_dev(wav):
    from misonet_amd import stft as S
    sig = torch.from_numpy(np.ascontiguousarray(wav, np.float32)).cuda()
    sig = torch.nn.functional.pad(sig, (0, 0, 0, (-sig.shape[0]) % S.HOP))[None].contiguous()
    return S.stft_hip(sig).permute(0, 3, 1, 2).contiguous()              # [1, F, M, T]


def test_simulated_room_into_localize_wav_music():
    _need_gpu()
    from misonet_amd import localize as LZ
    sc, mic, dirs, truth = _e2e_scene(E2E_SEED)
    tau = LZ.far_field_delays(mic, dirs)
    sep = 2.0 * np.sin(np.radians(12.5))
    kw = dict(f_lo=8, f_hi=100, min_sep=sep)
    spec = _stft_dev(sc.wav).cpu().numpy()
    want = R.localize(spec, tau, dirs, float(E2E_FS), "music", 2, **kw)
    found = np.sort(want["peak"][0, 0, 0])
    print(f"[doa] e2e music seed {E2E_SEED}: truth {truth.tolist()} restatement {found.tolist()}")
    assert (R.grid_distance(found, truth, E2E_D) <= 1).all(), (found, truth)       # the restatement finds the truth ...
    res, cm = LZ.localize_wav(sc.wav, tau, dirs, E2E_FS, kind="music", num_src=2, bins=(8, 100), min_sep=sep, return_debug=True)
    got = dict(q=res.q, peak=res.peak, value=res.value, used=res.used, fail=res.fail, C=cm)
    perm = R.cov_steer(spec, tau, float(E2E_FS), "music", S=2, frame_order=5, f_lo=8, f_hi=100)
    _hold("e2e music", got, want, perm)                                             # ... and the device equals the restatement
    err = LZ.angular_error(dirs, res.peak[0, 0, 0], truth)
    print(f"[doa] e2e music angular error {err.tolist()} degrees")
    assert (err <= 5.0 + 1e-9).all()


def test_auxiva_images_into_srp_phat():
    _need_gpu()
    from misonet_amd import localize as LZ
    from misonet_amd.blind import auxiva
    sc, mic, dirs, truth = _e2e_scene(E2E_SEED)
    tau = LZ.far_field_delays(mic, dirs)
    images = auxiva(_stft_dev(sc.wav), 2)                                # [1, 2, F, M, T] on the device
    res, cm = LZ.localize(images, tau, dirs, float(E2E_FS), kind="srp_phat", bins=(8, 100), return_debug=True)
    assert res.q.shape == (1, 2, 1, 1, E2E_D)
    img = images.cpu().numpy()[0]                                        # [2, F, M, T]: two recordings
    want = R.localize(img, tau, dirs, float(E2E_FS), "srp_phat", 1, f_lo=8, f_hi=100)
    perm = R.cov_steer(img, tau, float(E2E_FS), "srp_phat", S=1, frame_order=5, f_lo=8, f_hi=100)
    got = {k: getattr(res, k).cpu().numpy()[0] for k in ("q", "peak", "value", "used", "fail")}
    got["C"] = cm.cpu().numpy()[0]
    print(f"[doa] e2e auxiva + srp_phat: truth {truth.tolist()} found {np.sort(got['peak'].ravel()).tolist()}")
    _hold("e2e auxiva srp_phat", got, want, perm)
