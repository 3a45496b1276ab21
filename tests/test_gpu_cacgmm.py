"""GPU tests of the guided cACGMM (csrc/cacgmm.hip, ``misonet_amd.refine``, the fused pass with ``refine`` set) against the
float64 NumPy restatement of tests/cacgmm_ref.py: masks, images, B_k, pi and the log-likelihood on every shape that takes
another path (below one tile, the smallest and the largest K and M, odd M, exactly one tile, one tile plus one frame, several
tiles), both priors, one and ten iterations; the masks of the estimates; zero iterations; empty frames; the failure rule;
bit-reproducibility and independence of the batch; buffers full of NaN; and the fused pass, its captured graph and the
beamform_* methods against the drop-in composition.

Bars (tests/cacgmm_ref.py ``figures``).  Masks: max-abs <= 2.4e-7 = 4 x 2^-24 (they lie in [0, 1]: one float32 rounding is
<= 2^-25; tests/test_cacgmm.py asserts that the float64 path's own sensitivity on these inputs is below 1e-10).  Images: rel-L2
<= 2.4e-7, one complex64 rounding.  B_k, pi, log-likelihood: rel-L2 <= 100 x the restatement's permuted-order difference on
that case, never below 1e-12.  The module prints every figure (``[cacgmm] ...``); LAB.md has them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cacgmm_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
IDS = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return R.case_inputs(shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, prior, iterations):
    """(the restatement, the restatement with the frames summed in a permuted order), computed once per case"""
    mix, init, _ = _inputs(shape)
    order = np.random.default_rng(5).permutation(shape[3])
    return R.cacgmm(mix, init, iterations, prior), R.cacgmm(mix, init, iterations, prior, frame_order=order)


def _run(mix, init, **kw):
    from misonet_amd.refine import cacgmm
    masks, images, dbg = cacgmm(torch.from_numpy(mix).cuda(), torch.from_numpy(init).cuda(), return_images=True,
                                return_debug=True, **kw)
    out = dict(masks=masks.cpu().numpy(), images=images.cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in dbg.items()})
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[x.dtype.itemsize])


def _same(a, b, names=("masks", "images", "B", "pi", "ll", "fail")):
    return all(np.array_equal(_bits(a[n]), _bits(b[n])) for n in names)


@pytest.mark.parametrize("iterations", [1, 10])
@pytest.mark.parametrize("prior", ["bin", "guided"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_against_restatement(shape, prior, iterations):
    _need_gpu()
    mix, init, _ = _inputs(shape)
    want, perm = _ref(shape, prior, iterations)
    got = _run(mix, init, iterations=iterations, prior=prior)
    fig = R.figures(got, want, perm)
    print(f"[cacgmm] {shape} {prior} {iterations} it: " + "  ".join(f"{k} {v:.3e} (bar {b:.3e})" for k, (v, b) in fig.items()))
    assert got["masks"].dtype == np.float32 and got["images"].dtype == np.complex64
    assert got["masks"].shape == want["masks"].shape and got["images"].shape == want["images"].shape
    assert not want["fail"].any() and not got["fail"].any()
    assert not R.missed(fig), fig


def test_masks_from_estimates():
    """against NumPy, a zero total included.  Bar: 2^-23 max-abs -- the values lie in [0, 1] and are float64 quotients rounded
    to float32 once on either side (<= 2^-25 each); where the roundings fall apart they differ by one float32 step (<= 2^-24)"""
    _need_gpu()
    from misonet_amd.refine import masks_from_estimates
    for shape in (R.SHAPES[0], R.SHAPES[5]):
        mix, _, est = (x.copy() for x in _inputs(shape))
        est[0, :, 1, :, 7] = 0
        mix[0, 1, :, 7] = 0
        want = R.masks_from_estimates(est, mix)
        got = masks_from_estimates(torch.from_numpy(est).cuda(), torch.from_numpy(mix).cuda())
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
        got = got.cpu().numpy()
        e = R.max_abs(got, want)
        print(f"[cacgmm] masks_from_estimates {shape}: max-abs {e:.3e} (bar {2.0 ** -23:.3e})")
        assert e <= 2.0 ** -23
        assert np.all(got[0, :, 1, 7] == np.float32(1.0 / 3))
    # one speaker, two microphones, ndarrays in: half the mixture as the estimate
    mix, _, _ = _inputs(R.SHAPES[1])
    est = (0.5 * mix)[:, None]
    assert R.max_abs(masks_from_estimates(est, mix).numpy(), R.masks_from_estimates(est, mix)) <= 2.0 ** -23


def test_zero_iterations_returns_the_initial_masks():
    _need_gpu()
    mix, init, _ = _inputs(R.SHAPES[2])
    got = _run(mix, init, iterations=0)
    assert np.array_equal(_bits(got["masks"]), _bits(init)) and not got["fail"].any() and not got["B"].any()
    assert R.rel(got["images"], init[:, :2, :, None, :].astype(np.float64) * mix[:, None]) <= R.OUT_BAR


@pytest.mark.parametrize("prior", ["bin", "guided"])
def test_empty_frames(prior):
    """a zero tail of 7 frames: the frames before it carry the bits of the same input cut to them, the tail its initial masks;
    isolated zero frames inside a tile: their initial masks bit for bit, the others inside the bar"""
    _need_gpu()
    shape = R.SHAPES[2]
    B, S, M, T, F = shape
    mix, init, _ = (x.copy() if x is not None else None for x in _inputs(shape))
    mix[..., T - 7:] = 0
    full = _run(mix, init, prior=prior)
    cut = _run(np.ascontiguousarray(mix[..., :T - 7]), np.ascontiguousarray(init[..., :T - 7]), prior=prior)
    assert not full["fail"].any() and np.abs(full["masks"] - init)[..., :T - 7].max() > 1e-3
    assert np.array_equal(_bits(full["masks"][..., :T - 7]), _bits(cut["masks"]))
    assert np.array_equal(_bits(full["images"][..., :T - 7]), _bits(cut["images"]))
    assert _same(full, cut, ("B", "pi", "ll", "fail"))
    assert np.array_equal(_bits(full["masks"][..., T - 7:]), _bits(init[..., T - 7:])) and not full["images"][..., T - 7:].any()
    holes = [5, 17, 18, 40, 63, 64]
    mix[..., holes] = 0
    want = R.cacgmm(mix, init, 10, prior)
    perm = R.cacgmm(mix, init, 10, prior, frame_order=np.random.default_rng(5).permutation(T))
    got = _run(mix, init, prior=prior)
    fig = R.figures(got, want, perm)
    print(f"[cacgmm] empty frames {shape} {prior}: " + "  ".join(f"{k} {v:.3e} (bar {b:.3e})" for k, (v, b) in fig.items()))
    assert np.array_equal(_bits(got["masks"][..., holes]), _bits(init[..., holes]))
    assert not got["fail"].any() and not R.missed(fig), fig


def test_failure_rule():
    """an all-zero bin and a class with an all-zero initial mask: fail = 1 and the initial masks there, the other bins as
    without them"""
    _need_gpu()
    shape = R.SHAPES[0]
    B, S, M, T, F = shape
    mix, init, _ = (x.copy() if x is not None else None for x in _inputs(shape))
    base = _run(mix, init)
    mix[1, 4] = 0
    init[0, 1, 2] = 0
    got = _run(mix, init)
    flags = np.zeros((B, F), np.int32)
    flags[1, 4] = flags[0, 2] = 1
    assert np.array_equal(got["fail"], flags) and np.array_equal(R.cacgmm(mix, init, 10)["fail"], flags)
    for b, f in ((1, 4), (0, 2)):
        assert np.array_equal(_bits(got["masks"][b, :, f]), _bits(init[b, :, f]))
        assert not got["B"][b, f].any() and not got["pi"][b, f].any() and got["ll"][b, f] == 0
    assert not got["images"][1, :, 4].any()                                    # the images of the initial masks: of Y = 0 ...
    assert R.rel(got["images"][0, :, 2], init[0, :2, 2, None, :].astype(np.float64) * mix[0, 2][None]) <= R.OUT_BAR
    keep = flags == 0
    for name in ("B", "pi", "ll"):
        assert np.array_equal(_bits(got[name][keep]), _bits(base[name][keep])), name
    assert np.array_equal(_bits(got["masks"].transpose(0, 2, 1, 3)[keep]), _bits(base["masks"].transpose(0, 2, 1, 3)[keep]))


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    mix, est, init = R.reverberant_inputs(3, 4, 150, 9)
    a = _run(mix, init, prior="guided")
    b = _run(mix, init, prior="guided")
    assert _same(a, b) and not a["fail"].any()
    for i in range(3):
        one = _run(np.ascontiguousarray(mix[i:i + 1]), np.ascontiguousarray(init[i:i + 1]), prior="guided")
        for n in ("masks", "images", "B", "pi", "ll"):
            assert np.array_equal(_bits(a[n][i]), _bits(one[n][0])), (i, n)


def test_nan_buffers_change_nothing():
    """a workspace and output buffers that held NaN before the call: the same bits as with zeros; and the argument checks of
    the library on the device as without one"""
    _need_gpu()
    from misonet_amd import _lib
    shape = R.SHAPES[2]
    B, S, M, T, F = shape
    K = S + 1
    mix, init, _ = _inputs(shape)
    y, g0 = torch.from_numpy(mix).cuda(), torch.from_numpy(init).cuda()
    L = _lib.lib()
    o = _lib.CacgmmOpts(10, 1, 1e-8, 1e-6)
    n = L.misonet_cacgmm_workspace_bytes(B, K, F, M)
    st = _lib.stream_ptr(y.device)
    got = []
    for fill in (0.0, float("nan")):
        ws = torch.full((n // 8 + 1,), fill, dtype=torch.float64, device="cuda")
        masks = torch.full((B, K, F, T), fill, dtype=torch.float32, device="cuda")
        images = torch.full((B, S, F, M, T), fill, dtype=torch.complex64, device="cuda")
        dbg = dict(B=torch.empty((B, F, K, M, M), dtype=torch.complex128, device="cuda"),
                   pi=torch.empty((B, F, K), dtype=torch.float64, device="cuda"),
                   ll=torch.empty((B, F), dtype=torch.float64, device="cuda"),
                   fail=torch.empty((B, F), dtype=torch.int32, device="cuda"))
        _lib.check(L.misonet_cacgmm(y.data_ptr(), g0.data_ptr(), B, K, F, M, T, C.byref(o), masks.data_ptr(),
                                    images.data_ptr(), ws.data_ptr(), n, st))
        _lib.check(L.misonet_cacgmm_debug(ws.data_ptr(), B, K, F, M, dbg["B"].data_ptr(), dbg["pi"].data_ptr(),
                                          dbg["ll"].data_ptr(), dbg["fail"].data_ptr(), st))
        r = dict(masks=masks.cpu().numpy(), images=images.cpu().numpy())
        r.update({k: v.cpu().numpy() for k, v in dbg.items()})
        got.append(r)
    assert np.isfinite(got[0]["masks"]).all() and np.isfinite(got[0]["images"]).all() and not got[0]["fail"].any()
    assert _same(got[0], got[1])
    assert L.misonet_cacgmm(y.data_ptr(), g0.data_ptr(), B, K, F, M, T, C.byref(o), masks.data_ptr(), None, ws.data_ptr(), n - 1,
                            st) == _lib.ENOMEM
    assert L.misonet_cacgmm(y.data_ptr(), g0.data_ptr(), B, K, F, M, T, C.byref(o), g0.data_ptr(), None, ws.data_ptr(), n,
                            st) == _lib.EINVAL


def test_numpy_in_numpy_out():
    _need_gpu()
    from misonet_amd.refine import cacgmm, masks_from_estimates
    shape = R.SHAPES[1]
    mix, init, _ = _inputs(shape)
    masks, images = cacgmm(mix, init, return_images=True)
    assert isinstance(masks, torch.Tensor) and masks.device.type == "cpu" and masks.dtype == torch.float32
    assert images.device.type == "cpu" and images.dtype == torch.complex64
    assert R.max_abs(masks.numpy(), _ref(shape, "bin", 10)[0]["masks"]) <= R.MASK_BAR
    g = masks_from_estimates((0.5 * mix)[:, None], mix)
    assert g.device.type == "cpu" and g.dtype == torch.float32 and tuple(g.shape) == (1, 2, 5, 40)
    only = cacgmm(torch.from_numpy(mix).cuda(), torch.from_numpy(init).cuda(), refine=dict(iterations=10))
    assert only.is_cuda and torch.equal(only.cpu(), masks)


# ---- the fused pass ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(sd1, sd3):
    """seed weights in the library's default arithmetic"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN")
    m1.cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN")
    m3.cuda(0)
    m3.load_state_dict(sd3)
    return m1.eval(), m3.eval()


def _chunks(B, T):
    from misonet_amd import stft as S
    from misonet_amd.weights import synthetic_utterance
    n = 64 * (T - 1)
    wav = np.stack([synthetic_utterance(31 + b, n)[0] for b in range(B)])                    # [B, n, 6]
    return S.stft_hip(torch.from_numpy(wav.astype(np.float32)).cuda()).contiguous()          # [B, 6, T, 129]


def _eq(a, b):
    return torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_fused_pass(nets):
    """step 4b of the fused pass is the drop-in composition through other views: the same bits, for souden and for wpd; a
    captured graph replays them; set_refine(None) restores the bits and the workspace size from before; beamform_chunks
    honours it"""
    import misonet_amd as mz
    from misonet_amd.beamform import Apply_Beamforming
    from misonet_amd.refine import Refine, cacgmm, masks_from_estimates
    m1, m3 = nets
    B, T = 2, 40
    mix = _chunks(B, T)
    mix_bf = mix.permute(0, 3, 1, 2)                                                         # [B, F, M, T]
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    out0, d0 = enh.enhance(mix, want_bf=True, want_miso1=True)
    n0 = enh.workspace(B, T).numel()
    rf = dict(iterations=3, prior="guided")
    for spec in (dict(kind="souden", ref_ch=1), dict(kind="wpd", taps=3, delay=2)):
        enh.set_beamformer(spec)
        enh.set_refine(None)
        plain = enh.enhance(mix, want_bf=True)[1]["bf"]
        n_plain = enh.workspace(B, T).numel()
        enh.set_refine(rf)
        assert enh.refine == Refine(**rf) and enh.workspace(B, T).numel() > n_plain
        out1, d1 = enh.enhance(mix, want_bf=True, want_miso1=True)
        assert torch.isfinite(torch.view_as_real(d1["bf"])).all() and not _eq(d1["bf"], plain)
        assert _eq(d1["miso1"], d0["miso1"])                                                 # the raw MISO1 estimate stays
        est = d1["miso1"].permute(0, 1, 4, 2, 3)                                             # [B, S, F, M, T]
        images = cacgmm(mix_bf, masks_from_estimates(est, mix_bf), return_images=True, refine=rf)[1]
        for s in range(2):
            assert _eq(d1["bf"][:, s], Apply_Beamforming(images[:, s], mix_bf, beamformer=spec)), (spec, s)
        assert _eq(enh.beamform_chunks(mix), d1["bf"]), spec
    # a captured graph replays the same bits, and refuses a change while it lives
    cp = enh.capture_graph(mix)
    cp.out.zero_()
    cp.graph.replay()
    torch.cuda.synchronize()
    assert _eq(cp.out, out1)
    with pytest.raises(RuntimeError):
        enh.set_refine(None)
    del cp
    with pytest.raises(ValueError):
        enh.set_refine(dict(iterations=-1))
    # back: the bits and the workspace size from before
    enh.set_refine(None)
    enh.set_beamformer(None)
    out2, d2 = enh.enhance(mix, want_bf=True)
    assert _eq(out2, out0) and _eq(d2["bf"], d0["bf"]) and enh.workspace(B, T).numel() == n0


def test_beamform_utterance_honours_refine(nets):
    """the utterance-wise path: one clustering over the whole recording's frames, then one beamformer per speaker"""
    import misonet_amd as mz
    from misonet_amd import stft as S
    from misonet_amd.beamform import Apply_Beamforming
    from misonet_amd.refine import cacgmm, masks_from_estimates
    m1, m3 = nets
    K, T = 2, 40
    obs = _chunks(K, T)
    clean = obs[:, :2].contiguous()                      # stand-ins for the clean references: they only order the speakers
    rf = dict(iterations=2)
    enh = mz.Enhancer(m1, None, num_spks=2, ref_ch=0, refine=rf)
    gap = 100
    got = enh.beamform_utterance(list(obs), list(clean), gap, to_host=False)
    est = enh.separate(obs, clean)
    e, o = S.istft(est), S.istft(obs)
    n = e.shape[-1]
    keep = [n, n - gap]
    est_t = torch.cat([e[k, ..., :keep[k]] for k in range(K)], dim=-1)
    obs_t = torch.cat([o[k, ..., :keep[k]] for k in range(K)], dim=-1)
    pad = (-obs_t.shape[-1]) % S.HOP
    sig = torch.nn.functional.pad(torch.cat([obs_t[None], est_t], dim=0), (0, pad)).permute(0, 2, 1).contiguous()
    spec = S.stft_hip(sig)
    mix_bf = spec[0].permute(2, 0, 1)[None]
    src = spec[1:].permute(0, 3, 1, 2)[None]
    images = cacgmm(mix_bf, masks_from_estimates(src, mix_bf), return_images=True, refine=rf)[1]
    bf = torch.stack([Apply_Beamforming(images[:, s], mix_bf)[0] for s in range(2)])
    assert torch.equal(got, S.istft_int16(bf))
    enh.set_refine(None)
    raw = enh.beamform_utterance(list(obs), list(clean), gap, to_host=False)
    assert raw.shape == got.shape and not torch.equal(raw, got)
