"""The 3x3 conv stack (csrc/conv.hip, conv_wino.hip, conv_bf16x6.hip, conv_few.hip, conv_epilogue.hpp) level by level on its OWN
input against the float64 oracle, at the frame counts where the tiling starts to matter; with a workspace whose previous contents
are NaN; and bit for bit across the tile-walk variants that the batch size selects.

a. One GPU forward of MISO_1 per case with kept activations; all taps are read back.  For each of the 15 conv steps (the first
   conv, 7 encoder levels, 7 decoder levels) the step's input is the GPU's own tap in front of it (a decoder level: the previous
   tap and the matching encoder tap), and on the CPU ``miso_oracle``'s level runs on that input in float64 (the truth) and in
   float32 (the yardstick).  The levels in front are the GPU's own, so their error is not part of what is measured, and the bound
   can be the one of tests/conv_ref.py: K = 4 times the float32 oracle's own distance from the truth, for the whole tensor, the
   worst frame, the worst frequency row and the worst channel (tests/test_conv_levels.py shows that this bound rejects a stale
   halo frame or row, a lost statistics tile, another sample's statistics, a 16-bit product, a lost second-order bf16 group and
   padding frames in the statistics).  Measured ratios: LAB.md, "Conv levels on their own input".
b. The workspace is ``torch.empty``: filled with 0xFF bytes (NaN as float32, bf16 and float64) or with zeros before the forward,
   the output and every tap are the same bits.
c. A sample inside a batch equals the same sample run alone, bit for bit at every tap, at the batch sizes that switch the tile
   walk of every conv kernel.

Everything here runs the default channel widths; tests/test_gpu_conv_widths.py holds the same three properties at other widths.
"""
import numpy as np
import pytest
import torch

import conv_ref
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

MODES = ("f32", "f32w", "bf16x6")
FRAMES = [
    64,       # one full Winograd tile, T == Tp: the halo frame is the next row's first word
    65,       # the second Winograd tile holds one frame = half a 2-frame Winograd tile; Tp = 96
    128,      # one full 128-frame tile of DIRECT / W1D / X6 / FEW, T == Tp
    129,      # one frame in the second 128-frame tile and in the third Winograd tile; Tp = 160
    130,      # Tp = 160: the even tail and the 16-byte store tails
]
TAPS = ("enc0_conv",) + tuple(f"enc{b}" for b in range(7)) + ("tcn_out",) + tuple(f"dec{b}" for b in range(7))


def _sd():
    from misonet_amd import weights as W
    return W.make_state_dict(W.miso1_spec(), seed=3)


@pytest.fixture(scope="module")
def net():
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    sd = _sd()
    m = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m.load_state_dict(sd)
    m.eval().keep_activations(True)
    yield sd, m
    m.keep_activations(False)


_inputs = {}


def _input(T):
    """complex [2, 6, T, 129], sample 1 three times as loud (per-sample indexing of the statistics); shared, never written"""
    if T not in _inputs:
        r = np.random.default_rng(6000 + T)
        x = (r.standard_normal((2, 6, T, 129)) + 1j * r.standard_normal((2, 6, T, 129))).astype(np.complex64)
        x[1] *= 3.0
        _inputs[T] = x
    return _inputs[T]


def _planar(*segs):
    """complex segments [B, c, T, F] -> the trunk's float input: the real parts of all segments, then the imaginary parts"""
    return np.concatenate([s.real for s in segs] + [s.imag for s in segs], axis=1).astype(np.float32)


def _taps(m, B, T, names=TAPS):
    return {k: m.tap(k, B, T).cpu().numpy() for k in names}


def _step_input(name, xin, taps):
    """(x, skip, from_conv) of a conv step from the GPU's own taps, as miso_oracle.trunk_forward chains them"""
    if name == "enc0_conv":
        return xin, None, False
    b = int(name[3:])
    if name.startswith("enc"):
        return (taps["enc0_conv"], None, True) if b == 0 else (taps[f"enc{b - 1}"], None, False)
    return taps["tcn_out"] if b == 0 else taps[f"dec{b - 1}"], taps[f"enc{6 - b}"], False


def _check_levels(sd, xin, taps, levels, samples, model, mode, T):
    """every figure of a case is printed before anything is asserted"""
    ref, what = [], f"{model} {mode} T={T}"
    for name in levels:
        x, skip, from_conv = _step_input(name, xin, taps)
        for b in samples:
            xb, sb = x[b:b + 1], None if skip is None else skip[b:b + 1]
            truth = conv_ref.oracle_level(name, xb, sd, sb, torch.float64, from_conv).numpy()[0]
            y32 = conv_ref.oracle_level(name, xb, sd, sb, torch.float32, from_conv).numpy()[0]
            assert taps[name].shape[1:] == truth.shape, (name, taps[name].shape, truth.shape)
            c = conv_ref.compare(taps[name][b], truth, y32)
            print(conv_ref.report(c, f"{name} {what} sample {b}"))
            print(f"[conv-ratio] {name} {mode} {T} {b} " + " ".join(f"{v:.3f}" for v in conv_ref.ratios(c)))
            ref.append((name, b, truth, y32))
    for name, b, truth, y32 in ref:
        conv_ref.check(taps[name][b], truth, y32, f"{name} {what} sample {b}")


@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("mode", MODES)
def test_conv_levels_on_their_own_input_vs_float64(net, mode, T):
    """sample 1 at every T, sample 0 (the first slot of every tile walk) at T = 65 only: the CPU oracle is the time of this test"""
    sd, m = net
    m.set_precision(mode)
    x = _input(T)
    y = m(torch.from_numpy(x).cuda())
    assert tuple(y.shape) == (2, 2, T, 129) and torch.isfinite(torch.view_as_real(y)).all()
    taps = _taps(m, 2, T)
    out = torch.cat((y.real, y.imag), dim=1).cpu().numpy()
    assert np.array_equal(taps["dec6"], out), "the tap dec6 is the network's output"
    _check_levels(sd, _planar(x), taps, conv_ref.LEVELS, (0, 1) if T == 65 else (1,), "MISO_1", mode, T)


def _first_layer(model, M, mode):
    """the first conv and the first encoder level of MISO_1 (2 M input channels) / MISO_3 (2 (M + 2)) with M microphones on their own
    input, T = 65, B = 2, both samples"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    T = 65
    segs = (M,) if model == "MISO_1" else (M, 1, 1)
    spec = W.miso1_spec(num_ch=M) if model == "MISO_1" else W.miso3_spec(num_ch=M)
    sd = W.make_state_dict(spec, seed=4)
    r = np.random.default_rng(6400 + T + (0 if (model, M) == ("MISO_3", 6) else 100 * M + (1000 if model == "MISO_1" else 0)))
    xs = [(r.standard_normal((2, c, T, 129)) + 1j * r.standard_normal((2, c, T, 129))).astype(np.complex64) for c in segs]
    for v in xs:
        v[1] *= 3.0
    cls = mz.MISO_1 if model == "MISO_1" else mz.MISO_3
    m = cls(2 if model == "MISO_1" else 1, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m.load_state_dict(sd)
    m.eval().keep_activations(True).set_precision(mode)
    y = m(*[torch.from_numpy(v).cuda() for v in xs])
    assert tuple(y.shape) == (2, m.num_spks, T, 129)
    assert sd["encoders.0.0.conv2d.weight"].shape[1] == 2 * sum(segs)
    taps = _taps(m, 2, T, ("enc0_conv", "enc0"))
    _check_levels(sd, _planar(*xs), taps, ("enc0_conv", "enc0"), (0, 1), f"{model} M={M} Cin={2 * sum(segs)}", mode, T)


@pytest.mark.parametrize("mode", MODES)
def test_miso3_first_layer_on_its_own_input_vs_float64(mode):
    """16 input channels: the other first-layer shape of DIRECT, W1D and X6_FIRST"""
    _first_layer("MISO_3", 6, mode)


# the first-layer input channels the fused pipeline can create besides 12 and 16 (misonet_pipeline_create admits 2-8 microphones):
# 4, 10, 14 are no multiples of the 8-channel chunk; 18 and 20 are past conv3x3_x6_first (Cin <= 16), so in bf16x6 the first layer
# is the exact-f32 kernel writing the oct3 layout
FIRST_SHAPES = [("MISO_1", 2), ("MISO_1", 5), ("MISO_1", 7), ("MISO_3", 2), ("MISO_3", 5), ("MISO_3", 7), ("MISO_3", 8)]


@pytest.mark.parametrize("model,M", FIRST_SHAPES, ids=[f"{n}-M{M}" for n, M in FIRST_SHAPES])
@pytest.mark.parametrize("mode", MODES)
def test_first_layer_at_every_admitted_microphone_count_vs_float64(mode, model, M):
    """Cin = 4, 10, 14 (MISO_1) and 8, 14, 18, 20 (MISO_3): same taps, same bound as the 12 and 16 channels above"""
    _first_layer(model, M, mode)


# ---- b. the workspace's previous contents ---------------------------------------------------------------------------------------

def _run_filled(m, x, T, byte, keep):
    ws = m._workspace(2, T)
    ws.fill_(byte)
    y = m(x)                                       # check_nan = True: misonet_net_check has passed when this returns
    assert m._workspace(2, T).data_ptr() == ws.data_ptr()
    res = {"out": torch.view_as_real(y).clone()}
    if keep:
        res.update({k: m.tap(k, 2, T) for k in TAPS})
    return res


@pytest.mark.parametrize("keep", [False, True], ids=["shared", "keep"])
@pytest.mark.parametrize("T", [65, 130])
@pytest.mark.parametrize("mode", MODES)
def test_workspace_previous_contents_do_not_matter(net, mode, T, keep):
    """Only the network's own workspace is poisoned, and only with data (the pipeline workspace carries selection indices)."""
    _, m = net
    m.set_precision(mode)
    m.keep_activations(keep)
    try:
        x = torch.from_numpy(_input(T)).cuda()
        nan, zero = _run_filled(m, x, T, 0xFF, keep), _run_filled(m, x, T, 0x00, keep)
        for k in nan:
            assert torch.isfinite(nan[k]).all() and torch.isfinite(zero[k]).all(), f"{mode} T={T} {k}: non-finite"
        for k in nan:
            assert torch.equal(nan[k], zero[k]), (f"{mode} T={T} {k}: a workspace of 0xFF bytes and one of zeros give different bits "
                                                  f"({int((nan[k] != zero[k]).sum())} elements)")
    finally:
        m.keep_activations(True)


# ---- c. batch invariance across the tile-walk variants -----------------------------------------------------------------------------

T_INV = 130
NTX = (T_INV + 127) // 128          # 128-frame tiles of a row: 2


def x6_flex_rows(n, F, cus, ncg=1, ntx=NTX):
    """Tile height the bf16x6 launcher picks for a stride-1 oct3 layer with 4 < F <= 31 (launch_conv_bf16x6): rounds of tiles per
    CU, r8 with 8-row and r4 with 4-row tiles, a 4-row tile at 0.54 of an 8-row tile's time: ``r4 * 54 < r8 * 100`` picks 4 rows."""
    r8 = -(-(n * ntx * ((F + 7) // 8) * ncg) // cus)
    r4 = -(-(n * ntx * ((F + 3) // 4) * ncg) // cus)
    return 4 if r4 * 54 < r8 * 100 else 8


def batch_sizes(cus):
    """{batch size: what it reaches} for a device with `cus` CUs (256: 6, 8, 24, 40, 72)"""
    b_wino = cus // (3 * 16) + 1                    # enc0 level in Winograd form: B * 3 frame tiles * 16 row tiles > CUs
    while b_wino % 8 == 0:
        b_wino += 1
    sizes = {b_wino: "non-XCD walks; some Winograd workgroups walk two tiles of the enc0 level", 8: "the XCD walk of every kernel"}
    # one batch per flex group, a multiple of 8 (XCD walk) with n * ntx in the window where 8-row tiles are one round and 4-row
    # tiles two: (c/8, c/4] for F = 31, (c/4, c/2] for F = 15, (c/2, c] for F = 7
    for F, lo, hi in ((31, cus / 8, cus / 4), (15, cus / 4, cus / 2), (7, cus / 2, cus)):
        n = (int(lo / NTX) // 8 + 1) * 8
        assert lo < n * NTX <= hi, (F, n, cus)
        assert x6_flex_rows(n, F, cus) == 8 and x6_flex_rows(1, F, cus) == 4, (F, n, cus)
        sizes[n] = f"8-row bf16x6 tiles on the F = {F} layers (4-row tiles for the lone sample)"
    return sizes


def _sample(i):
    r = np.random.default_rng(7000 + i)
    x = (r.standard_normal((6, T_INV, 129)) + 1j * r.standard_normal((6, T_INV, 129))).astype(np.complex64)
    return x * np.float32(1.0 + 0.5 * (i % 4))


_alone = {}


def _run_alone(m, mode, i):
    """output and taps of sample i run alone (B = 1), computed once per mode"""
    if (mode, i) not in _alone:
        y = m(torch.from_numpy(_sample(i)[None]).cuda())
        res = {"out": torch.view_as_real(y)[0].clone()}
        res.update({k: m.tap(k, 1, T_INV)[0] for k in TAPS})
        _alone[(mode, i)] = res
    return _alone[(mode, i)]


@pytest.mark.parametrize("which", range(5), ids=["wino2", "xcd", "flex31", "flex15", "flex7"])
@pytest.mark.parametrize("mode", MODES)
def test_batch_invariance_bit_exact_across_tile_walks(net, mode, which):
    """Independent random samples, T = 130, kept activations: for samples {0, 1, 13, B - 1} the output and every tap of the sample
    inside the batch equal those of the same sample run alone.  The batch sizes come from the device's CU count (batch_sizes;
    256 CUs: 6, 8, 24, 40, 72): a B that is no multiple of 8 takes the plain tile walks (xcd = 2 in bf16x6) and gives the persistent
    Winograd kernel more enc0 tiles than CUs; a multiple of 8 takes the XCD walk of every kernel; and one B per bf16x6 "flex" group
    puts that group's layers on 8-row tiles while the lone sample takes 4-row tiles (the launcher's rule: ``r4 * 54 < r8 * 100``
    picks 4-row tiles, x6_flex_rows)."""
    _, m = net
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = batch_sizes(cus)
    B = list(sizes)[which]
    print(f"[conv-batch] {mode} B={B} on {cus} CUs: {sizes[B]}")
    m.set_precision(mode)
    picks = sorted({0, 1, B - 1} | ({13} if B > 13 else set()))
    alone = {i: _run_alone(m, mode, i) for i in picks}
    y = m(torch.from_numpy(np.stack([_sample(i) for i in range(B)])).cuda())
    got = {"out": torch.view_as_real(y)}
    got.update({k: m.tap(k, B, T_INV) for k in TAPS})
    bad = [(i, k) for i in picks for k in got if not torch.equal(got[k][i], alone[i][k])]
    assert not bad, f"{mode} B={B} ({sizes[B]}): sample in the batch differs from the sample alone at (sample, tap) {bad}"
