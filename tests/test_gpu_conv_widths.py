"""The 3x3 conv stack at channel widths OTHER than the default (24, 32, 32, 32, 32, 64, 128): misonet_net_create admits every list of
multiples of 8 up to 128, the kernels are written around the default, and tests/test_gpu_conv_levels.py runs nothing else.

The width sets are conv_ref.WIDTH_SETS (``narrow_to_wide`` with 3 speakers, ``wide_first`` with 4); which kernel runs which layer
there is pinned on the host by tests/test_lib_abi.py (test_conv_plan_kernel_per_layer_at_other_widths).  Reached here and nowhere
else: f32w DenseBlocks whose convs run on two kernels (W1D + WINO, WINO + DIRECT) writing slices of one dense buffer; WINO at 8,
16 (the 16-row body alone), 40, 48, 56 and 64 output channels; 64-channel DIRECT groups at 72 ... 128 output channels and up to
384 input channels; the stride-2 transposed layers at 8 ... 64 and dec0 at 72 and 128 output channels; a first layer of 40 output
channels (in bf16x6: the exact-f32 kernel writing oct3 in two 32-channel halves); bf16x6 tiles with Cout & 31 in {8, 16, 24} at two
and more channel groups and weight preparation over 48 chunks; a last layer of 6 / 8 channels, which is neither conv3x3_few nor the
rows_in_m tile; and other placements of the lifetime-shared arena.

a. Every one of the 15 conv levels on the GPU's OWN previous tap against the float64 oracle, with the helpers and the bound of
   tests/test_gpu_conv_levels.py (conv_ref.K = 4 times the float32 oracle's distance, whole tensor / worst frame / row / channel):
   both samples at T = 65, sample 1 at T = 129.  And ``dec6`` alone at the default widths for 1, 3 and 4 speakers (2 is held there).
b. Bits: a workspace of 0xFF bytes and one of zeros give the same output and taps; the shared-arena forward gives the output of the
   kept-activations forward; samples 0, 1 and B - 1 of a batch of 8 (the XCD walk) and of 3 (the plain walk) equal the sample alone
   at every tap.
Measured ratios: LAB.md, "Conv levels on their own input".
"""
import numpy as np
import pytest
import torch

import conv_ref
from test_gpu_conv_levels import MODES, TAPS, _check_levels, _planar, _run_filled, _taps
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

WIDTHS = conv_ref.OTHER_WIDTHS

_nets = {}


def _net(ws, spks=None):
    """(state_dict, MISO_1 with kept activations) of a width set, built once; `spks` overrides the set's speaker count"""
    _need_gpu()
    if (ws, spks) not in _nets:
        import misonet_amd as mz
        from misonet_amd import weights as W
        en, de, s = conv_ref.widths(ws)
        s = s if spks is None else spks
        sd = W.make_state_dict(W.miso1_spec(num_spks=s, en_ch=en, de_ch=de), seed=3)
        m = mz.MISO_1(s, 6, 7, list(en), list(de), "IN").cuda(0)
        m.load_state_dict(sd)
        m.eval().keep_activations(True)
        _nets[(ws, spks)] = (sd, m)
    return _nets[(ws, spks)]


_inputs = {}


def _input(T):
    """complex [2, 6, T, 129], sample 1 three times as loud; shared, never written"""
    if T not in _inputs:
        r = np.random.default_rng(8000 + T)
        x = (r.standard_normal((2, 6, T, 129)) + 1j * r.standard_normal((2, 6, T, 129))).astype(np.complex64)
        x[1] *= 3.0
        x.setflags(write=False)
        _inputs[T] = x
    return _inputs[T]


# ---- a. the levels on their own input -----------------------------------------------------------------------------------------------

_forward = {}


def _forward_taps(ws, mode, T, spks=None):
    """all taps of one forward (B = 2, kept activations) as NumPy arrays, read back once per (set, mode, T)"""
    key = (ws, mode, T, spks)
    if key not in _forward:
        _forward.clear()                               # one case's taps at a time
        sd, m = _net(ws, spks)
        m.set_precision(mode)
        y = m(torch.from_numpy(_input(T).copy()).cuda())
        assert tuple(y.shape) == (2, m.num_spks, T, 129) and torch.isfinite(torch.view_as_real(y)).all()
        taps = _taps(m, 2, T)
        out = torch.cat((y.real, y.imag), dim=1).cpu().numpy()
        assert np.array_equal(taps["dec6"], out), "the tap dec6 is the network's output"
        _forward[key] = taps
    return _forward[key]


# T = 65: the second Winograd tile holds one frame, Tp = 96, both samples; T = 129: one frame in the second 128-frame tile and in the
# third Winograd tile, sample 1.  One (T, sample) per case: the float64 oracle of one sample is the time of a case
LEVEL_CASES = [(65, 0), (65, 1), (129, 1)]


@pytest.mark.parametrize("T,sample", LEVEL_CASES, ids=[f"T{T}-s{b}" for T, b in LEVEL_CASES])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ws", WIDTHS)
def test_conv_levels_at_other_widths_vs_float64(ws, mode, T, sample):
    sd, _ = _net(ws)
    taps = _forward_taps(ws, mode, T)
    _check_levels(sd, _planar(_input(T)), taps, conv_ref.LEVELS, (sample,), f"MISO_1 {ws}", f"{mode}@{ws}", T)


@pytest.mark.parametrize("spks", [1, 3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_last_level_at_every_speaker_count_vs_float64(mode, spks):
    """dec6 at the default widths ends in 48 -> 2 (conv3x3_few<2> / the rows_in_m tile), 6 or 8 channels (DIRECT without
    activation in f32 and f32w, the generic X6 tile in bf16x6): T = 65, both samples"""
    T = 65
    sd, _ = _net("default", spks)
    taps = _forward_taps("default", mode, T, spks)
    assert taps["dec6"].shape == (2, 2 * spks, T, 129)
    _check_levels(sd, _planar(_input(T)), taps, ("dec6",), (0, 1), f"MISO_1 default {spks} speakers", f"{mode}@spk{spks}", T)


# ---- b. bits --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep", [False, True], ids=["shared", "keep"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ws", WIDTHS)
def test_workspace_previous_contents_do_not_matter_at_other_widths(ws, mode, keep):
    _, m = _net(ws)
    m.set_precision(mode)
    m.keep_activations(keep)
    try:
        T = 65
        x = torch.from_numpy(_input(T).copy()).cuda()
        nan, zero = _run_filled(m, x, T, 0xFF, keep), _run_filled(m, x, T, 0x00, keep)
        assert set(nan) == ({"out"} | set(TAPS) if keep else {"out"})
        for k in nan:
            assert torch.isfinite(nan[k]).all() and torch.isfinite(zero[k]).all(), f"{ws} {mode} {k}: non-finite"
        for k in nan:
            assert torch.equal(nan[k], zero[k]), (f"{ws} {mode} {k}: a workspace of 0xFF bytes and one of zeros give different bits "
                                                  f"({int((nan[k] != zero[k]).sum())} elements)")
    finally:
        m.keep_activations(True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ws", WIDTHS)
def test_shared_arena_gives_the_bits_of_kept_activations(ws, mode):
    """make_layout places the buffers largest first, so other widths are another placement: the output with buffers of disjoint
    lifetimes sharing memory equals the output with every buffer on its own, bit for bit (T = 65 and 130)"""
    _, m = _net(ws)
    m.set_precision(mode)
    try:
        for T in (65, 130):
            x = torch.from_numpy(_input(T).copy()).cuda()
            m.keep_activations(True)
            kept = torch.view_as_real(m(x)).clone()
            m.keep_activations(False)
            shared = torch.view_as_real(m(x)).clone()
            assert torch.isfinite(kept).all()
            assert torch.equal(kept, shared), f"{ws} {mode} T={T}: {int((kept != shared).sum())} elements differ"
    finally:
        m.keep_activations(True)


T_INV = 130


def _sample(i):
    r = np.random.default_rng(9000 + i)
    x = (r.standard_normal((6, T_INV, 129)) + 1j * r.standard_normal((6, T_INV, 129))).astype(np.complex64)
    return x * np.float32(1.0 + 0.5 * (i % 4))


_alone = {}


def _run_alone(m, ws, mode, i):
    """output and taps of sample i run alone (B = 1), computed once per set and mode"""
    if (ws, mode, i) not in _alone:
        y = m(torch.from_numpy(_sample(i)[None]).cuda())
        res = {"out": torch.view_as_real(y)[0].clone()}
        res.update({k: m.tap(k, 1, T_INV)[0] for k in TAPS})
        _alone[(ws, mode, i)] = res
    return _alone[(ws, mode, i)]


@pytest.mark.parametrize("B", [8, 3], ids=["xcd", "plain"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ws", WIDTHS)
def test_batch_invariance_bit_exact_at_other_widths(ws, mode, B):
    """T = 130, independent samples: the output and every tap of samples 0, 1 and B - 1 inside a batch of 8 (the XCD walk of every
    kernel) and of 3 (the plain walks) equal those of the sample run alone"""
    _, m = _net(ws)
    m.set_precision(mode)
    picks = sorted({0, 1, B - 1})
    alone = {i: _run_alone(m, ws, mode, i) for i in picks}
    y = m(torch.from_numpy(np.stack([_sample(i) for i in range(B)])).cuda())
    got = {"out": torch.view_as_real(y)}
    got.update({k: m.tap(k, B, T_INV) for k in TAPS})
    bad = [(i, k) for i in picks for k in got if not torch.equal(got[k][i], alone[i][k])]
    assert not bad, f"{ws} {mode} B={B}: sample in the batch differs from the sample alone at (sample, tap) {bad}"
