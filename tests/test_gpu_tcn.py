"""The TCN kernels (csrc/tcn.hip) on their OWN input against the float64 oracle: all four outer norms (tcn_dw_k<0..3>,
tcn_cln_stats_k), both point-wise arithmetics (tcn_pw_k fp32 MFMA / split-bf16, planar / oct3 destination), at the frame counts
where the tiling starts to matter.

One GPU forward of MISO_1 per case with kept activations; the taps ``enc6`` (the instance-normed encoder output = the TCN's
input) and ``tcn_out`` are read back, and on the CPU, per sample, ``miso_oracle.tcn_forward(enc6_gpu)`` runs in float64 (the
truth) and in float32 (the yardstick).  The encoder is the GPU's own, so its error is not part of what is measured, and the
bound can be the one of tests/tcn_ref.py: K times the float32 oracle's own distance from the truth, for the whole tensor and for
the worst single frame (tests/test_tcn.py shows that this bound rejects a lost partial, a wrong sample's statistics, a dead
seam, a leaking tail and a lost low-order product).  Measured ratios: LAB.md, "TCN on its own input".
"""
import numpy as np
import pytest
import torch

import tcn_ref
from test_gpu_parity import _assert_parity, _need_gpu

pytestmark = pytest.mark.gpu

NORMS = ("IN", "gLN", "cLN", "BN")
MODES = ("f32", "f32w", "bf16x6")          # bf16x6: the X6 point-wise conv, oct3 source and destination; f32w: never ran a non-IN net
FRAMES = [
    40,       # every dilation >= 64 outside the signal; one partial slot
    128,      # exactly one full point-wise tile, nothing masked
    129,      # second tile of one frame: the pivot frame is the only valid one; 2 slots; Tp = 160
    130,      # Tq = 132 > T: the float4 tail of tcn_dw_k and the cLN fs + t + 2 read past T
    257,      # three slots; a second block of tcn_cln_stats_k (Tp = 288 > 256)
    1920,     # exactly one depth-wise segment (seg_f == DW_SEG)
    1921,     # a second segment holding one frame
    1985,     # a second segment longer than the 64-frame halo: dilation-64 taps cross the seam both ways
]


def _sd(nt):
    from misonet_amd import weights as W
    return W.make_state_dict(W.miso1_spec(norm_type=nt), seed=3)


@pytest.fixture(scope="module", params=NORMS)
def net(request):
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    nt = request.param
    sd = _sd(nt)
    m = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), nt).cuda(0)
    m.load_state_dict(sd)
    m.eval().keep_activations(True)
    request.addfinalizer(lambda: m.keep_activations(False))
    return nt, sd, m


_inputs = {}


def _input(T):
    """complex [2, 6, T, 129], sample 1 three times as loud (per-sample indexing of the statistics); shared, never written"""
    if T not in _inputs:
        r = np.random.default_rng(4000 + T)
        x = (r.standard_normal((2, 6, T, 129)) + 1j * r.standard_normal((2, 6, T, 129))).astype(np.complex64)
        x[1] *= 3.0
        _inputs[T] = x
    return _inputs[T]


@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("mode", MODES)
def test_tcn_on_its_own_input_vs_float64(net, mode, T):
    from oracle import miso_oracle
    nt, sd, m = net
    m.set_precision(mode)
    y = m(torch.from_numpy(_input(T)).cuda())
    assert tuple(y.shape) == (2, 2, T, 129) and torch.isfinite(torch.view_as_real(y)).all()
    enc6 = m.tap("enc6", 2, T).cpu().numpy()
    tcn = m.tap("tcn_out", 2, T).cpu().numpy()
    assert enc6.shape == (2, 128, T, 1) and tcn.shape == (2, 128, T, 1)
    enc6, tcn = enc6[..., 0], tcn[..., 0].astype(np.float64)
    ref = []
    for b in range(2):
        with miso_oracle.precision(torch.float64):
            truth = miso_oracle.tcn_forward(torch.from_numpy(enc6[b:b + 1].astype(np.float64)), sd, norm_type=nt).numpy()[0]
        y32 = miso_oracle.tcn_forward(torch.from_numpy(enc6[b:b + 1]), sd, norm_type=nt).numpy()[0]
        ref.append((truth, y32))
        c = tcn_ref.compare(tcn[b], truth, y32)                 # every figure is printed before anything is asserted
        print(tcn_ref.report(c, f"{nt} {mode} T={T} sample {b}"))
        print(f"[tcn-ratio] {nt} {mode} {T} {b} {c['err'] / c['e32']:.3f} {c['ferr'] / c['f32max']:.3f} {c['err']:.3e} {c['t']}")
    for b, (truth, y32) in enumerate(ref):
        tcn_ref.check(tcn[b], truth, y32, f"{nt} {mode} T={T} sample {b}")


@pytest.mark.parametrize("T", [257, 1985])
@pytest.mark.parametrize("mode", MODES)
def test_tcn_batch_invariance_bit_exact(net, mode, T):
    """Samples run one by one equal the batch, a second run of the batch equals the first: bit for bit, at the TCN output and at
    the network output (every statistic is a fixed-order sum of per-tile / per-group float64 partials)."""
    nt, _, m = net
    m.set_precision(mode)
    x = torch.from_numpy(_input(T)).cuda()
    y = m(x)
    tcn = m.tap("tcn_out", 2, T)
    for b in range(2):
        yb = m(x[b:b + 1])
        tb = m.tap("tcn_out", 1, T)
        assert torch.equal(tb[0], tcn[b]), f"{nt} {mode} T={T}: tcn_out of sample {b} alone differs from the batch"
        assert torch.equal(yb[0], y[b]), f"{nt} {mode} T={T}: output of sample {b} alone differs from the batch"
    y2 = m(x)
    assert torch.equal(m.tap("tcn_out", 2, T), tcn) and torch.equal(y2, y), f"{nt} {mode} T={T}: two runs of the batch differ"


_miso3_ref = {}


def _miso3_case(nt, T):
    """inputs and the oracle's answer for MISO_3(norm_type = nt), computed once for the three modes"""
    if (nt, T) not in _miso3_ref:
        from misonet_amd import weights as W
        from oracle import miso_oracle
        sd3 = W.make_state_dict(W.miso3_spec(norm_type=nt), seed=4)
        r = np.random.default_rng(4400 + T)
        x, a, b = [(r.standard_normal((2, c, T, 129)) + 1j * r.standard_normal((2, c, T, 129))).astype(np.complex64) for c in (6, 1, 1)]
        for v in (x, a, b):
            v[1] *= 3.0
        ref = np.concatenate([miso_oracle.miso3_forward(*[torch.from_numpy(v[i:i + 1]) for v in (x, a, b)], sd3, norm_type=nt).numpy()
                              for i in range(2)])
        _miso3_ref[(nt, T)] = (sd3, x, a, b, ref)
    return _miso3_ref[(nt, T)]


@pytest.mark.parametrize("T", [40, 130])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nt", ["gLN", "BN"])
def test_miso3_gln_bn_vs_oracle(nt, mode, T):
    """MISO_3 with the gLN and BatchNorm1d outer norms (cLN: test_norm_type_variants_vs_reference_golden), below and above one
    frame tile, against the oracle built with the same norm type."""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    sd3, x, a, b, ref = _miso3_case(nt, T)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), nt).cuda(0)
    m3.load_state_dict(sd3)
    m3.eval().set_precision(mode)
    y = m3(torch.from_numpy(x).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert tuple(y.shape) == (2, 1, T, 129)
    _assert_parity(y.cpu().numpy(), ref, f"MISO_3(norm_type={nt}) [{mode}] T={T} vs oracle")
