"""CPU tests of tests/conv_ref.py and of the oracle's level split: the comparator of the GPU conv-level tests
(tests/test_gpu_conv_levels.py) must be able to fail.

* ``miso_oracle.trunk_forward`` through ``encoder_level`` / ``decoder_level`` gives bit for bit the taps of the unsplit forward
  it replaced (kept below as ``_trunk_forward_unsplit``), and a level run alone on the previous taps reproduces its tap;
* the clean restatement of a level equals the oracle's level in float64 (<= 1e-12) on shallow, middle and deep levels: the
  stride-1 first conv, stride-2 conv + DenseBlock, the stride-1 bottleneck conv, the stride-1 and stride-2 transposed convs,
  DenseBlock + transposed conv, and ``dec6`` with the 48-channel dense conv and the raw 4-channel last layer;
* K * (float32 oracle's distance) is not vacuous: measured here, the float32 oracle's own per-level distance from the float64
  truth is 1.5e-7 ... 4.7e-7 for the whole tensor and at most 6.3e-7 for the worst frame, row or channel (band asserted: 1e-7 ...
  6e-7 and 8e-7), and an INDEPENDENT healthy float32 evaluation (the restatement in float32, every conv summed tap by tap:
  another summation order, explicit padding, float64 statistics like the kernels) passes at the K the GPU tests use;
* every injected fault, at the smallest frame count of the GPU matrix that reaches it, is rejected at that K -- in every conv of
  the level and in the LAST conv alone -- and by the right metric: frame T - 1 for ``halo_t``, the last row for ``halo_f``,
  sample 1 only for ``stat_sample``, the one channel for ``stat_tile`` / ``stat_wtile``;
* the same at the channel widths of the other sets of ``conv_ref.WIDTH_SETS`` (the ``*_at_other_widths`` tests: the GPU tests of
  tests/test_gpu_conv_widths.py use the comparator there): restatement, input rounding and all 24 faults as above; the yardstick
  lies in a band measured per set (``YARDSTICK_BAND``: whole tensor 1.5e-7 ... 5.9e-7, worst frame / row / channel up to 6.5e-7 on
  ``narrow_to_wide`` and 9.3e-7 on ``wide_first``, whose ``dec1`` sums 256 channels into 16 on 7 rows); and ``halo_t`` in ALL convs
  of a level is held to the frames the level's depth can reach from the halo, not to frame T - 1 alone, which is a matter of the
  weights (``narrow_to_wide`` ``dec6``: T - 2).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref

EN_F, DE_F = conv_ref.EN_F, conv_ref.DE_F
WIDTHS = conv_ref.OTHER_WIDTHS                    # the width sets beside "default" (conv_ref.WIDTH_SETS)


def _sd(ws="default"):
    return conv_ref.state_dict(ws, seed=3)


def _normed(r, shape):
    x = r.standard_normal(shape)
    x[1] *= 3.0
    x = (x - x.mean((-2, -1), keepdims=True)) / x.std((-2, -1), keepdims=True)
    return x.astype(np.float32).astype(np.float64)                  # the device hands over float32 values


_cache = {}


def _case(name, T, ws="default"):
    """(sd, x, skip, truth, y32): seeded instance-normed input of the level at the channel widths of the set `ws` (B = 2; the raw
    network input of ``enc0_conv`` keeps sample 1 three times as loud), the float64 and the float32 oracle on it (computed once,
    read-only)"""
    if (name, T, ws) not in _cache:
        sd = _sd(ws)
        EN, DE = conv_ref.level_channels(ws)
        r = np.random.default_rng(1000 + T + 7 * conv_ref.LEVELS.index(name))
        b = 0 if name == "enc0_conv" else int(name[3:])
        skip = None
        if name == "enc0_conv":
            x = r.standard_normal((2, EN[0], T, EN_F[0]))
            x[1] *= 3.0
            x = x.astype(np.float32).astype(np.float64)
        elif name.startswith("enc"):
            x = _normed(r, (2, EN[b], T, EN_F[b]))
        else:
            x, skip = _normed(r, (2, DE[b], T, DE_F[b])), _normed(r, (2, DE[b], T, DE_F[b]))
        truth = conv_ref.oracle_level(name, x, sd, skip).numpy()
        y32 = conv_ref.oracle_level(name, x, sd, skip, dtype=torch.float32).numpy()
        for a in (x, skip, truth, y32):
            if a is not None:
                a.setflags(write=False)
        _cache[(name, T, ws)] = (sd, x, skip, truth, y32)
    return _cache[(name, T, ws)]


# ---- the level split of the oracle ---------------------------------------------------------------------------------------

def _trunk_forward_unsplit(x, sd, taps):
    """miso_oracle.trunk_forward as it stood before encoder_level / decoder_level were cut out of it"""
    from oracle.miso_oracle import _conv_elu_in, _dense_block, _t, tcn_forward
    xs = []
    for b in range(7):
        if b == 0:
            x = F.conv2d(x, _t(sd, "encoders.0.0.conv2d.weight"), _t(sd, "encoders.0.0.conv2d.bias"), stride=(1, 1), padding=(1, 0))
            taps["enc0_conv"] = x
            x = _dense_block(x, sd, "encoders.0.1")
        else:
            stride = (1, 1) if b == 6 else (1, 2)
            x = _conv_elu_in(x, _t(sd, f"encoders.{b}.0.net.0.weight"), _t(sd, f"encoders.{b}.0.net.0.bias"), stride, (1, 0))
            if b < 5:
                x = _dense_block(x, sd, f"encoders.{b}.1")
        xs.append(x)
        taps[f"enc{b}"] = x
    x = tcn_forward(x[..., 0], sd, taps, "IN")
    taps["tcn_out"] = x
    de = x.unsqueeze(-1)
    for b in range(7):
        de = torch.cat((de, xs[6 - b]), dim=1)
        if b >= 2:
            de = _dense_block(de, sd, f"decoders.{b}.0")
            if b == 6:
                de = F.conv_transpose2d(de, _t(sd, "decoders.6.1.deconv2d.weight"), _t(sd, "decoders.6.1.deconv2d.bias"),
                                        stride=(1, 1), padding=(1, 0))
            else:
                de = _conv_elu_in(de, _t(sd, f"decoders.{b}.1.net.0.weight"), _t(sd, f"decoders.{b}.1.net.0.bias"),
                                  (1, 2), (1, 0), transposed=True)
        else:
            stride = (1, 1) if b == 0 else (1, 2)
            de = _conv_elu_in(de, _t(sd, f"decoders.{b}.0.net.0.weight"), _t(sd, f"decoders.{b}.0.net.0.bias"),
                              stride, (1, 0), transposed=True)
        taps[f"dec{b}"] = de
    return de


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_level_split_is_bit_neutral(dtype):
    from oracle import miso_oracle
    sd = _sd()
    r = np.random.default_rng(77)
    x = torch.from_numpy(r.standard_normal((2, 12, 33, 129)).astype(np.float32))
    with torch.no_grad(), miso_oracle.precision(dtype):
        x = x.to(dtype)
        old, new = {}, {}
        y_old = _trunk_forward_unsplit(x, sd, old)
        y_new = miso_oracle.trunk_forward(x, sd, new)
        assert torch.equal(y_old, y_new)
        assert sorted(old) == sorted(new) and len(new) == 17             # enc0_conv, enc0..6, tcn_block0, tcn_out, dec0..6
        for k in old:
            assert torch.equal(old[k], new[k]), k
        # a level alone on the previous taps is that level of the forward
        assert torch.equal(miso_oracle.enc0_conv(x, sd), new["enc0_conv"])
        assert torch.equal(miso_oracle.encoder_level(0, new["enc0_conv"], sd, from_conv=True), new["enc0"])
        for b in range(1, 7):
            assert torch.equal(miso_oracle.encoder_level(b, new[f"enc{b - 1}"], sd), new[f"enc{b}"]), b
        for b in range(7):
            prev = new["tcn_out"].unsqueeze(-1) if b == 0 else new[f"dec{b - 1}"]
            assert torch.equal(miso_oracle.decoder_level(b, prev, new[f"enc{6 - b}"], sd), new[f"dec{b}"]), b


# ---- the restatement ---------------------------------------------------------------------------------------------------------

# shallow (F = 127 / 129), middle, deep (F <= 3): stride 1 (enc0_conv, enc6), stride 2 (enc4, with its DenseBlock), transposed with
# stride 1 (dec0, dec6) and 2 (dec1, dec2), the 48-channel dense conv and the 4-channel last layer (dec6)
EQ_LEVELS = ("enc0_conv", "enc4", "enc6", "dec0", "dec1", "dec2", "dec6")


# dec6 (F = 127, up to 144 input channels) at T = 65 only: nothing in the restatement depends on T
@pytest.mark.parametrize("name,T", [(n, T) for n in EQ_LEVELS for T in (65, 130) if (n, T) != ("dec6", 130)])
def test_restatement_equals_oracle_float64(name, T):
    _restatement_equals_oracle_float64(name, T, "default")


def _restatement_equals_oracle_float64(name, T, ws):
    sd, x, skip, truth, _ = _case(name, T, ws)
    for by_taps in (False, True):
        y = conv_ref.level(name, x, sd, skip, by_taps=by_taps).numpy()
        e = conv_ref.rel_l2(y, truth)
        print(f"[conv_ref] {ws} {name} T={T}: restatement{' tap by tap' if by_taps else ''} vs float64 oracle {e:.2e}")
        assert y.shape == truth.shape and e <= 1e-12, (ws, name, T, by_taps, e)


@pytest.mark.parametrize("name,T", [(n, T) for n in EQ_LEVELS for T in (65, 130) if (n, T) != ("dec6", 130)])
@pytest.mark.parametrize("ws", WIDTHS)
def test_restatement_equals_oracle_float64_at_other_widths(ws, name, T):
    """the same levels at the channel widths of conv_ref.WIDTH_SETS: dec6 then ends in a raw 6- / 8-channel layer, dec1 reads 144 /
    256 channels, the dense convs up to 384"""
    _restatement_equals_oracle_float64(name, T, ws)


def test_enc0_from_conv_restatement():
    sd, x, _, _, _ = _case("enc0_conv", 65)
    c0 = conv_ref.oracle_level("enc0_conv", x, sd)
    truth = conv_ref.oracle_level("enc0", c0, sd, from_conv=True).numpy()
    assert np.array_equal(truth, conv_ref.oracle_level("enc0", x, sd).numpy())
    assert conv_ref.rel_l2(conv_ref.level("enc0", c0, sd, from_conv=True).numpy(), truth) <= 1e-12


@pytest.mark.parametrize("T", [64, 65])
@pytest.mark.parametrize("name", EQ_LEVELS)
def test_bound_is_not_vacuous(name, T):
    _bound_is_not_vacuous(name, T, "default")


# (lowest, highest whole-tensor figure, highest worst-frame / row / channel figure) of the float32 oracle against the float64 oracle
# over EQ_LEVELS x T in {64, 65} x both samples: "default" as asserted since the test exists; the other sets as measured on the CPU
# with this file's inputs and rounded outward to one digit
YARDSTICK_BAND = {
    "default": (1e-7, 6e-7, 8e-7),
    "narrow_to_wide": (1e-7, 6e-7, 7e-7),         # whole 1.54e-7 (dec0) ... 5.43e-7 (dec2); worst 6.45e-7: a frame of dec2, T = 64
    "wide_first": (1e-7, 6e-7, 1e-6),             # whole 1.53e-7 (dec0) ... 5.88e-7 (dec1); worst 9.26e-7: a frame of dec1 (256 -> 16
                                                  # channels on 7 rows: a frame is 112 values), T = 64
}


def _bound_is_not_vacuous(name, T, ws):
    sd, x, skip, truth, y32 = _case(name, T, ws)
    lo, hi, worst = YARDSTICK_BAND[ws]
    r32 = conv_ref.level(name, x, sd, skip, dtype=torch.float32, by_taps=True).numpy()
    for b in range(2):
        what = f"{ws} {name} T={T} sample {b}"
        c = conv_ref.check(y32[b], truth[b], y32[b], "float32 oracle against itself " + what)
        print(f"[conv_ref] yardstick {what}: whole {c['whole32']:.2e} frame {c['frame32']:.2e} row {c['row32']:.2e} chan {c['chan32']:.2e}")
        assert lo <= c["whole32"] <= hi, c                            # float32 round-off through at most six convs, nothing else
        assert max(c["frame32"], c["row32"], c["chan32"]) <= worst, c
        c = conv_ref.check(r32[b], truth[b], y32[b], "float32 restatement " + what)
        print(conv_ref.report(c, "float32 restatement " + what))


@pytest.mark.parametrize("T", [64, 65])
@pytest.mark.parametrize("name", EQ_LEVELS)
@pytest.mark.parametrize("ws", WIDTHS)
def test_bound_is_not_vacuous_at_other_widths(ws, name, T):
    """The yardstick of the other width sets lies in a band of its own (YARDSTICK_BAND): a level of 8 channels sums fewer products
    than one of 32, one that reads 256 or 384 channels more.  Figures: the [conv_ref] yardstick lines of this test on the CPU.
    The independent tap-by-tap float32 restatement passes conv_ref.check at the same K = 4."""
    _bound_is_not_vacuous(name, T, ws)


@pytest.mark.parametrize("name", EQ_LEVELS)
def test_input_rounding_moves_a_level_less_than_the_yardstick(name):
    """What a +-1 float32 ulp difference of the level's INPUT is worth (the consumer kernels normalise RAW + statistics on load,
    the tap was normalised by the export kernel): the float64 level on the perturbed input against the float64 level on the
    input, in units of the yardstick.  Measured here: 0.15 ... 0.49 of it for every metric, so input rounding alone cannot carry
    a device reading over K = 4; bound asserted: under one yardstick (a perturbation of half an ulp r.m.s. per element cannot move
    the result further than float32 round-off inside the level does)."""
    _input_rounding(name, "default")


def _input_rounding(name, ws):
    T = 65
    sd, x, skip, truth, y32 = _case(name, T, ws)
    moved = conv_ref.oracle_level(name, conv_ref.perturb_ulp(x, 11), sd, None if skip is None else conv_ref.perturb_ulp(skip, 12)).numpy()
    for b in range(2):
        c = conv_ref.compare(moved[b], truth[b], y32[b])
        r = conv_ref.ratios(c)
        print(f"[conv-ulp] {ws} {name} T={T} sample {b}: " + " ".join(f"{v:.3f}" for v in r))
        assert 0 < max(r) < 1.0, (ws, name, b, r)


@pytest.mark.parametrize("name", EQ_LEVELS)
@pytest.mark.parametrize("ws", WIDTHS)
def test_input_rounding_moves_a_level_less_than_the_yardstick_at_other_widths(ws, name):
    """the same bound (under one yardstick) at the other width sets"""
    _input_rounding(name, ws)


# ---- the faults ----------------------------------------------------------------------------------------------------------------

# fault, level, the smallest T of the GPU matrix that reaches it
FAULT_CASES = [
    ("halo_t", "enc0_conv", 64),     # T == Tp: the halo frame is the next row's first word
    ("halo_t", "enc4", 64),
    ("halo_t", "dec1", 64),          # transposed
    ("halo_t", "dec6", 64),          # the raw last layer
    ("halo_f", "enc4", 64),          # DenseBlock convs: padding 1 in frequency
    ("halo_f", "dec0", 64),          # transposed, stride 1: rows Fin and Fin + 1 of the output see the halo row
    ("halo_f", "dec1", 64),          # transposed, stride 2: the last output row sees it
    ("halo_f", "dec6", 64),
    ("stat_tile", "enc4", 129),      # the second 128-frame tile holds one frame: the smallest partial there is to lose
    ("stat_tile", "dec2", 129),
    ("stat_wtile", "enc4", 65),      # the same for the Winograd kernel's 64-frame tiles (the DenseBlock convs of f32w)
    ("stat_wtile", "dec6", 65),
    ("stat_sample", "enc4", 64),
    ("stat_sample", "dec1", 64),
    ("stat_sample", "enc6", 64),
    ("prod16", "enc0_conv", 64),
    ("prod16", "enc4", 64),
    ("prod16", "dec6", 64),
    ("drop2", "enc0_conv", 64),
    ("drop2", "enc4", 64),
    ("drop2", "enc6", 64),
    ("drop2", "dec6", 64),
    ("pad_leak", "enc4", 65),        # Tp = 96: 31 padding frames
    ("pad_leak", "dec2", 130),       # Tp = 160
]

@pytest.mark.parametrize("where", ["all", "last"])
@pytest.mark.parametrize("fault,name,T", FAULT_CASES)
def test_fault_is_rejected(fault, name, T, where):
    _fault_is_rejected(fault, name, T, where, "default")


@pytest.mark.parametrize("where", ["all", "last"])
@pytest.mark.parametrize("fault,name,T", FAULT_CASES)
@pytest.mark.parametrize("ws", WIDTHS)
def test_fault_is_rejected_at_other_widths(ws, fault, name, T, where):
    """the same 24 faults, both `where`, the same factor 2 over K and the same metric at the other width sets: the comparator
    has to be able to fail where the GPU tests use it (tests/test_gpu_conv_widths.py)"""
    _fault_is_rejected(fault, name, T, where, ws)


def _fault_is_rejected(fault, name, T, where, ws):
    sd, x, skip, truth, y32 = _case(name, T, ws)
    y = conv_ref.level(name, x, sd, skip, fault=fault, where=where).numpy()
    hit = []
    one_sample = fault in ("stat_tile", "stat_wtile", "stat_sample")
    for b in range(2):
        c = conv_ref.compare(y[b], truth[b], y32[b])
        bad = conv_ref.failures(c)
        r = conv_ref.ratios(c)
        print(conv_ref.report(c, f"fault {fault} ({where}) {name} T={T} sample {b}"))
        print(f"[fault-ratio] {fault} {where} {name} {T} {b} " + " ".join(f"{v:.3g}" for v in r))
        if bad:
            hit.append(b)
            with pytest.raises(AssertionError) as ei:
                conv_ref.check(y[b], truth[b], y32[b], f"fault {fault}")
            assert f"(K = {conv_ref.K:g})" in str(ei.value)
        if one_sample and b == 0:
            continue
        # the strongest ratio of the sample is what rejects it: it has to clear K by a factor of two
        assert max(r) >= 2 * conv_ref.K, (fault, where, name, T, b, r)
        n_last = sum(conv_ref.applies(fault, cv) for cv in conv_ref.level_convs(name)[-1:])
        if fault == "halo_t" and (ws == "default" or where == "last"):
            assert "frame" in bad and c["t"] == T - 1, c                   # the frame next to the halo
        elif fault == "halo_t":
            # every conv of the level reads the stale frame and hands its wrong last frame one frame further back to the next:
            # behind n convs the frames T - n ... T - 1 are wrong and which of them is worst is a matter of the weights
            # (narrow_to_wide dec6, six convs of 8 and 16 channels: T - 2)
            assert "frame" in bad and c["t"] >= T - len(conv_ref.level_convs(name)), c
        if fault == "halo_f" and where == "last" and n_last:
            assert "row" in bad and c["f"] >= truth.shape[-1] - 2, c         # the rows next to the halo row
        if fault in ("stat_tile", "stat_wtile") and where == "last" and name != "dec6":
            assert "chan" in bad and c["c"] == conv_ref.STAT_ROW[1], c       # the channel whose statistics lost a tile
    assert hit, f"fault {fault!r} ({conv_ref.FAULTS[fault]}) passed the comparator at K = {conv_ref.K:g}"
    if one_sample:
        assert hit == [1], hit                                              # only the sample whose statistics are wrong
    else:
        assert hit == [0, 1], hit


# ---- the batch sizes of the GPU file's batch-invariance test ------------------------------------------------------------------------

def test_batch_size_windows():
    """the window arithmetic of test_gpu_conv_levels.batch_sizes on the host, for CU counts of the CDNA3 / CDNA4 parts"""
    from test_gpu_conv_levels import batch_sizes, x6_flex_rows
    assert list(batch_sizes(256)) == [6, 8, 24, 40, 72]
    assert 6 * 3 * 16 > 256 >= 5 * 3 * 16
    assert [x6_flex_rows(1, F, 256) for F in (31, 15, 7)] == [4, 4, 4]
    assert [x6_flex_rows(n, F, 256) for n, F in ((24, 31), (40, 15), (72, 7))] == [8, 8, 8]
    # B = 9 at T = 1001 (8 frame tiles, test_bf16x6_batch_invariance): only the F = 15 layers leave the lone sample's 4-row tiles
    assert [x6_flex_rows(9, F, 256, ntx=8) for F in (31, 15, 7)] == [4, 8, 4] and [x6_flex_rows(1, F, 256, ntx=8) for F in (31, 15, 7)] == [4, 4, 4]
    for cus in (228, 256, 304):
        sizes = batch_sizes(cus)
        assert len(sizes) == 5
        for n in sizes:
            assert n % 8 == 0 or n * 3 * 16 > cus
