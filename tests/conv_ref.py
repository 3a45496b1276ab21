"""Float64 torch restatement of ONE conv level of the trunk (the first conv, an encoder level, a decoder level) with the places
where the conv kernels can go wrong made explicit, and the comparator of the conv-level tests.

The restatement uses the ops of oracle/miso_oracle.py (F.conv2d, F.conv_transpose2d, F.elu) but spells out what the oracle
leaves to torch, because that is where csrc/conv*.hip carry their own code:

    halo        every conv runs on an explicitly padded input: one frame before and after the T frames, and (DenseBlock convs,
                transposed convs) one frequency row before and after the F rows; the padding is zero
    statistics  the instance norm is (y - mean) * rstd from float64 (sum, sum of squares) over the T x F plane of a
                (sample, channel), the way the kernels' epilogues and consumers form it
    product     x * w of both operands as given

``fault=`` breaks exactly one of these on purpose (FAULTS below), in every conv of the level the fault applies to
(``where="all"``, as a faulty kernel would) or in the last such conv alone (``where="last"``: nothing downstream amplifies it).
tests/test_conv_levels.py checks that the clean restatement equals the oracle's level and that the comparator rejects every
fault at the bound the GPU tests use.

The comparator measures one sample [C, T, F] of a level's output against the float64 oracle on the SAME input and bounds it by K
times the distance of the float32 oracle (stock torch on the CPU) from that truth: for the whole tensor, the worst frame, the
worst frequency row and the worst channel, each against the same figure of the float32 oracle.

The channel widths the CPU and the GPU tests run are defined here once (WIDTH_SETS), with the layer list they give (conv_layers).
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import tcn_ref

K = tcn_ref.K                    # 4: never tuned on the device (tests/tcn_ref.py)
WHOLE_CAP = tcn_ref.WHOLE_CAP    # no level may be further than this from the truth, whatever the float32 oracle does
EPS_IN = 1e-5
STALE = 0.75                     # what a halo frame / row / padding frame holds when it is not the zero it should be
TT = 128                         # frames per tile of DIRECT, W1D, X6, FEW
WTT = 64                         # frames per tile of the Winograd kernel
STAT_ROW = (-1, 5)               # the (sample, channel) of the "stat_tile" / "stat_wtile" faults

FAULTS = {
    "halo_t": "frame T (the frame after the last) is read as a stale non-zero value instead of zero",
    "halo_f": "the row past the last frequency row is read as stale (DenseBlock and transposed convs: the others have no such row)",
    "stat_tile": "instance-norm statistics of one (sample, channel) without the last 128-frame tile",
    "stat_wtile": "instance-norm statistics of one (sample, channel) without the last 64-frame tile",
    "stat_sample": "sample 1 normalised with sample 0's statistics",
    "prod16": "product with both operands rounded to 16 significant bits",
    "drop2": "split-bf16 product without its second-order group: three 8-bit pieces per operand, only hh + hm + mh kept",
    "pad_leak": "padding frames [T, Tp) of the output (stale) counted in the statistics",
}

LEVELS = ("enc0_conv",) + tuple(f"enc{b}" for b in range(7)) + tuple(f"dec{b}" for b in range(7))

# ---- channel widths --------------------------------------------------------------------------------------------------------
# misonet_net_create admits every encoder list of positive multiples of 8 up to 128 with en[6] == 128 and de = en[::-1]; the conv
# kernels are written around DEFAULT.  The two other sets reach what DEFAULT never does (tests/test_lib_abi.py pins the kernel of
# every layer): f32w DenseBlocks that mix W1D + WINO and WINO + DIRECT (Cin > 192 or Cout > 64), WINO at 8 / 16 (the 16-row body
# alone) / 40 / 48 / 56 / 64 output channels, 64-channel DIRECT groups at 72 ... 128 output channels and up to 384 input channels,
# the stride-2 transposed layers at 8 / 16 / 40 / 48 / 56 / 64, dec0 at 72 and 128, a first layer of 40 output channels, bf16x6
# tiles with Cout & 31 in {8, 16, 24} at two and more channel groups, and a last layer of 6 / 8 channels (3 / 4 speakers), which
# is neither conv3x3_few nor the rows_in_m tile.  The small and odd widths sit on the rows with many frequency bins, the wide ones
# where F <= 31, so the float64 oracle of a sample costs about what DEFAULT's does.
# name: (encoder channels, num_spks); the decoder channels are the encoder's reversed
WIDTH_SETS = {
    "default": ((24, 32, 32, 32, 32, 64, 128), 2),
    "narrow_to_wide": ((8, 16, 40, 48, 56, 72, 128), 3),
    "wide_first": ((40, 24, 64, 8, 16, 128, 128), 4),
}
NARROW_TO_WIDE, WIDE_FIRST = WIDTH_SETS["narrow_to_wide"][0], WIDTH_SETS["wide_first"][0]
OTHER_WIDTHS = ("narrow_to_wide", "wide_first")
EN_F = (129, 127, 63, 31, 15, 7, 3, 1)             # frequency rows in front of encoder level b; EN_F[b + 1] behind it
DE_F = EN_F[::-1]                                  # in front of decoder level b; DE_F[b + 1] behind it


def widths(ws):
    """(en, de, num_spks) of a width set"""
    en, spks = WIDTH_SETS[ws]
    return tuple(en), tuple(en[::-1]), spks


def level_channels(ws, num_ch=6):
    """(EN, DE): EN[b] the channels in front of encoder level b (EN[0] the network input) and EN[b + 1] behind it; DE[b] the
    channels of EACH of the two inputs of decoder level b (the previous level's output and the skip) and DE[b + 1] behind it"""
    en, de, spks = widths(ws)
    return (2 * num_ch,) + en, de + (2 * spks,)


def state_dict(ws, seed=3):
    """seeded MISO_1 weights of a width set (6 microphones)"""
    from misonet_amd import weights as W
    en, de, spks = widths(ws)
    return W.make_state_dict(W.miso1_spec(num_spks=spks, en_ch=en, de_ch=de), seed=seed)


def conv_layers(ws, num_ch=6):
    """the 64 conv layers of MISO_1 in launch order (encoders, then decoders), as dicts: name, Cin, Cout, F (output rows), act
    (ELU + instance norm behind the conv), dense (a DenseBlock conv), block (the DenseBlock's name or None)"""
    EN, DE = level_channels(ws, num_ch)
    out = []

    def add(name, cin, cout, f, act, block):
        out.append({"name": name, "Cin": cin, "Cout": cout, "F": f, "act": act, "dense": block is not None, "block": block})

    for b in range(7):
        add(f"enc{b}.0", EN[b], EN[b + 1], EN_F[b + 1], b > 0, None)          # encoders.0.0.conv2d has no activation
        if b < 5:
            for i in range(5):
                add(f"enc{b}.db{i + 1}", (i + 1) * EN[b + 1], EN[b + 1], EN_F[b + 1], True, f"enc{b}")
    for b in range(7):
        cin = 2 * DE[b]
        if b >= 2:
            for i in range(5):
                add(f"dec{b}.db{i + 1}", cin + i * (cin // 2), cin // 2 if i < 4 else cin, DE_F[b], True, f"dec{b}")
        add(f"dec{b}.t", cin, DE[b + 1], DE_F[b + 1], b < 6, None)             # the last deconv has none
    return out

# one conv: state_dict prefix, transposed, frequency stride, frequency padding (plain convs), ELU + instance norm, position in a
# DenseBlock (None: not in one)
Conv = namedtuple("Conv", "prefix transposed sf padf act dense")


def frames_pitch(T):
    return (T + 31) // 32 * 32


def _dense(prefix):
    return [Conv(f"{prefix}.conv{i + 1}.0", False, 1, 1, True, i) for i in range(5)]


def level_convs(name, from_conv=False):
    """the convs of a level in execution order (oracle/miso_oracle.encoder_level / decoder_level)"""
    if name == "enc0_conv":
        return [Conv("encoders.0.0.conv2d", False, 1, 0, False, None)]
    b = int(name[3:])
    if name.startswith("enc"):
        if b == 0:
            return ([] if from_conv else level_convs("enc0_conv")) + _dense("encoders.0.1")
        first = [Conv(f"encoders.{b}.0.net.0", False, 1 if b == 6 else 2, 0, True, None)]
        return first + (_dense(f"encoders.{b}.1") if b < 5 else [])
    if b >= 2:
        last = Conv("decoders.6.1.deconv2d", True, 1, 0, False, None) if b == 6 else Conv(f"decoders.{b}.1.net.0", True, 2, 0, True, None)
        return _dense(f"decoders.{b}.0") + [last]
    return [Conv(f"decoders.{b}.0.net.0", True, 1 if b == 0 else 2, 0, True, None)]


def applies(fault, c):
    if fault == "halo_f":
        return c.transposed or c.padf == 1
    if fault in ("stat_tile", "stat_wtile", "stat_sample", "pad_leak"):
        return c.act
    return True


def round_bits(v, bits=16):
    """v rounded to `bits` significant bits (round to nearest)"""
    m, e = torch.frexp(v)
    return torch.ldexp(torch.round(m * 2.0 ** bits), e - bits).to(v.dtype)


def split3(v):
    """v = h + m + l (+ a remainder below 24 bits): three pieces of 8 significant bits, the way bf16x6 splits an operand"""
    h = round_bits(v, 8)
    m = round_bits(v - h, 8)
    return h, m, round_bits(v - h - m, 8)


def _tt(v, dtype):
    """a torch tensor of `dtype` (a copy of a NumPy array: the shared test inputs are read-only)"""
    return torch.tensor(v, dtype=dtype) if isinstance(v, np.ndarray) else v.to(dtype)


def _w(sd, key, dtype):
    return _tt(sd[key], dtype)


def _unit(x, w, bias, c, fault, by_taps=False):
    """conv (-> ELU -> instance norm) of one layer on [B, C, T, F]; `by_taps`: the conv as the sum of its nine taps, each a 1x1
    conv on a shifted view (another summation order than torch's 3x3 conv: an independent evaluation)"""
    B, _, T, Fin = x.shape
    pf = 1 if c.transposed else c.padf
    if c.transposed:
        Fout = (Fin - 1) * c.sf + 3

        def conv(a, ww, bb):
            # the padded transposed conv, cropped to the frames / rows the unpadded one with padding (1, 0) gives
            if not by_taps:
                return F.conv_transpose2d(a, ww, bb, stride=(1, c.sf))[:, :, 2:2 + T, c.sf:c.sf + Fout]
            Tp, Fp = a.shape[2:]
            full = a.new_zeros((B, ww.shape[1], Tp + 2, (Fp - 1) * c.sf + 3))
            for kt in range(3):
                for kf in range(3):
                    full[:, :, kt:kt + Tp, kf:kf + (Fp - 1) * c.sf + 1:c.sf] += F.conv2d(a, ww[:, :, kt, kf].t()[:, :, None, None])
            y = full[:, :, 2:2 + T, c.sf:c.sf + Fout]
            return y if bb is None else y + bb[None, :, None, None]
    else:
        Fout = (Fin + 2 * pf - 3) // c.sf + 1

        def conv(a, ww, bb):
            if not by_taps:
                return F.conv2d(a, ww, bb, stride=(1, c.sf))
            y = 0
            for kt in range(3):
                for kf in range(3):
                    y = y + F.conv2d(a[:, :, kt:kt + T, kf:kf + c.sf * (Fout - 1) + 1], ww[:, :, kt:kt + 1, kf:kf + 1], None, stride=(1, c.sf))
            return y if bb is None else y + bb[None, :, None, None]

    def padded(a, stale=True):
        ap = F.pad(a, (pf, pf, 1, 1))
        if stale and fault == "halo_t":
            ap[:, :, T + 1, :] = STALE
        if stale and fault == "halo_f":
            assert pf == 1
            ap[:, :, :, Fin + 1] = STALE
        return ap

    if fault == "prod16":
        y = conv(padded(round_bits(x)), round_bits(w), bias)
    elif fault == "drop2":
        (xh, xm, _), (wh, wm, _) = split3(x), split3(w)
        y = conv(padded(xh), wh, bias) + conv(padded(xh), wm, None) + conv(padded(xm), wh, None)
    else:
        y = conv(padded(x), w, bias)
    if not c.act:
        return y
    y = F.elu(y)
    y64 = y.double()
    s1, s2 = y64.sum((2, 3)), (y64 * y64).sum((2, 3))
    if fault in ("stat_tile", "stat_wtile"):
        tile = TT if fault == "stat_tile" else WTT
        assert T > tile, (fault, T)
        lost = y64[STAT_ROW[0], STAT_ROW[1], (T - 1) // tile * tile:]
        s1[STAT_ROW] -= lost.sum()
        s2[STAT_ROW] -= (lost * lost).sum()
    if fault == "pad_leak":
        npad = (frames_pitch(T) - T) * Fout
        s1 = s1 + npad * STALE
        s2 = s2 + npad * STALE * STALE
    mean = s1 / (T * Fout)
    var = (s2 / (T * Fout) - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + EPS_IN)
    if fault == "stat_sample":
        assert B >= 2
        mean[1], rstd[1] = mean[0].clone(), rstd[0].clone()
    return (y - mean[:, :, None, None].to(y.dtype)) * rstd[:, :, None, None].to(y.dtype)


@torch.no_grad()
def level(name, x, sd, skip=None, fault=None, where="all", dtype=torch.float64, from_conv=False, by_taps=False):
    """One level on its input: x [B, C, T, F] (a decoder level: the previous decoder output, with `skip` the matching encoder
    output).  `fault` (a key of FAULTS) goes into every conv of the level it applies to, or (`where="last"`) the last of them."""
    assert name in LEVELS and (fault is None or fault in FAULTS) and where in ("all", "last"), (name, fault, where)
    x = _tt(x, dtype)
    if name.startswith("dec"):
        x = torch.cat((x, _tt(skip, dtype)), dim=1)
    convs = level_convs(name, from_conv)
    hit = [k for k, c in enumerate(convs) if fault is not None and applies(fault, c)]
    assert fault is None or hit, f"fault {fault!r} does not apply to any conv of {name}"
    hit = set(hit if where == "all" else hit[-1:])
    feats = None
    for k, c in enumerate(convs):
        if c.dense == 0:
            feats = [x]
        inp = torch.cat(feats, dim=1) if c.dense is not None else x
        x = _unit(inp, _w(sd, c.prefix + ".weight", dtype), _w(sd, c.prefix + ".bias", dtype), c, fault if k in hit else None, by_taps)
        if c.dense is not None:
            feats.append(x)
    return x


@torch.no_grad()
def oracle_level(name, x, sd, skip=None, dtype=torch.float64, from_conv=False):
    """the same level by oracle/miso_oracle.py (the truth in float64, the yardstick in float32)"""
    from oracle import miso_oracle
    with miso_oracle.precision(dtype):
        x = _tt(x, dtype)
        if name == "enc0_conv":
            return miso_oracle.enc0_conv(x, sd)
        if name.startswith("enc"):
            return miso_oracle.encoder_level(int(name[3:]), x, sd, from_conv=from_conv)
        return miso_oracle.decoder_level(int(name[3:]), x, _tt(skip, dtype), sd)


def perturb_ulp(x, seed):
    """float32 x with every element moved by -1, 0 or +1 float32 ulp (seeded): how far two float32 evaluations of the same
    normalisation (the export kernel's tap, the consumer's on-load form) can be apart"""
    x = np.asarray(x, np.float32)
    step = np.random.default_rng(seed).integers(-1, 2, x.shape)
    return np.where(step > 0, np.nextafter(x, np.float32(np.inf)), np.where(step < 0, np.nextafter(x, np.float32(-np.inf)), x)).astype(np.float32)


# ---- comparator ----------------------------------------------------------------------------------------------------------

METRICS = ("whole", "frame", "row", "chan")
_KEEP = {"frame": 1, "row": 2, "chan": 0}         # the axis of [C, T, F] a metric keeps
_INDEX = {"frame": "t", "row": "f", "chan": "c"}


def rel_l2(a, b):
    return tcn_ref.rel_l2(a, b)


def _err_along(y, truth, keep):
    ax = tuple(a for a in range(3) if a != keep)
    return np.sqrt(((y - truth) ** 2).sum(ax)) / np.maximum(np.sqrt((truth ** 2).sum(ax)), 1e-300)


def compare(got, truth, y32):
    """got, truth, y32: [C, T, F] of ONE sample (the output under test, the float64 oracle, the float32 oracle on the same input).
    For every metric m: c[m] the error of `got`, c[m + "32"] the same figure of the float32 oracle, and for the frame / row /
    channel metrics the index of the worst one (c["t"], c["f"], c["c"])."""
    got, truth, y32 = (np.asarray(a, np.float64) for a in (got, truth, y32))
    c = {"whole": rel_l2(got, truth), "whole32": rel_l2(y32, truth)}
    for m, keep in _KEEP.items():
        e = _err_along(got, truth, keep)
        i = int(np.argmax(e))
        c[m], c[_INDEX[m]], c[m + "32"] = float(e[i]), i, float(_err_along(y32, truth, keep).max())
    return c


def ratios(c):
    return tuple(c[m] / max(c[m + "32"], 1e-300) for m in METRICS)


def bounds(c, k=K):
    b = {m: k * c[m + "32"] for m in METRICS}
    b["whole"] = min(b["whole"], WHOLE_CAP)
    return b


def report(c, what):
    r = ratios(c)
    return (f"[conv] {what}: whole {c['whole']:.3e} = {r[0]:.2f} x f32 ({c['whole32']:.3e}); frame t={c['t']}: {c['frame']:.3e} = "
            f"{r[1]:.2f} x; row f={c['f']}: {c['row']:.3e} = {r[2]:.2f} x; channel c={c['c']}: {c['chan']:.3e} = {r[3]:.2f} x")


def failures(c, k=K):
    """the metrics over their bound"""
    b = bounds(c, k)
    return [m for m in METRICS if not c[m] <= b[m]]


def check(got, truth, y32, what, k=K):
    """assert the four bounds; the message names the worst frame, row and channel, so a halo, tile or statistics bug reports
    its own index"""
    got = np.asarray(got)
    assert got.shape == np.asarray(truth).shape, (what, got.shape, np.asarray(truth).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    c = compare(got, truth, y32)
    b = bounds(c, k)
    for m in METRICS:
        where = "whole tensor" if m == "whole" else f"{m} {_INDEX[m]}={c[_INDEX[m]]}"
        assert c[m] <= b[m], f"{where} over {b[m]:.3e} (K = {k:g}) -- " + report(c, what)
    return c
