"""Float64 NumPy restatement of one TemporalBlock the way csrc/tcn.hip computes it, and the comparator of the TCN tests.

The restatement keeps the STRUCTURE of the kernels, because that structure is where they can go wrong:

    rows        planar [B][C][Tp], Tp = T rounded up to 32; frames >= T are never written (they hold STALE here)
    statistics  float64 (sum, sum of squares) partials, one per 128-frame tile of a (sample, channel) row (tcn_pw_k's
                epilogue); the consumer adds the partials of a row (IN) or of a whole sample (gLN) -- tcn_dw_k
    cLN         per-frame (mean, rstd) over the channels, [B][Tp], zero for frames >= T (tcn_cln_stats_k)
    depth-wise  a = ELU(norm(x)), zero outside [0, T), walked in segments of DW_SEG frames with a DW_HALO-frame halo
    point-wise  W @ (gamma * (d - mean) * rstd + beta), frames >= T masked, + residual

``fault=`` breaks exactly one of these on purpose (FAULTS below): tests/test_tcn.py checks that the comparator rejects
every one of them at the bound the GPU tests use, and that the clean restatement equals oracle/miso_oracle.tcn_forward.

The comparator measures a TCN output against the float64 oracle on the SAME input and bounds it by K times the distance
of the float32 oracle (stock torch on the CPU) from that truth, for the whole tensor and for the worst single frame.
"""
import numpy as np

PW_TT = 128                      # frames per point-wise workgroup = per statistics partial
DW_HALO = 64                     # largest dilation
DW_SEG = 2048 - 2 * DW_HALO      # output frames per depth-wise segment
EPS_IN = 1e-5
EPS_GLN = 1e-8
STALE = 0.75                     # what the never-written frames >= T of a row hold here

# K: a healthy kernel differs from the float64 truth by at most K times what the float32 oracle does.  The kernels sum in
# another order, use a fast ELU and (bf16x6) six-product split arithmetic: rounding-level effects.  A lost term or a wrong
# statistic is 10 ... 1e4 times the yardstick (tests/test_tcn.py prints the ratio of every fault).
K = 4.0
WHOLE_CAP = 1e-4                 # the bound test_long_utterance_no_frame_limit applies to tcn_out; never exceeded

FAULTS = {
    "gln_tile": "gLN outer-norm statistics without the partial of the last 128-frame tile",
    "in_tile": "IN statistics of one (sample, channel) row without the partial of the last 128-frame tile",
    "cln_sample": "cLN frame statistics of sample 1 read from sample 0",
    "seam": "depth-wise taps see zero across a segment seam (frame 1920)",
    "tail": "frames T .. Tq-1 of the padded row (stale values) leak into the depth-wise taps",
    "pw16": "point-wise product with both inputs rounded to 16 significant bits",
}
IN_TILE_ROW = (-1, 5)            # the (sample, channel) row of the "in_tile" fault


def frames_pitch(T):
    return (T + 31) // 32 * 32


def part_slots(T):
    return (T + PW_TT - 1) // PW_TT


def _elu(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))


def round_bits(v, bits=16):
    """v rounded to `bits` significant bits (round to nearest)"""
    m, e = np.frexp(v)
    return np.ldexp(np.round(m * 2.0 ** bits), e - bits).astype(v.dtype)


def tile_partials(v, T):
    """v [B, C, Tp] -> float64 [B, C, slots, 2]: (sum, sum of squares) over the valid frames of every 128-frame tile"""
    p = np.zeros(v.shape[:2] + (part_slots(T), 2), np.float64)
    for s in range(part_slots(T)):
        w = v[:, :, s * PW_TT:min((s + 1) * PW_TT, T)].astype(np.float64)
        p[:, :, s, 0] = w.sum(-1)
        p[:, :, s, 1] = (w * w).sum(-1)
    return p


def _w(sd, key, dtype):
    return np.asarray(sd[key]).astype(dtype)


def _outer_norm(x, part, sd, q, nt, T, fault, dtype):
    """the norm in front of the ELU on the whole padded row [B, C, Tp] (frames >= T: whatever comes out of the stale values)"""
    B, C, Tp = x.shape
    if nt == "IN":
        p = part.copy()
        if fault == "in_tile":
            p[IN_TILE_ROW[0], IN_TILE_ROW[1], -1] = 0.0
        st = p.sum(2)
        mean = st[..., 0] / T
        var = np.maximum(st[..., 1] / T - mean * mean, 0.0)
        return (x - mean[..., None].astype(dtype)) * (1.0 / np.sqrt(var + EPS_IN))[..., None].astype(dtype)
    if nt == "gLN":
        p = part[:, :, :-1] if fault == "gln_tile" else part
        st = p.sum((1, 2))
        mean = st[:, 0] / (C * T)
        var = np.maximum(st[:, 1] / (C * T) - mean * mean, 0.0)
        rstd = (1.0 / np.sqrt(var + EPS_GLN)).astype(dtype)
        return _w(sd, f"{q}.gamma", dtype) * ((x - mean[:, None, None].astype(dtype)) * rstd[:, None, None]) + _w(sd, f"{q}.beta", dtype)
    if nt == "cLN":
        v = x[:, :, :T]
        mean = np.zeros((B, 1, Tp), dtype)
        rstd = np.zeros((B, 1, Tp), dtype)
        mean[:, :, :T] = v.mean(1, keepdims=True)
        rstd[:, :, :T] = 1.0 / np.sqrt(((v - mean[:, :, :T]) ** 2).mean(1, keepdims=True) + dtype(EPS_GLN))
        if fault == "cln_sample":
            mean[1], rstd[1] = mean[0], rstd[0]
        return _w(sd, f"{q}.gamma", dtype) * ((x - mean) * rstd) + _w(sd, f"{q}.beta", dtype)
    sc = _w(sd, f"{q}.weight", np.float64) / np.sqrt(_w(sd, f"{q}.running_var", np.float64) + EPS_IN)      # BatchNorm1d, eval
    return (x - _w(sd, f"{q}.running_mean", dtype)[:, None]) * sc.astype(dtype)[:, None] + _w(sd, f"{q}.bias", dtype)[:, None]


def _depthwise(a, w, dil, T, fault):
    """a [B, C, Tp], zero (or, faulty, not) for frames >= T -> d [B, C, Tq]: segments of seg_f frames read from a row that holds
    the segment and a DW_HALO-frame halo on both sides, zero outside [0, Tq)"""
    B, C, _ = a.shape
    Tq = (T + 3) & ~3
    seg_f = min(Tq, DW_SEG)
    d = np.zeros((B, C, Tq), a.dtype)
    for ts in range(0, Tq, seg_f):
        row = np.zeros((B, C, seg_f + 2 * DW_HALO), a.dtype)
        lo, hi = max(ts - DW_HALO, 0), min(ts + seg_f + DW_HALO, Tq)
        if fault == "seam":
            lo, hi = max(ts, 0), min(ts + seg_f, Tq)
        row[:, :, lo - ts + DW_HALO:hi - ts + DW_HALO] = a[:, :, lo:hi]
        te = min(ts + seg_f, Tq)
        j = np.arange(ts, te) - ts + DW_HALO
        d[:, :, ts:te] = w[:, 1, None] * row[:, :, j] + w[:, 0, None] * row[:, :, j - dil] + w[:, 2, None] * row[:, :, j + dil]
    return d


def _half(x, part, sd, p_norm, p_ds, nt, dil, T, residual, fault, dtype):
    """ELU(outer norm) -> depth-wise dilated conv -> PReLU -> gLN -> point-wise conv (+ residual); returns the padded row
    and its tile partials"""
    B, C, Tp = x.shape
    Tq = (T + 3) & ~3
    a = _elu(_outer_norm(x, part, sd, p_norm, nt, T, fault, dtype))
    a[:, :, (Tq if fault == "tail" else T):] = 0
    d = _depthwise(a, _w(sd, f"{p_ds}.0.weight", dtype)[:, 0, :], dil, T, fault)
    slope = _w(sd, f"{p_ds}.1.weight", dtype)[0]
    d = np.where(d > 0, d, slope * d)[:, :, :T]
    d64 = d.astype(np.float64)
    mean = d64.mean((1, 2), keepdims=True)
    var = np.maximum((d64 * d64).mean((1, 2), keepdims=True) - mean * mean, 0.0)
    g = _w(sd, f"{p_ds}.2.gamma", dtype) * ((d - mean.astype(dtype)) * (1.0 / np.sqrt(var + EPS_GLN)).astype(dtype)) + _w(sd, f"{p_ds}.2.beta", dtype)
    wpw = _w(sd, f"{p_ds}.3.weight", dtype)[:, :, 0]
    if fault == "pw16":
        g, wpw = round_bits(g), round_bits(wpw)
    y = np.full((B, C, Tp), STALE, dtype)
    y[:, :, :T] = np.matmul(wpw, g)
    if residual is not None:
        y[:, :, :T] += residual[:, :, :T]
    return y, tile_partials(y, T)


def temporal_block(x, part, sd, r, blk, norm_type, T, fault=None, dtype=np.float64):
    """x + DS2(ELU(norm(DS1(ELU(norm(x)))))) of block (r, blk) on padded rows [B, 128, Tp] with their tile partials"""
    p = f"TCN.temporal_conv_net.{r}.{blk}.net"
    y, yp = _half(x, part, sd, f"{p}.0", f"{p}.2.net", norm_type, 2 ** blk, T, None, fault, dtype)
    return _half(y, yp, sd, f"{p}.3", f"{p}.5.net", norm_type, 2 ** blk, T, x, fault, dtype)


def tcn_forward(x, sd, norm_type="IN", fault=None, fault_blocks=None, dtype=np.float64):
    """x [B, 128, T] -> [B, 128, T]: the 2 x 7 TemporalBlocks.  `fault` (a key of FAULTS) is injected in the blocks listed in
    `fault_blocks` (indices 0 .. 13; None = all of them, as a faulty kernel would)."""
    assert fault is None or fault in FAULTS, fault
    x = np.asarray(x)
    B, C, T = x.shape
    cur = np.full((B, C, frames_pitch(T)), STALE, dtype)
    cur[:, :, :T] = x
    part = tile_partials(cur, T)
    for k in range(14):
        f = fault if (fault_blocks is None or k in fault_blocks) else None
        cur, part = temporal_block(cur, part, sd, k // 7, k % 7, norm_type, T, f, dtype)
    return cur[:, :, :T]


# ---- comparator ----------------------------------------------------------------------------------------------------------

def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def frame_err(y, truth):
    """[C, T] -> [T]: L2 over the channels of y - truth, relative to the L2 of truth, frame by frame"""
    y, truth = np.asarray(y, np.float64), np.asarray(truth, np.float64)
    return np.linalg.norm(y - truth, axis=0) / np.maximum(np.linalg.norm(truth, axis=0), 1e-300)


def compare(got, truth, y32):
    """got, truth, y32: [C, T] of ONE sample (the output under test, the float64 oracle, the float32 oracle on the same input)"""
    ferr = frame_err(got, truth)
    t = int(np.argmax(ferr))
    return {"err": rel_l2(got, truth), "e32": rel_l2(y32, truth), "ferr": float(ferr[t]), "t": t,
            "f32max": float(frame_err(y32, truth).max())}


def bounds(c, k=K):
    return min(k * c["e32"], WHOLE_CAP), k * c["f32max"]


def report(c, what):
    return (f"[tcn] {what}: err {c['err']:.3e} = {c['err'] / c['e32']:.2f} x e32 ({c['e32']:.3e}); worst frame t={c['t']}: "
            f"{c['ferr']:.3e} = {c['ferr'] / c['f32max']:.2f} x f32max ({c['f32max']:.3e})")


def check(got, truth, y32, what, k=K):
    """assert the two bounds; the message names the worst frame, so a seam or halo bug reports its own frame index"""
    got = np.asarray(got)
    assert got.shape == np.asarray(truth).shape, (what, got.shape, np.asarray(truth).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    c = compare(got, truth, y32)
    whole, frame = bounds(c, k)
    assert c["err"] <= whole, f"whole tensor over {whole:.3e} (K = {k:g}) -- " + report(c, what)
    assert c["ferr"] <= frame, f"frame t={c['t']} over {frame:.3e} (K = {k:g}) -- " + report(c, what)
    return c
