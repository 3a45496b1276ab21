"""Float64 NumPy restatement of the GLUE of the fused pass (csrc/api_pipeline.hip, pipeline_run_impl): which speaker plane of which
MISO_1 forward ends up where.  No device, no network: the inputs are the device's own raw MISO_1 outputs.

    raw[b*M + k]   = MISO_1(roll(mix[b], -k, axis=0)), [S, T, F] complex                      (tester.py:1033-1051; pack_k / stft_pack_k)
    sel_shift[b,m] = the permutation p that minimises  sum_i sum_{t,f} | |A_i| - |B_p(i)| |   (tester.py:1047-1064; pit_dist_k, pit_pick_k)
                     with A = raw[b*M + ref_ch], B = raw[b*M + m]
    sel_clean[b]   = the same with A = clean[b], B = raw[b*M + ref_ch]; identity without clean  (tester.py:906-915)
    sel_final[b,m,j] = sel_shift[b, m, sel_clean[b, j]]                                       (tester.py:1065 then 915; compose_sel_k)
    miso1[b,j,m]   = raw[b*M + m, sel_final[b,m,j]]                                           (unpack_k, mode 1)
    MISO_3 input of sample b*S + j = [mix[b] | beamformer(b, j) | miso1[b, j, ref_ch]]        (tester.py:936-939; assemble3_k)

Permutations are in ``itertools.permutations`` order and the first minimum wins (torch.argmin).

The device forms its distances in float32 per term (``sqrtf(re^2 + im^2)`` twice and one subtraction) and sums them in float64.  A term
is off by at most about 3 * 2^-24 * (|a| + |b|); every permutation's cost uses every A_i and every B_j exactly once, so every cost of an
item is off by at most  tol = 4 * 2^-24 * (sum_i sum |A_i| + sum_j sum |B_j|)  (the 4 is the slack over the 3).  An item whose best and
second-best float64 costs are more than 2 * tol apart is DECIDED: the device must pick the same permutation.  For an undecided item the
permutation the device picked must cost no more than 2 * tol above the minimum.  More than one undecided (b, m) in a case is refused:
another input seed is the remedy, not a wider cap.

What the device actually picked is read off its output (``observed_sel``): the glue moves planes and never computes on them, so
miso1[b,j,m] is bit for bit one of the S raw planes of sample b*M + m."""
from itertools import permutations

import numpy as np

MAX_UNDECIDED = 1
TOL_FACTOR = 4.0 * 2.0 ** -24


def perms(S):
    return np.array(list(permutations(range(S))), dtype=np.int64)


def _mag(x):
    x = np.asarray(x)
    return np.hypot(x.real.astype(np.float64), x.imag.astype(np.float64))


def pit(A, Bc):
    """A (anchors), Bc (candidates): magnitudes [S, T, F] float64 -> (perm [S], cost of every permutation [S!], margin between the
    best and the second-best cost (inf for S = 1), tol)"""
    S = A.shape[0]
    D = np.array([[np.abs(A[i] - Bc[j]).sum() for j in range(S)] for i in range(S)])
    P = perms(S)
    cost = D[np.arange(S)[None, :], P].sum(1)
    best = int(np.argmin(cost))                                # first minimum
    margin = float(np.partition(cost, 1)[1] - cost[best]) if len(cost) > 1 else float("inf")
    return P[best], cost, margin, TOL_FACTOR * float(A.sum() + Bc.sum())


def expected(raw, clean, M, S, ref_ch):
    """raw complex [B*M, S, T, F]; clean complex [B, S, T, F] or None.  Returns a dict: sel_shift [B,M,S], sel_clean [B,S], sel_final
    [B,M,S]; for the shift items cost_shift [B,M,S!], margin_shift / tol_shift [B,M]; for the clean items cost_clean [B,S!],
    margin_clean / tol_clean [B] (without clean: identity, no costs, margin inf)."""
    raw = np.asarray(raw)
    assert raw.ndim == 4 and raw.shape[1] == S and raw.shape[0] % M == 0 and 0 <= ref_ch < M, (raw.shape, M, S, ref_ch)
    B, nP = raw.shape[0] // M, len(perms(S))
    mag = _mag(raw).reshape(B, M, S, *raw.shape[2:])
    e = dict(sel_shift=np.zeros((B, M, S), np.int64), sel_clean=np.tile(np.arange(S), (B, 1)), cost_shift=np.zeros((B, M, nP)),
             margin_shift=np.zeros((B, M)), tol_shift=np.zeros((B, M)), cost_clean=None, margin_clean=np.full(B, np.inf),
             tol_clean=np.zeros(B))
    for b in range(B):
        for m in range(M):
            e["sel_shift"][b, m], e["cost_shift"][b, m], e["margin_shift"][b, m], e["tol_shift"][b, m] = pit(mag[b, ref_ch], mag[b, m])
    if clean is not None:
        cm = _mag(clean)
        assert cm.shape == (B, S) + raw.shape[2:], (cm.shape, raw.shape)
        e["cost_clean"] = np.zeros((B, nP))
        for b in range(B):
            e["sel_clean"][b], e["cost_clean"][b], e["margin_clean"][b], e["tol_clean"][b] = pit(cm[b], mag[b, ref_ch])
    e["sel_final"] = np.stack([e["sel_shift"][b][:, e["sel_clean"][b]] for b in range(B)])
    return e


def gather(raw, sel, M):
    """miso1[b,j,m] = raw[b*M + m, sel[b,m,j]]: [B, S, M, T, F]"""
    raw = np.asarray(raw)
    B, _, S = sel.shape
    out = np.empty((B, S, M) + raw.shape[2:], raw.dtype)
    for b in range(B):
        for m in range(M):
            for j in range(S):
                out[b, j, m] = raw[b * M + m, sel[b, m, j]]
    return out


# ---- the read path of steps 4b and 5 (csrc/kernels.hpp, src_row in pipeline mode) ---------------------------------------------------
# The beamformers and masks_from_est_k do not read the exported miso1: they read the raw planar MISO_1 output [B*M][2 S][F][Tp]
# through sel_final, with n = b*M + m, q = sel[n*S + spk], the real plane q and the imaginary plane S + q of sample n.

READ_FAULTS = {
    "mic0": "the sel row of microphone 0 for every microphone: sel[(b*M)*S + spk]",
    "item0": "the sel rows of item 0 for every item: sel[m*S + spk]",
    "inverse": "the inverse permutation: the q with sel[n*S + q] == spk",
    "imag": "the imaginary plane of speaker spk instead of q: (S + spk) * plane",
}
# what a geometry must have for a variant to be able to differ from the healthy read (S, B) -> bool.  Two speakers cannot see the
# inverse (every permutation of two is its own inverse), one item cannot see item0, one speaker nothing.
READ_FAULT_NEEDS = {
    "mic0": lambda S, B: S >= 2,
    "item0": lambda S, B: S >= 2 and B >= 2,
    "inverse": lambda S, B: S >= 3,
    "imag": lambda S, B: S >= 2,
}


def read_est(raw, sel, M, S, fault=None):
    """src_row in pipeline mode over every (b, spk, m): raw complex [B*M, S, T, F] (plane q of sample n = real plane q + i imaginary
    plane S + q), sel [B, M, S] -> what step 4b / 5 reads as the estimate of aligned speaker spk at microphone m, [B, S, M, T, F].
    ``fault``: one of READ_FAULTS planted in the index arithmetic."""
    assert fault is None or fault in READ_FAULTS, fault
    raw, sel = np.asarray(raw), np.asarray(sel)
    B = sel.shape[0]
    assert sel.shape == (B, M, S) and raw.shape[:2] == (B * M, S), (sel.shape, raw.shape, M, S)
    out = np.empty((B, S, M) + raw.shape[2:], raw.dtype)
    for b in range(B):
        for m in range(M):
            n = b * M + m
            row = sel[b, 0] if fault == "mic0" else sel[0, m] if fault == "item0" else sel[b, m]
            if fault == "inverse":
                row = np.argsort(row)
            for spk in range(S):
                q = int(row[spk])
                qi = spk if fault == "imag" else q
                out[b, spk, m] = raw[n, q].real + 1j * raw[n, qi].imag
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.complex64 else np.uint64)


def observed_sel(miso1, raw, M):
    """miso1 complex [B, S, M, T, F] (the pass's aligned estimates), raw complex [B*M, S, T, F] -> the selection the device used,
    [B, M, S]: for every (b, m, j) the ONE q with miso1[b,j,m] bit-equal to raw[b*M + m, q], in every frame and bin.  AssertionError
    if no q or more than one matches, or if the q of a (b, m) are not a permutation."""
    miso1, raw = np.asarray(miso1), np.asarray(raw)
    B, S = miso1.shape[:2]
    assert miso1.dtype == raw.dtype and miso1.shape[2] == M and raw.shape == (B * M, S) + miso1.shape[3:], (miso1.shape, raw.shape, M)
    mb, rb = _bits(miso1), _bits(raw)
    sel = np.zeros((B, M, S), np.int64)
    for b in range(B):
        for m in range(M):
            for j in range(S):
                hit = [q for q in range(S) if np.array_equal(mb[b, j, m], rb[b * M + m, q])]
                if len(hit) != 1:
                    near = [int((mb[b, j, m] != rb[b * M + m, q]).any(-1).sum()) for q in range(S)]
                    raise AssertionError(f"miso1[b={b}, j={j}, m={m}] is bit-equal to {len(hit)} of the {S} raw planes of sample "
                                         f"{b * M + m} (differing frames x bins per plane: {near})")
                sel[b, m, j] = hit[0]
            assert sorted(sel[b, m]) == list(range(S)), f"the selection of (b={b}, m={m}) is no permutation: {sel[b, m].tolist()}"
    return sel


def _index(S, p):
    return int(np.flatnonzero((perms(S) == np.asarray(p)[None, :]).all(1))[0])


def check(e, obs, ref_ch, what=""):
    """e: expected(...); obs: observed_sel(...) [B, M, S].  Applies the rules of the module docstring and returns a dict with the
    undecided (b, m), and the worst (smallest) margin / (2 tol) of the shift and of the clean items."""
    B, M, S = obs.shape
    with_clean = e["cost_clean"] is not None
    # the ref_ch forward against itself: distance matrix with a zero diagonal, so the identity unless two speakers coincide
    obs_clean = obs[:, ref_ch]                                   # sel_shift[b, ref_ch] = identity -> sel_final[b, ref_ch] = sel_clean[b]
    undecided, bad = [], []
    for b in range(B):
        assert e["margin_shift"][b, ref_ch] > 2 * e["tol_shift"][b, ref_ch] and list(e["sel_shift"][b, ref_ch]) == list(range(S)), \
            f"{what}: item {b}: the speakers of the ref_ch forward are not distinct (degenerate input)"
        clean_decided = e["margin_clean"][b] > 2 * e["tol_clean"][b]
        if not with_clean:
            if list(obs_clean[b]) != list(range(S)):
                bad.append(f"b={b}: no clean references, but the estimates at ref_ch are permuted by {obs_clean[b].tolist()}")
        elif clean_decided:
            if list(obs_clean[b]) != list(e["sel_clean"][b]):
                bad.append(f"b={b}: sel_clean observed {obs_clean[b].tolist()}, expected {e['sel_clean'][b].tolist()}")
        else:
            c = e["cost_clean"][b]
            if not c[_index(S, obs_clean[b])] <= c.min() + 2 * e["tol_clean"][b]:
                bad.append(f"b={b}: undecided clean item, but the observed {obs_clean[b].tolist()} costs "
                           f"{c[_index(S, obs_clean[b])] - c.min():.3e} over the minimum (2 tol = {2 * e['tol_clean'][b]:.3e})")
        inv = np.argsort(obs_clean[b])
        for m in range(M):
            decided = e["margin_shift"][b, m] > 2 * e["tol_shift"][b, m]
            if not (decided and clean_decided):
                undecided.append((b, m))
            obs_shift = obs[b, m][inv]                           # obs_final[j] = obs_shift[obs_clean[j]]
            if decided:
                if list(obs_shift) != list(e["sel_shift"][b, m]):
                    bad.append(f"(b={b}, m={m}): sel_shift observed {obs_shift.tolist()}, expected {e['sel_shift'][b, m].tolist()} "
                               f"(observed final {obs[b, m].tolist()}, expected {e['sel_final'][b, m].tolist()})")
            else:
                c = e["cost_shift"][b, m]
                if not c[_index(S, obs_shift)] <= c.min() + 2 * e["tol_shift"][b, m]:
                    bad.append(f"(b={b}, m={m}): undecided shift item, but the observed {obs_shift.tolist()} costs "
                               f"{c[_index(S, obs_shift)] - c.min():.3e} over the minimum (2 tol = {2 * e['tol_shift'][b, m]:.3e})")
            if decided and clean_decided and list(obs[b, m]) != list(e["sel_final"][b, m]):
                bad.append(f"(b={b}, m={m}): sel_final observed {obs[b, m].tolist()}, expected {e['sel_final'][b, m].tolist()}")
    assert not bad, f"{what}: " + "; ".join(dict.fromkeys(bad))
    assert len(undecided) <= MAX_UNDECIDED, (f"{what}: {len(undecided)} undecided (b, m) {undecided}: margin <= 2 tol on more than "
                                             f"{MAX_UNDECIDED} item; use another input seed")
    off = np.ones((B, M), bool)
    off[:, ref_ch] = False                                       # (the ref_ch forward against itself is not a measurement)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_shift = (e["margin_shift"] / (2 * e["tol_shift"]))[off]
        r_clean = e["margin_clean"] / (2 * e["tol_clean"]) if with_clean else np.array([np.inf])
    return dict(undecided=undecided, ratio_shift=float(r_shift.min()) if r_shift.size else float("inf"), ratio_clean=float(r_clean.min()))


def coverage(sel_shift, sel_clean):
    """what the selections of a case can tell apart: (some sel_shift[b,m] is not its own inverse, some pair sel_shift[b,m], sel_clean[b]
    does not commute, two batch items have different sel_clean) with the counts behind the first two"""
    sel_shift, sel_clean = np.asarray(sel_shift), np.asarray(sel_clean)
    B, M, S = sel_shift.shape
    non_inv = sum(1 for b in range(B) for m in range(M) if list(sel_shift[b, m][sel_shift[b, m]]) != list(range(S)))
    non_com = sum(1 for b in range(B) for m in range(M)
                  if list(sel_shift[b, m][sel_clean[b]]) != list(sel_clean[b][sel_shift[b, m]]))
    differ = any(list(sel_clean[b]) != list(sel_clean[0]) for b in range(1, B))
    return dict(non_involutive=non_inv, non_commuting=non_com, clean_differs=bool(differ))


def coverage_line(what, cov, res):
    return (f"[glue] {what}: non-involutive shifts {cov['non_involutive']}, non-commuting pairs {cov['non_commuting']}, clean differs "
            f"{cov['clean_differs']}, undecided {len(res['undecided'])} {res['undecided']}, worst margin/(2 tol) shift "
            f"{res['ratio_shift']:.3g} clean {res['ratio_clean']:.3g}")


def miso3_inputs(mix, bf, miso1, ref_ch):
    """The three MISO_3 input segments of the B*S samples, sample b*S + j: (mix[b] [M,T,F], bf[b,j] [1,T,F], miso1[b,j,ref_ch] [1,T,F])
    -> arrays [B*S, M, T, F], [B*S, 1, T, F], [B*S, 1, T, F]  (tester.py:936-939)"""
    mix, bf, miso1 = np.asarray(mix), np.asarray(bf), np.asarray(miso1)
    B, S = bf.shape[:2]
    return (np.repeat(mix, S, axis=0), bf.reshape((B * S, 1) + bf.shape[2:]),
            miso1[:, :, ref_ch].reshape((B * S, 1) + miso1.shape[3:]))


def planar(*segs):
    """complex segments [N, c, T, F] -> the trunk's input channels: the real parts of all segments, then the imaginary parts
    (model.py:360-364)"""
    return np.concatenate([s.real for s in segs] + [s.imag for s in segs], axis=1)


# ---- a NumPy emulation of pipeline_run_impl with one fault at a time (tests/test_pipeline_glue.py) ---------------------------------

FAULTS = {
    "compose_swapped": "sel_final = sel_clean[sel_shift[.]] instead of sel_shift[sel_clean[.]]",
    "gather_inverse": "the planes gathered with the inverse of sel_final",
    "anchor_shift0": "the anchors of the shift alignment taken from shift 0 instead of ref_ch",
    "roll_plus": "sample b*M + k = roll(mix[b], +k): channel md = (m + k) mod M",
    "clean_item0": "item 1 aligned with item 0's sel_clean",
    "clean_ignored": "sel_clean ignored",
    "est_mic0": "the MISO_3 estimate plane taken at microphone 0 instead of ref_ch",
    "est_speaker_j": "the MISO_3 estimate plane taken from speaker j instead of sel_final[b, ref_ch, j]",
    "est_re_im": "real and imaginary estimate planes swapped in the MISO_3 input",
    "unpack_last_frame": "frame T - 1 not written by the unpack (left at zero)",
}
BLIND_AT_S2 = ("compose_swapped", "gather_inverse")


def emulate(net, mix, clean, M, S, ref_ch, fault=None):
    """pipeline_run_impl in NumPy.  net: [N, M, T, F] complex -> [N, S, T, F] (deterministic); mix [B, M, T, F]; clean [B, S, T, F] or
    None.  The beamformer planes are a stand-in (the mean of the aligned estimates over the microphones): the glue only places them.
    Returns dict(miso1 [B,S,M,T,F], bf [B,S,T,F], in3 [B*S, 2(M+2), T, F] float, sel [B,M,S])."""
    assert fault is None or fault in FAULTS, fault
    B = mix.shape[0]
    rolled = np.stack([np.roll(mix[b], k if fault == "roll_plus" else -k, axis=0) for b in range(B) for k in range(M)])
    raw = net(rolled)
    mag = _mag(raw).reshape(B, M, S, *raw.shape[2:])
    anchor = 0 if fault == "anchor_shift0" else ref_ch
    sel_shift = np.array([[pit(mag[b, anchor], mag[b, m])[0] for m in range(M)] for b in range(B)])
    sel_clean = np.tile(np.arange(S), (B, 1))
    if clean is not None and fault != "clean_ignored":
        cm = _mag(clean)
        sel_clean = np.array([pit(cm[b], mag[b, ref_ch])[0] for b in range(B)])
        if fault == "clean_item0" and B > 1:
            sel_clean[1] = sel_clean[0]
    if fault == "compose_swapped":
        sel = np.stack([sel_clean[b][sel_shift[b]] for b in range(B)])
    else:
        sel = np.stack([sel_shift[b][:, sel_clean[b]] for b in range(B)])
    miso1 = gather(raw, np.argsort(sel, axis=-1) if fault == "gather_inverse" else sel, M)
    bf = miso1.mean(axis=2)
    est = np.stack([raw[b * M + (0 if fault == "est_mic0" else ref_ch), j if fault == "est_speaker_j" else sel[b, ref_ch, j]]
                    for b in range(B) for j in range(S)])[:, None]
    if fault == "est_re_im":
        est = est.imag + 1j * est.real
    in3 = planar(np.repeat(mix, S, axis=0), bf.reshape((B * S, 1) + bf.shape[2:]), est)
    if fault == "unpack_last_frame":
        miso1 = miso1.copy()
        miso1[..., -1, :] = 0
    return dict(miso1=miso1, bf=bf, in3=in3, sel=sel)


def judge(mix, clean, raw, got, M, S, ref_ch, what=""):
    """Everything the device test asserts about the glue, on emulated (or real) results: the observed selection against the
    restatement, the aligned estimates against the gather of raw, the MISO_3 input planes against (mix, bf, miso1 at ref_ch)."""
    e = expected(raw, clean, M, S, ref_ch)
    obs = observed_sel(got["miso1"], raw, M)
    res = check(e, obs, ref_ch, what)
    assert np.array_equal(_bits(got["miso1"]), _bits(gather(raw, obs, M)))
    want3 = planar(*miso3_inputs(mix, got["bf"], got["miso1"], ref_ch))
    assert got["in3"].shape == want3.shape, (got["in3"].shape, want3.shape)
    diff = [c for c in range(want3.shape[1]) if not np.array_equal(got["in3"][:, c], want3[:, c])]
    assert not diff, f"{what}: MISO_3 input channels {diff} differ from [mix | bf | miso1 at ref_ch]"
    return e, obs, res
