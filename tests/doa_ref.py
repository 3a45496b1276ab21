"""NumPy float64 restatement of the source localisation of csrc/doa.hip (include/misonet.h misonet_doa): the
SRP, SRP-PHAT and MUSIC maps of a mixture over a delay table, and their peaks.  It states the definition on its own -- the
eigenpairs come from np.linalg.eigh, the frame sum runs in a selectable order (``frame_order``: the floor every bar is taken
from), the peak rule is written out -- and holds the case lists, the bars (``figures``) and the planted faults (``plant``) of
tests/test_doa.py and tests/test_gpu_doa.py.  pyroomacoustics is not available: nothing here is compared against it."""
import contextlib

import numpy as np

KINDS = ("srp", "srp_phat", "music")
RANK_TOL = 1e-12
FAULTS = ("conj_phase", "no_diag", "drop_pair", "no_phat", "bin_off", "seam_off", "used_nodiv", "subspace_swap", "class_swap")
_FAULT = None


@contextlib.contextmanager
def plant(fault):
    """run the restatement with one fault: conjugated steering phase, lost diagonal, one dropped microphone pair, PHAT skipped,
    bin index off by one, block seam off by one frame, ``used`` not dividing, the signal subspace taken for the noise subspace,
    a class reading another class's weights"""
    global _FAULT
    assert fault in FAULTS, fault
    _FAULT = fault
    try:
        yield
    finally:
        _FAULT = None


def blocks(T, block, hop):
    """(block, hop, N) resolved; ValueError for block > T"""
    if block < 0 or hop < 0 or block > T or T < 1:
        raise ValueError("block must be in [0, T], hop >= 0")
    if block == 0:
        return T, T, 1
    hop = hop or block
    return block, hop, 1 + (T - block) // hop


def omega(F, fs):
    nfft = 2 * (F - 1) if F > 1 else 2
    return 2.0 * np.pi * np.arange(F, dtype=np.float64) * fs / nfft


def cov(mix, weight, kind, S, block=0, hop=0, f_lo=0, f_hi=None, frame_order=None):
    """step 1 -> (C complex128 [B, K, N, F, M, M], state int [B, K, N, F]: 0 used, 1 non-finite, 2 skipped, 3 outside the band)"""
    x = np.asarray(mix).astype(np.complex128)
    B, F, M, T = x.shape
    f_hi = F - 1 if f_hi is None else f_hi
    w = np.ones((B, 1, F, T)) if weight is None else np.asarray(weight).astype(np.float64)
    K = w.shape[1]
    if _FAULT == "class_swap" and K > 1:
        w = np.roll(w, -1, axis=1)
    block, hop, N = blocks(T, block, hop)
    start = np.arange(N) * hop + (1 if _FAULT == "seam_off" else 0)
    order = np.arange(block) if frame_order is None else np.random.default_rng(frame_order).permutation(block)
    okx = np.isfinite(x.real) & np.isfinite(x.imag)
    okw = np.isfinite(w)
    xs = np.where(okx, x, 0.0)
    ws = np.where(okw, w, 0.0)
    if kind == "srp_phat" and _FAULT != "no_phat":
        a = np.sqrt(xs.real * xs.real + xs.imag * xs.imag)
        xs = np.where(a > 0, xs / np.where(a > 0, a, 1.0), 0.0)
    R = np.zeros((B, K, N, F, M, M), np.complex128)
    badx = np.zeros((B, N, F), bool)
    badw = np.zeros((B, K, N, F), bool)
    for tt in order:
        idx = np.minimum(start + tt, T - 1)                               # [N]
        xt = xs[:, :, :, idx].transpose(0, 3, 1, 2)                       # [B, N, F, M]
        wt = ws[:, :, :, idx].transpose(0, 1, 3, 2)                       # [B, K, N, F]
        R += wt[..., None, None] * (xt[..., :, None] * np.conj(xt[..., None, :]))[:, None]
        badx |= ~okx[:, :, :, idx].all(axis=2).transpose(0, 2, 1)
        badw |= ~okw[:, :, :, idx].transpose(0, 1, 3, 2)
    state = np.zeros((B, K, N, F), np.int64)
    tr = np.einsum("...mm->...", R).real
    state[tr == 0] = 2
    state[badx[:, None] | badw] = 1
    if kind == "music":
        lam, vec = np.linalg.eigh(np.where((state == 0)[..., None, None], R, 0.0))      # ascending
        lam, vec = lam[..., ::-1], vec[..., ::-1]
        low = (lam[..., S - 1] <= RANK_TOL * lam[..., 0]) & (state == 0)
        state[low] = 2
        e = vec[..., :S] if _FAULT == "subspace_swap" else vec[..., S:]
        R = np.einsum("...ik,...jk->...ij", e, np.conj(e)) / M
    C = np.where((state == 0)[..., None, None], R, 0.0)
    band = np.zeros(F, bool)
    band[f_lo:f_hi + 1] = True
    state[..., ~band] = 3
    C[..., ~band, :, :] = 0.0
    return C, state


def steer(C, state, tau, fs, kind):
    """step 2 -> (q float64 [B, K, N, D], used int [B, K, N])"""
    B, K, N, F, M, _ = C.shape
    tau = np.asarray(tau, np.float64)
    tau = tau[None] if tau.ndim == 2 else tau
    D = tau.shape[1]
    om = omega(F, fs)
    q = np.zeros((B, K, N, D))
    used = (state == 0).sum(axis=-1)
    iu, ju = np.triu_indices(M, 1)
    if _FAULT == "drop_pair":
        iu, ju = iu[:-1], ju[:-1]
    for f in range(F):
        on = state[..., f] == 0                                           # [B, K, N]
        if not on.any():
            continue
        o = om[min(f + 1, F - 1)] if _FAULT == "bin_off" else om[f]
        z = np.exp((-1j if _FAULT == "conj_phase" else 1j) * o * tau)     # [Bg, D, M]
        ph = (z[:, :, iu] * np.conj(z[:, :, ju]))[:, None, None]          # [Bg, 1, 1, D, P]
        cf = C[:, :, :, f]
        pair = np.einsum("bknp,bkndp->bknd", cf[..., iu, ju], np.broadcast_to(ph, (B, K, N) + ph.shape[3:])).real
        diag = 0.0 if _FAULT == "no_diag" else np.einsum("...mm->...", cf).real[..., None]
        q += np.where(on[..., None], diag + 2.0 * pair, 0.0)
    if kind == "music" and _FAULT != "used_nodiv":
        q = np.where(used[..., None] > 0, q / np.maximum(used, 1)[..., None], 0.0)
    return q, used


def peaks(q, pts, S, kind, min_sep):
    """step 3 -> (peak int32 [B, K, N, S], value [B, K, N, S], margin [B, K, N, S]: the distance of the taken candidate to the
    next one left, relative to max q - min q; inf where no other is left or the map is flat)"""
    pts = np.asarray(pts, np.float64)
    lead = q.shape[:-1]
    peak = np.full(lead + (S,), -1, np.int32)
    value = np.zeros(lead + (S,))
    margin = np.full(lead + (S,), np.inf)
    sign = -1.0 if kind == "music" else 1.0
    for at in np.ndindex(*lead):
        v = q[at]
        rng = v.max() - v.min()
        alive = np.ones(v.shape[0], bool)
        for r in range(S):
            if not alive.any():
                break
            sv = np.where(alive, sign * v, -np.inf)
            best = int(np.argmax(sv))                                     # the first maximum: ties to the lower index
            peak[at + (r,)], value[at + (r,)] = best, v[best]
            rest = alive.copy()
            rest[best] = False
            if rest.any() and rng > 0:
                margin[at + (r,)] = (sv[best] - sv[rest].max()) / rng
            dx, dy, dz = (pts - pts[best]).T
            alive &= ~(dx * dx + dy * dy + dz * dz < min_sep * min_sep)
            alive[best] = False
    return peak, value, margin


def localize(mix, tau, pts, fs, kind="srp_phat", S=1, block=0, hop=0, f_lo=0, f_hi=None, min_sep=0.0, weight=None, frame_order=None):
    """the whole definition -> dict(q, peak, value, margin, used, fail, C, state)"""
    C, state = cov(mix, weight, kind, S, block, hop, f_lo, f_hi, frame_order)
    q, used = steer(C, state, tau, fs, kind)
    fail = ((state == 1).any(axis=-1) * 1 + (used == 0) * 2).astype(np.int32)
    peak, value, margin = peaks(q, pts, S, kind, min_sep)
    return dict(q=q, peak=peak, value=value, margin=margin, used=used.astype(np.int32), fail=fail, C=C, state=state)


def cov_steer(mix, tau, fs, kind, S=1, block=0, hop=0, f_lo=0, f_hi=None, weight=None, frame_order=None):
    """steps 1 and 2 only -> q: what the bars need of the permuted frame order"""
    C, state = cov(mix, weight, kind, S, block, hop, f_lo, f_hi, frame_order)
    return steer(C, state, tau, fs, kind)[0]


# ---- the bars -------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    d = np.linalg.norm(np.ravel(b))
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / (d if d > 0 else 1.0))


def figures(got, want, perm):
    """{name: (value, bar)} of a map against the restatement: rel-L2 and the worst candidate's error relative to max q - min q,
    each held under max(100 x the restatement's own difference under a permuted frame order, 1e-12); a flat map (one bin at
    omega = 0, a map of zeros) is judged relative to its level instead"""
    rng = float(want.max() - want.min())
    rng = rng if rng > 0 else (float(np.abs(want).max()) or 1.0)
    cand = lambda a: float(np.abs(a - want).max() / rng)
    return {"rel_l2": (rel_l2(got, want), max(100.0 * rel_l2(perm, want), 1e-12)),
            "cand": (cand(got), max(100.0 * cand(perm), 1e-12))}


def missed(fig):
    return {k: v for k, v in fig.items() if not v[0] <= v[1]}


PEAK_MARGIN = 1e-9


# ---- geometry (restated, not imported from the package) -----------------------------------------------------------------------
def circle(M, radius=0.05, z=0.0):
    a = 2.0 * np.pi * np.arange(M) / M
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.full(M, z)], axis=1)


def azimuths(D):
    a = 2.0 * np.pi * np.arange(D) / D
    return np.stack([np.cos(a), np.sin(a), np.zeros(D)], axis=1)


def far_delays(mic, dirs, c=343.0):
    mic = np.asarray(mic, np.float64)
    return -(np.asarray(dirs, np.float64) @ (mic - mic.mean(axis=0)).T) / c


def plane_wave_scene(M, seed, D=72, T=64, F=129, fs=16000.0, snr_db=20.0, min_gap_deg=30.0, B=1):
    """circular array of M microphones, 5 cm radius, D azimuths, two plane waves on grid azimuths at least min_gap_deg apart, white
    sources and noise at snr_db -> (mix complex64 [B, F, M, T], tau [D, M], dirs [D, 3], truth int [B, 2])"""
    rng = np.random.default_rng(seed)
    mic, dirs = circle(M), azimuths(D)
    tau = far_delays(mic, dirs)
    om = omega(F, fs)
    gap = int(np.ceil(min_gap_deg / (360.0 / D)))
    mix = np.zeros((B, F, M, T), np.complex128)
    truth = np.zeros((B, 2), np.int64)
    for b in range(B):
        while True:
            d = rng.choice(D, 2, replace=False)
            if gap <= abs(int(d[0]) - int(d[1])) <= D - gap:
                break
        truth[b] = np.sort(d)
        for s in range(2):
            sig = (rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T))) / np.sqrt(2.0)
            mix[b] += np.exp(-1j * om[:, None] * tau[truth[b, s]][None, :])[:, :, None] * sig[:, None, :]
        noise = (rng.standard_normal((F, M, T)) + 1j * rng.standard_normal((F, M, T))) / np.sqrt(2.0)
        mix[b] += noise * np.sqrt(2.0 * 10.0 ** (-snr_db / 10.0))
    return mix.astype(np.complex64), tau, dirs, truth


SCENE_M = (3, 6, 8)
SCENE_SEEDS = (0, 1, 2, 3)               # every seed tried is kept: 12 scenes
SCENE_BAND = (4, 100)


def grid_distance(a, b, D):
    d = np.abs(np.asarray(a) - np.asarray(b)) % D
    return np.minimum(d, D - d)


# ---- the GPU cases --------------------------------------------------------------------------------------------------------------
def gpu_cases(tile, chunk):
    """dicts of B, K, Bg, F, M, T, D, S, block, hop, f_lo, f_hi, weights ("none", "random", "zero": zero on the last class),
    min_sep, seed: every size of the issue's lists at least once, the others at small defaults"""
    base = dict(B=1, K=1, Bg=1, F=33, M=4, T=24, D=37, S=2, block=0, hop=0, f_lo=2, f_hi=30, weights="none", min_sep=0.3)
    out = []

    def add(tag, **kw):
        c = dict(base, **kw)
        c["tag"] = tag
        c["seed"] = len(out)
        if c["weights"] == "none":
            assert c["K"] == 1
        out.append(c)

    for D in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
        add(f"D{D}", D=D, S=1 if D == 1 else 2)
    for nb in (chunk - 1, chunk, chunk + 1):
        add(f"band{nb}", f_lo=3, f_hi=3 + nb - 1)
    for F in (1, 2, 129):
        add(f"F{F}-onebin", F=F, f_lo=F - 1, f_hi=F - 1)
    for M in (2, 3, 5, 6, 8):
        add(f"M{M}", M=M, S=1 if M == 2 else 2)
    for M, top in ((3, 2), (6, 4)):
        for S in range(1, top + 1):
            add(f"M{M}-S{S}", M=M, S=S, T=40, min_sep=0.2)
    for T in (1, 2, 63, 64, 65, 200):
        add(f"T{T}", T=T, f_hi=12 if T > 100 else 30)
    for T in (24, 200):
        for bh in ((0, 0), (16, 16), (16, 8), (T, 1)):
            add(f"T{T}-block{bh[0]}-hop{bh[1]}", T=T, block=bh[0], hop=bh[1], f_hi=9)
    for B in (1, 3):
        for K in (1, 3):
            for Bg in sorted({1, B}):
                add(f"B{B}-K{K}-Bg{Bg}", B=B, K=K, Bg=Bg, weights="random", block=8, hop=8, f_hi=12)
    add("weights-zero-class", B=2, K=3, weights="zero")
    add("weights-none-B3", B=3, Bg=3)
    return out


def case_kind_S(case, kind):
    """music cannot take S = M: its S is min(S, M - 1)"""
    return min(case["S"], case["M"] - 1) if kind == "music" else case["S"]


def case_inputs(case):
    """(mix complex64 [B, F, M, T], weight float32 [B, K, F, T] or None, tau [Bg, D, M], pts [D, 3]): two planted plane waves in
    noise at 10 dB on a random planar array of about 5 cm, candidates on a circle (so every map has one clear order)"""
    c = case
    rng = np.random.default_rng(1000 + c["seed"])
    B, K, Bg, F, M, T, D = (c[k] for k in ("B", "K", "Bg", "F", "M", "T", "D"))
    fs = 16000.0
    om = omega(F, fs)
    pts = azimuths(D)
    tau = np.zeros((Bg, D, M))
    for g in range(Bg):
        mic = np.concatenate([rng.uniform(-0.05, 0.05, (M, 2)), np.zeros((M, 1))], axis=1)
        tau[g] = far_delays(mic, pts)
    mix = np.zeros((B, F, M, T), np.complex128)
    for b in range(B):
        tb = tau[b if Bg > 1 else 0]
        for s, d in enumerate(rng.choice(D, min(2, D), replace=False)):
            sig = (rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T))) * (1.0 - 0.3 * s)
            mix[b] += np.exp(-1j * om[:, None] * tb[d][None, :])[:, :, None] * sig[:, None, :]
        mix[b] += 0.3 * (rng.standard_normal((F, M, T)) + 1j * rng.standard_normal((F, M, T)))
    weight = None
    if c["weights"] != "none":
        weight = rng.uniform(0.0, 1.0, (B, K, F, T)).astype(np.float32)
        if c["weights"] == "zero":
            weight[:, K - 1] = 0.0
    return mix.astype(np.complex64), weight, tau, pts
