"""Float64 NumPy restatement of the room simulator (csrc/room.hip): image-source RIRs of a shoebox and the
scene mixer, with the hooks the tests need -- ``image_order`` permutes the sum over the kept images (the restatement's own
rounding, which sets the bars), ``fault`` plants one of FAULTS / MIX_FAULTS -- and the case generators.  No GPU, no library.
The project's own definition in the Allen & Berkley (1979) family; not compared against pyroomacoustics, gpuRIR, rir_generator
or sms_wsj."""
import numpy as np

W = 80                       # support of the fractional-delay kernel in samples
MAX_N = 255                  # the largest image index per axis
MAX_IMAGES = 2 ** 27
TILE = 256                   # misonet_room_tile(), for the fault that needs it (the tests check it against the library)
NEAR = 1e-3

FAULTS = ("swap_exp", "lost_octant", "beta_x1_for_y1", "window_shift", "support_w", "tile_first_only", "wrap", "inv_d2")
MIX_FAULTS = ("split_off_by_one", "lost_source", "f32_acc")


def orders(room, fs, Lh, c=343.0):
    """N_i = ceil((Lh + W/2) c / (fs 2 L_i)), as floats (they may be inf)"""
    room = np.asarray(room, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.ceil((float(Lh) + W / 2.0) * c / (fs * 2.0 * room))


def check(room, beta, s, r, fs, Lh, c=343.0):
    """flag bits 0 and 2 of one pair"""
    room, beta, s, r = (np.asarray(a, np.float64) for a in (room, beta, s, r))
    bad = not (np.isfinite(room).all() and (room > 0).all())
    bad = bad or not ((s >= 0) & (s <= room)).all() or not ((r >= 0) & (r <= room)).all()      # a NaN fails
    bad = bad or not ((beta >= 0) & (beta < 1)).all()
    if bad:
        return 1
    N = orders(room, fs, Lh, c)
    if not (N <= MAX_N).all() or not 8.0 * np.prod(2.0 * N + 1.0) <= MAX_IMAGES:
        return 4
    return 0


def images(room, beta, s, r, fs, Lh, c=343.0, max_order=None, fault=None):
    """The kept images of one pair in the enumeration order: (d, g, near), near = some kept image was closer than 1e-3 m
    (it is dropped)."""
    room, beta, s, r = (np.asarray(a, np.float64) for a in (room, beta, s, r))
    N = orders(room, fs, Lh, c).astype(int)
    d2ax, gax, oax = [], [], []
    for i in range(3):
        n = np.arange(-N[i], N[i] + 1)[:, None]
        q = np.arange(2)[None, :]
        off = (1.0 - 2.0 * q) * s[i] + 2.0 * n * room[i] - r[i]
        k0, k1 = np.abs(n - q), np.abs(n) + 0 * q
        if fault == "swap_exp":
            k0, k1 = k1, k0
        b0, b1 = beta[2 * i], beta[2 * i + 1]
        if fault == "beta_x1_for_y1" and i == 1:
            b1 = beta[1]
        d2ax.append(off * off)
        gax.append(np.power(b0, k0.astype(np.float64)) * np.power(b1, k1.astype(np.float64)))     # 0 ** 0 = 1
        oax.append(k0 + k1)

    def grid(t):                                           # [nx, ny, nz, qx, qy, qz]: C order is the enumeration order
        return (t[0][:, None, None, :, None, None], t[1][None, :, None, None, :, None], t[2][None, None, :, None, None, :])

    x, y, z = grid(d2ax)
    d2 = ((x + y) + z).ravel()
    x, y, z = grid(gax)
    g = ((x * y) * z).ravel()
    x, y, z = grid(oax)
    rho = ((x + y) + z).ravel()
    keep = g > 0
    if max_order is not None and max_order >= 0:
        keep &= rho <= max_order
    if fault == "lost_octant":
        keep &= (np.arange(keep.size) % 8) != 5
    d = np.sqrt(d2[keep])
    g = g[keep]
    near = d < NEAR
    return d[~near], g[~near], bool(near.any())


def rir_pair(room, beta, s, r, fs, Lh, c=343.0, max_order=None, image_order=None, fault=None, return_count=False):
    """h [Lh] and the flags of one source-microphone pair.  ``image_order``: None, or a seed: the kept images are summed in
    that permutation of the enumeration order."""
    flag = check(room, beta, s, r, fs, Lh, c)
    h = np.zeros(Lh)
    if flag:
        return (h, flag, 0) if return_count else (h, flag)
    d, g, near = images(room, beta, s, r, fs, Lh, c, max_order, fault)
    if image_order is not None:
        p = np.random.default_rng(image_order).permutation(d.size)
        d, g = d[p], g[p]
    tau = d * fs / c
    a = g / (4.0 * np.pi * (d * d if fault == "inv_d2" else d))
    half = float(W) if fault == "support_w" else W / 2.0
    span = int(2 * half) + 1
    k = np.arange(span)[None, :]
    for i0 in range(0, d.size, 1 << 16):                   # np.add.at adds one by one in index order: the sum stays sequential
        t = tau[i0:i0 + (1 << 16), None]
        n = (np.floor(t - half).astype(np.int64) + 1) + k
        x = n - t
        sinc = np.sin(np.pi * x) / np.where(x == 0.0, 1.0, np.pi * x)
        sinc = np.where(x == 0.0, 1.0, sinc)
        xw = x + 1.0 if fault == "window_shift" else x
        v = a[i0:i0 + (1 << 16), None] * (0.5 * (1.0 + np.cos(2.0 * np.pi * xw / W))) * sinc
        ok = (np.abs(x) < half) & (n >= 0)
        if fault == "wrap":
            ok &= n < 2 * Lh
            n = n % Lh
        else:
            ok &= n < Lh
        if fault == "tile_first_only":
            first = np.maximum(n[:, :1], 0)
            ok &= (n // TILE) == (first // TILE)
        np.add.at(h, n[ok], v[ok])
    flag |= 2 if near else 0
    return (h, flag, int(d.size)) if return_count else (h, flag)


def rir(room, beta, src, mic, fs, Lh, c=343.0, max_order=None, image_order=None, fault=None):
    """room [3] or [B, 3], beta [6] or [B, 6], src [S, 3] or [B, S, 3], mic [M, 3] or [B, M, 3] -> (rir float64 [(B,) S, M, Lh],
    fail int32 [(B,) S, M])"""
    room, beta, src, mic = (np.asarray(a, np.float64) for a in (room, beta, src, mic))
    if src.ndim == 2:
        h, f = rir(room[None], beta[None], src[None], mic[None], fs, Lh, c, max_order, image_order, fault)
        return h[0], f[0]
    B, S, M = src.shape[0], src.shape[1], mic.shape[1]
    h = np.zeros((B, S, M, Lh))
    f = np.zeros((B, S, M), np.int32)
    for b in range(B):
        for s in range(S):
            for m in range(M):
                h[b, s, m], f[b, s, m] = rir_pair(room[b], beta[b], src[b, s], mic[b, m], fs, Lh, c, max_order, image_order, fault)
    return h, f


def direct_sample(src, mic, fs, c=343.0):
    """floor of the smallest direct-path delay over the microphones, per source: src [S, 3], mic [M, 3] -> int [S]"""
    src, mic = np.asarray(src, np.float64), np.asarray(mic, np.float64)
    d = np.sqrt(((src[:, None, :] - mic[None, :, :]) ** 2).sum(-1))
    return np.floor(d.min(1) * fs / c).astype(np.int64)


def mix(x, h, split=None, Lo=None, fault=None):
    """x float32 [S, L], h float64 [S, M, Lh], split int [S] or None -> (images, early, mix) in float64, NOT rounded:
    [S, M, Lo], [S, M, Lo], [M, Lo].  np.convolve in float64 is the reference (its order of summation is its own)."""
    x = np.asarray(x)
    S, L = x.shape
    M, Lh = h.shape[1], h.shape[2]
    Lo = L + Lh - 1 if Lo is None else Lo
    split = np.full(S, Lh) if split is None else np.asarray(split)
    img, early = np.zeros((S, M, Lo)), np.zeros((S, M, Lo))
    x64 = x.astype(np.float64)
    for s in range(S):
        sp = int(np.clip(split[s] + (1 if fault == "split_off_by_one" else 0), 0, Lh))
        for m in range(M):
            if fault == "f32_acc":
                img[s, m] = _conv_f32(h[s, m], x64[s])[:Lo]
                if sp:
                    e = _conv_f32(h[s, m, :sp], x64[s])[:Lo]
                    early[s, m, :e.size] = e
                continue
            img[s, m] = np.convolve(h[s, m], x64[s])[:Lo]
            if sp:
                e = np.convolve(h[s, m, :sp], x64[s])[:Lo]
                early[s, m, :e.size] = e
    srcs = range(S - 1) if (fault == "lost_source" and S > 1) else range(S)
    total = np.zeros((M, Lo))
    for s in srcs:
        total = total + img[s]
    return img, early, total


def _conv_f32(h, x):
    """the direct form with a float32 accumulator, k ascending: one rounding per added term"""
    n = x.size + h.size - 1
    acc = np.zeros(n, np.float32)
    xp = np.concatenate([x, np.zeros(h.size - 1)])
    for k in range(h.size):
        acc[k:] = (acc[k:].astype(np.float64) + h[k] * xp[:n - k]).astype(np.float32)
    out = np.zeros(n)
    out[:] = acc
    return out


def rel_l2(a, b):
    den = np.linalg.norm(np.ravel(b))
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / den) if den > 0 else float(np.linalg.norm(np.ravel(a)))


def figures(got, want, perm):
    """{name: (value, bar)} of a RIR against the restatement: rel-L2 and the worst tap error relative to the peak, each held
    under max(100 x the restatement's own permuted-order difference, 1e-12)"""
    peak = np.abs(want).max()
    peak = peak if peak > 0 else 1.0
    tap = lambda a: float(np.abs(a - want).max() / peak)
    return {"rel_l2": (rel_l2(got, want), max(100.0 * rel_l2(perm, want), 1e-12)),
            "tap": (tap(got), max(100.0 * tap(perm), 1e-12))}


def missed(fig):
    return {k: v for k, v in fig.items() if not v[0] <= v[1]}


MIX_BAR = 1.2e-7             # 2 x 2^-24: one float32 rounding of a float64 sum, plus a rare flipped rounding


def schroeder_t30(h, fs):
    """Schroeder backward integration; the line fitted to the decay between -5 and -35 dB, extrapolated to 60 dB.  NaN where
    the response does not fall 35 dB."""
    e = np.cumsum((np.asarray(h, np.float64) ** 2)[::-1])[::-1]
    if not e[0] > 0:
        return float("nan")
    db = 10.0 * np.log10(np.maximum(e / e[0], 1e-300))
    i0 = int(np.argmax(db <= -5.0))
    i1 = int(np.argmax(db <= -35.0))
    if not (db <= -35.0).any() or i1 <= i0 + 1:
        return float("nan")
    slope = np.polyfit(np.arange(i0, i1) / fs, db[i0:i1], 1)[0]
    return float(-60.0 / slope)


# ---- case generators --------------------------------------------------------------------------------------------------------
FS = 8000
BETAS = {"distinct": (0.62, 0.71, 0.55, 0.8, 0.45, 0.67), "zero": (0.0,) * 6, "one_zero": (0.62, 0.71, 0.0, 0.8, 0.45, 0.67)}


def geometry(B, S, M, seed=0, wall=False):
    """B rooms of about 3 x 2.5 x 2 m with S sources and M microphones at least 0.2 m off every wall; ``wall``: source 0 of item
    0 stands 2 cm from the wall x = 0"""
    rng = np.random.default_rng(seed)
    room = np.array([3.0, 2.5, 2.0]) + rng.uniform(-0.2, 0.2, (B, 3))
    src = 0.2 + rng.uniform(0, 1, (B, S, 3)) * (room[:, None, :] - 0.4)
    mic = 0.2 + rng.uniform(0, 1, (B, M, 3)) * (room[:, None, :] - 0.4)
    if wall:
        src[0, 0, 0] = 0.02
    return room, src, mic


def rir_cases(tile):
    """(Lh, (B, S, M), beta name, max_order, wall): every Lh at the smallest geometry, every geometry, beta and max_order at one
    Lh past the tile, and the source at the wall"""
    cases = [(Lh, (1, 1, 1), "distinct", None, False) for Lh in (1, tile - 1, tile, tile + 1, 600)]
    cases += [(tile + 1, g, "distinct", None, False) for g in ((2, 2, 3), (1, 4, 8))]
    cases += [(tile + 1, (1, 1, 1), b, None, False) for b in ("zero", "one_zero")]
    cases += [(tile + 1, (1, 1, 1), "distinct", mo, False) for mo in (0, 1, 3)]
    cases += [(tile + 1, (1, 2, 2), "distinct", None, True)]
    return cases


def rir_case_inputs(case):
    Lh, (B, S, M), bname, mo, wall = case
    room, src, mic = geometry(B, S, M, seed=Lh + 7 * B + S + M, wall=wall)
    beta = np.tile(np.array(BETAS[bname]), (B, 1))
    if B > 1:
        beta = beta * np.linspace(1.0, 0.9, B)[:, None]
    return room, beta, src, mic


MIX_L, MIX_LH, MIX_SPLITS = (1, 255, 257, 1000), (1, 80, 300), (0, 40, None)        # split None: Lh + 5, past the last tap


def mix_case_inputs(L, Lh, S=2, M=3):
    """x float32 [S, L] and a decaying h float64 [S, M, Lh]"""
    rng = np.random.default_rng(L * 1000 + Lh)
    x = rng.standard_normal((S, L)).astype(np.float32)
    h = rng.standard_normal((S, M, Lh)) * np.exp(-np.arange(Lh) / 60.0)
    return x, h


def mix_split(split, Lh, S=2):
    """the per-source splits of a case: source 0 at ``split``, the others 3 samples earlier"""
    sp = Lh + 5 if split is None else split
    return np.array([sp] + [max(sp - 3, 0)] * (S - 1), np.int32)
