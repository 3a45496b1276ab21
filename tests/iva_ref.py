"""Float64 NumPy restatement of the blind separation of csrc/iva.hip (include/misonet.h, "AuxIVA (ABI 580)"):
auxiliary-function independent vector analysis with iterative source steering behind a per-bin PCA to K channels, projected back
to all microphones by least squares.

mix complex64 [B, F, M, T]; float64 after the loads; every recording on its own:

    0. a bin that holds a non-finite sample: fail |= 1, all zero in every step below, its images are 0
    1. per bin: R = X X^H / T, eigenvalues descending (equal ones: the lower index first), each eigenvector rotated so that its
       ref_ch component is real and >= 0 (left alone when that component is 0); an eigenvalue not above 1e-12 times the largest
       counts as 0 and its eigenvector is 0 (a bin of lower rank -- T < K, dead or identical microphones -- has no such
       direction: in exact arithmetic its row of Z is 0; left to rounding it would be noise in an arbitrary direction of the null
       space, which the iterations scale up to a source); Z = E_K^H X, Y = Z
    2. per iteration, once, from all bins (f ascending):  gauss   phi_k[t] = 1 / max(1 / F sum_f |y_k[f, t]|^2, floor)
                                                          laplace phi_k[t] = 1 / max(2 sqrt(sum_f |y_k[f, t]|^2), floor)
    3. per iteration and bin, s = 0 .. K - 1 in order, y_s as it stands before the step:
         num_k = sum_t phi_k y_k conj(y_s),  den_k = sum_t phi_k |y_s|^2,  v_k = num_k / den_k (k != s; 0 when den_k = 0),
         d = den_s / T, v_s = 1 - 1 / sqrt(d) (0 when d = 0),  y_k <- y_k - v_k y_s;  a non-finite v_k -> 0, fail |= 2
    4. A[f, m, k] = sum_t x_m conj(y_k) / sum_t |y_k|^2 (0 when the denominator is 0),  power_k = sum_{f, t} |A[f, ref_ch, k] y_k|^2,
       order = the S rows of largest power, descending (ties: the lower index),  images[s, f, m, t] = A[f, m, order_s] y_{order_s}

The eigenvectors come from np.linalg.eigh here and from a cyclic Jacobi on the device; the generators below keep the K leading
eigenvalues distinct and apart from the rest (tests/test_iva.py asserts it), so that the two agree vector by vector.  Repeated
and near-repeated eigenvalues, ranks 1 .. M - 1, dead and identical microphones and graded spectra are the business of
tests/jacobi_ref.py and tests/test_gpu_eig_edges.py, which judge the PCA by figures that do not depend on the basis chosen
inside a degenerate subspace.  The device tests compare against this file; it also holds their input generators and the planted faults their bars have to reject
(``fault=``).  Nothing here was compared against pyroomacoustics or torchiva.
"""
import os

import numpy as np

OUT_BAR = 2.4e-7            # 4 x 2^-24: one complex64 rounding of a float64 result
MODELS = ("gauss", "laplace")
RANK_TOL = 1e-12            # an eigenvalue of R not above this times the largest is rounding, not data: it counts as 0
THREADS = 512               # the workgroup of the kernels: thread tid owns the frames tid + n 512
# every wrong evaluation auxiva() can plant
FAULTS = ("phi_per_bin", "phi_row", "ys_after", "lost_wave", "frame_past_T", "vs_no_T", "order_asc", "proj_mic0", "f32den")


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    n = np.linalg.norm(b.ravel())
    d = np.linalg.norm((a - b).ravel())
    return float(d / n) if n > 0 else float(d)


def _tsum(a, order):
    """the sum over the last axis with the frames taken in ``order``"""
    return a.sum(axis=-1) if order is None else a[..., order].sum(axis=-1)


def pca(X, K, ref_ch=0, frame_order=None):
    """X [F, M, T] complex128 -> (E [F, M, K], Z [F, K, T], lam [F, M] descending)"""
    F, M, T = X.shape
    Xo = X if frame_order is None else X[..., frame_order]
    R = Xo @ Xo.conj().transpose(0, 2, 1) / T
    E = np.zeros((F, M, K), np.complex128)
    lam = np.zeros((F, M))
    for f in range(F):
        w, V = np.linalg.eigh(R[f])
        w, V = w[::-1], V[:, ::-1]                                   # descending
        idx = np.argsort(-w, kind="stable")                          # equal values keep the lower index
        w, V = w[idx], V[:, idx]
        live = w > RANK_TOL * w[0]                                   # the others count as 0: eigenvector 0, row of Z 0
        w = np.where(live, w, 0.0)
        for k in range(K):
            e = V[ref_ch, k]
            if np.abs(e) != 0:
                V[:, k] = V[:, k] * (np.conj(e) / np.abs(e))
        E[f], lam[f] = V[:, :K] * live[None, :K], w
    return E, E.conj().transpose(0, 2, 1) @ X, lam


def weights(Y, model="gauss", floor=1e-10, fault=None):
    """Y [F, K, T] -> phi [K, T] (``phi_per_bin``: [F, K, T], every bin from itself)"""
    p = Y.real ** 2 + Y.imag ** 2
    if fault == "phi_per_bin":
        r = p if model == "gauss" else 2.0 * np.sqrt(p)
        return 1.0 / np.maximum(r, floor)
    s = np.zeros(p.shape[1:])
    for f in range(p.shape[0]):                                      # ascending f
        s = s + p[f]
    r = s / p.shape[0] if model == "gauss" else 2.0 * np.sqrt(s)
    return 1.0 / np.maximum(r, floor)


def steer(Y, phi, frame_order=None, fault=None):
    """one iteration of step 3 on all bins: Y [F, K, T] (changed in place), phi [K, T] or [F, K, T] -> fail bits [F]"""
    F, K, T = Y.shape
    phi = np.broadcast_to(phi, Y.shape)
    fail = np.zeros(F, np.int32)
    lost = np.zeros(T, bool)
    if fault == "lost_wave":                                         # the partial of one wave never reaches num
        wave = (np.arange(T) % THREADS) // 64
        lost = wave == (1 if T > 64 else 0)
    for s in range(K):
        ys = Y[:, s].copy()                                          # [F, T]
        p2 = ys.real ** 2 + ys.imag ** 2
        w = phi[:, [s] * K] if fault == "phi_row" else phi
        num_t = w * Y * ys.conj()[:, None, :]
        den_t = w * p2[:, None, :]
        num = _tsum(np.where(lost, 0.0, num_t), frame_order)
        if fault == "f32den":
            den = _tsum(den_t.astype(np.float32), frame_order).astype(np.float64)
        else:
            den = _tsum(den_t, frame_order)
        if fault == "frame_past_T":                                  # one frame past the row: the first of the next row
            nxt = np.roll(np.arange(K), -1)
            y1, ys1 = Y[:, nxt, 0], Y[:, (s + 1) % K, 0]
            w1 = w[:, nxt, 0]
            num = num + w1 * y1 * ys1.conj()[:, None]
            den = den + w1 * (np.abs(ys1) ** 2)[:, None]
        with np.errstate(all="ignore"):
            v = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)
            d = den[:, s] if fault == "vs_no_T" else den[:, s] / T
            v[:, s] = np.where(d != 0, 1.0 - 1.0 / np.sqrt(np.where(d != 0, d, 1.0)), 0.0)
        bad = ~(np.isfinite(v.real) & np.isfinite(v.imag))
        fail |= np.where(bad.any(axis=1), 2, 0).astype(np.int32)
        v = np.where(bad, 0.0, v)
        if fault == "ys_after":                                      # y_s is updated first and read afterwards
            Y[:, s] = ys - v[:, s, None] * ys
            ys = Y[:, s].copy()
            others = [k for k in range(K) if k != s]
            Y[:, others] -= v[:, others, None] * ys[:, None, :]
        else:
            Y -= v[:, :, None] * ys[:, None, :]
    return fail


def project(X, Y, frame_order=None):
    """A [F, M, K] = sum_t x_m conj(y_k) / sum_t |y_k|^2 (0 where that is 0)"""
    num = _tsum(X[:, :, None, :] * Y.conj()[:, None, :, :], frame_order)
    den = _tsum(Y.real ** 2 + Y.imag ** 2, frame_order)
    with np.errstate(all="ignore"):
        return np.where(den[:, None, :] != 0, num / np.where(den != 0, den, 1.0)[:, None, :], 0.0)


def select(power, S, fault=None):
    """the S rows of largest power, descending, ties to the lower index"""
    idx = np.argsort(-power, kind="stable")[:S]
    return idx[::-1].copy() if fault == "order_asc" else idx


def auxiva_item(X, S, K=None, iterations=20, model="gauss", floor=1e-10, ref_ch=0, frame_order=None, fault=None, Z=None):
    """One recording.  X [F, M, T] complex.  Returns a dict: images complex128 [S, F, M, T], Y [F, K, T], A [F, M, K], evec
    [F, M, K], lam [F, M], power [K], order [S], fail int32 [F].  ``frame_order``: a permutation of range(T) applied to EVERY
    sum over t.  ``Z``: start the iterations from this [F, K, T] instead of the PCA's.  ``fault``: one of FAULTS."""
    X = np.asarray(X).astype(np.complex128)
    F, M, T = X.shape
    K = S if K is None else K
    fail = np.where(np.isfinite(X.real).all(axis=(1, 2)) & np.isfinite(X.imag).all(axis=(1, 2)), 0, 1).astype(np.int32)
    X = np.where(fail[:, None, None] != 0, 0.0, X)
    E, Y, lam = pca(X, K, ref_ch, frame_order)
    if Z is not None:
        Y = np.array(Z, dtype=np.complex128)
    Y = np.ascontiguousarray(Y)
    for _ in range(iterations):
        fail |= steer(Y, weights(Y, model, floor, fault), frame_order, fault)
    A = project(X, Y, frame_order)
    a_ref = A[:, 0 if fault == "proj_mic0" else ref_ch, :]
    power = (np.abs(a_ref[:, :, None] * Y) ** 2).sum(axis=(0, 2))
    order = select(power, S, fault)
    images = A[:, :, order].transpose(2, 0, 1)[..., None] * Y[:, order].transpose(1, 0, 2)[:, :, None, :]
    return dict(images=images, Y=Y, A=A, evec=E, lam=lam, power=power, order=order.astype(np.int32), fail=fail)


def auxiva(mix, S, K=None, iterations=20, model="gauss", floor=1e-10, ref_ch=0, frame_order=None, fault=None):
    """mix [B, F, M, T] -> the dict of auxiva_item with a leading B on every entry"""
    items = [auxiva_item(x, S, K, iterations, model, floor, ref_ch, frame_order, fault) for x in np.asarray(mix)]
    return {k: np.stack([it[k] for it in items]) for k in items[0]}


def cost(X, Y, Z, model="gauss"):
    """the cost the auxiliary function majorises, with W recovered by least squares from Y = W Z (Z = the PCA projection of X):
    sum_k 1 / T sum_t G(r_k[t]) - 2 sum_f log |det W_f|,  r_k[t]^2 = sum_f |y_k[f, t]|^2,  G(r) = F log r^2 (gauss) or r (laplace):
    phi = G'(r) / (2 r) is the weight of step 2 (above its floor)"""
    F, K, T = Y.shape
    r2 = (np.abs(Y) ** 2).sum(axis=0)
    g = F * np.log(r2) if model == "gauss" else np.sqrt(r2)
    W = Y @ Z.conj().transpose(0, 2, 1) @ np.linalg.inv(Z @ Z.conj().transpose(0, 2, 1))
    return float(g.sum() / T - 2.0 * np.log(np.abs(np.linalg.det(W))).sum())


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def sparse_mixture(B, N, M, T, F, seed=0, noise=0.01, activity=0.5, silence=0.02):
    """N sources with sparse envelopes shared by all bins (what IVA separates by: blocks of 8 frames, each on with probability
    ``activity`` at a level in [0.3, 1.3], ``silence`` added everywhere), gains 0.7^n, through random per-bin mixing, plus
    noise at ``noise``.  Returns mix complex64 [B, F, M, T] and the true images complex128 [B, N, F, M, T].  The projection
    back is a least-squares fit per row, so the sample correlation of two sources over the T frames leaks one into the other's
    image: sources that overlap half of the time stop near 10 log10(T) dB, sources that are rarely on together go far beyond."""
    rng = np.random.default_rng(2000 + seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    blocks = max(1, (T + 7) // 8)
    env = np.repeat(rng.random((B, N, blocks)) < activity, 8, axis=-1)[..., :T] * (0.3 + rng.random((B, N, blocks)).repeat(8, -1)[..., :T])
    env = env + silence                                              # never exactly silent
    src = env[:, :, None, :] * cn(B, N, F, T) * (0.7 ** np.arange(N))[None, :, None, None]
    H = cn(B, N, F, M)
    img = H[..., None] * src[:, :, :, None, :]                       # [B, N, F, M, T]
    mix = img.sum(axis=1) + noise * cn(B, F, M, T)
    return mix.astype(np.complex64), img


def _golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))


def g8_sample(fs=8000):
    """the real six-microphone two-speaker mixture of tests/golden: (wav float32 [32000, 6], clean float32 [2, 32000] = the
    speakers' images at microphone 0, fs)"""
    wav = _golden("g8_sample_clean_miso1.npz")["obs_wav_f16"].astype(np.float32)
    clean = _golden("g16_stoi.npz")["clean"][:, :wav.shape[0]].astype(np.float32)
    return wav, clean, fs


def stft(wav):
    """float [L, M] -> complex64 [F, M, T]: the un-normalised hann-256 / hop-64 STFT of the pipeline (oracle/pipeline_oracle.py)"""
    from oracle import pipeline_oracle
    return np.ascontiguousarray(pipeline_oracle.stft_chunk(np.asarray(wav, np.float32), 8000).transpose(2, 0, 1))


def istft(spec_ft, n):
    """complex [F, T] -> float64 [n]"""
    import scipy.signal
    from oracle import pipeline_oracle as P
    _, x = scipy.signal.istft(np.asarray(spec_ft) * P.SCALE, fs=8000, window=P.WINDOW, nperseg=P.NPERSEG, noverlap=P.NOVERLAP)
    return x[:n]


def si_sdr(est, ref):
    est, ref = est - est.mean(), ref - ref.mean()
    t = np.dot(est, ref) / np.dot(ref, ref) * ref
    return float(10.0 * np.log10(np.dot(t, t) / np.dot(est - t, est - t)))


def si_sdr_improvement(est, clean, mix):
    """est [S, L], clean [S, L], mix [L] -> (the mean SI-SDR of the best permutation, its improvement over the mixture)"""
    import itertools
    S = clean.shape[0]
    best = max(np.mean([si_sdr(est[p[s]], clean[s]) for s in range(S)]) for p in itertools.permutations(range(S)))
    base = np.mean([si_sdr(mix, clean[s]) for s in range(S)])
    return float(best), float(best - base)


def image_sdr(images, truth):
    """images [S, F, M, T] against the true images [S, F, M, T], the best permutation: the mean over the sources, dB"""
    import itertools
    S = truth.shape[0]

    def sdr(a, b):
        return 10.0 * np.log10(np.sum(np.abs(b) ** 2) / np.sum(np.abs(a - b) ** 2))
    return float(max(np.mean([sdr(images[p[s]], truth[s]) for s in range(S)]) for p in itertools.permutations(range(S))))


# ---- the device tests' cases -------------------------------------------------------------------------------------------------
def shapes(resident):
    """the shapes (B, S, K, M, T, F) of the device tests; ``resident(K)`` = misonet_auxiva_resident_frames(K).  The streaming
    path has no chunk length of its own (it walks 512 frames at a time, the stride of the resident path)."""
    R2, R8 = resident(2), resident(8)
    return [(2, 2, 2, 4, 60, 9), (1, 1, 1, 2, 40, 5), (1, 2, 2, 3, 1, 4), (1, 2, 3, 6, 63, 3), (1, 2, 2, 6, 64, 3),
            (1, 2, 2, 6, 65, 3), (1, 3, 3, 5, 300, 17), (1, 4, 8, 8, 200, 3), (1, 2, 2, 6, R2, 2), (1, 2, 2, 6, R2 + 1, 2),
            (1, 2, 8, 8, R8 + 1, 2)]


def case_ref_ch(shape):
    """the reference microphone of a device case: 2 where there are three, so that a projection at microphone 0 shows"""
    return 2 if shape[3] >= 3 else 0


def case_inputs(shape):
    """mix complex64 [B, F, M, T] of a device test shape: K sources (so that the K leading eigenvalues stand apart)"""
    B, S, K, M, T, F = shape
    return sparse_mixture(B, K, M, T, F, seed=sum(shape))[0]


def figures(got, want, perm):
    """The figures the device tests assert and their bars, {name: (figure, bar)}: got / want / perm = dicts as auxiva() returns
    them (got: the evaluation under test, want: the restatement, perm: the restatement with every sum over t in a permuted
    order).  images: rel-L2 <= OUT_BAR; Y, A, evec, power: rel-L2 <= 100 x the restatement's permuted-order difference on that
    case, never below 1e-12."""
    out = dict(images=(rel(got["images"], want["images"]), OUT_BAR))
    for name in ("Y", "A", "evec", "power"):
        out[name] = (rel(got[name], want[name]), max(100.0 * rel(perm[name], want[name]), 1e-12))
    return out


def missed(fig):
    return [name for name, (v, bar) in fig.items() if not v <= bar]
