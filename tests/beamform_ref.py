"""Test oracle (never imported by the product): a NumPy / SciPy float64 restatement of the selectable beamformers, in the
reference's own terms where it has them (line numbers into the reference's tester.py):

  covariances          Phi = X X^H / T, then 0.5 (Phi + Phi^H)                       :1091-1100, :1138-1152
  noise                "residual" N = Y - S (:1095) / "mix" N = Y (:1096, the commented-out MPDR line)
  condition            (Phi_n + gamma tr(Phi_n) / M I) / (1 + gamma), PER BIN: equation (2.3) of the paper that :1170 cites
                       (the dead code at :1169-1176 takes np.trace of a whole [F, C, C] slab, which sums over the wrong axes)
  trace_normalize      Phi_n / tr(Phi_n)                                             :1099
  epsi                 Phi_n' = Phi_n + epsi I, last                                 :1086-1088, :1221
  mvdr                 eigh(Phi_s) -> d / d[0] -> sqrt(M / ||d||) -> PhaseCorrection -> solve     :1107-1129, :1211-1225
  souden               G = solve(Phi_n', Phi_s), w = G[:, ref_ch] / tr G; 0 where tr G == 0
  gev                  scipy.linalg.eigh(Phi_s, Phi_n'): the last eigenvector (w^H Phi_n' w = 1), rotated per bin so that
                       (Phi_n' w)[ref_ch] is real and >= 0 (left alone where that entry is 0)
  ban                  w sqrt|w^H Phi_n' Phi_n' w| / |w^H Phi_n' w| (:1196-1208 with eps = 0); w stays where the denominator is 0
  output               out[b, t, f] = sum_m conj(w[b, f, m]) Y[b, f, m, t]           :1227-1228, :1134
"""
import numpy as np
import scipy.linalg

KINDS = ("mvdr", "souden", "gev")


def covariance(x):
    T = x.shape[-1]
    r = np.einsum("...dt,...et->...de", x, x.conj()) / T                  # :1148-1151
    return 0.5 * (r + np.conj(r.swapaxes(-1, -2)))                        # :1092 / :1100


def phase_correction(w):                                                  # :1154-1167
    w = w.copy()
    for b in range(w.shape[0]):
        for f in range(1, w.shape[1]):
            w[b, f] = w[b, f] * np.exp(-1j * np.angle(np.sum(w[b, f] * w[b, f - 1].conj())))
    return w


def ban(w, phin):                                                         # :1196-1208, eps = 0
    nom = np.abs(np.sqrt(np.einsum("...a,...ab,...bc,...c->...", w.conj(), phin, phin, w)))
    den = np.abs(np.einsum("...a,...ab,...b->...", w.conj(), phin, w))
    g = np.where(den == 0, 1.0, nom / np.where(den == 0, 1.0, den))
    return w * g[..., None]


def noise_covariance(source, mix, noise="residual", condition=0.0, trace_normalize=False, epsi=1e-6):
    """Phi_n' [B, F, M, M] complex128"""
    M = source.shape[2]
    n = mix - source if noise == "residual" else mix                       # :1095 / :1096
    phin = covariance(n)
    eye = np.eye(M)[None, None]
    if condition:
        tr = np.trace(phin, axis1=-2, axis2=-1).real[..., None, None]
        phin = (phin + condition * tr / M * eye) / (1 + condition)
    if trace_normalize:
        phin = phin / np.trace(phin, axis1=-2, axis2=-1).real[..., None, None]     # :1099
    return phin + epsi * eye                                              # :1221


def beamform_parts(source, mix, kind="mvdr", noise="residual", condition=0.0, trace_normalize=False, epsi=1e-6, ban_=False,
                   ref_ch=0, dtype=np.complex128):
    """source, mix complex [B, F, M, T] -> dict(phis, phin (= Phi_n'), w [B, F, M], lam [B, F] (gev), out [B, T, F]).
    ``dtype``: the precision the covariances are accumulated in (complex128: the exact answer; complex64: what a float32
    accumulation moves it by)."""
    if kind not in KINDS or noise not in ("residual", "mix"):
        raise ValueError((kind, noise))
    source = np.asarray(source).astype(dtype)
    mix = np.asarray(mix).astype(dtype)
    B, F, M, T = source.shape
    if not 0 <= ref_ch < M or condition < 0:
        raise ValueError((ref_ch, condition))
    phis = covariance(source).astype(np.complex128)
    phin = noise_covariance(source, mix, noise, condition, trace_normalize, epsi).astype(np.complex128)
    lam = None
    if kind == "mvdr":
        vals, vecs = np.linalg.eigh(phis.reshape(-1, M, M))               # :1107-1112
        idx = np.argmax(vals, axis=-1)
        d = np.stack([vecs[i, :, idx[i]] for i in range(len(idx))]).reshape(B, F, M)
        d = d / d[:, :, :1]                                               # :1119
        d = d * np.sqrt(M / np.linalg.norm(d, axis=-1, keepdims=True))    # :1123
        d = phase_correction(d)                                           # :1128
        num = np.linalg.solve(phin, d[..., None])[..., 0]                 # :1222
        w = num / np.einsum("...d,...d->...", d.conj(), num)[..., None]   # :1223-1224
    elif kind == "souden":
        G = np.linalg.solve(phin, phis)
        tr = np.trace(G, axis1=-2, axis2=-1)
        w = np.where((tr == 0)[..., None], 0.0, G[..., ref_ch] / np.where(tr == 0, 1.0, tr)[..., None])
    else:
        w = np.empty((B, F, M), np.complex128)
        lam = np.empty((B, F))
        for b in range(B):
            for f in range(F):
                vals, vecs = scipy.linalg.eigh(phis[b, f], phin[b, f])    # ascending; v^H Phi_n' v = 1
                v = vecs[:, -1]
                z = (phin[b, f] @ v)[ref_ch]
                if z != 0:
                    v = v * np.exp(-1j * np.angle(z))
                w[b, f], lam[b, f] = v, vals[-1]
    if ban_:
        w = ban(w, phin)
    out = np.einsum("...a,...at->...t", w.conj(), mix.astype(np.complex128))        # :1228
    return dict(phis=phis, phin=phin, w=w, lam=lam, out=np.transpose(out, (0, 2, 1)))  # :1134


def rank1_inputs(B, F, M, T, seed=7):
    """the inputs of the device tests: a dominant rank-1 source, src = a[b,f,m] s[b,f,t] + 0.1 cn, mix = src + 0.5 cn
    (cn complex standard normal), complex64"""
    r = np.random.default_rng(seed)

    def cn(*shape):
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)) / np.sqrt(2.0)      # E|cn|^2 = 1
    a, s = cn(B, F, M, 1), cn(B, F, 1, T)
    src = (a * s + 0.1 * cn(B, F, M, T)).astype(np.complex64)
    mix = (src + 0.5 * cn(B, F, M, T)).astype(np.complex64)
    return src, mix
