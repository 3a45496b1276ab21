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


# ---- stage comparator ------------------------------------------------------------------------------------------------------------
# What the debug calls export (steer1, w, lam, out) is enough to judge every stage on its OWN input: the error of the stage in
# front of it is not in the measurement.
#   eig     steer0_dev (steer1_dev with every bin rotated so that component 0 is real and positive: steer0[0] = sqrt(M / ||d||) > 0
#           by construction) against float64 steer0 of the inputs
#   phase   phase_correction(steer0_dev) in float64 against steer1_dev
#   solve   float64 w from float64 Phi_n' of the inputs and the DEVICE's steer1, against w_dev (souden / gev have no intermediate:
#           w_dev and lam_dev against float64 from the inputs)
#   apply   float64 conj(w_dev) . Y against out_dev
# The yardstick e32 of a stage is the same computation with the covariances accumulated in complex64 (apply: the product in
# complex64 with w_dev rounded to float32), and a stage passes with err <= K e32 for the whole tensor of an item (never above CAP, the
# bar of the whole-tensor tests) and max_f err[f] <= K max_f e32[f] for the worst bin (apply: the worst frame too).  The phase
# stage has float64 on both sides and F steps of a few operations: its bound is derived, PHASE_C F 2^-53 relative per bin, and is
# carried as e32 = bound / K so that every stage reads "ratio <= K".
K = 4.0
CAP = 1e-4
PHASE_C = 64.0
EIG_FLOOR = 64.0 * 2.0 ** -53


def steer0_from_cov(phis):
    """Phi_s [..., M, M] -> the normalised principal eigenvector [..., M] (:1107-1123), float64"""
    phis = np.asarray(phis).astype(np.complex128)
    M = phis.shape[-1]
    vals, vecs = np.linalg.eigh(phis)
    idx = np.argmax(vals, axis=-1)
    d = np.take_along_axis(vecs, idx[..., None, None], axis=-1)[..., 0]
    d = d / d[..., :1]
    return d * np.sqrt(M / np.linalg.norm(d, axis=-1, keepdims=True))


def steer0_of_steer1(steer1):
    """undo the phase correction: a unit rotation per bin, and steer0[0] is real and > 0"""
    z = steer1[..., :1]
    return steer1 * (np.conj(z) / np.abs(z))


def prime(phin, condition=0.0, trace_normalize=False, epsi=1e-6):
    """Phi_n -> Phi_n' (the steps of noise_covariance behind the accumulation)"""
    phin = np.asarray(phin).astype(np.complex128)
    M = phin.shape[-1]
    eye = np.eye(M)
    if condition:
        tr = np.trace(phin, axis1=-2, axis2=-1).real[..., None, None]
        phin = (phin + condition * tr / M * eye) / (1 + condition)
    if trace_normalize:
        phin = phin / np.trace(phin, axis1=-2, axis2=-1).real[..., None, None]
    return phin + epsi * eye


def mvdr_weights(phin_prime, steer1, ban_=False):
    num = np.linalg.solve(phin_prime, steer1[..., None])[..., 0]
    w = num / np.einsum("...d,...d->...", steer1.conj(), num)[..., None]
    return ban(w, phin_prime) if ban_ else w


def weights_from_cov(phis, phin_prime, kind, ref_ch=0, ban_=False):
    """souden / gev of beamform_parts from given covariances [B, F, M, M] -> (w, lam)"""
    B, F, M, _ = phis.shape
    lam = None
    if kind == "souden":
        G = np.linalg.solve(phin_prime, phis)
        tr = np.trace(G, axis1=-2, axis2=-1)
        w = np.where((tr == 0)[..., None], 0.0, G[..., ref_ch] / np.where(tr == 0, 1.0, tr)[..., None])
    else:
        w = np.empty((B, F, M), np.complex128)
        lam = np.empty((B, F))
        for b in range(B):
            for f in range(F):
                vals, vecs = scipy.linalg.eigh(phis[b, f], phin_prime[b, f])
                v = vecs[:, -1]
                z = (phin_prime[b, f] @ v)[ref_ch]
                if z != 0:
                    v = v * np.exp(-1j * np.angle(z))
                w[b, f], lam[b, f] = v, vals[-1]
    return (ban(w, phin_prime) if ban_ else w), lam


def _norm_but(x, axis):
    """2-norm over every axis but ``axis``"""
    x = np.moveaxis(np.asarray(x), axis, 0)
    return np.sqrt((np.abs(x.reshape(x.shape[0], -1)) ** 2).sum(-1))


def compare(x, truth, y32, frame_axis=None, e32=None):
    """One item of one stage, bins on axis 0: x the device's result, truth float64, y32 the yardstick evaluation (or ``e32``: a
    derived relative bound per bin, already divided by K).  -> dict(whole, whole32, bin, bin32, f[, frame, frame32, t])"""
    x, truth = np.asarray(x), np.asarray(truth)
    if x.ndim == 1:
        x, truth = x[:, None], truth[:, None]
        y32 = None if y32 is None else np.asarray(y32)[:, None]
    tn = max(np.linalg.norm(truth), 1e-300)
    tb = np.maximum(_norm_but(truth, 0), 1e-300)
    eb = _norm_but(x - truth, 0) / tb
    c = dict(whole=float(np.linalg.norm(x - truth) / tn), bin=float(np.max(eb)) if np.isfinite(eb).all() else float("nan"),
             f=int(np.argmax(np.where(np.isfinite(eb), eb, np.inf))))
    if e32 is not None:
        c.update(whole32=float(e32), bin32=float(e32))
    else:
        c.update(whole32=float(np.linalg.norm(y32 - truth) / tn), bin32=float(np.max(_norm_but(y32 - truth, 0) / tb)))
    if frame_axis is not None:
        tf = np.maximum(_norm_but(truth, frame_axis), 1e-300)
        ef = _norm_but(x - truth, frame_axis) / tf
        c.update(frame=float(np.max(ef)) if np.isfinite(ef).all() else float("nan"),
                 t=int(np.argmax(np.where(np.isfinite(ef), ef, np.inf))),
                 frame32=float(np.max(_norm_but(y32 - truth, frame_axis) / tf)))
    return c


METRICS = ("whole", "bin", "frame")


def ratios(c):
    """err / e32 per metric the comparison has; inf where the yardstick is 0 and the error is not"""
    out = []
    for m in METRICS:
        if m in c:
            e, y = c[m], c[m + "32"]
            out.append(e / y if y > 0 else (0.0 if e == 0 else float("inf")))
    return tuple(out)


def failures(c):
    """the metrics over their bound; a NaN is over every bound"""
    bad = [m for m in METRICS if m in c and not c[m] <= K * c[m + "32"]]
    if not c["whole"] <= CAP and "whole" not in bad:
        bad.append("whole")
    return bad


def check(c, label):
    bad = failures(c)
    where = f"worst bin f = {c['f']}" + (f", worst frame t = {c['t']}" if "t" in c else "")
    msg = ", ".join(f"{m} {c[m]:.3e} > K x {c[m + '32']:.3e}" + (f" (or the cap {CAP:g})" if m == "whole" else "") for m in bad)
    assert not bad, f"{label}: {msg} (K = {K:g}); {where}"


def stage_compare(src, mix, dev, kind="mvdr", noise="residual", condition=0.0, trace_normalize=False, epsi=1e-6, ban_=False,
                  ref_ch=0):
    """src, mix complex64 [B, F, M, T]; dev: dict of the device's steer1 / w [B, F, M] (complex128), lam [B, F], out [B, T, F].
    -> {stage: [comparison of item 0, item 1, ...]} with the stages the kind has ("eig", "phase", "solve", "apply"; "lam" for gev)"""
    B, F, M, T = src.shape
    kw = dict(noise=noise, condition=condition, trace_normalize=trace_normalize, epsi=epsi)
    res = {}
    w_dev = np.asarray(dev["w"]).astype(np.complex128)
    if kind == "mvdr":
        s1 = np.asarray(dev["steer1"]).astype(np.complex128)
        s0 = steer0_of_steer1(s1)
        t0, y0 = steer0_from_cov(covariance(src.astype(np.complex128))), steer0_from_cov(covariance(src.astype(np.complex64)))
        res["eig"] = [compare(s0[b], t0[b], y0[b]) for b in range(B)]
        res["phase"] = [compare(phase_correction(s0[b:b + 1])[0], s1[b], None, e32=PHASE_C * F * 2.0 ** -53 / K) for b in range(B)]
        tw = mvdr_weights(noise_covariance(src.astype(np.complex128), mix.astype(np.complex128), **kw), s1, ban_)
        yw = mvdr_weights(noise_covariance(src.astype(np.complex64), mix.astype(np.complex64), **kw).astype(np.complex128), s1, ban_)
        res["solve"] = [compare(w_dev[b], tw[b], yw[b]) for b in range(B)]
    else:
        t = beamform_parts(src, mix, kind=kind, ban_=ban_, ref_ch=ref_ch, **kw)
        y = beamform_parts(src, mix, kind=kind, ban_=ban_, ref_ch=ref_ch, dtype=np.complex64, **kw)
        res["solve"] = [compare(w_dev[b], t["w"][b], y["w"][b]) for b in range(B)]
        if kind == "gev":
            lam = np.asarray(dev["lam"]).astype(np.float64)
            res["lam"] = [compare(lam[b], t["lam"][b], y["lam"][b]) for b in range(B)]
    out = np.transpose(np.asarray(dev["out"]), (0, 2, 1)).astype(np.complex128)                         # [B, F, T]
    to = np.einsum("bfm,bfmt->bft", w_dev.conj(), mix.astype(np.complex128))
    yo = np.einsum("bfm,bfmt->bft", w_dev.astype(np.complex64).conj(), mix.astype(np.complex64)).astype(np.complex128)
    res["apply"] = [compare(out[b], to[b], yo[b], frame_axis=1) for b in range(B)]
    return res


def ratio_line(stage, kind, M, T, c):
    r = ratios(c)
    return f"[bf-ratio] {stage} {kind} {M} {T} " + " ".join(f"{v:.3g}" for v in r)


def check_stages(res, kind, M, T, log=print):
    """print every [bf-ratio] line, then assert every stage of every item"""
    for stage, items in res.items():
        for c in items:
            log(ratio_line(stage, kind, M, T, c))
    for stage, items in res.items():
        for b, c in enumerate(items):
            check(c, f"stage {stage}, kind {kind}, M = {M}, T = {T}, item {b}")


def rayleigh_deficit(v, phis):
    """1 - (v^H Phi_s v / v^H v) / lambda_max per bin, v [..., M], Phi_s [..., M, M] float64: how far v is from the principal
    eigenvector, judged by the property and not by the (possibly ill-conditioned) vector.  Extended precision, with lambda_max
    refined by the Rayleigh quotient of eigh's vector (second order in its error), so that the figure is not its own round-off."""
    L = np.clongdouble
    P = np.asarray(phis).astype(L)

    def rq(u):
        u = np.asarray(u).astype(L)
        return (np.einsum("...a,...ab,...b->...", u.conj(), P, u).real / np.einsum("...a,...a->...", u.conj(), u).real)
    vals, vecs = np.linalg.eigh(np.asarray(phis).astype(np.complex128))
    top = np.take_along_axis(vecs, np.argmax(vals, -1)[..., None, None], axis=-1)[..., 0]
    return np.asarray(1 - rq(v) / rq(top), dtype=np.float64)


# ---- the device's summation order, restated, with faults to inject ---------------------------------------------------------------
FAULTS = {
    "phis_last": "the last frame missing from Phi_s of ONE (item, bin)",
    "phin_last": "the last frame missing from Phi_n of ONE (item, bin)",
    "w16": "w rounded to 16-bit floats in the apply stage",
    "out_hole": "one output frame of one bin not written (left at zero)",
    "phase_prev": "phase correction against the UN-corrected neighbour",
    "item_swap": "item 1's covariances read from item 0",
    "stale_T": "a stale frame at index T counted in both covariances of ONE (item, bin) (frames [T, Tp) of the padded planes)",
    "argmax2": "the second eigenvalue's vector taken in ONE (item, bin)",
    "conj_s": "one off-diagonal pair of Phi_s with the wrong conjugate in ONE (item, bin)",
    "conj_n": "the same for Phi_n",
    "eps0": "eps I not added",
    "eps2": "2 eps I added",
}
FAULT_ITEM = 1


def lane_covariance(x):
    """x complex64 [B, F, M, T] -> X X^H / T as mvdr_scm_body.inc sums it: lane l of 64 adds frames l, l + 64, ... in float32,
    the 64 partials are reduced and divided by T in float64"""
    x = np.asarray(x).astype(np.complex64)
    B, F, M, T = x.shape
    P = -(-T // 64)
    xp = np.zeros((B, F, M, P * 64), np.complex64)
    xp[..., :T] = x
    xr = np.ascontiguousarray(xp.real).reshape(B, F, M, P, 64)
    xi = np.ascontiguousarray(xp.imag).reshape(B, F, M, P, 64)
    re = np.zeros((B, F, M, M, 64), np.float32)
    im = np.zeros((B, F, M, M, 64), np.float32)
    for p in range(P):
        ar, ai = xr[:, :, :, p], xi[:, :, :, p]
        re += ar[:, :, :, None] * ar[:, :, None] + ai[:, :, :, None] * ai[:, :, None]
        im += ai[:, :, :, None] * ar[:, :, None] - ar[:, :, :, None] * ai[:, :, None]
    return (re.astype(np.float64).sum(-1) + 1j * im.astype(np.float64).sum(-1)) * (1.0 / T)


def device_order(src, mix, kind="mvdr", noise="residual", condition=0.0, trace_normalize=False, epsi=1e-6, ban_=False, ref_ch=0,
                 fault=None, stale=None):
    """A healthy SECOND evaluation, in the kernels' order: covariances by lane_covariance, the eigen-solve, the phase correction and
    the solve in float64 (LAPACK, not Jacobi / Gaussian elimination), w rounded to float32 and the sum over the microphones in
    float32.  -> dict(steer1, w, lam, out) like the debug calls.  ``fault``: one of FAULTS, injected at item FAULT_ITEM, bin F // 2
    where the fault is local (``stale``: the frame that "stale_T" counts, complex64 [M]; a unit frame when None)."""
    if fault is not None and fault not in FAULTS:
        raise ValueError(fault)
    src, mix = np.asarray(src).astype(np.complex64), np.asarray(mix).astype(np.complex64)
    B, F, M, T = src.shape
    fb, ff = min(FAULT_ITEM, B - 1), F // 2
    nz = mix if noise == "mix" else mix - src
    phis, phin = lane_covariance(src), lane_covariance(nz)
    if fault in ("phis_last", "phin_last"):
        x = src if fault == "phis_last" else nz
        (phis if fault == "phis_last" else phin)[fb, ff] = lane_covariance(x[fb:fb + 1, ff:ff + 1, :, :T - 1])[0, 0] * ((T - 1) / T)
    if fault == "stale_T":
        g = np.ones(M, np.complex64) if stale is None else np.asarray(stale).astype(np.complex64)
        for x, phi in ((src, phis), (nz, phin)):
            ext = np.concatenate([x[fb, ff], g[:, None]], axis=1)[None, None]
            phi[fb, ff] = lane_covariance(ext)[0, 0] * ((T + 1) / T)
    if fault == "item_swap":
        phis[fb], phin[fb] = phis[0], phin[0]
    for name, phi in (("conj_s", phis), ("conj_n", phin)):
        if fault == name:
            i, j = M - 1, 0
            phi[fb, ff, i, j], phi[fb, ff, j, i] = phi[fb, ff, j, i], phi[fb, ff, i, j]
    pp = prime(phin, condition, trace_normalize, {"eps0": 0.0, "eps2": 2.0 * epsi}.get(fault, epsi))
    res = dict(lam=None)
    if kind == "mvdr":
        s0 = steer0_from_cov(phis)
        if fault == "argmax2":
            vals, vecs = np.linalg.eigh(phis[fb, ff])
            d = vecs[:, -2] / vecs[0, -2]
            s0[fb, ff] = d * np.sqrt(M / np.linalg.norm(d))
        if fault == "phase_prev":
            s1 = s0.copy()
            for f in range(1, F):
                s1[:, f] = s0[:, f] * np.exp(-1j * np.angle(np.sum(s0[:, f] * s0[:, f - 1].conj(), -1)))[:, None]
        else:
            s1 = phase_correction(s0)
        res["steer1"] = s1
        try:
            w = mvdr_weights(pp, s1, ban_)
        except np.linalg.LinAlgError:
            w = np.full((B, F, M), np.nan + 0j)
    else:
        w, res["lam"] = weights_from_cov(phis, pp, kind, ref_ch, ban_)
    res["w"] = w
    wa = w.astype(np.complex64)
    if fault == "w16":
        wa = (wa.real.astype(np.float16) + 1j * wa.imag.astype(np.float16)).astype(np.complex64)
    wr, wi = wa.real[..., None], wa.imag[..., None]                                                     # [B, F, M, 1]
    yr, yi = np.ascontiguousarray(mix.real), np.ascontiguousarray(mix.imag)
    re, im = np.zeros((B, F, T), np.float32), np.zeros((B, F, T), np.float32)
    with np.errstate(invalid="ignore"):
        for m in range(M):
            re += wr[:, :, m] * yr[:, :, m] + wi[:, :, m] * yi[:, :, m]
            im += wr[:, :, m] * yi[:, :, m] - wi[:, :, m] * yr[:, :, m]
    out = (re + 1j * im).astype(np.complex64)
    if fault == "out_hole":
        out[fb, ff, T // 2] = 0
    res["out"] = np.ascontiguousarray(np.transpose(out, (0, 2, 1)))
    return res


def stage_inputs(B, F, M, T, seed):
    """rank1_inputs with item 1 three times as loud (the covariances nine times: an item read for another shows)"""
    src, mix = rank1_inputs(B, F, M, T, seed)
    if B > 1:
        src[1] *= 3
        mix[1] *= 3
    return src, mix


def eps_inputs(B, F, M, T, seed, frames=None, level=0.01):
    """an input on which eps decides: the residual lives in M - 2 frames only (Phi_n has rank M - 2: singular without eps) and is
    small enough that its eigenvalues are within two orders of eps = 1e-6"""
    src, _ = rank1_inputs(B, F, M, T, seed)
    r = np.random.default_rng(seed + 1)
    n = np.zeros(src.shape, np.complex64)
    k = M - 2 if frames is None else frames
    n[..., :k] = level * (r.standard_normal(src.shape[:3] + (k,)) + 1j * r.standard_normal(src.shape[:3] + (k,))) / np.sqrt(2.0)
    return src, (src + n).astype(np.complex64)


# ---- PIT -----------------------------------------------------------------------------------------------------------------------------
def pit_dist(anchor, cand, dtype=np.complex128, device_order_=False, drop_from=None):
    """dist[b, i, j] = sum_{t, f} | |A_i| - |C_j| |, anchor / cand complex [B, S, T, F].  complex128: the answer; complex64: the
    yardstick (float32 magnitudes, np.abs, summed in float64).  ``device_order_``: pit_dist_k's arithmetic (sqrtf(re^2 + im^2) and
    the difference in float32, the sum in float64); ``drop_from``: a fault, frames >= drop_from missing."""
    a, c = np.asarray(anchor).astype(dtype), np.asarray(cand).astype(dtype)
    if drop_from is not None:
        a, c = a[:, :, :drop_from], c[:, :, :drop_from]
    if device_order_:
        am = np.sqrt(a.real * a.real + a.imag * a.imag)
        cm = np.sqrt(c.real * c.real + c.imag * c.imag)
        return np.abs(am[:, :, None] - cm[:, None]).astype(np.float64).sum((-1, -2))
    am, cm = np.abs(a).astype(np.float64), np.abs(c).astype(np.float64)
    return np.abs(am[:, :, None] - cm[:, None]).sum((-1, -2))


def pit_compare(dist, anchor, cand):
    """-> (worst relative entry error of ``dist``, the same of the float32-magnitude evaluation, the index of the worst entry).
    An entry's own yardstick error is a sum of T F round-offs that passes through zero, so the ratio entry by entry has no bound
    a healthy evaluation keeps; every entry is held to K times the WORST entry of the yardstick, as the beamformer's bins are."""
    t = pit_dist(anchor, cand)
    e = np.abs(np.asarray(dist) - t) / t
    e32 = np.abs(pit_dist(anchor, cand, np.complex64) - t) / t
    return float(e.max()), float(e32.max()), tuple(int(i) for i in np.unravel_index(np.argmax(e), e.shape))


def pit_inputs(B, S, T, F, seed):
    r = np.random.default_rng(seed)
    a = (r.standard_normal((B, S, T, F)) + 1j * r.standard_normal((B, S, T, F))).astype(np.complex64)
    c = np.empty_like(a)
    for b in range(B):
        c[b] = a[b, r.permutation(S)]
    c += 0.1 * (r.standard_normal(c.shape) + 1j * r.standard_normal(c.shape)).astype(np.complex64)
    return a, c


# ---- inputs for the edges of the eigen-solver ----------------------------------------------------------------------------------------
EDGES = ("white", "loud0", "diagonal", "one_frame")


def edge_inputs(name, B, F, M, seed):
    """white: white sources, the eigen-gap falls to about 1 %; loud0: microphone 0 a thousand times louder than the rest;
    diagonal: one microphone per frame (t mod M), so Phi_s is exactly diagonal -- microphone 0 four times as loud, so that the
    principal vector has the component the normalisation divides by; one_frame: T = 1, Phi_s has rank 1 and M - 1 tied zeros"""
    r = np.random.default_rng(seed)
    T = 1 if name == "one_frame" else 65

    def cn(*shape):
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)) / np.sqrt(2.0)
    if name in ("white", "one_frame"):
        src = cn(B, F, M, T)
    elif name == "loud0":
        src = cn(B, F, M, 1) * cn(B, F, 1, T) + 0.1 * cn(B, F, M, T)
        src[:, :, 0] *= 1000.0
    elif name == "diagonal":
        src = cn(B, F, M, T) * (np.arange(T)[None, :] % M == np.arange(M)[:, None])
        src[:, :, 0] *= 4.0
    else:
        raise ValueError(name)
    noise = 0.5 * cn(B, F, M, T)
    if name == "loud0":
        noise[:, :, 0] *= 1000.0
    src = src.astype(np.complex64)
    return src, (src + noise).astype(np.complex64)


def eig_property(steer1, src):
    """-> (deficit of the device's vector, of the complex64 evaluation's, the bound) per (item, bin): K times the yardstick's
    figure, EIG_FLOOR where that is 0.  "Is 0" is taken at the precision the figure can be known to: Phi_s is a float64 matrix and the
    quadratic form has M^2 <= 64 terms, so a figure under 64 * 2^-53 is round-off of Phi_s (it comes out as +-1e-19, not as 0.0, for
    an exact eigenvector) and the bound is max(K y32, EIG_FLOOR).  A vector off by 1e-7 has a figure of 1e-14 already."""
    phis = covariance(src.astype(np.complex128))
    dev = rayleigh_deficit(steer0_of_steer1(np.asarray(steer1).astype(np.complex128)), phis)
    y32 = rayleigh_deficit(steer0_from_cov(covariance(src.astype(np.complex64))), phis)
    return dev, y32, np.maximum(K * y32, EIG_FLOOR)
