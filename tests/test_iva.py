"""CPU checks of the blind separation: the NumPy restatement (tests/iva_ref.py) separates -- a synthetic mixture and the real
six-microphone recording of tests/golden --, its cost never increases, zero iterations are the PCA projection, a phase on the
rows of Z changes nothing; its inputs are as benign as the device bars assume; the bars reject every planted fault; and the
host side of the C ABI (version 580, prototypes, defaults, validation) and of the Python options behaves.  No kernel is
launched here."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import iva_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = lambda s: "x".join(map(str, s))


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


SHAPES = R.shapes(lambda K: int(_lib().lib().misonet_auxiva_resident_frames(K)))


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return R.case_inputs(shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, model="gauss", iterations=20):
    B, S, K, M, T, F = shape
    return R.auxiva(_inputs(shape), S, K, iterations, model, ref_ch=R.case_ref_ch(shape))


@functools.lru_cache(maxsize=None)
def _perm(shape, model="gauss", iterations=20):
    B, S, K, M, T, F = shape
    order = np.random.default_rng(5).permutation(T)
    return R.auxiva(_inputs(shape), S, K, iterations, model, ref_ch=R.case_ref_ch(shape), frame_order=order)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_separates_a_synthetic_mixture():
    """two sparse-envelope sources (each on a tenth of the time) on four microphones, noise 60 dB under them: image SDR
    >= 30 dB after 20 gauss iterations (51.6 dB here; 47 .. 53 dB on the seeds 0 .. 3)"""
    mix, truth = R.sparse_mixture(1, 2, 4, 300, 17, seed=0, noise=1e-3, activity=0.1, silence=1e-3)
    r = R.auxiva_item(mix[0], 2, 2, 20)
    sdr = R.image_sdr(r["images"], truth[0])
    print(f"[iva] synthetic 2 sources, M = 4, F = 17, T = 300: image SDR {sdr:.1f} dB")
    assert not r["fail"].any() and sdr >= 30.0, sdr


def test_separates_real_speech():
    """the real six-microphone two-speaker mixture, the defaults (K = 2, gauss, 20 iterations), the image at microphone 0:
    SI-SDR improvement >= 15 dB (21.1 dB here; the margin is for another SciPy's STFT rounding, nothing else)"""
    wav, clean, fs = R.g8_sample()
    X = R.stft(wav)
    assert X.shape == (129, 6, 501)
    r = R.auxiva_item(X, 2)
    est = np.stack([R.istft(r["images"][s, :, 0, :], wav.shape[0]) for s in range(2)])
    best, gain = R.si_sdr_improvement(est, clean.astype(np.float64), wav[:, 0].astype(np.float64))
    print(f"[iva] g8 sample, restatement: SI-SDR {best:.2f} dB, improvement {gain:.2f} dB")
    assert not r["fail"].any() and gain >= 15.0, gain


@pytest.mark.parametrize("model", R.MODELS)
def test_cost_never_increases(model):
    """the cost the auxiliary function majorises, W by least squares from Y = W Z, after every iteration"""
    for seed, (N, M, T, F) in enumerate([(2, 4, 300, 17), (3, 5, 200, 9)]):
        X = R.sparse_mixture(1, N, M, T, F, seed=seed)[0][0].astype(np.complex128)
        _, Z, _ = R.pca(X, N)
        Y = Z.copy()
        costs = [R.cost(X, Y, Z, model)]
        for _ in range(12):
            assert not R.steer(Y, R.weights(Y, model)).any()
            costs.append(R.cost(X, Y, Z, model))
        costs = np.array(costs)
        assert np.all(np.diff(costs) <= 1e-9 * np.abs(costs[:-1])), costs
        assert costs[-1] < costs[0] - 1.0


def test_zero_iterations_is_the_pca_projection():
    mix = R.sparse_mixture(1, 3, 5, 80, 6, seed=7)[0]
    X = mix[0].astype(np.complex128)
    r = R.auxiva_item(X, 3, 3, 0)
    E, Z, lam = R.pca(X, 3, 0)
    assert np.array_equal(r["Y"], Z) and np.all(np.diff(lam, axis=1) <= 0)
    assert np.allclose(E.conj().transpose(0, 2, 1) @ E, np.eye(3)[None], atol=1e-12)
    assert np.all(np.abs(E[:, 0, :].imag) < 1e-15) and np.all(E[:, 0, :].real >= 0)
    # the rows of Z are orthogonal, so the least-squares images of all K rows add up to the projection E E^H X
    assert R.rel(r["images"].sum(axis=0), E @ Z) < 1e-12
    assert list(r["order"]) == list(np.argsort(-r["power"], kind="stable"))


def test_images_do_not_depend_on_the_phase_of_z():
    mix = R.sparse_mixture(1, 2, 4, 120, 8, seed=9)[0]
    X = mix[0].astype(np.complex128)
    _, Z, _ = R.pca(X, 2)
    ph = np.exp(1j * np.random.default_rng(1).uniform(0, 2 * np.pi, (8, 2, 1)))
    a, b = R.auxiva_item(X, 2, 2, 20, Z=Z), R.auxiva_item(X, 2, 2, 20, Z=Z * ph)
    assert R.rel(b["images"], a["images"]) < 1e-10 and R.rel(b["Y"], a["Y"] * ph) < 1e-10
    assert np.array_equal(R.auxiva_item(X, 2, 2, 20)["images"], a["images"])


# ---- the conditions the device bars rest on -----------------------------------------------------------------------------
@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_float64_path_is_benign(shape, model):
    """on every case of the device tests: a permuted summation order moves Y, A and power by less than 1e-10; the K leading
    eigenvalues stand a factor 4 above the rest; the powers around the selection are 1 % apart.

    The case 1x2x2x3x1x4 (T = 1) has rank one: its second eigenvalue counts as 0 (iva_ref.RANK_TOL), so the eigenvalue
    condition holds as 0 >= 4 x 0, the second row is 0 and its power is 0."""
    B, S, K, M, T, F = shape
    want, perm = _ref(shape, model), _perm(shape, model)
    assert not want["fail"].any()
    for name in ("Y", "A", "power"):
        assert R.rel(perm[name], want[name]) < 1e-10, (name, R.rel(perm[name], want[name]))
    if K < M:
        lam = want["lam"]
        assert np.all(lam[..., K - 1] >= 4.0 * lam[..., K]), float(np.min(lam[..., K - 1] / lam[..., K]))
    p = -np.sort(-want["power"], axis=1)
    for j in range(max(0, S - 1), min(S + 1, K)):                  # the pairs (S - 1, S) and (S, S + 1) of the descending list
        if j >= 1:
            assert np.all(p[:, j - 1] - p[:, j] >= 0.01 * p[:, j - 1]), (j, p)
    for j in range(1, S):                                          # and the chosen ones among themselves (their order)
        assert np.all(p[:, j - 1] - p[:, j] >= 0.01 * p[:, j - 1]), (j, p)


def _applies(fault, shape):
    B, S, K, M, T, F = shape
    cross = K >= 2 and T >= 2                  # faults in the terms between two rows: a bin of one frame has one live row
    return {"phi_row": cross, "ys_after": cross, "lost_wave": cross, "frame_past_T": T >= 2, "vs_no_T": T > 1, "order_asc": S >= 2,
            "proj_mic0": R.case_ref_ch(shape) != 0}.get(fault, True)


@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bars_reject_planted_faults(shape, model):
    """a second evaluation with one thing wrong misses a bar of tests/test_gpu_iva.py (20 iterations), a right one does not"""
    B, S, K, M, T, F = shape
    want, perm = _ref(shape, model), _perm(shape, model)
    assert not R.missed(R.figures(perm, want, perm))
    for fault in R.FAULTS:
        if not _applies(fault, shape):
            continue
        got = R.auxiva(_inputs(shape), S, K, 20, model, ref_ch=R.case_ref_ch(shape), fault=fault)
        fig = R.figures(got, want, perm)
        assert R.missed(fig) or not np.array_equal(got["order"], want["order"]), (fault, fig)


def test_non_finite_bins_and_generators():
    B, S, K, M, T, F = shape = SHAPES[0]
    mix = _inputs(shape).copy()
    assert mix.dtype == np.complex64 and mix.shape == (B, F, M, T)
    zeroed = mix.copy()
    zeroed[1, 4] = 0
    mix[1, 4, 2, 17] = complex(np.nan, 0.0)
    a, b = R.auxiva(mix, S, K), R.auxiva(zeroed, S, K)
    flags = np.zeros((B, F), np.int32)
    flags[1, 4] = 1
    assert np.array_equal(a["fail"], flags) and not b["fail"].any()
    assert not a["images"][1, :, 4].any() and np.isfinite(a["images"]).all()
    assert np.array_equal(a["images"], b["images"]) and np.array_equal(a["power"], b["power"])
    mix2, img = R.sparse_mixture(2, 3, 5, 50, 4, seed=1)
    assert img.shape == (2, 3, 4, 5, 50) and R.rel(img.sum(axis=1), mix2) < 0.05


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_iva_opts_default", "misonet_auxiva_workspace_bytes", "misonet_auxiva_resident_frames", "misonet_auxiva",
       "misonet_auxiva_debug"}


def test_abi_580_symbols():
    L = _lib()
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES) and declared == set(L.SIGNATURES)
    assert "misonet_iva_opts;" in hdr and "AuxIVA (ABI 580)" in hdr
    assert "nothing here was compared against those packages" in hdr
    for name in NEW:
        assert hasattr(lib, name), name


def test_abi_580_version_and_defaults():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 580
    o = L.IvaOpts(1, 1, 1, 1, 1.0)
    assert lib.misonet_iva_opts_default(C.byref(o)) == L.OK
    assert (o.iterations, o.model, o.channels, o.ref_ch, o.floor) == (20, 0, 0, 0, 1e-10)
    assert lib.misonet_iva_opts_default(None) == L.EINVAL
    frames = [lib.misonet_auxiva_resident_frames(K) for K in range(1, 9)]
    assert all(f >= 512 and f % 512 == 0 for f in frames) and frames == sorted(frames, reverse=True)
    assert frames[7] >= 1001                                       # the bench geometry stays resident at the largest K


def _opts(**kw):
    L = _lib()
    o = L.IvaOpts()
    L.lib().misonet_iva_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD_OPTS = [dict(iterations=-1), dict(iterations=1001), dict(model=2), dict(model=-1), dict(channels=1), dict(channels=7),
            dict(channels=-1), dict(ref_ch=-1), dict(ref_ch=6), dict(floor=0.0), dict(floor=-1e-10), dict(floor=math.nan),
            dict(floor=math.inf)]


def test_invalid_arguments_report_einval_without_a_device():
    """the checks come before any launch and before any pointer is looked at"""
    L = _lib()
    lib = L.lib()
    p, q = C.c_void_p(256), C.c_void_p(512)
    B, S, K, F, M, T = 2, 2, 3, 129, 6, 50
    n = lib.misonet_auxiva_workspace_bytes(B, S, K, F, M, T)
    need = B * F * (4 + 2 * M * K * 16 + K * 8 + K * T * 16) + B * K * 8 + B * K * T * 8
    assert need <= n <= need + 16 * 256
    assert lib.misonet_auxiva_workspace_bytes(B, S, K, F, M, 2 * T) > n      # it holds Y: it grows with T
    run = lambda o, B=B, S=S, F=F, M=M, T=T, x=p, out=q, ws=p, nws=1 << 40: lib.misonet_auxiva(
        x, B, S, F, M, T, C.byref(o) if o is not None else None, out, None, ws, nws, None)
    for kw in BAD_OPTS:
        assert run(_opts(**kw)) == L.EINVAL, kw
        assert lib.misonet_last_error(), kw
    for bad in (dict(M=1), dict(M=9), dict(S=0), dict(S=5), dict(B=0), dict(F=0), dict(T=0)):
        assert run(_opts(), **bad) == L.EINVAL, bad
        g = {**dict(B=B, S=S, F=F, M=M, T=T), **bad}
        assert lib.misonet_auxiva_workspace_bytes(g["B"], g["S"], g["S"], g["F"], g["M"], g["T"]) == -1, bad
        if "S" not in bad:                                                   # the diagnostic takes K, not S
            assert lib.misonet_auxiva_debug(p, g["B"], K, g["F"], g["M"], g["T"], p, None, None, None, None, None) == L.EINVAL, bad
    assert run(_opts(), S=3, M=2) == L.EINVAL                                # more sources than microphones
    for k in (1, 7):
        assert lib.misonet_auxiva_workspace_bytes(B, S, k, F, M, T) == -1
    assert run(None) == L.EINVAL
    assert run(_opts(), x=None) == L.EINVAL and run(_opts(), out=None) == L.EINVAL and run(_opts(), ws=None) == L.EINVAL
    assert lib.misonet_auxiva_debug(None, B, K, F, M, T, p, None, None, None, None, None) == L.EINVAL
    small = lib.misonet_auxiva_workspace_bytes(B, S, S, F, M, T)
    assert run(_opts(), nws=small - 1) == L.ENOMEM                           # a short workspace, still before any launch
    assert run(_opts(channels=K), nws=small) == L.ENOMEM and small < n


# ---- the Python side ------------------------------------------------------------------------------------------------------
def test_python_options():
    import misonet_amd as mz
    import misonet_amd.blind as BL
    assert mz.AuxIVA is BL.AuxIVA and mz.auxiva is BL.auxiva and mz.BlindSeparator is BL.BlindSeparator
    iv = BL.AuxIVA()
    assert (iv.iterations, iv.model, iv.channels, iv.floor, iv.ref_ch) == (20, "gauss", None, 1e-10, 0)
    assert BL.AuxIVA.of(None) == iv == BL.AuxIVA.of(True) and BL.AuxIVA.of("laplace") == BL.AuxIVA(model="laplace")
    assert BL.AuxIVA.of(dict(iterations=3)) == BL.AuxIVA(iterations=3) and iv.validate(6, 2) is iv and iv.validate() is iv
    o = BL.AuxIVA(iterations=4, model="laplace", channels=3, floor=1e-6, ref_ch=2).c_opts()
    assert (o.iterations, o.model, o.channels, o.ref_ch, o.floor) == (4, 1, 3, 2, 1e-6)
    assert iv.c_opts().channels == 0 and iv.num_channels(2) == 2 and BL.AuxIVA(channels=4).num_channels(2) == 4
    for bad in (dict(iterations=-1), dict(iterations=1001), dict(iterations=2.5), dict(iterations=True), dict(model="cauchy"),
                dict(floor=0.0), dict(floor=math.nan), dict(floor=math.inf), dict(channels=0), dict(channels=2.0),
                dict(ref_ch=-1)):
        with pytest.raises(ValueError):
            BL.AuxIVA(**bad).validate()
    for m, s in ((1, 1), (9, 2), (6, 0), (6, 5), (3, 4)):
        with pytest.raises(ValueError):
            iv.validate(m, s)
    for kw, (m, s) in ((dict(channels=1), (6, 2)), (dict(channels=7), (6, 2)), (dict(ref_ch=6), (6, 2))):
        with pytest.raises(ValueError):
            BL.AuxIVA(**kw).validate(m, s)
    with pytest.raises(ValueError):
        BL.AuxIVA.of(dict(iteration=3))
    with pytest.raises(TypeError):
        BL.AuxIVA.of(3)
    # the call refuses on the host: no device, no library call
    y = np.zeros((1, 5, 4, 20), np.complex64)
    for bad in (dict(iterations=-1), dict(model="x"), dict(floor=0.0), dict(channels=5), dict(ref_ch=4)):
        with pytest.raises(ValueError):
            BL.auxiva(y, 2, **bad)
    for s in (0, 5, 2.0):
        with pytest.raises(ValueError):
            BL.auxiva(y, s)
    with pytest.raises(ValueError):
        BL.auxiva(y[0], 2)
