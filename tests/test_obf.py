"""CPU checks of the online beamformer: the NumPy restatement (tests/obf_ref.py) has the properties the device tests lean on -- it
does not depend on how the stream is cut, its covariances are exactly Hermitian, the Souden filter is distortionless on a rank-one
source, mu scales the filter as den(0) / den(mu), MPDR on the mixture itself returns the reference microphone, every device case's
bar stays under the cap, and every planted mistake misses the device tests' bars -- and the host side of the C ABI (version,
prototypes, defaults, validation) and of the Python options behaves.  No kernel is launched here."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

import obf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = [1, 1, 2, 17]
# the device cases that do not depend on misonet_obf_cells_per_block, (B, S, M, T, F): tests/test_gpu_obf.py runs these and the edges
CASES = [(2, 2, 2, 40, 5), (1, 1, 2, 1, 1), (1, 3, 3, 30, 3), (1, 2, 4, 40, 2), (1, 5, 5, 30, 2), (1, 6, 6, 40, 3), (1, 7, 7, 30, 2),
         (1, 8, 8, 30, 2), (1, 2, 2, 300, 5), (1, 6, 6, 300, 3)]
# (noise, alpha, mu, diag_load, ref_ch)
VARIANTS = [("residual", 0.98, 0.0, 1e-3, 0), ("mix", 0.9, 0.0, 1e-3, 1), ("residual", 0.98, 1.0, 0.0, 0)]
IDS = lambda s: "x".join(map(str, s))


def _kw(v):
    return dict(noise=v[0], alpha=v[1], mu=v[2], diag_load=v[3], ref_ch=v[4])


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_state(a, b):
    return all(np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))) for k in ("phi_s", "phi_n", "w", "n", "fail"))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_is_cut_invariant_and_hermitian():
    images, mix = R.inputs(2, 2, 3, 40, 4)
    o0, s0 = R.obf(images, mix, alpha=0.9, noise="mix")
    o1, s1 = R.obf(images, mix, alpha=0.9, noise="mix", cuts=CUTS)
    assert R.pieces(40, CUTS) == [(0, 1), (1, 2), (2, 4), (4, 21), (21, 40)]
    assert np.array_equal(_bits(o0), _bits(o1)) and _same_state(s0, s1)
    o2, s2 = R.obf(images, mix, cuts=[1] * 40)
    o3, s3 = R.obf(images, mix)
    assert np.array_equal(_bits(o2), _bits(o3)) and _same_state(s2, s3)
    for s in (s0, s3):
        assert R.hermitian(s.phi_s) and R.hermitian(s.phi_n) and (s.n == 40).all() and not s.fail.any()
    assert o0.dtype == np.complex64 and o0.shape == (2, 2, 40, 4) and o0.any()


@pytest.mark.parametrize("M", [2, 6])
@pytest.mark.parametrize("ref_ch", [0, 1])
def test_distortionless_identity(M, ref_ch):
    """mu = 0 and Phi_s of rank one (images = a (x) s_t): w^H a = a[ref_ch], whatever Phi_n is"""
    images, mix, a = R.rank_one(M, 50, 3, seed=M + ref_ch)
    for noise in R.NOISES:
        out, st = R.obf(images, mix, ref_ch=ref_ch, noise=noise)
        got = np.einsum("fm,fm->f", np.conj(st.w[0, 0]), a.astype(np.complex128))
        err = np.abs(got - a[:, ref_ch]) / np.abs(a[:, ref_ch])
        print(f"[obf] distortionless M {M} ref {ref_ch} {noise}: |w^H a - a_ref| / |a_ref| <= {err.max():.3e}")
        assert not st.fail.any() and err.max() <= 1e-9


def test_mu_scales_the_filter():
    """w(mu) = w(0) den(0) / den(mu) with den(mu) = mu + tr G: the covariances do not depend on mu"""
    images, mix = R.inputs(1, 3, 3, 30, 3)
    _, s0 = R.obf(images, mix, mu=0.0)
    _, s1 = R.obf(images, mix, mu=2.5)
    assert np.array_equal(s0.phi_s, s1.phi_s) and np.array_equal(s0.phi_n, s1.phi_n)
    M = 3
    load = 1e-3 * np.trace(s0.phi_n, axis1=-2, axis2=-1).real / M + 1e-10
    G = np.linalg.solve(s0.phi_n + load[..., None, None] * np.eye(M), s0.phi_s)
    den0 = np.trace(G, axis1=-2, axis2=-1)
    assert R.rel(s1.w, s0.w * (den0 / (2.5 + den0))[..., None]) <= 1e-9
    assert R.rel(s0.w, G[..., :, 0] / den0[..., None]) <= 1e-9                      # and the filter is Souden's


def test_mpdr_on_the_mixture_itself_returns_the_reference_microphone():
    """noise "mix", S = 1 and images = mix: v = x, so Phi_n = Phi_s bit for bit once nothing else is in Phi_n (init = 0, no
    loading), G = I and tr G = M: the filter of the definition is e_ref / M and M out = mix[ref_ch], within 1e-9, from the frame
    on at which Phi has full rank.  (The issue states this property as out = mix[ref_ch]; under its own step 5, w = G[:, ref] /
    tr G, the factor 1 / M = 1 / tr I belongs to it.  M = 4 keeps M out exact in complex64.)"""
    M = 4
    _, mix = R.inputs(1, 1, M, 40, 2)
    for ref_ch in (0, 2):
        out, st = R.obf(mix[:, None], mix, noise="mix", ref_ch=ref_ch, init=0.0, diag_load=0.0, epsi=0.0)
        assert np.array_equal(st.phi_s, st.phi_n)
        want = mix[0, ref_ch, 2 * M:]
        err = np.abs(M * out[0, 0, 2 * M:].astype(np.complex128) - want).max() / np.abs(want).max()
        e = np.zeros(M)
        e[ref_ch] = 1.0 / M
        werr = np.abs(st.w[0, 0] - e).max()
        print(f"[obf] MPDR on the mixture, ref {ref_ch}: |M out - mix[ref]| {err:.3e}  |w - e_ref / M| {werr:.3e}")
        assert err <= 1e-9 and werr <= 1e-9


@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_every_device_case_stays_under_the_cap(shape):
    images, mix = R.inputs(*shape)
    for v in VARIANTS:
        ref = R.figures(images, mix, **_kw(v))
        print(f"[obf] case {shape} {v}: own {ref['own']:.3e}  bar {ref['bar']:.3e}")
        assert ref["bar"] <= R.BAR_CAP and not ref["st"].fail.any()
        assert not R.rejected(R.as_candidate(ref["out"], ref["st"]), ref)
        out_rev, rev = R.obf(images, mix, reverse=True, **_kw(v))
        assert not R.rejected(R.as_candidate(out_rev, rev), ref)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_miss_the_device_bars(fault):
    """each mistake a kernel could make, planted in the restatement, is rejected by what tests/test_gpu_obf.py asserts
    (``obf_ref.rejected``) on the device case (1, 6, 6, 40, 3)"""
    images, mix = R.inputs(1, 6, 6, 40, 3)
    kw = _kw(VARIANTS[1] if fault == "no_conjugate" else VARIANTS[0])
    ref = R.figures(images, mix, **kw)
    fo, fs = R.obf(images, mix, fault=fault, **kw)
    print(f"[obf] fault {fault}: out {R.rel(fo, ref['out']):.3e}  Phi_s {R.rel(fs.phi_s, ref['ext'].phi_s):.3e}  "
          f"Phi_n {R.rel(fs.phi_n, ref['ext'].phi_n):.3e}  w {R.rel(fs.w, ref['ext'].w):.3e}  (bars {R.OUT_BAR:g}, {ref['bar']:g})")
    assert R.rejected(R.as_candidate(fo, fs), ref), fault


def test_failing_frames_silence_and_the_count():
    images, mix = (a.copy() for a in R.inputs(1, 2, 3, 30, 3))
    o0, s0 = R.obf(images[:, :, :, :10], mix[:, :, :10])
    mix[0, 1, 10, 1] = np.nan                                                       # every source of bin 1
    images[0, 1, 0, 10, 2] = complex(0.0, np.inf)                                   # source 1 of bin 2
    o1, s1 = R.obf(images[:, :, :, :11], mix[:, :, :11])
    assert s1.fail.tolist() == [[[0, 1, 0], [0, 1, 1]]] and (s1.n == 11).all()
    assert not o1[0, :, 10, 1].any() and not o1[0, 1, 10, 2] and o1[0, 0, 10, 2]
    for k in ("phi_s", "phi_n", "w"):
        assert np.array_equal(getattr(s1, k)[0, :, 1], getattr(s0, k)[0, :, 1]), k
        assert not np.array_equal(getattr(s1, k)[0, :, 0], getattr(s0, k)[0, :, 0]), k
    o2, s2 = R.obf(images, mix)
    assert np.isfinite(o2).all() and np.isfinite(s2.phi_s).all() and np.isfinite(s2.w).all()
    # a source silent so far: out 0, no flag
    images, mix = (a.copy() for a in R.inputs(1, 2, 3, 30, 3))
    images[0, 1, :, :5] = 0
    o3, s3 = R.obf(images, mix)
    assert not o3[0, 1, :5].any() and o3[0, 1, 5:].all() and not s3.fail.any()
    # a pivot that is not > 0: images = mix, so v = 0 exactly, and nothing loads the diagonal
    o4, s4 = R.obf(mix[:, None], mix, init=0.0, diag_load=0.0, epsi=0.0)
    assert (s4.fail == 2).all() and not o4.any() and not s4.w.any() and s4.phi_s.any()
    o5, s5 = R.obf(mix[:, None], mix, init=0.0, diag_load=0.0, epsi=1e-10)
    assert not s5.fail.any() and o5.any()
    st = R.State(1, 1, 2, 1)
    st.n[:] = R.N_MAX
    R.step(st, np.ones((1, 1, 2, 1), np.complex64), np.ones((1, 2, 1), np.complex64))
    assert st.n.tolist() == [[[R.N_MAX]]]


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_obf_opts_default", "misonet_obf_state_bytes", "misonet_obf_cells_per_block", "misonet_obf_reset", "misonet_obf",
       "misonet_obf_debug"}


def test_abi_640():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 640
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    assert "misonet_obf_opts;" in hdr
    for name in NEW:
        assert hasattr(lib, name), name
    o = L.ObfOpts(7, 7, 0.0, 7.0, 7.0, 7.0, 7.0)
    assert lib.misonet_obf_opts_default(C.byref(o)) == L.OK
    assert (o.noise, o.ref_ch, o.alpha, o.mu, o.diag_load, o.epsi, o.init) == (0, 0, 0.98, 0.0, 1e-3, 1e-10, 1.0)
    assert lib.misonet_obf_opts_default(None) == L.EINVAL


def _opts(**kw):
    L = _lib()
    o = L.ObfOpts()
    L.lib().misonet_obf_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD_OPTS = ([dict(noise=2), dict(noise=-1), dict(ref_ch=-1), dict(ref_ch=6), dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.0),
             dict(alpha=1.5), dict(alpha=math.nan), dict(alpha=math.inf)]
            + [{k: v} for k in ("mu", "diag_load", "epsi", "init") for v in (-1.0, math.nan, math.inf)])
# (B, S, M, F)
BAD_GEOM = [(0, 6, 6, 129), (-1, 6, 6, 129), (2, 0, 6, 129), (2, 9, 6, 129), (2, 6, 1, 129), (2, 6, 9, 129), (2, 6, 6, 0),
            (2, 6, 6, 1026), (1 << 20, 8, 6, 1 << 9)]


def test_sizes_and_invalid_arguments():
    L = _lib()
    lib = L.lib()
    assert len(L.SIGNATURES["misonet_obf_state_bytes"][1]) == 4                     # B, S, M, F: no T
    n = lib.misonet_obf_state_bytes(16, 6, 6, 129)
    per_cell = 2 * 6 * 6 * 16 + 6 * 16 + 8
    assert 16 * 6 * 129 * per_cell <= n <= 16 * 6 * 129 * per_cell + 2 * 16 and n % 16 == 0
    assert lib.misonet_obf_state_bytes(1, 1, 2, 1) > 0 and lib.misonet_obf_state_bytes(1, 8, 8, 1025) > 0
    for g in BAD_GEOM:
        assert lib.misonet_obf_state_bytes(*g) == -1, g
        assert lib.misonet_last_error(), g
    P = [lib.misonet_obf_cells_per_block(M) for M in range(2, 9)]
    assert all(p >= 1 for p in P) and P[0] + 1 <= 1025, P
    assert lib.misonet_obf_cells_per_block(1) == -1 and lib.misonet_obf_cells_per_block(9) == -1
    # every limit is refused before any pointer is looked at: the pointers here are null or not addresses at all
    junk = C.c_void_p(8)
    for kw in BAD_OPTS:
        o = _opts(**kw)
        assert lib.misonet_obf(junk, junk, 2, 6, 6, 10, 129, C.byref(o), junk, junk, 1 << 40, None) == L.EINVAL, kw
        assert lib.misonet_last_error(), kw
        assert lib.misonet_obf_reset(junk, 2, 6, 6, 129, C.byref(o), None) == L.EINVAL, kw
    o = _opts(init=0.0, diag_load=0.0, epsi=0.0, mu=0.0)                            # legal: the pivot failure is reachable
    for B, S, M, F in BAD_GEOM:
        assert lib.misonet_obf(junk, junk, B, S, M, 10, F, C.byref(o), junk, junk, 1 << 40, None) == L.EINVAL, (B, S, M, F)
        assert lib.misonet_obf_reset(junk, B, S, M, F, C.byref(o), None) == L.EINVAL, (B, S, M, F)
        assert lib.misonet_obf_debug(junk, B, S, M, F, None, None, None, None, None, None) == L.EINVAL, (B, S, M, F)
    for T in (0, -3):
        assert lib.misonet_obf(junk, junk, 2, 6, 6, T, 129, C.byref(o), junk, junk, 1 << 40, None) == L.EINVAL
    assert lib.misonet_obf(junk, junk, 2, 6, 6, 10, 129, None, junk, junk, 1 << 40, None) == L.EINVAL
    assert lib.misonet_obf(None, None, 2, 6, 6, 10, 129, C.byref(o), None, None, 0, None) == L.EINVAL
    assert lib.misonet_obf_reset(None, 2, 6, 6, 129, C.byref(o), None) == L.EINVAL
    assert lib.misonet_obf_debug(None, 2, 6, 6, 129, None, None, None, None, None, None) == L.EINVAL
    # mix, images, out and the state must not overlap; a short state is ENOMEM (addresses only: nothing is launched)
    a, b, c, s = C.c_void_p(1 << 30), C.c_void_p(2 << 30), C.c_void_p(3 << 30), C.c_void_p(4 << 30)
    need = lib.misonet_obf_state_bytes(1, 2, 2, 5)
    call = lambda mix, img, out, st, nb: lib.misonet_obf(mix, img, 1, 2, 2, 4, 5, C.byref(o), out, st, nb, None)
    assert call(a, a, c, s, need) == L.EINVAL
    assert call(a, b, a, s, need) == L.EINVAL
    assert call(a, b, b, s, need) == L.EINVAL
    assert call(a, b, C.c_void_p((2 << 30) + 2 * 2 * 4 * 5 * 8 - 8), s, need) == L.EINVAL
    assert call(a, b, c, a, need) == L.EINVAL and call(a, b, c, c, need) == L.EINVAL
    assert call(a, b, c, s, need - 1) == L.ENOMEM


# ---- the Python options -------------------------------------------------------------------------------------------------
def test_online_beamformer_options():
    import misonet_amd as mz
    from misonet_amd.beamform import Beamformer, OnlineBeamformer
    assert mz.OnlineBeamformer is OnlineBeamformer and callable(mz.beamform_online) and isinstance(mz.BeamformStream, type)
    d = OnlineBeamformer()
    assert dataclasses.astuple(d) == ("residual", 0, 0.98, 0.0, 1e-3, 1e-10, 1.0)
    assert OnlineBeamformer.of(None) == d and OnlineBeamformer.of(True) == d and OnlineBeamformer.of(d) is d
    assert OnlineBeamformer.of("mix") == OnlineBeamformer(noise="mix")
    assert OnlineBeamformer.of(dict(alpha=0.9, ref_ch=1)) == OnlineBeamformer(alpha=0.9, ref_ch=1)
    with pytest.raises(ValueError):
        OnlineBeamformer.of(dict(kind="souden"))
    with pytest.raises(TypeError):
        OnlineBeamformer.of(3)
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.alpha = 0.5
    assert d.validate(2, 1) is d and d.validate(8, 8) is d and d.validate() is d
    assert OnlineBeamformer(noise=1).c_opts().noise == 1 and OnlineBeamformer(noise="mix").c_opts().noise == 1
    assert OnlineBeamformer(init=0.0, diag_load=0.0, epsi=0.0).validate(2, 1).c_opts().init == 0.0
    for kw in BAD_OPTS:
        kw = dict(kw)
        if "noise" in kw:
            kw["noise"] = "speech" if kw["noise"] == 2 else kw["noise"]
        with pytest.raises(ValueError):
            OnlineBeamformer(**kw).validate(6, 6)
    for m in (1, 9):
        with pytest.raises(ValueError):
            d.validate(m)
    for s in (0, 9):
        with pytest.raises(ValueError):
            d.validate(6, s)
    with pytest.raises(ValueError):
        OnlineBeamformer(ref_ch=1.0).validate(2)
    with pytest.raises(ValueError):
        OnlineBeamformer(noise=True).validate(2)
    o = OnlineBeamformer(noise="mix", ref_ch=2, alpha=0.9, mu=1.5, diag_load=1e-2, epsi=1e-8, init=5.0).c_opts()
    assert (o.noise, o.ref_ch, o.alpha, o.mu, o.diag_load, o.epsi, o.init) == (1, 2, 0.9, 1.5, 1e-2, 1e-8, 5.0)
    assert Beamformer.of(None) == Beamformer()                                  # the block beamformers' options are what they were
    with pytest.raises(TypeError):
        Beamformer.of(d)


def test_online_calls_refuse_before_any_launch():
    """bad shapes and fields raise on the host: no device is needed to see them"""
    from misonet_amd.beamform import BeamformStream, OnlineBeamformer, beamform_online
    from misonet_amd.blind import BlindSeparator
    images, mix = R.inputs(1, 2, 2, 40, 5)
    with pytest.raises(ValueError):
        beamform_online(images, mix, alpha=1.0)
    with pytest.raises(ValueError):
        beamform_online(images, mix, ref_ch=2)
    with pytest.raises(ValueError):
        beamform_online(images, mix, noise="speech")
    with pytest.raises(ValueError):
        beamform_online(images[0], mix)
    with pytest.raises(ValueError):
        beamform_online(images, mix[:, :, :39])
    with pytest.raises(ValueError):
        beamform_online(images[:, :, :, :0], mix[:, :, :0])
    with pytest.raises(ValueError):
        beamform_online(images[:, :, :1], mix[:, :1])
    with pytest.raises(ValueError):
        BeamformStream(9, 2)
    with pytest.raises(ValueError):
        BeamformStream(2, 9)
    with pytest.raises(ValueError):
        BeamformStream(2, 2, num_bins=1026)
    with pytest.raises((TypeError, ValueError)):
        BeamformStream(2, 2, kind="souden")
    sep = BlindSeparator(num_spks=2, num_ch=2, device="cuda:0")
    with pytest.raises(ValueError):                                              # the online beamformer belongs to the online path
        sep.separate_recording(np.zeros((1600, 2), np.float32), beamform=OnlineBeamformer())
