"""The selectable beamformers on the CPU: the NumPy / SciPy restatement (tests/beamform_ref.py, the oracle of
tests/test_gpu_beamform.py) against the MVDR oracle, against the reference's own helpers where it has them, and against the
properties that define each kind; then the host side of the C ABI (version 510, the symbols, option validation).  No device
is needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import beamform_ref as R
from conftest import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 17, 4, 50), (1, 9, 2, 7), (1, 5, 8, 33)]


def test_defaults_equal_the_mvdr_oracle():
    from oracle import mvdr_oracle
    for shape in SHAPES:
        src, mix = R.rank1_inputs(*shape)
        a = R.beamform_parts(src, mix)
        b = mvdr_oracle.mvdr_parts(src, mix, dtype=np.complex128)
        assert rel_l2(a["phin"], b["scm_n"] + 1e-6 * np.eye(shape[2])) < 1e-14
        assert rel_l2(a["w"], b["w"]) < 1e-12 and rel_l2(a["out"], b["out"]) < 1e-12, shape


@pytest.fixture(scope="module")
def ref_tester():
    """the reference's tester module through the shims of oracle/gen_golden.py; what the import adds to sys.path and
    sys.modules is taken out again"""
    from oracle import gen_golden
    if not os.path.isfile(os.path.join(gen_golden.REF, "tester.py")):
        pytest.skip("the reference tree is not on this machine")
    path, mods = list(sys.path), dict(sys.modules)
    had_complex = hasattr(np, "complex")
    try:
        _, tester, _ = gen_golden.import_reference()
        yield tester
    finally:
        sys.path[:] = path
        for k in set(sys.modules) - set(mods):
            del sys.modules[k]
        for k in ("soundfile", "model", "tester"):
            if k in mods:
                sys.modules[k] = mods[k]
        if not had_complex and hasattr(np, "complex"):
            del np.complex


def test_ban_and_mix_equal_the_reference(ref_tester):
    tst = object.__new__(ref_tester.Tester_Enhance)        # the array helpers use no attribute of the instance
    src, mix = R.rank1_inputs(2, 17, 4, 50)
    p = R.beamform_parts(src, mix)
    # BAN: the reference's helper on the restatement's own w and Phi_n' (tester.py:1186-1208)
    want = tst.blind_analytic_normalization(p["w"].copy(), p["phin"].copy())
    assert rel_l2(R.ban(p["w"], p["phin"]), want) < 1e-14
    got = R.beamform_parts(src, mix, ban_=True)
    assert rel_l2(got["w"], want) < 1e-14
    # noise = "mix": the reference with tester.py:1095 swapped for :1096 -- its second covariance (the noise one) takes the
    # mixture instead of mix - source
    scm, calls = tst.get_spatial_covariance_matrix, []

    def swapped(observation, normalize):
        calls.append(1)
        return scm(mix.astype(np.complex128) if len(calls) == 2 else observation, normalize)
    tst.get_spatial_covariance_matrix = swapped
    out = tst.Apply_Beamforming(src.astype(np.complex128), mix.astype(np.complex128)).numpy()
    assert len(calls) == 2
    e = rel_l2(R.beamform_parts(src, mix, noise="mix")["out"], out)
    print(f"[beamform] noise=mix against the reference with :1095 swapped: {e:.3e}")
    assert e < 1e-10
    assert rel_l2(R.beamform_parts(src, mix)["out"], out) > 1e-3            # and the swap is not a no-op


def _snr(w, phis, phin):
    num = np.einsum("...a,...ab,...b->...", w.conj(), phis, w).real
    return num / np.einsum("...a,...ab,...b->...", w.conj(), phin, w).real


@pytest.mark.parametrize("opts", [dict(), dict(noise="mix"), dict(condition=1e-3, trace_normalize=True), dict(ref_ch=1)])
def test_properties_of_the_kinds(opts):
    for shape in SHAPES:
        src, mix = R.rank1_inputs(*shape)
        ref_ch = opts.get("ref_ch", 0)
        g = R.beamform_parts(src, mix, kind="gev", **opts)
        m = R.beamform_parts(src, mix, kind="mvdr", **opts)
        s = R.beamform_parts(src, mix, kind="souden", **opts)
        phis, phin, w, lam = g["phis"], g["phin"], g["w"], g["lam"]
        lhs = np.einsum("...ab,...b->...a", phis, w)
        rhs = lam[..., None] * np.einsum("...ab,...b->...a", phin, w)
        assert np.all(np.linalg.norm(lhs - rhs, axis=-1) <= 1e-10 * np.linalg.norm(lhs, axis=-1))
        assert np.allclose(np.einsum("...a,...ab,...b->...", w.conj(), phin, w), 1.0, rtol=1e-12, atol=0)
        z = np.einsum("...ab,...b->...a", phin, w)[..., ref_ch]
        assert np.all(z.real >= 0) and np.all(np.abs(z.imag) <= 1e-14 * np.abs(z))
        # lambda_max is the largest output SNR any w can reach (Rayleigh quotient): on every bin
        sg, sm, ss = _snr(w, phis, phin), _snr(m["w"], phis, phin), _snr(s["w"], phis, phin)
        assert np.all(sg >= sm * (1 - 1e-12)) and np.all(sg >= ss * (1 - 1e-12))
        assert np.allclose(sg, lam, rtol=1e-10, atol=0)
        # BAN only scales w: the SNR and the direction stay
        gb = R.beamform_parts(src, mix, kind="gev", ban_=True, **opts)
        assert np.allclose(_snr(gb["w"], phis, phin), sg, rtol=1e-10, atol=0)


def test_souden_on_rank_one_is_mvdr_towards_the_relative_transfer_function():
    """Phi_s = sigma a a^H exactly: G = sigma Phi_n'^-1 a a^H, tr G = sigma a^H Phi_n'^-1 a, so
    w = Phi_n'^-1 a conj(a[ref]) / (a^H Phi_n'^-1 a) = MVDR with d = a / a[ref]"""
    r = np.random.default_rng(3)
    B, F, M, T = 1, 7, 5, 40
    a = r.standard_normal((B, F, M, 1)) + 1j * r.standard_normal((B, F, M, 1))
    s = r.standard_normal((B, F, 1, T)) + 1j * r.standard_normal((B, F, 1, T))
    src = a * s
    mix = src + 0.5 * (r.standard_normal((B, F, M, T)) + 1j * r.standard_normal((B, F, M, T)))
    for ref_ch in (0, 3):
        p = R.beamform_parts(src, mix, kind="souden", ref_ch=ref_ch)
        d = a[..., 0] / a[..., ref_ch:ref_ch + 1, 0]
        num = np.linalg.solve(p["phin"], d[..., None])[..., 0]
        w = num / np.einsum("...d,...d->...", d.conj(), num)[..., None]
        assert rel_l2(p["w"], w) < 1e-9


def test_edges_of_the_restatement():
    src, mix = R.rank1_inputs(1, 5, 4, 20)
    z = np.zeros_like(src)
    assert np.all(R.beamform_parts(z, mix, kind="souden")["out"] == 0)
    assert np.all(np.isfinite(R.beamform_parts(z, mix, kind="gev")["out"]))
    for bad in (dict(kind="lcmv"), dict(noise="all"), dict(ref_ch=4), dict(ref_ch=-1), dict(condition=-1e-3)):
        with pytest.raises(ValueError):
            R.beamform_parts(src, mix, **bad)


# ---- the host side of the C ABI ------------------------------------------------------------------------------------
NEW = {"misonet_bf_opts_default", "misonet_beamform_workspace_bytes", "misonet_beamform", "misonet_beamform_debug",
       "misonet_pipeline_set_beamformer"}


def test_abi_510_header_exports_and_signatures():
    from misonet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(_lib.SIGNATURES)
    assert "misonet_bf_opts;" in hdr
    lib = _lib.lib()
    assert lib.misonet_version() >= 510
    for name in NEW:
        assert hasattr(lib, name)
    o = _lib.BfOpts(9, 9, 9.0, 9, 9.0, 9, 9)
    assert lib.misonet_bf_opts_default(C.byref(o)) == _lib.OK
    assert (o.kind, o.noise, o.condition, o.trace_normalize, o.ban, o.ref_ch) == (0, 0, 0.0, 0, 0, 0)
    assert o.epsi == np.float32(1e-6)
    assert lib.misonet_bf_opts_default(None) == _lib.EINVAL


def _opts(**kw):
    from misonet_amd import _lib
    o = _lib.BfOpts()
    _lib.lib().misonet_bf_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD = [dict(kind=3), dict(kind=-1), dict(noise=2), dict(condition=-1e-3), dict(condition=float("nan")),
       dict(condition=float("inf")), dict(epsi=-1.0), dict(ref_ch=6), dict(ref_ch=-1)]


def test_option_validation_reports_einval_without_a_device():
    """the checks come before any launch: the pointers are never dereferenced"""
    from misonet_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(256)
    B, F, M, T = 2, 129, 6, 50
    n_mvdr = lib.misonet_mvdr_workspace_bytes(B, F, M)
    assert lib.misonet_beamform_workspace_bytes(B, F, M, C.byref(_opts())) == n_mvdr
    for kind in (1, 2):                                    # souden / gev: Phi_s [B, F, M, M] complex128 and lambda [B, F] more
        assert lib.misonet_beamform_workspace_bytes(B, F, M, C.byref(_opts(kind=kind))) == n_mvdr + B * F * (M * M * 16 + 8)
    for bad in BAD:
        o = _opts(**bad)
        assert lib.misonet_beamform_workspace_bytes(B, F, M, C.byref(o)) == -1, bad
        assert lib.misonet_beamform(p, p, B, F, M, T, C.byref(o), p, p, 1 << 40, None) == _lib.EINVAL, bad
        assert lib.misonet_last_error(), bad
        assert lib.misonet_beamform_debug(p, B, F, M, C.byref(o), p, None, None) == _lib.EINVAL, bad
    assert lib.misonet_beamform(p, p, B, F, M, T, None, p, p, 1 << 40, None) == _lib.EINVAL
    assert lib.misonet_beamform(p, p, B, F, 9, T, C.byref(_opts()), p, p, 1 << 40, None) == _lib.EINVAL
    assert lib.misonet_beamform(p, p, B, F, M, T, C.byref(_opts(kind=2)), p, p, n_mvdr, None) == _lib.ENOMEM
    assert lib.misonet_beamform_debug(p, B, F, M, C.byref(_opts(kind=1)), None, C.cast(p, C.c_void_p), None) == _lib.EINVAL
    assert lib.misonet_pipeline_set_beamformer(None, C.byref(_opts())) == _lib.EINVAL


def test_python_options_raise_before_any_launch():
    """ValueError from the host-side check: no device, no library call"""
    from misonet_amd.beamform import Apply_Beamforming, Beamformer
    x = np.zeros((1, 5, 4, 20), np.complex64)
    for bad in (dict(beamformer="lcmv"), dict(noise="all"), dict(ref_ch=4), dict(ref_ch=-1), dict(condition=-1e-3),
                dict(beamformer={"kind": "gev", "gamma": 1.0})):
        with pytest.raises(ValueError):
            Apply_Beamforming(x, x, **bad)
    assert Beamformer.of({"kind": "gev", "ban": True}) == Beamformer(kind="gev", ban=True)
    assert Beamformer.of(None) == Beamformer() and Beamformer.of("souden").kind == "souden"
    o = Beamformer(kind="gev", noise="mix", condition=1e-3, trace_normalize=True, ban=True, ref_ch=2).c_opts()
    assert (o.kind, o.noise, o.condition, o.trace_normalize, o.ban, o.ref_ch) == (2, 1, 1e-3, 1, 1, 2)
    assert o.epsi == np.float32(1e-6)
