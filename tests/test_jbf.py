"""The joint multi-speaker beamformers (LCMV, SDW-MWF, rank-1 MWF) on the CPU: the NumPy restatement tests/jbf_ref.py -- the
oracle of tests/test_gpu_jbf.py -- against its second route, against the closed forms that define each kind and against the
conditions the device tests' bars rest on; the faults those bars have to reject; then the host side of the C ABI (version 570,
the symbols, option validation) and of the Python options.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jbf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(sh, kind, kw) for sh in R.SHAPES for kind, kw in R.options(sh)]
NEW = {"misonet_jbf_opts_default", "misonet_beamform_joint_workspace_bytes", "misonet_beamform_joint",
       "misonet_beamform_joint_debug", "misonet_pipeline_set_joint"}


def test_every_device_case_is_well_posed():
    """what the bars of the device tests assume, for every case they use: the two routes of the restatement agree to 1e-12 (the
    weight bar is 100 times their difference), the leading eigenvalue behind every relative transfer function is at least twice
    the second (d_s is not arbitrary), no bin fails"""
    assert len(CASES) == 7 * 32
    worst = dict(diff=0.0, gap=np.inf, cond=0.0, resid=0.0)
    for sh, kind, kw in CASES:
        a, b = R.case(sh, kind, kw, "a"), R.case(sh, kind, kw, "b")
        diff, bar = R.bars(sh, kind, kw)
        label = R.case_id(sh, kind, kw)
        assert diff <= 1e-12 and bar <= 1e-10, (label, diff)
        assert R.rel(b["out"], a["out"]) <= 1e-12, label
        assert a["gap"] >= 2.0 and b["gap"] >= 2.0, (label, a["gap"], b["gap"])
        assert not a["fail"].any() and not b["fail"].any(), label
        if kind == "lcmv":
            assert max(a["resid"], b["resid"]) <= 1e-11, (label, a["resid"], b["resid"])
        worst = dict(diff=max(worst["diff"], diff), gap=min(worst["gap"], a["gap"]), cond=max(worst["cond"], a["cond"]),
                     resid=max(worst["resid"], a["resid"], b["resid"]))
    print(f"[jbf-ref] route difference {worst['diff']:.2e}  gap {worst['gap']:.2f}  cond(R) {worst['cond']:.1f}  "
          f"constraint residual {worst['resid']:.2e}")
    # the rounding of the float64 output to complex64, the one thing the output bar has to cover
    out = R.case(R.SHAPES[4], "lcmv", dict(noise="residual", rtf="cw", diag_load=0.0, ref_ch=0))["out"]
    assert R.rel(out.astype(np.complex64), out) <= R.OUT_BAR / 4


def _covs(sh):
    src, mix = R.inputs(sh)
    X = src.astype(np.complex128)
    Y = mix.astype(np.complex128)
    T = X.shape[-1]
    V = Y - X.sum(axis=1)
    cov = lambda A: A @ np.conj(np.swapaxes(A, -1, -2)) / T
    return cov(X), cov(V), Y


@pytest.mark.parametrize("dl", [0.0, 1e-6])
def test_closed_forms(dl):
    """lcmv with S = 1 is the MVDR R^-1 d / (d^H R^-1 d); r1mwf with S = 1, mu = 0 is souden on (Phi_s, Phi_v + gamma tr / M I);
    mwf with mu = 1 is (sum_j Phi_j + R)^-1 Phi_s e_ref; all to 1e-12"""
    sh = R.SHAPES[0]                                                   # S = 1
    M = sh[2]
    phis, phiv, _ = _covs(sh)
    Rm = phiv + dl * np.real(np.trace(phiv, axis1=-2, axis2=-1))[..., None, None] / M * np.eye(M)
    for ref in (0, M - 1):
        r = R.case(sh, "lcmv", dict(noise="residual", rtf="cw", diag_load=dl, ref_ch=ref))
        d = r["rtf"][:, 0]                                             # [B, F, M]
        assert np.allclose(d[..., ref], 1.0, atol=1e-15)
        rid = np.linalg.solve(Rm, d[..., None])[..., 0]
        w = rid / np.einsum("bfm,bfm->bf", np.conj(d), rid)[..., None]
        assert R.rel(r["w"][:, 0], w) <= 1e-12
        # d is the principal generalised eigenvector of (Phi_s, R), scaled to 1 at ref
        lam, vec = np.linalg.eig(np.linalg.solve(Rm, phis[:, 0]))
        v = np.take_along_axis(vec, np.argmax(lam.real, axis=-1)[..., None, None], axis=-1)[..., 0]
        a = np.einsum("bfij,bfj->bfi", Rm, v)
        assert R.rel(d, a / a[..., ref:ref + 1]) <= 1e-12
        r = R.case(sh, "r1mwf", dict(mu=0.0, diag_load=dl, ref_ch=ref))
        G = np.linalg.solve(Rm, phis[:, 0])
        w = G[..., ref] / np.trace(G, axis1=-2, axis2=-1)[..., None]
        assert R.rel(r["w"][:, 0], w) <= 1e-12
    for sh in (R.SHAPES[4], R.SHAPES[5]):                              # S = 2 and 4
        M, S = sh[2], sh[1]
        phis, phiv, Y = _covs(sh)
        Rm = phiv + dl * np.real(np.trace(phiv, axis1=-2, axis2=-1))[..., None, None] / M * np.eye(M)
        r = R.case(sh, "mwf", dict(mu=1.0, diag_load=dl, ref_ch=M - 1))
        tot = phis.sum(axis=1) + Rm
        for s in range(S):
            w = np.linalg.solve(tot, phis[:, s, :, :, M - 1][..., None])[..., 0]
            assert R.rel(r["w"][:, s], w) <= 1e-12
        assert R.rel(r["out"], np.einsum("bsfm,bfmt->bstf", np.conj(r["w"]), Y)) <= 1e-14
        l = R.case(sh, "lcmv", dict(noise="residual", rtf="cw", diag_load=dl, ref_ch=0))
        g = np.einsum("bsfm,bjfm->bfsj", np.conj(l["w"]), l["rtf"])                   # w_s^H d_j = delta_sj
        assert np.max(np.abs(g - np.eye(S))) <= 1e-12


FAULT_CASES = [("other_rtf", "lcmv", dict(noise="residual", rtf="cw", diag_load=1e-6, ref_ch=0)),
               ("mirror", "lcmv", dict(noise="residual", rtf="cw", diag_load=1e-6, ref_ch=0)),
               ("mirror", "mwf", dict(mu=1.0, diag_load=1e-6, ref_ch=0)),
               ("load", "lcmv", dict(noise="mix", rtf="eig", diag_load=1e-6, ref_ch=0)),
               ("load", "mwf", dict(mu=4.0, diag_load=1e-6, ref_ch=0)),
               ("load", "r1mwf", dict(mu=1.0, diag_load=1e-6, ref_ch=0)),
               ("conj", "lcmv", dict(noise="residual", rtf="cw", diag_load=0.0, ref_ch=0)),
               ("conj", "r1mwf", dict(mu=0.0, diag_load=0.0, ref_ch=0)),
               ("ns", "mwf", dict(mu=1.0, diag_load=0.0, ref_ch=0)),
               ("ns", "r1mwf", dict(mu=1.0, diag_load=0.0, ref_ch=0))]


@pytest.mark.parametrize("fault,kind,kw", FAULT_CASES, ids=[f"{f}-{k}" for f, k, _ in FAULT_CASES])
def test_the_bars_reject_planted_faults(fault, kind, kw):
    """a wrong evaluation of the restatement misses the bars the device is held to (tests/test_gpu_jbf.py): the bars are shown to
    reject something"""
    for sh in (R.SHAPES[2], R.SHAPES[4]):                              # S = 2: one tile + 1 with odd M, and the product's shape
        good = R.case(sh, kind, kw)
        src, mix = R.inputs(sh)
        bad = R.jbf(src, mix, kind=kind, fault=fault, **kw)
        _, wbar = R.bars(sh, kind, kw)
        e_out, e_w = R.rel(bad["out"], good["out"]), R.rel(bad["w"], good["w"])
        if fault == "conj":
            assert e_w == 0.0 and e_out > 1e3 * R.OUT_BAR, (sh, e_out)
        else:
            assert e_w > 1e3 * wbar, (sh, e_w, wbar)
            if fault != "load":                                        # a loading of 1e-6 is under the output's rounding
                assert e_out > 10 * R.OUT_BAR, (sh, e_out)


def test_failure_rule_of_the_restatement():
    """an all-zero bin and an all-zero estimate of one speaker: lcmv fails as a bin, mwf gives an exact zero without a flag,
    r1mwf with mu = 0 flags that speaker; the other bins are untouched"""
    sh = R.SHAPES[2]
    src, mix = (x.copy() for x in R.inputs(sh))
    src[0, :, 1] = 0
    mix[0, 1] = 0
    src[1, 1, 3] = 0
    for route in ("a", "b"):
        l = R.jbf(src, mix, "lcmv", route=route)
        assert l["fail"][0, :, 1].all() and l["fail"][1, :, 3].all() and l["fail"].sum() == 4
        assert not l["out"][0, :, :, 1].any() and not l["out"][1, :, :, 3].any() and not l["w"][1, :, 3].any()
        m = R.jbf(src, mix, "mwf", route=route)
        assert m["fail"][0, :, 1].all() and m["fail"].sum() == 2
        assert not m["out"][1, 1, :, 3].any() and m["out"][1, 0, :, 3].any()
        r = R.jbf(src, mix, "r1mwf", mu=0.0, route=route)
        assert r["fail"][0, :, 1].all() and r["fail"][1, 1, 3] == 1 and r["fail"].sum() == 3
        r1 = R.jbf(src, mix, "r1mwf", mu=1.0, route=route)
        assert r1["fail"].sum() == 2 and not r1["out"][1, 1, :, 3].any()
        keep = np.ones(l["fail"].shape, bool)
        keep[0, :, 1] = keep[1, :, 3] = False
        assert R.rel(l["w"][keep], R.case(sh, "lcmv", dict(noise="residual", rtf="cw", diag_load=0.0, ref_ch=0), route)["w"][keep]) <= 1e-14


def test_abi_570_header_exports_and_signatures():
    from misonet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(_lib.SIGNATURES)
    assert "misonet_jbf_opts;" in hdr and "(ABI 570)" in hdr
    lib = _lib.lib()
    assert lib.misonet_version() >= 570
    for name in NEW:
        assert hasattr(lib, name)
    o = _lib.JbfOpts(9, 9, 9, 9.0, 9.0, 9)
    assert lib.misonet_jbf_opts_default(C.byref(o)) == _lib.OK
    assert (o.kind, o.noise, o.rtf, o.mu, o.diag_load, o.ref_ch) == (0, 0, 0, 1.0, 0.0, 0)
    assert lib.misonet_jbf_opts_default(None) == _lib.EINVAL
    # misonet_bf_opts and misonet_wpd_opts keep their layout
    assert C.sizeof(_lib.BfOpts) == 32 and C.sizeof(_lib.WpdOpts) == 32 and C.sizeof(_lib.JbfOpts) == 40


def _opts(**kw):
    from misonet_amd import _lib
    o = _lib.JbfOpts()
    _lib.lib().misonet_jbf_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD = [dict(kind=3), dict(kind=-1), dict(noise=2), dict(rtf=2), dict(rtf=-1), dict(diag_load=-1e-3), dict(diag_load=float("nan")),
       dict(diag_load=float("inf")), dict(ref_ch=6), dict(ref_ch=-1), dict(kind=1, mu=0.0), dict(kind=1, mu=-1.0),
       dict(kind=1, mu=float("nan")), dict(kind=2, mu=-1e-3), dict(kind=2, mu=float("inf")), dict(kind=1, noise=1),
       dict(kind=2, rtf=1), dict(kind=2, noise=1)]


def test_option_validation_reports_einval_without_a_device():
    """the checks come before any launch: the pointers are never dereferenced"""
    from misonet_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(256)
    B, S, F, M, T = 2, 2, 129, 6, 50
    al = lambda x: (x + 255) & ~255
    n_w = al(al(B * S * F * 4) + B * S * F * M * 16)
    assert lib.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(_opts())) == al(n_w + B * S * F * M * 16)
    for kind in (1, 2):                                    # no relative transfer functions
        assert lib.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(_opts(kind=kind))) == n_w
    assert lib.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(_opts(mu=-5.0))) > 0       # mu is ignored by lcmv
    assert lib.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(_opts(kind=2, mu=0.0))) == n_w
    for bad in BAD:
        o = _opts(**bad)
        assert lib.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(o)) == -1, bad
        assert lib.misonet_beamform_joint(p, p, B, S, F, M, T, C.byref(o), p, p, 1 << 40, None) == _lib.EINVAL, bad
        assert lib.misonet_last_error(), bad
        assert lib.misonet_beamform_joint_debug(p, B, S, F, M, C.byref(o), p, None, None, None) == _lib.EINVAL, bad
    big = 1 << 40
    for geo in (dict(S=0), dict(S=5), dict(S=3, M=2), dict(M=1), dict(M=9), dict(B=0), dict(F=0), dict(T=0)):
        g = dict(B=B, S=S, F=F, M=M, T=T)
        g.update(geo)
        assert lib.misonet_beamform_joint(p, p, g["B"], g["S"], g["F"], g["M"], g["T"], C.byref(_opts()), p, p, big,
                                          None) == _lib.EINVAL, geo
        if "T" not in geo:
            assert lib.misonet_beamform_joint_workspace_bytes(g["B"], g["S"], g["F"], g["M"], C.byref(_opts())) == -1, geo
    assert lib.misonet_beamform_joint(p, p, B, S, F, M, T, None, p, p, big, None) == _lib.EINVAL
    assert lib.misonet_beamform_joint_workspace_bytes(B, S, F, M, None) == -1
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.misonet_beamform_joint(args[0], args[1], B, S, F, M, T, C.byref(_opts()), args[2], args[3], big,
                                          None) == _lib.EINVAL
    assert lib.misonet_beamform_joint(p, p, B, S, F, M, T, C.byref(_opts()), p, p, n_w, None) == _lib.ENOMEM
    assert lib.misonet_beamform_joint(p, p, B, S, F, M, T, C.byref(_opts(kind=1)), p, p, n_w - 1, None) == _lib.ENOMEM
    assert lib.misonet_beamform_joint_debug(p, B, S, F, M, C.byref(_opts(kind=1)), None, p, None, None) == _lib.EINVAL
    assert lib.misonet_beamform_joint_debug(None, B, S, F, M, C.byref(_opts()), p, p, None, None) == _lib.EINVAL
    assert lib.misonet_pipeline_set_joint(None, C.byref(_opts())) == _lib.EINVAL


def test_python_options_raise_before_any_launch():
    """ValueError from the host-side check: no device, no library call"""
    from misonet_amd import Apply_Beamforming_Joint, JointBeamformer
    from misonet_amd.beamform import Beamformer
    x = np.zeros((1, 2, 5, 4, 20), np.complex64)
    y = np.zeros((1, 5, 4, 20), np.complex64)
    for bad in (dict(beamformer="mvdr"), dict(beamformer="souden"), dict(noise="all"), dict(rtf="svd"), dict(ref_ch=4),
                dict(ref_ch=-1), dict(diag_load=-1e-3), dict(diag_load=float("nan")), dict(beamformer="mwf", mu=0.0),
                dict(beamformer="r1mwf", mu=-1.0), dict(beamformer="mwf", noise="mix"), dict(beamformer="r1mwf", rtf="eig"),
                dict(beamformer={"kind": "lcmv", "gamma": 1.0})):
        with pytest.raises(ValueError):
            Apply_Beamforming_Joint(x, y, **bad)
    with pytest.raises(ValueError):                                    # more speakers than microphones
        Apply_Beamforming_Joint(np.zeros((1, 3, 5, 2, 20), np.complex64), np.zeros((1, 5, 2, 20), np.complex64))
    with pytest.raises(ValueError):
        JointBeamformer().validate(6, 5)
    with pytest.raises(TypeError):
        JointBeamformer.of(3)
    assert JointBeamformer.of(None) == JointBeamformer() and JointBeamformer.of("r1mwf").kind == "r1mwf"
    assert JointBeamformer.of({"kind": "mwf", "mu": 4.0}) == JointBeamformer(kind="mwf", mu=4.0)
    assert JointBeamformer(kind="sdw_mwf") == JointBeamformer(kind="mwf")
    jb = JointBeamformer(kind="lcmv", noise="mix", rtf="eig", diag_load=1e-6, ref_ch=2)
    assert JointBeamformer.of(jb) is jb and jb.validate(6, 2) is jb
    o = jb.c_opts()
    assert (o.kind, o.noise, o.rtf, o.mu, o.diag_load, o.ref_ch) == (0, 1, 1, 1.0, 1e-6, 2)
    o = JointBeamformer(kind="r1mwf", mu=0.0).validate(2, 2).c_opts()
    assert (o.kind, o.noise, o.rtf, o.mu) == (2, 0, 0, 0.0)
    # the joint kinds are not Beamformer kinds: a name or a dict still means Beamformer
    for kind in ("lcmv", "mwf", "r1mwf", "sdw_mwf"):
        with pytest.raises(ValueError, match="JointBeamformer"):
            Beamformer.of(kind).validate(6)
        with pytest.raises(ValueError):
            Beamformer.of({"kind": kind}).validate(6)
