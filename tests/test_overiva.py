"""CPU checks of the online AuxIVA for fewer sources than microphones: the NumPy restatement (tests/overiva_ref.py) has the
properties the device tests lean on -- it separates, its three invariants hold, it does not depend on how the stream is cut,
every device case's bar stays under the cap and sets no flag, and every planted mistake misses the device tests' bars on at least
one device case -- and the host side of the C ABI (version, prototypes, refusals with their messages) and of the Python options
behaves.  No kernel is launched here.

Quality, measured with this file, float64: ``sparse_mixture(1, 2, 6, 600, 16, seed=1, noise=0.1)`` at alpha 0.98, laplace, the
images at microphone 0 over the frames 300 .. 599 against the true images: 18.9 dB in the mean; the mixture itself -0.3 dB.  J
re-solved once per frame instead of after every k, on ``sparse_mixture(1, 2, 6, 400, 16, seed=1)`` at alpha 0.96, gauss: 0.2 dB
where the definition has 10.9 dB."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import iva_ref
import overiva_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = [1, 1, 2, 17]
IDS = lambda c: "x".join(map(str, c[0]))


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _kw(shape, variant):
    return dict(model=variant[0], alpha=variant[1], ref_ch=R.ref_ch_of(shape, variant))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_the_definition_separates():
    mix, img = iva_ref.sparse_mixture(1, 2, 6, 600, 16, seed=1, noise=0.1)
    x = R.to_stream(mix)
    est, images, st = R.overiva(x, 2, alpha=0.98, model="laplace")
    got = R.image_sdr_m0(images[0], img[0], 300)
    base = R.image_sdr_m0(np.stack([x[0]] * 2), img[0], 300)
    print(f"[overiva] quality: images {got:.1f} dB, mixture {base:.1f} dB")
    assert got >= base + 10.0 and not st.fail.any()
    assert est.shape == (1, 2, 600, 16) and images.shape == (1, 2, 6, 600, 16)
    assert np.array_equal(est, images[:, :, 0])                                    # est is the image at ref_ch
    # the background is what is left: the images do not add up to the input any more
    assert R.rel(images.sum(axis=1), x) > 1e-2


def test_j_once_per_frame_is_a_worse_algorithm():
    mix, img = iva_ref.sparse_mixture(1, 2, 6, 400, 16, seed=1)
    x = R.to_stream(mix)
    good = R.image_sdr_m0(R.overiva(x, 2, alpha=0.96)[1][0], img[0], 200)
    once = R.image_sdr_m0(R.overiva(x, 2, alpha=0.96, fault="j_once_per_frame")[1][0], img[0], 200)
    print(f"[overiva] J after every k {good:.1f} dB, once per frame {once:.1f} dB")
    assert good >= once + 5.0


def _same_state(a, b):
    return all(np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)) for k in R.PARTS + ("n", "fail"))


def test_restatement_is_cut_invariant():
    mix = R.inputs(2, 4, 2, 40, 4)
    e0, i0, s0 = R.overiva(mix, 2, alpha=0.96, model="laplace")
    e1, i1, s1 = R.overiva(mix, 2, alpha=0.96, model="laplace", cuts=CUTS)
    assert np.array_equal(e0.view(np.uint64), e1.view(np.uint64)) and np.array_equal(i0.view(np.uint64), i1.view(np.uint64))
    assert _same_state(s0, s1)
    e2, i2, s2 = R.overiva(mix[:, :, :12], 3, cuts=[1] * 12)
    e3, i3, s3 = R.overiva(mix[:, :, :12], 3)
    assert np.array_equal(e2.view(np.uint64), e3.view(np.uint64)) and _same_state(s2, s3)


def test_the_device_cases_cover_the_contract():
    assert len(R.PAIRS) == 28 and all(2 <= M <= 8 and 1 <= K < M for M, K in R.PAIRS)
    shapes = [c[0] for c in R.CASES]
    assert [s for s in shapes if s[3:] == (30, 2)] == [(1, M, K, 30, 2) for M, K in R.PAIRS]
    assert {(2, 6, 2, 40, 5), (1, 6, 2, 1, 1), (1, 6, 2, 300, 5)} <= set(shapes)
    used = {v for _, vs in R.CASES for v in vs}
    assert used == set(R.VARIANTS) and {v[0] for v in used} == set(R.MODELS) and {v[1] for v in used} == {0.98, 0.96}
    assert any(v[2] for v in used) and any(not v[2] for v in used)
    assert any(R.ref_ch_of(s, v) >= s[2] for s, vs in R.CASES for v in vs)
    edges = R.edge_cases(lambda M, K: 64)
    assert [c[0][4] for c in edges] == [63, 64, 65, 129] * 2 and {c[0][1:3] for c in edges} == {(2, 1), (6, 2)}


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_device_case_stays_under_the_cap(case):
    shape, variants = case
    for v in variants:
        ref = R.figures(R.case_inputs(shape), shape[2], **_kw(shape, v))
        st = ref["st"]
        orth, unit, inv = R.orthogonality_error(st.Ws, st.J, st.C), R.unit_norm_error(st.Ws, st.V), R.inverse_error(st.Ws, st.J)
        print(f"[overiva] case {shape} {v[0]} alpha {v[1]:g}: own {ref['own']:.3e}  bar {ref['bar']:.3e}  |[J, -I] C Ws^H| "
              f"{orth:.3e}  |w^H V w - 1| {unit:.3e}  |W A - [I; 0]| {inv:.3e}")
        assert ref["bar"] <= R.BAR_CAP and not st.fail.any()
        assert orth <= 1e-12 and unit <= 1e-9 and inv <= 1e-9
        assert not R.rejected(R.as_candidate(ref["est"], ref["images"], st), ref)
        rev = R.overiva(R.case_inputs(shape), shape[2], reverse=True, **_kw(shape, v))
        assert not R.rejected(R.as_candidate(*rev), ref)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_miss_the_device_bars(fault):
    """each mistake a kernel could make, planted in the restatement, is rejected by what tests/test_gpu_overiva.py asserts
    (``overiva_ref.rejected``) on a device case"""
    hits = []
    for shape, v in (((2, 6, 2, 40, 5), R.VARIANTS[3]), ((1, 4, 2, 30, 2), R.VARIANTS[0]), ((1, 3, 1, 30, 2), R.VARIANTS[1])):
        ref = R.figures(R.case_inputs(shape), shape[2], **_kw(shape, v))
        fe, fi, fs = R.overiva(R.case_inputs(shape), shape[2], fault=fault, **_kw(shape, v))
        print(f"[overiva] fault {fault} on {shape}: est {R.rel(fe, ref['est']):.3e}  images {R.rel(fi, ref['images']):.3e}  "
              + "  ".join(f"{p} {R.rel(getattr(fs, p), getattr(ref['ext'], p)):.3e}" for p in R.PARTS)
              + f"  (bars {R.OUT_BAR:g}, {ref['bar']:g})")
        hits.append(R.rejected(R.as_candidate(fe, fi, fs), ref))
    assert any(hits), fault


def test_failing_frames_and_silence():
    mix = R.inputs(1, 4, 2, 30, 3).copy()
    e0, i0, s0 = R.overiva(mix[:, :, :10], 2)
    mix[0, 1, 10, 1] = np.nan
    mix[0, 0, 10, 1] = complex(0.0, np.inf)
    e1, i1, s1 = R.overiva(mix[:, :, :11], 2)
    assert s1.fail.tolist() == [[0, 1, 0]] and s1.n.tolist() == [[11] * 3]
    assert not e1[0, :, 10, 1].any() and not i1[0, :, :, 10, 1].any()
    for p in R.PARTS:
        assert np.array_equal(getattr(s1, p)[0, 1], getattr(s0, p)[0, 1]), p
        assert not np.array_equal(getattr(s1, p)[0, 0], getattr(s0, p)[0, 0]), p
    e2, i2, s2 = R.overiva(mix, 2)
    assert np.isfinite(e2).all() and all(np.isfinite(getattr(s2, p)).all() for p in R.PARTS)
    mix = R.inputs(1, 4, 2, 30, 3).copy()
    mix[..., 2] = 0
    e3, i3, s3 = R.overiva(mix, 2)
    assert not (s3.fail & 1).any() and np.isfinite(e3).all() and not e3[..., 2].any()
    st = R.State(1, 3, 1, 1)
    st.n[:] = R.N_MAX
    R.step(st, np.ones((1, 3, 1), np.complex64))
    assert st.n.tolist() == [[R.N_MAX]]
    for M, K in ((2, 2), (3, 0), (9, 2), (1, 1)):
        with pytest.raises(ValueError):
            R.State(1, M, K, 1)


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
NEW = {"misonet_overiva_state_bytes", "misonet_overiva_bins_per_pass", "misonet_overiva_reset", "misonet_overiva",
       "misonet_overiva_debug"}


def test_abi_670():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 670
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(L.SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name), name
    assert "misonet_overiva_opts" not in hdr                                   # K is a dimension: the options are misonet_oiva_opts


def _opts(**kw):
    L = _lib()
    o = L.OivaOpts()
    L.lib().misonet_oiva_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _msg(lib):
    m = lib.misonet_last_error()
    return m.decode() if isinstance(m, bytes) else str(m)


BAD_GEOM = [(0, 6, 2, 129), (2, 1, 1, 129), (2, 9, 2, 129), (2, 6, 0, 129), (2, 6, -1, 129), (2, 6, 6, 129), (2, 6, 7, 129),
            (2, 6, 2, 0), (2, 6, 2, 1026), (1 << 22, 6, 2, 1 << 9)]


def test_sizes_and_invalid_arguments():
    L = _lib()
    lib = L.lib()
    M, K = 6, 2
    n = lib.misonet_overiva_state_bytes(16, M, K, 129)
    per_bin = (K * M + (M - K) * K + K * M * M + M * M) * 16 + 8
    assert 16 * 129 * per_bin <= n <= 16 * 129 * per_bin + 2 * 16 and n % 16 == 0     # nothing in it grows with T
    assert lib.misonet_overiva_state_bytes(1, M, K, 129) < 0.4 * 1024 * 1024
    assert n < lib.misonet_oiva_state_bytes(16, M, 129)
    for M_, K_ in R.PAIRS:
        assert lib.misonet_overiva_state_bytes(1, M_, K_, 1025) > 0
        p = lib.misonet_overiva_bins_per_pass(M_, K_)
        assert p >= 8 and p % 8 == 0, (M_, K_, p)
    assert 2 * lib.misonet_overiva_bins_per_pass(2, 1) + 1 <= 1025
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    proto = re.search(r"misonet_overiva_state_bytes\(([^)]*)\)", hdr).group(1)
    assert proto.replace(" ", "") == "intB,intM,intK,intF", proto                      # the size function is free of T
    for g in BAD_GEOM:
        assert lib.misonet_overiva_state_bytes(*g) == -1, g
        assert _msg(lib), g
    for M_, K_ in ((1, 1), (9, 2), (6, 0), (6, 7), (6, 6)):
        assert lib.misonet_overiva_bins_per_pass(M_, K_) == -1
    # K = M is refused with a message that names the determined call
    assert lib.misonet_overiva_state_bytes(1, 6, 6, 129) == -1 and "misonet_oiva" in _msg(lib)
    junk = C.c_void_p(8)
    o = _opts()
    assert lib.misonet_overiva(junk, 1, 6, 6, 10, 129, C.byref(o), junk, junk, junk, 1 << 40, None) == L.EINVAL
    assert "misonet_oiva" in _msg(lib) and "misonet_overiva" not in _msg(lib)
    assert lib.misonet_overiva(junk, 1, 6, 0, 10, 129, C.byref(o), junk, junk, junk, 1 << 40, None) == L.EINVAL
    assert "K must be in [1, M - 1]" in _msg(lib)
    # every limit is refused before any pointer is looked at: the pointers here are null or not addresses at all
    for kw in (dict(model=2), dict(ref_ch=-1), dict(ref_ch=6), dict(alpha=0.0), dict(alpha=1.0), dict(alpha=float("nan")),
               dict(floor=0.0), dict(floor=float("inf")), dict(init=0.0), dict(init=float("nan"))):
        ob = _opts(**kw)
        assert lib.misonet_overiva(junk, 2, 6, 2, 10, 129, C.byref(ob), junk, junk, junk, 1 << 40, None) == L.EINVAL, kw
        assert _msg(lib), kw
        assert lib.misonet_overiva_reset(junk, 2, 6, 2, 129, C.byref(ob), None) == L.EINVAL, kw
    for B, M_, K_, F in BAD_GEOM:
        assert lib.misonet_overiva(junk, B, M_, K_, 10, F, C.byref(o), junk, junk, junk, 1 << 40, None) == L.EINVAL, (B, M_, K_, F)
        assert lib.misonet_overiva_reset(junk, B, M_, K_, F, C.byref(o), None) == L.EINVAL, (B, M_, K_, F)
        assert lib.misonet_overiva_debug(junk, B, M_, K_, F, None, None, None, None, None, None, None) == L.EINVAL, (B, M_, K_, F)
    for T in (0, -3):
        assert lib.misonet_overiva(junk, 2, 6, 2, T, 129, C.byref(o), junk, junk, junk, 1 << 40, None) == L.EINVAL
    assert lib.misonet_overiva(junk, 2, 6, 2, 10, 129, None, junk, junk, junk, 1 << 40, None) == L.EINVAL
    assert lib.misonet_overiva(None, 2, 6, 2, 10, 129, C.byref(o), None, None, None, 0, None) == L.EINVAL
    assert lib.misonet_overiva_reset(None, 2, 6, 2, 129, C.byref(o), None) == L.EINVAL
    assert lib.misonet_overiva_debug(None, 2, 6, 2, 129, None, None, None, None, None, None, None) == L.EINVAL
    # mix and the outputs must not overlap; a short state is ENOMEM (addresses only: nothing is launched)
    a, b, c, s = C.c_void_p(1 << 30), C.c_void_p(2 << 30), C.c_void_p(3 << 30), C.c_void_p(4 << 30)
    need = lib.misonet_overiva_state_bytes(1, 3, 2, 5)
    assert lib.misonet_overiva(a, 1, 3, 2, 4, 5, C.byref(o), a, None, s, need, None) == L.EINVAL
    assert lib.misonet_overiva(a, 1, 3, 2, 4, 5, C.byref(o), C.c_void_p((1 << 30) + 8), None, s, need, None) == L.EINVAL
    assert lib.misonet_overiva(a, 1, 3, 2, 4, 5, C.byref(o), b, b, s, need, None) == L.EINVAL
    assert lib.misonet_overiva(a, 1, 3, 2, 4, 5, C.byref(o), b, a, s, need, None) == L.EINVAL
    assert lib.misonet_overiva(a, 1, 3, 2, 4, 5, C.byref(o), b, c, s, need - 1, None) == L.ENOMEM


# ---- the Python options -------------------------------------------------------------------------------------------------
def test_num_src_option():
    import misonet_amd as mz
    from misonet_amd.blind import OnlineAuxIVA
    d = OnlineAuxIVA()
    assert d.num_src is None and mz.OnlineAuxIVA is OnlineAuxIVA
    assert list(OnlineAuxIVA.__dataclass_fields__)[0] == "alpha" and list(OnlineAuxIVA.__dataclass_fields__)[-1] == "num_src"
    o = OnlineAuxIVA(num_src=2)
    assert o.num_src == 2 and o != d and o == OnlineAuxIVA(num_src=2) and OnlineAuxIVA(0.98, "gauss", 1e-10, 1.0, 0, 2) == o
    assert "num_src=2" in repr(o) and o.as_kwargs()["num_src"] == 2 and OnlineAuxIVA(**o.as_kwargs()) == o
    assert OnlineAuxIVA.of(dict(num_src=2)) == o and OnlineAuxIVA.of(o) is o
    assert OnlineAuxIVA.of(dict(num_src=2, alpha=0.96)) == OnlineAuxIVA(alpha=0.96, num_src=2)
    assert dataclasses.replace(o, ref_ch=1).num_src == 2 and dataclasses.replace(o, num_src=3).num_src == 3
    with pytest.raises(ValueError):
        OnlineAuxIVA.of(dict(sources=2))
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.alpha = 0.5
    # c_opts() is what it was: K is a dimension of the call, not a member of misonet_oiva_opts
    a, b = o.c_opts(), d.c_opts()
    assert (a.model, a.ref_ch, a.alpha, a.floor, a.init) == (b.model, b.ref_ch, b.alpha, b.floor, b.init)
    assert o.validate(6) is o and o.validate(2) is o and o.validate() is o and OnlineAuxIVA(num_src=6).validate(6).sources(6) == 6
    assert d.sources(6) == 6 and o.sources(6) == 2 and OnlineAuxIVA(num_src=1).validate(2).sources(2) == 1
    for k in (0, -1, 7, 2.0, True, "2"):
        with pytest.raises(ValueError):
            OnlineAuxIVA(num_src=k).validate(6)


def test_online_calls_refuse_before_any_launch():
    """bad shapes and fields raise on the host: no device is needed to see them"""
    from misonet_amd.beamform import OnlineBeamformer
    from misonet_amd.blind import SeparateStream, auxiva_online
    from misonet_amd.stream import StreamSeparator
    mix = R.inputs(1, 3, 2, 20, 3)
    with pytest.raises(ValueError):
        auxiva_online(mix, num_src=4)
    with pytest.raises(ValueError):
        auxiva_online(mix, num_src=0)
    with pytest.raises(ValueError):
        SeparateStream(6, num_src=7)
    with pytest.raises(ValueError):
        SeparateStream(6, num_bins=1026, num_src=2)
    with pytest.raises(ValueError):
        StreamSeparator(6, separate=dict(num_src=7))
    with pytest.raises(ValueError):
        StreamSeparator(6, separate=dict(num_src=2), rows=[2])                  # the stream has two rows: 0 and 1
    with pytest.raises(ValueError):
        StreamSeparator(6, separate=dict(num_src=2), beamform=OnlineBeamformer(), rows=[0, 5])
