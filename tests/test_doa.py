"""CPU tests of the source localisation: the host functions of ``misonet_amd.localize`` against hand values, what the library
checks without a device (ABI 610, every MISONET_EINVAL / -1 case reached with null pointers), the float64 restatement of
tests/doa_ref.py on seeded plane-wave scenes (it must find the truth), and the bars of tests/test_gpu_doa.py against every
planted fault."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import doa_ref as R

FS, C0 = 16000.0, 343.0


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


# ---- host functions ---------------------------------------------------------------------------------------------------------------
def test_delays_of_a_two_microphone_array_by_hand():
    from misonet_amd import localize as LZ
    mic = np.array([[0.1, 0.0, 0.0], [-0.1, 0.0, 0.0]])
    dirs = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [np.sqrt(0.5), np.sqrt(0.5), 0.0]])
    tau = LZ.far_field_delays(mic, dirs, C0)
    want = np.array([[-0.1, 0.1], [0.0, 0.0], [0.1, -0.1], [-0.1 * np.sqrt(0.5), 0.1 * np.sqrt(0.5)]]) / C0
    assert tau.shape == (4, 2) and tau.dtype == np.float64 and np.allclose(tau, want, rtol=0, atol=1e-18)
    # an offset of the whole array changes nothing; the wave from +x reaches the microphone at +x first
    assert np.allclose(LZ.far_field_delays(mic + 5.0, dirs, C0), tau, rtol=0, atol=1e-15) and tau[0, 0] < tau[0, 1]
    assert np.allclose(tau, R.far_delays(mic, dirs, C0), rtol=0, atol=0)
    pts = np.array([[1.1, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 0.0]])
    near = LZ.near_field_delays(mic, pts, C0)
    assert np.allclose(near[0], np.array([-0.1, 0.1]) / C0, rtol=0, atol=1e-17)               # |1.0| and |1.2|, mean removed
    assert np.allclose(near[1:], 0.0, atol=1e-18) and np.allclose(near.sum(axis=1), 0.0, atol=1e-18)
    far = LZ.near_field_delays(mic, 1e4 * dirs, C0)                                           # far points: the far field
    assert np.allclose(far, tau, rtol=0, atol=1e-9)


def test_directions():
    from misonet_amd import localize as LZ
    d = LZ.directions(4)
    assert d.shape == (4, 3) and np.allclose(d, [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], atol=1e-15)
    d = LZ.directions(72, (0.0, np.pi / 6, np.pi / 2))
    assert d.shape == (216, 3) and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
    assert np.allclose(d[72:144, 2], 0.5, atol=1e-15) and np.allclose(d[144:, 2], 1.0) and np.allclose(d[:72], R.azimuths(72), atol=1e-15)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            LZ.directions(bad)
    with pytest.raises(ValueError):
        LZ.directions(4, (float("nan"),))


def test_angular_error():
    from misonet_amd import localize as LZ
    dirs = LZ.directions(72)
    e = LZ.angular_error(dirs, np.array([[10, 40], [41, 10], [-1, 11]]), np.array([10, 40]))
    assert e.shape == (3, 2) and np.allclose(e, [[0, 0], [0, 5], [5, 180]], atol=1e-9)
    assert np.allclose(LZ.angular_error(dirs, np.array([3]), dirs[[5]]), [10.0], atol=1e-9)
    with pytest.raises(ValueError):
        LZ.angular_error(dirs, np.array([1, 2]), np.array([1]))


def test_python_validators():
    import misonet_amd as mz
    from misonet_amd import localize as LZ
    for name in ("Localizer", "localize", "localize_wav", "DoaResult", "directions", "far_field_delays", "near_field_delays",
                 "angular_error"):
        assert name in mz.__all__ and (getattr(mz, name) is getattr(LZ, name) or (name == "localize" and mz.localize is LZ))
    assert callable(mz.localize)                           # the module stands in for its function, as misonet_amd.resample does
    Z = LZ.Localizer
    assert Z.of(None) == Z() and Z.of("music").kind == "music" and Z.of(dict(num_src=2)).num_src == 2 and Z.of(Z()) == Z()
    assert Z().validate(6, 72, 10) == Z(kind="srp_phat", num_src=1, block=0, hop=0, band=None, bins=None, min_sep=0.0)
    with pytest.raises(ValueError):
        Z.of(dict(nope=1))
    with pytest.raises(TypeError):
        Z.of(3)
    for bad in (dict(kind="gcc"), dict(num_src=0), dict(num_src=5), dict(num_src=True), dict(num_src=1.0), dict(block=-1),
                dict(hop=-1), dict(block=1.5), dict(min_sep=-0.1), dict(min_sep=float("nan")), dict(min_sep=float("inf")),
                dict(band=(100.0, 50.0)), dict(band=(-1.0, 50.0)), dict(band=(0.0,)), dict(bins=(3, 2)), dict(bins=(-1, 2)),
                dict(bins=(1.0, 2)), dict(band=(0.0, 100.0), bins=(0, 1))):
        with pytest.raises(ValueError):
            Z(**bad).validate()
    for kw, dims in ((dict(), (1, 72, 10)), (dict(), (9, 72, 10)), (dict(kind="music", num_src=3), (3, 72, 10)),
                     (dict(num_src=2), (6, 1, 10)), (dict(), (6, 0, 10)), (dict(), (6, 65537, 10)), (dict(block=11), (6, 72, 10))):
        with pytest.raises(ValueError):
            Z(**kw).validate(*dims)
    assert Z(kind="music", num_src=2).validate(3, 72, 10).num_src == 2
    assert Z().bin_range(129, FS) == (0, 128) and Z(bins=(4, 100)).bin_range(129, FS) == (4, 100)
    assert Z(band=(250.0, 6250.0)).bin_range(129, FS) == (4, 100) and Z(band=(251.0, 6249.0)).bin_range(129, FS) == (5, 99)
    assert Z(band=(0.0, 1e6)).bin_range(129, FS) == (0, 128) and Z().bin_range(1, FS) == (0, 0)
    for z in (Z(bins=(4, 129)), Z(band=(9000.0, 9001.0)), Z(band=(260.0, 300.0))):
        with pytest.raises(ValueError):
            z.bin_range(129, FS)
    o = Z(kind="music", num_src=2, block=16, hop=8, bins=(4, 100), min_sep=0.3).c_opts(129, FS)
    assert (o.kind, o.num_src, o.block, o.hop, o.f_lo, o.f_hi, o.min_sep) == (2, 2, 16, 8, 4, 100, 0.3)
    # every argument error of localize is a ValueError before anything is launched (no device here)
    spec = np.zeros((1, 9, 3, 8), np.complex64)
    tau, pts = np.zeros((5, 3)), np.zeros((5, 3))
    for args, kw in (((spec[0], tau, pts, FS), {}), ((spec, tau[:, :2], pts, FS), {}), ((spec, tau, pts[:4], FS), {}),
                     ((spec, np.zeros((2, 5, 3)), pts, FS), {}), ((spec, tau * np.nan, pts, FS), {}), ((spec, tau, pts, 0.0), {}),
                     ((spec, tau, pts, float("nan")), {}), ((spec, tau, pts, FS), dict(kind="music", num_src=3)),
                     ((spec, tau, pts, FS), dict(block=9)), ((spec, tau, pts, FS), dict(bins=(0, 9))),
                     ((spec, tau, pts, FS), dict(weight=np.zeros((1, 2, 9, 7), np.float32))),
                     ((spec, tau, pts, FS), dict(weight=np.zeros((1, 9, 9, 8), np.float32))),
                     ((spec, tau, pts, FS), dict(num_src=6)), ((spec, tau, pts, FS), dict(localizer=dict(kind="x")))):
        with pytest.raises(ValueError):
            LZ.localize(*args, **kw)
    for wav in (np.zeros((640,), np.float32), np.zeros((640, 1), np.float32), np.zeros((640, 9), np.float32)):
        with pytest.raises(ValueError):
            LZ.localize_wav(wav, tau, pts, FS)
    with pytest.raises(ValueError):
        LZ.localize_wav(np.zeros((640, 3), np.float32), tau, pts, FS, block=100)


# ---- the library without a device ------------------------------------------------------------------------------------------------
def test_abi_610_and_einval_without_a_device():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 610
    for name in ("misonet_doa_opts_default", "misonet_doa_tile", "misonet_doa_bin_chunk", "misonet_doa_blocks",
                 "misonet_doa_workspace_bytes", "misonet_doa", "misonet_doa_debug"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.misonet_doa_tile() >= 64 and lib.misonet_doa_tile() % 64 == 0 and lib.misonet_doa_bin_chunk() >= 1
    # misonet_doa_blocks: the block rule of the definition
    for (T, block, hop), n in (((10, 0, 0), 1), ((10, 0, 3), 1), ((10, 10, 1), 1), ((10, 4, 0), 2), ((10, 4, 4), 2), ((10, 4, 2), 4),
                               ((10, 4, 3), 3), ((10, 1, 1), 10), ((200, 16, 8), 24), ((1001, 16, 16), 62), ((1, 1, 0), 1)):
        assert lib.misonet_doa_blocks(T, block, hop) == n == R.blocks(T, block, hop)[2], (T, block, hop)
    for bad in ((0, 0, 0), (10, 11, 1), (10, -1, 0), (10, 4, -1)):
        assert lib.misonet_doa_blocks(*bad) == -1, bad
    o = L.DoaOpts()
    assert lib.misonet_doa_opts_default(C.byref(o)) == L.OK and lib.misonet_doa_opts_default(None) == L.EINVAL
    assert (o.kind, o.num_src, o.block, o.hop, o.f_lo, o.f_hi, o.min_sep) == (1, 1, 0, 0, 0, -1, 0.0)

    buf = (C.c_double * 64)()
    p = C.addressof(buf)                                   # never read: every check below comes before any launch

    def opts(**kw):
        v = dict(kind=1, num_src=1, block=0, hop=0, f_lo=0, f_hi=8, min_sep=0.0)
        v.update(kw)
        return L.DoaOpts(*(v[k] for k in ("kind", "num_src", "block", "hop", "f_lo", "f_hi", "min_sep")))

    def size(B=1, K=1, F=9, M=3, T=8, D=5, o=None, **kw):
        return lib.misonet_doa_workspace_bytes(B, K, F, M, T, D, C.byref(opts(**kw)) if o is None else o)

    def call(B=1, K=1, F=9, M=3, T=8, D=5, Bg=1, fs=FS, ptrs=(p,) * 9, ws_bytes=1 << 40, **kw):
        return lib.misonet_doa(ptrs[0], ptrs[1], ptrs[2], Bg, ptrs[3], B, K, F, M, T, D, fs, C.byref(opts(**kw)), ptrs[4], ptrs[5],
                               ptrs[6], ptrs[7], ptrs[8], ws_bytes, None)

    n_ws = size()
    assert n_ws >= 9 * 3 * 3 * 16 and size(f_hi=-1) == n_ws and size(K=3) > n_ws and size(block=4, hop=2) >= 3 * 9 * 9 * 16
    bad = (dict(M=1), dict(M=9), dict(K=0), dict(K=9), dict(num_src=0), dict(num_src=5), dict(num_src=3, D=2),
           dict(kind=2, num_src=3, M=3), dict(kind=2, num_src=2, M=2), dict(D=0), dict(D=65537), dict(B=0), dict(F=0), dict(T=0),
           dict(f_lo=-1), dict(f_lo=5, f_hi=4), dict(f_hi=9), dict(f_hi=-2), dict(min_sep=-1.0), dict(min_sep=float("nan")),
           dict(min_sep=float("inf")), dict(block=9), dict(block=-1), dict(hop=-1), dict(kind=3), dict(kind=-1),
           dict(B=1 << 15, D=1 << 16), dict(B=1 << 12, K=8, D=1 << 16), dict(B=1 << 20, T=1 << 12, block=1, hop=1, D=1))
    for kw in bad:
        assert size(**kw) == -1, kw
        assert call(**kw) == L.EINVAL and lib.misonet_last_error(), kw
    assert size(o=None) > 0 and lib.misonet_doa_workspace_bytes(1, 1, 9, 3, 8, 5, None) == -1
    assert size(kind=2, num_src=2, M=3) > 0 and size(num_src=4, D=4) > 0 and size(M=8, K=8, D=65536) > 0
    assert size(B=1 << 14, D=1 << 16) > 0                  # B K N D = 2^30
    for kw in (dict(Bg=2), dict(Bg=0), dict(fs=0.0), dict(fs=float("nan")), dict(fs=float("inf")), dict(fs=-1.0)):
        assert call(**kw) == L.EINVAL, kw
    for i in range(9):
        if i == 1:
            continue                                       # the weights may be NULL
        assert call(ptrs=tuple(None if j == i else p for j in range(9))) == L.EINVAL, i
        assert b"null" in lib.misonet_last_error()
    assert call(K=2, ptrs=(p, None) + (p,) * 7) == L.EINVAL            # no weights: K = 1
    assert call(ws_bytes=n_ws - 1) == L.ENOMEM
    assert lib.misonet_doa_debug(None, 1, 1, 9, 3, 8, 5, C.byref(opts()), None, None, None, None) == L.EINVAL
    assert lib.misonet_doa_debug(p, 1, 1, 9, 1, 8, 5, C.byref(opts()), None, None, None, None) == L.EINVAL


# ---- the restatement finds the truth ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(M, seed):
    return R.plane_wave_scene(M, seed)


@pytest.mark.parametrize("seed", R.SCENE_SEEDS)
@pytest.mark.parametrize("M", R.SCENE_M)
def test_restatement_finds_two_plane_waves(M, seed):
    """circular array, 5 cm radius, 72 azimuths, two sources at least 30 degrees apart, 64 frames, 20 dB SNR, bins 4 .. 100,
    16 kHz: music finds exactly the two true indices, srp and srp_phat find them within one grid step"""
    mix, tau, dirs, truth = _scene(M, seed)
    assert R.grid_distance(truth[0, 0], truth[0, 1], 72) >= 6
    sep = 2.0 * np.sin(np.radians(12.5))                   # candidates closer than 12.5 degrees to a peak are retired
    for kind in R.KINDS:
        r = R.localize(mix, tau, dirs, FS, kind, 2, f_lo=R.SCENE_BAND[0], f_hi=R.SCENE_BAND[1], min_sep=sep)
        found = np.sort(r["peak"][0, 0, 0])
        dist = R.grid_distance(found, truth[0], 72)
        print(f"[doa] scene M{M} seed {seed} {kind}: truth {truth[0].tolist()} found {found.tolist()}")
        assert r["used"][0, 0, 0] == 97 and r["fail"][0, 0, 0] == 0
        assert (dist == 0).all() if kind == "music" else (dist <= 1).all(), (kind, found, truth[0])
        if kind == "music":
            assert (r["q"] >= -1e-12).all() and (r["q"] <= 1.0 + 1e-12).all()


def test_restatement_flags_blocks_and_peak_rule():
    mix, tau, dirs, _ = _scene(6, 0)
    mix = mix[:, :20].copy()
    mix[0, 5, 2, 40] = np.nan
    r = R.localize(mix, tau, dirs, FS, "srp", 1, block=16, hop=16, f_lo=2, f_hi=9)
    assert r["q"].shape == (1, 1, 4, 72) and r["used"].tolist() == [[[8, 8, 7, 8]]] and r["fail"].tolist() == [[[0, 0, 1, 0]]]
    assert np.isfinite(r["q"]).all() and r["state"][0, 0, 2, 5] == 1 and (r["state"][0, 0, :, 10:] == 3).all()
    z = R.localize(np.zeros_like(mix), tau, dirs, FS, "music", 2)
    assert (z["fail"] == 2).all() and (z["used"] == 0).all() and not z["q"].any() and z["peak"].tolist() == [[[[0, 1]]]]
    one = mix[:, :, :, :1]                                  # rank 1: music with S = 2 skips every bin, with S = 1 none
    assert (R.localize(one, tau, dirs, FS, "music", 2, f_hi=9)["fail"] == 2).all()
    assert (R.localize(one, tau, dirs, FS, "music", 1, f_hi=9)["used"] == 10).all()
    q = np.array([[[[1.0, 5.0, 5.0, 4.0, 0.0]]]])
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [1.5, 0, 0], [9.0, 0, 0]])
    assert R.peaks(q, pts, 3, "srp", 0.0)[0].tolist() == [[[[1, 2, 3]]]]                     # the lower of two equal ones first
    assert R.peaks(q, pts, 3, "srp", 0.6)[0].tolist() == [[[[1, 0, 4]]]]
    assert R.peaks(q, pts, 3, "srp", 100.0)[0].tolist() == [[[[1, -1, -1]]]]
    assert R.peaks(q, pts, 2, "music", 0.0)[0].tolist() == [[[[4, 0]]]]


# ---- the bars reject every planted fault ------------------------------------------------------------------------------------------
FAULT_KIND = dict(conj_phase="srp", no_diag="srp", drop_pair="srp_phat", no_phat="srp_phat", bin_off="srp", seam_off="srp_phat",
                  used_nodiv="music", subspace_swap="music", class_swap="srp")


@functools.lru_cache(maxsize=None)
def _fault_case():
    case = dict(B=2, K=2, Bg=1, F=33, M=4, T=40, D=37, S=2, block=16, hop=8, f_lo=2, f_hi=30, weights="random", min_sep=0.3, seed=77)
    return case, R.case_inputs(case)


def _run(case, inp, kind, **kw):
    mix, w, tau, pts = inp
    return R.localize(mix, tau, pts, FS, kind, R.case_kind_S(case, kind), case["block"], case["hop"], case["f_lo"], case["f_hi"],
                      case["min_sep"], w, **kw)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_bars_reject_planted_fault(fault):
    assert set(FAULT_KIND) == set(R.FAULTS)
    case, inp = _fault_case()
    kind = FAULT_KIND[fault]
    want, perm = _run(case, inp, kind), _run(case, inp, kind, frame_order=5)
    clean = R.figures(perm["q"], want["q"], perm["q"])
    assert not R.missed(clean) and all(bar <= 1e-11 for _, bar in clean.values()), clean
    with R.plant(fault):
        got = _run(case, inp, kind)
    fig = R.figures(got["q"], want["q"], perm["q"])
    print(f"[doa] fault {fault} ({kind}): " + "  ".join(f"{k} {v:.3e} (bar {bar:.3e})" for k, (v, bar) in fig.items()))
    assert sorted(R.missed(fig)) == ["cand", "rel_l2"], fig
    assert np.array_equal(_run(case, inp, kind)["q"], want["q"])       # the fault is gone again
