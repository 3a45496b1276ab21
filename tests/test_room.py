"""CPU tests of the room simulator: the float64 restatement of tests/room_ref.py against closed forms (an anechoic pair, seven
images written out by hand, reciprocity, the order limit, decay against beta, np.convolve), the bars of tests/test_gpu_room.py
against every planted fault, and what the library and ``misonet_amd.room`` check without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import room_ref as R

FS, C0 = R.FS, 343.0


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_anechoic_pair_is_one_exact_tap():
    """beta = 0, the source on the wall x = 0 (so p - r is -d exactly) and d = 20 c / fs: tau = 20, tap 20 is 1 / (4 pi d) bit for
    bit, and every other tap is the rounding of sin(pi k) -- a handful above 1e-15 of the peak, all far below 1e-12"""
    d = 20 * C0 / FS
    assert d * FS / C0 == 20.0
    h, f = R.rir_pair([6.0, 5.0, 3.0], [0.0] * 6, [0.0, 2.0, 1.5], [d, 2.0, 1.5], FS, 64)
    assert f == 0 and h[20] == 1.0 / (4.0 * np.pi * d)
    rest = np.abs(np.delete(h, 20)) / h[20]
    assert rest.max() < 1e-13 and (rest > 1e-15).sum() <= 12
    assert not h[61:].any()                                # past the support: exactly nothing


def _one_image(p, r, g, Lh):
    """one image at position p with gain g, written out tap by tap"""
    d = float(np.sqrt(((np.asarray(p) - np.asarray(r)) ** 2).sum()))
    tau = d * FS / C0
    h = np.zeros(Lh)
    for n in range(Lh):
        x = n - tau
        if abs(x) < 40:
            h[n] = g / (4 * np.pi * d) * 0.5 * (1 + np.cos(2 * np.pi * x / 80)) * (1.0 if x == 0 else np.sin(np.pi * x) / (np.pi * x))
    return h


def test_max_order_one_is_seven_images_by_hand():
    """the direct path and one mirror per wall, each with that wall's beta: positions by mirroring, not by the enumeration"""
    Lx, Ly, Lz = room = (3.1, 2.4, 2.2)
    beta = (0.9, 0.8, 0.7, 0.6, 0.5, 0.4)
    s, r = (1.0, 0.7, 1.2), (2.2, 1.6, 0.9)
    by_hand = [((s[0], s[1], s[2]), 1.0),
               ((-s[0], s[1], s[2]), beta[0]), ((2 * Lx - s[0], s[1], s[2]), beta[1]),
               ((s[0], -s[1], s[2]), beta[2]), ((s[0], 2 * Ly - s[1], s[2]), beta[3]),
               ((s[0], s[1], -s[2]), beta[4]), ((s[0], s[1], 2 * Lz - s[2]), beta[5])]
    want = sum(_one_image(p, r, g, 200) for p, g in by_hand)
    h, f, n = R.rir_pair(room, beta, s, r, FS, 200, max_order=1, return_count=True)
    assert f == 0 and n == 7 and R.rel_l2(h, want) <= 1e-13
    h0, _, n0 = R.rir_pair(room, beta, s, r, FS, 200, max_order=0, return_count=True)
    assert n0 == 1 and R.rel_l2(h0, _one_image(s, r, 1.0, 200)) <= 1e-13


def test_reciprocity_and_order_limit():
    room, beta = (3.0, 2.5, 2.0), R.BETAS["distinct"]
    s, r = (0.9, 1.7, 0.6), (2.3, 0.8, 1.4)
    a, _, n = R.rir_pair(room, beta, s, r, FS, 600, return_count=True)
    b, _ = R.rir_pair(room, beta, r, s, FS, 600)
    assert 15000 < n < 25000 and R.rel_l2(a, b) <= 1e-12
    big, _ = R.rir_pair(room, beta, s, r, FS, 600, max_order=10 ** 6)
    assert np.array_equal(a, big)
    few, _ = R.rir_pair(room, beta, s, r, FS, 600, max_order=3)
    assert R.rel_l2(few, a) > 1e-3                         # ... and a small one is not


def test_t30_grows_with_beta():
    """beta is the contract, rt60 nominal: nothing here holds T30 to Sabine's figure"""
    t = [R.schroeder_t30(R.rir_pair((3.0, 2.5, 2.0), [b] * 6, (1.0, 1.0, 1.0), (2.0, 1.5, 1.2), FS, 1200)[0], FS)
         for b in (0.4, 0.6, 0.75)]
    print("[room] T30 at beta 0.4 / 0.6 / 0.75:", t)
    assert all(np.isfinite(t)) and t[0] < t[1] < t[2]


def test_flags_of_the_restatement():
    room, beta, s, r = (3.0, 2.5, 2.0), [0.5] * 6, (1.0, 1.0, 1.0), (2.0, 1.5, 1.2)
    assert R.rir_pair(room, beta, s, r, FS, 50)[1] == 0
    for bad in ((room, beta, (3.1, 1, 1), r), (room, beta, s, (2, np.nan, 1)), (room, [0.5] * 5 + [1.0], s, r),
                (room, [-0.1] + [0.5] * 5, s, r), ((3.0, 0.0, 2.0), beta, (1, 0, 1), (2, 0, 1)), ((np.inf, 2.5, 2), beta, s, r)):
        h, f = R.rir_pair(*bad, FS, 50)
        assert f == 1 and not h.any()
    h, f = R.rir_pair(room, beta, s, s, FS, 50)
    assert f == 2 and np.isfinite(h).all() and h.any()
    h, f = R.rir_pair((0.004, 2.5, 2.0), beta, (0.002, 1, 1), (0.002, 1.5, 1.2), FS, 50)
    assert f == 4 and not h.any()
    assert (R.orders((7.0, 7.0, 7.0), FS, 65536) == 201).all()                                  # inside 255, but 8 x 403^3 > 2^27
    h, f = R.rir_pair((7.0, 7.0, 7.0), beta, (3.0, 3.0, 3.0), (2.0, 2.0, 2.0), FS, 65536)
    assert f == 4 and not h.any()


def test_mix_is_np_convolve_and_early_plus_late_is_full():
    x, h = R.mix_case_inputs(257, 80)
    sp = R.mix_split(40, 80)
    img, early, total = R.mix(x, h, sp)
    for s in range(2):
        for m in range(3):
            full = np.convolve(h[s, m], x[s].astype(np.float64))
            late = np.convolve(np.concatenate([np.zeros(sp[s]), h[s, m, sp[s]:]]), x[s].astype(np.float64))
            assert np.array_equal(img[s, m], full)
            assert R.rel_l2(early[s, m] + late, full) <= 1e-15
    assert np.array_equal(total, img[0] + img[1])
    cut = R.mix(x, h, sp, Lo=257)
    assert all(np.array_equal(c, f[..., :257]) for c, f in zip(cut, (img, early, total)))
    assert np.array_equal(R.mix(x, h, R.mix_split(None, 80))[1], img) and not R.mix(x, h, [0, 0])[1].any()
    assert list(R.direct_sample([[0, 0, 0], [1, 0, 0]], [[0, 0, 3.0], [0, 4.0, 0]], FS)) == [int(3.0 * FS / C0), int(np.sqrt(10) * FS / C0)]


@functools.lru_cache(maxsize=None)
def _fault_case():
    room, src, mic = R.geometry(1, 1, 1, seed=3)
    args = (room[0], R.BETAS["distinct"], src[0, 0], mic[0, 0], FS, 600)
    return args, R.rir_pair(*args)[0], R.rir_pair(*args, image_order=5)[0]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_rir_bars_reject_planted_fault(fault):
    """the bars of tests/test_gpu_room.py, on a case of its list (Lh = 600: three tiles, images past the last tap)"""
    assert R.TILE == _lib().lib().misonet_room_tile()
    args, want, perm = _fault_case()
    fig = R.figures(R.rir_pair(*args, fault=fault)[0], want, perm)
    print(f"[room] fault {fault}: " + "  ".join(f"{k} {v:.3e} (bar {b:.3e})" for k, (v, b) in fig.items()))
    assert set(R.missed(fig)) == {"rel_l2", "tap"}, fig
    assert not R.missed(R.figures(want, want, perm)) and fig["rel_l2"][1] == 1e-12 == fig["tap"][1]


@pytest.mark.parametrize("fault", R.MIX_FAULTS)
def test_mix_bars_reject_planted_fault(fault):
    """float64 -> float32 of the faulty result against the float64 reference, as the GPU test compares the kernel's; the
    float32 accumulator at every (L, Lh) of the GPU test where a sum has more than one term"""
    shapes = [(L, Lh) for L in R.MIX_L for Lh in R.MIX_LH if min(L, Lh) > 1] if fault == "f32_acc" else [(257, 300)]
    for L, Lh in shapes:
        x, h = R.mix_case_inputs(L, Lh)
        sp = R.mix_split(40, Lh)
        want = R.mix(x, h, sp)
        got = [a.astype(np.float32) for a in R.mix(x, h, sp, fault=fault)]
        clean = [a.astype(np.float32) for a in want]
        errs = {n: R.rel_l2(g, w) for n, g, w in zip(("images", "early", "mix"), got, want)}
        print(f"[room] fault {fault} L {L} Lh {Lh}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        assert all(R.rel_l2(c, w) <= R.MIX_BAR for c, w in zip(clean, want))
        hit = {"split_off_by_one": ("early",), "lost_source": ("mix",), "f32_acc": ("images", "mix")}[fault]
        assert all(errs[n] > R.MIX_BAR for n in hit), errs


def test_abi_600_and_einval_without_a_device():
    L = _lib()
    lib = L.lib()
    assert lib.misonet_version() >= 600 and lib.misonet_room_tile() == 256
    assert lib.misonet_room_rir_len(2, 2, 6, 4096) == 2 * 2 * 6 * 4096 and lib.misonet_room_mix_len(64000, 4096) == 68095
    for bad in ((0, 1, 1, 1), (4097, 1, 1, 1), (1, 0, 1, 1), (1, 5, 1, 1), (1, 1, 0, 1), (1, 1, 17, 1), (1, 1, 1, 0), (1, 1, 1, 65537)):
        assert lib.misonet_room_rir_len(*bad) == -1, bad
    assert lib.misonet_room_rir_len(4096, 4, 16, 65536) == 4096 * 4 * 16 * 65536
    for bad in ((0, 1), ((1 << 24) + 1, 1), (1, 0), (1, 65537)):
        assert lib.misonet_room_mix_len(*bad) == -1, bad
    buf = (C.c_double * 64)()
    p = C.addressof(buf)                                   # never read: every check below comes before any launch

    def rir(B=1, S=1, M=1, fs=8000.0, c=343.0, Lh=16, mo=-1, ptrs=(p, p, p, p, p, p)):
        return lib.misonet_room_rir(ptrs[0], ptrs[1], ptrs[2], ptrs[3], B, S, M, fs, c, Lh, mo, ptrs[4], ptrs[5], None)

    for kw in (dict(B=0), dict(B=4097), dict(S=0), dict(S=5), dict(M=0), dict(M=17), dict(Lh=0), dict(Lh=65537), dict(fs=0.0),
               dict(fs=float("nan")), dict(fs=float("inf")), dict(c=-1.0), dict(c=float("nan")), dict(mo=-2)):
        assert rir(**kw) == L.EINVAL, kw
    for i in range(6):
        assert rir(ptrs=tuple(None if j == i else p for j in range(6))) == L.EINVAL, i
    assert b"null" in lib.misonet_last_error()

    def mix(sb=0, ss=16, st=1, B=1, S=1, M=1, Ls=16, Lh=4, Lo=16, ptrs=(p, p, p)):
        return lib.misonet_room_mix(ptrs[0], sb, ss, st, ptrs[1], None, B, S, M, Ls, Lh, Lo, ptrs[2], None, None, None)

    for kw in (dict(B=0), dict(B=4097), dict(S=0), dict(S=5), dict(M=0), dict(M=17), dict(Lh=0), dict(Lh=65537), dict(Ls=0),
               dict(Ls=(1 << 24) + 1), dict(Lo=0), dict(Lo=20), dict(st=0), dict(ss=-1), dict(sb=-1),
               dict(B=4096, M=16, Ls=1 << 24, Lo=1 << 24)):
        assert mix(**kw) == L.EINVAL, kw
    for i in range(3):
        assert mix(ptrs=tuple(None if j == i else p for j in range(3))) == L.EINVAL, i


def test_python_validators():
    import misonet_amd as mz
    from misonet_amd import room as RM
    assert mz.Room is RM.Room and mz.simulate is RM.simulate and mz.beta_from_rt60 is RM.beta_from_rt60 and mz.Scene is RM.Scene
    dim = (6.0, 5.0, 3.0)
    b = RM.beta_from_rt60(dim, 0.4)
    assert b == np.sqrt(1 - 0.161 * 90.0 / (126.0 * 0.4)) and 0 < RM.beta_from_rt60(dim, 0.2) < b < RM.beta_from_rt60(dim, 0.6) < 1
    for bad in ((dim, 0.05), (dim, 0.0), (dim, float("nan")), ((6.0, 0.0, 3.0), 0.4)):
        with pytest.raises(ValueError):
            RM.beta_from_rt60(*bad)
    assert np.array_equal(RM.Room(dim, rt60=0.4).validate().betas(), np.full(6, b))
    assert np.array_equal(RM.Room(dim, beta=0.5).betas(), np.full(6, 0.5))
    assert np.array_equal(RM.Room(dim, beta=R.BETAS["distinct"]).validate().betas(), R.BETAS["distinct"])
    for kw in (dict(dim=dim), dict(dim=dim, beta=0.5, rt60=0.4), dict(dim=dim, beta=1.0), dict(dim=dim, beta=-0.1),
               dict(dim=dim, beta=(0.5,) * 5), dict(dim=(6.0, 5.0), beta=0.5), dict(dim=(6.0, -5.0, 3.0), beta=0.5),
               dict(dim=(6.0, np.inf, 3.0), beta=0.5), dict(dim=dim, beta=0.5, c=0.0), dict(dim=dim, rt60=0.01)):
        with pytest.raises(ValueError):
            RM.Room(**kw).validate()
    room = RM.Room(dim, beta=0.5)
    s, m = np.ones((2, 3)), np.ones((6, 3)) * 2
    for args, kw in (((room, s, m, 0, 100), {}), ((room, s, m, FS, 0), {}), ((room, s, m, FS, 65537), {}), ((room, s, m, FS, 1.5), {}),
                     ((room, s, m, FS, 100), dict(max_order=-1)), ((room, s, m, FS, 100), dict(max_order=1.0)),
                     ((room, s[None], m, FS, 100), {}), ((room, np.ones((5, 3)), m, FS, 100), {}),
                     ((room, s, np.ones((17, 3)), FS, 100), {}), ((room, s[:, :2], m, FS, 100), {}),
                     (([room, room], s, m, FS, 100), {}), (([room, RM.Room(dim, beta=0.5, c=340.0)], np.ones((2, 2, 3)), np.ones((2, 6, 3)), FS, 100), {})):
        with pytest.raises(ValueError):
            RM.rir(*args, **kw)
    with pytest.raises(TypeError):
        RM.rir(dim, s, m, FS, 100)
    assert list(RM.direct_sample(room, [[0, 0, 0], [1, 0, 0]], [[0, 0, 3.0], [0, 4.0, 0]], FS)) == \
        list(R.direct_sample([[0, 0, 0], [1, 0, 0]], [[0, 0, 3.0], [0, 4.0, 0]], FS))
    x, h = np.zeros((2, 100), np.float32), np.zeros((2, 6, 50))
    for args, kw in (((x, h, 0), {}), ((x, h, FS), dict(early_ms=-1.0)), ((x[0], h, FS), {}), ((x, h[0], FS), {}),
                     ((x, h[:1], FS), {}), ((x, h, FS), dict(out_len=0)), ((x, h, FS), dict(out_len=150)),
                     ((np.zeros((5, 100), np.float32), np.zeros((5, 6, 50)), FS), {})):
        with pytest.raises(ValueError):
            RM.mix(*args, **kw)
    for args, kw in (((x[0], room, s, m, FS, 100), {}), ((x, room, s[:1], m, FS, 100), {}),
                     ((x, room, s, m, FS, 100), dict(snr_db=float("nan")))):
        with pytest.raises(ValueError):
            RM.simulate(*args, **kw)
    with pytest.raises(TypeError):
        RM.simulate(x, [room], s, m, FS, 100)
    h = R.rir_pair((3.0, 2.5, 2.0), [0.6] * 6, (1.0, 1.0, 1.0), (2.0, 1.5, 1.2), FS, 1200)[0]
    assert RM.schroeder_t30(h, FS) == R.schroeder_t30(h, FS)
