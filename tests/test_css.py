"""Continuous separation on the CPU: the window plan of misonet_amd.css, the cross-fade ramp and the NumPy restatement
(tests/css_ref.py) on signals whose answer is known, and the ABI version that carries the two new entry points."""
import os

import numpy as np
import pytest

import css_ref

W0 = 64000


@pytest.mark.parametrize("H", [W0 // 2, 3 * W0 // 4])
@pytest.mark.parametrize("L", [W0 - 100, W0, W0 + 1, int(3.4 * W0)])
def test_plan_windows(L, H):
    from misonet_amd import css
    starts, K, Lp = css.plan_windows(L, W0, H)
    want = 1 if L <= W0 else 1 + -(-(L - W0) // H)
    assert K == want and starts == [k * H for k in range(K)] and Lp == (K - 1) * H + W0
    assert (starts, K, Lp) == tuple(css_ref.plan(L, W0, H))
    assert Lp >= L                                            # the windows cover the recording
    if K > 1:
        assert (K - 2) * H + W0 < L                           # ... and no window lies wholly in the padding
        assert starts[-1] + (W0 - H) <= L                     # every overlap region lies inside the real signal
    if H == W0 // 2:
        assert css.plan_windows(L, W0) == (starts, K, Lp)     # default hop: W // 2


@pytest.mark.parametrize("W,H", [(64000, 31936), (64000, 63808), (64000, 32032), (64001, 32000), (64000, 32001),
                                 (64000, 0), (0, 0), (512, 320), (-64, -32), (64000, 64000)])
def test_plan_windows_rejects(W, H):
    from misonet_amd import css
    with pytest.raises(ValueError):
        css.plan_windows(100000, W, H)


def test_plan_windows_limits():
    from misonet_amd import css
    assert css.plan_windows(100000, 64000, 32000)[1] == 3
    assert css.plan_windows(100000, 64000, 63744)[1] == 2      # W - 256: the smallest overlap
    assert css.plan_windows(100000, 512, 256)[1] > 1
    with pytest.raises(ValueError):
        css.plan_windows(0, 64000, 32000)


@pytest.mark.parametrize("ov", [256, 768, 16000, 32000])
def test_ramp_is_a_partition_of_unity(ov):
    c, r = css_ref.ramp(ov)
    assert c.dtype == np.float32 and r.dtype == np.float32
    s = c.astype(np.float64) + r.astype(np.float64)
    assert np.all(np.abs(s - 1.0) <= np.spacing(np.float32(1.0)))       # 1 float32 ulp
    assert np.all(np.diff(r) >= 0) and np.all(np.diff(c) <= 0) and r[0] < 1e-3 and c[-1] < 1e-3
    assert np.all(np.abs(r - c[::-1]) <= np.spacing(np.float32(1.0)))   # symmetric about the overlap's middle


@pytest.mark.parametrize("H", [1536, 2304])
def test_identity_windows_stitch_back(H):
    """windows cut from one signal, no permutation: the cross-fade returns the signal within 4 float32 ulp"""
    W, S = 3072, 3
    rng = np.random.default_rng(5)
    L = int(3.4 * W)
    x = rng.standard_normal((L, S)).astype(np.float32) * 0.3
    y = css_ref.windows(x, W, H).transpose(0, 2, 1).copy()            # [K, S, W]
    P = np.tile(np.arange(S, dtype=np.int32), (y.shape[0], 1))
    f32, i16 = css_ref.stitch(y, P, H, L)
    ulp = np.spacing(np.abs(x.T)).astype(np.float32)
    assert np.all(np.abs(f32 - x.T) <= 4 * ulp)
    assert np.array_equal(f32[:, :H], x.T[:, :H])                       # window 0 alone: exact


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_ref_recovers_known_shuffles(S):
    rng = np.random.default_rng(10 + S)
    K, T, d, F = 12, 49, 24, 129
    Z = (rng.standard_normal((S, (K - 1) * d + T, F)) + 1j * rng.standard_normal((S, (K - 1) * d + T, F))).astype(np.complex64)
    sig = [rng.permutation(S) for _ in range(K)]
    X = np.stack([Z[sig[k], k * d: k * d + T] for k in range(K)])        # X_k[j] = Z[sigma_k[j]]
    D = css_ref.distances(X, d)
    P = css_ref.chain(D, S)
    for k in range(K):
        inv = np.argsort(sig[k])
        assert np.array_equal(P[k], inv[sig[0]])                         # P_k[s] = sigma_k^-1[sigma_0[s]]
        assert all(sig[k][P[k][s]] == sig[0][s] for s in range(S))       # one source per output along the recording
    # an all-silent overlap keeps the previous order
    X0 = X.copy()
    X0[4, :, d:] = 0
    X0[5, :, : T - d] = 0
    P0 = css_ref.chain(css_ref.distances(X0, d), S)
    assert np.array_equal(P0[5], P0[4])


def test_ref_pick_first_minimum():
    assert list(css_ref.pick(np.zeros((3, 3)))) == [0, 1, 2]
    D = np.array([[1.0, 0.0], [0.0, 1.0]])
    assert list(css_ref.pick(D)) == [1, 0]
    assert list(css_ref.pick(np.ones((2, 2)))) == [0, 1]


def test_abi_version():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    assert L.misonet_version() >= 460
    assert L.misonet_css_scratch_bytes(5, 2, 129) == 4 * 2 * 2 * 130 * 8
    assert L.misonet_css_scratch_bytes(1, 2, 129) == 0 and L.misonet_css_scratch_bytes(0, 2, 129) == -1


def test_abi_validation_without_gpu():
    """argument checks run before any launch: bad geometries are refused on the host"""
    import ctypes as C
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib, EINVAL = _lib.lib(), _lib.EINVAL
    p = C.c_void_p(16)                                                   # never dereferenced: every call below fails first
    assert lib.misonet_css_align(p, 3, 5, 49, 129, 24, None, p, p, 1 << 20, None) == EINVAL       # S = 5
    assert lib.misonet_css_align(p, 3, 2, 49, 257, 24, None, p, p, 1 << 20, None) == EINVAL       # F != 129
    assert lib.misonet_css_align(p, 0, 2, 49, 129, 24, None, p, p, 1 << 20, None) == EINVAL       # K < 1
    assert lib.misonet_css_align(p, 3, 2, 49, 129, 0, None, p, p, 1 << 20, None) == EINVAL        # hop_frames <= 0
    assert lib.misonet_css_align(p, 3, 2, 49, 129, 45, None, p, p, 1 << 20, None) == EINVAL       # 4 shared frames
    assert lib.misonet_css_align(p, 3, 2, 49, 129, 24, None, p, p, 8, None) == _lib.ENOMEM
    assert lib.misonet_css_stitch(p, p, 3, 2, 3072, 1535, 1, 100, p, None, None) == EINVAL         # H < W/2
    assert lib.misonet_css_stitch(p, p, 3, 2, 3072, 2817, 1, 100, p, None, None) == EINVAL         # H > W - 256
    assert lib.misonet_css_stitch(p, p, 0, 2, 3072, 1536, 1, 100, p, None, None) == EINVAL         # K < 1
    assert lib.misonet_css_stitch(p, p, 3, 0, 3072, 1536, 1, 100, p, None, None) == EINVAL         # S < 1
    assert lib.misonet_css_stitch(p, p, 3, 2, 3072, 1536, 1, 2 * 1536 + 3072 + 1, p, None, None) == EINVAL   # past the end
    assert lib.misonet_css_stitch(p, p, 3, 2, 3072, 1536, 0, 1536 + 3072 + 1, p, None, None) == EINVAL
    assert lib.misonet_css_stitch(p, p, 3, 2, 3072, 1536, 1, 100, None, None, None) == EINVAL      # no output
