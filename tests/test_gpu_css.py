"""GPU tests of continuous separation (csrc/css.hip, misonet_amd/css.py, Enhancer.enhance_continuous): speaker tracking
across overlapping windows and the cross-fade stitch, against the NumPy restatement in tests/css_ref.py, the existing
window-wise entry points and the CPU oracle."""
import numpy as np
import pytest
import torch

import css_ref
from test_gpu_parity import nets, _need_gpu      # noqa: F401

pytestmark = pytest.mark.gpu

F = 129


def _shuffled_windows(rng, S, K, T, d):
    """a consistent random complex signal [S, Ttot, F] cut into K windows of T frames d apart, each window's speakers
    shuffled by sigma_k: X_k[j] = Z[sigma_k[j]]"""
    Ttot = (K - 1) * d + T
    Z = (rng.standard_normal((S, Ttot, F)) + 1j * rng.standard_normal((S, Ttot, F))).astype(np.complex64)
    sig = [rng.permutation(S) for _ in range(K)]
    return np.stack([Z[sig[k], k * d: k * d + T] for k in range(K)]), sig


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_align_recovers_known_shuffles(S):
    _need_gpu()
    from misonet_amd import css
    rng = np.random.default_rng(100 + S)
    K, T, d = 200, 49, 24
    X, sig = _shuffled_windows(rng, S, K, T, d)
    est = torch.from_numpy(X).cuda()
    P, D = css.align(est, d)
    P2, D2 = css.align(est, d)
    torch.cuda.synchronize()
    assert torch.equal(P, P2) and torch.equal(D, D2)                 # bit-reproducible
    P, D = P.cpu().numpy(), D.cpu().numpy()
    for k in range(K):
        assert np.array_equal(P[k], np.argsort(sig[k])[sig[0]]), k     # P_k[s] = sigma_k^-1[sigma_0[s]]
    Dref = css_ref.distances(X, d)
    assert D.shape == (K - 1, S, S)
    assert np.all(np.abs(D - Dref) <= 1e-12 * np.abs(Dref)), np.max(np.abs(D - Dref) / np.maximum(np.abs(Dref), 1e-300))
    # an all-zero overlap keeps the previous P; a given perm0 is composed through
    X0 = X.copy()
    X0[50, :, d:] = 0
    X0[51, :, : T - d] = 0
    P0, D0 = css.align(torch.from_numpy(X0).cuda(), d)
    P0 = P0.cpu().numpy()
    assert np.all(D0[50].cpu().numpy() == 0) and np.array_equal(P0[51], P0[50])
    if S > 1:
        p0 = np.roll(np.arange(S), 1).astype(np.int32)
        Pc, _ = css.align(est, d, perm0=torch.from_numpy(p0).cuda())
        Pc = Pc.cpu().numpy()
        assert np.array_equal(Pc, css_ref.chain(Dref, S, p0))
        assert np.array_equal(Pc[0], p0)


def _stitch_case(rng, K, S, W, H):
    y = (0.4 * rng.standard_normal((K, S, W))).astype(np.float32)
    P = np.stack([rng.permutation(S) for _ in range(K)]).astype(np.int32)
    return y, P


@pytest.mark.parametrize("H", [1536, 2304])
def test_stitch_against_ref(H):
    _need_gpu()
    from misonet_amd import css
    rng = np.random.default_rng(H)
    W, S, K = 3072, 2, 6
    L = (K - 1) * H + W - 777                                          # a trimmed tail
    y, P = _stitch_case(rng, K, S, W, H)
    yd, Pd = torch.from_numpy(y).cuda(), torch.from_numpy(P).cuda()
    f32 = css.stitch(yd, Pd, H, True, L, dtype=torch.float32).cpu().numpy()
    i16 = css.stitch(yd, Pd, H, True, L).cpu().numpy()
    rf, ri = css_ref.stitch(y, P, H, L)
    assert f32.shape == (S, L) and i16.shape == (S, L) and i16.dtype == np.int16
    assert np.abs(f32 - rf).max() <= 1e-6
    assert np.abs(i16.astype(np.int32) - ri.astype(np.int32)).max() <= 1
    # windows cut from one random signal, identity P: the signal back within 4 float32 ulp
    x = (0.3 * rng.standard_normal((L, S))).astype(np.float32)
    yw = css_ref.windows(x, W, H).transpose(0, 2, 1).copy()
    Pi = np.tile(np.arange(S, dtype=np.int32), (yw.shape[0], 1))
    back = css.stitch(torch.from_numpy(yw).cuda(), torch.from_numpy(Pi).cuda(), H, True, L, dtype=torch.float32).cpu().numpy()
    assert np.all(np.abs(back - x.T) <= 4 * np.spacing(np.abs(x.T)))


def _batched(est, y, d, H, L, nb):
    """align + stitch in batches of nb windows, each batch carrying the previous one's last window"""
    from misonet_amd import css
    K, S = est.shape[:2]
    P_all, outs, outs32, lo, prev = [], [], [], 0, None
    while lo < K:
        hi = min(K, lo + nb)
        c = 1 if lo else 0
        P, _ = css.align(est[lo - c: hi], d, perm0=prev)
        n_out = (L if hi == K else hi * H) - lo * H
        outs.append(css.stitch(y[lo - c: hi], P, H, c == 0, n_out))
        outs32.append(css.stitch(y[lo - c: hi], P, H, c == 0, n_out, dtype=torch.float32))
        P_all.append(P[c:])
        prev = P[-1].clone()
        lo = hi
    return torch.cat(P_all), torch.cat(outs, 1), torch.cat(outs32, 1)


@pytest.mark.parametrize("H", [1536, 2304])
def test_carry_equivalence(H):
    _need_gpu()
    from misonet_amd import css
    rng = np.random.default_rng(7 + H)
    W, S, K = 3072, 3, 15
    T, d = W // 64 + 1, H // 64
    L = (K - 1) * H + W - 300
    X, _ = _shuffled_windows(rng, S, K, T, d)
    X = X + (0.05 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))).astype(np.complex64)
    est = torch.from_numpy(X).cuda()
    y = torch.from_numpy((0.4 * rng.standard_normal((K, S, W))).astype(np.float32)).cuda()
    P1, _ = css.align(est, d)
    o1 = css.stitch(y, P1, H, True, L)
    o1f = css.stitch(y, P1, H, True, L, dtype=torch.float32)
    for nb in (1, 2, 7):
        Pb, ob, obf = _batched(est, y, d, H, L, nb)
        assert torch.equal(Pb, P1), nb
        assert torch.equal(ob, o1) and torch.equal(obf, o1f), nb


def _enhancer(nets):
    import misonet_amd as mz
    m1, m3 = nets
    return mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)


def _recording(seed, L, mics=6):
    r = np.random.default_rng(seed)
    src = [(0.05 * r.standard_normal((L, mics))).astype(np.float32) for _ in range(2)]
    return src[0] + src[1]


@pytest.mark.parametrize("H", [1536, 2304])
def test_enhance_continuous_is_the_windowwise_composition(nets, H):
    from misonet_amd import stft as S
    enh = _enhancer(nets)
    W = 3072
    L = int(3.4 * W)
    rec = _recording(31, L)
    win = css_ref.windows(rec, W, H)                                   # [K, W, 6], host-cut
    X = enh.enhance_wav(torch.from_numpy(win).cuda(), None)            # [K, S, T, F]
    y = S.istft(X)                                                     # [K, S, W] float32
    P_ref, _, _, i16_ref = css_ref.continuous(X.cpu().numpy(), y.cpu().numpy(), H, L)
    first = enh.enhance_wav_int16(torch.from_numpy(win[:1]).cuda(), None)[0].cpu().numpy()
    runs = {}
    for mb in (1, 2, 16):
        got, P = enh.enhance_continuous(rec, window=W, hop=H, max_batch=mb, return_perms=True)
        runs[mb] = (got, P)
        assert got.shape == (2, L) and got.dtype == np.int16 and P.shape == (win.shape[0], 2)
        assert np.array_equal(P, P_ref), (mb, P, P_ref)
        d = np.abs(got.astype(np.int32) - i16_ref.astype(np.int32))
        assert d.max() <= 1, (mb, d.max())
        assert np.array_equal(got[:, :H], first[:, :H])              # window 0 alone: bit for bit
    for mb in (2, 16):
        assert np.array_equal(runs[mb][0], runs[1][0]) and np.array_equal(runs[mb][1], runs[1][1])


@pytest.mark.parametrize("L", [3072 - 100, 3072])
def test_single_window_equals_chunkwise(nets, L):
    enh = _enhancer(nets)
    rec = _recording(41, L)
    got = enh.enhance_continuous(rec, window=3072)
    want = enh.enhance_recording(rec, None, chunk_size=3072)
    assert got.shape == (2, L) and np.array_equal(got, want)


_ORACLE = {}


def _oracle_windows(sd1, sd3, win):
    """per window: MISO1 x M + shift alignment, MVDR x S, MISO3 x S on the CPU oracle, no clean alignment -> [K, S, T, F]"""
    from oracle import miso_oracle, mvdr_oracle, pipeline_oracle
    key = (win.shape, float(win.sum()))
    if key not in _ORACLE:
        outs = []
        for w in win:
            mix = pipeline_oracle.stft_chunk(w)                                  # [M, T, F]
            est, _ = pipeline_oracle.miso1_inference(mix, sd1, 0)                # [S, M, T, F]
            mix_bf = np.transpose(mix, (2, 0, 1))[None]
            mix_t = torch.as_tensor(mix)[None]
            o = []
            for s in range(est.shape[0]):
                b = mvdr_oracle.apply_beamforming(np.transpose(est[s], (2, 0, 1))[None], mix_bf, 1e-6)
                o.append(miso_oracle.miso3_forward(mix_t, torch.from_numpy(b)[:, None],
                                                   torch.from_numpy(est[s, 0])[None, None], sd3)[0, 0].numpy())
            outs.append(np.stack(o))
        _ORACLE[key] = np.stack(outs).astype(np.complex64)
    return _ORACLE[key]


def test_enhance_continuous_against_the_oracle(nets, sd1, sd3):
    from misonet_amd import stft as S
    enh = _enhancer(nets)
    W, H = 3072, 1536
    L = 3 * H + W - 80                                                 # K = 4
    rec = _recording(51, L)
    win = css_ref.windows(rec, W, H)
    assert win.shape[0] == 4
    Xo = _oracle_windows(sd1, sd3, win)
    yo = S.istft(torch.from_numpy(Xo)).numpy()                         # torch.istft on the host
    P_ref, D, _, i16_ref = css_ref.continuous(Xo, yo, H, L)
    for k in range(D.shape[0]):
        best, second = css_ref.margins(D[k])
        assert second > 1.01 * best, (f"window pair {k}/{k + 1}: the best permutation ({best:.6g}) is within 1 % of the "
                                      f"runner-up ({second:.6g}); the oracle comparison would hang on a near-tie")
    got, P = enh.enhance_continuous(rec, window=W, hop=H, max_batch=3, return_perms=True)
    assert np.array_equal(P, P_ref), (P, P_ref)
    d = np.abs(got.astype(np.int32) - i16_ref.astype(np.int32))
    print(f"[continuous vs oracle] max |diff| {d.max()} LSB, {float((d > 0).mean()):.2e} of the samples differ")
    assert d.max() <= 1


def test_files_and_inputs(nets, tmp_path):
    import misonet_amd as mz
    from misonet_amd import stft as S
    enh = _enhancer(nets)
    W, H = 3072, 1536
    L = 2 * W + 500
    rec12 = _recording(61, L, mics=12)
    got = enh.enhance_continuous(rec12, num_ch_utilize=6, window=W, hop=H, max_batch=2, save_path=str(tmp_path / "cont"))
    assert np.array_equal(got, enh.enhance_continuous(np.ascontiguousarray(rec12[:, ::2]), window=W, hop=H))
    for s in range(2):
        v, fs = S.read_wav_pcm24(str(tmp_path / f"cont_{s}.wav"))
        assert fs == 16000 and v.shape == (L, 1) and np.array_equal(v[:, 0], got[s].astype(np.int32) << 8)
        ref = tmp_path / f"ref_{s}.wav"
        S.write_wav_pcm24(str(ref), got[s], 16000)
        assert (tmp_path / f"cont_{s}.wav").read_bytes() == ref.read_bytes()
    for bad in (dict(hop=1535), dict(hop=2880), dict(hop=1500), dict(window=3000)):
        with pytest.raises(ValueError):
            enh.enhance_continuous(rec12, num_ch_utilize=6, **{**dict(window=W, hop=H), **bad})
    with pytest.raises(ValueError):
        enh.enhance_continuous(rec12, num_ch_utilize=4, window=W)    # [0:12:3] selects 4 microphones, the networks take 6
    sep = mz.Enhancer(nets[0], None, num_spks=2, ref_ch=0)
    with pytest.raises(RuntimeError):
        sep.enhance_continuous(rec12, num_ch_utilize=6, window=W)


def test_bench_geometry_and_memory(sd1, sd3):
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as Wt
    m1 = mz.MISO_1(2, 6, 7, list(Wt.DEFAULT_EN_CH), list(Wt.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(Wt.DEFAULT_EN_CH), list(Wt.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    m1.eval().set_precision("f32w")
    m3.eval().set_precision("f32w")
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    L = 30 * 16000 + 1234
    rec = _recording(71, L)
    a, P = enh.enhance_continuous(rec, max_batch=4, return_perms=True)
    b, P2 = enh.enhance_continuous(rec, max_batch=4, return_perms=True)
    assert a.shape == (2, L) and np.array_equal(a, b) and np.array_equal(P, P2)
    assert P.shape == (1 + -(-(L - 64000) // 32000), 2)
    assert all(sorted(p) == [0, 1] for p in P.tolist())
    rec120 = _recording(72, 120 * 16000)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    enh.enhance_continuous(rec, max_batch=4)
    p30 = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    enh.enhance_continuous(rec120, max_batch=4)
    p120 = torch.cuda.max_memory_allocated()
    print(f"[continuous] peak device memory at max_batch 4: 30 s {p30 / 2**20:.1f} MiB, 120 s {p120 / 2**20:.1f} MiB")
    assert p120 - p30 < 64 * 2**20
