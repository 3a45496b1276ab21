"""GPU tests of the coalesced drop-ins (misonet_amd/coalesce.py): launches filled with chunks of several loader items give
the bits and the files of the item-by-item schedule, in every product mode, whatever max_batch is; the launch shape; the
wav-level twin; NaN reporting; and the rate of the harness path against the direct pass."""
import filecmp
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import nets, _need_gpu      # noqa: F401

pytestmark = pytest.mark.gpu

FRAMES = 48
CHUNK = (FRAMES - 1) * 64


def _spec(x):
    """host STFT of a [L, M] recording piece -> complex64 [M, T, F]"""
    from misonet_amd import stft as S
    return S.stft(torch.from_numpy(np.ascontiguousarray(x.T)))


def _item(us, n_split, gap, name):
    """one loader item: B = len(us) synthetic utterances of n_split splits, last split zero-padded by gap (per utterance)"""
    from misonet_amd import stft as S
    from misonet_amd.weights import synthetic_utterance
    od, d0, d1 = {}, {}, {}
    gaps = []
    per = []
    for b, u in enumerate(us):
        g = gap + 64 * b
        obs, s0, s1 = synthetic_utterance(u, n_split * CHUNK - g)
        parts = [S.split_chunks(x, CHUNK) for x in (obs, s0, s1)]
        assert parts[0][1] == g and len(parts[0][0]) == n_split
        per.append([[_spec(p) for p in pp[0]] for pp in parts])
        gaps.append(g)
    for k in range(n_split):
        od[str(k)] = torch.stack([p[0][k] for p in per])                  # [B, 6, T, F]
        d0[str(k)] = torch.stack([p[1][k] for p in per])
        d1[str(k)] = torch.stack([p[2][k] for p in per])
    names = [f"{name}b{b}" for b in range(len(us))]
    return od, d0, d1, gaps, names


def _loader():
    """12 items: 1-3 splits, B = 1 and B = 2, a non-zero gap on every one"""
    items, u = [], 100
    for i in range(12):
        B = 2 if i % 4 == 3 else 1
        items.append(_item(list(range(u, u + B)), 1 + (i * 7) % 3, 100 + 37 * i, f"it{i:02d}"))
        u += B
    return items


@pytest.fixture(scope="module")
def loader():
    _need_gpu()
    return _loader()


def _assert_same(a, b, da=None, db=None):
    assert list(a) == list(b)                                               # same names, same (loader) order
    for k in a:
        assert a[k].dtype == np.int16 and np.array_equal(a[k], b[k]), k
        if da is not None:
            for s in range(2):
                fa, fb = os.path.join(da, f"{k}_{s}.wav"), os.path.join(db, f"{k}_{s}.wav")
                assert filecmp.cmp(fa, fb, shallow=False), (fa, fb)


def test_inference_coalesced_equals_per_item(nets, loader, tmp_path):
    import misonet_amd as mz
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    ref_dir = str(tmp_path / "per_item")
    want = enh.inference(loader, ref_dir, coalesce=False)
    assert len(want) == 15
    for mb in (1, 4, 16):
        d = str(tmp_path / f"mb{mb}")
        got = enh.inference(iter(loader), d, max_batch=mb)
        _assert_same(got, want, d, ref_dir)


def test_golden_item_straddling_a_batch_boundary(nets, sd1, sd3, tmp_path):
    """the two-split item of test_gpu_parity.test_inference_loader_two_splits in the middle of a coalesced stream, its
    splits in two different launches: within 1 LSB of the oracle run split by split"""
    import misonet_amd as mz
    from misonet_amd import stft as S
    from misonet_amd.weights import synthetic_utterance
    from oracle import pipeline_oracle
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    chunk = 47 * 64
    obs, s0, s1 = synthetic_utterance(21, 2 * chunk - 500)
    parts = [S.split_chunks(x, chunk) for x in (obs, s0, s1)]
    gap = parts[0][1]
    od, d0, d1 = ({str(k): torch.from_numpy(pipeline_oracle.stft_chunk(p))[None] for k, p in enumerate(pp[0])}
                  for pp in parts)
    stream = [_item([5], 1, 64, "a"), _item([6], 3, 128, "b"), (od, d0, d1, [gap], ["rec"]), _item([7], 2, 0, "c")]
    res = enh.inference(stream, str(tmp_path), max_batch=5)               # rows 0-3: a, b; row 4: rec split 0 | rec split 1
    assert list(res) == ["ab0", "bb0", "rec", "cb0"]
    wav = res["rec"]
    assert wav.shape == (2, 2 * chunk - 500)
    ref = []
    for k in range(2):
        r = pipeline_oracle.enhance_utterance(od[str(k)][0].numpy(), np.stack([d0[str(k)][0, 0].numpy(),
                                              d1[str(k)][0, 0].numpy()]), sd1, sd3, ref_ch=0)
        ref.append([pipeline_oracle.istft_int16(r["out"][s]) for s in range(2)])
    for s in range(2):
        full = np.concatenate([ref[0][s], ref[1][s][: chunk - gap]])
        d = np.abs(wav[s].astype(np.int32) - full.astype(np.int32))
        print(f"[coalesced] straddling item spk{s}: max |diff| {d.max()} LSB vs the oracle")
        assert d.max() <= 1
        v, fs = S.read_wav_pcm24(str(tmp_path / f"rec_{s}.wav"))
        assert fs == 16000 and np.array_equal(v[:, 0], wav[s].astype(np.int32) << 8)


def test_launch_shape(nets, loader, tmp_path):
    """every launch but the last holds max_batch chunks (item by item, a launch holds one item's splits)"""
    import misonet_amd as mz
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    rows = []
    inner = enh.enhance

    def counting(mix, *a, **k):
        rows.append(int(mix.shape[0]))
        return inner(mix, *a, **k)

    enh.enhance = counting
    n_chunks = sum(len(it[0]) * len(it[4]) for it in loader)
    for mb in (4, 16):
        rows.clear()
        enh.inference(loader, str(tmp_path), write=False, max_batch=mb)
        assert sum(rows) == n_chunks
        assert rows[:-1] == [mb] * (len(rows) - 1) and 1 <= rows[-1] <= mb, rows


def test_tester_classes_coalesced_equal_per_item(nets, loader, tmp_path):
    from misonet_amd.tester import Tester_Beamforming, Tester_Enhance
    m1, m3 = nets
    args = dict(fs=16000, window="hann", length=256, overlap=192)
    tst = Tester_Enhance("SMS_WSJ", "MISO3", loader, loader, m1, m3, 6, 0, 2, CHUNK / 16000, str(tmp_path / "e"), 0, True,
                         **args)
    d_got, d_want = str(tmp_path / "e_got"), str(tmp_path / "e_want")
    _assert_same(tst.inference(loader, d_got), tst._enh.inference(loader, d_want, coalesce=False), d_got, d_want)
    for utt in (False, True):
        tb = Tester_Beamforming("SMS_WSJ", loader, loader, loader, m1, 6, 0, 2, CHUNK / 16000, str(tmp_path / "b"), 0, True,
                                False, utt, **args)
        want_dir = str(tmp_path / f"b{utt}_want")
        want = tb.inference(loader, want_dir, coalesce=False)
        for mb in (3, 16):
            d = str(tmp_path / f"b{utt}_{mb}")
            _assert_same(tb.inference(iter(loader), d, max_batch=mb), want, d, want_dir)
        assert tuple(tb.inference(loader, d, max_batch=4)) == tuple(want)     # the defaulted signature too


def test_enhance_recordings_equals_enhance_recording(nets, tmp_path):
    import misonet_amd as mz
    from misonet_amd.weights import synthetic_utterance
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    recs = []
    for u, L in ((31, CHUNK - 300), (32, 2 * CHUNK), (33, 3 * CHUNK + 700)):   # one chunk, an exact multiple, 3 + a tail
        obs, s0, s1 = synthetic_utterance(u, L)
        recs.append((obs, (s0, s1), f"r{u}"))
    for mb in (1, 2, 16):
        got = enh.enhance_recordings(iter(recs), chunk_size=CHUNK, max_batch=mb, save_path=str(tmp_path / f"mb{mb}"))
        assert list(got) == [r[2] for r in recs]
        for obs, cl, name in recs:
            want = enh.enhance_recording(obs, cl, chunk_size=CHUNK, max_batch=mb, save_path=str(tmp_path / "one" / name))
            assert got[name].shape == (2, obs.shape[0]) and np.array_equal(got[name], want), (mb, name)
            for s in range(2):
                assert filecmp.cmp(str(tmp_path / f"mb{mb}" / f"{name}_{s}.wav"), str(tmp_path / "one" / f"{name}_{s}.wav"),
                                   shallow=False)
    # without clean references, and mixed with and without (a flush between them)
    mixed = [(recs[0][0], None, "n0"), (recs[1][0], None, "n1"), recs[2]]
    got = enh.enhance_recordings(mixed, chunk_size=CHUNK, max_batch=4)
    for obs, cl, name in mixed:
        assert np.array_equal(got[name], enh.enhance_recording(obs, cl, chunk_size=CHUNK)), name


def test_nan_names_the_item(nets, loader, tmp_path):
    import misonet_amd as mz
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    od, d0, d1, gaps, names = loader[5]
    bad_obs = {k: v.clone() for k, v in od.items()}
    bad_obs["0"][0, 2, 10, 7] = float("nan")
    bad = (bad_obs, d0, d1, gaps, ["poisoned"] * len(names))
    stream = loader[:5] + [bad] + loader[6:]
    with pytest.raises(FloatingPointError, match="poisoned"):
        enh.inference(stream, str(tmp_path), write=False, max_batch=16)
    with pytest.raises(FloatingPointError, match="poisoned"):
        enh.inference(stream, str(tmp_path), write=False, max_batch=1)
    # the Enhancer stays usable, and the clean stream still gives the per-item bits
    _assert_same(enh.inference(loader[:4], str(tmp_path), write=False, max_batch=3),
                 enh.inference(loader[:4], str(tmp_path), write=False, coalesce=False))


def test_harness_rate_coalesced_vs_per_item_and_direct():
    """tools/harness_rate.py's loader (64 items, B = 1, 1-3 splits, bench geometry) in the headline mode: coalesced >= 1.2 x
    the item-by-item schedule and >= 0.85 x the direct enhance() rate at B = max_batch, all measured in this process"""
    _need_gpu()
    from tools import harness_rate as H
    enh = H.build_enhancer("bf16x6")
    items, n_chunks = H.synthetic_loader(64)
    r = H.measure(enh, items, n_chunks, 16, reps=2)
    print(f"[harness rate] {r}")
    assert r["coalesced_utt_s"] >= 1.2 * r["per_item_utt_s"], r
    assert r["coalesced_utt_s"] >= 0.85 * r["direct_utt_s"], r
