"""Throughput of the drop-in harness path: ``Enhancer.inference`` over a loader shaped like the reference's
(``batch_size: 1``, one to three 4 s splits per item, host-resident STFT dicts), coalesced and item by item, against the
direct ``enhance()`` rate at B = ``max_batch`` on device-resident inputs, all in one process.

    python tools/harness_rate.py [--precision bf16x6] [--items 64] [--reps 3] [--max-batch 16 32]

Prints one JSON line: per ``max_batch`` the utterances (4 s chunks) per second of each schedule and
``coalesced_over_direct``.  Bench geometry: 6 microphones, T = 1001 frames, F = 129, ``weights.synthetic_utterance``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_enhancer(precision="bf16x6", device=0):
    import misonet_amd as mz
    from misonet_amd import weights as W
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(device)
    m1.load_state_dict(W.make_state_dict(W.miso1_spec(), 0))
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(device)
    m3.load_state_dict(W.make_state_dict(W.miso3_spec(), 1))
    m1.eval().set_precision(precision)
    m3.eval().set_precision(precision)
    return mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)


def synthetic_loader(n_items=64, frames=1001, n_distinct=6):
    """``n_items`` loader items ``(obs_dict, s0_dict, s1_dict, gap, [name])`` with B = 1 and 1, 2, 3, 1, ... splits; dict
    values complex64 [1, 6, T, 129] on the host (STFT on the host).  The splits cycle through ``n_distinct`` synthetic
    utterances, so host memory stays small whatever ``n_items`` is.  Returns (items, number of chunks)."""
    import torch
    from misonet_amd import stft as S
    from misonet_amd.weights import synthetic_utterance
    pool = []
    for u in range(n_distinct):
        obs, s0, s1 = synthetic_utterance(u, (frames - 1) * S.HOP)                        # [L, 6] each
        pool.append(tuple(S.stft(torch.from_numpy(x.T.copy()))[None].contiguous() for x in (obs, s0, s1)))
    items, n_chunks = [], 0
    for i in range(n_items):
        k = 1 + i % 3
        sel = [pool[(i + j) % n_distinct] for j in range(k)]
        items.append(({str(j): p[0] for j, p in enumerate(sel)}, {str(j): p[1] for j, p in enumerate(sel)},
                      {str(j): p[2] for j, p in enumerate(sel)}, [0], [f"utt{i:03d}"]))
        n_chunks += k
    return items, n_chunks


def _best(fn, reps):
    import torch
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def measure(enh, items, n_chunks, max_batch, reps=3, direct_iters=8):
    """utt/s of the coalesced and the per-item ``inference`` over ``items`` and of ``enhance()`` at B = ``max_batch``
    (best of ``reps`` after one warm-up each)"""
    import tempfile
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        def coalesced():
            enh.inference(items, tmp, write=False, max_batch=max_batch)

        def per_item():
            enh.inference(items, tmp, write=False, max_batch=max_batch, coalesce=False)

        obs, s0, s1 = items[0][0]["0"][0], items[0][1]["0"][0, 0], items[0][2]["0"][0, 0]
        mix = obs[None].expand(max_batch, -1, -1, -1).contiguous().cuda()
        clean = torch.stack((s0, s1))[None].expand(max_batch, -1, -1, -1).contiguous().cuda()

        def direct():
            for _ in range(direct_iters):
                enh.enhance(mix, clean, check_nan=False)

        out = {}
        for name, fn, n in (("coalesced", coalesced, n_chunks), ("per_item", per_item, n_chunks),
                            ("direct", direct, direct_iters * max_batch)):
            fn()                                                                      # warm-up: workspaces, pinned slots
            out[f"{name}_utt_s"] = round(n / _best(fn, reps), 2)
    out["coalesced_over_direct"] = round(out["coalesced_utt_s"] / out["direct_utt_s"], 4)
    out["coalesced_over_per_item"] = round(out["coalesced_utt_s"] / out["per_item_utt_s"], 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", default="bf16x6", choices=("bf16x6", "f32w", "f32"))
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-batch", type=int, nargs="+", default=[16, 32])
    a = ap.parse_args(argv)
    import torch
    enh = build_enhancer(a.precision)
    items, n_chunks = synthetic_loader(a.items)
    line = {"metric": "harness_rate", "dtype": a.precision, "device": torch.cuda.get_device_name(0),
            "items": a.items, "chunks": n_chunks, "frames": 1001, "mics": 6}
    for mb in a.max_batch:
        line[f"max_batch_{mb}"] = dict(max_batch=mb, **measure(enh, items, n_chunks, mb, a.reps))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
