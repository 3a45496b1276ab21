"""Throughput of continuous separation: ``Enhancer.enhance_continuous`` (windows at a hop of half a window, speaker tracking
across them, cross-fade stitch) on one synthetic long recording, beside the chunk-wise ``enhance_recording(wav, None)`` of
the same recording (independent 4 s chunks, no tracking), both host array in -> int16 out, in one process.

    python tools/css_rate.py [--precision f32w bf16x6] [--seconds 60] [--reps 3] [--max-batch 16]

Prints one JSON line: per arithmetic mode the x real time of both paths and ``continuous_over_chunkwise`` (every sample is
processed twice at a hop of half a window, so about 0.5 is expected).  Recording: ``--seconds`` of 6-microphone 16 kHz
synthetic audio (two 0.05 N(0, 1) sources, as ``weights.synthetic_utterance``), window 64000 samples.
For the share of the new kernels run it under ``rocprofv3 --kernel-trace --stats -- python tools/css_rate.py``:
css_stitch_k, css_chain_k and the pit_dist_k / pit_pick_k launches of the alignment beside the pass's kernels.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def recording(seconds, fs=16000, mics=6, seed=0):
    import numpy as np
    r = np.random.default_rng(seed)
    n = int(seconds * fs)
    return (0.05 * r.standard_normal((n, mics))).astype(np.float32) + (0.05 * r.standard_normal((n, mics))).astype(np.float32)


def measure(enh, rec, fs, max_batch, reps=3, window=64000):
    from harness_rate import _best
    secs = rec.shape[0] / fs
    out = {}
    for name, fn in (("continuous", lambda: enh.enhance_continuous(rec, window=window, max_batch=max_batch)),
                     ("chunkwise", lambda: enh.enhance_recording(rec, None, chunk_size=window, max_batch=max_batch))):
        fn()                                                                  # warm-up: workspaces, pinned slots
        t = _best(fn, reps)
        out[f"{name}_s"] = round(t, 4)
        out[f"{name}_x_realtime"] = round(secs / t, 2)
    out["continuous_over_chunkwise"] = round(out["continuous_x_realtime"] / out["chunkwise_x_realtime"], 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", nargs="+", default=["f32w", "bf16x6"], choices=("bf16x6", "f32w", "f32"))
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=16)
    a = ap.parse_args(argv)
    import torch
    from harness_rate import build_enhancer
    rec = recording(a.seconds)
    line = {"metric": "css_rate", "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "fs": 16000, "mics": 6,
            "window": 64000, "hop": 32000, "max_batch": a.max_batch}
    for prec in a.precision:
        line[prec] = measure(build_enhancer(prec), rec, 16000, a.max_batch, a.reps)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
