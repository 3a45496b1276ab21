"""Cost of STOI / ESTOI: beside the pass and on its own.

    python tools/stoi_rate.py [--precision bf16x6] [--recordings 64] [--seconds 12] [--rounds 3] [--max-batch 16]
                              [--only score|stoi|standalone]

``Enhancer.enhance_recordings`` over 64 synthetic recordings of 12 s, ``score=True`` and ``score=True, stoi=True`` alternated
in one process (arms "score" and "stoi"); then ``score.stoi_block`` alone (S = 2, L = 192000, fs = 16000, device arrays in,
one host row per recording out) at B = 1 and B = 16, in milliseconds per recording.  Prints one JSON line.  ``score=True`` is
a call the parent commit has: for the "nothing existing changed" check run ``--only score`` on both trees, processes
alternated.  For the share of the new kernels run it under ``rocprofv3 --kernel-trace --stats -- python tools/stoi_rate.py
--only stoi``: stoi_resample_k, stoi_band_k, stoi_seg_k, ... beside the pass's kernels.
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(enh, recs, secs, max_batch, rounds, arms):
    import torch
    fns = {"score": lambda: enh.enhance_recordings(recs, max_batch=max_batch, score=True)}
    if "stoi" in inspect.signature(enh.enhance_recordings).parameters:         # the parent commit has no such argument
        fns["stoi"] = lambda: enh.enhance_recordings(recs, max_batch=max_batch, score=True, stoi=True)
    arms = [a for a in arms if a in fns]
    for a in arms:
        fns[a]()                                                           # warm-up: workspaces, pinned slots
    xs = {a: [] for a in arms}
    for _ in range(rounds):
        for a in arms:                                                     # alternated: drift hits both arms alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[a]()
            torch.cuda.synchronize()
            xs[a].append(round(secs / (time.perf_counter() - t0), 2))
    out = {}
    for a in arms:
        med = statistics.median(xs[a])
        out[a] = {"x_realtime": xs[a], "median": med, "spread": round((max(xs[a]) - min(xs[a])) / med, 4)}
    if "stoi" in out and "score" in out:
        out["stoi_over_score"] = round(out["stoi"]["median"] / out["score"]["median"], 4)
    return out


def standalone(rounds, L=192000, S=2, fs=16000):
    """ms per recording of resampler + mask + bands + segments + the D2H of the row, inputs already on the device"""
    import numpy as np
    import torch
    from misonet_amd import score
    rng = np.random.default_rng(0)
    out = {}
    for B in (1, 16):
        ref = torch.from_numpy((0.1 * rng.standard_normal((B, S, L))).astype(np.float32)).cuda()
        est = (ref * 0.7 + 0.02 * torch.randn_like(ref)).mul(32767.0).round().to(torch.int16)
        mix = ref.sum(1, keepdim=True)
        score.stoi_block(est, ref, mix, None, fs).cpu()
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score.stoi_block(est, ref, mix, None, fs).cpu()
            ms.append(round(1e3 * (time.perf_counter() - t0) / B, 3))
        out[f"B{B}_ms_per_recording"] = ms
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", nargs="+", default=["bf16x6"], choices=("bf16x6", "f32w", "f32"))
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--only", choices=("score", "stoi", "standalone"), default=None, help="one arm (profiling, parent tree)")
    a = ap.parse_args(argv)
    import torch
    from harness_rate import build_enhancer
    from score_rate import recordings
    line = {"metric": "stoi_rate", "device": torch.cuda.get_device_name(0), "recordings": a.recordings,
            "seconds_each": a.seconds, "fs": 16000, "mics": 6, "max_batch": a.max_batch, "rounds": a.rounds}
    if a.only != "standalone":
        recs = recordings(a.recordings, a.seconds)
        for prec in a.precision:
            line[prec] = measure(build_enhancer(prec), recs, a.recordings * a.seconds, a.max_batch, a.rounds,
                                 [a.only] if a.only else ["score", "stoi"])
    if a.only in (None, "standalone"):
        line["standalone"] = standalone(a.rounds)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
