"""Cost of scoring beside the pass: ``Enhancer.enhance_recordings`` over 64 synthetic recordings of 12 s (three 4 s chunks
each, coalesced across recordings), ``score`` off and on alternated in one process, host arrays in -> int16 (and Score) out.

    python tools/score_rate.py [--precision f32w bf16x6] [--recordings 64] [--seconds 12] [--rounds 3] [--max-batch 16]

Prints one JSON line: per arithmetic mode the x real time of every round of both arms, their medians and spread
(max - min over median), and ``on_over_off`` = the ratio of the medians.  ``score=False`` is the call the parent commit has:
for the "nothing existing changed" check run this tool on both trees, arms alternated (tools/gpu_ab_tree.sh does that for
bench.py).  For the share of the new kernels run it under ``rocprofv3 --kernel-trace --stats -- python
tools/score_rate.py --only on``: score_wave_k, score_wave_fold_k beside the pass's kernels.
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


def recordings(n, seconds, fs=16000, n_distinct=6):
    from misonet_amd.weights import synthetic_utterance
    distinct = [synthetic_utterance(500 + i, int(seconds * fs)) for i in range(n_distinct)]
    return [(distinct[i % n_distinct][0], [distinct[i % n_distinct][1], distinct[i % n_distinct][2]], f"r{i:03d}")
            for i in range(n)]


def measure(enh, recs, secs, max_batch, rounds, arms):
    import torch
    can_score = "score" in inspect.signature(enh.enhance_recordings).parameters     # the parent commit has no such argument
    fns = {"off": lambda: enh.enhance_recordings(recs, max_batch=max_batch)}
    if can_score:
        fns["on"] = lambda: enh.enhance_recordings(recs, max_batch=max_batch, score=True)
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
    if "on" in out and "off" in out:
        out["on_over_off"] = round(out["on"]["median"] / out["off"]["median"], 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", nargs="+", default=["f32w", "bf16x6"], choices=("bf16x6", "f32w", "f32"))
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--only", choices=("off", "on"), default=None, help="one arm (profiling runs)")
    a = ap.parse_args(argv)
    import torch
    from harness_rate import build_enhancer
    recs = recordings(a.recordings, a.seconds)
    line = {"metric": "score_rate", "device": torch.cuda.get_device_name(0), "recordings": a.recordings,
            "seconds_each": a.seconds, "fs": 16000, "mics": 6, "max_batch": a.max_batch, "rounds": a.rounds}
    for prec in a.precision:
        line[prec] = measure(build_enhancer(prec), recs, a.recordings * a.seconds, a.max_batch, a.rounds,
                             [a.only] if a.only else ["off", "on"])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
