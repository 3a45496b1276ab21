"""Cost of cepstral distance, LLR and fwSegSNR: beside the pass and on its own.

    python tools/reverb_rate.py [--precision bf16x6] [--recordings 64] [--seconds 12] [--rounds 3] [--max-batch 16]
                                [--only score|reverb|standalone] [--out profiles/reverb_rate.txt]

``Enhancer.enhance_recordings`` over 64 synthetic recordings of 12 s, ``score=True`` and ``score=True, reverb=True`` alternated
in one process (arms "score" and "reverb"); then ``score.reverb_block`` alone (S = 2, L = 192000, fs = 16000, device arrays in,
one host row per recording out) at B = 1 and B = 16, in milliseconds per recording.  Prints the table and one JSON line;
``--out`` also writes the table.  No rate is fixed in advance: the ratio is a cost report, not a pass criterion.  ``score=True``
is a call the parent commit has: for the "nothing existing changed" check run ``--only score`` on both trees, processes
alternated.  For the share of the new kernels run it under ``rocprofv3 --kernel-trace --stats -- python tools/reverb_rate.py
--only reverb``: rvb_level_k, rvb_frame_k, rvb_pair_k beside the pass's kernels.
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
    if "reverb" in inspect.signature(enh.enhance_recordings).parameters:       # the parent commit has no such argument
        fns["reverb"] = lambda: enh.enhance_recordings(recs, max_batch=max_batch, score=True, reverb=True)
    arms = [a for a in arms if a in fns]
    for a in arms:
        fns[a]()                                                           # warm-up: workspaces, pinned slots, the table
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
    if "reverb" in out and "score" in out:
        out["reverb_over_score"] = round(out["reverb"]["median"] / out["score"]["median"], 4)
    return out


def standalone(rounds, L=192000, S=2, fs=16000):
    """ms per recording of level + frames + pairs + the D2H of the row, inputs already on the device; B = 16 as one batch and
    as sixteen calls of one"""
    import numpy as np
    import torch
    from misonet_amd import score
    rng = np.random.default_rng(0)
    ref = torch.from_numpy((0.1 * rng.standard_normal((16, S, L))).astype(np.float32)).cuda()
    est = (ref * 0.7 + 0.02 * torch.randn_like(ref)).mul(32767.0).round().to(torch.int16)
    mix = ref.sum(1, keepdim=True)

    def batched():
        score.reverb_block(est, ref, mix, None, fs).cpu()

    def one_by_one():
        for b in range(16):
            score.reverb_block(est[b:b + 1], ref[b:b + 1], mix[b:b + 1], None, fs).cpu()

    out = {}
    for name, fn in (("batched_B16", batched), ("one_by_one", one_by_one)):
        fn()
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(round(1e3 * (time.perf_counter() - t0) / 16, 3))
        out[f"{name}_ms_per_recording"] = ms
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", nargs="+", default=["bf16x6"], choices=("bf16x6", "f32w", "f32"))
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--only", choices=("score", "reverb", "standalone"), default=None, help="one arm (profiling, parent tree)")
    ap.add_argument("--out", default=None, help="write the table here (profiles/reverb_rate.txt)")
    a = ap.parse_args(argv)
    import torch
    from harness_rate import build_enhancer
    from score_rate import recordings
    line = {"metric": "reverb_rate", "device": torch.cuda.get_device_name(0), "recordings": a.recordings,
            "seconds_each": a.seconds, "fs": 16000, "mics": 6, "max_batch": a.max_batch, "rounds": a.rounds}
    text = [f"reverb_rate: {a.recordings} recordings of {a.seconds:g} s, 16 kHz, 6 microphones, max_batch {a.max_batch}, "
            f"{line['device']}", f"wall clock, one warm-up, {a.rounds} rounds alternated in one process", ""]
    if a.only != "standalone":
        recs = recordings(a.recordings, a.seconds)
        for prec in a.precision:
            m = line[prec] = measure(build_enhancer(prec), recs, a.recordings * a.seconds, a.max_batch, a.rounds,
                                     [a.only] if a.only else ["score", "reverb"])
            for arm in ("score", "reverb"):
                if arm in m:
                    text.append(f"{prec:8s} {arm:8s} {m[arm]['median']:9.2f} x real time   {m[arm]['x_realtime']}")
            if "reverb_over_score" in m:
                text.append(f"{prec:8s} reverb=True / score=True alone = {m['reverb_over_score']:.4f}")
    if a.only in (None, "standalone"):
        s = line["standalone"] = standalone(a.rounds)
        text += ["", "score.reverb_block alone, S = 2, 12 s at 16 kHz, the mixture included, ms per recording:"]
        for k, v in s.items():
            text.append(f"  {k:32s} {statistics.median(v):8.3f}   {v}")
    text = "\n".join(text) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
