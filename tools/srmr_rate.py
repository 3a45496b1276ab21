"""Cost of SRMR: beside the continuous pass and on its own.

    python tools/srmr_rate.py [--precision bf16x6] [--seconds 60] [--rounds 3] [--max-batch 16]
                              [--only plain|srmr|standalone] [--out profiles/srmr_rate.txt]

``Enhancer.enhance_continuous`` over one synthetic recording of 60 s, ``srmr=False`` and ``srmr=True`` alternated in one process
(arms "plain" and "srmr"); then ``score.srmr_block`` alone (S = 2 and the mixture, L = 192000, fs = 16000, device arrays in, one
host row per recording out) over 64 recordings as one batch and one by one, in milliseconds per recording.  Prints the table and
one JSON line; ``--out`` also writes the table.  No rate is fixed in advance: this is a cost report, not a pass criterion.
``srmr=False`` is a call the parent commit has: for the "nothing existing changed" check run ``--only plain`` on both trees,
processes alternated.
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


def measure(enh, rec, secs, max_batch, rounds, arms):
    import torch
    fns = {"plain": lambda: enh.enhance_continuous(rec, max_batch=max_batch)}
    if "srmr" in inspect.signature(enh.enhance_continuous).parameters:        # the parent commit has no such argument
        fns["srmr"] = lambda: enh.enhance_continuous(rec, max_batch=max_batch, srmr=True)
    arms = [a for a in arms if a in fns]
    for a in arms:
        fns[a]()                                                            # warm-up: workspaces, the table
    xs = {a: [] for a in arms}
    for _ in range(rounds):
        for a in arms:                                                      # alternated: drift hits both arms alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[a]()
            torch.cuda.synchronize()
            xs[a].append(round(secs / (time.perf_counter() - t0), 2))
    out = {}
    for a in arms:
        med = statistics.median(xs[a])
        out[a] = {"x_realtime": xs[a], "median": med, "spread": round((max(xs[a]) - min(xs[a])) / med, 4)}
    if "srmr" in out and "plain" in out:
        out["srmr_over_plain"] = round(out["srmr"]["median"] / out["plain"]["median"], 4)
    return out


def standalone(rounds, B=64, L=192000, S=2, fs=16000):
    """ms per recording of the whole measurement + the D2H of the row, inputs already on the device; B recordings as one batch
    and as B calls of one"""
    import numpy as np
    import torch
    from misonet_amd import score
    rng = np.random.default_rng(0)
    sig = torch.from_numpy((0.1 * rng.standard_normal((B, S, L))).astype(np.float32)).cuda()
    mix = sig.sum(1, keepdim=True)
    sig = sig.mul(32767.0).round().to(torch.int16)

    def batched():
        score.srmr_block(sig, mix, None, fs).cpu()

    def one_by_one():
        for b in range(B):
            score.srmr_block(sig[b:b + 1], mix[b:b + 1], None, fs).cpu()

    out = {}
    for name, fn in ((f"batched_B{B}", batched), ("one_by_one", one_by_one)):
        fn()
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(round(1e3 * (time.perf_counter() - t0) / B, 3))
        out[f"{name}_ms_per_recording"] = ms
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", nargs="+", default=["bf16x6"], choices=("bf16x6", "f32w", "f32"))
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--only", choices=("plain", "srmr", "standalone"), default=None, help="one arm (profiling, parent tree)")
    ap.add_argument("--out", default=None, help="write the table here (profiles/srmr_rate.txt)")
    a = ap.parse_args(argv)
    import torch
    from harness_rate import build_enhancer
    from score_rate import recordings
    line = {"metric": "srmr_rate", "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "fs": 16000, "mics": 6,
            "max_batch": a.max_batch, "rounds": a.rounds}
    text = [f"srmr_rate: one recording of {a.seconds:g} s through enhance_continuous, 16 kHz, 6 microphones, max_batch "
            f"{a.max_batch}, {line['device']}", f"wall clock, one warm-up, {a.rounds} rounds alternated in one process", ""]
    if a.only != "standalone":
        rec = recordings(1, a.seconds)[0][0]
        for prec in a.precision:
            m = line[prec] = measure(build_enhancer(prec), rec, a.seconds, a.max_batch, a.rounds,
                                     [a.only] if a.only else ["plain", "srmr"])
            for arm in ("plain", "srmr"):
                if arm in m:
                    text.append(f"{prec:8s} {arm:8s} {m[arm]['median']:9.2f} x real time   {m[arm]['x_realtime']}")
            if "srmr_over_plain" in m:
                text.append(f"{prec:8s} srmr=True / srmr=False = {m['srmr_over_plain']:.4f}")
    if a.only in (None, "standalone"):
        s = line["standalone"] = standalone(a.rounds)
        text += ["", "score.srmr_block alone, 64 recordings, S = 2 and the mixture, 12 s at 16 kHz, ms per recording:"]
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
