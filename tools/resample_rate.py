"""Cost of the polyphase resampler (``misonet_resample``) alone, beside two yardsticks measured on the same box.

    python tools/resample_rate.py [--seconds 60] [--mics 6] [--warmup 3] [--iters 10] [--rounds 3] [--no-pipeline]
                                  [--out profiles/resample_rate.txt]

For a recording of ``--seconds`` x ``--mics`` channels, float32, time-major and device-resident, at 48 -> 16, 44.1 -> 16, 16 -> 8
and 16 -> 48 kHz, in this one process:

  resample          the call into a buffer of the caller's (``resample_into``): one launch
  the floor         the bytes the call must move -- the input read once, the output written once -- at the copy bandwidth
                    measured here: a device-to-device copy of 1 GiB, read + write counted, the best of its timings
  resample_poly     ``scipy.signal.resample_poly`` of the same float32 array on the host (wall clock, best of 3): what a user
                    without this call would run, serially in front of the device work.  The error column is against
                    resample_poly of the array in float64, beside e0, the error of rounding that answer to float32

and, unless ``--no-pipeline``, ``Enhancer.enhance_continuous`` on seed weights over the same recording at 16 kHz and with
``fs_in=48000`` from the 48 kHz recording (wall clock, host copies included, the median of 3 after one warm-up).

Per arm ``--rounds`` times: ``--warmup`` calls, then ``--iters`` single-call timings (HIP events on the caller's stream); the
table has the minimum over everything and the median over the rounds of the per-round medians.  Prints one JSON line and writes
the table to ``--out``.  No time is fixed anywhere: the file records what was measured.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RATES = ((48000, 16000), (44100, 16000), (16000, 8000), (16000, 48000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_rate.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from scipy.signal import resample_poly
    import misonet_amd as mz
    from misonet_amd import resample as RS
    M = a.mics
    g = torch.Generator(device="cuda")
    g.manual_seed(11)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the copy bandwidth of this box, in this process: 1 GiB device to device, read + write counted
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(a.warmup):
        dst.copy_(src)
    copy_ms = min(timed(lambda: dst.copy_(src)) for _ in range(a.iters))
    gbps = 2 * src.numel() / copy_ms / 1e6
    del src, dst

    arms = {}
    for fs_in, fs_out in RATES:
        n = int(round(a.seconds * fs_in))
        x = (torch.randn((1, n, M), generator=g, device="cuda") * 0.1).contiguous()
        y = torch.empty((1, RS.resampled_len(n, fs_in, fs_out), M), dtype=torch.float32, device="cuda")
        RS.resample_into(x, y, None, fs_in, fs_out)                    # builds the taps of this ratio
        meds, best = [], float("inf")
        for _ in range(a.rounds):
            for _ in range(a.warmup):
                RS.resample_into(x, y, None, fs_in, fs_out)
            ms = [timed(lambda: RS.resample_into(x, y, None, fs_in, fs_out)) for _ in range(a.iters)]
            meds.append(statistics.median(ms))
            best = min(best, min(ms))
        host = x[0].cpu().numpy()
        p, q = RS.ratio(fs_in, fs_out)
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = resample_poly(host, p, q, axis=0)
            cpu.append((time.perf_counter() - t0) * 1e3)
        ref = resample_poly(host.astype(np.float64), p, q, axis=0)     # the float64 oracle (SciPy filters float32 in float32)
        err = float(np.linalg.norm(y[0].cpu().numpy().astype(np.float64) - ref) / np.linalg.norm(ref))
        e0 = float(np.linalg.norm(ref.astype(np.float32).astype(np.float64) - ref) / np.linalg.norm(ref))
        traffic = (x.numel() + y.numel()) * 4
        arms[f"{fs_in} -> {fs_out}"] = {
            "p": p, "q": q, "taps_per_output": (2 * 10 * max(p, q)) // p + 1, "samples_in": n, "samples_out": int(y.shape[1]),
            "min_ms": round(best, 4), "median_ms": round(statistics.median(meds), 4),
            "spread": round((max(meds) - min(meds)) / statistics.median(meds), 4), "traffic_bytes": traffic,
            "floor_ms": round(traffic / gbps / 1e6, 4), "resample_poly_ms": round(min(cpu), 2), "rel_l2_vs_resample_poly_f64": err,
            "e0": e0}
        del x, y

    pipe = None
    if not a.no_pipeline:
        from misonet_amd import weights as W
        m1 = mz.MISO_1(2, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m1.load_state_dict(W.make_state_dict(W.miso1_spec(), 0))
        m3 = mz.MISO_3(1, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m3.load_state_dict(W.make_state_dict(W.miso3_spec(), 1))
        enh = mz.Enhancer(m1.eval(), m3.eval(), num_spks=2, ref_ch=0)
        n16 = int(round(a.seconds * 16000))
        rec16 = W.synthetic_utterance(5, n16)[0].astype(np.float32)
        rec48 = RS.resample(rec16, 16000, 48000)

        def wall(fn):
            fn()
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts)
        pipe = {"enhance_continuous_ms": round(wall(lambda: enh.enhance_continuous(rec16, fs=16000)), 2),
                "enhance_continuous_fs_in_48000_ms": round(wall(lambda: enh.enhance_continuous(rec48, fs=16000, fs_in=48000)), 2)}
        t0 = time.perf_counter()
        resample_poly(rec48, 1, 3, axis=0)
        pipe["resample_poly_48_to_16_ms"] = round((time.perf_counter() - t0) * 1e3, 2)

    doc = {"metric": "resample_rate", "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "M": M, "warmup": a.warmup,
           "iters": a.iters, "rounds": a.rounds, "copy_gb_per_s": round(gbps, 1), "tile": RS.tile(), "arms": arms, "pipeline": pipe}
    print(json.dumps(doc))
    lines = [f"polyphase resampler (misonet_resample) on {a.seconds:g} s x {M} channels, float32 time-major, on {doc['device']}: one "
             f"launch, {RS.tile()} output samples x {M} channels per workgroup",
             f"{a.rounds} rounds in one process; per round {a.warmup} warm-up calls, then {a.iters} single-call timings (HIP events); "
             "min over all timings, median over the rounds of the per-round medians, spread = (max - min) / median over the rounds",
             f"copy bandwidth measured here (1 GiB device to device, read + write, best of {a.iters}): {gbps:.0f} GB/s",
             "the floor = the input read once and the output written once at that bandwidth; resample_poly = SciPy on the host, "
             "same float32 array, wall clock, best of 3; rel-L2 = the result against resample_poly of the array in float64, e0 = that "
             "float64 answer rounded to float32 against itself", "",
             f"{'rates':<16} {'p/q':>8} {'taps/out':>8} {'min ms':>9} {'median ms':>10} {'spread':>7} {'MB':>7} {'floor ms':>9} "
             f"{'x floor':>8} {'SciPy ms':>9} {'x SciPy':>8} {'rel-L2':>9} {'e0':>9}"]
    for k, r in arms.items():
        lines.append(f"{k:<16} {str(r['p']) + '/' + str(r['q']):>8} {r['taps_per_output']:>8} {r['min_ms']:>9.4f} "
                     f"{r['median_ms']:>10.4f} {r['spread']:>7.4f} {r['traffic_bytes'] / 1e6:>7.1f} {r['floor_ms']:>9.4f} "
                     f"{r['min_ms'] / r['floor_ms']:>8.1f} {r['resample_poly_ms']:>9.2f} "
                     f"{r['resample_poly_ms'] / r['min_ms']:>8.0f} {r['rel_l2_vs_resample_poly_f64']:>9.2e} {r['e0']:>9.2e}")
    if pipe is not None:
        lines += ["", f"Enhancer.enhance_continuous, seed weights, {a.seconds:g} s x {M} channels, wall clock with host copies, median of "
                  f"3: {pipe['enhance_continuous_ms']:.1f} ms at 16 kHz; {pipe['enhance_continuous_fs_in_48000_ms']:.1f} ms from the 48 kHz "
                  f"recording with fs_in=48000 (resampled on the device, one copy back to the host for the window cutting); "
                  f"resample_poly of that recording on the host alone: {pipe['resample_poly_48_to_16_ms']:.1f} ms"]
    lines += ["a first version, not tuned"]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
