"""Cost of the online AuxIVA (``misonet_oiva``) at the bench geometry, beside the offline ``misonet_auxiva`` at K = M timed in the
same process.

    python tools/oiva_rate.py [--freq 129] [--warmup 3] [--iters 10] [--rounds 3] [--out profiles/oiva_rate.txt]

For M = 2 and M = 6 microphones (= sources), B = 1 and B = 16 recordings of ``--freq`` bins: one ``misonet_oiva`` call (est and
images) of T = 1, 16 and 501 frames on a stream that has already seen 501 frames (seeded random spectra resident on the device),
and one ``misonet_auxiva`` call (K = M channels and sources, 20 iterations) over the same 501 frames.  Per arm ``--rounds``
times: ``--warmup`` calls, then ``--iters`` single-call timings (HIP events on the caller's stream around the whole call); the
table has the minimum over everything and the median over the rounds of the per-round medians.  "ms per second of audio" is the
call's time times 250 / T (frames of 64 samples at 16 kHz).

The kernel reads and writes the whole state (W and V) in EVERY frame -- it does not fit the LDS -- so the last column is the time
T times the state, both ways, and the call's input and outputs take at the device-to-device copy bandwidth measured in this
process on a 256 MB buffer.  One workgroup walks an item: with B = 1 a single CU works.  Prints one JSON line and writes the table
to ``--out``.  No time is fixed anywhere: the file records what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAMES_PER_S = 250.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--freq", type=int, default=129)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oiva_rate.txt"))
    a = ap.parse_args()

    import torch
    from misonet_amd import _lib
    from misonet_amd.blind import SeparateStream, auxiva, bins_per_pass
    if not torch.cuda.is_available():
        raise SystemExit("oiva_rate needs the GPU: nothing is measured without one")
    F, TS, TL = a.freq, (1, 16, 501), 501
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    calls, nbytes, frames, keep = {}, {}, {}, []
    for M in (2, 6):
        for B in (1, 16):
            mix = torch.view_as_complex(torch.randn((B, M, TL, F, 2), device="cuda", generator=g)).contiguous()
            st = SeparateStream(M, F, B)
            st.process(mix)                                              # a stream in progress, not a cold start
            for T in TS:
                x = mix[:, :, :T].contiguous()
                est = torch.empty_like(x)
                img = torch.empty((B, M, M, T, F), dtype=torch.complex64, device="cuda")
                arm = f"oiva M {M} B {B} T {T}"
                calls[arm] = (lambda st=st, x=x, est=est, img=img: st.process_into(x, est, img) is None)
                nbytes[arm] = 2 * T * st.state.numel() + (2 + M) * x.numel() * 8
                frames[arm] = T
            bf = mix.permute(0, 3, 1, 2).contiguous()                    # [B, F, M, T], the offline call's layout
            arm = f"auxiva M {M} B {B} T {TL} (offline, K = M, 20 iterations)"
            calls[arm] = (lambda bf=bf, M=M: auxiva(bf, min(M, 4), iterations=20, channels=M) is None)
            frames[arm] = TL
            keep.append((mix, st, bf))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        e1.synchronize()
        if rc not in (0, None, False):
            raise RuntimeError(f"the library call failed: {L.misonet_last_error().decode()}")
        return e0.elapsed_time(e1)

    # the box's device-to-device copy bandwidth: read + written bytes per second
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy_ms = min(timed(lambda: dst.copy_(src) is None) for _ in range(8))
    copy_bw = 2.0 * src.numel() / (copy_ms * 1e-3)

    meds, mins = {arm: [] for arm in calls}, {arm: float("inf") for arm in calls}
    for _ in range(a.rounds):
        for arm, fn in calls.items():
            for _ in range(a.warmup):
                timed(fn)
            ms = [timed(fn) for _ in range(a.iters)]
            meds[arm].append(statistics.median(ms))
            mins[arm] = min(mins[arm], min(ms))
    res = {}
    for arm, v in meds.items():
        med = statistics.median(v)
        res[arm] = {"min_ms": round(mins[arm], 4), "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                    "ms_per_s_audio": round(med * FRAMES_PER_S / frames[arm], 4)}
        if arm in nbytes:
            res[arm]["bytes"] = nbytes[arm]
            res[arm]["copy_ms"] = round(nbytes[arm] / copy_bw * 1e3, 4)
    flags = [int(k[1].fail.max().item()) for k in keep]
    doc = {"metric": "oiva_rate", "device": torch.cuda.get_device_name(0), "F": F, "bins_per_pass": {M: bins_per_pass(M) for M in (2, 6)},
           "copy_GBps": round(copy_bw / 1e9, 1), "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "arms": res, "flags": flags}
    lines = [f"online AuxIVA at F {F}, alpha 0.98, gauss, est and images written, on {doc['device']}; one workgroup per item, "
             f"{bins_per_pass(2)} bins per pass at M 2 and {bins_per_pass(6)} at M 6",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events around the whole call); min over all timings, median over the rounds of the per-round medians, "
             "spread = (max - min) / median over the rounds; ms per second of audio = median x 250 / T (16 kHz, hop 64)",
             f"device-to-device copy of 256 MB in this process: {copy_ms:.3f} ms = {copy_bw / 1e9:.0f} GB/s read + written; "
             "state+io = T x the state both ways + the input + est + images", "",
             f"{'arm':<58} {'min ms':>10} {'median ms':>10} {'spread':>8} {'ms / s audio':>13} {'state+io MB':>12} {'at copy bw ms':>14}"]
    for arm, r in res.items():
        tail = f" {r['bytes'] / 1e6:>12.2f} {r['copy_ms']:>14.4f}" if "bytes" in r else ""
        lines.append(f"{arm:<58} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f} {r['ms_per_s_audio']:>13.4f}{tail}")
    lines += ["", f"fail words after the runs (random spectra, not speech): {flags}",
              "the offline call sees the whole recording, reduces it by a PCA and iterates twenty times (at M 6 it returns 4 of the "
              "6 rows: the call's limit); the recursion is causal, keeps its state between calls and takes the same memory however "
              "long the stream: it is not a better separator", "a first version, not tuned"]
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
