"""Cost of the online WPE (``misonet_owpe``) at the bench geometry, beside the offline ``misonet_wpe`` at the same taps timed in
the same process.

    python tools/owpe_rate.py [--freq 129] [--mics 6] [--taps 10] [--delay 3] [--warmup 3] [--iters 10] [--rounds 3]
                              [--out profiles/owpe_rate.txt]

For B = 1 and B = 16 recordings of ``--mics`` microphones and ``--freq`` bins: one ``misonet_owpe`` call of T = 1, 16 and 501
frames on a stream that has already seen 501 frames (seeded random spectra resident on the device), and one ``misonet_wpe`` call
(3 iterations) over the same 501 frames.  Per arm ``--rounds`` times: ``--warmup`` calls, then ``--iters`` single-call timings
(HIP events on the caller's stream around the whole call); the table has the minimum over everything and the median over the
rounds of the per-round medians.  "ms per second of audio" is the call's time times 250 / T (frames of 64 samples at 16 kHz).

Every call reads and writes the whole state (P, G and the rings go to LDS once and come back once): the last column is the time
those bytes, and the call's input and output, take at the device-to-device copy bandwidth measured in this process on a 256 MB
buffer -- the floor of a call, which T = 1 sits nearest to.  Prints one JSON line and writes the table to ``--out``.  No time is
fixed anywhere: the file records what was measured."""
import argparse
import ctypes as C
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
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--taps", type=int, default=10)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "owpe_rate.txt"))
    a = ap.parse_args()

    import torch
    from misonet_amd import _lib
    from misonet_amd.dereverb import Dereverb, DereverbStream, _wpe_device
    if not torch.cuda.is_available():
        raise SystemExit("owpe_rate needs the GPU: nothing is measured without one")
    F, M, TS, TL = a.freq, a.mics, (1, 16, 501), 501
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    calls, nbytes, frames, keep = {}, {}, {}, []
    for B in (1, 16):
        mix = torch.view_as_complex(torch.randn((B, M, TL, F, 2), device="cuda", generator=g)).contiguous()
        st = DereverbStream(M, F, B, taps=a.taps, delay=a.delay)
        st.process(mix)                                                  # a stream in progress, not a cold start
        for T in TS:
            x = mix[:, :, :T].contiguous()
            y = torch.empty_like(x)
            keep.append((x, y))
            arm = f"owpe B {B} T {T}"
            calls[arm] = (lambda st=st, x=x, y=y: st.process_into(x, y) is None)
            nbytes[arm] = 2 * st.state.numel() + 2 * x.numel() * 8
            frames[arm] = T
        wopts = Dereverb(taps=a.taps, delay=a.delay).c_opts()
        arm = f"wpe B {B} T {TL} (offline, 3 iterations)"
        calls[arm] = (lambda mix=mix, o=wopts: _wpe_device(mix, None, o, False) is None)
        frames[arm] = TL
        keep.append((mix, st))

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
    flags = [int(k[1].fail.max().item()) for k in keep if isinstance(k[1], DereverbStream)]
    lds = L.misonet_owpe_lds_bytes(M, C.byref(keep[-1][1]._c))
    doc = {"metric": "owpe_rate", "device": torch.cuda.get_device_name(0), "F": F, "M": M, "taps": a.taps, "delay": a.delay,
           "lds_bytes": lds, "copy_GBps": round(copy_bw / 1e9, 1), "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "arms": res, "flags": flags}
    lines = [f"online WPE at F {F}, M {M}, taps {a.taps} (N = {M * a.taps}), delay {a.delay}, alpha 0.999, context 0 on {doc['device']}; "
             f"one workgroup of 512 threads per bin, {lds} bytes of LDS each",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events around the whole call); min over all timings, median over the rounds of the per-round medians, "
             "spread = (max - min) / median over the rounds; ms per second of audio = median x 250 / T (16 kHz, hop 64)",
             f"device-to-device copy of 256 MB in this process: {copy_ms:.3f} ms = {copy_bw / 1e9:.0f} GB/s read + written", "",
             f"{'arm':<40} {'min ms':>10} {'median ms':>10} {'spread':>8} {'ms / s audio':>13} {'state+io MB':>12} {'at copy bw ms':>14}"]
    for arm, r in res.items():
        tail = f" {r['bytes'] / 1e6:>12.2f} {r['copy_ms']:>14.4f}" if "bytes" in r else ""
        lines.append(f"{arm:<40} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f} {r['ms_per_s_audio']:>13.4f}{tail}")
    lines += ["", "the offline filter sees the whole recording and iterates three times; the recursion is causal, keeps its state between "
              "calls and takes the same memory however long the stream: it is not a better filter", "a first version, not tuned"]
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
