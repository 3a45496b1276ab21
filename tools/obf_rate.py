"""Cost of the online beamformer (``misonet_obf``) at the bench geometry, beside the offline Souden beamformer over the same frames
and the online AuxIVA (``misonet_oiva``) at the same M, timed in the same process.

    python tools/obf_rate.py [--freq 129] [--warmup 3] [--iters 10] [--rounds 3] [--out profiles/obf_rate.txt]

For M = S = 2 and M = S = 6 (microphones = sources), B = 1 and B = 16 recordings of ``--freq`` bins: one ``misonet_obf`` call of
T = 1, 16 and 501 frames on a stream that has already seen 501 frames (seeded random spectra resident on the device; the images
are random as well and do not sum to the mixture), S offline ``Apply_Beamforming(beamformer="souden")`` calls over the same 501
frames, and one ``misonet_oiva`` call (est and images) of 501 frames.  Per arm ``--rounds`` times: ``--warmup`` calls, then
``--iters`` single-call timings (HIP events on the caller's stream around the whole call); the table has the minimum over
everything and the median over the rounds of the per-round medians.  "ms per second of audio" is the call's time times 250 / T
(frames of 64 samples at 16 kHz).

The kernel keeps a cell's state in registers for the whole call: it is read once and written once, whatever T.  The last column
is the time the state, both ways, and the call's inputs and output take at the device-to-device copy bandwidth measured in this
process on a 256 MB buffer.  Prints one JSON line and writes the table to ``--out``.  No time is fixed anywhere: the file records
what was measured."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obf_rate.txt"))
    a = ap.parse_args()

    import torch
    from misonet_amd import _lib
    from misonet_amd.beamform import Apply_Beamforming, BeamformStream, cells_per_block
    from misonet_amd.blind import SeparateStream
    if not torch.cuda.is_available():
        raise SystemExit("obf_rate needs the GPU: nothing is measured without one")
    F, TS, TL = a.freq, (1, 16, 501), 501
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    calls, nbytes, frames, keep = {}, {}, {}, []
    for M in (2, 6):
        for B in (1, 16):
            mix = torch.view_as_complex(torch.randn((B, M, TL, F, 2), device="cuda", generator=g)).contiguous()
            img = torch.view_as_complex(torch.randn((B, M, M, TL, F, 2), device="cuda", generator=g)).contiguous()
            st = BeamformStream(M, M, F, B)
            st.process(img, mix)                                         # a stream in progress, not a cold start
            for T in TS:
                x, y = img[:, :, :, :T].contiguous(), mix[:, :, :T].contiguous()
                out = torch.empty((B, M, T, F), dtype=torch.complex64, device="cuda")
                arm = f"obf M {M} S {M} B {B} T {T}"
                calls[arm] = (lambda st=st, x=x, y=y, out=out: st.process_into(x, y, out) is None)
                nbytes[arm] = 2 * st.state.numel() + (x.numel() + y.numel() + out.numel()) * 8
                frames[arm] = T
            src = img.permute(0, 1, 4, 2, 3).contiguous()                # [B, S, F, M, T], the offline call's layout
            bf = mix.permute(0, 3, 1, 2).contiguous()                    # [B, F, M, T]
            arm = f"souden M {M} S {M} B {B} T {TL} (offline, S calls)"
            calls[arm] = (lambda src=src, bf=bf, M=M: [Apply_Beamforming(src[:, s], bf, beamformer="souden") for s in range(M)] is None)
            frames[arm] = TL
            sep = SeparateStream(M, F, B)
            sep.process(mix)
            est, im2 = torch.empty_like(mix), torch.empty_like(img)
            arm = f"oiva M {M} B {B} T {TL} (online AuxIVA, est and images)"
            calls[arm] = (lambda sep=sep, mix=mix, est=est, im2=im2: sep.process_into(mix, est, im2) is None)
            frames[arm] = TL
            keep.append((mix, img, st, src, bf, sep))

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
    flags = [int(k[2].fail.max().item()) for k in keep]
    cpb = {M: cells_per_block(M) for M in (2, 6)}
    doc = {"metric": "obf_rate", "device": torch.cuda.get_device_name(0), "F": F, "cells_per_block": cpb,
           "copy_GBps": round(copy_bw / 1e9, 1), "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "arms": res, "flags": flags}
    lines = [f"online beamformer at F {F}, the defaults (residual, alpha 0.98, mu 0, diag_load 1e-3), on {doc['device']}; one wave per "
             f"workgroup, {cpb[2]} cells per workgroup at M 2 and {cpb[6]} at M 6",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events around the whole call); min over all timings, median over the rounds of the per-round medians, "
             "spread = (max - min) / median over the rounds; ms per second of audio = median x 250 / T (16 kHz, hop 64)",
             f"device-to-device copy of 256 MB in this process: {copy_ms:.3f} ms = {copy_bw / 1e9:.0f} GB/s read + written; "
             "state+io = the state both ways (once per call) + images + mix + out", "",
             f"{'arm':<58} {'min ms':>10} {'median ms':>10} {'spread':>8} {'ms / s audio':>13} {'state+io MB':>12} {'at copy bw ms':>14}"]
    for arm, r in res.items():
        tail = f" {r['bytes'] / 1e6:>12.2f} {r['copy_ms']:>14.4f}" if "bytes" in r else ""
        lines.append(f"{arm:<58} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f} {r['ms_per_s_audio']:>13.4f}{tail}")
    lines += ["", f"fail words of the beamformer after the runs (random spectra, not speech): {flags}",
              "the offline call sees all 501 frames before its first output and solves once per bin; the recursion solves once per "
              "frame and bin, is causal, keeps its state between calls and takes the same memory however long the stream",
              "a first version, not tuned"]
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
