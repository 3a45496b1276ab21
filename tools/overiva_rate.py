"""Cost of the online AuxIVA for fewer sources than microphones (``misonet_overiva``) at the bench geometry, beside the determined
``misonet_oiva`` timed in the same process.

    python tools/overiva_rate.py [--freq 129] [--warmup 3] [--iters 10] [--rounds 3] [--out profiles/overiva_rate.txt]

M = 6 microphones with K = 2 and K = 1 sources, and beside them ``oiva M 6`` and ``oiva M 2`` (K = M), each at B = 1 and B = 16
recordings of ``--freq`` bins: one call (est and images) of T = 1, 16 and 501 frames on a stream that has already seen 501 frames
(seeded random spectra resident on the device).  Per arm ``--rounds`` times: ``--warmup`` calls, then ``--iters`` single-call
timings (HIP events on the caller's stream around the whole call); the table has the minimum over everything and the median over
the rounds of the per-round medians.  "ms per second of audio" is the call's time times 250 / T (frames of 64 samples at 16 kHz).
The last column is the arm's median over that of ``oiva M 6`` at the same B and T.

Both kernels read and write the whole state in EVERY frame; "state+io" is T times the state, both ways, and the call's input and
outputs.  One workgroup walks an item: with B = 1 a single CU works.  Prints one JSON line and writes the table to ``--out``.  No
time is fixed anywhere: the file records what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAMES_PER_S = 250.0
ARMS = (("overiva M 6 K 2", 6, 2), ("overiva M 6 K 1", 6, 1), ("oiva M 6", 6, None), ("oiva M 2", 2, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--freq", type=int, default=129)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overiva_rate.txt"))
    a = ap.parse_args()

    import torch
    from misonet_amd import _lib
    from misonet_amd.blind import SeparateStream, bins_per_pass
    if not torch.cuda.is_available():
        raise SystemExit("overiva_rate needs the GPU: nothing is measured without one")
    F, TS, TL = a.freq, (1, 16, 501), 501
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    calls, nbytes, frames, base, keep = {}, {}, {}, {}, []
    for B in (1, 16):
        mixes = {M: torch.view_as_complex(torch.randn((B, M, TL, F, 2), device="cuda", generator=g)).contiguous() for M in (6, 2)}
        for name, M, K in ARMS:
            mix = mixes[M]
            st = SeparateStream(M, F, B, num_src=K)
            st.process(mix)                                              # a stream in progress, not a cold start
            Kn = st.num_src
            for T in TS:
                x = mix[:, :, :T].contiguous()
                est = torch.empty((B, Kn, T, F), dtype=torch.complex64, device="cuda")
                img = torch.empty((B, Kn, M, T, F), dtype=torch.complex64, device="cuda")
                arm = f"{name} B {B} T {T}"
                calls[arm] = (lambda st=st, x=x, est=est, img=img: st.process_into(x, est, img) is None)
                nbytes[arm] = 2 * T * st.state.numel() + x.numel() * 8 + est.numel() * 8 + img.numel() * 8
                frames[arm] = T
                base[arm] = f"oiva M 6 B {B} T {T}"
            keep.append((name, B, st))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        e1.synchronize()
        if rc not in (0, None, False):
            raise RuntimeError(f"the library call failed: {L.misonet_last_error().decode()}")
        return e0.elapsed_time(e1)

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
                    "ms_per_s_audio": round(med * FRAMES_PER_S / frames[arm], 4), "bytes": nbytes[arm]}
    for arm, r in res.items():
        r["over_oiva_m6"] = round(r["median_ms"] / res[base[arm]]["median_ms"], 4)
    flags = {f"{name} B {B}": int(st.fail.max().item()) for name, B, st in keep}
    P = {"overiva M 6 K 2": bins_per_pass(6, 2), "overiva M 6 K 1": bins_per_pass(6, 1), "oiva M 6": bins_per_pass(6),
         "oiva M 2": bins_per_pass(2)}
    doc = {"metric": "overiva_rate", "device": torch.cuda.get_device_name(0), "F": F, "bins_per_pass": P, "warmup": a.warmup,
           "iters": a.iters, "rounds": a.rounds, "arms": res, "flags": flags}
    lines = [f"online AuxIVA with K < M sources (overiva) beside the determined kernel (oiva) at F {F}, alpha 0.98, gauss, est and "
             f"images written, on {doc['device']}; one workgroup per item; bins per pass: {P}",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events around the whole call); min over all timings, median over the rounds of the per-round medians, "
             "spread = (max - min) / median over the rounds; ms per second of audio = median x 250 / T (16 kHz, hop 64)",
             "state+io = T x the state both ways + the input + est + images; / oiva M 6 = the median over that of oiva M 6 at the "
             "same B and T", "",
             f"{'arm':<34} {'min ms':>10} {'median ms':>10} {'spread':>8} {'ms / s audio':>13} {'state+io MB':>12} {'/ oiva M 6':>11}"]
    for arm, r in res.items():
        lines.append(f"{arm:<34} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f} {r['ms_per_s_audio']:>13.4f} "
                     f"{r['bytes'] / 1e6:>12.2f} {r['over_oiva_m6']:>11.4f}")
    lines += ["", f"fail words after the runs (random spectra, not speech): {flags}",
              "the project's own definition in the OverIVA family, not compared against other packages; a first version, not tuned"]
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
