"""Cost of the source localisation (``misonet_doa``) at the bench geometry, beside AuxIVA and the Souden beamformer timed in the
same process.

    python tools/doa_rate.py [--batch 16] [--freq 129] [--mics 6] [--frames 1001] [--cand 2562] [--kind srp_phat]
                             [--block 40] [--hop 16] [--warmup 3] [--iters 10] [--rounds 3] [--kernel-csv FILE]
                             [--out profiles/doa_rate.txt]

Two geometries in one process on one box: one map per recording (N = 1) and block maps (``--block`` frames every ``--hop``: N = 61
at the defaults).  Inputs are seeded random spectra resident on the device; the candidates are a Fibonacci lattice of ``--cand``
unit vectors, the array a 5 cm circle.  Per arm ``--rounds`` times: ``--warmup`` calls, then ``--iters`` single-call timings (HIP
events on the caller's stream around the whole call); the table has the minimum over everything and the median over the rounds of
the per-round medians.

The three kernels inside a call cannot be bracketed by events from outside it.  Their times come from a run of this tool under
``rocprofv3 --kernel-trace --stats`` (a run of its own, with ``--iters 2 --rounds 1 --only doa``); ``--kernel-csv`` takes the
kernel-stats CSV of that run and adds the per-kernel table and the steering kernel's rate.  The rate counts the definition's
B K N D nF M (M - 1) / 2 complex multiply-adds as 4 real float64 FMAs each; the phasors (M sincos per chunk of bins, M complex
rotations per bin) and the M - 1 closing products are not counted.  Prints one JSON line and writes the table to ``--out``.
No time is fixed anywhere: the file records what was measured."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# float64 vector FMAs per second on an MI355X: 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz -- half the float32 rate of one
# v_fma_f32 per wave64 per 2 cycles; = the 78.6 TFLOPS float64 vector peak of the data sheet
PEAK_F64_FMA = 256 * 4 * 16 * 2.4e9


def fibonacci_sphere(n):
    import numpy as np
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = np.pi * (1.0 + 5.0 ** 0.5) * i
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def kernel_table(path):
    """{kernel family: (calls, average ms)} from a rocprofv3 kernel-stats CSV"""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            m = re.search(r"doa_(cov|steer|peak)_k", name)
            if not m:
                continue
            calls = int(float(row.get("Calls", 0)))
            total = float(row.get("TotalDurationNs", 0.0))
            key = f"doa_{m.group(1)}_k"
            c0, t0 = out.get(key, (0, 0.0))
            out[key] = (c0 + calls, t0 + total)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--freq", type=int, default=129)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--cand", type=int, default=2562)
    ap.add_argument("--kind", default="srp_phat")
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--hop", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("all", "doa"), default="all")
    ap.add_argument("--kernel-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doa_rate.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from misonet_amd import _lib
    from misonet_amd import localize as LZ
    B, F, M, T, D, fs = a.batch, a.freq, a.mics, a.frames, a.cand, 8000.0
    if not torch.cuda.is_available():
        raise SystemExit("doa_rate needs the GPU: nothing is measured without one")
    g = torch.Generator(device="cuda").manual_seed(7)
    mix = torch.view_as_complex(torch.randn((B, F, M, T, 2), device="cuda", generator=g)).contiguous()
    ang = 2.0 * np.pi * np.arange(M) / M
    mic = np.stack([0.05 * np.cos(ang), 0.05 * np.sin(ang), np.zeros(M)], axis=1)
    dirs = fibonacci_sphere(D)
    tau = torch.from_numpy(LZ.far_field_delays(mic, dirs)).cuda()
    pts = torch.from_numpy(dirs).cuda()
    L = _lib.lib()
    st = _lib.stream_ptr(mix.device)
    S = 2
    geos = {"N=1": (0, 0), f"block {a.block} hop {a.hop}": (a.block, a.hop)}
    calls, Ns = {}, {}
    keep = []
    for name, (block, hop) in geos.items():
        opts = LZ.Localizer(kind=a.kind, num_src=S, block=block, hop=hop, min_sep=0.3).validate(M, D, T).c_opts(F, fs)
        N = L.misonet_doa_blocks(T, block, hop)
        nws = L.misonet_doa_workspace_bytes(B, 1, F, M, T, D, C.byref(opts))
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        q = torch.empty((B, 1, N, D), dtype=torch.float64, device="cuda")
        peak = torch.empty((B, 1, N, S), dtype=torch.int32, device="cuda")
        value = torch.empty((B, 1, N, S), dtype=torch.float64, device="cuda")
        fail = torch.empty((B, 1, N), dtype=torch.int32, device="cuda")
        keep.append((opts, ws, q, peak, value, fail))
        Ns[f"doa {name}"] = N
        calls[f"doa {name}"] = (lambda o=opts, w=ws, q=q, p=peak, v=value, f=fail: L.misonet_doa(
            mix.data_ptr(), None, tau.data_ptr(), 1, pts.data_ptr(), B, 1, F, M, T, D, fs, C.byref(o), q.data_ptr(), p.data_ptr(),
            v.data_ptr(), f.data_ptr(), w.data_ptr(), w.numel(), st))
    if a.only == "all":
        from misonet_amd.beamform import Apply_Beamforming, Beamformer
        from misonet_amd.blind import auxiva
        est = mix * 0.5
        souden = Beamformer(kind="souden")
        calls["auxiva (2 sources, 20 iterations)"] = lambda: auxiva(mix, 2) is None
        calls["souden (one source)"] = lambda: Apply_Beamforming(est, mix, beamformer=souden) is None

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
    res = {arm: {"min_ms": round(mins[arm], 4), "median_ms": round(statistics.median(v), 4),
                 "spread": round((max(v) - min(v)) / statistics.median(v), 4)} for arm, v in meds.items()}
    cmacs = {arm: B * N * D * F * M * (M - 1) // 2 for arm, N in Ns.items()}
    doc = {"metric": "doa_rate", "device": torch.cuda.get_device_name(0), "B": B, "F": F, "M": M, "T": T, "D": D, "kind": a.kind,
           "blocks": Ns, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "arms": res,
           "steer_complex_macs": cmacs, "flags": [int(k[5].max().item()) for k in keep]}
    lines = [f"source localisation ({a.kind}, {S} peaks) at B {B}, F {F} (all bins), M {M}, T {T}, D {D} on {doc['device']}",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events around the whole call); min over all timings, median over the rounds of the per-round medians, "
             "spread = (max - min) / median over the rounds", "",
             f"{'arm':<36} {'maps':>6} {'min ms':>10} {'median ms':>10} {'spread':>8}"]
    lines += [f"{arm:<36} {B * Ns.get(arm, 0) or '':>6} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f}"
              for arm, r in res.items()]
    lines += ["", "steering work by the definition's count, 4 real float64 FMAs per complex multiply-add, over the WHOLE call's time "
              "(a lower bound of the kernel's rate):"]
    for arm, n in cmacs.items():
        rate = 4.0 * n / (res[arm]["min_ms"] * 1e-3)
        lines.append(f"  {arm}: {n / 1e9:.2f} G complex multiply-adds, {rate / 1e12:.3f} T FMA/s = {100 * rate / PEAK_F64_FMA:.1f} % of "
                     f"{PEAK_F64_FMA / 1e12:.1f} T FMA/s")
    if a.kernel_csv:
        kt = kernel_table(a.kernel_csv)
        doc["kernels"] = {k: {"calls": c, "avg_ms": round(t / max(c, 1) / 1e6, 4)} for k, (c, t) in kt.items()}
        lines += ["", "kernel times from a separate run under rocprofv3 --kernel-trace --stats (both geometries' launches averaged "
                  "together; the block geometry dominates):", f"  {'kernel':<14} {'calls':>6} {'average ms':>12} {'total ms':>10}"]
        lines += [f"  {k:<14} {c:>6} {t / max(c, 1) / 1e6:>12.4f} {t / 1e6:>10.3f}" for k, (c, t) in sorted(kt.items())]
        if "doa_steer_k" in kt:
            c, t = kt["doa_steer_k"]
            per_pair = sum(cmacs.values())                 # one launch of each geometry per pair of calls
            rate = 4.0 * per_pair * (c / len(cmacs)) / (t * 1e-9)
            doc["steer_fma_per_s"] = rate
            lines.append(f"  doa_steer_k alone: {rate / 1e12:.3f} T FMA/s = {100 * rate / PEAK_F64_FMA:.1f} % of the float64 vector FMA "
                         f"rate ({PEAK_F64_FMA / 1e12:.1f} T FMA/s = 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz)")
    lines += ["", "the phasors (per candidate M float64 sincos per chunk of bins and M complex rotations per bin) and the M - 1 closing "
              "products are not counted as work", "a first version, not tuned"]
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
