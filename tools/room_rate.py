"""Cost of the room simulator (``misonet_room_rir``, ``misonet_room_mix``) alone, beside the NumPy restatement on the same host
and beside the time the mixer's bytes would take at the copy bandwidth of the same box.

    python tools/room_rate.py [--scenes 16] [--speakers 2] [--mics 6] [--fs 8000] [--rir-len 4096] [--samples 64000]
                              [--rt60 0.4] [--warmup 3] [--iters 10] [--rounds 3] [--host-pairs 2]
                              [--out profiles/room_rate.txt]

In this one process, on one box: ``--scenes`` seeded rooms of 5-8 x 4-6 x 2.5-3 m at one nominal RT60 (Sabine), S sources and M
microphones each.

  rir               one call for all scenes: B S M RIRs of ``--rir-len`` taps, geometry already on the device
  mix               one call for all scenes: images, early and mix of ``--samples`` samples out of device-resident sources and RIRs
  the floor of mix  its minimum traffic -- sources and RIRs read once, images, early and mix written once -- at the copy bandwidth
                    measured here: a device-to-device copy of 1 GiB, read + write counted, the best of its timings
  NumPy             tests/room_ref.py on this host's CPU (at most 16 threads): ``--host-pairs`` pairs of the RIR and one
                    (source, microphone) convolution of the mixer, scaled to the whole batch by the pair count

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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(var, "16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--speakers", type=int, default=2)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--fs", type=int, default=8000)
    ap.add_argument("--rir-len", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--rt60", type=float, default=0.4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "room_rate.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import room_ref as R
    from misonet_amd import _lib
    from misonet_amd import room as RM
    B, S, M, fs, Lh, Ls = a.scenes, a.speakers, a.mics, a.fs, a.rir_len, a.samples
    rng = np.random.default_rng(7)
    dim = np.stack([rng.uniform(5, 8, B), rng.uniform(4, 6, B), rng.uniform(2.5, 3, B)], 1)
    beta = np.stack([np.full(6, RM.beta_from_rt60(d, a.rt60)) for d in dim])
    src = 0.5 + rng.uniform(0, 1, (B, S, 3)) * (dim[:, None, :] - 1.0)
    mic = 0.5 + rng.uniform(0, 1, (B, M, 3)) * (dim[:, None, :] - 1.0)
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    room_d, beta_d, src_d, mic_d = (dev(x, np.float64) for x in (dim, beta, src, mic))
    L = _lib.lib()
    st = _lib.stream_ptr(room_d.device)
    rir = torch.empty((B, S, M, Lh), dtype=torch.float64, device="cuda")
    fail = torch.empty((B, S, M), dtype=torch.int32, device="cuda")
    x = torch.randn((B, S, Ls), device="cuda", dtype=torch.float32)
    split = torch.full((B, S), 450, dtype=torch.int32, device="cuda")
    images, early = (torch.empty((B, S, M, Ls), dtype=torch.float32, device="cuda") for _ in range(2))
    mixd = torch.empty((B, M, Ls), dtype=torch.float32, device="cuda")
    calls = {
        "rir": lambda: L.misonet_room_rir(room_d.data_ptr(), beta_d.data_ptr(), src_d.data_ptr(), mic_d.data_ptr(), B, S, M,
                                          float(fs), 343.0, Lh, -1, rir.data_ptr(), fail.data_ptr(), st),
        "mix": lambda: L.misonet_room_mix(x.data_ptr(), S * Ls, Ls, 1, rir.data_ptr(), split.data_ptr(), B, S, M, Ls, Lh, Ls,
                                          images.data_ptr(), early.data_ptr(), mixd.data_ptr(), st),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        e1.synchronize()
        if rc not in (0, None):
            raise RuntimeError(f"the library call failed: {L.misonet_last_error().decode()}")
        return e0.elapsed_time(e1)

    cs = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    cd = torch.empty_like(cs)
    def copy():
        cd.copy_(cs)
    for _ in range(a.warmup):
        copy()
    copy_ms = min(timed(copy) for _ in range(a.iters))
    gbps = 2 * cs.numel() / copy_ms / 1e6
    del cs, cd

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
    flags = int((fail != 0).sum().item())

    # the restatement on this host, a few pairs, scaled by the pair count; and its answer against the device's
    h_dev = rir.cpu().numpy()
    n_img, t_rir, worst = [], 0.0, 0.0
    for k in range(a.host_pairs):
        b, s, m = k % B, k % S, k % M
        t0 = time.perf_counter()
        h, _, n = R.rir_pair(dim[b], beta[b], src[b, s], mic[b, m], fs, Lh, return_count=True)
        t_rir += time.perf_counter() - t0
        n_img.append(n)
        worst = max(worst, R.rel_l2(h_dev[b, s, m], h))
    host_rir_ms = t_rir / a.host_pairs * B * S * M * 1e3
    xh = x[0, 0].cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    y = np.convolve(h_dev[0, 0, 0], xh)[:Ls]
    host_mix_ms = (time.perf_counter() - t0) * B * S * M * 1e3
    mix_err = R.rel_l2(images[0, 0, 0].cpu().numpy(), y)
    traffic = B * S * Ls * 4 + B * S * M * Lh * 8 + 2 * B * S * M * Ls * 4 + B * M * Ls * 4
    floor_ms = traffic / gbps / 1e6
    macs = B * S * M * Ls * Lh
    doc = {"metric": "room_rate", "device": torch.cuda.get_device_name(0), "scenes": B, "S": S, "M": M, "fs": fs, "Lh": Lh,
           "L": Ls, "rt60_nominal": a.rt60, "images_per_pair": n_img, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "copy_gb_per_s": round(gbps, 1), "arms": res, "flags": flags, "host_rir_ms": round(host_rir_ms, 1),
           "host_mix_ms": round(host_mix_ms, 1), "mix_traffic_bytes": traffic, "mix_floor_ms": round(floor_ms, 4),
           "rir_rel_l2_vs_host": worst, "mix_rel_l2_vs_host": mix_err}
    print(json.dumps(doc))
    lines = [f"room simulator at {B} scenes, S {S}, M {M}, fs {fs}, Lh {Lh}, L {Ls}, nominal RT60 {a.rt60} s on {doc['device']}: "
             f"{B * S * M} pairs, {n_img} images per pair (the first {a.host_pairs})",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events); min over all timings, median over the rounds of the per-round medians, spread = (max - min) "
             "/ median over the rounds",
             f"copy bandwidth measured here (1 GiB device to device, read + write, best of {a.iters}): {gbps:.0f} GB/s",
             "", f"{'arm':<12} {'min ms':>10} {'median ms':>10} {'spread':>8}"]
    lines += [f"{arm:<12} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f}" for arm, r in res.items()]
    lines += ["", f"rir: {res['rir']['min_ms'] / (B * S * M):.4f} ms per pair; NumPy restatement on this host {host_rir_ms / (B * S * M):.0f} ms "
              f"per pair, {host_rir_ms:.0f} ms for the batch: x {host_rir_ms / res['rir']['min_ms']:.0f}; device against host rel-L2 "
              f"{worst:.2e}",
              f"mix: {macs / 1e9:.1f} G float64 FMAs, {macs / res['mix']['min_ms'] / 1e9:.2f} T FMA/s; np.convolve on this host "
              f"{host_mix_ms:.0f} ms for the batch: x {host_mix_ms / res['mix']['min_ms']:.0f}; device against host rel-L2 {mix_err:.2e}",
              f"mix floor: {traffic / 1e6:.1f} MB at the copy bandwidth = {floor_ms:.4f} ms: x {res['mix']['min_ms'] / floor_ms:.1f} "
              "(direct form: bound by the float64 FMAs, not by memory)",
              f"pairs with a flag: {flags}", "a first version, not tuned"]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
