"""Cost of step 5 of the fused pass with the WPD convolutional beamformer, against "souden" (and the reference's MVDR).

    python tools/wpd_rate.py [--batch 16] [--speakers 2] [--frames 1001] [--mics 6] [--bins 129] [--taps 5] [--delay 3]
                             [--warmup 5] [--iters 20] [--rounds 5] [--out profiles/wpd_rate.txt]

Step 5 of a pass at the bench geometry beamforms batch x speakers = 32 (item, speaker) pairs of 129 bins: 4128 workgroups of
``wpd_bin_k``.  The drop-in calls take one source per item, so the tool times ONE ``misonet_wpd`` / ``misonet_beamform`` /
``misonet_mvdr`` call on batch x speakers items -- the same grids and the same bytes, read through the interleaved views
instead of the planar ones -- on device-resident complex64 [B S, F, M, T] inputs (a dominant rank-1 source with an echo, plus
noise), with HIP events on the caller's stream.  All arms run in this one process, in turn, ``--rounds`` times: ``--warmup``
calls, then the median of ``--iters`` single-call timings; the table has, per arm, the median over the rounds of those medians
and the spread (max - min) / median over the rounds.  Prints one JSON line and writes the table to ``--out``.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--speakers", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--bins", type=int, default=129)
    ap.add_argument("--taps", type=int, default=5)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpd_rate.txt"))
    a = ap.parse_args()

    import torch
    from misonet_amd import _lib
    N, F, M, T = a.batch * a.speakers, a.bins, a.mics, a.frames
    g = torch.Generator(device="cuda")
    g.manual_seed(7)

    def cn(*shape):
        return torch.view_as_complex(torch.randn(*shape, 2, generator=g, device="cuda") * 0.5 ** 0.5)
    s = cn(N, F, 1, T)
    src = cn(N, F, M, 1) * s + 0.1 * cn(N, F, M, T)
    mix = src + 0.5 * cn(N, F, M, 1) * torch.roll(s, 4, dims=-1) + 0.5 * cn(N, F, M, T)     # an echo four frames later
    src, mix = src.contiguous(), mix.contiguous()
    out = torch.empty((N, T, F), dtype=torch.complex64, device="cuda")
    L = _lib.lib()
    st = _lib.stream_ptr(src.device)
    calls = {}

    def ws_of(n):
        if n < 0:
            raise RuntimeError("the size function refused the options")
        return torch.empty(max(int(n), 8), dtype=torch.uint8, device="cuda")
    w0 = ws_of(L.misonet_mvdr_workspace_bytes(N, F, M))
    calls["mvdr"] = lambda: L.misonet_mvdr(src.data_ptr(), mix.data_ptr(), N, F, M, T, 1e-6, out.data_ptr(), w0.data_ptr(),
                                           w0.numel(), st)
    ob = _lib.BfOpts()
    L.misonet_bf_opts_default(C.byref(ob))
    ob.kind = 1
    w1 = ws_of(L.misonet_beamform_workspace_bytes(N, F, M, C.byref(ob)))
    calls["souden"] = lambda: L.misonet_beamform(src.data_ptr(), mix.data_ptr(), N, F, M, T, C.byref(ob), out.data_ptr(),
                                                 w1.data_ptr(), w1.numel(), st)
    ow = _lib.WpdOpts()
    L.misonet_wpd_opts_default(C.byref(ow))
    ow.taps, ow.delay = a.taps, a.delay
    w2 = ws_of(L.misonet_wpd_workspace_bytes(N, F, M, C.byref(ow)))
    calls["wpd"] = lambda: L.misonet_wpd(src.data_ptr(), mix.data_ptr(), N, F, M, T, C.byref(ow), out.data_ptr(), w2.data_ptr(),
                                         w2.numel(), st)

    meds = {arm: [] for arm in calls}
    for _ in range(a.rounds):
        for arm, fn in calls.items():
            for _ in range(a.warmup):
                if fn() != 0:
                    raise RuntimeError(f"{arm}: the library call failed: {L.misonet_last_error().decode()}")
            ms = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            meds[arm].append(statistics.median(ms))
    bad = torch.empty((N, F), dtype=torch.int32, device="cuda")
    _lib.check(L.misonet_wpd_debug(w2.data_ptr(), N, F, M, C.byref(ow), None, bad.data_ptr(), st))
    failed = int(bad.sum().item())
    res = {arm: {"median_ms": round(statistics.median(v), 4), "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
           for arm, v in meds.items()}
    ratio = res["wpd"]["median_ms"] / res["souden"]["median_ms"]
    doc = {"metric": "wpd_rate", "device": torch.cuda.get_device_name(0), "batch": a.batch, "speakers": a.speakers, "F": F, "M": M,
           "T": T, "taps": a.taps, "delay": a.delay, "K": M * (a.taps + 1), "workgroups": N * F, "warmup": a.warmup,
           "iters": a.iters, "rounds": a.rounds, "failed_bins": failed, "arms": res, "wpd_over_souden": round(ratio, 3)}
    print(json.dumps(doc))
    lines = [f"step 5 at batch {a.batch} x {a.speakers} speakers, F {F}, M {M}, T {T} on {doc['device']}: one call on {N} items "
             f"({N * F} workgroups of wpd_bin_k), WPD with taps {a.taps}, delay {a.delay} (K = {doc['K']})",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then the median of {a.iters} "
             "single-call timings (HIP events); median over the rounds, spread = (max - min) / median over the rounds",
             "", f"{'arm':<8} {'median ms':>10} {'spread':>8}"]
    lines += [f"{arm:<8} {r['median_ms']:>10.4f} {r['spread']:>8.4f}" for arm, r in res.items()]
    lines += ["", f"wpd / souden = {ratio:.3f}   (bins that failed in the WPD arm: {failed})"]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
