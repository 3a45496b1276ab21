"""Cost of the WPE dereverberation.

    python tools/wpe_rate.py [--batch 16] [--frames 1001] [--mics 6] [--bins 129] [--warmup 3] [--iters 10]
                             [--recordings 4] [--seconds 8] [--out profiles/wpe_rate.txt]

Three measurements in one process, HIP events on the caller's stream, ``--warmup`` calls, then the median of ``--iters``:

  batch      one ``misonet_wpe`` call (transpose in, the per-bin kernel, transpose out) on a device-resident complex64
             [B, M, T, F] batch of 4 s chunks with the default options (10 taps, delay 3, 3 iterations)
  recording  the same call on ONE 60 s recording ([1, M, 15001, F]): 129 workgroups, the T loop carries the time
  pass       ``Enhancer.enhance_recordings`` over ``--recordings`` recordings of ``--seconds`` s (seed weights, bf16x6) with
             ``dereverb`` unset and set, wall clock around the whole call, in turn: x real time of each and their ratio

Prints one JSON line; ``--out`` also writes the table.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed_call(a, B, M, T, F):
    import numpy as np
    import torch
    from misonet_amd import _lib
    r = np.random.default_rng(7)
    mix = ((r.standard_normal((B, M, T, F)) + 1j * r.standard_normal((B, M, T, F))) * 0.05).astype(np.complex64)
    mix = torch.from_numpy(mix).cuda()
    out = torch.empty_like(mix)
    L = _lib.lib()
    o = _lib.WpeOpts()
    L.misonet_wpe_opts_default(C.byref(o))
    ws = torch.empty(L.misonet_wpe_workspace_bytes(B, M, T, F, C.byref(o)), dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr(mix.device)

    def fn():
        return L.misonet_wpe(mix.data_ptr(), None, B, M, T, F, C.byref(o), out.data_ptr(), ws.data_ptr(), ws.numel(), st)
    for _ in range(a.warmup):
        _lib.check(fn())
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    bad = torch.empty((B, F), dtype=torch.int32, device="cuda")
    _lib.check(L.misonet_wpe_debug(ws.data_ptr(), B, M, F, C.byref(o), None, bad.data_ptr(), st))
    N = M * o.taps
    K2 = 2 * (N + M)
    flop = 2.0 * T * (K2 * (K2 + 1) / 2) * o.iterations * B * F            # the lower half of the real Gram matrix
    med = statistics.median(ms)
    return {"B": B, "M": M, "T": T, "F": F, "median_ms": round(med, 3), "min_ms": round(min(ms), 3),
            "gram_gflop": round(flop / 1e9, 2), "gram_tflops_at_median": round(flop / med / 1e9, 3),
            "workspace_mb": round(ws.numel() / 1e6, 1), "failed_bins": int(bad.sum().item())}


def timed_pass(a):
    import torch
    import misonet_amd as mz
    from misonet_amd import weights as W
    m1 = mz.MISO_1(2, a.mics, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(W.make_state_dict(W.miso1_spec(), 0))
    m3 = mz.MISO_3(1, a.mics, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(W.make_state_dict(W.miso3_spec(), 1))
    enh = mz.Enhancer(m1.eval(), m3.eval(), num_spks=2, ref_ch=0)
    n = a.seconds * 16000
    recs = [(W.synthetic_utterance(60 + i, n)[0], None, f"r{i}") for i in range(a.recordings)]
    res = {}
    for arm, spec in (("plain", None), ("dereverb", True), ("plain_again", None)):
        enh.set_dereverb(spec)
        enh.enhance_recordings(recs[:1])                                   # warm-up: workspaces, pinned buffers
        ts = []
        for _ in range(max(1, a.iters // 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enh.enhance_recordings(recs)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        res[arm] = {"median_s": round(med, 4), "x_real_time": round(a.recordings * a.seconds / med, 1)}
    res["dereverb_over_plain"] = round(res["dereverb"]["median_s"] / res["plain"]["median_s"], 3)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--bins", type=int, default=129)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--recordings", type=int, default=4)
    ap.add_argument("--seconds", type=int, default=8)
    ap.add_argument("--out", default=None, help="write the table here (profiles/wpe_rate.txt)")
    a = ap.parse_args(argv)
    import torch
    res = {"metric": "wpe_rate", "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters,
           "batch": timed_call(a, a.batch, a.mics, a.frames, a.bins),
           "recording": timed_call(a, 1, a.mics, 15001, a.bins),
           "pass": timed_pass(a)}
    b, r, p = res["batch"], res["recording"], res["pass"]
    lines = [f"wpe_rate: misonet_wpe with the default options (10 taps, delay 3, 3 iterations), {res['device']}",
             f"HIP events, {a.warmup} warm-ups, median of {a.iters} calls, one process",
             "",
             f"{'case':10s} {'shape [B,M,T,F]':>22s} {'median_ms':>10s} {'min_ms':>9s} {'Gram GFLOP':>11s} {'TFLOP/s':>8s} {'ws MB':>8s}"]
    for name, x in (("batch", b), ("recording", r)):
        lines.append(f"{name:10s} {str([x['B'], x['M'], x['T'], x['F']]):>22s} {x['median_ms']:10.3f} {x['min_ms']:9.3f} "
                     f"{x['gram_gflop']:11.2f} {x['gram_tflops_at_median']:8.3f} {x['workspace_mb']:8.1f}")
    lines += ["", f"enhance_recordings, {a.recordings} recordings of {a.seconds} s, wall clock, median of {max(1, a.iters // 3)}:"]
    for arm in ("plain", "dereverb", "plain_again"):
        lines.append(f"  {arm:12s} {p[arm]['median_s']:8.4f} s   {p[arm]['x_real_time']:8.1f} x real time")
    lines.append(f"  dereverb / plain = {p['dereverb_over_plain']:.3f}")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
