"""Cost of the blind separation (``misonet_auxiva``) alone, beside the time its minimum memory traffic would take.

    python tools/iva_rate.py [--batch 16] [--speakers 2] [--frames 1001] [--mics 6] [--bins 129] [--iterations 20]
                             [--channels 2 6] [--warmup 3] [--iters 10] [--rounds 3] [--no-context]
                             [--out profiles/iva_rate.txt]

At the bench geometry, in this one process, on one box, per ``--channels`` value K:

  auxiva            the whole call (PCA, ``iterations`` x (weights + steering), projection, selection, images) on device-resident
                    input: S sources with sparse envelopes through random per-bin mixing plus noise
  auxiva, 0 it.     the same call with iterations = 0; (auxiva - this) / iterations is the time of ONE iteration
  the floor         the minimum traffic of one iteration -- Y complex128 [B, F, K, T] read once and written once, phi float64
                    [B, K, T] read once per bin -- at the copy bandwidth measured here: a device-to-device copy of 1 GiB, read +
                    write counted, the best of its timings

and, as context only (``--no-context`` leaves them out): ``misonet_cacgmm`` (10 iterations, K = S + 1 classes) and
``Enhancer.separate`` on seed weights at the same geometry.

Per arm ``--rounds`` times: ``--warmup`` calls, then ``--iters`` single-call timings (HIP events on the caller's stream); the
table has the minimum over everything and the median over the rounds of the per-round medians.  Prints one JSON line and writes
the table to ``--out``.  No time is fixed anywhere: the file records what was measured.
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
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--channels", type=int, nargs="+", default=[2, 6])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-context", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iva_rate.txt"))
    a = ap.parse_args()

    import torch
    import misonet_amd as mz
    from misonet_amd import _lib
    B, S, F, M, T, IT = a.batch, a.speakers, a.bins, a.mics, a.frames, a.iterations
    g = torch.Generator(device="cuda")
    g.manual_seed(7)

    def cn(*shape):
        return torch.view_as_complex(torch.randn(*shape, 2, generator=g, device="cuda") * 0.5 ** 0.5)
    env = (torch.rand(B, S, 1, 1, (T + 7) // 8, generator=g, device="cuda") < 0.4).repeat_interleave(8, dim=-1)[..., :T] + 0.02
    img = cn(B, S, F, M, 1) * cn(B, S, F, 1, T) * env                                                 # [B, S, F, M, T]
    mix = (img.sum(dim=1) + 0.05 * cn(B, F, M, T)).contiguous()
    L = _lib.lib()
    st = _lib.stream_ptr(mix.device)
    images = torch.empty((B, S, F, M, T), dtype=torch.complex64, device="cuda")
    calls, bufs = {}, {}
    for K in a.channels:
        bufs[K] = torch.empty(L.misonet_auxiva_workspace_bytes(B, S, K, F, M, T), dtype=torch.uint8, device="cuda")
        for it in (IT, 0):
            o = _lib.IvaOpts(it, 0, K, 0, 1e-10)
            calls[f"auxiva K = {K}, {it} it."] = lambda o=o, K=K: L.misonet_auxiva(
                mix.data_ptr(), B, S, F, M, T, C.byref(o), images.data_ptr(), None, bufs[K].data_ptr(), bufs[K].numel(), st)
    if not a.no_context:
        from misonet_amd import weights as W
        from misonet_amd.refine import Refine
        co = Refine(iterations=10).c_opts()
        cws = torch.empty(L.misonet_cacgmm_workspace_bytes(B, S + 1, F, M), dtype=torch.uint8, device="cuda")
        g0 = torch.rand((B, S + 1, F, T), generator=g, device="cuda")
        g0 = (g0 / g0.sum(dim=1, keepdim=True)).contiguous()
        masks = torch.empty_like(g0)
        calls["(context) cacgmm, 10 it."] = lambda: L.misonet_cacgmm(mix.data_ptr(), g0.data_ptr(), B, S + 1, F, M, T, C.byref(co),
                                                                      masks.data_ptr(), images.data_ptr(), cws.data_ptr(),
                                                                      cws.numel(), st)
        m1 = mz.MISO_1(S, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m1.load_state_dict(W.make_state_dict(W.miso1_spec(), 0))
        enh = mz.Enhancer(m1.eval(), None, num_spks=S)
        obs = mix.permute(0, 2, 3, 1).contiguous()                                                    # [B, M, T, F]

        def separate():
            enh.separate(obs, check_nan=False)
            return 0
        calls["(context) Enhancer.separate"] = separate

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        e1.synchronize()
        if rc not in (0, None):
            raise RuntimeError(f"the library call failed: {L.misonet_last_error().decode()}")
        return e0.elapsed_time(e1)

    # the copy bandwidth of this box, in this process: 1 GiB device to device, read + write counted
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    def copy():
        dst.copy_(src)
    for _ in range(a.warmup):
        copy()
    copy_ms = min(timed(copy) for _ in range(a.iters))
    gbps = 2 * src.numel() / copy_ms / 1e6
    del src, dst

    meds, mins = {arm: [] for arm in calls}, {arm: float("inf") for arm in calls}
    for _ in range(a.rounds):
        for arm, fn in calls.items():
            for _ in range(a.warmup):
                timed(fn)
            ms = [timed(fn) for _ in range(a.iters)]
            meds[arm].append(statistics.median(ms))
            mins[arm] = min(mins[arm], min(ms))
    failed = {}
    for K in a.channels:                                  # the workspace of K holds the flags of its last call (0 iterations)
        bad = torch.empty((B, F), dtype=torch.int32, device="cuda")
        _lib.check(L.misonet_auxiva_debug(bufs[K].data_ptr(), B, K, F, M, T, None, None, None, None, bad.data_ptr(), st))
        failed[K] = int((bad != 0).sum().item())
    res = {arm: {"min_ms": round(mins[arm], 4), "median_ms": round(statistics.median(v), 4),
                 "spread": round((max(v) - min(v)) / statistics.median(v), 4)} for arm, v in meds.items()}
    per_it = {}
    for K in a.channels:
        full, zero = res[f"auxiva K = {K}, {IT} it."], res[f"auxiva K = {K}, 0 it."]
        traffic = B * F * K * T * 16 * 2 + B * F * K * T * 8
        per_it[K] = {"ms_per_iteration_min": round((full["min_ms"] - zero["min_ms"]) / max(IT, 1), 4),
                     "ms_per_iteration_median": round((full["median_ms"] - zero["median_ms"]) / max(IT, 1), 4),
                     "traffic_bytes": traffic, "floor_ms": round(traffic / gbps / 1e6, 4),
                     "resident": bool(T <= L.misonet_auxiva_resident_frames(K))}
    doc = {"metric": "iva_rate", "device": torch.cuda.get_device_name(0), "batch": B, "speakers": S, "F": F, "M": M, "T": T,
           "iterations": IT, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "copy_gb_per_s": round(gbps, 1),
           "failed_bins": failed, "arms": res, "per_iteration": per_it}
    print(json.dumps(doc))
    lines = [f"blind separation (AuxIVA-ISS, gauss) at batch {B}, {S} sources, F {F}, M {M}, T {T} on {doc['device']}: {B * F} "
             f"workgroups per steering launch, {IT} iterations = {3 + 2 * IT} launches",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events); min over all timings, median over the rounds of the per-round medians, spread = (max - min) "
             "/ median over the rounds",
             f"copy bandwidth measured here (1 GiB device to device, read + write, best of {a.iters}): {gbps:.0f} GB/s",
             "", f"{'arm':<32} {'min ms':>10} {'median ms':>10} {'spread':>8}"]
    lines += [f"{arm:<32} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f}" for arm, r in res.items()]
    lines += ["", "one iteration = (auxiva - auxiva with 0 iterations) / iterations; the floor = Y read once and written once, phi "
              "read once per bin, at the copy bandwidth above"]
    for K, r in per_it.items():
        lines += [f"K = {K}: {r['ms_per_iteration_min']:.4f} ms per iteration (min; median {r['ms_per_iteration_median']:.4f}), "
                  f"floor {r['floor_ms']:.4f} ms for {r['traffic_bytes'] / 1e6:.1f} MB: x {r['ms_per_iteration_min'] / r['floor_ms']:.1f}"
                  f" ({'resident' if r['resident'] else 'streaming'} steering kernel)"]
    lines += [f"bins with a flag: {failed}", "a first version, not tuned"]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
