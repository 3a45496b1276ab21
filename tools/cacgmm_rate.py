"""Cost of the guided spatial clustering (step 4b of the fused pass), alone and inside the fused step.

    python tools/cacgmm_rate.py [--batch 16] [--speakers 2] [--frames 1001] [--mics 6] [--bins 129] [--iterations 10]
                                [--prior bin] [--warmup 3] [--iters 10] [--rounds 3] [--no-fused]
                                [--out profiles/cacgmm_rate.txt]

Two measurements at the bench geometry, in this one process, on one box:

  step 4b alone   ``misonet_masks_from_estimates`` + ``misonet_cacgmm`` (images included) on device-resident inputs: two
                  rank-1 sources that alternate in activity plus noise, and their noisy images as the estimates;
                  batch x bins workgroups of ``cacgmm_bin_k``, iterations + 1 sweeps each
  the fused step  ``Enhancer.enhance`` on seed weights in the library's default arithmetic with refine off and on, arms in turn.
                  With refine off the pass is bit for bit the parent commit's, so that arm is the parent's step time measured
                  beside the new one.

Per arm ``--rounds`` times: ``--warmup`` calls, then the median of ``--iters`` single-call timings (HIP events on the caller's
stream); the table has the median over the rounds of those medians and the spread (max - min) / median over the rounds.
Prints one JSON line and writes the table to ``--out``.
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
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--prior", default="bin")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-fused", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cacgmm_rate.txt"))
    a = ap.parse_args()

    import torch
    import misonet_amd as mz
    from misonet_amd import _lib
    from misonet_amd.refine import Refine
    B, S, F, M, T = a.batch, a.speakers, a.bins, a.mics, a.frames
    K = S + 1
    rf = Refine(iterations=a.iterations, prior=a.prior).validate(M, S)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)

    def cn(*shape):
        return torch.view_as_complex(torch.randn(*shape, 2, generator=g, device="cuda") * 0.5 ** 0.5)
    act = torch.randint(0, K, (B, 1, F, 1, T), generator=g, device="cuda")
    img = torch.cat([cn(B, 1, F, M, 1) * cn(B, 1, F, 1, T) * (act == s) for s in range(S)], dim=1)       # [B, S, F, M, T]
    mix = (img.sum(dim=1) + 0.1 * cn(B, F, M, T)).contiguous()
    est = (img + 0.2 * cn(B, S, F, M, T)).contiguous()
    L = _lib.lib()
    st = _lib.stream_ptr(mix.device)
    opts = rf.c_opts()
    ws = torch.empty(L.misonet_cacgmm_workspace_bytes(B, K, F, M), dtype=torch.uint8, device="cuda")
    g0 = torch.empty((B, K, F, T), dtype=torch.float32, device="cuda")
    masks = torch.empty_like(g0)
    images = torch.empty_like(est)

    def step4b():
        r = L.misonet_masks_from_estimates(est.data_ptr(), mix.data_ptr(), B, S, F, M, T, g0.data_ptr(), st)
        return r or L.misonet_cacgmm(mix.data_ptr(), g0.data_ptr(), B, K, F, M, T, C.byref(opts), masks.data_ptr(),
                                     images.data_ptr(), ws.data_ptr(), ws.numel(), st)
    calls = {"step 4b alone": step4b}
    if not a.no_fused:
        from misonet_amd import weights as W
        m1 = mz.MISO_1(S, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m1.load_state_dict(W.make_state_dict(W.miso1_spec(), 0))
        m3 = mz.MISO_3(1, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m3.load_state_dict(W.make_state_dict(W.miso3_spec(), 1))
        enh = {False: mz.Enhancer(m1.eval(), m3.eval(), num_spks=S), True: mz.Enhancer(m1.eval(), m3.eval(), num_spks=S, refine=rf)}
        obs = mix.permute(0, 2, 3, 1).contiguous()                                                       # [B, M, T, F]

        def fused(on):
            enh[on].enhance(obs, check_nan=False)
            return 0
        calls["fused, refine off"] = lambda: fused(False)
        calls["fused, refine on"] = lambda: fused(True)

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
    bad = torch.empty((B, F), dtype=torch.int32, device="cuda")
    _lib.check(L.misonet_cacgmm_debug(ws.data_ptr(), B, K, F, M, None, None, None, bad.data_ptr(), st))
    failed = int(bad.sum().item())
    res = {arm: {"median_ms": round(statistics.median(v), 4), "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
           for arm, v in meds.items()}
    doc = {"metric": "cacgmm_rate", "device": torch.cuda.get_device_name(0), "batch": B, "speakers": S, "F": F, "M": M, "T": T,
           "iterations": a.iterations, "prior": a.prior, "workgroups": B * F, "warmup": a.warmup, "iters": a.iters,
           "rounds": a.rounds, "failed_bins": failed, "arms": res}
    print(json.dumps(doc))
    lines = [f"guided spatial clustering at batch {B}, {S} speakers, F {F}, M {M}, T {T} on {doc['device']}: {B * F} workgroups "
             f"of cacgmm_bin_k, {a.iterations} iterations ({a.iterations + 1} sweeps), prior {a.prior}",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then the median of {a.iters} "
             "single-call timings (HIP events); median over the rounds, spread = (max - min) / median over the rounds",
             "", f"{'arm':<20} {'median ms':>10} {'spread':>8}"]
    lines += [f"{arm:<20} {r['median_ms']:>10.4f} {r['spread']:>8.4f}" for arm, r in res.items()]
    if not a.no_fused:
        off, on = res["fused, refine off"]["median_ms"], res["fused, refine on"]["median_ms"]
        lines += ["", f"fused on / off = {on / off:.3f} (+{on - off:.3f} ms; refine off is the parent commit's pass, bit for bit)"]
    lines += [f"bins that failed in the stand-alone arm: {failed}"]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
