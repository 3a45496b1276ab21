"""Cost of step 5 of the fused pass with a joint multi-speaker beamformer (LCMV, SDW-MWF, rank-1 MWF), against "souden" and the
reference's MVDR.

    python tools/jbf_rate.py [--batch 16] [--speakers 2] [--frames 1001] [--mics 6] [--bins 129] [--warmup 5] [--iters 20]
                             [--rounds 5] [--fused-iters 10] [--out profiles/jbf_rate.txt]

Step 5 alone.  At the bench geometry step 5 beamforms batch x speakers = 32 (item, speaker) pairs of 129 bins.  The per-speaker
kinds take one source per item, so those arms time ONE ``misonet_beamform`` / ``misonet_mvdr`` call on batch x speakers items
(as tools/wpd_rate.py does); the joint arms time ONE ``misonet_beamform_joint`` call on batch items of ``speakers`` sources:
batch x 129 workgroups of ``jbf_bin_k`` that read the mixture once for all speakers.  The same device-resident complex64 data
serves every arm (per item a rank-1 source per speaker plus noise; the mixture is their sum plus noise), with HIP events on the
caller's stream.  All arms run in this one process, in turn, ``--rounds`` times: ``--warmup`` calls, then the median of
``--iters`` single-call timings; the table has, per arm, the median over the rounds of those medians and the spread
(max - min) / median over the rounds.

The fused step.  ``Enhancer.enhance`` on seed weights and synthetic utterances at the same geometry, with the default step 5 and
with each joint kind: per arm ``--warmup`` passes, then ``--fused-iters`` passes timed as a whole with HIP events (the pass),
then ``--fused-iters`` passes under the library's per-launch profiler (``misonet_profile_begin`` / ``misonet_profile_end``): the
time of the launches of step 5 per pass.  Prints one JSON line and writes the table to ``--out``.
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

JOINT = (("lcmv", dict()), ("mwf", dict(mu=1.0)), ("r1mwf", dict(mu=1.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--speakers", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--bins", type=int, default=129)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fused-iters", type=int, default=10, help="0: leave the fused arms out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jbf_rate.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from misonet_amd import _lib
    from misonet_amd.beamform import JointBeamformer
    B, S, F, M, T = a.batch, a.speakers, a.bins, a.mics, a.frames
    g = torch.Generator(device="cuda")
    g.manual_seed(7)

    def cn(*shape):
        return torch.view_as_complex(torch.randn(*shape, 2, generator=g, device="cuda") * 0.5 ** 0.5)
    src = (cn(B, S, F, M, 1) * cn(B, S, F, 1, T) + 0.1 * cn(B, S, F, M, T)).contiguous()
    mix = (src.sum(dim=1) + 0.3 * cn(B, F, M, T)).contiguous()
    src1 = src.reshape(B * S, F, M, T)                                     # one source per item: item (b, s)
    mix1 = mix[:, None].expand(B, S, F, M, T).reshape(B * S, F, M, T).contiguous()
    out = torch.empty((B, S, T, F), dtype=torch.complex64, device="cuda")
    L = _lib.lib()
    st = _lib.stream_ptr(src.device)
    calls, keep = {}, []

    def ws_of(n):
        if n < 0:
            raise RuntimeError("the size function refused the options")
        keep.append(torch.empty(max(int(n), 8), dtype=torch.uint8, device="cuda"))
        return keep[-1]
    N = B * S
    w0 = ws_of(L.misonet_mvdr_workspace_bytes(N, F, M))
    calls["mvdr"] = lambda: L.misonet_mvdr(src1.data_ptr(), mix1.data_ptr(), N, F, M, T, 1e-6, out.data_ptr(), w0.data_ptr(),
                                           w0.numel(), st)
    ob = _lib.BfOpts()
    L.misonet_bf_opts_default(C.byref(ob))
    ob.kind = 1
    w1 = ws_of(L.misonet_beamform_workspace_bytes(N, F, M, C.byref(ob)))
    calls["souden"] = lambda: L.misonet_beamform(src1.data_ptr(), mix1.data_ptr(), N, F, M, T, C.byref(ob), out.data_ptr(),
                                                 w1.data_ptr(), w1.numel(), st)
    jopts = {}
    for kind, kw in JOINT:
        o = JointBeamformer(kind=kind, **kw).validate(M, S).c_opts()
        w = ws_of(L.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(o)))
        jopts[kind] = (o, w)
        calls[kind] = (lambda o=o, w=w: L.misonet_beamform_joint(src.data_ptr(), mix.data_ptr(), B, S, F, M, T, C.byref(o),
                                                                 out.data_ptr(), w.data_ptr(), w.numel(), st))

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
    failed = {}
    for kind, (o, w) in jopts.items():
        bad = torch.empty((B, S, F), dtype=torch.int32, device="cuda")
        _lib.check(L.misonet_beamform_joint_debug(w.data_ptr(), B, S, F, M, C.byref(o), None, None, bad.data_ptr(), st))
        failed[kind] = int(bad.sum().item())
    res = {arm: {"median_ms": round(statistics.median(v), 4), "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
           for arm, v in meds.items()}
    ratios = {kind: round(res[kind]["median_ms"] / res["souden"]["median_ms"], 3) for kind, _ in JOINT}

    fused = {}
    if a.fused_iters > 0:
        if (M, S, F) != (6, 2, 129):
            raise SystemExit("the fused arms use the seed networks: --mics 6 --speakers 2 --bins 129 (or --fused-iters 0)")
        import misonet_amd as mz
        from misonet_amd import stft as St
        from misonet_amd import weights as W
        m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m1.load_state_dict(W.make_state_dict(W.miso1_spec(), 0))
        m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m3.load_state_dict(W.make_state_dict(W.miso3_spec(), 1))
        enh = mz.Enhancer(m1.eval(), m3.eval(), num_spks=2, ref_ch=0)
        wav = np.stack([W.synthetic_utterance(b, 64 * (T - 1))[0] for b in range(B)]).astype(np.float32)     # [B, n, 6]
        fmix = St.stft_hip(torch.from_numpy(wav).cuda()).contiguous()                                        # [B, 6, T, 129]
        arms = [("mvdr", None)] + [(kind, JointBeamformer(kind=kind, **kw)) for kind, kw in JOINT]
        for arm, bf in arms:
            enh.set_beamformer(bf)
            for _ in range(a.warmup):
                enh.enhance(fmix)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.fused_iters):                             # the whole pass with the profiler off
                enh.enhance(fmix)
            e1.record()
            e1.synchronize()
            _lib.check(L.misonet_profile_begin(a.fused_iters * 400))
            for _ in range(a.fused_iters):
                enh.enhance(fmix)
            ms, cnt = (C.c_double * 4)(), (C.c_longlong * 4)()
            _lib.check(L.misonet_profile_end(ms, cnt))
            fused[arm] = {"step5_ms_per_pass": round(ms[2] / a.fused_iters, 4), "step5_records_per_pass": cnt[2] // a.fused_iters,
                          "pass_ms": round(e0.elapsed_time(e1) / a.fused_iters, 3)}

    doc = {"metric": "jbf_rate", "device": torch.cuda.get_device_name(0), "batch": B, "speakers": S, "F": F, "M": M, "T": T,
           "workgroups_joint": B * F, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds, "failed_bins": failed, "arms": res,
           "over_souden": ratios, "fused": fused}
    print(json.dumps(doc))
    lines = [f"step 5 at batch {B} x {S} speakers, F {F}, M {M}, T {T} on {doc['device']}",
             f"per-speaker arms: one call on {N} items; joint arms: one call on {B} items of {S} sources ({B * F} workgroups of "
             "jbf_bin_k)",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then the median of {a.iters} "
             "single-call timings (HIP events); median over the rounds, spread = (max - min) / median over the rounds",
             "", f"{'arm':<8} {'median ms':>10} {'spread':>8} {'/ souden':>9}"]
    lines += [f"{arm:<8} {r['median_ms']:>10.4f} {r['spread']:>8.4f} {r['median_ms'] / res['souden']['median_ms']:>9.3f}"
              for arm, r in res.items()]
    lines += ["", "(item, speaker, bin) that failed in the joint arms: " + ", ".join(f"{k} {v}" for k, v in failed.items())]
    if fused:
        lines += ["", f"the fused pass (Enhancer.enhance, seed weights, synthetic utterances) at the same geometry: {a.warmup} warm-up "
                  f"passes, {a.fused_iters} passes timed as a whole (pass ms), then {a.fused_iters} passes under the per-launch profiler (step 5 "
                  "= the launches of the beamformer)",
                  "", f"{'step 5':<8} {'step 5 ms':>10} {'records':>9} {'pass ms':>9}"]
        lines += [f"{arm:<8} {r['step5_ms_per_pass']:>10.4f} {r['step5_records_per_pass']:>9d} {r['pass_ms']:>9.3f}"
                  for arm, r in fused.items()]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
