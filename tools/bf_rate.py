"""Cost of the beamforming section per kind.

    python tools/bf_rate.py [--batch 16] [--frames 1001] [--mics 6] [--bins 129] [--warmup 10] [--iters 50]
                            [--parent-lib PATH --rounds 5 --out profiles/bf_rate.txt]

One ``misonet_mvdr`` / ``misonet_beamform`` call (covariances, solve, apply: the three launches the fused pass brackets as its
beamforming section) on device-resident complex64 [B, F, M, T] inputs with a dominant rank-1 source, timed with HIP events
on the caller's stream: ``--warmup`` calls, then the median of ``--iters`` single-call timings.  Arms: "abi_mvdr" =
``misonet_mvdr``, the call every build has; "mvdr", "mvdr_mix", "souden", "gev", "gev_ban" = ``misonet_beamform`` with those
options, where the loaded library exports it.  Prints one JSON line.

``--parent-lib``: the library of the parent commit (built from its tree, loaded through MISONET_LIB_PATH).  Then this
process measures nothing itself: it starts ``--rounds`` pairs of fresh child processes, parent and this tree's library in
turn, so that drift hits both alike, and writes the table (per arm: median over the rounds of the children's medians, and
the spread (max - min) / median over the rounds) to ``--out`` besides printing it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = {"mvdr": {}, "mvdr_mix": {"noise": 1}, "souden": {"kind": 1}, "gev": {"kind": 2}, "gev_ban": {"kind": 2, "ban": 1}}


def measure(a):
    import numpy as np
    import torch
    from misonet_amd import _lib
    B, F, M, T = a.batch, a.bins, a.mics, a.frames
    r = np.random.default_rng(7)

    def cn(*shape):
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)) / np.sqrt(2.0)
    src = (cn(B, F, M, 1) * cn(B, F, 1, T) + 0.1 * cn(B, F, M, T)).astype(np.complex64)
    mix = (src + 0.5 * cn(B, F, M, T)).astype(np.complex64)
    src, mix = torch.from_numpy(src).cuda(), torch.from_numpy(mix).cuda()
    out = torch.empty((B, T, F), dtype=torch.complex64, device="cuda")
    L = C.CDLL(_lib.LIB_PATH)                               # a parent library lacks symbols _lib.lib() insists on
    L.misonet_mvdr_workspace_bytes.restype = C.c_longlong
    st = _lib.stream_ptr(src.device)
    calls = {}
    ws = torch.empty(L.misonet_mvdr_workspace_bytes(B, F, M), dtype=torch.uint8, device="cuda")
    p = [C.c_void_p(t.data_ptr()) for t in (src, mix, out, ws)]
    calls["abi_mvdr"] = lambda: L.misonet_mvdr(p[0], p[1], B, F, M, T, C.c_float(1e-6), p[2], p[3], C.c_longlong(ws.numel()), st)
    if hasattr(L, "misonet_beamform"):
        L.misonet_beamform_workspace_bytes.restype = C.c_longlong
        for arm, fields in ARMS.items():
            o = _lib.BfOpts()
            L.misonet_bf_opts_default(C.byref(o))
            for k, v in fields.items():
                setattr(o, k, v)
            w = torch.empty(L.misonet_beamform_workspace_bytes(B, F, M, C.byref(o)), dtype=torch.uint8, device="cuda")
            calls[arm] = (lambda o=o, w=w: L.misonet_beamform(p[0], p[1], B, F, M, T, C.byref(o), p[2], C.c_void_p(w.data_ptr()),
                                                              C.c_longlong(w.numel()), st))
    res = {}
    for arm, fn in calls.items():
        for _ in range(a.warmup):
            if fn() != 0:
                raise RuntimeError(f"{arm}: the library call failed")
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res[arm] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}
    return {"metric": "bf_rate", "device": torch.cuda.get_device_name(0), "lib": os.path.basename(_lib.LIB_PATH),
            "B": B, "F": F, "M": M, "T": T, "warmup": a.warmup, "iters": a.iters, "arms": res}


def alternate(a):
    """parent / this tree in turn, a fresh process each"""
    rows = {"parent": [], "this": []}
    child = [sys.executable, os.path.abspath(__file__)]
    for k in ("batch", "bins", "mics", "frames", "warmup", "iters"):
        child += [f"--{k}", str(getattr(a, k))]
    for _ in range(a.rounds):
        for side in ("parent", "this"):
            env = dict(os.environ)
            env.pop("MISONET_LIB_PATH", None)
            if side == "parent":
                env["MISONET_LIB_PATH"] = os.path.abspath(a.parent_lib)
            r = subprocess.run(child, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"{side} child failed: {r.stderr[-2000:]}")
            rows[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
    head = rows["this"][0]
    lines = [f"bf_rate: one beamforming section (covariances + solve + apply), B={head['B']} F={head['F']} M={head['M']} "
             f"T={head['T']}, {head['device']}",
             f"HIP events, {head['warmup']} warm-ups, median of {head['iters']} calls per process; {a.rounds} rounds of "
             "(parent commit's library, this tree's library) in alternating fresh processes",
             "per arm: median over the rounds [ms], spread = (max - min) / median over the rounds, then the rounds",
             "",
             f"{'library':8s} {'arm':10s} {'median_ms':>10s} {'spread':>8s}  rounds"]
    table = {}
    for side in ("parent", "this"):
        for arm in rows[side][0]["arms"]:
            xs = [r["arms"][arm]["median_ms"] for r in rows[side]]
            med = statistics.median(xs)
            table[f"{side}/{arm}"] = {"median_ms": med, "spread": round((max(xs) - min(xs)) / med, 4), "rounds": xs}
            lines.append(f"{side:8s} {arm:10s} {med:10.4f} {(max(xs) - min(xs)) / med:8.3f}  {xs}")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps({"metric": "bf_rate_ab", "table": table}))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--bins", type=int, default=129)
    ap.add_argument("--mics", type=int, default=6)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="libmisonet_hip.so built from the parent commit: alternate with it")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="with --parent-lib: write the table here (profiles/bf_rate.txt)")
    a = ap.parse_args(argv)
    if a.parent_lib:
        alternate(a)
    else:
        print(json.dumps(measure(a)))


if __name__ == "__main__":
    main()
