#!/usr/bin/env python3
"""The weight-free chain on simulated scenes: what every front end does to reverberant, noisy two-speaker mixtures whose early
images are known exactly.

    python tools/scenario_eval.py [--scenes 8] [--seed 0] [--rir-len 4096] [--ref-ch 0] [--arms all|quick]
                                  [--out profiles/scenario_eval.txt]

Scenes (``misonet_amd.room.simulate``), seeded: a room of 5-8 x 4-6 x 2.5-3 m, a six-microphone circular array of 5 cm radius,
two sources 1-2 m from its centre and at least 30 degrees apart, a nominal RT60 from {0.2, 0.4, 0.6} s in turn (Sabine; the T30 read
off each RIR by Schroeder integration on the host is printed beside it), sensor noise at 20-30 dB SNR, the dry speech of
tests/golden/g16_stoi.npz (8 s, 8 kHz).  Nothing outside the repository is read.

Front ends, all through ``BlindSeparator.separate_recording``: the AuxIVA image at ``ref_ch``; AuxIVA followed by each
beamformer kind (MVDR, MPDR, Souden, GEV with BAN, WPD, LCMV, SDW-MWF, r1-MWF); the same with WPE (``dereverb_wav``) in front;
online WPE (``dereverb_wav(online=True)``: causal, frame-recursive) in front of AuxIVA alone and of MVDR and LCMV; the beamformer arms with the guided cACGMM between AuxIVA and the beamformer;
online AuxIVA (``separate_recording(online=True)``: causal, frame-recursive, M sources at M microphones) on 2 of the 6 microphones
(``[0:6:3]``) and on all 6 with the two strongest rows kept, alone (``oiva``, ``oiva6``) and behind the online WPE stream
(``owpe+oiva``, ``owpe+oiva6``), and with the online beamformer on the images of the online AuxIVA
(``separate_recording(online=True, beamform=OnlineBeamformer())``, its defaults: ``oiva+obf``, ``oiva6+obf``, ``owpe+oiva6+obf``);
the online AuxIVA for K = 2 sources at all 6 microphones (``online=dict(num_src=2)``: two rows out, no choice after the fact), alone
(``overiva``), behind the online WPE stream (``owpe+overiva``) and with the online beamformer behind it (``owpe+overiva+obf``).
Every output is scored against the EARLY images at
``ref_ch`` (the direct path and the first 50 ms) on the device: SI-SDR of the best assignment and its improvement over the
mixture, BSS-eval SDR, STOI, cepstral distance, LLR, fwSegSNR and SRMR, averaged over the speakers and the scenes.  No figure is
required to come out any particular way: the table is what was measured, a front end that makes things worse included.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS = 8000
RT60S = (0.2, 0.4, 0.6)


def draw_scene(rng, i):
    """(dim, nominal rt60, src [2, 3], mic [6, 3], snr_db) of scene i; the nominal RT60s take turns"""
    dim = np.array([rng.uniform(5, 8), rng.uniform(4, 6), rng.uniform(2.5, 3)])
    rt60 = RT60S[i % len(RT60S)]
    while True:
        centre = np.array([rng.uniform(0.3, 0.7) * dim[0], rng.uniform(0.3, 0.7) * dim[1], rng.uniform(1.0, 1.5)])
        az = rng.uniform(0, 2 * np.pi, 2)
        dist = rng.uniform(1.0, 2.0, 2)
        src = centre + np.stack([dist * np.cos(az), dist * np.sin(az), rng.uniform(-0.3, 0.3, 2)], 1)
        apart = abs((az[0] - az[1] + np.pi) % (2 * np.pi) - np.pi)
        if apart >= np.pi / 6 and (src > 0.3).all() and (src < dim - 0.3).all():
            break
    ang = 2 * np.pi * np.arange(6) / 6
    mic = centre + np.stack([0.05 * np.cos(ang), 0.05 * np.sin(ang), np.zeros(6)], 1)
    return dim, rt60, src, mic, float(rng.uniform(20, 30))


def arms(which):
    """name -> (WPE in front: False, True or "online", beamform, BlindSeparator keywords)"""
    from misonet_amd.beamform import Beamformer, JointBeamformer
    bfs = {"mvdr": Beamformer(kind="mvdr"), "mpdr": Beamformer(kind="mvdr", noise="mix"), "souden": Beamformer(kind="souden"),
           "gev+ban": Beamformer(kind="gev", ban=True), "wpd": Beamformer(kind="wpd"), "lcmv": JointBeamformer(kind="lcmv"),
           "sdw-mwf": JointBeamformer(kind="mwf"), "r1-mwf": JointBeamformer(kind="r1mwf")}
    if which == "quick":
        bfs = {k: bfs[k] for k in ("mvdr", "lcmv")}
    out = {"auxiva": (False, False, {})}
    out.update({f"auxiva+{k}": (False, True, dict(beamformer=b)) for k, b in bfs.items()})
    out["wpe+auxiva"] = (True, False, {})
    out.update({f"wpe+auxiva+{k}": (True, True, dict(beamformer=b)) for k, b in bfs.items()})
    out["owpe+auxiva"] = ("online", False, {})
    out.update({f"owpe+auxiva+{k}": ("online", True, dict(beamformer=bfs[k])) for k in ("mvdr", "lcmv")})
    out.update({f"auxiva+cacgmm+{k}": (False, True, dict(beamformer=b, refine=True)) for k, b in bfs.items()})
    # the causal chain: "mics" = the microphones (and so the rows) of the online AuxIVA, "owpe" = the online WPE stream in front
    out["oiva"] = (False, False, dict(mics=2))
    out["owpe+oiva"] = (False, False, dict(mics=2, owpe=True))
    out["oiva6"] = (False, False, dict(mics=6))
    out["owpe+oiva6"] = (False, False, dict(mics=6, owpe=True))
    out["oiva+obf"] = (False, False, dict(mics=2, obf=True))
    out["oiva6+obf"] = (False, False, dict(mics=6, obf=True))
    out["owpe+oiva6+obf"] = (False, False, dict(mics=6, owpe=True, obf=True))
    # the same chain with K = 2 sources at the 6 microphones ("src"): two rows out, nothing chosen after the fact
    out["overiva"] = (False, False, dict(mics=6, src=2))
    out["owpe+overiva"] = (False, False, dict(mics=6, src=2, owpe=True))
    out["owpe+overiva+obf"] = (False, False, dict(mics=6, src=2, owpe=True, obf=True))
    return out


COLS = ("si_sdr", "si_sdri", "sdr", "stoi", "cd", "llr", "fwsegsnr", "srmr")


def score_all(pcm, ref, mix):
    """the eight columns of one output, each the mean over the speakers; and the mixture's own"""
    from misonet_amd import score as SC
    a = SC.score_waves(pcm, ref, mix, fs=FS)
    b = SC.bss_eval_waves(pcm, ref, mix)
    c = SC.stoi_waves(pcm, ref, mix, fs=FS)
    d = SC.reverb_waves(pcm, ref, mix, fs=FS)
    e = SC.srmr_waves(pcm, mix, fs=FS)
    m = lambda v: float(np.nanmean(np.asarray(v, np.float64)))
    got = dict(si_sdr=m(a.si_sdr_best), si_sdri=m(a.si_sdr_best - a.si_sdr_mix), sdr=m(b.sdr_best), stoi=m(c.stoi_best),
               cd=m(d.cd_best), llr=m(d.llr_best), fwsegsnr=m(d.fwsegsnr_best), srmr=m(e.srmr))
    base = dict(si_sdr=m(a.si_sdr_mix), si_sdri=0.0, sdr=m(b.sdr_mix), stoi=m(c.stoi_mix), cd=m(d.cd_mix), llr=m(d.llr_mix),
                fwsegsnr=m(d.fwsegsnr_mix), srmr=float(e.srmr_mix))
    return got, base


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rir-len", type=int, default=4096)
    ap.add_argument("--ref-ch", type=int, default=0)
    ap.add_argument("--arms", choices=("all", "quick"), default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenario_eval.txt"))
    a = ap.parse_args(argv)
    import torch
    import misonet_amd as mz
    from misonet_amd import room as RM
    from misonet_amd.dereverb import dereverb_wav
    dry = np.load(os.path.join(ROOT, "tests", "golden", "g16_stoi.npz"))["clean"].astype(np.float32)          # [2, 64059]
    rng = np.random.default_rng(a.seed)
    table = arms(a.arms)
    rows = {name: [] for name in ["mixture"] + list(table)}
    by_rt = {name: {rt: [] for rt in RT60S} for name in rows}
    head, failed = [], {}
    t_start = time.time()
    for i in range(a.scenes):
        dim, rt60, src, mic, snr = draw_scene(rng, i)
        room = RM.Room(tuple(dim), rt60=rt60)
        sc = RM.simulate(dry, room, src, mic, FS, a.rir_len, snr_db=snr, seed=a.seed * 1000 + i)
        t30 = [float(np.mean([RM.schroeder_t30(sc.rir[s, m], FS) for m in range(mic.shape[0])])) for s in range(src.shape[0])]
        late = 10 * np.log10((sc.early.astype(np.float64) ** 2).sum() /
                             max(((sc.images.astype(np.float64) - sc.early) ** 2).sum(), 1e-300))
        head.append(f"scene {i}: room {dim[0]:.2f} x {dim[1]:.2f} x {dim[2]:.2f} m, nominal RT60 {rt60:.1f} s (beta "
                    f"{room.betas()[0]:.3f}), T30 read off the RIRs {t30[0]:.3f} / {t30[1]:.3f} s, early-to-late {late:.1f} dB, "
                    f"SNR {snr:.1f} dB, flags {int(np.bitwise_or.reduce(sc.fail.ravel()))}")
        print(head[-1], flush=True)
        ref = np.ascontiguousarray(sc.early[:, :, a.ref_ch])
        mixture = np.ascontiguousarray(sc.wav[:, a.ref_ch])
        dewav = {}
        for name, (wpe, beamform, kw) in table.items():
            wav = sc.wav
            if wpe:
                if wpe not in dewav:
                    dewav[wpe] = dereverb_wav(sc.wav, fs=FS, online=True if wpe == "online" else None)
                wav = dewav[wpe]
            try:
                if "mics" in kw:
                    sep = mz.BlindSeparator(2, kw["mics"], ref_ch=a.ref_ch)
                    online = dict(num_src=kw["src"]) if "src" in kw else True
                    pcm = sep.separate_recording(wav, fs=FS, online=online, dereverb=True if kw.get("owpe") else None,
                                                 beamform=mz.OnlineBeamformer() if kw.get("obf") else None)
                else:
                    sep = mz.BlindSeparator(2, 6, ref_ch=a.ref_ch, **kw)
                    pcm = sep.separate_recording(wav, fs=FS, beamform=beamform)
                got, base = score_all(pcm, ref, mixture)
            except Exception as exc:                       # an arm that cannot run is a finding to print, not a reason to stop
                failed[name] = f"{type(exc).__name__}: {exc}"
                continue
            rows[name].append(got)
            by_rt[name][rt60].append(got["si_sdri"])
            if name == "auxiva":
                rows["mixture"].append(base)
                by_rt["mixture"][rt60].append(0.0)
        torch.cuda.synchronize()
        print(f"  scene {i} done, {time.time() - t_start:.0f} s so far", flush=True)
    mean = lambda name, col: float(np.mean([r[col] for r in rows[name]])) if rows[name] else float("nan")
    doc = {"metric": "scenario_eval", "scenes": a.scenes, "seed": a.seed, "rir_len": a.rir_len, "fs": FS, "ref_ch": a.ref_ch,
           "device": torch.cuda.get_device_name(0), "arms": {n: {c: round(mean(n, c), 3) for c in COLS} for n in rows},
           "failed": failed}
    print(json.dumps(doc))
    lines = [f"simulated scenes: {a.scenes} (seed {a.seed}), two speakers (tests/golden/g16_stoi.npz, {dry.shape[1]} samples at "
             f"{FS} Hz), six microphones on a 5 cm circle, RIRs of {a.rir_len} taps, on {doc['device']}",
             f"every output scored against the EARLY image (direct path + 50 ms) at microphone {a.ref_ch}; mean over the two "
             "speakers (best assignment) and the scenes; CD and LLR: smaller is better", ""] + head
    lines += ["", f"{'front end':<26}" + "".join(f"{c:>10}" for c in COLS) + "   SI-SDRi at nominal RT60 0.2 / 0.4 / 0.6 s"]
    for n in rows:
        rt = " / ".join(f"{np.mean(v):6.2f}" if v else "   n/a" for v in by_rt[n].values())
        lines.append(f"{n:<26}" + "".join(f"{mean(n, c):>10.3f}" for c in COLS) + "   " + rt)
    lines += [f"FAILED {n}: {msg}" for n, msg in failed.items()]
    lines += ["", "as measured; nothing here was tuned, and no figure was required to come out any particular way"]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
