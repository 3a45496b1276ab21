#!/usr/bin/env python3
"""Source localisation on simulated scenes whose source directions are known exactly: the angular error of SRP, SRP-PHAT and
MUSIC in four settings.

    python tools/doa_eval.py [--scenes 8] [--seed 0] [--rir-len 4096] [--out profiles/doa_eval.txt]

Scenes: the seeded scenes of tools/scenario_eval.py (rooms of 5-8 x 4-6 x 2.5-3 m, six microphones on a 5 cm circle, two
sources 1-2 m away and at least 30 degrees apart, nominal RT60 0.2 / 0.4 / 0.6 s in turn, 20-30 dB SNR, the dry speech of
tests/golden/g16_stoi.npz at 8 kHz), and the same geometries once more with beta = 0 (anechoic).  Candidates: 360 azimuths in
the array's plane, far-field delays; bins 8 .. 120 (250 .. 3750 Hz); peaks kept 20 degrees apart.  A planar array cannot tell
+e from -e degrees of elevation and barely resolves small elevations, so the grid has none: the truth is the source's direction
projected into the array's plane (the sources stand within about 17 degrees of it).  Settings:

  mixture          the mixture's map with S = 2 peaks
  auxiva images    AuxIVA's two images, each its own map with S = 1
  cacgmm masks     the mixture weighted by the cACGMM masks (initialised from AuxIVA's images): one map per speaker class, S = 1
  wpe + mixture    the mixture behind WPE dereverberation, S = 2

The error is the angle between a found direction and a true azimuth in degrees, the found peaks matched to the truths by the
better assignment (a missing peak counts 180).  It is a table, as measured: no figure is required to come out any particular
way."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS = 8000
BINS = (8, 120)
KINDS = ("srp", "srp_phat", "music")
SETTINGS = ("mixture", "auxiva images", "cacgmm masks", "wpe + mixture")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rir-len", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doa_eval.txt"))
    a = ap.parse_args(argv)
    import torch
    from scenario_eval import RT60S, draw_scene
    from misonet_amd import localize as LZ
    from misonet_amd import room as RM
    from misonet_amd import stft as S
    from misonet_amd.blind import auxiva
    from misonet_amd.dereverb import dereverb_wav
    from misonet_amd.refine import cacgmm, masks_from_estimates
    if not torch.cuda.is_available():
        raise SystemExit("doa_eval needs the GPU")
    dry = np.load(os.path.join(ROOT, "tests", "golden", "g16_stoi.npz"))["clean"].astype(np.float32)
    dirs = LZ.directions(360)
    sep = 2.0 * np.sin(np.radians(10.0))
    rng = np.random.default_rng(a.seed)
    groups = ["anechoic"] + [f"RT60 {rt:.1f} s" for rt in RT60S]
    errs = {g: {s: {k: [] for k in KINDS} for s in SETTINGS} for g in groups}
    head = []

    def spec_of(wav):
        sig = torch.from_numpy(np.ascontiguousarray(wav, np.float32)).cuda()
        sig = torch.nn.functional.pad(sig, (0, 0, 0, (-sig.shape[0]) % S.HOP))[None].contiguous()
        return S.stft_hip(sig).permute(0, 3, 1, 2).contiguous()          # [1, F, M, T]

    for i in range(a.scenes):
        dim, rt60, src, mic, snr = draw_scene(rng, i)
        centre = mic.mean(axis=0)
        full = (src - centre) / np.linalg.norm(src - centre, axis=1, keepdims=True)
        truth = full * np.array([1.0, 1.0, 0.0])
        truth /= np.linalg.norm(truth, axis=1, keepdims=True)
        tau = LZ.far_field_delays(mic, dirs)
        for group, room in ((f"RT60 {rt60:.1f} s", RM.Room(tuple(dim), rt60=rt60)), ("anechoic", RM.Room(tuple(dim), beta=(0.0,) * 6))):
            sc = RM.simulate(dry, room, src, mic, FS, a.rir_len, snr_db=snr, seed=a.seed * 1000 + i)
            mix = spec_of(sc.wav)
            images = auxiva(mix, 2)                                       # [1, 2, F, M, T]
            masks = cacgmm(mix, masks_from_estimates(images, mix))[:, :2].contiguous()      # the two speaker classes
            dewav = dereverb_wav(sc.wav, fs=FS)
            demix = spec_of(dewav if isinstance(dewav, np.ndarray) else dewav.cpu().numpy())
            for kind in KINDS:
                kw = dict(kind=kind, bins=BINS, min_sep=sep)
                runs = {"mixture": LZ.localize(mix, tau, dirs, FS, num_src=2, **kw).peak[0, 0, 0],
                        "auxiva images": LZ.localize(images, tau, dirs, FS, num_src=1, **kw).peak[0, :, 0, 0, 0],
                        "cacgmm masks": LZ.localize(mix, tau, dirs, FS, num_src=1, weight=masks, **kw).peak[0, :, 0, 0],
                        "wpe + mixture": LZ.localize(demix, tau, dirs, FS, num_src=2, **kw).peak[0, 0, 0]}
                for setting, peak in runs.items():
                    e = LZ.angular_error(dirs, peak.cpu().numpy(), truth)
                    errs[group][setting][kind].extend(float(v) for v in e)
            head.append(f"scene {i} {group}: room {dim[0]:.2f} x {dim[1]:.2f} x {dim[2]:.2f} m, SNR {snr:.1f} dB, true azimuth / "
                        "elevation " + ", ".join(f"{np.degrees(np.arctan2(t[1], t[0])) % 360:.1f} / {np.degrees(np.arcsin(t[2])):.1f}"
                                                 for t in full))
            print(head[-1], flush=True)
    doc = {"metric": "doa_eval", "scenes": a.scenes, "seed": a.seed, "fs": FS, "device": torch.cuda.get_device_name(0),
           "mean_worst": {g: {s: {k: [round(float(np.mean(v)), 2), round(float(np.max(v)), 2)] for k, v in d.items() if v}
                              for s, d in sd.items()} for g, sd in errs.items()}}
    print(json.dumps(doc))
    lines = [f"source localisation on {a.scenes} simulated scenes (seed {a.seed}) and the same geometries with beta = 0, two speakers, "
             f"six microphones on a 5 cm circle, {FS} Hz, RIRs of {a.rir_len} taps, on {doc['device']}",
             f"360 candidate azimuths in the array's plane, bins {BINS[0]} .. {BINS[1]}, peaks 20 degrees apart; azimuth error in degrees, "
             "mean / worst over the sources of the group's scenes", ""] + head + [""]
    for g in groups:
        n = len(errs[g]["mixture"]["srp"]) // 2
        lines.append(f"{g} ({n} scenes)" + " " * max(1, 22 - len(g) - len(str(n))) + "".join(f"{k:>20}" for k in KINDS))
        for s in SETTINGS:
            cells = [f"{np.mean(v):8.2f} / {np.max(v):6.2f}" if v else "n/a" for v in (errs[g][s][k] for k in KINDS)]
            lines.append(f"  {s:<28}" + "".join(f"{c:>20}" for c in cells))
        lines.append("")
    lines.append("as measured; nothing here was tuned, and no figure was required to come out any particular way")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
