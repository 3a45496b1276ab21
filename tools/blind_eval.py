#!/usr/bin/env python3
"""The blind separator on the real recording the repository carries: a quality figure on real speech that needs no weights.

    python tools/blind_eval.py [--beamform] [--model gauss] [--iterations 20] [--channels K] [--save DIR] [--out blind.json]

Runs ``BlindSeparator.separate_recording`` with the default options on the six-microphone two-speaker mixture of
tests/golden/g8_sample_clean_miso1.npz (``obs_wav_f16``, 4 s at 8 kHz) and scores the int16 result with
``misonet_amd.score.score_waves`` against the speakers' clean images at microphone 0 (tests/golden/g16_stoi.npz, ``clean``):
SI-SDR of the best assignment of outputs to speakers, the mixture's SI-SDR at microphone 0 and the improvement.  Without
``--beamform`` the outputs are the separated images at microphone 0; with it the MVDR on those images.  ``--save DIR`` also
writes ``DIR/g8_{s}.wav``, the files ``tools/score_eval.py`` reads.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--beamform", action="store_true")
    ap.add_argument("--model", default="gauss")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--channels", type=int, default=None)
    ap.add_argument("--save", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import misonet_amd as mz
    from misonet_amd import score
    golden = os.path.join(ROOT, "tests", "golden")
    wav = np.load(os.path.join(golden, "g8_sample_clean_miso1.npz"))["obs_wav_f16"].astype(np.float32)      # [32000, 6]
    clean = np.load(os.path.join(golden, "g16_stoi.npz"))["clean"][:, :wav.shape[0]].astype(np.float32)     # [2, 32000]
    fs = 8000
    sep = mz.BlindSeparator(2, 6, ref_ch=0, blind=dict(model=a.model, iterations=a.iterations, channels=a.channels))
    pcm = sep.separate_recording(wav, save_path=os.path.join(a.save, "g8") if a.save else None, fs=fs, beamform=a.beamform)
    sc = score.score_waves(pcm, clean, wav[:, 0], fs=fs)
    doc = {"metric": "blind_eval", "recording": "g8_sample_clean_miso1", "fs": fs, "samples": int(wav.shape[0]),
           "model": a.model, "iterations": a.iterations, "channels": a.channels or 2, "beamform": bool(a.beamform),
           "perm_best": [int(p) for p in sc.perm_best], "si_sdr": [round(float(v), 2) for v in sc.si_sdr_best],
           "si_sdr_mix": [round(float(v), 2) for v in sc.si_sdr_mix],
           "si_sdr_mean": round(float(np.mean(sc.si_sdr_best)), 2),
           "si_sdr_improvement": round(float(np.mean(sc.si_sdr_best - sc.si_sdr_mix)), 2)}
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
