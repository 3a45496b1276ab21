#!/usr/bin/env python3
"""Writes tests/golden/g16_stoi.npz: real speech for the STOI / ESTOI tests and the oracle's figures.

    python tools/gen_golden_stoi.py SAMPLE_DIR [--out tests/golden/g16_stoi.npz]

SAMPLE_DIR is the reference project's ``sample/`` directory: ``Clean/<name>_{0,1}.wav`` (the clean sources, any channel
count: channel 0 is kept, float32) and ``MISO3/<name>_{0,1}.wav`` (the separated outputs, mono 24-bit PCM, kept as the
integers the files hold).  CPU only; the figures are those of tests/stoi_ref.py ``explicit`` (estimate = q / 2^23, the
mixture = clean 0 + clean 1).  Arrays: clean float32 [2, n], est_q int32 [2, n], fs, stoi / estoi [2 estimates, 2 references],
stoi_mix / estoi_mix [2], frames / frames_kept [2], margin [2] (dB).
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("sample_dir")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g16_stoi.npz"))
    a = ap.parse_args(argv)
    import stoi_ref
    from misonet_amd.stft import read_wav_pcm24
    import scipy.io.wavfile as wavfile
    names = sorted(m.group(1) for m in (re.match(r"^(.*)_0\.wav$", f) for f in os.listdir(os.path.join(a.sample_dir, "Clean"))) if m)
    if len(names) != 1:
        raise SystemExit(f"expected one recording under {a.sample_dir}/Clean, found {names}")
    name = names[0]
    clean, est_q, rates = [], [], set()
    for s in range(2):
        fs, c = wavfile.read(os.path.join(a.sample_dir, "Clean", f"{name}_{s}.wav"))      # IEEE float files
        if c.dtype.kind != "f":
            raise SystemExit("the clean sources are expected as float wav files")
        clean.append(np.asarray(c, dtype=np.float32).reshape(len(c), -1)[:, 0])
        rates.add(int(fs))
        v, fs = read_wav_pcm24(os.path.join(a.sample_dir, "MISO3", f"{name}_{s}.wav"))
        est_q.append(np.asarray(v).reshape(len(v), -1)[:, 0].astype(np.int32))
        rates.add(int(fs))
    if len(rates) != 1:
        raise SystemExit(f"the files disagree about the rate: {rates}")
    fs = rates.pop()
    n = min(len(x) for x in clean + est_q)
    clean = np.stack([x[:n] for x in clean]).astype(np.float32)
    est_q = np.stack([x[:n] for x in est_q])
    est = est_q.astype(np.float64) / float(1 << 23)
    mix = clean[0].astype(np.float64) + clean[1].astype(np.float64)
    st, es = np.zeros((2, 2)), np.zeros((2, 2))
    frames, kept, margin = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2)
    sm, em = np.zeros(2), np.zeros(2)
    for j in range(2):
        for i in range(2):
            r = stoi_ref.explicit(clean[j], est[i], fs)
            st[i, j], es[i, j] = r["stoi"], r["estoi"]
            frames[j], kept[j], margin[j] = r["frames"], r["frames_kept"], r["margin"]
        r = stoi_ref.explicit(clean[j], mix, fs)
        sm[j], em[j] = r["stoi"], r["estoi"]
        print(f"speaker {j}: STOI {st[j, j]:.6f} ESTOI {es[j, j]:.6f}, {kept[j]} of {frames[j]} frames kept (margin "
              f"{margin[j]:.4f} dB); mixture STOI {sm[j]:.6f} ESTOI {em[j]:.6f}")
    print(f"crossed pairs: STOI {st[0, 1]:.6f} {st[1, 0]:.6f}")
    np.savez_compressed(a.out, clean=clean, est_q=est_q, fs=np.int64(fs), stoi=st, estoi=es, stoi_mix=sm, estoi_mix=em,
                        frames=frames, frames_kept=kept, margin=margin, name=np.array(name))
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, fs {fs}, n {n}")


if __name__ == "__main__":
    main()
