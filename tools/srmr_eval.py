#!/usr/bin/env python3
"""SRMR of a directory of wav files that has no clean references, on the device.

    python tools/srmr_eval.py DIR [--mix DIR] [--num-spks 2] [--ref-ch 0] [--out srmr.json]

DIR holds ``<name>_{s}.wav`` (what ``enhance_continuous(save_path=...)`` / ``enhance_recording(save_path=...)`` write: 24-bit or
16-bit PCM, mono) or, with ``--num-spks 0``, plain ``<name>.wav`` files of one signal each (channel ``--ref-ch``).  ``--mix DIR``
holds the observations as ``<name>.wav`` (channel ``--ref-ch``): with it every entry also carries the figure of the observation
and the improvement ``srmr_i`` (positive is better).  Prints (or writes) ``{name: Srmr.as_dict()}`` plus ``"mean"``.  The rate
comes from the files: 8 or 16 kHz.  The definition is INTEGRATION.md 4k; the figure has not been compared against the
SRMRToolbox.  Lengths may differ by the padding of the last hop: the common length is measured.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("dir")
    ap.add_argument("--mix", default=None, help="directory of the observations <name>.wav")
    ap.add_argument("--num-spks", type=int, default=2, help="0: plain <name>.wav files of one signal each")
    ap.add_argument("--ref-ch", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from misonet_amd import score
    from score_eval import read_wav
    pat = re.compile(r"^(.*)_0\.wav$" if a.num_spks else r"^(.*)\.wav$")
    names = sorted(m.group(1) for m in map(pat.match, os.listdir(a.dir)) if m)
    if not names:
        raise SystemExit(f"no {'<name>_0.wav' if a.num_spks else '<name>.wav'} in {a.dir}")
    items = {}
    for name in names:
        sigs, rates = [], set()
        for s in range(max(a.num_spks, 1)):
            path = os.path.join(a.dir, f"{name}_{s}.wav" if a.num_spks else f"{name}.wav")
            f32, i16, fs = read_wav(path)
            rates.add(int(fs))
            ch = 0 if a.num_spks else a.ref_ch
            sigs.append(i16[:, ch] if i16 is not None else f32[:, ch])
        if len(rates) != 1:
            raise SystemExit(f"{name}: the files disagree about the rate ({sorted(rates)})")
        mix = None
        if a.mix is not None:
            mix_path = os.path.join(a.mix, f"{name}.wav")
            if not os.path.exists(mix_path):
                raise SystemExit(f"{mix_path} is missing")
            mix = read_wav(mix_path)[0][:, a.ref_ch]
        n = min([len(x) for x in sigs] + ([len(mix)] if mix is not None else []))
        if any(x.dtype != sigs[0].dtype for x in sigs):
            sigs = [x.astype(np.float32) / (32767.0 if x.dtype == np.int16 else 1.0) for x in sigs]
        items[name] = score.srmr_waves(np.stack([x[:n] for x in sigs]), mix[:n] if mix is not None else None, fs=min(rates))
    doc = {name: v.as_dict() for name, v in items.items()}
    doc["mean"] = score.srmr_mean_of(list(items.values()))
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
