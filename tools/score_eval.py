#!/usr/bin/env python3
"""Scores a directory of separated wav files against a directory of clean ones, on the device.

    python tools/score_eval.py EST_DIR REF_DIR [--num-spks 2] [--ref-ch 0] [--mix-dir DIR] [--out scores.json] [--bss [--filt-len 512]] [--stoi] [--reverb] [--srmr]

EST_DIR holds ``<name>_{s}.wav`` (what ``enhance_recording(save_path=...)`` / ``inference`` write: 24-bit or 16-bit PCM, mono);
REF_DIR holds the clean sources under the same names (``<name>_{s}.wav``, any channel count: channel ``--ref-ch`` is used)
and, there or in ``--mix-dir``, the observation as ``<name>.wav`` (optional: without it no SI-SDR improvement is reported).
Prints (or writes) the JSON ``Enhancer.inference(..., score=True)`` writes: ``{name: Score.as_dict()}`` plus ``"mean"``.
``--bss`` adds BSS-eval SDR, SIR and SAR (``BssEval.as_dict()``, INTEGRATION.md 4e, filters of ``--filt-len`` taps) as a
``"bss"`` entry of every recording and of ``"mean"``; ``--stoi`` adds STOI and ESTOI (``Stoi.as_dict()``, INTEGRATION.md 4f, at
the rate the files carry: 8, 10 or 16 kHz) as a ``"stoi"`` entry likewise; ``--reverb`` adds the cepstral distance, the
log-likelihood ratio and the frequency-weighted segmental SNR (``Reverb.as_dict()``, INTEGRATION.md 4j, at the rate the files
carry: 8 or 16 kHz) as a ``"reverb"`` entry; ``--srmr`` adds the speech-to-reverberation modulation energy ratio of the
estimates and of the observation (``Srmr.as_dict()``, INTEGRATION.md 4k, the figure that uses no reference; 8 or 16 kHz) as a
``"srmr"`` entry; without the flags the output is what it always was.  For a directory that has no references at all use
tools/srmr_eval.py.
Definitions: INTEGRATION.md 4d.  Lengths may differ by the padding of the last hop: the common length is scored.
"""
import argparse
import json
import os
import re
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_wav(path):
    """PCM wav (16 or 24 bit) -> (float32 [n, ch] in [-1, 1), int16 [n, ch] when the file holds int16 << 8 or int16, fs)"""
    from misonet_amd.stft import read_wav_pcm24
    with wave.open(path, "rb") as w:
        width, ch, fs, n = w.getsampwidth(), w.getnchannels(), w.getframerate(), w.getnframes()
        raw = w.readframes(n) if width == 2 else None
    if width == 3:
        v, fs = read_wav_pcm24(path)
        i16 = (v >> 8).astype(np.int16) if not np.any(v & 0xFF) else None
        return (v / float(1 << 23)).astype(np.float32), i16, fs
    if width == 2:
        q = np.frombuffer(raw, dtype="<i2").reshape(n, ch)
        return (q / 32768.0).astype(np.float32), q.copy(), fs
    raise ValueError(f"{path}: {8 * width}-bit PCM is not supported (16 or 24)")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("est_dir")
    ap.add_argument("ref_dir")
    ap.add_argument("--num-spks", type=int, default=2)
    ap.add_argument("--ref-ch", type=int, default=0)
    ap.add_argument("--mix-dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bss", action="store_true", help="also BSS-eval SDR / SIR / SAR")
    ap.add_argument("--filt-len", type=int, default=512, help="taps of the BSS-eval projection filters")
    ap.add_argument("--stoi", action="store_true", help="also STOI and ESTOI (the rate comes from the files)")
    ap.add_argument("--reverb", action="store_true", help="also cepstral distance, LLR and fwSegSNR (the rate comes from the files)")
    ap.add_argument("--srmr", action="store_true", help="also SRMR of the estimates and the observation (the rate comes from the files)")
    a = ap.parse_args(argv)
    from misonet_amd import score
    pat = re.compile(r"^(.*)_0\.wav$")
    names = sorted(m.group(1) for m in map(pat.match, os.listdir(a.est_dir)) if m)
    if not names:
        raise SystemExit(f"no <name>_0.wav in {a.est_dir}")
    scores, evals, stois, reverbs, srmrs = {}, {}, {}, {}, {}
    for name in names:
        est, ref, rates = [], [], set()
        for s in range(a.num_spks):
            f32, i16, fs = read_wav(os.path.join(a.est_dir, f"{name}_{s}.wav"))
            rates.add(int(fs))
            est.append(i16[:, 0] if i16 is not None else f32[:, 0])       # the library's own files: int16, scored as such
            ref.append(read_wav(os.path.join(a.ref_dir, f"{name}_{s}.wav"))[0][:, a.ref_ch])
        mix_path = os.path.join(a.mix_dir or a.ref_dir, f"{name}.wav")
        mix = read_wav(mix_path)[0][:, a.ref_ch] if os.path.exists(mix_path) else None
        n = min([len(x) for x in est + ref] + ([len(mix)] if mix is not None else []))
        if any(x.dtype != est[0].dtype for x in est):
            est = [x.astype(np.float32) / (32767.0 if x.dtype == np.int16 else 1.0) for x in est]
        scores[name] = score.score_waves(np.stack([x[:n] for x in est]), np.stack([x[:n] for x in ref]),
                                         mix[:n] if mix is not None else None)
        if a.bss:
            evals[name] = score.bss_eval_waves(np.stack([x[:n] for x in est]), np.stack([x[:n] for x in ref]),
                                               mix[:n] if mix is not None else None, filt_len=a.filt_len)
        if a.stoi:
            if len(rates) != 1:
                raise SystemExit(f"{name}: the estimates disagree about the rate ({sorted(rates)})")
            stois[name] = score.stoi_waves(np.stack([x[:n] for x in est]), np.stack([x[:n] for x in ref]),
                                           mix[:n] if mix is not None else None, fs=min(rates))
        if a.reverb:
            if len(rates) != 1:
                raise SystemExit(f"{name}: the estimates disagree about the rate ({sorted(rates)})")
            reverbs[name] = score.reverb_waves(np.stack([x[:n] for x in est]), np.stack([x[:n] for x in ref]),
                                               mix[:n] if mix is not None else None, fs=min(rates))
        if a.srmr:
            if len(rates) != 1:
                raise SystemExit(f"{name}: the estimates disagree about the rate ({sorted(rates)})")
            srmrs[name] = score.srmr_waves(np.stack([x[:n] for x in est]), mix[:n] if mix is not None else None, fs=min(rates))
    doc = {name: sc.as_dict() for name, sc in scores.items()}
    doc["mean"] = score.mean_of(list(scores.values()))
    if a.bss:
        for name, ev in evals.items():
            doc[name]["bss"] = ev.as_dict()
        doc["mean"]["bss"] = score.bss_mean_of(list(evals.values()))
    if a.stoi:
        for name, st in stois.items():
            doc[name]["stoi"] = st.as_dict()
        doc["mean"]["stoi"] = score.stoi_mean_of(list(stois.values()))
    if a.reverb:
        for name, rv in reverbs.items():
            doc[name]["reverb"] = rv.as_dict()
        doc["mean"]["reverb"] = score.reverb_mean_of(list(reverbs.values()))
    if a.srmr:
        for name, sv in srmrs.items():
            doc[name]["srmr"] = sv.as_dict()
        doc["mean"]["srmr"] = score.srmr_mean_of(list(srmrs.values()))
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
