"""Cost of the streaming resampler per call (``misonet_resample_stream``), beside three yardsticks timed in the same process: the
``stft stream`` call of the same block, ``misonet_resample`` of the whole recording in one call, and ``StreamSeparator`` with and
without ``fs_in`` / ``fs_out="in"``.

    python tools/resample_stream_rate.py [--warmup 3] [--iters 10] [--rounds 3] [--out profiles/resample_stream_rate.txt]

For 48 -> 16, 44.1 -> 16 and 16 -> 48 kHz, M = 2 and 6 channels (one recording, float32, time-major) and blocks that give 64, 256
and 1024 samples at the model's rate (16 kHz; for 16 -> 48 kHz the block itself is at the model's rate): one
``ResampleStream.process_into`` of a block on a stream in progress (each timed call advances the host's sample count, so the phase
moves as it does in use).  The offline arm resamples the 32000 model-rate samples (501 frames) of the recording in one
``misonet_resample`` call.  ``StreamSeparator`` (``dereverb=True, separate=True, beamform=True``, int16 out) takes the same block
at 16 kHz without rates and at 48 / 44.1 kHz with ``fs_in`` and ``fs_out="in"``.  The input is seeded noise resident on the device.
Per arm ``--rounds`` times: ``--warmup`` calls, then ``--iters`` single-call timings (HIP events on the caller's stream around the
whole call); the table has the minimum over everything and the median over the rounds of the per-round medians.  "ms per second of
audio" is the call's time times the input rate / the input samples the call covers.  Prints one JSON line and writes the table to
``--out``.  No time is fixed anywhere: the file records what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS, L_OFF = 16000, 32000
RATES = [(48000, 16000), (44100, 16000), (16000, 48000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_stream_rate.txt"))
    a = ap.parse_args()

    import torch
    from misonet_amd import _lib
    from misonet_amd import stft as S
    from misonet_amd.resample import ResampleStream, ratio, resample_into
    from misonet_amd.stream import StreamSeparator
    if not torch.cuda.is_available():
        raise SystemExit("resample_stream_rate needs the GPU: nothing is measured without one")
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    calls, per_s, keep = {}, {}, []
    for M in (2, 6):
        for fi, fo in RATES:
            p, q = ratio(fi, fo)
            n_full = L_OFF * fi // FS if fo == FS else L_OFF                 # the recording at the input rate
            wav = (0.05 * torch.randn((1, n_full, M), device="cuda", generator=g)).contiguous()
            for n16 in (64, 256, 1024):
                n = -(-n16 * fi // FS) if fo == FS else n16
                st = ResampleStream(M, fi, fo)
                st.process(wav)                                          # a stream in progress, not a cold start
                block = wav[:, :n].contiguous()
                out = torch.empty((1, -(-(n + 1) * p // q) + 1, M), dtype=torch.float32, device="cuda")

                def call(st=st, block=block, out=out):
                    st.process_into(block, out[:, :st.outputs(block.shape[1])])

                arm = f"resample stream {fi} -> {fo} M {M} block {n} ({n16} at 16 kHz)"
                calls[arm], per_s[arm] = call, fi / n
                keep.append((st, block, out))
            full = torch.empty((1, (n_full * p + q - 1) // q, M), dtype=torch.float32, device="cuda")
            arm = f"misonet_resample {fi} -> {fo} M {M}, {n_full} samples in one call"
            calls[arm] = (lambda wav=wav, full=full, fi=fi, fo=fo: resample_into(wav, full, None, fi, fo))
            per_s[arm] = fi / n_full
            keep.append((wav, full))
        wav16 = (0.05 * torch.randn((1, L_OFF, M), device="cuda", generator=g)).contiguous()
        for n16 in (64, 256, 1024):
            st = S.StftStream(M)
            st.process(wav16)
            block = wav16[:, :n16].contiguous()
            out = torch.empty((1, M, st.frames(n16), S.N_FREQ), dtype=torch.complex64, device="cuda")
            arm = f"stft stream M {M} block {n16}"
            calls[arm], per_s[arm] = (lambda st=st, block=block, out=out: st.process_into(block, out) is None), FS / n16
            sep = StreamSeparator(M, dereverb=True, separate=True, beamform=True)
            sep.process(wav16)
            arm = f"StreamSeparator M {M} block {n16} (no rates)"
            calls[arm], per_s[arm] = (lambda sep=sep, block=block: sep.process(block) is None), FS / n16
            keep.append((st, sep, block, out))
            for fi in (48000, 44100):
                n = -(-n16 * fi // FS)
                wav_in = (0.05 * torch.randn((1, L_OFF * fi // FS, M), device="cuda", generator=g)).contiguous()
                rsep = StreamSeparator(M, dereverb=True, separate=True, beamform=True, fs=FS, fs_in=fi, fs_out="in")
                rsep.process(wav_in)
                blk = wav_in[:, :n].contiguous()
                arm = f"StreamSeparator M {M} block {n} (fs_in {fi}, fs_out in)"
                calls[arm], per_s[arm] = (lambda rsep=rsep, blk=blk: rsep.process(blk) is None), fi / n
                keep.append((rsep, blk))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        e1.synchronize()
        if rc not in (0, None, False):
            raise RuntimeError(f"the library call failed: {L.misonet_last_error().decode()}")
        return e0.elapsed_time(e1)

    meds, mins = {arm: [] for arm in calls}, {arm: float("inf") for arm in calls}
    for _ in range(a.rounds):
        for arm, fn in calls.items():
            for _ in range(a.warmup):
                timed(fn)
            ms = [timed(fn) for _ in range(a.iters)]
            meds[arm].append(statistics.median(ms))
            mins[arm] = min(mins[arm], min(ms))
    res = {}
    for arm, v in meds.items():
        med = statistics.median(v)
        res[arm] = {"min_ms": round(mins[arm], 4), "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                    "ms_per_s_audio": round(med * per_s[arm], 4)}
    doc = {"metric": "resample_stream_rate", "device": torch.cuda.get_device_name(0), "fs": FS, "warmup": a.warmup,
           "iters": a.iters, "rounds": a.rounds, "tile": int(L.misonet_resample_stream_tile()), "arms": res}
    lines = [f"streaming polyphase resampler on {doc['device']}: one recording, float32 time-major, {doc['tile']} outputs per "
             f"workgroup, blocks that give 64, 256 and 1024 samples at 16 kHz on streams that have seen the whole recording "
             f"({L_OFF} samples at 16 kHz); StreamSeparator = online WPE -> online AuxIVA -> online beamformer between the "
             "transforms at the defaults, all M rows out, int16, with a resampler at each end where rates are given",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events around the whole call); min over all timings, median over the rounds of the per-round medians, "
             "spread = (max - min) / median over the rounds; ms per second of audio = median x input rate / input samples per call",
             "a stream call is two launches (the outputs, then the state); StreamSeparator.process also allocates its outputs", "",
             f"{'arm':<72} {'min ms':>10} {'median ms':>10} {'spread':>8} {'ms / s audio':>13}"]
    for arm, r in res.items():
        lines.append(f"{arm:<72} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f} {r['ms_per_s_audio']:>13.4f}")
    lines += ["", "a first version, not tuned"]
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
