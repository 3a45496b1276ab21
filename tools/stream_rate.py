"""Cost of the streaming front end per call: the STFT stream, the iSTFT stream and the whole ``StreamSeparator`` (online WPE ->
online AuxIVA -> online beamformer between the two transforms), beside the offline ``misonet_stft`` / ``misonet_istft`` over the
same 501 frames in one call, timed in the same process.

    python tools/stream_rate.py [--warmup 3] [--iters 10] [--rounds 3] [--out profiles/stream_rate.txt]

For M = 2 and M = 6 microphones (one recording) and blocks of 64, 256 and 1024 samples (1, 4 and 16 frames): one
``StftStream.process_into`` of a block, one ``IstftStream.process_into`` of the block's frames for M rows (int16 out), and one
``StreamSeparator.process`` of a block (``dereverb=True, separate=True, beamform=True``, all M rows out, int16), each on a stream in
progress -- it has seen the 32000 samples (501 frames) the offline arms transform in one call.  The input is seeded noise resident
on the device.  Per arm ``--rounds`` times: ``--warmup`` calls, then ``--iters`` single-call timings (HIP events on the caller's
stream around the whole call); the table has the minimum over everything and the median over the rounds of the per-round medians.
"ms per second of audio" is the call's time times 16000 / the samples the call covers.  Prints one JSON line and writes the table
to ``--out``.  No time is fixed anywhere: the file records what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS, L_OFF = 16000, 32000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_rate.txt"))
    a = ap.parse_args()

    import torch
    from misonet_amd import _lib
    from misonet_amd import stft as S
    from misonet_amd.stream import StreamSeparator
    if not torch.cuda.is_available():
        raise SystemExit("stream_rate needs the GPU: nothing is measured without one")
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    calls, samples, keep = {}, {}, []
    for M in (2, 6):
        wav = (0.05 * torch.randn((1, L_OFF, M), device="cuda", generator=g)).contiguous()
        spec = S.stft_hip(wav)                                           # [1, M, 501, 129]
        T = spec.shape[2]
        rows = spec[0].contiguous()                                      # [M, 501, 129]
        for n in (64, 256, 1024):
            t = n // S.HOP
            st = S.StftStream(M)
            st.process(wav)                                              # a stream in progress, not a cold start
            block = wav[:, :n].contiguous()
            out = torch.empty((1, M, st.frames(n), S.N_FREQ), dtype=torch.complex64, device="cuda")
            assert out.shape[2] == t
            arm = f"stft stream M {M} block {n}"
            calls[arm] = (lambda st=st, block=block, out=out: st.process_into(block, out) is None)
            samples[arm] = n
            ist = S.IstftStream(M, int16=True)
            ist.process(rows)
            fr = rows[:, :t].contiguous()
            pcm = torch.empty((M, S.HOP * ist.hops(t)), dtype=torch.int16, device="cuda")
            assert pcm.shape[1] == n
            arm = f"istft stream M {M} block {n} ({t} frames, int16)"
            calls[arm] = (lambda ist=ist, fr=fr, pcm=pcm: ist.process_into(fr, pcm) is None)
            samples[arm] = n
            sep = StreamSeparator(M, dereverb=True, separate=True, beamform=True)
            sep.process(wav)
            arm = f"StreamSeparator M {M} block {n} (owpe+oiva+obf)"
            calls[arm] = (lambda sep=sep, block=block: sep.process(block) is None)
            samples[arm] = n
            keep.append((st, ist, sep, block, out, fr, pcm))
        ws = torch.empty(L.misonet_stft_workspace_bytes(1, M, L_OFF), dtype=torch.uint8, device="cuda")
        full = torch.empty_like(spec)
        arm = f"misonet_stft M {M}, {L_OFF} samples = {T} frames in one call"
        calls[arm] = (lambda wav=wav, M=M, full=full, ws=ws: L.misonet_stft(wav.data_ptr(), 1, L_OFF, M, full.data_ptr(), ws.data_ptr(),
                                                                            ws.numel(), _lib.stream_ptr(wav.device)))
        samples[arm] = L_OFF
        pcm_full = torch.empty((M, S.HOP * (T - 1)), dtype=torch.int16, device="cuda")
        arm = f"misonet_istft M {M}, {T} frames in one call (int16)"
        calls[arm] = (lambda rows=rows, M=M, T=T, pcm_full=pcm_full: L.misonet_istft(rows.data_ptr(), M, T, pcm_full.data_ptr(), None,
                                                                                     _lib.stream_ptr(rows.device)))
        samples[arm] = L_OFF
        keep.append((wav, spec, rows, ws, full, pcm_full))

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
                    "ms_per_s_audio": round(med * FS / samples[arm], 4)}
    flags = [{k: int(v.max().item()) for k, v in k3[2].fail.items()} for k3 in keep if len(k3) == 7]
    doc = {"metric": "stream_rate", "device": torch.cuda.get_device_name(0), "fs": FS, "warmup": a.warmup, "iters": a.iters,
           "rounds": a.rounds, "arms": res, "flags": flags}
    lines = [f"streaming front end on {doc['device']}: one recording, hann-256 / hop 64, blocks of 64, 256 and 1024 samples on streams "
             f"that have seen {L_OFF} samples; StreamSeparator = StftStream -> online WPE -> online AuxIVA -> online beamformer -> "
             "IstftStream at the defaults, all M rows out",
             f"{a.rounds} rounds in one process, arms in turn; per round {a.warmup} warm-up calls, then {a.iters} single-call "
             "timings (HIP events around the whole call); min over all timings, median over the rounds of the per-round medians, "
             f"spread = (max - min) / median over the rounds; ms per second of audio = median x {FS} / samples per call",
             "a stream call is two launches (the output, then the state); StreamSeparator.process also allocates its outputs", "",
             f"{'arm':<62} {'min ms':>10} {'median ms':>10} {'spread':>8} {'ms / s audio':>13}"]
    for arm, r in res.items():
        lines.append(f"{arm:<62} {r['min_ms']:>10.4f} {r['median_ms']:>10.4f} {r['spread']:>8.4f} {r['ms_per_s_audio']:>13.4f}")
    lines += ["", f"fail words of the recursions after the runs (seeded noise, not speech): {flags}",
              "a first version, not tuned"]
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
