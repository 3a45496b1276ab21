"""The table of the side figures (score.SIDE_FIGURES) on the CPU, with stubbed blocks: side_queue's historical tuple shapes, the
order in which the blocks are queued, and the flag checks of the recording paths -- which error comes first.  No device is needed."""
import dataclasses

import numpy as np
import pytest

NO_DEVICE = -1          # torch.cuda.device(-1) is a no-op: the guard of side_queue runs without a GPU


def _stubbed(monkeypatch, calls):
    """the table with every block replaced by one that records (name, parameter) and returns the name; the batch is not built"""
    from misonet_amd import score

    def stub(f):
        if f.needs_clean:
            return lambda est, clean, mix, nv, par: calls.append((f.name, par)) or f.name
        return lambda est, mix, nv, par: calls.append((f.name, par)) or f.name

    def batch(items, dev, pinned, limits):
        for est, _, _ in items:
            limits(*np.shape(est))
        return "est", "clean", "mix", None

    monkeypatch.setattr(score, "SIDE_FIGURES", tuple(dataclasses.replace(f, block=stub(f)) for f in score.SIDE_FIGURES))
    monkeypatch.setattr(score, "_wave_batch", batch)
    return score


def test_side_queue_keeps_its_tuple_shapes(monkeypatch):
    calls = []
    score = _stubbed(monkeypatch, calls)
    items = [(np.zeros((2, 4000), np.int16), np.zeros((2, 4000), np.float32), None)]
    assert [f.name for f in score.SIDE_FIGURES] == ["bss", "stoi", "reverb", "srmr"]
    assert score.side_queue(items, NO_DEVICE) == (None, None)
    assert score.side_queue(items, NO_DEVICE, bss_filt_len=64) == ("bss", None)
    assert score.side_queue(items, NO_DEVICE, stoi_fs=8000) == (None, "stoi")
    assert score.side_queue(items, NO_DEVICE, bss_filt_len=64, stoi_fs=16000.0, reverb_fs=16000) == ("bss", "stoi", "reverb")
    assert score.side_queue(items, NO_DEVICE, reverb_fs=8000) == (None, None, "reverb")
    assert score.side_queue(items, NO_DEVICE, srmr_fs=8000) == (None, None, None, "srmr")
    calls.clear()
    assert score.side_queue(items, NO_DEVICE, True, 32, 16000, 16000, 16000) == ("bss", "stoi", "reverb", "srmr")
    assert calls == [("bss", 32), ("stoi", 16000), ("reverb", 16000), ("srmr", 16000)]      # queued in the table's order
    assert score.bss_queue(items, 64, NO_DEVICE) == "bss" and score.stoi_queue(items, 10000, NO_DEVICE) == "stoi"
    assert score.reverb_queue(items, 8000, NO_DEVICE) == "reverb"
    calls.clear()
    with pytest.raises(ValueError, match="8000, 10000 or 16000"):                            # a bad rate: before the batch
        score.side_queue(items, NO_DEVICE, bss_filt_len=64, stoi_fs=44100)
    with pytest.raises(ValueError, match="8000 or 16000"):
        score.side_queue(items, NO_DEVICE, reverb_fs=10000)
    with pytest.raises(ValueError, match="8000 or 16000"):
        score.side_queue(items, NO_DEVICE, srmr_fs=10000)
    with pytest.raises(ValueError, match="multiple of 16"):                                  # every asked figure's limits
        score.side_queue(items, NO_DEVICE, bss_filt_len=100, stoi_fs=8000)
    with pytest.raises(ValueError, match="S <= 4"):
        score.side_queue([(np.zeros((5, 100)), np.zeros((5, 100)), None)], NO_DEVICE, stoi_fs=8000)
    assert calls == []


@pytest.mark.parametrize("path", ["enhance_recording", "enhance_recordings"])
def test_flag_checks_of_the_recording_paths(path):
    """refused before anything touches a device, the first of bss / stoi / reverb without score=True named, then the clean
    sources, then the rates"""
    from misonet_amd.pipeline import Enhancer
    enh = Enhancer.__new__(Enhancer)
    obs, clean = np.zeros((1000, 6), np.float32), [np.zeros((1000, 6), np.float32)] * 2

    def run(wav_clean=None, **kw):
        if path == "enhance_recording":
            return enh.enhance_recording(obs, wav_clean, **kw)
        return enh.enhance_recordings([(obs, wav_clean, "a")], **kw)

    for flags, first in ((dict(bss=True), "bss"), (dict(stoi=True), "stoi"), (dict(reverb=True), "reverb"),
                         (dict(stoi=True, reverb=True), "stoi"), (dict(bss=True, stoi=True, reverb=True, fs=44100), "bss")):
        with pytest.raises(ValueError, match=f"^{first}=True needs score=True"):
            run(clean, **flags)
    with pytest.raises(ValueError, match="8000, 10000 or 16000"):
        run(clean, score=True, stoi=True, reverb=True, fs=44100)
    with pytest.raises(ValueError, match="8000 or 16000"):
        run(clean, score=True, stoi=True, reverb=True, fs=10000)                             # STOI takes 10 kHz, the others do not
    with pytest.raises(ValueError, match="8000 or 16000"):
        run(clean, srmr=True, fs=10000)                                                      # needs neither score nor clean
    if path == "enhance_recording":
        with pytest.raises(ValueError, match="clean sources"):                               # before the rate
            run(None, score=True, stoi=True, fs=44100)
