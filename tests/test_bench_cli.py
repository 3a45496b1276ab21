"""bench.py's command line and output dump without a GPU: --full / --dump-outputs exist, and the dump writer stores the
enhanced spectrograms as float32 (real, imaginary) within its size budget."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _spectrograms(B, S=2, T=7, F=129, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(B, S, T, F, generator=g), torch.randn(B, S, T, F, generator=g))


def test_dump_outputs_float32_real_imag(tmp_path):
    import bench
    out = _spectrograms(3)
    path = bench.dump_outputs(str(tmp_path / "d"), "enhanced", out)
    assert path == str(tmp_path / "d" / "enhanced.npy")
    y = np.load(path)
    assert y.dtype == np.float32 and y.shape == (3, 2, 7, 129, 2)
    assert np.array_equal(y[..., 0], out.real.numpy()) and np.array_equal(y[..., 1], out.imag.numpy())


def test_dump_outputs_keeps_to_the_budget(tmp_path):
    import bench
    out = _spectrograms(5)
    per_utt = 2 * 7 * 129 * 2 * 4
    path = bench.dump_outputs(str(tmp_path), "enhanced", out, budget=3 * per_utt + 17)
    y = np.load(path)
    assert y.shape[0] == 3 and y.nbytes <= 3 * per_utt + 17
    assert np.array_equal(y[..., 0], out[:3].real.numpy())       # the fixed sample: the first utterances
    assert bench.DUMP_BUDGET_BYTES == 64 << 20
    # the bench batch (16 x 2 x 1001 x 129 complex) fits whole
    assert 16 * 2 * 1001 * 129 * 2 * 4 <= bench.DUMP_BUDGET_BYTES
