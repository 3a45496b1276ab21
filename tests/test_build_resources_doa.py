"""Register and LDS budget of the localisation kernels (csrc/doa.hip), checked at BUILD time from the compiler's remarks
(tools/kernel_resources.py; no GPU): the three kernels exist (doa_cov_k and doa_steer_k once per microphone count 2 .. 8), none
uses scratch or spills, none declares dynamic LDS, and the static LDS stays within 16 bytes of its stated bound -- doa_cov_k's
staged frames (M x 64 complex128), weights (8 x 64 float64), accumulators (8 x M^2 complex128), the two Jacobi matrices and the
flags; doa_steer_k's chunk of upper triangles (CHUNK x M (M - 1) / 2 complex128) with one diagonal sum and one flag per bin;
doa_peak_k's reduction (TILE values and two TILE index arrays).  CHUNK and TILE are the exported constants."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")
MICS = range(2, 9)
KERNELS = [f"mn::doa_cov_k<{m}>" for m in MICS] + [f"mn::doa_steer_k<{m}>" for m in MICS] + ["mn::doa_peak_k"]
FRAMES, MAX_K = 64, 8


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "doa.hip"}
    assert t, "no remarks of doa.hip in build/*.res: was the library built by this Makefile?"
    return t


@pytest.fixture(scope="module")
def consts():
    from misonet_amd import _lib
    L = _lib.lib()
    return int(L.misonet_doa_tile()), int(L.misonet_doa_bin_chunk())


def lds_bound(kernel, tile, chunk):
    m = re.search(r"<(\d+)>", kernel)
    M = int(m.group(1)) if m else 0
    if "doa_cov_k" in kernel:
        return M * FRAMES * 16 + MAX_K * FRAMES * 8 + MAX_K * M * M * 16 + 2 * M * M * 16 + (1 + MAX_K) * 4 + M * 4
    if "doa_steer_k" in kernel:
        return chunk * (M * (M - 1) // 2 * 16 + 8 + 4)
    return tile * (8 + 4 + 4)


def test_every_kernel_is_there(table):
    assert sorted(table) == sorted(KERNELS)


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_static_lds_only_and_within_its_bound(table, consts):
    tile, chunk = consts
    src = open(os.path.join(CSRC, "doa.hip")).read()
    assert "extern __shared__" not in src and "HIP_DYNAMIC_SHARED" not in src
    assert "atomic" not in src.lower()
    launches = re.findall(r"hipLaunchKernelGGL\((doa_\w+)(?:<M>)?, dim3\([^;]*?\), dim3\((\w+)\), (\w+), s,", src)
    assert sorted(launches) == [("doa_cov_k", "DOA_FRAMES", "0"), ("doa_peak_k", "DOA_TILE", "0"),
                                ("doa_steer_k", "DOA_TILE", "0")], launches
    assert f"DOA_TILE = {tile};" in src and f"DOA_CHUNK = {chunk};" in src and f"DOA_FRAMES = {FRAMES};" in src
    assert f"DOA_MAX_K = {MAX_K}," in open(os.path.join(CSRC, "kernels.hpp")).read()
    for k, r in table.items():
        bound = lds_bound(k, tile, chunk)
        assert bound - 16 <= r["lds"] <= bound + 16, (k, r["lds"], bound)
        assert r["lds"] <= 64 * 1024 and r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] >= 2, (k, r)
