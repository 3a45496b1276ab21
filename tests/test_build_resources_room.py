"""Register and LDS budget of the room simulator's kernels (csrc/room.hip), checked at BUILD time from the compiler's remarks
(tools/kernel_resources.py; no GPU): both kernels exist, neither uses scratch or spills, neither declares dynamic LDS, and the
static LDS stays under its stated bound -- room_rir_k's per-axis tables (squared offset and gain as float64, the reflection count
as 16 bits, 2 (2 x 255 + 1) entries for each of three axes) and room_mix_k's staged chunk (512 float64 taps, 512 + 256 float32
input samples)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")

KERNELS = ["mn::room_rir_k", "mn::room_mix_k"]
MAX_N, KC, TILE = 255, 512, 256
LDS_BOUND = {"mn::room_rir_k": 3 * 2 * (2 * MAX_N + 1) * (8 + 8 + 2), "mn::room_mix_k": KC * 8 + (KC + TILE) * 4}


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "room.hip"}
    assert t, "no remarks of room.hip in build/*.res: was the library built by this Makefile?"
    return t


def test_every_kernel_is_there(table):
    assert sorted(table) == sorted(KERNELS)


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_static_lds_only_and_under_its_bound(table):
    src = open(os.path.join(CSRC, "room.hip")).read()
    assert "extern __shared__" not in src and "HIP_DYNAMIC_SHARED" not in src
    assert "atomic" not in src.replace("without atomics", "")
    launches = re.findall(r"hipLaunchKernelGGL\((room_\w+), grid, dim3\(RM_TILE\), (\w+), s,", src)
    assert sorted(k for k, _ in launches) == ["room_mix_k", "room_rir_k"] and all(dyn == "0" for _, dyn in launches), launches
    assert f"ROOM_MAX_N = {MAX_N};" in open(os.path.join(CSRC, "kernels.hpp")).read()
    assert f"RM_KC = {KC};" in src and f"RM_TILE = {TILE};" in src
    for k, r in table.items():
        assert LDS_BOUND[k] - 16 <= r["lds"] <= LDS_BOUND[k] + 16, (k, r["lds"], LDS_BOUND[k])
        assert r["lds"] <= 64 * 1024 and r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] >= 2, (k, r)
