"""Register and LDS budget of the resampler's kernel (csrc/resample.hip), checked at BUILD time from the compiler's remarks
(tools/kernel_resources.py; no GPU): the five instantiations exist, none uses scratch or spills -- each thread keeps up to 16
float64 sums and their index ranges in registers across the chunks of a tile -- and the staging buffer is the 48 KB of static LDS
that leaves room for three workgroups per CU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")

KERNELS = [f"mn::resample_k<{k}>" for k in (1, 2, 4, 8, 16)]


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "resample.hip"}
    assert t, "no remarks of resample.hip in build/*.res: was the library built by this Makefile?"
    return t


def test_every_kernel_is_there(table):
    assert sorted(table) == sorted(KERNELS)


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_registers_and_lds(table):
    src = open(os.path.join(CSRC, "resample.hip")).read()
    assert "extern __shared__" not in src and "atomic" not in src.replace("No atomics", "")
    for k, r in table.items():
        assert r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] >= 2, (k, r)
        assert r["lds"] == 12288 * 4, (k, r["lds"])
