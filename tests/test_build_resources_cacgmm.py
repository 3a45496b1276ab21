"""Register and memory budget of the cACGMM kernels (csrc/cacgmm.hip), checked at BUILD time (no GPU) from the remarks the Makefile
leaves in misonet_amd/csrc/build/*.res, as tests/test_build_resources.py reads them."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", os.path.join(ROOT, "misonet_amd", "csrc"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    return kernel_resources.parse()


def test_cacgmm_kernels_use_no_scratch(table):
    """cacgmm_bin_k: a 512-thread workgroup, one float64 accumulator tile per wave, static LDS that does not depend on T and
    leaves room for more than one workgroup per CU; masks_from_est_k: one thread per frame.  Neither spills, neither uses
    scratch memory"""
    for k in ("mn::cacgmm_bin_k", "mn::masks_from_est_k"):
        assert k in table, f"{k} not found in the build remarks"
        r = table[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
    r = table["mn::cacgmm_bin_k"]
    assert r["vgprs"] <= 256 and r["occupancy"] >= 2, r
    assert r["lds"] <= 64 * 1024, r
