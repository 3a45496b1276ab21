"""Register and memory budget of the joint beamformer kernel (csrc/jbf.hip), checked at BUILD time (no GPU) from the remarks the
Makefile leaves in misonet_amd/csrc/build/*.res, as tests/test_build_resources_cacgmm.py reads them."""
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


def test_jbf_kernel_uses_no_scratch(table):
    """jbf_bin_k: a 512-thread workgroup, one float64 accumulator tile per wave, static LDS that does not depend on T (the small
    matrices of the solve lie over the float64 rows) and leaves room for two workgroups per CU.  It does not spill and uses no
    scratch memory"""
    k = "mn::jbf_bin_k"
    assert k in table, f"{k} not found in the build remarks"
    r = table[k]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgprs"] <= 256 and r["occupancy"] >= 2, r
    assert r["lds"] <= 64 * 1024, r
