"""Register and LDS budget of the blind-separation kernels (csrc/iva.hip), checked at BUILD time from the compiler's remarks
(tools/kernel_resources.py; no GPU): no scratch and no spills in any of them, the resident steering kernel inside the 256
registers of one 512-thread workgroup per CU, and an LDS footprint that is static -- the kernels declare no dynamic LDS and
take T as a run-time argument only, so nothing in it can grow with T."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")

KERNELS = (["mn::iva_weights_k", "mn::iva_order_k", "mn::iva_image_k"] + [f"mn::iva_pca_k<{m}>" for m in range(2, 9)] +
           [f"mn::{k}<{n}>" for n in range(1, 9) for k in ("iva_steer_res_k", "iva_steer_str_k", "iva_project_k")])


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "iva.hip"}
    assert t, "no remarks of iva.hip in build/*.res: was the library built by this Makefile?"
    return t


def test_every_kernel_is_there(table):
    assert sorted(table) == sorted(KERNELS)


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_resident_steering_kernel_fits_one_workgroup_per_cu(table):
    for n in range(1, 9):
        r = table[f"mn::iva_steer_res_k<{n}>"]
        assert r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] >= 2, (n, r)


def test_lds_does_not_depend_on_t(table):
    """static LDS only: a few KB of reduction partials and the Jacobi matrices, fixed by K or M at compile time"""
    src = open(os.path.join(CSRC, "iva.hip")).read()
    assert "extern __shared__" not in src and "HIP_DYNAMIC_SHARED" not in src
    launches = re.findall(r"hipLaunchKernelGGL\((iva_\w+)(?:<\w+>)?, dim3\([^;]*?\), dim3\(\w+\), (\w+), s,", src)
    assert len(launches) == 7 and all(dyn == "0" for _, dyn in launches), launches
    assert all(r["lds"] <= 8 * 1024 for r in table.values()), {k: r["lds"] for k, r in table.items()}
    for n in range(1, 9):                               # [2][8 waves][3 K] partials + [2][2 K] steps + the flag
        want = 2 * 8 * 3 * n * 8 + 2 * 2 * n * 8
        for k in ("iva_steer_res_k", "iva_steer_str_k"):
            assert want <= table[f"mn::{k}<{n}>"]["lds"] <= want + 16, (k, n, table[f"mn::{k}<{n}>"]["lds"])
