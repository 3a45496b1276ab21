"""Register and LDS budget of the online-WPE kernels (csrc/owpe.hip), checked at BUILD time from the compiler's remarks
(tools/kernel_resources.py; no GPU): no scratch and no spills, the static LDS of the frame loop a few KB, the whole workgroup
(static + dynamic, ``misonet_owpe_lds_bytes``) within the 160 KB of a CU at every order the call admits, and nothing that grows
with T -- neither the LDS nor the state takes T as an argument."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")

KERNELS = ["mn::owpe_k", "mn::owpe_reset_k"]


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "owpe.hip"}
    assert t, "no remarks of owpe.hip in build/*.res: was the library built by this Makefile?"
    return t


def test_every_kernel_is_there(table):
    assert sorted(k.split("(")[0] for k in table) == sorted(KERNELS), sorted(table)


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_one_workgroup_of_512_fits(table):
    r = next(r for k, r in table.items() if k.startswith("mn::owpe_k"))
    assert r["vgprs"] + r["agprs"] <= 128, r            # 8 waves of one workgroup on the 4 SIMDs of a CU: two per SIMD


def test_lds_within_160_kb_and_nothing_grows_with_t(table):
    from misonet_amd import _lib as L
    lib = L.lib()
    static = next(r for k, r in table.items() if k.startswith("mn::owpe_k"))["lds"]
    assert 0 < static <= 4 * 1024, static               # u, z, x, y, the two power rings, the flags, three parameters
    worst = 0
    for M in range(1, 9):
        for taps in sorted({1, 80 // M}):
            o = L.OwpeOpts()
            lib.misonet_owpe_opts_default(C.byref(o))
            o.taps = taps
            n = lib.misonet_owpe_lds_bytes(M, C.byref(o))
            N, R = M * taps, o.delay + taps - 1
            assert n == N * (N | 1) * 16 + M * N * 16 + R * M * 8 + static, (M, taps, n)
            worst = max(worst, n)
    assert worst <= 160 * 1024 and worst >= 80 * 81 * 16, worst
    # T reaches the kernel as a loop bound only: no size function takes it, and the launch's dynamic LDS is that of (M, taps, delay)
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    for name in ("misonet_owpe_state_bytes", "misonet_owpe_lds_bytes"):
        proto = re.search(name + r"\(([^)]*)\)", hdr).group(1)
        assert " T" not in proto and "T," not in proto, proto
    src = open(os.path.join(CSRC, "owpe.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\((owpe_\w+), dim3\([^;]*?\), dim3\(\w+\), (\w+), s,", src)
    assert sorted(launches) == [("owpe_k", "lds"), ("owpe_reset_k", "0")], launches
    assert "const int lds = owpe_lds(M, taps, delay).total - (int)sizeof(OwpeFrame);" in src
