"""Register and LDS budget of the online-beamformer kernels (csrc/obf.hip), checked at BUILD time from the compiler's remarks
(tools/kernel_resources.py; no GPU): both kernels present in every M instantiation, no scratch and no spills, the registers of
the workgroup within the 512 of a SIMD, no LDS beyond a static one, and nothing that grows with T -- neither the state's size
function nor the launch takes it."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "obf.hip"}
    assert t, "no remarks of obf.hip in build/*.res: was the library built by this Makefile?"
    return t


def test_every_kernel_is_there_in_every_instantiation(table):
    names = sorted(table)
    assert sum(k.startswith("mn::obf_reset_k") for k in names) == 1, names
    inst = sorted(int(m) for k in names for m in re.findall(r"obf_k<(\d+)>", k))
    assert inst == [2, 3, 4, 5, 6, 7, 8], names
    assert len(names) == 8, names


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_registers_fit_the_workgroup(table):
    """the waves of one workgroup share the 4 SIMDs of a CU: 512 registers (VGPRs + AGPRs) per SIMD over its waves; the workgroup
    is cells_per_block(M) groups of G lanes"""
    from misonet_amd import _lib as L
    lib = L.lib()
    seen = 0
    for k, r in table.items():
        m = re.findall(r"obf_k<(\d+)>", k)
        if not m:
            continue
        M = int(m[0])
        G = 2 if M <= 2 else 4 if M <= 4 else 8
        threads = lib.misonet_obf_cells_per_block(M) * G
        assert threads % 64 == 0 and 64 <= threads <= 1024, (M, threads)
        per_simd = -(-(threads // 64) // 4)
        assert (r["vgprs"] + r["agprs"]) * per_simd <= 512, (M, threads, r)
        seen += 1
    assert seen == 7


def test_lds_is_static_and_nothing_grows_with_t(table):
    for k, r in table.items():
        assert r["lds"] <= 160 * 1024, (k, r["lds"])
    # T reaches the kernel as a loop bound only: the size function does not take it, and the launches have no dynamic LDS
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    proto = re.search(r"misonet_obf_state_bytes\(([^)]*)\)", hdr).group(1)
    assert proto.replace(" ", "") == "intB,intS,intM,intF", proto
    src = open(os.path.join(CSRC, "obf.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\((obf_\w+)(?:<M>)?, dim3\(([^;]*?)\), dim3\(([^;]*?)\), (\w+), s,", src)
    assert sorted(l[0] for l in launches) == ["obf_k", "obf_reset_k"], launches
    for name, grid, block, dyn in launches:
        assert dyn == "0" and "T" not in re.findall(r"\b[A-Z]\b", grid + " " + block), (name, grid, block, dyn)
        assert not re.search(r"\bT\b", grid + " " + block), (name, grid, block)
    assert "extern __shared__" not in src
