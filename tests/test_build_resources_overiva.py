"""Register and LDS budget of the kernels of the online AuxIVA for fewer sources than microphones (csrc/overiva.hip), checked at
BUILD time from the compiler's remarks (tools/kernel_resources.py; no GPU): the reset kernel and all 28 (M, K) instantiations
present, no scratch and no spills, the registers of a workgroup's waves within a SIMD's 512, the static LDS |yt|^2 [K][1025] and
phi and nothing else, and nothing that grows with T -- neither the state's size function nor the launch takes it.  Resource
figures only: nothing else of the generated code is looked at."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")
PAIRS = [(M, K) for M in range(2, 9) for K in range(1, M)]


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "overiva.hip"}
    assert t, "no remarks of overiva.hip in build/*.res: was the library built by this Makefile?"
    return t


def _pair(name):
    m = re.findall(r"overiva_k<(\d+), ?(\d+)>", name)
    return (int(m[0][0]), int(m[0][1])) if m else None


def test_every_kernel_is_there_in_every_instantiation(table):
    names = sorted(table)
    assert sum(k.startswith("mn::overiva_reset_k") for k in names) == 1, names
    assert sorted(p for p in map(_pair, names) if p) == PAIRS, names
    assert len(names) == 29, names


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_registers_fit_the_workgroup(table):
    """the waves of one workgroup share the 4 SIMDs of a CU: 512 registers (VGPRs + AGPRs) per SIMD over its waves"""
    from misonet_amd import _lib as L
    lib = L.lib()
    for k, r in table.items():
        p = _pair(k)
        if not p:
            continue
        M, K = p
        G = 2 if M <= 2 else 4 if M <= 4 else 8
        threads = lib.misonet_overiva_bins_per_pass(M, K) * G
        assert threads % 64 == 0 and threads <= 1024, (M, K, threads)
        per_simd = -(-(threads // 64) // 4)
        assert (r["vgprs"] + r["agprs"]) * per_simd <= 512, (M, K, threads, r)


def test_lds_is_static_and_nothing_grows_with_t(table):
    lds = {_pair(k): r["lds"] for k, r in table.items() if _pair(k)}
    for (M, K), n in lds.items():
        assert K * 1025 * 8 <= n <= K * 1025 * 8 + 256, (M, K, n)       # |yt|^2 [K][1025] and phi: F = 1025 is the largest admitted
        assert n <= 160 * 1024
    # T reaches the kernel as a loop bound only: the size function does not take it, and the launch has no dynamic LDS
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    proto = re.search(r"misonet_overiva_state_bytes\(([^)]*)\)", hdr).group(1)
    assert proto.replace(" ", "") == "intB,intM,intK,intF", proto
    src = open(os.path.join(CSRC, "overiva.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(\(?(overiva_\w+)(?:<M, K>\))?, dim3\(([^;]*?)\), dim3\(([^;]*?)\), (\w+), s,", src)
    assert sorted(l[0] for l in launches) == ["overiva_k", "overiva_reset_k"], launches
    for name, grid, block, dyn in launches:
        assert dyn == "0" and "T" not in re.findall(r"\b[A-Z]\b", grid + " " + block), (name, grid, block, dyn)
    assert "extern __shared__" not in src
