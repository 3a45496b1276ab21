"""Register and LDS budget of the streaming resampler's kernels (csrc/resample_stream.hip), checked at BUILD time from the
compiler's remarks (tools/kernel_resources.py; no GPU): the three kernels present, no scratch and no spills, the registers of a
workgroup within the 512 of a SIMD, static LDS only and no more than the offline kernel's 48 KB, nothing that grows with the stream
-- the state's size function takes no length -- and the offline file still holds exactly its five kernels."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")
NEW = ["mn::resample_stream_k<1>", "mn::resample_stream_k<2>", "mn::resample_tail_k"]
OFFLINE = [f"mn::resample_k<{k}>" for k in (1, 2, 4, 8, 16)]


@pytest.fixture(scope="module")
def tables():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    every = kernel_resources.parse()
    new = {k: r for k, r in every.items() if r["file"] == "resample_stream.hip"}
    assert new, "no remarks of resample_stream.hip in build/*.res: was the library built by this Makefile?"
    return new, {k: r for k, r in every.items() if r["file"] == "resample.hip"}


def test_every_kernel_is_there(tables):
    assert sorted(tables[0]) == sorted(NEW), sorted(tables[0])


def test_the_offline_file_still_has_exactly_its_five_kernels(tables):
    assert sorted(tables[1]) == sorted(OFFLINE), sorted(tables[1])


def test_no_scratch_and_no_spills(tables):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in tables[0].items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_registers_fit_the_workgroup(tables):
    """every kernel runs 256 threads: 4 waves, one per SIMD, 512 registers each; the output kernel keeps at most two float64 sums
    and their ranges per thread, so it leaves room for a second workgroup per SIMD as the offline kernel does"""
    src = open(os.path.join(CSRC, "resample_stream.hip")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", src)}
    assert c["RSS_THREADS"] == 256
    for k in NEW:
        assert re.search(r"__launch_bounds__\(RSS_THREADS\) void " + re.sub(r"<\d>", "", k[4:]) + r"\(", src), k
        r = tables[0][k]
        assert r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] >= 2, (k, r)


def test_lds_is_static_and_no_more_than_the_offline_kernel(tables):
    src = open(os.path.join(CSRC, "resample_stream.hip")).read()
    assert "extern __shared__" not in src
    launches = re.findall(r"hipLaunchKernelGGL\((\w+(?:<\d>)?), [^;]*?, (\w+), s,", src)
    assert sorted(k for k, _ in launches) == sorted(k[4:] for k in NEW) and all(dyn == "0" for _, dyn in launches), launches
    c = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", src)}
    for k in NEW[:2]:
        assert tables[0][k]["lds"] == c["RSS_LDS"] * 4 + c["RSS_TAPS"] * 8 <= 12288 * 4, (k, tables[0][k]["lds"])
    assert tables[0]["mn::resample_tail_k"]["lds"] == 0
    # a chunk holds at least one sample of 16 channels, and a tile's sums fit the two instantiations
    assert c["RSS_LDS"] >= 16 and c["RSS_TILE"] * 8 <= c["RSS_THREADS"] and c["RSS_TILE"] * 16 <= 2 * c["RSS_THREADS"]


def test_the_state_does_not_grow_with_the_stream():
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    proto = re.search(r"long long misonet_resample_stream_state_bytes\(([^)]*)\);", hdr).group(1).replace(" ", "")
    assert proto == "intB,intM,longlongfs_in,longlongfs_out"
    assert "atomic" not in open(os.path.join(CSRC, "resample_stream.hip")).read().lower()
