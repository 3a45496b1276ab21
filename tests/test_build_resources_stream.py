"""Register and LDS budget of the streaming STFT / iSTFT kernels (csrc/stft.hip), checked at BUILD time from the compiler's remarks
(tools/kernel_resources.py; no GPU): the four kernels present, no scratch and no spills, the registers of a workgroup within the
512 of a SIMD, no LDS beyond what the offline kernels take, and nothing that grows with the stream -- the state's size functions
take no length."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "misonet_amd", "csrc")
# the streaming kernels come in two instantiations: one 32-frame column tile (calls of up to 32 frames / 29 hops) and two
OFFLINE = {"mn::stft_stream_k<1>": "mn::stft_pack_k", "mn::stft_stream_k<2>": "mn::stft_pack_k",
           "mn::istft_stream_k<1>": "mn::istft_k", "mn::istft_stream_k<2>": "mn::istft_k"}
NEW = sorted(OFFLINE) + ["mn::istft_carry_k", "mn::stft_tail_k"]


@pytest.fixture(scope="module")
def table():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    import kernel_resources
    t = {k: r for k, r in kernel_resources.parse().items() if r["file"] == "stft.hip"}
    assert t, "no remarks of stft.hip in build/*.res: was the library built by this Makefile?"
    return t


def test_every_kernel_is_there(table):
    assert sorted(table) == sorted(NEW + sorted(set(OFFLINE.values()))), sorted(table)


def test_no_scratch_and_no_spills(table):
    bad = {k: (r["scratch"], r["vgpr_spill"], r["sgpr_spill"]) for k, r in table.items()
           if r["scratch"] or r["vgpr_spill"] or r["sgpr_spill"]}
    assert not bad, f"(scratch bytes, VGPR spills, SGPR spills): {bad}"


def test_registers_fit_the_workgroup(table):
    """every kernel runs 256 threads: 4 waves, one per SIMD, 512 registers (VGPRs + AGPRs) each; the streaming kernels keep the
    accumulators of the offline ones (at most 96 and 64 registers of MFMA results) and two chunks of twiddles in flight"""
    src = open(os.path.join(CSRC, "stft.hip")).read()
    for k in NEW:
        assert re.search(r"__launch_bounds__\(256\) void " + re.sub(r"<\d>", "", k[4:]) + r"\(", src), k
        assert table[k]["vgprs"] + table[k]["agprs"] <= 512, (k, table[k])
        assert table[k]["occupancy"] >= 1, (k, table[k])


def test_lds_is_no_more_than_the_offline_kernels(table):
    """no static LDS anywhere; the dynamic LDS of a streaming launch is the very expression of its offline kernel's launch"""
    for k, r in table.items():
        assert r["lds"] == 0, (k, r["lds"])
    src = open(os.path.join(CSRC, "stft.hip")).read()
    launches = dict((m[0], m[1]) for m in
                    re.findall(r"hipLaunchKernelGGL\((\w+(?:<\d>)?), dim3\([^;]*?\), dim3\(256\), (\w+(?:\(\))?), s,", src))
    assert sorted(launches) == sorted(k[4:] for k in table), launches
    assert launches["stft_stream_k<1>"] == launches["stft_stream_k<2>"] == launches["stft_pack_k"] == "stft_lds_bytes()"
    assert launches["istft_stream_k<1>"] == launches["istft_stream_k<2>"] == launches["istft_k"] == "istft_lds_bytes()"
    assert launches["stft_tail_k"] == launches["istft_carry_k"] == "0"
    # the output tile the analysis stages in LDS lies inside the offline kernel's allocation
    c = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", src)}
    offline_floats = (c["ST_FR"] * c["ST_HOP"] + 192 + 63) // 64 * 64 + c["ST_FR"] * c["ST_PITCH"]
    assert c["ST_FR"] * c["SS_OP"] <= offline_floats and c["SS_OP"] >= 2 * 129
    assert offline_floats * 4 <= 160 * 1024


def test_the_state_does_not_grow_with_the_stream():
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    proto = lambda name: re.search(r"long long " + name + r"\(([^)]*)\);", hdr).group(1).replace(" ", "")
    assert proto("misonet_stft_stream_state_bytes") == "intB,intM"
    assert proto("misonet_istft_stream_state_bytes") == "intR"
    src = open(os.path.join(CSRC, "stft.hip")).read()
    assert "atomic" not in src.lower()
