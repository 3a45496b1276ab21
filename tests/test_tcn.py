"""CPU tests of tests/tcn_ref.py: the comparator of the GPU TCN tests (tests/test_gpu_tcn.py) must be able to fail.

* the clean restatement of the TemporalBlocks equals oracle/miso_oracle.tcn_forward in float64, all four norm types;
* K * e32 is not vacuous: the float32 oracle's own distance from the float64 truth is the 5e-7 ... 1e-6 of float32
  round-off through 14 blocks, and an INDEPENDENT healthy float32 evaluation (the restatement in float32: other summation
  order, other ELU, float64 statistics like the kernels) passes at the K the GPU tests use;
* every injected fault, at the smallest frame count of the GPU matrix that reaches it, is rejected at that K -- both as a faulty
  kernel would show it (in all 14 blocks) and in the LAST block alone (nothing downstream amplifies it).
"""
import numpy as np
import pytest
import torch

import tcn_ref

NORMS = ("IN", "gLN", "cLN", "BN")


def _sd(nt):
    from misonet_amd import weights as W
    return W.make_state_dict(W.miso1_spec(norm_type=nt), seed=3)


_cache = {}


def _case(nt, T):
    """(x, truth, y32): instance-normed input [2, 128, T], the float64 and the float32 oracle on it (computed once, read-only)"""
    if (nt, T) not in _cache:
        from oracle import miso_oracle
        sd = _sd(nt)
        x = np.random.default_rng(1000 + T).standard_normal((2, 128, T))
        x[1] *= 3.0
        x = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
        x = x.astype(np.float32).astype(np.float64)                   # the device hands over float32 values
        with miso_oracle.precision(torch.float64):
            truth = np.concatenate([miso_oracle.tcn_forward(torch.from_numpy(x[b:b + 1]), sd, norm_type=nt).numpy() for b in range(2)])
        y32 = np.concatenate([miso_oracle.tcn_forward(torch.from_numpy(x[b:b + 1].astype(np.float32)), sd, norm_type=nt).numpy()
                              for b in range(2)])
        for a in (x, truth, y32):
            a.setflags(write=False)
        _cache[(nt, T)] = (sd, x, truth, y32)
    return _cache[(nt, T)]


# every norm type below and above one tile; the segment walk (the same code for every norm type) at the two long cases
@pytest.mark.parametrize("nt,T", [(nt, T) for nt in NORMS for T in (40, 130)] + [("gLN", 1921), ("IN", 1985)])
def test_restatement_equals_oracle_float64(nt, T):
    sd, x, truth, _ = _case(nt, T)
    y = tcn_ref.tcn_forward(x, sd, nt)
    e = tcn_ref.rel_l2(y, truth)
    print(f"[tcn_ref] {nt} T={T}: restatement vs float64 oracle {e:.2e}")
    assert y.shape == truth.shape and e <= 1e-12, (nt, T, e)


@pytest.mark.parametrize("T", [40, 130, 257])
@pytest.mark.parametrize("nt", NORMS)
def test_bound_is_not_vacuous(nt, T):
    sd, x, truth, y32 = _case(nt, T)
    r32 = tcn_ref.tcn_forward(x, sd, nt, dtype=np.float32)
    for b in range(2):
        c = tcn_ref.check(y32[b], truth[b], y32[b], f"float32 oracle against itself {nt} T={T} sample {b}")
        assert 1e-7 <= c["e32"] <= 2e-6 and c["f32max"] <= 4e-6, c      # float32 round-off through 14 blocks, nothing else
        c = tcn_ref.check(r32[b], truth[b], y32[b], f"float32 restatement {nt} T={T} sample {b}")
        print(tcn_ref.report(c, f"float32 restatement {nt} T={T} sample {b}"))


# fault, norm type, the smallest T of the GPU matrix that reaches it
FAULT_CASES = [
    ("gln_tile", "gLN", 129),        # the second tile holds one frame: the smallest partial there is to lose
    ("in_tile", "IN", 129),
    ("cln_sample", "cLN", 40),
    ("seam", "gLN", 1921),           # the second segment holds one frame
    ("seam", "IN", 1985),            # dilation-64 taps cross the seam both ways
    ("tail", "IN", 130),             # Tq = 132: two stale frames inside the float4 tail
    ("tail", "cLN", 130),
    ("pw16", "IN", 40),
    ("pw16", "BN", 128),
]


@pytest.mark.parametrize("blocks", [None, (13,)], ids=["all_blocks", "last_block"])
@pytest.mark.parametrize("fault,nt,T", FAULT_CASES)
def test_fault_is_rejected(fault, nt, T, blocks):
    sd, x, truth, y32 = _case(nt, T)
    y = tcn_ref.tcn_forward(x, sd, nt, fault=fault, fault_blocks=blocks)
    hit = []
    for b in range(2):
        c = tcn_ref.compare(y[b], truth[b], y32[b])
        print(tcn_ref.report(c, f"fault {fault} {nt} T={T} sample {b}"))
        try:
            tcn_ref.check(y[b], truth[b], y32[b], f"fault {fault}")
        except AssertionError as e:
            hit.append(b)
            assert f"t={c['t']}" in str(e)                           # the message names the worst frame
        if fault == "seam" and blocks is not None:                   # ... which lies next to the seam
            assert abs(c["t"] - tcn_ref.DW_SEG) <= tcn_ref.DW_HALO, c
    assert hit, f"fault {fault!r} ({tcn_ref.FAULTS[fault]}) passed the comparator at K = {tcn_ref.K:g}"
    if fault in ("in_tile", "cln_sample"):
        assert hit == [1]                                            # only the sample whose statistics are wrong
