#!/usr/bin/env python3
"""Writes tests/golden/g15_score.npz: seeded complex64 spectrograms and what the reference's own training criterion
(criterion.py ``loss_uPIT`` / ``loss_Enhance``) answers for them.  Runs on a development machine that has a checkout of the
reference (``--reference <dir>``); the fixture holds arrays only, the tests never need the checkout.

    python tools/gen_golden_score.py --reference /path/to/MISOnet

Per S in {2, 3} (B = 2, T = 24, F = 129): ``ref{S}`` complex64 [B, S, T, F]; ``est{S}`` = the references in a shuffled order
(not the identity), scaled and with a little noise, so that the winning permutation is not the identity and wins by a wide
margin; ``upit{S}`` = loss_uPIT (the batch mean of the per-item minimum), ``upit_idx{S}`` int64 [B] = the index into
itertools.permutations that its argmin picks, ``enh{S}`` [S] = loss_Enhance of est[:, j:j+1] against ref[:, j:j+1]."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, F = 2, 24, 129
SHUFFLE = {2: [1, 0], 3: [2, 0, 1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds criterion.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g15_score.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import criterion

    picked = []
    argmin = torch.argmin

    def recording_argmin(*args, **kw):            # loss_uPIT computes its pick and drops it: keep what it computed
        r = argmin(*args, **kw)
        picked.append(r.clone())
        return r

    arrays = {}
    for S in (2, 3):
        rng = np.random.default_rng(1500 + S)
        ref = (rng.standard_normal((B, S, T, F)) + 1j * rng.standard_normal((B, S, T, F))).astype(np.complex64)
        noise = (rng.standard_normal((B, S, T, F)) + 1j * rng.standard_normal((B, S, T, F))).astype(np.complex64)
        # est[i] = 0.8 ref[SHUFFLE[i]] + noise: estimate i belongs to reference SHUFFLE[i]
        est = (np.float32(0.8) * ref[:, SHUFFLE[S]] + np.float32(0.05) * noise).astype(np.complex64)
        te, tr = torch.from_numpy(est), torch.from_numpy(ref)
        picked.clear()
        torch.argmin = recording_argmin
        try:
            val = criterion.loss_uPIT(S, te, [tr[:, s:s + 1].clone() for s in range(S)])
        finally:
            torch.argmin = argmin
        assert len(picked) == 1
        enh = [float(criterion.loss_Enhance(te[:, j:j + 1], tr[:, j:j + 1])) for j in range(S)]
        arrays[f"ref{S}"] = ref
        arrays[f"est{S}"] = est
        arrays[f"upit{S}"] = np.float64(float(val))
        arrays[f"upit_idx{S}"] = picked[0].numpy().astype(np.int64)
        arrays[f"enh{S}"] = np.asarray(enh, dtype=np.float64)
    np.savez(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes;", {k: (v.shape if v.ndim else float(v)) for k, v in arrays.items()})


if __name__ == "__main__":
    main()
