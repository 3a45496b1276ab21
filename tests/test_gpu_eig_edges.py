"""GPU tests of the shared eigen-solver (csrc/jacobi.hpp, ``jacobi_hermitian<M>``) through its call sites, on the spectra a
Jacobi method finds hard: the cases of tests/jacobi_ref.py (exactly repeated and near-repeated eigenvalues, rank 1 .. M - 1,
identical and dead microphones, a flat floor under one or two sources, graded matrices, an eigenvalue below the 1e-12 rank
rule, an exactly diagonal R with ties), M = 2 .. 8.  One launch per M puts every case in its own bin (F = the number of cases,
B = 1, T = 16).  The covariance of every case is exact in float64 in any summation order, so host R and device R agree to the
bit and what is compared is the solver.

    AuxIVA PCA (iva_pca_k, 512 threads)   misonet_auxiva with 0 iterations, K = M: evec, Y, A of misonet_auxiva_debug
    MUSIC (doa_cov_k, 64 threads)         misonet_doa, kind music, tau = 0 (D = 3 candidates: the call wants D >= num_src): C and
                                          used of misonet_doa_debug
    mvdr_scm_eig, bf_solve / gev,         the debug copies of misonet_mvdr / misonet_beamform / misonet_beamform_joint, on the
    jbf_bin_k / lcmv                      cases with one leader apart from the rest (equal leaders make a steering vector
                                          arbitrary) and on C = I + rank 1, an (M - 1)-fold cluster; the existing restatements
                                          (tests/beamform_ref.py, tests/jbf_ref.py) and their bars

Figures and bars of the first two are those of tests/jacobi_ref.py (backward, orth, eigs, proj(S); all invariant to the basis
inside a degenerate subspace); tests/test_eig_cases.py holds the float64 restatement of the solver to the same bars on the
same cases and shows which planted faults they reject.  "A Y = X on the live span" is held to 1e-12 on every case but
``graded`` at M = 7, where the restatement itself measures 3.3e-11 (LAPACK's eigenvectors 6.5e-16) and the bar is what the
stopping rule admits, 9.6e-11 (jacobi_ref.bar_span).

The beamformer section reads the issue as follows: the steering vector of mvdr_scm_eig and d_s of lcmv "eig" see Phi_s = the
R of a leading-gap case; gev and lcmv "cw", which solve C = L^-1 Phi_s L^-H, see the cluster input only (M = 3, 6, 8), not the
leading-gap cases.  The existing bar of the mvdr steering vector is a Rayleigh deficit, second order in the vector's error (a
vector off by 5e-8 passes it); the covariance of these inputs is exact in the kernel's float32 partials too (at most one frame
per thread, every product under 2^24), so the vector is also held to proj(1) of tests/jacobi_ref.py, first order.
Bit-exact claims are asserted on bit patterns.  Every test prints its figures as ``[eig] ...``; LAB.md has the worst per call
site."""
import functools

import numpy as np
import pytest

import jacobi_ref as J
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
FS = 16000.0


def _worst(tag, figs):
    """print the worst figure / bar of every name over ``figs`` = [(label, {name: (figure, bar)})] and return the misses"""
    worst, bad = {}, []
    for label, fig in figs:
        assert J.capped(fig), (label, fig)
        for name, (v, bar) in fig.items():
            key = name.split("(")[0]
            if key not in worst or v / bar > worst[key][0] / worst[key][1]:
                worst[key] = (v, bar, label)
            if not v <= bar:
                bad.append((label, name, v, bar))
    print(f"[eig] {tag}: " + "  ".join(f"{k} {v:.2e} (bar {b:.2e}, {l})" for k, (v, b, l) in worst.items()))
    return bad


# ---- AuxIVA PCA ---------------------------------------------------------------------------------------------------------------
def _pca(Xs, ref_ch):
    """iva_pca_k on the bins Xs (a list of complex [M, T]): evec [F, M, M], Y [F, M, T], A [F, M, M], fail [F]"""
    from test_gpu_iva import _run
    M = Xs[0].shape[0]
    mix = np.ascontiguousarray(np.stack(Xs)[None].astype(np.complex64))
    assert np.array_equal(mix[0].astype(np.complex128), np.stack(Xs))               # the float32 holds the case exactly
    got = _run(mix, min(M, 4), iterations=0, channels=M, ref_ch=ref_ch)
    return {k: got[k][0] for k in ("evec", "Y", "A", "fail")}


def _check_pca(tag, names, Xs, ranks, ref_ch):
    """every per-bin assertion on the PCA of the bins Xs with the designed ranks; returns the device's result"""
    M = Xs[0].shape[0]
    got = _pca(Xs, ref_ch)
    assert not got["fail"].any()
    figs = []
    for f, (name, X, rank) in enumerate(zip(names, Xs, ranks)):
        X = np.asarray(X, np.complex128)
        R = J.cov(X)
        V, Y, A = got["evec"][f], got["Y"][f], got["A"][f]
        assert np.isfinite(V).all() and np.isfinite(Y).all() and np.isfinite(A).all(), name
        zero = ~V.any(axis=0)
        assert int(zero.sum()) == M - rank and zero[rank:].all() and not zero[:rank].any(), (name, zero)
        live = ~zero
        lam = J.rayleigh(R, V)
        fig = J.figures(R, lam, V, live=live)
        figs.append((f"{name} M={M} ref {ref_ch}", fig))
        bar = fig["eigs"][1]
        assert (np.diff(lam) <= bar * lam[0]).all(), (name, lam)                     # non-increasing, up to the eigs bar
        r = V[ref_ch, live]
        assert (r.real >= 0).all() and (np.abs(r.imag) <= 1e-15).all(), (name, r)
        assert J.fro(Y - V.conj().T @ X) <= 1e-12 * J.fro(X), name
        assert not Y[zero].any() and not A[:, zero].any(), name
        span, bar_s = J.span_figure(X, V, Y, A), J.bar_span(J.reference(R), X)
        if bar_s > 1e-12 or span > 1e-13:
            print(f"[eig] {tag} {name}: A Y = X on the live span {span:.2e} (bar {bar_s:.2e})")
        assert span <= bar_s, (name, span, bar_s)
        if name in ("diag", "scalar"):
            assert np.array_equal(J.bits(V + 0.0), J.bits(np.eye(M, dtype=np.complex128))), (name, V)
    bad = _worst(tag, figs)
    assert not bad, bad
    return got


@pytest.mark.parametrize("M", J.MS)
def test_auxiva_pca(M):
    """every case at both ends of ref_ch: the figures within their bars, the Rayleigh quotients in order, exactly the designed
    number of zero columns and those trailing, the ref component real and >= 0, Y = E^H X and A Y = X on the live span, the
    identity bit for bit on ``diag`` and ``scalar``; and X 2^40 and X 2^-40 give the bits of X's eigenvectors"""
    _need_gpu()
    cs = J.cases(M)
    names, ranks = [c["name"] for c in cs], [c["rank"] for c in cs]
    Xs = [c["X"].astype(np.complex128) for c in cs]
    for ref_ch in (0, M - 1):
        got = _check_pca(f"auxiva M={M} ref {ref_ch}", names, Xs, ranks, ref_ch)
        for s in (2.0 ** 40, 2.0 ** -40):
            scaled = _pca([X * s for X in Xs], ref_ch)
            assert not scaled["fail"].any()
            assert np.array_equal(J.bits(scaled["evec"]), J.bits(got["evec"])), (M, ref_ch, s)


@pytest.mark.parametrize("M", [3, 5, 8])
def test_auxiva_pca_fewer_frames_than_channels(M):
    """literal T = 1 and T = 2: rank < K without any padding"""
    _need_gpu()
    for fams in (("rank1",), ("rank2", "rank2eq")):
        Xs = [J.frames(f, M)[0] for f in fams]
        ranks = [J.frames(f, M)[1] for f in fams]
        assert all(X.shape == (M, len(fams)) for X in Xs) and all(r == len(fams) for r in ranks)
        for ref_ch in (0, M - 1):
            _check_pca(f"auxiva M={M} T={len(fams)} ref {ref_ch}", list(fams), Xs, ranks, ref_ch)


# ---- MUSIC ----------------------------------------------------------------------------------------------------------------
def _music(mix, S, weight=None):
    """misonet_doa, kind music, tau = 0, one block: C [K, F, M, M], used [K], q [K], fail [K].  The call wants as many
    candidates as sources: D = 3 of them, all with zero delays, and q is the same on each"""
    from test_gpu_doa import _raw
    M = mix.shape[2]
    got = _raw(mix, weight, np.zeros((3, M)), np.eye(3), "music", S, fs=FS)
    assert np.array_equal(J.bits(got["q"][..., 1:]), J.bits(got["q"][..., :1].repeat(2, axis=-1)))
    return dict(C=got["C"][0, :, 0], used=got["used"][0, :, 0], q=got["q"][0, :, 0, 0], fail=got["fail"][0, :, 0])


@functools.lru_cache(maxsize=None)
def _mix(M):
    return np.ascontiguousarray(np.stack([c["X"] for c in J.cases(M)])[None])      # [1, F, M, T]


def _check_music(tag, M, S, C, used, q):
    """one class's C [F, M, M], used and q against the float64 noise projector of every case"""
    cs = J.cases(M)
    figs, kept, q_want, q_bar = [], 0, 0.0, 0.0
    ones = np.ones(M)
    for f, c in enumerate(cs):
        name = f"{c['name']} M={M} S={S}"
        if c["rank"] < S:                                            # the signal subspace has rank below S: skipped
            assert not C[f].any(), name
            continue
        kept += 1                                                    # rank exactly S is kept: the noise cluster sits at 0
        P = M * C[f]
        assert np.isfinite(P).all() and P.any(), name
        assert np.array_equal(J.bits(C[f] + 0.0), J.bits(C[f].conj().T + 0.0)), name            # exactly Hermitian
        assert abs(np.trace(C[f]).real - (M - S) / M) <= 1e-13, name
        assert J.fro(P @ P - P) <= 1e-13, (name, J.fro(P @ P - P))
        ref = J.reference(J.cov(c["X"]))
        bar = J.bar_proj(ref, S)
        if bar is None:                                              # no gap after S: the projector is anybody's
            q_want += float((ones @ C[f] @ ones).real)
            continue
        figs.append((name, {f"proj({S})": (J.proj(ref, P, S), bar)}))
        q_want += float((ones @ J.noise_projector(ref["E"], S) @ ones).real) / M
        q_bar += bar
    assert used == kept, (tag, used, kept)
    bad = _worst(tag, figs)
    assert not bad, bad
    if kept:
        print(f"[eig] {tag}: q {q:.15e} want {q_want / kept:.15e} (bar {q_bar / kept + 1e-13:.2e})  used {used} of {len(cs)}")
        assert abs(q - q_want / kept) <= q_bar / kept + 1e-13
    return len(figs)


@pytest.mark.parametrize("M", J.MS)
def test_music_projector(M):
    """M C against eigh's noise projector within proj(S) wherever the gap after S qualifies -- clusters inside the signal
    subspace (floor+2eq, rank2eq at S = 2) and inside the noise subspace (every floor+*) must not matter; C exactly Hermitian,
    tr C = (M - S) / M, (M C)^2 = M C; bins of designed rank below S skipped and counted out of ``used``; q = the mean of
    1^H C_f 1 over the used bins (eigh's projector where it is defined, the device's own C_f where the split has no gap)"""
    _need_gpu()
    judged = 0
    for S in J.splits(M):
        got = _music(_mix(M), S)
        assert got["fail"][0] == 0
        judged += _check_music(f"music M={M} S={S}", M, S, got["C"][0], int(got["used"][0]), float(got["q"][0]))
    assert judged >= 6, judged


@pytest.mark.parametrize("M", J.MS[1:])
def test_music_second_class_after_a_skipped_first(M):
    """K = 2 classes in one workgroup at S = 2: float32 weights in {0, 1} leave class 0 one frame of every bin, a rank-1 block
    that the rank rule skips, and class 1 the full case.  Class 1's C carries the bits of the unweighted single-class run"""
    _need_gpu()
    S, mix = 2, _mix(M)
    F = mix.shape[1]
    w = np.zeros((1, 2, F, J.T), np.float32)
    w[0, 0, :, 0] = 1.0
    w[0, 1] = 1.0
    assert all(np.abs(mix[0, f, :, 0]).sum() > 0 for f in range(F))                 # class 0 is not silent: it is rank 1
    got, alone = _music(mix, S, w), _music(mix, S)
    assert not got["C"][0].any() and got["used"][0] == 0 and got["fail"][0] == 2 and got["q"][0] == 0.0
    assert got["fail"][1] == 0 and got["used"][1] == alone["used"][0] > 0
    assert np.array_equal(J.bits(got["C"][1]), J.bits(alone["C"][0]))
    assert np.array_equal(J.bits(got["q"][1:]), J.bits(alone["q"]))
    _check_music(f"music M={M} S={S} class 1 of 2", M, S, got["C"][1], int(got["used"][1]), float(got["q"][1]))


# ---- the beamformers: cases with a leading gap only (equal leaders make the steering vector arbitrary) ------------------------
@pytest.mark.parametrize("M", J.MS)
def test_mvdr_steering_vector(M):
    """mvdr_scm_eig: Phi_s of bin f is the R of a leading-gap case (floor+1, rank1, graded, twin, generic); the steering vector
    of misonet_mvdr's debug copy by the bar of the existing eigen-solver edges (beamform_ref.eig_property: the Rayleigh deficit
    against lambda_max, max(K x the complex64 yardstick, 64 x 2^-53))"""
    _need_gpu()
    import beamform_ref as BR
    from test_gpu_beamform_stages import _run
    src, mix, cs = J.leading_gap_inputs(M)
    dev = _run(src[None], mix[None])
    d, y32, lim = BR.eig_property(dev["steer1"], src[None])
    print(f"[eig] mvdr M={M}: " + "  ".join(f"{c['name']} deficit {d[0, f]:.2e} (bar {lim[0, f]:.2e})" for f, c in enumerate(cs)))
    figs = []
    for f, c in enumerate(cs):                                       # first order: the vector's direction against eigh's
        v = dev["steer1"][0, f].astype(np.complex128)
        ref = J.reference(J.cov(c["X"]))
        P = np.eye(M) - np.outer(v, v.conj()) / np.vdot(v, v).real
        figs.append((f"{c['name']} M={M}", {"proj(1)": (J.proj(ref, P, 1), J.bar_proj(ref, 1))}))
    bad = _worst(f"mvdr M={M}", figs)
    assert (d <= lim).all(), (d, lim)
    assert not bad, bad


def _per_bin(got, want, other, key):
    """per bin: (rel-L2 of got against want, the bar of tests/jbf_ref.py: max(100 x the route (a) - (b) difference, 1e-12))"""
    import jbf_ref as JR
    F = want[key].shape[2]
    return [(JR.rel(got[key][0, 0, f], want[key][0, 0, f]),
             max(100.0 * JR.rel(other[key][0, 0, f], want[key][0, 0, f]), JR.W_FLOOR)) for f in range(F)]


def _check_lcmv(tag, names, src, mix, rtf, ref_ch):
    import jbf_ref as JR
    from test_gpu_jbf import _run
    src5, mix4 = np.ascontiguousarray(src[None, None]), np.ascontiguousarray(mix[None])
    kw = dict(noise="residual", rtf=rtf, diag_load=0.0, ref_ch=ref_ch)
    want, other = JR.jbf(src5, mix4, "lcmv", **kw), JR.jbf(src5, mix4, "lcmv", route="b", **kw)
    got = _run(src5, mix4, "lcmv", **kw)
    assert not want["fail"].any() and not other["fail"].any() and not got["fail"].any()
    d_s, w = _per_bin(got, want, other, "rtf"), _per_bin(got, want, other, "w")
    print(f"[eig] {tag}: " + "  ".join(f"{n} d_s {e:.2e} (bar {b:.2e}) w {ew:.2e} (bar {bw:.2e})"
                                       for n, (e, b), (ew, bw) in zip(names, d_s, w)))
    assert all(b <= 1e-10 for _, b in d_s + w)                       # the routes agree: the bars mean something
    assert all(e <= b for e, b in d_s), (tag, d_s)
    assert all(e <= b for e, b in w), (tag, w)


@pytest.mark.parametrize("M", J.MS)
def test_lcmv_rtf_eig(M):
    """jbf_bin_k, rtf "eig": d_s = the principal eigenvector of Phi_s = a leading-gap case's R over its ref component, both
    ends of ref_ch, against tests/jbf_ref.py within its own bar, bin by bin"""
    _need_gpu()
    src, mix, cs = J.leading_gap_inputs(M)
    for ref_ch in (0, M - 1):
        _check_lcmv(f"lcmv eig M={M} ref {ref_ch}", [c["name"] for c in cs], src, mix, "eig", ref_ch)


@pytest.mark.parametrize("M", [3, 6, 8])
def test_lcmv_rtf_cw_cluster(M):
    """jbf_bin_k, rtf "cw": C = L^-1 Phi_s L^-H is the identity plus a rank-1 term, an (M - 1)-fold cluster under the leader"""
    _need_gpu()
    src, mix = J.cluster_inputs(M)
    for ref_ch in (0, M - 1):
        _check_lcmv(f"lcmv cw cluster M={M} ref {ref_ch}", [f"bin{f}" for f in range(src.shape[0])], src, mix, "cw", ref_ch)


@pytest.mark.parametrize("M", [3, 6, 8])
def test_gev_cluster(M):
    """bf_solve, gev: the same cluster in C = L^-1 Phi_s L^-H; lambda_max, w (up to its documented normalisation) and the
    output by the stage comparator of tests/beamform_ref.py and its bars.  Those bars are multiples of a complex64 yardstick,
    which is exactly 0 on integer inputs (float32 sums them without rounding): the inputs are the cluster inputs times
    float32(1 / 3), so that the cluster is degenerate to 6e-8 instead of to the bit and the yardstick exists."""
    _need_gpu()
    import beamform_ref as BR
    from test_gpu_beamform_stages import _run
    src, mix = J.cluster_inputs(M)
    third = np.float32(1.0) / np.float32(3.0)
    src, mix = np.ascontiguousarray((src * third)[None]), np.ascontiguousarray((mix * third)[None])
    for ref_ch in (0, M - 1):
        dev = _run(src, mix, beamformer="gev", ref_ch=ref_ch)
        res = BR.stage_compare(src, mix, dev, kind="gev", ref_ch=ref_ch)
        assert all(c["whole32"] > 0 for items in res.values() for c in items)
        print(f"[eig] gev cluster M={M} ref {ref_ch}: lambda_max {dev['lam'][0]}")
        BR.check_stages(res, "gev", M, J.T)
