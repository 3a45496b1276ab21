"""The array processing between the two networks (csrc/mvdr.hip: mvdr_scm_eig / bf_scm, jacobi_hermitian, mvdr_solve(_ext),
bf_solve, mvdr_apply, pit_dist_k / pit_pick_k) stage by stage against float64, each stage on its OWN input, with the comparator of
tests/beamform_ref.py (eig, phase, solve, apply; K = 4 times the complex64 yardstick for the whole tensor of an item and for the
worst bin, apply for the worst frame too; tests/test_beamform_stages.py shows on the CPU that it passes a healthy second evaluation
and rejects every injected fault).  Every case prints its ``[bf-ratio] stage kind M T whole bin`` lines before anything is asserted.

M: every instantiation of launch_mvdr, 2 ... 8.  For odd M the round-robin Jacobi seats a dummy player (ME = M + 1, ``act = q < M``),
the 8-lane butterfly of the phase correction carries dead lanes, and bf_solve's ``tid < M`` Cholesky lanes meet that Jacobi.
T: 2 M   the shortest the bound is meant for (under M frames the result is set by eps)
   64    one full pass of the 64-lane covariance loop and nothing behind it
   65    one frame in the second pass: 63 lanes add nothing
   257   the second pass of mvdr_apply's 256-thread loop holds one frame
B = 2 with item 1 three times as loud, F = 9, one seed per case.
PIT: T in {63, 64, 65, 255, 256, 257, 600} around the wave and workgroup sizes of pit_dist_k; 600 is the third pass.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import beamform_ref as R

pytestmark = pytest.mark.gpu
F = 9


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(src, mix, **o):
    """Apply_Beamforming with the debug exports, as numpy: dict(out, w[, steer1][, lam])"""
    from misonet_amd import Apply_Beamforming
    out, dbg = Apply_Beamforming(torch.from_numpy(src).cuda(), torch.from_numpy(mix).cuda(), return_debug=True, **o)
    dev = {k: v.cpu().numpy() for k, v in dbg.items()}
    dev["out"] = out.cpu().numpy()
    for k, v in dev.items():
        assert np.isfinite(v).all(), k
    return dev


def _ref_opts(o):
    return dict(kind=o.get("beamformer", "mvdr"), noise=o.get("noise", "residual"), condition=o.get("condition", 0.0),
                trace_normalize=o.get("trace_normalize", False), ban_=o.get("ban", False), ref_ch=o.get("ref_ch", 0))


def _stages(M, T, label, **o):
    src, mix = R.stage_inputs(2, F, M, T, 100 * M + T)
    dev = _run(src, mix, **o)
    assert dev["out"].shape == (2, T, F)
    R.check_stages(R.stage_compare(src, mix, dev, **_ref_opts(o)), label, M, T)


@pytest.mark.parametrize("T", ["2M", 64, 65, 257])
@pytest.mark.parametrize("M", [2, 3, 4, 5, 6, 7, 8])
def test_mvdr_stages(M, T):
    _need_gpu()
    _stages(M, 2 * M if T == "2M" else T, "mvdr")


@pytest.mark.parametrize("noise", ["residual", "mix"])
@pytest.mark.parametrize("T", ["2M", 65])
@pytest.mark.parametrize("M", [3, 5, 7])
@pytest.mark.parametrize("kind", ["souden", "gev"])
def test_souden_gev_stages(kind, M, T, noise):
    _need_gpu()
    _stages(M, 2 * M if T == "2M" else T, f"{kind}/{noise}", beamformer=kind, noise=noise)


@pytest.mark.parametrize("M", [3, 5, 7])
def test_mvdr_with_every_option(M):
    """mvdr_solve_ext and ban_scale"""
    _need_gpu()
    _stages(M, 65, "mvdr+options", condition=1e-3, trace_normalize=True, ban=True)


def test_last_microphone_as_reference():
    _need_gpu()
    for kind in ("souden", "gev"):
        _stages(5, 65, f"{kind}/ref4", beamformer=kind, ref_ch=4)


def test_eps_decides_on_a_rank_deficient_residual():
    """beamform_ref.eps_inputs: Phi_n has rank M - 2 and eigenvalues near eps; on the CPU a missing or doubled eps is over the
    bound by 4e5 and more there, the healthy restatement at 0.4 ... 1.1 yardsticks"""
    _need_gpu()
    M, T = 5, 65
    src, mix = R.eps_inputs(2, F, M, T, 7 + M)
    R.check_stages(R.stage_compare(src, mix, _run(src, mix)), "mvdr/eps", M, T)


@pytest.mark.parametrize("M", [5, 8])
@pytest.mark.parametrize("name", R.EDGES)
def test_eigen_solver_edges(name, M):
    """judged by the property (the Rayleigh quotient of the device's vector against lambda_max), not by the ill-conditioned vector"""
    _need_gpu()
    src, mix = R.edge_inputs(name, 2, F, M, 40 + M)
    dev = _run(src, mix)                                                     # finite, or it raises
    d, y32, lim = R.eig_property(dev["steer1"], src)
    b, f = np.unravel_index(np.argmax(d / lim), d.shape)
    print(f"[bf-eig] {name} M={M}: deficit {d.max():.2e} yardstick {y32.max():.2e} worst deficit / bound {d[b, f] / lim[b, f]:.3g}")
    assert (d <= lim).all(), f"{name}, M = {M}: item {b}, bin {f}: 1 - rq / lambda_max = {d[b, f]:.3e} > {lim[b, f]:.3e}"


def _direct(s_dev, m_dev, opts, fill):
    """misonet_beamform on a workspace with chosen previous contents"""
    from misonet_amd import _lib
    L = _lib.lib()
    B, F_, M, T = s_dev.shape
    n = L.misonet_beamform_workspace_bytes(B, F_, M, C.byref(opts))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda") if fill is None else torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    out = torch.empty((B, T, F_), dtype=torch.complex64, device="cuda")
    _lib.check(L.misonet_beamform(s_dev.data_ptr(), m_dev.data_ptr(), B, F_, M, T, C.byref(opts), out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr(s_dev.device)))
    return out


def test_bit_exactness():
    """M = 5, T = 65, B = 3: an item alone is the item in the batch, a second run is the first, and the previous contents of the
    workspace (0xFF bytes: NaN as float64; zeros) do not matter -- for the three kinds"""
    _need_gpu()
    from misonet_amd import Apply_Beamforming
    from misonet_amd.beamform import Beamformer
    src, mix = R.stage_inputs(3, F, 5, 65, 565)
    s_dev, m_dev = torch.from_numpy(src).cuda(), torch.from_numpy(mix).cuda()
    all3, d3 = Apply_Beamforming(s_dev, m_dev, return_debug=True)
    one, d1 = Apply_Beamforming(s_dev[1:2].contiguous(), m_dev[1:2].contiguous(), return_debug=True)
    assert torch.equal(all3[1:2], one)
    for k in ("w", "steer1"):
        assert torch.equal(d3[k][1:2], d1[k]), k
    again, d3b = Apply_Beamforming(s_dev, m_dev, return_debug=True)
    assert torch.equal(again, all3) and torch.equal(d3b["w"], d3["w"]) and torch.equal(d3b["steer1"], d3["steer1"])
    for kind in R.KINDS:
        opts = Beamformer(kind=kind).c_opts()
        fresh = _direct(s_dev, m_dev, opts, None)
        assert bool(torch.isfinite(torch.view_as_real(fresh)).all()), kind
        if kind == "mvdr":
            assert torch.equal(fresh, all3)
        for fill in (0xFF, 0):
            assert torch.equal(_direct(s_dev, m_dev, opts, fill), fresh), (kind, fill)


@pytest.mark.parametrize("T", [63, 64, 65, 255, 256, 257, 600])
@pytest.mark.parametrize("S", [2, 3])
def test_pit_distances(S, T):
    _need_gpu()
    from misonet_amd.beamform import pit_select
    from oracle import mvdr_oracle
    a, c = R.pit_inputs(3, S, T, F, 1000 * S + T)
    a_dev, c_dev = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
    sel, dist = pit_select(a_dev, c_dev, return_dist=True)
    sel2, dist2 = pit_select(a_dev, c_dev, return_dist=True)
    e, e32, where = R.pit_compare(dist.cpu().numpy(), a, c)
    print(f"[pit-ratio] S={S} T={T}: yardstick {e32:.2e} device {e / e32:.3g}")
    assert np.array_equal(sel.cpu().numpy(), mvdr_oracle.pit_select(a, c)[0])
    assert e <= R.K * e32, f"S = {S}, T = {T}: dist{list(where)} off by {e:.3e} > K x {e32:.3e} (K = {R.K:g})"
    assert torch.equal(sel, sel2) and torch.equal(dist, dist2)


@pytest.fixture(scope="module")
def nets(sd1, sd3):
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    return m1.eval(), m3.eval()


UTTS = (3, 5, 11)            # the CPU oracle re-orders the speakers of at least one microphone of each at T = 65 and 130, ref_ch 0 and 2
_chunk_cache = {}


def _chunks(frames, ref_ch, sd1):
    """mix [B, M, T, F], clean [B, S, T, F] on the device; checks once per (T, ref_ch) that the selection is exercised"""
    if (frames, ref_ch) not in _chunk_cache:
        from misonet_amd.weights import synthetic_utterance
        from oracle import pipeline_oracle
        mixs, cleans = [], []
        for u in UTTS:
            obs, s0, s1 = synthetic_utterance(u, (frames - 1) * 64)
            mixs.append(pipeline_oracle.stft_chunk(obs))
            cleans.append(np.stack([pipeline_oracle.stft_chunk(s)[ref_ch] for s in (s0, s1)]))
        sel = pipeline_oracle.miso1_inference(mixs[0], sd1, ref_ch=ref_ch)[1]
        assert (sel != np.arange(2)).any(), (frames, ref_ch, sel)             # a non-identity ``sel`` reaches src_row
        _chunk_cache[(frames, ref_ch)] = (torch.from_numpy(np.stack(mixs)).cuda(), torch.from_numpy(np.stack(cleans)).cuda())
    return _chunk_cache[(frames, ref_ch)]


@pytest.mark.parametrize("bf,T,ref_ch,with_clean", [
    (None, 65, 0, True), (None, 130, 0, True),                                # Tp = 96 and 160: padding frames behind T
    ({"kind": "souden"}, 65, 0, True), ({"kind": "souden"}, 130, 0, True),
    ({"kind": "souden", "ref_ch": 2}, 65, 2, False)],
    ids=["mvdr-65", "mvdr-130", "souden-65", "souden-130", "souden-65-ref2-noclean"])
def test_pipeline_path_equals_direct_path(nets, sd1, bf, T, ref_ch, with_clean):
    """The fused pass reads the MISO1 planes through ``sel`` (src_row with a.est), the mixture from strided planes of Tp > T
    frames; Apply_Beamforming reads contiguous complex tensors.  Same float32 values, same kernels, same order: bit for bit, in
    the default arithmetic, B = 3."""
    import misonet_amd as mz
    from misonet_amd import Apply_Beamforming
    m1, m3 = nets
    mix, clean = _chunks(T, ref_ch, sd1)
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=ref_ch, beamformer=bf)
    out, ex = enh.enhance(mix, clean if with_clean else None, want_bf=True, want_miso1=True)
    assert tuple(ex["bf"].shape) == (3, 2, T, 129) and bool(torch.isfinite(torch.view_as_real(ex["bf"])).all())
    mix_bf = mix.permute(0, 3, 1, 2)
    kw = {} if bf is None else dict(beamformer=bf["kind"], ref_ch=bf.get("ref_ch", 0))
    for s in range(2):
        want = Apply_Beamforming(ex["miso1"][:, s].permute(0, 3, 1, 2), mix_bf, **kw)
        assert torch.equal(ex["bf"][:, s], want), (bf, T, s)
    assert not torch.equal(ex["bf"][:, 0], ex["bf"][:, 1])
