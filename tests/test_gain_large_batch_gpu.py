"""The gain block above 1,024 volumes on the MI355X: the tiled path (vg_gp_gain_* route 1024 < B <= 4096 to it, vg_gp_gain_*_tiled take
it at any B) against the float64 oracle, against the blocked path where both exist, run to run and under hipGraph replay, and the
train step above B = 1024 through VAE on one process and on two data-parallel ranks (dp_gain='global').
Every case at B > 1024 here raised VgError before the tiled path existed."""
import os

import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
from vae_gam_amd.vae_reg_GP import VAE
import kernel_cases as K
import gain_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available()
    import emu_inject; emu_inject.use_product_library()
    _lib.get_lib()
    yield


_posterior_fp32_distances = G.posterior_fp32_distances        # the jitter-0 reference of every gain test (tests/gain_cases.py)


@pytest.mark.parametrize('B,n,jitter', [(1025, 6, 0.0), (1536, 6, 0.0), (2048, 6, 0.0), (2048, 64, 1e-4), (4096, 6, 0.0)])
def test_large_batch_gain_block_matches_float64_oracle(monkeypatch, B, n, jitter):
    import vaegam_oracle as O
    if not jitter:                                             # the distances as the kernel forms them (see above)
        monkeypatch.setattr(O, 'gp_posterior', _posterior_fp32_distances)
    K.run_gain_case('cuda', B=B, n=n, jitter=jitter, seed=B)


def _inputs(B, n=6, seed=3, kinds=G.DEFAULT_KINDS):
    """the shared builder's inputs on the GPU: (consts, flat parameters, covariates, eps, weights of the gains in the loss)"""
    inp = G.build_inputs(B, n, seed, kinds)
    return G.consts_of(inp, 'cuda'), inp.flat.cuda(), inp.cov.cuda(), inp.eps.cuda(), inp.wt.cuda()


def _fwd_bwd(consts, flat, cov, eps, wt):
    fp = flat.clone().requires_grad_(True)
    fg = torch.zeros_like(fp)
    tv, kl, bm, bc, fb, sg, klt = ops.GpGain.apply(cov, eps, consts, fp.detach(), fg, None, fp)
    ((tv * wt).sum() + 0.7 * kl.sum()).backward()
    torch.cuda.synchronize()
    return tv.detach(), kl.detach(), fg, bc, sg


def test_batch_above_4096_is_refused():
    consts, flat, cov, eps, wt = _inputs(4097)
    with pytest.raises(_lib.VgError, match='4096'):
        _fwd_bwd(consts, flat, cov, eps, wt)


TILED_VS_BLOCKED_BAND = G.TILED_VS_BLOCKED_BAND


@pytest.mark.parametrize('B', [256, 1024])
def test_tiled_path_matches_the_blocked_path(monkeypatch, B):
    inp = _inputs(B, seed=B)
    tv0, kl0, g0, bc0, sg0 = _fwd_bwd(*inp)
    monkeypatch.setattr(ops, 'GAIN_FORCE_TILED', True)
    tv1, kl1, g1, bc1, sg1 = _fwd_bwd(*inp)
    d_tv = float((tv1 - tv0).abs().max() / tv0.abs().max())
    d_g = float((g1 - g0).abs().max() / g0.abs().max())
    print('B=%d tiled vs blocked: task_var %.3g, grads %.3g (relative to max)' % (B, d_tv, d_g))
    assert torch.equal(bc1, bc0) and torch.equal(sg1, sg0)     # the covariance is formed element by element the same way
    assert d_tv <= TILED_VS_BLOCKED_BAND['task_var'] and d_g <= TILED_VS_BLOCKED_BAND['grads'], (d_tv, d_g)
    np.testing.assert_allclose(float(kl1), float(kl0), rtol=1e-7)


def test_tiled_path_is_bit_reproducible():
    inp = _inputs(2048, seed=5)
    a, b = _fwd_bwd(*inp), _fwd_bwd(*inp)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_tiled_path_replays_from_a_hipgraph_bit_for_bit():
    """vg_gp_gain_fwd + _bwd at B = 2048 captured into one hipGraph: every replay == the eager calls, bit for bit."""
    import ctypes
    B = 2048
    consts, flat, cov, eps, wt = _inputs(B, seed=6)
    lib = _lib.get_lib()
    d = consts.desc(B)
    ws = torch.empty(lib.size('vg_gp_gain_ws_bytes', consts.C, B, consts.n) // 8, dtype=torch.float64, device='cuda')
    tv = torch.empty(consts.C, B, device='cuda'); kl = torch.empty(1, device='cuda'); fg = torch.zeros_like(flat)
    g_kl = torch.full((1,), 0.7, device='cuda')
    P = ops._p

    def launch():
        st = torch.cuda.current_stream().cuda_stream
        lib.call('vg_gp_gain_fwd', ctypes.byref(d), P(consts.table), P(flat), P(consts.xu), P(cov), int(cov.stride(0)), P(eps),
                 P(consts.hrf), P(ws), P(tv), P(kl), None, None, None, None, st)
        lib.call('vg_gp_gain_bwd', ctypes.byref(d), P(consts.table), P(flat), P(consts.xu), P(cov), int(cov.stride(0)), P(eps),
                 P(consts.hrf), P(ws), P(wt), P(g_kl), P(fg), st)
    launch()
    torch.cuda.synchronize()
    eager = (tv.clone(), kl.clone(), fg.clone())
    ref = _fwd_bwd(consts, flat, cov, eps, wt)                 # the same calls through ops.GpGain / autograd
    assert torch.equal(ref[0], eager[0]) and torch.equal(ref[2], eager[2])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            launch()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        tv.zero_(); kl.zero_(); fg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tv, eager[0]) and torch.equal(kl, eager[1]) and torch.equal(fg, eager[2])


# ------------------------------------------------------------------------------------------------ the train step above B = 1024
def _dataset(n_vol, seed):
    from vae_gam_amd import synthetic
    return synthetic.make_dataset(num_subjects=2, vols_per_subject=(n_vol + 1) // 2, num_covariates=3, seed=seed)


def _noise(Bg, C=3, L=32, seed=1234):
    gen = torch.Generator(device='cuda'); gen.manual_seed(seed)
    return {'eps_w': torch.randn(Bg, 1, device='cuda', generator=gen), 'eps_d': torch.randn(Bg, L, device='cuda', generator=gen),
            'eps_beta': torch.randn(C, Bg, device='cuda', generator=gen)}


def _oracle_gains(model, cov, eps_beta):
    """task_var (C, B) and the per-covariate KL terms in float64 from the model's own gain parameters (vae_reg_GP.py:345-378)."""
    import vaegam_oracle as O
    K_ = model._gain_consts(cov.device)
    consts = K_['consts']
    table = consts.table.cpu().numpy()
    p = model.optimizer.groups[torch.float32]['p'].detach().cpu().double()
    B, n = cov.shape[0], consts.n
    tvs, kls = [], []
    for i, row in enumerate(table):
        xq = cov[:, i].detach().cpu().float().double()
        sa, std = p[row[3]], p[row[4]].exp()
        kl = O.lin_gain_kl(sa, std)
        bm = sa * xq
        bc = torch.diag(std ** 2 * xq ** 2)
        if row[0]:
            qm, qS = p[row[5]:row[5] + n].reshape(1, n), p[row[6]:row[6] + n * n].reshape(n, n)
            kvar, ls = p[row[7]].exp() + 0.1, 3.0 * torch.sigmoid(p[row[8]].exp() + 0.5)
            post = O.gp_posterior if model.gp_jitter else _posterior_fp32_distances
            fb, Sg = post(consts.xu[row[2]].cpu(), kvar, ls, qm, qS, xq, model.gp_jitter)
            bm, bc = bm + fb, bc + Sg
            kl = kl + O.gp_kl(qm, qS, n)
        L = torch.linalg.cholesky(bc + 1e-5 * torch.eye(B, dtype=torch.float64))
        tv = bm + L @ eps_beta[i].cpu().double()
        if row[1]:
            tv = K._hrf64(tv)
        tvs.append(tv); kls.append(float(kl))
    return torch.stack(tvs), np.array(kls)


def test_train_step_at_1040_graph_equals_eager_and_gains_match_oracle():
    """One train step at B = 1040 (C = 3: HRF, GP and linear covariates): replayed from the captured hipGraph == launched eagerly, bit
    for bit; the gains the step drew and its KL terms against the float64 oracle on the model's own parameters and draws."""
    ds = _dataset(1040, seed=9)
    B = 1040
    x = torch.from_numpy(ds['volumes'][:B]).cuda(); cov = torch.from_numpy(ds['covariates'][:B]).cuda()
    ids = torch.zeros(B, dtype=torch.int64, device='cuda')
    res = {}
    for mode in ('eager', 'graph'):
        torch.manual_seed(1)
        model = VAE(num_covariates=3, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda')
        model.use_hip_graph = (mode == 'graph')
        torch.manual_seed(77)
        loss = float(model.train_step(ids, cov, x))
        if mode == 'graph':
            assert model._graphs and all(v is not False for v in model._graphs.values()), 'capture fell back to eager'
        torch.cuda.synchronize()
        res[mode] = (loss, model.optimizer.groups[torch.float32]['g'].clone())
    print('peak allocated at B = 1040, C = 3: %.2f GB' % (torch.cuda.max_memory_allocated() / 1e9))
    assert res['eager'][0] == res['graph'][0], (res['eager'][0], res['graph'][0])
    assert torch.equal(res['eager'][1], res['graph'][1])
    # the gains of one forward with fixed draws against the float64 oracle
    noise = _noise(B)
    with torch.no_grad():
        out = model.forward_core(cov, x, noise=noise)
    tv_ref, kl_ref = _oracle_gains(model, cov[:, :3].float(), noise['eps_beta'])
    tv = out['task_var'].double().cpu()
    np.testing.assert_allclose(tv.numpy(), tv_ref.numpy(), rtol=2e-6, atol=2e-6 * float(tv_ref.abs().max()))
    np.testing.assert_allclose(model.last_gp_kl.cpu().numpy(), kl_ref, rtol=1e-6)


def test_batch_above_the_limit_is_refused_before_any_launch():
    ds = _dataset(8, seed=2)
    model = VAE(num_covariates=3, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda')
    x = torch.zeros(4097, *model.img_shape, device='cuda'); cov = torch.zeros(4097, 8, device='cuda')
    with pytest.raises(ValueError, match='4096'):
        model.train_step(torch.zeros(4097, dtype=torch.int64, device='cuda'), cov, x)


def _dp_rank(rank, world, port, out_dir, B):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    from vae_gam_amd import dp as dpmod
    ctx = dpmod.DataParallelContext.from_env(backend='gloo')
    ds = _dataset(B, seed=6)
    torch.manual_seed(1)
    model = VAE(num_covariates=3, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda', data_parallel=ctx, dp_gain='global')
    b = B // world
    x = torch.from_numpy(ds['volumes'][rank * b:(rank + 1) * b]).cuda(); cov = torch.from_numpy(ds['covariates'][rank * b:(rank + 1) * b]).cuda()
    loss = model.train_step(torch.zeros(b, dtype=torch.int64, device='cuda'), cov, x)
    g32 = model.optimizer.groups[torch.float32]
    torch.save({'loss': float(loss), 'g': g32['g'].cpu()}, os.path.join(out_dir, 'rank%d.pt' % rank))
    ctx.shutdown()


def test_data_parallel_two_ranks_at_2x520_equal_one_process_at_1040(tmp_path):
    """2 ranks (both on one GPU, gloo) x 520 volumes, dp_gain='global' (the joint draw over 1,040 volumes on every rank) == one process
    at 1,040, to the bands of test_data_parallel_two_ranks_on_gpu_equal_global_batch."""
    import socket
    import torch.multiprocessing as mp
    B = 1040
    ds = _dataset(B, seed=6)
    torch.manual_seed(1)
    model = VAE(num_covariates=3, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda')
    x = torch.from_numpy(ds['volumes'][:B]).cuda(); cov = torch.from_numpy(ds['covariates'][:B]).cuda()
    ref_loss = float(model.train_step(torch.zeros(B, dtype=torch.int64, device='cuda'), cov, x, noise=_noise(B)))
    ref_g = model.optimizer.groups[torch.float32]['g'].cpu()
    del model, x, cov
    torch.cuda.empty_cache()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_rank, args=(2, port, str(tmp_path), B), nprocs=2, join=True)
    for r in range(2):
        o = torch.load(os.path.join(tmp_path, 'rank%d.pt' % r))
        np.testing.assert_allclose(o['loss'], ref_loss, rtol=2e-5)
        assert float((o['g'] - ref_g).norm()) <= 5e-4 * float(ref_g.norm()), (float((o['g'] - ref_g).norm()), float(ref_g.norm()))
