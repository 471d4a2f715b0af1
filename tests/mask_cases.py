"""Shared bodies of the brain-mask tests: the masked GAM/ELBO kernels (ops.GamElboMasked, ops.gam_maps(mask=...)) against float64
on the voxels of the mask, and the masked model (VAE(mask=...)): loss, parameter gradients, the log-precision map under training, the
exports, checkpoints and refusals.  Run on CPU tensors through the host build of the kernels (test_mask_emu.py) and on the GPU through
libvaegam_hip.so (test_mask_gpu.py)."""
import os

import numpy as np
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops, schema
from vae_gam_amd.vae_reg_GP import VAE
import bridge
import grid_cases as GC
import kernel_cases as K
import vaegam_oracle as O


# ------------------------------------------------------------------------------------------------ masks
def random_mask(nat, seed=3, p=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(tuple(nat), generator=g) < p).to(torch.uint8)


def block_out_mask(nat, seed=3):
    """scattered random mask with the flat voxels 1024..2047 all out: one forward block (256 threads x 4 voxels) and four backward
    blocks (16 waves) without a single voxel that counts"""
    m = random_mask(nat, seed).reshape(-1)
    m[1024:2048] = 0
    return m.reshape(tuple(nat))


def one_voxel_mask(nat):
    m = torch.zeros(tuple(nat), dtype=torch.uint8)
    m[3, 5, 2] = 1
    return m


def ones_mask(nat):
    return torch.ones(tuple(nat), dtype=torch.uint8)


def box_mask(nat, box):
    m = torch.zeros(tuple(nat), dtype=torch.uint8)
    m[:box[0], :box[1], :box[2]] = 1
    return m


def ellipsoid_mask(nat):
    """the ellipsoid inscribed in the box: about half of its voxels"""
    ax = [(np.arange(n) - (n - 1) / 2.0) / (n / 2.0) for n in nat]
    r2 = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2
    return torch.from_numpy((r2 <= 1.0).astype(np.uint8))


# (native, grid, B, C, mask) of the kernel-level cases
KERNEL_CASES = [((12, 13, 14), (12, 13, 14), 3, 2, block_out_mask), ((5, 6, 7), (6, 9, 8), 3, 1, random_mask),
                ((9, 4, 33), (9, 6, 34), 9, 9, random_mask), ((6, 9, 8), (6, 9, 8), 2, 2, one_voxel_mask),
                ((6, 9, 8), (6, 9, 8), 2, 0, ones_mask), ((6, 9, 8), (6, 9, 8), 2, 2, ones_mask)]
KERNEL_IDS = ['12x13x14_block_out_C2', '5x6x7_in_6x9x8_C1', '9x4x33_in_9x6x34_B9_C9', 'one_voxel_C2', 'all_ones_C0', 'all_ones_C2']


def _kernel_inputs(nat, grid, B, C, seed):
    """the draws of grid_cases.run_gam_embed_case, in its order"""
    Vn = int(np.prod(nat))
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((C + 1, B) + tuple(grid), generator=g)
    gain = torch.randn(C, B, generator=g)
    x = torch.rand(B, Vn, generator=g)
    eps = (-np.log(10) + 0.3 * torch.randn(Vn, generator=g, dtype=torch.float64))
    glm = torch.rand(C, Vn, generator=g)
    g1 = torch.randn(B, generator=g); g2 = torch.randn(C, B, generator=g)
    return logits, gain, x, eps, glm, g1, g2


def _device_args(dev, logits, gain, x, eps, glm):
    G, B = logits.shape[:2]
    return [logits.reshape(G, B, -1).to(dev).clone().requires_grad_(True), gain.to(dev).clone().requires_grad_(True), x.to(dev),
            eps.to(dev).clone().requires_grad_(True), glm.to(dev)]


def _bias(dev):
    b = torch.nn.Parameter(torch.zeros(1, device=dev))
    b.grad = torch.zeros_like(b)
    return b


def run_gam_masked_case(dev, nat, grid, B, C, make_mask, seed=0):
    """GamElboMasked / gam_maps(mask=...) against kernel_cases.ref_gam in float64 on the voxels of the mask only (logits cropped to
    nat, then logits, x, eps and glm indexed with the boolean mask; autograd for the gradients, which scatters them back), with the
    bands of grid_cases.run_gam_embed_case.  Exactly: d_logits == 0 at every masked-out and every padding voxel, d_eps == 0.0 and
    maps == 0 outside the mask.  An unmasked case of the same shape runs first, so that the allocator's cached workspace holds
    non-zero data where the masked backward must store its own partials.  With an all-ones mask on one grid also against the plain
    GamElbo."""
    nat, grid = tuple(nat), tuple(grid)
    Vn, Vg = int(np.prod(nat)), int(np.prod(grid))
    logits, gain, x, eps, glm, g1, g2 = _kernel_inputs(nat, grid, B, C, seed)
    mask = make_mask(nat)
    mb = mask.reshape(-1).bool()
    assert mask.dtype == torch.uint8 and int(mb.sum()) > 0
    # float64 reference on the voxels of the mask
    lr_ = logits.double().requires_grad_(True); gr_ = gain.double().requires_grad_(True); er_ = eps.clone().requires_grad_(True)
    slp_r, dist_r = K.ref_gam(GC.crop_to(lr_, nat).reshape(C + 1, B, Vn)[:, :, mb], gr_, x.double()[:, mb], er_[mb], glm.double()[:, mb])
    tgt = [lr_, er_] + ([gr_] if C > 0 else [])
    gr = torch.autograd.grad((slp_r * g1.double()).sum() + (dist_r * g2.double()).sum(), tgt)
    # the unmasked step of the same shape first: its backward leaves d sigma partials of every native voxel in the workspace
    uv = _device_args(dev, logits, gain, x, eps, glm)
    if nat == grid:
        slp_u, dist_u = ops.GamElbo.apply(*uv, _bias(dev))
    else:
        slp_u, dist_u = ops.GamElboEmbed.apply(*uv, nat, grid, _bias(dev))
    gu = torch.autograd.grad((slp_u * g1.to(dev)).sum() + (dist_u * g2.to(dev)).sum(), [uv[0], uv[3]])
    assert int((gu[1] != 0).sum()) == Vn                # (every voxel's d_eps is non-zero there)
    del slp_u, dist_u, gu
    dv = _device_args(dev, logits, gain, x, eps, glm)
    md = mask.to(dev)
    lbias = _bias(dev)
    slp, dist = ops.GamElboMasked.apply(*dv, md, nat, grid, lbias)
    np.testing.assert_allclose(slp.detach().cpu().numpy(), slp_r.detach().numpy(), rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(dist.detach().cpu().numpy(), dist_r.detach().numpy(), rtol=2e-5, atol=1e-5)
    dtgt = [dv[0], dv[3]] + ([dv[1]] if C > 0 else [])
    gd = torch.autograd.grad((slp * g1.to(dev)).sum() + (dist * g2.to(dev)).sum(), dtgt)
    Vm = int(mb.sum())
    np.testing.assert_allclose(float(lbias.grad), float(gr[0].sum()), rtol=2e-4, atol=2e-4 * float(gr[0].abs().sum()) / max(Vn * (C + 1) * B, 1) ** 0.5)
    shapes = ((C + 1, B) + grid, (Vn,), (C, B))
    for a, b_, nm, sh in zip(gd, gr, ('d_logits', 'd_eps', 'd_gain'), shapes):
        sc = max(1.0, float(b_.abs().max()))
        np.testing.assert_allclose(a.cpu().numpy().reshape(sh), b_.numpy().reshape(sh), rtol=2e-4, atol=2e-5 * sc, err_msg=nm)
    # exact zeros: d_logits at every masked-out and every padding voxel, d_eps outside the mask
    counts = torch.zeros(grid, dtype=torch.bool)
    counts[:nat[0], :nat[1], :nat[2]] = mask.bool()
    dl = gd[0].cpu().reshape((C + 1, B) + grid)
    out_vals = dl[..., ~counts]
    assert out_vals.numel() == (C + 1) * B * (Vg - Vm)
    assert torch.equal(out_vals, torch.zeros_like(out_vals)), 'd_logits must be exactly zero outside the mask and in the padding'
    de = gd[1].cpu()
    assert de.dtype == torch.float64 and torch.equal(de[~mb], torch.zeros(Vn - Vm, dtype=torch.float64)), 'd_eps must be exactly 0.0 outside the mask'
    if Vm > 1:
        assert int((de[mb] != 0).sum()) == Vm
    # maps: as run_gam_embed_case inside the mask, exactly zero outside; on a destination that held something else
    torch.full((C + 2, B, Vn), 7.0, device=dev)
    maps = ops.gam_maps(dv[0].detach(), dv[1].detach(), dv[2], dv[3].detach(), dv[4], nat, grid, mask=md)
    assert maps.shape == (C + 2, B, Vn)
    mc = maps.cpu()
    assert torch.equal(mc[:, :, ~mb], torch.zeros(C + 2, B, Vn - Vm)), 'maps must be exactly zero outside the mask'
    s = torch.sigmoid(GC.crop_to(logits.double(), nat).reshape(C + 1, B, Vn))[:, :, mb]
    np.testing.assert_allclose(mc[0][:, mb].numpy(), s[0].numpy(), atol=1e-6)
    for i in range(C):
        np.testing.assert_allclose(mc[i + 1][:, mb].numpy(), (gain[i].double()[:, None] * s[i + 1]).numpy(), atol=1e-5 * max(1.0, float(gain[i].abs().max())))
    full = s[0] + sum(gain[i].double()[:, None] * s[i + 1] for i in range(C))
    np.testing.assert_allclose(mc[C + 1][:, mb].numpy(), full.numpy(), atol=1e-5)
    if nat == grid and Vm == Vn:
        # all ones: the plain kernels with the mask test, equal up to how the compiler contracts each instance (run_gam_embed_case's
        # instance-to-instance bands)
        pv = [t.detach().clone().requires_grad_(t.requires_grad) for t in dv]
        pb = _bias(dev)
        slp_p, dist_p = ops.GamElbo.apply(*pv, pb)
        gp = torch.autograd.grad((slp_p * g1.to(dev)).sum() + (dist_p * g2.to(dev)).sum(), [pv[0], pv[3]] + ([pv[1]] if C > 0 else []))
        np.testing.assert_allclose(slp.detach().cpu().numpy(), slp_p.detach().cpu().numpy(), rtol=1e-6)
        np.testing.assert_allclose(dist.detach().cpu().numpy(), dist_p.detach().cpu().numpy(), rtol=1e-6)
        np.testing.assert_allclose(float(lbias.grad), float(pb.grad), rtol=1e-5, atol=1e-6)
        for a, b_ in zip(gd, gp):
            np.testing.assert_allclose(a.cpu().numpy(), b_.cpu().numpy(), rtol=1e-5, atol=1e-7 * max(1.0, float(b_.abs().max())))


def run_box_mask_equals_embed_case(dev, grid=(6, 9, 8), box=(5, 7, 6), B=2, C=2, seed=0):
    """'masked out' and 'padding' are one notion: GamElboMasked on `grid` with the box mask [:5,:7,:6] against GamElboEmbed with
    nat = the box inside the same grid, on the same logits and on data / eps / glm that are the box of the masked case's.  Same
    per-voxel arithmetic, same threads, same reduction order: the instance-to-instance bands of run_gam_embed_case."""
    grid, box = tuple(grid), tuple(box)
    Vg, Vb = int(np.prod(grid)), int(np.prod(box))
    logits, gain, x, eps, glm, g1, g2 = _kernel_inputs(grid, grid, B, C, seed)
    mask = box_mask(grid, box)
    mb = mask.reshape(-1).bool()
    dv = _device_args(dev, logits, gain, x, eps, glm)
    lb = _bias(dev)
    slp, dist = ops.GamElboMasked.apply(*dv, mask.to(dev), grid, grid, lb)
    gd = torch.autograd.grad((slp * g1.to(dev)).sum() + (dist * g2.to(dev)).sum(), [dv[0], dv[3], dv[1]])
    ev = _device_args(dev, logits, gain, x[:, mb].contiguous(), eps[mb].contiguous(), glm[:, mb].contiguous())
    eb = _bias(dev)
    slp_e, dist_e = ops.GamElboEmbed.apply(*ev, box, grid, eb)
    ge = torch.autograd.grad((slp_e * g1.to(dev)).sum() + (dist_e * g2.to(dev)).sum(), [ev[0], ev[3], ev[1]])
    np.testing.assert_allclose(slp.detach().cpu().numpy(), slp_e.detach().cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(dist.detach().cpu().numpy(), dist_e.detach().cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(float(lb.grad), float(eb.grad), rtol=1e-5, atol=1e-6)
    d_eps_box = gd[1].cpu()[mb]
    assert torch.equal(gd[1].cpu()[~mb], torch.zeros(Vg - Vb, dtype=torch.float64))
    for a, b_ in ((gd[0].cpu(), ge[0].cpu()), (d_eps_box, ge[1].cpu()), (gd[2].cpu(), ge[2].cpu())):
        np.testing.assert_allclose(a.numpy(), b_.numpy(), rtol=1e-5, atol=1e-7 * max(1.0, float(b_.abs().max())))
    m_mask = ops.gam_maps(dv[0].detach(), dv[1].detach(), dv[2], dv[3].detach(), dv[4], grid, grid, mask=mask.to(dev)).cpu()
    m_emb = ops.gam_maps(ev[0].detach(), ev[1].detach(), ev[2], ev[3].detach(), ev[4], box, grid).cpu()
    np.testing.assert_allclose(m_mask[:, :, mb].numpy(), m_emb.numpy(), rtol=1e-6, atol=1e-7)
    assert torch.equal(m_mask[:, :, ~mb], torch.zeros(C + 2, B, Vg - Vb))


def run_bad_arguments_case(dev):
    """the _masked entry points report a null mask and a native grid that does not fit through the library's status"""
    from vae_gam_amd import _lib
    nat, grid, B, C = (5, 6, 7), (6, 9, 8), 2, 1
    logits, gain, x, eps, glm, _, _ = _kernel_inputs(nat, grid, B, C, 0)
    dv = [t.detach() for t in _device_args(dev, logits, gain, x, eps, glm)]
    lib = _lib.get_lib()
    ws = torch.empty(lib.size('vg_gam_ws_bytes', C, B, int(np.prod(grid))) // 4 + 1, dtype=torch.float32, device=dev)
    slp = torch.zeros(B, device=dev); dist = torch.zeros(C, B, device=dev)
    m = ones_mask(nat).to(dev)
    p = ops._p
    for mask_p, n_, g_, pat in ((None, nat, grid, 'no mask'), (p(m), grid, nat, 'must fit'), (p(m), (1 << 11,) * 3, (1 << 11,) * 3, 'must fit')):
        try:
            ops._call(dv[2], 'vg_gam_elbo_fwd_masked', p(dv[0]), p(dv[1]), p(dv[2]), p(dv[3]), p(dv[4]), mask_p, C, B, ops._i3(n_), ops._i3(g_),
                      p(ws), p(slp), p(dist), None)
        except _lib.VgError as e:
            assert pat in str(e), (pat, str(e))
        else:
            raise AssertionError('vg_gam_elbo_fwd_masked accepted bad arguments (%s)' % pat)
    with np.testing.assert_raises(ValueError):
        ops.gam_maps(dv[0], dv[1], dv[2], dv[3], dv[4], nat, grid, mask=m[:-1])
    with np.testing.assert_raises(ValueError):
        ops.gam_maps(dv[0], dv[1], dv[2], dv[3], dv[4], nat, grid, mask=m.float())


# ------------------------------------------------------------------------------------------------ model
MODEL_B, MODEL_C = 3, 3
MODEL_SHAPES = [(22, 22, 22), (19, 21, 20)]
MODEL_IDS = ['22x22x22', '19x21x20_in_22x22x22']


def make_model(dev, img, xu, glm, seed=1, **kw):
    torch.manual_seed(seed)
    return VAE(num_covariates=MODEL_C, glm_maps=glm, xu_ranges=xu, device_name=dev, img_shape=img, **kw)


def _case(dev, img, seed=7):
    img = tuple(img)
    x, cov, xu, glm = GC.make_inputs(img, MODEL_B, MODEL_C, seed)
    mask = ellipsoid_mask(img)
    probe = make_model(dev, img, xu, glm)
    noise = bridge.noise_to(O.draw_noise(MODEL_B, bridge.oracle_config(probe), torch.Generator().manual_seed(9)), dev)
    ids = torch.zeros(MODEL_B, dtype=torch.int64, device=dev)
    return dict(img=img, x=x.to(dev), cov=cov.to(dev), xu=xu, glm=glm, mask=mask, noise=noise, ids=ids, plain=probe)


def _restated_loss(m, out, x, mb):
    """ops.ElboLoss's assembly in float64 from the step's own logits, task_var, kl_z and gp_kl_loss, with ref_gam on the voxels of the
    mask (mb: flat boolean mask on the native grid, on the device)"""
    C, B, nat, grid = m.num_covariates, x.shape[0], m.img_shape, m.grid_shape
    Vn = m.img_dim
    lg = GC.crop_to(out['logits'].view(C + 1, B, *grid), nat).reshape(C + 1, B, Vn).double()[:, :, mb]
    glm_n = m.glm_maps[:, 1:C + 1].t().contiguous().float().double()[:, mb]
    slp, dist = K.ref_gam(lg, out['task_var'].double(), x.reshape(B, Vn).double()[:, mb], m.epsilon.view(-1)[mb], glm_n)
    loss = -(-out['kl_z'].double() + slp).mean() + float(m.gp_kl_scale) * out['gp_kl_loss'].double().sum() \
        + float(m.glm_reg_scale) * B * dist.sum()
    return loss, slp, dist


def run_masked_model_loss_and_grads(dev, img):
    """forward_core of the masked model: loss, sum_log_prob and dist against the float64 restatement on the mask (kernel-level bands,
    loss rel 1e-4), and every parameter gradient but convt5.bias's against the gradients of that restatement back-propagated from the
    logits of an identical second forward (|a - b| <= 1e-3 rms(b) + 1e-6 per entry)."""
    c = _case(dev, img)
    m = make_model(dev, c['img'], c['xu'], c['glm'], mask=c['mask'])
    assert m.mask.dtype == torch.uint8 and tuple(m.mask.shape) == c['img'] and m.mask.device.type == torch.device(dev).type
    assert m.mask_voxels == int(c['mask'].sum()) and 0 < m.mask_voxels < m.img_dim
    with torch.no_grad():
        m.epsilon.add_(0.3 * torch.randn(c['img'], generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dev))
    mb = m.mask.view(-1).bool()
    used = [m.optimizer.names[i] for i in sorted(m.optimizer.used)]
    params = dict(m.named_parameters())
    m.optimizer.zero_grad()
    out = m.forward_core(c['cov'], c['x'], c['noise'])
    loss64, slp64, dist64 = _restated_loss(m, out, c['x'], mb)
    print('masked %r: loss %.6f, float64 restatement %.6f' % (c['img'], float(out['loss'].detach()), float(loss64.detach())))
    np.testing.assert_allclose(out['sum_log_prob'].detach().cpu().numpy(), slp64.detach().cpu().numpy(), rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(out['dist'].detach().cpu().numpy(), dist64.detach().cpu().numpy(), rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(float(out['loss'].detach()), float(loss64.detach()), rtol=1e-4)
    out['loss'].backward()
    ops.join_side_stream(c['x'].device)
    got = {k: params[k].grad.detach().double().cpu().clone() for k in used}
    m.optimizer.zero_grad()
    out2 = m.forward_core(c['cov'], c['x'], c['noise'])
    assert torch.equal(out2['logits'].detach(), out['logits'].detach())
    loss64b, _, _ = _restated_loss(m, out2, c['x'], mb)
    loss64b.backward()
    ops.join_side_stream(c['x'].device)
    for k in used:
        if k == 'convt5.bias':          # travels by the hand-off of the GAM/ELBO node, which the restatement bypasses: kernel level
            continue
        a, b = got[k], params[k].grad.detach().double().cpu()
        rms = float(b.pow(2).mean().sqrt())
        err = float((a - b).abs().max())
        assert err <= 1e-3 * rms + 1e-6, (k, err, rms)
    eg = got['epsilon'].reshape(-1)
    assert torch.equal(eg[~mb.cpu()], torch.zeros(int((~mb).sum()), dtype=torch.float64))
    return c, m


def run_masked_model_training(dev, img, graph=False):
    """Two train steps: epsilon outside the mask keeps its initial bits, inside it moves, the loss is finite.  graph: the captured
    step replays to the same losses and parameters as the eager one."""
    c = _case(dev, img)
    res = {}
    for mode in (('eager', 'graph') if graph else ('eager',)):
        m = make_model(dev, c['img'], c['xu'], c['glm'], mask=c['mask'])
        m.use_hip_graph = mode == 'graph'
        eps0 = m.epsilon.detach().clone()
        torch.manual_seed(77)
        losses = [float(m.train_step(c['ids'], c['cov'], c['x'])) for _ in range(2)]
        if mode == 'graph':
            assert m._graphs and all(v is not False for v in m._graphs.values()), 'capture fell back to eager'
        assert all(np.isfinite(v) for v in losses), losses
        mb = m.mask.bool()
        eps1 = m.epsilon.detach()
        assert torch.equal(eps1[~mb], eps0[~mb]), 'epsilon outside the mask must keep its bits'
        assert bool((eps1[mb] != eps0[mb]).all()), 'epsilon inside the mask must move'
        res[mode] = (losses, m.optimizer.groups[torch.float32]['p'].clone(), eps1.clone())
    if graph:
        assert res['eager'][0] == res['graph'][0], (res['eager'][0], res['graph'][0])
        assert torch.equal(res['eager'][1], res['graph'][1]) and torch.equal(res['eager'][2], res['graph'][2])


def _loss_and_grads(m, c):
    m.optimizer.zero_grad()
    out = m.forward_core(c['cov'], c['x'], c['noise'])
    out['loss'].backward()
    ops.join_side_stream(c['x'].device)
    return out['loss'].detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def run_mask_none_and_all_ones(dev, img):
    """mask=None: bit-identical loss and gradients to a model built without the argument (and on the entry points it used before).
    All-ones mask: the loss within rel 1e-6 of the mask-free model's."""
    c = _case(dev, img)
    plain = c['plain']
    assert plain.mask is None and plain.mask_voxels is None
    l0, g0 = _loss_and_grads(plain, c)
    none = make_model(dev, c['img'], c['xu'], c['glm'], mask=None)
    l1, g1 = _loss_and_grads(none, c)
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    ones = make_model(dev, c['img'], c['xu'], c['glm'], mask=np.ones(c['img'], dtype=np.float32))
    assert ones.mask_voxels == ones.img_dim
    with torch.no_grad():
        l2 = ones.forward_core(c['cov'], c['x'], c['noise'])['loss']
    np.testing.assert_allclose(float(l2), float(l0), rtol=1e-6)


def run_export_case(dev, img, tmp_path):
    """reconstruct(..., write_volumes=True): every NIfTI written is exactly 0 outside the mask, and so are the recon_sums; the
    averages of build_model_recons.mk_avg_maps likewise."""
    from vae_gam_amd import DataClass_GP as D, build_model_recons as R
    c = _case(dev, img)
    m = make_model(dev, c['img'], c['xu'], c['glm'], mask=c['mask'], save_dir=str(tmp_path))
    sample = {'volume': c['x'].cpu(), 'covariates': torch.cat([c['cov'].cpu(), torch.zeros(MODEL_B, 8 - MODEL_C)], 1),
              'subjid': torch.tensor([0, 0, 1]), 'vol_num': torch.tensor([0, 1, 0])}
    dirs = [str(tmp_path / 's0'), str(tmp_path / 's1')]
    sums, counts = m.reconstruct([sample], [], dirs, write_volumes=True, noise=lambda bi, n: c['noise'])
    out = ~c['mask'].bool().numpy()
    files = [os.path.join(dirs[s], 'vol_%d' % v, f) for s, v in ((0, 0), (0, 1), (1, 0)) for f in sorted(os.listdir(os.path.join(dirs[s], 'vol_%d' % v)))]
    assert len(files) == 3 * (MODEL_C + 2)
    for f in files:
        a = np.asarray(D.read_nifti1(f))
        assert tuple(a.shape[:3]) == c['img']
        assert np.isfinite(a).all() and (a[out] == 0).all(), f
        assert (a[~out] != 0).any(), f
    assert counts.tolist() == [2.0, 1.0]
    for k, s in sums.items():
        s = s.cpu().reshape(2, *c['img'])
        assert bool((s[:, torch.from_numpy(out)] == 0).all()), k
    ref = m.recon_sums
    assert ref[0] is sums


def run_checkpoint_case(dev, img, tmp_path):
    """A checkpoint carries the mask (and only a masked model's does); a mask-free model that loads it evaluates the masked loss."""
    c = _case(dev, img)
    m = make_model(dev, c['img'], c['xu'], c['glm'], mask=c['mask'], save_dir=str(tmp_path))
    m.train_step(c['ids'], c['cov'], c['x'], noise=c['noise'])
    m.save_state('masked.tar')
    ck = torch.load(str(tmp_path / 'masked.tar'), map_location='cpu', weights_only=False)
    assert ck['mask'].dtype == torch.uint8 and tuple(ck['mask'].shape) == c['img'] and torch.equal(ck['mask'], c['mask'])
    with torch.no_grad():
        want = m.forward_core(c['cov'], c['x'], c['noise'])['loss'].clone()
    plain = c['plain']
    plain.save_dir = str(tmp_path)
    plain.save_state('plain.tar')
    assert 'mask' not in torch.load(str(tmp_path / 'plain.tar'), map_location='cpu', weights_only=False)
    with torch.no_grad():
        before = plain.forward_core(c['cov'], c['x'], c['noise'])['loss'].clone()
    plain._graphs['stale'] = False
    plain.load_state(str(tmp_path / 'masked.tar'))
    assert not plain._graphs                                  # a captured step would hold the previous mask pointer
    assert torch.equal(plain.mask.cpu(), c['mask']) and plain.mask_voxels == m.mask_voxels
    with torch.no_grad():
        got = plain.forward_core(c['cov'], c['x'], c['noise'])['loss']
    assert torch.equal(got, want) and not torch.equal(before, want)
    # a checkpoint without the key leaves the mask as constructed
    m.load_state(str(tmp_path / 'plain.tar'))
    assert torch.equal(m.mask.cpu(), c['mask'])


def run_refusals(dev, tmp_path):
    import pytest
    from vae_gam_amd import multsubj_reg_run_GP as cli, nifti
    img = (19, 21, 20)
    _, _, xu, glm = GC.make_inputs(img, MODEL_B, MODEL_C, 7)
    with pytest.raises(ValueError, match=r'mask has the shape 19x21x21.*19x21x20'):
        make_model(dev, img, xu, glm, mask=np.ones((19, 21, 21), dtype=np.uint8))
    with pytest.raises(ValueError, match='no voxel set'):
        make_model(dev, img, xu, glm, mask=torch.zeros(img))
    # files: .npy, .nii (4-D: the first volume), and a --mask that disagrees with --img_shape
    np.save(str(tmp_path / 'm.npy'), ellipsoid_mask(img).numpy().astype(np.float32))
    four_d = np.stack([ellipsoid_mask(img).numpy().astype(np.int16), np.zeros(img, dtype=np.int16)], -1)
    nifti.write_nifti1(str(tmp_path / 'm4.nii'), four_d)
    for f in ('m.npy', 'm4.nii'):
        mm = make_model(dev, img, xu, glm, mask=str(tmp_path / f))
        assert torch.equal(mm.mask.cpu(), ellipsoid_mask(img)), f
    with pytest.raises(ValueError, match=r'--img_shape is 22x22x22 but the mask .*m\.npy has the spatial shape 19x21x20'):
        cli.main(['--mask', str(tmp_path / 'm.npy'), '--img_shape', '22', '22', '22', '--save_dir', str(tmp_path)])
    with pytest.raises(SystemExit, match='does not exist'):
        cli.main(['--mask', str(tmp_path / 'nothing.nii'), '--save_dir', str(tmp_path)])
    assert schema.grid_for(img) == (22, 22, 22)
