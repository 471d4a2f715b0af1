"""Shared bodies of the derived-grid tests (schema.net_geometry's family rule and the embedding of any other grid): the embed copy
and the embedded GAM/ELBO kernels against float64, family grids against the CPU oracle, and the embedded model against the same
model built on its network grid.  Run on CPU tensors through the host build of the kernels (test_grid_emu.py) and on the GPU
through libvaegam_hip.so (test_grid_gpu.py)."""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops, schema
from vae_gam_amd.vae_reg_GP import VAE
import bridge
import kernel_cases as K
import vaegam_oracle as O

# (native, grid, B, C) of the kernel-level cases: mixed pads including 0 and a voxel count that is no multiple of the block tile;
# the smallest embedded model shape; the wider covariate instance (C > 8) with odd row lengths; native == grid
EMBED_CASES = [((5, 6, 7), (6, 9, 8), 3, 1), ((19, 21, 20), (22, 22, 22), 2, 3), ((9, 4, 33), (9, 6, 34), 5, 9),
               ((6, 9, 8), (6, 9, 8), 2, 0), ((6, 9, 8), (6, 9, 8), 2, 2)]
EMBED_IDS = ['5x6x7_in_6x9x8_C1', '19x21x20_in_22x22x22_C3', '9x4x33_in_9x6x34_C9', 'same_grid_C0', 'same_grid_C2']


def pad_to(x, nat, grid):
    """(..., *nat) -> (..., *grid), zeros at the high end of each axis"""
    return F.pad(x, (0, grid[2] - nat[2], 0, grid[1] - nat[1], 0, grid[0] - nat[0]))


def crop_to(x, nat):
    return x[..., :nat[0], :nat[1], :nat[2]]


def run_embed_copy_case(dev, nat, grid, B, seed=0):
    """vg_embed_volumes == torch.nn.functional.pad, bit for bit, on a destination that held garbage."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B,) + tuple(nat), generator=g)
    got = ops.embed_volumes(x.to(dev), nat, grid)
    assert got.shape == (B,) + tuple(grid)
    assert torch.equal(got.cpu(), pad_to(x, nat, grid))
    got2 = ops.embed_volumes(x.reshape(B, -1).to(dev), nat, grid)          # the flat layout the model hands over
    assert torch.equal(got2.cpu(), pad_to(x, nat, grid))


def run_gam_embed_case(dev, nat, grid, B, C, seed=0):
    """GamElboEmbed / gam_maps(nat, grid) against kernel_cases.ref_gam in float64 on the cropped logits (autograd for the
    gradients), with run_gam_case's tolerances; d_logits exactly zero in the padding; the bias hand-off; with nat == grid also
    against the plain GamElbo."""
    nat, grid = tuple(nat), tuple(grid)
    Vn, Vg = int(np.prod(nat)), int(np.prod(grid))
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((C + 1, B) + grid, generator=g)
    gain = torch.randn(C, B, generator=g)
    x = torch.rand(B, Vn, generator=g)
    eps = (-np.log(10) + 0.3 * torch.randn(Vn, generator=g, dtype=torch.float64))
    glm = torch.rand(C, Vn, generator=g)
    g1 = torch.randn(B, generator=g); g2 = torch.randn(C, B, generator=g)
    # float64 reference on the crop; the gradient w.r.t. the whole grid tensor is zero outside it by construction
    lr_ = logits.double().requires_grad_(True); gr_ = gain.double().requires_grad_(True); er_ = eps.clone().requires_grad_(True)
    slp_r, dist_r = K.ref_gam(crop_to(lr_, nat).reshape(C + 1, B, Vn), gr_, x.double(), er_, glm.double())
    tgt = [lr_, er_] + ([gr_] if C > 0 else [])
    gr = torch.autograd.grad((slp_r * g1.double()).sum() + (dist_r * g2.double()).sum(), tgt)
    dv = [logits.reshape(C + 1, B, Vg).to(dev).clone().requires_grad_(True), gain.to(dev).clone().requires_grad_(True), x.to(dev),
          eps.to(dev).clone().requires_grad_(True), glm.to(dev)]
    lbias = torch.nn.Parameter(torch.zeros(1, device=dev))
    lbias.grad = torch.zeros_like(lbias)
    slp, dist = ops.GamElboEmbed.apply(*dv, nat, grid, lbias)
    np.testing.assert_allclose(slp.detach().cpu().numpy(), slp_r.detach().numpy(), rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(dist.detach().cpu().numpy(), dist_r.detach().numpy(), rtol=2e-5, atol=1e-5)
    dtgt = [dv[0], dv[3]] + ([dv[1]] if C > 0 else [])
    gd = torch.autograd.grad((slp * g1.to(dev)).sum() + (dist * g2.to(dev)).sum(), dtgt)
    np.testing.assert_allclose(float(lbias.grad), float(gr[0].sum()), rtol=2e-4, atol=2e-4 * float(gr[0].abs().sum()) / max(Vn * (C + 1) * B, 1) ** 0.5)
    shapes = ((C + 1, B) + grid, (Vn,), (C, B))
    for a, b_, nm, sh in zip(gd, gr, ('d_logits', 'd_eps', 'd_gain'), shapes):
        sc = max(1.0, float(b_.abs().max()))
        np.testing.assert_allclose(a.cpu().numpy().reshape(sh), b_.numpy().reshape(sh), rtol=2e-4, atol=2e-5 * sc, err_msg=nm)
    dl = gd[0].cpu().reshape((C + 1, B) + grid)
    inside = torch.zeros(grid, dtype=torch.bool); inside[:nat[0], :nat[1], :nat[2]] = True
    pad_vals = dl[..., ~inside]
    assert pad_vals.numel() == (C + 1) * B * (Vg - Vn)
    assert torch.equal(pad_vals, torch.zeros_like(pad_vals)), 'd_logits must be exactly zero in the padding'
    maps = ops.gam_maps(dv[0].detach(), dv[1].detach(), dv[2], dv[3].detach(), dv[4], nat, grid)
    assert maps.shape == (C + 2, B, Vn)
    s = torch.sigmoid(crop_to(logits.double(), nat).reshape(C + 1, B, Vn))
    np.testing.assert_allclose(maps[0].cpu().numpy(), s[0].numpy(), atol=1e-6)
    for i in range(C):
        np.testing.assert_allclose(maps[i + 1].cpu().numpy(), (gain[i].double()[:, None] * s[i + 1]).numpy(), atol=1e-5 * max(1.0, float(gain[i].abs().max())))
    full = s[0] + sum(gain[i].double()[:, None] * s[i + 1] for i in range(C))
    np.testing.assert_allclose(maps[C + 1].cpu().numpy(), full.numpy(), atol=1e-5)
    if nat == grid:
        # the same kernels without the index decode: equal up to how the compiler contracts each instance (reduction order is shared)
        pv = [t.detach().clone().requires_grad_(t.requires_grad) for t in dv]
        pb = torch.nn.Parameter(torch.zeros(1, device=dev)); pb.grad = torch.zeros_like(pb)
        slp_p, dist_p = ops.GamElbo.apply(*pv, pb)
        gp = torch.autograd.grad((slp_p * g1.to(dev)).sum() + (dist_p * g2.to(dev)).sum(), [pv[0], pv[3]] + ([pv[1]] if C > 0 else []))
        np.testing.assert_allclose(slp.detach().cpu().numpy(), slp_p.detach().cpu().numpy(), rtol=1e-6)
        np.testing.assert_allclose(dist.detach().cpu().numpy(), dist_p.detach().cpu().numpy(), rtol=1e-6)
        np.testing.assert_allclose(float(lbias.grad), float(pb.grad), rtol=1e-5, atol=1e-6)
        for a, b_ in zip(gd, gp):
            np.testing.assert_allclose(a.cpu().numpy(), b_.cpu().numpy(), rtol=1e-5, atol=1e-7 * max(1.0, float(b_.abs().max())))


# ------------------------------------------------------------------------------------------------ models
def make_inputs(img, B, C, seed=0):
    """toy_case.make_inputs for any volume shape"""
    rng = np.random.Generator(np.random.PCG64(seed))
    V = int(np.prod(img))
    x = np.clip(0.5 + 0.25 * rng.normal(size=(B,) + tuple(img)), 0, 1).astype(np.float32)
    cont = rng.normal(size=(B, 6)); cont[0] = 6.0
    if B > 1:
        cont[1] = -4.0                      # (B = 1: the inducing points span [-4, 6] all the same)
    task = (np.arange(B) % 2).astype(np.float64); sex = (np.arange(B) >= B // 2).astype(np.float64)
    cov = np.stack([task, *cont.T, sex], 1)[:, :C].astype(np.float32)
    xu = [[min(float(cont[:, j].min()), -4.0) - 1e-3, float(cont[:, j].max()) + 1e-3] for j in range(6)]
    glm = rng.uniform(size=(V, 8)); glm = glm / glm.max(0, keepdims=True)
    glm = np.concatenate([np.arange(V, dtype=np.float64)[:, None], glm], 1)
    return torch.from_numpy(x), torch.from_numpy(cov), xu, glm


def make_model(dev, img, C, xu, glm, seed=1):
    torch.manual_seed(seed)
    return VAE(num_covariates=C, glm_maps=glm, xu_ranges=xu, device_name=dev, img_shape=img)


@dataclass
class FamilyOracleConfig(O.OracleConfig):
    """The oracle on a family grid: its own layer code, told the geometry the family rule derives."""

    @property
    def geom(self):
        g = schema.net_geometry(self.img, self.nf)
        assert g.pad == (0, 0, 0)
        return O.Geometry(self.img, self.nf, dec_seed=g.dec_seed, convt2_pad=(0, 0, 0), convt2_outpad=(0, 0, 0), convt4_kernel=(4, 4, 4))


def run_family_oracle_step(dev, img, B, C, seed=5):
    """One train step of the product model on a family grid against the CPU oracle on identical weights, inputs and noise:
    test_model_emu's tolerances (loss rtol 1e-4, per-tensor gradient error <= 5e-3 |g| + 1e-6)."""
    x, cov, xu, glm = make_inputs(img, B, C, seed)
    model = make_model(dev, img, C, xu, glm)
    assert model.img_pad == (0, 0, 0) and model.grid_shape == tuple(img)
    base = bridge.oracle_config(model)
    cfg = FamilyOracleConfig(**{k: getattr(base, k) for k in base.__dataclass_fields__})
    params = bridge.params_from_model(model)
    noise = O.draw_noise(B, cfg, torch.Generator().manual_seed(9))
    out, grads = O.loss_and_grads(params, cfg, x, cov, torch.from_numpy(glm), noise)
    ids = torch.zeros(B, dtype=torch.int64, device=dev)
    loss = model.train_step(ids, cov.to(dev), x.to(dev), noise=bridge.noise_to(noise, dev))
    np.testing.assert_allclose(loss.cpu().numpy(), out['loss'].detach().numpy(), rtol=1e-4)
    byname = bridge.model_param_by_oracle_name(model)
    for k, g in grads.items():
        if g is None or k.endswith(('.logkvar', '.log_ls')):
            continue
        a = byname[k].grad.double().flatten().cpu().numpy(); b = g.double().flatten().numpy()
        nb = np.sqrt((b * b).sum()); err = np.sqrt(((a - b) ** 2).sum())
        assert err <= 5e-3 * nb + 1e-6, (k, err, nb)


def _copy_model(E, F_):
    """E's parameters into F_ (built on E's network grid): everything but the log-precision map has the same shape; F_'s map equals
    E's on the native voxels."""
    with torch.no_grad():
        pe, pf = dict(E.named_parameters()), dict(F_.named_parameters())
        assert pe.keys() == pf.keys()
        for k, v in pe.items():
            if k == 'epsilon':
                pf[k].fill_(-np.log(10)); crop_to(pf[k], E.img_shape).copy_(v)
            else:
                assert pf[k].shape == v.shape, k
                pf[k].copy_(v)


def run_embedded_model_case(dev, nat, B, C, seed=7, grads=True, graph=False):
    """Model E on the native shape against model F on E's network grid with E's parameters, a grid-sized log-precision map equal to E's on
    the native part, the zero-padded batch and the same injected noise (see the checks' comments)."""
    nat = tuple(nat)
    grid = schema.grid_for(nat)
    assert grid != nat
    x, cov, xu, glm = make_inputs(nat, B, C, seed)
    _, _, _, glm_g = make_inputs(grid, B, C, seed + 1)                   # F's GLM maps only feed F's own (unused) loss
    E = make_model(dev, nat, C, xu, glm)
    Fm = make_model(dev, grid, C, xu, glm_g)
    assert E.img_shape == nat and E.grid_shape == grid and E.img_pad == tuple(g_ - n for g_, n in zip(grid, nat))
    assert E.img_dim == int(np.prod(nat)) and E.epsilon.shape == nat and E.glm_maps.shape[0] == E.img_dim
    with torch.no_grad():
        E.epsilon.add_(0.3 * torch.randn(nat, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dev))
    _copy_model(E, Fm)
    cfg = bridge.oracle_config(Fm)
    noise = bridge.noise_to(O.draw_noise(B, cfg, torch.Generator().manual_seed(9)), dev)
    xd, covd = x.to(dev), cov.to(dev)
    xg = pad_to(x, nat, grid).to(dev)
    ids = torch.zeros(B, dtype=torch.int64, device=dev)
    with torch.no_grad():
        oe = E.forward_core(covd, xd, noise, want_maps=True)
    assert B in E._plans_checked                     # the planners were asked about this batch size before its first launch
    Fm.optimizer.zero_grad()
    of = Fm.forward_core(covd, xg, noise, want_maps=True)
    # upstream of the loss E and F run the same launches on the same data
    for k in ('mu', 'u', 'd', 'z', 'logits'):
        assert torch.equal(oe[k], of[k].detach()), k
    # maps: native columns, equal to the crop of F's
    Vn = E.img_dim
    assert oe['maps'].shape == (C + 2, B, Vn)
    assert torch.equal(oe['maps'], crop_to(of['maps'].view(C + 2, B, *grid), nat).reshape(C + 2, B, Vn))
    _, _, imgs = E.forward(ids, covd, xd, 'test', return_latent_rec=True, train_mode=False, noise=noise)
    assert imgs['base'].shape == (B, Vn) and imgs['full_rec'].shape == (B, Vn)
    dec = E.decode(oe['z'].new_zeros(B, E.z_dim))
    assert dec.shape == (B, Vn)
    # the loss restated in float64 from F's outputs: -mean(-kl_z + slp) + gp_kl_scale*gp_kl + glm_reg_scale*B*sum(dist), with slp / dist
    # from ref_gam on the cropped logits, the native data, the native part of F's log-precision map and E's GLM maps
    logits_f = of['logits']
    dl = {}
    logits_f.register_hook(lambda g_: dl.__setitem__('g', g_))
    eps_n = crop_to(Fm.epsilon, nat).reshape(-1)
    glm_n = torch.from_numpy(glm[:, 1:C + 1].T.copy()).to(dev)
    slp, dist = K.ref_gam(crop_to(logits_f.view(C + 1, B, *grid), nat).reshape(C + 1, B, Vn).double(), of['task_var'].double(),
                          xd.reshape(B, Vn).double(), eps_n, glm_n)
    loss64 = -(-of['kl_z'].double() + slp).mean() + float(Fm.gp_kl_scale) * of['gp_kl_loss'].double().sum() \
        + float(Fm.glm_reg_scale) * B * dist.sum()
    loss_e = E.train_step(ids, covd, xd, noise=noise)
    print('embedded %r in %r: loss %.6f, float64 restatement %.6f' % (nat, grid, float(loss_e), float(loss64.detach())))
    assert np.isfinite(float(loss_e))
    np.testing.assert_allclose(float(loss_e), float(loss64.detach()), rtol=1e-4)
    np.testing.assert_allclose(float(oe['loss']), float(loss64.detach()), rtol=1e-4)
    for k in (E.optimizer.names[i] for i in sorted(E.optimizer.used)):
        assert torch.isfinite(dict(E.named_parameters())[k].grad).all(), k
    if grads:
        loss64.backward()
        ops.join_side_stream(xd.device)
        pe, pf = dict(E.named_parameters()), dict(Fm.named_parameters())
        used = [E.optimizer.names[i] for i in sorted(E.optimizer.used)]
        for k in used:
            a = pe[k].grad.double().cpu()
            if k == 'convt5.bias':                   # F's forward left this gradient to its own GAM/ELBO node, which the restated loss bypasses
                b = dl['g'].double().sum().reshape(a.shape).cpu()
            elif k == 'epsilon':
                b = crop_to(pf[k].grad.double().cpu(), nat)
            else:
                b = pf[k].grad.double().cpu()
            err = float((a - b).norm()); nb = float(b.norm())
            assert err <= 5e-3 * nb + 1e-6, (k, err, nb)
    if graph:
        res = {}
        for mode in ('eager', 'graph'):
            m = make_model(dev, nat, C, xu, glm)
            m.use_hip_graph = mode == 'graph'
            torch.manual_seed(77)
            res[mode] = [float(m.train_step(ids, covd, xd)) for _ in range(2)]
            if mode == 'graph':
                assert m._graphs and all(v is not False for v in m._graphs.values()), 'capture fell back to eager'
        assert res['eager'] == res['graph'], res
    return E
