"""Shared bodies of the kernel parity tests: each HIP operator against a plain PyTorch reference of the same
maths -- fp32 for the layer and chain cases, float64 where a case's docstring says so (the conv_mm, weight-gradient,
FC and gain case matrices; the batch-norm kernels have theirs in bn_cases.py).  Run on CPU tensors through the host build of the kernels
(tests/emu, index-arithmetic check) and on the GPU through libvaegam_hip.so (-m gpu)."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
from vae_gam_amd.ops import ConvSpec

# (name, spec, small input size) -- one entry per layer of vae_reg_GP.py:189-215, spatial sizes shrunk
LAYERS = [
    ('conv1', ConvSpec('conv', 1, 8, (3, 3, 3), 1), (7, 9, 8)),
    ('conv2', ConvSpec('conv', 8, 8, (3, 3, 3), 2), (9, 11, 8)),
    ('conv3', ConvSpec('conv', 8, 16, (3, 3, 3), 1), (5, 7, 6)),
    ('conv4', ConvSpec('conv', 16, 16, (3, 3, 3), 2), (7, 9, 6)),
    ('conv5', ConvSpec('conv', 16, 16, (3, 3, 3), 1), (4, 5, 3)),
    ('convt1', ConvSpec('convt', 16, 16, (3, 3, 3), 1), (3, 4, 5)),
    ('convt2', ConvSpec('convt', 16, 16, (3, 3, 3), 2, (1, 0, 1), (1, 0, 1)), (4, 5, 4)),
    ('convt3', ConvSpec('convt', 16, 8, (3, 3, 3), 1), (4, 6, 5)),
    ('convt4', ConvSpec('convt', 8, 8, (5, 3, 3), 2), (4, 5, 4)),
    ('convt5', ConvSpec('convt', 8, 1, (3, 3, 3), 1), (5, 7, 6)),
]

# wide rows (>= 12 positions per row): the geometries that take the row-walking weight-gradient kernel and whole-plane tiles
WIDE_LAYERS = [
    ('conv1_wide', ConvSpec('conv', 1, 8, (3, 3, 3), 1), (5, 9, 16)),
    ('conv2_wide', ConvSpec('conv', 8, 8, (3, 3, 3), 2), (7, 11, 27)),
    ('conv3_wide', ConvSpec('conv', 8, 16, (3, 3, 3), 1), (4, 7, 15)),
    ('convt3_wide', ConvSpec('convt', 16, 8, (3, 3, 3), 1), (3, 6, 12)),
    ('convt4_wide', ConvSpec('convt', 8, 8, (5, 3, 3), 2), (3, 5, 12)),
    ('convt4hr_wide', ConvSpec('convt', 8, 8, (4, 4, 4), 2), (3, 3, 12)),
    ('convt5_wide', ConvSpec('convt', 8, 1, (3, 3, 3), 1), (4, 7, 13)),
    # large planes (36x36 / 33x33 window rows).  Their weight gradients run on the row-walking kernel like every other case, with tiles
    # ONE position row high (3 planes deep) and so 36 / 16 row blocks per plane: convt5_split's single window channel in the general
    # k-step loop (rows of 36 = 9 k-steps in blocks of 3), convt4_split with the plane-shift packing, its 8 window channels resident,
    # rows of 16 = one block of 4 k-steps
    ('convt5_split', ConvSpec('convt', 3, 1, (3, 3, 3), 1), (4, 36, 36)),
    ('convt4_split', ConvSpec('convt', 8, 8, (5, 3, 3), 2), (3, 16, 16)),
    # 33 positions per row (the first and the last layer of the 41x49x35 network): the weight-gradient rows as three compile-time blocks
    ('conv1_w33', ConvSpec('conv', 1, 8, (3, 3, 3), 1), (4, 5, 35)),
    ('convt5_w33', ConvSpec('convt', 8, 1, (3, 3, 3), 1), (3, 4, 33)),
    # 30 / 32 positions per row (the large layers of the 82x98x70 network): two compile-time blocks of 4 k-steps
    ('convt3_w30', ConvSpec('convt', 16, 8, (3, 3, 3), 1), (3, 4, 30)),
    ('convt4hr_w32', ConvSpec('convt', 8, 8, (4, 4, 4), 2), (3, 3, 32)),
]


def ref_layer(p, w, b, gamma, beta, spec, relu_in, per_group):
    h = F.relu(p) if relu_in else p
    if gamma is not None:
        N, C = h.shape[:2]
        G = N // per_group
        hg = h.reshape(G, per_group, C, -1)
        mean = hg.mean((1, 3), keepdim=True)
        var = hg.var((1, 3), unbiased=False, keepdim=True)
        hg = (hg - mean) / torch.sqrt(var + 1e-5) * gamma.view(1, 1, -1, 1) + beta.view(1, 1, -1, 1)
        h = hg.reshape(h.shape)
    if spec.kind == 'conv':
        return F.conv3d(h, w, b, spec.stride)
    return F.conv_transpose3d(h, w, b, spec.stride, spec.pad, spec.outpad)


def _bind_random_grads(params, g):
    """nn.Parameters whose .grad is prefilled with random values r (what the optimiser's flat gradient buffer holds mid-accumulation):
    -> [r] (CPU copies)"""
    rs = []
    for t in params:
        r = 2 * torch.randn(t.shape, generator=g)
        t.grad = r.clone().to(t.device)
        rs.append(r)
    return rs


def run_layer_case(dev, name, spec, isz, with_bn, relu_in, groups, input_is_data=False, seed=0, tol=2e-4, bound_grads=False):
    """bound_grads: weight, bias, gamma and beta are nn.Parameters with a bound, randomly prefilled .grad: the backward must add its
    gradients straight into those buffers (the accumulate forms of vg_wgrad3d, vg_channel_sum, vg_bn_param_grad, vg_bn_tconv1_sums,
    vg_data_bn_grads; on the GPU the side-stream branch), hand autograd None for them, and .grad - r must be the reference gradient."""
    g = torch.Generator().manual_seed(seed)
    per_group = 2
    N = per_group * groups
    wshape = ((spec.co, spec.ci) if spec.kind == 'conv' else (spec.ci, spec.co)) + tuple(spec.k)
    p = torch.randn((N, spec.ci) + tuple(isz), generator=g)
    w = torch.randn(wshape, generator=g) * 0.2
    b = torch.randn(spec.co, generator=g) * 0.1
    gamma = (1 + 0.3 * torch.randn(spec.ci, generator=g)) if with_bn else None
    beta = (0.2 * torch.randn(spec.ci, generator=g)) if with_bn else None
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (p, w, b, gamma, beta)]
    y_ref = ref_layer(*leaves, spec, relu_in, per_group)
    gy = torch.randn(y_ref.shape, generator=g)
    ref_grads = torch.autograd.grad(y_ref, [t for t in leaves if t is not None], gy)
    ref_grads = list(ref_grads)
    if gamma is None:
        ref_grads += [None, None]

    dleaves = [t.to(dev).clone().requires_grad_(True) if t is not None else None for t in (p, w, b, gamma, beta)]
    prefill = [None] * 5
    if bound_grads:
        for i in range(1, 5):
            if dleaves[i] is not None:
                dleaves[i] = torch.nn.Parameter(dleaves[i].detach())
        rs = iter(_bind_random_grads([t for t in dleaves[1:] if t is not None], g))
        prefill = [None] + [None if t is None else next(rs) for t in dleaves[1:]]
    if input_is_data:
        dleaves[0] = dleaves[0].detach()
    y = ops.bn_conv_act(dleaves[0], dleaves[1], dleaves[2], dleaves[3], dleaves[4], spec, relu_in, per_group, input_is_data)
    assert y.shape == y_ref.shape, (y.shape, y_ref.shape)
    np.testing.assert_allclose(y.detach().cpu().numpy(), y_ref.detach().numpy(), rtol=tol, atol=tol, err_msg=name + ' fwd')
    ins = [t for t in dleaves if t is not None and t.requires_grad]
    grads = list(torch.autograd.grad(y, ins, gy.to(dev), allow_unused=bound_grads))
    if bound_grads and y.is_cuda:
        ops.join_side_stream(y.device)
    names = ['p', 'w', 'b', 'gamma', 'beta']
    k = 0
    for i, t in enumerate(dleaves):
        if t is None or not t.requires_grad:
            continue
        got = grads[k]; k += 1
        if bound_grads and i > 0:
            assert got is None, '%s d%s: autograd was handed a tensor although .grad is bound' % (name, names[i])
            got = t.grad.cpu() - prefill[i]
        got = got.cpu().numpy()
        want = ref_grads[i].numpy()
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=5 * tol, atol=5 * tol * scale, err_msg='%s d%s' % (name, names[i]))


def run_chain_case(dev, isz=(3, 4, 5), groups=2, per_group=3, seed=0, tol=2e-4):
    """convt4 -> batch norm -> convt5 as the decoder chains them: convt4 also accumulates the batch norm's statistics (next_bn) and
    leaves its bias gradient to the consumer (bias_grad_by_consumer=True), convt5 gets producer_bias=convt4's bias, whose gradient
    then comes out of vg_bn_bwd_apply_tconv1.  Every parameter has a bound, randomly prefilled .grad; against float64 autograd of
    the same chain: each gradient must have been added exactly once (the producer's bias gradient too), at the tolerances of
    run_layer_case."""
    g = torch.Generator().manual_seed(seed)
    s4 = ConvSpec('convt', 8, 8, (5, 3, 3), 2, name='convt4'); s5 = ConvSpec('convt', 8, 1, _K3, 1, name='convt5')
    N = groups * per_group
    x = torch.randn((N, 8) + tuple(isz), generator=g)
    vals = [0.2 * torch.randn(8, 8, 5, 3, 3, generator=g), 0.1 * torch.randn(8, generator=g), 0.2 * torch.randn(8, 1, 3, 3, 3, generator=g),
            0.1 * torch.randn(1, generator=g), 1 + 0.3 * torch.randn(8, generator=g), 0.2 * torch.randn(8, generator=g)]
    names = ['w4', 'b4', 'w5', 'b5', 'gamma', 'beta']
    rl = [x.double().requires_grad_(True)] + [v.double().requires_grad_(True) for v in vals]
    p1 = ref_layer(rl[0], rl[1], rl[2], None, None, s4, True, per_group)
    y_ref = ref_layer(p1, rl[3], rl[4], rl[5], rl[6], s5, True, per_group)
    gy = torch.randn(y_ref.shape, generator=g)
    ref_grads = torch.autograd.grad(y_ref, rl, gy.double())
    xd = x.to(dev).requires_grad_(True)
    w4, b4, w5, b5, gamma, beta = params = [torch.nn.Parameter(v.to(dev)) for v in vals]
    rs = _bind_random_grads(params, g)
    p1d, st = ops.bn_conv_act(xd, w4, b4, None, None, s4, True, per_group, next_bn=per_group, bias_grad_by_consumer=True)
    y = ops.bn_conv_act(p1d, w5, b5, gamma, beta, s5, True, per_group, pre_stats=st, producer_bias=b4)
    np.testing.assert_allclose(y.detach().cpu().numpy(), y_ref.detach().numpy(), rtol=tol, atol=tol, err_msg='chain fwd')
    got = torch.autograd.grad(y, [xd] + params, gy.to(dev), allow_unused=True)
    if xd.is_cuda:
        ops.join_side_stream(xd.device)
    for t, r, gr, want, nm in zip(params, rs, got[1:], ref_grads[1:], names):
        assert gr is None, 'chain d%s: autograd was handed a tensor although .grad is bound' % nm
        want = want.numpy()
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose((t.grad.cpu() - r).numpy(), want, rtol=5 * tol, atol=5 * tol * scale, err_msg='chain d' + nm)
    want = ref_grads[0].numpy()
    np.testing.assert_allclose(got[0].cpu().numpy(), want, rtol=5 * tol, atol=5 * tol * max(1.0, float(np.abs(want).max())), err_msg='chain dx')


def ref_gam(logits, gain, x, eps, glm):
    G, B, V = logits.shape
    s = torch.sigmoid(logits)
    xrec = s[0]
    dist = []
    for i in range(1, G):
        cons = gain[i - 1][:, None] * s[i]
        dist.append(torch.linalg.vector_norm(cons - glm[i - 1][None], dim=1))
        xrec = xrec + cons
    scale = torch.exp(-eps).float()[None]
    lp = -((x - xrec) ** 2) / (2 * scale ** 2) - scale.log() - np.log(np.sqrt(2 * np.pi))
    return lp.sum(1), (torch.stack(dist) if dist else torch.zeros(0, B))


def run_gam_case(dev, C, B, V, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(C + 1, B, V, generator=g)
    gain = torch.randn(C, B, generator=g)
    x = torch.rand(B, V, generator=g)
    eps = (-np.log(10) + 0.3 * torch.randn(V, generator=g, dtype=torch.float64))
    glm = torch.rand(C, V, generator=g)
    lv = [logits.clone().requires_grad_(True), gain.clone().requires_grad_(True), x, eps.clone().requires_grad_(True), glm]
    slp_r, dist_r = ref_gam(*lv)
    g1 = torch.randn(B, generator=g); g2 = torch.randn(C, B, generator=g)
    tgt = [lv[0], lv[3]] + ([lv[1]] if C > 0 else [])
    gr = torch.autograd.grad((slp_r * g1).sum() + (dist_r * g2).sum(), tgt)
    dv = [logits.to(dev).clone().requires_grad_(True), gain.to(dev).clone().requires_grad_(True), x.to(dev), eps.to(dev).clone().requires_grad_(True), glm.to(dev)]
    lbias = torch.nn.Parameter(torch.zeros(1, device=dev))          # stands for the bias of the layer that produced the logits
    lbias.grad = torch.zeros_like(lbias)                            # the caller binds the buffer the backward adds into (the optimiser does in the model)
    slp, dist = ops.GamElbo.apply(*dv, lbias)
    np.testing.assert_allclose(slp.detach().cpu().numpy(), slp_r.detach().numpy(), rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(dist.detach().cpu().numpy(), dist_r.detach().numpy(), rtol=2e-5, atol=1e-5)
    dtgt = [dv[0], dv[3]] + ([dv[1]] if C > 0 else [])
    gd = torch.autograd.grad((slp * g1.to(dev)).sum() + (dist * g2.to(dev)).sum(), dtgt)
    # explicit hand-off: the backward left sum(d_logits) in the producing layer's bias gradient
    np.testing.assert_allclose(float(lbias.grad), float(gr[0].double().sum()), rtol=2e-4, atol=2e-4 * float(gr[0].abs().sum()) / max(gr[0].numel() ** 0.5, 1))
    for a, b_, nm in zip(gd, gr, ('d_logits', 'd_eps', 'd_gain')):
        sc = max(1.0, float(b_.abs().max()))
        np.testing.assert_allclose(a.cpu().numpy(), b_.numpy(), rtol=2e-4, atol=2e-5 * sc, err_msg=nm)
    maps = ops.gam_maps(dv[0].detach(), dv[1].detach(), dv[2], dv[3].detach(), dv[4])
    s = torch.sigmoid(logits)
    np.testing.assert_allclose(maps[0].cpu().numpy(), s[0].numpy(), atol=1e-6)
    full = s[0] + sum(gain[i][:, None] * s[i + 1] for i in range(C))
    np.testing.assert_allclose(maps[C + 1].cpu().numpy(), full.numpy(), atol=1e-5)


def ref_latent(mu, w, a, eps_w, eps_d, G):
    """The reference's operator sequence (vae_reg_GP.py:321-329, 339-342, 400) through its own distribution classes."""
    B, L = mu.shape
    d = torch.exp(a)
    if (d < 1e-6).any():
        d = d + 1e-6
    q = torch.distributions.LowRankMultivariateNormal(mu, w.unsqueeze(-1), d)
    z = mu + w * eps_w.view(B, 1) + d.sqrt() * eps_d            # rsample with the given draws
    p = torch.distributions.MultivariateNormal(torch.zeros(L), torch.eye(L))
    kl = torch.distributions.kl_divergence(q, p)
    oh = torch.eye(G).unsqueeze(1).expand(G, B, G)
    zcat = torch.cat([z.unsqueeze(0).expand(G, B, L), oh], 2).reshape(G * B, L + G)
    return zcat, kl, d


def run_latent_case(dev, B, L, G, seed=0, tiny_d=False):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, L, generator=g); w = 0.5 * torch.randn(B, L, generator=g); a = 0.7 * torch.randn(B, L, generator=g) - 0.5
    if tiny_d:
        a[B // 2, L // 3] = -15.0                                 # exp(a) < 1e-6: the batch-wide floor kicks in
    eps_w = torch.randn(B, 1, generator=g); eps_d = torch.randn(B, L, generator=g)
    gz = torch.randn(G * B, L + G, generator=g); gk = torch.randn(B, generator=g)
    rv = [t.clone().requires_grad_(True) for t in (mu, w, a)]
    zc_r, kl_r, d_r = ref_latent(*rv, eps_w, eps_d, G)
    gr = torch.autograd.grad((zc_r * gz).sum() + (kl_r * gk).sum(), rv)
    dv = [t.to(dev).clone().requires_grad_(True) for t in (mu, w, a)]
    zc, kl, d = ops.LatentSample.apply(*dv, eps_w.to(dev), eps_d.to(dev), G)
    np.testing.assert_allclose(zc.detach().cpu().numpy(), zc_r.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(kl.detach().cpu().numpy(), kl_r.detach().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(d.cpu().numpy(), d_r.detach().numpy(), rtol=1e-6, atol=0)
    gd = torch.autograd.grad((zc * gz.to(dev)).sum() + (kl * gk.to(dev)).sum(), dv)
    for x_, y_, nm in zip(gd, gr, ('g_mu', 'g_w', 'g_a')):
        np.testing.assert_allclose(x_.cpu().numpy(), y_.numpy(), rtol=2e-4, atol=2e-5, err_msg=nm)


def run_loss_case(dev, B, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    kl = torch.rand(B, generator=g) * 30; slp = -1e4 * torch.rand(B, generator=g); dist = torch.rand(C, B, generator=g) * 50
    gp = torch.rand(1, generator=g) * 100
    coef = (1.0 / B, -1.0 / B, 0.37, 1e-3 * B)
    rv = [t.clone().requires_grad_(True) for t in (kl, slp, dist, gp)]
    loss_r = -((-rv[0] + rv[1]).sum(0) / B) + coef[2] * rv[3] + 1e-3 * (B * rv[2].sum())       # vae_reg_GP.py:388-389, 406-410
    gr = torch.autograd.grad(loss_r.sum(), rv)
    dv = [t.to(dev).clone().requires_grad_(True) for t in (kl, slp, dist, gp)]
    loss = ops.ElboLoss.apply(*dv, coef)
    assert loss.shape == (1,)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), loss_r.detach().numpy(), rtol=1e-5)
    gd = torch.autograd.grad(loss.sum(), dv)
    for x_, y_ in zip(gd, gr):
        np.testing.assert_allclose(x_.cpu().numpy(), y_.numpy(), rtol=1e-6, atol=0)


def run_linear_case(dev, B=24, fin=40, fout=17, seed=0):
    """LinearAct with direct accumulation into existing .grad buffers == nn.Linear + relu under autograd."""
    g = torch.Generator().manual_seed(seed)
    ref = torch.nn.Linear(fin, fout); lay = torch.nn.Linear(fin, fout).to(dev)
    with torch.no_grad():
        lay.weight.copy_(ref.weight); lay.bias.copy_(ref.bias)
    x = torch.randn(B, fin, generator=g); gy = torch.randn(B, fout, generator=g)
    for relu, relu_in in ((True, False), (False, False), (True, True)):
        xr = x.clone().requires_grad_(True)
        yr = ref(torch.relu(xr) if relu_in else xr); yr = torch.relu(yr) if relu else yr
        ref.zero_grad(); (yr * gy).sum().backward()
        for prefilled in (False, True):
            xd = x.to(dev).clone().requires_grad_(True)
            lay.weight.grad = torch.ones_like(lay.weight) if prefilled else None
            lay.bias.grad = torch.ones_like(lay.bias) if prefilled else None
            y = ops.linear_act(lay, xd, relu, relu_in=relu_in)
            (y * gy.to(dev)).sum().backward()
            off = 1.0 if prefilled else 0.0
            np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(xd.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(lay.weight.grad.cpu().numpy() - off, ref.weight.grad.numpy(), rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(lay.bias.grad.cpu().numpy() - off, ref.bias.grad.numpy(), rtol=1e-4, atol=1e-5)


def run_fc_gemm_case(dev, M, N, K, a_kc, b_kc, flags=(), batch=1, ksplit=None, seed=0):
    """vg_fc_gemm (the strided product behind every fully connected layer, vae_reg_GP.py:197-210) against a float64 einsum with the
    same operand options: each operand k-contiguous or m/n-contiguous, ReLU / mask on load, the ones column (bias gradient), bias, ReLU,
    output mask, accumulation, split-K, batch."""
    from vae_gam_amd import _lib
    g = torch.Generator().manual_seed(seed + 7 * M + N + K)
    fl = 0
    for f in flags:
        fl |= getattr(_lib, 'FC_' + f)
    A = torch.randn(batch, M, K, generator=g); Bm = torch.randn(batch, K, N, generator=g)
    amask = torch.randn(batch, M, K, generator=g); cmask = torch.randn(batch, M, N, generator=g)
    bias = torch.randn(batch, N, generator=g); C0 = torch.randn(batch, M, N, generator=g); cx0 = torch.randn(batch, M, generator=g)
    Ae = A.double()
    if 'A_RELU' in flags: Ae = Ae.clamp_min(0)
    if 'A_MASK' in flags: Ae = Ae * (amask > 0)
    Be = Bm.double().clamp_min(0) if 'B_RELU' in flags else Bm.double()
    want = torch.einsum('zmk,zkn->zmn', Ae, Be)
    wx = Ae.sum(2)
    if 'C_BIAS' in flags: want = want + bias.double()[:, None, :]
    if 'C_RELU' in flags: want = want.clamp_min(0)
    if 'C_MASK' in flags: want = want * (cmask > 0)
    if 'C_ACCUM' in flags: want = want + C0.double(); wx = wx + cx0.double()
    # device layouts: A as [z][m][k] (k contiguous) or [z][k][m]; B as [z][n][k] (k contiguous) or [z][k][n]
    Ad = (A if a_kc else A.transpose(1, 2)).contiguous().to(dev); Md = (amask if a_kc else amask.transpose(1, 2)).contiguous().to(dev)
    Bd = (Bm.transpose(1, 2) if b_kc else Bm).contiguous().to(dev)
    Cd = C0.clone().to(dev); cxd = cx0.clone().to(dev)
    a_str = (K, 1, M * K) if a_kc else (1, M, M * K)
    b_str = (1, K, N * K) if b_kc else (N, 1, N * K)
    ops.fc_gemm(Ad, Bd, Cd, M, N, K, a_str, b_str, (N, M * N), fl, batch=batch, bias=bias.to(dev), bias_sb=N, amask=Md, cmask=cmask.to(dev),
                cx=cxd, cx_sb=M, ksplit=ksplit)
    scale = max(1.0, float(want.abs().max()))
    np.testing.assert_allclose(Cd.cpu().double().numpy(), want.numpy(), rtol=0, atol=2e-6 * scale * max(1.0, K ** 0.5))
    if 'B_ONES' in flags:
        np.testing.assert_allclose(cxd.cpu().double().numpy(), wx.numpy(), rtol=0, atol=2e-6 * max(1.0, float(wx.abs().max())) * max(1.0, K ** 0.5))
    else:
        assert torch.equal(cxd.cpu(), cx0), 'cx touched without VG_FC_B_ONES'


FC_GEMM_CASES = [
    # M, N, K, a_kc, b_kc, flags, batch, ksplit
    (24, 17, 40, True, True, ('C_BIAS', 'C_RELU'), 1, None),                    # a layer's forward, ragged everywhere
    (64, 200, 256, True, True, ('A_RELU', 'C_BIAS', 'C_RELU'), 1, 4),           # fc1-like: pre-activation input, split-K
    (70, 33, 100, True, False, ('A_MASK', 'C_MASK'), 1, None),                  # data gradient through two ReLUs
    (130, 41, 300, True, False, ('A_MASK',), 1, 3),                             # ... with split-K (fc8's data gradient)
    (50, 37, 64, False, False, ('A_MASK', 'B_ONES', 'B_RELU', 'C_ACCUM'), 1, None),   # weight + bias gradient, accumulated
    (150, 101, 80, False, False, ('B_ONES',), 1, 2),                            # ... written, split-K, several tiles
    (64, 32, 50, True, True, ('C_BIAS',), 3, None),                             # the three heads, batched
    (32, 50, 64, False, False, ('B_ONES', 'C_ACCUM'), 3, None),                 # their weight gradients
    (5, 3, 2, False, True, (), 1, None),                                        # smaller than a tile in every direction
    (64, 40, 96, False, False, ('A_MASK', 'B_ONES', 'C_ACCUM'), 1, None),       # both operands contiguous along m / n, multiples of 4: 16-byte loads across rows
    (36, 44, 70, False, False, ('A_RELU', 'B_ONES', 'B_RELU'), 1, None),        # ... ragged tile edges and a partial last step
    (72, 36, 200, True, False, ('A_MASK', 'C_MASK'), 1, 2),                     # data gradient with the weights read across rows, split-K
    (870, 900, 20, True, False, ('A_MASK', 'C_BIAS'), 1, None),                 # >= 768 tiles of 32 x 32: the 64 x 64 kernel, ragged edges
]


def run_fused_stats_case(dev, spec, isz, groups=2, per_group=3, seed=0):
    """Transposed-conv forward that also leaves the next BatchNorm's statistics == a separate bn_stats pass over its output;
    bn_backward_'s fused per-channel sum == channel_sum of its result."""
    g = torch.Generator().manual_seed(seed)
    N = groups * per_group
    x = torch.randn(N, spec.ci, *isz, generator=g).to(dev)
    w = (0.2 * torch.randn(spec.ci, spec.co, *spec.k, generator=g)).to(dev)
    b = torch.randn(spec.co, generator=g).to(dev)
    gamma = (1 + 0.1 * torch.randn(spec.co, generator=g)).to(dev); beta = (0.1 * torch.randn(spec.co, generator=g)).to(dev)
    wf = ops.pack_weight(w, spec, 'fwd')
    y, part = ops.conv_forward(x, wf, b, spec, True, None, None, per_group, next_bn=per_group)   # explicit hand-off
    fused = [t.clone() for t in ops.bn_stats(y, gamma, beta, True, per_group, pre=part)]
    plain = ops.bn_stats(y, gamma, beta, True, per_group)
    for a_, b_, nm in zip(fused, plain, ('scale', 'shift', 'mean', 'rstd')):
        np.testing.assert_allclose(a_.cpu().numpy(), b_.cpu().numpy(), rtol=2e-5, atol=2e-6, err_msg=nm)
    # fused bias-gradient sum of the batch-norm backward
    dxe = torch.randn(y.shape, generator=g).to(dev)
    pbg = torch.full((spec.co,), 0.5, device=dev)             # the producing layer's bias.grad: the sum is ADDED to it
    ops.bn_backward_(dxe, y, gamma, plain[2], plain[3], True, per_group, producer_bias_grad=pbg)
    want = dxe.sum((0, 2, 3, 4)) + 0.5
    np.testing.assert_allclose(pbg.cpu().numpy(), want.cpu().numpy(), rtol=2e-4, atol=2e-4 * float(want.abs().max()))


def run_conv_mm_plan_case(dev, kind, force, seed=0):
    """vg_conv_mm with a PINNED tile -- waves per workgroup, PD planes x PHB rows per block, channels per chunk, single / double
    buffered input -- against torch's own convolution: the row-slab staging (one span per plane, padded LDS pitch), the 4-wave
    workgroups, the counted-vmcnt single-buffer order, the ReLU mask fetched ahead of the last matrix phase and the per-group-run
    statistics flush must all give what the whole-plane 8-wave plan gives.
    kind: 'convt3_fwd' (16->8, 3x3x3 stride-1 transposed conv as a padded correlation, prologue = ReLU + batch-norm affine),
          'convt3_bwd' (its data gradient: 8->16 correlation, ReLU mask of the producer fused into the epilogue),
          'convt4_fwd' (8->8, 5x3x3 stride-2 transposed conv: 4 output-parity classes, statistics of the next batch norm)."""
    g = torch.Generator().manual_seed(seed)
    per_group, groups = 3, 2
    N = per_group * groups
    if kind == 'convt4_fwd':
        spec = ops.ConvSpec('convt', 8, 8, (5, 3, 3), 2); isz = (5, 9, 6)
    else:
        spec = ops.ConvSpec('convt', 16, 8, (3, 3, 3), 1); isz = (5, 9, 6)
    osz = spec.out_size(isz)
    x = torch.randn((N, spec.ci) + isz, generator=g)
    w = 0.2 * torch.randn((spec.ci, spec.co) + tuple(spec.k), generator=g)
    b = 0.1 * torch.randn(spec.co, generator=g)
    sc = 1 + 0.3 * torch.randn(groups * spec.ci, generator=g); sh = 0.2 * torch.randn(groups * spec.ci, generator=g)
    if kind.endswith('_fwd'):
        h = torch.relu(x) * sc.view(groups, 1, spec.ci, 1, 1, 1).expand(groups, per_group, spec.ci, 1, 1, 1).reshape(N, spec.ci, 1, 1, 1) \
            + sh.view(groups, 1, spec.ci, 1, 1, 1).expand(groups, per_group, spec.ci, 1, 1, 1).reshape(N, spec.ci, 1, 1, 1)
        want = F.conv_transpose3d(h, w, b, spec.stride)
        plan = ops.mm_plan(spec, 'fwd', isz, None, force=force)
        assert plan is not None, force
        nb = per_group if kind == 'convt4_fwd' else None
        got = ops.conv_mm(x.to(dev), plan, plan.gather(w.to(dev)), b.to(dev), True, sc.to(dev), sh.to(dev), per_group, None, nb)
        if nb:
            got, part = got
            gamma = torch.ones(spec.co, device=dev); beta = torch.zeros(spec.co, device=dev)
            fused = ops.bn_stats(got, gamma, beta, True, per_group, pre=part)
            plain = ops.bn_stats(got, gamma, beta, True, per_group)
            for a_, b_, nm in zip(fused, plain, ('scale', 'shift', 'mean', 'rstd')):
                np.testing.assert_allclose(a_.cpu().numpy(), b_.cpu().numpy(), rtol=2e-5, atol=2e-6, err_msg='%s %r' % (nm, force))
    else:
        dy = torch.randn((N, spec.co) + osz, generator=g)
        xm = torch.randn((N, spec.ci) + isz, generator=g)              # the producer's pre-activation: ReLU mask of the data gradient
        want = F.conv3d(dy, w) * (xm > 0)                              # d/dx of conv_transpose3d(x, w) = correlation of dy with w
        plan = ops.mm_plan(spec, 'bwd', osz, isz, force=force)
        assert plan is not None, force
        got = ops.conv_mm(dy.to(dev), plan, plan.gather(w.to(dev)), None, False, None, None, 1, xm.to(dev))
    assert (plan.waves, plan.PD, plan.PHB, plan.cc, plan.dbuf) == tuple(force)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-4, atol=2e-4, err_msg='%s %r' % (kind, force))


_K3 = (3, 3, 3)
# the layers whose launches vg_conv_mm carries in the three schema.net_geometry networks (41x49x35, 82x98x70, 21x21x21)
MM_SPECS = {
    'conv2': ConvSpec('conv', 8, 8, _K3, 2),
    'conv3': ConvSpec('conv', 8, 16, _K3, 1),
    'conv4': ConvSpec('conv', 16, 16, _K3, 2),
    'conv5': ConvSpec('conv', 16, 16, _K3, 1),
    'convt1': ConvSpec('convt', 16, 16, _K3, 1),
    'convt2p': ConvSpec('convt', 16, 16, _K3, 2, (1, 0, 1), (1, 0, 1)),      # the padded convt2 of the 41x49x35 network
    'convt2': ConvSpec('convt', 16, 16, _K3, 2),                             # the plain one of the 82x98x70 network
    'convt3': ConvSpec('convt', 16, 8, _K3, 1),
    'convt4': ConvSpec('convt', 8, 8, (5, 3, 3), 2),
    'convt4hr': ConvSpec('convt', 8, 8, (4, 4, 4), 2),                       # 82x98x70
    'convt4toy': ConvSpec('convt', 8, 8, _K3, 2),                            # 21x21x21
}


def mm_instance(plan, masked):
    """(W, NQ, TPC, ks, DB, MASKED) of the conv_mm_k instance vg_conv_mm launches for this plan -- a restatement of its dispatch, for
    the record a case prints (ks 0 = the generic instance that reads the step counts from the descriptor)."""
    ks = list(plan.ks)
    if plan.nq == 1:
        static = ks[0] in (7, 9, 12) or (ks[0] == 19 and plan.tpc <= 3)
    else:
        static = ks in ([3, 2, 2, 1], [2, 1, 1, 1], [2, 2, 2, 2])
    return (plan.waves, plan.nq, plan.tpc, tuple(ks) if static else 0, plan.dbuf, int(bool(masked)))


def run_conv_mm_case(dev, spec, direction, isz, force, groups=2, per_group=3, stats=False, seed=0, tpc=None, loop=False):
    """One vg_conv_mm launch with a PINNED tile (waves, PD planes, PHB rows, channels per chunk, double buffering) against float64
    F.conv3d / F.conv_transpose3d on the CPU.  `isz` is the LAYER's input size: 'fwd' reads it (prologue = ReLU + per-(group, channel)
    affine, bias added; with `stats` also the partial sums of the next batch norm), 'bwd' reads dy of the layer's output size and
    writes the data gradient, masked by the producer's pre-activation.  `loop`: the case is sized so that a block of the persistent
    grid must visit several samples (N * blocks per sample > 2048 = 256 CUs x at most 8 resident blocks).

    Tolerance: tol = max(4 * d32, eps32 * sqrt(K) * max|want|) with d32 = the distance of torch's own fp32 CPU convolution to the
    float64 result on the same inputs and K = CI * taps the contraction length (the random-walk rounding floor of an fp32 sum of K
    terms: guards against a lucky tiny d32).  The fp32 matrix cores are exact fp32 FMAs in another summation order, so the kernel's
    error is of d32's size: 0.6x to 2.4x over the listed cases on the host build; a path that lost precision would sit at 100x or more.

    Statistics: mean and rstd of relu(y) per (group, channel) from the kernel's partials against float64 statistics of the float64
    reference.  Bound: every element of y is within tol and relu is 1-Lipschitz; the partial sums are fp32 chains of non-negative
    terms, at most m = tpc * nq * per_group elements per lane and run plus 6 shuffle stages, so they are relatively exact to
    m * eps32 (sums) / (m + 1) * eps32 (squares, one fma rounding more): |d mean| <= tol + m eps32 mean,
    |d E[h^2]| <= 2 max|h| tol + (m + 1) eps32 E[h^2], |d var| <= |d E[h^2]| + 2 mean |d mean| + |d mean|^2, and rstd moves by what
    var +- d var moves it; both are stored in fp32 (one more eps32).

    Returns the record of the case: plan, instance, err, d32, tol."""
    g = torch.Generator().manual_seed(seed)
    N = groups * per_group
    isz = tuple(isz)
    osz = spec.out_size(isz)
    conv = spec.kind == 'conv'
    wshape = ((spec.co, spec.ci) if conv else (spec.ci, spec.co)) + tuple(spec.k)
    w = 0.2 * torch.randn(wshape, generator=g)
    taps = spec.k[0] * spec.k[1] * spec.k[2]
    eps32 = float(np.finfo(np.float32).eps)

    def layer(h, wt, bias):
        if conv:
            return F.conv3d(h, wt, bias, spec.stride)
        return F.conv_transpose3d(h, wt, bias, spec.stride, spec.pad, spec.outpad)

    if direction == 'fwd':
        plan = ops.mm_plan(spec, 'fwd', isz, None, force=force)
    else:
        plan = ops.mm_plan(spec, 'bwd', osz, isz, force=force)
    assert plan is not None, (spec, direction, isz, force)
    assert (plan.waves, plan.PD, plan.PHB, plan.cc, plan.dbuf) == tuple(force)
    if tpc is not None:
        assert plan.tpc == tpc, (plan.tpc, tpc)
    nslab = (plan.PH + plan.PHB - 1) // plan.PHB
    bps = ((plan.PDT + plan.PD - 1) // plan.PD) * nslab
    if loop:
        assert N * bps > 2048, (N, bps)

    if direction == 'fwd':
        x = torch.randn((N, spec.ci) + isz, generator=g)
        b = 0.1 * torch.randn(spec.co, generator=g)
        sc = 1 + 0.3 * torch.randn(groups * spec.ci, generator=g); sh = 0.2 * torch.randn(groups * spec.ci, generator=g)

        def pro(t, dt):
            a = sc.to(dt).view(groups, 1, spec.ci, 1, 1, 1).expand(groups, per_group, spec.ci, 1, 1, 1).reshape(N, spec.ci, 1, 1, 1)
            c = sh.to(dt).view(groups, 1, spec.ci, 1, 1, 1).expand(groups, per_group, spec.ci, 1, 1, 1).reshape(N, spec.ci, 1, 1, 1)
            return torch.relu(t.to(dt)) * a + c
        want = layer(pro(x, torch.float64), w.double(), b.double())
        own32 = layer(pro(x, torch.float32), w, b)
        K = spec.ci * taps
        nb = per_group if stats else None
        got = ops.conv_mm(x.to(dev), plan, plan.gather(w.to(dev)), b.to(dev), True, sc.to(dev), sh.to(dev), per_group, None, nb)
        if stats:
            got, part = got
    else:
        assert not stats
        dy = torch.randn((N, spec.co) + osz, generator=g)
        xm = torch.randn((N, spec.ci) + isz, generator=g)              # the producer's pre-activation: ReLU mask of the data gradient

        def dgrad(dt):
            x0 = torch.zeros((N, spec.ci) + isz, dtype=dt, requires_grad=True)
            (gx,) = torch.autograd.grad(layer(x0, w.to(dt), None), x0, dy.to(dt))
            return gx * (xm > 0)
        want = dgrad(torch.float64)
        own32 = dgrad(torch.float32)
        K = spec.co * taps
        got = ops.conv_mm(dy.to(dev), plan, plan.gather(w.to(dev)), None, False, None, None, 1, xm.to(dev))
    assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    d32 = float((own32.double() - want).abs().max())
    wmax = float(want.abs().max())
    tol = max(4 * d32, eps32 * K ** 0.5 * wmax)
    err = float((got.cpu().double() - want).abs().max())
    rec = dict(spec=spec, direction=direction, isz=isz, force=tuple(force), N=N, bps=bps, nslab=nslab, mode=plan.mode, stride=spec.stride,
               cc=plan.cc, CI=plan.CI, instance=mm_instance(plan, direction == 'bwd'), err=err, d32=d32, tol=tol, stats=stats)
    print('conv_mm %s %s isz %r force %r N %d bps %d nslab %d instance (W, NQ, TPC, ks, DB, MASKED) %r: err %.3g d32 %.3g err/d32 %.2f tol %.3g'
          % (spec.kind + 'x'.join(map(str, spec.k)) + '_%d>%d_s%d' % (spec.ci, spec.co, spec.stride), direction, isz, tuple(force), N, bps,
             nslab, rec['instance'], err, d32, err / max(d32, 1e-30), tol))
    assert err <= tol, 'conv_mm %s %r %r: max error %.3g > tol %.3g (d32 %.3g)' % (direction, isz, tuple(force), err, tol, d32)
    if stats:
        gamma = torch.ones(spec.co, device=dev); beta = torch.zeros(spec.co, device=dev)
        _, _, mean, rstd = ops.bn_stats(got, gamma, beta, True, per_group, pre=part)
        h = torch.relu(want).reshape(groups, per_group, spec.co, -1)
        mean_w = h.mean((1, 3)).reshape(-1); e2_w = (h * h).mean((1, 3)).reshape(-1)
        var_w = e2_w - mean_w * mean_w
        rstd_w = (var_w + ops.BN_EPS).rsqrt()
        m = plan.tpc * plan.nq * per_group + 6
        hmax = float(h.max())
        dmean = tol + m * eps32 * mean_w
        de2 = 2 * hmax * tol + (m + 1) * eps32 * e2_w
        dvar = de2 + 2 * mean_w * dmean + dmean * dmean
        assert float((var_w + ops.BN_EPS - dvar).min()) > 0
        drstd = torch.maximum((var_w + ops.BN_EPS - dvar).rsqrt() - rstd_w, rstd_w - (var_w + ops.BN_EPS + dvar).rsqrt())
        em = (mean.cpu().double() - mean_w).abs(); er = (rstd.cpu().double() - rstd_w).abs()
        bm = dmean + eps32 * mean_w.abs(); br = drstd + eps32 * rstd_w
        print('  statistics: mean err / bound %.3g, rstd err / bound %.3g' % (float((em / bm).max()), float((er / br).max())))
        assert bool((em <= bm).all()), 'mean of relu(y): worst error / bound %.3g' % float((em / bm).max())
        assert bool((er <= br).all()), 'rstd of relu(y): worst error / bound %.3g' % float((er / br).max())
    return rec


# (id, spec, direction, layer input size, force = (waves, PD, PHB, cc, dbuf), tpc the plan selects, statistics)
# N = 6 (2 groups of 3); every size <= 11x13x9.  s = row slabs (nslab >= 2), w = whole planes.
CONV_MM_CASES = [
    # conv2 bwd: 4 parity classes ks [2,1,1,1], masked
    ('conv2_bwd-s', 'conv2', 'bwd', (11, 13, 9), (8, 2, 3, 8, 0), 4, False),
    ('conv2_bwd-s-w4-db', 'conv2', 'bwd', (11, 13, 9), (4, 1, 2, 8, 1), 4, False),
    ('conv2_bwd-w-db', 'conv2', 'bwd', (11, 13, 9), (8, 3, 7, 8, 1), 4, False),
    # conv2 fwd (VG_CONV_MM=2): stride-2 correlation, ks 12, one channel per chunk
    ('conv2_fwd-s-cc1', 'conv2', 'fwd', (11, 13, 9), (8, 2, 3, 1, 0), 3, False),
    ('conv2_fwd-w-cc1-db', 'conv2', 'fwd', (11, 13, 9), (4, 5, 6, 1, 1), 3, False),
    # conv3 fwd (ks 7) / bwd (ks 9): every tiles-per-wave instance
    ('conv3_fwd-s-cc4', 'conv3', 'fwd', (7, 11, 8), (8, 1, 3, 4, 0), 3, False),
    ('conv3_fwd-w-db-tpc4', 'conv3', 'fwd', (11, 13, 9), (8, 5, 11, 8, 1), 4, False),
    ('conv3_fwd-w-cc2-tpc5', 'conv3', 'fwd', (11, 13, 9), (8, 7, 11, 2, 0), 5, False),
    ('conv3_fwd-s-w4-db-tpc6', 'conv3', 'fwd', (11, 13, 9), (4, 8, 6, 4, 1), 6, False),
    ('conv3_fwd-w-w4-tpc8', 'conv3', 'fwd', (11, 13, 9), (4, 5, 11, 8, 0), 8, False),
    ('conv3_bwd-s-db', 'conv3', 'bwd', (7, 11, 8), (8, 2, 4, 4, 1), 3, False),
    ('conv3_bwd-w-w4-tpc4', 'conv3', 'bwd', (9, 11, 8), (4, 5, 11, 16, 0), 4, False),
    ('conv3_bwd-w-w4-db-tpc5', 'conv3', 'bwd', (9, 11, 8), (4, 6, 11, 8, 1), 5, False),
    ('conv3_bwd-w-w4-cc4-tpc6', 'conv3', 'bwd', (9, 11, 8), (4, 8, 11, 4, 0), 6, False),
    ('convt3_fwd-w-w4-db-tpc8', 'convt3', 'fwd', (7, 11, 7), (4, 6, 13, 8, 1), 8, False),
    # conv4 fwd: stride-2 correlation, ks 7
    ('conv4_fwd-s-cc2', 'conv4', 'fwd', (9, 13, 8), (8, 1, 3, 2, 0), 3, False),
    ('conv4_fwd-s-w4-db', 'conv4', 'fwd', (9, 13, 8), (4, 2, 2, 4, 1), 3, False),
    ('conv4_fwd-w', 'conv4', 'fwd', (9, 13, 8), (8, 2, 6, 16, 0), 3, False),
    # conv5 / convt1: the 16 -> 16 stride-1 layers
    ('conv5_fwd-s-db', 'conv5', 'fwd', (6, 8, 6), (8, 2, 3, 8, 1), 3, False),
    ('conv5_fwd-w-w4', 'conv5', 'fwd', (6, 8, 6), (4, 4, 6, 16, 0), 3, False),
    ('conv5_bwd-s-w4', 'conv5', 'bwd', (6, 8, 6), (4, 3, 4, 16, 0), 3, False),
    ('conv5_bwd-w-db', 'conv5', 'bwd', (6, 8, 6), (8, 3, 8, 8, 1), 3, False),
    ('convt1_fwd-s', 'convt1', 'fwd', (4, 6, 5), (8, 3, 4, 8, 0), 3, False),
    ('convt1_fwd-w-db', 'convt1', 'fwd', (4, 6, 5), (8, 3, 8, 16, 1), 3, False),
    ('convt1_bwd-s-db', 'convt1', 'bwd', (4, 6, 5), (8, 2, 2, 16, 1), 3, False),
    ('convt1_bwd-w-cc4', 'convt1', 'bwd', (4, 6, 5), (8, 4, 6, 4, 0), 3, False),
    # convt2 bwd: stride-2 correlation, padded (41x49x35) and plain (82x98x70)
    ('convt2p_bwd-s-cc2', 'convt2p', 'bwd', (5, 6, 4), (8, 1, 3, 2, 0), 3, False),
    ('convt2p_bwd-w-db', 'convt2p', 'bwd', (5, 6, 4), (8, 3, 6, 16, 1), 3, False),
    ('convt2_bwd-s-db', 'convt2', 'bwd', (5, 6, 4), (8, 2, 2, 8, 1), 3, False),
    ('convt2_bwd-w-w4', 'convt2', 'bwd', (5, 6, 4), (4, 2, 6, 4, 0), 3, False),
    # convt4 bwd (VG_CONV_MM=2): stride-2 correlation, ks 19, one channel per chunk
    ('convt4_bwd-s-cc1', 'convt4', 'bwd', (4, 5, 4), (8, 2, 2, 1, 0), 3, False),
    ('convt4_bwd-w-cc1-db', 'convt4', 'bwd', (4, 5, 4), (8, 4, 5, 1, 1), 3, False),
    # 4x4x4 convt4 bwd (VG_CONV_MM=2): ks 24, the generic instance
    ('convt4hr_bwd-s-cc1', 'convt4hr', 'bwd', (4, 5, 3), (8, 2, 3, 1, 0), 3, False),
    ('convt4hr_bwd-w-w4-cc1-db', 'convt4hr', 'bwd', (4, 5, 3), (4, 2, 5, 1, 1), 3, False),
    # stride-2 transposed convs forward, statistics of the next batch norm: 4x4x4 (ks [2,2,2,2]) and 3x3x3 (ks [2,1,1,1])
    ('convt4hr_fwd-s-stats', 'convt4hr', 'fwd', (4, 7, 5), (8, 2, 3, 8, 0), 4, True),
    ('convt4hr_fwd-s-w4-db-stats', 'convt4hr', 'fwd', (4, 7, 5), (4, 1, 4, 8, 1), 4, True),
    ('convt4hr_fwd-w-db-stats', 'convt4hr', 'fwd', (4, 7, 5), (8, 2, 8, 8, 1), 4, True),
    ('convt4toy_fwd-s-stats', 'convt4toy', 'fwd', (4, 7, 5), (8, 2, 4, 8, 0), 4, True),
    ('convt4toy_fwd-w-w4-db-stats', 'convt4toy', 'fwd', (4, 7, 5), (4, 2, 8, 8, 1), 4, True),
]

# The persistent sample loop: N * blocks per sample > 2048, so that some block visits several samples whatever the occupancy query
# returns (nsplit <= 256 * blocks_per_cu / bps, blocks_per_cu <= 8).  per_group 8 / 13 / 7 against strides nsplit = 12, 25, 51, 102:
# a block's visits cross groups; 2 groups of 103 samples: they also stay inside a group at every possible stride (< 103).
# (id, spec, direction, layer input size, force, tpc, statistics, groups, per_group)
CONV_MM_LOOP_CASES = [
    ('convt4_fwd-stats-13x8', 'convt4', 'fwd', (3, 7, 4), (4, 1, 2, 8, 0), 4, True, 13, 8),
    ('convt4_fwd-db-stats-8x13', 'convt4', 'fwd', (3, 7, 4), (4, 1, 2, 8, 1), 4, True, 8, 13),
    ('convt4_fwd-stats-2x103', 'convt4', 'fwd', (3, 7, 1), (4, 1, 2, 8, 0), 4, True, 2, 103),
    ('convt3_fwd-cc8-11x7', 'convt3', 'fwd', (5, 6, 2), (4, 1, 2, 8, 0), 3, False, 11, 7),
    ('convt3_bwd-db-masked-11x7', 'convt3', 'bwd', (7, 8, 4), (4, 1, 2, 4, 1), 3, False, 11, 7),
]

# On the host build a looping case costs what its N * bps * chunks units cost, whatever its shape: these two measured 24 s each
# (the others 8 to 11 s), above the 20 s a host case may take, so they run on the GPU only (milliseconds there).
CONV_MM_LOOP_GPU_ONLY = ('convt4_fwd-stats-2x103', 'convt3_fwd-cc8-11x7')


def run_conv_mm_listed(dev, case, seed=0):
    cid, sname, direction, isz, force, tpc, stats = case[:7]
    groups, per_group = case[7:9] if len(case) > 7 else (2, 3)
    return run_conv_mm_case(dev, MM_SPECS[sname], direction, isz, force, groups, per_group, stats, seed, tpc=tpc, loop=len(case) > 7)


def conv_mm_coverage(dev=None):
    """What the union of CONV_MM_CASES and CONV_MM_LOOP_CASES pins, from the plans alone (no launch): the sets the issue asks for."""
    cov = dict(kinds=set(), slab_modes=set(), cc_lt_ci=0, dbuf=set(), waves=set(), masked=set(), tpc=set(), loops=0, loops_stats=0)
    for case in CONV_MM_CASES + CONV_MM_LOOP_CASES:
        cid, sname, direction, isz, force, tpc, stats = case[:7]
        spec = MM_SPECS[sname]
        plan = ops.mm_plan(spec, 'fwd', isz, None, force=force) if direction == 'fwd' else ops.mm_plan(spec, 'bwd', spec.out_size(isz), isz, force=force)
        assert plan is not None, cid
        nslab = (plan.PH + plan.PHB - 1) // plan.PHB
        bps = ((plan.PDT + plan.PD - 1) // plan.PD) * nslab
        cov['kinds'].add((sname, direction, 'slab' if nslab > 1 else 'whole'))
        if nslab > 1:
            cov['slab_modes'].add('class4' if plan.nq == 4 else 'corr_s%d' % plan.sdi)
        cov['cc_lt_ci'] += plan.cc < plan.CI
        cov['dbuf'].add(plan.dbuf); cov['waves'].add(plan.waves); cov['masked'].add(direction == 'bwd')
        if plan.nq == 1 and plan.ks[0] in (7, 9):
            cov['tpc'].add((plan.ks[0], plan.tpc))
        if len(case) > 7:
            N = case[7] * case[8]
            assert N * bps > 2048, cid
            cov['loops'] += 1; cov['loops_stats'] += bool(stats)
    return cov


# --------------------------------------------------------------------------- weight gradient (vg_wgrad3d), directly
WG_SPECS = {
    'conv1': ConvSpec('conv', 1, 8, _K3, 1),
    'conv2': ConvSpec('conv', 8, 8, _K3, 2),
    'conv3': ConvSpec('conv', 8, 16, _K3, 1),
    'conv4': ConvSpec('conv', 16, 16, _K3, 2),
    'conv5': ConvSpec('conv', 16, 16, _K3, 1),
    'convt1': ConvSpec('convt', 16, 16, _K3, 1),
    'convt2p': ConvSpec('convt', 16, 16, _K3, 2, (1, 0, 1), (1, 0, 1)),      # the padded convt2 of the 41x49x35 network
    'convt2': ConvSpec('convt', 16, 16, _K3, 2),                             # the plain one of the other two
    'convt3': ConvSpec('convt', 16, 8, _K3, 1),
    'convt4': ConvSpec('convt', 8, 8, (5, 3, 3), 2),
    'convt4hr': ConvSpec('convt', 8, 8, (4, 4, 4), 2),                       # 82x98x70
    'convt4toy': ConvSpec('convt', 8, 8, _K3, 2),                            # 21x21x21
    'convt5': ConvSpec('convt', 8, 1, _K3, 1),
    # no layer of the networks: the PA = 1 instances of the two plane-shift (DSH) families, which the library builds and the planner selects
    'conv5x3x3': ConvSpec('conv', 8, 8, (5, 3, 3), 2),
    'conv4x4x4': ConvSpec('conv', 8, 8, (4, 4, 4), 2),
}
EPS32 = float(np.finfo(np.float32).eps)


def wgrad_tuple(plan):
    """What names a launch of wgrad_rows_k for the coverage test: (family, PA, UG, RES, GRP, ONE, nbuf class, wave_slabs, loops)."""
    family = (plan.CA, plan.KD, plan.KH, plan.KW, plan.stride, plan.PAD, plan.DSH)
    nbuf = 'CA' if plan.nbuf == plan.CA else plan.nbuf
    return (family, plan.PA, plan.UG, plan.RES, plan.GRP, plan.ONE, nbuf, plan.wave_slabs, int(plan.items > plan.grid))


def _wgrad_shapes(spec, isz, N):
    isz = tuple(isz)
    return (N, spec.ci) + isz, (N, spec.co) + tuple(spec.out_size(isz))


def _check_plan(plan, expect, loop, what):
    for k, v in (expect or {}).items():
        have = ('CA' if plan.nbuf == plan.CA else plan.nbuf) if k == 'nbuf' else getattr(plan, k)
        assert have == v, '%s: plan.%s = %r, the case is there for %r (%r)' % (what, k, have, v, plan)
    if loop:
        assert plan.items >= 4097 and plan.items >= 2 * plan.grid and plan.items % plan.grid != 0, (what, plan)


def _per_sample(v, groups, per_group, C, dt):
    """[groups * C] -> [N][C][1][1][1]"""
    return v.to(dt).view(groups, 1, C, 1, 1, 1).expand(groups, per_group, C, 1, 1, 1).reshape(groups * per_group, C, 1, 1, 1)


def run_wgrad_case(dev, spec, isz, groups, per_group, prologue, accumulate, expect, seed=0, loop=False, what=''):
    """One vg_wgrad3d launch (ops.conv_weight_grad) against the float64 autograd weight gradient of F.conv3d / F.conv_transpose3d
    applied to the prologue'd input, on the CPU.  `isz` is the LAYER's input size, N = groups * per_group samples.
    prologue: 'none', 'relu', or 'affine' (ReLU, then a per-(group, channel) scale and shift), applied to x as the forward does --
    for a conv layer x is the window tensor (PA = 1), for a transposed one the position tensor (PA = 0).
    accumulate: the output buffer is prefilled with random values r and must hold r + dw afterwards.
    expect: plan fields the case is there to hit, asserted from ops.wgrad_plan before anything is launched.
    loop: the case is a persistent-loop case: items >= 4097 > 2 * 2048 >= 2 * grid whatever the occupancy query answers, so every
    block makes at least two trips, and items is no multiple of the grid.

    Tolerance: tol = max(4 * d32, eps32 * sqrt(K) * max|want|) [+ eps32 * max|r| with accumulate: the one rounding of the final add],
    d32 = the distance of torch's own fp32 CPU weight gradient to the float64 one on the same inputs, K = N * PD * PH * PW the
    contraction length (the random-walk rounding floor of an fp32 sum of K terms).  The kernel multiplies in exact fp32 on the matrix
    cores and sums 4 positions per instruction, per wave, per block and then over the slabs: a pairwise-like order, where torch's
    CPU kernel is closer to one long chain per sample.
    Measured err / d32 over WGRAD_CASES, WGRAD_MID_CASES and WGRAD_LOOP_CASES: 0.03 to 1.39 on the host build, 0.06 to 1.40 on the
    MI355X (the grouped cases 0.05 to 0.45); a launch that lost one item of 4,097 or one wave's share sits at 1e3 to 1e6.

    Returns the record of the case: plan, err, d32, tol."""
    g = torch.Generator().manual_seed(seed)
    N = groups * per_group
    conv = spec.kind == 'conv'
    xs, ys = _wgrad_shapes(spec, isz, N)
    relu_in = prologue != 'none'
    plan = ops.wgrad_plan(spec, xs, ys, relu_in, per_group)
    _check_plan(plan, expect, loop, what)
    x = torch.randn(xs, generator=g)
    dy = torch.randn(ys, generator=g)
    sc = sh = None
    if prologue == 'affine':
        sc = 1 + 0.3 * torch.randn(groups * spec.ci, generator=g); sh = 0.2 * torch.randn(groups * spec.ci, generator=g)
    wshape = ((spec.co, spec.ci) if conv else (spec.ci, spec.co)) + tuple(spec.k)
    r = torch.randn(wshape, generator=g) * 3

    def wgrad(dt):
        h = x.to(dt)
        if relu_in:
            h = torch.relu(h)
        if sc is not None:
            h = h * _per_sample(sc, groups, per_group, spec.ci, dt) + _per_sample(sh, groups, per_group, spec.ci, dt)
        w0 = torch.zeros(wshape, dtype=dt, requires_grad=True)
        y = F.conv3d(h, w0, None, spec.stride) if conv else F.conv_transpose3d(h, w0, None, spec.stride, spec.pad, spec.outpad)
        return torch.autograd.grad(y, w0, dy.to(dt))[0]
    want = wgrad(torch.float64)
    d32 = float((wgrad(torch.float32).double() - want).abs().max())
    P = ys[2:] if conv else xs[2:]
    K = N * P[0] * P[1] * P[2]
    wmax = float(want.abs().max())
    tol = max(4 * d32, EPS32 * K ** 0.5 * wmax)
    scd = sc.to(dev) if sc is not None else None; shd = sh.to(dev) if sh is not None else None
    xd, dyd = x.to(dev), dy.to(dev)
    rec = dict(plan=plan, d32=d32)
    for acc in (accumulate if isinstance(accumulate, (tuple, list)) else (accumulate,)):
        tol_a = tol
        if acc:
            out = r.clone().to(dev)
            assert ops.conv_weight_grad(xd, dyd, spec, relu_in, scd, shd, per_group, out=out) is None
            want_out = r.double() + want
            tol_a += EPS32 * float(r.abs().max())
        else:
            out = ops.conv_weight_grad(xd, dyd, spec, relu_in, scd, shd, per_group)
            want_out = want
        assert tuple(out.shape) == wshape
        err = float((out.cpu().double() - want_out).abs().max())
        print('wgrad %s%s isz %r N %d (%d x %d) %s acc %d plan %r: err %.3g d32 %.3g err/d32 %.2f tol %.3g'
              % (what + ' ' if what else '', spec.kind + 'x'.join(map(str, spec.k)) + '_%d>%d_s%d' % (spec.ci, spec.co, spec.stride), tuple(isz), N,
                 groups, per_group, prologue, int(bool(acc)), tuple(plan), err, d32, err / max(d32, 1e-30), tol_a))
        assert err <= tol_a, 'wgrad %s %r accumulate %d: max error %.3g > tol %.3g (d32 %.3g, plan %r)' % (what, tuple(isz), acc, err, tol_a, d32, plan)
        rec.update(err=max(err, rec.get('err', 0.0)), tol=tol_a)
    return rec


def run_wgrad_grouped_case(dev, C, isz, groups, per_group, relu, expect, sums_after=False, seed=0, loop=False, what=''):
    """vg_wgrad3d_grouped (ops.wgrad_grouped) for a C -> 1 channel 3x3x3 stride-1 transposed conv with input size `isz`, in_scale /
    in_shift = rstd / -mean * rstd of relu?(p) per (group, channel), against float64: rows c < C = per-group weight gradients against
    the normalised activation, row C = the per-tap sums of dy over the positions each tap meets.  Tolerance per group as in
    run_wgrad_case with K = per_group * D * H * W and d32 from torch's fp32 weight gradient of the same group (the row of sums has
    the same contraction length; its fp32 reference is F.conv_transpose3d's weight gradient against a tensor of ones).
    loop: grp_items >= 2 * ipb, every block of a group walks at least two of its items.
    sums_after: follow with vg_bn_tconv1_sums (ops.bn_tconv1_sums) and check `sums` (float64 from the fp32 q: bound = the
    propagated tolerance of q, sum_k |w| tol) and dw = gamma * sum_g q[g][c] + beta * sum_g q[g][C] with accumulate 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    N = groups * per_group
    spec = ConvSpec('convt', C, 1, _K3, 1)
    xs, ys = _wgrad_shapes(spec, isz, N)
    plan = ops.wgrad_plan(spec, xs, ys, relu, per_group, grouped=True)
    _check_plan(plan, expect, False, what)
    if loop:
        assert plan.grp_items >= 2 * plan.ipb and plan.grp_items % plan.ipb != 0, (what, plan)
    p = torch.randn(xs, generator=g) + 0.3
    dy = torch.randn(ys, generator=g)
    h = torch.relu(p.double()) if relu else p.double()
    hg = h.reshape(groups, per_group, C, -1)
    mean = hg.mean((1, 3)); rstd = (hg.var((1, 3), unbiased=False) + ops.BN_EPS).rsqrt()          # [G][C]
    scale = rstd.float().reshape(-1); shift = (-(mean * rstd)).float().reshape(-1)                # what the model passes (fp32)

    def ref(dt):
        hh = (torch.relu(p.to(dt)) if relu else p.to(dt)) * _per_sample(scale, groups, per_group, C, dt) + _per_sample(shift, groups, per_group, C, dt)
        hh = torch.cat([hh, torch.ones((N, 1) + tuple(isz), dtype=dt)], 1)                     # the constant-one position channel
        rows = []
        for gi in range(groups):
            w0 = torch.zeros((C + 1, 1, 3, 3, 3), dtype=dt, requires_grad=True)
            sl = slice(gi * per_group, (gi + 1) * per_group)
            rows.append(torch.autograd.grad(F.conv_transpose3d(hh[sl], w0), w0, dy[sl].to(dt))[0].reshape(C + 1, 27))
        return torch.stack(rows)
    want = ref(torch.float64)
    d32 = float((ref(torch.float32).double() - want).abs().max())
    K = per_group * isz[0] * isz[1] * isz[2]
    tol = max(4 * d32, EPS32 * K ** 0.5 * float(want.abs().max()))
    q = ops.wgrad_grouped(dy.to(dev), p.to(dev), scale.to(dev), shift.to(dev), relu, per_group)
    assert tuple(q.shape) == (groups, C + 1, 27)
    err = float((q.cpu().double() - want).abs().max())
    print('wgrad grouped %s C %d isz %r N %d (%d x %d) relu %d plan %r: err %.3g d32 %.3g err/d32 %.2f tol %.3g'
          % (what, C, tuple(isz), N, groups, per_group, int(relu), tuple(plan), err, d32, err / max(d32, 1e-30), tol))
    assert err <= tol, 'wgrad grouped %s: max error %.3g > tol %.3g (d32 %.3g, plan %r)' % (what, err, tol, d32, plan)
    if sums_after:
        w = 0.2 * torch.randn(C, 1, 3, 3, 3, generator=g); gamma = 1 + 0.3 * torch.randn(C, generator=g); beta = 0.2 * torch.randn(C, generator=g)
        w2 = w.double().reshape(C, 27)
        sums_w = torch.stack([(w2[None] * want[:, C:C + 1]).sum(2), (w2[None] * want[:, :C]).sum(2)], 2).reshape(groups * C, 2)
        dw_w = gamma.double()[:, None] * want[:, :C].sum(0) + beta.double()[:, None] * want[:, C].sum(0)[None]
        wabs = float(w2.abs().sum(1).max())
        # dw: |gamma| * G * tol + |beta| * G * tol from q, one fp32 rounding of the result
        tol_dw = (float(gamma.abs().max()) + float(beta.abs().max())) * groups * tol + EPS32 * float(dw_w.abs().max())
        for acc in (0, 1):
            r = 3 * torch.randn(C, 1, 3, 3, 3, generator=g)
            dw = r.clone().to(dev)
            sums = ops.bn_tconv1_sums(q, w.to(dev), gamma.to(dev), beta.to(dev), dw, acc)
            es = float((sums.cpu() - sums_w).abs().max())
            want_dw = dw_w.reshape(C, 1, 3, 3, 3) + (r.double() if acc else 0)
            ed = float((dw.cpu().double() - want_dw).abs().max())
            td = tol_dw + (EPS32 * float(r.abs().max() + dw_w.abs().max()) if acc else 0)
            print('  bn_tconv1_sums acc %d: sums err %.3g bound %.3g, dw err %.3g bound %.3g' % (acc, es, wabs * tol, ed, td))
            assert es <= wabs * tol, 'sums: %.3g > %.3g' % (es, wabs * tol)
            assert ed <= td, 'dw (accumulate %d): %.3g > %.3g' % (acc, ed, td)
    return dict(plan=plan, err=err, d32=d32, tol=tol)


# One item per block (items <= 512 <= grid: every block closes per-wave slabs after its only item): the (family, PA, UG, RES, ONE)
# instances of wgrad_rows_k and, for CA > 1, the slot schemes (nbuf = CA, 2, 1) that launch_rows selects over the scan of
# wgrad_selectable(); check_wgrad_coverage repeats that scan and asserts that a listed case runs each combination it finds (155).  Found with ops.wgrad_plan: per instance the cheapest shape of a scan over row widths
# (every k-step count class), plane heights (tall planes push the best tile out of the all-channels-resident budget) and sample
# counts (below 512 items the planner prefers small tiles, so the non-resident ONE = 2 / 3 instances need 32 to 128 samples).
# Each runs with accumulate 0 and 1.  (id, spec, layer input size, groups, per_group, prologue, plan fields asserted)
WGRAD_CASES = [
    ('conv1-ug2', 'conv1', (4, 5, 7), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv1-ug3', 'conv1', (4, 5, 12), 2, 1, 'relu', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv1-ug3-one6', 'conv1', (4, 5, 35), 2, 1, 'affine', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 6, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv1-ug4', 'conv1', (4, 5, 28), 2, 1, 'none', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv1-ug4-one2', 'conv1', (4, 5, 16), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv1-ug4-one3', 'conv1', (4, 5, 18), 2, 1, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv2-ug2-nbuf2', 'conv2', (5, 9, 77), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x3, 8 items
    ('conv2-ug2-res', 'conv2', (5, 7, 77), 2, 1, 'none', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv2-ug2-res-one2', 'conv2', (5, 7, 11), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv2-ug2-res-one3', 'conv2', (5, 7, 17), 2, 1, 'relu', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv2-ug3-res', 'conv2', (5, 7, 21), 2, 1, 'affine', {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv2-ug4-nbuf2', 'conv2', (3, 9, 257), 2, 1, 'none', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 8 items
    ('conv2-ug4-one2-nbuf2', 'conv2', (17, 43, 29), 4, 8, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 2x6, 512 items
    ('conv2-ug4-one3-nbuf2', 'conv2', (17, 25, 33), 4, 8, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 1x8, 512 items
    ('conv2-ug4-res', 'conv2', (5, 7, 29), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv3-ug2-nbuf2', 'conv3', (6, 98, 102), 2, 1, 'none', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 3x1, 384 items
    ('conv3-ug2-res', 'conv3', (4, 5, 40), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv3-ug2-res-one2', 'conv3', (4, 5, 7), 2, 1, 'relu', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv3-ug2-res-one3', 'conv3', (4, 5, 10), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv3-ug3-res', 'conv3', (4, 5, 12), 2, 1, 'none', {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv3-ug4-nbuf2', 'conv3', (10, 50, 130), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 384 items
    ('conv3-ug4-one2-nbuf2', 'conv3', (10, 23, 16), 4, 32, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 4x11, 512 items
    ('conv3-ug4-res', 'conv3', (4, 5, 16), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv4-ug2-nbuf2', 'conv4', (5, 7, 77), 2, 1, 'none', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 8 items
    ('conv4-ug2-res', 'conv4', (5, 13, 77), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x1, 24 items
    ('conv4-ug2-res-one2', 'conv4', (5, 7, 11), 2, 1, 'relu', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv4-ug2-res-one3', 'conv4', (5, 7, 17), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv4-ug3-nbuf2', 'conv4', (5, 9, 37), 2, 1, 'none', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x3, 8 items
    ('conv4-ug3-res', 'conv4', (5, 7, 21), 2, 1, 'affine', {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv4-ug4-nbuf1', 'conv4', (17, 193, 257), 2, 1, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 1}),   # tile 1x3, 512 items
    ('conv4-ug4-nbuf2', 'conv4', (5, 7, 53), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 8 items
    ('conv4-ug4-one2-nbuf2', 'conv4', (5, 13, 29), 2, 1, 'none', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 1x4, 8 items
    ('conv4-ug4-one3-nbuf2', 'conv4', (7, 7, 33), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 2x2, 8 items
    ('conv4-ug4-res', 'conv4', (5, 7, 29), 2, 1, 'relu', {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv5-ug2-nbuf2', 'conv5', (3, 6, 102), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 8 items
    ('conv5-ug2-res', 'conv5', (4, 5, 40), 2, 1, 'none', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv5-ug2-res-one2', 'conv5', (4, 5, 7), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv5-ug2-res-one3', 'conv5', (4, 5, 10), 2, 1, 'relu', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv5-ug3-res', 'conv5', (4, 5, 12), 2, 1, 'affine', {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv5-ug4-nbuf2', 'conv5', (3, 6, 130), 2, 1, 'none', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 8 items
    ('conv5-ug4-one2-nbuf2', 'conv5', (6, 23, 16), 4, 32, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 4x6, 512 items
    ('conv5-ug4-one3-nbuf2', 'conv5', (6, 23, 18), 4, 32, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 4x6, 512 items
    ('conv5-ug4-res', 'conv5', (4, 5, 16), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt1-ug2-nbuf2', 'convt1', (1, 4, 100), 2, 1, 'none', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 8 items
    ('convt1-ug2-res', 'convt1', (2, 3, 38), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt1-ug2-res-one2', 'convt1', (2, 3, 5), 2, 1, 'relu', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt1-ug2-res-one3', 'convt1', (2, 3, 8), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt1-ug3-res', 'convt1', (2, 3, 10), 2, 1, 'none', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt1-ug4-nbuf2', 'convt1', (1, 4, 128), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 8 items
    ('convt1-ug4-one2-nbuf2', 'convt1', (4, 21, 14), 4, 32, 'relu', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 4x6, 512 items
    ('convt1-ug4-one3-nbuf2', 'convt1', (4, 21, 16), 4, 32, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 4x6, 512 items
    ('convt1-ug4-res', 'convt1', (2, 3, 14), 2, 1, 'none', {'PA': 0, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2p-ug2-nbuf2', 'convt2p', (2, 3, 38), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 8 items
    ('convt2p-ug2-res', 'convt2p', (2, 6, 38), 2, 1, 'relu', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x1, 24 items
    ('convt2p-ug2-res-one2', 'convt2p', (2, 3, 5), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2p-ug2-res-one3', 'convt2p', (2, 3, 8), 2, 1, 'none', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2p-ug3-nbuf2', 'convt2p', (2, 4, 18), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x3, 8 items
    ('convt2p-ug3-res', 'convt2p', (2, 3, 10), 2, 1, 'relu', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2p-ug4-nbuf1', 'convt2p', (8, 96, 128), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 1}),   # tile 1x3, 512 items
    ('convt2p-ug4-nbuf2', 'convt2p', (2, 3, 26), 2, 1, 'none', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 8 items
    ('convt2p-ug4-one2-nbuf2', 'convt2p', (2, 6, 14), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 1x4, 8 items
    ('convt2p-ug4-one3-nbuf2', 'convt2p', (3, 3, 16), 2, 1, 'relu', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 2x2, 8 items
    ('convt2p-ug4-res', 'convt2p', (2, 3, 14), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2-ug2-nbuf2', 'convt2', (2, 3, 38), 2, 1, 'none', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 8 items
    ('convt2-ug2-res', 'convt2', (2, 6, 38), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x1, 24 items
    ('convt2-ug2-res-one2', 'convt2', (2, 3, 5), 2, 1, 'relu', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2-ug2-res-one3', 'convt2', (2, 3, 8), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2-ug3-nbuf2', 'convt2', (2, 4, 18), 2, 1, 'none', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x3, 8 items
    ('convt2-ug3-res', 'convt2', (2, 3, 10), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt2-ug4-nbuf1', 'convt2', (8, 96, 128), 2, 1, 'relu', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 1}),   # tile 1x3, 512 items
    ('convt2-ug4-nbuf2', 'convt2', (2, 3, 26), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 8 items
    ('convt2-ug4-one2-nbuf2', 'convt2', (2, 6, 14), 2, 1, 'none', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 1x4, 8 items
    ('convt2-ug4-one3-nbuf2', 'convt2', (3, 3, 16), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 2x2, 8 items
    ('convt2-ug4-res', 'convt2', (2, 3, 14), 2, 1, 'relu', {'PA': 0, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt3-ug2-nbuf2', 'convt3', (4, 96, 100), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 3x1, 384 items
    ('convt3-ug2-res', 'convt3', (2, 3, 38), 2, 1, 'none', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt3-ug2-res-one2', 'convt3', (2, 3, 5), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt3-ug2-res-one3', 'convt3', (2, 3, 8), 2, 1, 'relu', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt3-ug3-res', 'convt3', (2, 3, 10), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt3-ug4-nbuf2', 'convt3', (8, 48, 128), 2, 1, 'none', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x2, 384 items
    ('convt3-ug4-one2-nbuf2', 'convt3', (8, 21, 14), 4, 32, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 4x11, 512 items
    ('convt3-ug4-res', 'convt3', (2, 3, 14), 2, 1, 'relu', {'PA': 0, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt4-ug2-nbuf2', 'convt4', (1, 4, 100), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 16 items
    ('convt4-ug2-res', 'convt4', (2, 3, 5), 2, 1, 'none', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('convt4-ug3-nbuf2', 'convt4', (3, 4, 36), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x3, 16 items
    ('convt4-ug3-res', 'convt4', (2, 3, 10), 2, 1, 'relu', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('convt4-ug4-nbuf1', 'convt4', (1, 96, 128), 2, 4, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 1}),   # tile 1x3, 512 items
    ('convt4-ug4-nbuf2', 'convt4', (2, 3, 30), 2, 1, 'none', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 2x2, 8 items
    ('convt4-ug4-one2-nbuf2', 'convt4', (4, 6, 14), 4, 32, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 3x4, 512 items
    ('convt4-ug4-one3-nbuf2', 'convt4', (4, 21, 16), 4, 8, 'relu', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 1x8, 480 items
    ('convt4-ug4-res', 'convt4', (2, 3, 14), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('convt4hr-ug2-nbuf2', 'convt4hr', (1, 4, 100), 2, 1, 'none', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 16 items
    ('convt4hr-ug2-res', 'convt4hr', (2, 3, 5), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('convt4hr-ug3-nbuf2', 'convt4hr', (4, 96, 33), 2, 1, 'relu', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 4x1, 384 items
    ('convt4hr-ug3-res', 'convt4hr', (2, 3, 10), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('convt4hr-ug4-nbuf1', 'convt4hr', (1, 96, 128), 2, 4, 'none', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 1}),   # tile 1x3, 512 items
    ('convt4hr-ug4-nbuf2', 'convt4hr', (1, 4, 128), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 16 items
    ('convt4hr-ug4-one2-nbuf2', 'convt4hr', (4, 6, 14), 4, 32, 'relu', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 3x4, 512 items
    ('convt4hr-ug4-one3-nbuf2', 'convt4hr', (4, 6, 16), 4, 32, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 3x4, 512 items
    ('convt4hr-ug4-res', 'convt4hr', (2, 3, 14), 2, 1, 'none', {'PA': 0, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('convt4toy-ug2-nbuf2', 'convt4toy', (2, 4, 38), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x3, 8 items
    ('convt4toy-ug2-res', 'convt4toy', (2, 3, 38), 2, 1, 'relu', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt4toy-ug2-res-one2', 'convt4toy', (2, 3, 5), 2, 1, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt4toy-ug2-res-one3', 'convt4toy', (2, 3, 8), 2, 1, 'none', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt4toy-ug3-res', 'convt4toy', (2, 3, 10), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt4toy-ug4-nbuf2', 'convt4toy', (1, 4, 128), 2, 1, 'relu', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 8 items
    ('convt4toy-ug4-one2-nbuf2', 'convt4toy', (8, 21, 14), 4, 8, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 2x6, 512 items
    ('convt4toy-ug4-one3-nbuf2', 'convt4toy', (8, 12, 16), 4, 8, 'none', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 1x8, 512 items
    ('convt4toy-ug4-res', 'convt4toy', (2, 3, 14), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt5-ug2', 'convt5', (2, 3, 5), 2, 1, 'relu', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt5-ug3', 'convt5', (2, 3, 10), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt5-ug3-one6', 'convt5', (2, 3, 33), 2, 1, 'none', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 6, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt5-ug4', 'convt5', (2, 3, 26), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt5-ug4-one2', 'convt5', (2, 3, 14), 2, 1, 'relu', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('convt5-ug4-one3', 'convt5', (2, 3, 16), 2, 1, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 'CA'}),   # tile 1x2, 8 items
    ('conv5x3x3-ug2-nbuf2', 'conv5x3x3', (5, 9, 201), 2, 1, 'none', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 16 items
    ('conv5x3x3-ug2-res', 'conv5x3x3', (7, 7, 11), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('conv5x3x3-ug3-nbuf2', 'conv5x3x3', (9, 9, 73), 2, 1, 'relu', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x3, 16 items
    ('conv5x3x3-ug3-res', 'conv5x3x3', (7, 7, 21), 2, 1, 'affine', {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('conv5x3x3-ug4-nbuf1', 'conv5x3x3', (5, 193, 257), 2, 4, 'none', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 1}),   # tile 1x3, 512 items
    ('conv5x3x3-ug4-nbuf2', 'conv5x3x3', (7, 7, 61), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 2x2, 8 items
    ('conv5x3x3-ug4-one2-nbuf2', 'conv5x3x3', (11, 13, 29), 4, 32, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 3x4, 512 items
    ('conv5x3x3-ug4-one3-nbuf2', 'conv5x3x3', (11, 43, 33), 4, 8, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 1x8, 480 items
    ('conv5x3x3-ug4-res', 'conv5x3x3', (7, 7, 29), 2, 1, 'none', {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('conv4x4x4-ug2-nbuf2', 'conv4x4x4', (4, 10, 202), 2, 1, 'affine', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 16 items
    ('conv4x4x4-ug2-res', 'conv4x4x4', (6, 8, 12), 2, 1, 'relu', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('conv4x4x4-ug3-nbuf2', 'conv4x4x4', (10, 194, 68), 2, 1, 'affine', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 4x1, 384 items
    ('conv4x4x4-ug3-res', 'conv4x4x4', (6, 8, 22), 2, 1, 'none', {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    ('conv4x4x4-ug4-nbuf1', 'conv4x4x4', (4, 194, 258), 2, 4, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 1}),   # tile 1x3, 512 items
    ('conv4x4x4-ug4-nbuf2', 'conv4x4x4', (4, 10, 258), 2, 1, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2}),   # tile 1x1, 16 items
    ('conv4x4x4-ug4-one2-nbuf2', 'conv4x4x4', (10, 14, 30), 4, 32, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2}),   # tile 3x4, 512 items
    ('conv4x4x4-ug4-one3-nbuf2', 'conv4x4x4', (10, 14, 34), 4, 32, 'none', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),   # tile 3x4, 512 items
    ('conv4x4x4-ug4-res', 'conv4x4x4', (6, 8, 30), 2, 1, 'affine', {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA'}),   # tile 2x2, 8 items
    # selected only from 512 items on (wide rows of 81 to 212 positions at 128 samples, or rows so wide that one item already fills the tile)
    ('conv3-ug3-nbuf2', 'conv3', (6, 23, 83), 2, 4, 'affine', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),
    ('conv3-ug4-one3-nbuf2', 'conv3', (8, 25, 18), 4, 32, 'relu', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),
    ('conv4-ug2-nbuf1', 'conv4', (5, 13, 205), 4, 32, 'affine', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('conv4-ug3-nbuf1', 'conv4', (5, 13, 211), 4, 32, 'none', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('conv5-ug3-nbuf2', 'conv5', (3, 3, 83), 2, 1, 'affine', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),
    ('convt1-ug3-nbuf2', 'convt1', (1, 1, 81), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),
    ('convt2p-ug2-nbuf1', 'convt2p', (2, 6, 102), 4, 32, 'affine', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt2p-ug3-nbuf1', 'convt2p', (2, 6, 105), 4, 32, 'relu', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt2-ug2-nbuf1', 'convt2', (2, 6, 102), 4, 32, 'none', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt2-ug3-nbuf1', 'convt2', (2, 6, 105), 4, 32, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt3-ug3-nbuf2', 'convt3', (4, 21, 81), 2, 4, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),
    ('convt3-ug4-one3-nbuf2', 'convt3', (6, 23, 16), 4, 32, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2}),
    ('convt4-ug2-nbuf1', 'convt4', (3, 4, 97), 4, 32, 'relu', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt4-ug3-nbuf1', 'convt4', (2, 3, 105), 4, 32, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt4hr-ug2-nbuf1', 'convt4hr', (3, 4, 97), 4, 32, 'affine', {'PA': 0, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt4hr-ug3-nbuf1', 'convt4hr', (3, 4, 105), 4, 32, 'none', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('convt4toy-ug3-nbuf2', 'convt4toy', (1, 1, 105), 2, 1, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2}),
    ('conv5x3x3-ug2-nbuf1', 'conv5x3x3', (9, 9, 195), 4, 32, 'affine', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('conv5x3x3-ug3-nbuf1', 'conv5x3x3', (7, 7, 211), 4, 32, 'relu', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('conv4x4x4-ug2-nbuf1', 'conv4x4x4', (8, 10, 196), 4, 32, 'affine', {'PA': 1, 'UG': 2, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
    ('conv4x4x4-ug3-nbuf1', 'conv4x4x4', (8, 10, 212), 4, 32, 'none', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 1}),
]

# 513 to 640 items with the tile a layer of the networks gets (named behind each case): one item per block where the occupancy query
# lets the grid grow past 512 blocks -- the cross-wave LDS reduction and one slab per block without the loop -- and a second trip
# for the first blocks where it stops at 512.  Same fields as WGRAD_CASES; run with accumulate 0 and 1.
WGRAD_MID_CASES = [
    ('conv2-mid-w16-3x43-pd-ph', 'conv2', (15, 23, 33), 3, 43, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2, 'TPD': 4, 'TPH': 6, 'items': 516}),   # 41x49x35 conv2
    ('conv3-mid-w14-2x43-pd-ph', 'conv3', (7, 23, 16), 2, 43, 'affine', {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA', 'TPD': 3, 'TPH': 8, 'items': 516}),   # 41x49x35 conv3
    ('convt2p-mid-w7-3x43-pd-ph', 'convt2p', (5, 3, 7), 3, 43, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 4, 'TPH': 2, 'items': 516}),   # 41x49x35 convt2
    ('convt3-mid-w14-3x43-pd-ph', 'convt3', (7, 21, 14), 3, 43, 'affine', {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 4, 'TPH': 11, 'items': 516}),   # 41x49x35 convt3
    ('conv3-mid-w14-3x19-pd', 'conv3', (19, 23, 16), 3, 19, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 2, 'TPH': 21, 'items': 513}),   # 41x49x35 conv3
    ('conv4-mid-w6-3x43-pd-ph', 'conv4', (11, 7, 13), 3, 43, 'affine', {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 4, 'TPH': 2, 'items': 516}),   # 41x49x35 conv4
    ('convt1-mid-w5-2x129-pd', 'convt1', (5, 8, 5), 2, 129, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 3, 'TPH': 8, 'items': 516}),   # 41x49x35 convt1
    ('conv4-mid-w15-2x43-pd-ph', 'conv4', (11, 45, 31), 2, 43, 'affine', {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 3, 'TPH': 8, 'items': 516}),   # 82x98x70 conv4
    ('conv1-mid-w19-3x43-pd-ph', 'conv1', (9, 11, 21), 3, 43, 'affine', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 5, 'items': 516}),   # 21x21x21 conv1
    ('convt1-mid-w1-3x171', 'convt1', (1, 1, 1), 3, 171, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 1, 'TPH': 1, 'items': 513}),   # 21x21x21 convt1
    ('convt4toy-mid-w9-3x43-pd-ph', 'convt4toy', (5, 9, 9), 3, 43, 'affine', {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA', 'TPD': 3, 'TPH': 5, 'items': 516}),   # 21x21x21 convt4
    ('convt5-mid-w19-3x43-pd-ph', 'convt5', (7, 19, 19), 3, 43, 'affine', {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 10, 'items': 516}),   # 21x21x21 convt5
    ('conv1-mid-w19-3x43-pd-ph-t4x10', 'conv1', (9, 21, 21), 3, 43, 'affine', {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 10, 'items': 516}),   # 21x21x21 conv1
    ('conv2-mid-w9-3x43-pd-ph', 'conv2', (11, 11, 19), 3, 43, 'affine', {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA', 'TPD': 3, 'TPH': 4, 'items': 516}),   # 21x21x21 conv2
    ('convt2-mid-w3-3x171', 'convt2', (3, 3, 3), 3, 171, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 3, 'TPH': 3, 'items': 513}),   # 21x21x21 convt2
    ('convt3-mid-w7-2x129-pd', 'convt3', (7, 7, 7), 2, 129, 'affine', {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 4, 'TPH': 7, 'items': 516}),   # 21x21x21 convt3
]

# The persistent item loop: items >= 4097 > 2 * 2048 >= 2 * grid whatever the occupancy query answers, and no multiple of 256, so of no
# grid.  Built by the rule: keep the row width PW of the production layer named behind the case (it alone decides UG and ONE), shrink
# depth and height as far as (instance, slot scheme, TPD, TPH) stay what production gets -- the same tile gives the same LDS size, so
# the occupancy query answers as in production and `grid` / `wave_slabs` follow it on either library -- then raise N.  -pd / -ph: the
# last tile in depth / in rows is partial (a short tile followed by a full one in the same block's LDS).  Groups: 3 x 683, 5 x 205 and
# 3 x 1366 samples against a stride of grid / items-per-sample samples: a block's successive items cross batch-norm groups;
# conv3-loop-w14-2x228-pd has 18 items per sample, a stride of at most 2048 / 18 = 113 < 228 samples: they also stay inside one.
# -small-tile: at the production tile the window tensor of 4,097 items passes 256 MB (16 or 8 channels at stride 2: 100 to 240 KB per item),
# so depth and height are shrunk further and the planner picks a smaller tile of the same instance and slot scheme; with less LDS the
# occupancy query may answer more blocks than in production (see WGRAD_NOT_COVERED).  convt4hr-loop-w33 keeps the production tile of
# the 4x4x4 plane-shift layer with a dy tensor of 428 MB, above the 256 MB limit: a scan of depths and heights on the host build finds no
# shape with the production tuple (1 x 12 tile, 2 blocks per CU) under about 321 MB at 4,097 items (about 100 KB of dy per item: four window
# planes of 8 channels per position plane), and a smaller tile changes the occupancy answer and with it `wave_slabs`.
# (id, spec, layer input size, groups, per_group, prologue, accumulate, plan fields asserted)
WGRAD_LOOP_CASES = [
    # the smallest tiles the one-channel family takes at 19-position rows (one item per sample): what the host build can walk in under 20 s
    ('convt5-loop-w19-7x586-host', 'convt5', (2, 3, 19), 7, 586, 'affine', 1, {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'items': 4102}),
    ('conv1-loop-w19-7x586-host', 'conv1', (4, 5, 21), 7, 586, 'affine', 0, {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'items': 4102}),
    ('conv1-loop-w33-3x683-pd', 'conv1', (7, 14, 35), 3, 683, 'affine', 0, {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 6, 'nbuf': 'CA', 'TPD': 3, 'TPH': 12, 'items': 4098}),   # 41x49x35 conv1
    ('conv2-loop-w16-5x410-small-tile', 'conv2', (11, 7, 33), 5, 410, 'affine', 1, {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2, 'TPD': 4, 'TPH': 3, 'items': 4100}),   # 41x49x35 conv2
    ('conv3-loop-w14-3x683-pd', 'conv3', (7, 10, 16), 3, 683, 'affine', 0, {'PA': 1, 'UG': 4, 'RES': 1, 'ONE': 0, 'nbuf': 'CA', 'TPD': 3, 'TPH': 8, 'items': 4098}),   # 41x49x35 conv3
    ('convt2p-loop-w7-3x683-pd', 'convt2p', (5, 2, 7), 3, 683, 'affine', 1, {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 4, 'TPH': 2, 'items': 4098}),   # 41x49x35 convt2
    ('convt3-loop-w14-5x205-pd-ph', 'convt3', (7, 21, 14), 5, 205, 'affine', 0, {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 4, 'TPH': 11, 'items': 4100}),   # 41x49x35 convt3
    ('convt4-loop-w16-5x410-small-tile', 'convt4', (2, 7, 16), 5, 410, 'affine', 1, {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 3, 'nbuf': 2, 'TPD': 2, 'TPH': 7, 'items': 4100}),   # 41x49x35 convt4
    ('convt5-loop-w33-3x683-ph', 'convt5', (3, 23, 33), 3, 683, 'affine', 0, {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 6, 'nbuf': 'CA', 'TPD': 3, 'TPH': 12, 'items': 4098}),   # 41x49x35 convt5
    ('conv3-loop-w14-2x228-pd', 'conv3', (19, 23, 16), 2, 228, 'affine', 1, {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 2, 'TPH': 21, 'items': 4104}),   # 41x49x35 conv3
    ('conv4-loop-w6-3x683-pd', 'conv4', (11, 5, 13), 3, 683, 'affine', 0, {'PA': 1, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 4, 'TPH': 2, 'items': 4098}),   # 41x49x35 conv4
    ('convt1-loop-w5-3x683-pd', 'convt1', (5, 8, 5), 3, 683, 'affine', 1, {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 3, 'TPH': 8, 'items': 4098}),   # 41x49x35 convt1
    ('conv1-loop-w68-5x205-pd-ph', 'conv1', (9, 9, 70), 5, 205, 'affine', 0, {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 4, 'items': 4100}),   # 82x98x70 conv1
    ('conv2-loop-w33-5x410-small-tile', 'conv2', (11, 3, 67), 5, 410, 'affine', 1, {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2, 'TPD': 4, 'TPH': 1, 'items': 4100}),   # 82x98x70 conv2
    ('conv3-loop-w31-5x205-pd-ph', 'conv3', (9, 11, 33), 5, 205, 'affine', 0, {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2, 'TPD': 4, 'TPH': 5, 'items': 4100}),   # 82x98x70 conv3
    ('conv4-loop-w15-5x410-small-tile', 'conv4', (11, 5, 31), 5, 410, 'affine', 1, {'PA': 1, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 4, 'TPH': 2, 'items': 4100}),   # 82x98x70 conv4
    ('convt1-loop-w13-5x205-pd-ph', 'convt1', (7, 19, 13), 5, 205, 'affine', 0, {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 4, 'TPH': 10, 'items': 4100}),   # 82x98x70 convt1
    ('convt2-loop-w15-5x410-small-tile', 'convt2', (5, 2, 15), 5, 410, 'affine', 1, {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 2, 'nbuf': 2, 'TPD': 4, 'TPH': 2, 'items': 4100}),   # 82x98x70 convt2
    ('convt3-loop-w31-5x205-pd-ph', 'convt3', (7, 9, 31), 5, 205, 'affine', 0, {'PA': 0, 'UG': 4, 'RES': 0, 'ONE': 0, 'nbuf': 2, 'TPD': 4, 'TPH': 5, 'items': 4100}),   # 82x98x70 convt3
    ('convt4hr-loop-w33-5x205-ph', 'convt4hr', (1, 23, 33), 5, 205, 'affine', 1, {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 2, 'TPD': 1, 'TPH': 12, 'items': 4100}),   # 82x98x70 convt4
    ('convt5-loop-w68-5x205-pd-ph', 'convt5', (7, 7, 68), 5, 205, 'affine', 0, {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 4, 'items': 4100}),   # 82x98x70 convt5
    ('conv1-loop-w19-3x683-pd', 'conv1', (9, 7, 21), 3, 683, 'affine', 1, {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 5, 'items': 4098}),   # 21x21x21 conv1
    ('convt1-loop-w1-3x1366', 'convt1', (1, 1, 1), 3, 1366, 'affine', 0, {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 1, 'TPH': 1, 'items': 4098}),   # 21x21x21 convt1
    ('convt4toy-loop-w9-5x205-pd-ph', 'convt4toy', (5, 9, 9), 5, 205, 'affine', 1, {'PA': 0, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA', 'TPD': 3, 'TPH': 5, 'items': 4100}),   # 21x21x21 convt4
    ('convt5-loop-w19-5x205-pd-ph', 'convt5', (7, 19, 19), 5, 205, 'affine', 0, {'PA': 0, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 10, 'items': 4100}),   # 21x21x21 convt5
    ('conv1-loop-w19-5x205-pd-ph', 'conv1', (9, 21, 21), 5, 205, 'affine', 1, {'PA': 1, 'UG': 3, 'RES': 0, 'ONE': 0, 'nbuf': 'CA', 'TPD': 4, 'TPH': 10, 'items': 4100}),   # 21x21x21 conv1
    ('conv2-loop-w9-3x683-pd', 'conv2', (11, 9, 19), 3, 683, 'affine', 0, {'PA': 1, 'UG': 3, 'RES': 1, 'ONE': 0, 'nbuf': 'CA', 'TPD': 3, 'TPH': 4, 'items': 4098}),   # 21x21x21 conv2
    ('convt2-loop-w3-3x1366', 'convt2', (3, 3, 3), 3, 1366, 'affine', 1, {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 3, 'TPH': 3, 'items': 4098}),   # 21x21x21 convt2
    ('convt3-loop-w7-3x683-pd', 'convt3', (7, 7, 7), 3, 683, 'affine', 0, {'PA': 0, 'UG': 2, 'RES': 1, 'ONE': 2, 'nbuf': 'CA', 'TPD': 4, 'TPH': 7, 'items': 4098}),   # 21x21x21 convt3
]

# (id, C, input size, groups, per_group, relu, plan fields asserted, follow with vg_bn_tconv1_sums, loop)
WGRAD_GROUPED_CASES = [
    ('grouped-small-w33', 8, (3, 4, 33), 2, 2, True, {'GRP': 1, 'ONE': 6, 'wave_slabs': 1}, False, False),          # ipb == grp_items, per-wave slabs
    ('grouped-mid-w19', 8, (2, 3, 19), 2, 300, True, {'GRP': 1, 'ONE': 0, 'items': 600}, True, False),               # ipb == grp_items where the grid may pass 512
    ('grouped-loop-w33-3x1366', 8, (2, 3, 33), 3, 1366, True, {'GRP': 1, 'ONE': 6, 'items': 4098}, False, True),     # odd number of groups; ipb <= 682 < grp_items / 2
    ('grouped-loop-w19-2x2051', 8, (2, 3, 19), 2, 2051, False, {'GRP': 1, 'ONE': 0, 'items': 4102}, True, True),     # ipb <= 1024 < grp_items / 2; then vg_bn_tconv1_sums
]

# On the host build a case costs what its items cost: these measured 20 to 52 s (the others 0.1 to 17 s), above the 20 s a host case
# may take, so they run on the GPU only (milliseconds there) -- the single-slot (nbuf = 1) cases with their 128-position rows and the
# non-resident compile-time-row instances that need 128 samples
WGRAD_GPU_ONLY = ('conv3-ug2-nbuf2', 'conv3-ug4-nbuf2', 'conv3-ug4-one2-nbuf2', 'conv4-ug4-nbuf1', 'conv5-ug4-one2-nbuf2', 'conv5-ug4-one3-nbuf2',
                  'convt1-ug4-one2-nbuf2', 'convt1-ug4-one3-nbuf2', 'convt2p-ug4-nbuf1', 'convt2-ug4-nbuf1', 'convt3-ug4-one2-nbuf2',
                  'convt4-ug4-nbuf1', 'convt4hr-ug4-nbuf1', 'conv5x3x3-ug4-nbuf1', 'conv4x4x4-ug4-nbuf1',
                  # mid cases on the large production tiles: 31 to 68 s
                  'conv2-mid-w16-3x43-pd-ph', 'conv3-mid-w14-2x43-pd-ph', 'convt3-mid-w14-3x43-pd-ph', 'conv3-mid-w14-3x19-pd',
                  'convt1-mid-w5-2x129-pd', 'conv4-mid-w15-2x43-pd-ph',
                  # selected only from 512 items on: 336 items on 81 / 83-position rows 27 and 23 s; the sixteen 128-sample cases (512 items on
                  # rows of 16 to 212 positions) were not timed one by one: a host run of them was cut off after 15 minutes
                  'conv3-ug3-nbuf2', 'convt3-ug3-nbuf2', 'conv3-ug4-one3-nbuf2', 'convt3-ug4-one3-nbuf2', 'conv4-ug2-nbuf1', 'conv4-ug3-nbuf1',
                  'convt2p-ug2-nbuf1', 'convt2p-ug3-nbuf1', 'convt2-ug2-nbuf1', 'convt2-ug3-nbuf1', 'convt4-ug2-nbuf1', 'convt4-ug3-nbuf1',
                  'convt4hr-ug2-nbuf1', 'convt4hr-ug3-nbuf1', 'conv5x3x3-ug2-nbuf1', 'conv5x3x3-ug3-nbuf1', 'conv4x4x4-ug2-nbuf1',
                  'conv4x4x4-ug3-nbuf1')

# Loop cases: a host item costs 3 to 6 ms, so 4,097 items take 11 s (these two: 11.7 and 10.7 s) on the smallest tiles and 23 to 70 s
# on the production tiles (convt1-loop-w1 25 s, conv1-loop-w19-3x683 24 s, conv4-loop-w6 41 s, convt2p-loop-w7 40 s, conv1-loop-w33 51 s,
# convt2-loop-w3 70 s; the larger ones were not waited for): every other plain loop case runs on the GPU only.  The grouped loop cases
# take 13 and 16 s and run on the host build.
WGRAD_LOOP_HOST = ('convt5-loop-w19-7x586-host', 'conv1-loop-w19-7x586-host')
WGRAD_LOOP_GPU_ONLY = tuple(c[0] for c in WGRAD_LOOP_CASES if c[0] not in WGRAD_LOOP_HOST)


def run_wgrad_instance_listed(dev, case, seed=0):
    """a case of WGRAD_CASES / WGRAD_MID_CASES: written and accumulated, one float64 reference"""
    cid, sname, isz, groups, per_group, prologue, expect = case
    return run_wgrad_case(dev, WG_SPECS[sname], isz, groups, per_group, prologue, (0, 1), expect, seed, what=cid)


def run_wgrad_loop_listed(dev, case, seed=0):
    cid, sname, isz, groups, per_group, prologue, acc, expect = case
    return run_wgrad_case(dev, WG_SPECS[sname], isz, groups, per_group, prologue, acc, expect, seed, loop=True, what=cid)


def run_wgrad_grouped_listed(dev, case, seed=0):
    cid, C, isz, groups, per_group, relu, expect, sums_after, loop = case
    return run_wgrad_grouped_case(dev, C, isz, groups, per_group, relu, expect, sums_after, seed, loop, what=cid)


# layers of LAYERS that test_layer_bound_gradients runs: name -> (index, with batch norm)
BOUND_LAYERS = {'conv3': (2, True), 'conv2': (1, False), 'convt2': (6, False), 'convt4': (8, False), 'convt5': (9, True)}


# the bench configurations: (image, ((batch B, covariates C), ...)); encoder launches see N = B samples, decoder launches N = B * (C + 1).
# 82x98x70: the per-GPU slice of `bench.py --hires` (batch 64, 12 covariates).
WGRAD_NETS = (((41, 49, 35), ((32, 3), (64, 8))), ((82, 98, 70), ((64, 12),)), ((21, 21, 21), ((32, 3), (64, 8))))


def wgrad_production_plans():
    """-> [(image, B, C, layer, plan)] for every weight-gradient launch of the three networks at the bench sample counts, plus the grouped
    launch of the last decoder stage ('convt5/grouped'), from the library's planner (nothing is launched)."""
    from vae_gam_amd.schema import net_geometry
    out = []
    for img, cfgs in WGRAD_NETS:
        geo = net_geometry(img)
        for B, C in cfgs:
            for specs, sizes, N in ((geo.enc, geo.enc_sizes(), B), (geo.dec, geo.dec_sizes(), B * (C + 1))):
                for spec, isz in zip(specs, sizes):
                    out.append((img, B, C, spec.name, ops.wgrad_plan(spec, *_wgrad_shapes(spec, isz, N), True, B)))
            spec, isz = geo.dec[-1], geo.dec_sizes()[-2]
            out.append((img, B, C, spec.name + '/grouped', ops.wgrad_plan(spec, *_wgrad_shapes(spec, isz, B * (C + 1)), True, B, grouped=True)))
    return out


def fc_production_plans(L=32):
    """-> [(what, plan, [(ksplit, batch) per job])] for every fully connected launch of a train step of the three networks at the bench
    sample counts: LinearAct and HeadsAct are driven forward and backward on CPU tensors of the production shapes (parameters with
    16-byte aligned .grad views, as the optimiser lays them out) with ops.fc_launch replaced by a recorder that asks ops.fc_plan:
    nothing is launched and no tensor is read, only shapes and pointers flow."""
    from vae_gam_amd.schema import net_geometry
    out, tag = [], ['']

    def record(ref, jobs):
        what = ' + '.join('%dx%dx%d' % (j[0].d.M, j[0].d.N, j[0].d.K) for j in jobs)
        out.append(('%s %s' % (tag[0], what), ops.fc_plan(jobs), [(int(j[0].d.ksplit), int(j[0].d.batch)) for j in jobs]))

    def linear(fin, fout):
        lay = types.SimpleNamespace(weight=torch.nn.Parameter(torch.empty(fout, fin)), bias=torch.nn.Parameter(torch.empty(fout)))
        lay.weight.grad = torch.empty_like(lay.weight); lay.bias.grad = torch.empty_like(lay.bias)
        return lay
    H = 50
    saved = ops.fc_launch
    ops.fc_launch = record
    try:
        for img, cfgs in WGRAD_NETS:
            geo = net_geometry(img)
            for B, C in cfgs:
                name = '%s B%d C%d ' % ('x'.join(map(str, img)), B, C)
                fc1, fc2 = linear(geo.enc_flat, 200), linear(200, 100)
                heads = [torch.empty(s) for s in ((3 * H, 100), (3 * H,), (3, L, H), (3, 1, L))] * 2
                tag[0] = name + 'encoder'
                x = torch.empty(B, geo.enc_flat, requires_grad=True)
                h = ops.linear_act(fc2, ops.linear_act(fc1, x, True, relu_in=True), True)
                mwa = ops.HeadsAct.apply(h, *heads)
                mwa.backward(torch.empty_like(mwa))
                tag[0] = name + 'decoder'
                z = torch.empty(B * (C + 1), L + C + 1, requires_grad=True)
                lays = [linear(L + C + 1, 50), linear(50, 100), linear(100, 200), linear(200, geo.dec_flat)]
                h = z
                for i, lay in enumerate(lays):
                    h = ops.linear_act(lay, h, i < 3)
                h.backward(torch.empty_like(h))
    finally:
        ops.fc_launch = saved
    return out


def wgrad_case_plans():
    """-> [(id, plan, accumulate values, loop, grouped, position size)] of every listed case"""
    out = []
    for cid, sname, isz, groups, per_group, prologue, expect in WGRAD_CASES + WGRAD_MID_CASES:
        spec = WG_SPECS[sname]; xs, ys = _wgrad_shapes(spec, isz, groups * per_group)
        out.append((cid, ops.wgrad_plan(spec, xs, ys, prologue != 'none', per_group), {0, 1}, False, False, (ys if spec.kind == 'conv' else xs)[2:]))
    for cid, sname, isz, groups, per_group, prologue, acc, expect in WGRAD_LOOP_CASES:
        spec = WG_SPECS[sname]; xs, ys = _wgrad_shapes(spec, isz, groups * per_group)
        out.append((cid, ops.wgrad_plan(spec, xs, ys, prologue != 'none', per_group), {acc}, True, False, (ys if spec.kind == 'conv' else xs)[2:]))
    for cid, C, isz, groups, per_group, relu, expect, sums_after, loop in WGRAD_GROUPED_CASES:
        spec = ConvSpec('convt', C, 1, _K3, 1); xs, ys = _wgrad_shapes(spec, isz, groups * per_group)
        out.append((cid, ops.wgrad_plan(spec, xs, ys, relu, per_group, grouped=True), {0, 1} if sums_after else {0}, loop, True, xs[2:]))
    return out


_SCAN_PLANES = ((1, 1), (2, 3), (2, 6), (3, 4), (4, 6), (4, 8), (6, 23), (8, 21), (10, 50), (4, 96), (8, 96), (2, 8), (4, 21), (8, 12))


def wgrad_selectable():
    """Every (family, PA, UG, RES, GRP = 0, ONE, nbuf class) the planner selects over a scan of what ops can describe: the WG_SPECS
    layers, rows of 1 to 130 positions, 14 plane sizes (depth x height of the position tensor) and 2, 8, 32 and 128 samples (the last
    reach the 512 items from which the planner stops preferring small tiles); launches nothing, about 2 s.  -> {combination: example}"""
    found = {}
    for sname, spec in WG_SPECS.items():
        for W in range(1, 131):
            for D, H in _SCAN_PLANES:
                P = (D, H, W)
                isz = tuple((P[a] - 1) * spec.stride + spec.k[a] for a in range(3)) if spec.kind == 'conv' else P
                for N in (2, 8, 32, 128):
                    if N * D * H * W * max(spec.ci, spec.co) * (8 if spec.stride == 2 else 1) * 4 > 250e6:
                        continue
                    try:
                        plan = ops.wgrad_plan(spec, *_wgrad_shapes(spec, isz, N), True, 1)
                    except _lib.VgError:
                        continue
                    found.setdefault(wgrad_tuple(plan)[:7], (sname, isz, N))
    return found


def wgrad_coverage():
    """What WGRAD_CASES, WGRAD_LOOP_CASES and WGRAD_GROUPED_CASES run against what the networks launch, from the plans alone
    (nothing is launched; `grid`, `wave_slabs` and so the tuples are those of the library that is loaded)."""
    cov = dict(production={}, cases={}, instances=set(), production_bpc={}, loop_case_bpc={}, accumulate=set(), wave_slabs=set(), nbuf=set(), PAD=set(), DSH=set(), partial_d=[], partial_h=[],
               loops=[], loops_grouped=[])
    for img, B, C, layer, plan in wgrad_production_plans():
        cov['production'].setdefault(img, {}).setdefault(wgrad_tuple(plan), []).append('%s B%d C%d' % (layer, B, C))
        cov['production_bpc'].setdefault(wgrad_tuple(plan), set()).add(plan.blocks_per_cu)
    for cid, plan, accs, loop, grouped, pos in wgrad_case_plans():
        if wgrad_tuple(plan)[-1] == int(loop):                      # a looping production launch is matched by loop cases only
            cov['cases'].setdefault(wgrad_tuple(plan), []).append(cid)
        cov['instances'].add(wgrad_tuple(plan)[:7])
        if loop:
            cov['loop_case_bpc'].setdefault(wgrad_tuple(plan)[:7], set()).add(plan.blocks_per_cu)
        cov['accumulate'] |= accs; cov['wave_slabs'].add(plan.wave_slabs); cov['PAD'].add(plan.PAD); cov['DSH'].add(plan.DSH)
        if plan.CA > 1:
            cov['nbuf'].add('CA' if plan.nbuf == plan.CA else plan.nbuf)
        looping = (plan.grp_items >= 2 * plan.ipb) if grouped else (plan.items >= 4097 and plan.items >= 2 * plan.grid)
        assert looping == loop, (cid, plan)
        if loop:
            cov['loops_grouped' if grouped else 'loops'].append(cid)
            if (pos[0] + plan.DSH) % plan.TPD:
                cov['partial_d'].append(cid)
            if pos[1] % plan.TPH:
                cov['partial_h'].append(cid)
    return cov


# Production launches of the 82x98x70 network that may go unmatched, as (first seven tuple fields, reason) -- at most two.  Both are
# 16-channel stride-2 layers whose production tile (3 x 8, 54,816 bytes of LDS) cannot be kept under the 256 MB limit at 4,097 items
# (693 MB); the -small-tile cases run the same instance with 32,768 bytes.  The exemption holds only under the condition that causes
# it: the occupancy query answers another number of blocks per CU for the case than for the production layer, so `wave_slabs` differs
# (the host build, where the answer follows the LDS size: 2 against 5).  Where both get the same answer (the MI355X: 2, by registers)
# the tuple must be covered like any other, so there nothing is left out.
_F16S2 = (16, 3, 3, 3, 2, 0, 0)
WGRAD_NOT_COVERED = (((_F16S2, 1, 4, 0, 0, 2, 2), 'conv4 of 82x98x70: production tile 693 MB at 4,097 items'),
                     ((_F16S2, 0, 4, 0, 0, 2, 2), 'convt2 of 82x98x70: production tile 693 MB at 4,097 items'))


def check_wgrad_coverage():
    """the assertions of test_wgrad_case_matrix_coverage (shared by the host-build and the GPU suite)"""
    cov = wgrad_coverage()
    left = {t for t, _ in WGRAD_NOT_COVERED}
    assert len(WGRAD_NOT_COVERED) <= 2
    missed = []
    for img, tuples in cov['production'].items():
        for t, layers in tuples.items():
            print('%s %r: %s <- %s' % ('x'.join(map(str, img)), t, ', '.join(layers), ', '.join(cov['cases'].get(t, [])) or 'NOT COVERED'))
    for img, tuples in cov['production'].items():
        for t, layers in tuples.items():
            case_bpc = cov['loop_case_bpc'].get(t[:7], set())
            if img == (82, 98, 70) and t[:7] in left and t not in cov['cases'] and case_bpc and case_bpc.isdisjoint(cov['production_bpc'][t]):
                missed.append(t)
                continue
            assert t in cov['cases'], 'no listed case runs %r (%s: %s)' % (t, 'x'.join(map(str, img)), ', '.join(layers))
    assert len(set(missed)) <= 2, missed
    cov['left_out'] = sorted(set(missed))
    print('left out: %r' % (cov['left_out'],))
    # every instance and slot scheme the planner can select is run by a listed case
    selectable = wgrad_selectable()
    not_run = {t: ex for t, ex in selectable.items() if t not in cov['instances']}
    assert not not_run, 'selectable, but run by no listed case: %r' % (not_run,)
    cov['selectable'] = len(selectable)
    assert cov['accumulate'] == {0, 1} and cov['wave_slabs'] == {0, 1} and cov['nbuf'] == {'CA', 2, 1}, cov
    assert cov['PAD'] == {0, 1} and cov['DSH'] == {0, 1}
    assert cov['partial_d'] and cov['partial_h'], (cov['partial_d'], cov['partial_h'])
    assert len(cov['loops']) + len(cov['loops_grouped']) >= 6 and len(cov['loops_grouped']) >= 2
    return cov


def run_adam_case(dev, dtype, n=5000, steps=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g, dtype=dtype)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    p = p0.to(dev).clone(); m = torch.zeros_like(p); v = torch.zeros_like(p)
    for t in range(1, steps + 1):
        gr = torch.randn(n, generator=g, dtype=dtype)
        ref.grad = gr.clone(); opt.step()
        if t == 1:
            sc = torch.zeros(3, dtype=torch.float64, device=dev)
        ops.adam_advance_(sc, 1e-3, 0.9, 0.999)                   # device-side step count + bias-correction scalars
        want_sc = [1e-3 / (1 - 0.9 ** t), np.sqrt(1 - 0.999 ** t), float(t)]
        np.testing.assert_allclose(sc.cpu().numpy(), want_sc, rtol=1e-14)
        ops.adam_step_(p, gr.to(dev), m, v, 0.9, 0.999, 1e-8, sc)
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    np.testing.assert_allclose(p.cpu().numpy(), ref.detach().numpy(), rtol=tol, atol=tol)


def run_cholesky_case(dev, batch=3, n=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(batch, n, n, generator=g, dtype=torch.float64)
    a = r @ r.transpose(1, 2) + 0.5 * torch.eye(n, dtype=torch.float64)
    a_ref = a.clone().requires_grad_(True)
    l_ref = torch.linalg.cholesky(a_ref)
    w = torch.randn(batch, n, n, generator=g, dtype=torch.float64)
    (ga_ref,) = torch.autograd.grad((l_ref * w).sum(), a_ref)
    a_d = a.to(dev).clone().requires_grad_(True)
    l = ops.cholesky(a_d)
    np.testing.assert_allclose(l.detach().cpu().numpy(), l_ref.detach().numpy(), rtol=1e-10, atol=1e-10)
    (ga,) = torch.autograd.grad((l * w.to(dev)).sum(), a_d)
    np.testing.assert_allclose(ga.cpu().numpy(), ga_ref.numpy(), rtol=1e-8, atol=1e-8)


def run_gain_case(dev, B=12, n=6, jitter=0.0, seed=0, kinds=('lin_hrf', 'gp', 'gp', 'gp_hrf', 'lin')):
    """vg_gp_gain_fwd / _bwd (one workgroup per covariate: GP posterior, gain covariance, B x B Cholesky, gain sample, HRF,
    both KLs) against the float64 oracle restatement of vae_reg_GP.py:345-378 / gp.py:41-110 with autograd for the gradients.
    Inputs, reference and bands are those of tests/gain_cases.py (the builder and runner every gain test shares).
    d log_ls / d logkvar are cancelling sums; these older cases keep the slack that was given them when the reference held the
    inducing-to-query distances in float64 (grow = B / 32 on the absolute part of their band); the cases of gain_cases.py run without."""
    import gain_cases
    return gain_cases.run_case(dev, B, n, jitter, seed=seed, kinds=kinds, grow=max(1.0, B / 32.0))


def _posterior_unit_variance(xu, k_var, ls, qu_m, qu_S, xq, jitter):
    """oracle.gp_posterior (gp.py:67-110) with A = Knu^T Ku^-1 formed from UNIT-variance kernels (k_var cancels in A)."""
    import vaegam_oracle as O
    n = xu.shape[0]
    step = (xu[1] - xu[0]).double()
    knu_d = (xu[0].double() - xq).unsqueeze(0) + torch.arange(n, dtype=torch.float64).unsqueeze(1) * step
    one = torch.ones((), dtype=torch.float64)
    knu1 = O.gp_kernel(knu_d, one, ls)
    knn1 = O.gp_kernel(xq.unsqueeze(0) - xq.unsqueeze(1), one, ls)
    idx = torch.arange(n, dtype=torch.float64)
    ku1 = O.gp_kernel((idx.unsqueeze(0) - idx.unsqueeze(1)).abs(), one, ls, step) + jitter * torch.eye(n, dtype=torch.float64)
    A = knu1.T @ torch.inverse(ku1)
    return A @ torch.squeeze(qu_m), k_var * knn1 + A @ (qu_S - k_var * ku1) @ A.T


def _hrf_taps():
    from vae_gam_amd import utils
    return torch.tensor(utils.hrf(np.arange(0, 20, 1.4))).float().double()


def _hrf64(tv):
    """causal HRF along the batch index with the fp32-rounded taps, float64 accumulate (vae_reg_GP.py:283-305)"""
    hk = _hrf_taps()
    B = tv.shape[0]
    T = torch.zeros(B, B, dtype=torch.float64)
    for i in range(B):
        m = min(hk.shape[0], B - i)
        T[i, i:i + m] = hk[:m]
    return tv @ T
