"""Shared bodies of the rectified hand-off tests: producers that store max(y, 0) (`relu_out`), consumers that are told so
(`rectified_in`) and the toy model with the hand-off on and off.  Run on CPU
tensors through the host build of the kernels (tests/test_rectified_emu.py) and on the GPU through libvaegam_hip.so
(tests/test_rectified_gpu.py).

Every case has N = 4 samples in two batch-norm groups of per_group = 2: two groups with different scale and shift, and a group
boundary inside every launch."""
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops
from vae_gam_amd.ops import ConvSpec
import kernel_cases as K
import toy_case as T

PG, GROUPS = 2, 2
N = PG * GROUPS
_K3 = (3, 3, 3)


def _affine(g, ci):
    return 1 + 0.3 * torch.randn(GROUPS * ci, generator=g), 0.2 * torch.randn(GROUPS * ci, generator=g)


def _wshape(spec):
    return ((spec.co, spec.ci) if spec.kind == 'conv' else (spec.ci, spec.co)) + tuple(spec.k)


# ------------------------------------------------------------------------------------------------ a. producers
# (name, spec, input size, k-steps per class the plan must have)
MM_PRODUCERS = [
    ('k7', ConvSpec('convt', 16, 16, _K3, 1), (3, 4, 5), [7]),
    ('k9', ConvSpec('convt', 16, 8, _K3, 1), (3, 4, 6), [9]),
    ('tconv533', ConvSpec('convt', 8, 8, (5, 3, 3), 2), (3, 4, 5), [3, 2, 2, 1]),
    ('tconv444', ConvSpec('convt', 8, 8, (4, 4, 4), 2), (3, 3, 4), [2, 2, 2, 2]),
]


def run_mm_producer_case(dev, name):
    """vg_conv_mm (conv_mm_k::store_class): relu_out = 1 stores clamp_min(the relu_out = 0 output, 0) bit for bit, and the
    statistics partials of the next batch norm (stats_relu = 1) do not change by a bit."""
    _, spec, isz, ks = next(c for c in MM_PRODUCERS if c[0] == name)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((N, spec.ci) + isz, generator=g).to(dev)
    w = (0.2 * torch.randn(_wshape(spec), generator=g)).to(dev)
    b = (0.1 * torch.randn(spec.co, generator=g)).to(dev)
    sc, sh = [t.to(dev) for t in _affine(g, spec.ci)]
    plan = ops.mm_plan(spec, 'fwd', isz)
    assert plan is not None and list(plan.ks)[:plan.nq] == ks, (name, plan and plan.ks)
    aimg = plan.gather(w)
    y0, part0 = ops.conv_mm(x, plan, aimg, b, True, sc, sh, PG, None, PG, relu_out=False)
    y1, part1 = ops.conv_mm(x, plan, aimg, b, True, sc, sh, PG, None, PG, relu_out=True)
    assert bool((y0 < 0).any()) and bool((y0 > 0).any())
    assert torch.equal(y1, y0.clamp_min(0)), name
    assert torch.equal(part1, part0), name + ': statistics partials'
    y2 = ops.conv_mm(x, plan, aimg, b, True, sc, sh, PG, None, None, relu_out=True)       # without the statistics epilogue
    assert torch.equal(y2, y1), name
    if plan.nq == 1:
        # a masked (data-gradient) store is not a forward store: the field is ignored
        m = torch.randn(y0.shape, generator=g).to(dev)
        d0 = ops.conv_mm(x, plan, aimg, None, False, None, None, 1, m, None, relu_out=False)
        d1 = ops.conv_mm(x, plan, aimg, None, False, None, None, 1, m, None, relu_out=True)
        assert bool((d0 < 0).any()) and torch.equal(d1, d0), name + ': masked store'


def run_tconv_producer_case(dev):
    """tconv3d_s2_k on the convt2 spec of kernel_cases.LAYERS, through vg_tconv3d_s2_stats and the plain entry, with a prologue
    (ReLU) and on the prologue-free instance (relu_in = 0, no affine)."""
    _, spec, isz = next(c for c in K.LAYERS if c[0] == 'convt2')
    g = torch.Generator().manual_seed(12)
    x = torch.randn((N, spec.ci) + tuple(isz), generator=g).to(dev)
    w = (0.2 * torch.randn(_wshape(spec), generator=g)).to(dev)
    b = (0.1 * torch.randn(spec.co, generator=g)).to(dev)
    wf = ops.pack_weight(w, spec, 'fwd')
    for relu_in in (True, False):
        y0, part0 = ops.conv_forward(x, wf, b, spec, relu_in, None, None, PG, next_bn=PG, relu_out=False)
        y1, part1 = ops.conv_forward(x, wf, b, spec, relu_in, None, None, PG, next_bn=PG, relu_out=True)
        assert bool((y0 < 0).any())
        assert torch.equal(y1, y0.clamp_min(0)), relu_in
        assert torch.equal(part1, part0), relu_in
        p0 = ops.conv_forward(x, wf, b, spec, relu_in, None, None, PG, relu_out=False)
        p1 = ops.conv_forward(x, wf, b, spec, relu_in, None, None, PG, relu_out=True)
        assert torch.equal(p0, y0) and torch.equal(p1, y1), relu_in
    # the prologue-free instance reads what the prologue instance computes from a rectified input
    xr = x.clamp_min(0)
    assert torch.equal(ops.conv_forward(xr, wf, b, spec, False, None, None, PG), ops.conv_forward(x, wf, b, spec, True, None, None, PG))


def run_corr_producer_case(dev, which):
    """corr3d_plane_k (8 -> 1 channels, 3x3x3, the last decoder stage's instance) and corr3d_direct_k (8 -> 8, the small-launch
    instance), both with ReLU + per-group affine on the input."""
    spec = ConvSpec('convt', 8, 1, _K3, 1) if which == 'plane' else ConvSpec('convt', 8, 8, _K3, 1)
    isz = (5, 6, 7)
    g = torch.Generator().manual_seed(13)
    x = torch.randn((N, spec.ci) + isz, generator=g).to(dev)
    w = (0.2 * torch.randn(_wshape(spec), generator=g)).to(dev)
    b = (0.1 * torch.randn(spec.co, generator=g)).to(dev)
    sc, sh = [t.to(dev) for t in _affine(g, spec.ci)]
    wf = ops.pack_weight(w, spec, 'fwd')
    y0 = ops.conv_forward(x, wf, b, spec, True, sc, sh, PG, relu_out=False)
    y1 = ops.conv_forward(x, wf, b, spec, True, sc, sh, PG, relu_out=True)
    assert bool((y0 < 0).any()) and bool((y0 > 0).any())
    assert torch.equal(y1, y0.clamp_min(0)), which
    # data gradient with the producer's ReLU mask: the field is ignored
    m = torch.randn(y0.shape, generator=g).to(dev)
    d = ops._conv_desc(N, spec.ci, spec.co, isz, tuple(y0.shape[2:]), spec.k, 1, (2, 2, 2), False, 1, False)
    outs = []
    for ro in (0, 1):
        d.relu_out = ro
        o = torch.empty_like(y0)
        ops._call(x, 'vg_corr3d', ops.ctypes.byref(d), ops._p(x), ops._p(wf), None, None, None, ops._p(m), ops._p(o))
        outs.append(o)
    assert bool((outs[0] < 0).any()) and torch.equal(outs[0], outs[1]), which + ': masked store'


# ------------------------------------------------------------------------------------------------ b. consumers
CONSUMERS = {
    # name: (spec, input size, batch norm, next_bn, use the matrix-core engine where it wins)
    'convt2_tconv_nopro': (ConvSpec('convt', 16, 16, _K3, 2, (1, 0, 1), (1, 0, 1), name='convt2'), (4, 5, 4), False, True, False),
    'convt2_mm': (ConvSpec('convt', 16, 16, _K3, 2, (1, 0, 1), (1, 0, 1), name='convt2'), (4, 5, 4), False, True, True),
    'convt4_mm_nopro': (ConvSpec('convt', 8, 8, (5, 3, 3), 2, name='convt4'), (4, 5, 4), False, True, True),
    'convt3_bn': (ConvSpec('convt', 16, 8, _K3, 1, name='convt3'), (4, 6, 5), True, False, True),
    'convt5_bn': (ConvSpec('convt', 8, 1, _K3, 1, name='convt5'), (5, 7, 6), True, False, True),
}


def _layer_run(dev, spec, p, vals, gy, pre, with_bn, next_bn, **kw):
    """One bn_conv_act forward + backward on fresh Parameters whose .grad buffers hold `pre` -> (y, part, dp, [grads])."""
    pd = p.to(dev).clone().requires_grad_(True)
    params = [torch.nn.Parameter(v.to(dev).clone()) for v in vals]
    for t, r in zip(params, pre):
        t.grad = r.to(dev).clone()
    w, b = params[0], params[1]
    gamma, beta = (params[2], params[3]) if with_bn else (None, None)
    out = ops.bn_conv_act(pd, w, b, gamma, beta, spec, True, PG, next_bn=PG if next_bn else None, **kw)
    y, part = out if next_bn else (out, None)
    got = torch.autograd.grad(y, [pd] + params, gy.to(dev), allow_unused=True)
    if pd.is_cuda:
        ops.join_side_stream(pd.device)
    assert all(t is None for t in got[1:]), 'autograd was handed a tensor although .grad is bound'
    return y.detach(), part, got[0], [t.grad.clone() for t in params]


def run_consumer_case(dev, name, monkeypatch):
    """bn_conv_act(p, relu_in=True) against bn_conv_act(relu(p), relu_in=True, rectified_in=True): the output, the statistics partials
    and EVERY gradient (dp, dw, db, dgamma, dbeta; bound .grad buffers prefilled with the same random values) bit for bit."""
    spec, isz, with_bn, next_bn, use_mm = CONSUMERS[name]
    if not use_mm:
        monkeypatch.setattr(ops, 'USE_MM', 0)             # the register-tiled kernels (what the 41x49x35 network runs convt2's forward on)
    g = torch.Generator().manual_seed(21)
    p = torch.randn((N, spec.ci) + isz, generator=g)
    vals = [0.2 * torch.randn(_wshape(spec), generator=g), 0.1 * torch.randn(spec.co, generator=g)]
    if with_bn:
        vals += [1 + 0.3 * torch.randn(spec.ci, generator=g), 0.2 * torch.randn(spec.ci, generator=g)]
    pre = [2 * torch.randn(v.shape, generator=g) for v in vals]
    gy = torch.randn((N, spec.co) + spec.out_size(isz), generator=g)
    raw = _layer_run(dev, spec, p, vals, gy, pre, with_bn, next_bn)
    rect = _layer_run(dev, spec, p.clamp_min(0), vals, gy, pre, with_bn, next_bn, rectified_in=True)
    assert torch.equal(raw[0], rect[0]), name + ' y'
    if next_bn:
        assert torch.equal(raw[1], rect[1]), name + ' statistics partials'
    assert torch.equal(raw[2], rect[2]), name + ' dp'
    for a, b_, nm in zip(raw[3], rect[3], ('dw', 'db', 'dgamma', 'dbeta')):
        assert torch.equal(a, b_), '%s %s' % (name, nm)
    assert not torch.equal(raw[3][0], pre[0].to(dev))     # (the gradients were added)


# ------------------------------------------------------------------------------------------------ c. model
B_TOY, C_TOY = 4, 3


def toy_model(dev, **attrs):
    x, cov, xu, glm = T.make_inputs(B_TOY, C_TOY, seed=5)
    torch.manual_seed(1)
    model = T.VAE(num_covariates=C_TOY, glm_maps=glm, xu_ranges=xu, device_name=dev, img_shape=T.IMG)
    for k, v in attrs.items():
        assert hasattr(model, k), k
        setattr(model, k, v)
    return model, x.to(dev), cov.to(dev)


def _toy_step(dev, **attrs):
    import bridge
    import vaegam_oracle as O
    model, x, cov = toy_model(dev, **attrs)
    noise = O.draw_noise(B_TOY, bridge.oracle_config(model), torch.Generator().manual_seed(9))
    noise = bridge.noise_to(noise, dev) if dev != 'cpu' else noise
    loss = model.train_step(torch.zeros(B_TOY, dtype=torch.int64, device=dev), cov, x, noise=noise)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach().clone(), grads, model


def run_model_bit_equal_case(dev):
    """One train step of the toy model with the hand-off on == the step with everything stored pre-activation: the loss and every
    .grad bit for bit."""
    l0, g0, _ = _toy_step(dev, rectified_handoff=False)
    l1, g1, m1 = _toy_step(dev, rectified_handoff=True)
    assert m1.rectified_handoff is True
    assert torch.equal(l0, l1), (l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 40
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
