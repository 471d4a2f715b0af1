"""Shared bodies of the model-path tests: the product model's own encode path (VAE._encode_heads) and decode path
(VAE._decode_logits) -- the autograd nodes BnConvAct / LinearAct / HeadsAct, the hand-offs next_bn / pre_stats, producer_bias /
bias_grad_by_consumer, relu_out / rectified_in, PackedWeights and the writes straight into the .grad views of FusedAdam's flat
buffer -- against a plain torch float64 restatement on the CPU built from model.named_parameters() and model.geom:
kernel_cases.ref_layer for the ten conv layers (batch-norm statistics per group of per_group samples), F.linear / relu for fc1, fc2,
fc31-33, fc41-43 and fc5-8.  Run on CPU tensors through the host build of the kernels (test_model_paths_emu.py) and on the GPU
through libvaegam_hip.so (test_model_paths_gpu.py).

Before a path runs: optimizer.zero_grad(), _packed.refresh() (as encode / decode do) and every batch-norm weight and bias moved away
from 1 / 0.  The encode path is driven backwards by three fixed random cotangents (mu, w, a), the decode path by one, with z a random
leaf of groups * per_group rows.  Compared: every forward output, the gradient of every parameter the path touches, read from the
parameter's bound .grad (32 for the encode path, 24 for the decode path), and dz; every parameter the path does not touch must be
left with a gradient of exactly zero.  For an embedded native grid the reference zero-pads x at the high end of each axis.

Bound, per tensor, the rule of kernel_cases.run_wgrad_case:  tol = max(4 * d32, eps32 * sqrt(K) * max|want|), err = max |got - want|,
d32 = the distance of the SAME torch code evaluated in fp32 from its float64 value, K = the number of addends that enter one entry:
  conv weight, conv bias of a layer      K = samples x output positions of that layer (samples = B in the encoder, groups * per_group
                                             in the decoder)
  batch-norm weight / bias               K = samples x positions of the tensor it normalises (= the input of the layer behind it)
  FC weight, FC bias                     K = rows (B in the encoder, groups * per_group in the decoder)
  mu, w, a                               K = 50 (fc41-43's contraction);   dz: K = 50 (fc5's 50 outputs)
  logits                                 K = 8 x 27 (convt5's channels x taps)
The floor is only there for tensors where torch's fp32 lands on the float64 value (the plain sums and the input_is_data
identities: bn1.weight sits at 24 x d32 on the host build with an error of 3e-7, under the floor of 1.1e-6).

ReLU branches (branch_masks).  A gradient is discontinuous in a pre-activation at zero, so a bound in d32 means something only where the
product and the reference stand on the same side of every ReLU.  Of the 4 to 6 * 10^5 values a ReLU is applied to in one path of
cases 1-3, 10 to 60 lie within 4 * d32 of zero (d32 of their own tensor: the bound the product's forward is held to); at those either
one-sided derivative is a correct fp32 gradient, and taking the other one moves every gradient upstream by a whole addend (5 to 15 % of
conv4's and conv3's gradients in case 1, where conv4's output holds a 3.9e-8), not by a rounding.  On those entries, and on no
others, the reference (float64 and fp32 alike, so that d32 stays a rounding distance) takes the branch the product took, read from
the layer outputs the product stores (the sign survives the rectified hand-off); values are never touched.  The count per tensor and
how often the product stood on the other side are printed: once on the host build (that conv4 entry), twice on the MI355X (it and
one entry of convt4's output in case 1), never in case 6.  The hidden FC activations cannot be seen from outside the nodes; they hold
at most 1,800 values a path, and a case must keep them out of the band (asserted: draw other inputs if not).

Cases (CASES; at least 3 volumes per batch-norm group everywhere, see TWO_VALUE_CASE):
  1  22x22x22, B 3, 3 decoder groups          family rule, convt4 4x4x4
  2  21x21x21, B 4, 2 decoder groups          toy network, convt4 3x3x3
  3  22x26x22, B 3, 2 decoder groups          non-cubic, decoder seed 1x2x1
  4  native 19x21x20 in 22x22x22, B 3         encode path only: vg_embed_volumes in front of conv1
  5  as 1 with rectified_handoff off          same bounds; outputs and gradients bit-equal to case 1
  6  41x49x35, B 3, 2 decoder groups          GPU only: the reference geometry (convt2 with padding / output padding, convt4 5x3x3);
                                              0.5 s on the MI355X, reference included

Worst err / d32 per tensor class over the cases (host build: cases 1-5; MI355X: cases 1-6; d32 is taken on the CPU of the machine
that runs the test, so the two columns do not share their denominators):
  class                  host build   MI355X
  outputs (mu, w, a)        3.03       2.37
  outputs (logits)          1.91       1.56
  conv weight               2.09       1.94
  conv bias                 1.75       1.53
  batch-norm weight/bias    2.13       2.83     (without bn1, the input_is_data identity: 23.90 / 1.51, under the floor on the host build)
  FC weight                 2.24       2.24
  FC bias                   2.00       2.10
  dz                        2.23       2.47
Relative errors (max error over max |want|) are 3e-7 to 6e-6.

TWO_VALUE_CASE (case 2 with B = 2, a documented property, not a parity case): on a grid whose decoder seed is 1x1x1, two volumes per
group leave bnt1 two values per (group, channel).  Where the two are nearly equal, |mean| * rstd reaches 1 / sqrt(eps) = 316 times
|mean| and the prologue's x * scale + shift cancels two numbers of that size; torch's fp32 subtracts the mean first, which
is exact for two values, so the output can sit tens of d32 from float64 (from convt1 through convt5) although it is well inside
run_layer_case's 2e-4.  How far depends on the draw: 2.1 to 3.1 x d32 per layer on the host build, 0.8 to 1.4 on the MI355X for this z.

Launch coverage (recorded through lib.call per case).  COVERAGE, asserted over cases 1-5 together: vg_conv_mm in a forward and in a
backward, vg_corr3d, a vg_tconv3d_s2* entry, vg_bn_stats_from_parts in convt3's and in convt5's forward (pre_stats taken), vg_wgrad3d,
vg_wgrad3d_grouped, vg_bn_bwd_apply_tconv1 (the one-pass form: the grouped weight gradient replaces vg_bn_bwd_reduce_tconv1
wherever it has an instance, and it has one at every case), vg_bn_bwd_reduce / _apply, vg_data_bn_grads, vg_fc_gemm_jobs and
vg_embed_volumes (case 4).  Not reached by cases 1-5: vg_tconv3d_s2_stats_of (and with it the two-halves vg_conv_mm launches of
convt2's forward and conv4's data gradient) -- ops._halves_win declines a launch whose block holds a whole sample's half, and on every
family grid under 30^3 convt2's input is at most 5x5x5; the planner first splits a sample at 41x49x35 (8x10x7).  COVERAGE_CASE6 asserts
them on case 6, on the GPU."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
import grid_cases as GC
import kernel_cases as K

EPS32 = float(np.finfo(np.float32).eps)

# id -> (native volume shape, B, decoder groups or None = encode path only, rectified_handoff)
CASES = {
    '1-22x22x22-B3-G3': ((22, 22, 22), 3, 3, True),
    '2-21x21x21-B4-G2': ((21, 21, 21), 4, 2, True),
    '3-22x26x22-B3-G2': ((22, 26, 22), 3, 2, True),
    '4-19x21x20-in-22x22x22-B3': ((19, 21, 20), 3, None, True),
    '5-22x22x22-B3-G3-unrectified': ((22, 22, 22), 3, 3, False),
    '6-41x49x35-B3-G2': ((41, 49, 35), 3, 2, True),
}
HOST_CASES = [c for c in CASES if not c.startswith('6-')]
GPU_ONLY = ['6-41x49x35-B3-G2']
BIT_EQUAL = ('5-22x22x22-B3-G3-unrectified', '1-22x22x22-B3-G3')
TWO_VALUE_CASE = ((21, 21, 21), 2, 2)           # case 2 again with 2 volumes per group

ENC_BN = {'conv1': 'bn1', 'conv3': 'bn3', 'conv5': 'bn5'}
DEC_BN = {'convt1': 'bnt1', 'convt3': 'bnt3', 'convt5': 'bnt5'}
NUM_COV = 2                                     # z_dim = 32 + 3; the decoder groups of a case are independent of it

# what cases 1-5 together must launch: (description, predicate over the recorded (entry, label) pairs)
COVERAGE = [
    ('vg_conv_mm forward', lambda n, l: n == 'vg_conv_mm' and l.endswith('/fwd')),
    ('vg_conv_mm data gradient', lambda n, l: n == 'vg_conv_mm' and l.endswith('/bwd')),
    ('vg_corr3d', lambda n, l: n == 'vg_corr3d'),
    ('vg_tconv3d_s2*', lambda n, l: n.startswith('vg_tconv3d_s2') and n != 'vg_tconv3d_s2_stats_of'),
    ('vg_bn_stats_from_parts in convt3/fwd (pre_stats taken)', lambda n, l: n == 'vg_bn_stats_from_parts' and l == 'convt3/fwd'),
    ('vg_bn_stats_from_parts in convt5/fwd (pre_stats taken)', lambda n, l: n == 'vg_bn_stats_from_parts' and l == 'convt5/fwd'),
    ('vg_wgrad3d',lambda n, l: n == 'vg_wgrad3d'),
    ('vg_wgrad3d_grouped', lambda n, l: n == 'vg_wgrad3d_grouped'),
    ('vg_bn_bwd_*_tconv1', lambda n, l: n.startswith('vg_bn_bwd_') and n.endswith('_tconv1')),
    ('vg_bn_bwd_reduce', lambda n, l: n == 'vg_bn_bwd_reduce'),
    ('vg_bn_bwd_apply', lambda n, l: n == 'vg_bn_bwd_apply'),
    ('vg_data_bn_grads', lambda n, l: n == 'vg_data_bn_grads'),
    ('vg_fc_gemm_jobs', lambda n, l: n == 'vg_fc_gemm_jobs'),
    ('vg_embed_volumes', lambda n, l: n == 'vg_embed_volumes'),
]
# ... and what case 6 adds: convt2's forward and conv4's data gradient as two channel halves on the matrix cores, with bnt3's
# statistics partials taken from the stored output.  No family grid under 30^3 reaches it: ops._halves_win declines a launch whose
# block holds a whole sample's half, and convt2's input is at most 5x5x5 there (the planner first splits a sample at 8x10x7)
COVERAGE_CASE6 = [
    ('vg_tconv3d_s2_stats_of', lambda n, l: n == 'vg_tconv3d_s2_stats_of'),
    ('vg_conv_mm in convt2/fwd', lambda n, l: n == 'vg_conv_mm' and l == 'convt2/fwd'),
    ('vg_conv_mm in conv4/bwd', lambda n, l: n == 'vg_conv_mm' and l == 'conv4/bwd'),
    # the consumer takes the partials (a convt3 that ignored pre_stats and ran vg_bn_stats itself would compute the same values)
    ('vg_bn_stats_from_parts in convt3/fwd', lambda n, l: n == 'vg_bn_stats_from_parts' and l == 'convt3/fwd'),
]


# ------------------------------------------------------------------------------------------------ reference
def _lin(P, name, t):
    return F.linear(t, P[name + '.weight'], P[name + '.bias'])


def _conv(P, h, sp, bn, relu_in, per_group):
    gamma, beta = (P[bn + '.weight'], P[bn + '.bias']) if bn else (None, None)
    return K.ref_layer(h, P[sp.name + '.weight'], P[sp.name + '.bias'], gamma, beta, sp, relu_in, per_group)


class Branches:
    """What the reference's ReLUs record and obey.  pre: name -> the tensor a ReLU was applied to (recorded when `record`).
    masks: name -> bool tensor; where given, the ReLU keeps its value max(t, 0) but takes the mask as its derivative."""
    def __init__(self, record=False, masks=None):
        self.pre = {} if record else None
        self.masks = masks or {}


def _relu(t, name, br):
    if br is not None and br.pre is not None:
        br.pre[name] = t.detach()
    m = None if br is None else br.masks.get(name)
    if m is None:
        return F.relu(t)
    return F.relu(t).detach() + (t - t.detach()) * m.reshape(t.shape).to(t.dtype)


def ref_encode(P, geom, x, br=None):
    """x (B, *native) -> (mu, w, a): the reference of VAE._encode_heads (one batch-norm group: the whole batch)"""
    B = x.shape[0]
    h = GC.pad_to(x, geom.native, geom.img).reshape(B, 1, *geom.img)
    for i, sp in enumerate(geom.enc):
        if i > 0:
            h = _relu(h, geom.enc[i - 1].name, br)
        h = _conv(P, h, sp, ENC_BN.get(sp.name), False, B)
    h = _relu(h, 'conv5', br).reshape(B, -1)
    h = _relu(_lin(P, 'fc2', _relu(_lin(P, 'fc1', h), 'fc1', br)), 'fc2', br)
    return tuple(_lin(P, 'fc4%d' % i, _relu(_lin(P, 'fc3%d' % i, h), 'fc3%d' % i, br)) for i in (1, 2, 3))


def ref_decode(P, geom, z, per_group, br=None, layers=None):
    """z (groups * per_group, z_dim) -> logits (N, V_grid): the reference of VAE._decode_logits; `layers` (a list) also gets every
    conv layer's output"""
    h = z
    for n in ('fc5', 'fc6', 'fc7'):
        h = _relu(_lin(P, n, h), n, br)
    h = _lin(P, 'fc8', h).reshape(-1, 2 * geom.nf, *geom.dec_seed)
    prev = 'fc8'
    for sp in geom.dec:
        h = _conv(P, _relu(h, prev, br), sp, DEC_BN.get(sp.name), False, per_group)
        prev = sp.name
        if layers is not None:
            layers.append(h)
    return (h.reshape(h.shape[0], -1),)


ENC_PARAMS = ['conv%d' % i for i in range(1, 6)] + ['bn1', 'bn3', 'bn5', 'fc1', 'fc2', 'fc31', 'fc32', 'fc33', 'fc41', 'fc42', 'fc43']
DEC_PARAMS = ['fc5', 'fc6', 'fc7', 'fc8'] + ['convt%d' % i for i in range(1, 6)] + ['bnt1', 'bnt3', 'bnt5']


def _names(layers):
    return [l + s for l in layers for s in ('.weight', '.bias')]


def _evaluate(fn, params, names, inputs, cots, dt, leaf=None, br=None):
    """fn(P, *inputs, br) in dtype dt -> (outputs, {name: gradient} of `names` [+ 'dz' of the leaf input]) for the cotangents"""
    P = {k: v.detach().cpu().to(dt) for k, v in params.items()}
    for n in names:
        P[n].requires_grad_(True)
    ins = [t.detach().cpu().to(dt) for t in inputs]
    wrt = [P[n] for n in names]
    if leaf is not None:
        ins[leaf].requires_grad_(True)
        wrt.append(ins[leaf])
    outs = fn(P, *ins, br)
    gr = torch.autograd.grad(outs, wrt, [c.to(dt) for c in cots])
    grads = {n: g.double() for n, g in zip(names, gr)}
    if leaf is not None:
        grads['dz'] = gr[-1].double()
    return [o.detach().double() for o in outs], grads


def _addends(geom, B, N):
    """name -> K (module docstring)"""
    esz, dsz = geom.enc_sizes(), geom.dec_sizes()
    Kd = {}
    for specs, sizes, n, bns in ((geom.enc, esz, B, ENC_BN), (geom.dec, dsz, N, DEC_BN)):
        if n is None:
            continue
        for i, sp in enumerate(specs):
            Kd[sp.name + '.weight'] = Kd[sp.name + '.bias'] = n * int(np.prod(sizes[i + 1]))
            if sp.name in bns:
                Kd[bns[sp.name] + '.weight'] = Kd[bns[sp.name] + '.bias'] = n * int(np.prod(sizes[i]))
    for l in ENC_PARAMS[8:]:
        Kd[l + '.weight'] = Kd[l + '.bias'] = B
    for l in DEC_PARAMS[:4]:
        Kd[l + '.weight'] = Kd[l + '.bias'] = N
    Kd.update(mu=50, w=50, a=50, dz=50, logits=geom.nf * 27)
    return Kd


def tensor_class(name):
    if name in ('mu', 'w', 'a'):
        return 'outputs (mu, w, a)'
    if name in ('logits', 'dz'):
        return 'outputs (logits)' if name == 'logits' else 'dz'
    kind = 'conv' if name.startswith('conv') else 'batch-norm' if name.startswith('bn') else 'FC'
    return 'batch-norm weight/bias' if kind == 'batch-norm' else '%s %s' % (kind, name.rsplit('.', 1)[1])


# ------------------------------------------------------------------------------------------------ the product's paths
@contextlib.contextmanager
def record_launches(names):
    """(C-ABI entry, ops label) of every launch that goes through lib.call, appended to `names`"""
    lib = _lib.get_lib()
    orig = lib.call
    lib.call = lambda name, *a: (names.append((name, ops._LABEL[0])), orig(name, *a))[1]
    try:
        yield names
    finally:
        del lib.call


@contextlib.contextmanager
def watch_layers(store):
    """store[layer] = the output of every ops.bn_conv_act call (by ConvSpec name), store['fc8'] = convt1's input, as CPU tensors"""
    orig = ops.bn_conv_act

    def spy(*a, **kw):
        y = orig(*a, **kw)
        store[a[5].name] = (y[0] if isinstance(y, tuple) else y).detach().cpu()
        if a[5].name == 'convt1':
            store['fc8'] = a[0].detach().cpu()
        return y
    ops.bn_conv_act = spy
    try:
        yield store
    finally:
        ops.bn_conv_act = orig


def _forward_pre(fn, params, inputs, dt):
    """name -> everything the reference applies a ReLU to, evaluated plainly in dtype dt (as float64 tensors)"""
    br = Branches(record=True)
    with torch.no_grad():
        fn({k: v.detach().cpu().to(dt) for k, v in params.items()}, *[t.detach().cpu().to(dt) for t in inputs], br)
    return {k: v.double() for k, v in br.pre.items()}


def branch_masks(what, pre64, pre32, seen):
    """The ReLU derivatives the reference takes.  A pre-activation p within 4 * d32 of zero (d32 = the fp32 distance of ITS tensor, the
    bound the product's forward is held to) has no branch an fp32 computation could be held to: either one-sided derivative is a
    correct gradient there, and the two differ by a whole addend, not by a rounding.  On those elements -- and on no others -- the
    reference takes the branch the product took (`seen`: the product's stored layer outputs, whose sign survives the rectified
    hand-off), in float64 and in fp32 alike, so that d32 stays a rounding distance.  The FC hidden layers are not visible from
    outside the nodes; they are small, and a case must keep them clear of the band (asserted)."""
    masks = {}
    for n, p in pre64.items():
        band = p.abs() <= 4 * float((pre32[n] - p).abs().max())
        if n not in seen:
            assert not bool(band.any()), '%s: the reference\'s %s has an entry within 4 d32 of zero: draw other inputs for this case' % (what, n)
            continue
        took = seen[n].reshape(p.shape) > 0
        masks[n] = torch.where(band, took, p > 0)
        if bool(band.any()):
            print('%s %s: %d of %d entries within 4 d32 of zero, the product took the other branch on %d'
                  % (what, n, int(band.sum()), p.numel(), int((band & (took != (p > 0))).sum())))
    return masks


def make_model(dev, img, B, rectified=True, seed=11):
    """The product model on `img` with every batch-norm weight and bias moved away from 1 / 0, and one minibatch for it"""
    x, _, xu, glm = GC.make_inputs(img, B, NUM_COV, seed)
    model = GC.make_model(dev, img, NUM_COV, xu, glm)
    model.rectified_handoff = bool(rectified)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for bn in ('bn1', 'bn3', 'bn5', 'bnt1', 'bnt3', 'bnt5'):
            m = getattr(model, bn)
            m.weight.add_((0.3 * torch.randn(m.weight.shape, generator=g)).to(dev))
            m.bias.add_((0.2 * torch.randn(m.bias.shape, generator=g)).to(dev))
    return model, x


def _run_path(model, dev, which, x, z, per_group, cots, touched):
    """One path of the product, forward and backward -> (outputs, {name: .grad} of every parameter [+ dz]), CPU float64"""
    if model._plan_sizes is not None and per_group not in model._plans_checked:
        model._check_layer_plans(per_group)              # a derived grid: the planners' word on this batch size, as forward_core asks
    model.optimizer.zero_grad()
    model._packed.refresh()
    zd = None
    seen = {}
    with watch_layers(seen):
        if which == 'encode':
            outs = model._encode_heads(x.to(dev))
        else:
            zd = z.to(dev).requires_grad_(True)
            outs = (model._decode_logits(zd, per_group),)
    torch.autograd.backward(list(outs), [c.to(dev) for c in cots])
    if outs[0].is_cuda:
        ops.join_side_stream(outs[0].device)
    params = dict(model.named_parameters())
    grads = {}
    for n, p in params.items():
        assert p.grad is not None, n
        grads[n] = p.grad.detach().cpu().double().clone()
    for n in grads:
        if n not in touched:
            assert not bool(grads[n].any()), '%s path wrote into the gradient of %s' % (which, n)
    if zd is not None:
        grads['dz'] = zd.grad.detach().cpu().double()
    return [o.detach().cpu().double() for o in outs], grads, seen


def _compare(what, out_names, names, got, want, w32, Kd):
    """-> rows (name, class, err, d32, tol, max|want|), printed; nothing is asserted here"""
    rows = []
    pairs = [(n, g, w, s) for n, g, w, s in zip(out_names, got[0], want[0], w32[0])]
    pairs += [(n, got[1][n], want[1][n], w32[1][n]) for n in names]
    for n, g, w, s in pairs:
        assert g.shape == w.shape, (what, n, g.shape, w.shape)
        err = float((g - w).abs().max()); d32 = float((s - w).abs().max()); wmax = float(w.abs().max())
        tol = max(4 * d32, EPS32 * Kd[n] ** 0.5 * wmax)
        rows.append((n, tensor_class(n), err, d32, tol, wmax))
        print('%s %-14s K %7d  max|want| %.3g  err %.3g  d32 %.3g  err/d32 %.2f  tol %.3g%s'
              % (what, n, Kd[n], wmax, err, d32, err / max(d32, 1e-300), tol, '' if err <= tol and np.isfinite(err) else '   <-- OVER'))
    return rows


_RECORDS = {}


def run_case(dev, cid):
    """One case, run once per device and kept: -> dict(rows, outs, grads, launches, failures).  `failures` lists every tensor beyond
    its bound; check_case asserts that it is empty."""
    key = (dev, cid)
    if key in _RECORDS:
        return _RECORDS[key]
    img, B, groups, rectified = CASES[cid]
    model, x = make_model(dev, img, B, rectified)
    geom = model.geom
    g = torch.Generator().manual_seed(101)
    L = model.num_latents
    N = None if groups is None else groups * B
    Kd = _addends(geom, B, N)
    params = {k: v.detach().cpu().clone() for k, v in model.named_parameters()}
    launches, rows, outs, grads = [], [], {}, {}
    paths = [('encode', _names(ENC_PARAMS), (x,), [torch.randn(B, L, generator=g) for _ in range(3)], None,
              lambda P, xx, br=None: ref_encode(P, geom, xx, br), ('mu', 'w', 'a'))]
    if groups is not None:
        z = torch.randn(N, model.z_dim, generator=g)
        paths.append(('decode', _names(DEC_PARAMS), (z,), [torch.randn(N, model.grid_dim, generator=g)], 0,
                      lambda P, zz, br=None: ref_decode(P, geom, zz, B, br), ('logits',)))
    for which, names, inputs, cots, leaf, fn, out_names in paths:
        with record_launches(launches):
            got = _run_path(model, dev, which, x, inputs[0], B, cots, set(names))
        what = '%s %s' % (cid, which)
        br = Branches(masks=branch_masks(what, _forward_pre(fn, params, inputs, torch.float64), _forward_pre(fn, params, inputs, torch.float32),
                                         got[2]))
        want = _evaluate(fn, params, names, inputs, cots, torch.float64, leaf, br)
        w32 = _evaluate(fn, params, names, inputs, cots, torch.float32, leaf, br)
        gnames = names + (['dz'] if leaf is not None else [])
        rows += _compare(what, out_names, gnames, got, want, w32, Kd)
        outs.update(dict(zip(out_names, got[0])))
        grads.update({n: got[1][n] for n in gnames})
    failures = [(n, err, tol) for n, _, err, _, tol, _ in rows if not (np.isfinite(err) and err <= tol)]
    rec = dict(rows=rows, outs=outs, grads=grads, launches=launches, failures=failures)
    _RECORDS[key] = rec
    worst = {}
    for n, cls, err, d32, _, _ in rows:
        worst[cls] = max(worst.get(cls, 0.0), err / max(d32, 1e-300))
    print('%s worst err/d32 per class: %s' % (cid, ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    return rec


def check_case(dev, cid):
    rec = run_case(dev, cid)
    assert not rec['failures'], '%s: beyond max(4 d32, eps32 sqrt(K) max|want|): %s' % (
        cid, ', '.join('%s err %.3g > tol %.3g' % f for f in rec['failures']))
    return rec


def check_bit_equal(dev):
    """rectified_handoff off (case 5) computes, bit for bit, what it computes on (case 1): every output and every gradient"""
    a, b = run_case(dev, BIT_EQUAL[0]), run_case(dev, BIT_EQUAL[1])
    for kind in ('outs', 'grads'):
        assert a[kind].keys() == b[kind].keys()
        for n in a[kind]:
            assert torch.equal(a[kind][n], b[kind][n]), '%s differs between rectified_handoff on and off' % n


def check_coverage(dev, cids=HOST_CASES, wanted=COVERAGE):
    seen = [p for c in cids for p in run_case(dev, c)['launches']]
    missing = [what for what, pred in wanted if not any(pred(n, l) for n, l in seen)]
    print('entries launched by %s: %s' % (', '.join(cids), ' '.join(sorted({n for n, _ in seen}))))
    assert not missing, 'never launched by cases %s: %s' % (', '.join(cids), ', '.join(missing))


def run_two_value_property(dev):
    """Case 2 with B = 2: bnt1 normalises TWO values per (group, channel).  Asserted: the logits are finite and within
    run_layer_case's 2e-4 of float64.  Printed: err / d32 of every decoder layer's output as its consumer reads it (rectified for
    convt1-4).  -> [(layer, err, d32)]"""
    img, B, groups = TWO_VALUE_CASE
    model, _ = make_model(dev, img, B)
    geom = model.geom
    N = groups * B
    z = torch.randn(N, model.z_dim, generator=torch.Generator().manual_seed(101))
    params = {k: v.detach().cpu().clone() for k, v in model.named_parameters()}
    ref = {}
    for dt in (torch.float64, torch.float32):
        P = {k: v.to(dt) for k, v in params.items()}
        ref[dt] = []
        with torch.no_grad():
            ref_decode(P, geom, z.to(dt), B, layers=ref[dt])
    got = []
    orig = ops.bn_conv_act

    def spy(*a, **kw):
        y = orig(*a, **kw)
        got.append((y[0] if isinstance(y, tuple) else y).detach().cpu().double())
        return y
    model.optimizer.zero_grad()
    model._packed.refresh()
    ops.bn_conv_act = spy
    try:
        with torch.no_grad():
            logits = model._decode_logits(z.to(dev), B)
    finally:
        ops.bn_conv_act = orig
    assert len(got) == 5
    rows = []
    for i, sp in enumerate(geom.dec):
        f = (lambda t: t) if i == 4 else torch.relu
        w = f(ref[torch.float64][i]); err = float((f(got[i]) - w).abs().max()); d32 = float((f(ref[torch.float32][i]).double() - w).abs().max())
        print('two values per group: %s err %.3g d32 %.3g err/d32 %.1f' % (sp.name, err, d32, err / max(d32, 1e-300)))
        rows.append((sp.name, err, d32))
    lg = logits.detach().cpu().double()
    assert bool(torch.isfinite(lg).all())
    np.testing.assert_allclose(lg.numpy(), ref[torch.float64][4].reshape(N, -1).numpy(), rtol=2e-4, atol=2e-4)
    return rows
