"""The epilogue of conv_mm_k (vg_conv_mm.hip: store_class) against float64, one launch per case at a few-sample shape.

The epilogue is compiled once per combination of what a launch fixes -- rectified storage (`relu_out`), statistics on / off, statistics
of max(v, 0) or of v (`stats_relu`) -- and picked with one wave-uniform branch; it stores through a scalar base per matrix row plus a
32-bit lane offset, keeps the statistics in register pairs, and leaves the accumulators zero for the next class.  The cases here drive
every instantiation at the smallest shapes where it can go wrong:

  flags     (relu_out, statistics, stats_relu) in {0, 1}^3 on the 4-class convt4 plan at input 3x4x5 and on convt3 (one class, 8 output
            channels) at 4x5x6.  ops.conv_mm only ever asks for the diagonal (statistics => stats_relu), so these launches go to
            vg_conv_mm directly (run_epilogue_case);
  CO = 16   convt1 at 3x4x5 (tests/kernel_cases.py:run_conv_mm_case);
  partial   every shape here has an output width that is no multiple of 16, a last tile that holds fewer than 16 positions and waves
            that own fewer tiles than the plan's tiles per wave (conv2's data gradient at 7x9x7: 5 tiles on 8 waves, three waves
            own none); y sits between two guard bands of a sentinel that must survive, and no element of y may keep the sentinel;
  masked    data gradients with one class (convt3: the mask is prefetched into registers) and four (conv2: fetched in the epilogue),
            mask source ~ N(0, 1), i.e. about half of the entries <= 0; `relu_out` set on one of them: masked stores ignore it;
  run       13 groups x 8 samples on convt4 at 3x7x4 with 20 blocks per sample: N * bps = 2080 > 2048 (the `loop` sizing rule of
            run_conv_mm_case), so a block visits several samples and flushes the statistics of more than one run; stored rectified,
            which is the combination the train step runs.

Tolerances.  y: run_conv_mm_case's own rule, tol = max(4 * d32, eps32 * sqrt(K) * max|want|), d32 = the distance of torch's fp32 CPU
convolution to the float64 one.  Statistics: the partials are [sum, sum of squares] of h = max(v, 0) or v per (group, channel, chunk)
as doubles; summed over the chunks in float64 they are compared with the float64 sums S_w, Q_w of the float64 reference.  Every h is
within tol of its reference (max is 1-Lipschitz); a lane's partial is an fp32 chain of at most m = tpc * nq * per_group terms plus 6
shuffle stages, relatively exact to m * eps32 of the sum of the terms' magnitudes (one more rounding for the fma of the squares); the
double additions behind it are exact at this size.  With n elements per (group, channel):
  |S - S_w| <= n tol + m eps32 (sum|h_w| + n tol),
  |Q - Q_w| <= e2 + (m + 1) eps32 (Q_w + e2),   e2 = sum(2 |h_w| tol + tol^2)."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
from kernel_cases import MM_SPECS, mm_instance, run_conv_mm_case

SENTINEL = 1.2345e30
GUARD = 4096          # floats in front of and behind y


def run_epilogue_case(dev, name, direction, isz, force, relu_out=False, stats=False, stats_relu=True, groups=2, per_group=3, seed=0, loop=False):
    """One vg_conv_mm launch with the given epilogue flags, y between two guard bands.  'fwd': prologue = ReLU + per-(group, channel)
    affine, bias added; 'bwd': the data gradient, masked by the producer's pre-activation.  Returns the record of the case."""
    spec = MM_SPECS[name]
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

    plan = ops.mm_plan(spec, 'fwd', isz, None, force=force) if direction == 'fwd' else ops.mm_plan(spec, 'bwd', osz, isz, force=force)
    assert plan is not None, (name, direction, isz, force)
    assert (plan.waves, plan.PD, plan.PHB, plan.cc, plan.dbuf) == tuple(force)
    nslab = (plan.PH + plan.PHB - 1) // plan.PHB
    bps = ((plan.PDT + plan.PD - 1) // plan.PD) * nslab
    if loop:
        assert N * bps > 2048, (N, bps)
    # the shape is what makes the case: waves that own fewer tiles than the plan's tiles per wave, and a ragged last tile or whole waves without one
    npos = min(plan.PD, plan.PDT) * min(plan.PHB, plan.PH) * plan.PW
    ntiles = (npos + 15) // 16
    assert plan.OW % 16 != 0 and ntiles < plan.tpc * plan.waves and (npos % 16 != 0 or ntiles < plan.waves), (plan.OW, npos, plan.tpc, plan.waves)

    mask = None
    if direction == 'fwd':
        x = torch.randn((N, spec.ci) + isz, generator=g)
        b = 0.1 * torch.randn(spec.co, generator=g)
        sc = 1 + 0.3 * torch.randn(groups * spec.ci, generator=g); sh = 0.2 * torch.randn(groups * spec.ci, generator=g)

        def pro(t, dt):
            a = sc.to(dt).view(groups, 1, spec.ci, 1, 1, 1).expand(groups, per_group, spec.ci, 1, 1, 1).reshape(N, spec.ci, 1, 1, 1)
            c = sh.to(dt).view(groups, 1, spec.ci, 1, 1, 1).expand(groups, per_group, spec.ci, 1, 1, 1).reshape(N, spec.ci, 1, 1, 1)
            return torch.relu(t.to(dt)) * a + c
        raw = layer(pro(x, torch.float64), w.double(), b.double())
        own32 = layer(pro(x, torch.float32), w, b)
        K = spec.ci * taps
        args = (x.to(dev), b.to(dev), sc.to(dev), sh.to(dev))
        stored_relu = bool(relu_out)
    else:
        assert not stats
        dy = torch.randn((N, spec.co) + osz, generator=g)
        xm = torch.randn((N, spec.ci) + isz, generator=g)              # the producer's pre-activation: ReLU mask of the data gradient
        assert 0.4 < float((xm <= 0).double().mean()) < 0.6

        def dgrad(dt):
            x0 = torch.zeros((N, spec.ci) + isz, dtype=dt, requires_grad=True)
            (gx,) = torch.autograd.grad(layer(x0, w.to(dt), None), x0, dy.to(dt))
            return gx * (xm > 0)
        raw = dgrad(torch.float64)
        own32 = dgrad(torch.float32)
        K = spec.co * taps
        args = (dy.to(dev), None, None, None)
        mask = xm.to(dev)
        stored_relu = False                                            # masked stores ignore relu_out
    want = torch.relu(raw) if stored_relu else raw
    own32 = torch.relu(own32) if stored_relu else own32

    xin, bias, scale, shift = args
    lib = _lib.get_lib()
    tau, dlt, _ = plan.tables(xin.device)
    aimg = plan.gather(w.to(dev))
    d = plan.desc(N, direction == 'fwd', per_group if scale is not None else 1, relu_out)
    numel = want.numel()
    ybuf = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    y = ybuf[GUARD:GUARD + numel]
    part = None
    if stats:
        chunks = lib.size('vg_conv_mm_stats_chunks', ctypes.byref(d), int(per_group))
        part = torch.zeros(groups * plan.CO * chunks * 2, dtype=torch.float64, device=dev)
    p = ops._p
    ops._call(xin, 'vg_conv_mm', ctypes.byref(d), p(xin), p(aimg), p(tau), p(dlt), p(bias), p(scale), p(shift), p(mask),
              ctypes.c_void_p(y.data_ptr()), int(per_group) if stats else 1, int(bool(stats_relu)), p(part))
    host = ybuf.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + numel:] == SENTINEL).all()), 'an element outside y was written'
    got = host[GUARD:GUARD + numel].reshape(want.shape)
    assert not bool((got == SENTINEL).any()), 'an element of y was not written'

    d32 = float((own32.double() - want).abs().max())
    wmax = float(want.abs().max())
    tol = max(4 * d32, eps32 * K ** 0.5 * wmax)
    err = float((got.double() - want).abs().max())
    rec = dict(name=name, direction=direction, isz=isz, force=tuple(force), N=N, bps=bps, instance=mm_instance(plan, direction == 'bwd'),
               flags=(int(bool(relu_out)), int(bool(stats)), int(bool(stats_relu))), err=err, d32=d32, tol=tol)
    print('conv_mm epilogue %s %s isz %r force %r N %d bps %d instance %r flags (relu_out, stats, stats_relu) %r: err %.3g d32 %.3g tol %.3g'
          % (name, direction, isz, tuple(force), N, bps, rec['instance'], rec['flags'], err, d32, tol))
    assert err <= tol, 'conv_mm epilogue %s %s %r: max error %.3g > tol %.3g (d32 %.3g)' % (name, direction, rec['flags'], err, tol, d32)
    if stats:
        pt = part.cpu().reshape(groups, plan.CO, -1, 2)
        S = pt[..., 0].sum(-1); Q = pt[..., 1].sum(-1)
        h = (torch.relu(raw) if stats_relu else raw).reshape(groups, per_group, spec.co, -1)
        n = per_group * h.shape[-1]
        S_w = h.sum((1, 3)); Q_w = (h * h).sum((1, 3)); A_w = h.abs().sum((1, 3))
        m = plan.tpc * plan.nq * per_group + 6
        bS = n * tol + m * eps32 * (A_w + n * tol)
        e2 = 2 * A_w * tol + n * tol * tol
        bQ = e2 + (m + 1) * eps32 * (Q_w + e2)
        eS = (S - S_w).abs(); eQ = (Q - Q_w).abs()
        print('  statistics: sum err / bound %.3g, sum of squares err / bound %.3g' % (float((eS / bS).max()), float((eQ / bQ).max())))
        assert bool((eS <= bS).all()), 'sum: worst error / bound %.3g' % float((eS / bS).max())
        assert bool((eQ <= bQ).all()), 'sum of squares: worst error / bound %.3g' % float((eQ / bQ).max())
    return rec


# (relu_out, statistics, stats_relu): the whole cube
FLAGS = [(r, s, sr) for r in (0, 1) for s in (0, 1) for sr in (0, 1)]
# (spec, layer input size, force = (waves, PD, PHB, cc, dbuf)): the tiles the planner itself picks at these sizes
FLAG_PLANS = {
    'convt4': ((3, 4, 5), (4, 5, 5, 8, 0)),         # 4 classes, 10 tiles on 4 waves x 4: waves own 3, 3, 2, 2; the last tile holds 6 positions
    'convt3': ((4, 5, 6), (4, 6, 7, 1, 0)),         # 1 class, 16 chunks of one channel, 11 tiles on 4 waves x 3; the last tile holds 8
}
# masked data gradients: (id, spec, layer input size, force, relu_out)
MASKED_CASES = [
    ('convt3_bwd-nq1', 'convt3', (4, 5, 6), (8, 4, 5, 8, 0), 0),       # mask prefetched; 8 tiles on 8 waves x 3
    ('convt3_bwd-nq1-db-relu_out', 'convt3', (4, 5, 6), (4, 1, 3, 8, 1), 1),   # ... double-buffered row slabs; relu_out must be ignored
    ('conv2_bwd-nq4', 'conv2', (7, 9, 7), (8, 4, 5, 8, 0), 0),         # mask fetched in the epilogue; 5 tiles on 8 waves: three waves own none
]


def run_co16_case(dev):
    """16 output channels (no replica rows): convt1 at 3x4x5, 14 tiles on 8 waves x 3."""
    return run_conv_mm_case(dev, MM_SPECS['convt1'], 'fwd', (3, 4, 5), (8, 5, 6, 16, 0), tpc=3)


def run_stats_run_case(dev):
    """Statistics over runs of samples: 13 groups x 8 samples, 20 blocks per sample, stored rectified."""
    return run_epilogue_case(dev, 'convt4', 'fwd', (3, 7, 4), (4, 1, 2, 8, 0), relu_out=True, stats=True, stats_relu=True, groups=13, per_group=8,
                             seed=4, loop=True)
