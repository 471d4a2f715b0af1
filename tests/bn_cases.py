"""Shared bodies of the batch-norm kernel tests (vg_bn.hip): every entry point against float64 torch on the CPU, at one case per
class of the launch plan (`ops.bn_plan`: cp position chunks per sample, ns sample splits per group).  Run on CPU tensors through the
host build of the kernels (tests/test_bn_emu.py) and on the GPU through libvaegam_hip.so (tests/test_bn_gpu.py).

Inputs: sample n has its own mean 0.3 * ((7 n) % 11 - 5) and spread 0.5 + (n % 5) / 4, so a dropped or doubled sample moves the
statistics of its group; the last position of every sample holds 16 x that sample's spread, so a dropped tail does.

Tolerances are derived, never measured from the kernel.  eps32 = 2^-23; d32 = the largest error of the same quantity computed in plain
fp32 torch on the CPU against float64; K = the number of terms summed.
  sums (channel sums, dgamma, dbeta, the producer's bias gradient, mean * count):
      max(4 d32, eps32 (|want| + sqrt(K) max|term|))
  rstd, scale (relative):  max(4 d32_rel, 16 eps32 (1 + mean^2 / var))
      the kernel sums squares in fp32 runs of 64 and the runs in double: a run carries about sqrt(64) eps32 / 2 relative error, the
      subtraction E[x^2] - mean^2 magnifies it by 1 + mean^2 / var; 16 is 4 x that
  shift = beta - mean * scale: the relative bound of scale applied to |beta| + |mean * scale| (the magnitude of the two terms: where
      they cancel, the difference itself is no scale for its error), plus |scale| x the bound of the mean
  dp and dw elementwise:  max(4 d32, 16 eps32 max|want|)
A result added into a prefilled buffer gets eps32 (|prefill| + |want|) for the rounding of that add.
Every check prints err, tol, err / tol and err / d32 before it asserts."""
import math

import torch
import torch.nn.functional as F

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops

EPS32 = 2.0 ** -23
BN_EPS = ops.BN_EPS

# id: (C, G, per_group, P, (cp, ns)) -- the expected plan is a hand evaluation of plan_for, asserted through ops.bn_plan
PLAN_CASES = {
    'one-sample': (8, 2, 2, 80, (1, 2)),                # one sample per block (the corner every layer test sits in)
    'even-stride': (16, 8, 32, 100, (1, 16)),           # 2 samples per block
    'uneven-stride': (16, 9, 33, 240, (1, 14)),         # 3 or 2 samples per block
    'all-in-one': (16, 129, 3, 50, (1, 1)),             # want < 1 clamp: one block walks the group
    'chunk-tail': (8, 2, 3, 8193, (3, 3)),              # chunk % cp with chunk / cp; the last position chunk holds one element
    'cap-flush': (1, 1, 1, 1100003, (64, 1)),           # cp cap, 68 elements per thread: the fp32 run is flushed at 64
    'cap-fold': (1, 1, 8, 270001, (64, 8)),             # 512 chunks: second trip of the fold loops
    'wide-c': (70, 2, 2, 30, (1, 2)),                   # G * C = 140: bn_finalize_k / bn_param_grad_k beyond one 64-thread block
    'flush-across': (16, 129, 17, 1000, (1, 1)),        # 68 elements per thread over 17 samples: the flush counter carried across samples
}
# 35 M elements (140 MB per tensor); no shape below about 33.5 M elements reaches that branch (about 2,048 blocks x 256 threads x more
# than 64 elements): on the GPU only
GPU_ONLY = ('flush-across',)
HOST_CASES = tuple(c for c in PLAN_CASES if c not in GPU_ONLY)
OFFSET_CASES = ('chunk-tail', 'cap-flush')              # run again with every value shifted so that |mean| / std = 10
TWO_RANK_CASES = ('uneven-stride', 'chunk-tail')
PART_CHUNKS = (1, 255, 257, 1300)
# (N, C, P): vg_channel_sum plans with per_group = N, G = 1
CHANNEL_SUM_CASES = {(6, 8, 80): (1, 6), (100, 16, 240): (1, 64), (3, 8, 8193): (3, 3), (1, 1, 1100003): (64, 1), (8, 1, 270001): (64, 8)}
# id: (C, (ID, IH, IW), per_group, G)
TCONV1_CASES = {
    'ct8-short-tile': (8, (1, 5, 6), 2, 2),             # CT = 8; npos = 30 < 256: the second position slot is all masked
    'ct8-depth-tail': (8, (4, 7, 13), 3, 2),            # nd = 1 in the last tile; chunk = (n % per_group) * tilesD + td
    'ct8-ragged': (8, (7, 20, 27), 5, 3),               # npos = 1620: 4 loop trips with a ragged end, 5 samples per group
    'generic-c3-plane': (3, (5, 36, 36), 2, 2),         # generic instance, large plane
    'generic-c16': (16, (2, 6, 9), 3, 2),               # C = FT_MAXC: full register arrays, nd = 2
    'generic-c1': (1, (3, 4, 33), 2, 1),                # single channel
}
DATA_BN_CASES = ((8, 1, 27), (16, 2, 27), (3, 5, 125))  # (CO, CI, T): the second and third take second trips of all three strided loops

RECORDS = []                                            # (what, quantity, err / tol, err / d32) of every check made in this process


def _check(what, qty, err, tol, d32):
    """err, tol: float64 tensors (or tol a float); d32: float.  Prints, records, asserts err <= tol everywhere."""
    err = torch.as_tensor(err, dtype=torch.float64)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    assert bool(torch.isfinite(err).all()), '%s %s: not finite' % (what, qty)
    i = int((err / tol).argmax())
    e, t = float(err.reshape(-1)[i]), float(tol.reshape(-1)[i])
    emax = float(err.max())
    rd = emax / d32 if d32 > 0 else float('inf') if emax > 0 else 0.0
    print('bn %s %s: err %.3g tol %.3g err/tol %.3g d32 %.3g err/d32 %.3g' % (what, qty, e, t, e / t, d32, rd))
    RECORDS.append((what, qty, e / t, rd))
    assert e <= t, '%s %s: error %.3g > tolerance %.3g (d32 %.3g)' % (what, qty, e, t, d32)


def tol_sum(want, d32, K, term_max):
    return torch.clamp(EPS32 * (want.abs() + math.sqrt(K) * term_max), min=4 * d32)


def _d(a, b):
    return float((a.double() - b).abs().max())


def case_plan(cid):
    """-> (C, G, per_group, P), after asserting the case's plan through the library's planner"""
    C, G, pg, P, want = PLAN_CASES[cid]
    got = ops.bn_plan(G * pg, C, P, pg)
    assert got == want, '%s: plan %r, the case is there for %r' % (cid, got, want)
    return C, G, pg, P


def make_x(N, C, P, seed, offset=False):
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(N)
    mean = 0.3 * (((7 * n) % 11) - 5).float()
    std = 0.5 + (n % 5).float() / 4
    x = torch.randn((N, C, P), generator=g)
    x.mul_(std.view(N, 1, 1)).add_(mean.view(N, 1, 1))
    x[:, :, -1] = (16 * std).view(N, 1)
    if offset:
        xd = x.double()
        x.add_(float(10 * xd.std() - xd.mean()))
    return x, g


def make_affine(C, g):
    return 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


class Sync:
    """Stand-in for the data-parallel all-reduce: records what it is handed; returns `total` when given (the sum over ranks), else its
    argument (one rank)."""
    def __init__(self, world_size=1, total=None):
        self.world_size, self.total, self.seen = world_size, total, []

    def __call__(self, t):
        self.seen.append(t.clone())
        return t if self.total is None else self.total


# ---------------------------------------------------------------------------------------------------------------- statistics
def ref_stats(x, G, pg, relu, gamma, beta, dt):
    N, C, P = x.shape
    h = x.to(dt)
    if relu:
        h = h.clamp_min(0)
    hg = h.reshape(G, pg, C, P)
    s = hg.sum((1, 3))
    mean = hg.mean((1, 3))
    var = hg.var((1, 3), unbiased=False)
    rstd = (var + BN_EPS).rsqrt()
    gm = gamma.to(dt) if gamma is not None else torch.ones(C, dtype=dt)
    bt = beta.to(dt) if beta is not None else torch.zeros(C, dtype=dt)
    scale = gm[None] * rstd
    return dict(sum=s, mean=mean, var=var, rstd=rstd, scale=scale, shift=bt[None] - mean * scale, beta=bt, hmax=float(h.abs().max()))


def check_stats(what, got, w, w32, K):
    """got = (scale, shift, mean, rstd) of the kernel, each [G * C]; w / w32 = ref_stats in float64 / float32"""
    sc, sh, mu, rs = [t.detach().cpu().double().reshape(w['mean'].shape) for t in got]
    d32s = _d(w32['sum'], w['sum'])
    ts = tol_sum(w['sum'], d32s, K, w['hmax'])
    _check(what, 'mean*count', (mu * K - w['sum']).abs(), ts, d32s)
    amp = 16 * EPS32 * (1 + w['mean'] ** 2 / w['var'])
    d32r = float(((w32['rstd'].double() - w['rstd']).abs() / w['rstd']).max())
    _check(what, 'rstd(rel)', (rs - w['rstd']).abs() / w['rstd'], torch.clamp(amp, min=4 * d32r), d32r)
    d32c = float(((w32['scale'].double() - w['scale']).abs() / w['scale'].abs()).max())
    _check(what, 'scale(rel)', (sc - w['scale']).abs() / w['scale'].abs(), torch.clamp(amp, min=4 * d32c), d32c)
    d32h = _d(w32['shift'], w['shift'])
    th = amp * (w['beta'].abs()[None] + (w['mean'] * w['scale']).abs()) + w['scale'].abs() * ts / K
    _check(what, 'shift', (sh - w['shift']).abs(), torch.clamp(th, min=4 * d32h), d32h)


def run_stats_case(dev, cid, relu, offset=False):
    """ops.bn_stats: the fused fold + finalize launch, and the sync= form with an identity sync (ext_sums, bn_fold_k with nout = 3,
    vg_bn_finalize; the count column must be per_group * P exactly); on 'one-sample' also gamma = beta = None."""
    C, G, pg, P = case_plan(cid)
    x, g = make_x(G * pg, C, P, seed=101, offset=offset)
    gamma, beta = make_affine(C, g)
    K = pg * P
    w = ref_stats(x, G, pg, relu, gamma, beta, torch.float64)
    w32 = ref_stats(x, G, pg, relu, gamma, beta, torch.float32)
    what = '%s%s relu %d' % (cid, ' offset' if offset else '', relu)
    if offset:
        r = (w['mean'].abs() * w['rstd'])
        print('bn %s: |mean| / std from %.2f to %.2f' % (what, float(r.min()), float(r.max())))
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    check_stats(what + ' stats', ops.bn_stats(xd, gd, bd, relu, pg), w, w32, K)
    sync = Sync()
    got = ops.bn_stats(xd, gd, bd, relu, pg, sync=sync)
    assert len(sync.seen) == 1 and tuple(sync.seen[0].shape) == (G * C, 3)
    sums = sync.seen[0].cpu()
    assert bool((sums[:, 2] == float(K)).all()), what + ': count column'
    _check(what + ' sync', 'sum', (sums[:, 0].reshape(G, C) - w['sum']).abs(), tol_sum(w['sum'], _d(w32['sum'], w['sum']), K, w['hmax']),
           _d(w32['sum'], w['sum']))
    check_stats(what + ' sync', got, w, w32, K)
    if cid == 'one-sample':
        w0 = ref_stats(x, G, pg, relu, None, None, torch.float64)
        check_stats(what + ' no-affine', ops.bn_stats(xd, None, None, relu, pg), w0, ref_stats(x, G, pg, relu, None, None, torch.float32), K)


def run_parts_case(dev, chunks):
    """ops.bn_stats(pre=part): synthetic float64 partials [G * C][chunks][2] folded by bn_fold_finalize_k, and by bn_fold_k (nout = 3) +
    vg_bn_finalize with a sync.  x is not read: one element per channel of the right N, C.  The fold is in double; what is left is the
    fp32 rounding of the results: mean, rstd one rounding (bound 2 eps32 relative), scale two (3 eps32), shift = beta - mean * scale
    three (4 eps32 (|beta| + |mean * scale|))."""
    G, C, pg = 2, 3, 4
    g = torch.Generator().manual_seed(300 + chunks)
    part = torch.empty((G * C, chunks, 2), dtype=torch.float64)
    part[:, :, 0] = 0.1 * torch.randn((G * C, chunks), generator=g, dtype=torch.float64)
    part[:, :, 1] = 1 + torch.rand((G * C, chunks), generator=g, dtype=torch.float64)
    part[:, -1, 0] += 5.0; part[:, -1, 1] += 40.0                           # the last chunk carries most of both sums
    gamma, beta = make_affine(C, g)
    count = float(pg)
    s = part.sum(1)
    mean = (s[:, 0] / count); var = s[:, 1] / count - mean ** 2
    assert bool((var > 0).all())
    rstd = (var + BN_EPS).rsqrt()
    gm, bt = gamma.double().repeat(G), beta.double().repeat(G)
    scale = gm * rstd; shift = bt - mean * scale
    x = torch.zeros((G * pg, C, 1), device=dev)
    pd, gd, bd = part.to(dev), gamma.to(dev), beta.to(dev)
    for form in ('fused', 'sync'):
        sync = Sync() if form == 'sync' else None
        sc, sh, mu, rs = [t.cpu().double() for t in ops.bn_stats(x, gd, bd, True, pg, sync=sync, pre=pd)]
        what = 'parts %d %s' % (chunks, form)
        if sync is not None:
            sums = sync.seen[0].cpu()
            assert bool((sums[:, 2] == count).all())
            bound = chunks * 2.0 ** -52 * part.abs().sum(1)
            _check(what, 'sums', (sums[:, :2] - s).abs(), bound, 0.0)
        _check(what, 'mean', (mu - mean).abs(), 2 * EPS32 * mean.abs(), 0.0)
        _check(what, 'rstd', (rs - rstd).abs(), 2 * EPS32 * rstd, 0.0)
        _check(what, 'scale', (sc - scale).abs(), 3 * EPS32 * scale.abs(), 0.0)
        _check(what, 'shift', (sh - shift).abs(), 4 * EPS32 * (bt.abs() + (mean * scale).abs()), 0.0)


# ---------------------------------------------------------------------------------------------------------------- backward
def ref_backward(p, dxe, gamma, beta, G, pg, relu, dt):
    """float64 (dt) autograd of BN(relu?(p)) per group with upstream gradient dxe"""
    N, C, P = p.shape
    pp = p.to(dt).requires_grad_(True)
    gm = gamma.to(dt).requires_grad_(True); bt = beta.to(dt).requires_grad_(True)
    h = torch.relu(pp) if relu else pp
    hg = h.reshape(G, pg, C, P)
    mean = hg.mean((1, 3), keepdim=True)
    rstd = (hg.var((1, 3), unbiased=False, keepdim=True) + BN_EPS).rsqrt()
    hhat = (hg - mean) * rstd
    y = hhat * gm.view(1, 1, C, 1) + bt.view(1, 1, C, 1)
    up = dxe.to(dt).reshape(G, pg, C, P)
    dp, dg, db = torch.autograd.grad(y, [pp, gm, bt], up)
    return dict(dp=dp, dgamma=dg, dbeta=db, pbg=dp.sum((0, 2)), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1),
                tg=float((up * hhat.detach()).abs().max()), tb=float(up.abs().max()), tp=float(dp.abs().max()))


def check_backward(what, dp, dg, db, pbg, w, w32, K, pre=None):
    """dp [N][C][P]; dg, db, pbg [C] as float64 CPU tensors with any prefill already subtracted; pre: |prefill| per quantity"""
    pre = pre or {}
    d = _d(w32['dp'], w['dp'])
    _check(what, 'dp', (dp - w['dp']).abs().amax((0, 2)), max(4 * d, 16 * EPS32 * w['tp']), d)
    for name, got, term in (('dgamma', dg, w['tg']), ('dbeta', db, w['tb']), ('pbg', pbg, w['tp'])):
        if got is None:
            continue
        d = _d(w32[name], w[name])
        tol = tol_sum(w[name], d, K, term) + EPS32 * (pre.get(name, 0.0) + w[name].abs())
        _check(what, name, (got - w[name]).abs(), tol, d)


def run_backward_case(dev, cid, relu):
    """ops.bn_backward_ with free gamma / beta (dgamma, dbeta returned) and with nn.Parameters whose .grad is prefilled at random
    ((None, None) returned, .grad - prefill is the gradient); producer_bias_grad prefilled with 0.5.  mean / rstd handed to the kernel are
    the float64 statistics rounded to fp32."""
    C, G, pg, P = case_plan(cid)
    N = G * pg
    p, g = make_x(N, C, P, seed=202)
    gamma, beta = make_affine(C, g)
    dxe = torch.randn((N, C, P), generator=g)
    K = N * P
    w = ref_backward(p, dxe, gamma, beta, G, pg, relu, torch.float64)
    w32 = ref_backward(p, dxe, gamma, beta, G, pg, relu, torch.float32)
    pd, md, rd = p.to(dev), w['mean'].float().to(dev), w['rstd'].float().to(dev)
    what = '%s relu %d' % (cid, relu)
    # free tensors
    dx = dxe.to(dev).clone(); pbg = torch.full((C,), 0.5, device=dev)
    dg, db = ops.bn_backward_(dx, pd, gamma.to(dev), md, rd, relu, pg, None, beta.to(dev), pbg)
    check_backward(what + ' free', dx.cpu().double(), dg.cpu().double(), db.cpu().double(), pbg.cpu().double() - 0.5, w, w32, K, dict(pbg=0.5))
    # bound .grad buffers
    gp, bp = torch.nn.Parameter(gamma.to(dev).clone()), torch.nn.Parameter(beta.to(dev).clone())
    rg, rb = 2 * torch.randn(C, generator=g), 2 * torch.randn(C, generator=g)
    gp.grad = rg.to(dev).clone(); bp.grad = rb.to(dev).clone()
    dx = dxe.to(dev).clone(); pbg = torch.full((C,), 0.5, device=dev)
    out = ops.bn_backward_(dx, pd, gp, md, rd, relu, pg, None, bp, pbg)
    assert out == (None, None), what + ': gradients were returned although .grad is bound'
    check_backward(what + ' bound', dx.cpu().double(), gp.grad.cpu().double() - rg.double(), bp.grad.cpu().double() - rb.double(),
                   pbg.cpu().double() - 0.5, w, w32, K, dict(pbg=0.5, dgamma=rg.abs().double(), dbeta=rb.abs().double()))


def run_two_rank_case(dev, cid):
    """Two data-parallel ranks in one process.  Each rank holds the case's shape (so each launch has the case's plan) -- the whole
    batch has 2 * per_group samples per group, rank r the r-th half of every group.  Pass 1 records each rank's raw sums with a
    one-rank sync; pass 2 hands both the total with world_size = 2.  Each rank's statistics == the whole batch's float64 statistics,
    the concatenated dp == the whole-batch dp, and the ranks' local dgamma / dbeta add up to the whole-batch values."""
    C, G, pg, P = case_plan(cid)
    relu = 1
    Nw = 2 * G * pg
    x, g = make_x(Nw, C, P, seed=303)
    gamma, beta = make_affine(C, g)
    dxe = torch.randn((Nw, C, P), generator=g)
    K = 2 * pg * P
    ws = ref_stats(x, G, 2 * pg, relu, gamma, beta, torch.float64)
    ws32 = ref_stats(x, G, 2 * pg, relu, gamma, beta, torch.float32)
    wb = ref_backward(x, dxe, gamma, beta, G, 2 * pg, relu, torch.float64)
    wb32 = ref_backward(x, dxe, gamma, beta, G, 2 * pg, relu, torch.float32)

    def half(t, r):
        return t.reshape(G, 2, pg, C, P)[:, r].reshape(G * pg, C, P).contiguous()
    gd, bd = gamma.to(dev), beta.to(dev)
    xs = [half(x, r).to(dev) for r in (0, 1)]
    rec = [Sync() for _ in (0, 1)]
    for r in (0, 1):
        ops.bn_stats(xs[r], gd, bd, relu, pg, sync=rec[r])
    total = rec[0].seen[0] + rec[1].seen[0]
    assert bool((total[:, 2] == float(K)).all())
    stats = []
    for r in (0, 1):
        stats.append(ops.bn_stats(xs[r], gd, bd, relu, pg, sync=Sync(2, total)))
        check_stats('%s rank %d of 2' % (cid, r), stats[r], ws, ws32, K)
    md, rd = wb['mean'].float().to(dev), wb['rstd'].float().to(dev)
    rec = [Sync() for _ in (0, 1)]
    for r in (0, 1):
        ops.bn_backward_(half(dxe, r).to(dev), xs[r], gd, md, rd, relu, pg, rec[r], bd)
    total = rec[0].seen[0] + rec[1].seen[0]
    dps, dgs, dbs, pbg = [], [], [], torch.full((C,), 0.5, device=dev)
    for r in (0, 1):
        dx = half(dxe, r).to(dev)
        dg, db = ops.bn_backward_(dx, xs[r], gd, md, rd, relu, pg, Sync(2, total), bd, pbg)
        dps.append(dx.cpu().double().reshape(G, 1, pg, C, P)); dgs.append(dg.cpu().double()); dbs.append(db.cpu().double())
    dp = torch.cat(dps, 1).reshape(Nw, C, P)
    check_backward('%s two ranks' % cid, dp, dgs[0] + dgs[1], dbs[0] + dbs[1], pbg.cpu().double() - 0.5, wb, wb32, Nw * P, dict(pbg=0.5))


# ---------------------------------------------------------------------------------------------------------------- channel sum
def run_channel_sum_case(dev, shape):
    N, C, P = shape
    assert ops.bn_plan(N, C, P, N) == CHANNEL_SUM_CASES[shape], shape
    x, g = make_x(N, C, P, seed=404)
    want = x.double().sum((0, 2))
    d32 = _d(x.sum((0, 2)), want)
    tol = tol_sum(want, d32, N * P, float(x.abs().max()))
    xd = x.to(dev)
    what = 'channel_sum %dx%dx%d' % shape
    _check(what, 'written', (ops.channel_sum(xd).cpu().double() - want).abs(), tol, d32)
    r = 3 * torch.randn(C, generator=g)
    out = r.to(dev).clone()
    assert ops.channel_sum(xd, out=out) is None
    _check(what, 'accumulated', (out.cpu().double() - r.double() - want).abs(), tol + EPS32 * (r.abs().double() + want.abs()), d32)


# ---------------------------------------------------------------------------------------------------------------- fused last stage
def ref_tconv1(p, dy, wt, gamma, beta, G, pg, relu, dt):
    """float64 (dt) autograd of conv_transpose3d(BN(relu?(p)), w) with upstream gradient dy"""
    N, C = p.shape[:2]
    pp = p.to(dt).requires_grad_(True)
    gm = gamma.to(dt).requires_grad_(True); bt = beta.to(dt).requires_grad_(True); ww = wt.to(dt).requires_grad_(True)
    h = torch.relu(pp) if relu else pp
    hg = h.reshape(G, pg, C, -1)
    mean = hg.mean((1, 3), keepdim=True)
    rstd = (hg.var((1, 3), unbiased=False, keepdim=True) + BN_EPS).rsqrt()
    hhat = (hg - mean) * rstd
    ybn = (hhat * gm.view(1, 1, C, 1) + bt.view(1, 1, C, 1)).reshape(p.shape)
    out = F.conv_transpose3d(ybn, ww)
    dp, dg, db, dw, dxe = torch.autograd.grad(out, [pp, gm, bt, ww, ybn], dy.to(dt))
    dxg = dxe.reshape(G, pg, C, -1)
    return dict(dp=dp.reshape(N, C, -1), dgamma=dg, dbeta=db, dw=dw, pbg=dp.sum((0, 2, 3, 4)), mean=mean.detach().reshape(-1),
                rstd=rstd.detach().reshape(-1), tg=float((dxg * hhat.detach()).abs().max()), tb=float(dxe.abs().max()),
                tp=float(dp.abs().max()))


def run_tconv1_case(dev, cid, relu):
    """ops.bn_backward_tconv1: dw_out = None (vg_bn_bwd_reduce_tconv1 + vg_bn_bwd_apply_tconv1) and dw_out prefilled (vg_wgrad3d_grouped +
    vg_bn_tconv1_sums + the apply pass) where the grouped weight gradient has an instance for the geometry."""
    C, isz, pg, G = TCONV1_CASES[cid]
    N = G * pg
    P = isz[0] * isz[1] * isz[2]
    x, g = make_x(N, C, P, seed=505)
    p = x.reshape((N, C) + isz)
    gamma, beta = make_affine(C, g)
    wt = 0.2 * torch.randn((C, 1, 3, 3, 3), generator=g)
    dy = torch.randn((N, 1, isz[0] + 2, isz[1] + 2, isz[2] + 2), generator=g)
    w = ref_tconv1(p, dy, wt, gamma, beta, G, pg, relu, torch.float64)
    w32 = ref_tconv1(p, dy, wt, gamma, beta, G, pg, relu, torch.float32)
    K = N * P
    pd, dyd, wd, gd, bd = p.to(dev), dy.to(dev), wt.to(dev), gamma.to(dev), beta.to(dev)
    md, rd = w['mean'].float().to(dev), w['rstd'].float().to(dev)
    grouped = ops._grouped_wgrad_ok(tuple(pd.shape), pg)
    forms = ('reduce', 'grouped') if grouped else ('reduce',)
    if not grouped:
        assert grouped is False
        print('bn tconv1 %s: no grouped weight-gradient instance for this geometry, reduce form only' % cid)
    for form in forms:
        what = 'tconv1 %s relu %d %s' % (cid, relu, form)
        pbg = torch.full((C,), 0.5, device=dev)
        r = 2 * torch.randn(wt.shape, generator=g)
        dw_out = r.to(dev).clone() if form == 'grouped' else None
        dp, dg, db = ops.bn_backward_tconv1(dyd, wd, pd, gd, md, rd, relu, pg, None, bd, pbg, dw_out=dw_out)
        check_backward(what, dp.cpu().double().reshape(N, C, P), dg.cpu().double(), db.cpu().double(), pbg.cpu().double() - 0.5, w, w32, K,
                       dict(pbg=0.5))
        if dw_out is not None:
            d = _d(w32['dw'], w['dw'])
            tol = max(4 * d, 16 * EPS32 * float(w['dw'].abs().max())) + EPS32 * (r.abs().double() + w['dw'].abs())
            _check(what, 'dw', (dw_out.cpu().double() - r.double() - w['dw']).abs(), tol, d)


def run_tconv1_rejects_wide(dev):
    """C = 17 > FT_MAXC: an error, no launch"""
    import pytest
    C, isz, N = 17, (2, 3, 4), 2
    p = torch.randn((N, C) + isz, device=dev); dy = torch.randn((N, 1, 4, 5, 6), device=dev); wt = torch.randn((C, 1, 3, 3, 3), device=dev)
    st = torch.ones(C, device=dev)
    with pytest.raises(_lib.VgError):
        ops.bn_backward_tconv1(dy, wt, p, st, st.clone(), st.clone(), 1, N, None, st.clone(), None)


# ---------------------------------------------------------------------------------------------------------------- data batch norm
def run_data_bn_case(dev, shape):
    """vg_data_bn_grads (one block of 256 threads), written and accumulated, against the formulas of its comment in float64:
    dw = gamma[ci] dw_hat + beta[ci] db[co], dbias = db, dgamma[ci] = sum_{co,t} w dw_hat, dbeta[ci] = sum_{co,t} w db[co]."""
    CO, CI, T = shape
    g = torch.Generator().manual_seed(606)
    dw_hat = torch.randn((CO, CI, T), generator=g); db = torch.randn(CO, generator=g); wt = 0.2 * torch.randn((CO, CI, T), generator=g)
    gamma, beta = make_affine(CI, g)

    def ref(dt):
        a, b, ww, gm, bt = [t.to(dt) for t in (dw_hat, db, wt, gamma, beta)]
        return dict(dw=gm.view(1, CI, 1) * a + bt.view(1, CI, 1) * b.view(CO, 1, 1), dbias=b, dgamma=(ww * a).sum((0, 2)),
                    dbeta=(ww * b.view(CO, 1, 1)).sum((0, 2)))
    w, w32 = ref(torch.float64), ref(torch.float32)
    terms = dict(dgamma=float((wt * dw_hat).abs().max()), dbeta=float((wt * db.view(CO, 1, 1)).abs().max()))
    dev_in = [t.to(dev).contiguous() for t in (dw_hat, db, wt, gamma, beta)]
    for acc in (0, 1):
        pre = {k: 2 * torch.randn(v.shape, generator=g) for k, v in w.items()}
        out = {k: v.to(dev).clone() for k, v in pre.items()}
        ops._call(dev_in[0], 'vg_data_bn_grads', *[ops._p(t) for t in dev_in], CO, CI, T, ops._p(out['dw']), ops._p(out['dbias']),
                  ops._p(out['dgamma']), ops._p(out['dbeta']), acc)
        what = 'data_bn_grads %dx%dx%d acc %d' % (CO, CI, T, acc)
        for k in ('dw', 'dbias', 'dgamma', 'dbeta'):
            got = out[k].cpu().double() - (pre[k].double() if acc else 0)
            d = _d(w32[k], w[k])
            if k in terms:
                tol = tol_sum(w[k], d, CO * T, terms[k])
            else:
                tol = max(4 * d, 16 * EPS32 * float(w[k].abs().max()))
            if acc:
                tol = tol + EPS32 * (pre[k].abs().double() + w[k].abs())
            _check(what, k, (got - w[k]).abs(), tol, d)


def run_nshift_case(dev, n):
    """vg_data_bn_nshift: out = -(mean * rstd), one fp32 product (bound: eps32 |want| against the float64 product of the fp32 inputs)"""
    g = torch.Generator().manual_seed(707)
    mean = torch.randn(n, generator=g); rstd = 0.5 + torch.rand(n, generator=g)
    out = torch.full((n + 3,), 7.0, device=dev)
    md, rd = mean.to(dev), rstd.to(dev)
    ops._call(md, 'vg_data_bn_nshift', ops._p(md), ops._p(rd), n, ops._p(out))
    want = -(mean.double() * rstd.double())
    _check('data_bn_nshift %d' % n, 'nshift', (out[:n].cpu().double() - want).abs(), EPS32 * want.abs() + 1e-300, _d(-(mean * rstd), want))
    assert bool((out[n:] == 7.0).all()), 'wrote past n'


# ---------------------------------------------------------------------------------------------------------------- coverage
BN_LAYERS = ('conv1', 'conv3', 'conv5', 'convt1', 'convt3', 'convt5')    # the layers with a BatchNorm3d on their input (vae_reg_GP.py)


def plan_class(N, C, P, pg):
    """(cp, ns) -> the classes the kernels branch on: cp 1 / between / 64; ns equal to per_group / 1 / capped at 64 / divides per_group /
    uneven; the fp32 run flush (more than 64 elements per thread): no / within one sample / only across samples; chunks > 256."""
    cp, ns = ops.bn_plan(N, C, P, pg)
    per_sample = -(-P // (cp * 256))
    ept = -(-pg // ns) * per_sample
    return dict(cp='1' if cp == 1 else '64' if cp == 64 else 'between',
                ns='equal' if ns == pg else '1' if ns == 1 else 'cap64' if ns == 64 else 'divides' if pg % ns == 0 else 'uneven',
                flush='no' if ept <= 64 else 'within' if per_sample > 64 else 'across',
                fold='yes' if cp * ns > 256 else 'no')


def production_launches():
    """-> [(what, N, C, P, per_group)]: the batch-norm launches (statistics, backward reduce and apply share one plan) and the
    channel-sum launches of the three networks at the bench sample counts (kernel_cases.WGRAD_NETS)"""
    import kernel_cases as K
    from vae_gam_amd.schema import net_geometry
    out = []
    for img, cfgs in K.WGRAD_NETS:
        geo = net_geometry(img)
        for B, Cv in cfgs:
            for specs, sizes, N in ((geo.enc, geo.enc_sizes(), B), (geo.dec, geo.dec_sizes(), B * (Cv + 1))):
                for i, spec in enumerate(specs):
                    tag = '%s B%d C%d %s' % ('x'.join(map(str, img)), B, Cv, spec.name)
                    if spec.name in BN_LAYERS:
                        out.append((tag + ' bn', N, spec.ci, int(math.prod(sizes[i])), B))
                    out.append((tag + ' channel_sum', N, spec.co, int(math.prod(sizes[i + 1])), N))
    return out


def check_coverage():
    """Every class (per dimension of plan_class) that a production launch falls in is put under test by a listed case; where only the
    GPU-only case does, the test says so."""
    cases = {}
    for cid, (C, G, pg, P, _) in PLAN_CASES.items():
        cases[cid] = plan_class(G * pg, C, P, pg)
    for (N, C, P) in CHANNEL_SUM_CASES:
        cases['channel_sum %dx%dx%d' % (N, C, P)] = plan_class(N, C, P, N)
    host = {(dim, v) for cid, cl in cases.items() if cid not in GPU_ONLY for dim, v in cl.items()}
    gpu = {(dim, v) for cid in GPU_ONLY for dim, v in cases[cid].items()}
    prod = {}
    for what, N, C, P, pg in production_launches():
        for dim, v in plan_class(N, C, P, pg).items():
            prod.setdefault((dim, v), []).append(what)
    gpu_only = []
    for key in sorted(prod):
        by = [cid for cid, cl in cases.items() if cl[key[0]] == key[1]]
        print('bn class %s = %s: %d production launches (%s, ...) <- %s' % (key[0], key[1], len(prod[key]), prod[key][0], ', '.join(by) or 'NOT COVERED'))
        assert key in host or key in gpu, 'no case runs the class %s = %s of %s' % (key[0], key[1], prod[key][0])
        if key not in host:
            gpu_only.append(key)
            print('  covered on the GPU only: %s' % ', '.join(c for c in GPU_ONLY if cases[c][key[0]] == key[1]))
    # every class of every dimension is met by a production launch, and the host cases alone leave out the across-sample flush only
    assert {k for k in prod if k[0] == 'cp'} == {('cp', '1'), ('cp', 'between'), ('cp', '64')}
    assert {v for d, v in prod if d == 'ns'} == {'equal', '1', 'cap64', 'divides', 'uneven'}
    assert {v for d, v in prod if d == 'fold'} == {'no', 'yes'} and ('flush', 'no') in prod and ('flush', 'across') in prod
    assert gpu_only == [('flush', 'across')], gpu_only
    assert ('flush', 'within') in host          # the flush itself runs on the host build too (cap-flush)
    return dict(production=prod, cases=cases, gpu_only=gpu_only)
