"""vg_conv_mm on the stride-2 transposed convs with 16 output channels, which run as TWO HALVES of 8 channels through the 4-class,
w-paired path (vg_mm_desc.co_tot = 16, CO = 8; ops._mm_build): convt2 forward (padded, the 41x49x35 network's, and plain) and conv4's
data gradient.  A block of the persistent grid owns channels [8h, 8h + 8); the half enters in five places -- the A image, the bias,
the sample base of y, the sample base of the mask source and the channel of the statistics partials -- and everywhere else the kernel
is the one the 8-channel layers run.

Every case runs twice, through the two harnesses the 8-channel layers are tested with (both float64 references, tolerance
max(4 * d32, eps32 * sqrt(K) * max|want|) and the derived statistics bounds; a lane sums as many elements as in an 8-channel launch,
so the bounds carry over):
  kernel_cases.run_conv_mm_case             through ops.conv_mm (which allocates y and the partials with 16 channels) and
                                            ops.bn_stats(pre=partials);
  conv_mm_epilogue_cases.run_epilogue_case  vg_conv_mm directly, y between two guard bands of a sentinel that must survive while no
                                            element of y keeps it, the partials summed over ALL their slots (a slot written twice or a
                                            stale one shows in the sums).
Weights, bias, mask source and input are random, so channels 0-7 and 8-15 differ in every one of the five places: a wrong half offset
moves the result by O(1), against tolerances of 1e-6.  run_distinct_halves_case adds the explicit check that channels 8-15 are not a
copy of 0-7 and that the partials' layout is the one a 16-channel launch produces (the slots no wave owns stay zero).

Shapes (N = 6: 2 groups of 3): the layer inputs the issue names, 5x6x4 (forward; position grid 6x7x5) and 9x13x8 (conv4's data
gradient; 5x7x4); each at a row-slab tile (2 slabs of 4 rows) and a whole-plane tile (3 planes: 2 blocks per sample), with ragged last
tiles and waves without a tile; waves 4 and 8, single- and double-buffered input between them.

Sample loop: convt2 (padded) at 3x4x2, 12 blocks per sample x 2 halves, 7 groups of 13 samples: N * bps * 2 = 2184 > 2048 = 256 CUs x
at most 8 resident blocks, so blocks visit several samples whatever the occupancy query returns.  The stride of a block's visits is
nsplit = floor(256 * blocks_per_cu / 24) in {10, 21, 32, 42, 53, 64, 74, 85}: none a multiple of 13, so its visits cross groups and
it flushes more than one run of statistics."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
from kernel_cases import MM_SPECS, run_conv_mm_case
from conv_mm_epilogue_cases import run_epilogue_case

# (id, spec, direction, layer input size, force = (waves, PD, PHB, cc, dbuf), relu_out).  s = row slabs, w = whole planes
FWD_CASES = [
    ('convt2p_fwd-s-w4', 'convt2p', 'fwd', (5, 6, 4), (4, 2, 4, 16, 0), 0),
    ('convt2p_fwd-w-db-relu_out', 'convt2p', 'fwd', (5, 6, 4), (8, 3, 7, 16, 1), 1),
    ('convt2_fwd-s-db', 'convt2', 'fwd', (5, 6, 4), (8, 2, 4, 16, 1), 0),
    ('convt2_fwd-w-w4', 'convt2', 'fwd', (5, 6, 4), (4, 3, 7, 16, 0), 0),
]
BWD_CASES = [
    ('conv4_bwd-s', 'conv4', 'bwd', (9, 13, 8), (8, 2, 4, 16, 0), 0),
    ('conv4_bwd-w-w4-db', 'conv4', 'bwd', (9, 13, 8), (4, 3, 7, 16, 1), 0),
]
# where ops.mm_wins keeps the launch on vg_conv_mm at the default VG_CONV_MM=1 (production_halves_launches' tags): the 21^3 toy's
# launches, one block per sample and half, measured slower there than on the register-tiled kernels (ops._halves_win)
EXPECT_ON_MM = {
    '41x49x35 convt2 fwd': True, '41x49x35 conv4 bwd': True,
    '82x98x70 convt2 fwd': True, '82x98x70 conv4 bwd': True,
    '21x21x21 convt2 fwd': False, '21x21x21 conv4 bwd': False,
}
LOOP_CASE = ('convt2p_fwd-stats-7x13', 'convt2p', 'fwd', (3, 4, 2), (4, 1, 2, 16, 0), 1, 7, 13)


def halves_instance(plan, masked):
    """(W, NQ, TPC, ks, DB, MASKED, halves) of the conv_mm_k instance a halves plan launches: the static [2, 1, 1, 1] one of the
    8-channel 3x3x3 stride-2 layers, on a grid of bps * nsplit * 2 blocks."""
    return (plan.waves, plan.nq, plan.tpc, tuple(plan.ks), plan.dbuf, int(bool(masked)), plan.CO // plan.co_blk)


def check_plan(plan, force):
    assert plan is not None
    assert (plan.CO, plan.co_blk, plan.nq, list(plan.ks), plan.tpc, plan.cc) == (16, 8, 4, [2, 1, 1, 1], 4, 16), plan.__dict__
    assert (plan.waves, plan.PD, plan.PHB, plan.cc, plan.dbuf) == tuple(force)
    one_half = sum(plan.CI * k * 64 for k in plan.ks)
    assert plan.aidx.size == 2 * one_half
    a = plan.aidx.reshape(2, -1)
    # the two halves' images hold the same taps of different output channels: same zero pattern, disjoint weights
    assert ((a[0] >= 0) == (a[1] >= 0)).all() and not np.intersect1d(a[0][a[0] >= 0], a[1][a[1] >= 0]).size
    d = plan.desc(6, False, 1)
    assert (d.CO, d.co_tot) == (8, 16)


def run_halves_case(dev, case, seed=0):
    """One listed case through both harnesses: statistics on for the forward cases, masked for the data gradient."""
    cid, name, direction, isz, force, relu_out = case[:6]
    groups, per_group = case[6:8] if len(case) > 6 else (2, 3)
    spec = MM_SPECS[name]
    fwd = direction == 'fwd'
    rec = run_conv_mm_case(dev, spec, direction, isz, force, groups, per_group, stats=fwd, seed=seed, tpc=4)
    plan = ops.mm_plan(spec, 'fwd', isz, None, force=force) if fwd else ops.mm_plan(spec, 'bwd', spec.out_size(tuple(isz)), isz, force=force)
    check_plan(plan, force)
    rec2 = run_epilogue_case(dev, name, direction, isz, force, relu_out=relu_out, stats=fwd, stats_relu=True, groups=groups,
                             per_group=per_group, seed=seed + 1)
    return rec, rec2


def run_loop_case(dev, seed=3):
    cid, name, direction, isz, force, relu_out, groups, per_group = LOOP_CASE
    plan = ops.mm_plan(MM_SPECS[name], 'fwd', isz, None, force=force)
    check_plan(plan, force)
    bps = ((plan.PDT + plan.PD - 1) // plan.PD) * ((plan.PH + plan.PHB - 1) // plan.PHB)
    N = groups * per_group
    assert N * bps * 2 > 2048, (N, bps)
    for bpc in range(1, 9):
        ns = min(max(256 * bpc // (bps * 2), 1), N)
        assert ns < N and ns % per_group != 0, (bpc, ns)
    # stored rectified with statistics: what the train step asks of convt2
    return run_epilogue_case(dev, name, 'fwd', isz, force, relu_out=relu_out, stats=True, stats_relu=True, groups=groups,
                             per_group=per_group, seed=seed)


def run_distinct_halves_case(dev, seed=5):
    """convt2 (padded) forward at 5x6x4 with statistics: every channel against float64 on its own, channels 8-15 no copy of 0-7, and the
    partials in the layout of a 16-channel launch -- [group][channel][sample][block][wave], the same slots written for every channel
    of either half and the rest still zero."""
    spec = MM_SPECS['convt2p']
    isz, force, groups, per_group = (5, 6, 4), (4, 2, 4, 16, 0), 2, 3
    N = groups * per_group
    g = torch.Generator().manual_seed(seed)
    plan = ops.mm_plan(spec, 'fwd', isz, None, force=force)
    check_plan(plan, force)
    w = 0.2 * torch.randn((spec.ci, spec.co) + tuple(spec.k), generator=g)
    x = torch.randn((N, spec.ci) + isz, generator=g)
    b = 0.5 + torch.arange(spec.co, dtype=torch.float32)            # a bias that names its channel
    want = F.conv_transpose3d(x.double(), w.double(), b.double(), spec.stride, spec.pad, spec.outpad)
    own32 = F.conv_transpose3d(x, w, b, spec.stride, spec.pad, spec.outpad)
    got, part = ops.conv_mm(x.to(dev), plan, plan.gather(w.to(dev)), b.to(dev), False, None, None, 1, None, per_group)
    got = got.cpu()
    assert tuple(got.shape) == tuple(want.shape) and got.shape[1] == 16
    eps32 = float(np.finfo(np.float32).eps)
    K = spec.ci * 27
    for c in range(16):
        d32 = float((own32[:, c].double() - want[:, c]).abs().max())
        tol = max(4 * d32, eps32 * K ** 0.5 * float(want[:, c].abs().max()))
        err = float((got[:, c].double() - want[:, c]).abs().max())
        assert err <= tol, 'channel %d: max error %.3g > tol %.3g' % (c, err, tol)
    lo, hi = got[:, :8], got[:, 8:]
    assert not torch.equal(lo, hi), 'channels 8-15 are a copy of channels 0-7'
    pt = part.cpu().reshape(groups, 16, per_group, -1, plan.waves, 2)  # [group][channel][sample of the group][block][wave]
    # 6 samples on 6 slabs x 2 halves: every block visits one sample, so every sample ends a run; the waves that own a tile write, and they
    # are the same waves for every channel of either half
    written = (pt != 0).all(-1)
    assert bool((written == written[:, :1]).all()), 'the written slots differ between channels'
    assert bool(written.any(-1).all()), 'a block wrote no partial'
    assert bool((pt[~written] == 0).all()), 'half-written slot'
    return dict(err=err, tol=tol)


# (id, spec, layer input size, groups, per_group, relu_out): N = 6; at 5x6x4 one block per sample; at 9x11x8 (3 groups of 2) the
# 10 x 12 x 9 bricks of 2x2x2 outputs run in blocks of 2 x 12 x 9 threads out of 256 (40 idle lanes), 5 blocks per sample
STATS_OF_CASES = [
    ('convt2p-5x6x4-rectified', 'convt2p', (5, 6, 4), 2, 3, 1),
    ('convt2-5x6x4', 'convt2', (5, 6, 4), 2, 3, 0),
    ('convt2p-9x11x8-rectified', 'convt2p', (9, 11, 8), 3, 2, 1),
]


def run_stats_of_case(dev, case, seed=7):
    """What the train step launches for convt2's forward -- vg_conv_mm in two halves without statistics, then
    vg_tconv3d_s2_stats_of on its output (ops.conv_mm(stats_like=spec)) -- against the register-tiled engine's fused launch
    (ops.conv_forward(next_bn=...)) on the same input: y AND the statistics partials must be equal bit for bit.  Both engines add a
    lane's products in the same order (input channel, then kd, kh, kw ascending; the fp32 matrix cores are exact FMAs), and the
    partials kernel repeats the fused launch's thread mapping and summation order; so the step's results do not depend on the engine."""
    cid, name, isz, groups, per_group, relu_out = case
    spec = MM_SPECS[name]
    N = groups * per_group
    g = torch.Generator().manual_seed(seed)
    w = (0.2 * torch.randn((spec.ci, spec.co) + tuple(spec.k), generator=g)).to(dev)
    x = torch.relu(torch.randn((N, spec.ci) + tuple(isz), generator=g)).to(dev)       # a rectified hand-off: no prologue
    b = (0.1 * torch.randn(spec.co, generator=g)).to(dev)
    plan = ops.mm_plan(spec, 'fwd', isz)
    assert plan is not None and (plan.CO, plan.co_blk) == (16, 8)
    ym, pm = ops.conv_mm(x, plan, plan.gather(w), b, False, None, None, 1, None, per_group, bool(relu_out), stats_like=spec)
    yd, pd = ops.conv_forward(x, ops.pack_weight(w, spec, 'fwd'), b, spec, False, None, None, 1, per_group, bool(relu_out))
    assert tuple(ym.shape) == tuple(yd.shape) and pm.shape == pd.shape
    ndiff = int((ym != yd).sum())
    assert ndiff == 0, '%s: %d elements of y differ between the engines (max %.3g)' % (cid, ndiff, float((ym - yd).abs().max()))
    assert float(pd.abs().max()) > 0
    nd = int((pm != pd).sum())
    assert nd == 0, '%s: %d of %d partials differ from the fused launch (max %.3g)' % (cid, nd, pd.numel(), float((pm - pd).abs().max()))
    gamma = torch.ones(spec.co, device=dev); beta = torch.zeros(spec.co, device=dev)
    for a_, b_ in zip(ops.bn_stats(ym, gamma, beta, True, per_group, pre=pm), ops.bn_stats(yd, gamma, beta, True, per_group, pre=pd)):
        assert torch.equal(a_, b_)
    # the pre-activation's statistics cannot be taken from a rectified tensor
    lib = _lib.get_lib()
    _, cd, _ = ops.conv_fwd_desc(spec, N, isz, False, 1, True)
    rc = lib.dll.vg_tconv3d_s2_stats_of(ctypes.byref(cd), ops._p(yd), per_group, 0, ops._p(pm), None)
    assert rc == 1 and b'rectified' in lib.dll.vg_last_error()
    return dict(id=cid, partials=pd.numel())


def check_descriptor_refusals():
    """co_tot / CO must be 1, or 2 with CO == 8: everything else is VG_ERR_ARG before any pointer is looked at (null pointers here:
    nothing can be launched)."""
    lib = _lib.get_lib()
    fn = lib.dll.vg_conv_mm

    def status(d):
        return fn(ctypes.byref(d), None, None, None, None, None, None, None, None, None, 1, 0, None, None)
    ARG = 1
    half = ops.mm_plan(MM_SPECS['convt2p'], 'fwd', (5, 6, 4), None, force=(4, 2, 4, 16, 0))
    full = ops.mm_plan(MM_SPECS['convt1'], 'fwd', (3, 4, 5), None, force=(8, 5, 6, 16, 0))
    for plan, co, co_tot in ((full, 16, 32), (half, 8, 12), (half, 8, 24), (half, 8, 4), (half, 8, -8), (full, 16, 8)):
        d = plan.desc(6, False, 1)
        d.CO, d.co_tot = co, co_tot
        assert status(d) == ARG, (co, co_tot)
        msg = lib.dll.vg_last_error()
        assert msg.startswith(b'vg_conv_mm:') and b'co_tot' in msg, msg
    # what is accepted gets as far as the pointer check
    for plan, co, co_tot in ((half, 8, 16), (half, 8, 8), (half, 8, 0), (full, 16, 16), (full, 16, 0)):
        d = plan.desc(6, False, 1)
        d.CO, d.co_tot = co, co_tot
        assert status(d) == ARG and b'null argument' in lib.dll.vg_last_error(), (co, co_tot, lib.dll.vg_last_error())
    d = half.desc(6, False, 1)
    assert lib.size('vg_conv_mm_stats_chunks', ctypes.byref(d), 3) == 3 * 3 * 2 * 4          # per_group x plane slabs x row slabs x waves: no factor for the halves


def production_halves_launches():
    """-> [(tag, spec, direction, read size, write size)]: convt2 forward and conv4's data gradient of the three networks"""
    import kernel_cases as K
    from vae_gam_amd.schema import net_geometry
    out = []
    for img, _ in K.WGRAD_NETS:
        geo = net_geometry(img)
        for specs, sizes in ((geo.enc, geo.enc_sizes()), (geo.dec, geo.dec_sizes())):
            for i, spec in enumerate(specs):
                tag = '%s %s' % ('x'.join(map(str, img)), spec.name)
                if spec.name == 'convt2':
                    out.append((tag + ' fwd', spec, 'fwd', tuple(sizes[i]), None))
                if spec.name == 'conv4':
                    out.append((tag + ' bwd', spec, 'bwd', tuple(sizes[i + 1]), tuple(sizes[i])))
    assert len(out) == 6, out
    return out
