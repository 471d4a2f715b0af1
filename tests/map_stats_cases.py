"""Shared bodies of the map-statistics tests: the accumulate kernel (ops.gam_stats_accumulate / vg_gam_stats_accumulate) on random
inputs, VAE.map_statistics and MapStatistics on small models, build_model_recons.mk_stat_maps.  Run on CPU tensors through the host
build of the kernels (test_map_stats_emu.py) and on the GPU through libvaegam_hip.so (test_map_stats_gpu.py).

Bounds of the kernel cases.  u = 2^-23.  Per volume and voxel the kernel forms base, cons_1..C, rec, r = x - rec in fp32 and every
square and sum in fp64; T = |base| + sum_i |cons_i| is the magnitude the fp32 error of rec (and so of r) is relative to.
  (a) against the fp32 maps of ops.gam_maps on the same inputs, accumulated in fp64 in the kernel's order: only the contraction of
      the rec sum can differ between the two kernels.  Map slots: |d| <= (C+2) u sum|m|, squared slots twice that relative to
      sum m^2, with m the slot's own map (rec included, as the issue states it).  The slots derived from r inherit rec's error, which
      is not relative to |r|: sum r: (C+2) u sum|rec|;  sum r^2: 2 (C+2) u sum |r||rec|;  sum (r+cons_i)^2: 2 (C+2) u sum |r+cons_i||rec|.
      sum x and sum x^2 hold no fp32 arithmetic at all.
  (b) against float64 numpy from the logits: fp32 expf, the divide, the product and the sum.  Map slots 16 u sum|m|, squares twice
      that relative to sum m^2 -- where for rec, a sum of C+1 rounded terms that may cancel, "|m|" is the magnitude of its terms T
      (the forward error of a floating-point sum is relative to the sum of the magnitudes, not to the result): sum rec: 16 u sum T,
      sum rec^2: 2 * 16 u sum |rec| T.  r = fl(x - rec) adds the rounding of the subtraction, relative to |x| + |rec|: with
      R = T + |x|, sum r: 16 u sum R;  sum r^2: 2 * 16 u sum |r| R;  sum (r+cons_i)^2: 2 * 16 u sum |r+cons_i| (R + |cons_i|).
      Every squared bound carries its second-order term (the first-order error squared).
Every bound also carries the fp64 accumulation itself: (n + 2) 2^-52 (sum |term| + |acc before|).
"""
import os

import numpy as np
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
import grid_cases as GC
import mask_cases as MC

U23 = 2.0 ** -23
U52 = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ kernel: inputs and references
def kernel_inputs(nat, grid, B, C, seed=0):
    """logits uniform in +-4 on the grid, gains uniform in +-2, data uniform in [0, 1) on the native grid"""
    Vn, Vg = int(np.prod(nat)), int(np.prod(grid))
    g = torch.Generator().manual_seed(seed)
    logits = (torch.rand((C + 1, B, Vg), generator=g) * 8.0 - 4.0)
    gain = (torch.rand((C, B), generator=g) * 4.0 - 2.0)
    x = torch.rand((B, Vn), generator=g)
    return logits, gain, x


def make_mask(kind, nat, seed=3):
    if kind is None:
        return None
    if kind == 'box':
        return MC.box_mask(nat, tuple(max(1, (2 * n) // 3) for n in nat))
    assert kind == 'random'
    return MC.random_mask(nat, seed)


def slot_values(maps, x):
    """per volume: the 3C+8 values a volume adds to its subject's slots, float64 [B, K, V], from maps [C+2, B, V] and x [B, V]
    (both float32: the kernel's own precision; both float64: the independent reference)"""
    C = maps.shape[0] - 2
    f = maps.dtype
    r = (x - maps[C + 1]).astype(f)
    m64, x64, r64 = maps.astype(np.float64), x.astype(np.float64), r.astype(np.float64)
    rows = [m64[j] for j in range(C + 2)] + [m64[j] ** 2 for j in range(C + 2)] + [x64, x64 ** 2, r64, r64 ** 2] + \
           [(r64 + m64[i + 1]) ** 2 for i in range(C)]
    return np.stack(rows, 1)                                     # [B, K, V]


def maps_f64(logits, gain, nat, grid):
    """the C+2 maps in float64 numpy from the logits cropped to the native grid"""
    C, B = gain.shape
    lg = GC.crop_to(logits.double().reshape((C + 1, B) + tuple(grid)), nat).reshape(C + 1, B, -1).numpy()
    s = 1.0 / (1.0 + np.exp(-lg))
    cons = gain.double().numpy()[:, :, None] * s[1:]
    rec = s[0] + cons.sum(0)
    return np.concatenate([s[:1], cons, rec[None]], 0)


def bound_magnitudes(maps, x, coef):
    """-> [B, K, V]: the per-volume share of every slot's bound, for maps of either precision (see the module docstring).
    coef = (first-order factor, 'a' or 'b')"""
    k, which = coef
    C = maps.shape[0] - 2
    m = np.abs(maps.astype(np.float64))
    x64 = x.astype(np.float64)
    rec = m[C + 1]
    T = m[:C + 1].sum(0)
    r = np.abs(x64 - maps[C + 1].astype(np.float64))
    e_rec = rec if which == 'a' else T                           # what rec's error is relative to
    e_r = rec if which == 'a' else T + np.abs(x64)               # and r's: (b) also rounds the subtraction x - rec itself
    first = [m[j] for j in range(C + 1)] + [e_rec]
    sq = [2 * m[j] ** 2 for j in range(C + 1)] + [2 * rec * e_rec]
    zero = np.zeros_like(rec)
    fit = [zero, zero, e_r, 2 * r * e_r]
    par = []
    for i in range(C):
        t = np.abs((x64 - maps[C + 1].astype(np.float64)) + maps[i + 1].astype(np.float64))
        e_t = e_r if which == 'a' else e_r + m[i + 1]
        par.append(2 * t * e_t + k * U23 * e_t ** 2)
    second = [k * U23 * e ** 2 for e in [m[j] for j in range(C + 1)] + [e_rec]]
    rows = first + [a + b for a, b in zip(sq, second)] + fit[:3] + [fit[3] + k * U23 * e_r ** 2] + par
    return k * U23 * np.stack(rows, 1)


def fold(vals, subj, acc0, mask=None, parts=None):
    """the kernel's order in float64 numpy: for every launch (parts: lists of volume indices, default one launch of all) and every
    subject with a volume in it, a partial that starts at 0 and takes the subject's volumes in ascending b, then acc += partial;
    voxels outside the mask untouched.  vals [B, K, V] -> (acc, n): n[s] volumes folded into subject s"""
    S = acc0.shape[0]
    acc = acc0.copy()
    n = np.zeros(S, dtype=np.int64)
    keep = slice(None) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    for part in (parts or [list(range(len(subj)))]):
        for s in range(S):
            mem = [b for b in part if subj[b] == s]
            if not mem:
                continue
            p = np.zeros(vals.shape[1:], dtype=np.float64)
            for b in mem:
                p += vals[b]
            acc[s][:, keep] += p[:, keep]
            n[s] += len(mem)
    return acc, n


def guarded_acc(dev, S, K, Vn, seed=11, guard=512):
    """random float64 accumulators between two guard regions, on the device: (whole buffer, the [S, K, V] view, host copy of the buffer)"""
    g = torch.Generator().manual_seed(seed)
    host = torch.randn(guard + S * K * Vn + guard, generator=g, dtype=torch.float64)
    buf = host.to(dev).clone()
    return buf, buf[guard:guard + S * K * Vn].view(S, K, Vn), host


def bits(t):
    return t.contiguous().view(torch.int64)


def launch(dev, logits, gain, x, subj, acc, nat, grid, mask):
    kw = {} if (mask is None and tuple(nat) == tuple(grid)) else dict(nat=nat, grid=grid)
    ops.gam_stats_accumulate(logits.to(dev), gain.to(dev), x.to(dev), torch.tensor(subj, dtype=torch.int32, device=dev), acc,
                             mask=None if mask is None else mask.to(dev), **kw)


# (native, grid, B, C, S, subj, mask kind)
KERNEL_CASES = [
    ((10, 10, 10), (10, 10, 10), 5, 3, 3, [2, 0, 2, 1, 2], None),          # V = 1000: a tail block; 3 volumes of a subject: a part group
    ((10, 10, 10), (10, 10, 10), 3, 0, 3, [2, 0, 2], None),                # the C <= 8 instance at its edges; subject 1 absent
    ((10, 10, 10), (10, 10, 10), 3, 8, 3, [2, 0, 2], None),
    ((10, 10, 10), (10, 10, 10), 5, 9, 3, [2, 0, 2, 1, 2], None),          # the C <= 16 instance at its edges; 3 volumes in groups of 2
    ((10, 10, 10), (10, 10, 10), 3, 16, 3, [2, 0, 2], None),
    ((10, 10, 10), (10, 10, 10), 1, 3, 1, [0], None),                      # B = 1 and S = 1
    ((5, 6, 10), (5, 6, 10), 70, 2, 2, [(b // 3) % 2 for b in range(70)], None),   # B > 64: a second chunk of the member scan
    ((19, 21, 20), (22, 22, 22), 3, 3, 2, [1, 0, 1], None),                # embedded
    ((10, 10, 10), (10, 10, 10), 3, 3, 2, [1, 0, 1], 'box'),               # masks, nat == grid
    ((10, 10, 10), (10, 10, 10), 3, 3, 2, [1, 0, 1], 'random'),
    ((19, 21, 20), (22, 22, 22), 3, 3, 2, [1, 0, 1], 'box'),               # masks, nat != grid
    ((19, 21, 20), (22, 22, 22), 3, 9, 3, [2, 0, 2], 'random'),
    ((10, 10, 10), (10, 10, 10), 5, 3, 3, [-1, 0, 3, 1, 0], None),         # ids -1 and S: skipped
]
KERNEL_IDS = ['V1000_B5_C3_S3', 'C0', 'C8', 'C9_B5', 'C16', 'B1_S1', 'B70_two_chunks', '19x21x20_in_22x22x22', 'box_mask', 'random_mask',
              'embedded_box_mask', 'embedded_random_mask_C9', 'ids_out_of_range']
BIG_CASE = ((41, 49, 35), (41, 49, 35), 8, 8, 2, [0, 1, 1, 0, 1, 1, 0, 1], None)


def run_kernel_case(dev, nat, grid, B, C, S, subj, mask_kind, seed=0):
    """One launch into accumulators prefilled with random float64 values, against (a) and (b) of the module docstring; the slab of a
    subject without a volume, the entries of voxels outside the mask and both guard regions keep their bits; a second launch on the
    same inputs gives the same bits."""
    nat, grid = tuple(nat), tuple(grid)
    Vn = int(np.prod(nat))
    K = ops.gam_stats_slots(C)
    assert K == 3 * C + 8
    logits, gain, x = kernel_inputs(nat, grid, B, C, seed)
    mask = make_mask(mask_kind, nat)
    buf, acc, host = guarded_acc(dev, S, K, Vn)
    G = (host.numel() - S * K * Vn) // 2
    acc0 = host[G:G + S * K * Vn].view(S, K, Vn).numpy().copy()
    launch(dev, logits, gain, x, subj, acc, nat, grid, mask)
    got_t = buf.cpu()
    got = got_t[G:G + S * K * Vn].view(S, K, Vn).numpy()
    assert torch.equal(bits(got_t[:G]), bits(host[:G])) and torch.equal(bits(got_t[-G:]), bits(host[-G:])), 'guard regions were written'
    # (a) the fp32 maps of gam_maps on the same inputs
    eps = torch.zeros(Vn, dtype=torch.float64, device=dev)
    glm = torch.zeros(C, Vn, device=dev)
    emb = (None, None) if nat == grid else (nat, grid)
    maps32 = ops.gam_maps(logits.to(dev), gain.to(dev), x.to(dev), eps, glm, *emb).cpu().numpy()     # (unmasked: the mask is applied by fold)
    xn = x.numpy()
    present = [s for s in range(S) if s in subj]
    inside = np.ones(Vn, dtype=bool) if mask is None else mask.reshape(-1).numpy().astype(bool)
    worst = {}
    for name, maps, coef in (('a', maps32, (C + 2, 'a')), ('b', maps_f64(logits, gain, nat, grid), (16, 'b'))):
        vals = slot_values(maps, xn if name == 'a' else xn.astype(np.float64))
        want, n = fold(vals, subj, acc0, mask)
        mag, _ = fold(bound_magnitudes(maps, xn, coef), subj, np.zeros_like(acc0), mask)
        absum, _ = fold(np.abs(vals), subj, np.zeros_like(acc0), mask)
        bound = mag + (n.max() + 2) * U52 * (absum + np.abs(acc0))
        err = np.abs(got - want)
        worst[name] = float((err / np.maximum(bound, 1e-300)).max())
        bad = err > bound
        assert not bad.any(), ('reference (%s): %d entries beyond their bound, first at [s, slot, v] = %s: |d| = %.3e, bound %.3e'
                               % (name, int(bad.sum()), np.argwhere(bad)[0].tolist(), err[bad][0], bound[bad][0]))
        assert n.tolist() == [sum(1 for v in subj if v == s) for s in range(S)]
    print('map statistics %s in %s B=%d C=%d S=%d mask=%s: worst |d| / bound (a) %.3g, (b) %.3g' % (nat, grid, B, C, S, mask_kind, worst['a'], worst['b']))
    # what the launch must not touch, as bits
    g64, a64 = got.view(np.int64), acc0.view(np.int64)
    for s in range(S):
        if s not in present:
            assert (g64[s] == a64[s]).all(), 'the slab of subject %d (no volume in the batch) changed' % s
        else:
            assert (g64[s][:, ~inside] == a64[s][:, ~inside]).all(), 'entries outside the mask changed'
            assert (g64[s][:, inside] != a64[s][:, inside]).any()
    # the same launch again: the same bits
    buf2, acc2, _ = guarded_acc(dev, S, K, Vn)
    launch(dev, logits, gain, x, subj, acc2, nat, grid, mask)
    assert torch.equal(bits(buf2.cpu()), bits(got_t)), 'two launches on the same inputs differ'


def run_halves_case(dev, nat=(10, 10, 10), B=6, C=3, S=2, subj=(0, 1, 1, 0, 1, 0), seed=1):
    """two successive launches on the halves of a batch == the reference that folds them the same way ((a): fp32 maps of gam_maps)"""
    nat = tuple(nat)
    Vn = int(np.prod(nat))
    K = ops.gam_stats_slots(C)
    logits, gain, x = kernel_inputs(nat, nat, B, C, seed)
    buf, acc, host = guarded_acc(dev, S, K, Vn)
    G = (host.numel() - S * K * Vn) // 2
    acc0 = host[G:G + S * K * Vn].view(S, K, Vn).numpy().copy()
    h = B // 2
    for sl in (slice(0, h), slice(h, B)):
        launch(dev, logits[:, sl].contiguous(), gain[:, sl].contiguous(), x[sl].contiguous(), list(subj[sl]), acc, nat, nat, None)
    got = buf.cpu()[G:G + S * K * Vn].view(S, K, Vn).numpy()
    maps32 = ops.gam_maps(logits.to(dev), gain.to(dev), x.to(dev), torch.zeros(Vn, dtype=torch.float64, device=dev),
                          torch.zeros(C, Vn, device=dev)).cpu().numpy()
    parts = [list(range(0, h)), list(range(h, B))]
    want, n = fold(slot_values(maps32, x.numpy()), list(subj), acc0, parts=parts)
    mag, _ = fold(bound_magnitudes(maps32, x.numpy(), (C + 2, 'a')), list(subj), np.zeros_like(acc0), parts=parts)
    absum, _ = fold(np.abs(slot_values(maps32, x.numpy())), list(subj), np.zeros_like(acc0), parts=parts)
    bound = mag + (n.max() + 4) * U52 * (absum + np.abs(acc0))
    assert (np.abs(got - want) <= bound).all()
    one, _ = fold(slot_values(maps32, x.numpy()), list(subj), acc0)
    assert not np.array_equal(one, want) or B < 4        # (the two foldings are different sums: the test would notice the other order)


def _status(fn, *args):
    """-> (status, text) of a raw entry point"""
    lib = _lib.get_lib()
    rc = getattr(lib.dll, fn)(*args)
    return int(rc), lib.dll.vg_last_error().decode()


def run_refusals_case(dev):
    """every refusal of vg_gam_stats_accumulate returns its status with the accumulators untouched; vg_gam_stats_slots"""
    lib = _lib.get_lib()
    assert [int(lib.dll.vg_gam_stats_slots(c)) for c in (0, 3, 8, 16)] == [8, 17, 32, 56]
    assert int(lib.dll.vg_gam_stats_slots(17)) == -1 and int(lib.dll.vg_gam_stats_slots(-1)) == -1
    nat, B, C, S = (5, 6, 7), 2, 1, 2
    Vn = int(np.prod(nat))
    logits, gain, x = (t.to(dev) for t in kernel_inputs(nat, nat, B, C))
    big = torch.zeros(18, B, Vn, device=dev)                     # the logits of 17 covariates, so that no refused launch could read past them
    subj = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    buf, acc, host = guarded_acc(dev, S, ops.gam_stats_slots(C), Vn)
    p, i3 = ops._p, ops._i3
    n3 = i3(nat)
    ARG, UNSUPPORTED = 1, 3
    cases = [
        ('C > 16', UNSUPPORTED, 'more than 16 covariates', (p(big), p(big), p(x), p(subj), None, 17, B, S, n3, n3, p(acc), None)),
        ('C < 0', ARG, 'bad arguments', (p(logits), p(gain), p(x), p(subj), None, -1, B, S, n3, n3, p(acc), None)),
        ('B = 0', ARG, 'bad arguments', (p(logits), p(gain), p(x), p(subj), None, C, 0, S, n3, n3, p(acc), None)),
        ('B < 0', ARG, 'bad arguments', (p(logits), p(gain), p(x), p(subj), None, C, -3, S, n3, n3, p(acc), None)),
        ('B > 65535', ARG, 'bad arguments', (p(logits), p(gain), p(x), p(subj), None, C, 65536, S, n3, n3, p(acc), None)),
        ('S = 0', ARG, 'bad arguments', (p(logits), p(gain), p(x), p(subj), None, C, B, 0, n3, n3, p(acc), None)),
        ('S < 0', ARG, 'bad arguments', (p(logits), p(gain), p(x), p(subj), None, C, B, -1, n3, n3, p(acc), None)),
        ('null logits', ARG, 'bad arguments', (None, p(gain), p(x), p(subj), None, C, B, S, n3, n3, p(acc), None)),
        ('null gain', ARG, 'bad arguments', (p(logits), None, p(x), p(subj), None, C, B, S, n3, n3, p(acc), None)),
        ('null x', ARG, 'bad arguments', (p(logits), p(gain), None, p(subj), None, C, B, S, n3, n3, p(acc), None)),
        ('null subj', ARG, 'bad arguments', (p(logits), p(gain), p(x), None, None, C, B, S, n3, n3, p(acc), None)),
        ('null acc', ARG, 'bad arguments', (p(logits), p(gain), p(x), p(subj), None, C, B, S, n3, n3, None, None)),
        ('null nat', ARG, 'must fit', (p(logits), p(gain), p(x), p(subj), None, C, B, S, None, n3, p(acc), None)),
        ('nat > grid', ARG, 'must fit', (p(logits), p(gain), p(x), p(subj), None, C, B, S, i3((5, 6, 8)), n3, p(acc), None)),
        ('2^31 voxels', ARG, 'must fit', (p(logits), p(gain), p(x), p(subj), None, C, B, S, n3, i3((1 << 11, 1 << 10, 1 << 10)), p(acc), None)),
        ('2^33 voxels', ARG, 'must fit', (p(logits), p(gain), p(x), p(subj), None, C, B, S, i3((1 << 11,) * 3), i3((1 << 11,) * 3), p(acc), None)),
    ]
    for what, status, pat, args in cases:
        rc, text = _status('vg_gam_stats_accumulate', *args)
        assert rc == status and pat in text and 'vg_gam_stats_accumulate' in text, (what, rc, text)
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    assert torch.equal(bits(buf.cpu()), bits(host)), 'a refused call wrote to the accumulators'
    # the tensor-level operator: shapes and dtypes are checked before anything is launched
    with np.testing.assert_raises(AssertionError):
        ops.gam_stats_accumulate(logits, gain, x, subj.long(), acc)
    with np.testing.assert_raises(AssertionError):
        ops.gam_stats_accumulate(logits, gain, x, subj, acc[:, :-1])
    with np.testing.assert_raises(ValueError):
        ops.gam_stats_accumulate(logits, gain, x, subj, acc, nat=nat, grid=nat, mask=torch.ones(Vn - 1, dtype=torch.uint8, device=dev))
    assert torch.equal(bits(buf.cpu()), bits(host))


# ------------------------------------------------------------------------------------------------ model
MODEL_C, MODEL_B, MODEL_BATCHES = 3, 3, 3
MODEL_KINDS = {'toy_21x21x21': ((21, 21, 21), False), '19x21x20_masked': ((19, 21, 20), True)}
SUBJ_2 = [[0, 0, 1], [1, 0, 1], [1, 1, 1]]              # two subjects, 3 and 6 volumes
SUBJ_3 = [[0, 1, 2], [2, 0, 1], [1, 2, 1]]              # three subjects, 2, 4 and 3 volumes
_RUNS = {}


def _noise(model, B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return {'eps_w': torch.randn(B, 1, generator=g).to(dev), 'eps_d': torch.randn(B, model.num_latents, generator=g).to(dev),
            'eps_beta': torch.randn(model.num_covariates, B, generator=g).to(dev)}


def _loader(x, cov, subj):
    B = MODEL_B
    return [{'volume': x[k * B:(k + 1) * B], 'covariates': torch.cat([cov[k * B:(k + 1) * B], torch.zeros(B, 8 - MODEL_C)], 1),
             'subjid': torch.tensor(subj[k]), 'vol_num': torch.arange(k * B, (k + 1) * B)} for k in range(MODEL_BATCHES)]


def model_run(dev, kind):
    """Built once per device and model kind and shared, unchanged, by the tests: the model, a loader of 3 batches, the replayed
    noise, the MapStatistics of two subjects, reconstruct's sums under the same noise and the per-volume maps that
    forward_core(want_maps=True) handed to reconstruct in that pass (float32, on the host)."""
    key = (str(dev), kind)
    if key in _RUNS:
        return _RUNS[key]
    img, masked = MODEL_KINDS[kind]
    N = MODEL_B * MODEL_BATCHES
    x, cov, xu, glm = GC.make_inputs(img, N, MODEL_C, 7)
    mask = MC.ellipsoid_mask(img) if masked else None
    m = MC.make_model(dev, img, xu, glm, **({'mask': mask} if masked else {}))
    noises = [_noise(m, MODEL_B, 100 + k, dev) for k in range(MODEL_BATCHES)]
    replay = lambda bi, n: noises[bi]                            # noqa: E731
    loader = _loader(x, cov, SUBJ_2)
    stats = m.map_statistics(loader, num_subjects=2, noise=replay)
    maps = []                                                    # what forward_core(want_maps=True) returns inside reconstruct, per batch
    real = m.forward_core

    def recording(*a, **k):
        out = real(*a, **k)
        assert k.get('want_maps') is True
        maps.append(out['maps'].cpu().numpy())
        return out
    m.forward_core = recording
    try:
        sums, counts = m.reconstruct(loader, [], ['unused0', 'unused1'], write_volumes=False, noise=replay)
    finally:
        del m.forward_core
    assert len(maps) == MODEL_BATCHES
    maps = np.concatenate(maps, 1)                               # (C+2, N, V) float32
    run = dict(model=m, img=img, mask=mask, loader=loader, noises=noises, replay=replay, stats=stats, sums=sums, counts=counts,
               maps=maps, x=x.reshape(N, -1).numpy(), inputs=(x, cov))
    _RUNS[key] = run
    return run


def _np_stats(maps, x, subj, S, mask=None):
    """every statistic of MapStatistics in float64 numpy from per-volume maps [C+2, N, V] and data [N, V], by the definitions
    (two-pass variances; undefined values 0).  A voxel outside the mask takes no part: the data there count as 0, like the maps."""
    C = maps.shape[0] - 2
    if mask is not None:
        x = x * np.asarray(mask).reshape(1, -1).astype(x.dtype)
    subj = np.asarray(subj)
    m64 = maps.astype(np.float64)
    r = (x - maps[C + 1]).astype(np.float64)                     # the fp32 residual, as the kernel forms it
    x64 = x.astype(np.float64)
    V = x.shape[1]
    z = lambda *s: np.zeros(s)                                   # noqa: E731
    out = dict(sum=z(C + 2, S, V), mean=z(C + 2, S, V), std=z(C + 2, S, V), r2=z(S, V), partial=z(C, S, V), resid=z(S, V), n=z(S))
    for s in range(S):
        sel = subj == s
        n = int(sel.sum())
        out['n'][s] = n
        if n == 0:
            continue
        out['sum'][:, s] = m64[:, sel].sum(1)
        out['mean'][:, s] = m64[:, sel].mean(1)
        if n >= 2:
            out['std'][:, s] = m64[:, sel].std(1, ddof=1)
        out['resid'][s] = r[sel].mean(0)
        sst = ((x64[sel] - x64[sel].mean(0)) ** 2).sum(0)
        ok = sst > 0
        srr = (r[sel] ** 2).sum(0)
        out['r2'][s][ok] = 1.0 - srr[ok] / sst[ok]
        for i in range(C):
            out['partial'][i, s][ok] = (((r[sel] + m64[i + 1, sel]) ** 2).sum(0)[ok] - srr[ok]) / sst[ok]
    out['gmean'] = out['mean'].mean(1)
    out['t'] = z(C + 2, V)
    if S >= 2:
        sd = out['mean'].std(1, ddof=1)
        ok = sd > 0
        out['t'][ok] = out['gmean'][ok] / (sd[ok] / np.sqrt(S))
    return out


def _check_derived(stats, ref, mask=None):
    """MapStatistics against _np_stats: rtol 1e-5 everywhere; atol 1e-6 x the map's scale for subject_std, 1e-4 for r2 and for
    partial_r2 (fp32 map error over SST both); the other statistics are sums of the same fp32 values in another fp64 order: an atol of
    1e-12 x scale only.  Every value finite; exactly 0 outside the mask."""
    C = stats.num_covariates
    h = lambda t: t.cpu().numpy()                                # noqa: E731
    outside = None if mask is None else ~mask.reshape(-1).numpy().astype(bool)

    def close(got, want, atol, what):
        assert got.dtype == np.float64 and np.isfinite(got).all(), what
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=atol, err_msg=what)
        if outside is not None:
            assert (got[..., outside] == 0).all(), what + ': not 0 outside the mask'

    assert h(stats.counts).tolist() == ref['n'].tolist()
    for j, k in enumerate(stats.keys):
        scale = max(1.0, float(np.abs(ref['mean'][j]).max()))
        close(h(stats.subject_mean(k)), ref['mean'][j], 1e-12 * scale, k + ' subject_mean')
        close(h(stats.subject_std(k)), ref['std'][j], 1e-6 * scale, k + ' subject_std')
        close(h(stats.group_mean(k)), ref['gmean'][j], 1e-12 * scale, k + ' group_mean')
        close(h(stats.group_t(k)), ref['t'][j], 1e-9, k + ' group_t')
    close(h(stats.r2()), ref['r2'], 1e-4, 'r2')
    close(h(stats.residual_mean()), ref['resid'], 1e-12, 'residual_mean')
    for i in range(C):
        close(h(stats.partial_r2(stats.keys[i + 1])), ref['partial'][i], 1e-4, stats.keys[i + 1] + ' partial_r2')


def run_sums_against_reconstruct(dev, kind):
    """map_statistics(...).sum(key) against the sums reconstruct(write_volumes=False) accumulates under the same noise:
    |d| <= (C+2) 2^-23 sum|m| + n 2^-52 sum|m| per subject and voxel, sum|m| from the per-volume maps; equal counts."""
    run = model_run(dev, kind)
    st, C = run['stats'], MODEL_C
    assert st.keys == list(run['sums'].keys()) and st.acc.shape == (2, 3 * C + 8, int(np.prod(run['img']))) and st.acc.dtype == torch.float64
    assert torch.equal(st.counts, run['counts']) and st.counts.tolist() == [3.0, 6.0]
    subj = np.asarray(sum(SUBJ_2, []))
    for j, k in enumerate(st.keys):
        got, want = st.sum(k).cpu().numpy(), run['sums'][k].cpu().numpy()
        for s in range(2):
            absum = np.abs(run['maps'][j][subj == s].astype(np.float64)).sum(0)
            n = int((subj == s).sum())
            bound = ((C + 2) * U23 + n * U52) * absum
            err = np.abs(got[s] - want[s])
            assert (err <= bound).all(), (k, s, float(err.max()), float(bound[err > bound][0]))
            assert absum.max() > 0


def run_derived_statistics(dev, kind):
    """every derived statistic of two subjects against float64 numpy from the per-volume maps"""
    run = model_run(dev, kind)
    ref = _np_stats(run['maps'], run['x'], sum(SUBJ_2, []), 2, run['mask'])
    _check_derived(run['stats'], ref, run['mask'])
    if run['mask'] is not None:
        inside = run['mask'].reshape(-1).numpy().astype(bool)
        assert (run['stats'].subject_std('base').cpu().numpy()[:, inside] > 0).all()


def run_group_t_three_subjects(dev, kind):
    """the same batches under the same noise with three subject ids: group_t with df = 2 (and everything else) against numpy"""
    run = model_run(dev, kind)
    m = run['model']
    x, cov = run['inputs']
    st = m.map_statistics(_loader(x, cov, SUBJ_3), num_subjects=3, noise=run['replay'])
    ref = _np_stats(run['maps'], run['x'], sum(SUBJ_3, []), 3, run['mask'])
    _check_derived(st, ref, run['mask'])
    assert float(np.abs(ref['t']).max()) > 1.0


def run_undefined_values(dev):
    """Every undefined value is exactly 0, never nan or inf -- on hand-made accumulators (MapStatistics alone, no kernel): one subject
    (no t), a subject with one volume (no std), a subject with no volume, a voxel whose data never varies (SST = 0) or whose map is the
    same in every subject (sd = 0)."""
    from vae_gam_amd.map_statistics import MapStatistics
    C, V = 1, 4
    K = 3 * C + 8
    keys = ['base', 'task', 'full_rec']
    rng = np.random.Generator(np.random.PCG64(5))
    N = 5
    maps = rng.uniform(0.1, 1.0, size=(C + 2, N, V)).astype(np.float32)
    x = rng.uniform(0.0, 1.0, size=(N, V)).astype(np.float32)
    x[:, 0] = 0.25                                               # a voxel whose data never varies: SST = 0 for every subject
    maps[0, :, 1] = 0.5                                          # a voxel whose base map is one constant: no variance anywhere
    subj = [0, 0, 0, 1, 3]                                       # subject 1: one volume; subject 2: none; subject 3: one volume
    S = 4
    vals = slot_values(maps, x)
    acc, n = fold(vals, subj, np.zeros((S, K, V)))
    st = MapStatistics(torch.from_numpy(acc).to(dev), torch.from_numpy(n.astype(np.float64)).to(dev), keys)
    every = [st.subject_mean(k) for k in keys] + [st.subject_std(k) for k in keys] + [st.group_mean(k) for k in keys] + \
            [st.group_t(k) for k in keys] + [st.r2(), st.partial_r2('task'), st.residual_mean(), st.group_r2()]
    assert all(bool(torch.isfinite(t).all()) for t in every)
    z = lambda t: bool((t == 0).all())                           # noqa: E731
    assert z(st.subject_std('base')[1:]) and z(st.subject_std('task')[1:]) and bool((st.subject_std('task')[0] > 0).all())     # n < 2
    assert z(st.subject_std('base')[:, 1])                                                                                      # no variance
    assert z(st.r2()[:, 0]) and z(st.partial_r2('task')[:, 0])                                                                 # SST = 0
    assert z(st.r2()[1:]) and z(st.partial_r2('task')[1:])                                                                     # n = 1: SST = 0
    assert z(st.subject_mean('base')[2]) and z(st.residual_mean()[2])                                                          # no volume
    assert bool((st.r2()[0, 1:] != 0).all())
    one = MapStatistics(st.acc[:1].clone(), st.counts[:1].clone(), keys)
    assert all(z(one.group_t(k)) for k in keys)                                                                                 # S < 2
    same = MapStatistics(st.acc[[0, 0, 0]].clone(), st.counts[[0, 0, 0]].clone(), keys)
    assert all(z(same.group_t(k)) for k in keys) and bool((same.group_mean('base') > 0).all())                                 # sd = 0
    ref = _np_stats(maps, x, subj, S)
    _check_derived(st, ref)
    with np.testing.assert_raises(KeyError):
        st.sum('nothing')
    with np.testing.assert_raises(KeyError):
        st.partial_r2('base')


def run_at_mean_is_deterministic(dev, kind):
    """at_mean=True twice: equal bits, whatever the generator's state; and not the statistics of a noisy pass.  The second pass
    runs with num_subjects=None: as many slots as the largest id seen needs -- the same accumulators."""
    run = model_run(dev, kind)
    m = run['model']
    torch.manual_seed(1)
    a = m.map_statistics(run['loader'], num_subjects=2, at_mean=True)
    torch.manual_seed(2)
    b = m.map_statistics(run['loader'], at_mean=True)
    assert b.num_subjects == 2 and torch.equal(bits(a.acc), bits(b.acc)) and torch.equal(a.counts, b.counts)
    assert not torch.equal(a.sum('task'), run['stats'].sum('task'))
    with np.testing.assert_raises(ValueError):
        m.map_statistics(run['loader'], num_subjects=2, at_mean=True, noise=run['replay'])


def run_bad_ids_raise_before_any_launch(dev, kind):
    run = model_run(dev, kind)
    m = run['model']
    x, cov = run['inputs']
    launched = []
    real = m.forward_core
    m.forward_core = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        for subj, S in (([[0, 0, 2]] + SUBJ_2[1:], 2), ([[0, -1, 1]] + SUBJ_2[1:], 2), ([[0, -1, 1]] + SUBJ_2[1:], None)):
            with np.testing.assert_raises(ValueError):
                m.map_statistics(_loader(x, cov, subj), num_subjects=S, noise=run['replay'])
            assert not launched, 'a batch with an id outside the range reached the device'
    finally:
        del m.forward_core
    with np.testing.assert_raises(ValueError):
        m.map_statistics(run['loader'], num_subjects=0)


def run_stat_maps_files(dev, kind, tmp_path, motion=True):
    """mk_stat_maps writes exactly the listed files into reconstructions/<ckpt>_stat_model_recons/, finite, with zeros outside the
    mask, equal to the MapStatistics it returns"""
    from vae_gam_amd import DataClass_GP as D, build_model_recons as R
    run = model_run(dev, kind)
    m = run['model']
    csv = str(tmp_path / 'subjects.csv')
    with open(csv, 'w') as f:
        f.write('idx,subjid,vol,nii_path\n0,sA,0,none_a\n1,sA,1,none_a\n2,sB,0,none_b\n')
    st = R.mk_stat_maps(csv, m, str(tmp_path), run['loader'])
    root = tmp_path / 'reconstructions' / ('%s_stat_model_recons' % str(m.epoch).zfill(3))
    assert sorted(os.listdir(str(tmp_path / 'reconstructions'))) == [root.name]
    maps = ['base', 'task', 'full_rec']                          # C = 3: task, x_mot, y_mot; the motion maps are off by default
    top = ['%s_t.nii' % k for k in maps] + ['r2_avg.nii']
    per = ['%s_std.nii' % k for k in maps] + ['r2.nii', 'task_partial_r2.nii']
    assert sorted(os.listdir(str(root))) == sorted(top + ['sA', 'sB'])
    outside = None if run['mask'] is None else ~run['mask'].numpy().astype(bool)
    for i, s in enumerate(('sA', 'sB')):
        assert sorted(os.listdir(str(root / s))) == sorted(per)
        for f in per:
            a = np.asarray(D.read_nifti1(str(root / s / f)))
            assert tuple(a.shape[:3]) == run['img'] and np.isfinite(a).all(), f
            if outside is not None:
                assert (a[outside] == 0).all() and (a[~outside] != 0).any(), f
        want = st.subject_std('task')[i].cpu().numpy().reshape(run['img'])
        np.testing.assert_allclose(np.asarray(D.read_nifti1(str(root / s / 'task_std.nii'))).reshape(run['img']), want, rtol=1e-6, atol=1e-12)
    for f in top:
        a = np.asarray(D.read_nifti1(str(root / f)))
        assert tuple(a.shape[:3]) == run['img'] and np.isfinite(a).all(), f
        if outside is not None:
            assert (a[outside] == 0).all(), f
    np.testing.assert_allclose(np.asarray(D.read_nifti1(str(root / 'r2_avg.nii'))).reshape(-1), st.group_r2().cpu().numpy(), rtol=1e-6, atol=1e-12)
    if not motion:                                               # (one more pass over the loader: seconds on the host build)
        return
    all_maps = R.mk_stat_maps(csv, m, str(tmp_path / 'motion'), run['loader'], mk_motion_maps=True, at_mean=True)
    root2 = tmp_path / 'motion' / 'reconstructions' / root.name
    assert sorted(f for f in os.listdir(str(root2)) if f.endswith('.nii')) == sorted(['%s_t.nii' % k for k in all_maps.keys] + ['r2_avg.nii'])
    assert sorted(os.listdir(str(root2 / 'sA'))) == sorted(['%s_std.nii' % k for k in all_maps.keys] + ['r2.nii'] +
                                                            ['%s_partial_r2.nii' % k for k in all_maps.keys[1:-1]])
