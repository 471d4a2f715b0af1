"""Shared bodies of the float64 tests of the kernels that turn the decoder's logits into the training loss: the GAM/ELBO pair and its
fold kernels (vg_gam.hip: gam_fwd_k, gam_bwd_k, gam_fwd_fold_k, gam_bwd_fold_{gain,eps,total}_k) in the plain, embedded and masked
form, the latent sample / KL and the loss assembly (vg_latent.hip: latent_*_k, loss_*_k), and the one-launch weight packing and
gather that feed every conv (vg_pack_weights, vg_gather_f32).  Run on CPU tensors through the host build of the kernels
(tests/test_gam_emu.py) and on the GPU through libvaegam_hip.so (tests/test_gam_gpu.py).

References are float64 throughout (exp(-eps) too), gradients by autograd.  Every bound is c u M with u = 2^-24, c = 16 for every output
and M a magnitude computed in float64 from the same inputs, never from what the kernel gives.  Notation: s = sigmoid(logits),
cons_i = gain_i s_i, xr = s_0 + sum cons_i, r = x - xr, sigma = exp(-eps), A = |x| + s_0 + sum |cons_i|, df = cons_i - glm_i.
  slp[b]        M = sum_v ( r^2/(2 sigma^2) + |r| A/sigma^2 + |log sigma| + log sqrt(2 pi) )
  dist[i,b]     M = D2/(2 dist) + dist,  D2 = sum_v ( df^2 + 2 |df| (|cons_i| + |glm_i|) );  reference 0 => the kernel's exactly 0
  d_logits      dxr = g_slp r/sigma^2, E = |g_slp|/sigma^2 (|r| + A); covariate: dcons = dxr + g_dist df/dist,
                E += |g_dist| (|cons_i| + |glm_i|)/dist (both extras 0 where dist = 0);  M = |gain_i| s_i ((1 - s_i) E + |dcons|)
                (base map: gain = 1, no extras).  M = 0 (gain 0) asks for an exact 0.
  d_gain[i,b]   M = sum_v s_i (E + |dcons|)
  d_eps[v]      M = sum_b |g_slp| ( r^2/sigma^2 + 2 |r| A/sigma^2 + 1 )
  sum(d_logits) added into the bias buffer:  M = |prefill| + sum of the d_logits M's
  maps          each map to 4 u (|value| + 1), the full reconstruction to (C + 4) u A
  kl[b]         M = ( |log(1 + sum w^2/d)| + sum |log d| + sum d + sum w^2 + sum mu^2 + L ) / 2
  z             M = |mu| + |w eps_w| + |sqrt(d) eps_d|;   d: M = d
  latent grads  M = the sum of the absolute values of their terms ((d - floor) counts as d + floor)
  loss          M = sum |c_k term|;  its gradients M = |g c_k|
That M is honest is asserted on the reference alone: the same GAM formulas evaluated in plain fp32 torch stay within (c/4) u M of the
float64 values in every case (host()).

Cases.  The plain form runs every pair of C in (0, 1, 8, 9, 16) (the edges of gam_bwd_k's CMAX = 8 and 16 instances and of the
forward's 17-column reduction scratch) and B in (1, 7, 8, 9, 17) (BS = min(B, 8): one sample per row, then uneven strides), with V
walking through (1, 63, 255, 256, 257, 1023, 1024, 1025, 2049) (last wave, block and 4-voxel chunk edges of both kernels): 25 cases
in which every C, every B and every V occurs, not the 225 of the full product, which would cost the suite minutes for no further
path.  Every second case prefills the bias buffer with a nonzero value.  Further plain cases: a zero distance (gain[i,b] = 0 and
glm[i] = 0: finite gradients, and the same bits whatever g_dist[i,b] is), saturated sigmoids (logits x 6), g_slp[b] = 0 for one
sample, g_dist all zero.  The embedded and masked forms run the shapes of grid_cases.EMBED_CASES and mask_cases.KERNEL_CASES plus one
C = 16 case each, the reference taken on the native / in-mask voxels and exact zeros required everywhere else.  WS_CASES call the C
ABI with a workspace of exactly vg_gam_ws_bytes filled with NaN and followed by 64 canaries of 777.0: the results must be the bits
of the ops path, the canaries intact.

All cases fit the host build, so GPU_ONLY is empty."""
import math

import numpy as np
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
import grid_cases as GC
import mask_cases as MC

U = 2.0 ** -24
C_BOUND = 16.0
GUARD = 777.0
CANARIES = 64
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)

RECORDS = []                                            # (case, quantity, err / (u M)) of every bounded check made in this process


def _check(what, qty, got, want, M, c=C_BOUND):
    """|got - want| <= c u M per element; an element with M == 0 must be equal.  Prints the worst err / (u M) before it asserts."""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    want = torch.as_tensor(want).detach().double().reshape(-1)
    M = torch.as_tensor(M).detach().double().reshape(-1).expand_as(want)
    assert got.shape == want.shape, (what, qty, got.shape, want.shape)
    if want.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), '%s %s: not finite' % (what, qty)
    err = (got - want).abs()
    ratio = torch.where(M > 0, err / (U * M.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    i = int(ratio.argmax())
    worst = float(ratio[i])
    print('%s %s: worst err/(u M) %.3g at %d (err %.3g, M %.3g, want %.6g)' % (what, qty, worst, i, float(err[i]), float(M[i]), float(want[i])))
    RECORDS.append((what, qty, worst))
    assert worst <= c, '%s %s: error %.3g = %.3g u M at element %d, the bound is %g u M' % (what, qty, float(err[i]), worst, i, c)
    return worst


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- GAM / ELBO cases
def _g(C, B, V=None, form='plain', nat=None, grid=None, mask=None, prefill=0.0, scale=1.0, zero=None, gslp0=None, gdist0=False):
    return dict(C=C, B=B, V=V, form=form, nat=nat, grid=grid, mask=mask, prefill=prefill, scale=scale, zero=zero, gslp0=gslp0, gdist0=gdist0)


CS, BS_, VS = (0, 1, 8, 9, 16), (1, 7, 8, 9, 17), (1, 63, 255, 256, 257, 1023, 1024, 1025, 2049)
PLAIN_CASES = {}
for _k, (_c, _b) in enumerate((c, b) for c in CS for b in BS_):
    PLAIN_CASES['C%d-B%d-V%d' % (_c, _b, VS[_k % 9])] = _g(_c, _b, VS[_k % 9], prefill=(0.0 if _k % 2 == 0 else (-1.0) ** (_k // 2) * (0.75 + _k)))
SPECIAL_CASES = {
    'zero-dist-C8-B9-V257': _g(8, 9, 257, zero=(2, 4), prefill=1.5),
    'zero-dist-C16-B3-V63': _g(16, 3, 63, zero=(15, 2)),
    'saturated-C16-B8-V1025': _g(16, 8, 1025, scale=6.0, prefill=-3.25),
    'saturated-C1-B9-V255': _g(1, 9, 255, scale=6.0),
    'gslp0-C9-B7-V256': _g(9, 7, 256, gslp0=3),
    'gdist0-C8-B8-V1023': _g(8, 8, 1023, gdist0=True, prefill=0.5),
}
EMBED_CASES = {}
for _id, (_n, _gr, _b, _c) in zip(GC.EMBED_IDS, GC.EMBED_CASES):
    EMBED_CASES['embed-' + _id] = _g(_c, _b, form='embed', nat=tuple(_n), grid=tuple(_gr), prefill=(2.5 if _c == 9 else 0.0))
EMBED_CASES['embed-5x6x7_in_6x9x8_B3_C16'] = _g(16, 3, form='embed', nat=(5, 6, 7), grid=(6, 9, 8), prefill=-1.25)
MASKED_CASES = {}
for _id, (_n, _gr, _b, _c, _m) in zip(MC.KERNEL_IDS, MC.KERNEL_CASES):
    MASKED_CASES['masked-' + _id] = _g(_c, _b, form='masked', nat=tuple(_n), grid=tuple(_gr), mask=_m, prefill=(-4.5 if _c == 9 else 0.0))
MASKED_CASES['masked-6x9x8_B3_C16'] = _g(16, 3, form='masked', nat=(6, 9, 8), grid=(6, 9, 8), mask=MC.random_mask, prefill=6.0)
MASKED_CASES['masked-5x6x7_in_6x9x8_B2_C16'] = _g(16, 2, form='masked', nat=(5, 6, 7), grid=(6, 9, 8), mask=MC.random_mask)
GAM_CASES = dict(PLAIN_CASES); GAM_CASES.update(SPECIAL_CASES); GAM_CASES.update(EMBED_CASES); GAM_CASES.update(MASKED_CASES)
# the C ABI with a workspace of exactly vg_gam_ws_bytes: both CMAX instances of the plain and of the embedded form, one masked
WS_CASES = ('C8-B17-V1023', 'C16-B17-V1024', 'C0-B7-V63', 'C1-B9-V2049', 'embed-9x4x33_in_9x6x34_C9', 'embed-5x6x7_in_6x9x8_C1',
            'masked-9x4x33_in_9x6x34_B9_C9')
assert all(c in GAM_CASES for c in WS_CASES)
# cases the host build cannot afford (a fifth of the cases at the most; test_gam_emu names what each alone reaches)
GPU_ONLY = ()
assert len(GPU_ONLY) * 5 <= len(GAM_CASES)


def instance(cid):
    """-> (CMAX of gam_bwd_k, EMB, MSK) of the kernels the case launches (vg_gam.hip: gam_fwd / gam_bwd)"""
    sp = GAM_CASES[cid]
    emb = sp['form'] == 'embed' or (sp['form'] == 'masked' and sp['nat'] != sp['grid'])
    return (8 if sp['C'] <= 8 else 16, emb, sp['form'] == 'masked')


def check_coverage():
    """Every (CMAX, EMB, MSK) instance of gam_bwd_k and every (EMB, MSK) instance of gam_fwd_k is launched by a listed case, C = 16
    runs in the plain, the embedded and the masked form, and every C, B and V the plain matrix is there for occurs in it."""
    by = {}
    for cid in GAM_CASES:
        by.setdefault(instance(cid), []).append(cid)
    missing = [(cm, e, m) for cm in (8, 16) for e in (False, True) for m in (False, True) if (cm, e, m) not in by]
    for k in sorted(by):
        print('gam_bwd_k<%d, %s, %s> / gam_fwd_k<%s, %s>: %s' % (k + k[1:] + (', '.join(by[k]),)))
    assert not missing, 'no case launches gam_bwd_k<CMAX, EMB, MSK> = %r' % missing
    gpu_only = sorted(k for k, v in by.items() if all(c in GPU_ONLY for c in v))
    for form in ('plain', 'embed', 'masked'):
        assert any(sp['form'] == form and sp['C'] == 16 for sp in GAM_CASES.values()), 'no C = 16 case in the %s form' % form
    for vals, key in ((CS, 'C'), (BS_, 'B'), (VS, 'V')):
        assert {sp[key] for sp in PLAIN_CASES.values()} == set(vals), key
    assert len(PLAIN_CASES) == 25 and sum(1 for sp in GAM_CASES.values() if sp['prefill'] != 0.0) >= 3
    return dict(instances=by, gpu_only=gpu_only)


# ---------------------------------------------------------------------------------------------------------------- GAM / ELBO reference
def _gam_math(dt, lg, gn, x, eps, glm, g1, g2):
    """The operation on the voxels that count.  lg [G,B,Vs] and gn [C,B] in dt, eps [Vs] float64 (sigma = exp(-eps) is formed in float64
    and cast, as the kernels do; in float64 the cast is none).  -> s, cons, xr, slp, dist, the scalar whose gradients are wanted.
    A zero distance has the gradient 0."""
    s = torch.sigmoid(lg)
    cons = gn[:, :, None] * s[1:]
    xr = s[0] + cons.sum(0)
    sig = torch.exp(-eps).to(dt)
    r = x.to(dt) - xr
    lp = -(r * r) / (2 * sig * sig) - torch.log(sig) - LOG_SQRT_2PI
    slp = lp.sum(1)
    df = cons - glm.to(dt)[:, None, :]
    d2 = (df * df).sum(2)
    pos = d2 > 0
    dist = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    obj = (slp * g1.to(dt)).sum() + (dist * g2.to(dt)).sum()
    return s, cons, xr, slp, dist, obj


def _gam_eval(dt, sel, g2):
    """-> dict of slp, dist, d_logits, d_gain, d_eps (None without covariates), s, cons, xr -- all detached, in dt (d_eps float64)"""
    lg = sel['logits'].to(dt).requires_grad_(True); gn = sel['gain'].to(dt).requires_grad_(True); ep = sel['eps'].clone().requires_grad_(True)
    s, cons, xr, slp, dist, obj = _gam_math(dt, lg, gn, sel['x'], ep, sel['glm'], sel['g1'], g2)
    C = gn.shape[0]
    gr = torch.autograd.grad(obj, [lg, ep] + ([gn] if C > 0 else []))
    return dict(slp=slp.detach(), dist=dist.detach(), d_logits=gr[0], d_eps=gr[1], d_gain=gr[2] if C > 0 else torch.zeros(0, lg.shape[1], dtype=dt),
                s=s.detach(), cons=cons.detach(), xr=xr.detach())


def _gam_bounds(ref, sel, g2, prefill):
    """the magnitudes M of the module docstring, in float64 from the float64 reference's own intermediates"""
    s, cons, xr, dist = ref['s'], ref['cons'], ref['xr'], ref['dist']
    x, glm, gain, g1 = sel['x'].double(), sel['glm'].double(), sel['gain'].double(), sel['g1'].double()
    g2 = g2.double()
    sig = torch.exp(-sel['eps']); iv = 1.0 / (sig * sig)
    r = x - xr
    A = x.abs() + s[0] + cons.abs().sum(0)
    M = dict(A=A)
    M['slp'] = (r * r * iv / 2 + r.abs() * A * iv + torch.log(sig).abs() + LOG_SQRT_2PI).sum(1)
    df = cons - glm[:, None, :]
    cg = cons.abs() + glm.abs()[:, None, :]
    D2 = (df * df + 2 * df.abs() * cg).sum(2)
    pos = dist > 0
    sd = torch.where(pos, dist, torch.ones_like(dist))
    M['dist'] = torch.where(pos, D2 / (2 * sd) + dist, torch.zeros_like(dist))
    dxr = g1[:, None] * r * iv
    E = g1.abs()[:, None] * iv * (r.abs() + A)
    w = torch.where(pos, 1.0 / sd, torch.zeros_like(dist))
    dcons = dxr[None] + (g2 * w)[:, :, None] * df
    Ei = E[None] + (g2.abs() * w)[:, :, None] * cg
    M0 = s[0] * ((1 - s[0]) * E + dxr.abs())
    Mi = gain.abs()[:, :, None] * s[1:] * ((1 - s[1:]) * Ei + dcons.abs())
    M['d_logits'] = torch.cat([M0[None], Mi], 0)
    M['d_gain'] = (s[1:] * (Ei + dcons.abs())).sum(2)
    M['d_eps'] = (g1.abs()[:, None] * (r * r * iv + 2 * r.abs() * A * iv + 1)).sum(0)
    M['dl_sum'] = float(M['d_logits'].sum())
    M['total'] = abs(prefill) + M['dl_sum']
    return M


def _selection(sp):
    """-> (Vg, Vn, sel_g, sel_n): the voxels that count as indices into the logits' grid and into the native tensors"""
    if sp['form'] == 'plain':
        V = sp['V']
        a = torch.arange(V)
        return V, V, a, a
    nat, grid = sp['nat'], sp['grid']
    Vg, Vn = int(np.prod(grid)), int(np.prod(nat))
    d, h, w = torch.meshgrid(torch.arange(nat[0]), torch.arange(nat[1]), torch.arange(nat[2]), indexing='ij')
    gidx = ((d * grid[1] + h) * grid[2] + w).reshape(-1)
    sel_n = torch.arange(Vn)
    if sp['form'] == 'masked':
        sel_n = sel_n[sp['mask'](nat).reshape(-1).bool()]
    return Vg, Vn, gidx[sel_n], sel_n


_HOST = {}


def host(cid):
    """The case's inputs, its float64 reference and bounds, computed once and shared (read-only) by every test that runs the case.
    Asserts that the fp32 evaluation of the reference's own formulas stays within (c/4) u M."""
    if cid in _HOST:
        return _HOST[cid]
    sp = GAM_CASES[cid]
    C, B = sp['C'], sp['B']
    Vg, Vn, sel_g, sel_n = _selection(sp)
    g = torch.Generator().manual_seed(7000 + list(GAM_CASES).index(cid))
    logits = torch.randn(C + 1, B, Vg, generator=g) * sp['scale']
    gain = torch.randn(C, B, generator=g)
    x = torch.rand(B, Vn, generator=g)
    eps = -math.log(10) + 0.3 * torch.randn(Vn, generator=g, dtype=torch.float64)
    glm = torch.rand(C, Vn, generator=g)
    g1 = torch.randn(B, generator=g); g2 = torch.randn(C, B, generator=g)
    if sp['zero'] is not None:
        i, b = sp['zero']
        gain[i, b] = 0.0; glm[i] = 0.0
    if sp['gslp0'] is not None:
        g1[sp['gslp0']] = 0.0
    if sp['gdist0']:
        g2.zero_()
    h = dict(sp=sp, Vg=Vg, Vn=Vn, sel_g=sel_g, sel_n=sel_n, logits=logits, gain=gain, x=x, eps=eps, glm=glm, g1=g1, g2=g2,
             mask=(sp['mask'](sp['nat']) if sp['form'] == 'masked' else None))
    sel = dict(logits=logits[:, :, sel_g], gain=gain, x=x[:, sel_n], eps=eps[sel_n], glm=glm[:, sel_n], g1=g1)
    ref = _gam_eval(torch.float64, sel, g2)
    M = _gam_bounds(ref, sel, g2, sp['prefill'])
    if sp['zero'] is not None:
        i, b = sp['zero']
        assert float(ref['dist'][i, b]) == 0.0 and bool((ref['dist'] > 0).sum() == C * B - 1)
    else:
        assert bool((ref['dist'] > 0).all())
    f32 = _gam_eval(torch.float32, sel, g2)
    for q in ('slp', 'dist', 'd_logits', 'd_gain', 'd_eps'):
        _check(cid + ' [reference in fp32]', q, f32[q], ref[q], M[q], c=C_BOUND / 4)
    _check(cid + ' [reference in fp32]', 'total', f32['d_logits'].sum(), ref['d_logits'].sum(), M['dl_sum'], c=C_BOUND / 4)
    h.update(sel=sel, ref=ref, M=M, total=sp['prefill'] + float(ref['d_logits'].sum()))
    _HOST[cid] = h
    return h


# ---------------------------------------------------------------------------------------------------------------- GAM / ELBO on the device
def _bias(dev, prefill):
    b = torch.nn.Parameter(torch.zeros(1, device=dev))
    b.grad = torch.full_like(b, prefill)
    return b


def _apply(dev, h, g2):
    """forward and backward through the autograd node of the case's form -> dict of CPU tensors"""
    sp = h['sp']
    C = sp['C']
    dv = [h['logits'].to(dev).clone().requires_grad_(True), h['gain'].to(dev).clone().requires_grad_(True), h['x'].to(dev),
          h['eps'].to(dev).clone().requires_grad_(True), h['glm'].to(dev)]
    lb = _bias(dev, sp['prefill'])
    if sp['form'] == 'plain':
        slp, dist = ops.GamElbo.apply(*dv, lb)
    elif sp['form'] == 'embed':
        slp, dist = ops.GamElboEmbed.apply(*dv, sp['nat'], sp['grid'], lb)
    else:
        slp, dist = ops.GamElboMasked.apply(*dv, h['mask'].to(dev), sp['nat'], sp['grid'], lb)
    gd = torch.autograd.grad((slp * h['g1'].to(dev)).sum() + (dist * g2.to(dev)).sum(), [dv[0], dv[3]] + ([dv[1]] if C > 0 else []))
    _sync(dev)
    return dict(slp=slp.detach().cpu(), dist=dist.detach().cpu(), d_logits=gd[0].cpu(), d_eps=gd[1].cpu(),
                d_gain=(gd[2].cpu() if C > 0 else torch.zeros(0, sp['B'])), total=lb.grad.detach().cpu().clone(), dv=dv)


def _rest(t, sel, dim_size):
    keep = torch.ones(dim_size, dtype=torch.bool); keep[sel] = False
    return t[..., keep]


_RUN = {}


def run_gam(dev, cid):
    """The case through ops.GamElbo / GamElboEmbed / GamElboMasked with a bound, prefilled bias buffer, and through ops.gam_maps:
    every output against the float64 reference within 16 u M, exact zeros wherever a voxel does not count.  -> the outputs (CPU),
    kept per device for the workspace cases."""
    if (dev, cid) in _RUN:
        return _RUN[(dev, cid)]
    h = host(cid)
    sp, ref, M = h['sp'], h['ref'], h['M']
    C, B, Vg, Vn, sel_g, sel_n = sp['C'], sp['B'], h['Vg'], h['Vn'], h['sel_g'], h['sel_n']
    out = _apply(dev, h, h['g2'])
    assert out['slp'].dtype == torch.float32 and out['d_eps'].dtype == torch.float64
    _check(cid, 'slp', out['slp'], ref['slp'], M['slp'])
    zero = ref['dist'] == 0
    assert torch.equal(out['dist'][zero], torch.zeros(int(zero.sum()))), cid + ': a zero distance must come out as exactly 0'
    _check(cid, 'dist', out['dist'], ref['dist'], M['dist'])
    _check(cid, 'd_logits', out['d_logits'][:, :, sel_g], ref['d_logits'], M['d_logits'])
    _check(cid, 'd_gain', out['d_gain'], ref['d_gain'], M['d_gain'])
    _check(cid, 'd_eps', out['d_eps'][sel_n], ref['d_eps'], M['d_eps'])
    _check(cid, 'total', out['total'], h['total'], M['total'])
    outside = _rest(out['d_logits'], sel_g, Vg)
    assert outside.numel() == (C + 1) * B * (Vg - len(sel_g))
    assert torch.equal(outside, torch.zeros_like(outside)), cid + ': d_logits must be exactly zero at every voxel that does not count'
    outside = _rest(out['d_eps'], sel_n, Vn)
    assert torch.equal(outside, torch.zeros_like(outside)), cid + ': d_eps must be exactly 0.0 outside the mask'
    if sp['zero'] is not None:
        # gain 0 against a zero GLM map: the pair's distance term contributes exactly nothing -- the same bits under any g_dist[i,b]
        i, b = sp['zero']
        assert torch.equal(out['d_logits'][i + 1, b], torch.zeros(Vg))
        g2b = h['g2'].clone(); g2b[i, b] = 1000.0 - g2b[i, b]
        again = _apply(dev, h, g2b)
        for q in ('slp', 'dist', 'd_logits', 'd_gain', 'd_eps', 'total'):
            assert torch.equal(out[q], again[q]), '%s: %s depends on g_dist[%d,%d] although that distance is 0' % (cid, q, i, b)
    # maps, on a destination that held something else
    dv = out.pop('dv')
    torch.full((C + 2, B, Vn), 7.0, device=dev)
    kw = {} if sp['form'] == 'plain' else dict(nat=sp['nat'], grid=sp['grid'])
    if sp['form'] == 'masked':
        kw['mask'] = h['mask'].to(dev)
    maps = ops.gam_maps(dv[0].detach(), dv[1].detach(), dv[2], dv[3].detach(), dv[4], **kw).cpu()
    assert maps.shape == (C + 2, B, Vn)
    outside = _rest(maps, sel_n, Vn)
    assert torch.equal(outside, torch.zeros_like(outside)), cid + ': maps must be exactly zero outside the mask'
    m = maps[:, :, sel_n]
    want = torch.cat([ref['s'][:1], ref['cons']], 0)
    _check(cid, 'maps', m[:C + 1], want, 4 * (want.abs() + 1), c=1.0)
    _check(cid, 'maps full', m[C + 1], ref['xr'], (C + 4) * M['A'], c=1.0)
    out['maps'] = maps
    _RUN[(dev, cid)] = out
    return out


def run_gam_workspace(dev, cid):
    """The C ABI (vg_gam_elbo_fwd / _bwd, their _embed and _masked twins) with a workspace of exactly vg_gam_ws_bytes, filled with NaN
    before each call and followed by 64 canaries: forward, then backward with the total requested (added into a prefilled buffer, and
    once more overwriting it).  The results are the bits of the ops path (which run_gam holds to float64), so nothing was read before
    it was written; the canaries are intact."""
    h = host(cid)
    sp, M = h['sp'], h['M']
    C, B, Vg, Vn = sp['C'], sp['B'], h['Vg'], h['Vn']
    want = run_gam(dev, cid)
    lib = _lib.get_lib()
    nbytes = lib.size('vg_gam_ws_bytes', C, B, Vg)
    assert nbytes > 0 and nbytes % 4 == 0
    n = nbytes // 4
    nan = float('nan')
    ws = torch.cat([torch.full((n,), nan), torch.full((CANARIES,), GUARD)]).to(dev)
    p = ops._p
    T = [h['logits'].to(dev), h['gain'].to(dev), h['x'].to(dev), h['eps'].to(dev), h['glm'].to(dev)]
    g1, g2 = h['g1'].to(dev), h['g2'].to(dev)
    slp = torch.full((B,), nan, device=dev); dist = torch.full((C, B), nan, device=dev)
    d_logits = torch.full((C + 1, B, Vg), nan, device=dev); d_gain = torch.full((C, B), nan, device=dev)
    d_eps = torch.full((Vn,), nan, dtype=torch.float64, device=dev)
    tot = torch.full((1,), sp['prefill'], device=dev)
    form = sp['form']
    sfx = {'plain': '', 'embed': '_embed', 'masked': '_masked'}[form]
    geo = (Vg,) if form == 'plain' else (ops._i3(sp['nat']), ops._i3(sp['grid']))
    md = h['mask'].reshape(-1).to(dev) if form == 'masked' else None     # (kept alive for the calls)
    mk = (p(md),) if form == 'masked' else ()

    def canaries(when):
        assert torch.equal(ws[n:].cpu(), torch.full((CANARIES,), GUARD)), '%s: wrote past vg_gam_ws_bytes (%s)' % (cid, when)
    ops._call(T[2], 'vg_gam_elbo_fwd' + sfx, *[p(t) for t in T], *mk, C, B, *geo, p(ws), p(slp), p(dist), None)
    _sync(dev)
    canaries('forward')
    assert torch.equal(slp.cpu(), want['slp']) and torch.equal(dist.cpu(), want['dist']), cid + ': forward differs from the ops path'
    for accumulate in (1, 0):
        ws[:n] = nan
        ops._call(T[2], 'vg_gam_elbo_bwd' + sfx, *[p(t) for t in T], *mk, p(dist), p(g1), p(g2), C, B, *geo, p(ws), p(d_logits), p(d_gain),
                  p(d_eps), p(tot), accumulate)
        _sync(dev)
        canaries('backward')
        assert torch.equal(d_logits.cpu(), want['d_logits']) and torch.equal(d_eps.cpu(), want['d_eps']), cid + ': backward differs from the ops path'
        assert torch.equal(d_gain.cpu(), want['d_gain'])
        if accumulate:
            assert torch.equal(tot.cpu(), want['total']), (cid, float(tot), float(want['total']))
            tot.fill_(5.0)
        else:
            _check(cid + ' [ws]', 'total, overwritten', tot, h['total'] - sp['prefill'], M['dl_sum'])


# ---------------------------------------------------------------------------------------------------------------- latent sample and KL
# id: (B, L, G, floor flag: 'clear', 'set' (an exp(a) < 1e-6 in the middle of the batch), 'last' (in the last row only))
LATENT_CASES = {
    'B1-L1-G1': (1, 1, 1, 'clear'), 'B1-L70-G9-set': (1, 70, 9, 'set'), 'B4-L32-G9-set': (4, 32, 9, 'set'), 'B5-L64-G17': (5, 64, 17, 'clear'),
    'B5-L65-G1-last': (5, 65, 1, 'last'), 'B256-L65-G1': (256, 65, 1, 'clear'), 'B256-L32-G9-last': (256, 32, 9, 'last'),
    'B257-L70-G9': (257, 70, 9, 'clear'), 'B257-L1-G17-set': (257, 1, 17, 'set'), 'B1040-L32-G17-last': (1040, 32, 17, 'last'),
    'B1040-L70-G1': (1040, 70, 1, 'clear'), 'B1040-L64-G9-set': (1040, 64, 9, 'set'),
}
LATENT_NULL_CASES = ('B4-L32-G9-set', 'B257-L70-G9', 'B1040-L32-G17-last')

_LHOST = {}


def _latent_ref(h, use_gz, use_gk):
    """float64 restatement of kernel_cases.ref_latent's formulas -> outputs, gradients and magnitudes"""
    B, L, G = h['B'], h['L'], h['G']
    mu, w, a = (h[k].double().requires_grad_(True) for k in ('mu', 'w', 'a'))
    ew, ed = h['eps_w'].double().view(B, 1), h['eps_d'].double()
    ea = torch.exp(a)
    fl = 1e-6 if bool((ea < 1e-6).any()) else 0.0
    d = ea + fl
    z = mu + w * ew + d.sqrt() * ed
    cap = 1 + (w * w / d).sum(1)
    kl = 0.5 * (-torch.log(cap) - torch.log(d).sum(1) + d.sum(1) + (w * w).sum(1) + (mu * mu).sum(1) - L)
    oh = torch.eye(G, dtype=torch.float64).unsqueeze(1).expand(G, B, G)
    zcat = torch.cat([z.unsqueeze(0).expand(G, B, L), oh], 2).reshape(G * B, L + G)
    gz = h['gz'].double() * (1.0 if use_gz else 0.0); gk = h['gk'].double() * (1.0 if use_gk else 0.0)
    gr = torch.autograd.grad((zcat * gz).sum() + (kl * gk).sum(), [mu, w, a], allow_unused=True)
    gr = [t if t is not None else torch.zeros(B, L, dtype=torch.float64) for t in gr]
    with torch.no_grad():
        gza = gz.view(G, B, L + G)[:, :, :L].abs().sum(0); gka = gk.abs()[:, None]; cp = cap[:, None]
        M = dict(kl=0.5 * (torch.log(cap).abs() + torch.log(d).abs().sum(1) + d.sum(1) + (w * w).sum(1) + (mu * mu).sum(1) + L),
                 z=mu.abs() + (w * ew).abs() + (d.sqrt() * ed).abs(), d=d.clone(),
                 g_mu=gza + gka * mu.abs(), g_w=gza * ew.abs() + gka * (w.abs() + w.abs() / (d * cp)),
                 g_a=(gza * ed.abs() * 0.5 / d.sqrt() + gka * 0.5 * (w * w / (d * d * cp) + 1 / d + 1)) * (d + fl))
    return dict(fl=fl, z=z.detach(), kl=kl.detach(), d=d.detach(), zcat=zcat.detach(), g_mu=gr[0], g_w=gr[1], g_a=gr[2], M=M)


def latent_host(cid):
    if cid in _LHOST:
        return _LHOST[cid]
    B, L, G, flag = LATENT_CASES[cid]
    g = torch.Generator().manual_seed(8000 + list(LATENT_CASES).index(cid))
    mu = torch.randn(B, L, generator=g); w = 0.5 * torch.randn(B, L, generator=g); a = 0.7 * torch.randn(B, L, generator=g) - 0.5
    if flag == 'set':
        a[B // 2, L // 3] = -15.0
    elif flag == 'last':
        a[B - 1, L - 1] = -15.0
    h = dict(B=B, L=L, G=G, mu=mu, w=w, a=a, eps_w=torch.randn(B, 1, generator=g), eps_d=torch.randn(B, L, generator=g),
             gz=torch.randn(G * B, L + G, generator=g), gk=torch.randn(B, generator=g))
    h['ref'] = _latent_ref(h, True, True)
    assert (h['ref']['fl'] > 0) == (flag != 'clear')
    assert float((torch.exp(a.double()) / 1e-6 - 1).abs().min()) > 0.1          # no element near the threshold: fp32 and float64 agree on the flag
    _LHOST[cid] = h
    return h


def _check_latent(what, got, ref):
    M = ref['M']
    for q in ('g_mu', 'g_w', 'g_a'):
        _check(what, q, got[q], ref[q], M[q])


def run_latent(dev, cid):
    """ops.LatentSample against float64 within 16 u M (forward and gradients), the one-hot columns and the G copies of z exact, and
    ops.LatentSampleStacked bit-equal to it in every output and gradient."""
    h = latent_host(cid)
    B, L, G, ref = h['B'], h['L'], h['G'], h['ref']
    M = ref['M']
    dv = [h[k].to(dev).clone().requires_grad_(True) for k in ('mu', 'w', 'a')]
    ew, ed, gz, gk = (h[k].to(dev) for k in ('eps_w', 'eps_d', 'gz', 'gk'))
    zc, kl, d = ops.LatentSample.apply(*dv, ew, ed, G)
    gd = torch.autograd.grad((zc * gz).sum() + (kl * gk).sum(), dv)
    _sync(dev)
    zc3 = zc.detach().cpu().view(G, B, L + G)
    assert torch.equal(zc3[:, :, L:], torch.eye(G).unsqueeze(1).expand(G, B, G)), cid + ': the one-hot columns'
    assert torch.equal(zc3[:, :, :L], zc3[:1, :, :L].expand(G, B, L)), cid + ': the G copies of z differ'
    _check(cid, 'z', zc3[0, :, :L], ref['z'], M['z'])
    _check(cid, 'kl', kl, ref['kl'], M['kl'])
    _check(cid, 'd', d, ref['d'], M['d'])
    _check_latent(cid, dict(zip(('g_mu', 'g_w', 'g_a'), gd)), ref)
    mwa = torch.stack([h[k] for k in ('mu', 'w', 'a')]).to(dev).requires_grad_(True)
    zs, ks, ds = ops.LatentSampleStacked.apply(mwa, ew, ed, G)
    gs, = torch.autograd.grad((zs * gz).sum() + (ks * gk).sum(), [mwa])
    _sync(dev)
    assert torch.equal(zs.detach(), zc.detach()) and torch.equal(ks.detach(), kl.detach()) and torch.equal(ds, d), cid + ': LatentSampleStacked forward'
    for i, q in enumerate(('g_mu', 'g_w', 'g_a')):
        assert torch.equal(gs[i], gd[i]), '%s: LatentSampleStacked %s' % (cid, q)


def run_latent_null(dev, cid):
    """vg_latent_bwd with g_zcat, g_kl or both absent (null pointers): the absent gradient counts as zero."""
    h = latent_host(cid)
    B, L, G = h['B'], h['L'], h['G']
    p = ops._p
    T = {k: h[k].to(dev) for k in ('mu', 'w', 'a', 'eps_w', 'eps_d', 'gz', 'gk')}
    zcat = torch.empty(G * B, L + G, device=dev); kl = torch.empty(B, device=dev); d = torch.empty(B, L, device=dev); flag = torch.empty(1, device=dev)
    ops._call(T['mu'], 'vg_latent_fwd', p(T['mu']), p(T['w']), p(T['a']), p(T['eps_w']), p(T['eps_d']), B, L, G, p(zcat), p(kl), p(d), p(flag))
    _sync(dev)
    assert (float(flag) > 0) == (h['ref']['fl'] > 0), cid + ': the floor flag'
    for use_gz, use_gk in ((False, True), (True, False), (False, False)):
        ref = _latent_ref(h, use_gz, use_gk)
        out = [torch.full((B, L), float('nan'), device=dev) for _ in range(3)]
        ops._call(T['mu'], 'vg_latent_bwd', p(T['mu']), p(T['w']), p(d), p(flag), p(T['eps_w']), p(T['eps_d']), p(T['gz']) if use_gz else None,
                  p(T['gk']) if use_gk else None, B, L, G, p(out[0]), p(out[1]), p(out[2]))
        _sync(dev)
        _check_latent('%s [g_zcat %s, g_kl %s]' % (cid, 'given' if use_gz else 'null', 'given' if use_gk else 'null'),
                      dict(zip(('g_mu', 'g_w', 'g_a'), out)), ref)


# ---------------------------------------------------------------------------------------------------------------- loss assembly
# id: (B, C): dist is [C, B], so C B runs from 0 to 16 x 4,096
LOSS_CASES = {'B1-C0': (1, 0), 'B255-C3': (255, 3), 'B256-C0': (256, 0), 'B257-C16': (257, 16), 'B4096-C0': (4096, 0), 'B4096-C16': (4096, 16)}


def run_loss(dev, cid):
    """ops.ElboLoss against a float64 sum, M = sum |c_k term|; every gradient element against g c_k."""
    B, C = LOSS_CASES[cid]
    g = torch.Generator().manual_seed(9000 + list(LOSS_CASES).index(cid))
    kl = torch.rand(B, generator=g) * 30; slp = -1e4 * torch.rand(B, generator=g); dist = torch.rand(C, B, generator=g) * 50
    gp = torch.rand(1, generator=g) * 100; go = torch.randn(1, generator=g)
    coef = (1.0 / B, -1.0 / B, 0.37, 1e-3 * B)
    terms = [coef[0] * kl.double(), coef[1] * slp.double(), coef[2] * gp.double(), coef[3] * dist.double().reshape(-1)]
    want = sum(t.sum() for t in terms); M = sum(t.abs().sum() for t in terms)
    dv = [t.to(dev).clone().requires_grad_(True) for t in (kl, slp, dist, gp)]
    loss = ops.ElboLoss.apply(*dv, coef)
    assert loss.shape == (1,)
    gd = torch.autograd.grad(loss, dv, grad_outputs=go.to(dev))
    _sync(dev)
    _check(cid, 'loss', loss, want, M)
    for t, src, k, q in zip(gd, dv, (0, 1, 3, 2), ('g_kl', 'g_slp', 'g_dist', 'g_gp')):
        assert t.shape == src.shape
        w = float(go.double()) * coef[k]
        _check(cid, q, t, torch.full(t.shape, w, dtype=torch.float64), abs(w))


# ---------------------------------------------------------------------------------------------------------------- weight packing, gather
def _many():
    shapes = [('conv', 2, 3, (3, 3, 3), 1), ('convt', 3, 2, (3, 3, 3), 2), ('conv', 1, 5, (5, 3, 3), 2), ('convt', 2, 1, (5, 3, 3), 1), ('conv', 3, 3, (3, 3, 3), 2)]
    return [shapes[i % 5] for i in range(36)]


# id: [(kind, ci, co, kernel, stride)]; every layer is packed in both directions, as ops.PackedWeights does
PACK_TABLES = {
    # every mode with kernel volumes 27 and 45; sizes 405, 945, 675, 405, 270, 54: none a multiple of 4
    'modes': [('conv', 5, 3, (3, 3, 3), 1), ('conv', 3, 7, (5, 3, 3), 2), ('convt', 5, 3, (5, 3, 3), 2), ('convt', 3, 5, (3, 3, 3), 1),
              ('convt', 2, 3, (5, 3, 3), 1), ('conv', 1, 2, (3, 3, 3), 2)],
    'many': _many(),                                                     # 72 segments > 64: the table is searched in global memory
    # 6 x 46,035 = 276,210 elements > 1,024 blocks x 256 threads: the grid-stride loop iterates
    'big': [('conv', 33, 31, (5, 3, 3), 1), ('convt', 33, 31, (5, 3, 3), 2), ('convt', 31, 33, (5, 3, 3), 1)],
}


def pack_table(tid):
    """-> (layers [(spec, weight shape, source offset)], segment rows as ops.PackedWeights builds them, source length, destination length)"""
    layers, segs, src, dst = [], [], 1, 0
    for k, (kind, ci, co, kern, stride) in enumerate(PACK_TABLES[tid]):
        spec = ops.ConvSpec(kind, ci, co, kern, stride)
        shape = ((co, ci) if kind == 'conv' else (ci, co)) + tuple(kern)
        n = int(np.prod(shape))
        layers.append((spec, shape, src))
        for direction in ('fwd', 'bwd'):
            segs.append([src, dst, shape[0], shape[1], int(np.prod(kern)), ops.pack_mode(spec, direction), n, 0])
            dst += ((n + 3) // 4) * 4
        src += n + k % 3                                                  # sources at every alignment
    return layers, segs, src, dst


def run_pack(dev, tid):
    """vg_pack_weights, one launch over the whole table, bit for bit against ops.pack_weight per layer and direction; the alignment
    gaps behind the segments and 64 elements behind the buffer keep their 777.0."""
    layers, segs, nsrc, total = pack_table(tid)
    modes = {(s[5], s[4]) for s in segs}
    if tid == 'modes':
        assert modes == {(m, kv) for m in (0, 1, 2) for kv in (27, 45)} and all(s[6] % 4 for s in segs)
    if tid == 'many':
        assert len(segs) > 64
    if tid == 'big':
        assert total > 262144
    g = torch.Generator().manual_seed(9500 + list(PACK_TABLES).index(tid))
    flat = torch.randn(nsrc, generator=g)
    packed = torch.full((total + CANARIES,), GUARD).to(dev)
    fd = flat.to(dev); sd = torch.tensor(segs, dtype=torch.int64).to(dev)
    ops._call(fd, 'vg_pack_weights', ops._p(fd), ops._p(packed), ops._p(sd), len(segs), total)
    _sync(dev)
    got = packed.cpu()
    want = torch.full((total + CANARIES,), GUARD)
    it = iter(segs)
    for spec, shape, off in layers:
        w = flat[off:off + int(np.prod(shape))].view(shape)
        for direction in ('fwd', 'bwd'):
            s = next(it)
            want[s[1]:s[1] + s[6]] = ops.pack_weight(w, spec, direction).reshape(-1)
    bad = (got != want).nonzero().reshape(-1)
    assert bad.numel() == 0, '%s: %d elements differ, the first at %d (segment rows: src, dst, d0, d1, kvol, mode, n)' % (tid, bad.numel(), int(bad[0]))


GATHER_CASES = {'n1': 1, 'n257': 257, 'n300001': 300001}                 # the last: more than 1,024 blocks x 256 threads


def run_gather(dev, gid):
    """vg_gather_f32 bit for bit against plain indexing, an index of -1 giving 0; 64 elements behind dst keep their 777.0."""
    n = GATHER_CASES[gid]
    g = torch.Generator().manual_seed(9700 + n)
    src = torch.randn(5000, generator=g)
    idx = torch.randint(0, 5000, (n,), generator=g, dtype=torch.int32)
    idx[torch.rand(n, generator=g) < 0.1] = -1
    idx[n - 1] = -1; idx[0] = 4999 if n > 1 else -1
    dst = torch.full((n + CANARIES,), GUARD).to(dev)
    sd, idd = src.to(dev), idx.to(dev)
    ops._call(sd, 'vg_gather_f32', ops._p(sd), ops._p(idd), ops._p(dst), n)
    _sync(dev)
    want = torch.cat([torch.where(idx >= 0, src[idx.clamp_min(0).long()], torch.zeros(n)), torch.full((CANARIES,), GUARD)])
    assert torch.equal(dst.cpu(), want), gid
