"""The gain block (vg_gp.hip) against float64: ONE input builder, ONE runner and the case matrix, chosen from the library's own plan
query (ops.gain_plan / vg_gp_gain_plan).  Shared by the host build (tests/test_gain_emu.py) and the MI355X (tests/test_gain_gpu.py);
the older gain tests (test_kernels_*, test_gain_large_batch_*) build their inputs here too.  DESIGN 4.5 has the table and the numbers.

Inputs (build_inputs):
  * every GP covariate has its OWN inducing grid (grid g = linspace(-4.1 + 0.3 g, 6.2 + 0.5 g, n)), and `gp_order` lets the table's
    gp_index run against the covariate order: a kernel that read row 0 of xu for every covariate, or the rows in covariate order, fails;
  * any `kinds` tuple: C = 1, no GP covariate at all (xu = None), B = 1 (the two extreme covariate rows are set only when B >= 2);
  * the covariate matrix has two more columns than covariates (ld_cov != C);
  * the gain parameters lie in a flat buffer BETWEEN guard segments that stand for the network's other parameters, and the gradient
    buffer is prefilled with random fp32 values: the backward must ADD, and only inside the parameters' own segments.
Reference (reference): the float64 restatement of vae_reg_GP.py:345-378 / gp.py:41-110 with autograd.  jitter 0: the posterior with the
inducing-to-query distances rounded to fp32 (posterior_fp32_distances), which is what the original (gp.py:90) and the kernel do at
jitter 0; jitter > 0: the plain oracle, gradients through kernel_cases._posterior_unit_variance, cross-checked against the oracle.
Bands (the project's own, run_case): gains 2e-6 of the largest gain, KL 1e-6 relative, f_bar and Sigma 2e-5 absolute, gradients
rtol 2e-4 with atol 2e-4 x scale (x `grow` on d logkvar / d log_ls: 1 for every case listed here, B / 32 for the older tests)."""
import ctypes
import functools
import types

import numpy as np
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
import kernel_cases as K

DEFAULT_KINDS = ('lin_hrf', 'gp', 'gp', 'gp_hrf', 'lin')
MIXED_KINDS = ('gp_hrf', 'lin', 'gp')          # GP first and last; run with the table's gp_index against the covariate order
NO_GP_KINDS = ('lin', 'lin_hrf')
LDS_LIMIT = 163840                             # the 160 KB of LDS of a CDNA4 workgroup
GRAD_NAMES = ('sa', 'logstd', 'qu_m', 'qu_S', 'logkvar', 'log_ls')


def inducing_grid(g, n):
    """the inducing grid of GP number g (row g of xu): no two alike"""
    return torch.linspace(-4.1 + 0.3 * g, 6.2 + 0.5 * g, n)


def build_inputs(B, n=6, seed=0, kinds=DEFAULT_KINDS, jitter=0.0, gp_order=None):
    """-> namespace of CPU tensors: table (C x 10 int64), xu (#gp x n or None), flat (parameters between guards), guard (bool mask of
    flat), prefill (what the gradient buffer holds before the backward), cov (B x (C + 2)), eps, wt (C x B), wk, leaves (per covariate:
    name -> fp32 tensor), kinds, n, jitter.  gp_order[j] = the gp_index of the j-th GP covariate (default: covariate order)."""
    g = torch.Generator().manual_seed(seed)
    C = len(kinds)
    ngp = sum(k.startswith('gp') for k in kinds)
    gp_order = list(range(ngp)) if gp_order is None else list(gp_order)
    assert sorted(gp_order) == list(range(ngp))
    P, guard, table, leaves = [], [], [], []

    def put(t):
        pad = 0.5 * torch.randn(int(torch.randint(1, 6, (1,), generator=g)), generator=g)      # the network's other parameters
        P.append(pad); guard.append(torch.ones(pad.numel(), dtype=torch.bool))
        off = sum(x.numel() for x in P)
        P.append(t.reshape(-1).float()); guard.append(torch.zeros(t.numel(), dtype=torch.bool))
        return off
    j = 0
    for kind in kinds:
        sa, logstd = 1 + torch.randn(1, 1, generator=g), 0.3 * torch.randn(1, 1, generator=g)
        row = [int(kind.startswith('gp')), int(kind.endswith('hrf')), 0, put(sa), put(logstd), 0, 0, 0, 0, 0]
        lv = {'sa': sa, 'logstd': logstd}
        if kind.startswith('gp'):
            qm = torch.randn(1, n, generator=g)
            r = 0.2 * torch.randn(n, n, generator=g)
            qS = 2 * torch.eye(n) + r @ r.t()
            lk, ll = 0.3 * torch.randn((), generator=g), 0.3 * torch.randn((), generator=g)
            row[2] = gp_order[j]; j += 1
            row[5], row[6], row[7], row[8] = put(qm), put(qS), put(lk), put(ll)
            lv.update(qu_m=qm, qu_S=qS, logkvar=lk, log_ls=ll, xu=inducing_grid(row[2], n))
        table.append(row); leaves.append(lv)
    tail = 0.5 * torch.randn(3, generator=g)
    P.append(tail); guard.append(torch.ones(3, dtype=torch.bool))
    flat, guard = torch.cat(P), torch.cat(guard)
    cov = torch.randn(B, C + 2, generator=g) * 1.5
    if B >= 2:
        cov[0, :] = 6.0; cov[1, :] = -4.0
    eps = torch.randn(C, B, generator=g)
    wt = torch.randn(C, B, generator=g)
    prefill = 0.1 * torch.randn(flat.numel(), generator=g)
    xu = torch.stack([inducing_grid(k, n) for k in range(ngp)]).float() if ngp else None
    return types.SimpleNamespace(B=B, n=n, C=C, kinds=tuple(kinds), jitter=float(jitter), table=torch.tensor(table, dtype=torch.int64),
                                 xu=xu, flat=flat, guard=guard, prefill=prefill, cov=cov, eps=eps, wt=wt, wk=0.7, leaves=leaves)


def consts_of(inp, dev):
    return ops.GainConsts(inp.table.to(dev), None if inp.xu is None else inp.xu.to(dev), K._hrf_taps().to(dev), inp.n,
                          jitter_ku=inp.jitter)


def plan_consts(n=6, C=1):
    """a GainConsts good for ops.gain_plan only (the plan depends on B and on what the descriptor check reads)"""
    return ops.GainConsts(torch.zeros(C, 10, dtype=torch.int64), None, K._hrf_taps(), n)


def posterior_fp32_distances(xu, k_var, ls, qu_m, qu_S, xq, jitter=0.0):
    """oracle.gp_posterior with the inducing-to-query distances rounded to fp32, as the reference's fp32 Knu (gp.py:90) and the
    kernel (jitter 0) form them.  The plain oracle keeps them in float64: ~1e-7 relative on a distance, times cond(Ku), moves Sigma by
    up to ~1e-5, and the factor of the near-singular B x B gain covariance (+1e-5 I) amplifies that: with float64 distances the
    REFERENCE leaves the gain band (2e-6 of the largest gain) at B = 33, n = 7 (1.3e-4), at B = 209 and 609 with n = 6 and above
    B = 1000, while with fp32 distances every one of those cases stays inside the unchanged bands."""
    import vaegam_oracle as O
    n = xu.shape[0]
    step = (xu[1] - xu[0]).detach()
    d0 = (xu[0].detach().double() - xq.detach().double())
    knu_d = (d0.unsqueeze(0) + torch.arange(n, dtype=torch.float64).unsqueeze(1) * step.double()).float().to(xq.dtype)
    knu = O.gp_kernel(knu_d, k_var, ls)
    knn = O.gp_kernel(xq.unsqueeze(0) - xq.unsqueeze(1), k_var, ls)
    idx = torch.arange(n, dtype=xq.dtype)
    ku = O.gp_kernel((idx.unsqueeze(0) - idx.unsqueeze(1)).abs(), k_var, ls, step)
    A = knu.T @ torch.inverse(ku)
    return A @ torch.squeeze(qu_m), knn + (A @ (qu_S - ku) @ A.T)


def reference(inp):
    """float64 gains, KL, f_bar / Sigma per GP covariate and the parameter gradients of  sum(task_var * wt) + wk * KL  by autograd"""
    import vaegam_oracle as O
    B, n = inp.B, inp.n
    ref_leaves, tv_ref, kl_ref, fb_ref, sg_ref = [], [], 0.0, {}, {}
    for i, (kind, lv) in enumerate(zip(inp.kinds, inp.leaves)):
        q = {k: v.float().double().clone().requires_grad_(k != 'xu') for k, v in lv.items()}
        ref_leaves.append(q)
        xq = inp.cov[:, i].double()
        sa, std = q['sa'][0], q['logstd'][0].exp()
        kl_ref = kl_ref + O.lin_gain_kl(sa, std)
        bm = sa * xq
        bc = std.pow(2) * xq.pow(2) * torch.eye(B, dtype=torch.float64)
        if kind.startswith('gp'):
            kvar = q['logkvar'].exp() + 0.1
            ls = 3.0 * torch.sigmoid(q['log_ls'].exp() + 0.5)
            if inp.jitter:
                # dense grid, cond(Ku) ~ n / jitter: autograd through the oracle's inverse(k_var Ku) makes d/d k_var a difference of
                # huge cancelling terms (A does not depend on k_var at all).  Gradients are therefore taken through the same
                # posterior written with A built from unit-variance kernels -- tied to the oracle by its forward values.
                fb_o, Sg_o = O.gp_posterior(q['xu'].float(), kvar, ls, q['qu_m'], q['qu_S'], xq, inp.jitter)
                fb_o, Sg_o = fb_o.detach(), Sg_o.detach()
                fb, Sg = K._posterior_unit_variance(q['xu'].float(), kvar, ls, q['qu_m'], q['qu_S'], xq, inp.jitter)
                np.testing.assert_allclose(fb.detach().numpy(), fb_o.numpy(), atol=2e-5 * max(1.0, float(fb_o.abs().max())))
                np.testing.assert_allclose(Sg.detach().numpy(), Sg_o.numpy(), atol=2e-5 * max(1.0, float(Sg_o.abs().max())))
            else:
                fb, Sg = posterior_fp32_distances(q['xu'].float(), kvar, ls, q['qu_m'], q['qu_S'], xq)
            bm = bm + fb; bc = bc + Sg
            kl_ref = kl_ref + O.gp_kl(q['qu_m'], q['qu_S'], n)
            fb_ref[i], sg_ref[i] = fb.detach(), Sg.detach()
        L = torch.linalg.cholesky(bc + 1e-5 * torch.eye(B, dtype=torch.float64))
        tv = bm + L @ inp.eps[i].double()
        if kind.endswith('hrf'):
            tv = K._hrf64(tv)
        tv_ref.append(tv)
    tv_ref = torch.stack(tv_ref)
    kl_ref = kl_ref.sum()
    ((tv_ref * inp.wt.double()).sum() + inp.wk * kl_ref).backward()
    grads = [{nm: q[nm].grad.reshape(-1).clone() for nm in GRAD_NAMES if nm in q} for q in ref_leaves]
    return types.SimpleNamespace(task_var=tv_ref.detach(), kl=float(kl_ref.detach()), f_bar=fb_ref, Sigma=sg_ref, grads=grads)


def launch(inp, dev, forced=False):
    """One forward + backward of ops.GpGain on the inputs (forced: the tiled path) -> namespace of CPU tensors; `grads` is the gradient
    buffer after the backward, which started as inp.prefill."""
    consts = consts_of(inp, dev)
    fp = inp.flat.to(dev).clone().requires_grad_(True)
    fg = inp.prefill.to(dev).clone()
    prev = ops.GAIN_FORCE_TILED
    ops.GAIN_FORCE_TILED = bool(forced) or prev
    try:
        tv, kl, bm, bc, fb, sg, klt = ops.GpGain.apply(inp.cov.to(dev), inp.eps.to(dev), consts, fp.detach(), fg, None, fp)
        ((tv * inp.wt.to(dev)).sum() + inp.wk * kl.sum()).backward()
    finally:
        ops.GAIN_FORCE_TILED = prev
    if dev != 'cpu':
        torch.cuda.synchronize()
    return types.SimpleNamespace(task_var=tv.detach().cpu(), kl=kl.detach().cpu(), beta_cov=bc.cpu(), f_bar=fb.cpu(), Sigma=sg.cpu(),
                                 grads=fg.cpu())


def compare(inp, ref, got, grow=1.0, what=''):
    """the bands of the module docstring; -> the measured figures (each relative to its band's absolute part)"""
    m = {}
    tv_band = 2e-6 * float(ref.task_var.abs().max())
    m['task_var'] = float((got.task_var.double() - ref.task_var).abs().max()) / tv_band
    m['kl'] = abs(float(got.kl) - ref.kl) / (1e-6 * abs(ref.kl))
    m['f_bar'] = max([float((got.f_bar[i] - ref.f_bar[i]).abs().max()) / 2e-5 for i in ref.f_bar] or [0.0])
    m['Sigma'] = max([float((got.Sigma[i] - ref.Sigma[i]).abs().max()) / 2e-5 for i in ref.Sigma] or [0.0])
    have_all = got.grads.double() - inp.prefill.double()
    m['hyper'] = 0.0                                           # d logkvar, d log_ls: largest |error| / (2e-4 x scale)
    m['grads'] = 0.0                                           # every other gradient, the same ratio
    for i, (kind, row) in enumerate(zip(inp.kinds, inp.table.tolist())):
        offs = dict(zip(GRAD_NAMES, row[3:9]))
        for nm, want in ref.grads[i].items():
            have = have_all[offs[nm]:offs[nm] + want.numel()]
            scale = max(float(want.abs().max()), 1e-2)
            r = float((have - want).abs().max()) / (2e-4 * scale)
            key = 'hyper' if nm in ('logkvar', 'log_ls') else 'grads'
            m[key] = max(m[key], r)
    print('gain %s: error / band  task_var %.3f  kl %.3f  f_bar %.3f  Sigma %.3f  grads %.3f  d logkvar, d log_ls %.3f'
          % (what, m['task_var'], m['kl'], m['f_bar'], m['Sigma'], m['grads'], m['hyper']))
    np.testing.assert_allclose(got.task_var.numpy(), ref.task_var.numpy(), rtol=2e-6, atol=tv_band)
    np.testing.assert_allclose(float(got.kl), ref.kl, rtol=1e-6)
    for i in ref.f_bar:
        np.testing.assert_allclose(got.f_bar[i].numpy(), ref.f_bar[i].numpy(), atol=2e-5)
        np.testing.assert_allclose(got.Sigma[i].numpy(), ref.Sigma[i].numpy(), atol=2e-5)
    # the backward adds, and only inside the gain parameters' own segments
    assert torch.equal(got.grads[inp.guard], inp.prefill[inp.guard]), 'the backward wrote outside the gain parameters\' segments'
    for i, (kind, row) in enumerate(zip(inp.kinds, inp.table.tolist())):
        offs = dict(zip(GRAD_NAMES, row[3:9]))
        for nm, want in ref.grads[i].items():
            have = have_all[offs[nm]:offs[nm] + want.numel()]
            scale = max(float(want.abs().max()), 1e-2)
            g_ = grow if nm in ('logkvar', 'log_ls') else 1.0
            np.testing.assert_allclose(have.numpy(), want.numpy(), rtol=2e-4, atol=2e-4 * scale * g_,
                                       err_msg='%s cov %d (%s) d%s' % (what, i, kind, nm))
    return m


@functools.lru_cache(maxsize=4)
def _inputs_and_reference(B, n, jitter, seed, kinds, gp_order):
    inp = build_inputs(B, n, seed, kinds, jitter, gp_order)
    return inp, reference(inp)


def run_case(dev, B, n=6, jitter=0.0, seed=0, kinds=DEFAULT_KINDS, gp_order=None, forced=False, grow=1.0, what=None):
    """forward + backward on `dev` against the float64 reference (shared between the calls that use the same inputs)"""
    inp, ref = _inputs_and_reference(B, n, float(jitter), seed, tuple(kinds), None if gp_order is None else tuple(gp_order))
    got = launch(inp, dev, forced)
    return compare(inp, ref, got, grow, what or 'B=%d n=%d jitter=%g%s' % (B, n, jitter, ' tiled' if forced else ''))


# ------------------------------------------------------------------------------------------------ the case matrix
# id: (B, n, jitter, kinds, gp_order, forced, where, what it pins).  where: 'both' = host build and MI355X, 'gpu' = MI355X only (the host
# build walks a workgroup's threads in order: 11.6 s at B = 609).  The B of a class is the smallest the plan sweep finds for it
# (check_gain_coverage).
def _c(B, n, jitter, kinds, gp_order, forced, where, pins):
    return types.SimpleNamespace(B=B, n=n, jitter=jitter, kinds=kinds, gp_order=gp_order, forced=forced, where=where, pins=pins)


CASES = {
    'lds-1': _c(1, 6, 0.0, DEFAULT_KINDS, None, False, 'both', '1 x 1 factor, HRF of one sample'),
    'lds-7': _c(7, 6, 0.0, DEFAULT_KINDS, None, False, 'both', 'fewer samples than HRF taps'),
    'lds-16': _c(16, 6, 0.0, DEFAULT_KINDS, None, False, 'both', 'last B of the LDS path'),
    'blocked-17-n2': _c(17, 2, 0.0, DEFAULT_KINDS, None, False, 'both', 'first blocked B; last panel and last slab of width 1; smallest n'),
    'blocked-31': _c(31, 6, 0.0, DEFAULT_KINDS, None, False, 'both', 'last panel 15, trailing blocks 15 = 3 * 4 + 3'),
    'blocked-50-mixed': _c(50, 7, 0.0, MIXED_KINDS, (1, 0), False, 'both', 'B % 4 = 2; odd n; GP first and last; permuted gp_index'),
    'blocked-19-nogp': _c(19, 6, 0.0, NO_GP_KINDS, None, False, 'both', 'no GP: xu = None, diagonal L'),
    'blocked-19-c1': _c(19, 9, 0.0, ('gp',), None, False, 'both', 'C = 1'),
    'blocked-18-n128': _c(18, 128, 1e-4, DEFAULT_KINDS, None, False, 'both', 'largest n'),
    'blocked-209': _c(209, 6, 0.0, DEFAULT_KINDS, None, False, 'both', '13 full panels + 1; more 4 x 4 trailing tiles (1,225) than threads'),
    'blocked-609': _c(609, 6, 0.0, DEFAULT_KINDS, None, False, 'both', 'first B of slab class 8; last slab of width 1'),
    'blocked-833': _c(833, 6, 0.0, DEFAULT_KINDS, None, False, 'gpu', 'first B of slab class 4; last slab of width 1'),
    'blocked-1000': _c(1000, 6, 0.0, DEFAULT_KINDS, None, False, 'gpu', 'class 4; last panel 8; LDS request near the limit'),
    'tiled-63': _c(63, 6, 0.0, DEFAULT_KINDS, None, True, 'both', 'short single tile'),
    'tiled-64': _c(64, 6, 0.0, DEFAULT_KINDS, None, True, 'both', 'exactly one tile'),
    'tiled-65': _c(65, 6, 0.0, DEFAULT_KINDS, None, True, 'both', 'second tile of one row'),
    'tiled-200-mixed': _c(200, 7, 0.0, MIXED_KINDS, (1, 0), True, 'both', 'four tiles, last of 8 rows; mixed diagonal and dense L'),
    'tiled-19-nogp': _c(19, 6, 0.0, NO_GP_KINDS, None, True, 'both', 'no GP on the tiled path'),
}
# |tiled - blocked| measured on the MI355X, relative to the largest |value|: 0 for task_var and 0 for the gradients at B = 256 and at
# 1024 (the float64 results of the two blockings round to the same fp32 outputs).  3 x 0 would demand bit equality, which
# the paths do not promise: the band is one fp32 ulp of the largest value instead
TILED_VS_BLOCKED_BAND = {'task_var': 1.2e-7, 'grads': 1.2e-7}
TILED_VS_BLOCKED_B = (17, 209, 608, 609, 832, 833)             # next to the older tests' 256 and 1024; the host build runs those <= 209
NULL_OUTPUT_CASES = ((17, False), (65, True))                  # (B, forced)


def case_ids(where):
    return [cid for cid, c in CASES.items() if where == 'gpu' or c.where == 'both']


def run_listed(dev, cid):
    c = CASES[cid]
    return run_case(dev, c.B, c.n, c.jitter, seed=c.B, kinds=c.kinds, gp_order=c.gp_order, forced=c.forced, grow=1.0, what=cid)


def run_pair(dev, B, n=6):
    """the same inputs through the blocked (B <= 16: LDS) and the tiled path -> the two results and their largest differences relative
    to the largest value: task_var, the gradients (what the backward added), KL; the caller asserts its bands"""
    inp = build_inputs(B, n, seed=B)
    a, b = launch(inp, dev, False), launch(inp, dev, True)
    ga, gb = a.grads.double() - inp.prefill.double(), b.grads.double() - inp.prefill.double()
    a.added, b.added = ga, gb
    d = {'task_var': float((b.task_var - a.task_var).abs().max() / a.task_var.abs().max()),
         'grads': float((gb - ga).abs().max() / ga.abs().max()),
         'kl': abs(float(b.kl) - float(a.kl)) / abs(float(a.kl))}
    print('B=%d tiled vs blocked: task_var %.3g, grads %.3g, kl %.3g (relative to max)' % (B, d['task_var'], d['grads'], d['kl']))
    assert torch.equal(a.grads[inp.guard], inp.prefill[inp.guard]) and torch.equal(b.grads[inp.guard], inp.prefill[inp.guard])
    return a, b, d


def run_null_outputs(dev, B, forced):
    """vg_gp_gain_fwd (forced: _tiled) through the C ABI with beta_mean, beta_cov, f_bar and Sigma null: gains and KL bit-equal to the
    call that passes the four"""
    inp = build_inputs(B, 6, seed=B)
    consts = consts_of(inp, dev)
    lib = _lib.get_lib()
    d = consts.desc(B)
    C = inp.C
    P = ops._p
    flat, cov, eps = inp.flat.to(dev), inp.cov.to(dev), inp.eps.to(dev)
    fn = 'vg_gp_gain_fwd_tiled' if forced else 'vg_gp_gain_fwd'
    res = []
    for with_outputs in (True, False):
        ws = torch.zeros(lib.size('vg_gp_gain_ws_bytes', C, B, inp.n) // 8, dtype=torch.float64, device=dev)
        tv = torch.zeros(C, B, device=dev); kl = torch.zeros(1, device=dev)
        outs = [torch.zeros(s, dtype=torch.float64, device=dev) for s in ((C, B), (C, B, B), (C, B), (C, B, B))] if with_outputs else [None] * 4
        st = torch.cuda.current_stream().cuda_stream if dev != 'cpu' else None
        lib.call(fn, ctypes.byref(d), P(consts.table), P(flat), P(consts.xu), P(cov), int(cov.stride(0)), P(eps), P(consts.hrf), P(ws),
                 P(tv), P(kl), *[P(o) for o in outs], st)
        if dev != 'cpu':
            torch.cuda.synchronize()
        res.append((tv.cpu(), kl.cpu()))
    assert torch.isfinite(res[0][0]).all() and float(res[0][0].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------ plan sweep and coverage
def plan_class(p):
    """the launch class of a plan: the path and, where a solve is cut into slabs, their width (the LDS path has neither panels nor slabs)"""
    return (p.path, 0 if p.path == 'lds' else p.slab)


def plan_sweep(max_b=4096, ns=(2, 6, 128)):
    """every B in 1..max_b x n x {by batch, forced tiled} through vg_gp_gain_plan (host only, no launch) with the invariants of the
    blocking and the LDS limit asserted -> {class: smallest B}, the B at which the path changes and at which the slab width changes
    (not forced)"""
    lib = _lib.get_lib()
    rec = (ctypes.c_int32 * len(ops.GainPlan._fields))()
    classes, path_steps, slab_steps = {}, [], []
    for n in ns:
        d = plan_consts(n).desc(1)
        steps_p, steps_s, prev = [], [], None
        for forced in (0, 1):
            for B in range(1, max_b + 1):
                d.B = B
                lib.call('vg_gp_gain_plan', ctypes.byref(d), forced, rec, len(rec))
                p = ops.GainPlan(_lib.GAIN_PATHS[rec[0]], *rec[1:])
                assert 0 < p.lds_fwd <= LDS_LIMIT and 0 < p.lds_bwd <= LDS_LIMIT, (B, n, forced, p)
                assert p.npanels * p.panel >= B > (p.npanels - 1) * p.panel and p.last_panel == B - (p.npanels - 1) * p.panel, (B, p)
                assert p.nslabs * p.slab >= B > (p.nslabs - 1) * p.slab and p.last_slab == B - (p.nslabs - 1) * p.slab, (B, p)
                assert p.threads in (256, 1024) and p.launches_fwd >= 2 and p.launches_bwd >= 1
                if forced:
                    assert p.path == 'tiled', (B, p)
                else:
                    if prev is not None and prev.path != p.path:
                        steps_p.append(B)
                    if prev is not None and prev.path == p.path == 'blocked' and prev.slab != p.slab:
                        steps_s.append(B)
                    prev = p
                classes.setdefault(plan_class(p), B)
        path_steps.append(steps_p); slab_steps.append(steps_s)
    assert all(s == path_steps[0] for s in path_steps) and all(s == slab_steps[0] for s in slab_steps)      # the blocking does not depend on n
    return classes, path_steps[0], slab_steps[0]


def check_plan_sweep():
    classes, path_steps, slab_steps = plan_sweep()
    assert path_steps == [17, 1025], path_steps                # the path changes exactly at 16|17 and 1024|1025
    assert slab_steps == [609, 833], slab_steps                # the slab width exactly at 608|609 and 832|833
    import pytest
    with pytest.raises(_lib.VgError, match='exceeds the gain block\'s limit of 4096 volumes'):
        ops.gain_plan(plan_consts(), 4097)
    return classes


def check_gain_coverage(cases=None):
    """The case matrix against what the plan sweep enumerates: every (path, slab width) class, a short last panel and a short last slab in
    each blocked / tiled class, a full and a short tile, C = 1, no GP, a permuted gp_index, n = 2 and n = 128, distinct inducing grids."""
    cases = CASES if cases is None else cases
    classes = check_plan_sweep()
    seen = {}
    for cid, c in cases.items():
        p = ops.gain_plan(plan_consts(c.n, len(c.kinds)), c.B, c.forced)
        seen.setdefault(plan_class(p), []).append((cid, c, p))
    for cls, first_b in sorted(classes.items()):
        print('%-14r first B = %4d <- %s' % (cls, first_b, ', '.join(cid for cid, _, _ in seen.get(cls, [])) or 'NOT COVERED'))
        assert cls in seen, 'no listed case runs class %r (first at B = %d)' % (cls, first_b)
        if cls[0] != 'lds':
            assert any(p.last_panel < p.panel for _, _, p in seen[cls]), 'class %r: no case with a short last panel' % (cls,)
            assert any(p.last_slab < p.slab for _, _, p in seen[cls]), 'class %r: no case with a short last slab' % (cls,)
            if cls[0] == 'blocked':
                assert any(c.B == first_b for _, c, _ in seen[cls]), 'class %r: its first B (%d) is not run' % (cls, first_b)
    tiled = [p for cls, v in seen.items() if cls[0] == 'tiled' for _, _, p in v]
    assert any(p.last_panel == p.panel for p in tiled) and any(p.last_panel < p.panel for p in tiled), 'a full and a short tile'
    assert any(p.npanels > 1 for p in tiled)
    assert any(c.B == 16 for v in seen.get(('lds', 0), []) for c in [v[1]]), 'the last B of the LDS path'
    paths_of = lambda pred: {plan_class(p)[0] for v in seen.values() for _, c, p in v if pred(c)}
    assert any(len(c.kinds) == 1 for c in cases.values()), 'C = 1'
    assert paths_of(lambda c: not any(k.startswith('gp') for k in c.kinds)) >= {'blocked', 'tiled'}, 'a case without a GP on both paths'
    assert any(c.gp_order is not None and list(c.gp_order) != sorted(c.gp_order) for c in cases.values()), 'a permuted gp_index'
    assert {2, 128} <= {c.n for c in cases.values()}, 'n = 2 and n = 128'
    assert any(c.B == 1 for c in cases.values()), 'B = 1'
    for cid, c in cases.items():                               # no two GP covariates of a case share an inducing grid
        inp = build_inputs(min(c.B, 4), c.n, seed=c.B, kinds=c.kinds, jitter=c.jitter, gp_order=c.gp_order)
        rows = [] if inp.xu is None else [tuple(r.tolist()) for r in inp.xu]
        assert len(set(rows)) == len(rows), '%s: two GP covariates share an inducing grid' % cid
        gk = [row[2] for row in inp.table.tolist() if row[0]]
        for i, lv in enumerate(x for x in inp.leaves if 'xu' in x):
            assert torch.equal(lv['xu'].float(), inp.xu[gk[i]]), '%s: the reference and the table disagree on the grid' % cid
    return seen
