"""Shared bodies of the gradient-guard tests (vg_grad_guard, vg_adam_advance_guarded, vg_adam_step_guarded): run on CPU tensors
through the host build of the kernels (tests/test_grad_guard_emu.py) and on the GPU through libvaegam_hip.so
(tests/test_grad_guard_gpu.py).  The references are numpy float64 (the norm) and torch.optim.Adam fed the clipped gradient."""
import numpy as np
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops

N32_MODEL, N64_MODEL = 1494109, 70315            # the 41x49x35 model's flat gradient buffers (fp32 parameters, fp64 epsilon map)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def new_state(dev):
    return torch.zeros(ops.GUARD_STATE_LEN, dtype=torch.float64, device=dev)


def guard(g32, g64, max_norm, skip, state):
    ops.grad_guard_(g32, g64, max_norm, skip, ops.grad_guard_ws(g32, g64), state)
    return state.cpu().numpy().copy()


def clip_factor(sumsq, max_norm):
    """torch.nn.utils.clip_grad_norm_'s factor, in float64 from the float64 sum of squares"""
    return min(1.0, max_norm / (float(np.sqrt(sumsq)) + 1e-6))


def run_norm_case(dev, n32, n64, seed=0):
    """total_norm against a float64 numpy norm of the same values (fp32 values are exact in fp64, so only the summation order
    differs: rtol 1e-12); two calls give the same bits; a finite gradient is applied, unclipped (clipping off), and counted."""
    g = torch.Generator().manual_seed(seed)
    a32 = torch.randn(n32, generator=g, dtype=torch.float32) * 3 if n32 else None
    a64 = torch.randn(n64, generator=g, dtype=torch.float64) * 0.1 if n64 else None
    want = 0.0
    for a in (a32, a64):
        if a is not None:
            want += float((a.numpy().astype(np.float64) ** 2).sum())
    want = np.sqrt(want)
    d32 = None if a32 is None else a32.to(dev); d64 = None if a64 is None else a64.to(dev)
    st = new_state(dev)
    s1 = guard(d32, d64, None, True, st)
    s2 = guard(d32, d64, None, True, st)
    print('n32=%d n64=%d norm %.17g want %.17g rel %.3g' % (n32, n64, s1[0], want, abs(s1[0] - want) / want))
    np.testing.assert_allclose(s1[ops.GUARD_NORM], want, rtol=1e-12)
    assert s1[ops.GUARD_NORM].tobytes() == s2[ops.GUARD_NORM].tobytes()
    assert s1[ops.GUARD_SCALE] == 1.0 and s1[ops.GUARD_APPLY] == 1.0
    assert (s2[ops.GUARD_SEEN], s2[ops.GUARD_SKIPPED], s2[ops.GUARD_CLIPPED]) == (2.0, 0.0, 0.0)
    np.testing.assert_allclose(s2[ops.GUARD_NORM_SUM], 2 * want, rtol=1e-12)
    np.testing.assert_allclose(s2[ops.GUARD_NORM_MAX], want, rtol=1e-12)


def run_unaligned_norm_case(dev, n=1003, seed=1):
    """A buffer that does not start on 16 bytes walks the same quads with scalar loads: the same bits as the aligned copy."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n + 1, generator=g, dtype=torch.float32).to(dev)
    aligned = base[1:].clone()
    assert aligned.data_ptr() % 16 == 0 and base[1:].data_ptr() % 16 != 0
    s1 = guard(base[1:], None, None, False, new_state(dev))
    s2 = guard(aligned, None, None, False, new_state(dev))
    assert s1[ops.GUARD_NORM].tobytes() == s2[ops.GUARD_NORM].tobytes()


def _buffers(g, dtype):
    return (g, None) if dtype == torch.float32 else (None, g)


def run_clip_case(dev, dtype, clips, n=5000, steps=3, seed=0):
    """Guarded advance + update against torch.optim.Adam fed g * c, c = min(1, max_norm / (||g|| + 1e-6)) computed here in float64
    from the same gradient.  clips=True: max_norm = a quarter of each step's norm's typical size (every step clips); clips=False:
    max_norm far above it (scale exactly 1: the result must also be BIT-equal to the unguarded kernels)."""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g, dtype=dtype)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR)
    p = p0.to(dev).clone(); m = torch.zeros_like(p); v = torch.zeros_like(p)
    pu = p0.to(dev).clone(); mu = torch.zeros_like(pu); vu = torch.zeros_like(pu)           # the unguarded kernels on the same gradients
    sc = torch.zeros(3, dtype=torch.float64, device=dev); scu = torch.zeros_like(sc)
    st = new_state(dev)
    max_norm = 0.25 * np.sqrt(n) if clips else 1e3 * np.sqrt(n)
    nclipped = 0
    for t in range(1, steps + 1):
        gr = torch.randn(n, generator=g, dtype=dtype)
        c = clip_factor((gr.numpy().astype(np.float64) ** 2).sum(), max_norm)
        nclipped += c < 1.0
        ref.grad = gr * c; opt.step()
        gd = gr.to(dev); before = gd.clone()
        s = guard(*_buffers(gd, dtype), max_norm, False, st)
        np.testing.assert_allclose(s[ops.GUARD_SCALE], c, rtol=1e-12)
        ops.adam_advance_guarded_(sc, LR, B1, B2, st)
        ops.adam_step_guarded_(p, gd, m, v, B1, B2, EPS, sc, st)
        assert torch.equal(gd, before)                              # the gradient buffer itself stays unscaled
        ops.adam_advance_(scu, LR, B1, B2)
        ops.adam_step_(pu, gd, mu, vu, B1, B2, EPS, scu)
    assert (nclipped == steps) if clips else (nclipped == 0)
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    print('clip %s %s max |p - ref| %.3g' % (dtype, clips, float((p.cpu() - ref.detach()).abs().max())))
    np.testing.assert_allclose(p.cpu().numpy(), ref.detach().numpy(), rtol=tol, atol=tol)
    s = st.cpu().numpy()
    assert (s[ops.GUARD_SEEN], s[ops.GUARD_SKIPPED], s[ops.GUARD_CLIPPED]) == (steps, 0, nclipped)
    assert torch.equal(sc, scu)
    if not clips:
        assert torch.equal(p, pu) and torch.equal(m, mu) and torch.equal(v, vu)
    else:
        assert not torch.equal(p, pu)


def run_skip_case(dev, dtype, bad, max_norm=None, n=5000, seed=0):
    """One `bad` (inf / nan) element in the gradient of step 2 of 3: p, m, v and the device's t after step 2 are bit-equal to their
    values after step 1; step 3 matches a torch.optim.Adam that took steps 1 and 3 only (t == 2); counters: seen 3, skipped 1."""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g, dtype=dtype)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR)
    p = p0.to(dev).clone(); m = torch.zeros_like(p); v = torch.zeros_like(p)
    sc = torch.zeros(3, dtype=torch.float64, device=dev)
    st = new_state(dev)
    for t in (1, 2, 3):
        gr = torch.randn(n, generator=g, dtype=dtype)
        if t == 2:
            gr[n // 3] = bad
            snap = [x.clone() for x in (p, m, v, sc)]
        else:
            c = 1.0 if max_norm is None else clip_factor((gr.numpy().astype(np.float64) ** 2).sum(), max_norm)
            ref.grad = gr * c; opt.step()
        gd = gr.to(dev)
        s = guard(*_buffers(gd, dtype), max_norm, True, st)
        ops.adam_advance_guarded_(sc, LR, B1, B2, st)
        ops.adam_step_guarded_(p, gd, m, v, B1, B2, EPS, sc, st)
        if t == 2:
            assert s[ops.GUARD_APPLY] == 0.0 and not np.isfinite(s[ops.GUARD_NORM])
            for got, want in zip((p, m, v, sc), snap):
                assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        else:
            assert s[ops.GUARD_APPLY] == 1.0 and np.isfinite(s[ops.GUARD_NORM])
    assert float(sc[2]) == 2.0
    np.testing.assert_allclose(sc.cpu().numpy(), [LR / (1 - B1 ** 2), np.sqrt(1 - B2 ** 2), 2.0], rtol=1e-14)
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    assert bool(torch.isfinite(p).all())
    np.testing.assert_allclose(p.cpu().numpy(), ref.detach().numpy(), rtol=tol, atol=tol)
    s = st.cpu().numpy()
    assert (s[ops.GUARD_SEEN], s[ops.GUARD_SKIPPED]) == (3.0, 1.0)
    assert np.isfinite(s[ops.GUARD_NORM_SUM]) and np.isfinite(s[ops.GUARD_NORM_MAX])       # the bad step stays out of the statistics


def run_nonfinite_without_skip_case(dev):
    """skip_nonfinite off: the step is applied (apply 1) and counted as seen only -- the plain optimiser's behaviour, made visible."""
    gd = torch.ones(300, dtype=torch.float32, device=dev); gd[7] = float('inf')
    s = guard(gd, None, 1.0, False, new_state(dev))
    assert s[ops.GUARD_APPLY] == 1.0 and s[ops.GUARD_SCALE] == 0.0 and np.isinf(s[ops.GUARD_NORM])
    assert (s[ops.GUARD_SEEN], s[ops.GUARD_SKIPPED], s[ops.GUARD_CLIPPED], s[ops.GUARD_NORM_SUM]) == (1.0, 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ model level
def flat_state(model):
    """clones of (p, m, v) of every dtype group, and the gradients"""
    out = {}
    for dt, gr in model.optimizer.groups.items():
        out[dt] = {k: gr[k].detach().clone() for k in ('p', 'g', 'm', 'v')}
    return out


def clipped_reference_update(before, grads, max_norm):
    """torch.optim.Adam's first step from the flat parameters `before` on grads * c (c from the float64 norm over BOTH buffers)."""
    sumsq = sum(float((g.cpu().numpy().astype(np.float64) ** 2).sum()) for g in grads.values())
    c = clip_factor(sumsq, max_norm)
    out = {}
    for dt, p0 in before.items():
        ref = p0.cpu().clone().requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=LR)
        ref.grad = grads[dt].cpu() * c
        opt.step()
        out[dt] = ref.detach()
    return out, c, float(np.sqrt(sumsq))
