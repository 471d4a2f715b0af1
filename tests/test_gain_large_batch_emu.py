"""The tiled path of the gain block (vg_gp_gain_fwd_tiled / _bwd_tiled: 64 x 64 tiles, a blocked right-looking Cholesky of three
launches per panel, left-looking slab solves, per-row-block partial sums) on the host build of the kernel sources (tests/emu,
g++ -DVG_EMU), at small batches: one partial panel (B = 40), several panels with a partial last one (97, 130).  The path serves
1024 < B <= 4096 on the GPU; the forced-tiled entry pair runs it at any B.  The -m gpu twin is tests/test_gain_large_batch_gpu.py."""
import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops
import kernel_cases as K
import gain_cases as G


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


@pytest.mark.parametrize('B,n,jitter', [(40, 6, 0.0), (97, 6, 0.0), (130, 6, 0.0), (40, 32, 1e-4)])
def test_tiled_gain_block_matches_float64_oracle(monkeypatch, B, n, jitter):
    monkeypatch.setattr(ops, 'GAIN_FORCE_TILED', True)
    K.run_gain_case('cpu', B=B, n=n, jitter=jitter, seed=B)


def _gain_run(B, n=6, seed=3, kinds=G.DEFAULT_KINDS):
    """One forward + backward of ops.GpGain on the shared builder's inputs (tests/gain_cases.py); -> dict of float64 ndarrays."""
    inp = G.build_inputs(B, n, seed, kinds)
    consts = G.consts_of(inp, 'cpu')
    fp = inp.flat.clone().requires_grad_(True)
    fg = torch.zeros_like(fp)
    tv, kl, bm, bc, fb, sg, klt = ops.GpGain.apply(inp.cov, inp.eps, consts, fp.detach(), fg, None, fp)
    ((tv * inp.wt).sum() + 0.7 * kl.sum()).backward()
    return {'task_var': tv.detach().double().numpy(), 'gp_kl': kl.detach().double().numpy(), 'beta_cov': bc.numpy(),
            'f_bar': fb.numpy(), 'Sigma': sg.numpy(), 'grads': fg.double().numpy()}


def test_tiled_path_matches_the_blocked_path_at_130(monkeypatch):
    """Same inputs through both paths of the library: the tiled path forms beta_cov / Sigma / f_bar element by element exactly as the
    blocked one (bit-identical where the host compiler makes the same contractions), the rest agrees to rounding."""
    ref = _gain_run(130)
    monkeypatch.setattr(ops, 'GAIN_FORCE_TILED', True)
    got = _gain_run(130)
    for k in ('beta_cov', 'Sigma', 'f_bar'):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-14, atol=1e-14, err_msg=k)
    np.testing.assert_allclose(got['task_var'], ref['task_var'], rtol=1e-6, atol=1e-6 * np.abs(ref['task_var']).max())
    np.testing.assert_allclose(got['gp_kl'], ref['gp_kl'], rtol=1e-7)
    scale = np.abs(ref['grads']).max()
    np.testing.assert_allclose(got['grads'], ref['grads'], rtol=1e-4, atol=1e-5 * scale)
