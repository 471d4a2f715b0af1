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


def _gain_run(B, n=6, seed=3, kinds=('lin_hrf', 'gp', 'gp', 'gp_hrf', 'lin')):
    """One forward + backward of ops.GpGain on the inputs run_gain_case builds; -> dict of float64 ndarrays."""
    g = torch.Generator().manual_seed(seed)
    P, table, xus = [], [], []

    def put(t):
        off = sum(x.numel() for x in P); P.append(t.reshape(-1).float()); return off
    for kind in kinds:
        row = [int(kind.startswith('gp')), int(kind.endswith('hrf')), len(xus), put(1 + torch.randn(1, 1, generator=g)),
               put(0.3 * torch.randn(1, 1, generator=g)), 0, 0, 0, 0, 0]
        if kind.startswith('gp'):
            r = 0.2 * torch.randn(n, n, generator=g)
            row[5], row[6] = put(torch.randn(1, n, generator=g)), put(2 * torch.eye(n) + r @ r.t())
            row[7], row[8] = put(0.3 * torch.randn((), generator=g)), put(0.3 * torch.randn((), generator=g))
            xus.append(torch.linspace(-4.1, 6.2, n))
        table.append(row)
    C = len(kinds)
    flat = torch.cat(P)
    cov = torch.randn(B, C + 2, generator=g) * 1.5
    eps = torch.randn(C, B, generator=g)
    wt = torch.randn(C, B, generator=g)
    consts = ops.GainConsts(torch.tensor(table, dtype=torch.int64), torch.stack(xus).float(), K._hrf_taps(), n)
    fp = flat.clone().requires_grad_(True)
    fg = torch.zeros_like(fp)
    tv, kl, bm, bc, fb, sg, klt = ops.GpGain.apply(cov, eps, consts, fp.detach(), fg, None, fp)
    ((tv * wt).sum() + 0.7 * kl.sum()).backward()
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
