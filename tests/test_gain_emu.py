"""The gain block (vg_gp.hip) on the host build of the kernel sources (tests/emu, g++ -DVG_EMU): the case matrix of tests/gain_cases.py
against float64 -- every path, the ragged panels / slabs / tiles, C = 1, no GP, permuted gp_index, interleaved parameters and a
prefilled gradient buffer --, the plan sweep and the coverage check, tiled against blocked, null optional outputs.  The host build runs
the threads of a workgroup in order: it checks arithmetic and indices, not barriers; the -m gpu twin is tests/test_gain_gpu.py.
The figures each case prints (error / band) are collected in DESIGN 4.5."""
import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops
import gain_cases as G


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


def test_gain_plan_sweep_and_case_matrix_coverage():
    """vg_gp_gain_plan over every B in 1..4096, n in {2, 6, 128}, forced and not; the case matrix reaches every class it enumerates"""
    G.check_gain_coverage()


def test_gain_plan_names_what_the_launchers_use():
    p = ops.gain_plan(G.plan_consts(), 1000)
    assert (p.path, p.threads, p.panel, p.npanels, p.last_panel, p.slab, p.nslabs, p.last_slab) == ('blocked', 1024, 16, 63, 8, 4, 250, 4)
    assert p.lds_fwd == 8 * (1024 + 1000 * 17) and p.lds_bwd == 8 * 1000 * (16 + 4) and (p.launches_fwd, p.launches_bwd) == (2, 4)
    p = ops.gain_plan(G.plan_consts(), 200, forced=True)
    assert (p.path, p.threads, p.panel, p.npanels, p.last_panel, p.slab, p.nslabs, p.last_slab) == ('tiled', 256, 64, 4, 8, 64, 4, 8)
    assert (p.launches_fwd, p.launches_bwd) == (2 + 4 + 2 * 3 + 3, 6)
    p = ops.gain_plan(G.plan_consts(), 16)
    assert (p.path, p.threads, p.npanels, p.nslabs, p.lds_fwd, p.launches_bwd) == ('lds', 256, 1, 1, 8 * (256 + 256), 1)


@pytest.mark.parametrize('cid', G.case_ids('emu'))
def test_gain_case_matches_float64(cid):
    m = G.run_listed('cpu', cid)
    assert m['hyper'] <= 1.0                                   # grow = 1: d logkvar and d log_ls get no extra slack


@pytest.mark.parametrize('B', [b for b in G.TILED_VS_BLOCKED_B if b <= 209])
def test_tiled_path_matches_the_blocked_path(B):
    """the bands of test_gain_large_batch_emu.py::test_tiled_path_matches_the_blocked_path_at_130"""
    a, b, d = G.run_pair('cpu', B)
    for k in ('beta_cov', 'Sigma', 'f_bar'):
        np.testing.assert_allclose(getattr(b, k).numpy(), getattr(a, k).numpy(), rtol=1e-14, atol=1e-14, err_msg=k)
    assert d['task_var'] <= 1e-6 and d['kl'] <= 1e-7, d
    ga, gb = a.added.numpy(), b.added.numpy()
    np.testing.assert_allclose(gb, ga, rtol=1e-4, atol=1e-5 * np.abs(ga).max())


@pytest.mark.parametrize('B,forced', G.NULL_OUTPUT_CASES)
def test_null_optional_outputs_change_nothing(B, forced):
    G.run_null_outputs('cpu', B, forced)
