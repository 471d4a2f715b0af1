"""The gain block (vg_gp.hip) against float64 on the MI355X: the case matrix of tests/gain_cases.py through libvaegam_hip.so -- the LDS,
blocked and tiled paths, every slab class of the blocked solves at its first batch, ragged panels / slabs / tiles (real wavefronts see
a missing barrier, the host build cannot), C = 1, no GP, permuted gp_index, interleaved parameters and a prefilled gradient buffer --,
the plan sweep and the coverage check, tiled against blocked at the class boundaries, null optional outputs.
CPU twin: tests/test_gain_emu.py.  The figures each case prints (error / band) are collected in DESIGN 4.5."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import gain_cases as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


def test_gain_plan_sweep_and_case_matrix_coverage():
    G.check_gain_coverage()


@pytest.mark.parametrize('cid', G.case_ids('gpu'))
def test_gain_case_matches_float64(cid):
    m = G.run_listed(DEV, cid)
    assert m['hyper'] <= 1.0                                   # grow = 1: d logkvar and d log_ls get no extra slack


@pytest.mark.parametrize('B', G.TILED_VS_BLOCKED_B)
def test_tiled_path_matches_the_blocked_path(B):
    """as test_gain_large_batch_gpu.py::test_tiled_path_matches_the_blocked_path, at the boundaries of the slab classes"""
    a, b, d = G.run_pair(DEV, B)
    assert torch.equal(b.beta_cov, a.beta_cov) and torch.equal(b.Sigma, a.Sigma)      # the covariance is formed element by element the same way
    assert d['task_var'] <= G.TILED_VS_BLOCKED_BAND['task_var'] and d['grads'] <= G.TILED_VS_BLOCKED_BAND['grads'], d
    assert d['kl'] <= 1e-7, d


@pytest.mark.parametrize('B,forced', G.NULL_OUTPUT_CASES)
def test_null_optional_outputs_change_nothing(B, forced):
    G.run_null_outputs(DEV, B, forced)
