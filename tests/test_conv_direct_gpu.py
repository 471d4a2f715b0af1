"""The direct conv engine (vg_conv.hip) against float64 on the MI355X: every case of tests/conv_direct_cases.py through
libvaegam_hip.so (CONV_DIRECT_GPU_ONLY is empty: the host build affords every case).  CPU twin: tests/test_conv_direct_emu.py."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import conv_direct_cases as D

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


def test_conv_direct_plan_queries_launch_nothing():
    D.run_queries_touch_no_memory()


@pytest.mark.parametrize('cid', [c.id for c in D.CASES])
def test_conv_direct_case(cid):
    D.run_case(DEV, cid)


def test_conv_direct_case_matrix_coverage():
    D.check_coverage()
