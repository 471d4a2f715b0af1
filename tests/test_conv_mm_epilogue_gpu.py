"""The conv_mm epilogue against float64 on the MI355X: every case of tests/conv_mm_epilogue_cases.py through libvaegam_hip.so.
CPU twin: tests/test_conv_mm_epilogue_emu.py."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import conv_mm_epilogue_cases as E

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('flags', E.FLAGS, ids=['relu_out%d-stats%d-stats_relu%d' % f for f in E.FLAGS])
@pytest.mark.parametrize('name', sorted(E.FLAG_PLANS))
def test_epilogue_flags(name, flags):
    isz, force = E.FLAG_PLANS[name]
    E.run_epilogue_case(DEV, name, 'fwd', isz, force, relu_out=flags[0], stats=flags[1], stats_relu=flags[2], seed=1 + sum(flags))


def test_epilogue_16_output_channels():
    E.run_co16_case(DEV)


@pytest.mark.parametrize('cid,name,isz,force,relu_out', E.MASKED_CASES, ids=[c[0] for c in E.MASKED_CASES])
def test_epilogue_masked(cid, name, isz, force, relu_out):
    E.run_epilogue_case(DEV, name, 'bwd', isz, force, relu_out=relu_out, seed=2)


def test_epilogue_statistics_over_runs():
    E.run_stats_run_case(DEV)
