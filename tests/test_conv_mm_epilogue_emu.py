"""The conv_mm epilogue against float64 on the host build of the kernel sources (tests/emu, g++ -DVG_EMU): the cases of
tests/conv_mm_epilogue_cases.py on CPU tensors.  The -m gpu twin is tests/test_conv_mm_epilogue_gpu.py."""
import pytest

import vae_gam_amd  # noqa: F401
import conv_mm_epilogue_cases as E

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


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
