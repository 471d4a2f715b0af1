"""The direct conv engine (vg_conv.hip) against float64 on the host build of the kernel sources (tests/emu, g++ -DVG_EMU): the cases
of tests/conv_direct_cases.py on CPU tensors, the two plan queries, and the coverage of the production launch classes by those cases.
The -m gpu twin is tests/test_conv_direct_gpu.py.  CONV_DIRECT_GPU_ONLY is empty: the cases that must pass a `small` gate (1.5 M / 8 M
outputs) take 0.1 to 5 s here."""
import pytest

import vae_gam_amd  # noqa: F401
import conv_direct_cases as D

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


@pytest.mark.parametrize('cid', [c.id for c in D.CASES])
def test_conv_direct_plans_pinned(cid):
    D.check_pins(D.CASE_BY_ID[cid])


def test_conv_direct_plan_queries_launch_nothing():
    D.run_queries_touch_no_memory()


@pytest.mark.parametrize('cid', D.HOST_CASES)
def test_conv_direct_case(cid):
    D.run_case(DEV, cid)


def test_conv_direct_case_matrix_coverage():
    cov = D.check_coverage()
    assert cov['gpu_only_classes'] == []                # no production class is left to the GPU suite alone
