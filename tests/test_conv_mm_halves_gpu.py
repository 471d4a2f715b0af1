"""The two-halves launches of vg_conv_mm (16-channel stride-2 transposed convs) against float64 on the MI355X: every case of
tests/conv_mm_halves_cases.py through libvaegam_hip.so.  CPU twin: tests/test_conv_mm_halves_emu.py."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import conv_mm_halves_cases as H

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('case', H.FWD_CASES + H.BWD_CASES, ids=[c[0] for c in H.FWD_CASES + H.BWD_CASES])
def test_halves_case(case):
    H.run_halves_case(DEV, case)


def test_halves_sample_loop():
    H.run_loop_case(DEV)


def test_halves_are_distinct_and_partials_layout():
    H.run_distinct_halves_case(DEV)


@pytest.mark.parametrize('case', H.STATS_OF_CASES, ids=[c[0] for c in H.STATS_OF_CASES])
def test_halves_step_launch_is_bit_equal_to_the_register_tiled_engine(case):
    H.run_stats_of_case(DEV, case)


def test_halves_descriptor_refusals():
    H.check_descriptor_refusals()
