"""The model's encode and decode paths (VAE._encode_heads, VAE._decode_logits) against a float64 restatement on the MI355X
(libvaegam_hip.so): the cases and the bound of tests/model_path_cases.py, the reference on the CPU.  Adds the 41x49x35 case (the
reference geometry: convt2 with padding / output padding, convt4 5x3x3), which is too slow for the host build."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import model_path_cases as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()                       # raises if libvaegam_hip.so is missing: no fallback
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('cid', M.HOST_CASES + M.GPU_ONLY)
def test_paths_match_float64(cid):
    M.check_case(DEV, cid)


def test_unrectified_handoff_is_bit_equal():
    M.check_bit_equal(DEV)


def test_cases_launch_every_entry_of_the_paths():
    M.check_coverage(DEV)


def test_reference_geometry_launches_the_two_halves_hand_off():
    M.check_coverage(DEV, M.GPU_ONLY, M.COVERAGE_CASE6)


def test_two_values_per_group_stay_finite_and_within_the_layer_tolerance():
    M.run_two_value_property(DEV)
