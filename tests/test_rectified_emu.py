"""The rectified decoder hand-off (relu_out / rectified_in) on the host build of the kernel sources (tests/emu,
g++ -DVG_EMU): index arithmetic, the autograd glue and the toy model without a GPU.  The -m gpu twin is tests/test_rectified_gpu.py."""
import pytest

import vae_gam_amd  # noqa: F401
import rectified_cases as R

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


# ------------------------------------------------------------------------------------------------ a. producers
@pytest.mark.parametrize('name', [c[0] for c in R.MM_PRODUCERS])
def test_conv_mm_stores_rectified(name):
    R.run_mm_producer_case(DEV, name)


def test_tconv3d_s2_stores_rectified():
    R.run_tconv_producer_case(DEV)


@pytest.mark.parametrize('which', ['plane', 'direct'])
def test_corr3d_stores_rectified(which):
    R.run_corr_producer_case(DEV, which)


# ------------------------------------------------------------------------------------------------ b. consumers
@pytest.mark.parametrize('name', list(R.CONSUMERS))
def test_rectified_input_changes_no_bit(name, monkeypatch):
    R.run_consumer_case(DEV, name, monkeypatch)


# ------------------------------------------------------------------------------------------------ c. model
def test_model_default_is_on():
    assert R.toy_model(DEV)[0].rectified_handoff is True


def test_toy_step_with_handoff_equals_step_without():
    R.run_model_bit_equal_case(DEV)
