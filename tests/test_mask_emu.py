"""The brain mask without a GPU: the masked GAM/ELBO kernels against float64 and the masked model through the host build of the HIP
kernels (tests/emu).  tests/test_mask_gpu.py repeats the cases on the real library and adds the captured step and the command line.
A model step takes ten seconds and more on the host build, so the loss / gradient and export cases run on both model shapes here and
the others on one (the GPU file runs every case on both)."""
import pytest

import toy_case as T
import mask_cases as MC
from vae_gam_amd import _lib


@pytest.fixture(scope='module')
def emu():
    prev = _lib._LIB
    T.load_emu_library()
    yield
    _lib._LIB = prev


@pytest.mark.parametrize('nat,grid,B,C,make_mask', MC.KERNEL_CASES, ids=MC.KERNEL_IDS)
def test_gam_elbo_masked(emu, nat, grid, B, C, make_mask):
    MC.run_gam_masked_case('cpu', nat, grid, B, C, make_mask)


def test_box_mask_equals_embedding(emu):
    MC.run_box_mask_equals_embed_case('cpu')


def test_masked_entry_points_report_bad_arguments(emu):
    MC.run_bad_arguments_case('cpu')


@pytest.mark.parametrize('img', MC.MODEL_SHAPES, ids=MC.MODEL_IDS)
def test_masked_model_loss_and_gradients(emu, img):
    MC.run_masked_model_loss_and_grads('cpu', img)


def test_masked_training_leaves_epsilon_outside_the_mask(emu):
    MC.run_masked_model_training('cpu', (19, 21, 20))


def test_mask_none_changes_nothing_and_all_ones_is_the_plain_loss(emu):
    MC.run_mask_none_and_all_ones('cpu', (22, 22, 22))


@pytest.mark.parametrize('img', MC.MODEL_SHAPES, ids=MC.MODEL_IDS)
def test_exports_are_zero_outside_the_mask(emu, img, tmp_path):
    MC.run_export_case('cpu', img, tmp_path)


def test_checkpoint_carries_the_mask(emu, tmp_path):
    MC.run_checkpoint_case('cpu', (19, 21, 20), tmp_path)


def test_refusals(emu, tmp_path):
    MC.run_refusals('cpu', tmp_path)
