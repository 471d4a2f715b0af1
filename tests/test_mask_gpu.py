"""The brain mask on the GPU (libvaegam_hip.so): the masked GAM/ELBO kernels against float64, the masked model (loss, gradients,
training eager and replayed from a hipGraph, exports, checkpoints, refusals) and the command line with --mask."""
import glob
import os

import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import mask_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()                       # raises if libvaegam_hip.so is missing: no fallback
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('nat,grid,B,C,make_mask', MC.KERNEL_CASES, ids=MC.KERNEL_IDS)
def test_gam_elbo_masked(nat, grid, B, C, make_mask):
    MC.run_gam_masked_case('cuda', nat, grid, B, C, make_mask)


def test_box_mask_equals_embedding():
    MC.run_box_mask_equals_embed_case('cuda')


def test_masked_entry_points_report_bad_arguments():
    MC.run_bad_arguments_case('cuda')


@pytest.mark.parametrize('img', MC.MODEL_SHAPES, ids=MC.MODEL_IDS)
def test_masked_model_loss_and_gradients(img):
    MC.run_masked_model_loss_and_grads('cuda', img)


@pytest.mark.parametrize('img', MC.MODEL_SHAPES, ids=MC.MODEL_IDS)
def test_masked_training_eager_and_replayed(img):
    MC.run_masked_model_training('cuda', img, graph=True)


@pytest.mark.parametrize('img', MC.MODEL_SHAPES, ids=MC.MODEL_IDS)
def test_mask_none_changes_nothing_and_all_ones_is_the_plain_loss(img):
    MC.run_mask_none_and_all_ones('cuda', img)


@pytest.mark.parametrize('img', MC.MODEL_SHAPES, ids=MC.MODEL_IDS)
def test_exports_are_zero_outside_the_mask(img, tmp_path):
    MC.run_export_case('cuda', img, tmp_path)


def test_checkpoint_carries_the_mask(tmp_path):
    MC.run_checkpoint_case('cuda', (19, 21, 20), tmp_path)


def test_refusals(tmp_path):
    MC.run_refusals('cuda', tmp_path)


def test_cli_trains_and_exports_with_a_mask(tmp_path):
    """main(argv) with --mask on a synthetic CSV data set: one epoch, then the export pipeline; every per-volume file and every
    subject / grand average is exactly 0 outside the mask."""
    from vae_gam_amd import multsubj_reg_run_GP as cli, synthetic
    from vae_gam_amd import DataClass_GP as D
    shape = (19, 21, 20)
    ds = synthetic.make_dataset(num_subjects=2, vols_per_subject=4, num_covariates=8, img_shape=shape, seed=3)
    csv, glm_csv = synthetic.write_csvs(ds, str(tmp_path / 'data'))
    mask = MC.ellipsoid_mask(shape)
    mpath = str(tmp_path / 'mask.npy')
    np.save(mpath, mask.numpy())
    out = str(tmp_path / 'out')
    m = cli.main(['--train_csv', csv, '--test_csv', csv, '--glm_maps', glm_csv, '--save_dir', out, '--batch-size', '4', '--epochs', '1',
                  '--test_freq', '1', '--seed', '5', '--img_shape', '19', '21', '20', '--mask', mpath])
    assert m.img_shape == shape and m.epoch == 1 and torch.equal(m.mask.cpu(), mask) and m.mask_voxels == int(mask.sum())
    assert np.isfinite(m.loss['train'][0]) and np.isfinite(m.loss['test'][0])
    recs = glob.glob(os.path.join(out, 'reconstructions', '001_model_recons', '*', 'vol_*', 'recon_*.nii'))
    avgs = glob.glob(os.path.join(out, 'reconstructions', '001_avg_model_recons', '**', '*.nii'), recursive=True)
    assert len(recs) == 2 * 4 * 10 and len(avgs) == 3 * 10
    outside = ~mask.bool().numpy()
    for f in recs + avgs:
        a = np.asarray(D.read_nifti1(f))
        assert tuple(a.shape[:3]) == shape, (f, a.shape)
        assert np.isfinite(a).all() and (a[outside] == 0).all(), f
    assert any((np.asarray(D.read_nifti1(f))[~outside] != 0).any() for f in avgs)
