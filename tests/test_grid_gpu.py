"""Derived grids on the GPU (libvaegam_hip.so): the embed copy and the embedded GAM/ELBO kernels against float64, family grids
against the CPU oracle, embedded models against the same model on its network grid (eager and replayed from a hipGraph), a grid a
user would bring, and the command line on a native-shape data set."""
import glob
import os

import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import grid_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()                       # raises if libvaegam_hip.so is missing: no fallback
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('nat,grid,B,C', GC.EMBED_CASES, ids=GC.EMBED_IDS)
def test_embed_copy(nat, grid, B, C):
    GC.run_embed_copy_case('cuda', nat, grid, B)


@pytest.mark.parametrize('nat,grid,B,C', GC.EMBED_CASES, ids=GC.EMBED_IDS)
def test_gam_elbo_embed(nat, grid, B, C):
    GC.run_gam_embed_case('cuda', nat, grid, B, C)


@pytest.mark.parametrize('img,B', [((22, 22, 22), 4), ((26, 34, 30), 2)], ids=['22x22x22_B4', '26x34x30_B2'])
def test_family_grid_train_step_matches_oracle(img, B):
    GC.run_family_oracle_step('cuda', img, B=B, C=3)


@pytest.mark.parametrize('nat', [(19, 21, 20), (22, 25, 23)], ids=['19x21x20_in_22x22x22', '22x25x23_in_22x26x26'])
def test_embedded_model_equals_model_on_its_grid(nat):
    GC.run_embedded_model_case('cuda', nat, B=2, C=3, graph=True)


def test_user_grid_53x63x52():
    """nat 53x63x52 in 54x66x54: one eager train step with a finite loss and finite gradients; upstream tensors and maps bit-identical
    to the model on the grid; the loss against its float64 restatement (ref_gam on one batch; no oracle at this size)."""
    E = GC.run_embedded_model_case('cuda', (53, 63, 52), B=2, C=3, grads=False)
    assert E.grid_shape == (54, 66, 54) and E.img_pad == (1, 3, 2)


def test_cli_trains_and_exports_on_the_native_grid(tmp_path):
    from vae_gam_amd import multsubj_reg_run_GP as cli, synthetic
    from vae_gam_amd import DataClass_GP as D
    shape = (19, 21, 20)
    ds = synthetic.make_dataset(num_subjects=2, vols_per_subject=8, num_covariates=8, img_shape=shape, seed=3)
    csv, glm_csv = synthetic.write_csvs(ds, str(tmp_path / 'data'))
    out = str(tmp_path / 'out')
    m = cli.main(['--train_csv', csv, '--test_csv', csv, '--glm_maps', glm_csv, '--save_dir', out, '--batch-size', '4', '--epochs', '1',
                  '--test_freq', '1', '--seed', '5', '--img_shape', '19', '21', '20', '--device_resident', 'True'])
    assert m.img_shape == shape and m.grid_shape == (22, 22, 22) and m.epoch == 1
    assert np.isfinite(m.loss['train'][0]) and np.isfinite(m.loss['test'][0])
    recs = glob.glob(os.path.join(out, 'reconstructions', '001_model_recons', '*', 'vol_*', 'recon_*.nii'))
    avgs = glob.glob(os.path.join(out, 'reconstructions', '001_avg_model_recons', '**', '*.nii'), recursive=True)
    assert len(recs) == 2 * 8 * 10 and avgs
    for f in recs[:3] + recs[-3:] + avgs[:2]:
        a = D.read_nifti1(f)
        assert tuple(a.shape[:3]) == shape, (f, a.shape)
        assert np.isfinite(a).all()


def test_cli_refuses_files_of_another_shape(tmp_path):
    from vae_gam_amd import multsubj_reg_run_GP as cli, synthetic
    ds = synthetic.make_dataset(num_subjects=1, vols_per_subject=4, num_covariates=8, seed=3)            # 41x49x35 files
    csv, glm_csv = synthetic.write_csvs(ds, str(tmp_path / 'data'))
    with pytest.raises(ValueError, match=r'19x21x20.*41x49x35'):
        cli.main(['--train_csv', csv, '--test_csv', csv, '--glm_maps', glm_csv, '--save_dir', str(tmp_path / 'out'), '--batch-size', '4',
                  '--epochs', '1', '--img_shape', '19', '21', '20'])
