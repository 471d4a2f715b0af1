"""Group permutation inference on the GPU (libvaegam_hip.so): the sign-flip max-statistic kernel against its numpy reference, to the
bit (the shared cases, and one at 41x49x35 voxels against the same ordered adds in torch on the device), MapStatistics.group_permutation,
mk_stat_maps with n_perm and the command line with --stat_perm."""
import filecmp
import os

import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import group_perm_cases as GP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()                       # raises if libvaegam_hip.so is missing: no fallback
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('S', GP.S_CASES)
def test_kernel_subjects(S):
    GP.run_subjects_case('cuda', S)


def test_every_instance_is_hit():
    GP.run_every_instance_is_hit()


@pytest.mark.parametrize('V', GP.V_CASES)
def test_kernel_voxels(V):
    GP.run_voxels_case('cuda', V)


@pytest.mark.parametrize('P', GP.P_CASES)
def test_kernel_permutations(P):
    GP.run_permutations_case('cuda', P)


@pytest.mark.parametrize('tail', GP.TAILS)
def test_kernel_tails(tail):
    GP.run_tail_case('cuda', tail)


@pytest.mark.parametrize('tail', GP.TAILS)
@pytest.mark.parametrize('kind', GP.ZERO_CASES)
def test_kernel_zero_scale(kind, tail):
    GP.run_zero_scale_case('cuda', kind, tail)


def test_dead_voxels_do_not_pollute_a_negative_maximum():
    GP.run_polluted_maximum_case('cuda')


@pytest.mark.parametrize('tail', GP.TAILS)
def test_kernel_exact_ties(tail):
    GP.run_ties_case('cuda', tail)


def test_kernel_hand_case():
    GP.run_hand_case('cuda')


def test_refusals_leave_the_outputs_untouched():
    GP.run_refusals_case('cuda')


def test_kernel_real_size():
    GP.run_real_size_case('cuda')


def test_group_permutation_basics():
    GP.run_basics_case('cuda')


def test_group_permutation_errors():
    GP.run_errors_case('cuda')


def test_planted_signal():
    GP.run_planted_signal_case('cuda')


def test_threshold():
    GP.run_threshold_case('cuda')


def test_stat_maps_files_with_permutations(tmp_path):
    GP.run_stat_maps_files('cuda', tmp_path)


def _tree(root):
    """every file under root but the scalar logs (run/<date>/: their names may carry a time stamp)"""
    paths = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    return [p for p in paths if not p.startswith('run' + os.sep)]


def test_cli_stat_perm_adds_its_files_and_changes_nothing_else(tmp_path):
    """main(argv) twice on one synthetic CSV data set (3 subjects x 4 volumes, 19x21x20, an ellipsoid mask) and seed, with --stat_maps
    alone and with --stat_perm 64 added: the second run adds exactly the new files, every other NIfTI and CSV is byte for byte the
    same; the new maps are finite, in [0, 1] and 0 outside the mask; three subjects make 8 patterns, so 1 - p is at most 1 - 2 / 8."""
    from vae_gam_amd import multsubj_reg_run_GP as cli, synthetic
    from vae_gam_amd import DataClass_GP as D
    import mask_cases as MC
    import pandas as pd
    shape = (19, 21, 20)
    ds = synthetic.make_dataset(num_subjects=3, vols_per_subject=4, num_covariates=8, img_shape=shape, seed=3)
    csv, glm_csv = synthetic.write_csvs(ds, str(tmp_path / 'data'))
    mask = MC.ellipsoid_mask(shape)
    mpath = str(tmp_path / 'mask.npy')
    np.save(mpath, mask.numpy())
    outs = {}
    for name, extra in (('stats', []), ('perm', ['--stat_perm', '64', '--stat_perm_seed', '2'])):
        outs[name] = str(tmp_path / name)
        m = cli.main(['--train_csv', csv, '--test_csv', csv, '--glm_maps', glm_csv, '--save_dir', outs[name], '--batch-size', '4',
                      '--epochs', '1', '--test_freq', '1', '--seed', '5', '--img_shape', '19', '21', '20', '--mask', mpath,
                      '--stat_maps', 'True'] + extra)
        assert m.epoch == 1
    sub = os.path.join('reconstructions', '001_stat_model_recons')
    keys = ['base', 'task', 'full_rec', 'x_mot', 'y_mot', 'z_mot', 'pitch_mot', 'roll_mot', 'yaw_mot', 'sex']
    new = [os.path.join(sub, '%s_%s_1mp.nii' % (k, c)) for k in keys for c in ('fwe', 'unc')] + [os.path.join(sub, 'perm_thresholds.csv')]
    stats, perm = _tree(outs['stats']), _tree(outs['perm'])
    assert sorted(perm) == sorted(stats + new)
    same = [p for p in stats if p.endswith(('.nii', '.csv'))]
    assert len(same) >= 3 * 4 * 10 + 4 * 10 and any(p.startswith(sub) for p in same)
    for p in same:
        assert filecmp.cmp(os.path.join(outs['stats'], p), os.path.join(outs['perm'], p), shallow=False), p
    outside = ~mask.bool().numpy()
    largest = 0.0
    for p in new[:-1]:
        a = np.asarray(D.read_nifti1(os.path.join(outs['perm'], p))).reshape(shape)
        assert np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all() and (a[outside] == 0).all(), p
        assert a.max() <= 1.0 - 2.0 / 8.0, (p, a.max())
        largest = max(largest, float(a.max()))
    assert largest == 1.0 - 2.0 / 8.0
    tab = pd.read_csv(os.path.join(outs['perm'], new[-1]))
    assert tab['map'].tolist() == keys and (tab['tail'] == 'two').all() and set(tab['P'].tolist()) <= {0, 8}
    assert tab['exhaustive'][tab['P'] == 8].all() and (tab['n_fwe_0.05'] == 0).all()
