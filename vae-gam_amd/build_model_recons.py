"""Single-volume, subject-average and grand-average reconstruction maps (reference: build_model_recons.py:15-116).

`mk_single_volumes` keeps the reference's interface and directory layout (one `recon_<map>.nii` per volume).
`mk_avg_maps` produces the same `<map>_avg.nii` files, but from sums that `VAE.reconstruct` accumulated ON THE
DEVICE while it made the single volumes (`model.recon_sums`), instead of re-reading every per-volume file the
way the reference does; called without a preceding `mk_single_volumes(..., write_volumes=...)` pass it runs the
loader itself with file writing off.
"""
import os

import numpy as np
import pandas as pd

from . import nifti
from .map_statistics import NoVoxelError

MAPS_ALL = ['base', 'task', 'full_rec', 'x_mot', 'y_mot', 'z_mot', 'pitch_mot', 'roll_mot', 'yaw_mot', 'sex']   # :66-67


def _subjects(csv_file):
    dset = pd.read_csv(csv_file)
    return dset.iloc[:, 1].unique().tolist(), dset.iloc[:, 3].unique().tolist()          # subjid, nii_path (positional, as DataClass_GP)


def mk_single_volumes(loader, model, csv_file, save_dir, write_volumes=True, noise=None):
    subjs, ref_niis = _subjects(csv_file)
    ckpt_num = str(model.epoch).zfill(3)
    subj_dirs = []
    for s in subjs:
        d = os.path.join(save_dir, 'reconstructions', '{}_model_recons'.format(ckpt_num), str(s))
        os.makedirs(d, exist_ok=True)
        subj_dirs.append(d)
    model.reconstruct(loader, ref_niis, subj_dirs, write_volumes=write_volumes, noise=noise)


def mk_avg_maps(csv_file, model, save_dir, mk_motion_maps=False, loader=None):
    subjs, ref_niis = _subjects(csv_file)
    if getattr(model, 'recon_sums', None) is None:
        if loader is None:
            raise ValueError('mk_avg_maps: run mk_single_volumes first or pass the loader')
        mk_single_volumes(loader, model, csv_file, save_dir, write_volumes=False)
    ckpt_num = str(model.epoch).zfill(3)
    avg_dir = os.path.join(save_dir, 'reconstructions', '{}_avg_model_recons'.format(ckpt_num))
    os.makedirs(avg_dir, exist_ok=True)
    sums, counts = model.recon_sums                          # {map: (S, V) device tensor}, (S,) device tensor
    keys = list(sums.keys())
    maps = [m for m in MAPS_ALL if m in keys] + [k for k in keys if k not in MAPS_ALL]
    if not mk_motion_maps:
        maps = [m for m in maps if m in ('base', 'task', 'full_rec', 'sex')]              # :68-70
    cnt = counts.clamp_min(1).unsqueeze(1)
    out = {}
    shape = tuple(model.img_shape)
    for m in maps:
        subj_avg = (sums[m] / cnt).cpu().numpy().astype(np.float64)                      # (S, V)
        for i, s in enumerate(subjs):
            d = os.path.join(avg_dir, str(s)); os.makedirs(d, exist_ok=True)
            ref = ref_niis[i] if (i < len(ref_niis) and str(ref_niis[i]).endswith(('.nii', '.nii.gz')) and os.path.exists(str(ref_niis[i]))) else None
            nifti.write_nifti1(os.path.join(d, '{}_avg.nii'.format(m)), subj_avg[i].reshape(shape), ref)
        grand = subj_avg[:len(subjs)].mean(0)                                            # mean of subject means, :96
        ref0 = ref_niis[0] if (ref_niis and str(ref_niis[0]).endswith(('.nii', '.nii.gz')) and os.path.exists(str(ref_niis[0]))) else None
        nifti.write_nifti1(os.path.join(avg_dir, '{}_avg.nii'.format(m)), grand.reshape(shape), ref0)
        out[m] = grand.reshape(shape)
    return out


def _ref_or_none(ref_niis, i):
    ok = i < len(ref_niis) and str(ref_niis[i]).endswith(('.nii', '.nii.gz')) and os.path.exists(str(ref_niis[i]))
    return ref_niis[i] if ok else None


def mk_stat_maps(csv_file, model, save_dir, loader, mk_motion_maps=False, at_mean=False, n_perm=0, perm_seed=0):
    """Voxel-wise statistics next to the averages (an extension; VAE.map_statistics): under
    reconstructions/<ckpt>_stat_model_recons/, per subject `<map>_std.nii` (standard deviation of the map over the subject's volumes),
    `r2.nii` (variance of the data the model explains) and `<covariate map>_partial_r2.nii`; at top level `<map>_t.nii` (one-sample t
    over the subject means) and `r2_avg.nii` (mean of the subjects' r2).  Reference geometry and map selection as mk_avg_maps; one
    pass over `loader`, nothing is read back from the per-volume files.  Returns the MapStatistics.
    n_perm > 0 adds group inference on every `<map>_t.nii` (MapStatistics.group_permutation: two-sided sign-flip permutation test with
    the max-statistic, n_perm sign patterns or all 2^S of them, seeded by perm_seed): `<map>_fwe_1mp.nii` and `<map>_unc_1mp.nii` hold
    1 - p, family-wise-error corrected and uncorrected (the convention of FSL randomise: large is significant; a voxel that takes no
    part has p = 1, so exactly 0), and `perm_thresholds.csv` lists per map the tail, the number of patterns P, whether they were exhaustive, the
    critical |t| at family-wise level 0.05 and the number of voxels with a corrected p <= 0.05."""
    subjs, ref_niis = _subjects(csv_file)
    stats = model.map_statistics(loader, num_subjects=len(subjs), at_mean=at_mean)
    ckpt_num = str(model.epoch).zfill(3)
    stat_dir = os.path.join(save_dir, 'reconstructions', '{}_stat_model_recons'.format(ckpt_num))
    os.makedirs(stat_dir, exist_ok=True)
    keys = list(stats.keys)
    maps = [m for m in MAPS_ALL if m in keys] + [k for k in keys if k not in MAPS_ALL]
    if not mk_motion_maps:
        maps = [m for m in maps if m in ('base', 'task', 'full_rec', 'sex')]
    covs = [m for m in maps if m in keys[1:-1]]
    shape = tuple(model.img_shape)

    def host(t):
        return t.cpu().numpy().astype(np.float64)

    per_subject = [('{}_std.nii'.format(m), host(stats.subject_std(m))) for m in maps] + [('r2.nii', host(stats.r2()))] + \
                  [('{}_partial_r2.nii'.format(m), host(stats.partial_r2(m))) for m in covs]
    for i, s in enumerate(subjs):
        d = os.path.join(stat_dir, str(s)); os.makedirs(d, exist_ok=True)
        for name, arr in per_subject:
            nifti.write_nifti1(os.path.join(d, name), arr[i].reshape(shape), _ref_or_none(ref_niis, i))
    ref0 = _ref_or_none(ref_niis, 0)
    for m in maps:
        nifti.write_nifti1(os.path.join(stat_dir, '{}_t.nii'.format(m)), host(stats.group_t(m)).reshape(shape), ref0)
    nifti.write_nifti1(os.path.join(stat_dir, 'r2_avg.nii'), host(stats.group_r2()).reshape(shape), ref0)
    if n_perm > 0:
        rows = []
        for m in maps:
            try:
                perm = stats.group_permutation(m, n_perm=n_perm, seed=perm_seed, tail='two')
            except NoVoxelError:                                                         # (a map that is the same in every subject: nothing to test)
                zero = np.zeros(shape)
                nifti.write_nifti1(os.path.join(stat_dir, '{}_fwe_1mp.nii'.format(m)), zero, ref0)
                nifti.write_nifti1(os.path.join(stat_dir, '{}_unc_1mp.nii'.format(m)), zero, ref0)
                rows.append({'map': m, 'tail': 'two', 'P': 0, 'exhaustive': False, 't_crit_0.05': float('nan'), 'n_fwe_0.05': 0})
                continue
            nifti.write_nifti1(os.path.join(stat_dir, '{}_fwe_1mp.nii'.format(m)), host(1.0 - perm.p_fwe).reshape(shape), ref0)
            nifti.write_nifti1(os.path.join(stat_dir, '{}_unc_1mp.nii'.format(m)), host(1.0 - perm.p_unc).reshape(shape), ref0)
            rows.append({'map': m, 'tail': perm.tail, 'P': perm.n_perm, 'exhaustive': perm.exhaustive, 't_crit_0.05': perm.threshold(0.05),
                         'n_fwe_0.05': int((perm.p_fwe <= 0.05).sum())})
        pd.DataFrame(rows, columns=['map', 'tail', 'P', 'exhaustive', 't_crit_0.05', 'n_fwe_0.05']).to_csv(
            os.path.join(stat_dir, 'perm_thresholds.csv'), index=False)
    return stats
