"""Command-line wrapper to train the VAE-GAM on MI355X (same flags as the reference's
multsubj_reg_run_GP.py:19-56; run as `python -m vae_gam_amd.multsubj_reg_run_GP ...`).

After training -- or straight from a checkpoint with `--recons_only` -- the wrapper runs the reference's export pipeline
(multsubj_reg_run_GP.py:79-92): `model.project_latent` (UMAP projection of the latent means on the HIP kernels of
latent_projection.py: `<epoch>_temp.pdf` and `<epoch>_latent_projection.csv`), `model.plot_GPs` (per-covariate GP posterior
CSVs), `recon.mk_single_volumes` (one NIfTI per volume and map) and `recon.mk_avg_maps(mk_motion_maps=True)` (subject and
grand averages), all on the training set as the reference does.  With `--stat_maps` (an extension) `recon.mk_stat_maps` follows:
voxel-wise standard deviations, second-level t maps and variance-explained maps in a directory of their own; `--stat_perm N` adds
permutation p-maps of the t maps (sign flips, max-statistic) next to them.

Multi-GPU: launch with torch.distributed.run, one process per GPU; the wrapper picks up RANK / LOCAL_RANK / WORLD_SIZE,
`--batch-size` stays the GLOBAL minibatch and every rank draws its own slice of it (dp.ShardedBatchSampler); checkpoints
and the export pipeline run on rank 0 only.
"""
import argparse
import os
import time

import torch

from . import DataClass_GP as data
from . import vae_reg_GP as vae_reg
from .utils import str2bool


def build_parser():
    parser = argparse.ArgumentParser(description='user args for vae_gam model')
    parser.add_argument('--train_csv', type=str, metavar='N', default='', help='Full path to csv file with train dset.')
    parser.add_argument('--test_csv', type=str, metavar='N', default='', help='Full path to csv file with test dset.')
    parser.add_argument('--save_dir', type=str, metavar='N', default='', help='Dir where model params are saved to.')
    parser.add_argument('--batch-size', type=int, default=32, metavar='N', help='Input batch size for training (default: 32)')
    parser.add_argument('--epochs', type=int, default=300, metavar='N', help='Number of epochs to train (default: 300)')
    parser.add_argument('--seed', type=int, default=1, metavar='S', help='Random seed (default: 1)')
    parser.add_argument('--save_freq', type=int, default=100, metavar='N', help='How many epochs to wait before saving training status.')
    parser.add_argument('--test_freq', type=int, default=200, metavar='N', help='How many epochs to wait before testing.')
    parser.add_argument('--split', type=int, metavar='N', default=98, help='# of volumes per subject (one colour per chunk of this size in the latent projection plot).')
    parser.add_argument('--glm_reg_scale', type=float, metavar='N', default=1.0, help='Scaling factor for GLM map regularization term (default: 1)')
    parser.add_argument('--glm_maps', type=str, metavar='N', default='', help='Path to csv file containing matrix with approximate GLM maps.')
    parser.add_argument('--num_inducing_pts', type=int, metavar='N', default=6, help='Number of inducing points for each regressor 1D GP.')
    parser.add_argument('--gp_kl_scale', type=float, metavar='N', default=10.0, help='Scaling factor for the gain KL terms.')
    parser.add_argument('--from_ckpt', type=str2bool, nargs='?', const=True, default=False, help='Start from a saved model state.')
    parser.add_argument('--ckpt_path', type=str, metavar='N', default='', help='Path to ckpt with saved model state to be loaded.')
    parser.add_argument('--recons_only', type=str2bool, nargs='?', const=True, default=False, help='Skip training.')
    parser.add_argument('--neural_covariates', type=str2bool, nargs='?', const=True, default=True,
                        help='Covariate set includes neural/biological effects to be convolved with the HRF.')
    parser.add_argument('--gp_jitter', type=float, metavar='N', default=0.0,
                        help='(extension) Ku + jitter*I in the GP posteriors; 0 = the reference\'s plain inverse. Needed for dense inducing grids '
                             '(e.g. --num_inducing_pts 64: 1e-4), where Ku is singular in any precision.')
    parser.add_argument('--max_grad_norm', type=float, metavar='N', default=None,
                        help='(extension) Clip the global gradient norm to N inside the step (torch.nn.utils.clip_grad_norm_\'s factor). Default: off.')
    parser.add_argument('--skip_nonfinite', type=str2bool, nargs='?', const=True, default=False,
                        help='(extension) Skip a step whose gradient holds an inf / nan (parameters and Adam state untouched) instead of '
                             'writing it into every parameter; skipped steps are counted and reported per epoch.')
    parser.add_argument('--device_resident', type=str2bool, nargs='?', const=True, default=False,
                        help='(extension) Upload every subject file once and assemble the minibatches on the GPU from an index list '
                             '(DataClass_GP.ResidentVolumes) instead of reading them through the host loaders; the same minibatches in '
                             'the same order.  The files must fit in half of the free device memory.')
    parser.add_argument('--hip_graph', type=str2bool, nargs='?', const=True, default=False,
                        help='(extension) Capture the train step into a hipGraph once per batch shape and replay it; where capture is '
                             'refused the step runs as eager launches and says so.')
    parser.add_argument('--img_shape', type=int, nargs=3, metavar=('X', 'Y', 'Z'), default=list(vae_reg.IMG_SHAPE),
                        help='(extension) Spatial shape of the volumes (default: the reference\'s 41 49 35).  Any grid with axes >= 19; one '
                             'whose axes are not all = 2 (mod 4) is zero-padded by up to 3 voxels per axis inside the network, while the '
                             'loss and every exported map stay on the grid given here.  The padded grid X x H x W must have W <= 130 and '
                             'H*W <= 7667 (91 109 91 -> 94x110x94 is refused).')
    parser.add_argument('--mask', type=str, metavar='PATH', default='',
                        help='(extension) Brain mask of --img_shape (.nii, .nii.gz or .npy; nonzero = in-brain; the first volume of a 4-D '
                             'file).  The log-likelihood and the GLM distance sum over the voxels of the mask only, and every exported map '
                             'is 0 outside it.  Default: every voxel counts, as the reference.')
    parser.add_argument('--stat_maps', type=str2bool, nargs='?', const=True, default=False,
                        help='(extension) After the averages, also write voxel-wise statistics under reconstructions/<ckpt>_stat_model_recons/: '
                             'per subject <map>_std.nii, r2.nii and <covariate map>_partial_r2.nii, at top level <map>_t.nii and r2_avg.nii '
                             '(one more pass over the training set; sums kept on the GPU).  Default: off.')
    parser.add_argument('--stat_perm', type=int, default=0, metavar='N',
                        help='(extension) With --stat_maps: group inference on every <map>_t.nii by a two-sided sign-flip permutation test with '
                             'the max-statistic, N sign patterns (all 2^S of them where 2^S <= N; at most 2^20, 2 to 64 subjects): adds '
                             '<map>_fwe_1mp.nii and <map>_unc_1mp.nii (1 - p, family-wise-error corrected and uncorrected) and '
                             'perm_thresholds.csv.  Default 0: off.')
    parser.add_argument('--stat_perm_seed', type=int, default=0, metavar='SEED',
                        help='(extension) Seed of the sign patterns of --stat_perm (drawn on the CPU: the same on every device).  Default 0.')
    return parser


def check_img_shape(img_shape, loaders):
    """ValueError if the first subject file of the training set does not hold volumes of --img_shape (read from the file's header)."""
    loader = loaders.get('UnShuffled_train')
    df = getattr(getattr(loader, 'dataset', None), 'df', None)
    if df is None or not len(df):
        return
    path = df.iloc[0, 3]
    found = tuple(int(v) for v in data._probe_volume_file(path)['shape'][:3])
    if found != tuple(img_shape):
        raise ValueError('--img_shape is %s but the volumes of %s have the spatial shape %s'
                         % ('x'.join(map(str, img_shape)), path, 'x'.join(map(str, found))))


def check_mask(mask_path, img_shape):
    """--mask read and checked against --img_shape before the model is built: SystemExit for a file that is missing or of an unknown
    kind, ValueError for a mask of another shape or with no voxel set.  Returns the mask array, or None without --mask."""
    if not mask_path:
        return None
    if not os.path.exists(mask_path):
        raise SystemExit('--mask %s does not exist' % mask_path)
    if not mask_path.endswith(('.nii', '.nii.gz', '.npy')):
        raise SystemExit('--mask %s: expected a .nii, .nii.gz or .npy file' % mask_path)
    mask = vae_reg.VAE.read_mask(mask_path)
    if tuple(mask.shape) != tuple(img_shape):
        raise ValueError('--img_shape is %s but the mask %s has the spatial shape %s'
                         % ('x'.join(map(str, img_shape)), mask_path, 'x'.join(map(str, mask.shape))))
    if not (mask != 0).any():
        raise ValueError('--mask %s has no voxel set' % mask_path)
    return mask


def main(argv=None):
    args = build_parser().parse_args(argv)
    torch.manual_seed(args.seed)
    if args.save_dir == '':
        args.save_dir = os.getcwd()
    if not os.path.exists(args.save_dir):
        os.makedirs(args.save_dir, exist_ok=True)
    main_start = time.time()
    dp = None
    if int(os.environ.get('WORLD_SIZE', '1')) > 1 or os.environ.get('VG_DP_FORCE') == '1':
        from . import dp as dpmod
        dp = dpmod.DataParallelContext.from_env()
    rank = 0 if dp is None else dp.rank
    if dp is not None and args.batch_size % dp.world_size:
        raise SystemExit('--batch-size %d (the GLOBAL minibatch) must be a multiple of the %d ranks' % (args.batch_size, dp.world_size))
    check_batch_size(args.batch_size, 1 if dp is None else dp.world_size, os.environ.get('VG_DP_GAIN', 'global'))
    mask = check_mask(args.mask, args.img_shape)
    # the reference's loaders (whole data set, GLOBAL minibatch, multsubj_reg_run_GP.py:69): what the export pipeline iterates -- gains
    # (joint draw, HRF along the batch) and the decoder's batch statistics depend on the batch composition, so the exported maps must
    # see the batches a single process would; under data parallelism the train / test loops get re-built loaders that hand each rank
    # its slice of every global minibatch (they only take the data sets from these)
    # (single process on a GPU: minibatches are staged in pinned memory and copied one batch ahead on a side stream)
    # (--device_resident: the subject files live in HBM and a kernel assembles the minibatches; every rank holds all of them)
    if args.device_resident:
        if not torch.cuda.is_available():
            raise SystemExit('--device_resident needs a GPU')
        full_loaders = data.setup_data_loaders(batch_size=args.batch_size, train_csv=args.train_csv, test_csv=args.test_csv,
                                               resident_device='cuda')
    else:
        full_loaders = data.setup_data_loaders(batch_size=args.batch_size, train_csv=args.train_csv, test_csv=args.test_csv,
                                               prefetch_device='cuda' if (dp is None and torch.cuda.is_available()) else None)
    loaders_dict = full_loaders if dp is None else dp.shard_loaders(full_loaders, args.batch_size, args.seed)
    check_img_shape(args.img_shape, full_loaders)
    model = vae_reg.VAE(num_inducing_pts=args.num_inducing_pts, gp_kl_scale=args.gp_kl_scale,
                        glm_reg_scale=args.glm_reg_scale, glm_maps=args.glm_maps, save_dir=args.save_dir,
                        csv_files=[args.train_csv, args.test_csv], neural_covariates=args.neural_covariates,
                        data_parallel=dp, dp_gain=os.environ.get('VG_DP_GAIN', 'global'), gp_jitter=args.gp_jitter,
                        max_grad_norm=args.max_grad_norm, skip_nonfinite=args.skip_nonfinite, img_shape=tuple(args.img_shape), mask=mask)
    model.use_hip_graph = bool(args.hip_graph)
    if args.from_ckpt:
        assert os.path.exists(args.ckpt_path), 'Oops, looks like ckpt file given does NOT exist!'
        print('=' * 40)
        print('Loading model state from: {}'.format(args.ckpt_path))
        model.load_state(filename=args.ckpt_path)
        if args.max_grad_norm is not None or args.skip_nonfinite:       # the checkpoint brings its own guard setting (none = off);
            model.set_grad_guard(args.max_grad_norm, args.skip_nonfinite)   # flags given on this command line take precedence
    if not args.recons_only:
        model.train_loop(loaders_dict, epochs=args.epochs, test_freq=args.test_freq, save_freq=args.save_freq,
                         save_dir=args.save_dir)
    else:
        assert args.from_ckpt, 'To choose recons_only option, --from_ckpt needs to be TRUE.'
    export_outputs(model, full_loaders, args, dp)
    if rank == 0:
        print('Total model runtime (seconds): {}'.format(time.time() - main_start))
    return model


def check_batch_size(batch_size, world_size=1, dp_gain='global'):
    """Refuse, before any data is loaded, a --batch-size whose gains the gain block cannot draw jointly (ops.GAIN_MAX_BATCH): the
    training step draws the global minibatch (dp_gain='global') or each rank's slice ('local'); the export pipeline always draws the
    whole minibatch in one process."""
    from . import ops
    train = batch_size if dp_gain == 'global' else batch_size // max(1, world_size)
    try:
        ops.check_gain_batch(train, '--batch-size %d on %d rank(s) with dp_gain=%r' % (batch_size, world_size, dp_gain))
        ops.check_gain_batch(batch_size, '--batch-size %d in the export pipeline (one process, whole minibatches)' % batch_size)
    except ValueError as e:
        raise SystemExit(str(e))


def export_outputs(model, loaders_dict, args, dp=None):
    """The post-training block of the reference wrapper (multsubj_reg_run_GP.py:83-86 and, for --recons_only, :89-92), on
    the training set.  Rank 0 only under data parallelism: the replicas are identical and the export runs single-process.  The
    process group is torn down FIRST (after one barrier): the other ranks return instead of sitting in a collective for as long as
    the export takes (file output of every volume x map: minutes on a real data set, past the RCCL watchdog's patience)."""
    from . import build_model_recons as recon
    if dp is not None:
        dp.barrier()
        dp.shutdown()
        if dp.rank != 0:
            return
    saved_dp, model.dp = model.dp, None
    try:
        model.project_latent(loaders_dict, title="Latent Space plot", split=args.split, save_dir=args.save_dir)
        model.plot_GPs(csv_file=args.train_csv, save_dir=args.save_dir)
        recon.mk_single_volumes(loaders_dict['UnShuffled_train'], model, args.train_csv, args.save_dir)
        recon.mk_avg_maps(args.train_csv, model, args.save_dir, mk_motion_maps=True)
        if getattr(args, 'stat_maps', False):
            recon.mk_stat_maps(args.train_csv, model, args.save_dir, loaders_dict['UnShuffled_train'], mk_motion_maps=True,
                               n_perm=getattr(args, 'stat_perm', 0), perm_seed=getattr(args, 'stat_perm_seed', 0))
    finally:
        model.dp = saved_dp


if __name__ == "__main__":
    main()
