"""Device-resident input path on the MI355X (-m gpu): vg_volume_gather at model shape for every dtype / byte order / scaling, a file
behind the 2^32-byte mark of the arena, the resident loaders and a train epoch against the file loaders, and the command line with
--device_resident --hip_graph against the same run without them.  Everything is compared bit for bit with the host path."""
import os

import numpy as np
import pytest
import torch

import resident_cases as R
import vae_gam_amd  # noqa: F401
from vae_gam_amd import DataClass_GP as D
from vae_gam_amd import _lib, ops, synthetic
from vae_gam_amd.vae_reg_GP import VAE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def product_library():
    import emu_inject; emu_inject.use_product_library()
    _lib.get_lib()
    yield


# the model's volume (ten y tiles of five rows, the last one short) and a shape whose x crosses a wavefront
SHAPES = [(41, 49, 35, 3), (65, 3, 33, 3)]
ROWS = [[2, 0, 2, 1, 1]]
GRID = [(code, en, sc) for code in R.CODES for en in '<>' for sc in R.SCALINGS]


@pytest.mark.parametrize('code,endian,scaling', GRID, ids=['%s-%s-%s' % (R.CODES[c], 'le' if e == '<' else 'be', s) for c, e, s in GRID])
def test_gather_equals_the_host_path_at_model_shape(tmp_path, code, endian, scaling):
    for k, shape in enumerate(SHAPES):
        R.check_file_against_host(tmp_path, 'cuda', shape, code, endian, 'nii', scaling, ROWS, seed=k)


@pytest.mark.parametrize('fmt', ['npyC', 'npyF', 'nii.gz'])
@pytest.mark.parametrize('code', [4, 16])
def test_gather_reads_npy_layouts_and_shapes_without_a_slab(tmp_path, code, fmt):
    for k, shape in enumerate([(41, 49, 35, 3), (70, 2, 120, 3)]):
        R.check_file_against_host(tmp_path, 'cuda', shape, code, '>', fmt, 'off', ROWS, seed=k)


def test_a_file_behind_the_4_gib_mark_of_the_arena(tmp_path):
    """64-bit byte offsets: a 4.5 GB arena, never filled, with one small int16 file placed behind byte 2^32."""
    shape = (7, 5, 9, 3)
    a = R.make_values(shape, 4, 0)
    path = R.write_volume_file(str(tmp_path / 'far'), a, 4, '<', 'nii', 'inexact')
    csv = R.write_csv(path + '.csv', [('s', t, path) for t in range(3)])
    raw = D.read_nifti1_raw(path)
    arena = torch.empty(4_500_000_000, dtype=torch.uint8, device='cuda')
    off = (1 << 32) + 3 * 256
    payload = torch.from_numpy(np.frombuffer(raw['payload'], dtype=np.uint8).copy())
    arena[off:off + payload.numel()].copy_(payload)
    table = np.zeros(1, dtype=D.VOL_FILE_DTYPE)
    table[0] = (off, 1, 7, 35, 315, raw['slope'], raw['inter'], 4, 0, int(raw['scale']), 0)
    files = torch.from_numpy(table.view(np.uint8).reshape(1, -1)).cuda()
    row_file = torch.zeros(3, dtype=torch.int32, device='cuda')
    row_vol = torch.arange(3, dtype=torch.int32, device='cuda')
    rows = [2, 0, 1, 2]
    got = ops.volume_gather(arena, files, row_file, row_vol, torch.tensor(rows, device='cuda'), shape[:3], 4, D.GLOBAL_MAX)
    assert R.same_bits(got, R.host_volumes(csv, rows))


def test_one_batch_draws_from_files_of_different_kinds(tmp_path):
    ds = synthetic.make_dataset(num_subjects=4, vols_per_subject=2, num_covariates=8, seed=5)
    train, test = R.subject_dataset(str(tmp_path), ds['volumes'].reshape(4, 2, 41, 49, 35))
    vols = D.ResidentVolumes([train, test], 'cuda')
    assert vols.dtype == 0 and len(vols.paths) == 4
    rows = [7, 0, 3, 4, 2, 5, 5]
    got = vols.views[0].batch(torch.tensor(rows, device='cuda'))['volume']
    assert R.same_bits(got, R.host_volumes(train, rows))


def test_resident_loaders_and_a_train_epoch_equal_the_file_loaders(tmp_path):
    ds = synthetic.make_dataset(num_subjects=2, vols_per_subject=5, num_covariates=8, seed=3)
    csv, _ = synthetic.write_csvs(ds, str(tmp_path))
    plain = D.setup_data_loaders(batch_size=4, train_csv=csv, test_csv=csv)
    res = D.setup_data_loaders(batch_size=4, train_csv=csv, test_csv=csv, resident_device='cuda')
    assert all(isinstance(v, D.ResidentLoader) for v in res.values())
    assert res['test'].view.volumes is res['Shuffled_train'].view.volumes and len(res['test'].view.volumes.paths) == 2
    for name in plain:
        assert len(res[name]) == len(plain[name]) == 3 and len(res[name].dataset) == len(plain[name].dataset) == 10
    torch.manual_seed(3)
    want = R.collect(plain)
    rng = torch.get_rng_state()
    torch.manual_seed(3)
    got = {k: v for k, v in R.collect(res).items()}
    assert torch.equal(torch.get_rng_state(), rng)
    assert all(t.is_cuda for b in res['test'] for t in b.values())
    assert R.assert_same_batches(got, want) == 18
    losses = []
    for ld in (plain['UnShuffled_train'], res['UnShuffled_train']):
        torch.manual_seed(1)
        m = VAE(num_covariates=8, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda', save_dir=str(tmp_path))
        torch.manual_seed(7)
        losses.append(m.train_epoch(ld))
    assert np.isfinite(losses[0]) and losses[0] == losses[1]


def test_cli_device_resident_with_hip_graph_trains_what_the_plain_cli_trains(tmp_path):
    """multsubj_reg_run_GP.main with --device_resident --hip_graph against the same call without them, same --seed: the same
    minibatches in the same order and a replayed step that equals the eager one, so the epoch losses are equal, and both runs write
    the export files of test_cli_trains_then_exports_like_the_reference_wrapper."""
    from vae_gam_amd import multsubj_reg_run_GP as cli
    ds = synthetic.make_dataset(num_subjects=2, vols_per_subject=6, num_covariates=8, seed=3)
    csv, glm_csv = synthetic.write_csvs(ds, str(tmp_path / 'data'))
    models = {}
    for name, extra in (('plain', []), ('resident', ['--device_resident', 'True', '--hip_graph', 'True'])):
        out = str(tmp_path / name)
        m = cli.main(['--train_csv', csv, '--test_csv', csv, '--glm_maps', glm_csv, '--save_dir', out, '--batch-size', '4',
                      '--epochs', '2', '--test_freq', '1', '--seed', '5'] + extra)
        models[name] = m
        assert m.epoch == 2
        gp_dir = os.path.join(out, '002_GP_plots')
        rec = os.path.join(out, 'reconstructions', '002_model_recons')
        avg = os.path.join(out, 'reconstructions', '002_avg_model_recons')
        assert sorted(os.listdir(gp_dir)) == sorted('002_GP_%s_full.csv' % n for n in ['x', 'y', 'z', 'xrot', 'yrot', 'zrot'])
        subj = sorted(os.listdir(rec))
        assert subj == ['subj00', 'subj01'] and len(os.listdir(os.path.join(rec, subj[0]))) == 6
        assert len(os.listdir(os.path.join(rec, subj[0], 'vol_0'))) == 10
        assert len([f for f in os.listdir(avg) if f.endswith('.nii')]) == 10
    assert models['resident'].use_hip_graph and not models['plain'].use_hip_graph
    graphs = models['resident']._graphs
    assert graphs and all(g is not False for g in graphs.values())           # the step was captured and replayed, not refused
    assert models['plain'].loss == models['resident'].loss
    assert len(models['plain'].loss['train']) == 2 and len(models['plain'].loss['test']) == 2
