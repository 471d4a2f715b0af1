"""Device-resident input path on the host build of the kernels (no GPU): vg_volume_gather, ResidentVolumes and ResidentLoader
against what the file loaders (setup_data_loaders without `resident_device`) yield from the same files.  Everything is compared
bit for bit; no tolerance is involved.  The -m gpu tests repeat this at model shape on the real library."""
import os

import numpy as np
import pytest
import torch

import resident_cases as R
import toy_case as T
from vae_gam_amd import DataClass_GP as D
from vae_gam_amd import _lib, dp, ops


@pytest.fixture(scope='module', autouse=True)
def emu():
    prev = _lib._LIB
    T.load_emu_library()
    yield
    _lib._LIB = prev


# (X, Y, Z, T): X = 65 and Z = 130 cross a wavefront in the load and in the store phase; (3, 19, 70) is cut into three y tiles, the
# last one short; the slab of (70, 2, 120) does not fit in LDS, so that shape is read in output order
SHAPES = [(3, 4, 5, 3), (65, 3, 33, 3), (7, 5, 130, 3)]
EDGE_SHAPES = [(3, 19, 70, 3), (70, 2, 120, 3)]
BATCHES = [[2, 0, 2, 1], [1]]

GRID = [(code, en, sc, fmt) for code in R.CODES for en in '<>' for fmt in R.FORMATS
        for sc in (('off',) if fmt.startswith('npy') else tuple(R.SCALINGS))]


@pytest.mark.parametrize('code,endian,scaling,fmt', GRID, ids=['%s-%s-%s-%s' % (R.CODES[c], 'le' if e == '<' else 'be', s, f) for c, e, s, f in GRID])
def test_gather_equals_the_host_path(tmp_path, code, endian, scaling, fmt):
    for k, shape in enumerate(SHAPES):
        R.check_file_against_host(tmp_path, 'cpu', shape, code, endian, fmt, scaling, BATCHES, seed=k)


@pytest.mark.parametrize('fmt', R.FORMATS)
@pytest.mark.parametrize('code', [4, 16, 64])
def test_gather_across_y_tiles_and_without_a_slab(tmp_path, code, fmt):
    for k, shape in enumerate(EDGE_SHAPES):
        R.check_file_against_host(tmp_path, 'cpu', shape, code, '>', fmt, 'off' if fmt.startswith('npy') else 'inexact', BATCHES, seed=k)


def test_one_batch_draws_from_files_of_different_dtype_and_byte_order(tmp_path):
    shape = (65, 3, 33, 3)
    pa = R.write_volume_file(str(tmp_path / 'a'), R.make_values(shape, 4, 1), 4, '>', 'nii.gz', 'inexact')
    pb = R.write_volume_file(str(tmp_path / 'b'), R.make_values(shape, 16, 2), 16, '<', 'npyC')
    pc = R.write_volume_file(str(tmp_path / 'c'), R.make_values(shape, 64, 3), 64, '>', 'nii', 'half')
    csv = R.write_csv(str(tmp_path / 'm.csv'), [(s, t, p) for s, p in (('a', pa), ('b', pb), ('c', pc)) for t in range(3)])
    vols = D.ResidentVolumes([csv], 'cpu')
    assert vols.dtype == 0 and len(vols.paths) == 3
    rows = [7, 1, 4, 8, 0, 4]
    got = vols.views[0].batch(torch.tensor(rows))['volume']
    assert R.same_bits(got, R.host_volumes(csv, rows))


@pytest.mark.parametrize('slope,inter,applies', [(0.0, 2.0, False), (1.0, 0.0, False), (1.0, 2.0, True), (0.0, 0.0, False)])
def test_degenerate_scaling_follows_read_nifti1(tmp_path, slope, inter, applies):
    shape = (3, 4, 5, 3)
    for code in (4, 16):
        path = str(tmp_path / ('d%d.nii' % code))
        R.write_nifti(path, R.make_values(shape, code, 5), code, '<', slope, inter)
        assert D.read_nifti1_raw(path)['scale'] is applies
        csv = R.write_csv(path + '.csv', [('s', t, path) for t in range(3)])
        got = D.ResidentVolumes([csv], 'cpu').views[0].batch(torch.tensor([0, 1, 2]))['volume']
        assert R.same_bits(got, R.host_volumes(csv, [0, 1, 2]))


def test_read_nifti1_raw_returns_the_payload_untouched(tmp_path):
    a = R.make_values((3, 4, 5, 2), 4, 0)
    path = str(tmp_path / 'r.nii.gz')
    R.write_nifti(path, a, 4, '>', 0.5, -3.0)
    h = D.read_nifti1_raw(path)
    assert (h['shape'], h['dtype'], h['endian'], h['slope'], h['inter'], h['scale']) == ((3, 4, 5, 2), 4, '>', 0.5, -3.0, True)
    assert bytes(h['payload']) == a.astype('>i2').tobytes(order='F')
    np.testing.assert_array_equal(D.read_nifti1(path), a * 0.5 + -3.0)


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    """2 subjects x 5 volumes at the toy model's 21 x 21 x 21 (an int16 .nii.gz with a slope and a float32 .npy), batch 4: the last
    minibatch is short.  The file loaders' minibatches of two epochs after torch.manual_seed(3) are drawn once and shared."""
    root = str(tmp_path_factory.mktemp('toy'))
    x, cov, xu, glm = T.make_inputs(10, 8, seed=4)
    train, test = R.subject_dataset(root, x.numpy().reshape(2, 5, *T.IMG), cov=cov.numpy().astype(np.float64))
    D._VOLUME_CACHE.clear()
    file_loaders = D.setup_data_loaders(batch_size=4, train_csv=train, test_csv=test)
    torch.manual_seed(3)
    want = R.collect(file_loaders)
    return dict(train=train, test=test, xu=xu, glm=glm, file_loaders=file_loaders, want=want, rng=torch.get_rng_state())


def test_resident_loaders_yield_the_file_loaders_batches(toy):
    res = D.setup_data_loaders(batch_size=4, train_csv=toy['train'], test_csv=toy['test'], resident_device='cpu')
    for name, ld in res.items():
        assert isinstance(ld, D.ResidentLoader)
        assert len(ld) == len(toy['file_loaders'][name]) == 3 and len(ld.dataset) == len(toy['file_loaders'][name].dataset) == 10
        assert ld.dataset.df.equals(toy['file_loaders'][name].dataset.df) and ld.batch_sampler is not None
    torch.manual_seed(3)
    got = R.collect(res)
    assert torch.equal(torch.get_rng_state(), toy['rng'])               # the same draws from the CPU generator
    assert R.assert_same_batches(got, toy['want']) == 18
    assert [int(b['volume'].shape[0]) for b in got['test'][:3]] == [4, 4, 2]
    first = torch.cat([b['vol_num'] for b in got['Shuffled_train'][:3]]).tolist()
    second = torch.cat([b['vol_num'] for b in got['Shuffled_train'][3:]]).tolist()
    assert first != second and first != sorted(first)                   # shuffled, and anew every epoch


def test_files_are_uploaded_once_and_subjects_numbered_per_csv(toy):
    vols = D.ResidentVolumes([toy['train'], toy['test']], 'cpu')
    assert len(vols.paths) == 2 and len(vols.views) == 2
    sizes = [21 ** 3 * 5 * 2, 21 ** 3 * 5 * 4]                          # int16 and float32 payloads
    assert vols.nbytes == sum(-(-s // 256) * 256 for s in sizes) == vols.arena.numel()
    offs = vols.files.numpy().view(D.VOL_FILE_DTYPE)['offset'].reshape(-1)
    assert offs.tolist() == [0, -(-sizes[0] // 256) * 256] and all(o % 256 == 0 for o in offs)
    train, test = vols.views
    assert train.subjid.tolist() == [0] * 5 + [1] * 5
    assert test.subjid.tolist() == [0] * 5 + [1] * 5                    # the test CSV starts with subj01: it is subject 0 THERE
    assert test.row_file.tolist() == [1] * 5 + [0] * 5 and test.row_vol.tolist() == [4, 3, 2, 1, 0] * 2
    assert train.covariates.dtype == torch.float32 and train.subjid.dtype == torch.int64 and train.vol_num.dtype == torch.float64


def test_refusals(tmp_path, toy):
    good = R.write_volume_file(str(tmp_path / 'good'), R.make_values((3, 4, 5, 3), 16, 0), 16, '<', 'nii')
    half = str(tmp_path / 'half.npy'); np.save(half, np.zeros((3, 4, 5, 3), dtype=np.float16))
    flat = str(tmp_path / 'flat.nii'); R.write_nifti(flat, R.make_values((3, 4, 5), 16, 0), 16)
    other = R.write_volume_file(str(tmp_path / 'other'), R.make_values((3, 4, 6, 3), 16, 0), 16, '<', 'npyC')
    for bad in (half, flat, other):
        csv = R.write_csv(str(tmp_path / 'bad.csv'), [('a', 0, good), ('b', 0, bad)])
        with pytest.raises(ValueError, match=os.path.basename(bad).replace('.', r'\.')):
            D.ResidentVolumes([csv], 'cpu')
    csv = R.write_csv(str(tmp_path / 'late.csv'), [('a', 3, good)])         # the file has volumes 0..2
    with pytest.raises(ValueError, match='good'):
        D.ResidentVolumes([csv], 'cpu')
    csv = R.write_csv(str(tmp_path / 'ok.csv'), [('a', t, good) for t in range(3)])
    with pytest.raises(ValueError, match=r'768 bytes.*more than the 1 allowed'):
        D.ResidentVolumes([csv], 'cpu', max_bytes=1)
    view = D.ResidentVolumes([csv], 'cpu').views[0]
    calls = []
    lib = _lib.get_lib()
    orig = lib.call
    lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        for rows in ([0, 3], [-1]):
            with pytest.raises(IndexError):
                list(D.ResidentLoader(view, [rows]))
        assert calls == []                                               # refused before any launch
        assert len(list(D.ResidentLoader(view, [[0, 2]]))) == 1 and calls == ['vg_volume_gather']
    finally:
        del lib.call
    idx = torch.zeros(1, dtype=torch.int64)
    vols = view.volumes
    with pytest.raises(_lib.VgError, match='unknown dtype code 3'):
        ops.volume_gather(vols.arena, vols.files, view.row_file, view.row_vol, idx, vols.shape, 3, D.GLOBAL_MAX)
    rc = lib.dll.vg_volume_gather(None, None, None, None, None, 1, 3, 4, 5, 16, 3284.5, None, None)
    assert rc == 1 and b'null argument' in lib.dll.vg_last_error()
    out = torch.empty(1, 3, 4, 5)
    rc = lib.dll.vg_volume_gather(vols.arena.data_ptr(), vols.files.data_ptr(), view.row_file.data_ptr(), view.row_vol.data_ptr(),
                                  idx.data_ptr(), 0, 3, 4, 5, 16, 3284.5, out.data_ptr(), None)
    assert rc == 1 and b'bad argument' in lib.dll.vg_last_error()


def test_product_library_refuses_host_tensors(tmp_path, monkeypatch):
    """Without the injected handle's host_pointers_ok the resident path refuses a CPU device, like the rest of ops."""
    class Product:
        host_pointers_ok = False
    monkeypatch.setattr(_lib, '_LIB', Product())
    good = R.write_volume_file(str(tmp_path / 'good'), R.make_values((3, 4, 5, 3), 16, 0), 16, '<', 'nii')
    csv = R.write_csv(str(tmp_path / 'ok.csv'), [('a', t, good) for t in range(3)])
    with pytest.raises(RuntimeError, match='no CPU path'):
        D.ResidentVolumes([csv], 'cpu')


def test_sharded_ranks_draw_the_halves_of_the_one_process_batches(toy):
    view = D.ResidentVolumes([toy['train']], 'cpu').views[0]
    n = len(view)
    whole = list(D.ResidentLoader(view, dp.ShardedBatchSampler(n, 4, 0, 1, shuffle=True, seed=1)))
    halves = [list(D.ResidentLoader(view, dp.ShardedBatchSampler(n, 4, r, 2, shuffle=True, seed=1))) for r in (0, 1)]
    assert len(whole) == len(halves[0]) == len(halves[1]) == 3
    for w, a, b in zip(whole, halves[0], halves[1]):
        for k in w:
            assert R.same_bits(torch.cat([a[k], b[k]]), w[k]), k
    assert [int(w['volume'].shape[0]) for w in whole] == [4, 4, 2]


def test_shard_loaders_rebuilds_resident_loaders_over_the_same_view(toy):
    res = D.setup_data_loaders(batch_size=4, train_csv=toy['train'], test_csv=toy['test'], resident_device='cpu')

    class Ctx:
        rank, world_size = 1, 2
    out = dp.DataParallelContext.shard_loaders(Ctx(), res, 4, seed=1)
    for name, ld in out.items():
        assert isinstance(ld, D.ResidentLoader) and ld.view is res[name].view and isinstance(ld.batch_sampler, dp.ShardedBatchSampler)
        assert ld.batch_sampler.rank == 1 and ld.batch_sampler.shuffle == (name == 'Shuffled_train')
    assert [int(b['volume'].shape[0]) for b in out['test']] == [2, 2, 1]


def test_train_epoch_over_the_resident_loader_equals_the_file_loader(tmp_path):
    """Two train steps (2 subjects x 2 volumes, batch 2: the emulated step costs seconds per sample) of identically seeded models,
    one fed by the file loader, one by the resident loader: the same epoch loss, as in test_device_prefetcher_...'s pattern."""
    x, cov, xu, glm = T.make_inputs(4, 8, seed=4)
    train, test = R.subject_dataset(str(tmp_path), x.numpy().reshape(2, 2, *T.IMG), cov=cov.numpy().astype(np.float64))
    D._VOLUME_CACHE.clear()
    plain = D.setup_data_loaders(batch_size=2, train_csv=train, test_csv=test)
    res = D.setup_data_loaders(batch_size=2, train_csv=train, test_csv=test, resident_device='cpu')
    losses = []
    for ld in (plain['UnShuffled_train'], res['UnShuffled_train']):
        m = T.make_model(3, xu, glm, seed=1)
        torch.manual_seed(7)
        losses.append(m.train_epoch(ld))
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
