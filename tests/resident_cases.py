"""Shared pieces of the device-resident input path tests (test_resident_input_emu.py on the host build of the kernels,
test_resident_input_gpu.py on the MI355X): subject files of every dtype / byte order / layout the volume gather reads, written with
`struct` (nifti.write_nifti1 only writes float32), the CSVs that name them, and the host path every result is compared with bit for bit:
what setup_data_loaders without `resident_device` yields from the same files (read_nifti1 -> FMRIDataset.__getitem__ -> ToTensor)."""
import gzip
import os
import struct

import numpy as np
import pandas as pd
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import DataClass_GP as D
from vae_gam_amd import ops

CODES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 256: 'i1', 512: 'u2', 768: 'u4'}
# scl_slope, scl_inter.  (0.5, -3) cannot tell v*slope + inter from a fused multiply-add (the product by a power of two is exact);
# (0.37, 1.7) can: there the product rounds.
SCALINGS = {'off': (1.0, 0.0), 'half': (0.5, -3.0), 'inexact': (0.37, 1.7)}
FORMATS = ('nii', 'nii.gz', 'npyC', 'npyF')
CSV_COLS = ['subjid', 'volume #', 'nii_path', 'task', 'x', 'y', 'z', 'rot_x', 'rot_y', 'rot_z', 'sex']


def make_values(shape, code, seed):
    """Finite values of NIfTI dtype `code` with zeros and negatives (where the dtype has them) and the dtype's extremes; floats stay
    between 1e-2 and 1e4 in magnitude (or are exactly 0), so no quotient by 3284.5 is subnormal at any of the scalings."""
    rng = np.random.Generator(np.random.PCG64(seed))
    dt = np.dtype(CODES[code])
    n = int(np.prod(shape))
    if dt.kind == 'f':
        v = rng.uniform(1e-2, 1e4, n) * rng.choice([-1.0, 1.0], n)
        v[rng.integers(0, n, max(1, n // 10))] = 0.0
        v = v.astype(dt)
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        v[rng.integers(0, n, max(1, n // 10))] = 0
        v[:2] = (info.min, info.max)
    return v.reshape(shape)


def write_nifti(path, a, code, endian='<', slope=1.0, inter=0.0):
    """`a` (any rank) as a single-file NIfTI-1 of datatype `code` in byte order `endian`, gzipped when the name says so."""
    h = bytearray(348)
    struct.pack_into(endian + 'i', h, 0, 348)
    struct.pack_into(endian + '8h', h, 40, a.ndim, *(list(a.shape) + [1] * (7 - a.ndim)))
    struct.pack_into(endian + '2h', h, 70, code, 8 * np.dtype(CODES[code]).itemsize)
    struct.pack_into(endian + '8f', h, 76, *([1.0] * 8))
    struct.pack_into(endian + 'f', h, 108, 352.0)
    struct.pack_into(endian + '2f', h, 112, slope, inter)
    h[344:348] = b'n+1\x00'
    data = np.asarray(a).astype(np.dtype(endian + CODES[code])).tobytes(order='F')
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'wb') as f:
        f.write(bytes(h) + b'\x00' * 4 + data)


def write_volume_file(stem, a, code, endian, fmt, scaling='off'):
    """`a` (X, Y, Z, T) in one of FORMATS -> the path.  .npy files carry no scaling."""
    if fmt.startswith('npy'):
        assert scaling == 'off'
        path = stem + '.npy'
        b = np.asarray(a).astype(np.dtype(endian + CODES[code]))
        np.save(path, np.asfortranarray(b) if fmt == 'npyF' else np.ascontiguousarray(b))
        return path
    path = stem + '.' + fmt
    write_nifti(path, a, code, endian, *SCALINGS[scaling])
    return path


def write_csv(csv, rows, seed=0):
    """rows: [(subject name, volume number, file path)] -> a CSV in the loaders' layout with seeded covariates."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cov = rng.normal(size=(len(rows), 8))
    df = pd.DataFrame([[s, t, p] + cov[i].tolist() for i, (s, t, p) in enumerate(rows)], columns=CSV_COLS)
    df.to_csv(csv)
    return csv


def host_volumes(csv, rows):
    """volume tensors of CSV rows `rows` through the file path: FMRIDataset.__getitem__ + ToTensor, stacked as the collate does."""
    D._VOLUME_CACHE.clear()
    ds = D.FMRIDataset(csv_file=csv, transform=D.ToTensor())
    out = torch.stack([ds[int(i)]['volume'] for i in rows])
    D._VOLUME_CACHE.clear()
    return out


def same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def check_file_against_host(tmp, device, shape, code, endian, fmt, scaling, batches, seed=0):
    """One subject file: the gather (through ResidentVolumes, i.e. the kernel instance of the file's dtype, and again with dtype 0,
    the instance that reads each descriptor's code) against the host path, for every index list of `batches`."""
    a = make_values(shape, code, seed)
    path = write_volume_file(os.path.join(str(tmp), 'f_%s_%d' % ('x'.join(map(str, shape)), seed)), a, code, endian, fmt, scaling)
    csv = write_csv(path + '.csv', [('s0', t, path) for t in range(shape[3])])
    vols = D.ResidentVolumes([csv], device)
    view = vols.views[0]
    assert vols.dtype == code and vols.shape == tuple(shape[:3])
    for rows in batches:
        ref = host_volumes(csv, rows)
        idx = torch.tensor(rows, dtype=torch.int64, device=device)
        got = view.batch(idx)['volume']
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (len(rows),) + tuple(shape[:3])
        assert same_bits(got, ref), (shape, code, endian, fmt, scaling, rows, float((got.cpu() - ref).abs().max()))
        got0 = ops.volume_gather(vols.arena, vols.files, view.row_file, view.row_vol, idx, vols.shape, 0, D.GLOBAL_MAX)
        assert same_bits(got0, ref), ('dtype 0', shape, code, endian, fmt, scaling, rows)


def subject_dataset(root, volumes, cov=None, seed=0):
    """volumes (S, T, X, Y, Z) in [0, 1] -> S subject files of DIFFERENT kinds (int16 .nii.gz with a slope, float32 C-order .npy,
    big-endian float32 .nii, ...), a train CSV and a test CSV that names the same files with the subjects in reverse order."""
    os.makedirs(root, exist_ok=True)
    S, T = volumes.shape[:2]
    kinds = [(4, '<', 'nii.gz', 'inexact'), (16, '<', 'npyC', 'off'), (16, '>', 'nii', 'off'), (512, '>', 'nii', 'half')]
    rows = []
    for s in range(S):
        code, en, fmt, sc = kinds[s % len(kinds)]
        slope, inter = struct.unpack('<2f', struct.pack('<2f', *SCALINGS[sc]))      # as the header holds them: fp32
        a = np.moveaxis(volumes[s], 0, -1) * 3284.5
        if np.dtype(CODES[code]).kind != 'f':
            a = np.rint((a - inter) / slope)
        path = write_volume_file(os.path.join(root, 'subj%02d' % s), a, code, en, fmt, sc)
        rows += [('subj%02d' % s, t, path) for t in range(T)]
    train = os.path.join(root, 'train.csv')
    write_csv(train, rows, seed)
    if cov is not None:
        df = pd.read_csv(train, index_col=0)
        df.iloc[:, 3:3 + cov.shape[1]] = cov
        df.to_csv(train)
    df = pd.read_csv(train, index_col=0)
    test = os.path.join(root, 'test.csv')
    df.iloc[::-1].reset_index(drop=True).to_csv(test)
    return train, test


def collect(loaders, epochs=2):
    """{loader name: every minibatch of `epochs` consecutive epochs, tensors on the host}, drawn in a fixed order of the loaders."""
    out = {}
    for name in ('Shuffled_train', 'UnShuffled_train', 'test'):
        out[name] = [{k: v.cpu() for k, v in b.items()} for _ in range(epochs) for b in loaders[name]]
    return out


def assert_same_batches(got, want):
    """Every key of every minibatch, bit for bit; -> number of minibatches compared."""
    n = 0
    for name in want:
        assert len(got[name]) == len(want[name]), name
        for a, b in zip(got[name], want[name]):
            assert list(a.keys()) == list(b.keys())
            for k in b:
                assert same_bits(a[k], b[k]), (name, k)
            n += 1
    return n
