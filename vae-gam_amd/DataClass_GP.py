"""Dataset / loaders for the VAE-GAM (drop-in surface of the reference's DataClass_GP.py).

Same CSV layout (positional columns: index, subjid, volume #, nii_path, task, x, y, z, rot_x,
rot_y, rot_z, sex; DataClass_GP.py:31-46), same sample dictionary (DataClass_GP.py:63-71) and
same loader dictionary (DataClass_GP.py:73-89).  Differences that matter on an MI355X node:
each 4-D file is decoded ONCE and kept (the reference re-reads the whole 4-D NIfTI for every
sample, DataClass_GP.py:48), `.npy` volumes are memory-mapped, and `DeviceResidentData` keeps a
whole synthetic or pre-loaded set in HBM so the train loop never touches the host.
"""
import gzip
import os
import struct
import warnings

import numpy as np
import pandas as pd
import torch
from torch.utils.data import DataLoader, Dataset

GLOBAL_MAX = 3284.5       # DataClass_GP.py:49


NIFTI_DTYPES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 256: 'i1', 512: 'u2', 768: 'u4'}


def _nifti1_header(head, path):
    """Fields of a NIfTI-1 header (its first 348 bytes) that the readers use."""
    if len(head) >= 348 and struct.unpack('<i', head[:4])[0] == 348:
        en = '<'
    elif len(head) >= 348 and struct.unpack('>i', head[:4])[0] == 348:
        en = '>'
    else:
        raise ValueError('%s: not a NIfTI-1 file' % path)
    dim = struct.unpack(en + '8h', head[40:56])
    datatype, bitpix = struct.unpack(en + '2h', head[70:74])
    vox_offset = int(struct.unpack(en + 'f', head[108:112])[0])
    slope, inter = struct.unpack(en + '2f', head[112:120])
    if datatype not in NIFTI_DTYPES:
        raise ValueError('%s: unsupported NIfTI datatype %d' % (path, datatype))
    shape = tuple(int(d) for d in dim[1:1 + dim[0]])
    # scl_slope / scl_inter apply unless they are the identity or slope is 0 ("no scaling" in the standard)
    scale = (slope not in (0.0, 1.0) or inter != 0.0) and slope != 0.0
    return {'endian': en, 'shape': shape, 'dtype': datatype, 'offset': max(vox_offset, 352), 'slope': slope, 'inter': inter,
            'scale': scale}


def read_nifti1_raw(path):
    """The payload of a NIfTI-1 file (.nii / .nii.gz, single file) as it sits on disk, untouched: dict(payload = a memoryview of the
    voxel bytes (Fortran order, shape dim[1..ndim]), shape, dtype (the NIfTI code, a key of NIFTI_DTYPES), endian ('<' or '>'),
    slope, inter, scale (whether read_nifti1 applies slope and inter)).  What ResidentVolumes uploads."""
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
        raw = f.read()
    h = _nifti1_header(raw[:348], path)
    nbytes = int(np.prod(h['shape'])) * np.dtype(NIFTI_DTYPES[h['dtype']]).itemsize
    if len(raw) < h['offset'] + nbytes:
        raise ValueError('%s: file ends before its %d voxel bytes' % (path, nbytes))
    h['payload'] = memoryview(raw)[h['offset']:h['offset'] + nbytes]
    del h['offset']
    return h


def read_nifti1(path):
    """Minimal NIfTI-1 reader (.nii / .nii.gz, single file): returns the data array in file
    order (Fortran layout -> shape dim[1..ndim]) with scl_slope/scl_inter applied.  nibabel is
    not available in the image; the reference goes through nib.load(...).dataobj."""
    h = read_nifti1_raw(path)
    a = np.frombuffer(h['payload'], dtype=np.dtype(h['endian'] + NIFTI_DTYPES[h['dtype']]))
    a = a.reshape(h['shape'], order='F')
    if h['scale']:
        a = a * h['slope'] + h['inter']
    return a


_VOLUME_CACHE = {}


def load_4d(path):
    """4-D array (X,Y,Z,T) of a subject, decoded once per process."""
    if path not in _VOLUME_CACHE:
        if path.endswith('.npy'):
            _VOLUME_CACHE[path] = np.load(path, mmap_mode='r')
        else:
            _VOLUME_CACHE[path] = read_nifti1(path)
    return _VOLUME_CACHE[path]


class FMRIDataset(Dataset):
    """CSV-indexed fMRI volumes (reference DataClass_GP.py:11-60)."""

    def __init__(self, csv_file, transform=None):
        self.df = pd.read_csv(csv_file)
        self.transform = transform
        self._subjects = self.df.subjid.unique().tolist()      # hoisted out of __getitem__ (DataClass_GP.py:31)

    def __len__(self):
        return len(self.df)

    def __getitem__(self, idx):
        row = self.df.iloc[idx]
        subj = row.iloc[1]
        vol_num = row.iloc[2]
        fmri = load_4d(row.iloc[3])
        volume = np.asarray(fmri[:, :, :, int(vol_num)])
        scld_vol = np.true_divide(volume.flatten(), GLOBAL_MAX).reshape(volume.shape)
        sample = {'subj_idx': self._subjects.index(subj), 'subj': subj, 'volume': scld_vol, 'vol_num': vol_num,
                  'task': row.iloc[4], 'trans_x': row.iloc[5], 'trans_y': row.iloc[6], 'trans_z': row.iloc[7],
                  'rot_x': row.iloc[8], 'rot_y': row.iloc[9], 'rot_z': row.iloc[10], 'sex': row.iloc[11]}
        if self.transform:
            sample = self.transform(sample)
        return sample


class ToTensor(object):
    """Sample dict -> tensors the model consumes (DataClass_GP.py:62-71)."""

    def __call__(self, sample):
        covars = np.array([sample['task'], sample['trans_x'], sample['trans_y'], sample['trans_z'], sample['rot_x'],
                           sample['rot_y'], sample['rot_z'], sample['sex']], dtype=np.float64)
        return {'covariates': torch.from_numpy(covars).float(),
                'volume': torch.from_numpy(np.ascontiguousarray(sample['volume'])).float(),
                'subjid': torch.tensor(sample['subj_idx'], dtype=torch.int64),
                'vol_num': torch.tensor(sample['vol_num'], dtype=torch.float64)}


def setup_data_loaders(batch_size=32, shuffle=(True, False, False), train_csv='', test_csv='', prefetch_device=None,
                       resident_device=None):
    """{'Shuffled_train', 'UnShuffled_train', 'test'} loaders (DataClass_GP.py:73-89).
    prefetch_device (extension): a CUDA device -> the loaders collate into pinned host memory and are wrapped in DevicePrefetcher.
    resident_device (extension): a device -> every subject file is uploaded once (ResidentVolumes) and the three loaders are
    ResidentLoaders over it: the same minibatches in the same order, assembled on the device."""
    if resident_device is not None:
        vols = ResidentVolumes([train_csv, test_csv], resident_device)
        mk = lambda view, sh: ResidentLoader(view, index_batches(len(view), batch_size, sh))
        return {'Shuffled_train': mk(vols.views[0], shuffle[0]), 'UnShuffled_train': mk(vols.views[0], shuffle[1]),
                'test': mk(vols.views[1], shuffle[2])}
    train_dataset = FMRIDataset(csv_file=train_csv, transform=ToTensor())
    test_dataset = FMRIDataset(csv_file=test_csv, transform=ToTensor())
    pin = prefetch_device is not None and torch.device(prefetch_device).type == 'cuda'
    mk = lambda ds, sh: DataLoader(ds, batch_size=batch_size, shuffle=sh, num_workers=0, pin_memory=pin)
    out = {'Shuffled_train': mk(train_dataset, shuffle[0]), 'UnShuffled_train': mk(train_dataset, shuffle[1]),
           'test': mk(test_dataset, shuffle[2])}
    return {k: DevicePrefetcher(v, prefetch_device) for k, v in out.items()} if pin else out


class DevicePrefetcher:
    """A DataLoader iterated ONE BATCH AHEAD (real-data input path): while the train step of minibatch k runs, minibatch
    k+1 is collated (into pinned host memory if the loader pins) and copied to the device on a separate HIP stream; the consumer's
    stream waits on the copy's event only when it takes the batch.  The reference copies every tensor of every minibatch with a
    blocking .to(device) inside the step loop (vae_reg_GP.py:420-423).  Yields the same sample dictionaries, tensors on the device.
    On a CPU device it is a pass-through."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)
        self.dataset = loader.dataset                           # len(loader.dataset) as the train loop uses it
        self.batch_sampler = getattr(loader, 'batch_sampler', None)
        self.collate_fn = getattr(loader, 'collate_fn', None)
        self._stream = torch.cuda.Stream(self.device) if self.device.type == 'cuda' else None

    def __len__(self):
        return len(self.loader)

    def _stage(self, sample):
        if sample is None:
            return None
        with torch.cuda.stream(self._stream):
            out = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in sample.items()}
            ev = torch.cuda.Event()
            ev.record(self._stream)
        return out, ev

    def __iter__(self):
        if self._stream is None:
            yield from self.loader
            return
        it = iter(self.loader)
        nxt = self._stage(next(it, None))
        while nxt is not None:
            cur, ev = nxt
            nxt = self._stage(next(it, None))                    # the next copy is queued before this batch is handed out
            here = torch.cuda.current_stream(self.device)
            here.wait_event(ev)
            for v in cur.values():
                if torch.is_tensor(v):
                    v.record_stream(here)                        # allocated on the copy stream, used on the consumer's
            yield cur


class DeviceResidentData:
    """A whole data set kept in HBM: volumes (N, X, Y, Z) fp32, covariates (N, C) fp32, subject ids.
    Iterating yields the same sample dictionaries as the DataLoaders above, already on the device;
    `rank`/`world` give each data-parallel rank a contiguous slice of every (global) minibatch."""

    def __init__(self, volumes, covariates, subjid, batch_size, shuffle=False, seed=0, device=None, rank=0, world=1,
                 drop_last=True):
        dev = device if device is not None else volumes.device
        self.volumes = volumes.to(dev); self.covariates = covariates.to(dev); self.subjid = subjid.to(dev)
        self.batch_size, self.shuffle, self.rank, self.world, self.drop_last = batch_size, shuffle, rank, world, drop_last
        self.gen = torch.Generator().manual_seed(seed)          # identical permutation on every rank
        assert batch_size % world == 0
        self.dataset = self                                     # len(loader.dataset) as the train loop uses it

    def __len__(self):
        return self.volumes.shape[0]

    def __iter__(self):
        N = len(self)
        order = torch.randperm(N, generator=self.gen) if self.shuffle else torch.arange(N)
        local = self.batch_size // self.world
        for s in range(0, N - (self.batch_size - 1 if self.drop_last else 0), self.batch_size):
            idx = order[s:s + self.batch_size]
            idx = idx[self.rank * local:(self.rank + 1) * local].to(self.volumes.device)
            yield {'volume': self.volumes[idx], 'covariates': self.covariates[idx], 'subjid': self.subjid[idx],
                   'vol_num': idx.double()}


# ---------------------------------------------------------------------------------------------------------------------------------
# Device-resident input path (extension): the subject files themselves live in HBM and a HIP kernel assembles every minibatch from
# an index list (include/vaegam.h: vg_volume_gather).  DeviceResidentData above needs the decoded fp32 volumes handed in; this path
# starts from the CSV of NIfTI / .npy files that the file loaders read, and yields bit for bit what they yield.

ARENA_ALIGN = 256
_NPY_DTYPES = {('u', 1): 2, ('i', 2): 4, ('i', 4): 8, ('f', 4): 16, ('f', 8): 64, ('i', 1): 256, ('u', 2): 512, ('u', 4): 768}
# one entry of the descriptor table: vg_vol_file of include/vaegam.h
VOL_FILE_DTYPE = np.dtype([('offset', '<i8'), ('sx', '<i8'), ('sy', '<i8'), ('sz', '<i8'), ('st', '<i8'), ('slope', '<f8'), ('inter', '<f8'),
                           ('dtype', '<i4'), ('swap', '<i4'), ('scale', '<i4'), ('reserved', '<i4')])


def _probe_volume_file(path):
    """What the descriptor of a 4-D subject file needs, without reading its voxels: dict(shape, dtype code, itemsize, swap,
    strides (elements), slope, inter, scale)."""
    if path.endswith('.npy'):
        a = np.load(path, mmap_mode='r')
        code = _NPY_DTYPES.get((a.dtype.kind, a.dtype.itemsize))
        if code is None:
            raise ValueError('%s: dtype %s is not one the volume gather reads (%s)' % (path, a.dtype, ', '.join(sorted(NIFTI_DTYPES.values()))))
        if a.ndim != 4:
            raise ValueError('%s: expected a 4-D array (X, Y, Z, T), got shape %s' % (path, a.shape))
        if a.flags.f_contiguous and not a.flags.c_contiguous:
            strides = tuple(int(np.prod(a.shape[:k])) for k in range(4))
        else:                                                    # C order as stored, or what the contiguous copy will be
            strides = tuple(int(np.prod(a.shape[k + 1:])) for k in range(4))
        big = a.dtype.byteorder == '>' or (a.dtype.byteorder == '=' and not np.little_endian)
        return {'shape': tuple(a.shape), 'dtype': code, 'itemsize': a.dtype.itemsize, 'swap': big and a.dtype.itemsize > 1, 'strides': strides,
                'slope': 1.0, 'inter': 0.0, 'scale': False}
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
        h = _nifti1_header(f.read(348), path)
    if len(h['shape']) != 4:
        raise ValueError('%s: expected a 4-D NIfTI (X, Y, Z, T), got shape %s' % (path, h['shape']))
    itemsize = np.dtype(NIFTI_DTYPES[h['dtype']]).itemsize
    return {'shape': h['shape'], 'dtype': h['dtype'], 'itemsize': itemsize, 'swap': h['endian'] == '>' and itemsize > 1,
            'strides': tuple(int(np.prod(h['shape'][:k])) for k in range(4)), 'slope': h['slope'], 'inter': h['inter'],
            'scale': bool(h['scale'])}


def _volume_file_bytes(path):
    """The voxel bytes of a subject file as a flat uint8 array, in the layout _probe_volume_file described."""
    if path.endswith('.npy'):
        a = np.load(path, mmap_mode='r')
        if a.flags.f_contiguous and not a.flags.c_contiguous:
            a = a.T                                              # the same bytes, seen in C order
        return np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.frombuffer(read_nifti1_raw(path)['payload'], dtype=np.uint8)


class ResidentView:
    """The rows of one CSV over a ResidentVolumes arena: which file and volume each row is, and the row's small tensors, all on the
    device.  It stands in for the data set of a loader (`len()`, `.df`)."""

    def __init__(self, volumes, csv_file, df, row_file, row_vol):
        dev = volumes.device
        self.volumes, self.csv_file, self.df = volumes, csv_file, df
        self.row_file = torch.from_numpy(row_file.astype(np.int32)).to(dev)
        self.row_vol = torch.from_numpy(row_vol.astype(np.int32)).to(dev)
        self.covariates = torch.from_numpy(df.iloc[:, 4:12].to_numpy(dtype=np.float64)).float().to(dev)      # = ToTensor
        self.subjid = torch.from_numpy(pd.factorize(df.iloc[:, 1])[0].astype(np.int64)).to(dev)              # first-appearance order of THIS csv
        self.vol_num = torch.from_numpy(df.iloc[:, 2].to_numpy(dtype=np.float64)).to(dev)

    def __len__(self):
        return len(self.df)

    def batch(self, idx):
        """The sample dictionary of rows `idx` (int64 tensor on the device, already validated)."""
        from . import ops
        v = self.volumes
        x = ops.volume_gather(v.arena, v.files, self.row_file, self.row_vol, idx, v.shape, v.dtype, GLOBAL_MAX)
        return {'covariates': self.covariates.index_select(0, idx), 'volume': x, 'subjid': self.subjid.index_select(0, idx),
                'vol_num': self.vol_num.index_select(0, idx)}


class ResidentVolumes:
    """Every distinct subject file named by `csv_files` (column 3, nii_path), decoded never and uploaded once: the raw payloads sit
    in one byte arena on `device`, each starting on a 256-byte boundary, next to a table that says how to read them (dtype, byte
    order, element strides, scl_slope / scl_inter).  `.views[i]` is the ResidentView of csv_files[i]; a file named by several CSVs
    is held once.  .npy files keep their own layout when C- or F-contiguous.  Raises ValueError naming the file for a dtype the
    gather does not read, a file that is not 4-D, a spatial shape that differs between files or a volume number outside its file,
    and -- before anything is allocated -- when the arena would exceed `max_bytes` (default: half of the free device memory)."""

    def __init__(self, csv_files, device, max_bytes=None):
        from . import _lib
        self.device = torch.device(device)
        if self.device.type != 'cuda' and not _lib.get_lib().host_pointers_ok:
            raise RuntimeError('ResidentVolumes needs a GPU device: the HIP kernels need device pointers (no CPU path)')
        frames = [pd.read_csv(c) for c in csv_files]
        paths = list(dict.fromkeys(p for df in frames for p in df.iloc[:, 3].tolist()))
        self.paths = paths
        info, offsets, total = [], [], 0
        for p in paths:
            m = _probe_volume_file(p)
            if info and m['shape'][:3] != info[0]['shape'][:3]:
                raise ValueError('%s: spatial shape %s differs from %s of %s' % (p, m['shape'][:3], info[0]['shape'][:3], paths[0]))
            info.append(m)
            offsets.append(total)
            total += -(-int(np.prod(m['shape'])) * m['itemsize'] // ARENA_ALIGN) * ARENA_ALIGN
        if max_bytes is None and self.device.type == 'cuda':
            max_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        if max_bytes is not None and total > max_bytes:
            raise ValueError('the %d subject files need %d bytes of device memory, more than the %d allowed (max_bytes); '
                             'use the file loaders for this data set' % (len(paths), total, max_bytes))
        self.shape = tuple(info[0]['shape'][:3]) if info else (0, 0, 0)
        self.nbytes = total
        codes = {m['dtype'] for m in info}
        self.dtype = codes.pop() if len(codes) == 1 else 0       # one code for the whole table, or 0: read each descriptor's
        table = np.zeros(len(paths), dtype=VOL_FILE_DTYPE)
        self.arena = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        for k, (p, m) in enumerate(zip(paths, info)):
            raw = _volume_file_bytes(p)
            assert raw.size == int(np.prod(m['shape'])) * m['itemsize'], p
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', UserWarning)     # read-only buffer: it is only copied from
                self.arena[offsets[k]:offsets[k] + raw.size].copy_(torch.from_numpy(raw))
            table[k] = (offsets[k],) + m['strides'] + (m['slope'], m['inter'], m['dtype'], int(m['swap']), int(m['scale']), 0)
        self.files = torch.from_numpy(table.view(np.uint8).reshape(len(paths), -1)).to(self.device)
        index = {p: k for k, p in enumerate(paths)}
        self.views = []
        for c, df in zip(csv_files, frames):
            row_file = df.iloc[:, 3].map(index).to_numpy(dtype=np.int64)
            row_vol = df.iloc[:, 2].to_numpy(dtype=np.int64)
            n_t = np.array([m['shape'][3] for m in info], dtype=np.int64)[row_file] if len(df) else row_vol
            bad = np.nonzero((row_vol < 0) | (row_vol >= n_t))[0]
            if bad.size:
                r = int(bad[0])
                raise ValueError('%s row %d: volume %d is outside %s (%d volumes)' % (c, r, row_vol[r], paths[row_file[r]], n_t[r]))
            self.views.append(ResidentView(self, c, df, row_file, row_vol))


class _RowIndices(Dataset):
    """The row numbers 0..n-1 as a data set: a DataLoader over it draws its seeds and shuffles exactly as one over FMRIDataset."""

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


def index_batches(n, batch_size, shuffle):
    """The minibatches of a DataLoader(dataset of n rows, batch_size, shuffle) as int64 index tensors: the same order under the same
    torch.manual_seed, epoch after epoch, and the same draws from the CPU generator."""
    return DataLoader(_RowIndices(n), batch_size=batch_size, shuffle=shuffle, num_workers=0,
                      collate_fn=lambda rows: torch.tensor(rows, dtype=torch.int64))


class ResidentLoader:
    """Minibatches of a ResidentView: iterates `batch_sampler` (anything that yields the row numbers of one minibatch at a time as a
    list or an int64 tensor: index_batches, dp.ShardedBatchSampler), copies the B indices to the device -- the only host work per
    batch -- and yields the sample dictionary of the file loaders ('covariates', 'volume', 'subjid', 'vol_num'; same dtypes and
    shapes) with every tensor on the device."""

    def __init__(self, view, batch_sampler):
        self.view, self.batch_sampler = view, batch_sampler
        self.dataset = view                                      # len(loader.dataset) and .df as the train loop uses them

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        n, dev = len(self.view), self.view.volumes.device
        for rows in self.batch_sampler:
            idx = torch.as_tensor(rows, dtype=torch.int64)
            if idx.ndim != 1 or idx.numel() == 0:
                raise ValueError('ResidentLoader: a minibatch is a non-empty list of row numbers, got shape %s' % (tuple(idx.shape),))
            if int(idx.min()) < 0 or int(idx.max()) >= n:
                raise IndexError('ResidentLoader: row numbers %d..%d are outside the %d rows of %s'
                                 % (int(idx.min()), int(idx.max()), n, self.view.csv_file))
            yield self.view.batch(idx.to(dev, non_blocking=True))
