"""The input path next to the train step (GPU): how fast the file loaders and the device-resident loaders hand out minibatches, what
the volume gather costs per batch against the replayed step, and what that does to a whole train_epoch.

Data set: 4 subjects x 98 volumes at 41x49x35 (synthetic.make_dataset), written once as float32 .nii and once as int16 .nii.gz with a
slope; batch 64, 8 covariates.  Every figure is taken after a warm-up pass over the same shapes and behind a device synchronise.

  python tools/input_path_bench.py                      one JSON object on stdout
  python tools/input_path_bench.py --trace-epochs 2     a few resident + graph epochs only (run under rocprofv3 --kernel-trace --stats)

Per file kind:
  file_loader_vps        (a) volumes/s of a bare epoch through the prefetching file loaders (no model)
  resident_loader_vps    (b) the same through the resident loaders
  gather_us              (c) device-event time of one vg_volume_gather of 64 volumes
  step_ms                (d) the replayed (hipGraph) train step on that batch;  gather_over_step = (c) / (d)
  epoch_vps              (e) train_epoch volumes/s: file loaders (eager), resident (eager), resident + graph, and the same steps fed from
                         DeviceResidentData + graph (decoded fp32 volumes already in HBM: the rate bench.py's workload runs at)
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subjects', type=int, default=4)
    ap.add_argument('--vols', type=int, default=98)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--epochs', type=int, default=8, help='epochs per timed window')
    ap.add_argument('--rounds', type=int, default=3, help='timed windows per figure (the median is reported)')
    ap.add_argument('--trace-epochs', type=int, default=0, help='run this many resident + graph epochs on the int16 files and exit')
    a = ap.parse_args()

    import numpy as np
    import pandas as pd
    import torch
    import vae_gam_amd  # noqa: F401
    from vae_gam_amd import DataClass_GP as D
    from vae_gam_amd import _lib, nifti, ops, synthetic
    from vae_gam_amd.vae_reg_GP import VAE
    assert torch.cuda.is_available(), 'needs an MI355X'
    _lib.get_lib()
    B, S, T = a.batch, a.subjects, a.vols
    N = S * T
    ds = synthetic.make_dataset(num_subjects=S, vols_per_subject=T, num_covariates=8, seed=0)
    tmp = tempfile.mkdtemp(prefix='input_path_bench_')
    csv_npy, _ = synthetic.write_csvs(ds, tmp)
    df = pd.read_csv(csv_npy, index_col=0)
    slope = 0.125                                                        # 3284.5 / 0.125 < 2^15
    csvs = {}
    for kind in ('f32_nii', 'i16_nii_gz'):
        paths = []
        for s in range(S):
            vol = np.moveaxis(ds['volumes'][s * T:(s + 1) * T], 0, -1) * 3284.5
            if kind == 'f32_nii':
                p = os.path.join(tmp, 'subj%02d.nii' % s)
                nifti.write_nifti1(p, vol)
            else:
                p = os.path.join(tmp, 'subj%02d_i16.nii.gz' % s)
                ref = os.path.join(tmp, 'subj%02d.nii' % s)
                h = bytearray(nifti.read_header(ref)[0])
                struct.pack_into('<2h', h, 70, 4, 16)                    # datatype int16, bitpix
                struct.pack_into('<2f', h, 112, slope, 0.0)
                with gzip.open(p, 'wb', compresslevel=1) as f:
                    f.write(bytes(h) + b'\x00' * 4 + np.rint(vol / slope).astype('<i2').tobytes(order='F'))
            paths += [p] * T
        d2 = df.copy(); d2['nii_path'] = paths
        csvs[kind] = os.path.join(tmp, kind + '.csv')
        d2.to_csv(csvs[kind])

    def sync():
        torch.cuda.synchronize()

    def window(fn, count):
        """median over --rounds of `count` / (seconds of one fn() that ends synchronised)"""
        out = []
        for _ in range(a.rounds):
            sync(); t0 = time.perf_counter(); fn(); sync()
            out.append(count / (time.perf_counter() - t0))
        return statistics.median(out)

    def bare_epochs(loader):
        def run():
            for _ in range(a.epochs):
                for smp in loader:
                    pass
        return run

    torch.manual_seed(1)
    model = VAE(num_covariates=8, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda', save_dir=tmp)

    def train_epochs(loader):
        def run():
            for _ in range(a.epochs):
                model.train_epoch(loader)
        return run

    def epoch_rate(loader, graph):
        model.use_hip_graph = graph
        model.train_epoch(loader)                                        # warm-up: every batch shape, graph capture
        if graph:
            assert model._graphs and all(g is not False for g in model._graphs.values()), 'capture fell back to eager'
        return window(train_epochs(loader), a.epochs * len(loader.dataset))

    devnull = open(os.devnull, 'w')
    stdout, sys.stdout = sys.stdout, devnull                             # train_epoch prints a line per epoch
    try:
        if a.trace_epochs:
            res = D.setup_data_loaders(batch_size=B, train_csv=csvs['i16_nii_gz'], test_csv=csvs['i16_nii_gz'], resident_device='cuda')
            model.use_hip_graph = True
            for _ in range(a.trace_epochs + 1):
                model.train_epoch(res['Shuffled_train'])
            sync()
            out = {'traced': 'resident + graph', 'epochs': a.trace_epochs + 1, 'steps_per_epoch': len(res['Shuffled_train'])}
        else:
            drd = D.DeviceResidentData(torch.from_numpy(ds['volumes']), torch.from_numpy(ds['covariates']), torch.from_numpy(ds['subjid']),
                                       batch_size=B, shuffle=True, seed=0, device='cuda', drop_last=False)
            out = {'config': {'subjects': S, 'vols_per_subject': T, 'volume': [41, 49, 35], 'batch': B, 'covariates': 8,
                              'epochs_per_window': a.epochs, 'rounds': a.rounds, 'steps_per_epoch': -(-N // B)},
                   'host_cpus': os.cpu_count(), 'device': torch.cuda.get_device_name(0), 'kinds': {}}
            for kind, csv in csvs.items():
                D._VOLUME_CACHE.clear()
                files = D.setup_data_loaders(batch_size=B, train_csv=csv, test_csv=csv, prefetch_device='cuda')
                res = D.setup_data_loaders(batch_size=B, train_csv=csv, test_csv=csv, resident_device='cuda')
                r = {}
                bare_epochs(files['Shuffled_train'])(); bare_epochs(res['Shuffled_train'])()          # warm-up (decodes the files once)
                r['file_loader_vps'] = window(bare_epochs(files['Shuffled_train']), a.epochs * N)
                r['resident_loader_vps'] = window(bare_epochs(res['Shuffled_train']), a.epochs * N)
                view = res['Shuffled_train'].view
                v = view.volumes
                idx = torch.randperm(N)[:B].cuda()
                x = torch.empty((B,) + v.shape, device='cuda')
                reps = 200
                for _ in range(20):
                    ops.volume_gather(v.arena, v.files, view.row_file, view.row_vol, idx, v.shape, v.dtype, D.GLOBAL_MAX, out=x)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                sync(); e0.record()
                for _ in range(reps):
                    ops.volume_gather(v.arena, v.files, view.row_file, view.row_vol, idx, v.shape, v.dtype, D.GLOBAL_MAX, out=x)
                e1.record(); sync()
                r['gather_us'] = 1e3 * e0.elapsed_time(e1) / reps
                r['gather_bytes'] = B * int(np.prod(v.shape)) * ({'f32_nii': 4, 'i16_nii_gz': 2}[kind] + 4)      # read + written
                smp = view.batch(idx)
                model.use_hip_graph = True
                for _ in range(5):
                    model.train_step(smp['subjid'], smp['covariates'], smp['volume'])
                assert model._graphs.get(tuple(smp['volume'].shape)), 'capture fell back to eager'
                steps = 50
                e0.record()
                for _ in range(steps):
                    model.train_step(smp['subjid'], smp['covariates'], smp['volume'])
                e1.record(); sync()
                r['step_ms'] = e0.elapsed_time(e1) / steps
                r['gather_over_step'] = r['gather_us'] / (1e3 * r['step_ms'])
                ep = {}
                ep['file_loaders_eager'] = epoch_rate(files['Shuffled_train'], False)
                ep['resident_eager'] = epoch_rate(res['Shuffled_train'], False)
                ep['resident_graph'] = epoch_rate(res['Shuffled_train'], True)
                ep['device_resident_data_graph'] = epoch_rate(drd, True)
                r['epoch_vps'] = ep
                r['resident_graph_over_file_loaders'] = ep['resident_graph'] / ep['file_loaders_eager']
                r['resident_graph_over_device_resident_data'] = ep['resident_graph'] / ep['device_resident_data_graph']
                out['kinds'][kind] = r
    finally:
        sys.stdout = stdout
        devnull.close()
        shutil.rmtree(tmp, ignore_errors=True)

    def rnd(o):
        if isinstance(o, dict):
            return {k: rnd(v) for k, v in o.items()}
        return round(o, 4) if isinstance(o, float) else o
    print(json.dumps(rnd(out)), flush=True)


if __name__ == '__main__':
    main()
