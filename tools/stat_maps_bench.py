"""What the voxel-wise statistics cost (MI355X): BASELINE configs[2] (41x49x35, batch 64, 8 covariates) on a synthetic data
set of 4 subjects x 98 volumes taken in order, batch by batch, as the unshuffled loader hands them over (6 batches of 64 volumes that
hold one or two subjects each, and a last one of 8).

Every batch goes through forward_core once; its logits, gains, data and subject ids stay on the device, and three things are timed
over them by device events, the codes alternated in --rounds rounds of one process after a warm-up, medians over the rounds:

  kernel      vg_gam_stats_accumulate alone (ops.gam_stats_accumulate on prepared int32 ids), with the bytes it moves -- (C+2) B V_n
              floats read, counting the logits of native voxels only, plus 3C+8 doubles read and written per voxel of every subject
              present in the batch -- and their share of the measured HBM rate (6.29 TB/s, MI355X_MICROARCH.md);
  new         the accumulate step of VAE.map_statistics (VAE._accumulate_statistics: the counts, the id cast, the kernel), 3C+8 sums;
  parent      the accumulate step VAE.reconstruct(write_volumes=False) does after forward_core: ops.gam_maps ([C+2, B, V] fp32) and
              its C+2 fp64 index_add_ passes plus the counts, C+2 sums -- code this tool restates from reconstruct, which is unchanged.

Times are per batch (a window runs all 7 batches).  Gate: new <= parent.  One JSON object per line; the last one carries the gate."""
import argparse
import json
import os
import statistics
import sys

HBM_MEASURED = 6.29e12          # bytes/s, float4 copy (MI355X_MICROARCH.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[41, 49, 35])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--covariates', type=int, default=8)
    ap.add_argument('--subjects', type=int, default=4)
    ap.add_argument('--volumes', type=int, default=98, help='volumes per subject')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--passes', type=int, default=100, help='passes over all batches per timed window')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))

    import numpy as np
    import torch
    import vae_gam_amd  # noqa: F401
    from vae_gam_amd import _lib, ops, synthetic
    from vae_gam_amd.vae_reg_GP import VAE
    assert torch.cuda.is_available(), 'needs an MI355X'
    lib = _lib.get_lib()
    shape = tuple(a.shape)
    B, C, S, T = a.batch, a.covariates, a.subjects, a.volumes
    V = int(np.prod(shape))
    K = ops.gam_stats_slots(C)
    dev = 'cuda'
    ds = synthetic.make_dataset(num_subjects=S, vols_per_subject=T, num_covariates=C, img_shape=shape, seed=0)
    torch.manual_seed(1)
    m = VAE(num_covariates=C, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name=dev, img_shape=shape)
    N = S * T
    batches = []
    with torch.no_grad():
        for lo in range(0, N, B):
            x = torch.from_numpy(ds['volumes'][lo:lo + B]).to(dev)
            cov = torch.from_numpy(ds['covariates'][lo:lo + B]).float().to(dev)
            ids = torch.from_numpy(np.asarray(ds['subjid'][lo:lo + B]).astype(np.int64)).to(dev)
            out = m.forward_core(cov, x, want_maps=False)
            batches.append(dict(x=x, ids=ids, subj=ids.to(torch.int32), xf=x.float().reshape(x.shape[0], V),
                                out={'logits': out['logits'].detach(), 'task_var': out['task_var'].detach()}))
    torch.cuda.synchronize()
    nb = len(batches)
    emb = (m.img_shape, m.grid_shape) if (m._embedded or m.mask is not None) else (None, None)
    keys = ['base'] + [c.img_key for c in m.schema] + ['full_rec']
    acc = torch.zeros(S, K, V, device=dev, dtype=torch.float64)
    counts = torch.zeros(S, device=dev, dtype=torch.float64)
    sums = {k: torch.zeros(S, V, device=dev, dtype=torch.float64) for k in keys}
    pcounts = torch.zeros(S, device=dev, dtype=torch.float64)
    eps, glm = m.epsilon.detach().view(-1), m._glm()

    def kernel():
        for b in batches:
            ops.gam_stats_accumulate(b['out']['logits'], b['out']['task_var'], b['xf'], b['subj'], acc, *emb, mask=m.mask)

    def new():
        for b in batches:
            m._accumulate_statistics(b['out'], b['x'], b['ids'], acc, counts)

    def parent():                                        # VAE.reconstruct's accumulate step, restated
        for b in batches:
            maps = ops.gam_maps(b['out']['logits'], b['out']['task_var'], b['xf'], eps, glm, *emb, mask=m.mask)
            idl = b['ids'].long()
            pcounts.index_add_(0, idl, torch.ones_like(idl, dtype=torch.float64))
            for j, k in enumerate(keys):
                sums[k].index_add_(0, idl, maps[j].double())

    codes = {'kernel': kernel, 'new': new, 'parent': parent}

    def timed_us(fn):
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.passes):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / (a.passes * nb)

    with torch.no_grad():
        for fn in codes.values():                        # warm-up: code objects, the allocator's blocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the two paths agree on what they both compute (on the same logits): the first-moment sums after the same number of passes
        acc.zero_(); counts.zero_(); pcounts.zero_()
        for s_ in sums.values():
            s_.zero_()
        new(); parent()
        torch.cuda.synchronize()
        worst = max(float((acc[:, j] - sums[k]).abs().max() / sums[k].abs().max().clamp_min(1e-30)) for j, k in enumerate(keys))
        assert torch.equal(counts, pcounts) and worst < 1e-6, worst         # (|difference| over the map's largest sum)
        res = {k: [] for k in codes}
        for _ in range(a.rounds):
            for name, fn in codes.items():
                res[name].append(timed_us(fn))
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in res.items()}
    present = [len(set(np.asarray(ds['subjid'][lo:lo + B]).tolist())) for lo in range(0, N, B)]
    nbytes = [(C + 2) * int(b['x'].shape[0]) * V * 4 + p * K * V * 8 * 2 for b, p in zip(batches, present)]
    common = {'shape': shape, 'grid': tuple(m.grid_shape), 'batch': B, 'covariates': C, 'subjects': S, 'volumes_per_subject': T,
              'batches': nb, 'rounds': a.rounds, 'passes': a.passes, 'library': lib.path}
    mean_bytes = sum(nbytes) / nb
    print(json.dumps(dict(common, bench='kernel', us_per_batch=round(med['kernel'], 2), spread=round(spread['kernel'], 4),
                          bytes_per_batch=int(mean_bytes), subjects_present=present, TB_per_s=round(mean_bytes / med['kernel'] / 1e6, 3),
                          share_of_measured_hbm=round(mean_bytes / (med['kernel'] * 1e-6) / HBM_MEASURED, 4))), flush=True)
    print(json.dumps(dict(common, bench='accumulate_step', us_per_batch={k: round(med[k], 2) for k in ('new', 'parent')},
                          spread={k: round(spread[k], 4) for k in ('new', 'parent')}, sums={'new': K, 'parent': C + 2},
                          first_moment_rel_diff=worst,
                          new_over_parent=round(med['new'] / med['parent'], 4), gate='new <= parent',
                          gate_met=bool(med['new'] <= med['parent']),
                          rounds_us={k: [round(t, 2) for t in v] for k, v in res.items()})), flush=True)


if __name__ == '__main__':
    main()
