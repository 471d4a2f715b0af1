"""Per-phase timing of the latent projection (VAE.project_latent) on the MI355X.

    python tools/latent_projection_bench.py [--sizes 5000,50000] [--dim 32] [--encode-vols 512]

Seeded synthetic latent means (10 Gaussian blobs) at each N; after one warm-up run of every phase, each phase is timed with device
events on the current stream: kNN, fuzzy set (rho / sigma / memberships and the symmetric union), graph assembly (pruning, CSR),
layout (all epochs).  The spectral initialisation runs on the host (scipy) and is timed with the host clock after a device
synchronise.  The encode pass (VAE.encode over --encode-vols volumes of the 41x49x35 geometry, batches of 32) is timed once.
Prints one JSON line per size.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vae_gam_amd  # noqa: E402,F401
from vae_gam_amd import latent_projection as LP  # noqa: E402


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def encode_ms(n_vols, batch=32):
    from vae_gam_amd.vae_reg_GP import VAE
    from vae_gam_amd import synthetic
    ds = synthetic.make_dataset(num_subjects=1, vols_per_subject=batch, num_covariates=8, seed=0)
    torch.manual_seed(1)
    m = VAE(num_covariates=8, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda')
    x = torch.as_tensor(ds['volumes'][:batch]).float().cuda()
    with torch.no_grad():
        m.encode(x)
        torch.cuda.synchronize()
        _, ms = timed(lambda: [m.encode(x) for _ in range(max(1, n_vols // batch))])
    return ms


def run(N, D, seed=0):
    rng = np.random.default_rng(seed)
    centers = rng.normal(scale=10.0, size=(10, D))
    x = torch.from_numpy((centers[np.arange(N) % 10] + rng.normal(size=(N, D))).astype(np.float32)).cuda()
    k = min(20, N)
    n_epochs = LP.default_n_epochs(N)
    a, b = LP.find_ab_params(1.0, 0.1)
    res = {'N': N, 'D': D, 'k': k, 'n_epochs': n_epochs}
    for rep in range(2):                                        # rep 0 warms every kernel and allocation up
        (idx, dist), t_knn = timed(lambda: LP.knn(x, k))
        coo, t_fz = timed(lambda: LP.fuzzy_simplicial_set(idx, dist))
        (rows, cols, vals, rowptr, col, eps), t_g = timed(lambda: (lambda r, c, v: (r, c, v) + LP.to_csr(r, c, v, N))(
            *LP.prune_graph(*coo, n_epochs)))
        t0 = time.perf_counter()
        Y, how = LP.spectral_init(rows, cols, vals, N, 42)
        t_init = (time.perf_counter() - t0) * 1e3
        y0 = torch.from_numpy(LP.normalise_layout(Y)).cuda()
        torch.cuda.synchronize()
        _, t_lay = timed(lambda: LP.layout(y0, rowptr, col, eps, n_epochs, a, b, 5, 42))
    res.update({'edges': int(col.numel()), 'init': how, 'knn_ms': round(t_knn, 3), 'fuzzy_ms': round(t_fz, 3),
                'graph_ms': round(t_g, 3), 'spectral_init_host_ms': round(t_init, 1), 'layout_ms': round(t_lay, 3),
                'layout_us_per_epoch': round(1e3 * t_lay / n_epochs, 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='5000,50000')
    ap.add_argument('--dim', type=int, default=32)
    ap.add_argument('--encode-vols', type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'latent_projection_bench needs a GPU'
    if args.encode_vols > 0:
        ms = encode_ms(args.encode_vols)
        print(json.dumps({'phase': 'encode', 'volumes': args.encode_vols, 'ms': round(ms, 3)}), flush=True)
    for N in [int(s) for s in args.sizes.split(',')]:
        print(json.dumps(run(N, args.dim)), flush=True)


if __name__ == '__main__':
    main()
