"""What embedding a volume grid costs (MI355X): nat 53x63x52 in the network grid 54x66x54, batch 64, 8 covariates.

  (a) the embedded GAM/ELBO forward and backward (vg_gam_elbo_fwd_embed / _bwd_embed) against the plain pair at V = 54*66*54:
      device events around --launches back-to-back calls, the two codes alternated in --rounds rounds of one process.  Gate: the
      embedded call may take 10 % longer than the plain one (index arithmetic plus spread); where the plain call's own spread over
      the rounds exceeds 5 %, twice that spread.  Exit status 1 if the gate fails.
  (b) the embed copy (vg_embed_volumes): time and bytes/s (B*(V_N+V_G)*4 bytes) against the HBM peak.
  (c) the captured train step of the embedded model against the step of the model built on the grid itself, alternated, device
      events around --steps replays; recorded, no gate.  --no-step leaves it out.

One JSON object per line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--native', type=int, nargs=3, default=[53, 63, 52])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--covariates', type=int, default=8)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()

    import numpy as np
    import torch
    import vae_gam_amd  # noqa: F401
    from vae_gam_amd import _lib, ops, schema, synthetic
    from vae_gam_amd.vae_reg_GP import VAE
    assert torch.cuda.is_available(), 'needs an MI355X'
    lib = _lib.get_lib()
    nat = tuple(a.native); grid = schema.grid_for(nat)
    B, C = a.batch, a.covariates
    Vn, Vg = int(np.prod(nat)), int(np.prod(grid))
    dev = 'cuda'
    p = ops._p
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(C + 1, B, Vg, device=dev, generator=g)
    gain = torch.randn(C, B, device=dev, generator=g)
    g_slp = torch.randn(B, device=dev, generator=g); g_dist = torch.randn(C, B, device=dev, generator=g)
    d_logits = torch.empty_like(logits); d_gain = torch.empty_like(gain); tot = torch.zeros(1, device=dev)
    ws = torch.empty(lib.size('vg_gam_ws_bytes', C, B, Vg) // 4 + 1, dtype=torch.float32, device=dev)
    slp = torch.empty(B, device=dev); dist = torch.empty(C, B, device=dev)
    data = {}
    for name, V in (('plain', Vg), ('embed', Vn)):
        data[name] = dict(x=torch.rand(B, V, device=dev, generator=g), glm=torch.rand(C, V, device=dev, generator=g),
                          eps=(-np.log(10) + 0.3 * torch.randn(V, device=dev, generator=g, dtype=torch.float64)),
                          d_eps=torch.empty(V, device=dev, dtype=torch.float64))
    n3, g3 = ops._i3(nat), ops._i3(grid)

    def fwd(name):
        d = data[name]
        if name == 'plain':
            ops._call(logits, 'vg_gam_elbo_fwd', p(logits), p(gain), p(d['x']), p(d['eps']), p(d['glm']), C, B, Vg, p(ws), p(slp), p(dist), None)
        else:
            ops._call(logits, 'vg_gam_elbo_fwd_embed', p(logits), p(gain), p(d['x']), p(d['eps']), p(d['glm']), C, B, n3, g3, p(ws), p(slp), p(dist), None)

    def bwd(name):
        d = data[name]
        if name == 'plain':
            ops._call(logits, 'vg_gam_elbo_bwd', p(logits), p(gain), p(d['x']), p(d['eps']), p(d['glm']), p(dist), p(g_slp), p(g_dist), C, B, Vg,
                      p(ws), p(d_logits), p(d_gain), p(d['d_eps']), p(tot), 0)
        else:
            ops._call(logits, 'vg_gam_elbo_bwd_embed', p(logits), p(gain), p(d['x']), p(d['eps']), p(d['glm']), p(dist), p(g_slp), p(g_dist), C, B,
                      n3, g3, p(ws), p(d_logits), p(d_gain), p(d['d_eps']), p(tot), 0)

    def timed_us(fn, n):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n

    def alternate(fns):
        """{name: [us per call, one entry per round]}; every code warmed up first"""
        for fn in fns.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        out = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                out[k].append(timed_us(fn, a.launches))
        return out

    failed = False
    for what, call in (('gam_fwd', fwd), ('gam_bwd', bwd)):
        fwd('plain')                                            # dist of the matching forward is what the backward reads
        r = alternate({'plain': lambda: call('plain'), 'embed': lambda: call('embed')})
        med = {k: statistics.median(v) for k, v in r.items()}
        spread = (max(r['plain']) - min(r['plain'])) / med['plain']
        allow = 0.10 if spread <= 0.05 else 2 * spread
        ratio = med['embed'] / med['plain']
        ok = ratio <= 1 + allow
        failed |= not ok
        print(json.dumps({'bench': what, 'native': nat, 'grid': grid, 'batch': B, 'covariates': C, 'launches': a.launches, 'rounds': a.rounds,
                          'plain_us': round(med['plain'], 2), 'embed_us': round(med['embed'], 2), 'embed_over_plain': round(ratio, 4),
                          'plain_spread': round(spread, 4), 'embed_spread': round((max(r['embed']) - min(r['embed'])) / med['embed'], 4),
                          'allowed': round(1 + allow, 4), 'pass': ok}), flush=True)

    xs = data['embed']['x']
    out = torch.empty(B, Vg, device=dev)
    r = alternate({'embed_copy': lambda: ops._call(xs, 'vg_embed_volumes', p(xs), n3, g3, B, p(out))})['embed_copy']
    us = statistics.median(r)
    nbytes = B * (Vn + Vg) * 4
    print(json.dumps({'bench': 'embed_copy', 'native': nat, 'grid': grid, 'batch': B, 'us': round(us, 2), 'spread': round((max(r) - min(r)) / us, 4),
                      'bytes': nbytes, 'GBps': round(nbytes / us / 1e3, 1), 'frac_of_hbm_peak': round(nbytes / us / 1e3 / HBM_PEAK_GBS, 4)}), flush=True)
    del logits, d_logits, ws, data, out
    torch.cuda.empty_cache()

    if not a.no_step:
        models = {}
        for name, shape in (('embedded', nat), ('grid', grid)):
            ds = synthetic.make_dataset(num_subjects=1, vols_per_subject=B, num_covariates=C, img_shape=shape, seed=0)
            torch.manual_seed(1)
            m = VAE(num_covariates=C, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda', img_shape=shape)
            m.use_hip_graph = True
            models[name] = (m, torch.zeros(B, dtype=torch.int64, device=dev), torch.from_numpy(ds['covariates']).to(dev),
                            torch.from_numpy(ds['volumes']).to(dev))
        torch.manual_seed(1234)

        def steps(name, n):
            m, ids, cov, x = models[name]
            for _ in range(n):
                m.train_step(ids, cov, x)

        for name in models:
            steps(name, 3)
            m = models[name][0]
            assert m._graphs and all(v is not False for v in m._graphs.values()), 'capture fell back to eager'
        res = {k: [] for k in models}
        for _ in range(a.rounds):
            for name in models:
                torch.cuda.synchronize()
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                steps(name, a.steps)
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) / a.steps)
        med = {k: statistics.median(v) for k, v in res.items()}
        print(json.dumps({'bench': 'captured_step', 'native': nat, 'grid': grid, 'batch': B, 'covariates': C, 'steps': a.steps, 'rounds': a.rounds,
                          'embedded_ms': round(med['embedded'], 4), 'grid_ms': round(med['grid'], 4),
                          'difference_ms': round(med['embedded'] - med['grid'], 4),
                          'embedded_spread': round((max(res['embedded']) - min(res['embedded'])) / med['embedded'], 4),
                          'grid_spread': round((max(res['grid']) - min(res['grid'])) / med['grid'], 4)}), flush=True)
    sys.exit(1 if failed else 0)


if __name__ == '__main__':
    main()
