"""What the brain mask costs (MI355X): BASELINE configs[2] (41x49x35, batch 64, 8 covariates) with no mask, with an all-ones
mask and with an ellipsoidal mask of about one third of the box.

  (a) the GAM/ELBO forward and backward launches: the plain pair (vg_gam_elbo_fwd / _bwd) against the masked pair
      (vg_gam_elbo_fwd_masked / _bwd_masked) under the two masks; device events around --launches back-to-back calls, the three codes
      alternated in --rounds rounds of one process.
  (b) the captured train step of the three models, alternated, device events around --steps replays per round.

Recorded, no gate: medians over the rounds and each code's spread (max - min over the median).

--mask-free-only times the mask-free step alone and uses nothing this tool's own checkout added; with --root DIR the package is
imported from another checkout (one that predates the mask, say), so that the mask-free step of two commits can be compared in runs
alternated on one machine.

One JSON object per line."""
import argparse
import json
import os
import statistics
import sys


def ellipsoid(shape, fraction):
    """uint8 mask: the centred ellipsoid with the box's aspect ratios that holds about `fraction` of the box's voxels"""
    import numpy as np
    scale = (fraction / (np.pi / 6)) ** (1.0 / 3.0)              # the inscribed ellipsoid holds pi/6 of the box
    ax = [(np.arange(n) - (n - 1) / 2.0) / (scale * n / 2.0) for n in shape]
    r2 = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2
    return (r2 <= 1.0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[41, 49, 35])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--covariates', type=int, default=8)
    ap.add_argument('--fraction', type=float, default=1.0 / 3.0, help='share of the box inside the ellipsoidal mask')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--mask-free-only', action='store_true', help='the captured mask-free step alone')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='checkout to import vae_gam_amd from (default: this one)')
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
    B, C = a.batch, a.covariates
    V = int(np.prod(shape))
    dev = 'cuda'
    masks = {'none': None}
    if not a.mask_free_only:
        masks['ones'] = np.ones(shape, dtype=np.uint8)
        masks['ellipsoid'] = ellipsoid(shape, a.fraction)
    common = {'shape': shape, 'batch': B, 'covariates': C, 'rounds': a.rounds, 'library': lib.path,
              'mask_voxels': {k: (V if m is None else int(m.sum())) for k, m in masks.items()}, 'box_voxels': V}

    def summary(res):
        med = {k: statistics.median(v) for k, v in res.items()}
        return med, {k: (max(v) - min(v)) / med[k] for k, v in res.items()}

    if not a.mask_free_only:
        p = ops._p
        g = torch.Generator(device=dev).manual_seed(0)
        logits = torch.randn(C + 1, B, V, device=dev, generator=g)
        gain = torch.randn(C, B, device=dev, generator=g)
        g_slp = torch.randn(B, device=dev, generator=g); g_dist = torch.randn(C, B, device=dev, generator=g)
        x = torch.rand(B, V, device=dev, generator=g); glm = torch.rand(C, V, device=dev, generator=g)
        eps = -np.log(10) + 0.3 * torch.randn(V, device=dev, generator=g, dtype=torch.float64)
        d_logits = torch.empty_like(logits); d_gain = torch.empty_like(gain); d_eps = torch.empty_like(eps); tot = torch.zeros(1, device=dev)
        ws = torch.empty(lib.size('vg_gam_ws_bytes', C, B, V) // 4 + 1, dtype=torch.float32, device=dev)
        slp = torch.empty(B, device=dev); dist = torch.empty(C, B, device=dev)
        dmask = {k: None if m is None else torch.from_numpy(m).to(dev).reshape(-1) for k, m in masks.items()}
        s3 = ops._i3(shape)

        def fwd(name):
            if dmask[name] is None:
                ops._call(logits, 'vg_gam_elbo_fwd', p(logits), p(gain), p(x), p(eps), p(glm), C, B, V, p(ws), p(slp), p(dist), None)
            else:
                ops._call(logits, 'vg_gam_elbo_fwd_masked', p(logits), p(gain), p(x), p(eps), p(glm), p(dmask[name]), C, B, s3, s3, p(ws), p(slp),
                          p(dist), None)

        def bwd(name):
            if dmask[name] is None:
                ops._call(logits, 'vg_gam_elbo_bwd', p(logits), p(gain), p(x), p(eps), p(glm), p(dist), p(g_slp), p(g_dist), C, B, V,
                          p(ws), p(d_logits), p(d_gain), p(d_eps), p(tot), 0)
            else:
                ops._call(logits, 'vg_gam_elbo_bwd_masked', p(logits), p(gain), p(x), p(eps), p(glm), p(dmask[name]), p(dist), p(g_slp), p(g_dist),
                          C, B, s3, s3, p(ws), p(d_logits), p(d_gain), p(d_eps), p(tot), 0)

        def timed_us(fn, n):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / n

        for what, call in (('gam_fwd', fwd), ('gam_bwd', bwd)):
            for name in masks:
                fwd(name)                                       # (dist of a forward is what the backward reads)
                for _ in range(10):
                    call(name)
            torch.cuda.synchronize()
            res = {k: [] for k in masks}
            for _ in range(a.rounds):
                for name in masks:
                    res[name].append(timed_us(lambda: call(name), a.launches))
            med, spread = summary(res)
            print(json.dumps(dict(common, bench=what, launches=a.launches, us={k: round(v, 2) for k, v in med.items()},
                                  spread={k: round(v, 4) for k, v in spread.items()},
                                  over_none={k: round(med[k] / med['none'], 4) for k in med})), flush=True)
        del logits, d_logits, ws, x, glm
        torch.cuda.empty_cache()

    if not a.no_step:
        ds = synthetic.make_dataset(num_subjects=1, vols_per_subject=B, num_covariates=C, img_shape=shape, seed=0)
        ids = torch.zeros(B, dtype=torch.int64, device=dev)
        cov = torch.from_numpy(ds['covariates']).to(dev); vol = torch.from_numpy(ds['volumes']).to(dev)
        models = {}
        for name, m_ in masks.items():
            torch.manual_seed(1)
            kw = {} if m_ is None else {'mask': m_}
            m = VAE(num_covariates=C, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda', img_shape=shape, **kw)
            m.use_hip_graph = True
            models[name] = m
        torch.manual_seed(1234)

        def steps(name, n):
            for _ in range(n):
                models[name].train_step(ids, cov, vol)

        for name, m in models.items():
            steps(name, 3)
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
        med, spread = summary(res)
        print(json.dumps(dict(common, bench='captured_step', steps=a.steps, ms={k: round(v, 4) for k, v in med.items()},
                              spread={k: round(v, 4) for k, v in spread.items()},
                              rounds_ms={k: [round(t, 4) for t in v] for k, v in res.items()})), flush=True)


if __name__ == '__main__':
    main()
