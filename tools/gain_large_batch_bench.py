"""Gain block forward + backward time on the GPU (device events after warm-up): C = 8 covariates (task with HRF, 6 GP motion
covariates, sex), n = 6 inducing points and n = 64 (jitter 1e-4), at B = 512 and 1024 on the blocked path, the same B forced onto the
tiled path (vg_gp_gain_*_tiled), and B = 1025, 2048, 4096 on the tiled path.  Gate: tiled at B = 2048 no slower than blocked at 1024.

    python tools/gain_large_batch_bench.py [--out gain_bench.json] [--iters 5]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vae_gam_amd  # noqa: E402,F401
from vae_gam_amd import _lib, ops, utils  # noqa: E402

KINDS = ('lin_hrf',) + ('gp',) * 6 + ('lin',)


def make_case(B, n, seed=0):
    import numpy as np
    g = torch.Generator().manual_seed(seed)
    P, table, xus = [], [], []

    def put(t):
        off = sum(x.numel() for x in P); P.append(t.reshape(-1).float()); return off
    for kind in KINDS:
        row = [int(kind.startswith('gp')), int(kind.endswith('hrf')), len(xus), put(1 + torch.randn(1, generator=g)),
               put(0.3 * torch.randn(1, generator=g)), 0, 0, 0, 0, 0]
        if kind.startswith('gp'):
            r = 0.2 * torch.randn(n, n, generator=g)
            row[5], row[6] = put(torch.randn(n, generator=g)), put(2 * torch.eye(n) + r @ r.t())
            row[7], row[8] = put(0.3 * torch.randn((), generator=g)), put(0.3 * torch.randn((), generator=g))
            xus.append(torch.linspace(-4.1, 6.2, n))
        table.append(row)
    C = len(KINDS)
    hrf = torch.tensor(utils.hrf(np.arange(0, 20, 1.4))).float().double()
    consts = ops.GainConsts(torch.tensor(table, dtype=torch.int64).cuda(), torch.stack(xus).float().cuda(), hrf.cuda(), n,
                            jitter_ku=1e-4 if n > 6 else 0.0)
    return dict(consts=consts, flat=torch.cat(P).cuda(), cov=(torch.randn(B, C, generator=g) * 1.5).cuda(),
                eps=torch.randn(C, B, generator=g).cuda(), g_tv=torch.randn(C, B, generator=g).cuda())


def time_case(B, n, tiled, iters):
    lib = _lib.get_lib()
    k = make_case(B, n)
    consts, flat, cov, eps, g_tv = k['consts'], k['flat'], k['cov'], k['eps'], k['g_tv']
    d = consts.desc(B)
    C = consts.C
    ws = torch.empty(lib.size('vg_gp_gain_ws_bytes', C, B, n) // 8, dtype=torch.float64, device='cuda')
    tv = torch.empty(C, B, device='cuda'); kl = torch.empty(1, device='cuda'); fg = torch.zeros_like(flat)
    g_kl = torch.ones(1, device='cuda')
    P = ops._p
    suf = '_tiled' if tiled else ''
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        lib.call('vg_gp_gain_fwd' + suf, ctypes.byref(d), P(consts.table), P(flat), P(consts.xu), P(cov), int(cov.stride(0)), P(eps),
                 P(consts.hrf), P(ws), P(tv), P(kl), None, None, None, None, st)

    def bwd():
        lib.call('vg_gp_gain_bwd' + suf, ctypes.byref(d), P(consts.table), P(flat), P(consts.xu), P(cov), int(cov.stride(0)), P(eps),
                 P(consts.hrf), P(ws), P(g_tv), P(g_kl), P(fg), st)
    for _ in range(2):
        fwd(); bwd()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf, tb = [], []
    for _ in range(iters):
        ev[0].record(); fwd(); ev[1].record(); bwd(); ev[2].record()
        torch.cuda.synchronize()
        tf.append(ev[0].elapsed_time(ev[1])); tb.append(ev[1].elapsed_time(ev[2]))
    tf.sort(); tb.sort()
    ok = bool(torch.isfinite(tv).all()) and bool(torch.isfinite(fg).all())
    return {'B': B, 'n': n, 'path': 'tiled' if (tiled or B > 1024) else 'blocked', 'fwd_ms': tf[len(tf) // 2], 'bwd_ms': tb[len(tb) // 2],
            'total_ms': tf[len(tf) // 2] + tb[len(tb) // 2], 'finite': ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--n', type=int, nargs='*', default=[6, 64])
    ap.add_argument('--B', type=int, nargs='*', default=None, help='only these batches (no gate)')
    args = ap.parse_args()
    cases = ((512, False), (1024, False), (512, True), (1024, True), (1025, False), (2048, False), (4096, False))
    if args.B:
        cases = tuple((B, False) for B in args.B)
    rows = []
    for n in args.n:
        for B, tiled in cases:
            r = time_case(B, n, tiled, args.iters)
            rows.append(r)
            print('n=%3d B=%5d %-7s fwd %8.3f ms  bwd %8.3f ms  total %8.3f ms%s' % (n, B, r['path'], r['fwd_ms'], r['bwd_ms'], r['total_ms'],
                                                                                  '' if r['finite'] else '  NON-FINITE'), flush=True)
            torch.cuda.empty_cache()
        if args.B:
            continue
        t1024 = [r['total_ms'] for r in rows if r['n'] == n and r['B'] == 1024 and r['path'] == 'blocked'][0]
        t2048 = [r['total_ms'] for r in rows if r['n'] == n and r['B'] == 2048][0]
        print('gate n=%d: tiled B=2048 %.3f ms vs blocked B=1024 %.3f ms -> %s' % (n, t2048, t1024, 'PASS' if t2048 <= t1024 else 'FAIL'))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
