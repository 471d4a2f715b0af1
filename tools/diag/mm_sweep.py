"""Sweep conv_mm's tile choice (waves, PD planes per block, PHB rows, cc channels per chunk, buffers) for one launch:
  [VG_IMG=82x98x70] python tools/diag/mm_sweep.py B C layer:dir ...
Prints us per launch for every tile the planner accepts, and first the register-tiled kernel's time for the same launch.  The
forward of a layer that feeds a batch norm without one on its own input (convt2, convt4) is launched as the train step launches
it: no prologue, statistics partials, stored rectified."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import vae_gam_amd
from vae_gam_amd import ops, _lib
from vae_gam_amd.schema import net_geometry
B, C = int(sys.argv[1]), int(sys.argv[2])
geom = net_geometry(tuple(int(v) for v in os.environ.get('VG_IMG', '41x49x35').split('x')))
dev = 'cuda'


def timeit(fn, n=10):
    fn(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


layers = {sp.name: (sp, i, 'enc') for i, sp in enumerate(geom.enc)}
layers.update({sp.name: (sp, i, 'dec') for i, sp in enumerate(geom.dec)})
for item in sys.argv[3:]:
    name, direction = item.split(':')
    sp, i, part = layers[name]
    sizes = geom.enc_sizes() if part == 'enc' else geom.dec_sizes()
    N = B if part == 'enc' else (C + 1) * B
    x = torch.randn((N, sp.ci) + sizes[i], device=dev)
    wshape = ((sp.co, sp.ci) if sp.kind == 'conv' else (sp.ci, sp.co)) + tuple(sp.k)
    w = torch.randn(wshape, device=dev) * 0.1
    b = torch.zeros(sp.co, device=dev)
    sc = torch.ones((N // B) * sp.ci, device=dev); sh = torch.zeros((N // B) * sp.ci, device=dev)
    dy = torch.randn((N, sp.co) + sizes[i + 1], device=dev)
    base = ops.mm_plan(sp, direction, sizes[i] if direction == 'fwd' else sizes[i + 1], None if direction == 'fwd' else sizes[i])
    print('%s: default PD %d cc %d tpc %d' % (item, base.PD, base.cc, base.tpc))
    ci = base.CI
    aimg0 = base.gather(w)
    step_like = name in ('convt2', 'convt4')
    if direction == 'fwd':
        run = (lambda pl, a: ops.conv_mm(x, pl, a, b, False, None, None, 1, None, B, True)[0]) if step_like else \
            (lambda pl, a: ops.conv_mm(x, pl, a, b, True, sc, sh, B, None, None))
        wf = ops.pack_weight(w, sp, 'fwd')
        direct = (lambda: ops.conv_forward(x, wf, b, sp, False, None, None, 1, B, True)) if step_like else \
            (lambda: ops.conv_forward(x, wf, b, sp, True, sc, sh, B))
    else:
        run = lambda pl, a: ops.conv_mm(dy, pl, a, None, False, None, None, 1, x)
        wb = ops.pack_weight(w, sp, 'bwd')
        direct = lambda: ops.conv_backward_data(dy, wb, sp, sizes[i], x)
    ref = run(base, aimg0)
    print('  register-tiled kernel %8.1f us    default tile (W %d PD %d PHB %d cc %d db %d) %8.1f us' % (
        timeit(direct, 20), base.waves, base.PD, base.PHB, base.cc, base.dbuf, timeit(lambda: run(base, aimg0), 20)), flush=True)
    shi = base.shi
    for W in (8, 4):
      for PD in range(1, 9):
        for nslab in (1, 2, 3, 4, 6):
          PHB = (base.PH + nslab - 1) // nslab
          if nslab > 1 and (base.PH + PHB - 1) // PHB != nslab:
              continue
          for cc in [c for c in range(ci, 0, -1) if ci % c == 0][:3]:
            for dbuf in (0, 1):
                pl = ops.mm_plan(sp, direction, sizes[i] if direction == 'fwd' else sizes[i + 1], None if direction == 'fwd' else sizes[i], force=(W, PD, PHB, cc, dbuf))
                if pl is None:
                    continue
                aimg = pl.gather(w)
                fn = lambda: run(pl, aimg)
                try:
                    out = fn()
                    err = float((out - ref).abs().max())
                    t = timeit(fn, 10)
                except Exception as e:
                    print('  W %d PD %d PHB %d cc %d db %d: %s' % (W, PD, PHB, cc, dbuf, str(e)[:80])); continue
                print('  W %d PD %d PHB %2d cc %2d db %d tpc %d  %8.1f us   maxdiff %.2e' % (W, PD, PHB, cc, dbuf, pl.tpc, t, err), flush=True)
