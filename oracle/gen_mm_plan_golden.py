#!/usr/bin/env python3
"""Golden record of what the vg_conv_mm planner (ops.mm_plan) chooses -- tests/golden/mm_plans.json, read by
tests/test_conv_mm_plan.py.

TEST INFRASTRUCTURE.  Pure host arithmetic: no library, no GPU.  Covered:
  every conv layer, both directions, of schema.net_geometry(img) for img in GRIDS (the production tiles: _MM_TUNED and the score);
  every (spec, direction, size, force) the conv_mm case lists of tests/kernel_cases.py and tests/conv_mm_halves_cases.py name
  (the pinned-tile path).
An entry is null where there is no plan; otherwise every scalar and list field of the plan, mm_wins at USE_MM = 1 and a SHA-256 of
the bytes of tau, dlt and aidx.   Usage:  python oracle/gen_mm_plan_golden.py   (rewrites the golden)
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import vae_gam_amd  # noqa: E402,F401
from vae_gam_amd import ops  # noqa: E402
from vae_gam_amd.schema import net_geometry  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mm_plans.json')
GRIDS = ((41, 49, 35), (82, 98, 70), (21, 21, 21), (40, 48, 34), (33, 37, 29), (64, 64, 40))


def plan_of(spec, direction, isz, force=None):
    """The plan of a layer's launch from the LAYER'S input size isz: the forward reads isz, the data gradient reads the output size."""
    isz = tuple(isz)
    if direction == 'fwd':
        return ops.mm_plan(spec, 'fwd', isz, None, force=force)
    return ops.mm_plan(spec, 'bwd', spec.out_size(isz), isz, force=force)


def launches():
    """-> [(key, spec, direction, layer input size, force)]"""
    import conv_mm_halves_cases as H
    import kernel_cases as K
    out = []
    for img in GRIDS:
        geo = net_geometry(img)
        for specs, sizes in ((geo.enc, geo.enc_sizes()), (geo.dec, geo.dec_sizes())):
            for i, spec in enumerate(specs):
                for direction in ('fwd', 'bwd'):
                    out.append(('net %s %s %s' % ('x'.join(map(str, img)), spec.name, direction), spec, direction, tuple(sizes[i]), None))
    for case in K.CONV_MM_CASES + K.CONV_MM_LOOP_CASES + H.FWD_CASES + H.BWD_CASES + [H.LOOP_CASE]:
        cid, sname, direction, isz, force = case[:5]
        out.append(('case %s' % cid, K.MM_SPECS[sname], direction, tuple(isz), tuple(force)))
    for cid, sname, isz, _, _, _ in H.STATS_OF_CASES:
        out.append(('case stats_of %s' % cid, K.MM_SPECS[sname], 'fwd', tuple(isz), None))
    assert len(set(k for k, *_ in out)) == len(out)
    return out


def record(plan):
    """What the golden keeps of one plan (None stays None)."""
    if plan is None:
        return None
    rec = {}
    for k, v in sorted(vars(plan).items()):
        if k.startswith('_') or isinstance(v, np.ndarray):
            continue
        rec[k] = [int(a) for a in v] if isinstance(v, (list, tuple)) else (v if isinstance(v, str) else int(v))
    h = hashlib.sha256()
    for k in ('tau', 'dlt', 'aidx'):
        a = getattr(plan, k)
        assert a.dtype == np.int32 and a.ndim == 1, (k, a.dtype, a.shape)
        rec['n_' + k] = int(a.size)
        h.update(np.ascontiguousarray(a).tobytes())
    rec['sha256'] = h.hexdigest()
    rec['mm_wins'] = bool(ops.mm_wins(plan))
    return rec


def entries():
    """{key: record} with ops.USE_MM = 1 while mm_wins is asked."""
    prev = ops.USE_MM
    ops.USE_MM = 1
    try:
        return {key: record(plan_of(spec, direction, isz, force)) for key, spec, direction, isz, force in launches()}
    finally:
        ops.USE_MM = prev


if __name__ == '__main__':
    e = entries()
    with open(GOLDEN, 'w') as f:
        f.write('{\n%s\n}\n' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(e[k], sort_keys=True)) for k in sorted(e)))   # an entry per line
    net = [k for k in e if k.startswith('net ')]
    print('%s: %d entries (%d network launches, %d of them plans), %d bytes'
          % (GOLDEN, len(e), len(net), sum(e[k] is not None for k in net), os.path.getsize(GOLDEN)))
