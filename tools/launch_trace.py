#!/usr/bin/env python3
"""Launch trace of one eager train step of the toy model on the host build of the kernels (tests/emu): one line per library call
(entry point, every argument), then a SHA-256 of the whole trace.  Numbers are printed as they are, descriptor structs field by
field, pointers as `ptr` / `null` (never an address), so two trees that launch the same kernels with the same arguments in the same
order print the same digest.  A diagnostic for refactors of ops.py / the model's wiring; not a test.

  python tools/launch_trace.py [--img X Y Z] [--mask] [--guard] [-B 4] [-C 3]
--img: the volume grid (21 21 21: the toy network; 22 22 22: a family grid; e.g. 20 21 19: an embedded one); --mask: a brain mask
(the _masked GAM entries); --guard: the gradient guard (vg_grad_guard and the guarded Adam pair)."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def render(a, ctype=None):
    if ctype is ctypes.c_void_p or isinstance(a, ctypes.c_void_p):
        return 'ptr' if getattr(a, 'value', a) else 'null'
    if a is None:
        return 'null'
    if hasattr(a, '_obj'):                                  # ctypes.byref(struct)
        return render(a._obj)
    if isinstance(a, ctypes.Structure):
        return '%s{%s}' % (type(a).__name__, ' '.join('%s=%s' % (n, render(getattr(a, n), t)) for n, t in a._fields_))
    if isinstance(a, ctypes.Array):
        return '[%s]' % ' '.join(render(e) for e in a)
    return repr(a)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--img', type=int, nargs=3, default=(21, 21, 21))
    ap.add_argument('--mask', action='store_true')
    ap.add_argument('--guard', action='store_true')
    ap.add_argument('-B', type=int, default=4)
    ap.add_argument('-C', type=int, default=3)
    args = ap.parse_args()
    import toy_case
    from vae_gam_amd import _lib
    from vae_gam_amd.vae_reg_GP import VAE
    toy_case.load_emu_library()
    img = toy_case.IMG = tuple(args.img)                    # make_inputs draws volumes of toy_case.IMG
    x, cov, xu, glm = toy_case.make_inputs(args.B, args.C)
    kw = {}
    if args.mask:
        m = np.zeros(img, np.uint8); m[2:-2, 3:-1, 1:-3] = 1
        kw['mask'] = m
    if args.guard:
        kw.update(max_grad_norm=1.0, skip_nonfinite=True)
    torch.manual_seed(1)
    model = VAE(num_covariates=args.C, glm_maps=glm, xu_ranges=xu, device_name='cpu', img_shape=img, **kw)
    lib, lines = _lib.get_lib(), []
    for kind in ('call', 'size'):
        def traced(name, *a, _inner=getattr(lib, kind), _kind=kind):
            lines.append('%s %s(%s)' % (_kind, name, ', '.join(render(v) for v in a)))
            return _inner(name, *a)
        setattr(lib, kind, traced)
    torch.manual_seed(2)
    loss = model.train_step(torch.zeros(args.B, dtype=torch.int64), cov, x)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    print('# %d calls, loss %r, sha256 %s' % (len(lines), float(loss), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == '__main__':
    main()
