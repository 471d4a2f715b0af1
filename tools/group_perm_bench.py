"""What the sign-flip max-statistic costs (MI355X): V = 70,315 voxels (41x49x35), P = 10,000 sign patterns, S = 12 and 24
subjects, two-sided, on standard normal subject means.

Two codes are timed by device events over the same device-resident inputs, alternated in --rounds rounds of one process after a
warm-up, medians over the rounds, the spread (max - min over the median) reported:

  kernel       ops.signflip_maxstat (vg_signflip_maxstat: two launches and the workspace allocation);
  composition  the only way to these numbers without it, in torch on the same device: a +-1 float64 sign matrix in chunks of --chunk
               patterns, matmul with the means, scale, abs, amax over the voxels, the comparison with the observed |sum| and its count.
               Its sums are rounded in another order (a matrix product), so its results differ from the kernel's in the last bits of T:
               a yardstick for the time, not a reference (the tool checks that the maxima agree to 1e-12 and every count to within the
               number of patterns that tie with the observed sum).

The kernel's arithmetic is P V S float64 additions; the rate is given against the float64 vector peak of the MI355X (78.6 TFLOP/s
counting a fused multiply-add as two: 39.3e12 additions per second).  Gate: kernel <= composition.  One JSON object per line; the last
one per S carries the gate."""
import argparse
import json
import os
import statistics
import sys

F64_ADDS_PEAK = 39.3e12         # float64 vector additions per second: 256 CUs x 64 lanes per clock x 2.4 GHz (spec: 78.6 TFLOP/s as FMAs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=41 * 49 * 35)
    ap.add_argument('--perms', type=int, default=10000)
    ap.add_argument('--subjects', type=int, nargs='+', default=[12, 24])
    ap.add_argument('--chunk', type=int, default=1000, help='patterns per chunk of the torch composition')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10, help='calls per timed window')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))

    import numpy as np
    import torch
    import vae_gam_amd  # noqa: F401
    from vae_gam_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs an MI355X'
    lib = _lib.get_lib()
    dev, V, P = 'cuda', a.voxels, a.perms

    for S in a.subjects:
        rng = np.random.default_rng(S)
        m = torch.from_numpy(rng.standard_normal((S, V))).to(dev)
        scale = 1.0 / ((m ** 2).sum(0) * S).sqrt()
        bits = torch.from_numpy(rng.integers(0, 2, size=(P, S))).to(dev)
        bits[0] = 0
        signs = (bits << torch.arange(S, device=dev)).sum(1)
        pm = (1.0 - 2.0 * bits).to(torch.float64)                 # [P, S] of +-1

        def kernel():
            return ops.signflip_maxstat(m, scale, signs, 'two')

        def composition():
            t0 = m.sum(0).abs()
            mx, cnt = [], torch.zeros(V, dtype=torch.int64, device=dev)
            for lo in range(0, P, a.chunk):
                T = pm[lo:lo + a.chunk] @ m
                mx.append((T * scale).abs().amax(1))
                cnt += (T.abs() >= t0).sum(0)
            return t0 * scale, torch.cat(mx), cnt

        codes = {'kernel': kernel, 'composition': composition}

        def timed_ms(fn):
            torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.reps

        for fn in codes.values():                                # warm-up: code objects, the allocator's blocks, the matmul's algorithm
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        k, c = kernel(), composition()
        torch.cuda.synchronize()
        rel = float(((k[1] - c[1]).abs() / c[1].abs()).max())
        ties = int(((signs == 0) | (signs == 2 ** S - 1)).sum())   # the identity, its complement and their repeats tie with the observed
        differ = int((k[2].long() - c[2]).abs().max())             # |sum| exactly; the matrix product rounds them either way
        assert rel < 1e-12 and differ <= ties, (rel, differ, ties)
        res = {n: [] for n in codes}
        for _ in range(a.rounds):
            for name, fn in codes.items():
                res[name].append(timed_ms(fn))
        med = {n: statistics.median(v) for n, v in res.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in res.items()}
        adds = float(P) * V * S
        plan = ops.signflip_plan(S, V, P)
        print(json.dumps({'bench': 'signflip_maxstat', 'S': S, 'V': V, 'P': P, 'tail': 'two', 'rounds': a.rounds, 'reps': a.reps,
                          'library': lib.path, 'plan': plan._asdict(), 'ms': {n: round(t, 4) for n, t in med.items()},
                          'spread': {n: round(t, 4) for n, t in spread.items()}, 'composition_chunk': a.chunk,
                          'kernel_over_composition': round(med['kernel'] / med['composition'], 4),
                          'f64_adds_per_s': round(adds / (med['kernel'] * 1e-3), 0),
                          'share_of_f64_vector_peak': round(adds / (med['kernel'] * 1e-3) / F64_ADDS_PEAK, 4),
                          'maxstat_rel_diff': rel, 'largest_count_diff': differ, 'tying_patterns': ties,
                          'gate': 'kernel <= composition', 'gate_met': bool(med['kernel'] <= med['composition']),
                          'rounds_ms': {n: [round(t, 4) for t in v] for n, v in res.items()}}), flush=True)


if __name__ == '__main__':
    main()
