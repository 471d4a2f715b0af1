"""Step time of bench.py's default configuration (B=64, C=8, 41x49x35, one GPU, captured step) with the gradient guard on.

bench.py never turns the guard on; this builds the same model from the same synthetic data and seeds, and times the same loop.

  python tools/grad_guard_bench.py --guard both                 one run, guard on: one JSON line (compare with bench.py's ms_per_step)
  python tools/grad_guard_bench.py --ab --rounds 7              off / on alternating in ONE process, median and min per arm
  python tools/grad_guard_bench.py --guard both --trace-steps 5 a few eager steps only (run under rocprofv3 --kernel-trace --stats:
                                                                  kernel durations, and the memcpy table shows the step copies nothing back)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUARDS = {'off': (None, False), 'clip': (1.0, False), 'skip': (None, True), 'both': (1.0, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--guard', choices=sorted(GUARDS), default='both')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--covariates', type=int, default=8)
    ap.add_argument('--ab', action='store_true', help='alternate guard off / --guard in one process')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--trace-steps', type=int, default=0, help='run this many eager steps and exit (for a profiler)')
    a = ap.parse_args()

    import torch
    import vae_gam_amd  # noqa: F401
    from vae_gam_amd import synthetic, _lib
    from vae_gam_amd.DataClass_GP import DeviceResidentData
    from vae_gam_amd.vae_reg_GP import VAE
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda', 0)
    _lib.get_lib()
    B, C = a.batch, a.covariates
    subjects = 2
    while subjects * 98 < 2 * B:
        subjects += 1
    ds = synthetic.make_dataset(num_subjects=subjects, vols_per_subject=98, num_covariates=C, seed=0)
    torch.manual_seed(1)
    model = VAE(num_covariates=C, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda')
    data = DeviceResidentData(torch.from_numpy(ds['volumes']), torch.from_numpy(ds['covariates']), torch.from_numpy(ds['subjid']),
                              batch_size=B, shuffle=True, seed=0, device=dev, rank=0, world=1)
    batches = list(iter(data))
    torch.manual_seed(1234)
    pos = [0]

    def run_steps(n):
        loss = None
        for _ in range(n):
            smp = batches[pos[0] % len(batches)]; pos[0] += 1
            loss = model.train_step(smp['subjid'], smp['covariates'], smp['volume'])
        return loss

    def timed(guard):
        model.set_grad_guard(*GUARDS[guard])                 # drops the captured step: the next train_step captures this arm's launches
        run_steps(a.warmup)
        assert model._graphs and all(v is not False for v in model._graphs.values()), 'capture fell back to eager'
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(a.steps)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    if a.trace_steps:
        model.set_grad_guard(*GUARDS[a.guard])
        run_steps(a.trace_steps)
        torch.cuda.synchronize()
        print(json.dumps({'guard': a.guard, 'eager_steps': a.trace_steps, 'stats': model.optimizer.guard_stats()}), flush=True)
        return
    model.use_hip_graph = True
    if not a.ab:
        ms = timed(a.guard)
        print(json.dumps({'guard': a.guard, 'ms_per_step': round(ms, 4), 'steps': a.steps, 'warmup': a.warmup,
                          'stats': model.optimizer.guard_stats()}), flush=True)
        return
    arms = {'off': [], a.guard: []}
    for _ in range(a.rounds):
        for g in arms:
            arms[g].append(timed(g))
    out = {g: {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'all_ms': [round(x, 4) for x in v]}
           for g, v in arms.items()}
    out['overhead_median_us'] = round(1e3 * (out[a.guard]['median_ms'] - out['off']['median_ms']), 2)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
