"""The gradient guard under data parallelism, on CPU: 2 ranks (gloo) running the product model on halves of a global minibatch
through the host build of the kernels.  The guard runs behind the gradient all-reduce, on buffers that are identical on every rank,
in a fixed summation order: both ranks compute the same norm bit for bit and take the same clip / skip decision with no further
collective -- also when only ONE rank's slice held the nan."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import toy_case as T
from vae_gam_amd import _lib

B_GLOBAL, C = 8, 3


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_main(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    from vae_gam_amd import dp as dpmod
    T.load_emu_library()
    ctx = dpmod.DataParallelContext.from_env(backend='gloo')
    x, cov, xu, glm = T.make_inputs(B_GLOBAL, C, seed=11)
    model = T.make_model(C, xu, glm, dp=ctx)
    model.set_grad_guard(max_grad_norm=1e-3, skip_nonfinite=True)        # far below any gradient norm of this model: step 1 clips
    b = B_GLOBAL // world
    sl = slice(rank * b, (rank + 1) * b)
    ids = torch.zeros(b, dtype=torch.int64)
    g32 = model.optimizer.groups[torch.float32]
    out = {'p0': g32['p'].clone()}
    model.train_step(ids, cov[sl], x[sl])
    out.update(p1=g32['p'].clone(), eps1=model.epsilon.detach().clone(), state1=model.optimizer.guard_state.clone())
    bad = x[sl].clone()
    if rank == 0:
        bad[1, 2, 3, 4] = float('nan')                                   # only rank 0's slice holds it
    model.train_step(ids, cov[sl], bad)
    out.update(p2=g32['p'].clone(), eps2=model.epsilon.detach().clone(), state2=model.optimizer.guard_state.clone(),
               t=model.optimizer.device_step_count(), stats=model.optimizer.guard_stats())
    torch.save(out, os.path.join(out_dir, 'rank%d.pt' % rank))
    ctx.shutdown()


@pytest.fixture(autouse=True)
def restore_library():
    prev = _lib._LIB
    yield
    _lib._LIB = prev


def test_both_ranks_clip_and_skip_alike(tmp_path):
    port = _free_port()
    mp.spawn(_rank_main, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = [torch.load(os.path.join(tmp_path, 'rank%d.pt' % r)) for r in range(2)]
    for k in ('p0', 'p1', 'eps1', 'state1', 'p2', 'eps2', 'state2'):
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k       # replicas and verdicts identical, bit for bit
    s1, s2 = a['state1'].numpy(), a['state2'].numpy()
    assert s1[2] == 1.0 and 0.0 < s1[1] < 1.0 and np.isfinite(s1[0])     # step 1: applied, clipped
    assert not torch.equal(a['p1'], a['p0'])
    assert s2[2] == 0.0 and not np.isfinite(s2[0])                       # step 2: skipped on BOTH ranks
    assert torch.equal(a['p2'], a['p1']) and torch.equal(a['eps2'], a['eps1'])
    for o in (a, b):
        assert o['t'] == 1
        assert (o['stats']['seen'], o['stats']['clipped'], o['stats']['skipped']) == (2, 1, 1)
