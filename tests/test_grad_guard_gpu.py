"""The gradient guard on the MI355X: the kernel cases of tests/grad_guard_cases.py through libvaegam_hip.so, and the guarded train
step of the bench model (B=64, C=8, 41x49x35) eager and replayed from the captured hipGraph.  CPU twin: tests/test_grad_guard_emu.py.

No-sync check: torch.cuda.set_sync_debug_mode('error') around train_step (the ROCm build honours it: the test first shows that a
device-to-host read raises in that mode)."""
import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
from vae_gam_amd.vae_reg_GP import VAE
import grad_guard_cases as G

pytestmark = pytest.mark.gpu
B, C = 64, 8


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.fixture(scope='module')
def bench_data():
    from vae_gam_amd import synthetic
    ds = synthetic.make_dataset(num_subjects=3, vols_per_subject=98, num_covariates=C, seed=0)
    ds['x'] = torch.from_numpy(ds['volumes']).cuda(); ds['cov'] = torch.from_numpy(ds['covariates']).cuda()
    return ds


def _model(ds, graph, **guard):
    torch.manual_seed(1)
    model = VAE(num_covariates=C, glm_maps=ds['glm'], xu_ranges=ds['xu_ranges'], device_name='cuda')
    model.set_grad_guard(**guard)
    model.use_hip_graph = graph
    return model


def _batch(ds, s):
    return torch.zeros(B, dtype=torch.int64, device='cuda'), ds['cov'][s * B:(s + 1) * B], ds['x'][s * B:(s + 1) * B]


def _captured(model):
    return bool(model._graphs) and all(v is not False for v in model._graphs.values())


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('n32', [1, 255, 256, 257, 5000, G.N32_MODEL])
def test_norm_fp32_lengths_with_the_fp64_buffer(n32):
    G.run_norm_case('cuda', n32, G.N64_MODEL, seed=n32)


@pytest.mark.parametrize('n32,n64', [(257, 0), (0, 1), (0, G.N64_MODEL), (4099, 3)])
def test_norm_single_buffers(n32, n64):
    G.run_norm_case('cuda', n32, n64, seed=7)


def test_norm_does_not_depend_on_alignment():
    G.run_unaligned_norm_case('cuda')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('clips', [True, False])
def test_clipping_matches_adam_on_the_clipped_gradient(dtype, clips):
    G.run_clip_case('cuda', dtype, clips, n=200000)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_nonfinite_step_is_skipped(dtype, bad):
    G.run_skip_case('cuda', dtype, bad, n=200000)


def test_nonfinite_step_is_applied_when_skipping_is_off():
    G.run_nonfinite_without_skip_case('cuda')


# ------------------------------------------------------------------------------------------------ model
def test_defaults_take_the_plain_entry_points(bench_data, monkeypatch):
    names = []
    lib = _lib.get_lib()
    orig = lib.call
    monkeypatch.setattr(lib, 'call', lambda name, *a: (names.append(name), orig(name, *a))[1], raising=False)
    model = _model(bench_data, graph=False)
    model.train_step(*_batch(bench_data, 0))
    torch.cuda.synchronize()
    assert names.count('vg_adam_advance') == 1 and names.count('vg_adam_step') == 2 and not [n for n in names if 'guard' in n]


def test_guarded_replay_equals_guarded_eager_launches(bench_data):
    """use_hip_graph with the guard on (clipping every step, skip armed): 4 replayed steps == 4 eager steps bit for bit --
    losses, parameters, Adam's device scalars and the guard's state block."""
    res = {}
    for mode in ('eager', 'graph'):
        model = _model(bench_data, graph=(mode == 'graph'), max_grad_norm=1.0, skip_nonfinite=True)
        torch.manual_seed(77)
        losses = [float(model.train_step(*_batch(bench_data, s))) for s in range(4)]
        if mode == 'graph':
            assert _captured(model), 'capture fell back to eager'
        torch.cuda.synchronize()
        res[mode] = (losses, model.optimizer.groups[torch.float32]['p'].clone(), model.epsilon.detach().clone(),
                     model.optimizer._scalars.cpu().numpy().copy(), model.optimizer.guard_state.cpu().numpy().copy())
    e, g = res['eager'], res['graph']
    assert e[0] == g[0], (e[0], g[0])
    assert torch.equal(e[1], g[1]) and torch.equal(e[2], g[2])
    assert e[3].tobytes() == g[3].tobytes() and e[4].tobytes() == g[4].tobytes()
    assert g[3][2] == 4.0
    st = g[4]
    print('guard state after 4 steps', st)
    assert (st[ops.GUARD_SEEN], st[ops.GUARD_SKIPPED], st[ops.GUARD_CLIPPED]) == (4.0, 0.0, 4.0)      # norms of this model are far above 1


def test_nan_voxel_under_replay_skips_the_step(bench_data):
    model = _model(bench_data, graph=True, skip_nonfinite=True)
    torch.manual_seed(77)
    model.train_step(*_batch(bench_data, 0))
    assert _captured(model), 'capture fell back to eager'
    torch.cuda.synchronize()
    before = {dt: {k: gr[k].clone() for k in ('p', 'm', 'v')} for dt, gr in model.optimizer.groups.items()}
    assert model.optimizer.device_step_count() == 1
    ids, cov, x = _batch(bench_data, 1)
    bad = x.clone(); bad[5, 20, 24, 17] = float('nan')
    loss = model.train_step(ids, cov, bad)
    torch.cuda.synchronize()
    assert not np.isfinite(float(loss))
    for dt, gr in model.optimizer.groups.items():
        for k in ('p', 'm', 'v'):
            assert torch.equal(gr[k], before[dt][k]), (dt, k)
    assert model.optimizer.device_step_count() == 1 and model.optimizer.step_count == 2
    loss = model.train_step(*_batch(bench_data, 2))
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    for dt, gr in model.optimizer.groups.items():
        assert not torch.equal(gr['p'], before[dt]['p']) and bool(torch.isfinite(gr['p']).all())
    st = model.optimizer.guard_stats()
    assert (st['seen'], st['skipped']) == (3, 1)
    assert model.optimizer.device_step_count() == 2


@pytest.mark.parametrize('graph', [True, False], ids=['replay', 'eager'])
def test_guarded_step_does_not_synchronise(bench_data, graph):
    model = _model(bench_data, graph=graph, max_grad_norm=1.0, skip_nonfinite=True)
    model.train_step(*_batch(bench_data, 0))                  # capture / lazy initialisations happen here
    model.train_step(*_batch(bench_data, 1))
    torch.cuda.synchronize()
    batch = _batch(bench_data, 2)
    probe = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):                     # the mode is honoured: a device-to-host read raises
            probe.item()
        model.train_step(*batch)                              # raises if anything in the step copies back or synchronises
        model.train_step(*batch)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert model.optimizer.guard_stats()['seen'] == 4
