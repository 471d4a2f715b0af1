"""The gradient guard (device-side global-norm clipping and non-finite step skip) on the host build of the kernel sources
(tests/emu, g++ -DVG_EMU): the kernels against numpy / torch.optim.Adam, the 21x21x21 toy model through optimiser, train step,
train_epoch and checkpoint, and the command-line flags.  The -m gpu twin is tests/test_grad_guard_gpu.py."""
import os

import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, multsubj_reg_run_GP, ops
import grad_guard_cases as G
import toy_case as T


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('n32', [1, 255, 256, 257, 5000, G.N32_MODEL])
def test_norm_fp32_lengths_with_the_fp64_buffer(n32):
    G.run_norm_case('cpu', n32, G.N64_MODEL, seed=n32)


@pytest.mark.parametrize('n32,n64', [(257, 0), (0, 1), (0, G.N64_MODEL), (4099, 3)])
def test_norm_single_buffers(n32, n64):
    G.run_norm_case('cpu', n32, n64, seed=7)


def test_norm_does_not_depend_on_alignment():
    G.run_unaligned_norm_case('cpu')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('clips', [True, False])
def test_clipping_matches_adam_on_the_clipped_gradient(dtype, clips):
    G.run_clip_case('cpu', dtype, clips)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')])
def test_nonfinite_step_is_skipped(dtype, bad):
    G.run_skip_case('cpu', dtype, bad)


def test_nonfinite_step_is_skipped_with_clipping_on():
    G.run_skip_case('cpu', torch.float32, float('nan'), max_norm=10.0)


def test_nonfinite_step_is_applied_when_skipping_is_off():
    G.run_nonfinite_without_skip_case('cpu')


def test_guard_rejects_bad_arguments():
    st = G.new_state('cpu')
    with pytest.raises(_lib.VgError):
        _lib.get_lib().call('vg_grad_guard', None, 0, None, 0, 0.0, 0, ops._p(st), ops._p(st), None)
    assert _lib.get_lib().dll.vg_grad_guard_ws_bytes(0, 0) < 0
    assert _lib.get_lib().size('vg_grad_guard_ws_bytes', G.N32_MODEL, G.N64_MODEL) == (256 + 64) * 8


# ------------------------------------------------------------------------------------------------ model
B, C = 4, 3


def _noise(seed, Bn=B):
    gen = torch.Generator().manual_seed(seed)
    return {'eps_w': torch.randn(Bn, 1, generator=gen), 'eps_d': torch.randn(Bn, 32, generator=gen),
            'eps_beta': torch.randn(C, Bn, generator=gen)}


def _model_and_inputs(seed=5):
    x, cov, xu, glm = T.make_inputs(B, C, seed=seed)
    return T.make_model(C, xu, glm), x, cov, torch.zeros(B, dtype=torch.int64)


def _entry_points(monkeypatch):
    names = []
    lib = _lib.get_lib()
    orig = lib.call
    monkeypatch.setattr(lib, 'call', lambda name, *a: (names.append(name), orig(name, *a))[1], raising=False)
    return names


def test_guard_off_is_the_plain_step_and_guard_at_scale_one_equals_it(monkeypatch):
    """Defaults: the step calls the plain entry points only (the launch list of a step is unchanged).  With the guard on and a
    max_grad_norm no gradient reaches, the guarded entry points give bit-equal parameters and moments after 2 steps."""
    names = _entry_points(monkeypatch)
    plain, x, cov, ids = _model_and_inputs()
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False and plain.optimizer.guard_state is None
    for s in (1, 2):
        plain.train_step(ids, cov, x, noise=_noise(s))
    assert names.count('vg_adam_advance') == 2 and names.count('vg_adam_step') == 4
    assert not [n for n in names if 'guard' in n]
    assert plain.optimizer.guard_stats() is None
    del names[:]
    guarded, _, _, _ = _model_and_inputs()
    guarded.set_grad_guard(max_grad_norm=1e30, skip_nonfinite=True)
    for s in (1, 2):
        guarded.train_step(ids, cov, x, noise=_noise(s))
    assert names.count('vg_grad_guard') == 2 and names.count('vg_adam_advance_guarded') == 2 and names.count('vg_adam_step_guarded') == 4
    assert 'vg_adam_advance' not in names and 'vg_adam_step' not in names
    a, b = G.flat_state(plain), G.flat_state(guarded)
    for dt in a:
        for k in ('p', 'g', 'm', 'v'):
            assert torch.equal(a[dt][k], b[dt][k]), (dt, k)
    st = guarded.optimizer.guard_stats()
    assert (st['seen'], st['skipped'], st['clipped'], st['last_scale']) == (2, 0, 0, 1.0)
    assert guarded.optimizer.device_step_count() == 2


def test_clipped_model_step_matches_the_clipped_reference_update():
    plain, x, cov, ids = _model_and_inputs()
    before = {dt: s['p'] for dt, s in G.flat_state(plain).items()}
    plain.train_step(ids, cov, x, noise=_noise(1))
    grads = {dt: s['g'] for dt, s in G.flat_state(plain).items()}
    norm = float(np.sqrt(sum(float((g.numpy().astype(np.float64) ** 2).sum()) for g in grads.values())))
    max_norm = 0.3 * norm                                             # well below the measured first-step norm
    want, c, _ = G.clipped_reference_update(before, grads, max_norm)
    assert c < 0.31
    clipped, _, _, _ = _model_and_inputs()
    clipped.set_grad_guard(max_grad_norm=max_norm)
    clipped.train_step(ids, cov, x, noise=_noise(1))
    got = G.flat_state(clipped)
    for dt in got:
        assert torch.equal(got[dt]['g'], grads[dt])                 # .grad stays the raw gradient
        tol = 1e-6 if dt == torch.float32 else 1e-12
        np.testing.assert_allclose(got[dt]['p'].numpy(), want[dt].numpy(), rtol=tol, atol=tol)
    st = clipped.optimizer.guard_stats()
    np.testing.assert_allclose(st['last_norm'], norm, rtol=1e-12)     # the reported norm is the pre-clip norm
    np.testing.assert_allclose(st['last_scale'], c, rtol=1e-12)
    assert (st['seen'], st['clipped'], st['skipped']) == (1, 1, 0)


class _Loader(list):
    """minimal loader: an iterable of sample dicts with a .dataset whose length is the number of volumes"""
    @property
    def dataset(self):
        return range(sum(s['volume'].shape[0] for s in self))


def test_nan_volume_skips_the_step_and_training_goes_on(capsys, tmp_path):
    model, x, cov, ids = _model_and_inputs()
    model.set_grad_guard(skip_nonfinite=True)
    bad = x.clone(); bad[1, 3, 4, 5] = float('nan')
    torch.manual_seed(3)
    before = G.flat_state(model)
    loss = model.train_step(ids, cov, bad)
    assert not bool(torch.isfinite(loss).all())
    after = G.flat_state(model)
    for dt in after:
        for k in ('p', 'm', 'v'):
            assert after[dt][k].numpy().tobytes() == before[dt][k].numpy().tobytes(), (dt, k)
        assert bool(torch.isfinite(after[dt]['p']).all())
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert model.optimizer.device_step_count() == 0 and model.optimizer.step_count == 1      # the host mirror counts the skipped step
    loss = model.train_step(ids, cov, x)
    assert bool(torch.isfinite(loss).all())
    moved = G.flat_state(model)
    assert all(not torch.equal(moved[dt]['p'], before[dt]['p']) for dt in moved)
    assert all(bool(torch.isfinite(moved[dt]['p']).all()) for dt in moved)
    st = model.optimizer.guard_stats()
    assert (st['seen'], st['skipped'], st['last_apply']) == (2, 1, 1) and np.isfinite(st['norm_mean'])
    assert model.optimizer.device_step_count() == 1
    # an epoch holding the bad minibatch reports a finite mean loss (the skipped step's loss is left out)
    sample = lambda v: {'volume': v, 'covariates': cov, 'subjid': ids}
    epoch_loss = model.train_epoch(_Loader([sample(bad), sample(x)]))
    assert np.isfinite(epoch_loss)
    assert model.optimizer.device_step_count() == 2
    # the per-epoch log line and scalars
    model.save_dir = str(tmp_path)
    from vae_gam_amd.vae_reg_GP import _JsonlWriter
    model.writer = _JsonlWriter(str(tmp_path))
    capsys.readouterr()
    model._log_grad_guard()
    assert 'skipped 2 of 4 steps' in capsys.readouterr().out
    model.writer.flush()
    import json
    rows = {r['tag']: r['value'] for r in map(json.loads, open(model.writer.path))}
    assert rows['GradGuard/skipped'] == 2.0 and rows['GradGuard/clipped'] == 0.0
    assert np.isfinite(rows['GradGuard/norm_mean']) and rows['GradGuard/norm_max'] >= rows['GradGuard/norm_mean']
    assert model.optimizer.guard_stats()['seen'] == 0                 # the counters restart with the epoch


def test_checkpoint_keeps_the_guard_settings_and_the_device_step_count(tmp_path):
    model, x, cov, ids = _model_and_inputs()
    model.save_dir = str(tmp_path)
    model.save_state('plain.tar')
    model.set_grad_guard(max_grad_norm=2.5, skip_nonfinite=True)
    bad = x.clone(); bad[0, 0, 0, 0] = float('inf')
    torch.manual_seed(3)
    model.train_step(ids, cov, bad)
    model.train_step(ids, cov, x)
    assert model.optimizer.step_count == 2
    model.save_state('guarded.tar')
    ck = torch.load(os.path.join(tmp_path, 'guarded.tar'), weights_only=False)
    assert ck['max_grad_norm'] == 2.5 and ck['skip_nonfinite'] is True
    assert {float(s['step']) for s in ck['optimizer_state']['state'].values()} == {1.0}      # the device's t, not the host mirror
    plain_ck = torch.load(os.path.join(tmp_path, 'plain.tar'), weights_only=False)
    assert 'max_grad_norm' not in plain_ck and 'skip_nonfinite' not in plain_ck
    other, _, _, _ = _model_and_inputs()
    other.save_dir = str(tmp_path)
    other._graphs['stale'] = object()
    other.load_state(os.path.join(tmp_path, 'guarded.tar'))
    assert other.max_grad_norm == 2.5 and other.skip_nonfinite is True and not other._graphs
    assert other.optimizer.step_count == 1 and other.optimizer.device_step_count() == 1
    for (n, p), (_, q) in zip(model.named_parameters(), other.named_parameters()):
        assert torch.equal(p, q), n
    # a checkpoint without the keys loads with the guard off
    other.load_state(os.path.join(tmp_path, 'plain.tar'))
    assert other.max_grad_norm is None and other.skip_nonfinite is False and other.optimizer.guard_state is None


def test_set_grad_guard_validates_and_drops_graphs():
    model, _, _, _ = _model_and_inputs()
    model._graphs['stale'] = object()
    model.set_grad_guard(max_grad_norm=1.0)
    assert not model._graphs and model.max_grad_norm == 1.0 and model.skip_nonfinite is False
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            model.set_grad_guard(max_grad_norm=bad)
    model.set_grad_guard()
    assert model.optimizer.guard_on is False


def test_constructor_keywords():
    from vae_gam_amd.vae_reg_GP import VAE
    x, cov, xu, glm = T.make_inputs(B, C, seed=5)
    torch.manual_seed(1)
    m = VAE(num_covariates=C, glm_maps=glm, xu_ranges=xu, device_name='cpu', img_shape=T.IMG, max_grad_norm=4.0, skip_nonfinite=True)
    assert m.max_grad_norm == 4.0 and m.skip_nonfinite is True and m.optimizer.guard_on


# ------------------------------------------------------------------------------------------------ command line
def test_cli_flags_parse_and_reach_the_model(monkeypatch, tmp_path):
    p = multsubj_reg_run_GP.build_parser()
    a = p.parse_args([])
    assert a.max_grad_norm is None and a.skip_nonfinite is False
    a = p.parse_args(['--max_grad_norm', '1.5', '--skip_nonfinite', 'true'])
    assert a.max_grad_norm == 1.5 and a.skip_nonfinite is True
    assert p.parse_args(['--skip_nonfinite']).skip_nonfinite is True
    seen = {}

    class Stop(Exception):
        pass

    def fake_vae(**kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(multsubj_reg_run_GP.vae_reg, 'VAE', fake_vae)
    monkeypatch.setattr(multsubj_reg_run_GP.data, 'setup_data_loaders', lambda **kw: {})
    monkeypatch.delenv('WORLD_SIZE', raising=False); monkeypatch.delenv('VG_DP_FORCE', raising=False)
    with pytest.raises(Stop):
        multsubj_reg_run_GP.main(['--max_grad_norm', '1.5', '--skip_nonfinite', 'yes', '--save_dir', str(tmp_path)])
    assert seen['max_grad_norm'] == 1.5 and seen['skip_nonfinite'] is True
