"""The gain block's batch limit on the host side: ops.check_gain_batch, the batch a VAE's gain block sees under data parallelism,
and the CLI refusing a --batch-size above 4,096 before it opens any data file (no GPU needed)."""
import types

import pytest

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops
from vae_gam_amd import multsubj_reg_run_GP as cli
from vae_gam_amd import vae_reg_GP as vae_reg


def test_check_gain_batch_names_the_limit():
    ops.check_gain_batch(4096)
    with pytest.raises(ValueError, match='4096'):
        ops.check_gain_batch(4097)


def _model_stub(world, dp_gain):
    m = types.SimpleNamespace(dp=None if world == 1 else types.SimpleNamespace(world_size=world), dp_gain=dp_gain)
    m.gain_batch = lambda B: vae_reg.VAE.gain_batch(m, B)
    return m


def test_vae_checks_the_batch_the_gain_block_sees():
    one = _model_stub(1, 'global')
    vae_reg.VAE.check_gain_batch(one, 4096)
    with pytest.raises(ValueError, match='4096'):
        vae_reg.VAE.check_gain_batch(one, 4097)
    glob = _model_stub(8, 'global')                            # 8 ranks x 513 = 4104 volumes in one joint draw
    assert glob.gain_batch(513) == 4104
    with pytest.raises(ValueError, match="dp_gain='local'"):
        vae_reg.VAE.check_gain_batch(glob, 513)
    vae_reg.VAE.check_gain_batch(_model_stub(8, 'local'), 513)


def test_cli_refuses_a_batch_above_the_limit_before_loading_data(tmp_path, monkeypatch):
    def no_loaders(*a, **k):
        raise AssertionError('data loaders built before the batch-size check')
    monkeypatch.setattr(cli.data, 'setup_data_loaders', no_loaders)
    missing = str(tmp_path / 'no_such.csv')
    with pytest.raises(SystemExit) as e:
        cli.main(['--train_csv', missing, '--test_csv', missing, '--batch-size', '4097', '--save_dir', str(tmp_path)])
    assert '4096' in str(e.value) and '4097' in str(e.value)
    with pytest.raises(SystemExit, match='4096'):          # dp_gain='local' trains on 1,025-volume slices, the export still draws 4,100
        cli.check_batch_size(4100, world_size=4, dp_gain='local')
    cli.check_batch_size(4096, world_size=8, dp_gain='global')
