"""The rectified decoder hand-off on the MI355X: the cases of tests/rectified_cases.py through libvaegam_hip.so, and the toy model's
captured train step against eager launches with everything on.  CPU twin: tests/test_rectified_emu.py."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import rectified_cases as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('name', [c[0] for c in R.MM_PRODUCERS])
def test_conv_mm_stores_rectified(name):
    R.run_mm_producer_case(DEV, name)


def test_tconv3d_s2_stores_rectified():
    R.run_tconv_producer_case(DEV)


@pytest.mark.parametrize('which', ['plane', 'direct'])
def test_corr3d_stores_rectified(which):
    R.run_corr_producer_case(DEV, which)


@pytest.mark.parametrize('name', list(R.CONSUMERS))
def test_rectified_input_changes_no_bit(name, monkeypatch):
    R.run_consumer_case(DEV, name, monkeypatch)


def test_toy_step_with_handoff_equals_step_without():
    R.run_model_bit_equal_case(DEV)


def test_captured_toy_step_equals_eager_launches_with_handoff_on():
    """Three train steps of the toy model replayed from the captured hipGraph == the same three steps launched eagerly, with the
    rectified hand-off on: losses and parameters bit for bit (as test_model_gpu.py's replay test asserts
    for the 41x49x35 model)."""
    res = {}
    for mode in ('eager', 'graph'):
        model, x, cov = R.toy_model(DEV)
        assert model.rectified_handoff is True
        model.use_hip_graph = (mode == 'graph')
        torch.manual_seed(77)
        ids = torch.zeros(R.B_TOY, dtype=torch.int64, device=DEV)
        losses = [float(model.train_step(ids, cov, x * (1 - 0.1 * s))) for s in range(3)]
        if mode == 'graph':
            assert model._graphs and all(v is not False for v in model._graphs.values()), 'capture fell back to eager'
        res[mode] = (losses, model.optimizer.groups[torch.float32]['p'].clone(), model.epsilon.detach().clone())
    assert res['eager'][0] == res['graph'][0], (res['eager'][0], res['graph'][0])
    assert torch.equal(res['eager'][1], res['graph'][1])
    assert torch.equal(res['eager'][2], res['graph'][2])
