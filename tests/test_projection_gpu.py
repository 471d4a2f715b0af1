"""The latent projection kernels (vg_latent.hip: vg_knn, vg_umap_fuzzy, vg_umap_layout_epoch) and the plan query vg_knn_plan against
float64 on the MI355X: the cases and the derived bounds of tests/projection_cases.py through libvaegam_hip.so.  CPU twin:
tests/test_projection_emu.py.  The worst err / bound per kernel and case family of an MI355X run is in DESIGN.md section 7.1."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import projection_cases as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


def test_knn_plan_is_the_restated_arithmetic():
    P.check_knn_plan()


def test_knn_case_matrix_covers_every_class():
    P.check_knn_coverage()


@pytest.mark.parametrize('cid', list(P.KNN_CASES))
def test_knn(cid):
    P.run_knn(DEV, cid)


@pytest.mark.parametrize('cid', list(P.KNN_GUARD_CASES))
def test_knn_workspace_and_output_guards(cid):
    P.run_knn_guard(DEV, cid)


@pytest.mark.parametrize('cid', list(P.FUZZY_CASES))
def test_fuzzy(cid):
    P.run_fuzzy(DEV, cid)


@pytest.mark.parametrize('cid', list(P.LAYOUT_CASES))
def test_layout_epoch(cid):
    P.run_layout(DEV, cid)


def test_layout_three_epochs_are_three_single_calls():
    P.run_layout_chain(DEV)
