"""The batch-norm kernels (vg_bn.hip) against float64 on the MI355X: the cases of tests/bn_cases.py through libvaegam_hip.so.
CPU twin: tests/test_bn_emu.py.  'flush-across' (C = 16, 129 groups of 17 samples, P = 1000: 35 M elements, 140 MB per tensor) runs
here only: the fp32 run counter carried across samples needs about 2,048 blocks x 256 threads x more than 64 elements, which the host
build cannot walk in seconds."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import bn_cases as B

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


def test_bn_plan_matches_every_case():
    for cid in B.PLAN_CASES:
        B.case_plan(cid)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('cid', list(B.PLAN_CASES))
def test_bn_stats(cid, relu):
    B.run_stats_case(DEV, cid, relu)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('cid', B.OFFSET_CASES)
def test_bn_stats_offset_mean(cid, relu):
    B.run_stats_case(DEV, cid, relu, offset=True)


@pytest.mark.parametrize('chunks', B.PART_CHUNKS)
def test_bn_stats_from_partials(chunks):
    B.run_parts_case(DEV, chunks)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('cid', list(B.PLAN_CASES))
def test_bn_backward(cid, relu):
    B.run_backward_case(DEV, cid, relu)


@pytest.mark.parametrize('cid', B.TWO_RANK_CASES)
def test_bn_two_ranks_in_one_process(cid):
    B.run_two_rank_case(DEV, cid)


@pytest.mark.parametrize('shape', list(B.CHANNEL_SUM_CASES), ids=lambda s: 'x'.join(map(str, s)))
def test_channel_sum(shape):
    B.run_channel_sum_case(DEV, shape)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('cid', list(B.TCONV1_CASES))
def test_bn_backward_tconv1(cid, relu):
    B.run_tconv1_case(DEV, cid, relu)


def test_bn_backward_tconv1_rejects_17_channels():
    B.run_tconv1_rejects_wide(DEV)


@pytest.mark.parametrize('shape', B.DATA_BN_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_data_bn_grads(shape):
    B.run_data_bn_case(DEV, shape)


@pytest.mark.parametrize('n', [1, 65, 130])
def test_data_bn_nshift(n):
    B.run_nshift_case(DEV, n)
