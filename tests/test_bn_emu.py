"""The batch-norm kernels (vg_bn.hip) against float64 on the host build of the kernel sources (tests/emu, g++ -DVG_EMU): the cases of
tests/bn_cases.py on CPU tensors, and the coverage of the production launch plans by those cases.  The -m gpu twin is
tests/test_bn_gpu.py; it also runs 'flush-across' (35 M elements), which no host run could finish in seconds."""
import pytest

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
import bn_cases as B

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


def test_bn_plan_matches_every_case_and_rejects_bad_arguments():
    for cid in B.PLAN_CASES:
        B.case_plan(cid)
    for args in ((3, 1, 10, 2), (0, 1, 10, 1), (2, 0, 10, 1), (2, 1, 0, 1), (2, 1, 10, 0)):
        with pytest.raises(_lib.VgError):
            ops.bn_plan(*args)
        assert _lib.get_lib().dll.vg_bn_ws_bytes(*args) == -1


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('cid', B.HOST_CASES)
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
@pytest.mark.parametrize('cid', B.HOST_CASES)
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


def test_bn_case_matrix_covers_production_plans():
    cov = B.check_coverage()
    assert cov['gpu_only'] == [('flush', 'across')]     # the one production class that only the GPU-only case 'flush-across' reaches
