"""The fully connected engine (vg_fc.hip) against float64 on the MI355X: the cases of tests/fc_cases.py through libvaegam_hip.so --
every body fc_body<W, a_vec, b_vec> of both tile sizes, the job mixes of one launch, the refusals.  CPU twin: tests/test_fc_emu.py.

Largest err / tol per case on an MI355X when the matrix was written (C, then cx where the case has the ones column; the error itself
was 0.5 to 3.5 x that of a plain fp32 torch product on the CPU in every case):
  t32-00 .030   t32-01 .022   t32-02 .027 .013   t32-10 .018   t32-11 .009   t32-12 .019   t32-20 .031 .012   t32-21 .030 .051
  t32-22 .014 .006   t64-00 .004   t64-11 .005   t64-22 .052 .024   t64-02 .068   t64-20 .054 .026   t64-10 .049   t64-01 .057
  t64-21 .050 .024   t64-12 .040   t32-12-split .008   t32-22-whole .025 .020   t64-11-whole .050   t64-12-split .004
  t64-22-whole .067 .026   a-ptr+1 .030   mask-ptr+2 .022   heads-fwd .032   batch-gap .035   k1 .061   k64-inside .027
  k192 .019 .009   heads-dgrad .041   heads-wgrad .088 .042
Largest at 32 x 32: 0.088 (heads-wgrad, K = 9); at 64 x 64: 0.068 (t64-02).  The job mixes repeat their jobs' single-launch values:
every job whose tile the joint launch keeps is bit-identical to its launch alone, and t64-11 run at 32 x 32 (vote-mixed) gives 0.005."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import fc_cases as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('cid', list(F.CLASS_CASES))
def test_fc_body_matches_float64(cid):
    F.run_single(DEV, cid)


@pytest.mark.parametrize('cid', list(F.PRODUCTION_CASES))
def test_fc_production_classes(cid):
    F.run_single(DEV, cid)


@pytest.mark.parametrize('cid', list(F.EXTRA_CASES))
def test_fc_strides_alignment_and_pipeline_lengths(cid):
    F.run_single(DEV, cid)


@pytest.mark.parametrize('mid', list(F.MIX_CASES))
def test_fc_job_mix(mid):
    F.run_mix(DEV, mid)


def test_fc_plan_and_launcher_refuse_alike():
    F.run_refusals(DEV)
