"""The latent projection kernels (vg_latent.hip: vg_knn, vg_umap_fuzzy, vg_umap_layout_epoch) and the plan query vg_knn_plan against
float64 on the host build of the kernel sources (tests/emu, g++ -DVG_EMU): the cases and the derived bounds of
tests/projection_cases.py on CPU tensors.  The -m gpu twin is tests/test_projection_gpu.py; every case fits the host build.

Mutants of vg_latent.hip (each applied alone to a scratch copy of the source, host build only, never committed) and what this file
made of them:
  knn_partial_k: `j != q` dropped from the insertion
      21 fail: every test_knn case with k > 1 and both test_knn_workspace_and_output_guards cases, "(b) the query after position 0".
  umap_fuzzy_k: `ii[j] == i ? 0.f :` dropped
      10 fail: w of every test_fuzzy case (error 1 at the row's own place).
  umap_layout_k: two_ab = 2.f * a * b (the sign lost)
      11 fail: every test_layout_epoch case in which an edge is due, from 698 bounds (blobs-n199-neg31-small) to 7.9e5 (blobs-n1-neg5).
  umap_layout_k: floor((double)n / ep) on both sides of the due test
      12 fail: the same 11 (nothing is due, the reference moves) and test_layout_three_epochs_are_three_single_calls.
  umap_layout_k: `% (uint64_t)(N - 1)` in the negative draw
      every test_layout_epoch case with a negative rate above 0 and an epoch >= 1 fails its bound (9 of them, blobs-n1-neg5 first);
      one-vertex-n3-neg31 then divides by zero.
  knn_insert: `key < kl[KB - 1]` made `<=`
      NOT caught, and no case can: the mutant computes the same lists.  Keys are (distance bits, index) and no index reaches a list
      twice (the splits are disjoint), so equality happens only between two "unfilled" keys, and inserting one of those below another
      changes nothing.
  knn_partial_k: `j < c1` made `j < N` in the insertion loop
      NOT caught, and no case can while chunk is a multiple of the 16-candidate tile (check_knn_plan asserts that it is over the plan
      sweep): c1 is then the end of a tile in every split but the last, where c1 = N.
  knn_partial_k / knn_merge_k: the min(q, N - 1) clamps removed
      NOT covered: the idle lanes then only READ past the end of x and of the workspace, which changes no result and no canary; it
      takes an address sanitizer on a stand-alone host program to see it."""
import pytest

import vae_gam_amd  # noqa: F401
import projection_cases as P

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


def test_knn_plan_is_the_restated_arithmetic():
    P.check_knn_plan()


def test_knn_case_matrix_covers_every_class():
    P.check_knn_coverage()


@pytest.mark.parametrize('drop', ['1-D1-k1', '300-D16-k17', '300-D128-k64', '255-D32-k20', '257-D32-k20', '2048-D8-k20', '2049-D5-k64',
                                  '4097-D3-k20', '300-D33-k34'])
def test_knn_coverage_fails_when_a_class_drops_out(drop):
    cases = {c: v for c, v in P.KNN_CASES.items() if c != drop}
    with pytest.raises(AssertionError):
        P.check_knn_coverage(cases)


@pytest.mark.parametrize('cid', list(P.KNN_CASES))
def test_knn(cid):
    P.run_knn(DEV, cid)


@pytest.mark.parametrize('cid', list(P.KNN_GUARD_CASES))
def test_knn_workspace_and_output_guards(cid):
    P.run_knn_guard(DEV, cid)


@pytest.mark.parametrize('cid', list(P.FUZZY_CASES))
def test_fuzzy(cid):
    P.run_fuzzy(DEV, cid)


def test_layout_restatements_agree():
    P.check_layout_restatements()


@pytest.mark.parametrize('cid', list(P.LAYOUT_CASES))
def test_layout_epoch(cid):
    P.run_layout(DEV, cid)


def test_layout_three_epochs_are_three_single_calls():
    P.run_layout_chain(DEV)
