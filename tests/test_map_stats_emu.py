"""Map statistics without a GPU: the accumulate kernel (vg_gam_stats_accumulate) on random inputs and VAE.map_statistics /
MapStatistics / mk_stat_maps on small models, through the host build of the HIP kernels (tests/emu).  tests/test_map_stats_gpu.py
repeats the cases on the real library and adds the 41x49x35 case and the command line.  A forward pass takes seconds on the host
build: the model cases share one run per model (map_stats_cases.model_run)."""
import pytest

import toy_case as T
import map_stats_cases as SC
from vae_gam_amd import _lib


@pytest.fixture(scope='module')
def emu():
    prev = _lib._LIB
    T.load_emu_library()
    yield
    _lib._LIB = prev


@pytest.mark.parametrize('nat,grid,B,C,S,subj,mask', SC.KERNEL_CASES, ids=SC.KERNEL_IDS)
def test_stats_kernel(emu, nat, grid, B, C, S, subj, mask):
    SC.run_kernel_case('cpu', nat, grid, B, C, S, subj, mask)


def test_two_launches_on_halves_fold_like_the_reference(emu):
    SC.run_halves_case('cpu')


def test_refusals_leave_the_accumulators_untouched(emu):
    SC.run_refusals_case('cpu')


def test_undefined_values_are_zero():
    SC.run_undefined_values('cpu')


@pytest.mark.parametrize('kind', list(SC.MODEL_KINDS))
def test_sums_against_reconstruct(emu, kind):
    SC.run_sums_against_reconstruct('cpu', kind)


@pytest.mark.parametrize('kind', list(SC.MODEL_KINDS))
def test_derived_statistics_against_numpy(emu, kind):
    SC.run_derived_statistics('cpu', kind)


def test_group_t_on_three_subjects(emu):
    SC.run_group_t_three_subjects('cpu', 'toy_21x21x21')


def test_at_mean_twice_gives_equal_bits(emu):
    SC.run_at_mean_is_deterministic('cpu', '19x21x20_masked')


def test_an_id_outside_the_range_raises_before_any_launch(emu):
    SC.run_bad_ids_raise_before_any_launch('cpu', '19x21x20_masked')


def test_stat_maps_files(emu, tmp_path):
    SC.run_stat_maps_files('cpu', '19x21x20_masked', tmp_path, motion=False)
