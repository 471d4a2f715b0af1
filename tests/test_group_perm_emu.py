"""Group permutation inference without a GPU: the sign-flip max-statistic kernel (vg_signflip_maxstat) against its numpy reference,
to the bit, MapStatistics.group_permutation on synthetic accumulators and mk_stat_maps with n_perm, through the host build of the HIP
kernels (tests/emu).  tests/test_group_perm_gpu.py repeats the cases on the real library and adds the real-size case and the command
line."""
import pytest

import toy_case as T
import group_perm_cases as GP
from vae_gam_amd import _lib


@pytest.fixture(scope='module')
def emu():
    prev = _lib._LIB
    T.load_emu_library()
    yield
    _lib._LIB = prev


@pytest.mark.parametrize('S', GP.S_CASES)
def test_kernel_subjects(emu, S):
    GP.run_subjects_case('cpu', S)


def test_every_instance_is_hit(emu):
    GP.run_every_instance_is_hit()


@pytest.mark.parametrize('V', GP.V_CASES)
def test_kernel_voxels(emu, V):
    GP.run_voxels_case('cpu', V)


@pytest.mark.parametrize('P', GP.P_CASES)
def test_kernel_permutations(emu, P):
    GP.run_permutations_case('cpu', P)


@pytest.mark.parametrize('tail', GP.TAILS)
def test_kernel_tails(emu, tail):
    GP.run_tail_case('cpu', tail)


@pytest.mark.parametrize('tail', GP.TAILS)
@pytest.mark.parametrize('kind', GP.ZERO_CASES)
def test_kernel_zero_scale(emu, kind, tail):
    GP.run_zero_scale_case('cpu', kind, tail)


def test_dead_voxels_do_not_pollute_a_negative_maximum(emu):
    GP.run_polluted_maximum_case('cpu')


@pytest.mark.parametrize('tail', GP.TAILS)
def test_kernel_exact_ties(emu, tail):
    GP.run_ties_case('cpu', tail)


def test_kernel_hand_case(emu):
    GP.run_hand_case('cpu')


def test_refusals_leave_the_outputs_untouched(emu):
    GP.run_refusals_case('cpu')


def test_group_permutation_basics(emu):
    GP.run_basics_case('cpu')


def test_group_permutation_errors(emu):
    GP.run_errors_case('cpu')


def test_planted_signal(emu):
    GP.run_planted_signal_case('cpu')


def test_threshold(emu):
    GP.run_threshold_case('cpu')


def test_stat_maps_files_with_permutations(emu, tmp_path):
    GP.run_stat_maps_files('cpu', tmp_path)
