"""The two-halves launches of vg_conv_mm (16-channel stride-2 transposed convs) against float64 on the host build of the kernel
sources (tests/emu, g++ -DVG_EMU), and the dispatch of those launches (host logic, nothing launched).  The cases are listed in
tests/conv_mm_halves_cases.py; the -m gpu twin is tests/test_conv_mm_halves_gpu.py."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import ops
import conv_mm_halves_cases as H

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


@pytest.mark.parametrize('case', H.FWD_CASES + H.BWD_CASES, ids=[c[0] for c in H.FWD_CASES + H.BWD_CASES])
def test_halves_case(case):
    H.run_halves_case(DEV, case)


def test_halves_sample_loop():
    H.run_loop_case(DEV)


def test_halves_are_distinct_and_partials_layout():
    H.run_distinct_halves_case(DEV)


@pytest.mark.parametrize('case', H.STATS_OF_CASES, ids=[c[0] for c in H.STATS_OF_CASES])
def test_halves_step_launch_is_bit_equal_to_the_register_tiled_engine(case):
    H.run_stats_of_case(DEV, case)


def test_halves_descriptor_refusals():
    H.check_descriptor_refusals()


def test_halves_cases_cover_what_they_are_there_for():
    cases = H.FWD_CASES + H.BWD_CASES
    assert {c[4][0] for c in cases} == {4, 8} and {c[4][4] for c in cases} == {0, 1}
    for name, direction in (('convt2p', 'fwd'), ('convt2', 'fwd'), ('conv4', 'bwd')):
        tiles = [c[4] for c in cases if (c[1], c[2]) == (name, direction)]
        plans = [ops.mm_plan(H.MM_SPECS[name], 'fwd', c[3], None, force=c[4]) if direction == 'fwd' else
                 ops.mm_plan(H.MM_SPECS[name], 'bwd', H.MM_SPECS[name].out_size(c[3]), c[3], force=c[4])
                 for c in cases if (c[1], c[2]) == (name, direction)]
        assert len(tiles) == 2
        assert {(p.PH + p.PHB - 1) // p.PHB > 1 for p in plans} == {False, True}, name       # a row-slab tile and a whole-plane tile
        assert all((p.PDT + p.PD - 1) // p.PD > 1 for p in plans)                            # several blocks per sample and half
    assert any(c[5] for c in H.FWD_CASES)


def test_halves_dispatch(monkeypatch):
    """convt2 forward and conv4's data gradient of the three networks: a two-halves plan on the static [2, 1, 1, 1] instance exists
    for each, VG_CONV_MM=2 takes it, VG_CONV_MM=0 leaves every one on the register-tiled kernels, and the default takes it exactly
    where ops.mm_wins says it measured faster."""
    for tag, spec, direction, read, write in H.production_halves_launches():
        w = torch.zeros(((spec.co, spec.ci) if spec.kind == 'conv' else (spec.ci, spec.co)) + tuple(spec.k))
        plan = ops.mm_plan(spec, direction, read, write)
        assert plan is not None, tag
        assert (plan.mode, plan.CO, plan.co_blk) == ('tconv', 16, 8), tag
        assert H.halves_instance(plan, direction == 'bwd')[1:4] == (4, 4, (2, 1, 1, 1)), tag
        assert (plan.PDT + plan.PD - 1) // plan.PD > 1 or plan.PHB < plan.PH or plan.PD * plan.PH * plan.PW <= 4 * plan.waves * 16, tag
        monkeypatch.setattr(ops, 'USE_MM', 2)
        got = ops._mm_for(None, w, spec, direction, read, write)
        assert got is not None and got[0] is plan and got[1].numel() == plan.aidx.size, tag
        monkeypatch.setattr(ops, 'USE_MM', 0)
        assert ops._mm_for(None, w, spec, direction, read, write) is None, tag
        monkeypatch.setattr(ops, 'USE_MM', 1)
        got = ops._mm_for(None, w, spec, direction, read, write)
        assert (got is not None) == ops.mm_wins(plan), tag
        assert (got is not None) == H.EXPECT_ON_MM[tag], tag
