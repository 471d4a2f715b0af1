"""The fully connected engine (vg_fc.hip) against float64 on the host build of the kernel sources (tests/emu, g++ -DVG_EMU): the cases
of tests/fc_cases.py on CPU tensors -- every body of both tile sizes, the job mixes, the refusals -- and the coverage of the production
launch plans by those cases.  The -m gpu twin is tests/test_fc_gpu.py; it also runs the six 64 x 64 bodies of fc_cases.GPU_ONLY, which
the host build walks too slowly for this file to stay under a minute."""
import os
import subprocess
import sys

import pytest

import vae_gam_amd  # noqa: F401
import fc_cases as F

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


@pytest.mark.parametrize('cid', [c for c in F.CLASS_CASES if c not in F.GPU_ONLY])
def test_fc_body_matches_float64(cid):
    F.run_single(DEV, cid)


@pytest.mark.parametrize('cid', [c for c in F.PRODUCTION_CASES if c not in F.GPU_ONLY])
def test_fc_production_classes(cid):
    F.run_single(DEV, cid)


@pytest.mark.parametrize('cid', list(F.EXTRA_CASES))
def test_fc_strides_alignment_and_pipeline_lengths(cid):
    F.run_single(DEV, cid)


@pytest.mark.parametrize('mid', [m for m in F.MIX_CASES if not any(c in F.GPU_ONLY for c in F.MIX_CASES[m][0])])
def test_fc_job_mix(mid):
    F.run_mix(DEV, mid)


def test_fc_plan_and_launcher_refuse_alike():
    F.run_refusals(DEV)


def test_fc_case_matrix_covers_production_plans():
    cov = F.check_coverage()
    # the one production class that only a GPU-only case reaches: fc1's data gradient at 82x98x70, 64 x 64 with the weights read across rows
    assert cov['gpu_only'] == [(64, 1, 2, False, False)]


def test_fc_reads_end_inside_the_operands():
    """fc_cases.run_guarded in a child process: every input buffer ends at an unreadable page, so a load past the end of an operand
    (a clamp of fetch() off by one) ends the child instead of going unnoticed."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = 'import sys; sys.path[:0] = [%r, %r]; import fc_cases; fc_cases.run_guarded()' % (os.path.dirname(tests), tests)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:]); print(r.stderr[-3000:])
    last = [l for l in r.stdout.splitlines() if l.startswith('fc guarded')][-1:]
    assert r.returncode == 0, 'the child ended with status %d after %r' % (r.returncode, last)
    assert last == ['fc guarded: done']
