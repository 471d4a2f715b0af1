"""What the vg_conv_mm planner (vae_gam_amd.conv_mm_plan, reached through ops.mm_plan) chooses, against the record taken before the
planner was split out of ops.py (tests/golden/mm_plans.json, oracle/gen_mm_plan_golden.py): every conv layer and direction of six
volume grids -- the production tiles, _MM_TUNED and the score -- and every pinned tile the conv_mm case lists name.  Host arithmetic
only: no library, no GPU.  A slip in the score or in the tables moves a layer to another tile or another A image; here it fails by
name instead of showing in the benchmark alone."""
import json

import pytest

import gen_mm_plan_golden as G

KEYS = sorted(k for k, *_ in G.launches())


@pytest.fixture(scope='module')
def golden():
    with open(G.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def entries():
    return G.entries()


def test_golden_covers_the_launch_list(golden):
    assert KEYS == sorted(golden)
    net = [k for k in KEYS if k.startswith('net ')]
    assert len(net) == len(G.GRIDS) * 10 * 2 == 120
    assert sum(golden[k] is not None for k in net) == 96
    forced = [f for k, _, _, _, f in G.launches() if k.startswith('case ')]
    assert sum(f is not None for f in forced) >= 40          # the pinned-tile path


@pytest.mark.parametrize('key', KEYS)
def test_plan_matches_golden(golden, entries, key):
    want, got = golden[key], entries[key]
    if want is None:
        assert got is None, key
        return
    assert got is not None, key
    assert sorted(got) == sorted(want), key
    for field in sorted(want):
        assert got[field] == want[field], '%s: %s = %r, recorded %r' % (key, field, got[field], want[field])
