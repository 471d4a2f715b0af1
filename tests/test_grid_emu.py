"""Derived grids without a GPU: the geometry rule (no library at all), and the embed copy, the embedded GAM/ELBO kernels, one
family-grid train step against the CPU oracle and the embedded model through the host build of the HIP kernels (tests/emu).
tests/test_grid_gpu.py repeats the kernel and model cases on the real library."""
from dataclasses import replace

import pytest
import torch

import toy_case as T
import grid_cases as GC
from vae_gam_amd import _lib, schema


@pytest.fixture(scope='module')
def emu():
    prev = _lib._LIB
    T.load_emu_library()
    yield
    _lib._LIB = prev


def test_geometry_rule_every_axis_length():
    """For every axis length 19..130: the grid is = 2 (mod 4), >= max(n, 22), at most 3 voxels larger; the derived network ends on
    its grid and the decoder sizes mirror the encoder's."""
    for n in range(19, 131):
        g = schema.grid_for((n, n, n))
        assert g[0] == g[1] == g[2]
        assert g[0] % 4 == 2 and g[0] >= max(n, 22) and 0 <= g[0] - n <= 3, (n, g)
        assert g[0] - 4 < max(n, 22)                          # the smallest such size
    for n in range(19, 131):
        geo = schema.net_geometry((n, 19 + (n * 7) % 112, 19 + (n * 13) % 112))
        grid = schema.grid_for(geo.native)
        assert geo.img == grid and geo.pad == tuple(a - b for a, b in zip(grid, geo.native)) and max(geo.pad) <= 3
        assert geo.native == (n, 19 + (n * 7) % 112, 19 + (n * 13) % 112)
        assert geo.dec_sizes()[-1] == grid
        assert geo.enc_sizes()[-1] == geo.dec_seed
        assert geo.dec_sizes()[::-1] == geo.enc_sizes(), (geo.enc_sizes(), geo.dec_sizes())
        for a in range(3):                                     # exact encoder sizes: no floor drops a voxel
            m = grid[a]
            assert [s[a] for s in geo.enc_sizes()] == [m, m - 2, (m - 2) // 2 - 1, (m - 2) // 2 - 3, ((m - 2) // 2 - 4) // 2, ((m - 2) // 2 - 4) // 2 - 2]
            assert (m - 2) % 2 == 0 and ((m - 2) // 2 - 4) % 2 == 0


def test_explicit_entries_and_family_rule_agree():
    hi = schema.net_geometry((82, 98, 70))
    dec, seed = schema.family_decoder((82, 98, 70), hi.enc)
    assert tuple(replace(sp, name='') for sp in hi.dec) == dec and hi.dec_seed == seed
    assert hi.pad == (0, 0, 0) and hi.native == hi.img == (82, 98, 70)
    assert schema.net_geometry((86, 98, 70)).dec == hi.dec                 # a family member takes the same layers
    for img in ((41, 49, 35), (21, 21, 21), (22, 26, 30)):
        geo = schema.net_geometry(img)
        assert geo.img == geo.native == img and geo.pad == (0, 0, 0)
    assert schema.net_geometry((41, 49, 35)).dec[3].k == (5, 3, 3)           # the reference's network, untouched
    assert schema.net_geometry((21, 21, 21)).dec_seed == (1, 1, 1)


def test_unsupported_shapes_are_refused():
    with pytest.raises(ValueError, match='at least 19'):
        schema.net_geometry((18, 22, 22))
    with pytest.raises(ValueError, match='at least 19'):
        schema.grid_for((30, 30, 18))
    with pytest.raises(ValueError, match='last axis'):
        schema.net_geometry((40, 40, 131))
    assert schema.net_geometry((40, 40, 130)).img == (42, 42, 130)


def test_synthetic_signal_is_placed_on_any_grid():
    import numpy as np
    from vae_gam_amd import synthetic
    for shape in ((19, 21, 20), (22, 22, 22), (53, 63, 52)):
        sig = synthetic.large3_signal(shape)
        assert sig.shape == shape and sig.max() > 0
        nz = np.argwhere(sig > 0)
        for a, (lo, hi, n) in enumerate(((15, 25, 41), (34, 47, 49), (9, 22, 35))):
            assert nz[:, a].min() >= int(np.floor(lo * shape[a] / n)) and nz[:, a].max() < int(np.ceil(hi * shape[a] / n)) + 1
    ds = synthetic.make_dataset(num_subjects=1, vols_per_subject=4, num_covariates=3, img_shape=(19, 21, 20))
    assert ds['volumes'].shape == (4, 19, 21, 20) and ds['glm'].shape[0] == 19 * 21 * 20


def test_vae_refuses_small_axis():
    with pytest.raises(ValueError, match='at least 19'):
        GC.make_model('cpu', (18, 21, 20), 3, [[-1, 1]] * 6, None)


@pytest.mark.parametrize('nat,grid,B,C', GC.EMBED_CASES, ids=GC.EMBED_IDS)
def test_embed_copy(emu, nat, grid, B, C):
    GC.run_embed_copy_case('cpu', nat, grid, B)


@pytest.mark.parametrize('nat,grid,B,C', GC.EMBED_CASES, ids=GC.EMBED_IDS)
def test_gam_elbo_embed(emu, nat, grid, B, C):
    GC.run_gam_embed_case('cpu', nat, grid, B, C)


def test_family_grid_train_step_matches_oracle(emu):
    GC.run_family_oracle_step('cpu', (22, 22, 22), B=2, C=3)


def test_embedded_model_equals_model_on_its_grid(emu):
    GC.run_embedded_model_case('cpu', (19, 21, 20), B=2, C=3)


def test_grid_without_a_launch_plan_is_refused_by_the_constructor(emu):
    """91x109x91 -> 94x110x94: bnt5's fused backward stages 110x94 planes of dy, which do not fit LDS; the constructor asks the
    library's planners layer by layer and names the layer, before anything is launched.
    This pins today's LDS budget of one kernel (vg_bn.hip: ft_setup): when that kernel learns to stage its planes in slabs the shape
    becomes legal and this test must move to the next shape a planner refuses."""
    _, _, xu, glm = GC.make_inputs((91, 109, 91), 1, 3)
    with pytest.raises(ValueError, match=r'\(94, 110, 94\).*convt5'):
        GC.make_model('cpu', (91, 109, 91), 3, xu, glm)
