"""The GAM/ELBO, latent, loss and weight-packing kernels (vg_gam.hip, vg_latent.hip, vg_gather_f32) against float64 on the host build of
the kernel sources (tests/emu, g++ -DVG_EMU): the cases and the derived bounds of tests/gam_cases.py on CPU tensors.  The -m gpu twin
is tests/test_gam_gpu.py.  Every case fits the host build, so gam_cases.GPU_ONLY is empty.

Mutants (each applied alone to a scratch copy of the sources, host build only, never committed), what this file made of them (80 tests)
and what test_kernels_emu.py's run_gam_case / run_latent_case / run_loss_case tests made of them:
  vg_gam.hip: LOG_SQRT_2PI = 0.9189f
      52 fail: the slp of every test_gam_plain / _special / _embedded / _masked case (207 u M already at C0-B1-V1) and with them
      test_gam_workspace.  The old tests pass.
  vg_gam.hip: the `dd > 0.f` guard of the distance gradient dropped
      2 fail: test_gam_special[zero-dist-C8-B9-V257] and [zero-dist-C16-B3-V63], "not finite".  The old tests pass.
  vg_gam.hip: total_accumulate ignored in gam_bwd_fold_total_k
      22 fail: `total` of every case with a prefilled bias buffer (the first is test_gam_plain[C0-B7-V63]) and the three prefilled
      test_gam_workspace cases.  The old tests pass.
  vg_latent.hip: latent_bwd_k's (d - floor_) replaced by d
      9 fail: g_a of the seven test_latent_sample cases with the floor flag set (-set, -last) and of test_latent_null_gradients
      [B4-L32-G9-set], [B1040-L32-G17-last].  Of the old tests test_latent_sample_kl fails too (its tiny_d case).
  vg_gam.hip: pack_weights_k's mode == 2 flip dropped
      3 fail: test_pack_weights[modes], [many], [big].  The old tests pass.
  vg_latent.hip: the row loop stride gridDim.x * nw replaced by nw (latent_fwd_k and latent_bwd_k)
      NOT caught: all 80 pass, and no comparison of values can catch it.  Every block then also walks the rows of the blocks above it
      and stores the same bits there again (the kernels read nothing they write), so the mutant computes the same results, only
      slower (this file took several times as long on it)."""
import pytest

import vae_gam_amd  # noqa: F401
import gam_cases as G

DEV = 'cpu'


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


def _host(cases):
    return [c for c in cases if c not in G.GPU_ONLY]


@pytest.mark.parametrize('cid', _host(G.PLAIN_CASES))
def test_gam_plain(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', _host(G.SPECIAL_CASES))
def test_gam_special(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', _host(G.EMBED_CASES))
def test_gam_embedded(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', _host(G.MASKED_CASES))
def test_gam_masked(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', _host(G.WS_CASES))
def test_gam_workspace(cid):
    G.run_gam_workspace(DEV, cid)


def test_gam_case_matrix_covers_every_instance():
    cov = G.check_coverage()
    # no instance is left to the GPU alone: the host build runs every case
    assert G.GPU_ONLY == () and cov['gpu_only'] == []


@pytest.mark.parametrize('cid', list(G.LATENT_CASES))
def test_latent_sample(cid):
    G.run_latent(DEV, cid)


@pytest.mark.parametrize('cid', list(G.LATENT_NULL_CASES))
def test_latent_null_gradients(cid):
    G.run_latent_null(DEV, cid)


@pytest.mark.parametrize('cid', list(G.LOSS_CASES))
def test_elbo_loss(cid):
    G.run_loss(DEV, cid)


@pytest.mark.parametrize('tid', list(G.PACK_TABLES))
def test_pack_weights(tid):
    G.run_pack(DEV, tid)


@pytest.mark.parametrize('gid', list(G.GATHER_CASES))
def test_gather(gid):
    G.run_gather(DEV, gid)
