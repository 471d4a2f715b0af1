"""The GAM/ELBO, latent, loss and weight-packing kernels (vg_gam.hip, vg_latent.hip, vg_gather_f32) against float64 on the MI355X: the
cases and the derived bounds of tests/gam_cases.py through libvaegam_hip.so.  CPU twin: tests/test_gam_emu.py.

Worst err / (u M) per case and output on an MI355X when the matrix was written (the bound is 16; `-`: no covariates).  Every map stayed
below 0.39 of its 4 u (|value| + 1) and every full reconstruction below 0.41 of its (C + 4) u A.
  GAM/ELBO                                 slp  dist  d_logits d_gain d_eps total
  C0-B1-V1                                 .47     -   .08     -   .76   .13
  C0-B7-V63                                .73     -  1.07     -   .77   .00
  C0-B8-V255                              1.22     -  1.43     -  1.33   .01
  C0-B9-V256                              1.37     -  1.13     -  1.14   .00
  C0-B17-V257                             1.72     -  1.38     -   .73   .00
  C1-B1-V1023                              .03   .15  1.95   .06  2.83   .45
  C1-B7-V1024                             1.45   .20  1.75   .25  1.41   .00
  C1-B8-V1025                             1.89   .41  1.80   .55  2.73   .00
  C1-B9-V2049                             1.65   .24  2.10   .26  1.30   .04
  C1-B17-V1                               2.29   .47   .84  1.31   .19   .00
  C8-B1-V63                                .27   .24  1.22   .33  1.58   .13
  C8-B7-V255                              1.15   .34  1.82   .66   .86   .00
  C8-B8-V256                              1.02   .44  2.09   .73  1.26   .02
  C8-B9-V257                              1.09   .60  1.89   .70  1.22   .03
  C8-B17-V1023                            2.51   .58  2.05   .44  1.74   .00
  C9-B1-V1024                              .18   .39  1.84   .55  2.47   .00
  C9-B7-V1025                              .80   .57  1.94   .63  1.14   .01
  C9-B8-V2049                             1.89   .40  2.00   .33  1.45   .00
  C9-B9-V1                                2.58   .80  1.01  1.04   .15   .06
  C9-B17-V63                              1.31   .60  1.70  1.05   .39   .01
  C16-B1-V255                              .01   .37  1.66   .29  1.75   .00
  C16-B7-V256                             1.83   .52  1.96   .63   .94   .02
  C16-B8-V257                             1.41   .56  2.05   .81  1.05   .00
  C16-B9-V1023                            1.59   .54  2.22   .62   .87   .00
  C16-B17-V1024                           1.53   .63  2.42   .72  1.02   .00
  zero-dist-C8-B9-V257                    1.29   .64  1.99   .72   .86   .03
  zero-dist-C16-B3-V63                     .84   .49  1.58   .65  1.53   .01
  saturated-C16-B8-V1025                  1.02   .60  2.45   .28  2.12   .01
  saturated-C1-B9-V255                    1.34   .37  1.97   .40  1.27   .02
  gslp0-C9-B7-V256                        1.39   .58  1.99   .72  1.20   .03
  gdist0-C8-B8-V1023                      1.78   .61  1.51   .16  1.34   .00
  embed-5x6x7_in_6x9x8_C1                 1.52   .30  1.64   .28  1.03   .00
  embed-19x21x20_in_22x22x22_C3            .68   .29  1.70   .15  2.70   .00
  embed-9x4x33_in_9x6x34_C9               1.44   .30  1.94   .51  1.96   .00
  embed-same_grid_C0                      1.01     -  1.53     -  1.42   .01
  embed-same_grid_C2                       .53   .22  1.59   .17  2.30   .00
  embed-5x6x7_in_6x9x8_B3_C16             1.70   .44  1.67   .55  1.17   .00
  masked-12x13x14_block_out_C2            1.63   .19  1.41   .38  2.57   .12
  masked-5x6x7_in_6x9x8_C1                 .69   .20  1.47   .21  2.35   .00
  masked-9x4x33_in_9x6x34_B9_C9           1.11   .45  2.09   .45  1.20   .02
  masked-one_voxel_C2                      .33   .68   .86  1.32   .32   .13
  masked-all_ones_C0                      1.26     -  1.10     -  1.59   .02
  masked-all_ones_C2                      1.10   .43  2.14   .28  2.48   .00
  masked-6x9x8_B3_C16                      .84   .47  2.04   .54  1.03   .04
  masked-5x6x7_in_6x9x8_B2_C16             .33   .52  1.59   .91  1.48   .00
  latent sample / KL                         z    kl     d  g_mu   g_w   g_a
  B1-L1-G1                                 .72   .28   .40   .62   .14   .19
  B1-L70-G9-set                           1.09   .67  1.46  1.32  1.41  1.81
  B4-L32-G9-set                           1.03   .73  1.72  1.77  1.61  1.90
  B5-L64-G17                              1.19   .62  1.00  1.99  2.21  2.33
  B5-L65-G1-last                          1.74   .95  1.80   .97  1.38  2.04
  B256-L65-G1                             1.97  1.42  1.33   .98  1.94  3.04
  B256-L32-G9-last                        1.83  1.28  1.84  2.45  2.53  2.75
  B257-L70-G9                             1.77  1.31  1.33  2.33  3.51  3.56
  B257-L1-G17-set                         1.31  1.28  1.79  1.91  1.73  2.14
  B1040-L32-G17-last                      2.03  1.50  2.07  3.01  2.98  3.14
  B1040-L70-G1                            1.95  1.56  1.35  1.00  2.16  3.41
  B1040-L64-G9-set                        2.09  1.71  2.07  3.00  3.03  4.06
  (g_zcat or g_kl null: at most 2.79, 3.51, 3.62 for g_mu, g_w, g_a; both null: exact zeros)
  loss                                    loss  g_kl g_slp g_dist g_gp
  B1-C0                                    .93   .00   .00     -   .09
  B255-C3                                  .85  1.52  1.52   .94   .09
  B256-C0                                 2.40   .00   .00     -   .07
  B257-C16                                 .59   .36   .36   .25   .45
  B4096-C0                                 .17   .00   .00     -   .53
  B4096-C16                               1.26   .00   .00   .80   .00
Largest of all: 4.06 (g_a of B1040-L64-G9-set); of the GAM/ELBO pair: 2.83 (d_eps of C1-B1-V1023).  The reference's own fp32 evaluation
(gam_cases.host, bound 4) reached 3.79 (d_eps of embed-19x21x20_in_22x22x22_C3), 2.65 on d_logits and 2.63 on slp.  The workspace cases
and the weight-packing and gather cases are bit-for-bit comparisons."""
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
import gam_cases as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('cid', list(G.PLAIN_CASES))
def test_gam_plain(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', list(G.SPECIAL_CASES))
def test_gam_special(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', list(G.EMBED_CASES))
def test_gam_embedded(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', list(G.MASKED_CASES))
def test_gam_masked(cid):
    G.run_gam(DEV, cid)


@pytest.mark.parametrize('cid', list(G.WS_CASES))
def test_gam_workspace(cid):
    G.run_gam_workspace(DEV, cid)


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
