"""Shared bodies of the direct conv engine's tests (vg_conv.hip: corr3d_direct_k, corr3d_plane_k, tconv3d_s2_k behind vg_corr3d,
vg_tconv3d_s2, vg_tconv3d_s2_stats): one ops.conv_forward / ops.conv_backward_data call per case against float64 F.conv3d /
F.conv_transpose3d on the CPU, at one case per launch class of `ops.conv_plan` (vg_corr3d_plan / vg_tconv3d_s2_plan).  Every case
asserts, from the query and before it launches, the plan fields it is there for (`pins`), so a planner change fails loudly instead of
moving a case out of its class.  Run on CPU tensors through the host build of the kernels (tests/test_conv_direct_emu.py) and on the
GPU through libvaegam_hip.so (tests/test_conv_direct_gpu.py).  The engine is called directly, not through bn_conv_act: which engine a
layer takes in the model plays no part.

Forward cases: random pre-activations in, prologue = ReLU + per-(group, channel) affine with 2 groups ('pro'), ReLU alone ('relu') or
none ('nopro': what the decoder's convt2 / convt4 take since their producers store rectified outputs), bias added, 'relu_out' stores
max(y, 0).  Data-gradient cases ('bwd'): random dy in; 'mask' multiplies by (mask_src > 0) with random mask_src, asserts exact zeros
there, and the reference is float64 autograd of the layer; 'relu_out_ignored' repeats the masked launch with relu_out set in the
descriptor and wants the same bits.  'stats' (vg_tconv3d_s2_stats): mean and rstd of relu(y) per (group, channel) through
ops.bn_stats(pre=partials) against float64 statistics of the float64 y.

Tolerance (the rule of kernel_cases.run_conv_mm_case / run_wgrad_case, never measured from the kernel):
    tol = max(4 * d32, eps32 * sqrt(K) * max|want|)
with d32 = the distance of torch's own fp32 CPU convolution from the float64 result on the same inputs and K = CI * taps of the
launch.  Statistics: the bound derivation of run_conv_mm_case with m = 8 elements a lane adds to a partial (its 2x2x2 brick of one
sample) + 6 shuffle stages.  Every case prints plan, err, d32, err / d32 and tol before it asserts.
Observed err / d32 over the 69 cases: 0.52 to 1.90, on the host build and on the MI355X alike (the kernels are plain fp32 FMA chains
in another summation order than torch's, the same order on both builds: an error of d32's size; a lost element or tap is 1e5 times
that).  Statistics: mean at most 0.003 of its bound, rstd 0.0004."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
from vae_gam_amd.ops import ConvSpec

EPS32 = 2.0 ** -23
_K3 = (3, 3, 3)

# spec name -> layer.  conv1 .. conv5, convt1 .. convt5, convt2p, convt4hr and convt4toy are the layers of the three networks; the
# others exist to reach an instance or a branch no layer reaches: the prologue (VEC_MASK, non-NOPRO) and COC 16 / 0 forms of the 5x3x3
# and 4x4x4 stride-2 correlations (c533, c444, ...c16, ...c24), run-time channel counts (24), rows in the padding for the NOPRO
# instance (convt4p: the zeroed slot tail is only read there), pad_w = 1 with a 5x3x3 kernel (convt4pw), other input channel counts of
# the last layer (convt5c3, convt5c1)
SPECS = {
    'convt5': ConvSpec('convt', 8, 1, _K3, 1), 'convt5c3': ConvSpec('convt', 3, 1, _K3, 1), 'convt5c1': ConvSpec('convt', 1, 1, _K3, 1),
    'convt4': ConvSpec('convt', 8, 8, (5, 3, 3), 2), 'convt4hr': ConvSpec('convt', 8, 8, (4, 4, 4), 2), 'convt4toy': ConvSpec('convt', 8, 8, _K3, 2),
    'convt4p': ConvSpec('convt', 8, 8, (5, 3, 3), 2, (1, 1, 1), (1, 1, 1)), 'convt4hrp': ConvSpec('convt', 8, 8, (4, 4, 4), 2, (1, 1, 1)),
    'convt4c16': ConvSpec('convt', 16, 8, (5, 3, 3), 2), 'convt4c24': ConvSpec('convt', 24, 8, (5, 3, 3), 2),
    'convt4hrc16': ConvSpec('convt', 16, 8, (4, 4, 4), 2), 'convt4hrc24': ConvSpec('convt', 24, 8, (4, 4, 4), 2),
    'c533': ConvSpec('conv', 8, 8, (5, 3, 3), 2), 'c444': ConvSpec('conv', 8, 8, (4, 4, 4), 2),
    'conv1': ConvSpec('conv', 1, 8, _K3, 1), 'conv2': ConvSpec('conv', 8, 8, _K3, 2), 'conv3': ConvSpec('conv', 8, 16, _K3, 1),
    'conv4': ConvSpec('conv', 16, 16, _K3, 2), 'conv5': ConvSpec('conv', 16, 16, _K3, 1), 'conv2c24': ConvSpec('conv', 8, 24, _K3, 2),
    'convt1': ConvSpec('convt', 16, 16, _K3, 1), 'convt3': ConvSpec('convt', 16, 8, _K3, 1),
    'convt2': ConvSpec('convt', 16, 16, _K3, 2), 'convt2p': ConvSpec('convt', 16, 16, _K3, 2, (1, 0, 1), (1, 0, 1)),
    'convt2c24': ConvSpec('convt', 16, 24, _K3, 2), 'convt4c24o': ConvSpec('convt', 8, 24, (5, 3, 3), 2), 'convt4hrc16o': ConvSpec('convt', 8, 16, (4, 4, 4), 2),
    'convt4pw': ConvSpec('convt', 8, 8, (5, 3, 3), 2, (0, 0, 1), (0, 0, 1)),
}

Case = namedtuple('Case', 'id spec direction isz groups per_group opts pins')


def _c(cid, spec, direction, isz, n, opts, **pins):
    return Case(cid, spec, direction, tuple(isz), n[0], n[1], frozenset(opts.split()), pins)


# pins: a plan field name -> the value it must have; or one of the derived properties of props() below (slabs, ragged, short_d, ...)
CASES = [
    # ---- (a) corr3d_plane_k<1,3,3,3,1,4,2,4>: the decoder's last layer (CI 8, CO 1, padding 2: the first tile starts in the depth padding)
    _c('convt5-one-chunk', 'convt5', 'fwd', (5, 7, 6), (2, 2), 'pro', family='plane', COT=1, TDt=4, chunks=1, nbuf=1, slabs=False, dst0=True),
    _c('convt5-one-chunk-relu-out', 'convt5', 'fwd', (5, 7, 6), (2, 2), 'pro relu_out', family='plane', COT=1, chunks=1, nbuf=1),
    _c('convt5-nbuf2-ragged', 'convt5', 'fwd', (3, 4, 33), (2, 2), 'pro', family='plane', COT=1, nbuf=2, CCH=7, chunks=2, ragged=True, slabs=False),
    _c('convt5-nbuf2-4chunks', 'convt5', 'fwd', (3, 20, 20), (2, 2), 'pro', family='plane', COT=1, nbuf=2, chunks=4, ragged=False, slabs=False),
    _c('convt5-tilesd2-short', 'convt5', 'fwd', (9, 24, 24), (2, 2), 'pro', family='plane', COT=1, tilesD=2, short_d=True, CCH=1, nbuf=2),
    _c('convt5-3slabs-nbuf1', 'convt5', 'fwd', (3, 70, 70), (2, 2), 'pro', family='plane', COT=1, nhb=3, nbuf=1, CCH=1),
    _c('convt5-2slabs-nbuf2', 'convt5', 'fwd', (3, 130, 20), (2, 2), 'pro', family='plane', COT=1, nhb=2, nbuf=2),
    _c('convt5-ci3-split', 'convt5c3', 'fwd', (4, 36, 36), (2, 2), 'pro', family='plane', COT=1, nbuf=2, chunks=3),
    _c('convt5-ci1', 'convt5c1', 'fwd', (3, 20, 20), (2, 2), 'pro', family='plane', COT=1, nbuf=1, chunks=1),
    # ---- (b) corr3d_plane_k<8,5,3,3,2,1,1,4,8> NOPRO: convt4's data gradient, masked
    _c('convt4-bwd-one-chunk', 'convt4', 'bwd', (4, 5, 4), (2, 2), 'mask relu_out_ignored', family='plane', KD=5, COC=8, NOPRO=1, chunks=1, slabs=False),
    _c('convt4-bwd-2chunks', 'convt4', 'bwd', (3, 5, 12), (2, 2), 'mask', family='plane', KD=5, COC=8, NOPRO=1, chunks=2, nbuf=1, slabs=False),
    _c('convt4-bwd-8chunks', 'convt4', 'bwd', (3, 16, 16), (2, 2), 'mask', family='plane', KD=5, COC=8, NOPRO=1, chunks=8, slabs=False),
    _c('convt4-bwd-3slabs-tilesd3', 'convt4', 'bwd', (3, 40, 40), (2, 2), 'mask', family='plane', KD=5, COC=8, NOPRO=1, nhb=3, tilesD=3),
    _c('convt4-bwd-unmasked', 'convt4', 'bwd', (3, 5, 12), (2, 2), '', family='plane', KD=5, NOPRO=1),
    # padded: rows in the padding read the zeroed tail of the channel slot (whole planes and slabs; the first tile starts in the depth padding)
    _c('convt4p-bwd-zero-rows', 'convt4p', 'bwd', (3, 5, 12), (2, 2), 'mask', family='plane', KD=5, NOPRO=1, slabs=False, dst0=True, chunks=2),
    _c('convt4p-bwd-zero-rows-slabs', 'convt4p', 'bwd', (3, 40, 40), (2, 2), 'mask', family='plane', KD=5, NOPRO=1, slabs=True, dst0=True),
    # the prologue form (VEC_MASK without NOPRO) and the COC 16 / 0 instances
    _c('k533-fwd-pro', 'c533', 'fwd', (11, 11, 11), (2, 2), 'pro', family='plane', KD=5, COC=8, NOPRO=0, slabs=False),
    _c('k533-fwd-pro-padded-slabs', 'convt4p', 'fwd_as_corr', (3, 40, 40), (2, 2), 'pro', family='plane', KD=5, COC=8, NOPRO=0, slabs=True, dst0=True),
    _c('k533-bwd-coc16', 'convt4c16', 'bwd', (3, 5, 12), (2, 2), 'mask', family='plane', KD=5, COC=16, NOPRO=1),
    _c('k533-bwd-coc0', 'convt4c24', 'bwd', (3, 5, 12), (2, 2), 'mask', family='plane', KD=5, COC=0, NOPRO=1),
    # ---- (b) corr3d_plane_k<8,4,4,4,2,1,1,4,8>: the 4x4x4 convt4 of the 82x98x70 network (no NOPRO twin: boolean predicates)
    _c('convt4hr-bwd-whole', 'convt4hr', 'bwd', (3, 5, 12), (2, 2), 'mask relu_out_ignored', family='plane', KD=4, COC=8, NOPRO=0, slabs=False),
    _c('convt4hr-bwd-slabs', 'convt4hr', 'bwd', (3, 40, 40), (2, 2), 'mask', family='plane', KD=4, COC=8, NOPRO=0, slabs=True, chunks=8),
    _c('convt4hr-bwd-padded', 'convt4hrp', 'bwd', (3, 5, 12), (2, 2), 'mask', family='plane', KD=4, COC=8, dst0=True),
    _c('k444-fwd-pro', 'c444', 'fwd', (10, 10, 12), (2, 2), 'pro', family='plane', KD=4, COC=8, NOPRO=0),
    _c('k444-bwd-coc16', 'convt4hrc16', 'bwd', (3, 5, 12), (2, 2), 'mask', family='plane', KD=4, COC=16),
    _c('k444-bwd-coc0', 'convt4hrc24', 'bwd', (3, 5, 12), (2, 2), 'mask', family='plane', KD=4, COC=0),
    # ---- (c) the 3x3x3 eight-wide plane instances: N * positions * CO >= 1,572,864 (tiny volumes, many samples)
    _c('conv1-whole-tilesd3', 'conv1', 'fwd', (5, 34, 34), (2, 32), 'pro', family='plane', COT=8, S=1, COC=0, small=0, slabs=False, tilesD=3, chunks=1),
    _c('conv1-4slabs', 'conv1', 'fwd', (5, 66, 66), (2, 8), 'pro', family='plane', COT=8, S=1, COC=0, small=0, nhb=4, chunks=1),
    _c('convt5-bwd-whole', 'convt5', 'bwd', (3, 26, 34), (2, 38), '', family='plane', COT=8, S=1, COC=0, small=0, slabs=False, chunks=1),
    _c('convt5-bwd-slabs-masked', 'convt5', 'bwd', (3, 66, 66), (2, 8), 'mask', family='plane', COT=8, S=1, COC=0, small=0, slabs=True, chunks=1),
    _c('conv3-rt-co16-ragged', 'conv3', 'fwd', (5, 18, 18), (2, 64), 'pro', family='plane', COT=8, S=1, COC=0, small=0, slabs=False, ragged=True),
    _c('conv3-rt-co16-slabs', 'conv3', 'fwd', (3, 66, 66), (2, 12), 'pro', family='plane', COT=8, S=1, COC=0, small=0, slabs=True, ragged=True),
    _c('conv3-rt-co16-slabs-even', 'conv3', 'fwd', (3, 70, 34), (2, 24), 'pro', family='plane', COT=8, S=1, COC=0, small=0, nhb=3, CCH=4, chunks=2, ragged=False),
    _c('conv3-bwd-padded', 'conv3', 'bwd', (5, 18, 18), (2, 61), '', family='plane', COT=8, S=1, COC=0, small=0, slabs=False, dst0=True, ragged=True),
    _c('convt3-fwd-padded-pro', 'convt3', 'fwd', (5, 18, 18), (2, 36), 'pro relu_out', family='plane', COT=8, S=1, COC=0, small=0, slabs=False, dst0=True,
       chunks_several=True),
    _c('conv2-2slabs-tilesd3', 'conv2', 'fwd', (7, 81, 67), (2, 25), 'relu', family='plane', COT=8, S=2, COC=8, small=0, nhb=2, tilesD=3, chunks=8),
    _c('conv2-whole', 'conv2', 'fwd', (7, 41, 67), (2, 50), 'relu', family='plane', COT=8, S=2, COC=8, small=0, slabs=False, chunks_several=True),
    _c('convt4toy-bwd-masked', 'convt4toy', 'bwd', (3, 10, 17), (2, 193), 'mask relu_out_ignored', family='plane', COT=8, S=2, COC=8, small=0, slabs=False,
       chunks_several=True),
    _c('conv4-coc16', 'conv4', 'fwd', (7, 41, 67), (2, 25), 'relu', family='plane', COT=8, S=2, COC=16, small=0, slabs=False, chunks_several=True),
    _c('convt2p-bwd-coc16-masked', 'convt2p', 'bwd', (3, 10, 17), (2, 97), 'mask', family='plane', COT=8, S=2, COC=16, small=0, slabs=False,
       chunks_several=True, dst0=True),
    _c('conv2-coc0', 'conv2c24', 'fwd', (7, 41, 67), (2, 17), 'pro', family='plane', COT=8, S=2, COC=0, small=0),
    # ---- (d) the 8-wide direct fallback: more than 256 thread columns (OW > 1024) is a geometry the plane planner refuses
    _c('conv1-direct8-ow1030', 'conv1', 'fwd', (4, 4, 1032), (2, 24), 'pro', family='direct', COT=8, COC=8, small=0),
    _c('conv3-direct8-rt', 'conv3', 'fwd', (3, 4, 1032), (2, 24), 'pro', family='direct', COT=8, COC=0, small=0),
    # ---- (e) corr3d_direct_k<4,...>: the small instances
    _c('conv5-small-s1', 'conv5', 'fwd', (4, 5, 3), (2, 2), 'pro', family='direct', COT=4, S=1, small=1),
    _c('convt1-small-s1-padded', 'convt1', 'fwd', (3, 4, 5), (2, 2), 'pro relu_out', family='direct', COT=4, S=1, small=1),
    _c('conv4-small-s2', 'conv4', 'fwd', (7, 9, 6), (2, 2), 'relu', family='direct', COT=4, S=2, small=1),
    _c('convt2p-bwd-small-s2-masked', 'convt2p', 'bwd', (4, 5, 4), (2, 2), 'mask relu_out_ignored', family='direct', COT=4, S=2, small=1),
    _c('conv2-small-tilesd2-th8', 'conv2', 'fwd', (11, 23, 67), (2, 1), 'relu', family='direct', COT=4, S=2, small=1, BH=8, tilesD=3, short_d=True),
    _c('conv5-small-s1-th8', 'conv5', 'fwd', (5, 11, 34), (1, 2), 'pro', family='direct', COT=4, S=1, small=1, BH=8, tilesD=2, short_d=True),
    # ---- (f) tconv3d_s2_k, COT 4 (small)
    _c('convt2-small-stats', 'convt2', 'fwd', (4, 5, 4), (2, 3), 'nopro stats relu_out', family='tconv', COT=4, COC=16, NOPRO=1, small=1, idle_lanes=True),
    _c('convt2p-small-pro-stats', 'convt2p', 'fwd', (4, 5, 4), (2, 3), 'pro stats', family='tconv', COT=4, COC=16, NOPRO=0, small=1, pad_w1=True),
    _c('conv4-bwd-small-masked', 'conv4', 'bwd', (7, 9, 6), (2, 2), 'mask relu_out_ignored', family='tconv', COT=4, COC=16, NOPRO=1, small=1),
    _c('convt4toy-small-stats', 'convt4toy', 'fwd', (4, 5, 4), (2, 3), 'nopro stats', family='tconv', COT=4, COC=8, NOPRO=1, small=1),
    _c('conv2-bwd-small-masked', 'conv2', 'bwd', (9, 11, 8), (2, 2), 'mask', family='tconv', COT=4, COC=8, NOPRO=1, small=1, odd_ow=False),
    _c('conv2-bwd-small-odd-ow', 'conv2', 'bwd', (9, 11, 9), (2, 2), 'mask', family='tconv', COT=4, COC=8, NOPRO=1, small=1, odd_ow=True),
    _c('convt2-small-coc0', 'convt2c24', 'fwd', (3, 4, 5), (2, 2), 'relu', family='tconv', COT=4, COC=0, NOPRO=0, small=1),
    _c('convt2-small-jw34-ragged-h', 'convt2', 'fwd', (2, 10, 33), (2, 2), 'nopro stats', family='tconv', COT=4, COC=16, small=1, tilesW=2, short_w=True, JW=34,
       tilesH=2, short_h=True),
    _c('convt2-small-ragged-d', 'convt2', 'fwd', (5, 5, 8), (2, 2), 'pro stats', family='tconv', COT=4, COC=16, small=1, tilesD=2, short_d=True, idle_lanes=True),
    # ---- (f) 5x3x3 and 4x4x4 (no `small` gate)
    _c('convt4-fwd-stats', 'convt4', 'fwd', (4, 5, 4), (2, 3), 'nopro stats relu_out', family='tconv', COT=8, KD=5, COC=8, NOPRO=1),
    _c('convt4-fwd-pro-tilesd', 'convt4', 'fwd', (12, 5, 4), (2, 2), 'pro stats', family='tconv', COT=8, KD=5, COC=8, NOPRO=0, short_d=True, idle_lanes=True),
    _c('convt4-fwd-padw1', 'convt4pw', 'fwd', (3, 5, 6), (2, 2), 'nopro', family='tconv', COT=8, KD=5, COC=8, NOPRO=1, pad_w1=True),
    _c('convt4-fwd-coc0', 'convt4c24o', 'fwd', (3, 4, 5), (2, 2), 'pro', family='tconv', COT=8, KD=5, COC=0),
    _c('convt4hr-fwd-stats', 'convt4hr', 'fwd', (4, 7, 5), (2, 3), 'nopro stats', family='tconv', COT=8, KD=4, COC=8, NOPRO=1),
    _c('convt4hr-fwd-pro', 'convt4hr', 'fwd', (3, 4, 5), (2, 2), 'pro relu_out', family='tconv', COT=8, KD=4, COC=8, NOPRO=0),
    _c('convt4hr-fwd-coc16', 'convt4hrc16o', 'fwd', (3, 4, 5), (2, 2), 'relu', family='tconv', COT=8, KD=4, COC=16),
    # ---- (f) COT 8 for 3x3x3: N * positions * CO >= 8,388,608
    _c('convt2-cot8-stats', 'convt2', 'fwd', (6, 8, 5), (2, 108), 'nopro stats relu_out', family='tconv', COT=8, KD=3, COC=16, NOPRO=1, small=0, idle_lanes=True, tilesD=2, short_d=True),
    _c('conv4-bwd-cot8-masked', 'conv4', 'bwd', (13, 17, 11), (2, 108), 'mask', family='tconv', COT=8, KD=3, COC=16, NOPRO=1, small=0, odd_ow=True),
    _c('convt4toy-cot8-stats', 'convt4toy', 'fwd', (6, 8, 5), (2, 216), 'nopro stats', family='tconv', COT=8, KD=3, COC=8, NOPRO=1, small=0),
    _c('conv2-bwd-cot8-masked', 'conv2', 'bwd', (13, 17, 12), (2, 198), 'mask', family='tconv', COT=8, KD=3, COC=8, NOPRO=1, small=0),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

# Cases the host build cannot afford.  None: the cases that must pass a `small` gate (1.5 M outputs for the 8-wide correlations, 8 M for
# the 8-wide 3x3x3 transposed convolution) were expected to need the GPU, but the host build walks them in 0.1 to 1.2 s and the two
# 8 M-output statistics cases in 4.6 and 4.2 s (float64 and fp32 references included), so every case runs on both builds.
CONV_DIRECT_GPU_ONLY = ()
HOST_CASES = tuple(c.id for c in CASES if c.id not in CONV_DIRECT_GPU_ONLY)

RECORDS = []                                            # (id, err, d32, tol) of every case run in this process


# ---------------------------------------------------------------------------------------------------------------- plans
def case_launch(case):
    """-> (spec, direction, relu_in, has_prologue, next_bn).  direction 'fwd_as_corr': a forward-style launch (prologue, bias) of the
    strided correlation that is the spec's DATA GRADIENT -- ops describes no padded stride-2 Conv3d, so the padded correlation with
    a prologue is launched through the descriptor of the padded transposed layer's data gradient (see run_case)."""
    spec = SPECS[case.spec]
    o = case.opts
    relu_in = 'pro' in o or 'relu' in o
    pro = 'pro' in o
    nb = case.per_group if 'stats' in o else None
    return spec, case.direction, relu_in, pro, nb


def case_desc(case):
    """-> (entry point, descriptor) of the case's launch, through the functions conv_forward / conv_backward_data use"""
    spec, direction, relu_in, pro, nb = case_launch(case)
    N = case.groups * case.per_group
    if direction == 'fwd':
        fn, d, _ = ops.conv_fwd_desc(spec, N, case.isz, relu_in, case.per_group, 'relu_out' in case.opts)
        return fn, d
    fn, d = ops.conv_bwd_desc(spec, N, spec.out_size(case.isz), case.isz)
    if direction == 'fwd_as_corr':
        d.relu_in = int(relu_in); d.per_group = case.per_group
    return fn, d


def case_plan(case):
    """the plan of the case's launch from the library's planner; nothing is launched"""
    spec, direction, relu_in, pro, nb = case_launch(case)
    N = case.groups * case.per_group
    if direction == 'fwd_as_corr':
        import ctypes
        fn, d = case_desc(case)
        rec = (ctypes.c_int32 * len(ops.ConvPlan._fields))()
        _lib.get_lib().call('vg_corr3d_plan', ctypes.byref(d), int(pro), rec, len(rec))
        return ops.ConvPlan(_lib.CONV_FAMILIES[rec[0]], *rec[1:])
    return ops.conv_plan(spec, direction, N, case.isz, relu_in, pro, case.per_group, nb)


def props(d, plan):
    """Derived properties of a launch (descriptor + plan) that the kernels branch on"""
    cdiv = lambda a, b: -(-a // b)
    p = {}
    if plan.family == 'plane':
        p['slabs'] = plan.nhb > 1
        p['ragged'] = d.CI % plan.CCH != 0
        p['chunks_several'] = plan.chunks > 1
        p['dst0'] = d.pad_d > 0                                  # ip0 = -pad_d < 0: the first tile's planes land dst0 > 0 into the slot
        p['short_d'] = plan.tilesD > 1 and cdiv(d.OD, plan.TDt) % plan.BD != 0
    elif plan.family == 'direct':
        p['short_d'] = plan.tilesD > 1 and cdiv(d.OD, plan.TDt) % plan.BD != 0
    else:
        p['short_d'] = plan.tilesD > 1 and plan.JD % plan.BD != 0
        p['short_h'] = plan.tilesH > 1 and plan.JH % plan.BH != 0
        p['short_w'] = plan.tilesW > 1 and plan.JW % plan.BW != 0
        p['idle_lanes'] = (plan.BW * plan.BH * plan.BD) % 64 != 0      # lanes past the tile, alive for the statistics shuffle
        p['pad_w1'] = d.pad_w % 2 == 1                           # ow0 = 2 jw - pad_w is odd: column -1 scalar, the rest in pairs
        p['odd_ow'] = (d.OW + d.pad_w) % 2 == 1                  # the last thread column holds one output: scalar store
    return p


def chunk_class(d, plan):
    return '1' if plan.chunks == 1 else 'ragged' if d.CI % plan.CCH else 'several'


def class_tuple(d, plan, masked, stats):
    """What a launch is reduced to for the coverage table.  plane: (family, instance, NOPRO, masked, whole / slabs, nbuf, chunks 1 /
    several / ragged); direct and tconv: (family, instance, NOPRO, small, masked, stats).  `small` is the dispatcher's switch between
    the 4-wide and the 8-wide 3x3x3 instances and nothing else -- no kernel and no planner sees it -- so it is part of the class only
    where the dispatcher consults it (3x3x3); for the 5x3x3 and 4x4x4 transposed convolutions, which have no gate, it is None."""
    inst = (plan.COT, plan.KD, plan.KH, plan.KW, plan.S, plan.TDt, plan.THt, plan.TW, plan.COC)
    if plan.family == 'plane':
        return ('plane', inst, plan.NOPRO, int(masked), 'slabs' if plan.nhb > 1 else 'whole', plan.nbuf, chunk_class(d, plan))
    gated = (plan.KD, plan.KH, plan.KW) == (3, 3, 3)
    return (plan.family, inst, plan.NOPRO, plan.small if gated else None, int(masked), int(stats))


def check_pins(case):
    """-> (descriptor, plan) after asserting every pinned field / property of the case"""
    fn, d = case_desc(case)
    plan = case_plan(case)
    pr = props(d, plan)
    for key, want in case.pins.items():
        got = pr[key] if key in pr else getattr(plan, key)
        assert got == want, '%s: plan has %s = %r, the case is there for %r (%r)' % (case.id, key, got, want, plan)
    assert (fn == 'vg_tconv3d_s2') == (plan.family == 'tconv')
    return d, plan


# ---------------------------------------------------------------------------------------------------------------- running a case
def _affine(sc, sh, groups, per_group, ci, dt):
    N = groups * per_group
    a = sc.to(dt).view(groups, 1, ci, 1, 1, 1).expand(groups, per_group, ci, 1, 1, 1).reshape(N, ci, 1, 1, 1)
    c = sh.to(dt).view(groups, 1, ci, 1, 1, 1).expand(groups, per_group, ci, 1, 1, 1).reshape(N, ci, 1, 1, 1)
    return a, c


def run_case(dev, case, seed=0):
    """One launch of the case against float64 on the CPU (module docstring); -> the record of the case"""
    import ctypes
    case = CASE_BY_ID[case] if isinstance(case, str) else case
    d, plan = check_pins(case)
    spec, direction, relu_in, pro, nb = case_launch(case)
    o = case.opts
    g = torch.Generator().manual_seed(seed)
    groups, per_group = case.groups, case.per_group
    N = groups * per_group
    isz, osz = case.isz, spec.out_size(case.isz)
    conv = spec.kind == 'conv'
    wshape = ((spec.co, spec.ci) if conv else (spec.ci, spec.co)) + tuple(spec.k)
    w = 0.2 * torch.randn(wshape, generator=g)
    taps = spec.k[0] * spec.k[1] * spec.k[2]

    def layer(h, wt, bias):
        if conv:
            return F.conv3d(h, wt, bias, spec.stride)
        return F.conv_transpose3d(h, wt, bias, spec.stride, spec.pad, spec.outpad)

    def dgrad(up, dt):
        x0 = torch.zeros((N, spec.ci) + isz, dtype=dt, requires_grad=True)
        (gx,) = torch.autograd.grad(layer(x0, w.to(dt), None), x0, up.to(dt))
        return gx

    part = None
    masked = 'mask' in o
    if direction == 'fwd':
        x = torch.randn((N, spec.ci) + isz, generator=g)
        b = 0.1 * torch.randn(spec.co, generator=g)
        sc = sh = None
        if pro:
            sc = 1 + 0.3 * torch.randn(groups * spec.ci, generator=g); sh = 0.2 * torch.randn(groups * spec.ci, generator=g)

        def ref(dt):
            h = x.to(dt)
            if relu_in:
                h = torch.relu(h)
            if pro:
                a, c = _affine(sc, sh, groups, per_group, spec.ci, dt)
                h = h * a + c
            return layer(h, w.to(dt), b.to(dt))
        want_pre = ref(torch.float64); own32 = ref(torch.float32)
        want = want_pre
        if 'relu_out' in o:
            want = torch.relu(want); own32 = torch.relu(own32)
        K = spec.ci * taps
        got = ops.conv_forward(x.to(dev), ops.pack_weight(w, spec, 'fwd').to(dev), b.to(dev), spec, relu_in,
                               None if sc is None else sc.to(dev), None if sh is None else sh.to(dev), per_group, nb, 'relu_out' in o)
        if nb:
            got, part = got
    elif direction == 'fwd_as_corr':
        # y = bias + corr(P(x), w) with the geometry (stride, padding) of the transposed layer's data gradient: x has the layer's
        # OUTPUT size and CO channels, y its input size and CI channels; float64: the data gradient of the layer at up = P(x), + bias
        x = torch.randn((N, spec.co) + osz, generator=g)
        b = 0.1 * torch.randn(spec.ci, generator=g)
        sc = 1 + 0.3 * torch.randn(groups * spec.co, generator=g); sh = 0.2 * torch.randn(groups * spec.co, generator=g)

        def ref(dt):
            a, c = _affine(sc, sh, groups, per_group, spec.co, dt)
            return dgrad(torch.relu(x.to(dt)) * a + c, dt) + b.to(dt).view(1, -1, 1, 1, 1)
        want = ref(torch.float64); own32 = ref(torch.float32)
        K = spec.co * taps
        got = torch.empty((N, spec.ci) + isz, dtype=torch.float32, device=dev)
        xd, wd, bd, scd, shd = x.to(dev), ops.pack_weight(w, spec, 'bwd').to(dev), b.to(dev), sc.to(dev), sh.to(dev)
        ops._call(xd, 'vg_corr3d', ctypes.byref(d), ops._p(xd), ops._p(wd), ops._p(bd), ops._p(scd), ops._p(shd), None, ops._p(got))
    else:
        dy = torch.randn((N, spec.co) + osz, generator=g)
        xm = torch.randn((N, spec.ci) + isz, generator=g)              # the producer's pre-activation: ReLU mask of the data gradient
        keep = (xm > 0) if masked else torch.ones_like(xm, dtype=torch.bool)
        want = dgrad(dy, torch.float64) * keep; own32 = dgrad(dy, torch.float32) * keep
        K = spec.co * taps
        dyd, wd = dy.to(dev), ops.pack_weight(w, spec, 'bwd').to(dev)
        xmd = xm.to(dev) if masked else None
        got = ops.conv_backward_data(dyd, wd, spec, isz, xmd)
        if masked:
            gz = got.cpu()[~keep]
            assert bool((gz == 0).all()) and not bool(torch.signbit(gz).any()), '%s: masked outputs are not exact +0' % case.id
        if 'relu_out_ignored' in o:
            assert masked
            fn, d2 = case_desc(case)
            d2.relu_out = 1
            again = torch.full_like(got, float('nan'))
            ops._call(dyd, fn, ctypes.byref(d2), ops._p(dyd), ops._p(wd), None, None, None, ops._p(xmd), ops._p(again))
            assert torch.equal(again, got), '%s: relu_out changed a masked (data-gradient) launch' % case.id
            assert bool((got < 0).any())
    assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    d32 = float((own32.double() - want).abs().max())
    wmax = float(want.abs().max())
    tol = max(4 * d32, EPS32 * math.sqrt(K) * wmax)
    gotc = got.cpu().double()
    assert bool(torch.isfinite(gotc).all()), '%s: result not finite' % case.id
    err = float((gotc - want).abs().max())
    print('conv_direct %s: %r\n  err %.3g d32 %.3g err/d32 %.2f tol %.3g' % (case.id, plan, err, d32, err / max(d32, 1e-30), tol))
    RECORDS.append((case.id, err, d32, tol))
    assert err <= tol, 'conv_direct %s: max error %.3g > tol %.3g (d32 %.3g)' % (case.id, err, tol, d32)
    if part is not None:
        assert part.numel() == groups * spec.co * plan.stats_chunks * 2, (part.numel(), plan.stats_chunks)
        gamma = torch.ones(spec.co, device=dev); beta = torch.zeros(spec.co, device=dev)
        _, _, mean, rstd = ops.bn_stats(got, gamma, beta, True, per_group, pre=part)
        h = torch.relu(want_pre).reshape(groups, per_group, spec.co, -1)
        mean_w = h.mean((1, 3)).reshape(-1); e2_w = (h * h).mean((1, 3)).reshape(-1)
        var_w = e2_w - mean_w * mean_w
        rstd_w = (var_w + ops.BN_EPS).rsqrt()
        m = 8 + 6
        hmax = float(h.max())
        dmean = tol + m * EPS32 * mean_w
        de2 = 2 * hmax * tol + (m + 1) * EPS32 * e2_w
        dvar = de2 + 2 * mean_w * dmean + dmean * dmean
        assert float((var_w + ops.BN_EPS - dvar).min()) > 0
        drstd = torch.maximum((var_w + ops.BN_EPS - dvar).rsqrt() - rstd_w, rstd_w - (var_w + ops.BN_EPS + dvar).rsqrt())
        em = (mean.cpu().double() - mean_w).abs(); er = (rstd.cpu().double() - rstd_w).abs()
        bm = dmean + EPS32 * mean_w.abs(); br = drstd + EPS32 * rstd_w
        print('  statistics: mean err / bound %.3g, rstd err / bound %.3g' % (float((em / bm).max()), float((er / br).max())))
        assert bool((em <= bm).all()), '%s: mean of relu(y): worst error / bound %.3g' % (case.id, float((em / bm).max()))
        assert bool((er <= br).all()), '%s: rstd of relu(y): worst error / bound %.3g' % (case.id, float((er / br).max()))
    return dict(id=case.id, plan=plan, err=err, d32=d32, tol=tol)


# ---------------------------------------------------------------------------------------------------------------- queries launch nothing
def run_queries_touch_no_memory():
    """The two queries launch nothing: they take a descriptor and no tensor at all (inside, one host-side dummy float stands for every
    pointer the launchers' checks want non-null -- on the host build and on the GPU alike, where reading it from a kernel would
    fault).  Every case's record is consistent with its descriptor, vg_tconv3d_s2_stats_chunks == the record's stats_chunks (one code
    path), and what the launchers refuse comes back with the launchers' status and message."""
    import ctypes
    import pytest
    lib = _lib.get_lib()
    n = len(ops.ConvPlan._fields)
    for case in CASES:
        fn, d = case_desc(case)
        plan = case_plan(case)
        if plan.family == 'tconv' and 'stats' in case.opts:
            assert plan.stats_chunks == lib.size('vg_tconv3d_s2_stats_chunks', ctypes.byref(d), case.per_group), case.id
            assert plan.stats_chunks == case.per_group * plan.grid_x * (plan.threads // 64)
        elif plan.family == 'tconv':
            assert plan.stats_chunks == 0
        assert plan.grid_y == case.groups * case.per_group and plan.grid_z * plan.COT == d.CO
        assert plan.threads % 64 == 0 and plan.BW * plan.BH * plan.BD <= plan.threads <= 256
    rec = (ctypes.c_int32 * n)()
    good = ops.conv_fwd_desc(SPECS['conv5'], 4, (4, 5, 3))[1]
    tgood = ops.conv_fwd_desc(SPECS['convt2'], 4, (4, 5, 4))[1]

    def status(fn, *args):
        return getattr(lib.dll, fn)(*args)
    ARG, UNSUPPORTED = 1, 3                                                                   # VG_ERR_ARG, VG_ERR_UNSUPPORTED (vg_common.h)
    assert status('vg_corr3d_plan', ctypes.byref(good), 0, rec, n) == 0
    assert status('vg_corr3d_plan', ctypes.byref(good), 0, rec, n - 1) == ARG                 # record too short
    assert status('vg_corr3d_plan', ctypes.byref(good), 0, None, n) == ARG
    assert status('vg_corr3d_plan', None, 0, rec, n) == ARG                                   # null descriptor
    assert status('vg_tconv3d_s2_plan', None, 0, 0, rec, n) == ARG
    assert status('vg_tconv3d_s2_plan', ctypes.byref(tgood), 0, 3, rec, n) == ARG             # N = 4 is no multiple of 3
    assert status('vg_tconv3d_s2_plan', ctypes.byref(tgood), 0, -1, rec, n) == ARG
    assert status('vg_tconv3d_s2_plan', ctypes.byref(tgood), 0, 0, rec, n - 1) == ARG
    # what the launchers refuse, with the launchers' status and message (the queries run the launchers' own checks and dispatch)
    for field, value, pro, want, text in (('N', 0, 0, ARG, b'bad shape'), ('stride', 3, 0, ARG, b'bad shape'), ('N', 70000, 0, ARG, b'exceeds grid.y'),
                                          ('OD', 40, 0, ARG, b'inconsistent with input'), ('per_group', 0, 1, ARG, b'per_group inconsistent'),
                                          ('CO', 6, 0, UNSUPPORTED, b'no kernel instance'), ('KD', 7, 0, UNSUPPORTED, b'no kernel instance')):
        bad = ops.conv_fwd_desc(SPECS['conv5'], 4, (4, 5, 3))[1]
        setattr(bad, field, value)
        assert status('vg_corr3d_plan', ctypes.byref(bad), pro, rec, n) == want, (field, value)
        assert lib.dll.vg_last_error().startswith(b'vg_corr3d:') and text in lib.dll.vg_last_error(), lib.dll.vg_last_error()
    for field, value, pro, want, text in (('stride', 1, 0, ARG, b'stride must be 2'), ('ID', 0, 0, ARG, b'bad shape'),
                                          ('per_group', 0, 1, ARG, b'per_group inconsistent'), ('CO', 6, 0, UNSUPPORTED, b'no kernel instance'),
                                          ('KH', 5, 0, UNSUPPORTED, b'no kernel instance')):
        bad = ops.conv_fwd_desc(SPECS['convt2'], 4, (4, 5, 4))[1]
        setattr(bad, field, value)
        assert status('vg_tconv3d_s2_plan', ctypes.byref(bad), pro, 0, rec, n) == want, (field, value)
        assert lib.dll.vg_last_error().startswith(b'vg_tconv3d_s2:') and text in lib.dll.vg_last_error(), lib.dll.vg_last_error()
    with pytest.raises(_lib.VgError):
        ops.conv_plan(ConvSpec('conv', 8, 6, _K3, 1), 'fwd', 2, (5, 5, 5))
    with pytest.raises(ValueError):
        ops.conv_plan(SPECS['conv5'], 'fwd', 2, (5, 5, 5), next_bn=2)


# ---------------------------------------------------------------------------------------------------------------- coverage
BN_LAYERS = ('conv1', 'conv3', 'conv5', 'convt1', 'convt3', 'convt5')    # the layers with a BatchNorm3d on their input (vae_reg_GP.py)
RECTIFIED_IN = ('convt2', 'convt3', 'convt4', 'convt5')                  # their producers store max(y, 0) (VAE.rectified_handoff)
NEXT_BN = ('convt2', 'convt4')                                           # they accumulate the next batch norm's statistics


def _takes_direct(spec, direction, read, write, use_mm):
    """ops._mm_for's decision for a launch with ops.USE_MM = use_mm: True where the register-tiled engine runs it"""
    prev = ops.USE_MM
    ops.USE_MM = use_mm
    try:
        if not use_mm or (direction == 'bwd' and spec.co == 1):
            return True
        return not ops.mm_wins(ops.mm_plan(spec, direction, read, write))
    finally:
        ops.USE_MM = prev


def production_launches():
    """-> [(what, class tuple)]: every forward and data-gradient launch of the three networks (kernel_cases.WGRAD_NETS) at the bench
    sample counts that goes to the direct engine, with ops.USE_MM at its default and with USE_MM = 0, as VAE._encode_pre / decode
    and BnConvAct make them: layers behind a batch norm get the affine prologue and an unmasked data gradient (the batch-norm
    backward masks), the others a masked one; convt2 / convt4 read rectified activations without any prologue and accumulate
    statistics; conv1 forms no data gradient.  convt5's data gradient is listed although the default step recomputes it inside the
    fused batch-norm backward (VG_FUSE_LAST_BN_BWD=0 launches it).  Nothing is launched."""
    import kernel_cases as K
    from vae_gam_amd.schema import net_geometry
    import ctypes
    out = []
    default = ops.USE_MM if ops.USE_MM else 1
    for img, cfgs in K.WGRAD_NETS:
        geo = net_geometry(img)
        for B, Cv in cfgs:
            for use_mm in (default, 0):
                for specs, sizes, N in ((geo.enc, geo.enc_sizes(), B), (geo.dec, geo.dec_sizes(), B * (Cv + 1))):
                    for i, spec in enumerate(specs):
                        isz, osz = sizes[i], sizes[i + 1]
                        has_bn = spec.name in BN_LAYERS
                        relu = spec.name != 'conv1'
                        fwd_relu = relu and not (spec.name in RECTIFIED_IN and not has_bn)
                        nb = B if spec.name in NEXT_BN else None
                        tag = '%s B%d C%d USE_MM=%d %s' % ('x'.join(map(str, img)), B, Cv, use_mm, spec.name)
                        if _takes_direct(spec, 'fwd', isz, None, use_mm):
                            d = ops.conv_fwd_desc(spec, N, isz, fwd_relu, B)[1]
                            plan = ops.conv_plan(spec, 'fwd', N, isz, fwd_relu, has_bn, B, nb)
                            out.append((tag + ' fwd', class_tuple(d, plan, False, bool(nb))))
                        if spec.name != 'conv1' and _takes_direct(spec, 'bwd', osz, isz, use_mm):
                            d = ops.conv_bwd_desc(spec, N, osz, isz)[1]
                            plan = ops.conv_plan(spec, 'bwd', N, isz)
                            out.append((tag + ' bwd', class_tuple(d, plan, not has_bn, False)))
    return out


def check_coverage():
    """the assertions of test_conv_direct_case_matrix_coverage (host build and GPU; launches nothing)"""
    cases, allp = {}, []
    for case in CASES:
        d, plan = check_pins(case)
        cases.setdefault(class_tuple(d, plan, 'mask' in case.opts, 'stats' in case.opts), []).append(case.id)
        allp.append((case, d, plan, props(d, plan)))
    prod = {}
    for what, t in production_launches():
        prod.setdefault(t, []).append(what)
    missing = []
    for t in sorted(prod, key=repr):
        by = cases.get(t, [])
        host = [c for c in by if c not in CONV_DIRECT_GPU_ONLY]
        print('conv_direct %r: %d launches (%s, ...) <- %s%s' % (t, len(prod[t]), prod[t][0], ', '.join(by) or 'NOT COVERED',
                                                                 '' if host or not by else '   (GPU only)'))
        if not by:
            missing.append((t, prod[t][0]))
    assert not missing, 'no listed case runs: %r' % (missing,)
    # what the case list as a whole must contain
    for fam, cot in (('plane', 8), ('tconv', 8)):
        cocs = {pl.COC for c, d, pl, pr in allp if pl.family == fam and pl.COT == cot}
        assert cocs == {cot, 2 * cot, 0}, (fam, cocs)
    plane = [(c, d, pl, pr) for c, d, pl, pr in allp if pl.family == 'plane']
    assert {pl.nbuf for c, d, pl, pr in plane} == {1, 2}
    assert {pr['slabs'] for c, d, pl, pr in plane} == {False, True}
    assert {(pr['slabs'], pl.nbuf) for c, d, pl, pr in plane} == {(False, 1), (False, 2), (True, 1), (True, 2)}
    assert any(pr['ragged'] for c, d, pl, pr in plane) and any(pr['short_d'] for c, d, pl, pr in plane)
    assert any(pr['dst0'] and pl.NOPRO for c, d, pl, pr in plane) and any(pr['dst0'] and pr['slabs'] for c, d, pl, pr in plane)
    tconv = [(c, d, pl, pr) for c, d, pl, pr in allp if pl.family == 'tconv']
    assert any(pr['idle_lanes'] and 'stats' in c.opts for c, d, pl, pr in tconv)
    assert any(pr['short_d'] and 'stats' in c.opts for c, d, pl, pr in tconv)
    assert any(pr['short_w'] for c, d, pl, pr in tconv) and any(pr['short_h'] for c, d, pl, pr in tconv)
    assert any(pr['pad_w1'] for c, d, pl, pr in tconv) and any(pr['odd_ow'] for c, d, pl, pr in tconv)
    assert any(not pr['pad_w1'] and not pr['odd_ow'] for c, d, pl, pr in tconv)
    assert {pl.NOPRO for c, d, pl, pr in tconv} == {0, 1} and {'mask' in c.opts for c, d, pl, pr in tconv} == {False, True}
    direct = [(c, d, pl, pr) for c, d, pl, pr in allp if pl.family == 'direct']
    assert {(pl.COT, pl.S) for c, d, pl, pr in direct} >= {(4, 1), (4, 2), (8, 1)}
    assert any(pl.COT == 4 and pr['short_d'] and pl.BH == 8 for c, d, pl, pr in direct)
    # every kernel family and every plane class runs on the host build too
    host = [(c, d, pl, pr) for c, d, pl, pr in allp if c.id in HOST_CASES]
    assert {pl.family for c, d, pl, pr in host} == {'direct', 'plane', 'tconv'}
    assert {(pr['slabs'], pl.nbuf, chunk_class(d, pl)) for c, d, pl, pr in host if pl.family == 'plane'} >= \
        {(pr['slabs'], pl.nbuf, chunk_class(d, pl)) for c, d, pl, pr in plane if pl.COT == 1 or pl.KD > 3}
    gpu_only_classes = sorted((t for t, by in cases.items() if t in prod and all(c in CONV_DIRECT_GPU_ONLY for c in by)), key=repr)
    return dict(production=prod, cases=cases, gpu_only_classes=gpu_only_classes)
