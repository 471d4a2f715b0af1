"""HIP kernels (libvaegam_hip.so, through the C ABI) against plain PyTorch fp32 references on
the GPU box: the shrunk per-layer cases of tests/kernel_cases.py plus every layer at the
reference's real 41x49x35 geometry.  The real geometry is not the production launch: at the 2 or 4 samples
these cases use, every 3x3x3 layer falls under the direct engine's `small` switch and runs the 4-channel
instances, not the 8-wide plane-staged / transposed ones a training batch takes.  Those are pinned, class by
class and against float64, by tests/conv_direct_cases.py (test_conv_direct_gpu.py).  Likewise the fully connected
cases here keep the network sizes; the bodies fc_body<W, a_vec, b_vec>, tile sizes and job mixes of vg_fc.hip are
pinned, plan by plan and against float64, in tests/fc_cases.py (test_fc_gpu.py)."""
import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
import kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    import emu_inject; emu_inject.use_product_library()
    lib = _lib.get_lib()                       # raises if libvaegam_hip.so is missing: no fallback
    assert lib.path.endswith('libvaegam_hip.so')
    yield


@pytest.mark.parametrize('name,spec,isz', K.LAYERS, ids=[l[0] for l in K.LAYERS])
def test_layer_bn_relu(name, spec, isz):
    K.run_layer_case('cuda', name, spec, isz, with_bn=True, relu_in=(name != 'conv1'), groups=2 if spec.kind == 'convt' else 1)


@pytest.mark.parametrize('name,spec,isz', [K.LAYERS[1], K.LAYERS[3], K.LAYERS[6], K.LAYERS[8]], ids=['conv2', 'conv4', 'convt2', 'convt4'])
def test_layer_relu_only(name, spec, isz):
    K.run_layer_case('cuda', name, spec, isz, with_bn=False, relu_in=True, groups=1, seed=3)


@pytest.mark.parametrize('name,spec,isz', K.WIDE_LAYERS, ids=[l[0] for l in K.WIDE_LAYERS])
def test_layer_wide_rows(name, spec, isz):
    K.run_layer_case('cuda', name, spec, isz, with_bn=name.startswith(('conv1', 'conv3', 'convt3', 'convt5')), relu_in=not name.startswith('conv1'),
                     groups=2 if spec.kind == 'convt' else 1, seed=11)


def test_first_layer_input_is_data():
    name, spec, isz = K.LAYERS[0]
    K.run_layer_case('cuda', name, spec, isz, with_bn=True, relu_in=False, groups=1, input_is_data=True, seed=5)


# the reference's real layer geometry (vae_reg_GP.py:187-218) -- at N = 2 (encoder) / 4 (decoder) samples, so the
# 3x3x3 layers run the `small` 4-channel instances; the production instances and plan classes: tests/conv_direct_cases.py
FULL = [(41, 49, 35), (39, 47, 33), (19, 23, 16), (17, 21, 14), (8, 10, 6), (6, 8, 5), (8, 10, 7), (16, 21, 14),
        (18, 23, 16), (39, 47, 33)]


@pytest.mark.parametrize('idx', range(10), ids=[l[0] for l in K.LAYERS])
def test_layer_full_geometry(idx):
    name, spec, _ = K.LAYERS[idx]
    K.run_layer_case('cuda', name + '_full', spec, FULL[idx], with_bn=idx in (0, 2, 4, 5, 7, 9), relu_in=(idx != 0),
                     groups=2 if spec.kind == 'convt' else 1, seed=7 + idx, tol=5e-4)


def test_fused_bn_statistics_and_bias_sum():
    K.run_fused_stats_case('cuda', K.LAYERS[8][1], K.LAYERS[8][2])        # convt4-shaped (5x3x3, stride 2)
    K.run_fused_stats_case('cuda', K.LAYERS[6][1], K.LAYERS[6][2], seed=1)
    K.run_fused_stats_case('cuda', K.LAYERS[8][1], (18, 23, 16), groups=2, per_group=4, seed=2)


def test_gam_elbo():
    K.run_gam_case('cuda', C=3, B=3, V=1500)
    K.run_gam_case('cuda', C=8, B=4, V=70315, seed=4)


def test_latent_sample_kl():
    K.run_latent_case('cuda', B=5, L=32, G=4)
    K.run_latent_case('cuda', B=7, L=70, G=2, seed=3, tiny_d=True)
    K.run_latent_case('cuda', B=64, L=32, G=9, seed=5)


def test_elbo_loss():
    K.run_loss_case('cuda', B=32, C=3)
    K.run_loss_case('cuda', B=300, C=8, seed=1)


def test_linear_act_accumulates_into_grad():
    K.run_linear_case('cuda')


@pytest.mark.parametrize('case', K.FC_GEMM_CASES, ids=lambda c: '%dx%dx%d%s%s' % (c[0], c[1], c[2], '-split' if c[7] else '', '-batch' if c[6] > 1 else ''))
def test_fc_gemm_matches_float64_product(case):
    M, N, Kd, a_kc, b_kc, flags, batch, ksplit = case
    K.run_fc_gemm_case('cuda', M, N, Kd, a_kc, b_kc, flags, batch, ksplit)


def test_fc_gemm_at_network_sizes():
    """the products of the 41x49x35 network at batch 64 / 8 covariates: fc1 forward (split-K), fc8 forward, its data gradient (split-K)
    and its weight gradient"""
    K.run_fc_gemm_case('cuda', 64, 200, 3072, True, True, ('A_RELU', 'C_BIAS', 'C_RELU'))
    K.run_fc_gemm_case('cuda', 576, 3840, 200, True, True, ('C_BIAS',))
    K.run_fc_gemm_case('cuda', 576, 200, 3840, True, False, ())
    K.run_fc_gemm_case('cuda', 3840, 200, 576, False, False, ('B_ONES', 'C_ACCUM'))


def test_gam_elbo_no_covariates():
    K.run_gam_case('cuda', C=0, B=2, V=700, seed=2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_adam(dtype):
    K.run_adam_case('cuda', dtype, n=200000)


def test_library_refuses_bad_shapes():
    spec = ops.ConvSpec('conv', 8, 3, (3, 3, 3), 1)                  # CO=3 has no kernel instance
    x = torch.zeros(1, 8, 5, 5, 5, device='cuda'); w = torch.zeros(3, 8, 3, 3, 3, device='cuda')
    with pytest.raises(_lib.VgError):
        ops.conv_forward(x, ops.pack_weight(w, spec, 'fwd'), None, spec)


@pytest.mark.parametrize('n', [6, 32, 64])
def test_cholesky(n):
    K.run_cholesky_case('cuda', batch=3, n=n)


@pytest.mark.parametrize('B,n,jitter', [(12, 6, 0.0), (64, 6, 0.0), (32, 64, 1e-4), (160, 6, 0.0), (256, 6, 0.0)])
def test_gain_block_matches_float64_oracle(B, n, jitter):
    """vg_gp_gain_fwd / _bwd on the MI355X: B = 64 is bench.py's configs[2] batch (B x B matrix in LDS), B = 160 and B = 256 (configs[3]'s global
    minibatch: 8 GPUs x 32) take the workspace path of data-parallel global batches (> 128), n = 64 with jitter is configs[4]'s inducing grid
    (jitter 1e-4: the gradient through Ku^-1 carries cond(Ku)^2 * eps -- at 1e-6, cond ~ 6e7, not even float64 resolves d/d ls)."""
    K.run_gain_case('cuda', B=B, n=n, jitter=jitter, seed=B)


@pytest.mark.parametrize('kind,force', [
    ('convt3_fwd', (8, 2, 11, 8, 0)),      # whole planes (PHB = PH = 11), 8 waves, two channel chunks, single-buffered
    ('convt3_fwd', (8, 2, 4, 16, 1)),      # row slabs of 4 rows (3 slabs), double-buffered
    ('convt3_fwd', (4, 1, 6, 4, 0)),       # 4-wave workgroups, 2 slabs, 4 chunks
    ('convt3_bwd', (8, 1, 9, 8, 0)),       # data gradient, whole planes
    ('convt3_bwd', (4, 2, 3, 4, 1)),       # data gradient, 4 waves, slabs of 3 rows, mask + double buffer
    ('convt4_fwd', (8, 1, 10, 8, 0)),      # 4 parity classes, whole planes, statistics
    ('convt4_fwd', (8, 2, 5, 8, 1)),       # ... row slabs
    ('convt4_fwd', (4, 1, 4, 8, 0)),       # ... 4-wave workgroups
])
def test_conv_mm_pinned_tiles(kind, force):
    K.run_conv_mm_plan_case('cuda', kind, force)


@pytest.mark.parametrize('case', K.CONV_MM_CASES, ids=[c[0] for c in K.CONV_MM_CASES])
def test_conv_mm_launch_kinds(case):
    """every launch kind vg_conv_mm carries in the networks, at a pinned row-slab tile and a pinned whole-plane tile, against float64"""
    K.run_conv_mm_listed('cuda', case)


@pytest.mark.parametrize('case', K.CONV_MM_LOOP_CASES, ids=[c[0] for c in K.CONV_MM_LOOP_CASES])
def test_conv_mm_sample_loop(case):
    """blocks of the persistent grid visit several samples: statistics flushed per group run, the prologue affine changing group
    between units, buffer parity / wait order / mask prefetch repeating"""
    K.run_conv_mm_listed('cuda', case, seed=1)


def test_conv_mm_case_matrix_coverage():
    cov = K.conv_mm_coverage()
    kinds = [('conv2', 'bwd'), ('conv2', 'fwd'), ('conv3', 'fwd'), ('conv3', 'bwd'), ('conv4', 'fwd'), ('conv5', 'fwd'), ('conv5', 'bwd'),
             ('convt1', 'fwd'), ('convt1', 'bwd'), ('convt2p', 'bwd'), ('convt2', 'bwd'), ('convt4', 'bwd'), ('convt4hr', 'fwd'),
             ('convt4hr', 'bwd'), ('convt4toy', 'fwd')]
    for s, d in kinds:
        assert (s, d, 'slab') in cov['kinds'] and (s, d, 'whole') in cov['kinds'], (s, d)
    assert cov['slab_modes'] == {'corr_s1', 'corr_s2', 'class4'}
    assert cov['cc_lt_ci'] > 0 and cov['dbuf'] == {0, 1} and cov['waves'] == {4, 8} and cov['masked'] == {False, True}
    assert cov['tpc'] == {(ks, t) for ks in (7, 9) for t in (3, 4, 5, 6, 8)}
    assert cov['loops'] >= 4 and cov['loops_stats'] >= 2


@pytest.mark.parametrize('case', K.WGRAD_CASES + K.WGRAD_MID_CASES, ids=[c[0] for c in K.WGRAD_CASES + K.WGRAD_MID_CASES])
def test_wgrad_instances(case):
    """every selectable instance and slot scheme of wgrad_rows_k, one item per block, written and accumulated, against float64"""
    K.run_wgrad_instance_listed('cuda', case)


@pytest.mark.parametrize('case', K.WGRAD_LOOP_CASES, ids=[c[0] for c in K.WGRAD_LOOP_CASES])
def test_wgrad_item_loop(case):
    """persistent blocks walk several items: accumulators kept across items, scale / shift reloaded when the group changes, a short
    tile followed by a full one in the same LDS, one slab per block"""
    K.run_wgrad_loop_listed('cuda', case, seed=1)


@pytest.mark.parametrize('case', K.WGRAD_GROUPED_CASES, ids=[c[0] for c in K.WGRAD_GROUPED_CASES])
def test_wgrad_grouped(case):
    """vg_wgrad3d_grouped: per-group partials and the row of per-tap sums, several items per block, then vg_bn_tconv1_sums"""
    K.run_wgrad_grouped_listed('cuda', case, seed=2)


def test_wgrad_case_matrix_coverage():
    K.check_wgrad_coverage()


@pytest.mark.parametrize('name', list(K.BOUND_LAYERS))
def test_layer_bound_gradients(name):
    """the backward adds straight into bound, prefilled .grad buffers: a stride-1 and a stride-2 conv layer, the padded convt2, convt4
    and the fused last stage (dw through vg_bn_tconv1_sums)"""
    idx, with_bn = K.BOUND_LAYERS[name]
    lname, spec, isz = K.LAYERS[idx]
    K.run_layer_case('cuda', lname, spec, isz, with_bn=with_bn, relu_in=True, groups=2, seed=21 + idx, bound_grads=True)


def test_first_layer_input_is_data_bound_gradients():
    name, spec, isz = K.LAYERS[0]
    K.run_layer_case('cuda', name, spec, isz, with_bn=True, relu_in=False, groups=1, input_is_data=True, seed=5, bound_grads=True)


def test_chain_producer_bias_handoff():
    K.run_chain_case('cuda')


def _layer_args(name, spec):
    """the arguments of test_layer_bn_relu / test_layer_wide_rows for this layer"""
    groups = 2 if spec.kind == 'convt' else 1
    if name in [l[0] for l in K.LAYERS]:
        return dict(with_bn=True, relu_in=(name != 'conv1'), groups=groups)
    return dict(with_bn=name.startswith(('conv1', 'conv3', 'convt3', 'convt5')), relu_in=not name.startswith('conv1'), groups=groups, seed=11)


@pytest.mark.parametrize('use_mm', [0, 2], ids=['register_tiled', 'matrix_cores'])
@pytest.mark.parametrize('name,spec,isz', K.LAYERS + K.WIDE_LAYERS, ids=[l[0] for l in K.LAYERS + K.WIDE_LAYERS])
def test_layer_both_engines(name, spec, isz, use_mm, monkeypatch):
    """the shrunk layers with the engine choice forced: 0 = the register-tiled kernels everywhere (what the large multi-channel
    launches run in production), 2 = vg_conv_mm wherever a plan exists (also the plans mm_wins declines)"""
    monkeypatch.setattr(ops, 'USE_MM', use_mm)
    K.run_layer_case('cuda', name, spec, isz, **_layer_args(name, spec))
