"""Host build of the HIP kernel sources (tests/emu, g++ -DVG_EMU) against PyTorch references on
tiny shapes: checks tile/halo/index arithmetic and barrier structure without a GPU.  The -m gpu
twin (tests/test_kernels_gpu.py) runs the same bodies on libvaegam_hip.so."""
import os
import subprocess

import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
import kernel_cases as K

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu')


@pytest.fixture(scope='module', autouse=True)
def emu_lib():
    import emu_inject
    prev = emu_inject.inject_emu()
    yield
    emu_inject.restore(prev)


@pytest.mark.parametrize('name,spec,isz', K.LAYERS, ids=[l[0] for l in K.LAYERS])
def test_layer_bn_relu(name, spec, isz):
    K.run_layer_case('cpu', name, spec, isz, with_bn=True, relu_in=(name != 'conv1'), groups=2 if spec.kind == 'convt' else 1)


@pytest.mark.parametrize('name,spec,isz', [K.LAYERS[1], K.LAYERS[3], K.LAYERS[6], K.LAYERS[8]], ids=['conv2', 'conv4', 'convt2', 'convt4'])
def test_layer_relu_only(name, spec, isz):
    K.run_layer_case('cpu', name, spec, isz, with_bn=False, relu_in=True, groups=1, seed=3)


@pytest.mark.parametrize('name,spec,isz', K.WIDE_LAYERS, ids=[l[0] for l in K.WIDE_LAYERS])
def test_layer_wide_rows(name, spec, isz):
    K.run_layer_case('cpu', name, spec, isz, with_bn=name.startswith(('conv1', 'conv3', 'convt3', 'convt5')), relu_in=not name.startswith('conv1'),
                     groups=2 if spec.kind == 'convt' else 1, seed=11)


def test_first_layer_input_is_data():
    name, spec, isz = K.LAYERS[0]
    K.run_layer_case('cpu', name, spec, isz, with_bn=True, relu_in=False, groups=1, input_is_data=True, seed=5)


def test_fused_bn_statistics_and_bias_sum():
    K.run_fused_stats_case('cpu', K.LAYERS[8][1], K.LAYERS[8][2])        # convt4-shaped (5x3x3, stride 2)
    K.run_fused_stats_case('cpu', K.LAYERS[6][1], K.LAYERS[6][2], seed=1)


def test_gam_elbo():
    K.run_gam_case('cpu', C=3, B=3, V=1500)


def test_latent_sample_kl():
    K.run_latent_case('cpu', B=5, L=32, G=4)
    K.run_latent_case('cpu', B=7, L=70, G=2, seed=3, tiny_d=True)


def test_elbo_loss():
    K.run_loss_case('cpu', B=32, C=3)
    K.run_loss_case('cpu', B=300, C=8, seed=1)


def test_linear_act_accumulates_into_grad():
    K.run_linear_case('cpu')


@pytest.mark.parametrize('case', K.FC_GEMM_CASES, ids=lambda c: '%dx%dx%d%s%s' % (c[0], c[1], c[2], '-split' if c[7] else '', '-batch' if c[6] > 1 else ''))
def test_fc_gemm_matches_float64_product(case):
    M, N, Kd, a_kc, b_kc, flags, batch, ksplit = case
    K.run_fc_gemm_case('cpu', M, N, Kd, a_kc, b_kc, flags, batch, ksplit)


def test_gam_elbo_no_covariates():
    K.run_gam_case('cpu', C=0, B=2, V=700, seed=2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_adam(dtype):
    K.run_adam_case('cpu', dtype)


@pytest.mark.parametrize('n', [6, 32, 64])
def test_cholesky(n):
    K.run_cholesky_case('cpu', batch=3, n=n)


@pytest.mark.parametrize('B,n,jitter', [(12, 6, 0.0), (17, 6, 0.0), (7, 12, 1e-5), (130, 6, 0.0)])    # 130: the large-batch path (blocked Cholesky, slab solves)
def test_gain_block_matches_float64_oracle(B, n, jitter):
    K.run_gain_case('cpu', B=B, n=n, jitter=jitter, seed=B)


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
    K.run_conv_mm_plan_case('cpu', kind, force)


@pytest.mark.parametrize('case', K.CONV_MM_CASES, ids=[c[0] for c in K.CONV_MM_CASES])
def test_conv_mm_launch_kinds(case):
    """every launch kind vg_conv_mm carries in the networks, at a pinned row-slab tile and a pinned whole-plane tile, against float64"""
    K.run_conv_mm_listed('cpu', case)


_HOST_LOOP_CASES = [c for c in K.CONV_MM_LOOP_CASES if c[0] not in K.CONV_MM_LOOP_GPU_ONLY]      # the reason stands next to that list


@pytest.mark.parametrize('case', _HOST_LOOP_CASES, ids=[c[0] for c in _HOST_LOOP_CASES])
def test_conv_mm_sample_loop(case):
    """blocks of the persistent grid visit several samples: statistics flushed per group run, the prologue affine changing group
    between units, buffer parity / wait order / mask prefetch repeating"""
    K.run_conv_mm_listed('cpu', case, seed=1)


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


_HOST_WGRAD_CASES = [c for c in K.WGRAD_CASES + K.WGRAD_MID_CASES if c[0] not in K.WGRAD_GPU_ONLY]                   # the reason stands next to that list


@pytest.mark.parametrize('case', _HOST_WGRAD_CASES, ids=[c[0] for c in _HOST_WGRAD_CASES])
def test_wgrad_instances(case):
    """every selectable instance and slot scheme of wgrad_rows_k, one item per block, written and accumulated, against float64"""
    K.run_wgrad_instance_listed('cpu', case)


_HOST_WGRAD_LOOPS = [c for c in K.WGRAD_LOOP_CASES if c[0] in K.WGRAD_LOOP_HOST]                 # the reason stands next to that list


@pytest.mark.parametrize('case', _HOST_WGRAD_LOOPS, ids=[c[0] for c in _HOST_WGRAD_LOOPS])
def test_wgrad_item_loop(case):
    """persistent blocks walk several items: accumulators kept across items, scale / shift reloaded when the group changes, a short
    tile followed by a full one in the same LDS, one slab per block"""
    K.run_wgrad_loop_listed('cpu', case, seed=1)


_HOST_WGRAD_GROUPED = [c for c in K.WGRAD_GROUPED_CASES if c[0] not in K.WGRAD_LOOP_GPU_ONLY]


@pytest.mark.parametrize('case', _HOST_WGRAD_GROUPED, ids=[c[0] for c in _HOST_WGRAD_GROUPED])
def test_wgrad_grouped(case):
    """vg_wgrad3d_grouped: per-group partials and the row of per-tap sums, several items per block, then vg_bn_tconv1_sums"""
    K.run_wgrad_grouped_listed('cpu', case, seed=2)


def test_wgrad_case_matrix_coverage():
    K.check_wgrad_coverage()


@pytest.mark.parametrize('name', list(K.BOUND_LAYERS))
def test_layer_bound_gradients(name):
    """the backward adds straight into bound, prefilled .grad buffers: a stride-1 and a stride-2 conv layer, the padded convt2, convt4
    and the fused last stage (dw through vg_bn_tconv1_sums)"""
    idx, with_bn = K.BOUND_LAYERS[name]
    lname, spec, isz = K.LAYERS[idx]
    K.run_layer_case('cpu', lname, spec, isz, with_bn=with_bn, relu_in=True, groups=2, seed=21 + idx, bound_grads=True)


def test_first_layer_input_is_data_bound_gradients():
    name, spec, isz = K.LAYERS[0]
    K.run_layer_case('cpu', name, spec, isz, with_bn=True, relu_in=False, groups=1, input_is_data=True, seed=5, bound_grads=True)


def test_chain_producer_bias_handoff():
    K.run_chain_case('cpu')


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
    K.run_layer_case('cpu', name, spec, isz, **_layer_args(name, spec))


class _WsQuery(Exception):
    """carries what vg_wgrad3d_ws_bytes answered for the descriptor ops.conv_weight_grad built"""


@pytest.fixture(scope='module')
def wgrad_ws_query(emu_lib):
    """query(spec, isz, N) -> (bytes or -1, vg_last_error()) for the descriptor that ops.conv_weight_grad ITSELF builds for the layer:
    it is called on shape-only tensors through a handle of the host library whose workspace query ends the call (nothing is
    allocated or launched)."""
    import emu_inject

    class QueryOnly(emu_inject.EmuLibrary):
        def size(self, name, *args):
            assert name == 'vg_wgrad3d_ws_bytes'
            raise _WsQuery(getattr(self.dll, name)(*args), self.dll.vg_last_error().decode())

    emu = _lib.get_lib()
    handle = QueryOnly(emu.path)

    def query(spec, isz, N):
        x = torch.empty((N, spec.ci) + tuple(isz), device='meta')
        dy = torch.empty((N, spec.co) + tuple(spec.out_size(isz)), device='meta')
        _lib._LIB = handle
        try:
            with pytest.raises(_WsQuery) as q:
                ops.conv_weight_grad(x, dy, spec, relu_in=True)
        finally:
            _lib._LIB = emu
        return q.value.args
    return query


@pytest.mark.parametrize('img', [(41, 49, 35), (82, 98, 70), (21, 21, 21)], ids=lambda s: '%dx%dx%d' % s)
def test_wgrad_has_an_instance_for_every_layer_of_every_geometry(img, wgrad_ws_query, monkeypatch):
    """every weight-gradient descriptor the three networks produce is inside vg_wgrad3d's supported set (a workspace size comes
    back), and so is the grouped query for the last decoder stage"""
    from vae_gam_amd.schema import net_geometry
    g = net_geometry(img)
    monkeypatch.setattr(ops, '_GROUPED_OK', {})
    for N in (2, 64):
        for spec, isz in list(zip(g.enc, g.enc_sizes())) + list(zip(g.dec, g.dec_sizes())):
            nbytes, err = wgrad_ws_query(spec, isz, N)
            assert nbytes >= 0, (img, spec.name, N, err)
        assert ops._grouped_wgrad_ok((N, g.nf) + tuple(g.dec_sizes()[-2]), N // 2), (img, N)


@pytest.mark.parametrize('spec,isz', [
    (ops.ConvSpec('convt', 8, 8, (3, 3, 3), 1, (1, 1, 1)), (5, 7, 6)),      # stride 1 with padding: no line of the instance table
    (ops.ConvSpec('conv', 1, 8, (3, 3, 3), 1), (4, 5, 131)),                # rows of 129 positions: PW > 128
], ids=['stride1_padded', 'pw129'])
def test_wgrad_outside_the_supported_set_is_refused(spec, isz, wgrad_ws_query):
    nbytes, err = wgrad_ws_query(spec, isz, 2)
    assert nbytes == -1 and err.startswith('vg_wgrad3d'), (nbytes, err)
