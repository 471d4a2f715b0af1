"""Tensor-level operators over the HIP kernels (C ABI: include/vaegam.h).

Every function takes torch tensors that already live where the library can reach them
(HBM for libvaegam_hip.so), passes raw pointers + the current HIP stream, and allocates
outputs/workspace through torch's caching allocator (so the whole train step can be captured
into a hipGraph).  `BnConvAct` and `GamElbo` are the autograd nodes the model is built from;
their backward passes are explicit kernel sequences, not autograd traces.

Storage convention: a layer stores its PRE-activation output; the consumer applies the ReLU
and the batch-norm affine while loading (`relu_in`, `gamma`/`beta`).  This removes every
stand-alone ReLU / batch-norm-apply pass of the reference graph (vae_reg_GP.py:238-264).
Where every consumer of an activation rectifies it anyway (the decoder), the producer may store
max(y, 0) instead and the consumer is told so (`BnConvAct`: relu_out / rectified_in): the same bits
downstream, and a consumer without a batch norm then runs without any prologue.
"""
import ctypes
from collections import namedtuple
from dataclasses import dataclass
from typing import Tuple

import torch

from . import _lib
from ._lib import ConvDesc, WgradDesc
from .conv_mm_plan import MmPlan, mm_plan     # the vg_conv_mm planner; what uses its plans (USE_MM, mm_wins, conv_mm) is below

BN_EPS = 1e-5            # nn.BatchNorm3d default (vae_reg_GP.py:194-196)

# Optional per-launch timing with HIP events recorded on the stream the kernels are launched on
# (bench.py's roofline leg).  PROFILE maps "<entry point>:<layer>" -> list of (start, end) events.
PROFILE = None
_LABEL = ['']


class label:
    """with ops.label('convt5'): ... tags the launches inside (profiling only)."""
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = _LABEL[0]; _LABEL[0] = self.name

    def __exit__(self, *a):
        _LABEL[0] = self.prev


def _call(t, fn, *args):
    """Launch one C-ABI entry point on t's current stream (optionally bracketed by HIP events)."""
    lib = _lib.get_lib()
    if not t.is_cuda and not lib.host_pointers_ok:
        raise RuntimeError('refusing to launch %s on a non-GPU tensor: the HIP kernels need device pointers (no CPU path)' % fn)
    if PROFILE is not None and t.is_cuda:
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.call(fn, *args, _stream(t))
        e1.record()
        PROFILE.setdefault('%s:%s' % (fn, _LABEL[0]), []).append((e0, e1))
    else:
        lib.call(fn, *args, _stream(t))


# Parameter-gradient kernels (weight gradient, bias sum) of a layer depend on dy but nothing downstream depends
# on them until the optimiser: they run on a second HIP stream beside the data-gradient chain (which is what the
# next layer's backward waits for).  Round 1 measured a LOSS (7.75 vs 7.29 ms/step at batch 32: the persistent
# weight-gradient blocks of that time held the LDS of every CU, so the chains did not overlap and the extra joins only
# added boundaries).  With round 2's kernels (2-3 weight-gradient blocks per CU at 56 KB, matrix-core data gradients)
# the two chains do overlap: 8.10 -> 7.85 ms/step at batch 64 / 8 covariates, 3.20 -> 3.03 at batch 32 / 3.  On.
import os as _os
SIDE_STREAM = bool(int(_os.environ.get('VG_SIDE_STREAM', '1')))
# (The fully connected dW/db on the second stream measured 4.41 vs 4.28 ms/step, worse: they stay on the main stream.)
_SIDE = {}


def _side_stream(device):
    key = (device.type, device.index)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


class on_side_stream:
    """with on_side_stream(ref, tensors...): launches inside go to the side stream, after everything already
    queued on the current stream; `tensors` are marked as used there (allocator safety)."""
    def __init__(self, ref, *tensors, enabled=None):
        self.active = bool((SIDE_STREAM if enabled is None else enabled) and ref.is_cuda)
        self.ref, self.tensors = ref, tensors

    def __enter__(self):
        if not self.active:
            return self
        self.side = _side_stream(self.ref.device)
        self.side.wait_stream(torch.cuda.current_stream(self.ref.device))
        _queue_join(self.ref.device)                     # the stream that ran backward() waits for the side work at its end
        for t in self.tensors:
            if t is not None:
                t.record_stream(self.side)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *a):
        if self.active:
            self.ctx.__exit__(*a)


_JOIN_QUEUED = set()


def _queue_join(device):
    key = (device.type, device.index)
    if key in _JOIN_QUEUED:
        return
    _JOIN_QUEUED.add(key)

    def _cb():
        _JOIN_QUEUED.discard(key)
        join_side_stream(device)
    try:
        torch.autograd.Variable._execution_engine.queue_callback(_cb)     # runs when this backward pass has finished
    except RuntimeError:                                                  # not inside a backward pass
        _JOIN_QUEUED.discard(key)


def join_side_stream(device):
    """The current stream waits for the parameter-gradient kernels queued on the side stream."""
    key = (device.type, device.index)
    if key in _SIDE:
        torch.cuda.current_stream(device).wait_stream(_SIDE[key])


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    if t.is_cuda:
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return None


def _chk(t, dtype=torch.float32):
    assert t.is_contiguous(), 'tensor must be contiguous'
    assert t.dtype == dtype, 'expected %s, got %s' % (dtype, t.dtype)
    return t


def _out_or_new(out, shape, like):
    """The `out=` convention of the parameter-gradient launches -> (tensor the launch writes, its accumulate flag): `out` (a
    parameter's .grad, a view of the flat gradient buffer) is added into; without one a fresh fp32 tensor is written."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device), 0
    assert out.shape == shape and out.is_contiguous() and out.dtype == torch.float32
    return out, 1


# --------------------------------------------------------------------------- layer geometry
@dataclass(frozen=True)
class ConvSpec:
    """One nn.Conv3d / nn.ConvTranspose3d of vae_reg_GP.py:189-215."""
    kind: str                      # 'conv' | 'convt'
    ci: int
    co: int
    k: Tuple[int, int, int]
    stride: int
    pad: Tuple[int, int, int] = (0, 0, 0)
    outpad: Tuple[int, int, int] = (0, 0, 0)
    name: str = ''

    def out_size(self, i):
        if self.kind == 'conv':
            return tuple((i[a] + 2 * self.pad[a] - self.k[a]) // self.stride + 1 for a in range(3))
        return tuple((i[a] - 1) * self.stride - 2 * self.pad[a] + self.k[a] + self.outpad[a] for a in range(3))


def pack_weight(w: torch.Tensor, spec: ConvSpec, direction: str) -> torch.Tensor:
    """Repack a layer weight into the [ci_launch][tap][co_launch] order the kernels read through
    the scalar path.  direction: 'fwd' (layer forward) or 'bwd' (data gradient)."""
    fwd = direction == 'fwd'
    if (spec.kind == 'conv') == fwd:
        # conv forward / convT data-gradient: strided correlation with the weight as stored
        # conv w[co][ci][k] -> [ci][k][co];   convT w[ci][co][k] (launch ci=co_l, co=ci_l) -> [co_l][k][ci_l]
        return w.permute(1, 2, 3, 4, 0).contiguous()
    # convT forward / conv data-gradient: transposed form.  stride 1 runs as a correlation with the
    # kernel flipped; stride 2 runs in gather form with the kernel as stored.
    if spec.stride == 1:
        w = w.flip(2, 3, 4)
    return w.permute(0, 2, 3, 4, 1).contiguous()


def pack_mode(spec: ConvSpec, direction: str) -> int:
    """vg_pack_weights mode producing the same image as pack_weight(w, spec, direction)."""
    if (spec.kind == 'conv') == (direction == 'fwd'):
        return 0
    return 2 if spec.stride == 1 else 1


class PackedWeights:
    """All packed conv-weight images of a model in one buffer, refreshed by ONE launch per step."""

    def __init__(self, layers, flat, offsets, sizes=None):
        """layers: [(name, spec, weight Parameter)], flat: the flat fp32 parameter buffer, offsets: {name: element offset},
        sizes: {name: (input spatial size, output spatial size)} -- with it the matrix-core plans (mm_plan) of every layer are
        built too and their A images are gathered from the flat buffer by one more launch per step."""
        self.mm = {}                                  # (name, direction) -> (MmPlan, A-image view)
        self._mm_idx = None
        if sizes is not None and USE_MM:
            import numpy as np
            idx_all, spans, pos = [], {}, 0
            for name, spec, w in layers:
                isz, osz = sizes[name]
                for direction in ('fwd', 'bwd'):
                    if direction == 'bwd' and name == 'conv1':
                        continue
                    plan = mm_plan(spec, 'fwd', isz) if direction == 'fwd' else mm_plan(spec, 'bwd', osz, isz)
                    if plan is None:
                        continue
                    gi = np.where(plan.aidx >= 0, plan.aidx + offsets[name], -1).astype(np.int32)
                    idx_all.append(gi); spans[(name, direction)] = (plan, pos, gi.size); pos += gi.size
            if idx_all:
                self._mm_idx = torch.from_numpy(np.concatenate(idx_all)).to(flat.device)
                self._mm_buf = torch.zeros(pos, dtype=torch.float32, device=flat.device)
                self.mm = {k: (plan, self._mm_buf[o:o + n]) for k, (plan, o, n) in spans.items()}
        segs, views, dst = [], {}, 0
        for name, spec, w in layers:
            for direction in ('fwd', 'bwd'):
                d0, d1 = w.shape[0], w.shape[1]
                kvol = w[0, 0].numel()
                n = w.numel()
                segs.append([offsets[name], dst, d0, d1, kvol, pack_mode(spec, direction), n, 0])
                views[(name, direction)] = (dst, n, pack_weight(w.detach(), spec, direction).shape)
                dst += ((n + 3) // 4) * 4
        self.total = dst
        self.flat = flat
        self.buf = torch.empty(dst, dtype=torch.float32, device=flat.device)
        self.segs = torch.tensor(segs, dtype=torch.int64).to(flat.device)
        self.nseg = len(segs)
        self._views = {k: self.buf[o:o + n].view(shape) for k, (o, n, shape) in views.items()}
        # the kernel walks every destination element, including the alignment gaps: give the last segment the tail
        self.elems = dst

    def refresh(self):
        _call(self.flat, 'vg_pack_weights', _p(self.flat), _p(self.buf), _p(self.segs), self.nseg, self.elems)
        if self._mm_idx is not None:
            _call(self.flat, 'vg_gather_f32', _p(self.flat), _p(self._mm_idx), _p(self._mm_buf), self._mm_idx.numel())

    def get_mm(self, name, direction):
        return self.mm.get((name, direction))

    def get(self, name, direction):
        return self._views[(name, direction)]


def _conv_desc(N, ci, co, isz, osz, k, stride, pad, relu_in, per_group, relu_out=False):
    return ConvDesc(N, ci, co, isz[0], isz[1], isz[2], osz[0], osz[1], osz[2], k[0], k[1], k[2], stride,
                    pad[0], pad[1], pad[2], int(relu_in), int(per_group), int(bool(relu_out)))


def conv_fwd_desc(spec: ConvSpec, N, isz, relu_in=False, per_group=1, relu_out=False):
    """-> (entry point, vg_conv_desc, output size) of a layer's forward launch on the register-tiled engine (vg_conv.hip): a Conv3d
    and a stride-1 ConvTranspose3d are correlations (the latter padded by k - 1 - pad), a stride-2 ConvTranspose3d runs in gather form."""
    isz = tuple(int(v) for v in isz); osz = spec.out_size(isz)
    if spec.kind == 'conv':
        assert spec.pad == (0, 0, 0)
        return 'vg_corr3d', _conv_desc(N, spec.ci, spec.co, isz, osz, spec.k, spec.stride, (0, 0, 0), relu_in, per_group, relu_out), osz
    if spec.stride == 1:
        padc = tuple(spec.k[a] - 1 - spec.pad[a] for a in range(3))
        return 'vg_corr3d', _conv_desc(N, spec.ci, spec.co, isz, osz, spec.k, 1, padc, relu_in, per_group, relu_out), osz
    return 'vg_tconv3d_s2', _conv_desc(N, spec.ci, spec.co, isz, osz, spec.k, 2, spec.pad, relu_in, per_group, relu_out), osz


def conv_bwd_desc(spec: ConvSpec, N, osz, isz):
    """-> (entry point, vg_conv_desc) of a layer's data-gradient launch: reads dy (the layer's output size osz), writes dx (isz)."""
    osz = tuple(int(v) for v in osz); isz = tuple(int(v) for v in isz)
    if spec.kind == 'convt':
        # dx[i] = sum_k dy[i*s - pad + k] w[k]: strided correlation over dy
        return 'vg_corr3d', _conv_desc(N, spec.co, spec.ci, osz, isz, spec.k, spec.stride, spec.pad, False, 1)
    if spec.stride == 1:
        padc = tuple(spec.k[a] - 1 for a in range(3))
        return 'vg_corr3d', _conv_desc(N, spec.co, spec.ci, osz, isz, spec.k, 1, padc, False, 1)
    return 'vg_tconv3d_s2', _conv_desc(N, spec.co, spec.ci, osz, isz, spec.k, 2, (0, 0, 0), False, 1)


ConvPlan = namedtuple('ConvPlan', _lib.CONV_PLAN_FIELDS)


def conv_plan(spec: ConvSpec, direction: str, N, isz, relu_in=False, has_prologue=False, per_group=1, next_bn=None) -> ConvPlan:
    """What conv_forward (direction 'fwd') / conv_backward_data ('bwd') would launch on the register-tiled engine for a layer with
    input size isz and N samples, from the launchers' own planners (vg_corr3d_plan / vg_tconv3d_s2_plan): nothing is launched,
    shapes only.  has_prologue: the forward is given scale / shift; next_bn as conv_forward.  `family` is 'direct', 'plane' or 'tconv'."""
    isz = tuple(int(v) for v in isz)
    if direction == 'fwd':
        fn, d, _ = conv_fwd_desc(spec, int(N), isz, relu_in, per_group)
    else:
        assert direction == 'bwd' and not has_prologue and not next_bn
        fn, d = conv_bwd_desc(spec, int(N), spec.out_size(isz), isz)
    rec = (ctypes.c_int32 * len(ConvPlan._fields))()
    if fn == 'vg_corr3d':
        if next_bn:
            raise ValueError('next_bn: only the stride-2 transposed-conv kernel accumulates the next layer\'s statistics')
        _lib.get_lib().call('vg_corr3d_plan', ctypes.byref(d), int(bool(has_prologue)), rec, len(rec))
    else:
        _lib.get_lib().call('vg_tconv3d_s2_plan', ctypes.byref(d), int(bool(has_prologue)), int(next_bn or 0), rec, len(rec))
    return ConvPlan(_lib.CONV_FAMILIES[rec[0]], *rec[1:])


def conv_forward(x, wpk, bias, spec: ConvSpec, relu_in=False, scale=None, shift=None, per_group=1, next_bn=None, relu_out=False):
    """Layer forward: y = conv/convT(P(x)) + bias, y is the pre-activation -- or, with relu_out, max(y, 0) (the rectified hand-off
    of BnConvAct; the statistics partials of next_bn are the same either way).
    next_bn = per_group of the BatchNorm3d that consumes relu(y): the stride-2 transposed-conv kernel then also accumulates
    the statistics partials for it (no separate pass over y) and the call returns (y, partials) -- the caller hands the
    partials to the consuming layer's bn_stats(pre=...) explicitly."""
    lib = _lib.get_lib()
    N = x.shape[0]
    fn, d, osz = conv_fwd_desc(spec, N, tuple(x.shape[2:]), relu_in, per_group, relu_out)
    y = torch.empty((N, spec.co) + osz, dtype=torch.float32, device=x.device)
    _chk(x); _chk(wpk)
    if fn == 'vg_tconv3d_s2' and next_bn:
        chunks = lib.size('vg_tconv3d_s2_stats_chunks', ctypes.byref(d), int(next_bn))
        G = N // int(next_bn)
        part = torch.empty(G * spec.co * chunks * 2, dtype=torch.float64, device=x.device)
        _call(x, 'vg_tconv3d_s2_stats', ctypes.byref(d), _p(x), _p(wpk), _p(bias), _p(scale), _p(shift), _p(y), int(next_bn), 1,
                 _p(part))
        return y, part
    _call(x, fn, ctypes.byref(d), _p(x), _p(wpk), _p(bias), _p(scale), _p(shift), None, _p(y))
    if next_bn:
        raise ValueError('next_bn: only the stride-2 transposed-conv kernel accumulates the next layer\'s statistics')
    return y


def conv_backward_data(dy, wpk_bwd, spec: ConvSpec, in_size, mask_src=None):
    """Gradient w.r.t. the layer's (post-prologue) input; `mask_src` fuses the producer's ReLU backward."""
    N = dy.shape[0]
    isz = tuple(in_size)
    fn, d = conv_bwd_desc(spec, N, tuple(dy.shape[2:]), isz)
    dx = torch.empty((N, spec.ci) + isz, dtype=torch.float32, device=dy.device)
    _chk(dy); _chk(wpk_bwd)
    _call(dy, fn, ctypes.byref(d), _p(dy), _p(wpk_bwd), None, None, None, _p(mask_src), _p(dx))
    return dx


def wgrad_desc(spec: ConvSpec, x_shape, dy_shape, relu_in=False, per_group=1):
    """The vg_wgrad_desc of a layer's weight gradient (x: the layer's input, dy: the gradient of its output)
    -> (descriptor, window tensor is x, shape of dw).  Conv3d: positions = dy, windows = x (prologue on the windows);
    ConvTranspose3d: positions = x (prologue on the positions), windows = dy."""
    N = int(x_shape[0])
    isz = tuple(int(v) for v in x_shape[2:]); osz = tuple(int(v) for v in dy_shape[2:])
    if spec.kind == 'conv':
        d = WgradDesc(N, spec.co, spec.ci, *osz, *isz, *spec.k, spec.stride, 0, 0, 0, 1, int(relu_in), int(per_group))
        return d, True, (spec.co, spec.ci) + tuple(spec.k)
    d = WgradDesc(N, spec.ci, spec.co, *isz, *osz, *spec.k, spec.stride, *spec.pad, 0, int(relu_in), int(per_group))
    return d, False, (spec.ci, spec.co) + tuple(spec.k)


WgradPlan = namedtuple('WgradPlan', _lib.WGRAD_PLAN_FIELDS)


def wgrad_plan(spec: ConvSpec, x_shape, dy_shape, relu_in=False, per_group=1, grouped=False) -> WgradPlan:
    """What vg_wgrad3d (grouped: vg_wgrad3d_grouped) would launch for this layer's weight gradient, from the library's own
    planner (vg_wgrad3d_plan): nothing is launched, shapes only."""
    d, _, _ = wgrad_desc(spec, x_shape, dy_shape, relu_in, per_group)
    rec = (ctypes.c_int32 * len(WgradPlan._fields))()
    _lib.get_lib().call('vg_wgrad3d_plan', ctypes.byref(d), int(bool(grouped)), rec, len(rec))
    return WgradPlan(*rec)


def conv_weight_grad(x, dy, spec: ConvSpec, relu_in=False, scale=None, shift=None, per_group=1, out=None):
    """dL/dW in the layer's own weight layout; the prologue of the forward is re-applied to x on load."""
    lib = _lib.get_lib()
    _chk(x); _chk(dy)
    d, a_is_x, shape = wgrad_desc(spec, x.shape, dy.shape, relu_in, per_group)
    a, b = (x, dy) if a_is_x else (dy, x)
    nbytes = lib.size('vg_wgrad3d_ws_bytes', ctypes.byref(d))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x.device)
    dw, acc = _out_or_new(out, shape, x)
    _call(x, 'vg_wgrad3d', ctypes.byref(d), _p(a), _p(b), _p(scale), _p(shift), _p(ws), _p(dw), acc)
    return None if acc else dw


# --------------------------------------------------------------------------- batch norm pieces
def _bn_ws(x, N, C, P, per_group):
    nbytes = _lib.get_lib().size('vg_bn_ws_bytes', N, C, P, per_group)
    return torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)


def bn_plan(N, C, P, per_group):
    """(cp, ns) of the batch-norm streaming launches for x [N][C][P] in groups of per_group samples (channel_sum: per_group = N),
    from the library's own planner (vg_bn_plan): cp position chunks per sample, ns sample splits; nothing is launched."""
    rec = (ctypes.c_int32 * 2)()
    _lib.get_lib().call('vg_bn_plan', int(N), int(C), int(P), int(per_group), rec)
    return int(rec[0]), int(rec[1])


def bn_stats(x, gamma, beta, relu, per_group, sync=None, pre=None):
    """Batch statistics of relu?(x) per (group, channel) -> (scale, shift, mean, rstd), each [G*C].
    `sync(t)` (optional) all-reduces the raw [sum, sumsq, count] triples across data-parallel ranks.
    `pre`: the partials of relu(x) with THIS per_group that the kernel which wrote x accumulated
    (conv_forward(..., next_bn=per_group)); x is then not read at all."""
    N, C = x.shape[0], x.shape[1]
    P = x[0, 0].numel()
    G = N // per_group
    out = torch.empty((4, G * C), dtype=torch.float32, device=x.device)
    outs = (_p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]))
    # the producer launch writes the outputs itself -- or, data parallel, only the raw sums, which are all-reduced and then finalised
    wr = outs if sync is None else (None,) * 4
    if pre is not None:
        assert relu, 'producer-side partials are statistics of relu(x)'
        assert pre.dtype == torch.float64 and pre.device == x.device and pre.numel() % (G * C * 2) == 0
        chunks = pre.numel() // (G * C * 2)
        sums = torch.empty((G * C, 3), dtype=torch.float64, device=x.device)       # without sync: the launch's workspace
        _call(x, 'vg_bn_stats_from_parts', _p(pre), G, C, chunks, float(per_group * P), _p(gamma), _p(beta), BN_EPS,
              *((None, _p(sums)) if sync is None else (_p(sums), None)), *wr)
    else:
        ws = _bn_ws(x, N, C, P, per_group)
        sums = None if sync is None else torch.empty((G * C, 3), dtype=torch.float64, device=x.device)
        _call(x, 'vg_bn_stats', _p(_chk(x)), N, C, P, per_group, int(relu), _p(gamma), _p(beta), BN_EPS, _p(ws), _p(sums), *wr)
    if sync is not None:
        sums = sync(sums)
        _call(x, 'vg_bn_finalize', _p(sums), G, C, _p(gamma), _p(beta), BN_EPS, *outs)
    return out[0], out[1], out[2], out[3]


def _grad_buf(t):
    """The parameter's contiguous fp32 .grad (a view of the flat gradient buffer) if it exists, else None."""
    if isinstance(t, torch.nn.Parameter) and t.grad is not None and t.grad.is_contiguous() and t.grad.dtype == torch.float32:
        return t.grad
    return None


def bn_backward_(dxe, p, gamma, mean, rstd, relu, per_group, sync=None, beta=None, producer_bias_grad=None):
    """In place: dxe (grad w.r.t. the normalised tensor) -> grad w.r.t. the stored pre-activation p.
    Returns (dgamma[C], dbeta[C]) summed over groups -- or (None, None) after adding them straight into
    gamma.grad / beta.grad when both exist (one launch instead of autograd's two sums + two adds).
    producer_bias_grad [C] (optional): += the per-channel sum of the result, i.e. the bias gradient of the layer that
    produced p, from the values the apply pass already holds (that layer then skips its own channel-sum pass)."""
    N, C = p.shape[0], p.shape[1]
    P = p[0, 0].numel()
    G = N // per_group
    ws = _bn_ws(p, N, C, P, per_group)
    sums = torch.empty((G * C, 2), dtype=torch.float64, device=p.device)
    _call(p, 'vg_bn_bwd_reduce', _p(_chk(dxe)), _p(_chk(p)), N, C, P, per_group, int(relu), _p(mean), _p(rstd), _p(ws),
             _p(sums))

    def apply(sums, count):
        parts = torch.empty((2, G, C), dtype=torch.float32, device=p.device)
        _call(p, 'vg_bn_bwd_apply', _p(dxe), _p(p), N, C, P, per_group, int(relu), _p(gamma), _p(mean), _p(rstd), _p(sums),
                 count, _p(parts[0]), _p(parts[1]), _p(ws), _p(producer_bias_grad), 1)
    return _bn_backward_tail(p, sums, per_group, sync, gamma, beta, producer_bias_grad, apply)


def _bn_backward_tail(p, sums, per_group, sync, gamma, beta, producer_bias_grad, apply):
    """What bn_backward_ and bn_backward_tconv1 do with the sums of their reduce launch: all-reduce them (data parallel), run the
    caller's apply(sums, count) launch, then vg_bn_param_grad -> (dgamma, dbeta) with the conventions of bn_backward_."""
    N, C = p.shape[0], p.shape[1]
    G = N // per_group
    count = float(per_group * p[0, 0].numel())
    local = sums
    if sync is not None:
        local = sums.clone()                       # this rank's share of dgamma / dbeta (the gradient all-reduce sums them)
        sums = sync(sums)
        count = count * sync.world_size
    if producer_bias_grad is not None:
        assert producer_bias_grad.shape == (C,) and producer_bias_grad.is_contiguous() and producer_bias_grad.dtype == torch.float32
    apply(sums, count)
    gg, bg = _grad_buf(gamma), _grad_buf(beta)
    if gg is None or bg is None:                   # straight into the .grad views only when both exist
        gg = bg = None
    dg, acc = _out_or_new(gg, (C,), p)
    db, _ = _out_or_new(bg, (C,), p)
    _call(p, 'vg_bn_param_grad', _p(local), G, C, _p(dg), _p(db), acc)
    return (None, None) if acc else (dg, db)


_GROUPED_OK = {}


def _last_stage(C):
    """the decoder's last stage: C -> 1 channels, 3x3x3 stride-1 transposed conv"""
    return ConvSpec('convt', C, 1, (3, 3, 3), 1)


def wgrad_grouped(dy, p, in_scale, in_shift, relu, per_group):
    """vg_wgrad3d_grouped for the last decoder stage: dy [N][1][D+2][H+2][W+2], p [N][C][D][H][W] -> q [G][C+1][27]: per batch-norm
    group the weight gradient against relu?(p) * in_scale + in_shift (rows c < C) and the per-tap sums of dy (row C)."""
    lib = _lib.get_lib()
    N, C = p.shape[0], p.shape[1]
    _chk(dy); _chk(p)
    d, _, _ = wgrad_desc(_last_stage(C), p.shape, dy.shape, relu, per_group)
    nbytes = lib.size('vg_wgrad3d_grouped_ws_bytes', ctypes.byref(d))
    wws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=p.device)
    q = torch.empty((N // per_group, C + 1, 27), dtype=torch.float32, device=p.device)
    _call(p, 'vg_wgrad3d_grouped', ctypes.byref(d), _p(dy), _p(p), _p(_chk(in_scale)), _p(_chk(in_shift)), _p(wws), _p(q))
    return q


def bn_tconv1_sums(q, w, gamma, beta, dw, accumulate):
    """vg_bn_tconv1_sums: q [G][C+1][27] of wgrad_grouped (taken against the normalised activation) -> sums double[G*C][2] =
    {sum dxe, sum dxe * hhat}; dw [C][1][3][3][3] (the conv's weight gradient) written, or added to when `accumulate`."""
    G, C1, K = q.shape
    sums = torch.empty((G * (C1 - 1), 2), dtype=torch.float64, device=q.device)
    _call(q, 'vg_bn_tconv1_sums', _p(_chk(q)), _p(_chk(w)), _p(gamma), _p(beta), G, C1 - 1, K, _p(sums), _p(dw), int(bool(accumulate)))
    return sums


def _grouped_wgrad_ok(p_shape, per_group):
    """Whether vg_wgrad3d_grouped has an instance for the last decoder stage at this geometry (asked once per shape)."""
    key = (tuple(p_shape), int(per_group))
    if key not in _GROUPED_OK:
        N, C, ID, IH, IW = key[0]
        d, _, _ = wgrad_desc(_last_stage(C), key[0], (N, 1, ID + 2, IH + 2, IW + 2), False, per_group)
        _GROUPED_OK[key] = _lib.get_lib().dll.vg_wgrad3d_grouped_ws_bytes(ctypes.byref(d)) >= 0
    return _GROUPED_OK[key]


def bn_backward_tconv1(dy, weight, p, gamma, mean, rstd, relu, per_group, sync=None, beta=None, producer_bias_grad=None, dw_out=None):
    """Batch-norm backward fused with the data gradient of the ONE-output-channel 3x3x3 stride-1 transposed conv behind it
    (the decoder's last stage): dy [N][1][D+2][H+2][W+2], weight [C][1][3][3][3], p [N][C][D][H][W] -> dp (new tensor).
    The C-channel gradient w.r.t. the normalised tensor is recomputed from dy and never stored.
    `dw_out` (the conv weight's gradient buffer, accumulated into) selects the one-pass form: the conv's weight gradient is taken per
    batch-norm group against the NORMALISED activation (vg_wgrad3d_grouped) and both the batch-norm reductions and dW follow from it
    algebraically (vg_bn_tconv1_sums) -- the reduce pass over p and dy (0.35 ms at batch 64 / 8 covariates) disappears; the caller
    must then NOT run the layer's ordinary weight gradient.  Returns (dp, dgamma, dbeta) with the conventions of bn_backward_."""
    lib = _lib.get_lib()
    N, C = p.shape[0], p.shape[1]
    ID, IH, IW = p.shape[2:]
    assert tuple(dy.shape) == (N, 1, ID + 2, IH + 2, IW + 2) and tuple(weight.shape) == (C, 1, 3, 3, 3)
    _chk(dy); _chk(p)
    w = _chk(weight.detach().contiguous())
    G = N // per_group
    ws = torch.empty(lib.size('vg_bn_tconv1_ws_bytes', N, C, ID, per_group) // 8, dtype=torch.float64, device=p.device)
    if dw_out is not None:
        assert dw_out.shape == weight.shape and dw_out.is_contiguous() and dw_out.dtype == torch.float32 and beta is not None
        q = wgrad_grouped(dy, p, rstd, -(mean * rstd), relu, per_group)
        sums = bn_tconv1_sums(q, w, gamma, beta, dw_out, True)
    else:
        sums = torch.empty((G * C, 2), dtype=torch.float64, device=p.device)
        _call(p, 'vg_bn_bwd_reduce_tconv1', _p(dy), _p(w), _p(p), N, C, ID, IH, IW, per_group, int(relu), _p(mean), _p(rstd), _p(ws), _p(sums))
    dp = torch.empty_like(p)

    def apply(sums, count):
        _call(p, 'vg_bn_bwd_apply_tconv1', _p(dy), _p(w), _p(p), _p(dp), N, C, ID, IH, IW, per_group, int(relu), _p(gamma), _p(mean), _p(rstd),
              _p(sums), count, _p(ws), _p(producer_bias_grad), 1)
    return (dp,) + _bn_backward_tail(p, sums, per_group, sync, gamma, beta, producer_bias_grad, apply)


def channel_sum(x, out=None):
    """Per-channel sum of x [N][C][...] -> [C]; added into `out` (a bias .grad) when given, and None is returned."""
    N, C = x.shape[0], x.shape[1]
    P = x[0, 0].numel()
    ws = _bn_ws(x, N, C, P, N)
    s, acc = _out_or_new(out, (C,), x)
    _call(x, 'vg_channel_sum', _p(_chk(x)), N, C, P, _p(ws), _p(s), acc)
    return None if acc else s


# --------------------------------------------------------------------------- autograd nodes
class BnConvAct(torch.autograd.Function):
    """y = conv( BN( relu?(p_in) ) ) + bias, stored pre-activation -- or rectified, where the layers agree on it (below).

    forward  : [bn_stats] -> corr3d / tconv3d_s2 with the ReLU + affine applied while staging tiles
    backward : channel_sum (bias), wgrad3d, data gradient (+ fused ReLU mask), [bn backward]
    `input_is_data=True` (first encoder layer): no data gradient is formed; the batch-norm
    parameter gradients follow from the weight gradient (valid conv, every tap hits the input).

    Two explicit hand-offs between neighbouring layers (arguments, no state outside the nodes):
      forward   `next_bn`   : this (stride-2 transposed-conv) layer also accumulates the statistics partials of the
                              BatchNorm3d that consumes its output; returned as a second output, which the caller passes
                              to that layer as `pre_stats`;
      backward  `producer_bias` : Parameter (bias of the layer that produced p_in).  This layer's batch-norm backward adds
                              the per-channel sum of the gradient it hands back straight into producer_bias.grad, and the
                              producing layer is built with `bias_grad_by_consumer=True` so that it skips its own pass.
      forward   `relu_out`  : this layer stores max(y, 0) instead of y.  Legal exactly where EVERY consumer of y rectifies it or only tests
                              its sign (the next layer's forward, weight gradient, ReLU mask, batch-norm statistics and backward all do):
                              relu(relu(y)) == relu(y) and relu(y) > 0 <=> y > 0, so no bit downstream changes.  The consuming layer
                              is built with `rectified_in=True`: `relu_in` keeps its mathematical meaning (the backward still masks
                              by p_in > 0), only the forward LAUNCH is told that the max is already done -- without a batch norm it
                              then has no prologue at all.
    """

    @staticmethod
    def forward(ctx, p_in, weight, bias, gamma, beta, spec: ConvSpec, relu_in: bool, per_group: int,
                input_is_data: bool, sync, packed=None, next_bn=None, pre_stats=None, producer_bias=None,
                bias_grad_by_consumer=False, relu_out=False, rectified_in=False):
        p_in = p_in.contiguous()
        has_bn = gamma is not None
        assert not rectified_in or relu_in, 'rectified_in: p_in = relu(p) only stands in for p where the layer rectifies its input'
        # what the forward launch is told: a rectified input without an affine needs no prologue; with one the max stays (harmless)
        fwd_relu = relu_in and not (rectified_in and not has_bn)
        assert producer_bias is None or has_bn, 'producer_bias: the hand-off happens in the batch-norm backward'
        scale = shift = mean = rstd = None
        part = None
        with label(spec.name + '/fwd'):
            if has_bn:
                scale, shift, mean, rstd = bn_stats(p_in, gamma, beta, relu_in, per_group, sync, pre_stats)
            mmf = _mm_for(packed, weight, spec, 'fwd', tuple(p_in.shape[2:]), None)
            if mmf is not None:
                y = conv_mm(p_in, mmf[0], mmf[1], bias, fwd_relu, scale, shift, per_group, None, next_bn, relu_out,
                            stats_like=spec if mmf[0].co_blk != mmf[0].CO else None)
            else:
                wf = packed.get(spec.name, 'fwd') if packed is not None else pack_weight(weight, spec, 'fwd')
                y = conv_forward(p_in, wf, bias, spec, fwd_relu, scale, shift, per_group, next_bn, relu_out)
            if next_bn:
                y, part = y
        ctx.spec, ctx.relu_in, ctx.per_group, ctx.input_is_data, ctx.sync, ctx.has_bn = \
            spec, relu_in, per_group, input_is_data, sync, has_bn
        ctx.save_for_backward(p_in, weight, gamma, beta, scale, shift, mean, rstd)
        ctx.bias_ref = bias
        ctx.packed = packed
        ctx.producer_bias, ctx.bias_grad_by_consumer = producer_bias, bool(bias_grad_by_consumer)
        ctx.nout = 2 if next_bn else 1
        if next_bn:
            ctx.mark_non_differentiable(part)
            return y, part
        return y

    @staticmethod
    def backward(ctx, dy, *_unused):
        with label(ctx.spec.name + '/bwd'):
            return BnConvAct._backward(ctx, dy) + (None,) * 12        # forward's arguments after beta

    @staticmethod
    def _backward(ctx, dy):
        """-> (dp, dweight, dbias, dgamma, dbeta)"""
        p_in, weight, gamma, beta, scale, shift, mean, rstd = ctx.saved_tensors
        spec, relu_in, per_group = ctx.spec, ctx.relu_in, ctx.per_group
        dy = dy.contiguous()
        # parameter gradients go straight into the parameters' .grad views of the flat gradient buffer when those
        # exist (no separate accumulate kernels); autograd then gets None for them
        wg, bg = _grad_buf(weight), _grad_buf(ctx.bias_ref)
        if ctx.input_is_data:
            return (None,) + _data_layer_param_grads(ctx, dy, p_in, weight, gamma, beta, mean, rstd, wg, bg)
        # last decoder stage: batch-norm backward fused with the recomputed data gradient (two passes); where the grouped weight
        # gradient has an instance its reductions AND dW come out of that one launch (one pass)
        fuse_last = ctx.has_bn and fuse_last_bn_bwd(spec)
        dw_by_bn = fuse_last and _grouped_wgrad_ok(p_in.shape, per_group)
        dw = db = dgamma = dbeta = None
        # the bias sum (unless the consuming layer's batch-norm backward already added it to bias.grad) and the weight gradient: on
        # the side stream when both go straight into .grad
        overlap = wg is not None and bg is not None and not dw_by_bn
        with on_side_stream(dy, dy, p_in, scale, shift, wg, bg, enabled=SIDE_STREAM and overlap):
            if not ctx.bias_grad_by_consumer:
                db = channel_sum(dy, out=bg)
            if not dw_by_bn:
                dw = conv_weight_grad(p_in, dy, spec, relu_in, scale, shift, per_group, out=wg)
        in_size = tuple(p_in.shape[2:])
        mmb = _mm_for(ctx.packed, weight, spec, 'bwd', tuple(dy.shape[2:]), in_size)
        wb = None
        if mmb is None:
            wb = ctx.packed.get(spec.name, 'bwd') if ctx.packed is not None else pack_weight(weight, spec, 'bwd')

        def data_grad(mask_src):
            if mmb is not None:
                return conv_mm(dy, mmb[0], mmb[1], None, False, None, None, 1, mask_src)
            return conv_backward_data(dy, wb, spec, in_size, mask_src)
        if not ctx.has_bn:
            return data_grad(p_in if relu_in else None), dw, db, None, None
        pbg = None
        if ctx.producer_bias is not None:
            pbg = ctx.producer_bias.grad
            if pbg is None:
                # allocating here would leave the gradient OUTSIDE the flat buffer the optimiser and the all-reduce read
                raise RuntimeError('bn_conv_act: producer_bias.grad is not bound -- the consumer adds the producer\'s bias gradient into it '
                                   '(FusedAdam binds every .grad to its flat buffer; a free-standing caller sets .grad = zeros first)')
        if fuse_last:
            # the data gradient is recomputed inside the batch-norm backward pass(es), never stored
            if dw_by_bn and wg is None:
                dw = torch.zeros_like(weight)
            dp, dgamma, dbeta = bn_backward_tconv1(dy, weight, p_in, gamma, mean, rstd, relu_in, per_group, ctx.sync, beta, pbg,
                                                   dw_out=(wg if wg is not None else dw) if dw_by_bn else None)
        else:
            dp = data_grad(None)
            dgamma, dbeta = bn_backward_(dp, p_in, gamma, mean, rstd, relu_in, per_group, ctx.sync, beta, pbg)
        return dp, dw, db, dgamma, dbeta


def fuse_last_bn_bwd(spec: ConvSpec):
    """Whether a layer behind a batch norm takes bn_backward_tconv1 instead of data gradient + bn_backward_: the decoder's last
    stage, a 3x3x3 stride-1 transposed conv without padding onto ONE output channel from at most 16."""
    return spec.kind == 'convt' and spec.stride == 1 and spec.co == 1 and tuple(spec.k) == (3, 3, 3) and tuple(spec.pad) == (0, 0, 0) \
        and spec.ci <= 16


def _data_layer_param_grads(ctx, dy, p_in, weight, gamma, beta, mean, rstd, wg, bg):
    """BnConvAct's backward for the first encoder layer (input_is_data): no data gradient -> (dweight, dbias, dgamma, dbeta)."""
    spec, per_group = ctx.spec, ctx.per_group
    if not ctx.has_bn:
        db = None if ctx.bias_grad_by_consumer else channel_sum(dy, out=bg)
        return conv_weight_grad(p_in, dy, spec, ctx.relu_in, None, None, per_group, out=wg), db, None, None
    assert spec.kind == 'conv' and spec.pad == (0, 0, 0) and not ctx.relu_in and not ctx.bias_grad_by_consumer
    assert p_in.shape[0] // per_group == 1                         # one batch-norm group
    # weight gradient against the NORMALISED input xhat = (x-mean)*rstd, then
    #   dw = gamma*dw_hat + beta*db ;  dgamma = <w, dw_hat> ; dbeta = <sum_k w, db>
    # (two small launches instead of 14 torch ones at the very end of the step: vg_data_bn_nshift, vg_data_bn_grads)
    db = channel_sum(dy)
    nshift = torch.empty_like(mean)
    _call(mean, 'vg_data_bn_nshift', _p(_chk(mean)), _p(_chk(rstd)), mean.numel(), _p(nshift))
    dw_hat = conv_weight_grad(p_in, dy, spec, False, rstd, nshift, per_group)
    grads = (wg, bg, _grad_buf(gamma), _grad_buf(beta))
    acc = all(g is not None for g in grads)                        # straight into the four .grad views, or four fresh tensors
    if not acc:
        grads = tuple(torch.empty_like(t) for t in (weight, db, gamma, beta))
    _call(dy, 'vg_data_bn_grads', _p(_chk(dw_hat)), _p(_chk(db)), _p(_chk(weight)), _p(_chk(gamma)), _p(_chk(beta)),
          spec.co, spec.ci, spec.k[0] * spec.k[1] * spec.k[2], *(_p(g) for g in grads), int(acc))
    return (None,) * 4 if acc else grads


def _halves_win(plan):
    """The 16-channel stride-2 transposed convs, run as two halves of 8 channels (mm_plan).  MI355X, tools/diag/mm_sweep.py, us,
    register-tiled kernel -> matrix-core kernel at the planner's tile (launched as the step launches them: convt2 forward without
    prologue, with statistics, stored rectified; conv4's data gradient masked):
      41x49x35, 576 / 64 samples:  convt2 fwd  247 ->  138 (two blocks of 5 / 4 position planes per sample and half);  conv4 bwd 33.8 -> 31.7
      82x98x70, 832 / 64 samples:  convt2 fwd 3214 -> 1619 (one position plane per block);                            conv4 bwd  325 ->  192
      21x21x21, 576 / 64 samples:  convt2 fwd 25.4 -> 30.6;  conv4 bwd 14.6 -> 15.8 -- a block holds a whole sample's half there: 4
        tiles per wave at most behind a 20 KB A image and one input copy, nothing to overlap them with.  Declined.
    In the step convt2's forward is followed by vg_tconv3d_s2_stats_of (conv_mm(stats_like=...): statistics bit-equal to the
    register-tiled engine's); bench.py --kernel-table, ms: 0.2435 -> 0.1255 + 0.0696; conv4 bwd 0.0464 -> 0.0338."""
    nslab = (plan.PH + plan.PHB - 1) // plan.PHB
    return ((plan.PDT + plan.PD - 1) // plan.PD) * nslab > 1


def mm_wins(plan):
    """Where vg_conv_mm is the faster (or an equally fast) engine -- MI355X, tools/layer_bench.py at batch 64 / 8 covariates, us,
    register-tiled kernel -> matrix-core kernel:
      blocks that hold a whole sample: convt1 fwd 234 -> 84, bwd 87 -> 50; convt2 bwd 238 -> 120; conv5 fwd 30 -> 20;
      the stride-2 transposed conv of the decoder (convt4 fwd, 4 parity classes): 890-930 -> 797, and its output is written
      with 1.04x instead of 1.88x write traffic;
      the 3x3x3 stride-1 layers with 8 <-> 16 channels (convt3 fwd 520-534 -> 516, bwd 442-446 -> 444; conv3): ties -- taken, so
      that the matrix cores carry every launch that is a real contraction and the register-tiled kernels keep the 1-channel ends.
    Kept on the register-tiled kernels: stride-2 correlations (convt4's data gradient 574 vs 714: one input channel fills the
    LDS budget, a unit is 57 MFMAs per wave between barriers; conv2 / conv4 forward).
    The 16-channel stride-2 transposed convs (convt2 forward, conv4's data gradient), two channel halves: _halves_win."""
    if plan is None:
        return False
    if USE_MM >= 2:
        return True
    if plan.co_blk != plan.CO:
        return _halves_win(plan)
    if (plan.PDT + plan.PD - 1) // plan.PD == 1:
        return True
    if plan.mode == 'tconv':
        return list(plan.ks) in ([3, 2, 2, 1], [2, 1, 1, 1], [2, 2, 2, 2])
    return plan.ks[0] in (7, 9)


def _mm_for(packed, weight, spec, direction, read_size, write_size):
    """(plan, A image) of the matrix-core kernel for this launch, or None (-> register-tiled kernels)."""
    if not USE_MM or (direction == 'bwd' and spec.co == 1):
        return None
    if packed is not None:
        got = packed.get_mm(spec.name, direction)
        if got is not None and (got[0].ID, got[0].IH, got[0].IW) == tuple(read_size):
            return got if mm_wins(got[0]) else None
    plan = mm_plan(spec, direction, read_size, write_size)
    if not mm_wins(plan):
        return None
    return plan, plan.gather(weight)


def bn_conv_act(p_in, weight, bias, gamma, beta, spec, relu_in, per_group=None, input_is_data=False, sync=None, packed=None,
                next_bn=None, pre_stats=None, producer_bias=None, bias_grad_by_consumer=False, relu_out=False, rectified_in=False):
    """-> y, or (y, statistics partials for the consuming BatchNorm3d) when next_bn is given.
    relu_out: y is stored rectified; rectified_in: p_in already is relu(p) (see BnConvAct)."""
    if per_group is None:
        per_group = p_in.shape[0]
    return BnConvAct.apply(p_in, weight, bias, gamma, beta, spec, relu_in, per_group, input_is_data, sync, packed, next_bn,
                           pre_stats, producer_bias, bias_grad_by_consumer, relu_out, rectified_in)


def _i3(v):
    v = tuple(int(a) for a in v)
    assert len(v) == 3
    return (ctypes.c_int32 * 3)(*v)


def _chk_mask(mask, Vn, like):
    """the voxel mask of the _masked entry points: [V_nat] uint8 on the data's device"""
    if mask.dtype != torch.uint8 or mask.device != like.device:
        raise ValueError(f'mask must be a uint8 tensor on {like.device}, got {mask.dtype} on {mask.device}')
    mask = mask.reshape(-1).contiguous()
    if mask.numel() != Vn:
        raise ValueError(f'mask has {mask.numel()} voxels, the native grid {Vn}')
    return mask


def _gam_launch(kind, logits, gain, x, eps, glm, nat, grid, mask, mid, tail):
    """One launch of the GAM/ELBO kernels, kind 'fwd' | 'bwd':
        vg_gam_elbo_<kind>[_embed | _masked](logits, gain, x, eps, glm, [mask,] *mid, C, B, V | nat, grid, ws, *tail)
    Everything on one grid (nat is None): the plain entry; logits on `grid`, data on `nat`: _embed; with a voxel mask: _masked (nat may
    equal grid).  The tensors are contiguous and of the kernels' dtypes (the callers' _chk); shapes and the mask are checked here."""
    G, B, V = logits.shape
    C = G - 1
    ws = torch.empty(_lib.get_lib().size('vg_gam_ws_bytes', C, B, V) // 4 + 1, dtype=torch.float32, device=x.device)
    ins = [_p(logits), _p(gain), _p(x), _p(eps), _p(glm)]
    if nat is None:
        assert mask is None, 'a mask needs nat and grid (they may be equal)'
        fn, dims = 'vg_gam_elbo_' + kind, (C, B, V)
    else:
        Vn = int(nat[0]) * int(nat[1]) * int(nat[2])
        assert V == int(grid[0]) * int(grid[1]) * int(grid[2]) and x.shape == (B, Vn) and eps.shape == (Vn,) and (C == 0 or glm.shape == (C, Vn))
        fn, dims = 'vg_gam_elbo_%s_%s' % (kind, 'embed' if mask is None else 'masked'), (C, B, _i3(nat), _i3(grid))
        if mask is not None:
            ins.append(_p(_chk_mask(mask, Vn, x)))
    _call(x, fn, *ins, *mid, *dims, _p(ws), *tail)


def _gam_forward(ctx, logits, gain, x, eps, glm, logits_bias, nat=None, grid=None, mask=None):
    """forward of GamElbo (nat is None: everything on one grid), GamElboEmbed and GamElboMasked (mask given; nat may equal grid)"""
    G, B, V = logits.shape
    logits = _chk(logits.contiguous()); gain = _chk(gain.contiguous()); x = _chk(x.contiguous())
    eps = _chk(eps.contiguous(), torch.float64); glm = _chk(glm.contiguous())
    slp = torch.empty(B, dtype=torch.float32, device=x.device)
    dist = torch.empty((G - 1, B), dtype=torch.float32, device=x.device)
    _gam_launch('fwd', logits, gain, x, eps, glm, nat, grid, mask, (), (_p(slp), _p(dist), None))
    ctx.save_for_backward(logits, gain, x, eps, glm, dist)
    ctx.logits_bias, ctx.nat, ctx.grid, ctx.mask = logits_bias, nat, grid, mask
    return slp, dist


def _gam_backward(ctx, g_slp, g_dist):
    """-> d_logits, d_gain, d_eps; sum(d_logits) is added into ctx.logits_bias.grad"""
    logits, gain, x, eps, glm, dist = ctx.saved_tensors
    tot = None
    if ctx.logits_bias is not None:
        pb = ctx.logits_bias
        assert pb.numel() == 1
        if pb.grad is None:
            raise RuntimeError('GamElbo: logits_bias.grad is not bound (see bn_conv_act: the bias gradient is added into the caller\'s buffer)')
        tot = pb.grad
    g_slp = _chk(g_slp.contiguous()); g_dist = _chk(g_dist.contiguous())
    d_logits = torch.empty_like(logits)
    d_gain = torch.empty_like(gain)
    d_eps = torch.empty_like(eps)
    _gam_launch('bwd', logits, gain, x, eps, glm, ctx.nat, ctx.grid, ctx.mask, (_p(dist), _p(g_slp), _p(g_dist)),
                (_p(d_logits), _p(d_gain), _p(d_eps), _p(tot), 1))
    return d_logits, d_gain, d_eps


class GamElbo(torch.autograd.Function):
    """(logits[G,B,V], gain[C,B], x[B,V], eps[V] f64, glm[C,V]) -> (sum_log_prob[B], dist[C,B]).
    `logits_bias` (optional Parameter of one element): the bias of the one-output-channel layer that produced `logits`; the backward
    then adds sum(d_logits) into its .grad (explicit hand-off: that layer is built with bias_grad_by_consumer=True)."""

    @staticmethod
    def forward(ctx, logits, gain, x, eps, glm, logits_bias=None):
        return _gam_forward(ctx, logits, gain, x, eps, glm, logits_bias)

    @staticmethod
    def backward(ctx, g_slp, g_dist):
        d_logits, d_gain, d_eps = _gam_backward(ctx, g_slp, g_dist)
        return d_logits, d_gain, None, d_eps, None, None


class GamElboEmbed(torch.autograd.Function):
    """GamElbo for a network that runs on a grid larger than the data's (schema.NetGeometry.pad != 0): logits[G,B,V_grid] on the
    grid, x[B,V_nat], eps[V_nat] f64, glm[C,V_nat] on the native grid `nat` at the low corner of `grid`
    -> (sum_log_prob[B], dist[C,B]) over native voxels only.  The gradient of the logits is exactly zero in the padding.
    `logits_bias`: as in GamElbo."""

    @staticmethod
    def forward(ctx, logits, gain, x, eps, glm, nat, grid, logits_bias=None):
        return _gam_forward(ctx, logits, gain, x, eps, glm, logits_bias, tuple(int(a) for a in nat), tuple(int(a) for a in grid))

    @staticmethod
    def backward(ctx, g_slp, g_dist):
        d_logits, d_gain, d_eps = _gam_backward(ctx, g_slp, g_dist)
        return d_logits, d_gain, None, d_eps, None, None, None, None


class GamElboMasked(torch.autograd.Function):
    """GamElbo / GamElboEmbed restricted to a voxel mask: `mask` is a uint8 tensor of V_nat voxels on the native grid `nat` (which may
    equal `grid`), nonzero = the voxel counts.  (sum_log_prob[B], dist[C,B]) run over the voxels of the mask only; the gradients of the
    logits and of eps are exactly zero at every other voxel, padding included.  The mask has no gradient.  `logits_bias`: as in GamElbo."""

    @staticmethod
    def forward(ctx, logits, gain, x, eps, glm, mask, nat, grid, logits_bias=None):
        return _gam_forward(ctx, logits, gain, x, eps, glm, logits_bias, tuple(int(a) for a in nat), tuple(int(a) for a in grid), mask)

    @staticmethod
    def backward(ctx, g_slp, g_dist):
        d_logits, d_gain, d_eps = _gam_backward(ctx, g_slp, g_dist)
        return d_logits, d_gain, None, d_eps, None, None, None, None, None


def embed_volumes(x, nat, grid):
    """x (B, *nat) or (B, V_nat) -> (B, *grid): zero-padded at the high end of each axis, one launch that writes every element
    (vg_embed_volumes).  No gradient: the data has none."""
    nat = tuple(int(a) for a in nat); grid = tuple(int(a) for a in grid)
    B = x.shape[0]
    x = _chk(x.detach().reshape(B, -1).contiguous())
    assert x.shape[1] == nat[0] * nat[1] * nat[2], (x.shape, nat)
    out = torch.empty((B,) + grid, dtype=torch.float32, device=x.device)
    _call(x, 'vg_embed_volumes', _p(x), _i3(nat), _i3(grid), B, _p(out))
    return out


def _latent_forward(ctx, mu, w, a, eps_w, eps_d, G):
    """vg_latent_fwd on mu, w, a [B, L] (contiguous fp32, each its own tensor or a slice of one) -> (zcat, kl, d, flag)"""
    B, L = mu.shape
    eps_w = _chk(eps_w.contiguous()); eps_d = _chk(eps_d.contiguous())
    assert w.shape == (B, L) and a.shape == (B, L) and eps_d.shape == (B, L) and eps_w.numel() == B
    zcat = torch.empty((G * B, L + G), dtype=torch.float32, device=mu.device)
    kl = torch.empty(B, dtype=torch.float32, device=mu.device)
    d = torch.empty((B, L), dtype=torch.float32, device=mu.device)
    flag = torch.empty(1, dtype=torch.float32, device=mu.device)
    _call(mu, 'vg_latent_fwd', _p(mu), _p(w), _p(a), _p(eps_w), _p(eps_d), B, L, G, _p(zcat), _p(kl), _p(d), _p(flag))
    ctx.G = G
    ctx.mark_non_differentiable(d)
    return zcat, kl, d, flag, eps_w, eps_d


def _latent_backward(ctx, mu, w, d, flag, eps_w, eps_d, g_zcat, g_kl, g_mu, g_w, g_a):
    """vg_latent_bwd: the gradients are written into g_mu, g_w, g_a [B, L]"""
    B, L = mu.shape
    gz = _p(_chk(g_zcat.contiguous())) if g_zcat is not None else None
    gk = _p(_chk(g_kl.contiguous())) if g_kl is not None else None
    _call(mu, 'vg_latent_bwd', _p(mu), _p(w), _p(d), _p(flag), _p(eps_w), _p(eps_d), gz, gk, B, L, ctx.G,
             _p(g_mu), _p(g_w), _p(g_a))


class LatentSample(torch.autograd.Function):
    """(mu, w, a, eps_w, eps_d, G) -> (zcat[G*B, L+G], kl_z[B], d[B, L]); one launch each way
    (vae_reg_GP.py:321-329, 339-342, 400).  `a` is fc43's output (d = exp(a) + the batch-wide 1e-6 floor)."""

    @staticmethod
    def forward(ctx, mu, w, a, eps_w, eps_d, G):
        mu = _chk(mu.contiguous()); w = _chk(w.contiguous()); a = _chk(a.contiguous())
        zcat, kl, d, flag, eps_w, eps_d = _latent_forward(ctx, mu, w, a, eps_w, eps_d, G)
        ctx.save_for_backward(mu, w, d, flag, eps_w, eps_d)
        return zcat, kl, d

    @staticmethod
    def backward(ctx, g_zcat, g_kl, _g_d):
        mu, w, d, flag, eps_w, eps_d = ctx.saved_tensors
        g_mu = torch.empty_like(mu); g_w = torch.empty_like(mu); g_a = torch.empty_like(mu)
        _latent_backward(ctx, mu, w, d, flag, eps_w, eps_d, g_zcat, g_kl, g_mu, g_w, g_a)
        return g_mu, g_w, g_a, None, None, None


class LatentSampleStacked(torch.autograd.Function):
    """LatentSample on the stacked heads output mwa[3, B, L] = (mu, w, a): one gradient tensor goes back to HeadsAct
    (indexing mwa[0..2] under autograd costs three select-backward fills + copies + two adds per step)."""

    @staticmethod
    def forward(ctx, mwa, eps_w, eps_d, G):
        mwa = _chk(mwa.contiguous())
        zcat, kl, d, flag, eps_w, eps_d = _latent_forward(ctx, mwa[0], mwa[1], mwa[2], eps_w, eps_d, G)
        ctx.save_for_backward(mwa, d, flag, eps_w, eps_d)
        return zcat, kl, d

    @staticmethod
    def backward(ctx, g_zcat, g_kl, _g_d):
        mwa, d, flag, eps_w, eps_d = ctx.saved_tensors
        g = torch.empty_like(mwa)
        _latent_backward(ctx, mwa[0], mwa[1], d, flag, eps_w, eps_d, g_zcat, g_kl, g[0], g[1], g[2])
        return g, None, None, None


class ElboLoss(torch.autograd.Function):
    """loss[1] = c_kl*sum(kl_z) + c_slp*sum(slp) + c_gp*gp_kl + c_dist*sum(dist)   (vae_reg_GP.py:406-410)."""

    @staticmethod
    def forward(ctx, kl_z, slp, dist, gp_kl, coef):
        kl_z = _chk(kl_z.contiguous()); slp = _chk(slp.contiguous()); dist = _chk(dist.contiguous()); gp_kl = _chk(gp_kl.contiguous())
        loss = torch.empty(1, dtype=torch.float32, device=kl_z.device)
        ctx.coef = tuple(float(c) for c in coef)
        ctx.shapes = (kl_z.shape, slp.shape, dist.shape, gp_kl.shape)
        _call(kl_z, 'vg_loss_fwd', _p(kl_z), _p(slp), _p(dist), _p(gp_kl), kl_z.numel(), dist.numel(), *ctx.coef, _p(loss))
        return loss

    @staticmethod
    def backward(ctx, g):
        sk, ss, sd, sg = ctx.shapes
        g = _chk(g.contiguous())
        g_kl = torch.empty(sk, dtype=torch.float32, device=g.device); g_slp = torch.empty(ss, dtype=torch.float32, device=g.device)
        g_dist = torch.empty(sd, dtype=torch.float32, device=g.device); g_gp = torch.empty(sg, dtype=torch.float32, device=g.device)
        _call(g, 'vg_loss_bwd', _p(g), g_kl.numel(), g_dist.numel(), *ctx.coef, _p(g_kl), _p(g_slp), _p(g_dist), _p(g_gp))
        return g_kl, g_slp, g_dist, g_gp, None


def _fc_split(M, N, K):
    """Split-K factor of a fully connected product.  The kernel keeps four 64-index steps in flight, so a reduction of a few hundred
    indices is one or two memory round trips and is left whole; a LONG reduction onto few output tiles (fc1: 3072 -> 64 x 200; fc8's data
    gradient: 3840 -> 576 x 200) is cut into pieces of >= 256 indices until ~1024 blocks exist.  The pieces are sized as the kernel
    sizes them (ceil(K / ksplit) rounded up to 64) and none may be empty."""
    tiles = ((M + 31) // 32) * ((N + 31) // 32)
    if K <= 1024:
        return 1
    ks = max(1, min(K // 256, 1024 // tiles))
    if ks <= 1:
        return 1
    kchunk = (((K + ks - 1) // ks) + 63) // 64 * 64
    return (K + kchunk - 1) // kchunk


def fc_job(A, B, C, M, N, K, a_strides, b_strides, c_strides, flags=0, batch=1, bias=None, bias_sb=0, amask=None, cmask=None,
           cx=None, cx_sb=0, ksplit=None, ws=None):
    """One product for vg_fc_gemm_jobs: C[z][m][n] (+)= epilogue(sum_k A[z](m,k) B[z](k,n)); a_strides = (sm, sk, sb),
    b_strides = (sk, sn, sb), c_strides = (sm, sb), all in elements (include/vaegam.h).  ws: the caller's own split-K workspace
    (at least vg_fc_ws_bytes; one is allocated when it is None).  Returns (job struct, tensors to keep alive)."""
    lib = _lib.get_lib()
    if ksplit is None:
        ksplit = _fc_split(M, N + (1 if flags & _lib.FC_B_ONES else 0), K) if batch == 1 else 1
    d = _lib.FcDesc(M, N, K, batch, a_strides[0], a_strides[1], a_strides[2], b_strides[0], b_strides[1], b_strides[2],
                    c_strides[0], c_strides[1], bias_sb, cx_sb, ksplit, flags)
    if ksplit > 1 and ws is None:
        ws = torch.empty(lib.size('vg_fc_ws_bytes', ctypes.byref(d)) // 4, dtype=torch.float32, device=C.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    return _lib.FcJob(d, ptr(A), ptr(amask), ptr(B), ptr(bias), ptr(cmask), ptr(C), ptr(cx), ptr(ws)), (A, B, C, bias, amask, cmask, cx, ws)


def fc_launch(ref, jobs):
    """vg_fc_gemm_jobs: the products of `jobs` (fc_job results, <= 4) in one launch on ref's stream."""
    arr = (_lib.FcJob * len(jobs))(*[j[0] for j in jobs])
    _call(ref, 'vg_fc_gemm_jobs', arr, len(jobs))


def fc_plan(jobs):
    """What fc_launch(jobs) would launch, from the launcher's own planner (vg_fc_plan): nothing is launched, no memory is touched.
    -> dict(tile, grid, reduce_blocks, njobs, jobs=[dict(a_vec, b_vec, big, kchunk, gx, gy, first, blocks), ...])."""
    arr = (_lib.FcJob * max(len(jobs), 1))(*[j[0] for j in jobs])
    rec = (ctypes.c_int32 * _lib.FC_PLAN_LEN)()
    _lib.get_lib().call('vg_fc_plan', arr, len(jobs), rec, len(rec))
    plan = dict(zip(_lib.FC_PLAN_HEAD_FIELDS, (int(v) for v in rec[:4])))
    plan['jobs'] = [dict(zip(_lib.FC_PLAN_JOB_FIELDS, (int(v) for v in rec[4 + 8 * j:12 + 8 * j]))) for j in range(plan['njobs'])]
    return plan


def fc_gemm(A, B, C, *args, **kw):
    """A single product (see fc_job)."""
    fc_launch(C, [fc_job(A, B, C, *args, **kw)])
    return C


def _fc_forward(x, weight, bias, relu, relu_in):
    M, K = x.shape; N = weight.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    fl = _lib.FC_C_BIAS | (_lib.FC_C_RELU if relu else 0) | (_lib.FC_A_RELU if relu_in else 0)
    return fc_gemm(x, weight, y, M, N, K, (x.stride(0), 1, 0), (1, weight.stride(0), 0), (N, 0), fl, bias=bias)


def _fc_backward(gy, x, weight, y, relu_in, need_gx, wg, bg):
    """Gradients of y = [relu](x' W^T + b), x' = relu(x) if relu_in: gy is masked with y > 0 inside both products (y None: no ReLU);
    -> (gx or None, gw or None, gb or None); wg / bg (the .grad views) are added into when given.  ONE launch: the data gradient and
    the weight gradient (whose extra column is the bias gradient) are two jobs of vg_fc_gemm_jobs."""
    M, N = gy.shape; K = x.shape[1]
    am = _lib.FC_A_MASK if y is not None else 0
    jobs = []
    gx = None
    if need_gx:
        gx = torch.empty((M, K), dtype=torch.float32, device=gy.device)
        jobs.append(fc_job(gy, weight, gx, M, K, N, (N, 1, 0), (weight.stride(0), 1, 0), (K, 0), am | (_lib.FC_C_MASK if relu_in else 0),
                           amask=y, cmask=x if relu_in else None))
    acc = wg is not None and bg is not None
    gw = wg if acc else torch.empty((N, K), dtype=torch.float32, device=gy.device)
    gb = bg if acc else torch.empty((N,), dtype=torch.float32, device=gy.device)
    jobs.append(fc_job(gy, x, gw, N, K, M, (1, N, 0), (x.stride(0), 1, 0), (K, 0),
                       am | _lib.FC_B_ONES | (_lib.FC_B_RELU if relu_in else 0) | (_lib.FC_C_ACCUM if acc else 0), amask=y, cx=gb))
    fc_launch(gy, jobs)
    return gx, (None if acc else gw), (None if acc else gb)


class LinearAct(torch.autograd.Function):
    """y = [relu]([relu](x) @ W^T + b) for the fully connected layers (vae_reg_GP.py:203-209, 224-234, 243-259) on vg_fc_gemm: bias and
    ReLU in the product's epilogue, the ReLU of a pre-activation input (conv5's output, :243) in its operand load; the backward is two
    launches -- the data gradient and the weight gradient whose extra column is the bias gradient, both masking the incoming gradient
    with y > 0 on load and adding dW / db straight into the .grad views of the flat gradient buffer."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, relu_in=False):
        x = _chk(x.contiguous()); _chk(weight); _chk(bias)
        y = _fc_forward(x, weight, bias, relu, relu_in)
        ctx.relu, ctx.relu_in = relu, relu_in
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.bias_ref = bias
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        bias = ctx.bias_ref
        gy = _chk(gy.contiguous())
        gx, gw, gb = _fc_backward(gy, x, weight, y, ctx.relu_in, ctx.needs_input_grad[0], _grad_buf(weight), _grad_buf(bias))
        return gx, gw, gb, None, None


class HeadsAct(torch.autograd.Function):
    """The three encoder heads (vae_reg_GP.py:205-209, 246-252: fc31/32/33 -> ReLU -> fc41/42/43) as ONE product over the stacked
    first-stage weights and ONE batched product over the second stage.  W3 [3*H, F], b3 [3*H], W4 [3, L, H], b4 [3, 1, L] are
    views of the flat parameter buffer (the optimiser lays the six weights / six biases out back to back), gW3.. the matching
    views of the flat gradient buffer, which the backward adds into directly.  9 -> 2 launches forward, 23 -> 2 backward."""

    @staticmethod
    def forward(ctx, h, W3, b3, W4, b4, gW3, gb3, gW4, gb4):
        B = h.shape[0]
        h = _chk(h.contiguous())
        G, L, H = W4.shape
        y = _fc_forward(h, W3, b3, True, False)                          # (B, 3H)
        out = torch.empty((G, B, L), dtype=torch.float32, device=h.device)
        fc_gemm(y, W4, out, B, L, H, (G * H, 1, H), (1, H, L * H), (L, B * L), _lib.FC_C_BIAS, batch=G, bias=b4, bias_sb=L)
        ctx.save_for_backward(h, y, W3, W4)
        ctx.grads = (gW3, gb3, gW4, gb4)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, y, W3, W4 = ctx.saved_tensors
        gW3, gb3, gW4, gb4 = ctx.grads
        B = h.shape[0]
        G, L, H = W4.shape
        gout = _chk(gout.contiguous())
        gX = torch.empty((B, G * H), dtype=torch.float32, device=h.device)           # gradient w.r.t. y, before its ReLU mask
        fc_launch(gout, [fc_job(gout, W4, gX, B, H, L, (L, 1, B * L), (H, 1, L * H), (G * H, H), 0, batch=G),
                         fc_job(gout, y, gW4, L, H, B, (1, L, B * L), (G * H, 1, H), (H, L * H), _lib.FC_B_ONES | _lib.FC_C_ACCUM, batch=G,
                                cx=gb4, cx_sb=L)])
        gh, _, _ = _fc_backward(gX, h, W3, y, False, True, gW3, gb3)
        return gh, None, None, None, None, None, None, None, None


def linear_act(layer, x, relu, relu_in=False):
    return LinearAct.apply(x, layer.weight, layer.bias, relu, relu_in)


def gam_maps(logits, gain, x, eps, glm, nat=None, grid=None, mask=None):
    """Reconstruction path (vae_reg_GP.py:331,391-392): the C+2 maps [base, cons_1..C, full_rec] as [C+2,B,V].
    With nat / grid (see GamElboEmbed) the logits are on the grid and the maps come out on the native grid: V = V_nat.
    With mask (see GamElboMasked; needs nat and grid, which may be equal) every map is exactly 0 outside the mask."""
    G, B, V = logits.shape
    Vn = V if nat is None else int(nat[0]) * int(nat[1]) * int(nat[2])
    slp = torch.empty(B, dtype=torch.float32, device=x.device)
    dist = torch.empty((max(G - 1, 1), B), dtype=torch.float32, device=x.device)
    maps = torch.empty((G + 1, B, Vn), dtype=torch.float32, device=x.device)
    _gam_launch('fwd', _chk(logits.contiguous()), _chk(gain.contiguous()), _chk(x.contiguous()), _chk(eps.contiguous(), torch.float64),
                _chk(glm.contiguous()), nat, grid, mask, (), (_p(slp), _p(dist), _p(maps)))
    return maps


def gam_stats_slots(C):
    """Accumulator slots per subject and voxel of gam_stats_accumulate: 3C + 8 (slot table: include/vaegam.h)."""
    return _lib.get_lib().size('vg_gam_stats_slots', int(C))


def gam_stats_accumulate(logits, gain, x, subj, acc, nat=None, grid=None, mask=None):
    """acc[s] += the per-voxel sums over the volumes b of this batch with subj[b] == s: first and second moments of the C+2 maps
    (gam_maps' values, never materialised), of the data and of the residual, and the sums of (r + cons_i)^2 (vg_gam_stats_accumulate).
    logits [C+1, B, V_grid], gain [C, B], x [B, V_nat] fp32; subj int32 [B]; acc float64 [S, 3C+8, V_nat], updated in place and
    returned.  nat / grid / mask as gam_maps (without nat everything is on one grid).  One launch, no atomics: bit-reproducible.  A
    subj entry outside [0, S) is skipped by the kernel; callers that want that refused check on the host."""
    G, B, V = logits.shape
    C = G - 1
    if nat is None:
        nat = grid = (1, 1, int(V))
    Vn = int(nat[0]) * int(nat[1]) * int(nat[2])
    assert V == int(grid[0]) * int(grid[1]) * int(grid[2]) and x.shape == (B, Vn) and subj.shape == (B,) and (C == 0 or gain.shape == (C, B))
    assert acc.dim() == 3 and acc.shape[1] == 3 * C + 8 and acc.shape[2] == Vn
    _call(x, 'vg_gam_stats_accumulate', _p(_chk(logits.contiguous())), _p(_chk(gain.contiguous())) if C > 0 else None, _p(_chk(x.contiguous())),
          _p(_chk(subj, torch.int32)), None if mask is None else _p(_chk_mask(mask, Vn, x)), C, B, int(acc.shape[0]), _i3(nat), _i3(grid),
          _p(_chk(acc, torch.float64)))
    return acc


SignflipPlan = namedtuple('SignflipPlan', _lib.SIGNFLIP_PLAN_FIELDS + ('ws_bytes',))


def signflip_plan(S, V, P) -> SignflipPlan:
    """What signflip_maxstat launches for S subjects, V voxels and P permutations, from vg_signflip_maxstat's own planner
    (vg_signflip_plan; slot table: include/vaegam.h): nothing is launched.  ws_bytes joins the two workspace slots.  A refused shape
    raises VgError."""
    rec = (ctypes.c_int32 * len(_lib.SIGNFLIP_PLAN_FIELDS))()
    _lib.get_lib().call('vg_signflip_plan', int(S), int(V), int(P), rec, len(rec))
    return SignflipPlan(*rec, ws_bytes=int(rec[-2]) + (int(rec[-1]) << 31))


def signflip_maxstat(m, scale, signs, tail='two'):
    """Sign-flip permutation test with the max-statistic in one pass (vg_signflip_maxstat; the statistic to the bit: include/vaegam.h).
    m float64 (S, V): one value per subject and voxel (subject means, or any contrast of maps), 2 <= S <= 64; scale float64 (V,):
    1 / sqrt(S * sum_s m^2), 0 at a voxel that takes no part; signs (P,) int64 or uint64 words, bit s flips subject s; tail 'two',
    'pos' or 'neg'.  Returns stat0 (V,) float64, maxstat (P,) float64, cnt_unc (V,) int32.  The (P, V) array of statistics is never
    formed; no atomics: bit-reproducible."""
    if tail not in _lib.SIGNFLIP_TAILS:
        raise ValueError('signflip_maxstat: tail must be one of %s, not %r' % (', '.join(_lib.SIGNFLIP_TAILS), tail))
    assert m.dim() == 2 and scale.shape == (m.shape[1],) and signs.dim() == 1 and signs.dtype in (torch.int64, torch.uint64)
    S, V = (int(n) for n in m.shape)
    P = int(signs.shape[0])
    m, scale, signs = _chk(m.contiguous(), torch.float64), _chk(scale.contiguous(), torch.float64), signs.contiguous()
    ws = torch.empty(_lib.get_lib().size('vg_signflip_ws_bytes', S, V, P), dtype=torch.uint8, device=m.device)
    stat0 = torch.empty(V, dtype=torch.float64, device=m.device)
    maxstat = torch.empty(P, dtype=torch.float64, device=m.device)
    cnt = torch.empty(V, dtype=torch.int32, device=m.device)
    _call(m, 'vg_signflip_maxstat', _p(m), _p(scale), _p(signs), S, V, P, _lib.SIGNFLIP_TAILS.index(tail), _p(ws), _p(stat0), _p(maxstat),
          _p(cnt))
    return stat0, maxstat, cnt


class CholeskyF64(torch.autograd.Function):
    """L = chol(A) for a batch of small float64 SPD matrices (vg_cholesky_f64; n <= 128).  Backward is the
    standard  dA = sym( L^-T  Phi(L^T dL)  L^-1 )  with two triangular solves (rocBLAS trsm, capturable)."""

    @staticmethod
    def forward(ctx, a):
        assert a.dtype == torch.float64 and a.dim() == 3 and a.shape[1] == a.shape[2]
        a = a.contiguous()
        l = torch.empty_like(a)
        _call(a, 'vg_cholesky_f64', _p(a), _p(l), a.shape[0], a.shape[1])
        ctx.save_for_backward(l)
        return l

    @staticmethod
    def backward(ctx, gl):
        (l,) = ctx.saved_tensors
        p = (l.transpose(1, 2) @ gl).tril()
        p = p - 0.5 * torch.diag_embed(p.diagonal(dim1=1, dim2=2))
        x = torch.linalg.solve_triangular(l.transpose(1, 2), p, upper=True)              # L^-T P
        s = torch.linalg.solve_triangular(l, x, upper=False, left=False)                  # (L^-T P) L^-1
        return 0.5 * (s + s.transpose(1, 2))


def cholesky(a):
    """Batched lower Cholesky factor; the HIP kernel for float64 n <= 128, torch otherwise."""
    if a.dtype == torch.float64 and a.shape[-1] <= 128 and (a.is_cuda or _lib.get_lib().host_pointers_ok):
        return CholeskyF64.apply(a)
    return torch.linalg.cholesky_ex(a, check_errors=False).L


GAIN_MAX_BATCH = 4096          # volumes per joint gain draw (vg_gp_gain_*: B > 1024 takes the tiled path, B > 4096 is refused)
# Tests only (set with monkeypatch): route every GpGain call through vg_gp_gain_fwd_tiled / _bwd_tiled, the tiled path at any B.
# Off: the library picks the path by batch size.
GAIN_FORCE_TILED = False


def check_gain_batch(B, what='the gain block'):
    """ValueError unless `B` volumes fit one joint gain draw (B <= GAIN_MAX_BATCH)."""
    if int(B) > GAIN_MAX_BATCH:
        raise ValueError('%s would draw the gains of %d volumes jointly: the limit is %d volumes per joint draw (vg_gp_gain_fwd). '
                         'Use a smaller minibatch or, under data parallelism, dp_gain=\'local\' (each rank draws its own slice).'
                         % (what, int(B), GAIN_MAX_BATCH))


class GainConsts:
    """Device-side constants of the gain block of one model: the parameter-offset table, the inducing grids, the HRF taps."""

    def __init__(self, table, xu, hrf, n, jitter_ku=0.0, jitter_b=1e-5, prior_var=10.0):
        self.table, self.xu, self.hrf = table, xu, hrf            # int64 [C][10], fp32 [K][n] (or None), float64 [taps]
        self.C, self.n = int(table.shape[0]), int(n)
        self.jitter_ku, self.jitter_b, self.prior_var = float(jitter_ku), float(jitter_b), float(prior_var)

    def desc(self, B):
        return _lib.GainDesc(self.C, int(B), self.n, int(self.hrf.numel()), self.jitter_b, self.jitter_ku, self.prior_var)


GainPlan = namedtuple('GainPlan', _lib.GAIN_PLAN_FIELDS)


def gain_plan(consts, B, forced=False) -> GainPlan:
    """What GpGain would launch for a minibatch of B volumes (forced: under GAIN_FORCE_TILED), from the launchers' own planner
    (vg_gp_gain_plan): nothing is launched.  `path` is 'lds', 'blocked' or 'tiled'; B > GAIN_MAX_BATCH raises VgError."""
    d = consts.desc(B)
    rec = (ctypes.c_int32 * len(GainPlan._fields))()
    _lib.get_lib().call('vg_gp_gain_plan', ctypes.byref(d), int(bool(forced)), rec, len(rec))
    return GainPlan(_lib.GAIN_PATHS[rec[0]], *rec[1:])


class GpGain(torch.autograd.Function):
    """(covariates (B, >=C) fp32, eps_beta (C, B) fp32) -> gains task_var (C, B) fp32, gp_kl (1,) fp32 and float64 copies of
    beta_mean (C,B), beta_cov (C,B,B), f_bar (C,B), Sigma (C,B,B), kl terms (C,) for exports / tests: vg_gp_gain_fwd, one
    workgroup per covariate up to B = 1024, the tiled multi-workgroup path up to B = 4096 (vae_reg_GP.py:345-378, gp.py:41-110;
    GAIN_FORCE_TILED: the tiled path at any B).  The backward launch adds the gain-parameter gradients
    straight into the flat fp32 gradient buffer; `params` are listed only so that autograd calls it.
    `join_stream`: the stream that must wait for the backward launch (the model runs this block on a second stream)."""

    @staticmethod
    def forward(ctx, covariates, eps_beta, consts, flat_p, flat_g, join_stream, *params):
        lib = _lib.get_lib()
        B = covariates.shape[0]
        C = consts.C
        assert covariates.dtype == torch.float32 and covariates.dim() == 2 and covariates.shape[1] >= C and covariates.stride(1) == 1
        eps_beta = _chk(eps_beta.contiguous())
        assert eps_beta.shape == (C, B)
        dev = covariates.device
        d = consts.desc(B)
        ws = torch.empty(lib.size('vg_gp_gain_ws_bytes', C, B, consts.n) // 8, dtype=torch.float64, device=dev)
        tv = torch.empty((C, B), dtype=torch.float32, device=dev)
        kl = torch.empty(1, dtype=torch.float32, device=dev)
        bm = torch.empty((C, B), dtype=torch.float64, device=dev)
        bc = torch.empty((C, B, B), dtype=torch.float64, device=dev)
        fb = torch.zeros((C, B), dtype=torch.float64, device=dev)
        sg = torch.zeros((C, B, B), dtype=torch.float64, device=dev)
        tiled = bool(GAIN_FORCE_TILED)
        _call(covariates, 'vg_gp_gain_fwd_tiled' if tiled else 'vg_gp_gain_fwd', ctypes.byref(d), _p(consts.table), _p(flat_p), _p(consts.xu), _p(covariates),
              int(covariates.stride(0)), _p(eps_beta), _p(consts.hrf), _p(ws), _p(tv), _p(kl), _p(bm), _p(bc), _p(fb), _p(sg))
        kl_terms = ws[-(C + 8):-8]                                # per-covariate kl_lin (+ kl_gp), float64
        ctx.save_for_backward(covariates, eps_beta, ws)
        ctx.consts, ctx.flat_p, ctx.flat_g, ctx.join_stream, ctx.tiled = consts, flat_p, flat_g, join_stream, tiled
        ctx.mark_non_differentiable(bm, bc, fb, sg, kl_terms)
        return tv, kl, bm, bc, fb, sg, kl_terms

    @staticmethod
    def backward(ctx, g_tv, g_kl, *_):
        covariates, eps_beta, ws = ctx.saved_tensors
        consts = ctx.consts
        B = covariates.shape[0]
        d = consts.desc(B)
        if g_tv is None:
            g_tv = torch.zeros((consts.C, B), dtype=torch.float32, device=covariates.device)
        if g_kl is None:
            g_kl = torch.zeros(1, dtype=torch.float32, device=covariates.device)
        g_tv = _chk(g_tv.contiguous()); g_kl = _chk(g_kl.contiguous())
        _call(covariates, 'vg_gp_gain_bwd_tiled' if ctx.tiled else 'vg_gp_gain_bwd', ctypes.byref(d), _p(consts.table), _p(ctx.flat_p), _p(consts.xu), _p(covariates),
              int(covariates.stride(0)), _p(eps_beta), _p(consts.hrf), _p(ws), _p(g_tv), _p(g_kl), _p(ctx.flat_g))
        if ctx.join_stream is not None and covariates.is_cuda:
            cur = torch.cuda.current_stream(covariates.device)
            if cur != ctx.join_stream:
                ctx.join_stream.wait_stream(cur)               # the gradients are written outside autograd's own stream bookkeeping
        return (None,) * len(ctx.needs_input_grad)


class HrfAcrossRanks(torch.autograd.Function):
    """Data parallel, dp_gain='local': the causal HRF convolution along the GLOBAL batch index (vae_reg_GP.py:283-305, 377-378) of
    gains that every rank drew for its own slice.  Forward: all-gather the pre-HRF gains of the HRF covariates ((Ch, B) -> (Ch, Bg):
    a few hundred floats), multiply by the (Bg, Bg) Toeplitz matrix of the 15 taps, keep this rank's columns.  Backward: a rank's
    loss also depends on the up to 14 volumes in front of its slice, which another rank drew -- the gradient with respect to the
    gathered gains is summed over ranks (one tiny all-reduce) and each rank keeps the columns it drew.  Without this the
    convolution would restart at every slice boundary."""

    @staticmethod
    def forward(ctx, pre, T, dp, lo):
        B = pre.shape[1]
        full = dp.all_gather_rows(pre.t().contiguous()).t()             # (Ch, Bg), rank order = batch order
        ctx.save_for_backward(T)
        ctx.dp, ctx.lo, ctx.B = dp, int(lo), int(B)
        return (full @ T)[:, lo:lo + B].contiguous()

    @staticmethod
    def backward(ctx, g):
        (T,) = ctx.saved_tensors
        lo, B = ctx.lo, ctx.B
        gp = g.contiguous() @ T[:, lo:lo + B].t()                       # (Ch, Bg): d(this rank's loss) / d(every pre-HRF gain it used)
        gp = ctx.dp.allreduce_sum_(gp)
        return gp[:, lo:lo + B].contiguous(), None, None, None


def adam_advance_(state, lr, b1, b2):
    """state = double[3] {lr/(1-b1^t), sqrt(1-b2^t), t} on the device: t += 1, scalars refreshed (one thread)."""
    _call(state, 'vg_adam_advance', _p(_chk(state, torch.float64)), float(lr), float(b1), float(b2))


def _adam_step(fn, p, g, m, v, b1, b2, eps, step_scalars, *guard):
    assert p.dtype == g.dtype == m.dtype == v.dtype and p.dtype in (torch.float32, torch.float64)
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    _call(p, fn, _p(p), _p(g), _p(m), _p(v), p.numel(), int(p.dtype == torch.float64), float(b1), float(b2),
          float(eps), *(_p(_chk(t, torch.float64)) for t in (step_scalars,) + guard))


def adam_step_(p, g, m, v, b1, b2, eps, step_scalars):
    """In-place fused Adam over one flat buffer (fp32 or fp64)."""
    _adam_step('vg_adam_step', p, g, m, v, b1, b2, eps, step_scalars)


# --------------------------------------------------------------------------- gradient guard (opt-in; include/vaegam.h)
GUARD_STATE_LEN = _lib.GUARD_STATE_LEN
GUARD_NORM, GUARD_SCALE, GUARD_APPLY, GUARD_SEEN, GUARD_SKIPPED, GUARD_CLIPPED, GUARD_NORM_SUM, GUARD_NORM_MAX = range(8)


def grad_guard_ws(g32, g64):
    """Workspace for grad_guard_ over these two flat gradient buffers (either may be None): the per-block partial sums."""
    ref = g32 if g32 is not None else g64
    n = _lib.get_lib().size('vg_grad_guard_ws_bytes', 0 if g32 is None else g32.numel(), 0 if g64 is None else g64.numel())
    return torch.empty(n // 8, dtype=torch.float64, device=ref.device)


def grad_guard_(g32, g64, max_norm, skip_nonfinite, ws, state):
    """Global norm of the two flat gradient buffers -> state = double[8] on the device: total_norm, clip scale, apply flag and the
    running counters.  max_norm None / <= 0: clipping off (scale 1).  Two launches, nothing comes back to the host."""
    ref = g32 if g32 is not None else g64
    if g32 is not None:
        _chk(g32, torch.float32)
    if g64 is not None:
        _chk(g64, torch.float64)
    assert state.numel() == GUARD_STATE_LEN
    _call(ref, 'vg_grad_guard', _p(g32), 0 if g32 is None else g32.numel(), _p(g64), 0 if g64 is None else g64.numel(),
          float(max_norm) if max_norm else 0.0, int(bool(skip_nonfinite)), _p(_chk(ws, torch.float64)), _p(_chk(state, torch.float64)))


def adam_advance_guarded_(state, lr, b1, b2, guard):
    """adam_advance_ that leaves t and the scalars alone when the guard's apply flag is 0."""
    _call(state, 'vg_adam_advance_guarded', _p(_chk(state, torch.float64)), float(lr), float(b1), float(b2),
          _p(_chk(guard, torch.float64)))


def adam_step_guarded_(p, g, m, v, b1, b2, eps, step_scalars, guard):
    """adam_step_ on g * scale; touches nothing when the guard's apply flag is 0.  g itself is left unscaled."""
    _adam_step('vg_adam_step_guarded', p, g, m, v, b1, b2, eps, step_scalars, guard)


# --------------------------------------------------------------------------- device-resident input path (include/vaegam.h)
def volume_gather(arena, files, row_file, row_vol, idx, shape, dtype, divisor, out=None):
    """x (B, X, Y, Z) fp32 = the volumes of data-set rows idx (int64, B of them), read from the raw file payloads in `arena` (uint8)
    through the descriptor table `files` (DataClass_GP.ResidentVolumes builds both) and divided by `divisor`.  dtype: the NIfTI code
    every file shares, or 0.  The caller has validated idx, row_file and row_vol: the kernel clamps nothing."""
    _chk(arena, torch.uint8); _chk(files, torch.uint8); _chk(row_file, torch.int32); _chk(row_vol, torch.int32); _chk(idx, torch.int64)
    assert files.ndim == 2 and files.shape[1] == ctypes.sizeof(_lib.VolFile), 'descriptor table does not match vg_vol_file'
    assert idx.ndim == 1 and idx.device == arena.device
    B, (X, Y, Z) = idx.numel(), shape
    if out is None:
        out = torch.empty((B, X, Y, Z), dtype=torch.float32, device=arena.device)
    assert tuple(out.shape) == (B, X, Y, Z)
    _call(arena, 'vg_volume_gather', _p(arena), _p(files), _p(row_file), _p(row_vol), _p(idx), B, X, Y, Z, int(dtype), float(divisor),
          _p(_chk(out)))
    return out


# --------------------------------------------------------------------------- matrix-core convolution (vg_conv_mm; plans: conv_mm_plan.py)
USE_MM = int(_os.environ.get('VG_CONV_MM', '1'))            # 0: off; 1: where it measured faster (mm_wins); 2: wherever a plan exists


def conv_mm(x, plan: MmPlan, aimg, bias, relu_in, scale, shift, per_group, mask_src=None, next_bn=None, relu_out=False, stats_like=None):
    """One vg_conv_mm launch: x [N][CI][...] -> y [N][CO][OD][OH][OW] (pre-activation; rectified with relu_out); with next_bn also
    the statistics partials.  stats_like = the ConvSpec of a stride-2 transposed conv: the partials are then taken from y by
    vg_tconv3d_s2_stats_of, in the layout and summation order of the register-tiled engine's fused launch, instead of in the
    epilogue: y is the same bit for bit on either engine, the epilogue's own partials are not (a lane sums other elements), and with
    this the consuming batch norm -- and so the step -- computes exactly what it computes on the register-tiled kernel."""
    lib = _lib.get_lib()
    N = x.shape[0]
    assert tuple(x.shape[1:]) == (plan.CI, plan.ID, plan.IH, plan.IW), (tuple(x.shape), plan.CI, plan.ID, plan.IH, plan.IW)
    tau, dlt, _ = plan.tables(x.device)
    d = plan.desc(N, relu_in, per_group if scale is not None else 1, relu_out)
    y = torch.empty((N, plan.CO, plan.OD, plan.OH, plan.OW), dtype=torch.float32, device=x.device)
    _chk(x); _chk(aimg)
    part, stats = None, (1, 0, None)                         # (statistics per_group, statistics on, partials) of the epilogue
    if next_bn and stats_like is None:
        chunks = lib.size('vg_conv_mm_stats_chunks', ctypes.byref(d), int(next_bn))
        part = torch.zeros((N // int(next_bn)) * plan.CO * chunks * 2, dtype=torch.float64, device=x.device)
        stats = (int(next_bn), 1, _p(part))
    _call(x, 'vg_conv_mm', ctypes.byref(d), _p(x), _p(aimg), _p(tau), _p(dlt), _p(bias), _p(scale), _p(shift), _p(mask_src), _p(y), *stats)
    if not next_bn:
        return y
    if stats_like is not None:
        _, cd, osz = conv_fwd_desc(stats_like, N, (plan.ID, plan.IH, plan.IW), relu_in, per_group if scale is not None else 1, relu_out)
        assert tuple(osz) == (plan.OD, plan.OH, plan.OW) and stats_like.co == plan.CO
        chunks = lib.size('vg_tconv3d_s2_stats_chunks', ctypes.byref(cd), int(next_bn))
        part = torch.empty((N // int(next_bn)) * plan.CO * chunks * 2, dtype=torch.float64, device=x.device)
        _call(x, 'vg_tconv3d_s2_stats_of', ctypes.byref(cd), _p(y), int(next_bn), 1, _p(part))
    return y, part
