"""Shared bodies of the fully connected engine tests (vg_fc.hip: vg_fc_gemm, vg_fc_gemm_jobs, vg_fc_plan): every body
fc_body<W, a_vec, b_vec> of both tile sizes, the job mixes of one launch and the split-K reduction against a float64 einsum, one case
per class of the launch plan (`ops.fc_plan`).  Run on CPU tensors through the host build of the kernels (tests/test_fc_emu.py) and on
the GPU through libvaegam_hip.so (tests/test_fc_gpu.py).  Every case first asserts the plan it was written for, then runs.

Inputs: every operand, mask, bias and prefill element is +-m, m uniform in [0.5, 1.5] with a random sign (seeded), so every unmasked
term of every dot product is at least 0.25 in magnitude: a dropped, doubled or misplaced element cannot hide in rounding.  The sign of
a mask element decides it (about half are open).

Tolerance, per element, derived and never measured from the kernel.  u = 2^-24; A', B' the operands after ReLU / mask;
S = |A'| . |B'| in float64 (for the ones column Sx = sum_k |A'|).  Any order of an fp32 dot product of K terms obeys
|err| <= lambda sqrt(K) u S with probability >= 1 - 2 K exp(-lambda^2 / 2) per element (Higham & Mary 2019); with lambda = 8 the chance
that any of the ~1e7 elements checked here exceeds it is below 1e-6.  Split-K sums ksplit partials in fp32: one more order of the same
K terms, inside the bound.
    tol = 8 sqrt(K) u S + 2 u |want|  + 2 u (|want| + |bias|)     [VG_FC_C_BIAS]
                                      + 2 u (|want| + |prefill|)  [VG_FC_C_ACCUM]
(want = the expected final value).  Each case asserts tol.max() < 0.0625, a quarter of the smallest term, on the reference alone.
Every check prints err, tol, err / tol and err / d32 before it asserts; d32 = the error of the same product in plain fp32 torch on the
CPU.

Guards, all torch.equal: C's pitch gaps, batch gaps and an 8-element tail hold 777.0 before and after (C_ACCUM included); cx is
untouched without VG_FC_B_ONES (its gaps and tail with it); the test owns the split-K workspace, vg_fc_ws_bytes long plus 64 canaries
that must be intact.  Operand, mask and output-mask gaps hold NaN: a gap element that reached a result would show there (a mask gap
closes the mask: a dropped term).

Limit: the float64 matrix does not detect out-of-bounds READS (a stray read whose value is then discarded leaves no trace in any
result), and no sanitizer run is part of it.  The clamps of fetch() only ever decide such reads (k clamped to the last index, the
form-2 row group clamped to M - 4), so on the host build alone run_guarded() repeats a few cases in a child process with every input
buffer ending at a page that may not be read: a load past the END of an operand ends that process.  Reads before an operand's
start or into its gaps stay undetected, as does everything of this kind on the GPU."""
import ctypes
import math
import mmap

import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops

U = 2.0 ** -24
LAMBDA = 8.0
GUARD = 777.0
TAIL = 8
CANARIES = 64
VG_ERR_ARG = 1


def _s(M, N, K, a, b, flags=(), **kw):
    """M x N x K, layout of A ('k': k-contiguous, 'm': m-contiguous) and of B ('k' / 'n'), flags without the VG_FC_ prefix.
    kw: batch, ksplit; a_pad / b_pad / c_pad (elements added to the row pitch), a_bgap / b_bgap / c_bgap (added to the batch pitch),
    a_off / m_off (elements the A / mask pointer sits inside its aligned buffer), a_str / b_str / c_str (explicit strides as
    ops.fc_job takes them), bias_sb, cx_sb."""
    return dict(M=M, N=N, K=K, a=a, b=b, flags=tuple(flags), **kw)


# id: (spec, (tile, a_vec, b_vec)) -- the expected plan is a hand evaluation of fc_prepare, asserted through ops.fc_plan
CLASS_CASES = {
    't32-00': (_s(37, 45, 70, 'k', 'k', ('C_BIAS', 'C_RELU')), (32, 0, 0)),
    't32-01': (_s(40, 36, 132, 'k', 'k', ('A_RELU', 'C_BIAS'), a_pad=1), (32, 0, 1)),                    # A's row pitch K + 1
    't32-02': (_s(34, 44, 65, 'm', 'n', ('A_MASK', 'B_ONES', 'C_ACCUM')), (32, 0, 2)),
    't32-10': (_s(33, 35, 128, 'k', 'n', ('A_MASK', 'C_MASK')), (32, 1, 0)),
    't32-11': (_s(40, 50, 300, 'k', 'k', ('C_BIAS', 'C_RELU', 'C_ACCUM'), ksplit=3), (32, 1, 1)),       # last piece 44
    't32-12': (_s(40, 36, 128, 'k', 'n', ('A_MASK', 'C_MASK', 'C_ACCUM'), c_pad=3), (32, 1, 2)),        # C's pitch N + 3
    't32-20': (_s(36, 33, 70, 'm', 'n', ('B_ONES', 'B_RELU')), (32, 2, 0)),
    't32-21': (_s(36, 40, 68, 'm', 'k', ('A_RELU', 'B_ONES', 'C_ACCUM')), (32, 2, 1)),
    't32-22': (_s(68, 36, 257, 'm', 'n', ('A_MASK', 'B_ONES', 'C_ACCUM'), ksplit=3), (32, 2, 2)),       # last piece 1
    't64-00': (_s(250, 371, 501, 'k', 'k', ('C_BIAS',), ksplit=8), (64, 0, 0)),                         # 8 x 12 tiles x 8 pieces = 768
    't64-11': (_s(250, 370, 500, 'k', 'k', ('A_RELU', 'C_BIAS', 'C_RELU'), ksplit=8), (64, 1, 1)),      # last piece 52
    't64-22': (_s(500, 504, 70, 'm', 'n', ('A_MASK', 'B_ONES', 'C_ACCUM'), batch=3), (64, 2, 2)),       # 16 x 16 tiles x 3 products
    't64-02': (_s(738, 1000, 66, 'm', 'n', ('B_RELU',)), (64, 0, 2)),                                   # 24 x 32 tiles
    't64-20': (_s(740, 1001, 66, 'm', 'n', ('B_ONES',)), (64, 2, 0)),
    't64-10': (_s(737, 993, 68, 'k', 'n', ('A_MASK', 'C_MASK')), (64, 1, 0)),
    't64-01': (_s(737, 996, 68, 'k', 'k', ('C_BIAS',), a_pad=1), (64, 0, 1)),
    't64-21': (_s(740, 996, 68, 'm', 'k', ('B_ONES', 'C_ACCUM')), (64, 2, 1)),
    't64-12': (_s(737, 996, 132, 'k', 'n', ('A_MASK',)), (64, 1, 2)),
}
# classes a train step launches (kernel_cases.fc_production_plans) that the 18 above reach only split, or only whole
PRODUCTION_CASES = {
    # fc8's data gradient at small batches: split-K with the weights read across rows; also VG_FC_C_MASK in fc_store on a pitched C
    't32-12-split': (_s(40, 36, 260, 'k', 'n', ('A_MASK', 'C_MASK'), ksplit=3, c_pad=3), (32, 1, 2)),   # last piece 4
    't32-22-whole': (_s(36, 40, 70, 'm', 'n', ('A_MASK', 'B_ONES', 'C_ACCUM')), (32, 2, 2)),            # a weight gradient, not split
    't64-11-whole': (_s(737, 996, 68, 'k', 'k', ('C_BIAS',)), (64, 1, 1)),                              # fc8 forward
    't64-12-split': (_s(250, 372, 500, 'k', 'n', ('A_MASK',), ksplit=8), (64, 1, 2)),                   # fc8's data gradient
    't64-22-whole': (_s(740, 996, 66, 'm', 'n', ('B_ONES', 'C_ACCUM')), (64, 2, 2)),                    # fc8's weight gradient
}
# all at 32 x 32
EXTRA_CASES = {
    'a-ptr+1': (_s(36, 40, 64, 'k', 'k', ('C_BIAS',), a_off=1), (32, 0, 1)),             # A one element into its buffer: form 0 by alignment
    'mask-ptr+2': (_s(36, 40, 64, 'm', 'n', ('A_MASK',), m_off=2), (32, 0, 2)),          # the mask pointer alone misaligned
    # the heads' forward: three products read interleaved column blocks of one [B][3H] buffer (a_sm = 3H > K, a_sb = H = 50)
    'heads-fwd': (_s(9, 32, 50, 'k', 'k', ('C_BIAS',), batch=3, a_str=(150, 1, 50)), (32, 0, 0)),
    # a batch pitch with a gap of 2 (a_sb % 4 != 0: form 0 by stride); c_sb leaves guard elements between the products
    'batch-gap': (_s(12, 20, 36, 'k', 'n', ('C_ACCUM',), batch=3, a_bgap=2, c_bgap=2), (32, 0, 2)),
    'k1': (_s(3, 2, 1, 'k', 'k'), (32, 0, 0)),                                           # one reduction index: one real step of two
    'k64-inside': (_s(32, 32, 64, 'k', 'k'), (32, 1, 1)),                                # every tile `inside`, K one whole step: the fast put only
    'k192': (_s(64, 31, 192, 'm', 'n', ('B_ONES',)), (32, 2, 0)),                        # three steps, rounded up to four
    # the heads' backward (HeadsAct.backward): the data gradient writes three products interleaved into one [B][3H] buffer
    # (c_sm = 3H > N: a write one column past N lands in a neighbour's output), the weight gradient reads that layout
    'heads-dgrad': (_s(9, 50, 32, 'k', 'n', (), batch=3, c_str=(150, 50)), (32, 1, 0)),
    'heads-wgrad': (_s(32, 50, 9, 'm', 'n', ('B_ONES', 'C_ACCUM'), batch=3, b_str=(150, 1, 50), cx_sb=32), (32, 2, 0)),
}
SINGLE_CASES = dict(CLASS_CASES); SINGLE_CASES.update(PRODUCTION_CASES); SINGLE_CASES.update(EXTRA_CASES)
# id: (jobs, tile of the joint launch, the jobs whose joint result must equal their single-job result bit for bit)
MIX_CASES = {
    # fc_reduce_k skips the unsplit jobs, first[] dispatch across four jobs, another body per job
    'four-small': (('t32-10', 't32-22', 't32-00', 't32-11'), 32, ('t32-10', 't32-22', 't32-00', 't32-11')),
    # a job voting 64 x 64 with one that does not: both run 32 x 32, the big job's gx / gy recomputed
    'vote-mixed': (('t64-11', 't32-21'), 32, ('t32-21',)),
    # fc8's backward: two jobs voting 64 x 64, one split and one batched
    'two-big': (('t64-11', 't64-22'), 64, ('t64-11', 't64-22')),
    # a layer's backward without split-K, here the heads': two batched jobs, no reduction launch
    'two-unsplit': (('heads-dgrad', 'heads-wgrad'), 32, ('heads-dgrad', 'heads-wgrad')),
}
# the host build walks a 64 x 64 case in 2 to 5 s: with all of them the host file ran over a minute, so the six that are not (0,0), (1,1)
# or (2,2) run on the GPU only (the same bodies run at 32 x 32 on the host build, and 64 x 64 itself with the other nine cases)
GPU_ONLY = ('t64-02', 't64-20', 't64-10', 't64-01', 't64-21', 't64-12')
HOST_SINGLE = tuple(c for c in SINGLE_CASES if c not in GPU_ONLY)

RECORDS = []                                            # (what, quantity, err / tol, err / d32) of every check made in this process


def _check(what, qty, err, tol, d32):
    err = torch.as_tensor(err, dtype=torch.float64)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    assert bool(torch.isfinite(err).all()), '%s %s: not finite (a gap element reached the result, or a NaN was computed)' % (what, qty)
    i = int((err / tol).argmax())
    e, t = float(err.reshape(-1)[i]), float(tol.reshape(-1)[i])
    emax = float(err.max())
    rd = emax / d32 if d32 > 0 else float('inf') if emax > 0 else 0.0
    print('fc %s %s: err %.3g tol %.3g err/tol %.3g d32 %.3g err/d32 %.3g' % (what, qty, e, t, e / t, d32, rd))
    RECORDS.append((what, qty, e / t, rd))
    assert e <= t, '%s %s: error %.3g > tolerance %.3g (d32 %.3g)' % (what, qty, e, t, d32)


# ---------------------------------------------------------------------------------------------------------------- layout
def _layout(sp):
    """-> dict of strides: a = (sm, sk, sb), b = (sk, sn, sb), c = (sm, sb), bias_sb, cx_sb"""
    M, N, K = sp['M'], sp['N'], sp['K']
    if 'a_str' in sp:
        a = sp['a_str']
    elif sp['a'] == 'k':
        sm = K + sp.get('a_pad', 0); a = (sm, 1, M * sm + sp.get('a_bgap', 0))
    else:
        sk = M + sp.get('a_pad', 0); a = (1, sk, K * sk + sp.get('a_bgap', 0))
    if 'b_str' in sp:
        b = sp['b_str']
    elif sp['b'] == 'k':
        sn = K + sp.get('b_pad', 0); b = (1, sn, N * sn + sp.get('b_bgap', 0))
    else:
        sk = N + sp.get('b_pad', 0); b = (sk, 1, K * sk + sp.get('b_bgap', 0))
    if 'c_str' in sp:
        c = sp['c_str']
    else:
        sm = N + sp.get('c_pad', 0); c = (sm, M * sm + sp.get('c_bgap', 0))
    batch = sp.get('batch', 1)
    return dict(a=a, b=b, c=c, bias_sb=sp.get('bias_sb', N + (1 if batch > 1 else 0)), cx_sb=sp.get('cx_sb', M + (2 if batch > 1 else 0)))


def _extent(shape, strides):
    return 1 + sum((n - 1) * s for n, s in zip(shape, strides))


def _pm(shape, g):
    m = 0.5 + torch.rand(shape, generator=g)
    return m * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


_HOST = {}


def host(cid):
    """The case's operands and its float64 reference, computed once and shared (read-only) by every test that runs the case."""
    if cid in _HOST:
        return _HOST[cid]
    sp = SINGLE_CASES[cid][0]
    M, N, K, z, fl = sp['M'], sp['N'], sp['K'], sp.get('batch', 1), sp['flags']
    g = torch.Generator().manual_seed(4000 + list(SINGLE_CASES).index(cid))
    h = dict(A=_pm((z, M, K), g), B=_pm((z, K, N), g), amask=_pm((z, M, K), g), cmask=_pm((z, M, N), g), bias=_pm((z, N), g),
             C0=_pm((z, M, N), g), cx0=_pm((z, M), g))

    def ref(dt):
        Ae = h['A'].to(dt)
        if 'A_RELU' in fl: Ae = Ae.clamp_min(0)
        if 'A_MASK' in fl: Ae = Ae * (h['amask'] > 0)
        Be = h['B'].to(dt)
        if 'B_RELU' in fl: Be = Be.clamp_min(0)
        w = torch.einsum('zmk,zkn->zmn', Ae, Be)
        if 'C_BIAS' in fl: w = w + h['bias'].to(dt)[:, None, :]
        if 'C_RELU' in fl: w = w.clamp_min(0)
        if 'C_MASK' in fl: w = w * (h['cmask'] > 0)
        wx = Ae.sum(2)
        if 'C_ACCUM' in fl: w = w + h['C0'].to(dt); wx = wx + h['cx0'].to(dt)
        return Ae, Be, w, wx
    Ae, Be, want, wx = ref(torch.float64)
    _, _, w32, wx32 = ref(torch.float32)
    S = torch.einsum('zmk,zkn->zmn', Ae.abs(), Be.abs()); Sx = Ae.abs().sum(2)
    g8 = LAMBDA * math.sqrt(K) * U
    tol = g8 * S + 2 * U * want.abs(); tolx = g8 * Sx + 2 * U * wx.abs()
    if 'C_BIAS' in fl: tol = tol + 2 * U * (want.abs() + h['bias'].double().abs()[:, None, :])
    if 'C_ACCUM' in fl:
        tol = tol + 2 * U * (want.abs() + h['C0'].double().abs()); tolx = tolx + 2 * U * (wx.abs() + h['cx0'].double().abs())
    h.update(want=want, wx=wx, tol=tol, tolx=tolx, d32=float((w32.double() - want).abs().max()), d32x=float((wx32.double() - wx).abs().max()))
    # the condition of the case, on the reference alone: the bound is a quarter of the smallest term
    assert float(tol.max()) < 0.0625 and float(tolx.max()) < 0.0625, '%s: tol.max() %.3g' % (cid, max(float(tol.max()), float(tolx.max())))
    _HOST[cid] = h
    return h


class Job:
    """One case's buffers on `dev` (fresh at every construction) and its ops.fc_job."""

    def __init__(self, dev, cid, guarded=False):
        sp = SINGLE_CASES[cid][0]
        self.cid, self.sp, self.h = cid, sp, host(cid)
        h, L = self.h, _layout(sp)
        M, N, K, z = sp['M'], sp['N'], sp['K'], sp.get('batch', 1)
        self.ksplit = sp.get('ksplit', 1); self.batch = z
        fl = 0
        for f in sp['flags']:
            fl |= getattr(_lib, 'FC_' + f)
        nan = float('nan')

        self.keep = []

        def place(vals, strides, off, fill, tail=0):
            if guarded and tail == 0:                                   # an input: its last element is the last of a readable page
                assert off == 0 and dev == 'cpu'
                buf, mm = _guarded_buffer(_extent(vals.shape, strides)); buf.fill_(fill); self.keep.append(mm)
            else:
                buf = torch.full((off + _extent(vals.shape, strides) + tail,), fill)
            torch.as_strided(buf, vals.shape, strides, off).copy_(vals)
            return buf
        a_str = (L['a'][2], L['a'][0], L['a'][1])                      # of the [z][m][k] view
        b_str = (L['b'][2], L['b'][0], L['b'][1])                      # of the [z][k][n] view
        self.c_str = (L['c'][1], L['c'][0], 1)
        self.cx_str = (L['cx_sb'], 1)
        a_off, m_off = sp.get('a_off', 0), sp.get('m_off', 0)
        self.Abuf = place(h['A'], a_str, a_off, nan).to(dev)
        self.Mbuf = place(h['amask'], a_str, m_off, nan).to(dev)
        self.Bbuf = place(h['B'], b_str, 0, nan).to(dev)
        self.cmbuf = place(h['cmask'], self.c_str, 0, nan).to(dev)
        self.biasbuf = place(h['bias'], (L['bias_sb'], 1), 0, nan).to(dev)
        self.C_before = place(h['C0'], self.c_str, 0, GUARD, TAIL)
        self.cx_before = place(h['cx0'], self.cx_str, 0, GUARD, TAIL)
        self.Cbuf = self.C_before.to(dev); self.cxbuf = self.cx_before.to(dev)
        for t in (self.Abuf, self.Mbuf, self.Bbuf, self.Cbuf):
            assert guarded or t.data_ptr() % 16 == 0, 'the allocator is expected to hand out 16-byte aligned buffers'
        d = _lib.FcDesc(M, N, K, z, *L['a'], *L['b'], *L['c'], L['bias_sb'], L['cx_sb'], self.ksplit, fl)
        self.ws_len = _lib.get_lib().size('vg_fc_ws_bytes', ctypes.byref(d)) // 4
        self.ws = torch.full((self.ws_len + CANARIES,), GUARD, device=dev)
        self.job = ops.fc_job(self.Abuf[a_off:], self.Bbuf, self.Cbuf, M, N, K, L['a'], L['b'], L['c'], fl, batch=z, bias=self.biasbuf,
                              bias_sb=L['bias_sb'], amask=self.Mbuf[m_off:], cmask=self.cmbuf, cx=self.cxbuf, cx_sb=L['cx_sb'],
                              ksplit=self.ksplit, ws=self.ws)
        assert self.job[0].ws == self.ws.data_ptr()

    def fetch(self):
        """-> (whole C buffer, whole cx buffer) on the CPU, after the guards"""
        C, cx, ws = self.Cbuf.cpu(), self.cxbuf.cpu(), self.ws.cpu()
        cid, h = self.cid, self.h
        assert torch.equal(ws[self.ws_len:], torch.full((CANARIES,), GUARD)), cid + ': wrote past the split-K workspace'
        g = C.clone(); torch.as_strided(g, h['C0'].shape, self.c_str, 0).fill_(GUARD)
        assert torch.equal(g, torch.full_like(g, GUARD)), cid + ': C written outside its M x N products (pitch gap, batch gap or tail)'
        if 'B_ONES' in self.sp['flags']:
            g = cx.clone(); torch.as_strided(g, h['cx0'].shape, self.cx_str, 0).fill_(GUARD)
            assert torch.equal(g, torch.full_like(g, GUARD)), cid + ': cx written outside its M sums'
        else:
            assert torch.equal(cx, self.cx_before), cid + ': cx touched without VG_FC_B_ONES'
        return C, cx

    def check(self, what, C, cx):
        h = self.h
        got = torch.as_strided(C, h['C0'].shape, self.c_str, 0).double()
        _check(what, 'C', (got - h['want']).abs(), h['tol'], h['d32'])
        if 'B_ONES' in self.sp['flags']:
            gx = torch.as_strided(cx, h['cx0'].shape, self.cx_str, 0).double()
            _check(what, 'cx', (gx - h['wx']).abs(), h['tolx'], h['d32x'])


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def single_plan(job):
    """The plan of the job alone, with what the case is there for asserted."""
    cid = job.cid
    tile, av, bv = SINGLE_CASES[cid][1]
    plan = ops.fc_plan([job.job])
    j = plan['jobs'][0]
    got = (plan['tile'], j['a_vec'], j['b_vec'])
    assert got == (tile, av, bv), '%s: plan %r, the case is there for %r' % (cid, got, (tile, av, bv))
    sp = job.sp
    NW = sp['N'] + (1 if 'B_ONES' in sp['flags'] else 0)
    assert plan['njobs'] == 1 and j['big'] == int(tile == 64) and j['first'] == 0
    assert (j['gx'], j['gy']) == (-(-sp['M'] // tile), -(-NW // tile)), (cid, j)
    assert j['blocks'] == plan['grid'] == j['gx'] * j['gy'] * (job.ksplit if job.ksplit > 1 else job.batch), (cid, plan)
    if job.ksplit > 1:
        kchunk = -(-(-(-sp['K'] // job.ksplit)) // 64) * 64
        assert j['kchunk'] == kchunk and plan['reduce_blocks'] == min(1024, -(-(sp['M'] * (sp['N'] + 1)) // 256)), (cid, plan)
    else:
        assert plan['reduce_blocks'] == 0, (cid, plan)
    return plan


_SINGLE = {}


def run_single(dev, cid):
    """Plan, launch alone, guards, float64 check; split cases run twice and must repeat bit for bit.  -> (C, cx) buffers on the CPU,
    kept per device for the job-mix cases."""
    if (dev, cid) in _SINGLE:
        return _SINGLE[(dev, cid)]
    job = Job(dev, cid)
    single_plan(job)
    ops.fc_launch(job.Cbuf, [job.job]); _sync(dev)
    C, cx = job.fetch()
    job.check(cid, C, cx)
    if job.ksplit > 1:
        again = Job(dev, cid)
        ops.fc_launch(again.Cbuf, [again.job]); _sync(dev)
        C2, cx2 = again.fetch()
        assert torch.equal(C, C2) and torch.equal(cx, cx2), cid + ': a split-K product did not repeat bit for bit'
    _SINGLE[(dev, cid)] = (C, cx)
    return C, cx


def run_mix(dev, mid):
    cids, tile, same = MIX_CASES[mid]
    jobs = [Job(dev, c) for c in cids]
    plan = ops.fc_plan([j.job for j in jobs])
    alone = [ops.fc_plan([j.job]) for j in jobs]
    votes = [p['jobs'][0]['big'] for p in alone]
    assert plan['tile'] == tile and plan['njobs'] == len(jobs), '%s: plan %r, the case is there for tile %d' % (mid, plan, tile)
    assert tile == (64 if all(votes) else 32)
    first = 0
    for job, pj, pa, v in zip(jobs, plan['jobs'], alone, votes):
        sp = job.sp
        NW = sp['N'] + (1 if 'B_ONES' in sp['flags'] else 0)
        assert (pj['a_vec'], pj['b_vec'], pj['big'], pj['kchunk']) == tuple(pa['jobs'][0][k] for k in ('a_vec', 'b_vec', 'big', 'kchunk'))
        assert (pj['gx'], pj['gy']) == (-(-sp['M'] // tile), -(-NW // tile)), '%s %s: gx, gy %r at tile %d' % (mid, job.cid, pj, tile)
        assert pj['first'] == first and pj['blocks'] == pj['gx'] * pj['gy'] * (job.ksplit if job.ksplit > 1 else job.batch)
        first += pj['blocks']
    assert plan['grid'] == first
    split = [j for j in jobs if j.ksplit > 1]
    assert plan['reduce_blocks'] == (min(1024, max(-(-(j.sp['M'] * (j.sp['N'] + 1)) // 256) for j in split)) if split else 0)
    assert tuple(j.cid for j, pa in zip(jobs, alone) if pa['tile'] == tile) == same, '%s: jobs that keep their tile' % mid
    ops.fc_launch(jobs[0].Cbuf, [j.job for j in jobs]); _sync(dev)
    outs = [j.fetch() for j in jobs]
    for job, (C, cx) in zip(jobs, outs):
        job.check('%s/%s' % (mid, job.cid), C, cx)
    if split:
        rerun = [Job(dev, c) for c in cids]
        ops.fc_launch(rerun[0].Cbuf, [j.job for j in rerun]); _sync(dev)
        for job, (C, cx) in zip(rerun, outs):
            C2, cx2 = job.fetch()
            assert torch.equal(C, C2) and torch.equal(cx, cx2), '%s/%s: did not repeat bit for bit' % (mid, job.cid)
    for job, (C, cx) in zip(jobs, outs):
        if job.cid in same:                                          # same body, same order: the same bits as the job alone
            Cs, cxs = run_single(dev, job.cid)
            assert torch.equal(C, Cs) and torch.equal(cx, cxs), '%s/%s: differs from the single-job launch' % (mid, job.cid)


# ---------------------------------------------------------------------------------------------------------------- reads past the end
# form 0 on both operands with a partial last step; form 2 on both with a ragged row tile and a partial last step; form 1 split;
# form 2 against form 1
GUARDED_CASES = ('t32-00', 't32-22-whole', 't32-11', 't32-21')


def _guarded_buffer(n):
    """-> (float32 tensor of n elements whose last element ends a page, the mapping that owns it); the page behind it is PROT_NONE"""
    page = mmap.PAGESIZE
    pages = -(-(4 * n) // page)
    mm = mmap.mmap(-1, (pages + 1) * page)
    addr = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(addr + pages * page, page, 0) == 0, 'mprotect: errno %d' % ctypes.get_errno()
    return torch.frombuffer(mm, dtype=torch.float32, count=n, offset=pages * page - 4 * n), mm


def run_guarded():
    """Host build only, in a process of its own (tests/test_fc_emu.py starts it): GUARDED_CASES with A, its mask, B, the bias and the
    output mask each ending at an unreadable page.  The plan must still be the case's (the buffers keep their alignment class), the
    result its float64 reference."""
    import emu_inject
    emu_inject.inject_emu()
    for cid in GUARDED_CASES:
        print('fc guarded %s' % cid, flush=True)
        job = Job('cpu', cid, guarded=True)
        single_plan(job)
        ops.fc_launch(job.Cbuf, [job.job])
        C, cx = job.fetch()
        job.check(cid + ' guarded', C, cx)
    print('fc guarded: done', flush=True)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _raw(jobs):
    return (_lib.FcJob * max(len(jobs), 1))(*[j[0] for j in jobs])


def refusal_cases(dev):
    """-> [(what, jobs, fragment of the expected text)]"""
    t = lambda *s: torch.ones(s, device=dev)
    A, B, C, v = t(8, 200), t(200, 8), t(8, 8), t(8)
    ok = lambda **kw: ops.fc_job(A, B, C, 8, 8, 8, (8, 1, 0), (8, 1, 0), (8, 0), **kw)
    nows = ops.fc_job(A, B, C, 8, 8, 200, (200, 1, 0), (8, 1, 0), (8, 0), ksplit=2)
    nows = (_lib.FcJob(nows[0].d, nows[0].A, None, nows[0].B, None, None, nows[0].C, None, None), nows[1])
    return [
        ('no jobs', [], '1..4 jobs'),
        ('five jobs', [ok()] * 5, '1..4 jobs'),
        ('A: both strides != 1', [ops.fc_job(A, B, C, 8, 8, 8, (16, 2, 0), (8, 1, 0), (8, 0))], 'one stride of each operand'),
        ('B: both strides != 1', [ops.fc_job(A, B, C, 8, 8, 8, (8, 1, 0), (16, 2, 0), (8, 0))], 'one stride of each operand'),
        ('split and batch', [ops.fc_job(A, B, C, 2, 2, 128, (128, 1, 256), (2, 1, 256), (2, 4), batch=2, ksplit=2)], 'exclude each other'),
        ('C_MASK with B_ONES', [ok(flags=_lib.FC_C_MASK | _lib.FC_B_ONES, cmask=C, cx=v)], 'VG_FC_C_MASK and VG_FC_B_ONES'),
        ('A_MASK without a mask', [ok(flags=_lib.FC_A_MASK)], 'buffer is null'),
        ('C_BIAS without a bias', [ok(flags=_lib.FC_C_BIAS)], 'buffer is null'),
        ('B_ONES without cx', [ok(flags=_lib.FC_B_ONES)], 'buffer is null'),
        ('split without a workspace', [nows], 'buffer is null'),
        ('empty piece', [ops.fc_job(A, B, C, 8, 8, 200, (200, 1, 0), (8, 1, 0), (8, 0), ksplit=3)], 'ksplit=3 leaves an empty piece of K=200'),
        ('second job refused', [ok(), ok(flags=_lib.FC_C_BIAS)], 'buffer is null'),
    ]


def run_refusals(dev):
    """The plan query and the launcher answer alike, in status and in text; a short record is VG_ERR_ARG."""
    dll = _lib.get_lib().dll
    rec = (ctypes.c_int32 * _lib.FC_PLAN_LEN)()
    stream = ops._stream(torch.ones(1, device=dev))
    good = refusal_cases(dev)[1][1][:1]
    assert dll.vg_fc_plan(_raw(good), 1, rec, _lib.FC_PLAN_LEN) == 0
    for n_out in (0, _lib.FC_PLAN_LEN - 1):
        assert dll.vg_fc_plan(_raw(good), 1, rec, n_out) == VG_ERR_ARG
        short = dll.vg_last_error().decode()
        assert 'vg_fc_plan' in short
    assert dll.vg_fc_plan(_raw(good), 1, None, _lib.FC_PLAN_LEN) == VG_ERR_ARG
    for what, jobs, frag in refusal_cases(dev):
        arr = _raw(jobs)
        rc_p = dll.vg_fc_plan(arr, len(jobs), rec, _lib.FC_PLAN_LEN)
        text_p = dll.vg_last_error().decode()
        assert dll.vg_fc_plan(_raw(good), 1, rec, 0) == VG_ERR_ARG and dll.vg_last_error().decode() == short    # another text in between
        rc_l = dll.vg_fc_gemm_jobs(arr, len(jobs), stream)
        text_l = dll.vg_last_error().decode()
        print('fc refusal %s: status %d / %d, "%s"' % (what, rc_p, rc_l, text_l))
        assert rc_p == rc_l == VG_ERR_ARG, what
        assert text_p == text_l and frag in text_l, (what, text_p, text_l)
        try:
            ops.fc_plan(jobs)
        except _lib.VgError as e:
            assert frag in str(e)
        else:
            raise AssertionError(what + ': ops.fc_plan did not raise')
    _sync(dev)


# ---------------------------------------------------------------------------------------------------------------- coverage
def launch_class(plan, descs):
    """-> ({(tile, a_vec, b_vec, split, batched) per job}, (jobs, any split, votes differ)); descs: (ksplit, batch) per job"""
    jobs = {(plan['tile'], j['a_vec'], j['b_vec'], ks > 1, bt > 1) for j, (ks, bt) in zip(plan['jobs'], descs)}
    return jobs, (plan['njobs'], any(ks > 1 for ks, _ in descs), len({j['big'] for j in plan['jobs']}) > 1)


def case_classes():
    """-> {case id: (job classes, mix signature)} from the plans of every listed case (nothing is launched)"""
    out = {}
    for cid in SINGLE_CASES:
        j = Job('cpu', cid)
        out[cid] = launch_class(ops.fc_plan([j.job]), [(j.ksplit, j.batch)])
    for mid, (cids, _, _) in MIX_CASES.items():
        js = [Job('cpu', c) for c in cids]
        out[mid] = launch_class(ops.fc_plan([j.job for j in js]), [(j.ksplit, j.batch) for j in js])
    return out


def check_coverage():
    """Every job class and every job-mix signature that a production launch falls in (kernel_cases.fc_production_plans) is reached by
    a listed case; names the ones that are not, and the ones only GPU-only cases reach."""
    import kernel_cases as K
    cases = case_classes()
    prod_jobs, prod_mix = {}, {}
    for what, plan, descs in K.fc_production_plans():
        jobs, mix = launch_class(plan, descs)
        for c in jobs:
            prod_jobs.setdefault(c, []).append(what)
        prod_mix.setdefault(mix, []).append(what)
    missing, gpu_only = [], []
    for kind, prod, pick in (('job class (tile, a_vec, b_vec, split, batched)', prod_jobs, lambda cl, key: key in cl[0]),
                             ('job mix (jobs, any split, votes differ)', prod_mix, lambda cl, key: key == cl[1])):
        for key in sorted(prod):
            by = [cid for cid, cl in cases.items() if pick(cl, key)]
            print('fc %s %r: %d production launches (%s, ...) <- %s' % (kind, key, len(prod[key]), prod[key][0], ', '.join(by) or 'NOT COVERED'))
            if not by:
                missing.append((kind, key, prod[key][0]))
            elif all(c in GPU_ONLY or (c in MIX_CASES and any(j in GPU_ONLY for j in MIX_CASES[c][0])) for c in by):
                gpu_only.append(key)
                print('  covered on the GPU only')
    assert not missing, 'no case runs: %s' % '; '.join('%s %r of %s' % m for m in missing)
    return dict(production_jobs=prod_jobs, production_mix=prod_mix, cases=cases, gpu_only=gpu_only)
