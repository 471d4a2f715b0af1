"""Shared bodies of the float64 tests of the three kernels behind VAE.project_latent (vg_latent.hip): vg_knn (knn_partial_k<KB>,
knn_merge_k<KB>), vg_umap_fuzzy (umap_mean_part_k, umap_fuzzy_k) and vg_umap_layout_epoch (umap_layout_k), and of the plan query
vg_knn_plan / latent_projection.knn_plan.  Run on CPU tensors through the host build of the kernels (tests/test_projection_emu.py)
and on the GPU through libvaegam_hip.so (tests/test_projection_gpu.py).  One input builder per kernel, the references, the bound checks
and the case lists live here; a reference is computed once per process and shared.  u = 2^-24 throughout; every bounded check prints
its worst err / bound before it asserts and leaves (case, quantity, worst) in RECORDS.

kNN.  Reference: float64 distances by direct differences (never the |a|^2 + |b|^2 - 2ab expansion), sorted by (distance, index), the
query first.  The kernel does one fp32 subtraction, D chained fmaf and one sqrtf per distance, so its relative error is at most
((D + 2)/2 + 2) u (4.0e-6 at D = 128).  For every case, no position left out: (a) idx[:,0] is the query at distance exactly 0, (b) every
index in [0, N), none repeated in a row, the query nowhere after position 0, (c) dist non-decreasing along a row and bit-equal distances
in index order, (d) dist[i,j] within the bound of the float64 distance of the pair (i, idx[i,j]), (e) dist[i,j] within the bound of the
reference's j-th distance.  idx equals the reference at every position whose reference distance is separated from both neighbours (the
first point outside the list counts) by more than 4 x the bound, relative; at most 5 % of the positions 1..k-1 of a case may be left out
by that rule.  A neighbouring position that holds a copy of the same point is no competitor (identical coordinates give the kernel
bit-equal distances too, and the index decides as in the reference): the separation is asked of the nearest other points.  Shares left
out, computed on the reference alone: 3.1 % at 300-D128-k64, 0.53 % at dups-512-D6-k8, 0.23 % at 300-D32-k33, 0.20 % at 257-D32-k20
and less everywhere else (knn_host prints them; KNN_SHARES_SEEN keeps them).

Fuzzy set.  Reference: the header's contract in float64, replaying the same bisection.  rho bit-equal to the smallest positive distance
of the row, sigma within 2 u relative (the reference is the fp32 rounding of a float64 value), w within 2 u absolute and exactly 0
where idx = i.  The stopping test |psum - log2 k| < 1e-5 is a discontinuity: a row whose | |psum - log2 k| - 1e-5 | came under 1e-9
in any step would be left out, and the module asserts that no row of any case is (the seeds are chosen so).  The kernel is fed the
float64 reference neighbour lists rounded to fp32, so a kNN failure cannot hide here.

Layout.  One epoch from a given y_in per check.  Reference: the documented formula in float64 from the fp32 inputs (a, b and 0.001
rounded to fp32 first, alpha formed in fp32, the due test in double and the negatives from the integer key: both exact).  Bound per
output coordinate: 16 u M with M = |y| + sum over its contributions of (|g| + |partial sum after the add|), from the reference; M = 0
asks for equality.  That M is honest is asserted on the reference alone: the same-order fp32 numpy restatement stays within 4 u M in
every case (and that restatement, vectorised here, is the bits of the scalar ref_epoch)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib
from vae_gam_amd import latent_projection as LP

U = 2.0 ** -24
GUARD = 777.0
CANARIES = 64
RECORDS = []                                            # (case, quantity, worst err / bound) of every bounded check made in this process


def _check(what, qty, got, want, bound):
    """|got - want| <= bound per element (bound broadcast); where bound == 0 the two must be equal.  Prints the worst err / bound
    before it asserts."""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, np.float64), np.asarray(want).shape).reshape(-1) if np.ndim(bound) == 0 else \
        np.asarray(bound, np.float64).reshape(-1)
    assert got.shape == want.shape == bound.shape, (what, qty, got.shape, want.shape, bound.shape)
    if want.size == 0:
        return 0.0
    assert np.isfinite(got).all(), '%s %s: not finite' % (what, qty)
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    i = int(ratio.argmax())
    worst = float(ratio[i])
    print('%s %s: worst err/bound %.3g at %d (err %.3g, bound %.3g, want %.9g)' % (what, qty, worst, i, err[i], bound[i], want[i]))
    RECORDS.append((what, qty, worst))
    assert worst <= 1.0, '%s %s: error %.3g is %.3g of the bound %.3g at element %d' % (what, qty, err[i], worst, bound[i], i)
    return worst


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _seed(cid):
    return zlib.crc32(cid.encode())


# ================================================================================================================ kNN
# id: (N, D, k, kind)
def _k(N, D, k, kind='normal'):
    return (N, D, k, kind)


KNN_CASES = {}
for _c in ((1, 1, 1), (2, 2, 2), (17, 1, 17), (12, 3, 12),                                  # smallest shapes, k = N, k = 1
           (300, 1, 2), (300, 7, 9), (300, 15, 10), (300, 16, 17), (300, 17, 18), (300, 32, 33), (300, 33, 34), (300, 128, 64),
           (255, 32, 20), (256, 32, 20), (257, 32, 20), (2048, 8, 20), (2049, 5, 64), (4097, 3, 20)):
    KNN_CASES['%d-D%d-k%d' % _c] = _k(*_c)
KNN_CASES['offset-1000-D7-k33'] = _k(1000, 7, 33, 'offset')
KNN_CASES['dups-512-D6-k8'] = _k(512, 6, 8, 'dups')
KNN_GUARD_CASES = ('300-D17-k18', '2049-D5-k64')         # S > 1, N no multiple of 256
KNN_SEP = 4.0                                           # index equality where the reference is separated by more than KNN_SEP bounds
KNN_LEFT_OUT_CAP = 0.05
KNN_SHARES_SEEN = {}


def knn_c(D):
    """the relative distance bound in units of u: one subtraction, D chained fmaf, one sqrtf"""
    return (D + 2) / 2.0 + 2.0


def knn_input(cid):
    N, D, k, kind = KNN_CASES[cid]
    x = np.random.default_rng(_seed(cid)).normal(size=(N, D)).astype(np.float32)
    if kind == 'offset':
        x = (x + np.float32(1000.0)).astype(np.float32)
    if kind == 'dups':                                  # S = 4, chunk 128: the three copies sit in splits 0, 2 and 3
        x[256:266] = x[:10]; x[384:394] = x[:10]
    return x


def pair_dist64(x, i, j):
    """float64 distances of the pairs (i[r], j[r, c]) by direct differences"""
    x = x.astype(np.float64)
    out = np.empty(j.shape)
    for r0 in range(0, len(i), 256):
        d = x[i[r0:r0 + 256], None, :] - x[j[r0:r0 + 256]]
        out[r0:r0 + 256] = np.sqrt((d * d).sum(-1))
    return out


def ref_knn(x, k):
    """-> (idx (N, k'), dist (N, k')) float64 reference with k' = min(k + 1, N): one place more than asked for, the first point
    outside the list.  Sorted by (distance, index), the query first."""
    N = len(x)
    x64 = x.astype(np.float64)
    kk = min(k + 1, N)
    idx = np.empty((N, kk), np.int64); dist = np.empty((N, kk))
    for q0 in range(0, N, 256):
        d = x64[q0:q0 + 256, None, :] - x64[None, :, :]
        d = np.sqrt((d * d).sum(-1))
        rows = np.arange(d.shape[0])
        d[rows, q0 + rows] = -1.0                       # the query first
        m = kk + 16
        if m < N:                                       # the m smallest in index order, provided place kk is settled among them
            c = np.sort(np.argpartition(d, m - 1, axis=1)[:, :m], axis=1)
            dc = d[rows[:, None], c]
            o = np.take_along_axis(c, np.argsort(dc, axis=1, kind='stable'), 1)     # stable: equal distances stay in index order
            if not (d[rows[:, None], o][:, kk - 1] < dc.max(1)).all():              # a tie that reaches the cut: sort the whole rows
                m = N
        if m >= N:
            o = np.argsort(d, axis=1, kind='stable')
        o = o[:, :kk]
        idx[q0:q0 + 256] = o
        dist[q0:q0 + 256] = d[rows[:, None], o]
    dist[:, 0] = 0.0
    return idx, dist


_KNN_HOST = {}


def knn_host(cid):
    """input, reference and the positions at which the index must equal the reference's; computed once per process"""
    if cid in _KNN_HOST:
        return _KNN_HOST[cid]
    N, D, k, kind = KNN_CASES[cid]
    x = knn_input(cid)
    ri1, rd1 = ref_knn(x, k)
    ri, rd = ri1[:, :k], rd1[:, :k]
    rel = KNN_SEP * knn_c(D) * U
    # A neighbour that is a copy of the position's own point is no competitor: identical coordinates give the kernel bit-equal
    # distances too, and the index decides as it does in the reference.  The separation is asked of the nearest positions on either
    # side that hold another point (position 0, the query, never competes with position 1).
    twin = (x[ri1[:, 1:]] == x[ri1[:, :-1]]).all(-1)                    # twin[:, j]: positions j and j + 1 hold copies of one point
    lo = np.full((N, k), -np.inf); hi = np.full((N, k), np.inf)
    for j in range(2, k):
        lo[:, j] = np.where(twin[:, j - 1], lo[:, j - 1], rd[:, j - 1])
    if k < N:                                                          # the first point outside the list; a copy of the last place
        hi[:, k - 1] = np.where(twin[:, k - 1], rd[:, k - 1], rd1[:, k])   # hides what follows it: that place is left out
    for j in range(k - 2, 0, -1):
        hi[:, j] = np.where(twin[:, j], hi[:, j + 1], rd[:, j + 1])
    sep = rel * rd
    sel = (rd - lo > sep) & (hi - rd > sep)
    sel[:, 0] = True
    left_out = float((~sel[:, 1:]).mean()) if k > 1 else 0.0
    KNN_SHARES_SEEN[cid] = left_out
    print('%s: %.3f %% of the positions 1..k-1 left out of the index comparison' % (cid, 100 * left_out))
    assert left_out <= KNN_LEFT_OUT_CAP, (cid, left_out)
    if kind == 'offset':                                # the expansion would lose these distances: they are small beside |x|^2
        assert rd[:, 1:].max() < 0.01 * np.sqrt((x.astype(np.float64) ** 2).sum(-1)).min()
    h = dict(x=x, ri=ri, rd=rd, sel=sel, N=N, D=D, k=k, kind=kind)
    _KNN_HOST[cid] = h
    return h


def check_knn_result(cid, idx, dist):
    h = knn_host(cid)
    x, ri, rd, N, D, k = h['x'], h['ri'], h['rd'], h['N'], h['D'], h['k']
    assert idx.shape == (N, k) and dist.shape == (N, k) and idx.dtype == np.int32 and dist.dtype == np.float32
    q = np.arange(N)
    assert (idx[:, 0] == q).all() and (dist[:, 0] == 0).all(), cid + ': (a) position 0 is not the query at distance 0'
    assert ((idx >= 0) & (idx < N)).all(), cid + ': (b) index out of range'
    assert (idx[:, 1:] != q[:, None]).all(), cid + ': (b) the query after position 0'
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), cid + ': (b) an index twice in a row'
    assert np.isfinite(dist).all() and (dist[:, 1:] >= dist[:, :-1]).all(), cid + ': (c) distances decrease along a row'
    tie = dist[:, 2:] == dist[:, 1:-1]
    assert (idx[:, 2:][tie] > idx[:, 1:-1][tie]).all(), cid + ': (c) bit-equal distances not in index order'
    c = knn_c(D) * U
    pd = pair_dist64(x, q, idx.astype(np.int64))
    _check(cid, 'dist vs its own pair', dist, pd, c * pd)
    _check(cid, 'dist vs reference', dist, rd, c * rd)
    sel = h['sel']
    bad = sel & (idx != ri)
    assert not bad.any(), '%s: index differs from the reference at a separated position, first (row, place) %r: got %r, want %r' % (
        cid, tuple(np.argwhere(bad)[0]), idx[np.argwhere(bad)[0][0]].tolist(), ri[np.argwhere(bad)[0][0]].tolist())
    if h['kind'] == 'dups':
        for i in range(10):
            copies = [i, 256 + i, 384 + i]
            for cpy in copies:                          # the two other copies next, at distance exactly 0, lower index first
                assert list(idx[cpy, 1:3]) == [o for o in copies if o != cpy] and (dist[cpy, 1:3] == 0).all(), (cid, cpy, idx[cpy])


_KNN_RUN = {}


def run_knn(dev, cid):
    """LP.knn on the case, every check of the module docstring -> (idx, dist) numpy"""
    if (dev, cid) in _KNN_RUN:
        return _KNN_RUN[(dev, cid)]
    h = knn_host(cid)
    idx, dist = LP.knn(_t(h['x'], dev), h['k'])
    _sync(dev)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    check_knn_result(cid, idx, dist)
    _KNN_RUN[(dev, cid)] = (idx, dist)
    return idx, dist


def run_knn_guard(dev, cid):
    """The C ABI with a workspace of exactly vg_knn_ws_bytes filled with NaN and followed by 64 canaries, idx and dist each followed by
    canaries: the bits of the LP.knn path (which run_knn holds to float64), the canaries intact.  An unwritten workspace entry read by
    the merge (a NaN whose bits, as an index, are 2143289344) or a store by one of the idle query lanes of the last block shows."""
    h = knn_host(cid)
    N, D, k = h['N'], h['D'], h['k']
    want_i, want_d = run_knn(dev, cid)
    lib = _lib.get_lib()
    nbytes = lib.size('vg_knn_ws_bytes', N, D, k)
    p = LP.knn_plan(N, D, k)
    assert nbytes == p.S * (k - 1) * N * 8 and p.S > 1 and N % 256 != 0
    n = nbytes // 4
    x = _t(h['x'], dev)
    ws = torch.cat([torch.full((n,), float('nan')), torch.full((CANARIES,), GUARD)]).to(dev)
    idx = torch.cat([torch.full((N * k,), -5, dtype=torch.int32), torch.full((CANARIES,), 777, dtype=torch.int32)]).to(dev)
    dist = torch.cat([torch.full((N * k,), float('nan')), torch.full((CANARIES,), GUARD)]).to(dev)
    LP._call(x, 'vg_knn', LP._p(x), N, D, k, LP._p(ws), LP._p(idx), LP._p(dist))
    _sync(dev)
    assert torch.equal(ws[n:].cpu(), torch.full((CANARIES,), GUARD)), cid + ': wrote past vg_knn_ws_bytes'
    assert torch.equal(idx[N * k:].cpu(), torch.full((CANARIES,), 777, dtype=torch.int32)), cid + ': wrote past idx'
    assert torch.equal(dist[N * k:].cpu(), torch.full((CANARIES,), GUARD)), cid + ': wrote past dist'
    assert np.array_equal(idx[:N * k].cpu().numpy().reshape(N, k), want_i), cid + ': idx differs from the LP.knn path'
    assert np.array_equal(dist[:N * k].cpu().numpy().reshape(N, k).view(np.uint32), want_d.view(np.uint32)), cid + ': dist differs'


# ---------------------------------------------------------------------------------------------------------------- plan and coverage
def ref_knn_splits(N):
    """vg_latent.hip: knn_splits -> (requested splits s, chunk, launched splits S, candidates in the last split)"""
    cdiv = lambda a, b: -(-a // b)
    s = min(cdiv(2048, cdiv(N, 256)), N // 128)
    s = max(1, min(16, s))
    chunk = cdiv(cdiv(N, s), 16) * 16
    S = cdiv(N, chunk)
    return s, chunk, S, N - (S - 1) * chunk


SPLIT_TABLE = ((255, 1, 256, 1, 255), (256, 2, 128, 2, 128), (257, 2, 144, 2, 113), (300, 2, 160, 2, 140), (2048, 16, 128, 16, 128),
               (2049, 16, 144, 15, 33), (4097, 16, 272, 16, 17))          # N, s, chunk, S, candidates in the last split


def check_knn_plan():
    """knn_plan against the restated arithmetic over a sweep of N, D and k; nothing is launched.  Bad shapes raise as
    vg_knn_ws_bytes does."""
    for row in SPLIT_TABLE:
        assert ref_knn_splits(row[0]) == row[1:], row
    ns = list(range(1, 700)) + [2047, 2048, 2049, 4095, 4096, 4097, 20000, 50000, 524287, 524288, 524289, 1000000]
    for N in ns:
        s, chunk, S, last = ref_knn_splits(N)
        for D, k in ((1, 1), (16, 2), (17, 9), (128, 10), (5, 17), (7, 18), (32, 33), (33, 34), (3, 64), (32, 20)):
            if k > N:
                continue
            p = LP.knn_plan(N, D, k)
            K1 = k - 1
            kb = 0 if K1 == 0 else min(b for b in (8, 16, 32, 64) if K1 <= b)
            dp = -(-D // 16) * 16
            assert p == LP.KnnPlan(kb, S, chunk, dp, -(-N // 256), last, 16 * (dp + 256) * 4 if kb else 0), (N, D, k, p)
            assert 0 < p.last <= p.chunk and (p.S - 1) * p.chunk + p.last == N and p.chunk % 16 == 0 and 1 <= p.S <= 16
            assert p.lds_bytes <= 64 * 1024
            assert _lib.get_lib().size('vg_knn_ws_bytes', N, D, k) == p.S * K1 * N * 8
    rec = (ctypes.c_int32 * 7)()
    for bad in ((0, 4, 1), (10, 0, 2), (10, 129, 2), (10, 4, 0), (100, 4, 65), (10, 4, 11)):
        with pytest.raises(_lib.VgError, match='bad shape'):
            LP.knn_plan(*bad)
        with pytest.raises(_lib.VgError, match='bad shape'):
            _lib.get_lib().size('vg_knn_ws_bytes', *bad)
    with pytest.raises(_lib.VgError, match='out must hold 7 values'):
        _lib.get_lib().call('vg_knn_plan', 300, 8, 20, rec, 6)
    with pytest.raises(_lib.VgError, match='out must hold 7 values'):
        _lib.get_lib().call('vg_knn_plan', 300, 8, 20, None, 7)


def check_knn_coverage(cases=None):
    """From knn_plan over the listed cases: every KB with both sides of each boundary, S = 1, 2, 16 and S != the requested count,
    Dp > D and D = Dp at 16 and at 128, a last split with fewer candidates than k - 1 (at k = 64 and at the default k = 20), a ragged
    last query block (and a second block holding one query), k = N."""
    cases = KNN_CASES if cases is None else cases
    plans = {cid: (c, LP.knn_plan(*c[:3])) for cid, c in cases.items()}
    for cid, (c, p) in plans.items():
        print('%-22s %s requested s = %d' % (cid, p, ref_knn_splits(c[0])[0]))
    P = list(plans.values())
    k1s = {c[2] - 1 for c, _ in P}
    assert {p.KB for _, p in P} == {0, 8, 16, 32, 64}, 'a KB instance is not launched'
    for edge in (0, 1, 8, 9, 16, 17, 32, 33, 63):
        assert edge in k1s, 'no case with k - 1 = %d (one side of a KB boundary)' % edge
    ss = {p.S for _, p in P}
    assert {1, 2, 16} <= ss, 'S = 1, 2 and 16'
    assert any(p.S == 16 and p.last == p.chunk for _, p in P), 'S = 16 with every split full'
    assert any(p.S != ref_knn_splits(c[0])[0] and p.KB for c, p in P), 'no case launches fewer splits than requested'
    assert any(p.Dp > c[1] for c, p in P) and any(c[1] == 16 for c, _ in P) and any(c[1] == 128 for c, _ in P), 'D padding classes'
    assert {1, 15, 16, 17, 32, 33} <= {c[1] for c, _ in P}, 'every edge of the D padding'
    short = [(c, p) for c, p in P if p.S > 1 and p.last < c[2] - 1]
    assert any(c[2] == 64 for c, _ in short) and any(c[2] == 20 for c, _ in short), 'a last split with fewer candidates than k - 1'
    assert any(p.last % 16 for _, p in P if p.S == 2), 'a ragged last tile in the second of two splits'
    assert any(c[0] % 256 and p.qblocks == 1 and p.S == 1 and c[0] // 128 == 1 for c, p in P), \
        'S = 1 from N / 128 = 1 (not from the clamp of 0), with a ragged query block'
    assert any(c[0] % 256 == 1 and p.qblocks == 2 for c, p in P), 'a second query block holding one query'
    assert any(c[0] % 256 == 0 for c, _ in P), 'a full last query block'
    assert any(c[2] == c[0] and c[2] > 1 for c, _ in P), 'k = N'
    assert any(c[3] == 'offset' for c, _ in P) and any(c[3] == 'dups' and p.S >= 3 for c, p in P)
    return plans


# ================================================================================================================ fuzzy set
# id: (N, D, k, scale, kind)
FUZZY_CASES = {
    '1-k1': (1, 3, 1, 1.0, 'normal'), '255-k2': (255, 4, 2, 1.0, 'normal'), '256-k15': (256, 9, 15, 1.0, 'normal'),
    '257-k33': (257, 6, 33, 1.0, 'normal'), '600-k64': (600, 12, 64, 1.0, 'normal'),
    'x100-300-k15': (300, 9, 15, 100.0, 'normal'), 'x0.01-300-k20': (300, 9, 20, 0.01, 'normal'),
    'dups-120-k15': (120, 9, 15, 1.0, 'dups'), 'zeros-30-k8': (30, 4, 8, 1.0, 'zeros'), 'equidistant-40-k15': (40, 40, 15, 1.0, 'equi'),
}
FUZZY_GUARD = 1e-9


def fuzzy_input(cid):
    """-> (idx int32, dist fp32): the float64 reference neighbour lists of the case's points, rounded to fp32"""
    N, D, k, scale, kind = FUZZY_CASES[cid]
    x = (np.random.default_rng(_seed('fuzzy' + cid)).normal(size=(N, D)) * scale).astype(np.float32)
    if kind == 'dups':
        x[100:110] = x[:10]                             # rho from the first NON-zero distance
    if kind == 'zeros':
        x[:25] = 0.0                                    # 25 points on one spot: every neighbour of theirs at distance 0
    if kind == 'equi':
        x = np.eye(N, dtype=np.float32) * np.float32(3.0)
    ri, rd = ref_knn(x, k)
    return ri[:, :k].astype(np.int32), rd[:, :k].astype(np.float32)


def ref_fuzzy(idx, dist):
    """include/vaegam.h: vg_umap_fuzzy in float64 -> (rho, sigma, w, per row the smallest | |psum - log2 k| - 1e-5 | seen)"""
    dist = dist.astype(np.float64)
    N, k = dist.shape
    mean_all = dist.mean()
    target = np.log2(k)
    rho = np.zeros(N); sigma = np.zeros(N); w = np.zeros((N, k)); near = np.full(N, np.inf)
    for i in range(N):
        nz = dist[i][dist[i] > 0]
        r = nz.min() if len(nz) else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            t = dist[i, 1:] - r
            psum = np.where(t > 0, np.exp(-(np.maximum(t, 0) / mid)), 1.0).sum()
            near[i] = min(near[i], abs(abs(psum - target) - 1e-5))
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid; mid = (lo + hi) / 2.0
            else:
                lo = mid; mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        mid = max(mid, 1e-3 * (dist[i].sum() / k if r > 0 else mean_all))
        rho[i], sigma[i] = r, mid
        for j in range(k):
            t = dist[i, j] - r
            w[i, j] = 0.0 if idx[i, j] == i else (1.0 if (t <= 0 or mid == 0) else np.exp(-t / mid))
    return rho, sigma, w, near


_FUZZY_HOST = {}


def fuzzy_host(cid):
    if cid not in _FUZZY_HOST:
        idx, dist = fuzzy_input(cid)
        rho, sigma, w, near = ref_fuzzy(idx, dist)
        keep = near >= FUZZY_GUARD
        print('%s: smallest | |psum - log2 k| - 1e-5 | over the rows %.3g, %d rows left out' % (cid, near.min(), int((~keep).sum())))
        assert keep.all(), '%s: %d rows sit on the stopping test; choose another seed' % (cid, int((~keep).sum()))
        _FUZZY_HOST[cid] = dict(idx=idx, dist=dist, rho=rho, sigma=sigma, w=w, keep=keep)
    return _FUZZY_HOST[cid]


def run_fuzzy(dev, cid):
    h = fuzzy_host(cid)
    N, D, k, scale, kind = FUZZY_CASES[cid]
    idx, dist = h['idx'], h['dist']
    rho, sigma, w = [t.cpu().numpy() for t in LP.smooth_knn(_t(idx, dev), _t(dist, dev))]
    _sync(dev)
    assert rho.dtype == np.float32 and sigma.shape == (N,) and w.shape == (N, k)
    pos = np.where(dist > 0, dist, np.float32(np.inf)).min(1)
    want_rho = np.where(np.isfinite(pos), pos, np.float32(0)).astype(np.float32)
    assert np.array_equal(want_rho.astype(np.float64), h['rho'])
    assert np.array_equal(rho.view(np.uint32), want_rho.view(np.uint32)), cid + ': rho is not the smallest positive distance of the row'
    keep = h['keep']
    s32 = h['sigma'].astype(np.float32).astype(np.float64)
    _check(cid, 'sigma', sigma[keep], s32[keep], 2 * U * s32[keep])
    _check(cid, 'w', w[keep], h['w'][keep], 2 * U)
    assert (w[idx == np.arange(N)[:, None]] == 0).all() and (w[:, 0] == 0).all(), cid + ': w of the point itself is not 0'
    assert (sigma > 0).all()
    d64 = dist.astype(np.float64)
    if k == 1:
        assert (sigma == 1).all() and (rho == 0).all()                  # an empty sum: log2 1 = 0 is met at once
    if k == 2:
        assert (sigma == 1).all()                                       # psum = 1 = log2 2 at the first step
    if scale == 100.0:
        assert (h['sigma'] > 2).all()                                   # the doubling branch ran in every row
    if scale == 0.01:
        assert (h['sigma'] < 0.5).all()                                 # and here the halving branch
    if kind == 'zeros':                                                 # the floor of an all-zero row comes from the global mean
        z = (d64 == 0).all(1)
        assert z.sum() == 25 and np.array_equal(sigma[z], np.full(25, np.float32(1e-3 * d64.mean())))
        assert (rho[z] == 0).all()
    if kind == 'equi':                                                  # psum = k - 1 whatever sigma is: 64 halvings, the row-mean floor
        assert len(np.unique(dist[:, 1:])) == 1
        assert np.array_equal(sigma, (1e-3 * (d64.sum(1) / k)).astype(np.float32)), cid
        assert (w[:, 1:] == 1).all()


# ================================================================================================================ layout
M64 = (1 << 64) - 1


def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_epoch(y, rowptr, col, eps, n, n_epochs, a, b, neg, seed):
    """include/vaegam.h: vg_umap_layout_epoch restated with numpy fp32 scalars, one vertex and one contribution at a time"""
    f = np.float32
    N = len(y)
    a, b = f(a), f(b)
    alpha = f(1) - f(n) / f(n_epochs)
    out = y.copy()
    two_ab, bm1, two_b = f(-2) * a * b, b - f(1), f(2) * b
    sk = (seed * 0x9E3779B97F4A7C15) & M64

    def clip(v):
        return min(max(v, f(-4)), f(4))

    for i in range(N):
        ox, oy = y[i, 0], y[i, 1]
        if n >= 1:
            for e in range(rowptr[i], rowptr[i + 1]):
                ep = float(eps[e])
                if not (np.floor(n / ep) > np.floor((n - 1) / ep)):
                    continue
                j = col[e]
                dx, dy = y[i, 0] - y[j, 0], y[i, 1] - y[j, 1]
                d2 = dx * dx + dy * dy
                if d2 > 0:
                    coef = (two_ab * np.power(d2, bm1)) / (a * np.power(d2, b) + f(1))
                    gx, gy = alpha * clip(coef * dx), alpha * clip(coef * dy)
                    ox = ox + gx; oy = oy + gy
                    ox = ox + gx; oy = oy + gy
                for s in range(neg):
                    kk = splitmix64(((((n << 44) | (e << 5)) | s) + sk) & M64) % N
                    if kk == i:
                        continue
                    dx, dy = y[i, 0] - y[kk, 0], y[i, 1] - y[kk, 1]
                    d2 = dx * dx + dy * dy
                    if not d2 > 0:
                        continue
                    coef = two_b / ((f(0.001) + d2) * (a * np.power(d2, b) + f(1)))
                    ox = ox + alpha * clip(coef * dx); oy = oy + alpha * clip(coef * dy)
        out[i, 0], out[i, 1] = ox, oy
    return out


def _splitmix64_np(z):
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def layout_contributions(y, rowptr, col, eps, n, n_epochs, a, b, neg, seed, dt):
    """Every contribution of the epoch in the order the kernel adds them, all due edges at once: -> (row (C,), g (C, 2) of dtype dt,
    counts) with the arithmetic of the header carried out in dt (np.float32: the kernel's own roundings; np.float64: the reference,
    from the same fp32 inputs and fp32-rounded constants).  Skipped contributions (d2 = 0, a negative that is the vertex) are absent."""
    N = len(y)
    f = np.float32
    empty = (np.zeros(0, np.int64), np.zeros((0, 2), dt), dict(due=0, coincident=0, self_neg=0, clipped=0))
    nnz = int(rowptr[-1])
    if n < 1 or nnz == 0:
        return empty
    a32, b32 = f(a), f(b)
    alpha = dt(f(1) - f(n) / f(n_epochs))
    A, B = dt(a32), dt(b32)
    two_ab, bm1, two_b, c001, one, four = dt(-2) * A * B, B - dt(1), dt(2) * B, dt(f(0.001)), dt(1), dt(4)
    row_of = np.repeat(np.arange(N), np.diff(rowptr))
    ep = eps.astype(np.float64)
    due = np.nonzero(np.floor(n / ep) > np.floor((n - 1) / ep))[0]
    if len(due) == 0:
        return empty
    Y = y.astype(dt)
    i = row_of[due]; j = col[due].astype(np.int64)
    slots = 2 + neg
    G = np.zeros((len(due), slots, 2), dt); V = np.zeros((len(due), slots), bool)
    d = Y[i] - Y[j]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    ok = d2 > 0
    d2s = np.where(ok, d2, one)
    coef = (two_ab * np.power(d2s, bm1)) / (A * np.power(d2s, B) + one)
    raw = coef[:, None] * d
    g = alpha * np.clip(raw, -four, four)
    clipped = int((np.abs(raw[ok]) > 4).sum())
    G[:, 0] = g; G[:, 1] = g; V[:, 0] = ok; V[:, 1] = ok
    self_neg = 0
    if neg:
        sk = np.uint64((seed * 0x9E3779B97F4A7C15) & M64)
        key = (np.uint64(n) << np.uint64(44)) | (due.astype(np.uint64) << np.uint64(5))
        with np.errstate(over='ignore'):
            z = (key[:, None] | np.arange(neg, dtype=np.uint64)[None, :]) + sk
        kk = (_splitmix64_np(z) % np.uint64(N)).astype(np.int64)
        d = Y[i][:, None, :] - Y[kk]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        okn = (kk != i[:, None]) & (d2 > 0)
        self_neg = int((kk == i[:, None]).sum())
        d2s = np.where(okn, d2, one)
        coef = two_b / ((c001 + d2s) * (A * np.power(d2s, B) + one))
        raw = coef[..., None] * d
        clipped += int((np.abs(raw[okn]) > 4).sum())
        G[:, 2:] = alpha * np.clip(raw, -four, four); V[:, 2:] = okn
    rows = np.repeat(i, slots).reshape(len(due), slots)
    assert G.dtype == dt
    return rows[V], G[V], dict(due=len(due), coincident=int((~ok).sum()), self_neg=self_neg, clipped=clipped)


def layout_accumulate(y, rows, G, dt):
    """y_i + its contributions one after the other in dt -> (out (N, 2) dt, M (N, 2) float64 = |y| + sum (|g| + |partial sum|))"""
    out = y.astype(dt).copy()
    M = np.abs(y.astype(np.float64))
    if len(rows):
        start = np.searchsorted(rows, np.arange(len(y)))
        cnt = np.bincount(rows, minlength=len(y))
        for t in range(int(cnt.max())):
            r = np.nonzero(cnt > t)[0]
            g = G[start[r] + t]
            out[r] = out[r] + g
            M[r] += np.abs(g.astype(np.float64)) + np.abs(out[r].astype(np.float64))
    return out, M


def ref_layout(y, rowptr, col, eps, n, n_epochs, a, b, neg, seed):
    """-> (float64 reference, M, the same-order fp32 restatement, counts)"""
    args = (y, rowptr, col, eps, n, n_epochs, a, b, neg, seed)
    r64, g64, counts = layout_contributions(*args, np.float64)
    want, M = layout_accumulate(y, r64, g64, np.float64)
    r32, g32, _ = layout_contributions(*args, np.float32)
    assert np.array_equal(r32, r64)
    y32, _ = layout_accumulate(y, r32, g32, np.float32)
    assert y32.dtype == np.float32
    return want, M, y32, counts


LAYOUT_C = 16.0
AB = {}


def ab():
    if not AB:
        AB['ab'] = LP.find_ab_params(1.0, 0.1)
    return AB['ab']


# id: (graph, epoch n, n_epochs, negative rate, scale of y_in, seed)
LAYOUT_CASES = {
    'blobs-n0-neg5': ('blobs', 0, 200, 5, 10.0, 1234),
    'blobs-n1-neg5': ('blobs', 1, 200, 5, 10.0, 1234),
    'blobs-n7-neg0': ('blobs', 7, 200, 0, 10.0, 1234),
    'blobs-n7-neg5': ('blobs', 7, 200, 5, 10.0, 42),
    'blobs-n7-neg31': ('blobs', 7, 200, 31, 10.0, 1234),
    'blobs-n199-neg5': ('blobs', 199, 200, 5, 10.0, (1 << 63) + 12345),
    'blobs-n199-neg31-small': ('blobs', 199, 200, 31, 0.05, 7),
    'blobs-n1-neg31-small': ('blobs', 1, 200, 31, 0.05, 1234),
    'blobs-n7-neg5-small': ('blobs', 7, 200, 5, 0.05, 0),
    'coincident-n7-neg5': ('coincident', 7, 200, 5, 10.0, 1234),
    'empty-rows-n7-neg5': ('empty-rows', 7, 200, 5, 10.0, 1234),
    'no-edges-n3-neg5': ('no-edges', 3, 200, 5, 10.0, 1234),
    'one-vertex-n3-neg31': ('one-vertex', 3, 200, 31, 10.0, 1234),
    'n257-n3-neg5': ('n257', 3, 50, 5, 10.0, 99),
}
_GRAPHS = {}


def layout_graph(dev, kind):
    """-> (rowptr, col, eps) numpy, col / eps None for the graph without edges.  Graphs come from LP.build_graph on the device under
    test (the reference takes the graph as given)."""
    base = {'coincident': 'blobs', 'empty-rows': 'blobs'}.get(kind, kind)
    if (dev, base) not in _GRAPHS:
        rng = np.random.default_rng(_seed(base))
        if base == 'blobs':                             # two blocks of vertices, about 7.8k edges
            x = np.concatenate([rng.normal(size=(150, 5)), rng.normal(size=(150, 5)) + 4]).astype(np.float32)
            g = LP.build_graph(_t(x, dev), 20, 200)
        elif base == 'n257':
            x = rng.normal(size=(257, 4)).astype(np.float32)
            g = LP.build_graph(_t(x, dev), 10, 50)
        elif base == 'no-edges':
            _GRAPHS[(dev, base)] = (np.zeros(6, np.int32), None, None)
        elif base == 'one-vertex':                      # a self-loop due at every epoch: d2 = 0, and every negative is the vertex itself
            _GRAPHS[(dev, base)] = (np.array([0, 1], np.int32), np.zeros(1, np.int32), np.ones(1, np.float32))
        if (dev, base) not in _GRAPHS:
            _sync(dev)
            _GRAPHS[(dev, base)] = tuple(t.cpu().numpy() for t in g[3:6])
    rowptr, col, eps = _GRAPHS[(dev, base)]
    if kind == 'empty-rows':                            # vertices 0..9, 255, 256 and 299 lose every edge, on both ends
        N = len(rowptr) - 1
        gone = np.zeros(N, bool); gone[:10] = True; gone[[255, 256, 299]] = True
        row_of = np.repeat(np.arange(N), np.diff(rowptr))
        keep = ~(gone[row_of] | gone[col])
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=N))]).astype(np.int32)
        col, eps = col[keep], eps[keep]
        assert (np.diff(rowptr)[gone] == 0).all() and len(col) > 5000
    return rowptr, col, eps


def layout_y(cid, rowptr, col, eps):
    kind, n, n_epochs, neg, scale, seed = LAYOUT_CASES[cid]
    N = len(rowptr) - 1
    y = (np.random.RandomState(_seed(cid) % (1 << 31)).uniform(0, 1, size=(N, 2)) * scale).astype(np.float32)
    if kind == 'coincident':                            # the far ends of the first three edges due at epoch n sit on their vertices
        ep = eps.astype(np.float64)
        due = np.nonzero(np.floor(n / ep) > np.floor((n - 1) / ep))[0]
        row_of = np.repeat(np.arange(N), np.diff(rowptr))
        for e in due[[0, len(due) // 2, -1]]:
            y[col[e]] = y[row_of[e]]
    return y


_LAYOUT_HOST = {}


def layout_host(dev, cid):
    kind, n, n_epochs, neg, scale, seed = LAYOUT_CASES[cid]
    rowptr, col, eps = layout_graph(dev, kind)
    key = (cid, rowptr.tobytes(), None if col is None else col.tobytes(), None if eps is None else eps.tobytes())
    if key in _LAYOUT_HOST:
        return _LAYOUT_HOST[key]
    y = layout_y(cid, rowptr, col, eps)
    a, b = ab()
    want, M, y32, counts = ref_layout(y, rowptr, col, eps, n, n_epochs, a, b, neg, seed)
    print('%s: N %d, nnz %d, %r' % (cid, len(y), int(rowptr[-1]), counts))
    # M is honest: the kernel's own arithmetic restated in numpy stays within a quarter of the bound
    _check(cid + ' [fp32 restatement]', 'y_out', y32, want, (LAYOUT_C / 4) * U * M)
    RECORDS.pop()                                       # (printed; RECORDS holds what the library under test gave)
    h = dict(y=y, rowptr=rowptr, col=col, eps=eps, want=want, M=M, y32=y32, counts=counts)
    _LAYOUT_HOST[key] = h
    return h


def _epoch_call(dev, rowptr, col, eps, y_in, n, n_epochs, a, b, neg, seed):
    """one vg_umap_layout_epoch through the C ABI, y_out followed by canaries -> y_out numpy"""
    N = y_in.shape[0]
    out = torch.cat([torch.full((2 * N,), float('nan')), torch.full((CANARIES,), GUARD)]).to(dev)
    nnz = 0 if col is None else int(col.numel())
    LP._call(y_in, 'vg_umap_layout_epoch', LP._p(rowptr), LP._p(col), LP._p(eps), LP._p(y_in), N, nnz, n, n_epochs, float(a), float(b), neg,
             seed & M64, LP._p(out))
    _sync(dev)
    assert torch.equal(out[2 * N:].cpu(), torch.full((CANARIES,), GUARD)), 'wrote past y_out'
    return out[:2 * N].cpu().numpy().reshape(N, 2)


def run_layout(dev, cid):
    kind, n, n_epochs, neg, scale, seed = LAYOUT_CASES[cid]
    h = layout_host(dev, cid)
    a, b = ab()
    dv = lambda v: None if v is None else _t(v, dev)
    rowptr, col, eps, y_in = dv(h['rowptr']), dv(h['col']), dv(h['eps']), dv(h['y'])
    got = _epoch_call(dev, rowptr, col, eps, y_in, n, n_epochs, a, b, neg, seed)
    again = _epoch_call(dev, rowptr, col, eps, y_in, n, n_epochs, a, b, neg, seed)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), cid + ': the same call twice gives different bits'
    assert np.array_equal(y_in.cpu().numpy(), h['y']), cid + ': y_in was written'
    _check(cid, 'y_out', got, h['want'], LAYOUT_C * U * h['M'])
    cn = h['counts']
    moved = not np.array_equal(got, h['y'])
    if n == 0 or kind in ('no-edges', 'one-vertex'):
        assert np.array_equal(got.view(np.uint32), h['y'].view(np.uint32)), cid + ': nothing is due, y_out must be the bits of y_in'
    else:
        assert moved and cn['due'] > 0
    if kind == 'blobs':
        assert len(h['rowptr']) - 1 == 300 and 6000 < int(h['rowptr'][-1]) < 10000
        if scale < 1 and n < 199:
            assert cn['clipped'] > cn['due']                            # the clips at +-4 are active at this scale
        if neg and n >= 1:
            assert cn['self_neg'] > 0                                   # some negatives were the vertex itself
    if kind == 'coincident':
        assert cn['coincident'] >= 3
    if kind == 'one-vertex':
        assert layout_contributions(h['y'], h['rowptr'], h['col'], h['eps'], n, n_epochs, a, b, neg, seed, np.float64)[2] == \
            dict(due=1, coincident=1, self_neg=31, clipped=0)


def check_layout_restatements():
    """On the references alone: the vectorised fp32 restatement is the bits of the scalar one (ref_epoch), on a graph with due and
    undue edges, coincident vertices and clipped steps."""
    rng = np.random.default_rng(11)
    N = 40
    deg = rng.integers(0, 6, size=N)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, N, size=int(rowptr[-1])).astype(np.int32)
    eps = (1.0 / rng.uniform(0.05, 1.0, size=len(col))).astype(np.float32); eps[::3] = 1.0
    a, b = ab()
    for scale, n, neg in ((10.0, 3, 5), (0.05, 1, 31), (10.0, 49, 0)):
        y = (rng.uniform(0, 1, size=(N, 2)) * scale).astype(np.float32)
        y[col[0]] = y[0]
        want, M, y32, counts = ref_layout(y, rowptr, col, eps, n, 50, a, b, neg, 5)
        one = ref_epoch(y, rowptr, col, eps, n, 50, a, b, neg, 5)
        assert counts['due'] > 0 and np.array_equal(one.view(np.uint32), y32.view(np.uint32)), (scale, n, neg)


def run_layout_chain(dev):
    """LP.layout for three epochs is the bits of three single calls chained by hand"""
    rowptr, col, eps = [_t(v, dev) for v in layout_graph(dev, 'blobs')]
    a, b = ab()
    N = rowptr.numel() - 1
    y0 = (np.random.RandomState(5).uniform(0, 10, size=(N, 2))).astype(np.float32)
    got = LP.layout(_t(y0, dev), rowptr, col, eps, 3, a, b, 5, 77).cpu().numpy()
    y = _t(y0, dev)
    for n in range(3):
        y = _t(_epoch_call(dev, rowptr, col, eps, y, n, 3, a, b, 5, 77), dev)
    assert np.array_equal(got.view(np.uint32), y.cpu().numpy().view(np.uint32)) and not np.array_equal(got, y0)


def print_records():
    """worst err / bound per case family (DESIGN.md section 7.1 is filled from this)"""
    fam = {}
    for what, qty, worst in RECORDS:
        key = (what.split('-')[0] if not what[0].isdigit() else 'N', qty)
        fam[key] = max(fam.get(key, 0.0), worst)
    for what, qty, worst in RECORDS:
        print('RECORD %-28s %-22s %.3f' % (what, qty, worst))
    return fam
