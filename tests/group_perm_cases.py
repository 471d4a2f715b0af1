"""Shared bodies of the group-permutation tests: the sign-flip max-statistic kernel (ops.signflip_maxstat / vg_signflip_maxstat) against
a numpy reference, MapStatistics.group_permutation on synthetic accumulators, build_model_recons.mk_stat_maps with n_perm.  Run on CPU
tensors through the host build of the kernels (test_group_perm_emu.py) and on the GPU through libvaegam_hip.so
(test_group_perm_gpu.py).

No tolerance anywhere: include/vaegam.h defines the statistic to the bit (the signed sum by adds in ascending subject order from +0.0,
one multiplication by the scale, maxima and integer counts, which do not depend on an order), and `reference` below does exactly that in
numpy.  stat0 and maxstat are compared as int64 bit patterns, cnt_unc as integers.
"""
import os

import numpy as np
import torch

import vae_gam_amd  # noqa: F401
from vae_gam_amd import _lib, ops
from vae_gam_amd.map_statistics import MapStatistics

TAILS = ('two', 'pos', 'neg')
ARG, UNSUPPORTED = 1, 3
GUARD = 300                                                      # elements around every output


# ------------------------------------------------------------------------------------------------ the reference
def _g(x, tail):
    return np.abs(x) if tail == 'two' else (x if tail == 'pos' else -x)


def signed_sums(m, signs):
    """T [P, V]: from +0.0, for s ascending T = T + (bit s of the word ? -m[s] : m[s]) -- the explicit loop, adds only"""
    S, V = m.shape
    signs = np.asarray(signs).astype(np.uint64)
    T = np.zeros((signs.shape[0], V), dtype=np.float64)
    for s in range(S):
        flip = ((signs >> np.uint64(s)) & np.uint64(1)).astype(bool)
        T = T + np.where(flip[:, None], -m[s][None, :], m[s][None, :])
    return T


def reference(m, scale, signs, tail):
    """-> stat0 [V] float64, maxstat [P] float64, cnt_unc [V] int32, by the definitions of include/vaegam.h"""
    S, V = m.shape
    live = scale > 0
    T = signed_sums(m, signs)
    Tid = np.zeros(V, dtype=np.float64)
    for s in range(S):
        Tid = Tid + m[s]
    stat0 = np.where(live, _g(Tid * scale, tail), 0.0)
    g = _g(T * scale[None, :], tail) + 0.0                        # (-0.0 enters a maximum as +0.0)
    maxstat = g[:, live].max(1) if live.any() else np.full(T.shape[0], -np.inf)
    cnt = (_g(T, tail) >= _g(Tid, tail)[None, :]).sum(0).astype(np.int32)
    cnt[~live] = T.shape[0]
    return stat0, maxstat, cnt


# ------------------------------------------------------------------------------------------------ inputs
def random_m(S, V, seed=0):
    return np.random.default_rng(seed).standard_normal((S, V))


def scale_of(m):
    """1 / sqrt(S sum_s m^2) in torch float64, as the Python layer forms it (0 where that sum is 0)"""
    t = torch.from_numpy(np.ascontiguousarray(m))
    sq = (t ** 2).sum(0)
    ok = sq > 0
    return torch.where(ok, 1.0 / torch.where(ok, sq * m.shape[0], torch.ones_like(sq)).sqrt(), torch.zeros_like(sq)).numpy()


def random_signs(S, P, seed=1):
    """P words with random bits below S; word 0 is the identity"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=(P, S), dtype=np.uint64)
    w = np.zeros(P, dtype=np.uint64)
    for s in range(S):
        w |= bits[:, s] << np.uint64(s)
    w[0] = 0
    return w


def zero_scale(scale, kind, lanes):
    """scale with zeros planted: scattered, a whole wave, a whole block, every voxel but one"""
    V = scale.shape[0]
    out = scale.copy()
    if kind == 'scattered':
        out[np.random.default_rng(5).random(V) < 0.3] = 0.0
    elif kind == 'wave':
        out[64:128] = 0.0
    elif kind == 'block':
        out[lanes:2 * lanes] = 0.0
    elif kind == 'all_but_one':
        keep = V - 3
        out[:] = 0.0
        out[keep] = scale[keep]
    else:
        assert kind is None
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def plan(S, V, P):
    return ops.signflip_plan(S, V, P)


def lanes():
    return plan(2, 1, 1).lanes


def chunk():
    """permutations per chunk at the test sizes (few voxel tiles: the planner's minimum)"""
    return plan(2, 300, 1).chunk


# ------------------------------------------------------------------------------------------------ the raw launch between guards
class Outputs:
    """stat0, maxstat (float64) and cnt_unc (int32), each between two guard regions of random contents, on the device"""

    def __init__(self, dev, V, P, seed=9):
        g = torch.Generator().manual_seed(seed)
        self.V, self.P = V, P
        self.f_host = torch.randn(3 * GUARD + V + P, generator=g, dtype=torch.float64)
        self.i_host = torch.randint(-2 ** 31, 2 ** 31 - 1, (2 * GUARD + V,), generator=g, dtype=torch.int64).to(torch.int32)
        self.f, self.i = self.f_host.to(dev).clone(), self.i_host.to(dev).clone()
        self.stat0 = self.f[GUARD:GUARD + V]
        self.maxstat = self.f[2 * GUARD + V:2 * GUARD + V + P]
        self.cnt = self.i[GUARD:GUARD + V]

    def untouched(self):
        return torch.equal(self.f.cpu().view(torch.int64), self.f_host.view(torch.int64)) and torch.equal(self.i.cpu(), self.i_host)

    def guards_kept(self):
        f, h, V, P = self.f.cpu().view(torch.int64), self.f_host.view(torch.int64), self.V, self.P
        i, ih = self.i.cpu(), self.i_host
        spans = [(0, GUARD), (GUARD + V, 2 * GUARD + V), (2 * GUARD + V + P, 3 * GUARD + V + P)]
        return all(torch.equal(f[a:b], h[a:b]) for a, b in spans) and torch.equal(i[:GUARD], ih[:GUARD]) and \
            torch.equal(i[GUARD + V:], ih[GUARD + V:])


def raw_args(m, scale, signs, tail, ws, out, S=None, V=None, P=None):
    p = ops._p
    return (p(m), p(scale), p(signs), m.shape[0] if S is None else S, m.shape[1] if V is None else V,
            signs.shape[0] if P is None else P, tail, p(ws), p(out.stat0), p(out.maxstat), p(out.cnt))


def launch(dev, m, scale, signs, tail, seed=9):
    """vg_signflip_maxstat on numpy inputs, outputs between guards -> (Outputs, stat0, maxstat, cnt as numpy)"""
    S, V = m.shape
    P = signs.shape[0]
    mt = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
    st = torch.from_numpy(np.ascontiguousarray(scale)).to(dev)
    wt = torch.from_numpy(np.ascontiguousarray(signs).view(np.int64)).to(dev)
    ws = torch.empty(_lib.get_lib().size('vg_signflip_ws_bytes', S, V, P), dtype=torch.uint8, device=dev)
    out = Outputs(dev, V, P, seed)
    ops._call(mt, 'vg_signflip_maxstat', *raw_args(mt, st, wt, TAILS.index(tail), ws, out))
    return out, out.stat0.cpu().numpy(), out.maxstat.cpu().numpy(), out.cnt.cpu().numpy()


def check(dev, m, scale, signs, tail):
    """one launch against the reference, exactly; guards kept; a second launch gives the same bits; also through ops.signflip_maxstat"""
    want = reference(m, scale, signs, tail)
    out, stat0, maxstat, cnt = launch(dev, m, scale, signs, tail)
    assert out.guards_kept(), 'guard regions were written'
    assert np.array_equal(bits(stat0), bits(want[0])), 'stat0: %d voxels differ' % int((bits(stat0) != bits(want[0])).sum())
    assert np.array_equal(bits(maxstat), bits(want[1])), 'maxstat: %d permutations differ' % int((bits(maxstat) != bits(want[1])).sum())
    assert cnt.dtype == np.int32 and np.array_equal(cnt, want[2]), 'cnt_unc: %d voxels differ' % int((cnt != want[2]).sum())
    _, stat0b, maxstatb, cntb = launch(dev, m, scale, signs, tail, seed=10)
    assert np.array_equal(bits(stat0b), bits(stat0)) and np.array_equal(bits(maxstatb), bits(maxstat)) and np.array_equal(cntb, cnt), \
        'two launches on the same inputs differ'
    a, b, c = ops.signflip_maxstat(torch.from_numpy(m).to(dev), torch.from_numpy(scale).to(dev),
                                   torch.from_numpy(signs.view(np.int64)).to(dev), tail)
    assert np.array_equal(bits(a.cpu().numpy()), bits(stat0)) and np.array_equal(bits(b.cpu().numpy()), bits(maxstat))
    assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy(), cnt)
    return want


# ------------------------------------------------------------------------------------------------ kernel cases
S_CASES = [2, 8, 9, 16, 17, 32, 33, 63, 64]                      # every instance at its edges; 64 uses bit 63
V_CASES = ['1', 'tile-1', 'tile', 'tile+1', '4tiles+76']
P_CASES = ['1', 'chunk-1', 'chunk', 'chunk+1', '3chunks+8']
ZERO_CASES = ['scattered', 'wave', 'block', 'all_but_one']


def _size(name, unit):
    table = {'1': 1, 'tile-1': unit - 1, 'tile': unit, 'tile+1': unit + 1, '4tiles+76': 4 * unit + 76,
             'chunk-1': unit - 1, 'chunk': unit, 'chunk+1': unit + 1, '3chunks+8': 3 * unit + 8}
    return table[name]


def run_subjects_case(dev, S):
    """V = a tile and 44 voxels, P = a chunk and 6 permutations (two chunks), the tail cycling with S"""
    V, P = lanes() + 44, chunk() + 6
    assert plan(S, V, P).SMAX == (8 if S <= 8 else 16 if S <= 16 else 32 if S <= 32 else 64) and plan(S, V, P).chunks == 2
    m = random_m(S, V, seed=S)
    check(dev, m, scale_of(m), random_signs(S, P, seed=100 + S), TAILS[S % 3])


def run_every_instance_is_hit():
    assert {plan(S, lanes() + 44, chunk() + 6).SMAX for S in S_CASES} == {8, 16, 32, 64}


def run_voxels_case(dev, name):
    V = _size(name, lanes())
    assert V < 1500 and plan(5, V, 20).tiles == (V + lanes() - 1) // lanes()
    m = random_m(5, V, seed=3)
    check(dev, m, scale_of(m), random_signs(5, 20), 'two')


def run_permutations_case(dev, name):
    P = _size(name, chunk())
    V = lanes() + 1
    pl = plan(3, V, P)
    assert pl.chunks == (P + chunk() - 1) // chunk() and (name != '3chunks+8' or pl.chunks >= 3)
    m = random_m(3, V, seed=4)
    signs = random_signs(3, P) if P > 1 else np.zeros(1, dtype=np.uint64)          # (P = 1: the identity alone)
    want = check(dev, m, scale_of(m), signs, 'two')
    if P == 1:
        assert (want[2] == 1).all() and want[1][0] == want[0].max()


def run_tail_case(dev, tail):
    V, P = lanes() + 44, chunk() + 6
    m = random_m(12, V, seed=6)
    check(dev, m, scale_of(m), random_signs(12, P), tail)


def run_zero_scale_case(dev, kind, tail):
    V, P = 2 * lanes() + 88, chunk() + 6
    m = random_m(7, V, seed=8)
    scale = zero_scale(scale_of(m), kind, lanes())
    assert (scale == 0).sum() >= 64 and (scale > 0).any()
    want = check(dev, m, scale, random_signs(7, P), tail)
    dead = scale == 0
    assert (want[0][dead] == 0).all() and (want[2][dead] == P).all()


def run_polluted_maximum_case(dev):
    """tail pos, every mean negative, the identity alone, some voxels out: the maximum is the negative one of the live voxels, not 0"""
    V = lanes() + 44
    m = -np.abs(random_m(6, V, seed=12)) - 0.1
    scale = zero_scale(scale_of(m), 'scattered', lanes())
    signs = np.zeros(1, dtype=np.uint64)
    want = check(dev, m, scale, signs, 'pos')
    assert want[1][0] < 0 and want[1][0] == want[0][scale > 0].max()
    _, _, maxstat, _ = launch(dev, m, scale, signs, 'pos')
    assert maxstat[0] < 0


def run_ties_case(dev, tail):
    """exact ties: duplicate words, a word and its complement, means of +-0.0, columns of equal magnitudes"""
    S, V = 6, lanes() + 44
    m = random_m(S, V, seed=13)
    m[:, 3] = 0.0                                                                  # all +0.0, and alternating +-0.0: no part taken
    m[:, 4] = np.where(np.arange(S) % 2 == 0, -0.0, 0.0)
    m[:, 5] = 1.25 * np.where(np.arange(S) % 2 == 0, 1.0, -1.0)                    # equal magnitudes: many patterns sum to exactly 0
    m[:, 6] = 0.75
    m[2, 7] = 0.0                                                                  # zeros of either sign among live means
    m[3, 8] = -0.0
    full = np.uint64(2 ** S - 1)
    base = random_signs(S, 12, seed=14)
    comp = base ^ full                                                             # every complement (word 0's: all flipped)
    signs = np.concatenate([base, comp, base[3:6], comp[3:6]])                     # and duplicates of three pairs
    T = signed_sums(m, signs)
    assert np.array_equal(bits(np.abs(T[:12])), bits(np.abs(T[12:24])))            # |T| of a word and of its complement: the same bits
    scale = scale_of(m)
    assert (scale[3:5] == 0).all()
    want = check(dev, m, scale, signs, tail)
    if tail == 'two':
        live = scale > 0
        assert (want[2][live] >= 2).all() and (want[2][live] % 2 == 0).all()       # the identity and its complement; ties come in pairs


def run_hand_case(dev):
    """S = 4, all 16 patterns, every mean positive: only the identity (and, two-sided, its complement) reaches the observed sum"""
    m = np.array([[1.0, 0.5, 3.0], [2.0, 0.25, 1.0], [0.5, 4.0, 1.5], [1.5, 1.0, 0.125]])
    signs = np.arange(16, dtype=np.uint64)
    assert (check(dev, m, scale_of(m), signs, 'two')[2] == 2).all()
    assert (check(dev, m, scale_of(m), signs, 'pos')[2] == 1).all()
    assert (check(dev, m, scale_of(m), signs, 'neg')[2] == 16).all()


def _status(fn, *args):
    lib = _lib.get_lib()
    rc = getattr(lib.dll, fn)(*args)
    return int(rc), lib.dll.vg_last_error().decode()


def run_refusals_case(dev):
    """every refusal returns its status and leaves the outputs untouched; the workspace and plan queries agree"""
    lib = _lib.get_lib()
    S, V, P = 5, 40, 9
    m = torch.from_numpy(random_m(S, V)).to(dev)
    big = torch.zeros(65, V, dtype=torch.float64, device=dev)     # 65 subjects, so that no refused launch could read past its input
    scale = torch.from_numpy(scale_of(m.cpu().numpy())).to(dev)
    signs = torch.from_numpy(random_signs(S, P).view(np.int64)).to(dev)
    ws = torch.empty(lib.size('vg_signflip_ws_bytes', S, V, P), dtype=torch.uint8, device=dev)
    out = Outputs(dev, V, P)
    a = lambda **k: raw_args(k.pop('m', m), scale, signs, k.pop('tail', 0), ws, out, **k) + (None,)      # noqa: E731
    nul = lambda i: tuple(None if j == i else v for j, v in enumerate(a()))                              # noqa: E731
    cases = [('S = 1', ARG, a(S=1)), ('S = 0', ARG, a(S=0)), ('V = 0', ARG, a(V=0)), ('V < 0', ARG, a(V=-4)), ('V = 2^31', ARG, a(V=2 ** 31)),
             ('P = 0', ARG, a(P=0)), ('P < 0', ARG, a(P=-1)), ('P > 2^20', ARG, a(P=2 ** 20 + 1)), ('tail 3', ARG, a(tail=3)),
             ('tail -1', ARG, a(tail=-1)), ('S = 65', UNSUPPORTED, a(m=big, S=65))] + \
            [('null argument %d' % i, ARG, nul(i)) for i in (0, 1, 2, 7, 8, 9, 10)]
    for what, status, args in cases:
        rc, text = _status('vg_signflip_maxstat', *args)
        assert rc == status and 'vg_signflip_maxstat' in text, (what, rc, text)
        assert ('more than 64 subjects' in text) == (status == UNSUPPORTED), (what, text)
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    assert out.untouched(), 'a refused call wrote to the outputs'
    rec = (_lib.i32 * len(_lib.SIGNFLIP_PLAN_FIELDS))()
    for shape in [(5, 40, 9), (2, 1, 1), (64, 2 ** 31 - 1, 2 ** 20), (1, 40, 9), (65, 40, 9), (5, 0, 9), (5, 2 ** 31, 9), (5, 40, 0),
                  (5, 40, 2 ** 20 + 1), (0, 40, 9), (5, -1, 9)]:
        nbytes = int(lib.dll.vg_signflip_ws_bytes(*shape))
        rc, text = _status('vg_signflip_plan', *shape, rec, len(rec))
        assert (rc == 0) == (nbytes != -1), (shape, rc, nbytes)
        if rc == 0:
            p = dict(zip(_lib.SIGNFLIP_PLAN_FIELDS, rec))
            assert nbytes == p['ws_lo'] + (p['ws_hi'] << 31) == p['tiles'] * shape[2] * 8 + p['chunks'] * shape[1] * 4
            assert (p['grid_x'], p['grid_y']) == (p['tiles'], p['chunks']) and p['chunk'] % 16 == 0 and p['chunks'] * p['chunk'] >= shape[2]
            assert p['fold_blocks'] == (shape[2] + p['lanes'] - 1) // p['lanes'] + p['tiles'] and p['grid_y'] <= 65535
        else:
            assert rc == (UNSUPPORTED if shape[0] > 64 else ARG) and 'vg_signflip_plan' in text
    assert _status('vg_signflip_plan', 5, 40, 9, rec, len(rec) - 1)[0] == ARG and _status('vg_signflip_plan', 5, 40, 9, None, len(rec))[0] == ARG
    with np.testing.assert_raises(ValueError):
        ops.signflip_maxstat(m, scale, signs, 'both')
    assert out.untouched()


def run_real_size_case(dev):
    """GPU only: V = 70,315, S = 20, P = 2,000, two-sided, against the same ordered adds in torch float64 on the device, 250
    permutations at a time"""
    S, V, P = 20, 70315, 2000
    m = torch.from_numpy(random_m(S, V, seed=21)).to(dev)
    scale = torch.from_numpy(scale_of(m.cpu().numpy())).to(dev)
    scale[torch.from_numpy(np.random.default_rng(22).random(V) < 0.2).to(dev)] = 0.0
    signs = torch.from_numpy(random_signs(S, P, seed=23).view(np.int64)).to(dev)
    stat0, maxstat, cnt = ops.signflip_maxstat(m, scale, signs, 'two')
    live = scale > 0
    Tid = torch.zeros(V, dtype=torch.float64, device=dev)
    for s in range(S):
        Tid = Tid + m[s]
    want_max, want_cnt = [], torch.zeros(V, dtype=torch.int64, device=dev)
    for lo in range(0, P, 250):
        w = signs[lo:lo + 250]
        T = torch.zeros(w.shape[0], V, dtype=torch.float64, device=dev)
        for s in range(S):
            T = T + torch.where(((w >> s) & 1).bool()[:, None], -m[s][None, :], m[s][None, :])
        want_max.append((T * scale[None, :]).abs()[:, live].amax(1))
        want_cnt += (T.abs() >= Tid.abs()[None, :]).sum(0)
    want_cnt[~live] = P
    i64 = lambda t: t.contiguous().view(torch.int64)             # noqa: E731
    assert torch.equal(i64(maxstat), i64(torch.cat(want_max)))
    assert torch.equal(cnt.long(), want_cnt)
    assert torch.equal(i64(stat0), i64(torch.where(live, (Tid * scale).abs(), torch.zeros_like(Tid))))
    pl = plan(S, V, P)
    assert pl.SMAX == 32 and pl.tiles == 275 and pl.chunks >= 2


# ------------------------------------------------------------------------------------------------ MapStatistics.group_permutation
def make_stats(dev, m):
    """a MapStatistics whose subject means of 'base' are m [S, V] (one volume per subject, no covariate), straight from accumulators"""
    S, V = m.shape
    acc = torch.zeros(S, 8, V, dtype=torch.float64)
    acc[:, 0] = torch.from_numpy(np.ascontiguousarray(m))
    return MapStatistics(acc.to(dev), torch.ones(S, dtype=torch.float64, device=dev), ['base', 'full_rec'])


def run_basics_case(dev):
    S, V = 7, 700
    m = random_m(S, V, seed=31)
    m[:, 10] = 0.0                                                # all zero: as outside a mask
    m[:, 11] = 0.625                                              # all equal: sd = 0
    m[:, 12:40] += 2.0
    st = make_stats(dev, m)
    undefined = np.zeros(V, dtype=bool)
    undefined[10:12] = True
    h = lambda t: t.cpu().numpy()                                 # noqa: E731
    for tail in TAILS:
        for n_perm in (100, 128, 200):                            # 2^7 = 128: sampled below it, exhaustive from it on
            r = st.group_permutation('base', n_perm=n_perm, seed=3, tail=tail)
            P = r.n_perm
            assert r.exhaustive == (2 ** S <= n_perm) and P == (128 if r.exhaustive else n_perm) and r.tail == tail
            assert r.signs.shape == (P,) and int(r.signs[0]) == 0 and r.max_stat.shape == (P,) and r.stat.shape == (V,)
            if r.exhaustive:
                assert h(r.signs).tolist() == list(range(128))
            assert torch.equal(r.t.view(torch.int64), st.group_t('base').view(torch.int64))
            assert (h(st.group_t('base'))[undefined] == 0).all() and (h(st.group_t('base'))[~undefined] != 0).all()
            pu, pf, stat = h(r.p_unc), h(r.p_fwe), h(r.stat)
            for p in (pu, pf):
                assert p.dtype == np.float64 and (p >= 1.0 / P).all() and (p <= 1.0).all()
            assert (pf >= pu).all()
            order = np.argsort(stat[~undefined], kind='stable')
            assert (np.diff(pf[~undefined][order]) <= 0).all(), 'p_fwe increases with the statistic'
            assert (pu[undefined] == 1).all() and (pf[undefined] == 1).all() and (stat[undefined] == 0).all()
            # against the reference on the same inputs: the scale is the one the layer formed on this device (a sum over the subjects in
            # torch, whose order is the device's), checked here against the host's to the rounding of that sum
            scale = h(r.scale)
            assert (scale[undefined] == 0).all() and np.allclose(scale[~undefined], scale_of(m)[~undefined], rtol=1e-14, atol=0)
            want = reference(m, scale, h(r.signs).view(np.uint64), tail)
            assert np.array_equal(bits(stat), bits(want[0])) and np.array_equal(bits(h(r.max_stat)), bits(want[1]))
            assert np.array_equal(pu, want[2] / P)
            assert np.array_equal(pf[~undefined], (want[1][None, :] >= want[0][~undefined][:, None]).sum(1) / P)
    a = st.group_permutation('base', n_perm=100, seed=3)
    b = st.group_permutation('base', n_perm=100, seed=3)
    c = st.group_permutation('base', n_perm=100, seed=4)
    i64 = lambda t: t.contiguous().view(torch.int64)              # noqa: E731
    assert torch.equal(a.signs, b.signs) and all(torch.equal(i64(getattr(a, k)), i64(getattr(b, k))) for k in ('stat', 'max_stat', 'p_unc', 'p_fwe'))
    assert not torch.equal(a.signs, c.signs)
    # the patterns: bit s of a word from column s of the CPU generator's draw
    draw = torch.randint(0, 2, (99, S), generator=torch.Generator('cpu').manual_seed(3)).numpy()
    assert h(a.signs)[1:].tolist() == [int(sum(int(b_) << s for s, b_ in enumerate(row))) for row in draw]


def run_errors_case(dev):
    m = random_m(4, 50, seed=32)
    st = make_stats(dev, m)
    bad = [dict(n_perm=0), dict(n_perm=-5), dict(n_perm=2 ** 20 + 1), dict(tail='both'), dict(tail=0)]
    for kw in bad:
        with np.testing.assert_raises(ValueError):
            st.group_permutation('base', **kw)
    with np.testing.assert_raises(ValueError):
        make_stats(dev, m[:1]).group_permutation('base')          # S < 2
    with np.testing.assert_raises(ValueError):
        make_stats(dev, random_m(65, 5)).group_permutation('base', n_perm=10)      # S > 64
    with np.testing.assert_raises(ValueError):
        make_stats(dev, np.full((4, 50), 0.5)).group_permutation('base')           # no voxel with a defined statistic
    with np.testing.assert_raises(KeyError):
        st.group_permutation('nothing')
    assert st.group_permutation('base', n_perm=1).n_perm == 1
    assert make_stats(dev, random_m(64, 5)).group_permutation('base', n_perm=70, tail='neg').n_perm == 70


_PLANTED = {}


def planted(dev):
    """S = 12, V = 2,000, standard normal with +6 on voxels 0..19, all 4,096 patterns, two-sided: one run per device, shared"""
    if str(dev) not in _PLANTED:
        m = np.random.default_rng(7).standard_normal((12, 2000))
        m[:, :20] += 6.0
        _PLANTED[str(dev)] = (m, make_stats(dev, m).group_permutation('base', n_perm=4096, tail='two'))
    return _PLANTED[str(dev)]


def run_planted_signal_case(dev):
    m, r = planted(dev)
    assert r.exhaustive and r.n_perm == 4096
    pf = r.p_fwe.cpu().numpy()
    assert (pf[:20] == 2.0 / 4096).all(), pf[:20]
    assert (pf[20:] > 0.05).all(), int((pf[20:] <= 0.05).sum())
    assert (r.p_unc.cpu().numpy()[:20] == 2.0 / 4096).all()


def run_threshold_case(dev):
    m, r = planted(dev)
    mx = np.sort(r.max_stat.cpu().numpy())
    for alpha in (0.05, 0.01, 0.5):
        k = int(np.ceil((1.0 - alpha) * 4096))
        u = mx[k - 1]
        assert r.threshold(alpha) == u * np.sqrt(11.0 / (1.0 - u * u))
        # what the critical value is for: corrected p <= alpha exactly where the statistic exceeds it
        assert np.array_equal(r.p_fwe.cpu().numpy() <= alpha, r.stat.cpu().numpy() > u)
    assert r.threshold(0.0) == mx[-1] * np.sqrt(11.0 / (1.0 - mx[-1] ** 2))
    one = make_stats(dev, np.array([[1.0, 2.0], [1.0, 0.5], [1.0, 1.0]]))          # voxel 0: undefined; voxel 1 under (+, +, +): u < 1
    assert np.isfinite(one.group_permutation('base', n_perm=8).threshold(0.05))
    neg = make_stats(dev, m).group_permutation('base', n_perm=300, tail='neg')
    pos = make_stats(dev, m).group_permutation('base', n_perm=300, tail='pos')
    assert neg.threshold(0.05) < 0 < pos.threshold(0.05)
    # (1, -1) with one of the two flipped: both subjects agree exactly, u = 2 / sqrt(2 * 2) = 1, t = inf
    assert make_stats(dev, np.array([[1.0], [-1.0]])).group_permutation('base', n_perm=4).threshold(0.05) == np.inf


# ------------------------------------------------------------------------------------------------ files
class _StubModel:
    """what mk_stat_maps needs of a model: the epoch, the grid and map_statistics -- here three subjects whose maps are 1 + 1 % noise
    inside an ellipsoid mask and 0 outside, straight from accumulators"""
    epoch, img_shape = 1, (19, 21, 20)

    def __init__(self, dev):
        import mask_cases as MC
        self.mask = MC.ellipsoid_mask(self.img_shape)
        inside = self.mask.reshape(-1).numpy().astype(bool)
        acc = np.zeros((3, 11, inside.shape[0]))
        acc[:, :3] = (1.0 + 0.01 * np.random.default_rng(41).standard_normal((3, 3, inside.shape[0]))) * inside
        self.stats = MapStatistics(torch.from_numpy(acc).to(dev), torch.ones(3, dtype=torch.float64, device=dev), ['base', 'task', 'full_rec'])

    def map_statistics(self, loader, num_subjects=None, at_mean=False):
        assert num_subjects == 3
        return self.stats


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def run_stat_maps_files(dev, tmp_path):
    """mk_stat_maps without and with n_perm on three subjects (all 8 patterns): the second call adds exactly the new files and every
    other file is byte for byte the same; 1 - p finite, in [0, 1], 0 outside the mask, at most 1 - 2 / 8; the table"""
    import filecmp
    import pandas as pd
    from vae_gam_amd import DataClass_GP as D, build_model_recons as R
    model = _StubModel(dev)
    csv = str(tmp_path / 'subjects.csv')
    with open(csv, 'w') as f:
        f.write('idx,subjid,vol,nii_path\n0,sA,0,none_a\n1,sB,0,none_b\n2,sC,0,none_c\n')
    R.mk_stat_maps(csv, model, str(tmp_path / 'plain'), None)
    R.mk_stat_maps(csv, model, str(tmp_path / 'perm'), None, n_perm=64, perm_seed=1)
    sub = os.path.join('reconstructions', '001_stat_model_recons')
    maps = ['base', 'task', 'full_rec']
    new = ['%s_%s_1mp.nii' % (k, c) for k in maps for c in ('fwe', 'unc')] + ['perm_thresholds.csv']
    plain, perm = _files(str(tmp_path / 'plain')), _files(str(tmp_path / 'perm'))
    assert sorted(perm) == sorted(plain + [os.path.join(sub, f) for f in new]) and len(plain) == 4 + 3 * 5
    for f in plain:
        assert filecmp.cmp(str(tmp_path / 'plain' / f), str(tmp_path / 'perm' / f), shallow=False), f
    root = tmp_path / 'perm' / sub
    outside = ~model.mask.numpy().astype(bool)
    for f in new[:-1]:
        a = np.asarray(D.read_nifti1(str(root / f))).reshape(model.img_shape)
        assert np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all() and (a[outside] == 0).all(), f
        assert (a[~outside] == 1.0 - 2.0 / 8.0).all(), f         # the maps agree in sign everywhere: only the identity and its complement reach
    tab = pd.read_csv(str(root / 'perm_thresholds.csv'))
    assert list(tab.columns) == ['map', 'tail', 'P', 'exhaustive', 't_crit_0.05', 'n_fwe_0.05']
    assert tab['map'].tolist() == maps and (tab['tail'] == 'two').all() and (tab['P'] == 8).all() and tab['exhaustive'].all()
    assert (tab['n_fwe_0.05'] == 0).all() and (tab['t_crit_0.05'] > 0).all() and np.isfinite(tab['t_crit_0.05']).all()
    # a map that is the same in every subject has nothing to test: zeros and a row with P = 0, not an error
    model.stats.acc[:, 1] = torch.from_numpy((~outside).reshape(-1).astype(np.float64)).to(dev)
    R.mk_stat_maps(csv, model, str(tmp_path / 'flat'), None, n_perm=64)
    flat = pd.read_csv(str(tmp_path / 'flat' / sub / 'perm_thresholds.csv'))
    assert flat['P'].tolist() == [8, 0, 8] and flat['n_fwe_0.05'].tolist() == [0, 0, 0]
    assert (np.asarray(D.read_nifti1(str(tmp_path / 'flat' / sub / 'task_fwe_1mp.nii'))) == 0).all()
