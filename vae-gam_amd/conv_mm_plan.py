"""Host-side planner of the matrix-core convolution (vg_conv_mm, include/vaegam.h): pure index arithmetic, no launch.

mm_plan(spec, direction, read size, write size) -> MmPlan or None, built in three steps:
  _mm_classes   the tap classes of the launch and the position grid they are computed on;
  _mm_tables    the window-offset tables and the A-image index of those classes;
  _mm_tile      the block tile: the candidates, their LDS / occupancy arithmetic, the score and the measured pins (_MM_TUNED).
What decides WHETHER a launch takes the plan (USE_MM, mm_wins) and the launch itself (conv_mm) live in ops.py, which re-exports
MmPlan and mm_plan."""
from collections import namedtuple
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _lib

_MM_LDS_BUDGET = 150 * 1024
_MM_LDS_CU = 160 * 1024                                     # LDS of a CU: what co-resident blocks share
# (mode, stride, CI, CO, kernel, read size, write size) -> (waves, PD, PHB, cc, dbuf): tools/diag/mm_sweep.py at batch 64, 8 covariates
_MM_TUNED = {
    ('corr', 1, 16, 16, (3, 3, 3), (6, 8, 5), (8, 10, 7)): (8, 4, 10, 16, 0),    # convt1 forward 66.7 us (score's choice: 78)
    ('corr', 1, 16, 16, (3, 3, 3), (8, 10, 7), (6, 8, 5)): (8, 3, 8, 16, 0),     # convt1 data gradient 37.8
    ('corr', 2, 16, 16, (3, 3, 3), (16, 21, 14), (8, 10, 7)): (8, 2, 10, 8, 0),   # convt2 data gradient 83.2
    ('corr', 1, 16, 8, (3, 3, 3), (17, 21, 14), (19, 23, 16)): (8, 1, 23, 8, 0),  # conv3 data gradient 61.6
    ('corr', 1, 8, 16, (3, 3, 3), (19, 23, 16), (17, 21, 14)): (8, 1, 21, 8, 0),  # conv3 forward 46 (score's choice, a 6-row slab: 51)
    ('corr', 1, 8, 16, (3, 3, 3), (18, 23, 16), (16, 21, 14)): (8, 2, 11, 8, 1),  # convt3 data gradient 242 (whole planes: 254)
    ('tconv', 2, 8, 8, (5, 3, 3), (18, 23, 16), (39, 47, 33)): (8, 2, 12, 8, 1),   # convt4 forward 610 (whole planes, single buffer: 656 in the same run)
    # two channel halves (the score's choices; the runners-up of the sweep behind them)
    ('tconv', 2, 16, 16, (3, 3, 3), (8, 10, 7), (16, 21, 14)): (8, 5, 11, 16, 0),  # convt2 forward 138-142 (3 planes, double-buffered: 158; 4-wave blocks of 2 planes: 166)
    ('tconv', 2, 16, 16, (3, 3, 3), (18, 22, 15), (37, 45, 31)): (8, 1, 23, 16, 0),  # 82x98x70 convt2 forward 1619-1686 (4 planes x 8-row slabs: 1747; double-buffered: 1856)
}


@dataclass(eq=False)
class MmPlan:
    """Host-side description of one conv / transposed-conv launch for vg_conv_mm (include/vaegam.h): position grid, staging
    geometry and the window-offset tables, plus `aidx` -- for every A-image slot the index of the weight it holds inside the
    layer's own weight tensor (-1 = zero).  CO: channels of y; co_blk: channels a block computes (CO, or 8 of 16: two halves, whose
    images sit back to back in `aidx`).  The scalar and per-class fields carry the names of vg_mm_desc's."""
    mode: str                      # 'corr' | 'tconv'
    CI: int
    CO: int
    co_blk: int
    ID: int
    IH: int
    IW: int
    OD: int
    OH: int
    OW: int
    nq: int                        # tap classes: 1, or the 4 (d, h) output parities of a stride-2 transposed conv
    ks: List[int]                  # per class: k-steps of 4 taps
    PDT: int                       # position grid
    PH: int
    PW: int
    PD: int                        # a block's tile: PD planes x PHB rows, `waves` waves, tpc tiles per wave, cc channels per chunk
    PHB: int
    waves: int
    tpc: int
    cc: int
    dbuf: int
    LD: int
    sdi: int                       # read strides of the position grid, first staged plane, write strides and per-class origins
    shi: int
    swi: int
    d0: int
    sdo: int
    sho: int
    swo: int
    od0: List[int]
    oh0: List[int]
    ow0: List[int]
    slack: int
    hlo: int
    hhi: int
    tau: np.ndarray                # int32, flat: [k-step row][4] element offsets, [row][4][3] (d, h, w) offsets, the A-image index
    dlt: np.ndarray
    aidx: np.ndarray
    _dev: dict = field(default_factory=dict, repr=False)     # device -> (tau, dlt, aidx) tensors

    def tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.tau).to(device), torch.from_numpy(self.dlt).to(device), torch.from_numpy(self.aidx).to(device))
        return self._dev[key]

    def desc(self, N, relu_in, per_group, relu_out=False):
        d = _lib.MmDesc()
        # what the launch decides; CO / co_tot: channels per block (the matrix rows' channels), channels of y
        launch = dict(N=int(N), relu_in=int(bool(relu_in)), per_group=int(per_group), relu_out=int(bool(relu_out)),
                      CO=int(self.co_blk), co_tot=int(self.CO))
        for name, ctype in _lib.MmDesc._fields_:
            if name in launch:
                setattr(d, name, launch[name])
            elif ctype is _lib.i32:
                setattr(d, name, int(getattr(self, name)))
            else:                                                        # one value per tap class
                own, arr = getattr(self, name), getattr(d, name)
                for q in range(4):
                    arr[q] = int(own[q]) if q < self.nq else 0
        return d

    def gather(self, weight):
        """A image from a weight tensor (layer tests / un-packed path; the model gathers all layers in one launch)."""
        _, _, aidx = self.tables(weight.device)
        flat = weight.detach().reshape(-1)
        a = flat[aidx.clamp_min(0).long()]
        return torch.where(aidx >= 0, a, torch.zeros_like(a)).contiguous()


def _mm_problem(spec, direction: str, in_size):
    """-> (mode, S, lead_pad, CI_l, CO_l, K, out_size, widx) of the launch: mode 'corr' (strided correlation with leading zero
    padding) or 'tconv' (stride-2 transposed convolution, gather form); widx(cin, kd, kh, kw, cout) = flat index of that weight in
    the layer's own weight tensor (conv: [co][ci][k], convt: [ci][co][k])."""
    KD, KH, KW = spec.k
    kvol = KD * KH * KW
    conv = spec.kind == 'conv'

    def w_at(ci_layer, co_layer, kd, kh, kw):
        t = (kd * KH + kh) * KW + kw
        return ((co_layer * spec.ci + ci_layer) if conv else (ci_layer * spec.co + co_layer)) * kvol + t
    fl = lambda kd, kh, kw: (KD - 1 - kd, KH - 1 - kh, KW - 1 - kw)
    if direction == 'fwd':
        osz = spec.out_size(in_size)
        if conv:
            return 'corr', spec.stride, (0, 0, 0), spec.ci, spec.co, spec.k, osz, (lambda cin, kd, kh, kw, cout: w_at(cin, cout, kd, kh, kw))
        if spec.stride == 1:
            pad = tuple(spec.k[a] - 1 - spec.pad[a] for a in range(3))
            return 'corr', 1, pad, spec.ci, spec.co, spec.k, osz, (lambda cin, kd, kh, kw, cout: w_at(cin, cout, *fl(kd, kh, kw)))
        return 'tconv', 2, tuple(spec.pad), spec.ci, spec.co, spec.k, osz, (lambda cin, kd, kh, kw, cout: w_at(cin, cout, kd, kh, kw))
    # data gradient: in_size is the size of dy (the layer's OUTPUT); the launch writes the layer's input size, which the caller passes
    if conv:
        if spec.stride == 1:
            pad = tuple(spec.k[a] - 1 for a in range(3))
            return 'corr', 1, pad, spec.co, spec.ci, spec.k, None, (lambda cin, kd, kh, kw, cout: w_at(cout, cin, *fl(kd, kh, kw)))
        return 'tconv', 2, (0, 0, 0), spec.co, spec.ci, spec.k, None, (lambda cin, kd, kh, kw, cout: w_at(cout, cin, kd, kh, kw))
    return 'corr', spec.stride, tuple(spec.pad), spec.co, spec.ci, spec.k, None, (lambda cin, kd, kh, kw, cout: w_at(cout, cin, kd, kh, kw))


_MM_PLANS = {}


def mm_plan(spec, direction: str, in_size, out_size=None, force=None) -> Optional[MmPlan]:
    """Plan for vg_conv_mm, or None when the launch is not covered (1-channel ends, shapes that do not fit LDS): the caller then
    uses the register-tiled kernels.  A stride-2 transposed conv with 16 output channels (forward of a convt layer with co == 16,
    data gradient of a conv layer with ci == 16) is planned as two halves of 8 channels: plan.CO = 16, plan.co_blk = 8.
    `spec`: the layer's ops.ConvSpec; `in_size`: spatial size of the tensor the launch READS (the layer input for 'fwd', dy for
    'bwd'); `out_size`: spatial size it writes (needed for 'bwd'); force = (waves, PD, PHB, cc, dbuf): tuning sweeps (tools/diag) and
    tests pin the tile instead of taking the scored choice."""
    key = (spec, direction, tuple(in_size), None if out_size is None else tuple(out_size), force)
    if key in _MM_PLANS:
        return _MM_PLANS[key]
    mode, S, pad, CI, CO, K, osz, widx = _mm_problem(spec, direction, tuple(in_size))
    if osz is None:
        osz = tuple(out_size)
    plan = None
    if CO in (8, 16) and CI >= 8:
        plan = _mm_build(mode, S, pad, CI, CO, K, tuple(in_size), tuple(osz), widx, force)
    _MM_PLANS[key] = plan
    return plan


# classes: per class a list of (dd, dh, dw, tap) -- the window offset of the entry and tap(rho) -> (kd, kh, kw) or None, the kernel tap
# it holds for the rho-th of the NR position replicas a 16-row tile carries; ld_of(PD): staged planes of a tile of PD position planes
_MmGrid = namedtuple('_MmGrid', 'classes PDT PH PW sdi shi swi sdo sho swo od0 oh0 ow0 d0 ld_of')


def _mm_classes(mode, S, pad, K, osz, NR) -> _MmGrid:
    """Tap classes and position grid of a launch."""
    KD, KH, KW = K
    OD, OH, OW = osz
    if mode == 'corr':
        KWp = KW + (NR - 1) * S
        ent = []
        for kd in range(KD):
            for kh in range(KH):
                for kwp in range(KWp):
                    def tap(rho, kd=kd, kh=kh, kwp=kwp):
                        kw = kwp - rho * S
                        return (kd, kh, kw) if 0 <= kw < KW else None
                    ent.append((kd - pad[0], kh - pad[1], kwp - pad[2], tap))
        return _MmGrid([ent], OD, OH, (OW + NR - 1) // NR, S, S, NR * S, 1, 1, NR, [0], [0], [0], -pad[0], lambda PD: (PD - 1) * S + KD)
    assert NR == 2 and S == 2
    MDm = (KD + 1) // 2
    classes, od0, oh0, ow0 = [], [], [], []
    for rd, rh in ((0, 0), (0, 1), (1, 0), (1, 1)):                # output parity in d and h; the w parities are the two replicas
        ent = []
        for md in range((KD - rd + 1) // 2):
            for mh in range((KH - rh + 1) // 2):
                for mw in range(2):
                    def tap(rho, rd=rd, rh=rh, md=md, mh=mh, mw=mw):
                        kw = rho + 2 * mw
                        return (rd + 2 * md, rh + 2 * mh, kw) if kw < KW else None
                    ent.append((-md, -mh, -mw, tap))
        classes.append(ent)
        od0.append(rd - pad[0]); oh0.append(rh - pad[1]); ow0.append(-pad[2])
    return _MmGrid(classes, (OD + pad[0] + 1) // 2, (OH + pad[1] + 1) // 2, (OW + pad[2] + 1) // 2, 1, 1, 1, 2, 2, 2, od0, oh0, ow0,
                   -(MDm - 1), lambda PD: PD + MDm - 1)


def _mm_tables(classes, widx, CI, CO_l, nco, IH, IW):
    """-> (ks, tau, dlt, aidx, slack, hlo, hhi) of the classes: per class ks k-steps of 4 taps; tau / dlt [k-step row][4] the element and
    (d, h, w) offsets of a step's windows; aidx per channel half the classes' A images [CI][ks][64 lanes] back to back."""
    ks = [(len(e) + 3) // 4 for e in classes]
    rows = sum(ks)
    tau = np.zeros((rows, 4), np.int32); dlt = np.zeros((rows, 4, 3), np.int32)
    aidx = [[] for _ in range(nco)]
    slack = 0
    r0 = 0
    for q, ent in enumerate(classes):
        a = -np.ones((nco, CI, ks[q], 64), np.int32)
        for s in range(ks[q]):
            for kk in range(4):
                kap = 4 * s + kk
                dd, dh, dw, tap = ent[kap] if kap < len(ent) else ent[0]     # padding entries: any readable offset, zero weights
                tau[r0 + s, kk] = dd * IH * IW + dh * IW + dw
                dlt[r0 + s, kk] = (dd, dh, dw)
                slack = max(slack, abs(dh) * IW + abs(dw) + 1)
                if kap >= len(ent):
                    continue
                for row in range(16):
                    rho, co = row // CO_l, row % CO_l
                    t = tap(rho)
                    if t is None:
                        continue
                    lane = kk * 16 + row
                    for h in range(nco):
                        for ci in range(CI):
                            a[h, ci, s, lane] = widx(ci, t[0], t[1], t[2], co + CO_l * h)
        for h in range(nco):
            aidx[h].append(a[h].reshape(-1))
        r0 += ks[q]
    aidx = np.concatenate([np.concatenate(a) for a in aidx])
    return ks, tau.reshape(-1), dlt.reshape(-1), aidx, slack, int(dlt[:, :, 1].min()), int(dlt[:, :, 1].max())


def _mm_tile(g: _MmGrid, ks, aimg_blk, hlo, hhi, CI, isz, pin):
    """-> (PD, LD, cc, tpc, dbuf, PHB, waves) of the block tile, or None when nothing fits.  aimg_blk: elements of the A image a block
    keeps in LDS; pin = (waves, PD, PHB, cc, dbuf): only that candidate is considered."""
    _, IH, IW = isz
    nq, rows = len(ks), sum(ks)
    PDT, PH, PW, sdi, shi = g.PDT, g.PH, g.PW, g.sdi, g.shi
    tpc_max = (8 if max(ks) <= 12 else 3) if nq == 1 else 4        # registers: one operand offset per (tile, k-step)
    # Tile choice: a block = W waves on PD position planes x PHB position rows (x all PW columns).  Measured (tools/diag/mm_sweep.py,
    # MI355X): what pays is SEVERAL co-resident blocks per CU -- their input waits, prologues, barriers and epilogues interleave with
    # each other's matrix phases -- i.e. a small LDS footprint (single-buffered input, row slabs instead of whole planes) and at most
    # 3 tiles per wave (the 128-register instances: 4 waves per SIMD); then full accumulator columns, a small halo and large channel
    # chunks.  _MM_TUNED pins the bench geometries where the sweep found a better tile than this score.
    cands = []
    for W in (8, 4):
        for PD in range(min(PDT, 16), 0, -1):
            LD = g.ld_of(PD)
            for nslab in (1, 2, 3, 4, 6, 8, 12):
                PHB = (PH + nslab - 1) // nslab
                if nslab > 1 and ((PH + PHB - 1) // PHB != nslab or PHB < 2):
                    continue
                npos = PD * PHB * PW
                tpc = (npos + W * 16 - 1) // (W * 16)
                if tpc > tpc_max:
                    continue
                rows_max = min((PHB - 1) * shi + (hhi - hlo) + 1, IH)
                whole = (nslab == 1 and hlo <= 0 and (PH - 1) * shi + hhi + 1 >= IH)
                LPH = IH * IW if whole else ((rows_max * IW + 3) // 4) * 4 + 4
                CHP = 64 + ((LD * LPH + 63) // 64) * 64
                for cc in ([CI] if nq > 1 else [c for c in range(CI, 0, -1) if CI % c == 0]):
                    for dbuf in (1, 0):
                        if pin and (W, PD, PHB, cc, dbuf) != tuple(pin):
                            continue
                        lds = (((aimg_blk + 63) // 64) * 64 + rows * 64 + (1 + dbuf) * cc * CHP + 64) * 4
                        if lds > _MM_LDS_BUDGET:
                            continue
                        per_simd = 4 if (tpc <= 3 or nq > 1) else 2                               # waves per SIMD the instance's registers allow
                        nblk = min(_MM_LDS_CU // lds, per_simd * 4 // W)
                        if nblk < 1:
                            continue
                        util = npos / float(tpc * W * 16) * (PDT / float(((PDT + PD - 1) // PD) * PD)) * (PH / float(nslab * PHB))   # filled accumulator columns
                        halo = ((PD * sdi) / float(LD)) * min(1.0, (PHB * shi) / float(rows_max))        # useful share of the staged elements
                        wps = nblk * W // 4                                                        # co-resident waves per SIMD
                        occ = {1: 0.45, 2: 0.6, 3: 0.8}.get(wps, 1.0)
                        # whole planes in 8-wave blocks measured best wherever they fit (41x49x35: row slabs / 4-wave blocks 3-20 % slower:
                        # more halo rows, fewer waves to balance a block's tiles over); slabs are what lets the 82x98x70 planes in at all
                        shape = (1.0 if nslab == 1 else 0.85) * (1.0 if W == 8 else 0.9)
                        score = util * (0.5 + 0.5 * halo) * (0.9 + 0.1 * cc / float(CI)) * occ * shape * (1.0 if (dbuf or nblk >= 2) else 0.9)
                        cands.append((score, PD, LD, cc, tpc, dbuf, PHB, W))
    if not cands:
        return None
    _, PD, LD, cc, tpc, dbuf, PHB, W = max(cands, key=lambda c: (round(c[0], 9), c[3], -c[5]))
    tpc = {1: (3 if tpc <= 3 else tpc if tpc <= 6 else 8), 4: 4}[nq]               # the instance that runs it
    return PD, LD, cc, tpc, dbuf, PHB, W


def _mm_build(mode, S, pad, CI, CO, K, isz, osz, widx, force=None):
    ID, IH, IW = isz
    OD, OH, OW = osz
    # 16 output channels of a stride-2 transposed conv: the w-parity pair needs the two 8-row replicas, so the layer runs as two halves
    # of 8 channels (a block of the grid owns one half: vg_mm_desc.co_tot), each through the 4-class plan of an 8-channel layer
    nco = 2 if (mode == 'tconv' and CO == 16) else 1
    CO_l = CO // nco
    g = _mm_classes(mode, S, pad, K, osz, 16 // CO_l)
    nq = len(g.classes)
    if nq not in (1, 4) or any(len(e) == 0 for e in g.classes) or max((len(e) + 3) // 4 for e in g.classes) > 32:
        return None
    ks, tau, dlt, aidx, slack, hlo, hhi = _mm_tables(g.classes, widx, CI, CO_l, nco, IH, IW)
    pin = force or _MM_TUNED.get((mode, S, CI, CO, tuple(K), tuple(isz), tuple(osz)))
    tile = _mm_tile(g, ks, aidx.size // nco, hlo, hhi, CI, isz, pin)        # a block keeps one half's image in LDS
    if tile is None:
        return None
    PD, LD, cc, tpc, dbuf, PHB, W = tile
    return MmPlan(mode=mode, CI=CI, CO=CO, co_blk=CO_l, ID=ID, IH=IH, IW=IW, OD=OD, OH=OH, OW=OW, nq=nq, ks=ks, PDT=g.PDT, PH=g.PH, PW=g.PW,
                  PD=PD, PHB=PHB, waves=W, tpc=tpc, cc=cc, dbuf=dbuf, LD=LD, sdi=g.sdi, shi=g.shi, swi=g.swi, d0=g.d0, sdo=g.sdo,
                  sho=g.sho, swo=g.swo, od0=g.od0, oh0=g.oh0, ow0=g.ow0, slack=slack, hlo=hlo, hhi=hhi, tau=tau, dlt=dlt, aidx=aidx)
