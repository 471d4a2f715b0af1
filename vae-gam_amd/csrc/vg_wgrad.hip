// vg_wgrad.hip -- convolution weight gradients (gfx950).
//
//   dw[cb][ca][k] = sum_{n,p} PB(b)[n][cb][p] * PA(a)[n][ca][p*S + k - pad]
//
// The output is tiny (<= 16*16*45 values) and the reduction runs over every position of every sample, so blocks are
// persistent: each walks a strided list of (sample, position-tile) work items keeping its share of dw in registers,
// writes ONE partial slab at the end (small grids: one per wave), and a second kernel sums the slabs in a fixed order
// (deterministic; no float atomics).
//
// One kernel, wgrad_rows_k, serves every layer.  dw[cb][col] (col = (ca, tap)) is a GEMM
//   D(16 x 16*NT) += A(16 x 4) * B(4 x 16*NT)     A[cb][k] = b[cb][p0+k],  B[k][col] = a[ca][(p0+k)*S + tap - pad]
// over groups of 4 consecutive positions of a row (a "k-step"), on the exact-fp32 matrix instruction
// v_mfma_f32_16x16x4_f32.  A wave keeps ALL of dw (NT = CA*TC accumulator tiles) and owns whole position rows of the
// block's tile, so (plane, row) are scalars and a k-step addresses both operands as row base + immediate.
// Both operands come from LDS images that keep the TENSORS' OWN row pitch and are filled by flat LDS-DMA copies
// (global_load_lds_dword, contiguous 256-byte wave-instructions, no VGPR round trip, no index arithmetic per element):
//   a slot : the rows of ONE `a` channel that the tile's windows touch ((TPH-1)*S+KH rows of each of its planes, one
//            contiguous span per plane);
//   b tile : for each of the (<= 16) `b` channels the rows [ph0, ph0+TPH) of the tile's TPD position planes.
// A tile is 20-30 KB, so several blocks share a CU: one block's DMA + barriers hide behind the others' MFMAs.
// ReLU / batch-norm affine are applied to an operand on its way from LDS into the MFMA (VALU work beside a matrix
// instruction); PAD adds the range masks of ConvTranspose3d padding (convt2 of the 41x49x35 network).
//
// Modes (template parameters of wgrad_rows_k; launch_rows chooses):
//   window channels : RES -- every channel's slot resident, rows outermost (the small layers); otherwise the channel
//                     loop is outermost and fully unrolled, the next channel's slot double-buffered behind the current
//                     one's MFMAs (nbuf == 2) or refilled between channels (nbuf == 1); CA == 1 has one slot.
//   GRP             : per batch-norm-group partials plus a constant-one position channel in MFMA row CB
//                     (vg_wgrad3d_grouped: the per-tap sums of the window tensor come with the weight gradient).
//   DSH             : plane-shift packing for 8 position channels at stride 2 (see above the kernel).
//   ONE             : a row as compile-time blocks of UG k-steps instead of the run-time step loop (see above the kernel).
#include "vg_common.h"
#include <stdlib.h>
#include "../../include/vaegam.h"

namespace {

// sum `nslab` slabs of `len` floats in a fixed order (run-to-run reproducible): a block owns 64 outputs, its 16
// thread rows take slabs r, r+16, ... (4 running sums each), LDS tree over the rows; optionally += into out
constexpr int SLAB_ROWS = 16;
__global__ void __launch_bounds__(64 * SLAB_ROWS)
slab_sum_k(const float* __restrict__ ws, int nslab, int len, int accumulate, float* __restrict__ out) {
    __shared__ float red[SLAB_ROWS][64];
    const int j = threadIdx.x % 64, r = threadIdx.x / 64;
    const int i = blockIdx.x * 64 + j;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < len) {
        int k = r;
        for (; k + 3 * SLAB_ROWS < nslab; k += 4 * SLAB_ROWS) {
            s0 += ws[(size_t)k * len + i]; s1 += ws[(size_t)(k + SLAB_ROWS) * len + i];
            s2 += ws[(size_t)(k + 2 * SLAB_ROWS) * len + i]; s3 += ws[(size_t)(k + 3 * SLAB_ROWS) * len + i];
        }
        for (; k < nslab; k += SLAB_ROWS) s0 += ws[(size_t)k * len + i];
    }
    red[r][j] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (r == 0 && i < len) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < SLAB_ROWS; ++q) t += red[q][j];
        out[i] = (accumulate ? out[i] : 0.f) + t;
    }
}

#ifdef VG_EMU
#define VG_WG_FENCE() ((void)0)
#else
#define VG_WG_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif
#ifndef VG_WG_MINB
#define VG_WG_MINB 1
#endif
#ifdef VG_STAMP
// Diagnostic build only (tools/diag): per-wave cycle sums of wgrad_rows_k's phases, read back through vg_stamp_read_wg.
__device__ unsigned long long vg_wg_stamp_out[2048 * 4 * 8];
#define VG_WS_T(t) do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define VG_WS_ADD(i) do { unsigned long long t_; VG_WS_T(t_); st_sum[i] += t_ - st_last; st_last = t_; } while (0)
#else
#define VG_WS_ADD(i) do {} while (0)
#endif
template <int V> struct vg_int { static constexpr int value = V; };
__host__ __device__ constexpr int vg_ival(int v) { return v; }
template <int V> __host__ __device__ constexpr int vg_ival(vg_int<V>) { return V; }
template <int N, int I = 0, typename F>
__host__ __device__ inline void vg_static_for(F&& f) { if constexpr (I < N) { f(vg_int<I>{}); vg_static_for<N, I + 1>(f); } }

struct WgradRowsParams {
    vg_wgrad_desc d;
    int TPD, TPH, nph, pdblocks;
    int LD, AR, apl;            // a planes / rows per plane in a slot; floats per slot plane (AR*AW)
    int a_slot, a_front;        // floats per a channel slot (with slack both ends); front slack
    int nbuf;                   // CA: all channels resident; 2: double-buffered over the channel loop; 1: single
    int b_off, bch;
    int lds_floats;
    int items;
    int wave_slabs;             // small grids: every wave writes its own slab (no cross-wave LDS reduction: 4 serial rounds, ~13 us)
    // grouped mode (vg_wgrad3d_grouped, template GRP): the grid is split evenly over the batch-norm groups (sample / per_group)
    int grp_items;              // items per group
    int ipb;                    // blocks per group
    int ones_row;               // 1: MFMA row CB carries a constant-one position channel -> per-tap sums of the window tensor
};

// DSH (stride-2 layers with 8 position channels, KD >= 2*S): the 8 idle MFMA rows carry the SAME channels one position plane further on.
// With the window operand restricted to the taps kd' in [S, KD), row (h = 0, cb) accumulates dw[cb][.][kd'] and row (h = 1, cb) -- whose
// position is one plane = S window planes ahead -- accumulates dw[cb][.][kd' - S]: together every kd in [0, KD), from (KD-S)*KH*KW instead
// of KD*KH*KW window taps (convt4: 27 instead of 45 = 2 instead of 3 matrix instructions per k-step and channel; the 4x4x4 layer of the
// 82x98x70 geometry: 32 instead of 64 = 2 instead of 4).  The position planes of a tile start at -1 (row h = 1 covers plane 0 there).
// ONE != 0: a row is ONE >> 1 unrolled blocks of UG k-steps at COMPILE-TIME offsets (rows of 13..16 positions = one block of 4: every
// large layer of the 41x49x35 network; 33 positions = three blocks of 3: its first and last layer): the LDS reads then carry their
// offsets as immediates (with the run-time step loop each read had its own address add: 39 vector + 23 scalar instructions per row
// beside 8 MFMAs, ISA of the convt4 instance); ONE & 1 (PW a multiple of 4): no position mask in the last block either.
// ONE == 0: the general step loop.  (convt4's weight gradient 627 -> 507 us, convt3's 361 -> 313.)
template <int CA, int TC, int KD, int KH, int KW, int S, bool PAD, bool PA, int UG, bool RES, bool GRP = false, bool DSH = false, int ONE = 0>
__global__ void __launch_bounds__(256, (CA * TC >= 32 ? 2 : CA * TC >= 16 ? VG_WG_MINB : 1))         // 32 accumulator tiles: keep two waves per SIMD (<= 256 registers)
wgrad_rows_k(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ in_scale,
             const float* __restrict__ in_shift, float* __restrict__ ws, WgradRowsParams p) {
    VG_DYN_SMEM(float, lds);
    constexpr int KVOL = KD * KH * KW;
    constexpr int KVW = DSH ? (KD - S) * KH * KW : KVOL;               // window taps the matrix columns enumerate
    constexpr int NT = CA * TC;
    const vg_wgrad_desc& d = p.d;
    const int CB = d.CB;
    const int tid = threadIdx.x, lane = tid % VG_WAVE;
    const int wave = vg_wave_id(), nwaves = blockDim.x / VG_WAVE;
    float* btile = lds + p.b_off;
    const int kq = lane >> 4, cbl = lane & 15;

    for (int i = tid; i < p.lds_floats; i += blockDim.x) lds[i] = 0.f;       // never-written words stay finite

    int colOff[TC], tkd[TC], tkh[TC], tkw[TC];
#pragma unroll
    for (int t = 0; t < TC; ++t) {
        const int tap = t * 16 + cbl;
        const bool ok = tap < KVW;
        tkd[t] = ok ? tap / (KH * KW) : 0; tkh[t] = ok ? (tap / KW) % KH : 0; tkw[t] = ok ? tap % KW : 0;     // DSH: tkd counts from kd' = S
        colOff[t] = tkd[t] * p.apl + tkh[t] * d.AW + tkw[t];
    }
    vg_f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { acc[t].v[0] = 0.f; acc[t].v[1] = 0.f; acc[t].v[2] = 0.f; acc[t].v[3] = 0.f; }

    const int rl_a = PA ? d.relu_in : 0, rl_b = PA ? 0 : d.relu_in;           // PA: the ReLU / BN affine belongs to the window tensor
    const float lo_a = rl_a ? 0.f : -__builtin_inff(), lo_b = rl_b ? 0.f : -__builtin_inff();
    const int ksteps = (d.PW + 3) / 4;
    const int aplane = d.AH * d.AW, bplane = d.PH * d.PW;
    const bool cb_ok = cbl < (DSH ? 2 * CB : CB);
    // DSH: lanes CB .. 2CB-1 read the same channels one position plane (TPH*PW floats of the tile) further on
    const float* bchan = btile + (DSH ? (cbl % CB) : min(cbl, CB - 1)) * p.bch + ((DSH && cbl >= CB) ? p.TPH * d.PW : 0) + kq;
    __syncthreads();

    const int CBW = CB + (GRP ? 1 : 0);                                  // rows of dw written out (grouped: + the ones row)
    const int ncol_o = CA * KVOL;
    // matrix row cbr, window tap -> (row of dw, tap of dw), or -1: plain = (cbr, tap); DSH: see above
    auto out_index = [&](int cbr, int tap, int ca) -> long long {
        if (!DSH) return (cbr < CBW && tap < KVOL) ? (long long)cbr * ncol_o + ca * KVOL + tap : -1;
        if (cbr >= 2 * CB || tap >= KVW) return -1;
        const int h = cbr / CB, cb = cbr % CB, kdw = tap / (KH * KW), rest = tap % (KH * KW);
        if (h == 1 && kdw >= S) return -1;                                // a duplicate of row h = 0's kd = kdw
        return (long long)cb * ncol_o + ca * KVOL + (h == 0 ? kdw + S : kdw) * (KH * KW) + rest;
    };
    // ---- close a slab: the block's (or, small grids, each wave's) partial dw -> workspace
    auto write_out = [&](int slab) {
        if (p.wave_slabs) {
            float* out = ws + ((size_t)slab * nwaves + wave) * CBW * ncol_o;
            const int cb0 = (lane >> 4) * 4, tapl = lane & 15;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int ca = t / TC, tap = (t % TC) * 16 + tapl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long oi = out_index(cb0 + r, tap, ca);
                    if (oi >= 0) out[oi] = acc[t].v[r];
                }
                VG_WG_FENCE();                      // one tile at a time: otherwise all NT*4 accumulators are copied to VGPRs up front
            }
            return;
        }
        // cross-wave reduction through LDS (one wave at a time), then one slab
        float* red = lds;
        __syncthreads();
        for (int w = 0; w < nwaves; ++w) {
            if (wave == w) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int idx = (t * 4 + r) * VG_WAVE + lane;
                        red[idx] = (w == 0 ? 0.f : red[idx]) + acc[t].v[r];
                        if (r == 3) VG_WG_FENCE();
                    }
            }
            __syncthreads();
        }
        float* out = ws + (size_t)slab * CBW * ncol_o;
        for (int i = tid; i < NT * 4 * VG_WAVE; i += blockDim.x) {
            const int l = i % VG_WAVE; const int r = (i / VG_WAVE) % 4; const int t = i / (4 * VG_WAVE);
            const int ca = t / TC, tap = (t % TC) * 16 + (l & 15);
            const int cb = (l >> 4) * 4 + r;
            const long long oi = out_index(cb, tap, ca);
            if (oi >= 0) out[oi] = red[i];
        }
    };
    // plain mode: items blockIdx.x, +gridDim.x, ...   grouped mode: the grid is split evenly over the batch-norm groups (ipb = blocks per
    // group); a group's blocks deal ITS items round-robin, so every slab belongs to one group and blocks running side by side still
    // work on neighbouring tiles (their halos meet in L2; contiguous item ranges per block cost 0.2 ms in re-fetched planes)
    const int it_step = GRP ? p.ipb : (int)gridDim.x;
    const int it0 = GRP ? ((int)blockIdx.x / p.ipb) * p.grp_items + (int)blockIdx.x % p.ipb : (int)blockIdx.x;
    const int it1 = GRP ? ((int)blockIdx.x / p.ipb + 1) * p.grp_items : p.items;

#ifdef VG_STAMP
    unsigned long long st_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_last;
    VG_WS_T(st_last);
#endif
    for (int item = it0; item < it1; item += it_step) {
        const int n = item / (p.pdblocks * p.nph); const int rem = item % (p.pdblocks * p.nph);
        const int pd0 = (rem / p.nph) * p.TPD - (DSH ? 1 : 0), ph0 = (rem % p.nph) * p.TPH;
        const int nrow = min(p.TPH, d.PH - ph0), ndz = min(p.TPD, d.PD - pd0);
        const int g = (in_scale != nullptr) ? n / d.per_group : 0;
        const int ap0 = pd0 * S - d.pad_d + (DSH ? S : 0), ih0 = ph0 * S - d.pad_h;
        const int pl_lo = max(ap0, 0), pl_hi = min(ap0 + p.LD, d.AD);
        const int r_lo = max(ih0, 0), r_hi = min(ih0 + p.AR, d.AH);
        const int npl = max(pl_hi - pl_lo, 0);
        const int cnt = max(r_hi - r_lo, 0) * d.AW;                         // contiguous floats per staged plane
        const int adst = p.a_front + (pl_lo - ap0) * p.apl + (r_lo - ih0) * d.AW;
        const float* abase = a + (((size_t)n * CA * d.AD + pl_lo) * d.AH + r_lo) * d.AW;
        float bsc = cb_ok ? 1.f : 0.f, bsh = 0.f;                        // lanes without a b channel contribute zeros
        if (!PA && in_scale && cb_ok) { bsc = in_scale[g * CB + (DSH ? cbl % CB : cbl)]; bsh = in_shift[g * CB + (DSH ? cbl % CB : cbl)]; }
        if (GRP && cbl == CB) bsh = 1.f;                                 // ones row (bsc stays 0: the lane reads channel CB-1's finite data)
        VG_WS_ADD(0);                                                     // item set-up
        __syncthreads();                                                  // previous item's tiles fully consumed
        VG_WS_ADD(1);                                                     // barrier (item start)
        // one (channel, plane) span per wave at a time: the span's base addresses are formed once, the 256-byte DMA
        // instructions of the span then cost a handful of scalar adds each (a flattened loop pays two scalar divisions
        // and 64-bit address arithmetic -- ~75 SALU instructions -- per DMA instruction)
        auto stage_a = [&](int c0, int nc, int slot0) {
            for (int c = 0; c < nc; ++c) {
                const float* src = abase + ((size_t)(c0 + c) * d.AD + wave) * aplane;
                float* dst = lds + (slot0 + c) * p.a_slot + adst + wave * p.apl;
                for (int pl = wave; pl < npl; pl += 4, src += 4 * (size_t)aplane, dst += 4 * p.apl) {
                    // (the 16-byte form, vg_dma_block, measured here: convt4 802 -> 793 us, convt5 508 -> 490, but convt2 224 -> 250-303 and the
                    //  small layers 5-20 % slower -- spans of a few hundred floats: its head / tail pieces cost what the wide body saves)
                    vg_dma_span(src + lane, dst, cnt, lane);
                }
            }
        };
        if (RES) stage_a(0, CA, 0);
        else stage_a(0, 1, 0);
        {
            const int nb = nrow * d.PW;
            const size_t bch_g = (size_t)d.PD * bplane;
            const float* src_c = b + ((size_t)n * CB + wave) * bch_g + (long long)pd0 * bplane + (size_t)ph0 * d.PW;     // (DSH: pd0 may be -1; such planes are not read)
            float* dst_c = btile + wave * p.bch;
            const int ndzs = DSH ? ndz + 1 : ndz;                         // DSH: + the plane behind the tile (rows h = 1 of its last plane)
            for (int c = wave; c < CB; c += 4, src_c += 4 * bch_g, dst_c += 4 * p.bch) {
                const float* src = src_c; float* dst = dst_c;
                for (int dz = 0; dz < ndzs; ++dz, src += bplane, dst += p.TPH * d.PW) {
                    if (!DSH || (pd0 + dz >= 0 && pd0 + dz < d.PD)) vg_dma_span(src + lane, dst, nb, lane);
                    else for (int o = lane; o < nb; o += VG_WAVE) dst[o] = 0.f;      // a plane outside the tensor: its positions contribute nothing
                }
            }
        }
        VG_WS_ADD(2);                                                     // copy issue (a slot 0 + b tile)
        vg_dma_wait();
        VG_WS_ADD(3);                                                     // copy wait
        __syncthreads();
        VG_WS_ADD(1);
        // DSH: a position plane outside the tensor (plane -1 of rows h = 0, plane PD of rows h = 1) contributes exactly nothing, whatever
        // the prologue's shift: its lanes' scale and shift are zeroed per plane (the tile holds zeros there)
        float bscz = bsc, bshz = bsh;
        auto plane_factors = [&](int dz) {
            if (DSH) {
                const int pl = pd0 + dz + (cbl >= CB ? 1 : 0);
                const bool v = pl >= 0 && pl < d.PD;
                bscz = v ? bsc : 0.f; bshz = v ? bsh : 0.f;
            }
        };
        // one position row against one `a` channel: UG k-steps per iteration, all operand reads first, then the matrix
        // instructions.  ONE branch-free loop whose trip count is rounded up to UG (surplus k-steps have px >= PW: their A
        // operand is zeroed, their reads stay inside the tiles' slack); only the LAST block can hold such positions and it
        // alone carries the mask.  (A remainder branch would split the accumulators' live ranges: the compiler then
        // shuffles all NT*4 of them between register sets on every row.)
        auto row_channel = [&](auto ca_tag, const float* bp, const float* ap, float sc, float sh, const bool* okdh) {
            constexpr int ca = decltype(ca_tag)::value;
            auto kblock = [&](auto masked_tag, auto ks_) {         // ks_: int, or vg_int<0> (ONE: compile-time 0)
                constexpr bool MASKED = decltype(masked_tag)::value != 0;
                const int ks = vg_ival(ks_);
                float av[UG], bv[UG][TC];
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    av[u] = bp[(ks + u) * 4];
#pragma unroll
                    for (int t = 0; t < TC; ++t) bv[u][t] = ap[colOff[t] + (ks + u) * 4 * S];
                }
#pragma unroll
                for (int u = 0; u < UG; ++u) {
                    const int px = (ks + u) * 4 + kq;
                    float a_ = fmaf(vg_max(av[u], lo_b), bscz, bshz);             // PA: lo_b = -inf, bsc = 1 (0 for idle lanes), bsh = 0
                    if (MASKED) a_ = px < d.PW ? a_ : 0.f;
#pragma unroll
                    for (int t = 0; t < TC; ++t) {
                        float b_ = bv[u][t];
                        if (PA) b_ = fmaf(vg_max(b_, lo_a), sc, sh);
                        if (PAD) {
                            const int iw = px * S - d.pad_w + tkw[t];
                            b_ = (okdh[t] && iw >= 0 && iw < d.AW) ? b_ : 0.f;
                        }
                        vg_mfma16(a_, b_, acc[ca * TC + t]);
                    }
                }
            };
            if constexpr (ONE != 0) {
                constexpr int NB = ONE >> 1;
                vg_static_for<NB>([&](auto i_tag) {
                    constexpr int I = decltype(i_tag)::value;
                    if constexpr (I + 1 < NB || (ONE & 1)) kblock(vg_int<0>{}, vg_int<I * UG>{});
                    else kblock(vg_int<1>{}, vg_int<I * UG>{});
                });
            } else {
                int ks = 0;
                for (; ks < ksteps - UG; ks += UG) kblock(vg_int<0>{}, ks);
                kblock(vg_int<1>{}, ks);
            }
        };
        auto row_masks = [&](int dz, int py, bool* okdh) {
#pragma unroll
            for (int t = 0; t < TC; ++t) {
                const int id = ap0 + dz * S + tkd[t], ih = ih0 + py * S + tkh[t];
                okdh[t] = !PAD || (id >= 0 && id < d.AD && ih >= 0 && ih < d.AH);
            }
        };
        if constexpr (RES) {
            // every channel's window rows are resident: rows outermost, so the row bookkeeping (and the masks) are paid
            // once per row, not once per (row, channel) -- the small layers (5..7 positions per row) live on this
            float scv[CA], shv[CA];
#pragma unroll
            for (int ca = 0; ca < CA; ++ca) {
                scv[ca] = 1.f; shv[ca] = 0.f;
                if (PA && in_scale) { scv[ca] = in_scale[g * CA + ca]; shv[ca] = in_shift[g * CA + ca]; }
            }
            for (int dz = 0; dz < ndz; ++dz)
            for (int py = (wave - dz * nrow) & 3; py < nrow; py += 4) {
                plane_factors(dz);
                const float* bp = bchan + (dz * p.TPH + py) * d.PW;
                const float* ap0_ = lds + p.a_front + (dz * S) * p.apl + (py * S) * d.AW + kq * S - d.pad_w;
                bool okdh[TC];
                row_masks(dz, py, okdh);
                vg_static_for<CA>([&](auto ca_tag) {
                    constexpr int ca = decltype(ca_tag)::value;
                    row_channel(ca_tag, bp, ap0_ + ca * p.a_slot, scv[ca], shv[ca], okdh);
                });
            }
        } else {
            vg_static_for<CA>([&](auto ca_tag) {
                constexpr int ca = decltype(ca_tag)::value;
                const float* cur = lds + (ca % p.nbuf) * p.a_slot;
                if (ca + 1 < CA && p.nbuf == 2) stage_a(ca + 1, 1, (ca + 1) & 1);    // in flight behind this channel's MFMAs
                VG_WS_ADD(4);                                                     // copy issue (next channel)
                float sc = 1.f, sh = 0.f;
                if (PA && in_scale) { sc = in_scale[g * CA + ca]; sh = in_shift[g * CA + ca]; }
                // rows of the tile dealt round-robin over the 4 waves ((plane, row) wave-uniform: scalars, no division)
                for (int dz = 0; dz < ndz; ++dz)
                for (int py = (wave - dz * nrow) & 3; py < nrow; py += 4) {
                    plane_factors(dz);
                    const float* bp = bchan + (dz * p.TPH + py) * d.PW;
                    const float* ap = cur + p.a_front + (dz * S) * p.apl + (py * S) * d.AW + kq * S - d.pad_w;
                    bool okdh[TC];
                    row_masks(dz, py, okdh);
                    row_channel(ca_tag, bp, ap, sc, sh, okdh);
                }
                VG_WS_ADD(5);                                                     // matrix work of a channel
                if (CA > 1) {
                    if (p.nbuf == 2) { vg_dma_wait(); VG_WS_ADD(6); __syncthreads(); VG_WS_ADD(7); }
                    else if (ca + 1 < CA) { __syncthreads(); stage_a(ca + 1, 1, 0); vg_dma_wait(); __syncthreads(); }
                }
            });
        }
    }
#ifdef VG_STAMP
    if (lane == 0 && blockIdx.x < 2048)
        for (int i = 0; i < 8; ++i) vg_wg_stamp_out[(blockIdx.x * 4 + wave) * 8 + i] = st_sum[i];
#endif
    write_out((int)blockIdx.x);
}

#ifdef VG_STAMP
extern "C" int vg_stamp_read_wg(unsigned long long* dst, int n) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(vg_wg_stamp_out), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
#endif

// Slabs of a grouped launch -> out[g][len]: group g owns the slabs [g*spg, (g+1)*spg)
__global__ void __launch_bounds__(64 * SLAB_ROWS)
slab_sum_groups_k(const float* __restrict__ ws, int spg, int len, float* __restrict__ out) {
    __shared__ float red[SLAB_ROWS][64];
    const int j = threadIdx.x % 64, r = threadIdx.x / 64;
    const int i = blockIdx.x * 64 + j, g = blockIdx.y;
    float s0 = 0.f;
    if (i < len)
        for (int k = g * spg + r; k < (g + 1) * spg; k += SLAB_ROWS) s0 += ws[(size_t)k * len + i];
    red[r][j] = s0;
    __syncthreads();
    if (r == 0 && i < len) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < SLAB_ROWS; ++q) t += red[q][j];
        out[(size_t)g * len + i] = t;
    }
}

// The instances of wgrad_rows_k that exist for one <CA, ..., PAD, DSH> family, as (PA, UG, RES, GRP, ONE): exactly what launch_rows
// can choose below.  ONE takes the values of ROWS_ONE.
constexpr int ROWS_ONE[4] = {0, 2, 3, 6};
template <int CA, bool PAD, bool DSH>
constexpr bool rows_instance(bool pa, int ug, bool res, bool grp, int one) {
    if (res && CA == 1) return false;                                   // a single channel is its own (only) slot
    if (grp) return CA == 1 && !PAD && !DSH && !pa && (one == 0 || (one == 6 && ug == 3));
    if (one == 0) return true;
    if (one == 6) return CA == 1 && !DSH && ug == 3;
    return (ug == 4 && !res) || (CA > 1 && !DSH && ug == 2 && res);      // one == 2, 3
}

// What a query call (no launch) wants back from launch_rows: the workspace size, the plan record of vg_wgrad3d_plan, or both
struct RowsQuery { int64_t* ws_bytes; int32_t* plan; };

// returns -1 when it has no plan or no instance for the descriptor (the caller reports VG_ERR_UNSUPPORTED)
template <int CA, int TC, int KD, int KH, int KW, int S, bool PAD, bool DSH = false>
int launch_rows(const vg_wgrad_desc* d, const float* a, const float* b, const float* in_scale, const float* in_shift,
                float* ws, float* dw, hipStream_t s, const RowsQuery* query, int accumulate, int grouped) {
    constexpr int KVOL = KD * KH * KW;
    constexpr int NT = CA * TC;
    constexpr int KDW = DSH ? KD - S : KD;                              // window planes a position touches (DSH: taps kd' in [S, KD) only)
    const bool padded = d->pad_d || d->pad_h || d->pad_w;
    if (padded != PAD || d->CA != CA || d->CB > 16) return -1;
    if (DSH && (2 * d->CB > 16 || grouped || KD < 2 * S)) return -1;       // (never on in_scale: the workspace query passes none)
    if (grouped && d->CB >= 16) return -1;                              // the ones row needs a free MFMA row
    const int PDE = DSH ? d->PD + 1 : d->PD;                            // position planes the tiles cover (DSH: from -1)
    const bool narrow = d->PW < 12;                 // 5..7-position rows: only worth it with every channel resident (rows outermost)
    if (!PAD && ((d->PD - 1) * S + KD > d->AD || (d->PH - 1) * S + KH > d->AH || (d->PW - 1) * S + KW > d->AW)) return -1;
    // LDS per block: measured sweep (tools/layer_bench.py over a build-time cap): 56 KB is best or equal for every layer of the net
    // (convt4 212 -> 187 us, convt2 104 -> 92, convt5 130 -> 119 vs 24-48 KB); 64 KB leaves one block per CU too few
    // (measured and NOT adopted: compiling the 16-24-tile instances for three waves per SIMD (-DVG_WG_MINB=3, 166 registers, no spills) with
    //  48 KB tiles is 6 % faster per layer in tools/layer_bench.py -- convt4 799 -> 753 us, convt3 345 -> 326 -- but not in the step, where these
    //  launches share the GPU with the gain block's backward on the second stream: 8.17-8.22 vs 8.21-8.24 ms)
    const size_t cap = (size_t)56 * 1024;
    const size_t red_fl = (size_t)NT * 4 * VG_WAVE;
    const int front = 4;                            // >= pad_w: the first window of a padded row starts before the slot's row
    WgradRowsParams best; double best_score = -1;
    for (int td = 1; td <= 4 && td <= d->PD; ++td)
        for (int th = 1; th <= d->PH; ++th) {
            WgradRowsParams p; p.d = *d;
            p.TPD = td; p.TPH = th; p.LD = (td - 1) * S + KDW; p.AR = (th - 1) * S + KH; p.apl = p.AR * d->AW;
            p.a_front = front;
            p.a_slot = (int)((((size_t)p.LD * p.apl + front + 4 + 16 * S + 3) / 4) * 4);     // back slack: rounded-up k-steps of the last row
            size_t f = (size_t)(td + (DSH ? 1 : 0)) * th * d->PW + 24; while (f % 32 != 2) ++f;       // +24: rounded-up k-steps read past the last row
            p.bch = (int)f;
            p.nbuf = 0;
            const int opts[3] = {CA, 2, 1};
            for (int k = 0; k < 3 && !p.nbuf; ++k) {
                const int nb = opts[k];
                if (nb > CA || (nb == 2 && CA <= 2 && k == 1)) continue;
                if (((size_t)nb * p.a_slot + (size_t)d->CB * p.bch + 64) * 4 <= cap) p.nbuf = nb;
            }
            if (!p.nbuf || (narrow && p.nbuf != CA)) continue;
            const int rows = td * th, pos = rows * d->PW;
            const double util = ((double)d->PH / (vg_cdiv(d->PH, th) * th)) * ((double)PDE / (vg_cdiv(PDE, td) * td)) *
                                ((double)rows / (4 * vg_cdiv(rows, 4)));
            const double halo = (double)(td * S) * (th * S) / ((double)p.LD * p.AR);
            double score = util * pos / (pos + 96.0) * (0.6 + 0.4 * halo);
            if (p.nbuf == 1 && CA > 1) score *= 0.6;
            // few-item layers (encoder end, 32 samples): one wave per SIMD runs its whole dependent chain exposed -- prefer
            // tiles small enough that every CU gets a couple of blocks
            const long items = (long)d->N * vg_cdiv(PDE, td) * vg_cdiv(d->PH, th);
            if (items < 512) score *= ((double)items / 512.0) * ((double)items / 512.0);
            if (score > best_score) { best_score = score; best = p; }
        }
    if (best_score < 0) return -1;
    WgradRowsParams p = best;
    p.nph = vg_cdiv(d->PH, p.TPH); p.pdblocks = vg_cdiv(PDE, p.TPD);
    p.b_off = p.nbuf * p.a_slot;
    size_t fl = (size_t)p.b_off + (size_t)d->CB * p.bch + 64;
    if (fl < red_fl) fl = red_fl;
    p.lds_floats = (int)fl;
    p.items = d->N * p.pdblocks * p.nph;
    // ---- the run-time choices that name the instance
    // k-steps (4 positions) per row, rounded up to the unroll that wastes the fewest
    const int ksteps = vg_cdiv(d->PW, 4);
    int ug = 4, waste = vg_cdiv(ksteps, 4) * 4 - ksteps;
    for (int u = 3; u >= 2; --u) { const int w_ = vg_cdiv(ksteps, u) * u - ksteps; if (w_ < waste) { waste = w_; ug = u; } }
    const bool pa = d->pro_on_a != 0;
    const bool res = CA > 1 && p.nbuf == CA;
    const bool grp = grouped != 0;
    int one = 0;                                            // compile-time row blocks (see ONE above the kernel)
    if (!grp && !res && ug == 4 && ksteps == 4) one = d->PW % 4 == 0 ? 3 : 2;                // one block of 4: convt4 / convt3 / conv2 / conv3 at 41x49x35
    else if (CA > 1 && !DSH && res && ug == 2 && ksteps <= 2) one = d->PW == 8 ? 3 : 2;      // one block of 2 (4..8 positions): convt1 / convt2 / conv4 / conv5
    else if (CA == 1 && !DSH && ug == 3 && ksteps == 9 && d->PW % 4 != 0) one = 6;           // three blocks of 3: the 33-position rows of conv1 / convt5
    // ---- ... mapped to the kernel: the one (PA, UG, RES, GRP, ONE) of the family's instances that equals them
    using kern_t = void (*)(const float*, const float*, const float*, const float*, float*, WgradRowsParams);
    kern_t kern = nullptr;
    vg_static_for<2 * 2 * 2 * 3 * 4>([&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value;
        constexpr bool PA = (I & 1) != 0, RES = (I & 2) != 0, GRP = (I & 4) != 0;
        constexpr int UG = 2 + (I >> 3) % 3, ONE = ROWS_ONE[(I >> 3) / 3];
        if constexpr (rows_instance<CA, PAD, DSH>(PA, UG, RES, GRP, ONE))
            if (pa == PA && ug == UG && res == RES && grp == GRP && one == ONE)
                kern = wgrad_rows_k<CA, TC, KD, KH, KW, S, PAD, PA, UG, RES, GRP, DSH, ONE>;
    });
    if (!kern) return -1;                                   // grouped: CA == 1, no padding, prologue on b only
    int per_cu = vg_blocks_per_cu((const void*)kern, 256, fl * sizeof(float));   // persistent grid == resident blocks
    if (per_cu > 8) per_cu = 8;
    int grid = 256 * per_cu; if (grid > p.items) grid = p.items;
    p.grp_items = 0; p.ipb = 0; p.ones_row = 0;
    if (grouped) {
        // per-group partials (+ the ones row): the same number of blocks for every group
        const int G = d->N / d->per_group;
        p.grp_items = d->per_group * p.pdblocks * p.nph; p.ones_row = 1;
        p.ipb = grid / G; if (p.ipb < 1) p.ipb = 1;
        if (p.ipb > p.grp_items) p.ipb = p.grp_items;
        grid = p.ipb * G;
    }
    const int len = (d->CB + p.ones_row) * CA * KVOL;
    p.wave_slabs = grid <= 512 ? 1 : 0;
    const int per_slab = p.wave_slabs ? 4 : 1;
    const int nslabs = grid * per_slab;
    if (query) {                                            // nothing is launched: the sizes and choices the launch below would use
        if (query->ws_bytes) *query->ws_bytes = (int64_t)nslabs * len * sizeof(float);
        if (query->plan) {
            const int32_t rec[VG_WGRAD_PLAN_LEN] = {
                CA, KD, KH, KW, S, PAD ? 1 : 0, DSH ? 1 : 0, pa ? 1 : 0, ug, res ? 1 : 0, grp ? 1 : 0, one, p.TPD, p.TPH, p.nbuf,
                p.pdblocks, p.nph, p.items, grid, p.wave_slabs, p.ipb, p.grp_items, nslabs, (int32_t)(fl * sizeof(float)), per_cu};
            for (int i = 0; i < VG_WGRAD_PLAN_LEN; ++i) query->plan[i] = rec[i];
        }
        return VG_OK;
    }
    vg_launch(kern, dim3(grid), dim3(256), fl * sizeof(float), s, a, b, in_scale, in_shift, ws, p);
    int rc = vg_check_launch("wgrad_rows");
    if (rc) return rc;
    if (grouped) {
        const int G = d->N / d->per_group;
        vg_launch(slab_sum_groups_k, dim3(vg_cdiv(len, 64), G), dim3(64 * SLAB_ROWS), 0, s, (const float*)ws, p.ipb * per_slab, len, dw);
        return vg_check_launch("wgrad slab_sum_groups");
    }
    vg_launch(slab_sum_k, dim3(vg_cdiv(len, 64)), dim3(64 * SLAB_ROWS), 0, s, (const float*)ws, nslabs, len, accumulate, dw);
    return vg_check_launch("wgrad slab_sum");
}

int dispatch(const vg_wgrad_desc* d, const float* a, const float* b, const float* in_scale, const float* in_shift,
             float* ws, float* dw, hipStream_t s, const RowsQuery* ws_only, int accumulate) {
    if (!d) { vg_set_error("vg_wgrad3d: null descriptor"); return VG_ERR_ARG; }
    if (d->N <= 0 || d->CA <= 0 || d->CB <= 0 || d->PD <= 0 || d->PH <= 0 || d->PW <= 0 || d->AD <= 0 || d->AH <= 0 ||
        d->AW <= 0 || (d->stride != 1 && d->stride != 2)) {
        vg_set_error("vg_wgrad3d: bad shape"); return VG_ERR_ARG;
    }
    if ((in_scale == nullptr) != (in_shift == nullptr) || (in_scale && d->per_group <= 0)) {
        vg_set_error("vg_wgrad3d: in_scale/in_shift/per_group inconsistent"); return VG_ERR_ARG;
    }
    // the instance table: kernel, window channels, stride, padding -> launch_rows<CA, TC, KD, KH, KW, S, PAD[, DSH]>
    // (TC = 16-tap tiles per window channel; DSH: 8 position channels at stride 2 fill the 8 idle matrix rows, 2 tap tiles instead of 3 / 4)
    auto rows = [&](auto launch) { return launch(d, a, b, in_scale, in_shift, ws, dw, s, ws_only, accumulate, 0); };
    auto k = [&](int kd, int kh, int kw) { return d->KD == kd && d->KH == kh && d->KW == kw; };
    const int CA = d->CA, S = d->stride;
    const bool padded = d->pad_d || d->pad_h || d->pad_w;
    int r = -1;                                             // stays -1: no line takes the descriptor, or launch_rows has no plan for it
    if (d->CB <= 16 && d->PW <= 128) {
        if (k(3, 3, 3) && CA == 1 && S == 1 && !padded) r = rows(launch_rows<1, 2, 3, 3, 3, 1, false>);
        else if (k(3, 3, 3) && CA == 8 && S == 1 && !padded) r = rows(launch_rows<8, 2, 3, 3, 3, 1, false>);
        else if (k(3, 3, 3) && CA == 8 && S == 2 && !padded) r = rows(launch_rows<8, 2, 3, 3, 3, 2, false>);
        else if (k(3, 3, 3) && CA == 16 && S == 1 && !padded) r = rows(launch_rows<16, 2, 3, 3, 3, 1, false>);
        else if (k(3, 3, 3) && CA == 16 && S == 2 && !padded) r = rows(launch_rows<16, 2, 3, 3, 3, 2, false>);
        else if (k(3, 3, 3) && CA == 16 && S == 2 && padded) r = rows(launch_rows<16, 2, 3, 3, 3, 2, true>);
        else if (k(5, 3, 3) && CA == 8 && S == 2 && !padded && d->CB == 8) r = rows(launch_rows<8, 2, 5, 3, 3, 2, false, true>);
        else if (k(4, 4, 4) && CA == 8 && S == 2 && !padded && d->CB == 8) r = rows(launch_rows<8, 2, 4, 4, 4, 2, false, true>);
    }
    if (r >= 0) return r;
    vg_set_error("vg_wgrad3d: no kernel instance for CB=%d CA=%d k=%dx%dx%d stride=%d pad=%d,%d,%d PW=%d (or the window leaves `a`)",
                 d->CB, CA, d->KD, d->KH, d->KW, S, d->pad_d, d->pad_h, d->pad_w, d->PW);
    return VG_ERR_UNSUPPORTED;
}

}  // namespace

static int grouped_dispatch(const vg_wgrad_desc* d, const float* a, const float* b, const float* in_scale, const float* in_shift,
                            float* ws, float* out, hipStream_t s, const RowsQuery* ws_only) {
    if (!d) { vg_set_error("vg_wgrad3d_grouped: null descriptor"); return VG_ERR_ARG; }
    if (d->N <= 0 || d->per_group <= 0 || d->N % d->per_group || d->CB <= 0 || d->CB >= 16 || d->PD <= 0 || d->PH <= 0 || d->PW <= 0) {
        vg_set_error("vg_wgrad3d_grouped: bad shape"); return VG_ERR_ARG;
    }
    const bool k333 = d->KD == 3 && d->KH == 3 && d->KW == 3;
    if (k333 && d->CA == 1 && d->stride == 1 && !d->pad_d && !d->pad_h && !d->pad_w && d->PW <= 128) {
        int r_ = launch_rows<1, 2, 3, 3, 3, 1, false>(d, a, b, in_scale, in_shift, ws, out, s, ws_only, 0, 1);
        if (r_ >= 0) return r_;
    }
    vg_set_error("vg_wgrad3d_grouped: no kernel instance for CB=%d CA=%d k=%dx%dx%d stride=%d", d->CB, d->CA, d->KD, d->KH, d->KW, d->stride);
    return VG_ERR_UNSUPPORTED;
}

extern "C" int64_t vg_wgrad3d_grouped_ws_bytes(const vg_wgrad_desc* d) {
    int64_t bytes = 0;
    const RowsQuery q = {&bytes, nullptr};
    int rc = grouped_dispatch(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &q);
    return rc ? -1 : bytes;
}

extern "C" int vg_wgrad3d_grouped(const vg_wgrad_desc* d, const float* a, const float* b, const float* in_scale,
                                  const float* in_shift, float* ws, float* out, void* stream) {
    if (!a || !b || !ws || !out || !in_scale || !in_shift) { vg_set_error("vg_wgrad3d_grouped: null argument"); return VG_ERR_ARG; }
    return grouped_dispatch(d, a, b, in_scale, in_shift, ws, out, (hipStream_t)stream, nullptr);
}

extern "C" int64_t vg_wgrad3d_ws_bytes(const vg_wgrad_desc* d) {
    int64_t bytes = 0;
    const RowsQuery q = {&bytes, nullptr};
    int rc = dispatch(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &q, 0);
    return rc ? -1 : bytes;
}

extern "C" int vg_wgrad3d(const vg_wgrad_desc* d, const float* a, const float* b, const float* in_scale,
                          const float* in_shift, float* ws, float* dw, int32_t accumulate, void* stream) {
    if (!a || !b || !ws || !dw) { vg_set_error("vg_wgrad3d: null argument"); return VG_ERR_ARG; }
    return dispatch(d, a, b, in_scale, in_shift, ws, dw, (hipStream_t)stream, nullptr, accumulate);
}

extern "C" int vg_wgrad3d_plan(const vg_wgrad_desc* d, int32_t grouped, int32_t* out, int32_t n_out) {
    if (!out || n_out < VG_WGRAD_PLAN_LEN) { vg_set_error("vg_wgrad3d_plan: out must hold VG_WGRAD_PLAN_LEN values"); return VG_ERR_ARG; }
    const RowsQuery q = {nullptr, out};
    if (grouped) return grouped_dispatch(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &q);
    return dispatch(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &q, 0);
}
