// vg_gam.hip -- fused GAM accumulate + Gaussian log-likelihood + GLM distance, and fused Adam (gfx950).
//
// Replaces, per minibatch (vae_reg_GP.py):
//   cons_i = task_var_i[:,None] * sigmoid(logits_i)   (:380, with the decoder's sigmoid :264 folded in)
//   x_rec  = sigmoid(logits_0) + sum_i cons_i         (:330, :390)
//   dist   = || cons_i[b] - glm_i ||_2                (:388; sum(cdist(..)) == B * sum_b dist)
//   slp[b] = sum_v log N(x[b,v] | x_rec[b,v], exp(-eps[v]))   (:401-405)
// in ONE pass over the (C+1) x B x V logits instead of 3-4 elementwise passes per covariate plus
// the (C+2) x B x V device-to-host copies, and the matching backward in one more pass.
// HBM-streaming kernels: coalesced loads, per-wave shuffle reductions, fixed-order second stage.
// Three entry-point pairs share the two kernels through compile-time flags: the plain pair (everything on one grid), the _embed pair
// (logits on a larger grid than the data; the padding takes no part) and the _masked pair (a voxel mask on the data's grid, with or
// without embedding; a voxel outside the mask takes no part, exactly like the padding).
#include <type_traits>
#include "vg_common.h"
#include "../../include/vaegam.h"

namespace {

constexpr int GT = 256;          // threads per block
constexpr int GV = 4;            // voxels per thread (strided by GT -> coalesced dword loads)
constexpr int GMAXC = 16;        // covariates supported by the LDS reduction scratch
constexpr float LOG_SQRT_2PI = 0.91893853320467274178f;

__device__ __forceinline__ float wsum(float v) { return vg_wave_sum(v); }     // (every lane gets the sum; callers use lane 0's)
__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

// An embedded grid (include/vaegam.h): the logits live on the grid G, the data on the native grid N at G's low corner.  A grid voxel
// index is split by two divisions by constants (gw, then gh) as multiply + shift with magic numbers prepared on the host:
// m = floor(2^s / d) + 1 with s = 31 + ceil(log2 d) is exact for every index below 2^31 and fits 32 bits.
struct GamGrid {
    int nd, nh, nw, gd, gh, gw;
    unsigned mw, mh;
    int sw, sh;
    long long Vn;
};

// grid voxel vg (< 2^31) -> is it a native voxel, and its index vn in the native tensor (meaningful only then)
__device__ __forceinline__ bool grid_to_native(const GamGrid& e, long long vg, long long& vn) {
    const unsigned v = (unsigned)vg;
    const unsigned row = (unsigned)(((unsigned long long)v * e.mw) >> e.sw);
    const unsigned w = v - row * (unsigned)e.gw;
    const unsigned d = (unsigned)(((unsigned long long)row * e.mh) >> e.sh);
    const unsigned h = row - d * (unsigned)e.gh;
    vn = ((long long)d * e.nh + h) * e.nw + w;
    return w < (unsigned)e.nw && h < (unsigned)e.nh && d < (unsigned)e.nd;
}

// out[b][vg] = x[b][vn] on native voxels, 0 in the padding.  grid (vchunks, B); consecutive lanes write consecutive floats and read
// runs of nw consecutive floats
__global__ void __launch_bounds__(GT)
embed_k(const float* __restrict__ x, float* __restrict__ out, long long V, GamGrid e) {
    const int b = blockIdx.y;
    const long long v0 = (long long)blockIdx.x * GT * GV + threadIdx.x;
#pragma unroll
    for (int k = 0; k < GV; ++k) {
        const long long v = v0 + (long long)k * GT;
        if (v < V) {
            long long n;
            const bool nat = grid_to_native(e, v, n);
            out[(size_t)b * V + v] = nat ? x[(size_t)b * e.Vn + n] : 0.f;
        }
    }
}

// grid (vchunks, B).  part_slp[b][chunk], part_d2[i][b][chunk]
// EMB: V counts the voxels of the grid the logits are on, x / eps / glm / maps_out are on the native grid e.Vn; a voxel of the padding
// is skipped like one behind the end.  Without EMB e is not read and the native index is the voxel index.
// MSK: mask[Vn] bytes on the native grid; a native voxel whose byte is 0 takes no part either -- it is skipped like one of the padding,
// except that it has a place in maps_out, which is written as 0 there.  Without MSK mask is not read.
template <bool EMB, bool MSK>
__global__ void __launch_bounds__(GT)
gam_fwd_k(const float* __restrict__ logits, const float* __restrict__ gain, const float* __restrict__ x,
          const double* __restrict__ eps, const float* __restrict__ glm, int C, int B, long long V,
          float* __restrict__ part_slp, float* __restrict__ part_d2, float* __restrict__ maps_out, GamGrid e,
          const uint8_t* __restrict__ mask) {
    __shared__ float red[GT / VG_WAVE][GMAXC + 1];
    const int chunk = blockIdx.x, b = blockIdx.y, chunks = gridDim.x;
    const int lane = threadIdx.x % VG_WAVE, wave = threadIdx.x / VG_WAVE;
    const long long v0 = (long long)chunk * GT * GV + threadIdx.x;
    float xrec[GV];
    bool ok[GV], out[GV];                                              // out: a native voxel outside the mask
    long long vn[GV];
#pragma unroll
    for (int k = 0; k < GV; ++k) {
        vn[k] = v0 + (long long)k * GT;
        ok[k] = vn[k] < V;
        if (EMB) { const bool nat = grid_to_native(e, v0 + (long long)k * GT, vn[k]); ok[k] = ok[k] && nat; }
        out[k] = false;
        if (MSK) { const bool in = ok[k] && mask[vn[k]] != 0; out[k] = ok[k] && !in; ok[k] = in; }
        xrec[k] = 0.f;
    }
    const long long Vn = EMB ? e.Vn : V;
    const size_t BV = (size_t)B * V, BVn = (size_t)B * Vn;
    if (MSK && maps_out) {
#pragma unroll
        for (int k = 0; k < GV; ++k)
            if (out[k])
                for (int g = 0; g <= C + 1; ++g) maps_out[(size_t)g * BVn + (size_t)b * Vn + vn[k]] = 0.f;
    }
    // base map
#pragma unroll
    for (int k = 0; k < GV; ++k)
        if (ok[k]) {
            const long long v = v0 + (long long)k * GT;
            const float s = sigmoidf_(logits[(size_t)b * V + v]);
            xrec[k] = s;
            if (maps_out) maps_out[(size_t)b * Vn + vn[k]] = s;
        }
    for (int i = 1; i <= C; ++i) {
        const float gn = gain[(size_t)(i - 1) * B + b];
        float d2 = 0.f;
#pragma unroll
        for (int k = 0; k < GV; ++k)
            if (ok[k]) {
                const long long v = v0 + (long long)k * GT;
                const float cons = gn * sigmoidf_(logits[(size_t)i * BV + (size_t)b * V + v]);
                const float df = cons - glm[(size_t)(i - 1) * Vn + vn[k]];
                d2 = fmaf(df, df, d2);
                xrec[k] += cons;
                if (maps_out) maps_out[(size_t)i * BVn + (size_t)b * Vn + vn[k]] = cons;
            }
        d2 = wsum(d2);
        if (lane == 0) red[wave][i] = d2;
    }
    float lp = 0.f;
#pragma unroll
    for (int k = 0; k < GV; ++k)
        if (ok[k]) {
            const long long v = vn[k];
            const float sg = (float)exp(-eps[v]);               // fp64 exp then cast, as :402
            const float r = x[(size_t)b * Vn + v] - xrec[k];
            lp += -(r * r) / (2.f * sg * sg) - logf(sg) - LOG_SQRT_2PI;   // Normal.log_prob
            if (maps_out) maps_out[(size_t)(C + 1) * BVn + (size_t)b * Vn + v] = xrec[k];
        }
    lp = wsum(lp);
    if (lane == 0) red[wave][0] = lp;
    __syncthreads();
    if (threadIdx.x <= C) {
        float t = 0.f;
        for (int w = 0; w < GT / VG_WAVE; ++w) t += red[w][threadIdx.x];
        if (threadIdx.x == 0) part_slp[(size_t)b * chunks + chunk] = t;
        else part_d2[((size_t)(threadIdx.x - 1) * B + b) * chunks + chunk] = t;
    }
}

// one thread per output: slp[b] = sum chunks; dist[i][b] = sqrt(sum chunks)
__global__ void __launch_bounds__(64)
gam_fwd_fold_k(const float* __restrict__ part_slp, const float* __restrict__ part_d2, int C, int B,
               int chunks, float* __restrict__ slp, float* __restrict__ dist) {
    const int i = blockIdx.x, lane = threadIdx.x;                          // one wavefront per output
    if (i >= (C + 1) * B) return;
    const float* src = (i < B) ? part_slp + (size_t)i * chunks : part_d2 + (size_t)(i - B) * chunks;
    double a = 0;
    for (int k = lane; k < chunks; k += VG_WAVE) a += src[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if (lane == 0) { if (i < B) slp[i] = (float)a; else dist[i - B] = (float)sqrt(a); }
}

// backward.  grid (vblocks, BS): block handles voxels [vb*GT, +GT) and samples b = bs, bs+BS, ...
//   part_dsig[bs][v], part_dgain[i][b][vb*4 + wave]
// Every logit is read ONCE and its sigmoid kept in a register for the second pass (CMAX = compile-time bound of the covariate
// loop, fully unrolled); the per-(covariate, sample) sums of d gain leave the block as one partial per WAVE, so the sample loop has
// no barrier at all (the first version re-read and re-evaluated all C+1 sigmoids and paid two __syncthreads per covariate and
// sample: 228 us at batch 64 / 8 covariates against 60 us of HBM time).
// EMB: as in gam_fwd_k; a thread on a voxel of the padding loads from clamped addresses like one behind the end, writes d_logits = 0
// and adds nothing to any sum.  part_dsig is [bs][Vn].
// MSK: as in gam_fwd_k; a thread on a native voxel outside the mask behaves like one of the padding and stores a 0 partial in part_dsig,
// which gam_bwd_fold_eps_k reads for every native voxel (d_eps = 0 there, not what the workspace held).
template <int CMAX, bool EMB, bool MSK>
__global__ void __launch_bounds__(GT)
gam_bwd_k(const float* __restrict__ logits, const float* __restrict__ gain, const float* __restrict__ x,
          const double* __restrict__ eps, const float* __restrict__ glm, const float* __restrict__ dist,
          const float* __restrict__ g_slp, const float* __restrict__ g_dist, int C, int B, long long V,
          float* __restrict__ d_logits, float* __restrict__ part_dsig, float* __restrict__ part_dgain, float* __restrict__ part_tot,
          GamGrid e, const uint8_t* __restrict__ mask) {
    const int vb = blockIdx.x, bs = blockIdx.y, BS = gridDim.y, nparts = gridDim.x * (GT / VG_WAVE);
    const int lane = threadIdx.x % VG_WAVE, wave = threadIdx.x / VG_WAVE;
    const long long v = (long long)vb * GT + threadIdx.x;
    const bool ok = v < V;
    const long long vc = ok ? v : V - 1;                               // clamped: loads stay unconditional, results are masked
    long long nc = vc;                                                 // the voxel's index in the native tensors, clamped likewise
    bool nat = ok;                                                     // a voxel that counts
    if (EMB) { nat = grid_to_native(e, vc, nc) && ok; if (!nat) nc = 0; }
    const bool native = nat;                                           // a voxel that has a place in the native tensors
    if (MSK) nat = nat && mask[nc] != 0;
    const long long Vn = EMB ? e.Vn : V;
    const size_t BV = (size_t)B * V;
    const float sg = (float)exp(-eps[nc]), inv_var = 1.f / (sg * sg);
    float glm_v[CMAX];
#pragma unroll
    for (int i = 0; i < CMAX; ++i) glm_v[i] = i < C ? glm[(size_t)i * Vn + nc] : 0.f;
    float dsig = 0.f, tot = 0.f;                                       // tot: sum of every d_logits element this thread writes
    for (int b = bs; b < B; b += BS) {
        const size_t row = (size_t)b * V + vc;
        float sgm[CMAX + 1], gn[CMAX];
        sgm[0] = logits[row];
#pragma unroll
        for (int i = 0; i < CMAX; ++i) {
            sgm[i + 1] = i < C ? logits[(size_t)(i + 1) * BV + row] : 0.f;
            gn[i] = i < C ? gain[(size_t)i * B + b] : 0.f;
        }
        const float xv = x[(size_t)b * Vn + nc], gs = g_slp[b];
#pragma unroll
        for (int i = 0; i <= CMAX; ++i) sgm[i] = sigmoidf_(sgm[i]);
        float xr = sgm[0];
#pragma unroll
        for (int i = 0; i < CMAX; ++i) xr += gn[i] * sgm[i + 1];         // (gn = 0 beyond C)
        const float r = xv - xr;
        const float dxr = gs * r * inv_var;                            // d slp / d x_rec = r / sigma^2
        if (nat) {
            dsig += gs * (r * r * inv_var / sg - 1.f / sg);            // d slp / d sigma
            const float dl = dxr * sgm[0] * (1.f - sgm[0]);
            d_logits[row] = dl; tot += dl;
        } else if ((EMB || MSK) && ok) d_logits[row] = 0.f;
#pragma unroll
        for (int i = 0; i < CMAX; ++i) {
            if (i < C) {                                               // wave-uniform
                const float s_ = sgm[i + 1];
                const float dd = dist[(size_t)i * B + b];
                float dcons = dxr;
                if (dd > 0.f) dcons += g_dist[(size_t)i * B + b] * (gn[i] * s_ - glm_v[i]) / dd;
                const float dl = dcons * gn[i] * s_ * (1.f - s_);
                if (nat) { d_logits[(size_t)(i + 1) * BV + row] = dl; tot += dl; }
                else if ((EMB || MSK) && ok) d_logits[(size_t)(i + 1) * BV + row] = 0.f;
                const float dg = wsum(nat ? dcons * s_ : 0.f);
                if (lane == 0) part_dgain[((size_t)i * B + b) * nparts + vb * (GT / VG_WAVE) + wave] = dg;
            }
        }
    }
    if (nat) part_dsig[(size_t)bs * Vn + nc] = dsig;
    else if (MSK && native) part_dsig[(size_t)bs * Vn + nc] = 0.f;
    if (part_tot) {
        tot = wsum(tot);
        if (lane == 0) part_tot[((size_t)bs * gridDim.x + vb) * (GT / VG_WAVE) + wave] = tot;
    }
}

// d_total (+)= sum of the per-wave totals (one block)
__global__ void __launch_bounds__(256)
gam_bwd_fold_total_k(const float* __restrict__ part_tot, int n, int accumulate, float* __restrict__ d_total) {
    __shared__ double red[256 / VG_WAVE];
    double a = 0;
    for (int k = threadIdx.x; k < n; k += 256) a += part_tot[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if (threadIdx.x % VG_WAVE == 0) red[threadIdx.x / VG_WAVE] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0;
        for (int w = 0; w < 256 / VG_WAVE; ++w) t += red[w];
        d_total[0] = (accumulate ? d_total[0] : 0.f) + (float)t;
    }
}

// one wavefront per (covariate, sample) entry: lanes stride over the per-block partials, then a shuffle reduction
// (one THREAD per entry walked ~V/256 dependent loads: 65 us for 96 numbers)
__global__ void __launch_bounds__(64)
gam_bwd_fold_gain_k(const float* __restrict__ part_dgain, int CB, int vblocks, float* __restrict__ d_gain) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= CB) return;
    double a = 0;
    for (int k = lane; k < vblocks; k += VG_WAVE) a += part_dgain[(size_t)i * vblocks + k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if (lane == 0) d_gain[i] = (float)a;
}

// d_eps[v] = dL/dsigma (fp32 sum over samples, cast to fp64) * dsigma/deps = -exp(-eps) (fp64)
__global__ void gam_bwd_fold_eps_k(const float* __restrict__ part_dsig, const double* __restrict__ eps, int BS, long long V,
                                   double* __restrict__ d_eps) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    float a = 0.f;
    for (int k = 0; k < BS; ++k) a += part_dsig[(size_t)k * V + v];
    d_eps[v] = (double)a * (-exp(-eps[v]));
}

// ---------------------------------------------------------------------------------- voxel-wise statistics of the maps and of the fit
// The volumes of subject s inside a batch, in ascending order.  subj[] is scanned 64 volumes at a time: every lane of a wave tests one
// entry and the ballot is a wave-uniform bit set, so walking the members costs scalar instructions only (one vector load per 64 volumes,
// not one dependent scalar load per volume).  An entry outside [0, S) matches no block's s and is never a member.
#ifdef VG_EMU
static inline unsigned long long stats_members(const int32_t* subj, int b0, int B, int s) {
    unsigned long long m = 0;
    for (int k = 0; k < VG_WAVE && b0 + k < B; ++k) if (subj[b0 + k] == s) m |= 1ull << k;
    return m;
}
#else
__device__ __forceinline__ unsigned long long stats_members(const int32_t* subj, int b0, int B, int s) {
    const int b = b0 + (int)(threadIdx.x % VG_WAVE);
    return __builtin_amdgcn_ballot_w64(b < B && subj[b] == s);
}
#endif
// No instruction: marks a wave-uniform value as redefined, in a scalar register.  The `i < C` tests of the unrolled covariate loops are
// loop invariants; hoisted, each is kept as a 64-bit lane mask for the whole batch loop (2 * CMAX scalar registers: spills).  Computed
// from a value redefined inside the loop they stay one s_cmp in front of their branch.
#ifdef VG_EMU
static inline int stats_here(int c) { return c; }
#else
__device__ __forceinline__ int stats_here(int c) { asm volatile("" : "+s"(c)); return c; }
#endif
struct StatsMembers {
    const int32_t* subj;
    int B, s, b0;
    unsigned long long m;
    __device__ __forceinline__ int next() {                            // -> the next member, or -1 (and -1 from then on)
        while (!m) {
            b0 += VG_WAVE;
            if (b0 >= B) { b0 = B; return -1; }
            m = stats_members(subj, b0, B, s);
        }
        const int k = __builtin_ctzll(m);
        m &= m - 1;
        return b0 + k;
    }
};

// what one thread loads of one volume ahead of its arithmetic: its voxel's C+1 logits and data value
template <int CMAX>
struct StatsRaw { float lg[CMAX + 1], x; };

// acc[s][k][vn] += the sums over subject s's volumes of this batch (slot table: include/vaegam.h).  grid (vblocks, S): a thread owns
// voxel v of subject blockIdx.y for the whole launch, folds that subject's volumes in ascending b into fp64 registers that start at
// 0 and adds each of them to its accumulator entry ONCE -- no atomics, the same bits on every run.  The map values are gam_fwd_k's, by
// the same fp32 expressions; sums and squares are formed in fp64 from them.
// Latency, not occupancy, is what has to be hidden (about one block per CU and subject at 41x49x35): the volumes go in groups of U
// whose (C+2) * U loads per lane are issued together, and the loads of group g+1 are issued BEFORE the arithmetic of group g.
// CMAX: compile-time bound of the covariate loops (fully unrolled: every register array is indexed by constants); EMB / MSK as in
// gam_bwd_k.  A thread on a voxel that does not count (behind the end, padding, outside the mask) loads nothing and writes nothing;
// a block whose subject has no volume in the batch writes nothing.
template <int CMAX, int U, bool EMB, bool MSK>
__global__ void __launch_bounds__(GT)
gam_stats_k(const float* __restrict__ logits, const float* __restrict__ gain, const float* __restrict__ x, const int32_t* __restrict__ subj,
            const uint8_t* __restrict__ mask, int C_, int B, long long V, double* __restrict__ acc, GamGrid e) {
    const int s = blockIdx.y;
    const long long v = (long long)blockIdx.x * GT + threadIdx.x;
    const bool ok = v < V;
    long long nc = ok ? v : 0;                                         // the voxel's index in the native tensors
    bool nat = ok;                                                     // a voxel that counts
    if (EMB) { nat = grid_to_native(e, ok ? v : 0, nc) && ok; if (!nat) nc = 0; }
    if (MSK) nat = nat && mask[nc] != 0;
    const long long Vn = EMB ? e.Vn : V;
    const size_t BV = (size_t)B * V;
    StatsMembers it{subj, B, s, -VG_WAVE, 0ull};
    StatsRaw<CMAX> nxt[U];
    int nb[U];
    auto fetch = [&]() {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            nb[u] = it.next();
            const int b = nb[u], C = stats_here(C_);
            nxt[u].x = 0.f;
#pragma unroll
            for (int i = 0; i <= CMAX; ++i) nxt[u].lg[i] = 0.f;
            if (b >= 0 && nat) {
                const float* lp = logits + ((size_t)b * V + v);          // a running pointer: one uniform stride, not CMAX offsets
                nxt[u].x = x[(size_t)b * Vn + nc];
                nxt[u].lg[0] = *lp;
#pragma unroll
                for (int i = 0; i < CMAX; ++i) if (i < C) { lp += BV; nxt[u].lg[i + 1] = *lp; }
            }
        }
    };
    double sm[CMAX + 1], sq[CMAX + 1], sp[CMAX];                       // base and cons_i: sums, sums of squares; sums of (r + cons_i)^2
#pragma unroll
    for (int i = 0; i <= CMAX; ++i) sm[i] = sq[i] = 0.0;
#pragma unroll
    for (int i = 0; i < CMAX; ++i) sp[i] = 0.0;
    double s_rec = 0.0, q_rec = 0.0, s_x = 0.0, q_x = 0.0, s_r = 0.0, q_r = 0.0;
    int n = 0;                                                         // volumes folded (block-uniform)
    fetch();
    while (nb[0] >= 0) {
        StatsRaw<CMAX> cur[U];
        int cb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { cur[u] = nxt[u]; cb[u] = nb[u]; }
        fetch();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (cb[u] < 0) continue;                                   // wave-uniform
            ++n;
            const int C = stats_here(C_);
            float cons[CMAX];
            const float base = sigmoidf_(cur[u].lg[0]);
            float xrec = base;
            const float* gp = gain + cb[u];                            // (the gains: scalar loads)
#pragma unroll
            for (int i = 0; i < CMAX; ++i) {
                cons[i] = 0.f;
                if (i < C) { cons[i] = *gp * sigmoidf_(cur[u].lg[i + 1]); xrec += cons[i]; gp += B; }
            }
            const float r = cur[u].x - xrec;
            const double bd = base, xd = cur[u].x, rd = r, recd = xrec;
            sm[0] += bd; sq[0] += bd * bd;
            s_rec += recd; q_rec += recd * recd;
            s_x += xd; q_x += xd * xd;
            s_r += rd; q_r += rd * rd;
#pragma unroll
            for (int i = 0; i < CMAX; ++i) {
                const double cd = cons[i], t = rd + cd;                // (beyond C: cons = 0, sums that are never written)
                sm[i + 1] += cd; sq[i + 1] += cd * cd; sp[i] += t * t;
            }
        }
    }
    if (!nat || n == 0) return;
    const int C = C_;
    const size_t Vs = (size_t)Vn;
    double* a = acc + (size_t)s * (size_t)(3 * C + 8) * Vs + (size_t)nc;      // walks the subject's slots in order
    *a += sm[0]; a += Vs;
#pragma unroll
    for (int i = 0; i < CMAX; ++i) if (i < C) { *a += sm[i + 1]; a += Vs; }
    *a += s_rec; a += Vs;
    *a += sq[0]; a += Vs;
#pragma unroll
    for (int i = 0; i < CMAX; ++i) if (i < C) { *a += sq[i + 1]; a += Vs; }
    *a += q_rec; a += Vs;
    *a += s_x; a += Vs;
    *a += q_x; a += Vs;
    *a += s_r; a += Vs;
    *a += q_r; a += Vs;
#pragma unroll
    for (int i = 0; i < CMAX; ++i) if (i < C) { *a += sp[i]; a += Vs; }
}

int fwd_chunks(long long V) { return (int)((V + (long long)GT * GV - 1) / ((long long)GT * GV)); }
int bwd_vblocks(long long V) { return (int)((V + GT - 1) / GT); }
int bwd_gain_parts(long long V) { return bwd_vblocks(V) * (GT / VG_WAVE); }
int bwd_bs(int B) { return B < 8 ? B : 8; }

// ---------------------------------------------------------------------------------- Adam
template <typename T>
__global__ void __launch_bounds__(256)
adam_k(T* __restrict__ p, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, long long n,
       double b1, double b2, double eps, const double* __restrict__ sc) {
    const T step_size = (T)sc[0], bc2_sqrt = (T)sc[1];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const T gi = g[i];
        const T mi = m[i] + (gi - m[i]) * (T)(1.0 - b1);               // lerp_(grad, 1-beta1)
        const T vi = v[i] * (T)b2 + (T)(1.0 - b2) * gi * gi;           // mul_(beta2).addcmul_(g, g, 1-beta2)
        m[i] = mi; v[i] = vi;
        const T denom = sqrt(vi) / bc2_sqrt + (T)eps;
        p[i] = p[i] - step_size * (mi / denom);
    }
}

// One thread: advance the optimiser's step count ON THE DEVICE and derive the two bias-correction scalars adam_k reads.
// st = [step_size, bc2_sqrt, t].  Living inside the (captured) step, the count can never run ahead of the launches that
// use it -- a host-staged scalar buffer rewritten for step t+1 could be read by step t's still-queued kernels.
__global__ void adam_advance_k(double* __restrict__ st, double lr, double b1, double b2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double t = st[2] + 1.0;
    st[2] = t;
    st[0] = lr / (1.0 - pow(b1, t));
    st[1] = sqrt(1.0 - pow(b2, t));
}

// ---------------------------------------------------------------------------------- gradient guard
// Global gradient norm, clip factor and skip decision on the device (state layout: include/vaegam.h).  Sum of squares in fp64 in a
// FIXED order: element -> thread -> block is a function of (n32, n64) alone (the grid is never sized by the device), each block folds
// its threads by the same shuffle tree, and one block folds the per-block partials the same way -- the same bits on every run and on
// every data-parallel rank.  fp32 elements go in quads (one 16-byte load where the buffer is 16-byte aligned; an unaligned buffer walks
// the same quads with scalar loads, so alignment does not change a bit of the result either).
constexpr int GG_T = 256, GG_MAXB32 = 256, GG_MAXB64 = 64;
int gg_blocks32(long long n) { const long long b = (n + GG_T * 16 - 1) / (GG_T * 16); return b > GG_MAXB32 ? GG_MAXB32 : (int)b; }
int gg_blocks64(long long n) { const long long b = (n + GG_T * 4 - 1) / (GG_T * 4); return b > GG_MAXB64 ? GG_MAXB64 : (int)b; }

__device__ __forceinline__ bool gg_finite(double x) {          // exponent field not all ones (no reliance on how the compiler treats isfinite)
    union { double d; unsigned long long u; } t; t.d = x;
    return (t.u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// sum over the block's GG_T threads in a fixed order, valid in thread 0
__device__ __forceinline__ double gg_block_sum(double a, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if (threadIdx.x % VG_WAVE == 0) red[threadIdx.x / VG_WAVE] = a;
    __syncthreads();
    double t = 0;
    if (threadIdx.x == 0) for (int w = 0; w < GG_T / VG_WAVE; ++w) t += red[w];
    return t;
}

// blocks [0, nb32): the fp32 buffer; blocks [nb32, gridDim.x): the fp64 buffer.  part[blockIdx.x] = this block's sum of squares.
__global__ void __launch_bounds__(GG_T)
grad_sumsq_k(const float* __restrict__ g32, long long n32, int nb32, const double* __restrict__ g64, long long n64,
             double* __restrict__ part) {
    __shared__ double red[GG_T / VG_WAVE];
    double a = 0;
    if ((int)blockIdx.x < nb32) {
        const long long nthr = (long long)nb32 * GG_T, nq = n32 >> 2, me = (long long)blockIdx.x * GG_T + threadIdx.x;
        const bool vec = ((uintptr_t)g32 & 15) == 0;
        for (long long q = me; q < nq; q += nthr) {
            float4 x;
            if (vec) x = reinterpret_cast<const float4*>(g32)[q];
            else { x.x = g32[4 * q]; x.y = g32[4 * q + 1]; x.z = g32[4 * q + 2]; x.w = g32[4 * q + 3]; }
            a += (double)x.x * (double)x.x; a += (double)x.y * (double)x.y; a += (double)x.z * (double)x.z; a += (double)x.w * (double)x.w;
        }
        if (me == 0) for (long long i = nq << 2; i < n32; ++i) a += (double)g32[i] * (double)g32[i];      // the up to 3 elements behind the quads
    } else {
        const long long nthr = (long long)(gridDim.x - nb32) * GG_T;
        for (long long i = (long long)(blockIdx.x - nb32) * GG_T + threadIdx.x; i < n64; i += nthr) a += g64[i] * g64[i];
    }
    const double t = gg_block_sum(a, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one block: fixed-order sum of the partials, then thread 0 derives norm / scale / apply and moves the counters
__global__ void __launch_bounds__(GG_T)
grad_guard_final_k(const double* __restrict__ part, int np, double max_norm, int skip_nonfinite, double* __restrict__ st) {
    __shared__ double red[GG_T / VG_WAVE];
    double a = 0;
    for (int k = threadIdx.x; k < np; k += GG_T) a += part[k];
    const double ss = gg_block_sum(a, red);
    if (threadIdx.x != 0) return;
    const bool finite = gg_finite(ss);
    const double norm = sqrt(ss);
    double scale = 1.0;
    if (max_norm > 0) { const double c = max_norm / (norm + 1e-6); scale = c > 1.0 ? 1.0 : c; }      // a nan norm stays nan, as clamp(max=1) leaves it
    const double apply = (!finite && skip_nonfinite) ? 0.0 : 1.0;
    st[0] = norm; st[1] = scale; st[2] = apply;
    st[3] += 1.0;
    if (apply == 0.0) st[4] += 1.0;
    if (finite) {
        if (scale < 1.0) st[5] += 1.0;
        st[6] += norm;
        if (norm > st[7]) st[7] = norm;
    }
}

// the scaled gradient as a LEAF of the update's arithmetic, as the loaded gradient is in adam_k: left visible, the compiler may contract
// g * scale into the expressions that use it and pick other fused multiply-adds than adam_k's -- measured on gfx950 as fp64 moments that
// differ in the last bit at scale = 1, where the guarded update promises adam_k's bits
#ifdef VG_EMU
template <typename T> static inline T gg_leaf(T v) { return v; }
#else
template <typename T> __device__ __forceinline__ T gg_leaf(T v) { asm volatile("" : "+v"(v)); return v; }
#endif

// adam_k reading the guard's verdict: the gradient is scaled on load (the buffer keeps the raw gradient), a skipped step writes nothing
template <typename T>
__global__ void __launch_bounds__(256)
adam_guarded_k(T* __restrict__ p, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, long long n,
               double b1, double b2, double eps, const double* __restrict__ sc, const double* __restrict__ guard) {
    if (guard[2] == 0.0) return;
    const T step_size = (T)sc[0], bc2_sqrt = (T)sc[1], scale = (T)guard[1];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const T gi = gg_leaf(g[i] * scale);
        const T mi = m[i] + (gi - m[i]) * (T)(1.0 - b1);
        const T vi = v[i] * (T)b2 + (T)(1.0 - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const T denom = sqrt(vi) / bc2_sqrt + (T)eps;
        p[i] = p[i] - step_size * (mi / denom);
    }
}

// adam_advance_k that stands still on a skipped step: t counts the updates that were applied
__global__ void adam_advance_guarded_k(double* __restrict__ st, double lr, double b1, double b2, const double* __restrict__ guard) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || guard[2] == 0.0) return;
    const double t = st[2] + 1.0;
    st[2] = t;
    st[0] = lr / (1.0 - pow(b1, t));
    st[1] = sqrt(1.0 - pow(b2, t));
}

// ---------------------------------------------------------------------------------- weight packing
// all conv / transposed-conv weights of the model -> the [ci][tap][co] images the conv kernels read through the scalar
// path (forward and data-gradient variants), in ONE launch straight from the flat parameter buffer
__global__ void __launch_bounds__(256)
pack_weights_k(const float* __restrict__ flat, float* __restrict__ packed, const long long* __restrict__ gsegs, int nseg, long long total) {
    // the segment table (a few hundred bytes) is searched per element: from LDS, not as a chain of dependent global loads
    constexpr int MAXSEG = 64;
    __shared__ long long ssegs[MAXSEG * 8];
    const bool in_lds = nseg <= MAXSEG;
    if (in_lds) for (int i = threadIdx.x; i < nseg * 8; i += blockDim.x) ssegs[i] = gsegs[i];
    __syncthreads();
    const long long* segs = in_lds ? ssegs : gsegs;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        int sgi = 0;
        while (sgi + 1 < nseg && e >= segs[(sgi + 1) * 8 + 1]) ++sgi;            // segments are sorted by destination offset
        const long long* sg = segs + sgi * 8;
        const long long src = sg[0], dst = sg[1];
        const int d0 = (int)sg[2], d1 = (int)sg[3], kvol = (int)sg[4], mode = (int)sg[5];
        const long long r = e - dst;
        if (r >= sg[6]) continue;            // alignment gap behind the segment
        long long si;
        if (mode == 0) {                     // out[i1][t][i0] = w[i0][i1][t]
            const int i0 = (int)(r % d0); const long long q = r / d0; const int t = (int)(q % kvol); const int i1 = (int)(q / kvol);
            si = ((long long)i0 * d1 + i1) * kvol + t;
        } else {                             // out[i0][t][i1] = w[i0][i1][t or kvol-1-t]
            const int i1 = (int)(r % d1); const long long q = r / d1; const int t = (int)(q % kvol); const int i0 = (int)(q / kvol);
            si = ((long long)i0 * d1 + i1) * kvol + (mode == 2 ? kvol - 1 - t : t);
        }
        packed[e] = flat[src + si];
    }
}

// ---------------------------------------------------------------------------------- sign-flip permutation test, max-statistic
// One lane owns one voxel: its S subject means sit in registers (mv[], indexed by constants only), and the lane walks the sign words of
// its block's permutation chunk.  Per permutation p (include/vaegam.h has the statistic to the bit):
//   T = +0.0;  for s ascending: T = T + sg * m[s]   (sg = -1.0 where bit s of the word is set, else 1.0: the product is exact, so the
//   fused and the unfused form give the same bits);  g = tail(T * scale);  count += tail(T) >= tail(T_id).
// The words are wave-uniform: read through the constant address space (scalar loads), each sign is a scalar select between the two
// inline constants and reaches the vector ALU as the scalar operand of one v_fma_f64 per subject and permutation.  SF_PU permutations
// run side by side (independent chains), subjects go in groups of 4 behind one scalar test of S (the means beyond S are 0.0, which
// changes no bit of T: T is never -0.0).
// The maximum over the block's voxels, per permutation, goes through LDS SF_PB permutations at a time: every lane writes its g (a lane
// without a live voxel: -inf) into tile[perm][lane]; then thread t folds 16 interleaved voxels of permutation t / 16 and the 16 threads
// of a permutation finish by four shuffles.  Row pitch 272 doubles: the two permutations a half-wave reads sit 32 banks apart.
// No floating-point atomics, no atomics at all: part_max[tile][p] and part_cnt[chunk][v] are folded by signflip_fold_k.
constexpr int SF_T = 256;        // lanes per block = voxels per tile
constexpr int SF_PB = 16;        // permutations per trip through LDS
constexpr int SF_PU = 4;         // permutations whose sums run side by side
constexpr int SF_PITCH = SF_T + 16;
constexpr int SF_MIN_CHUNK = 64; // fewest permutations a block walks (but for the last chunk)
constexpr int SF_BLOCKS = 2048;  // blocks the planner aims at: 8 per CU

#ifdef VG_EMU
typedef const unsigned long long* sf_words;
static inline double sf_max(double a, double b) { return a > b ? a : b; }
#else
typedef const __attribute__((address_space(4))) unsigned long long* sf_words;
// one v_max_f64; the same value as the host form: no operand is a nan, and no -0.0 reaches a maximum (signflip_k)
__device__ __forceinline__ double sf_max(double a, double b) { return fmax(a, b); }
#endif
#define SF_NEG_INF (-__builtin_inf())

// -1.0 where bit SB of the (wave-uniform) word is set, else 1.0.  On the GPU as two scalar instructions, a bit test and a select of two
// inline constants into a register pair, which is then the scalar operand of one v_fma_f64: written in C++ the compiler sees through
// the +-1.0 and turns sg * m into a per-lane select of -m or m (a lane mask, a v_cndmask and an add per subject and permutation).
// volatile keeps each select next to its fma: free to hoist them, the scheduler holds more pairs than the SMAX = 64 instance has scalar
// registers for (5 scalar spills).
#ifdef VG_EMU
template <int SB> static inline double sf_sign(unsigned long long w) { return (w >> SB) & 1ull ? -1.0 : 1.0; }
#else
template <int SB> __device__ __forceinline__ double sf_sign(unsigned long long w) {
    double sg;
    asm volatile("s_bitcmp1_b64 %1, %2\n\ts_cselect_b64 %0, -1.0, 1.0" : "=s"(sg) : "s"(w), "n"(SB) : "scc");
    return sg;
}
#endif
// f(integral_constant<int, J>) for J = J0 .. N-1: loops whose counter is a constant expression (a bit number, a register array index)
template <int J, int N, typename F> __device__ __forceinline__ void sf_unroll(F&& f) {
    if constexpr (J < N) { f(std::integral_constant<int, J>{}); sf_unroll<J + 1, N>(f); }
}

// TAIL 0: |.|, 1: as it is, 2: negated
template <int TAIL> __device__ __forceinline__ bool sf_reaches(double T, double Tid) {
    return TAIL == 0 ? fabs(T) >= fabs(Tid) : (TAIL == 1 ? T >= Tid : T <= Tid);
}

// grid (voxel tiles, permutation chunks).  ssc = scale, negated for TAIL 2: T * -scale = -(T * scale) to the bit.
template <int SMAX, int TAIL>
__global__ void __launch_bounds__(SF_T)
signflip_k(const double* __restrict__ m, const double* __restrict__ scale, sf_words signs, int S, int V, int P, int chunk,
           double* __restrict__ part_max, int* __restrict__ part_cnt, double* __restrict__ stat0) {
    __shared__ double tile[SF_PB * SF_PITCH];
    const int tid = threadIdx.x;
    const long long v = (long long)blockIdx.x * SF_T + tid;
    const int p0 = (int)blockIdx.y * chunk, p1 = min(P, p0 + chunk);
    const bool in = v < V;
    const double sc = in ? scale[v] : 0.0;
    const bool live = sc > 0.0;
    const double ssc = TAIL == 2 ? -sc : sc;
    double mv[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) { mv[s] = 0.0; if (s < S && live) mv[s] = m[(size_t)s * (size_t)V + (size_t)v]; }
    double Tid = 0.0;                                                  // the identity, apart from the sign list
#pragma unroll
    for (int s = 0; s < SMAX; ++s) Tid = Tid + mv[s];
    if (blockIdx.y == 0 && in) {
        const double u = Tid * ssc;
        stat0[v] = live ? (TAIL == 0 ? fabs(u) : u) : 0.0;
    }
    int cnt = 0;
    for (int pb = p0; pb < p1; pb += SF_PB) {
#pragma unroll
        for (int q = 0; q < SF_PB; q += SF_PU) {
            unsigned long long w[SF_PU];
            double T[SF_PU];
#pragma unroll
            for (int k = 0; k < SF_PU; ++k) { w[k] = signs[min(pb + q + k, p1 - 1)]; T[k] = 0.0; }      // (behind the chunk: a word again, result dropped)
            sf_unroll<0, SMAX / 4>([&](auto g4) {
                constexpr int s4 = 4 * decltype(g4)::value;
                if (s4 < S) {                                          // scalar
                    sf_unroll<0, 4>([&](auto j) {
                        constexpr int s = s4 + decltype(j)::value;
#pragma unroll
                        for (int k = 0; k < SF_PU; ++k) T[k] += sf_sign<s>(w[k]) * mv[s];
                    });
                }
            });
#pragma unroll
            for (int k = 0; k < SF_PU; ++k) {
                double g = T[k] * ssc;
                if (TAIL == 0) g = fabs(g); else g = g + 0.0;          // (-0.0 -> +0.0: a zero maximum has defined bits)
                tile[(q + k) * SF_PITCH + tid] = live ? g : SF_NEG_INF;
                cnt += (pb + q + k < p1 && sf_reaches<TAIL>(T[k], Tid)) ? 1 : 0;
            }
        }
        __syncthreads();
        const int pr = tid >> 4, seg = tid & 15;
        double a = SF_NEG_INF;
#pragma unroll
        for (int j = 0; j < 16; ++j) a = sf_max(a, tile[pr * SF_PITCH + j * 16 + seg]);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) a = sf_max(a, __shfl_down(a, off));
        if (seg == 0 && pb + pr < p1) part_max[(size_t)blockIdx.x * (size_t)P + (size_t)(pb + pr)] = a;
        __syncthreads();
    }
    if (in) part_cnt[(size_t)blockIdx.y * (size_t)V + (size_t)v] = cnt;   // (a voxel that takes no part: T = T_id = 0, every permutation counted)
}

// blocks [0, nbp): maxstat[p] = max over the tiles; the others: cnt_unc[v] = sum over the chunks
__global__ void __launch_bounds__(SF_T)
signflip_fold_k(const double* __restrict__ part_max, const int* __restrict__ part_cnt, int tiles, int chunks, int V, int P, int nbp,
                double* __restrict__ maxstat, int* __restrict__ cnt_unc) {
    if ((int)blockIdx.x < nbp) {
        const int p = (int)blockIdx.x * SF_T + threadIdx.x;
        if (p >= P) return;
        double a = SF_NEG_INF;
        for (int t = 0; t < tiles; ++t) a = sf_max(a, part_max[(size_t)t * (size_t)P + (size_t)p]);
        maxstat[p] = a;
    } else {
        const long long v = (long long)((int)blockIdx.x - nbp) * SF_T + threadIdx.x;
        if (v >= V) return;
        int c = 0;
        for (int k = 0; k < chunks; ++k) c += part_cnt[(size_t)k * (size_t)V + (size_t)v];
        cnt_unc[v] = c;
    }
}

// every launch decision of vg_signflip_maxstat, in the order vg_signflip_plan reports it
struct SignflipPlan { int smax, tiles, chunk, chunks, fold_blocks; long long ws; };

// 0 fine, VG_ERR_ARG, or VG_ERR_UNSUPPORTED (S > 64)
int signflip_shape(int S, long long V, int P) {
    if (S < 2 || V <= 0 || V >= (1LL << 31) || P <= 0 || P > (1 << 20)) return VG_ERR_ARG;
    return S > 64 ? VG_ERR_UNSUPPORTED : VG_OK;
}

SignflipPlan signflip_plan(int S, long long V, int P) {
    SignflipPlan p;
    p.smax = S <= 8 ? 8 : (S <= 16 ? 16 : (S <= 32 ? 32 : 64));
    p.tiles = (int)((V + SF_T - 1) / SF_T);
    const int want = p.tiles >= SF_BLOCKS ? 1 : vg_cdiv(SF_BLOCKS, p.tiles);
    p.chunk = vg_cdiv(vg_cdiv(P, want), SF_PB) * SF_PB;
    if (p.chunk < SF_MIN_CHUNK) p.chunk = SF_MIN_CHUNK;
    p.chunks = vg_cdiv(P, p.chunk);
    p.fold_blocks = vg_cdiv(P, SF_T) + p.tiles;
    p.ws = (long long)p.tiles * P * (long long)sizeof(double) + (long long)p.chunks * V * (long long)sizeof(int);
    return p;
}

}  // namespace

extern "C" int vg_pack_weights(const float* flat, float* packed, const int64_t* segs, int32_t nseg, int64_t total, void* stream) {
    if (!flat || !packed || !segs || nseg <= 0 || total <= 0) { vg_set_error("vg_pack_weights: bad arguments"); return VG_ERR_ARG; }
    long long blocks = (total + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    vg_launch(pack_weights_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flat, packed, (const long long*)segs, (int)nseg, (long long)total);
    return vg_check_launch("pack_weights");
}

extern "C" int64_t vg_gam_ws_bytes(int32_t C, int32_t B, int64_t V) {
    if (C < 0 || C > GMAXC || B <= 0 || V <= 0) return -1;
    const int64_t fwd = ((int64_t)B * fwd_chunks(V) + (int64_t)C * B * fwd_chunks(V)) * sizeof(float);
    const int64_t bwd = ((int64_t)bwd_bs(B) * V + (int64_t)C * B * bwd_gain_parts(V) + (int64_t)bwd_bs(B) * bwd_gain_parts(V)) * sizeof(float);
    return fwd > bwd ? fwd : bwd;
}

namespace {

void grid_magic(unsigned d, unsigned& m, int& s) {
    int c = 0;
    while ((1u << c) < d) ++c;
    s = 31 + c;
    m = (unsigned)(((1ull << s) / d) + 1);
}

// -> V_G, or -1: nat must fit into grid and the grid's voxel indices (plus a block's overhang) into 31 bits
long long make_grid(const int32_t* nat, const int32_t* grid, GamGrid& e) {
    if (!nat || !grid) return -1;
    for (int a = 0; a < 3; ++a) if (nat[a] < 1 || grid[a] < nat[a]) return -1;
    const long long Vg = (long long)grid[0] * grid[1] * grid[2];
    if (Vg > 0x7fffffffLL - 2 * GT * GV) return -1;
    e.nd = nat[0]; e.nh = nat[1]; e.nw = nat[2]; e.gd = grid[0]; e.gh = grid[1]; e.gw = grid[2];
    grid_magic((unsigned)e.gw, e.mw, e.sw);
    grid_magic((unsigned)e.gh, e.mh, e.sh);
    e.Vn = (long long)nat[0] * nat[1] * nat[2];
    return Vg;
}

int gam_fwd(const float* logits, const float* gain, const float* x, const double* eps, const float* glm, int32_t C, int32_t B, int64_t V,
            const GamGrid* e, const uint8_t* mask, void* ws, float* sum_log_prob, float* dist, float* maps_out, void* stream);
int gam_bwd(const float* logits, const float* gain, const float* x, const double* eps, const float* glm, const float* dist,
            const float* g_slp, const float* g_dist, int32_t C, int32_t B, int64_t V, const GamGrid* e, const uint8_t* mask,
            void* ws, float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream);

}  // namespace

extern "C" int vg_embed_volumes(const float* x, const int32_t* nat, const int32_t* grid, int32_t B, float* out, void* stream) {
    GamGrid e;
    const long long V = make_grid(nat, grid, e);
    if (!x || !out || V < 0 || B <= 0 || B > 65535) { vg_set_error("vg_embed_volumes: bad arguments B=%d", B); return VG_ERR_ARG; }
    vg_launch(embed_k, dim3(fwd_chunks(V), B), dim3(GT), 0, (hipStream_t)stream, x, out, V, e);
    return vg_check_launch("embed_volumes");
}

extern "C" int vg_gam_elbo_fwd(const float* logits, const float* gain, const float* x, const double* eps,
                               const float* glm, int32_t C, int32_t B, int64_t V, void* ws,
                               float* sum_log_prob, float* dist, float* maps_out, void* stream) {
    return gam_fwd(logits, gain, x, eps, glm, C, B, V, nullptr, nullptr, ws, sum_log_prob, dist, maps_out, stream);
}

extern "C" int vg_gam_elbo_fwd_embed(const float* logits, const float* gain, const float* x, const double* eps,
                                     const float* glm, int32_t C, int32_t B, const int32_t* nat, const int32_t* grid, void* ws,
                                     float* sum_log_prob, float* dist, float* maps_out, void* stream) {
    GamGrid e;
    const long long V = make_grid(nat, grid, e);
    if (V < 0) { vg_set_error("vg_gam_elbo_fwd_embed: the native grid must fit into a grid of less than 2^31 voxels"); return VG_ERR_ARG; }
    return gam_fwd(logits, gain, x, eps, glm, C, B, V, &e, nullptr, ws, sum_log_prob, dist, maps_out, stream);
}

extern "C" int vg_gam_elbo_bwd(const float* logits, const float* gain, const float* x, const double* eps,
                               const float* glm, const float* dist, const float* g_slp, const float* g_dist,
                               int32_t C, int32_t B, int64_t V, void* ws,
                               float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream) {
    return gam_bwd(logits, gain, x, eps, glm, dist, g_slp, g_dist, C, B, V, nullptr, nullptr, ws, d_logits, d_gain, d_eps, d_total, total_accumulate, stream);
}

extern "C" int vg_gam_elbo_bwd_embed(const float* logits, const float* gain, const float* x, const double* eps,
                                     const float* glm, const float* dist, const float* g_slp, const float* g_dist,
                                     int32_t C, int32_t B, const int32_t* nat, const int32_t* grid, void* ws,
                                     float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream) {
    GamGrid e;
    const long long V = make_grid(nat, grid, e);
    if (V < 0) { vg_set_error("vg_gam_elbo_bwd_embed: the native grid must fit into a grid of less than 2^31 voxels"); return VG_ERR_ARG; }
    return gam_bwd(logits, gain, x, eps, glm, dist, g_slp, g_dist, C, B, V, &e, nullptr, ws, d_logits, d_gain, d_eps, d_total, total_accumulate, stream);
}

// nat == grid: the kernels without the index decode, as the plain pair; any other nat: those of the _embed pair
extern "C" int vg_gam_elbo_fwd_masked(const float* logits, const float* gain, const float* x, const double* eps,
                                      const float* glm, const uint8_t* mask, int32_t C, int32_t B, const int32_t* nat, const int32_t* grid,
                                      void* ws, float* sum_log_prob, float* dist, float* maps_out, void* stream) {
    GamGrid e;
    const long long V = make_grid(nat, grid, e);
    if (V < 0) { vg_set_error("vg_gam_elbo_fwd_masked: the native grid must fit into a grid of less than 2^31 voxels"); return VG_ERR_ARG; }
    if (!mask) { vg_set_error("vg_gam_elbo_fwd_masked: no mask"); return VG_ERR_ARG; }
    return gam_fwd(logits, gain, x, eps, glm, C, B, V, e.Vn == V ? nullptr : &e, mask, ws, sum_log_prob, dist, maps_out, stream);
}

extern "C" int vg_gam_elbo_bwd_masked(const float* logits, const float* gain, const float* x, const double* eps,
                                      const float* glm, const uint8_t* mask, const float* dist, const float* g_slp, const float* g_dist,
                                      int32_t C, int32_t B, const int32_t* nat, const int32_t* grid, void* ws,
                                      float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream) {
    GamGrid e;
    const long long V = make_grid(nat, grid, e);
    if (V < 0) { vg_set_error("vg_gam_elbo_bwd_masked: the native grid must fit into a grid of less than 2^31 voxels"); return VG_ERR_ARG; }
    if (!mask) { vg_set_error("vg_gam_elbo_bwd_masked: no mask"); return VG_ERR_ARG; }
    return gam_bwd(logits, gain, x, eps, glm, dist, g_slp, g_dist, C, B, V, e.Vn == V ? nullptr : &e, mask, ws, d_logits, d_gain, d_eps, d_total,
                   total_accumulate, stream);
}

extern "C" int32_t vg_gam_stats_slots(int32_t C) { return (C < 0 || C > GMAXC) ? -1 : 3 * C + 8; }

// nat == grid: the instances without the index decode; mask may be null
extern "C" int vg_gam_stats_accumulate(const float* logits, const float* gain, const float* x, const int32_t* subj, const uint8_t* mask,
                                       int32_t C, int32_t B, int32_t S, const int32_t* nat, const int32_t* grid, double* acc, void* stream) {
    if (!logits || !x || !subj || !acc || (C > 0 && !gain) || C < 0 || B <= 0 || B > 65535 || S <= 0 || S > 65535) {
        vg_set_error("vg_gam_stats_accumulate: bad arguments C=%d B=%d S=%d", C, B, S); return VG_ERR_ARG;
    }
    if (C > GMAXC) { vg_set_error("vg_gam_stats_accumulate: more than 16 covariates"); return VG_ERR_UNSUPPORTED; }
    GamGrid e;
    const long long V = make_grid(nat, grid, e);
    if (V < 0) { vg_set_error("vg_gam_stats_accumulate: the native grid must fit into a grid of less than 2^31 voxels"); return VG_ERR_ARG; }
    const bool emb = e.Vn != V;
    hipStream_t s = (hipStream_t)stream;
#define VG_GAM_STATS(CMAX, U, EMB, MSK)                                                                                                \
    vg_launch(gam_stats_k<CMAX, U, EMB, MSK>, dim3(bwd_vblocks(V), S), dim3(GT), 0, s, logits, gain, x, subj, mask, (int)C, (int)B, V, acc, e)
#define VG_GAM_STATS_C(CMAX, U)                                                                      \
    if (mask) { if (emb) VG_GAM_STATS(CMAX, U, true, true); else VG_GAM_STATS(CMAX, U, false, true); } \
    else { if (emb) VG_GAM_STATS(CMAX, U, true, false); else VG_GAM_STATS(CMAX, U, false, false); }
    if (C <= 8) { VG_GAM_STATS_C(8, 4) }
    else { VG_GAM_STATS_C(16, 2) }
#undef VG_GAM_STATS_C
#undef VG_GAM_STATS
    return vg_check_launch("gam_stats");
}

namespace {

// V: voxels of the tensor the logits are on; emb: the embedded grid, or nullptr (everything on one grid); mask: [Vn] bytes, or nullptr
int gam_fwd(const float* logits, const float* gain, const float* x, const double* eps, const float* glm, int32_t C, int32_t B, int64_t V,
            const GamGrid* emb, const uint8_t* mask, void* ws, float* sum_log_prob, float* dist, float* maps_out, void* stream) {
    if (!logits || !x || !eps || !ws || !sum_log_prob || (C > 0 && (!gain || !glm || !dist)) || C < 0 || C > GMAXC || B <= 0 ||
        B > 65535 || V <= 0) {
        vg_set_error("vg_gam_elbo_fwd: bad arguments C=%d B=%d V=%lld", C, B, (long long)V); return VG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int chunks = fwd_chunks(V);
    float* part_slp = (float*)ws;
    float* part_d2 = part_slp + (size_t)B * chunks;
    const GamGrid e = emb ? *emb : GamGrid{};
#define VG_GAM_FWD(EMB, MSK)                                                                                                               \
    vg_launch(gam_fwd_k<EMB, MSK>, dim3(chunks, B), dim3(GT), 0, s, logits, gain, x, eps, glm, (int)C, (int)B, (long long)V, part_slp, part_d2, \
              maps_out, e, mask)
    if (mask) { if (emb) VG_GAM_FWD(true, true); else VG_GAM_FWD(false, true); }
    else { if (emb) VG_GAM_FWD(true, false); else VG_GAM_FWD(false, false); }
#undef VG_GAM_FWD
    int rc = vg_check_launch("gam_fwd");
    if (rc) return rc;
    vg_launch(gam_fwd_fold_k, dim3((C + 1) * B), dim3(64), 0, s, (const float*)part_slp, (const float*)part_d2,
              (int)C, (int)B, chunks, sum_log_prob, dist);
    return vg_check_launch("gam_fwd_fold");
}

int gam_bwd(const float* logits, const float* gain, const float* x, const double* eps, const float* glm, const float* dist,
            const float* g_slp, const float* g_dist, int32_t C, int32_t B, int64_t V, const GamGrid* emb, const uint8_t* mask,
            void* ws, float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream) {
    if (!logits || !x || !eps || !ws || !g_slp || !d_logits || !d_eps || (C > 0 && (!gain || !glm || !dist || !g_dist || !d_gain)) ||
        C < 0 || C > GMAXC || B <= 0 || V <= 0) {
        vg_set_error("vg_gam_elbo_bwd: bad arguments C=%d B=%d V=%lld", C, B, (long long)V); return VG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int vblocks = bwd_vblocks(V), BS = bwd_bs(B);
    float* part_dsig = (float*)ws;
    float* part_dgain = part_dsig + (size_t)BS * V;
    float* part_tot = d_total ? part_dgain + (size_t)C * B * bwd_gain_parts(V) : nullptr;
    const GamGrid e = emb ? *emb : GamGrid{};
    const long long Vn = emb ? emb->Vn : (long long)V;                   // voxels of x / eps / d_eps
#define VG_GAM_BWD(CMAX, EMB, MSK)                                                                                                     \
    vg_launch(gam_bwd_k<CMAX, EMB, MSK>, dim3(vblocks, BS), dim3(GT), 0, s, logits, gain, x, eps, glm, dist, g_slp, g_dist, (int)C, (int)B, \
              (long long)V, d_logits, part_dsig, part_dgain, part_tot, e, mask)
#define VG_GAM_BWD_C(CMAX)                                                                  \
    if (mask) { if (emb) VG_GAM_BWD(CMAX, true, true); else VG_GAM_BWD(CMAX, false, true); } \
    else { if (emb) VG_GAM_BWD(CMAX, true, false); else VG_GAM_BWD(CMAX, false, false); }
    if (C <= 8) { VG_GAM_BWD_C(8) }
    else if (C <= 16) { VG_GAM_BWD_C(16) }
    else { vg_set_error("vg_gam_elbo_bwd: more than 16 covariates"); return VG_ERR_UNSUPPORTED; }
#undef VG_GAM_BWD_C
#undef VG_GAM_BWD
    int rc = vg_check_launch("gam_bwd");
    if (rc) return rc;
    if (C > 0) {
        vg_launch(gam_bwd_fold_gain_k, dim3(C * B), dim3(64), 0, s, (const float*)part_dgain, (int)(C * B), bwd_gain_parts(V), d_gain);
        if ((rc = vg_check_launch("gam_bwd_fold_gain"))) return rc;
    }
    vg_launch(gam_bwd_fold_eps_k, dim3((unsigned)((Vn + 255) / 256)), dim3(256), 0, s, (const float*)part_dsig, eps, BS, Vn, d_eps);
    if ((rc = vg_check_launch("gam_bwd_fold_eps"))) return rc;
    if (d_total) {
        vg_launch(gam_bwd_fold_total_k, dim3(1), dim3(256), 0, s, (const float*)part_tot, BS * bwd_gain_parts(V), (int)total_accumulate, d_total);
        return vg_check_launch("gam_bwd_fold_total");
    }
    return VG_OK;
}

}  // namespace

extern "C" int vg_adam_advance(double* state, double lr, double b1, double b2, void* stream) {
    if (!state || !(lr > 0) || !(b1 >= 0 && b1 < 1) || !(b2 >= 0 && b2 < 1)) { vg_set_error("vg_adam_advance: bad arguments"); return VG_ERR_ARG; }
    vg_launch(adam_advance_k, dim3(1), dim3(64), 0, (hipStream_t)stream, state, lr, b1, b2);
    return vg_check_launch("adam_advance");
}

extern "C" int vg_adam_step(void* p, const void* g, void* m, void* v, int64_t n, int32_t is_f64,
                            double b1, double b2, double eps, const double* step_scalars, void* stream) {
    if (!p || !g || !m || !v || !step_scalars || n <= 0) { vg_set_error("vg_adam_step: bad arguments"); return VG_ERR_ARG; }
    long long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = (hipStream_t)stream;
    if (is_f64)
        vg_launch(adam_k<double>, dim3((unsigned)blocks), dim3(256), 0, s, (double*)p, (const double*)g, (double*)m, (double*)v,
                  (long long)n, b1, b2, eps, step_scalars);
    else
        vg_launch(adam_k<float>, dim3((unsigned)blocks), dim3(256), 0, s, (float*)p, (const float*)g, (float*)m, (float*)v,
                  (long long)n, b1, b2, eps, step_scalars);
    return vg_check_launch("adam");
}

extern "C" int64_t vg_grad_guard_ws_bytes(int64_t n32, int64_t n64) {
    if (n32 < 0 || n64 < 0 || n32 + n64 <= 0) return -1;
    return (int64_t)(gg_blocks32(n32) + gg_blocks64(n64)) * (int64_t)sizeof(double);
}

extern "C" int vg_grad_guard(const float* g32, int64_t n32, const double* g64, int64_t n64, double max_norm, int32_t skip_nonfinite,
                             void* ws, double* state, void* stream) {
    if (n32 < 0 || n64 < 0 || n32 + n64 <= 0 || (n32 > 0 && !g32) || (n64 > 0 && !g64) || !ws || !state || max_norm != max_norm) {
        vg_set_error("vg_grad_guard: bad arguments n32=%lld n64=%lld", (long long)n32, (long long)n64); return VG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int nb32 = gg_blocks32(n32), nb = nb32 + gg_blocks64(n64);
    vg_launch(grad_sumsq_k, dim3((unsigned)nb), dim3(GG_T), 0, s, g32, (long long)n32, nb32, g64, (long long)n64, (double*)ws);
    int rc = vg_check_launch("grad_sumsq");
    if (rc) return rc;
    vg_launch(grad_guard_final_k, dim3(1), dim3(GG_T), 0, s, (const double*)ws, nb, max_norm, (int)(skip_nonfinite != 0), state);
    return vg_check_launch("grad_guard_final");
}

extern "C" int vg_adam_advance_guarded(double* state, double lr, double b1, double b2, const double* guard, void* stream) {
    if (!state || !guard || !(lr > 0) || !(b1 >= 0 && b1 < 1) || !(b2 >= 0 && b2 < 1)) {
        vg_set_error("vg_adam_advance_guarded: bad arguments"); return VG_ERR_ARG;
    }
    vg_launch(adam_advance_guarded_k, dim3(1), dim3(64), 0, (hipStream_t)stream, state, lr, b1, b2, guard);
    return vg_check_launch("adam_advance_guarded");
}

extern "C" int vg_adam_step_guarded(void* p, const void* g, void* m, void* v, int64_t n, int32_t is_f64,
                                    double b1, double b2, double eps, const double* step_scalars, const double* guard, void* stream) {
    if (!p || !g || !m || !v || !step_scalars || !guard || n <= 0) { vg_set_error("vg_adam_step_guarded: bad arguments"); return VG_ERR_ARG; }
    long long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = (hipStream_t)stream;
    if (is_f64)
        vg_launch(adam_guarded_k<double>, dim3((unsigned)blocks), dim3(256), 0, s, (double*)p, (const double*)g, (double*)m, (double*)v,
                  (long long)n, b1, b2, eps, step_scalars, guard);
    else
        vg_launch(adam_guarded_k<float>, dim3((unsigned)blocks), dim3(256), 0, s, (float*)p, (const float*)g, (float*)m, (float*)v,
                  (long long)n, b1, b2, eps, step_scalars, guard);
    return vg_check_launch("adam_guarded");
}

extern "C" int64_t vg_signflip_ws_bytes(int32_t S, int64_t V, int32_t P) {
    if (signflip_shape(S, V, P)) { vg_set_error("vg_signflip_ws_bytes: bad shape (S %d, V %lld, P %d)", S, (long long)V, P); return -1; }
    return (int64_t)signflip_plan(S, V, P).ws;
}

extern "C" int vg_signflip_plan(int32_t S, int64_t V, int32_t P, int32_t* out, int32_t n_out) {
    if (!out || n_out < VG_SIGNFLIP_PLAN_LEN) { vg_set_error("vg_signflip_plan: out must hold %d values", VG_SIGNFLIP_PLAN_LEN); return VG_ERR_ARG; }
    const int rc = signflip_shape(S, V, P);
    if (rc == VG_ERR_UNSUPPORTED) { vg_set_error("vg_signflip_plan: more than 64 subjects"); return rc; }
    if (rc) { vg_set_error("vg_signflip_plan: bad shape (S %d, V %lld, P %d)", S, (long long)V, P); return rc; }
    const SignflipPlan p = signflip_plan(S, V, P);
    const int v[VG_SIGNFLIP_PLAN_LEN] = {p.smax, SF_T, p.tiles, p.chunk, p.chunks, p.tiles, p.chunks, p.fold_blocks,
                                         (int)(SF_PB * SF_PITCH * sizeof(double)), (int)(p.ws & 0x7fffffffLL), (int)(p.ws >> 31)};
    for (int i = 0; i < VG_SIGNFLIP_PLAN_LEN; ++i) out[i] = v[i];
    return VG_OK;
}

extern "C" int vg_signflip_maxstat(const double* m, const double* scale, const uint64_t* signs, int32_t S, int64_t V, int32_t P, int32_t tail,
                                   void* ws, double* stat0, double* maxstat, int32_t* cnt_unc, void* stream) {
    const int rc = signflip_shape(S, V, P);
    if (!m || !scale || !signs || !ws || !stat0 || !maxstat || !cnt_unc || rc == VG_ERR_ARG || tail < 0 || tail > 2) {
        vg_set_error("vg_signflip_maxstat: bad arguments S=%d V=%lld P=%d tail=%d", S, (long long)V, P, tail); return VG_ERR_ARG;
    }
    if (rc) { vg_set_error("vg_signflip_maxstat: more than 64 subjects"); return rc; }
    const SignflipPlan p = signflip_plan(S, V, P);
    double* part_max = (double*)ws;
    int* part_cnt = (int*)(part_max + (size_t)p.tiles * (size_t)P);
    hipStream_t s = (hipStream_t)stream;
#define VG_SIGNFLIP(SMAX, TAIL)                                                                                                     \
    vg_launch(signflip_k<SMAX, TAIL>, dim3(p.tiles, p.chunks), dim3(SF_T), 0, s, m, scale, (sf_words)signs, (int)S, (int)V, (int)P, \
              p.chunk, part_max, part_cnt, stat0)
#define VG_SIGNFLIP_T(SMAX) \
    if (tail == 0) VG_SIGNFLIP(SMAX, 0); else if (tail == 1) VG_SIGNFLIP(SMAX, 1); else VG_SIGNFLIP(SMAX, 2)
    if (p.smax == 8) { VG_SIGNFLIP_T(8); }
    else if (p.smax == 16) { VG_SIGNFLIP_T(16); }
    else if (p.smax == 32) { VG_SIGNFLIP_T(32); }
    else { VG_SIGNFLIP_T(64); }
#undef VG_SIGNFLIP_T
#undef VG_SIGNFLIP
    int lrc = vg_check_launch("signflip");
    if (lrc) return lrc;
    vg_launch(signflip_fold_k, dim3(p.fold_blocks), dim3(SF_T), 0, s, (const double*)part_max, (const int*)part_cnt, p.tiles, p.chunks,
              (int)V, (int)P, vg_cdiv(P, SF_T), maxstat, cnt_unc);
    return vg_check_launch("signflip_fold");
}
