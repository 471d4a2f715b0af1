// Latent sample + KL of the low-rank Gaussian posterior, and the ELBO assembly, as single launches.
//
// The reference does these with ~35 + ~45 elementwise/reduction operators per step (vae_reg_GP.py:321-329, 339-342,
// 400, 406-410).  On a 32 x 32 latent every one of them is a ~2 us kernel on the step's critical path, so the
// arithmetic is fused here: one launch forward, one backward, a few KB of traffic each.
//
//   d      = exp(a) + 1e-6 * [any(exp(a) < 1e-6)]                      (:321-323, batch-wide floor)
//   z      = mu + w * eps_w + sqrt(d) * eps_d                          (:325, LowRankMultivariateNormal.rsample)
//   kl     = 0.5 * ( -log(1 + sum w^2/d) - sum log d + sum d + sum w^2 + sum mu^2 - L )          (:400)
//   zcat   = [z, onehot(g)] for the G = C+1 decoder variants                                  (:326-329, 339-342)
#include "vg_common.h"

namespace {

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// wave per row, 4 rows per block; every block scans all of `a` for the batch-wide floor flag itself (B*L is ~1 K numbers:
// cheaper than a second launch or a grid-wide handshake)
__global__ void __launch_bounds__(256)
latent_fwd_k(const float* __restrict__ mu, const float* __restrict__ w, const float* __restrict__ a,
             const float* __restrict__ eps_w, const float* __restrict__ eps_d, int B, int L, int G,
             float* __restrict__ zcat, float* __restrict__ kl, float* __restrict__ d_out, float* __restrict__ flag_out) {
    __shared__ int s_flag;
    const int tid = threadIdx.x, lane = tid % VG_WAVE, wave = vg_wave_id(), nw = blockDim.x / VG_WAVE;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    int f = 0;
    for (int i = tid; i < B * L; i += blockDim.x) f |= (expf(a[i]) < 1e-6f) ? 1 : 0;
    if (f) s_flag = 1;                                   // benign race: every writer stores 1
    __syncthreads();
    const float floor_ = s_flag ? 1e-6f : 0.f;
    if (tid == 0 && blockIdx.x == 0) flag_out[0] = floor_;
    const int Z = L + G;
    for (int b = blockIdx.x * nw + wave; b < B; b += gridDim.x * nw) {
        float s_wd = 0.f, s_ld = 0.f, s_d = 0.f, s_w = 0.f, s_m = 0.f;
        const float ew = eps_w[b];
        for (int l = lane; l < L; l += VG_WAVE) {
            const int i = b * L + l;
            const float d = expf(a[i]) + floor_;
            const float m = mu[i], ww = w[i];
            const float z = m + ww * ew + sqrtf(d) * eps_d[i];
            d_out[i] = d;
            for (int g = 0; g < G; ++g) zcat[((size_t)g * B + b) * Z + l] = z;
            s_wd += ww * ww / d; s_ld += logf(d); s_d += d; s_w += ww * ww; s_m += m * m;
        }
        s_wd = wsum(s_wd); s_ld = wsum(s_ld); s_d = wsum(s_d); s_w = wsum(s_w); s_m = wsum(s_m);
        if (lane == 0) kl[b] = 0.5f * (-(logf(1.f + s_wd) + s_ld) + s_d + s_w + s_m - (float)L);
        for (int j = lane; j < G * G; j += VG_WAVE) {
            const int g = j / G, c = j % G;
            zcat[((size_t)g * B + b) * Z + L + c] = (g == c) ? 1.f : 0.f;
        }
    }
}

__global__ void __launch_bounds__(256)
latent_bwd_k(const float* __restrict__ mu, const float* __restrict__ w, const float* __restrict__ d_in,
             const float* __restrict__ flag, const float* __restrict__ eps_w, const float* __restrict__ eps_d,
             const float* __restrict__ g_zcat, const float* __restrict__ g_kl, int B, int L, int G,
             float* __restrict__ g_mu, float* __restrict__ g_w, float* __restrict__ g_a) {
    const int lane = threadIdx.x % VG_WAVE, wave = vg_wave_id(), nw = blockDim.x / VG_WAVE;
    const int Z = L + G;
    const float floor_ = flag[0];
    for (int b = blockIdx.x * nw + wave; b < B; b += gridDim.x * nw) {
        float s_wd = 0.f;
        for (int l = lane; l < L; l += VG_WAVE) { const int i = b * L + l; s_wd += w[i] * w[i] / d_in[i]; }
        const float cap = 1.f + wsum(s_wd);
        const float gk = g_kl ? g_kl[b] : 0.f, ew = eps_w[b];
        for (int l = lane; l < L; l += VG_WAVE) {
            const int i = b * L + l;
            float gz = 0.f;
            if (g_zcat) for (int g = 0; g < G; ++g) gz += g_zcat[((size_t)g * B + b) * Z + l];
            const float d = d_in[i], m = mu[i], ww = w[i];
            g_mu[i] = gz + gk * m;
            g_w[i] = gz * ew + gk * (ww - ww / (d * cap));
            const float gd = gz * eps_d[i] * 0.5f / sqrtf(d) + gk * 0.5f * (ww * ww / (d * d * cap) - 1.f / d + 1.f);
            g_a[i] = gd * (d - floor_);                  // d(d)/d(a) = exp(a)
        }
    }
}

// loss = coef0 * sum kl + coef1 * sum slp + coef2 * gp_kl + coef3 * sum dist          (:406-410)
__global__ void __launch_bounds__(256)
loss_fwd_k(const float* __restrict__ kl, const float* __restrict__ slp, const float* __restrict__ dist,
           const float* __restrict__ gp_kl, int B, int CB, float c0, float c1, float c2, float c3, float* __restrict__ loss) {
    __shared__ float red[3][4];
    const int tid = threadIdx.x, lane = tid % VG_WAVE, wave = vg_wave_id();
    float a = 0.f, b = 0.f, c = 0.f;
    for (int i = tid; i < B; i += blockDim.x) { a += kl[i]; b += slp[i]; }
    for (int i = tid; i < CB; i += blockDim.x) c += dist[i];
    a = wsum(a); b = wsum(b); c = wsum(c);
    if (lane == 0) { red[0][wave] = a; red[1][wave] = b; red[2][wave] = c; }
    __syncthreads();
    if (tid == 0) {
        float sa = 0.f, sb = 0.f, sc = 0.f;
        for (int k = 0; k < (int)(blockDim.x / VG_WAVE); ++k) { sa += red[0][k]; sb += red[1][k]; sc += red[2][k]; }
        loss[0] = c0 * sa + c1 * sb + c2 * gp_kl[0] + c3 * sc;
    }
}

__global__ void __launch_bounds__(256)
loss_bwd_k(const float* __restrict__ g, int B, int CB, float c0, float c1, float c2, float c3,
           float* __restrict__ g_kl, float* __restrict__ g_slp, float* __restrict__ g_dist, float* __restrict__ g_gp) {
    const float go = g[0];
    for (int i = threadIdx.x; i < B; i += blockDim.x) { g_kl[i] = go * c0; g_slp[i] = go * c1; }
    for (int i = threadIdx.x; i < CB; i += blockDim.x) g_dist[i] = go * c3;
    if (threadIdx.x == 0) g_gp[0] = go * c2;
}

}  // namespace

extern "C" int vg_latent_fwd(const float* mu, const float* w, const float* a, const float* eps_w, const float* eps_d,
                             int32_t B, int32_t L, int32_t G, float* zcat, float* kl, float* d_out, float* flag_out,
                             void* stream) {
    if (!mu || !w || !a || !eps_w || !eps_d || !zcat || !kl || !d_out || !flag_out) { vg_set_error("vg_latent_fwd: null argument"); return VG_ERR_ARG; }
    if (B <= 0 || L <= 0 || G <= 0 || (int64_t)B * L > (1 << 24)) { vg_set_error("vg_latent_fwd: bad shape"); return VG_ERR_ARG; }
    vg_launch(latent_fwd_k, dim3((B + 3) / 4 < 64 ? (B + 3) / 4 : 64), dim3(256), 0, (hipStream_t)stream, mu, w, a, eps_w, eps_d, (int)B, (int)L, (int)G, zcat, kl,
              d_out, flag_out);
    return vg_check_launch("latent_fwd");
}

extern "C" int vg_latent_bwd(const float* mu, const float* w, const float* d, const float* flag, const float* eps_w,
                             const float* eps_d, const float* g_zcat, const float* g_kl, int32_t B, int32_t L, int32_t G,
                             float* g_mu, float* g_w, float* g_a, void* stream) {
    if (!mu || !w || !d || !flag || !eps_w || !eps_d || !g_mu || !g_w || !g_a) { vg_set_error("vg_latent_bwd: null argument"); return VG_ERR_ARG; }
    if (B <= 0 || L <= 0 || G <= 0 || (int64_t)B * L > (1 << 24)) { vg_set_error("vg_latent_bwd: bad shape"); return VG_ERR_ARG; }
    vg_launch(latent_bwd_k, dim3((B + 3) / 4 < 64 ? (B + 3) / 4 : 64), dim3(256), 0, (hipStream_t)stream, mu, w, d, flag, eps_w, eps_d, g_zcat, g_kl, (int)B, (int)L,
              (int)G, g_mu, g_w, g_a);
    return vg_check_launch("latent_bwd");
}

extern "C" int vg_loss_fwd(const float* kl, const float* slp, const float* dist, const float* gp_kl, int32_t B, int32_t CB,
                           double c_kl, double c_slp, double c_gp, double c_dist, float* loss, void* stream) {
    if (!kl || !slp || (CB > 0 && !dist) || !gp_kl || !loss || B <= 0 || CB < 0) { vg_set_error("vg_loss_fwd: bad argument"); return VG_ERR_ARG; }
    vg_launch(loss_fwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, kl, slp, dist, gp_kl, (int)B, (int)CB, (float)c_kl,
              (float)c_slp, (float)c_gp, (float)c_dist, loss);
    return vg_check_launch("loss_fwd");
}

extern "C" int vg_loss_bwd(const float* g_loss, int32_t B, int32_t CB, double c_kl, double c_slp, double c_gp, double c_dist,
                           float* g_kl, float* g_slp, float* g_dist, float* g_gp, void* stream) {
    if (!g_loss || !g_kl || !g_slp || (CB > 0 && !g_dist) || !g_gp || B <= 0 || CB < 0) { vg_set_error("vg_loss_bwd: bad argument"); return VG_ERR_ARG; }
    vg_launch(loss_bwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, g_loss, (int)B, (int)CB, (float)c_kl, (float)c_slp,
              (float)c_gp, (float)c_dist, g_kl, g_slp, g_dist, g_gp);
    return vg_check_launch("loss_bwd");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Projection of the latent means (vae_reg_GP.py:542-583 project_latent: UMAP, n_neighbors 20, min_dist 0.1, Euclidean): the exact
// k-nearest-neighbour graph, the fuzzy simplicial set of each neighbour list and one synchronous SGD epoch of the 2-D layout.  The
// host side (graph union, spectral init, the epoch loop) is vae_gam_amd/latent_projection.py.  None of this runs in the train step.
#include <climits>
#include <math.h>
#include "../../include/vaegam.h"                       // VG_KNN_PLAN_LEN

namespace {

constexpr int KNN_Q = 256;      // queries per block, one per thread
constexpr int KNN_TC = 16;      // candidates per LDS tile
constexpr int KNN_DC = 16;      // dimensions per register chunk (D is zero-padded to a multiple of it; (0-0)^2 adds exactly 0)

// a (distance, index) pair as one unsigned 64-bit key: a distance is >= 0 (or +inf), so its bit pattern orders like its value, and
// ordering the keys orders by distance, then by index
__device__ __forceinline__ uint64_t knn_key(float d, int j) {
    union { float f; uint32_t u; } t; t.f = d;
    return ((uint64_t)t.u << 32) | (uint32_t)j;
}
__device__ __forceinline__ float knn_key_dist(uint64_t k) { union { float f; uint32_t u; } t; t.u = (uint32_t)(k >> 32); return t.f; }
__device__ __forceinline__ int knn_key_idx(uint64_t k) { return (int)(uint32_t)k; }
constexpr uint64_t KNN_NONE = ~0ull;

// sorted key list in registers, insertion by shifting the larger entries down one place: every index is a compile-time constant
// (nothing goes to scratch).  The branch is taken by the whole wave when any lane inserts and the chain inside is branchless.
// Call from wave-uniform control flow only.
template <int KB>
__device__ __forceinline__ void knn_insert(uint64_t (&kl)[KB], uint64_t key, bool valid) {
    bool go = valid && key < kl[KB - 1];                 // key belongs at or above position m
    if (!vg_any(go)) return;
#pragma unroll
    for (int m = KB - 1; m > 0; --m) {
        const bool up = go && key < kl[m - 1];
        kl[m] = up ? kl[m - 1] : (go ? key : kl[m]);
        go = up;
    }
    kl[0] = go ? key : kl[0];
}

// block (query tile, candidate split): the K1 = k-1 nearest OTHER points of each query among candidates [c0, c1), written to
// ws_d / ws_i [split][K1][N] (unfilled entries: distance NaN-bits, index -1, never inserted by the merge).  Candidate tiles of KNN_TC x Dp floats are staged in LDS and read
// as broadcasts; a query accumulates sum (q-c)^2 over d = 0..D-1 in that order for KNN_TC candidates at a time.
template <int KB>
__global__ void __launch_bounds__(256)
knn_partial_k(const float* __restrict__ x, int N, int D, int Dp, int K1, int chunk, float* __restrict__ ws_d, int* __restrict__ ws_i) {
    VG_DYN_SMEM(float, tile);                            // [KNN_TC][Dp] candidates, then [KNN_TC][KNN_Q] this tile's distances
    const int tid = threadIdx.x, q = blockIdx.x * KNN_Q + tid, split = blockIdx.y;
    float* tdist = tile + KNN_TC * Dp;                   // each thread reads back only what it wrote: no barrier needed
    const int c0 = split * chunk, c1 = min(N, c0 + chunk);
    uint64_t kl[KB];
#pragma unroll
    for (int m = 0; m < KB; ++m) kl[m] = KNN_NONE;
    const float* xq = x + (size_t)min(q, N - 1) * D;
    for (int t0 = c0; t0 < c1; t0 += KNN_TC) {
        __syncthreads();
        for (int e = tid; e < KNN_TC * Dp; e += blockDim.x) {
            const int c = e / Dp, d = e - c * Dp, j = t0 + c;
            tile[e] = (j < c1 && d < D) ? x[(size_t)j * D + d] : 0.f;
        }
        __syncthreads();
        float acc[KNN_TC];
#pragma unroll
        for (int c = 0; c < KNN_TC; ++c) acc[c] = 0.f;
        for (int d0 = 0; d0 < Dp; d0 += KNN_DC) {
            float qv[KNN_DC];
#pragma unroll
            for (int d = 0; d < KNN_DC; ++d) qv[d] = (d0 + d < D) ? xq[d0 + d] : 0.f;
#pragma unroll
            for (int c = 0; c < KNN_TC; ++c) {
                const float* row = tile + c * Dp + d0;
#pragma unroll
                for (int d = 0; d < KNN_DC; d += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(row + d);
                    float t;
                    t = qv[d] - v.x; acc[c] = fmaf(t, t, acc[c]);
                    t = qv[d + 1] - v.y; acc[c] = fmaf(t, t, acc[c]);
                    t = qv[d + 2] - v.z; acc[c] = fmaf(t, t, acc[c]);
                    t = qv[d + 3] - v.w; acc[c] = fmaf(t, t, acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KNN_TC; ++c) tdist[c * KNN_Q + tid] = sqrtf(acc[c]);
#pragma unroll 1
        for (int c = 0; c < KNN_TC; ++c) {             // one copy of the insertion code, not KNN_TC
            const int j = t0 + c;
            knn_insert(kl, knn_key(tdist[c * KNN_Q + tid], j), j < c1 && j != q);
        }
    }
    if (q >= N) return;
#pragma unroll
    for (int m = 0; m < KB; ++m)
        if (m < K1) { const size_t o = ((size_t)split * K1 + m) * N + q; ws_d[o] = knn_key_dist(kl[m]); ws_i[o] = knn_key_idx(kl[m]); }
}

// merge the S partial lists of each query; position 0 is the query itself at distance 0
template <int KB>
__global__ void __launch_bounds__(256)
knn_merge_k(const float* __restrict__ ws_d, const int* __restrict__ ws_i, int N, int K1, int S, int32_t* __restrict__ idx,
            float* __restrict__ dist) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t kl[KB];
#pragma unroll
    for (int m = 0; m < KB; ++m) kl[m] = KNN_NONE;
#pragma unroll 1
    for (int s = 0; s < S; ++s)
#pragma unroll 1
        for (int m = 0; m < K1; ++m) { const size_t o = ((size_t)s * K1 + m) * N + min(q, N - 1); knn_insert(kl, knn_key(ws_d[o], ws_i[o]), q < N); }
    if (q >= N) return;
    const size_t r = (size_t)q * (K1 + 1);
    idx[r] = q; dist[r] = 0.f;
#pragma unroll
    for (int m = 0; m < KB; ++m)
        if (m < K1) { idx[r + 1 + m] = knn_key_idx(kl[m]); dist[r + 1 + m] = knn_key_dist(kl[m]); }
}

// candidate splits: enough blocks to fill the CUs at large N (~2048), at least 128 candidates per split, at most 16 splits
void knn_splits(int N, int* S, int* chunk) {
    const int qt = vg_cdiv(N, KNN_Q);
    int s = min(vg_cdiv(2048, qt), N / 128);
    s = s < 1 ? 1 : (s > 16 ? 16 : s);
    *chunk = vg_cdiv(vg_cdiv(N, s), KNN_TC) * KNN_TC;
    *S = vg_cdiv(N, *chunk);
}

// every launch decision of vg_knn, in the order vg_knn_plan reports it; vg_knn_ws_bytes sizes the workspace from the same record
struct KnnPlan { int KB, S, chunk, Dp, qblocks, last, lds; };

bool knn_shape_ok(int N, int D, int k) { return N > 0 && D >= 1 && D <= 128 && k >= 1 && k <= 64 && k <= N; }

KnnPlan knn_plan(int N, int D, int k) {
    KnnPlan p;
    const int K1 = k - 1;
    p.KB = K1 == 0 ? 0 : (K1 <= 8 ? 8 : (K1 <= 16 ? 16 : (K1 <= 32 ? 32 : 64)));
    knn_splits(N, &p.S, &p.chunk);
    p.Dp = vg_cdiv(D, KNN_DC) * KNN_DC;
    p.qblocks = vg_cdiv(N, KNN_Q);
    p.last = N - (p.S - 1) * p.chunk;
    p.lds = p.KB ? KNN_TC * (p.Dp + KNN_Q) * (int)sizeof(float) : 0;
    return p;
}

template <int KB>
void knn_launch(const float* x, int N, int D, int K1, float* ws_d, int* ws_i, const KnnPlan& p, int32_t* idx, float* dist, hipStream_t s) {
    if (p.KB)
        vg_launch(knn_partial_k<KB>, dim3(p.qblocks, p.S), dim3(KNN_Q), (size_t)p.lds, s, x, N, D, p.Dp, K1, p.chunk, ws_d, ws_i);
    vg_launch(knn_merge_k<KB>, dim3(p.qblocks), dim3(KNN_Q), 0, s, (const float*)ws_d, (const int*)ws_i, N, K1, p.S, idx, dist);
}

constexpr int FZ_PARTS = 256;   // blocks of the fixed-order global mean

// partial sums of all N*k distances over FZ_PARTS contiguous segments, each a fixed-order tree: deterministic
__global__ void __launch_bounds__(256)
umap_mean_part_k(const float* __restrict__ dist, int64_t n, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t seg = (n + FZ_PARTS - 1) / FZ_PARTS, b0 = blockIdx.x * seg, b1 = min(n, b0 + seg);
    double s = 0.0;
    for (int64_t i = b0 + tid; i < b1; i += blockDim.x) s += (double)dist[i];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

// rho, sigma (binary search to |psum - log2 k| < 1e-5) and memberships of one neighbour row per thread, in fp64
// (local_connectivity = 1, bandwidth = 1: umap-learn's smooth_knn_dist + compute_membership_strengths)
__global__ void __launch_bounds__(256)
umap_fuzzy_k(const float* __restrict__ dist, const int32_t* __restrict__ idx, int N, int k, const double* __restrict__ part,
             float* __restrict__ rho, float* __restrict__ sigma, float* __restrict__ w) {
    __shared__ double red[FZ_PARTS];
    const int tid = threadIdx.x;
    red[tid] = part[tid];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double mean_all = red[0] / ((double)N * k);
    const int i = blockIdx.x * blockDim.x + tid;
    if (i >= N) return;
    const float* di = dist + (size_t)i * k;
    double r = 0.0, rowsum = 0.0;
    for (int j = 0; j < k; ++j) {
        const double d = di[j];
        rowsum += d;
        if (d > 0.0 && (r == 0.0 || d < r)) r = d;
    }
    const double target = log2((double)k);
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int it = 0; it < 64; ++it) {
        double psum = 0.0;
        for (int j = 1; j < k; ++j) {
            const double d = (double)di[j] - r;
            psum += d > 0.0 ? exp(-(d / mid)) : 1.0;
        }
        if (fabs(psum - target) < 1e-5) break;
        if (psum > target) { hi = mid; mid = (lo + hi) / 2.0; }
        else { lo = mid; mid = (hi == INFINITY) ? mid * 2.0 : (lo + hi) / 2.0; }
    }
    const double floor_ = 1e-3 * (r > 0.0 ? rowsum / k : mean_all);
    if (mid < floor_) mid = floor_;
    rho[i] = (float)r; sigma[i] = (float)mid;
    const int32_t* ii = idx + (size_t)i * k;
    for (int j = 0; j < k; ++j) {
        const double d = (double)di[j] - r;
        w[(size_t)i * k + j] = ii[j] == i ? 0.f : ((d <= 0.0 || mid == 0.0) ? 1.f : (float)exp(-(d / mid)));
    }
}

__device__ __forceinline__ uint64_t vg_splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ float clip4(float v) { return v > 4.f ? 4.f : (v < -4.f ? -4.f : v); }

// one synchronous epoch: thread i walks row i of the symmetric CSR graph, reads Y_n only and writes its own row of Y_{n+1}.  Every
// contribution is added to y_i in CSR order, then sample order (no fused multiply-adds: the order and rounding are the documented ones).
__global__ void __launch_bounds__(256)
umap_layout_k(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ eps,
              const float* __restrict__ yin, int N, int n, int n_epochs, float a, float b, int neg, uint64_t seed,
              float* __restrict__ yout) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float alpha = 1.f - (float)n / (float)n_epochs;
    const float yx = yin[2 * i], yy = yin[2 * i + 1];
    float ox = yx, oy = yy;
    const float two_ab = -2.f * a * b, bm1 = b - 1.f, two_b = 2.f * b;
    const uint64_t sk = seed * 0x9E3779B97F4A7C15ull;
    if (n >= 1) {
        const int e1 = rowptr[i + 1];
        for (int e = rowptr[i]; e < e1; ++e) {
            const double ep = eps[e];
            if (!(floor((double)n / ep) > floor((double)(n - 1) / ep))) continue;
            const int j = col[e];
            float dx = yx - yin[2 * j], dy = yy - yin[2 * j + 1];
            float d2 = dx * dx + dy * dy;
            if (d2 > 0.f) {
                const float coef = (two_ab * powf(d2, bm1)) / (a * powf(d2, b) + 1.f);
                const float gx = alpha * clip4(coef * dx), gy = alpha * clip4(coef * dy);
                ox = ox + gx; oy = oy + gy;              // as head of (i, j)
                ox = ox + gx; oy = oy + gy;              // as the other end of (j, i)
            }
            const uint64_t key = ((uint64_t)n << 44) | ((uint64_t)e << 5);
            for (int s = 0; s < neg; ++s) {
                const int kk = (int)(vg_splitmix64((key | (uint64_t)s) + sk) % (uint64_t)N);
                if (kk == i) continue;
                dx = yx - yin[2 * kk]; dy = yy - yin[2 * kk + 1];
                d2 = dx * dx + dy * dy;
                if (!(d2 > 0.f)) continue;
                const float coef = two_b / ((0.001f + d2) * (a * powf(d2, b) + 1.f));
                ox = ox + alpha * clip4(coef * dx); oy = oy + alpha * clip4(coef * dy);
            }
        }
    }
    yout[2 * i] = ox; yout[2 * i + 1] = oy;
}

}  // namespace

extern "C" int64_t vg_knn_ws_bytes(int32_t N, int32_t D, int32_t k) {
    if (!knn_shape_ok(N, D, k)) { vg_set_error("vg_knn_ws_bytes: bad shape (N %d, D %d, k %d)", N, D, k); return -1; }
    return (int64_t)knn_plan(N, D, k).S * (k - 1) * N * 8;
}

extern "C" int vg_knn_plan(int32_t N, int32_t D, int32_t k, int32_t* out, int32_t n_out) {
    if (!out || n_out < VG_KNN_PLAN_LEN) { vg_set_error("vg_knn_plan: out must hold %d values", VG_KNN_PLAN_LEN); return VG_ERR_ARG; }
    if (!knn_shape_ok(N, D, k)) { vg_set_error("vg_knn_plan: bad shape (N %d, D %d, k %d)", N, D, k); return VG_ERR_ARG; }
    const KnnPlan p = knn_plan(N, D, k);
    const int v[VG_KNN_PLAN_LEN] = {p.KB, p.S, p.chunk, p.Dp, p.qblocks, p.last, p.lds};
    for (int i = 0; i < VG_KNN_PLAN_LEN; ++i) out[i] = v[i];
    return VG_OK;
}

extern "C" int vg_knn(const float* x, int32_t N, int32_t D, int32_t k, void* ws, int32_t* idx, float* dist, void* stream) {
    if (!x || !idx || !dist || (k > 1 && !ws)) { vg_set_error("vg_knn: null argument"); return VG_ERR_ARG; }
    if (!knn_shape_ok(N, D, k) || (int64_t)N * k > INT_MAX) { vg_set_error("vg_knn: bad shape (N %d, D %d, k %d)", N, D, k); return VG_ERR_ARG; }
    const KnnPlan p = knn_plan(N, D, k);
    const int K1 = k - 1;
    float* ws_d = (float*)ws;
    int* ws_i = ws ? (int*)((char*)ws + (size_t)p.S * K1 * N * 4) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (p.KB <= 8) knn_launch<8>(x, N, D, K1, ws_d, ws_i, p, idx, dist, s);      // KB = 0 (k = 1): the merge alone, position 0
    else if (p.KB == 16) knn_launch<16>(x, N, D, K1, ws_d, ws_i, p, idx, dist, s);
    else if (p.KB == 32) knn_launch<32>(x, N, D, K1, ws_d, ws_i, p, idx, dist, s);
    else knn_launch<64>(x, N, D, K1, ws_d, ws_i, p, idx, dist, s);
    return vg_check_launch("knn");
}

extern "C" int vg_umap_fuzzy(const float* dist, const int32_t* idx, int32_t N, int32_t k, double* ws, float* rho, float* sigma,
                             float* w, void* stream) {
    if (!dist || !idx || !ws || !rho || !sigma || !w) { vg_set_error("vg_umap_fuzzy: null argument"); return VG_ERR_ARG; }
    if (N <= 0 || k < 1 || k > 64 || (int64_t)N * k > INT_MAX) { vg_set_error("vg_umap_fuzzy: bad shape (N %d, k %d)", N, k); return VG_ERR_ARG; }
    vg_launch(umap_mean_part_k, dim3(FZ_PARTS), dim3(256), 0, (hipStream_t)stream, dist, (int64_t)N * k, ws);
    vg_launch(umap_fuzzy_k, dim3(vg_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, dist, idx, (int)N, (int)k, (const double*)ws,
              rho, sigma, w);
    return vg_check_launch("umap_fuzzy");
}

extern "C" int vg_umap_layout_epoch(const int32_t* rowptr, const int32_t* col, const float* eps, const float* y_in, int32_t N,
                                    int32_t nnz, int32_t epoch, int32_t n_epochs, double a, double b, int32_t negative_sample_rate,
                                    uint64_t seed, float* y_out, void* stream) {
    if (!rowptr || !y_in || !y_out || (nnz > 0 && (!col || !eps)) || y_in == y_out) { vg_set_error("vg_umap_layout_epoch: bad pointer argument"); return VG_ERR_ARG; }
    if (N <= 0 || nnz < 0 || (int64_t)nnz >= ((int64_t)1 << 39) || n_epochs < 1 || n_epochs >= (1 << 20) || epoch < 0 || epoch >= n_epochs ||
        negative_sample_rate < 0 || negative_sample_rate > 31) {
        vg_set_error("vg_umap_layout_epoch: bad argument (N %d, nnz %d, epoch %d of %d, negative_sample_rate %d)", N, nnz, epoch, n_epochs,
                     negative_sample_rate);
        return VG_ERR_ARG;
    }
    vg_launch(umap_layout_k, dim3(vg_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, eps, y_in, (int)N, (int)epoch,
              (int)n_epochs, (float)a, (float)b, (int)negative_sample_rate, seed, y_out);
    return vg_check_launch("umap_layout_epoch");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Device-resident input path (an extension; include/vaegam.h: vg_volume_gather): the minibatch x[B][X][Y][Z] assembled in one launch
// from the raw payloads of the subject files, kept in HBM as they sit on disk.  Not part of the captured step: it fills the tensor the
// step's graph copies in.
//
// A workgroup owns the slab (all x, TY consecutive y, all z) of one volume.  NIfTI is x-fastest, the output z-fastest; for a fixed z the
// source of the slab is one contiguous run over (x, y) and for a fixed x its destination is one contiguous run over (y, z), so staging
// the converted slab in LDS makes both the loads and the stores of a wavefront contiguous.  LDS element (x, q = yy*Z + z) sits at
// q*P + x with P odd: the store phase reads it with consecutive lanes on consecutive q -- a stride of P words, conflict-free -- and the
// load phase writes runs of consecutive x.  Files that are not x-fastest (a C-order .npy has t, then z fastest) gain nothing from the
// transposition and are read in output order, as are shapes whose slab does not fit in LDS even at TY = 1.
#include "../../include/vaegam.h"

namespace {

constexpr int VOLG_LDS_BYTES = 32 * 1024;   // slab budget: 5 workgroups per CU
constexpr int VOLG_TY_MAX = 8;

__host__ __device__ static inline int volg_esize(int dt) {
    return (dt == 2 || dt == 256) ? 1 : (dt == 4 || dt == 512) ? 2 : dt == 64 ? 8 : 4;
}

// one stored element -> the fp32 value the host path computes for it (the arithmetic contract of include/vaegam.h).  DT: the dtype code
// when the whole table shares one (the switch folds away), 0: the descriptor's.
template <int DT>
__device__ __forceinline__ float volg_value(const unsigned char* p, int dt_file, int swap, int scale, double slope, double inter, double divisor) {
#pragma clang fp contract(off)
    const int dt = DT ? DT : dt_file;
    if (dt == 16) {
        union { uint32_t u; float f; } t;
        t.u = *reinterpret_cast<const uint32_t*>(p);
        if (swap) t.u = __builtin_bswap32(t.u);
        float v = t.f;
        if (scale) { v = v * (float)slope; v = v + (float)inter; }
        return v / (float)divisor;
    }
    double v;
    switch (dt) {
        case 2: v = (double)*p; break;
        case 256: v = (double)*reinterpret_cast<const int8_t*>(p); break;
        case 4: case 512: {
            uint16_t u = *reinterpret_cast<const uint16_t*>(p);
            if (swap) u = __builtin_bswap16(u);
            v = dt == 4 ? (double)(int16_t)u : (double)u;
        } break;
        case 8: case 768: {
            uint32_t u = *reinterpret_cast<const uint32_t*>(p);
            if (swap) u = __builtin_bswap32(u);
            v = dt == 8 ? (double)(int32_t)u : (double)u;
        } break;
        default: {                                       // 64
            union { uint64_t u; double f; } t;
            t.u = *reinterpret_cast<const uint64_t*>(p);
            if (swap) t.u = __builtin_bswap64(t.u);
            v = t.f;
        } break;
    }
    if (scale) { v = v * slope; v = v + inter; }
    return (float)(v / divisor);
}

// block = (volume b, y tile): ntile = ceil(Y / TY) tiles per volume.  P: LDS pitch (odd, >= X), 0 = no LDS slab (read in output order).
template <int DT>
__global__ void __launch_bounds__(256)
volume_gather_k(const unsigned char* __restrict__ arena, const vg_vol_file* __restrict__ files, const int32_t* __restrict__ row_file,
                const int32_t* __restrict__ row_vol, const int64_t* __restrict__ idx, int X, int Y, int Z, int TY, int P, int ntile,
                double divisor, float* __restrict__ out) {
    VG_DYN_SMEM(float, tile);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int b = blockIdx.x / ntile, y0 = (blockIdx.x - b * ntile) * TY, ty = min(TY, Y - y0);
    const int64_t row = idx[b];
    const vg_vol_file f = files[row_file[row]];
    const int64_t es = volg_esize(DT ? DT : f.dtype);
    const unsigned char* src = arena + f.offset + ((int64_t)row_vol[row] * f.st + (int64_t)y0 * f.sy) * es;
    float* dst = out + ((size_t)b * X * Y + y0) * Z;     // element (x, yy, z) of the slab: dst[x*Y*Z + yy*Z + z]
    const int nq = ty * Z, n = X * nq;
    const size_t YZ = (size_t)Y * Z;
    if (P > 0 && f.sx < f.sz) {
        const int nr = ty * X;                           // for a fixed z: (yy, x) is one run of the file when sy = X*sx
#pragma unroll 4
        for (int e = tid; e < n; e += nt) {
            const int z = e / nr, r = e - z * nr, yy = r / X, xx = r - yy * X;
            tile[(yy * Z + z) * P + xx] = volg_value<DT>(src + (xx * f.sx + yy * f.sy + z * f.sz) * es, f.dtype, f.swap, f.scale, f.slope,
                                                         f.inter, divisor);
        }
        __syncthreads();
        for (int e = tid; e < n; e += nt) {
            const int xx = e / nq, q = e - xx * nq;
            dst[xx * YZ + q] = tile[q * P + xx];
        }
    } else {
#pragma unroll 4
        for (int e = tid; e < n; e += nt) {
            const int xx = e / nq, q = e - xx * nq, yy = q / Z, z = q - yy * Z;
            dst[xx * YZ + q] = volg_value<DT>(src + (xx * f.sx + yy * f.sy + z * f.sz) * es, f.dtype, f.swap, f.scale, f.slope, f.inter,
                                              divisor);
        }
    }
}

template <int DT>
void volg_launch(int grid, size_t shmem, hipStream_t s, const void* arena, const vg_vol_file* files, const int32_t* row_file,
                 const int32_t* row_vol, const int64_t* idx, int X, int Y, int Z, int TY, int P, int ntile, double divisor, float* x) {
    vg_launch(volume_gather_k<DT>, dim3(grid), dim3(256), shmem, s, (const unsigned char*)arena, files, row_file, row_vol, idx, X, Y, Z,
              TY, P, ntile, divisor, x);
}

}  // namespace

extern "C" int vg_volume_gather(const void* arena, const vg_vol_file* files, const int32_t* row_file, const int32_t* row_vol,
                                const int64_t* idx, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t dtype, double divisor, float* x,
                                void* stream) {
    if (!arena || !files || !row_file || !row_vol || !idx || !x) { vg_set_error("vg_volume_gather: null argument"); return VG_ERR_ARG; }
    if (B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || (int64_t)X * Z > (1 << 27) || !(divisor != 0.0)) {
        vg_set_error("vg_volume_gather: bad argument (B %d, volume %d x %d x %d, divisor %g)", B, X, Y, Z, divisor);
        return VG_ERR_ARG;
    }
    int P = X | 1;                                       // odd pitch
    const int64_t per_y = (int64_t)Z * P * (int64_t)sizeof(float);
    int TY = (int)(VOLG_LDS_BYTES / per_y);
    if (TY < 1) P = 0;                                   // not even one y fits: no slab
    if (TY < 1 || TY > VOLG_TY_MAX) TY = VOLG_TY_MAX;
    if (TY > Y) TY = Y;
    const int ntile = vg_cdiv(Y, TY);
    if ((int64_t)ntile * B > INT_MAX) { vg_set_error("vg_volume_gather: B %d x %d tiles exceeds the grid", B, ntile); return VG_ERR_ARG; }
    const int grid = ntile * B;
    const size_t shmem = (size_t)TY * Z * P * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
#define VOLG_CASE(DT) case DT: volg_launch<DT>(grid, shmem, s, arena, files, row_file, row_vol, idx, X, Y, Z, TY, P, ntile, divisor, x); break
    switch (dtype) {
        VOLG_CASE(0); VOLG_CASE(2); VOLG_CASE(4); VOLG_CASE(8); VOLG_CASE(16); VOLG_CASE(64); VOLG_CASE(256); VOLG_CASE(512); VOLG_CASE(768);
        default: vg_set_error("vg_volume_gather: unknown dtype code %d", dtype); return VG_ERR_ARG;
    }
#undef VOLG_CASE
    return vg_check_launch("volume_gather");
}
