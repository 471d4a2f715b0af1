// vg_gp.hip -- the per-covariate gain block of the VAE-GAM (gfx950): sparse variational GP posterior, gain covariance,
// B x B Cholesky, reparameterised gain sample, HRF along the batch axis, both KL terms -- forward and hand-derived
// backward, ONE workgroup per covariate, float64 -- up to B = 1024.  Batches of 1025..4096 take the TILED path further down (the same
// arithmetic on at least C * ceil(B / 64) workgroups per O(B^2) / O(B^3) launch); vg_gp_gain_*_tiled take it at any B.
//
// Replaces, per covariate i (vae_reg_GP.py:345-378 with gp.py:41-110), what the reference does as two Python loops over the
// minibatch with a float() host sync per query point, an fp32 torch.inverse, a MultivariateNormal constructor (Cholesky) and
// an rsample -- and what round 1 of this build did as ~300 batched ATen launches:
//   std = exp(logstd);  kl_lin = KL(N(sa, std^2) || N(1, 0.5^2))                                    (:266-281, :346-348)
//   beta_mean = sa x,  beta_cov = diag(std^2 x^2)                                                   (:349-351)
//   continuous covariates:  kvar = exp(logkvar) + 0.1,  ls = 3 sigmoid(exp(log_ls) + 0.5)           (:355-357)
//       Knu[k][b] = k((Xu0 - x_b) + k step)  (distance rounded to fp32 as gp.py:90),  Knn[i][j] = k(x_j - x_i),
//       Ku[a][b] = k(|a-b| step),  k(d) = exp(-(d / (sqrt2 ls))^2)  (unit variance: it cancels in A)  (gp.py:88-105, 121-136)
//       A = Knu^T Ku^-1,  f = A m,  Sigma = kvar Knn + A (S - kvar Ku) A^T                          (gp.py:107-109)
//       beta_mean += f,  beta_cov += Sigma,  kl_gp = KL(N(m, S) || N(0, 10 I)) via chol(S)          (:363-367, gp.py:41-65)
//   L = chol(beta_cov + 1e-5 I),  gain = beta_mean + L eps                                          (:368-369)
//   neural covariates:  gain <- causal 15-tap HRF convolution of gain along the BATCH index         (:283-305, :377-378)
// Everything is evaluated in float64 (parameters, covariates and noise are fp32 values widened on load): the gain covariance
// is within 1e-5 of singular and the reference's own fp32 gradients through this block are rounding noise.
// Ku^-1 comes from a Cholesky factorisation of Ku + jitter_ku I (jitter_ku = 0 reproduces the reference's inverse; > 0 is the
// remedy for dense inducing grids where Ku is singular in any precision).
//
// Memory: tiny batches (B <= 16) keep the B x B matrix in LDS in one 256-thread workgroup; everything else -- the bench batch of 64
// and the data-parallel global minibatches (256, 512: dp_gain='global') -- takes a second path through the same arithmetic with the
// matrix in the caller's workspace (L2-resident) (round 2 ran every size through the small-batch code: one 256-thread workgroup walking B unblocked columns with the matrix in L2 --
// 14 + 40 ms at B = 512): 1024-thread workgroups, a BLOCKED Cholesky whose 16-column panel lives in LDS (the trailing update reads
// its operands from LDS and touches every matrix element once per panel), and a backward whose two triangular solves L^-T Phi L^-1
// run as column slabs of the right-hand side on several workgroups per covariate (the columns of a triangular solve are independent).  Every other array (B x n, n x n, vectors) is in the
// workspace.  Parameter gradients are ADDED straight into the flat fp32 gradient buffer at the parameters' own offsets.
#include "vg_common.h"
#include "../../include/vaegam.h"

namespace {

constexpr int GP_T = 256;                  // threads per workgroup (B <= GP_LDS_MAXB)
constexpr int GP_TB = 1024;                // threads per workgroup of the large-batch path
constexpr int GP_LDS_MAXB = 16;            // up to here the one-workgroup path with the B x B matrix in LDS; beyond it the blocked / slab path, which
                                           // measured faster from B = 32 on (B = 64: 0.74 -> 0.51 ms forward + backward, 128: 2.6 -> 0.52, 512: 54 -> 3.7)
constexpr int GP_NB = 16;                  // panel width of the blocked factorisation / block rows of the blocked solves
constexpr int GP_NBP = GP_NB + 1;          // LDS row pitch of a panel in doubles: odd, so that the rows a wavefront's lanes read fall into different banks
constexpr int TAB_W = 10;                  // table row: {is_gp, is_hrf, gp_index, off_sa, off_logstd, off_qu_m, off_qu_S, off_logkvar, off_log_ls, 0}

struct GpLayout {                          // workspace of ONE covariate, in doubles
    long long Lc, A, kinv, Ls, M, N1, N2, N3, N4, T1, T2, T3, G, x, e, bm, v1, v2, v3, sc, total;
};

__host__ __device__ inline GpLayout gp_layout(long long B, long long n) {
    GpLayout w; long long o = 0;
    w.Lc = o; o += B * B;                  // chol(beta_cov + jitter)            saved for the backward pass
    w.A = o; o += B * n;                   // A = Knu^T Ku^-1                    saved
    w.kinv = o; o += n * n;                // (Ku + jitter)^-1                   saved
    w.Ls = o; o += n * n;                  // chol(S)                            saved
    w.M = o; o += n * n;                   // S - kvar Ku
    w.N1 = o; o += n * n; w.N2 = o; o += n * n; w.N3 = o; o += n * n; w.N4 = o; o += n * n;     // n x n scratch
    w.T1 = o; o += B * n; w.T2 = o; o += B * n; w.T3 = o; o += B * n;
    w.G = o; o += B * B;                   // backward: d loss / d beta_cov (when it does not fit LDS)
    w.x = o; o += B; w.e = o; o += B; w.bm = o; o += B; w.v1 = o; o += B; w.v2 = o; o += B; w.v3 = o; o += B;
    w.sc = o; o += 16;
    w.total = (o + 7) / 8 * 8;
    return w;
}

// ---- block-cooperative dense helpers (all threads of the workgroup call them; `m` may point to LDS or global memory)

// in-place right-looking Cholesky of the lower triangle of m (n x n, row-major); the upper triangle is zeroed
__device__ void chol_inplace(double* m, int n) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int j = 0; j < n; ++j) {
        __syncthreads();
        const double d = sqrt(m[j * n + j]);           // NaN for a non-positive pivot, as cholesky_ex(check_errors=False)
        __syncthreads();
        for (int i = j + tid; i < n; i += nt) m[i * n + j] = (i == j) ? d : m[i * n + j] / d;
        __syncthreads();
        const int r = n - j - 1;
        for (long long t = tid; t < (long long)r * r; t += nt) {
            const int i = j + 1 + (int)(t / r), k = j + 1 + (int)(t % r);
            if (k <= i) m[i * n + k] -= m[i * n + j] * m[k * n + j];
        }
    }
    __syncthreads();
    for (long long t = tid; t < (long long)n * n; t += nt) { const int i = (int)(t / n), k = (int)(t % n); if (k > i) m[t] = 0.0; }
    __syncthreads();
}

// X <- L^-T X in place (L lower triangular n x n, X n x nc row-major with leading dimension ldx): right-looking back substitution
__device__ void solve_LT_inplace(const double* L, int n, double* X, int nc, int ldx) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = n - 1; i >= 0; --i) {
        __syncthreads();
        const double inv = 1.0 / L[i * n + i];
        for (int c = tid; c < nc; c += nt) X[(long long)i * ldx + c] *= inv;
        __syncthreads();
        for (long long t = tid; t < (long long)i * nc; t += nt) {
            const int r = (int)(t / nc), c = (int)(t % nc);
            X[(long long)r * ldx + c] -= L[i * n + r] * X[(long long)i * ldx + c];
        }
    }
    __syncthreads();
}

// In-place BLOCKED right-looking Cholesky of the lower triangle of m (n x n, row-major, in global memory / L2); the upper triangle is
// zeroed.  pan: n * GP_NBP doubles of LDS.  Per panel of GP_NB columns: the panel (all rows from its diagonal block down) is copied to
// LDS and factorised there by the unblocked recurrence (a thread per row, two barriers per column), written back, and the trailing
// matrix is updated from the LDS copy -- a thread owns 4 x 4 blocks of it: 32 panel values from LDS, 16 elements of m read and
// written once per panel, 256 fused multiply-adds.
__device__ void chol_blocked(double* m, int n, double* pan) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int k0 = 0; k0 < n; k0 += GP_NB) {
        const int nb = min(GP_NB, n - k0), r = n - k0;
        __syncthreads();
        for (int t = tid; t < r * GP_NB; t += nt) {
            const int i = t / GP_NB, j = t % GP_NB;
            pan[i * GP_NBP + j] = (j < nb) ? m[(long long)(k0 + i) * n + k0 + j] : 0.0;
        }
        for (int j = 0; j < nb; ++j) {
            __syncthreads();
            const double d = sqrt(pan[j * GP_NBP + j]);     // NaN for a non-positive pivot, as cholesky_ex(check_errors=False)
            __syncthreads();
            for (int i = j + tid; i < r; i += nt) pan[i * GP_NBP + j] = (i == j) ? d : pan[i * GP_NBP + j] / d;
            __syncthreads();
            for (int i = j + 1 + tid; i < r; i += nt) {
                const double lij = pan[i * GP_NBP + j];
                const int tmax = min(i, nb - 1);
                for (int t = j + 1; t <= tmax; ++t) pan[i * GP_NBP + t] -= lij * pan[t * GP_NBP + j];
            }
        }
        __syncthreads();
        for (int t = tid; t < r * nb; t += nt) {
            const int i = t / nb, j = t % nb;
            m[(long long)(k0 + i) * n + k0 + j] = pan[i * GP_NBP + j];
        }
        // trailing update: m[i][j] -= sum_t pan[i][t] pan[j][t] for k0+nb <= j <= i < n, in 4 x 4 blocks (bj <= bi)
        const int r2 = r - nb;
        if (r2 > 0) {
            const double* P = pan + nb * GP_NBP;                // panel rows below the diagonal block
            const int nblk = (r2 + 3) / 4;
            const long long ntile = (long long)nblk * (nblk + 1) / 2;
            for (long long t = tid; t < ntile; t += nt) {
                // t -> (bi, bj), bj <= bi: row bi holds bi + 1 tiles
                int bi = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
                while ((long long)(bi + 1) * (bi + 2) / 2 <= t) ++bi;
                while ((long long)bi * (bi + 1) / 2 > t) --bi;
                const int bj = (int)(t - (long long)bi * (bi + 1) / 2);
                double acc[4][4];
#pragma unroll
                for (int a_ = 0; a_ < 4; ++a_)
#pragma unroll
                    for (int b_ = 0; b_ < 4; ++b_) acc[a_][b_] = 0.0;
                for (int q = 0; q < nb; ++q) {
                    double pi[4], pj[4];
#pragma unroll
                    for (int a_ = 0; a_ < 4; ++a_) {
                        pi[a_] = P[min(bi * 4 + a_, r2 - 1) * GP_NBP + q];
                        pj[a_] = P[min(bj * 4 + a_, r2 - 1) * GP_NBP + q];
                    }
#pragma unroll
                    for (int a_ = 0; a_ < 4; ++a_)
#pragma unroll
                        for (int b_ = 0; b_ < 4; ++b_) acc[a_][b_] = fma(pi[a_], pj[b_], acc[a_][b_]);
                }
#pragma unroll
                for (int a_ = 0; a_ < 4; ++a_)
#pragma unroll
                    for (int b_ = 0; b_ < 4; ++b_) {
                        const int i = bi * 4 + a_, j = bj * 4 + b_;
                        if (i < r2 && j <= i) m[(long long)(k0 + nb + i) * n + k0 + nb + j] -= acc[a_][b_];
                    }
            }
        }
    }
    __syncthreads();
    for (long long t = tid; t < (long long)n * n; t += nt) { const int i = (int)(t / n), k = (int)(t % n); if (k > i) m[t] = 0.0; }
    __syncthreads();
}

// One slab of nc right-hand sides of  L^T Y = X  (L lower triangular n x n, X n x n row-major, both in global memory), solved in
// LDS, blocked.  by_rows = false: the slab is the columns [c0, c0 + nc) of X (Y overwrites them);  by_rows = true: the slab is the
// ROWS [c0, c0 + nc) of X read as columns (i.e. the slab of X^T), and Y is written back into those rows -- the matrix then holds
// (L^-T X^T)^T = X L^-1, which is what the second solve of  L^-T Phi L^-1  needs, without a transposition pass.
// The slab stays in LDS for the whole solve (round-3 first version updated it in global memory: one dependent read-modify-write per
// element and block row, 0.9 ms per solve at B = 512); block rows of GP_NB from the bottom: the block's rows against the diagonal
// block of L (a thread per column), then every row above gets  X[r'] -= sum_t L[t][r'] X[t].   lds: n * (GP_NB + nc) doubles.
__device__ void solve_LT_slab(const double* L, int n, double* X, int c0, int nc, bool by_rows, double* lds) {
    const int tid = threadIdx.x, nt = blockDim.x;
    double* Lb = lds;                                          // [GP_NB][n]: rows of the block, columns 0 .. i0 + nb
    double* Xs = lds + (size_t)GP_NB * n;                      // [n][nc]: the slab
    for (long long t = tid; t < (long long)n * nc; t += nt) {
        if (by_rows) { const int c = (int)(t / n), r = (int)(t % n); Xs[r * nc + c] = X[(long long)(c0 + c) * n + r]; }
        else { const int r = (int)(t / nc), c = (int)(t % nc); Xs[r * nc + c] = X[(long long)r * n + c0 + c]; }
    }
    for (int i0 = ((n - 1) / GP_NB) * GP_NB; i0 >= 0; i0 -= GP_NB) {
        const int nb = min(GP_NB, n - i0);
        __syncthreads();
        for (int t = tid; t < nb * (i0 + nb); t += nt) { const int r = t / (i0 + nb), c = t % (i0 + nb); Lb[r * n + c] = L[(long long)(i0 + r) * n + c]; }
        __syncthreads();
        for (int c = tid; c < nc; c += nt) {                   // the block's own rows: back substitution, one column per thread
            for (int r = nb - 1; r >= 0; --r) {
                double v = Xs[(i0 + r) * nc + c];
                for (int q = r + 1; q < nb; ++q) v -= Lb[q * n + i0 + r] * Xs[(i0 + q) * nc + c];
                Xs[(i0 + r) * nc + c] = v / Lb[r * n + i0 + r];
            }
        }
        __syncthreads();
        for (int t = tid; t < i0 * nc; t += nt) {
            const int r = t / nc, c = t % nc;
            double v = 0.0;
            for (int q = 0; q < nb; ++q) v = fma(Lb[q * n + r], Xs[(i0 + q) * nc + c], v);
            Xs[r * nc + c] -= v;
        }
    }
    __syncthreads();
    for (long long t = tid; t < (long long)n * nc; t += nt) {
        if (by_rows) { const int c = (int)(t / n), r = (int)(t % n); X[(long long)(c0 + c) * n + r] = Xs[r * nc + c]; }
        else { const int r = (int)(t / nc), c = (int)(t % nc); X[(long long)r * n + c0 + c] = Xs[r * nc + c]; }
    }
    __syncthreads();
}

// inv <- (L L^T)^-1 for lower-triangular L (n x n); tmp: n x n scratch (receives L^-1)
__device__ void spd_inverse_from_chol(const double* L, int n, double* tmp, double* inv) {
    const int tid = threadIdx.x, nt = blockDim.x;
    // column j of L^-1 by forward substitution (one thread per column; n <= a few dozen)
    for (int j = tid; j < n; j += nt) {
        for (int i = 0; i < n; ++i) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= L[i * n + k] * tmp[k * n + j];
            tmp[i * n + j] = (i < j) ? 0.0 : s / L[i * n + i];
        }
    }
    __syncthreads();
    for (int t = tid; t < n * n; t += nt) {
        const int a = t / n, b = t % n;
        double s = 0.0;
        for (int k = max(a, b); k < n; ++k) s += tmp[k * n + a] * tmp[k * n + b];
        inv[t] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ double kern1(double d, double inv_s2ls) { const double t = inv_s2ls * d; return exp(-(t * t)); }

// inducing point k to query point x: (Xu0 - x) + k step.  The reference builds Knu in fp32 (gp.py:90), i.e. on distances rounded to
// fp32; that rounding is reproduced in the bug-compatible mode (jitter_ku == 0, well-conditioned grids).  With the H2 remedy
// switched on the grid is dense, cond(Ku) reaches 1e6..1e8 and a 1e-7 relative perturbation of a distance would move the
// posterior by percents: the distance then stays in float64.
__device__ __forceinline__ double knu_dist(double xu0, double xb, int k, double step, bool round32) {
    const double d = (xu0 - xb) + (double)k * step;
    return round32 ? (double)(float)d : d;
}

// block-wide sum of one double per thread (fixed order): red = blockDim.x (a power of two) doubles of LDS
__device__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = (int)blockDim.x / 2; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const double r = red[0];
    __syncthreads();
    return r;
}

struct GainArgs {
    int C, B, n, taps;
    double jitter_b, jitter_ku, prior_var;
    const long long* tab; const float* P; const float* xu; const float* cov; long long ldc; const float* eps; const double* hrf;
    double* ws;
};

// ------------------------------------------------------------------------------------------------ forward
// The per-covariate prelude of the forward pass, shared by both paths (O(n^3 + B n^2) work, one workgroup per covariate): x, eps and
// beta_mean = sa x (+ f) into the workspace; for a GP covariate the Ku factor and inverse, A = Knu^T Ku^-1, M = S - kvar Ku,
// f = A m (also into o_fb), T2 = A M, chol(S) and kl_gp.  Returns kl_lin (+ kl_gp) and sets kvar, ls, step (GP covariates only).
// bm[b] is last written by the thread that owns b (b = tid, tid + nt, ...); everything else is behind a barrier.
__device__ double gain_prelude(const GainArgs& a, int c, double* W, const GpLayout& w, double* red, double* o_fb,
                               double& kvar, double& ls, double& step) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int B = a.B, n = a.n;
    const long long* tb = a.tab + (size_t)c * TAB_W;
    const bool is_gp = tb[0] != 0;
    const int gk = (int)tb[2];
    double* x = W + w.x; double* e = W + w.e; double* bm = W + w.bm;
    const double sa = (double)a.P[tb[3]], std_ = exp((double)a.P[tb[4]]);
    for (int b = tid; b < B; b += nt) {
        const double xv = (double)a.cov[(size_t)b * a.ldc + c];
        x[b] = xv; e[b] = (double)a.eps[(size_t)c * B + b]; bm[b] = sa * xv;
    }
    const double vr = (std_ / 0.5) * (std_ / 0.5), t1 = ((sa - 1.0) / 0.5) * ((sa - 1.0) / 0.5);
    double kl = 0.5 * (vr + t1 - 1.0 - log(vr));               // calc_linW_KL
    kvar = 0.0; ls = 1.0; step = 0.0;
    __syncthreads();
    if (is_gp) {
        const float* xu = a.xu + (size_t)gk * n;
        const float stepf = xu[1] - xu[0];                     // fp32, as (xu[1] - xu[0]) of the reference
        step = (double)stepf;
        const double xu0 = (double)xu[0];
        kvar = exp((double)a.P[tb[7]]) + 0.1;
        ls = 3.0 / (1.0 + exp(-(exp((double)a.P[tb[8]]) + 0.5)));
        const double isl = 1.0 / sqrt(2.0) / ls;
        const float* qm = a.P + tb[5]; const float* qS = a.P + tb[6];
        double* N1 = W + w.N1; double* N2 = W + w.N2; double* kinv = W + w.kinv; double* A = W + w.A; double* M = W + w.M;
        double* T1 = W + w.T1; double* T2 = W + w.T2; double* Ls = W + w.Ls;
        // Ku (+ jitter) -> Cholesky -> inverse
        for (int t = tid; t < n * n; t += nt) {
            const int p = t / n, q = t % n;
            N1[t] = kern1(fabs((double)(p - q)) * step, isl) + (p == q ? a.jitter_ku : 0.0);
        }
        __syncthreads();
        chol_inplace(N1, n);
        spd_inverse_from_chol(N1, n, N2, kinv);
        // Knu^T (B x n), distances rounded to fp32 as the reference builds them; A = Knu^T Ku^-1
        for (int t = tid; t < B * n; t += nt) {
            const int b = t / n, k = t % n;
            T1[t] = kern1(knu_dist(xu0, x[b], k, step, a.jitter_ku == 0.0), isl);
        }
        __syncthreads();
        for (int t = tid; t < B * n; t += nt) {
            const int b = t / n, k = t % n;
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += T1[b * n + j] * kinv[j * n + k];
            A[t] = s;
        }
        // M = S - kvar (Ku + jitter)
        for (int t = tid; t < n * n; t += nt) {
            const int p = t / n, q = t % n;
            M[t] = (double)qS[t] - kvar * (kern1(fabs((double)(p - q)) * step, isl) + (p == q ? a.jitter_ku : 0.0));
        }
        __syncthreads();
        // f = A m ; T2 = A M
        for (int b = tid; b < B; b += nt) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += A[b * n + k] * (double)qm[k];
            if (o_fb) o_fb[(size_t)c * B + b] = s;
            bm[b] += s;
        }
        for (int t = tid; t < B * n; t += nt) {
            const int b = t / n, k = t % n;
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += A[b * n + j] * M[j * n + k];
            T2[t] = s;
        }
        // KL(N(m, S) || N(0, pv I)) through chol(S)
        for (int t = tid; t < n * n; t += nt) Ls[t] = (double)qS[t];
        __syncthreads();
        chol_inplace(Ls, n);
        double part = 0.0;
        for (int t = tid; t < n * n; t += nt) {
            const int p = t / n, q = t % n;
            if (q <= p) part += Ls[t] * Ls[t] / a.prior_var;
            if (q == p) part += -2.0 * log(Ls[t]) + (double)qm[p] * (double)qm[p] / a.prior_var;
        }
        const double tot = block_sum(part, red);
        kl += 0.5 * (n * log(a.prior_var) + tot - n);
    }
    return kl;
}

template <int T>
__global__ void __launch_bounds__(T)
gain_fwd_k(GainArgs a, float* __restrict__ task_var, double* __restrict__ kl_part,
           double* __restrict__ o_bm, double* __restrict__ o_bc, double* __restrict__ o_fb, double* __restrict__ o_sg) {
    VG_DYN_SMEM(double, lds);
    double* red = lds;                                         // T doubles
    const int c = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int B = a.B, n = a.n;
    const GpLayout w = gp_layout(B, n);
    double* W = a.ws + (size_t)c * w.total;
    const bool in_lds = B <= GP_LDS_MAXB;
    double* Cm = in_lds ? lds + T : W + w.Lc;                  // the B x B matrix being built / factorised
    const long long* tb = a.tab + (size_t)c * TAB_W;
    const bool is_gp = tb[0] != 0, is_hrf = tb[1] != 0;
    double* x = W + w.x; double* e = W + w.e; double* bm = W + w.bm;
    const double sa = (double)a.P[tb[3]], std_ = exp((double)a.P[tb[4]]);
    double kvar, ls, step;
    const double kl = gain_prelude(a, c, W, w, red, o_fb, kvar, ls, step);
    // beta_cov (+ jitter_b on the diagonal for the factorisation)
    {
        const double* A = W + w.A; const double* T2 = W + w.T2;
        const double isl = 1.0 / sqrt(2.0) / ls;
        const double s2 = std_ * std_;
        for (long long t = tid; t < (long long)B * B; t += nt) {
            const int i = (int)(t / B), j = (int)(t % B);
            double v = (i == j) ? s2 * x[i] * x[i] : 0.0;
            if (is_gp) {
                double sg = kvar * kern1(x[j] - x[i], isl);
                for (int k = 0; k < n; ++k) sg += T2[i * n + k] * A[j * n + k];
                if (o_sg) o_sg[((size_t)c * B + i) * B + j] = sg;
                v += sg;
            }
            if (o_bc) o_bc[((size_t)c * B + i) * B + j] = v;
            Cm[t] = v + (i == j ? a.jitter_b : 0.0);
        }
        if (o_bm) for (int b = tid; b < B; b += nt) o_bm[(size_t)c * B + b] = bm[b];
    }
    __syncthreads();
    if (in_lds) chol_inplace(Cm, B);
    else chol_blocked(Cm, B, lds + T);                         // large batches: 16-column panels in LDS
    if (in_lds) {
        double* Lc = W + w.Lc;
        for (long long t = tid; t < (long long)B * B; t += nt) Lc[t] = Cm[t];
    }
    // gain = beta_mean + L eps, then the HRF along the batch index
    double* tv = W + w.v1;
    if (in_lds) {
        for (int b = tid; b < B; b += nt) {
            double s = bm[b];
            for (int j = 0; j <= b; ++j) s += Cm[(long long)b * B + j] * e[j];
            tv[b] = s;
        }
    } else {
        // the factor is in global memory: a WAVEFRONT per row (lanes along the row: coalesced), fixed-order shuffle reduction
        const int lane = tid % VG_WAVE, wv = tid / VG_WAVE, nwv = nt / VG_WAVE;
        for (int b = wv; b < B; b += nwv) {
            double s = 0.0;
            for (int j = lane; j <= b; j += VG_WAVE) s += Cm[(long long)b * B + j] * e[j];
            for (int off = VG_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
            if (lane == 0) tv[b] = bm[b] + s;
        }
    }
    __syncthreads();
    for (int b = tid; b < B; b += nt) {
        double s = tv[b];
        if (is_hrf) {
            s = 0.0;
            for (int t = 0; t < a.taps && t <= b; ++t) s += a.hrf[t] * tv[b - t];
        }
        task_var[(size_t)c * B + b] = (float)s;
    }
    if (tid == 0) {
        kl_part[c] = kl;
        double* sc = W + w.sc;
        sc[0] = sa; sc[1] = std_; sc[2] = kvar; sc[3] = ls; sc[4] = step;
    }
}

__global__ void gain_kl_sum_k(const double* __restrict__ kl_part, int C, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += kl_part[c];
        out[0] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ double wave_sum_f64(double v) {     // fixed-order shuffle reduction; the total lands in lane 0
    for (int off = VG_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// linear gain (both paths): beta_mean = sa x, beta_cov diag = std^2 x^2, kl_lin(sa, std).  Gm: d loss / d beta_cov (its diagonal is read)
__device__ void gain_bwd_linear(const GainArgs& a, const long long* tb, const double* x, const double* g, const double* Gm, int B,
                                double sa, double std_, double gkl, double* red, float* G32) {
    const int tid = threadIdx.x, nt = blockDim.x;
    double p_sa = 0.0, p_sd = 0.0;
    for (int b = tid; b < B; b += nt) { p_sa += g[b] * x[b]; p_sd += Gm[(long long)b * B + b] * x[b] * x[b]; }
    const double s_sa = block_sum(p_sa, red), s_sd = block_sum(p_sd, red);
    if (tid == 0) {
        const double d_sa = s_sa + gkl * (sa - 1.0) / 0.25;
        // d/dstd: 2 std * sum(..) + kl: 0.5 (2 std / 0.25 - 2 / std);  d std / d logstd = std
        const double d_std = 2.0 * std_ * s_sd + gkl * 0.5 * (2.0 * std_ / 0.25 - 2.0 / std_);
        G32[tb[3]] += (float)d_sa;
        G32[tb[4]] += (float)(d_std * std_);
    }
}

// dM = A^T G2 and dm = A^T g (+ KL), G2 = dSigma A already in the workspace: a WAVEFRONT per output, lanes along the B-term sum
__device__ void gain_bwd_dm_wave(const GainArgs& a, const long long* tb, double* W, const GpLayout& w, const double* g, double gkl, float* G32) {
    const int tid = threadIdx.x, nt = blockDim.x, B = a.B, n = a.n;
    const int lane = tid % VG_WAVE, wv = tid / VG_WAVE, nwv = nt / VG_WAVE;
    const float* qm = a.P + tb[5];
    const double* A = W + w.A; const double* G2 = W + w.T1; double* gM = W + w.N1;
    for (int t = wv; t < n * n; t += nwv) {
        const int p = t / n, q = t % n;
        double s = 0.0;
        for (int b = lane; b < B; b += VG_WAVE) s += A[b * n + p] * G2[b * n + q];
        s = wave_sum_f64(s);
        if (lane == 0) gM[t] = s;
    }
    for (int k = wv; k < n; k += nwv) {
        double s = 0.0;
        for (int b = lane; b < B; b += VG_WAVE) s += A[b * n + k] * g[b];
        s = wave_sum_f64(s);
        if (lane == 0) G32[tb[5] + k] += (float)(s + gkl * (double)qm[k] / a.prior_var);
    }
}

// The GP hyper-parameter gradients behind G2 = dSigma A and dM (both paths): dA, dS (qu_S), d kvar, d ls.  p_kv / p_ls: this thread's
// share of the B x B sums  sum dSigma . Knn1  and  sum dSigma . kvar Knn1 d^2,  already accumulated by the caller.
__device__ void gain_bwd_gp_tail(const GainArgs& a, const long long* tb, double* W, const GpLayout& w, const double* x, const double* g,
                                 double kvar, double ls, double step, double gkl, bool in_lds, double p_kv, double p_ls, double* red,
                                 float* G32) {
    const int tid = threadIdx.x, nt = blockDim.x, B = a.B, n = a.n;
    const float* qm = a.P + tb[5];
    const double* kinv = W + w.kinv; const double* M = W + w.M; const double* Ls = W + w.Ls;
    const double* G2 = W + w.T1; double* gA = W + w.T2; double* gKnuT = W + w.T3; const double* gM = W + w.N1; double* gKinv = W + w.N2;
    const double isl = 1.0 / sqrt(2.0) / ls;
    const float* xu = a.xu + (size_t)tb[2] * n;
    const double xu0 = (double)xu[0];
    for (int t = tid; t < B * n; t += nt) {
        const int b = t / n, k = t % n;
        double s = g[b] * (double)qm[k];
        for (int j = 0; j < n; ++j) s += G2[b * n + j] * (M[j * n + k] + M[k * n + j]);
        gA[t] = s;
    }
    __syncthreads();
    // dS = dM + gkl * 0.5 (I / pv - S^-1),  S^-1 from chol(S)
    double* tmp = W + w.N3; double* Sinv = W + w.N4;
    spd_inverse_from_chol(Ls, n, tmp, Sinv);
    for (int t = tid; t < n * n; t += nt) {
        const int p = t / n, q = t % n;
        G32[tb[6] + t] += (float)(gM[t] + gkl * 0.5 * ((p == q ? 1.0 / a.prior_var : 0.0) - Sinv[t]));
    }
    // d kvar = sum dSigma . Knn1  -  sum dM . (Ku1 + jitter)
    for (int t = tid; t < n * n; t += nt) {
        const int p = t / n, q = t % n;
        const double d = fabs((double)(p - q)) * step;
        p_kv -= gM[t] * (kern1(d, isl) + (p == q ? a.jitter_ku : 0.0));
    }
    // A = Knu^T Kinv:  dKnu^T = dA Kinv^T ;  dKinv = Knu dA ;  dKu = -Kinv^T dKinv Kinv^T - kvar dM
    for (int t = tid; t < B * n; t += nt) {
        const int b = t / n, k = t % n;
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += gA[b * n + j] * kinv[k * n + j];
        gKnuT[t] = s;
    }
    if (in_lds) {
        for (int t = tid; t < n * n; t += nt) {
            const int p = t / n, q = t % n;
            double s = 0.0;
            for (int b = 0; b < B; ++b) {
                s += kern1(knu_dist(xu0, x[b], p, step, a.jitter_ku == 0.0), isl) * gA[b * n + q];
            }
            gKinv[t] = s;
        }
    } else {
        const int lane = tid % VG_WAVE, wv = tid / VG_WAVE, nwv = nt / VG_WAVE;
        for (int t = wv; t < n * n; t += nwv) {
            const int p = t / n, q = t % n;
            double s = 0.0;
            for (int b = lane; b < B; b += VG_WAVE) s += kern1(knu_dist(xu0, x[b], p, step, a.jitter_ku == 0.0), isl) * gA[b * n + q];
            s = wave_sum_f64(s);
            if (lane == 0) gKinv[t] = s;
        }
    }
    __syncthreads();
    for (int t = tid; t < B * n; t += nt) {
        const int b = t / n, k = t % n;
        const double d = knu_dist(xu0, x[b], k, step, a.jitter_ku == 0.0);
        p_ls += gKnuT[t] * kern1(d, isl) * d * d;
    }
    for (int t = tid; t < n * n; t += nt) {                    // tmp = Kinv^T dKinv
        const int p = t / n, q = t % n;
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += kinv[j * n + p] * gKinv[j * n + q];
        tmp[t] = s;
    }
    __syncthreads();
    for (int t = tid; t < n * n; t += nt) {
        const int p = t / n, q = t % n;
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += tmp[p * n + j] * kinv[q * n + j];
        const double gku = -s - kvar * gM[t];
        const double d = fabs((double)(p - q)) * step;
        p_ls += gku * kern1(d, isl) * d * d;
    }
    const double s_kv = block_sum(p_kv, red), s_ls = block_sum(p_ls, red);
    if (tid == 0) {
        const double lk = (double)a.P[tb[7]], ll = (double)a.P[tb[8]];
        G32[tb[7]] += (float)(s_kv * exp(lk));                                  // kvar = exp(logkvar) + 0.1
        const double sg = ls / 3.0;                                             // ls = 3 sigmoid(exp(log_ls) + 0.5)
        G32[tb[8]] += (float)(s_ls / (ls * ls * ls) * 3.0 * sg * (1.0 - sg) * exp(ll));
    }
}

// g_tv [C][B]: d loss / d gain (fp32),  g_kl [1]: d loss / d (sum of the KL terms).  Parameter gradients are added into G32
// (the flat fp32 gradient buffer, same offsets as P).
// PHASE 0: the whole backward (B x B matrix in LDS).  Large batches: PHASE 1 = up to Phi (left in the workspace), then the two
// triangular solves as slab launches (gain_trsm_k), PHASE 2 = everything behind them.
template <int T, int PHASE>
__global__ void __launch_bounds__(T)
gain_bwd_k(GainArgs a, const float* __restrict__ g_tv, const float* __restrict__ g_kl, float* __restrict__ G32) {
    VG_DYN_SMEM(double, lds);
    double* red = lds;
    const int c = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int B = a.B, n = a.n;
    const GpLayout w = gp_layout(B, n);
    double* W = a.ws + (size_t)c * w.total;
    const bool in_lds = B <= GP_LDS_MAXB;
    double* Gm = in_lds ? lds + T : W + w.G;                   // d loss / d beta_cov, built in place
    const long long* tb = a.tab + (size_t)c * TAB_W;
    const bool is_gp = tb[0] != 0, is_hrf = tb[1] != 0;
    const double* x = W + w.x; const double* e = W + w.e; const double* Lc = W + w.Lc;
    const double* sc = W + w.sc;
    const double sa = sc[0], std_ = sc[1], kvar = sc[2], ls = sc[3], step = sc[4];
    const double gkl = (double)g_kl[0];
    double* g = W + w.v1; double* u = W + w.v2; double* gin = W + w.v3;
    if (PHASE != 2) {
    // HRF transposed: g[i] = sum_t hk[t] gin[i + t]
    for (int b = tid; b < B; b += nt) gin[b] = (double)g_tv[(size_t)c * B + b];
    __syncthreads();
    for (int b = tid; b < B; b += nt) {
        double s = gin[b];
        if (is_hrf) {
            s = 0.0;
            for (int t = 0; t < a.taps && b + t < B; ++t) s += a.hrf[t] * gin[b + t];
        }
        g[b] = s;
    }
    __syncthreads();
    // u = L^T g ;  Phi = tril(u eps^T) with the diagonal halved  (L^T dL for dL = tril(g eps^T))
    for (int i = tid; i < B; i += nt) {
        double s = 0.0;
        for (int k = i; k < B; ++k) s += Lc[(long long)k * B + i] * g[k];
        u[i] = s;
    }
    __syncthreads();
    for (long long t = tid; t < (long long)B * B; t += nt) {
        const int i = (int)(t / B), j = (int)(t % B);
        Gm[t] = (j < i) ? u[i] * e[j] : (j == i ? 0.5 * u[i] * e[i] : 0.0);
    }
    __syncthreads();
    if (PHASE == 1) return;
    // S = L^-T Phi L^-1:  X = L^-T Phi;  S^T = L^-T X^T;  d beta_cov = (S + S^T) / 2
    solve_LT_inplace(Lc, B, Gm, B, B);
    for (long long t = tid; t < (long long)B * B; t += nt) {   // transpose in place (pairwise swap)
        const int i = (int)(t / B), j = (int)(t % B);
        if (j < i) { const double p = Gm[(long long)i * B + j]; Gm[(long long)i * B + j] = Gm[(long long)j * B + i]; Gm[(long long)j * B + i] = p; }
    }
    __syncthreads();
    solve_LT_inplace(Lc, B, Gm, B, B);
    }                                                          // (PHASE 2 starts here: Gm = L^-T Phi L^-1 from the slab launches)
    for (long long t = tid; t < (long long)B * B; t += nt) {
        const int i = (int)(t / B), j = (int)(t % B);
        if (j < i) { const double s = 0.5 * (Gm[(long long)i * B + j] + Gm[(long long)j * B + i]); Gm[(long long)i * B + j] = s; Gm[(long long)j * B + i] = s; }
    }
    __syncthreads();
    gain_bwd_linear(a, tb, x, g, Gm, B, sa, std_, gkl, red, G32);
    if (!is_gp) return;
    const float* qm = a.P + tb[5];
    const double* A = W + w.A;
    double* G2 = W + w.T1; double* gM = W + w.N1;
    const double isl = 1.0 / sqrt(2.0) / ls;
    // G2 = dSigma A  (dSigma symmetric);  dM = A^T G2 ; dm = A^T g (+ KL)
    if (in_lds) {
        for (int t = tid; t < B * n; t += nt) {
            const int b = t / n, k = t % n;
            double s = 0.0;
            for (int j = 0; j < B; ++j) s += Gm[(long long)b * B + j] * A[j * n + k];
            G2[t] = s;
        }
        __syncthreads();
        for (int t = tid; t < n * n; t += nt) {
            const int p = t / n, q = t % n;
            double s = 0.0;
            for (int b = 0; b < B; ++b) s += A[b * n + p] * G2[b * n + q];
            gM[t] = s;
        }
        for (int k = tid; k < n; k += nt) {
            double s = 0.0;
            for (int b = 0; b < B; ++b) s += A[b * n + k] * g[b];
            G32[tb[5] + k] += (float)(s + gkl * (double)qm[k] / a.prior_var);
        }
    } else {
        // large batches: the sums run over B = 256..1000 terms held in global memory -- a WAVEFRONT per output, lanes along the sum
        // (coalesced), fixed-order shuffle reduction (a thread per output walked them one dependent load at a time: with n*n or n
        // outputs only a few dozen threads were busy for hundreds of microseconds)
        const int lane = tid % VG_WAVE, wv = tid / VG_WAVE, nwv = nt / VG_WAVE;
        for (int t = wv; t < B * n; t += nwv) {
            const int b = t / n, k = t % n;
            double s = 0.0;
            for (int j = lane; j < B; j += VG_WAVE) s += Gm[(long long)b * B + j] * A[j * n + k];
            s = wave_sum_f64(s);
            if (lane == 0) G2[t] = s;
        }
        __syncthreads();
        gain_bwd_dm_wave(a, tb, W, w, g, gkl, G32);
    }
    // d kvar, d ls: this thread's share of  sum dSigma . Knn1  and  sum dSigma . kvar Knn1 d^2
    double p_kv = 0.0, p_ls = 0.0;
    for (long long t = tid; t < (long long)B * B; t += nt) {
        const int i = (int)(t / B), j = (int)(t % B);
        const double d = x[j] - x[i], kv = kern1(d, isl), gs = Gm[t];
        p_kv += gs * kv;
        p_ls += kvar * gs * kv * d * d;                        // d Knn / d ls = Knn d^2 / ls^3  (the 1/ls^3 is applied at the end)
    }
    gain_bwd_gp_tail(a, tb, W, w, x, g, kvar, ls, step, gkl, in_lds, p_kv, p_ls, red, G32);
}

// right-hand sides per slab of a large-batch solve: the slab (B x nc) and a block row of L (GP_NB x B) share the 160 KB of LDS
__host__ __device__ inline int gp_slab_cols(int B) { return B <= 608 ? 16 : (B <= 832 ? 8 : 4); }

// large batches: one slab of  L^-T (.)  on the B x B matrix at w.G (L at w.Lc); grid = C * ceil(B / gp_slab_cols(B)) workgroups
__global__ void __launch_bounds__(GP_TB)
gain_trsm_k(GainArgs a, int by_rows) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B;
    const int per = gp_slab_cols(B), nsl = (B + per - 1) / per;
    const int c = blockIdx.x / nsl, sl = blockIdx.x % nsl;
    const GpLayout w = gp_layout(B, a.n);
    double* W = a.ws + (size_t)c * w.total;
    const int c0 = sl * per, nc = min(per, B - c0);
    solve_LT_slab(W + w.Lc, B, W + w.G, c0, nc, by_rows != 0, lds);
}

// ================================================================================================ tiled path (any B up to 4096)
// The same arithmetic as above for batches whose panel / slab no longer fits LDS (B > 1024), spread over many workgroups: every O(B^2)
// and O(B^3) launch has a grid of at least C * ceil(B / 64) workgroups, all C covariates in every grid.  Ordering comes only from launch
// boundaries on the stream (no inter-workgroup flags, no host sync, no allocation: the whole path can be captured in a hipGraph).  Every
// sum runs in a fixed order and no float atomics are used, so the path is run-to-run bit-reproducible.
//   forward:  prelude (gain_pre_k, a workgroup per covariate: gain_prelude) -> beta_cov in 64 x 64 tiles -> per 64-column panel of the
//             right-looking Cholesky: factor the diagonal block, solve the panel below it, update the trailing lower triangle in tiles
//             -> gain = beta_mean + L eps (a wavefront per row) -> HRF along the batch index -> gain_kl_sum_k.
//   backward: transposed HRF, u = L^T g -> X = L^-T Phi (column slabs of 64, Phi generated on the fly) -> X L^-1 (row slabs, in place)
//             -> dSigma = (S + S^T) / 2 in tile pairs -> G2 = dSigma A and the B x B sums per 64-row block -> the rest per covariate.
constexpr int GT = 64;                     // tile edge / panel width / slab width of the tiled path
constexpr int GTP = GT + 1;                // LDS pitch of a tile in doubles
constexpr int GP_TT = 256;                 // threads per workgroup of the tiled kernels (4 x 4 outputs per thread of a 64 x 64 tile)
constexpr int GP_MAXB_BLOCKED = 1024;      // largest batch of the blocked path (its panel / slab lives in LDS)
constexpr int GP_MAXB = 4096;              // largest batch of the gain block

__host__ __device__ inline int gt_tiles(int B) { return (B + GT - 1) / GT; }

// lower-triangle tile index t -> (bi, bj), bj <= bi (row bi holds bi + 1 tiles)
__device__ __forceinline__ void tri_decode(long long t, int& bi, int& bj) {
    bi = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long long)(bi + 1) * (bi + 2) / 2 <= t) ++bi;
    while ((long long)bi * (bi + 1) / 2 > t) --bi;
    bj = (int)(t - (long long)bi * (bi + 1) / 2);
}

// acc[a][b] += sum_{q < K} As[q][ty*4 + a] * Bs[q][tx*4 + b]: two K-major 64-wide LDS tiles (pitch GTP), thread (ty, tx) = (tid / 16, tid % 16)
__device__ __forceinline__ void mm4x4(const double* As, const double* Bs, int K, double acc[4][4]) {
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    for (int q = 0; q < K; ++q) {
        double pa[4], pb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { pa[i] = As[q * GTP + ty * 4 + i]; pb[i] = Bs[q * GTP + tx * 4 + i]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fma(pa[i], pb[j], acc[i][j]);
    }
}

// ---- forward
__global__ void __launch_bounds__(GP_TB)
gain_pre_k(GainArgs a, double* __restrict__ kl_part, double* __restrict__ o_bm, double* __restrict__ o_fb) {
    VG_DYN_SMEM(double, red);                                  // GP_TB doubles
    const int c = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const GpLayout w = gp_layout(a.B, a.n);
    double* W = a.ws + (size_t)c * w.total;
    const long long* tb = a.tab + (size_t)c * TAB_W;
    double kvar, ls, step;
    const double kl = gain_prelude(a, c, W, w, red, o_fb, kvar, ls, step);
    if (o_bm) for (int b = tid; b < a.B; b += nt) o_bm[(size_t)c * a.B + b] = W[w.bm + b];
    if (tid == 0) {
        kl_part[c] = kl;
        double* sc = W + w.sc;
        sc[0] = (double)a.P[tb[3]]; sc[1] = exp((double)a.P[tb[4]]); sc[2] = kvar; sc[3] = ls; sc[4] = step;
    }
}

// beta_cov (+ jitter_b on the diagonal) in 64 x 64 tiles, grid C * T * T: the lower triangle goes to the factor's slot (upper
// triangle zeroed); the optional full outputs beta_cov / Sigma get every tile.  Each element is formed exactly as in gain_fwd_k.
__global__ void __launch_bounds__(GP_TT)
gain_cov_k(GainArgs a, double* __restrict__ o_bc, double* __restrict__ o_sg) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B, n = a.n, T = gt_tiles(B);
    const int c = blockIdx.x / (T * T), bi = (blockIdx.x / T) % T, bj = blockIdx.x % T;
    const GpLayout w = gp_layout(B, n);
    double* W = a.ws + (size_t)c * w.total;
    double* Lc = W + w.Lc;
    const long long* tb = a.tab + (size_t)c * TAB_W;
    const bool is_gp = tb[0] != 0;
    const int tid = threadIdx.x, ty = tid / 16, tx = tid % 16;
    const int i0 = bi * GT, j0 = bj * GT;
    if (bj > bi && !o_bc && !o_sg) {                           // upper tile, nothing but zeros wanted
        for (int t = tid; t < GT * GT; t += GP_TT) {
            const int i = i0 + t / GT, j = j0 + t % GT;
            if (i < B && j < B) Lc[(long long)i * B + j] = 0.0;
        }
        return;
    }
    const double* x = W + w.x; const double* sc = W + w.sc;
    const double std_ = sc[1], kvar = sc[2], ls = sc[3];
    const double isl = 1.0 / sqrt(2.0) / ls, s2 = std_ * std_;
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = min(i0 + ty * 4 + p, B - 1), j = min(j0 + tx * 4 + q, B - 1);
            acc[p][q] = is_gp ? kvar * kern1(x[j] - x[i], isl) : 0.0;
        }
    if (is_gp) {                                               // sg += sum_k T2[i][k] A[j][k], k in order, in chunks of 64
        const double* A = W + w.A; const double* T2 = W + w.T2;
        double* Ts = lds; double* As = lds + GT * GTP;         // K-major: Ts[k][i], As[k][j]
        for (int k0 = 0; k0 < n; k0 += GT) {
            const int kc = min(GT, n - k0);
            __syncthreads();
            for (int t = tid; t < GT * GT; t += GP_TT) {
                const int r = t / GT, k = t % GT;
                const bool ok = k < kc;
                Ts[k * GTP + r] = (ok && i0 + r < B) ? T2[(long long)(i0 + r) * n + k0 + k] : 0.0;
                As[k * GTP + r] = (ok && j0 + r < B) ? A[(long long)(j0 + r) * n + k0 + k] : 0.0;
            }
            __syncthreads();
            mm4x4(Ts, As, kc, acc);
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + ty * 4 + p, j = j0 + tx * 4 + q;
            if (i >= B || j >= B) continue;
            double v = (i == j) ? s2 * x[i] * x[i] : 0.0;
            if (is_gp) {
                if (o_sg) o_sg[((size_t)c * B + i) * B + j] = acc[p][q];
                v += acc[p][q];
            }
            if (o_bc) o_bc[((size_t)c * B + i) * B + j] = v;
            Lc[(long long)i * B + j] = (j > i) ? 0.0 : v + (i == j ? a.jitter_b : 0.0);
        }
}

// Cholesky panel p, step 1: factor the diagonal block in LDS (the unblocked recurrence of chol_blocked), grid C
__global__ void __launch_bounds__(GP_TT)
gain_potrf_diag_k(GainArgs a, int p) {
    VG_DYN_SMEM(double, D);                                    // GT x GTP
    const int B = a.B, c = blockIdx.x, tid = threadIdx.x;
    const GpLayout w = gp_layout(B, a.n);
    double* Lc = a.ws + (size_t)c * w.total + w.Lc;
    const int k0 = p * GT, nb = min(GT, B - k0);
    for (int t = tid; t < nb * nb; t += GP_TT) { const int i = t / nb, j = t % nb; D[i * GTP + j] = Lc[(long long)(k0 + i) * B + k0 + j]; }
    for (int j = 0; j < nb; ++j) {
        __syncthreads();
        const double d = sqrt(D[j * GTP + j]);                 // NaN for a non-positive pivot, as cholesky_ex(check_errors=False)
        __syncthreads();
        for (int i = j + tid; i < nb; i += GP_TT) D[i * GTP + j] = (i == j) ? d : D[i * GTP + j] / d;
        __syncthreads();
        for (int t = tid; t < (nb - j - 1) * (nb - j - 1); t += GP_TT) {
            const int i = j + 1 + t / (nb - j - 1), k = j + 1 + t % (nb - j - 1);
            if (k <= i) D[i * GTP + k] -= D[i * GTP + j] * D[k * GTP + j];
        }
    }
    __syncthreads();
    for (int t = tid; t < nb * nb; t += GP_TT) { const int i = t / nb, j = t % nb; if (j <= i) Lc[(long long)(k0 + i) * B + k0 + j] = D[i * GTP + j]; }
}

// step 2: L21 = A21 L11^-T for the 64-row blocks below the diagonal block, grid C * T (blocks p+1 .. T-1 work).  A covariate without a
// GP has a diagonal beta_cov: its A21 and therefore L21 are exactly zero already, and so is every trailing update.
__global__ void __launch_bounds__(GP_TT)
gain_potrf_panel_k(GainArgs a, int p) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B, T = gt_tiles(B), tid = threadIdx.x;
    const int c = blockIdx.x / T, rb = p + 1 + blockIdx.x % T;
    if (rb >= T || a.tab[(size_t)c * TAB_W] == 0) return;
    const GpLayout w = gp_layout(B, a.n);
    double* Lc = a.ws + (size_t)c * w.total + w.Lc;
    const int k0 = p * GT, r0 = rb * GT, nr = min(GT, B - r0);   // the diagonal block is full: k0 + GT < B
    double* D = lds; double* X = lds + GT * GTP;
    for (int t = tid; t < GT * GT; t += GP_TT) {
        const int i = t / GT, j = t % GT;
        D[i * GTP + j] = Lc[(long long)(k0 + i) * B + k0 + j];
        X[i * GTP + j] = (i < nr) ? Lc[(long long)(r0 + i) * B + k0 + j] : 0.0;
    }
    for (int j = 0; j < GT; ++j) {
        __syncthreads();
        const double d = D[j * GTP + j];
        for (int i = tid; i < nr; i += GP_TT) X[i * GTP + j] /= d;
        __syncthreads();
        for (int t = tid; t < nr * (GT - j - 1); t += GP_TT) {
            const int i = t / (GT - j - 1), k = j + 1 + t % (GT - j - 1);
            X[i * GTP + k] -= X[i * GTP + j] * D[k * GTP + j];
        }
    }
    __syncthreads();
    for (int t = tid; t < nr * GT; t += GP_TT) { const int i = t / GT, j = t % GT; Lc[(long long)(r0 + i) * B + k0 + j] = X[i * GTP + j]; }
}

// step 3: trailing update  A22 -= L21 L21^T  on the lower-triangle tiles behind panel p, grid C * max(#tiles, T)
__global__ void __launch_bounds__(GP_TT)
gain_potrf_update_k(GainArgs a, int p, int per) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B, T = gt_tiles(B), tid = threadIdx.x;
    const int c = blockIdx.x / per, ti = blockIdx.x % per;
    const int nt = T - 1 - p;
    if (ti >= nt * (nt + 1) / 2 || a.tab[(size_t)c * TAB_W] == 0) return;
    int bi, bj;
    tri_decode(ti, bi, bj);
    bi += p + 1; bj += p + 1;
    const GpLayout w = gp_layout(B, a.n);
    double* Lc = a.ws + (size_t)c * w.total + w.Lc;
    const int k0 = p * GT, i0 = bi * GT, j0 = bj * GT;
    double* Pi = lds; double* Pj = lds + GT * GTP;             // K-major: Pi[q][i] = L[i0 + i][k0 + q]
    for (int t = tid; t < GT * GT; t += GP_TT) {
        const int r = t / GT, q = t % GT;
        Pi[q * GTP + r] = (i0 + r < B) ? Lc[(long long)(i0 + r) * B + k0 + q] : 0.0;
        Pj[q * GTP + r] = (j0 + r < B) ? Lc[(long long)(j0 + r) * B + k0 + q] : 0.0;
    }
    __syncthreads();
    double acc[4][4] = {};
    mm4x4(Pi, Pj, GT, acc);
    const int ty = tid / 16, tx = tid % 16;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < B && j <= i) Lc[(long long)i * B + j] -= acc[u][v];
        }
}

// gain = beta_mean + L eps: a WAVEFRONT per row (lanes along the row, fixed-order shuffle reduction, as gain_fwd_k), grid C * T
__global__ void __launch_bounds__(GP_TT)
gain_sample_k(GainArgs a) {
    const int B = a.B, T = gt_tiles(B);
    const int c = blockIdx.x / T, r0 = (blockIdx.x % T) * GT;
    const GpLayout w = gp_layout(B, a.n);
    double* W = a.ws + (size_t)c * w.total;
    const double* Lc = W + w.Lc; const double* e = W + w.e; const double* bm = W + w.bm;
    double* tv = W + w.v1;
    const int lane = threadIdx.x % VG_WAVE, wv = threadIdx.x / VG_WAVE;
    for (int b = r0 + wv; b < min(B, r0 + GT); b += GP_TT / VG_WAVE) {
        double s = 0.0;
        for (int j = lane; j <= b; j += VG_WAVE) s += Lc[(long long)b * B + j] * e[j];
        s = wave_sum_f64(s);
        if (lane == 0) tv[b] = bm[b] + s;
    }
}

// the HRF along the batch index (needs every gain of the covariate: its own launch), grid C * T of GT threads
__global__ void __launch_bounds__(GT)
gain_hrf_k(GainArgs a, float* __restrict__ task_var) {
    const int B = a.B, T = gt_tiles(B);
    const int c = blockIdx.x / T, b = (blockIdx.x % T) * GT + threadIdx.x;
    if (b >= B) return;
    const GpLayout w = gp_layout(B, a.n);
    const double* tv = a.ws + (size_t)c * w.total + w.v1;
    double s = tv[b];
    if (a.tab[(size_t)c * TAB_W + 1] != 0) {
        s = 0.0;
        for (int t = 0; t < a.taps && t <= b; ++t) s += a.hrf[t] * tv[b - t];
    }
    task_var[(size_t)c * B + b] = (float)s;
}

// ---- backward
// phase 1, grid C * T: g = HRF^T g_tv (every workgroup forms all of it in LDS), then u = L^T g for the workgroup's 64 columns (4 fixed
// stripes of the column sum, combined in order).  g and u go to the workspace (v1, v2).
__global__ void __launch_bounds__(GP_TT)
gain_bwd_p1_k(GainArgs a, const float* __restrict__ g_tv) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B, T = gt_tiles(B), tid = threadIdx.x;
    const int c = blockIdx.x / T, i0 = (blockIdx.x % T) * GT;
    const GpLayout w = gp_layout(B, a.n);
    double* W = a.ws + (size_t)c * w.total;
    const double* Lc = W + w.Lc;
    const bool is_hrf = a.tab[(size_t)c * TAB_W + 1] != 0;
    double* g = lds; double* red = lds + B;                    // B + GP_TT doubles
    const float* gin = g_tv + (size_t)c * B;
    for (int b = tid; b < B; b += GP_TT) {
        double s = (double)gin[b];
        if (is_hrf) {
            s = 0.0;
            for (int t = 0; t < a.taps && b + t < B; ++t) s += a.hrf[t] * (double)gin[b + t];
        }
        g[b] = s;
    }
    __syncthreads();
    const int col = tid % GT, st = tid / GT, i = i0 + col;
    double s = 0.0;
    if (i < B) for (int k = i + st; k < B; k += GP_TT / GT) s += Lc[(long long)k * B + i] * g[k];
    red[tid] = s;
    __syncthreads();
    if (st == 0 && i < B) {
        W[w.v2 + i] = ((red[col] + red[col + GT]) + red[col + 2 * GT]) + red[col + 3 * GT];
        W[w.v1 + i] = g[i];
    }
}

// One 64-wide slab of  L^T Y = X  (grid C * T), left-looking by 64-row blocks from the bottom: a block of the slab gets the
// contributions of the blocks already solved below it (L^T tiles streamed through LDS, 4 x 4 register tiles), then the back
// substitution against the diagonal block of L.  by_rows = 0: X = Phi = tril(u eps^T) with the diagonal halved, formed on the fly, and
// Y goes to the columns of the matrix at w.G;  by_rows = 1: the slab is ROWS of that matrix read as columns, solved in place, which
// leaves (L^-T X^T)^T = X L^-1 there.  A covariate without a GP has a diagonal L: the slab is only divided by it.
__global__ void __launch_bounds__(GP_TT)
gain_trsm_tiled_k(GainArgs a, int by_rows) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B, T = gt_tiles(B), tid = threadIdx.x;
    const int c = blockIdx.x / T, c0 = (blockIdx.x % T) * GT, ncv = min(GT, B - c0);
    const GpLayout w = gp_layout(B, a.n);
    double* W = a.ws + (size_t)c * w.total;
    const double* Lc = W + w.Lc; const double* u = W + w.v2; const double* e = W + w.e;
    double* G = W + w.G;
    const bool is_gp = a.tab[(size_t)c * TAB_W] != 0;
    // element (r, cc) of the slab: row r of the system, right-hand side c0 + cc
    auto at = [&](int r, int cc) -> long long { return by_rows ? (long long)(c0 + cc) * B + r : (long long)r * B + c0 + cc; };
    auto rhs = [&](int r, int cc) -> double {
        if (by_rows) return G[at(r, cc)];
        const int j = c0 + cc;
        return (j < r) ? u[r] * e[j] : (j == r ? 0.5 * u[r] * e[r] : 0.0);
    };
    // lanes along the contiguous index: the row index r (by_rows) or the column cc
    auto dec = [&](int t, int& r, int& cc) { if (by_rows) { cc = t / GT; r = t % GT; } else { r = t / GT; cc = t % GT; } };
    if (!is_gp) {
        for (long long t = tid; t < (long long)B * GT; t += GP_TT) {
            int r, cc;
            if (by_rows) { cc = (int)(t / B); r = (int)(t % B); } else { r = (int)(t / GT); cc = (int)(t % GT); }
            if (cc < ncv) G[at(r, cc)] = rhs(r, cc) / Lc[(long long)r * B + r];
        }
        return;
    }
    double* Lt = lds; double* Ys = lds + GT * GTP;             // K-major: Lt[q][r] = L[q0 + q][r0 + r], Ys[q][cc] = Y[q0 + q][cc]
    const int ty = tid / 16, tx = tid % 16;
    constexpr int PER = GT * GT / GP_TT;                       // tile elements per thread
    double lv[PER], yv[PER];                                   // the next tile pair, fetched while the current one is multiplied
    auto fetch = [&](int ib, int jb) {
        const int r0 = ib * GT, nr = min(GT, B - r0), q0 = jb * GT, nq = min(GT, B - q0);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int t = tid + k * GP_TT, q = t / GT, r = t % GT;
            lv[k] = (q < nq && r < nr) ? Lc[(long long)(q0 + q) * B + r0 + r] : 0.0;
            int yr, ycc;
            dec(t, yr, ycc);
            yv[k] = (yr < nq && ycc < ncv) ? G[at(q0 + yr, ycc)] : 0.0;
        }
    };
    for (int ib = T - 1; ib >= 0; --ib) {
        const int r0 = ib * GT, nr = min(GT, B - r0);
        double acc[4][4] = {};
        __syncthreads();                                       // the block solved last (ib + 1) is in global memory
        if (ib + 1 < T) fetch(ib, ib + 1);
        for (int jb = ib + 1; jb < T; ++jb) {
            const int nq = min(GT, B - jb * GT);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int t = tid + k * GP_TT;
                Lt[(t / GT) * GTP + t % GT] = lv[k];
                int yr, ycc;
                dec(t, yr, ycc);
                Ys[yr * GTP + ycc] = yv[k];
            }
            __syncthreads();
            if (jb + 1 < T) fetch(ib, jb + 1);
            mm4x4(Lt, Ys, nq, acc);
        }
        __syncthreads();
        // V = X - (contributions) into Ys as [r][cc]; the diagonal block of L into Lt as [r][q] = L[r0 + r][r0 + q]
        double* V = Ys; double* D = Lt;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = ty * 4 + p, cc = tx * 4 + q;
                V[r * GTP + cc] = (r < nr && cc < ncv) ? rhs(r0 + r, cc) - acc[p][q] : 0.0;
            }
        for (int t = tid; t < GT * GT; t += GP_TT) {
            const int r = t / GT, q = t % GT;
            D[r * GTP + q] = (r < nr && q < nr) ? Lc[(long long)(r0 + r) * B + r0 + q] : 0.0;
        }
        for (int r = nr - 1; r >= 0; --r) {                    // back substitution: Y[r] = V[r] / L[r][r];  V[q] -= L[r][q] Y[r], q < r
            __syncthreads();
            for (int cc = tid; cc < ncv; cc += GP_TT) V[r * GTP + cc] /= D[r * GTP + r];
            __syncthreads();
            for (int t = tid; t < r * ncv; t += GP_TT) {
                const int q = t / ncv, cc = t % ncv;
                V[q * GTP + cc] -= D[r * GTP + q] * V[r * GTP + cc];
            }
        }
        __syncthreads();
        for (int t = tid; t < GT * GT; t += GP_TT) {
            int r, cc;
            dec(t, r, cc);
            if (r < nr && cc < ncv) G[at(r0 + r, cc)] = V[r * GTP + cc];
        }
    }
}

// dSigma = (S + S^T) / 2 in place, one lower-triangle tile and its mirror per workgroup, grid C * T (T + 1) / 2
__global__ void __launch_bounds__(GP_TT)
gain_sym_k(GainArgs a) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B, T = gt_tiles(B), tid = threadIdx.x;
    const int per = T * (T + 1) / 2;
    const int c = blockIdx.x / per;
    if (a.tab[(size_t)c * TAB_W] == 0) return;                // diagonal beta_cov: only the diagonal of dSigma is read
    int bi, bj;
    tri_decode(blockIdx.x % per, bi, bj);
    const GpLayout w = gp_layout(B, a.n);
    double* G = a.ws + (size_t)c * w.total + w.G;
    const int i0 = bi * GT, j0 = bj * GT;
    double* Lo = lds; double* Up = lds + GT * GTP;             // Lo[i][j] = S[i0 + i][j0 + j],  Up[j][i] = S[j0 + j][i0 + i]
    for (int t = tid; t < GT * GT; t += GP_TT) {
        const int r = t / GT, q = t % GT;
        Lo[r * GTP + q] = (i0 + r < B && j0 + q < B) ? G[(long long)(i0 + r) * B + j0 + q] : 0.0;
        Up[r * GTP + q] = (j0 + r < B && i0 + q < B) ? G[(long long)(j0 + r) * B + i0 + q] : 0.0;
    }
    __syncthreads();
    for (int t = tid; t < GT * GT; t += GP_TT) {
        const int r = t / GT, q = t % GT;                      // lower element (i0 + r, j0 + q), mirror (j0 + q, i0 + r)
        const int i = i0 + r, j = j0 + q;
        if (i < B && j < i) G[(long long)i * B + j] = 0.5 * (Lo[r * GTP + q] + Up[q * GTP + r]);
        const int i2 = j0 + r, j2 = i0 + q;                    // upper element (j0 + r, i0 + q): coalesced along q
        if (j2 < B && i2 < j2) G[(long long)i2 * B + j2] = 0.5 * (Lo[q * GTP + r] + Up[r * GTP + q]);
    }
}

// per 64-row block of dSigma (grid C * T): G2 = dSigma A for those rows (64 x 64 output tiles through the register tiles) and the block's
// partial sums of  dSigma . Knn1  and  dSigma . kvar Knn1 d^2, into T-long arrays at v3 / bm (free in the backward pass)
__global__ void __launch_bounds__(GP_TT)
gain_bwd_rows_k(GainArgs a) {
    VG_DYN_SMEM(double, lds);
    const int B = a.B, n = a.n, T = gt_tiles(B), tid = threadIdx.x;
    const int c = blockIdx.x / T, rb = blockIdx.x % T, r0 = rb * GT, nr = min(GT, B - r0);
    if (a.tab[(size_t)c * TAB_W] == 0) return;
    const GpLayout w = gp_layout(B, n);
    double* W = a.ws + (size_t)c * w.total;
    const double* G = W + w.G; const double* A = W + w.A; const double* x = W + w.x;
    double* G2 = W + w.T1;
    const double kvar = W[w.sc + 2], ls = W[w.sc + 3];
    const double isl = 1.0 / sqrt(2.0) / ls;
    double* Gt = lds; double* As = lds + GT * GTP; double* red = lds + 2 * GT * GTP;   // Gt[j][r] = dSigma[r0 + r][j0 + j]
    const int ty = tid / 16, tx = tid % 16;
    double p_kv = 0.0, p_ls = 0.0;
    for (int k0 = 0; k0 < n; k0 += GT) {
        const int kc = min(GT, n - k0);
        double acc[4][4] = {};
        for (int jb = 0; jb < T; ++jb) {
            const int j0 = jb * GT, nj = min(GT, B - j0);
            __syncthreads();
            for (int t = tid; t < GT * GT; t += GP_TT) {
                const int r = t / GT, q = t % GT;
                Gt[q * GTP + r] = (r < nr && q < nj) ? G[(long long)(r0 + r) * B + j0 + q] : 0.0;
                As[r * GTP + q] = (r < nj && q < kc) ? A[(long long)(j0 + r) * n + k0 + q] : 0.0;
            }
            __syncthreads();
            mm4x4(Gt, As, nj, acc);
            if (k0 == 0) {
                for (int t = tid; t < nr * nj; t += GP_TT) {
                    const int r = t / nj, q = t % nj;
                    const double d = x[j0 + q] - x[r0 + r], kv = kern1(d, isl), gs = Gt[q * GTP + r];
                    p_kv += gs * kv;
                    p_ls += kvar * gs * kv * d * d;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = ty * 4 + p, k = tx * 4 + q;
                if (r < nr && k < kc) G2[(long long)(r0 + r) * n + k0 + k] = acc[p][q];
            }
    }
    const double s_kv = block_sum(p_kv, red), s_ls = block_sum(p_ls, red);
    if (tid == 0) { W[w.v3 + rb] = s_kv; W[w.bm + rb] = s_ls; }
}

// everything behind the B x B work, a workgroup per covariate (grid C): the linear gain, dM / dm, and the GP tail with the fixed-order
// sum of the row blocks' partials
__global__ void __launch_bounds__(GP_TB)
gain_bwd_fin_k(GainArgs a, const float* __restrict__ g_kl, float* __restrict__ G32) {
    VG_DYN_SMEM(double, red);                                  // GP_TB doubles
    const int c = blockIdx.x, tid = threadIdx.x;
    const int B = a.B, T = gt_tiles(B);
    const GpLayout w = gp_layout(B, a.n);
    double* W = a.ws + (size_t)c * w.total;
    const long long* tb = a.tab + (size_t)c * TAB_W;
    const double* x = W + w.x; const double* g = W + w.v1; const double* sc = W + w.sc;
    const double gkl = (double)g_kl[0];
    gain_bwd_linear(a, tb, x, g, W + w.G, B, sc[0], sc[1], gkl, red, G32);
    if (tb[0] == 0) return;
    gain_bwd_dm_wave(a, tb, W, w, g, gkl, G32);
    double p_kv = 0.0, p_ls = 0.0;
    if (tid == 0) for (int r = 0; r < T; ++r) { p_kv += W[w.v3 + r]; p_ls += W[w.bm + r]; }
    gain_bwd_gp_tail(a, tb, W, w, x, g, sc[2], sc[3], sc[4], gkl, false, p_kv, p_ls, red, G32);
}

GainArgs mk_args(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu, const float* cov, int64_t ldc,
                 const float* eps, const double* hrf, double* ws) {
    GainArgs a;
    a.C = d->C; a.B = d->B; a.n = d->n; a.taps = d->hrf_taps;
    a.jitter_b = d->jitter_b; a.jitter_ku = d->jitter_ku; a.prior_var = d->prior_var;
    a.tab = (const long long*)table; a.P = params; a.xu = xu; a.cov = cov; a.ldc = ldc; a.eps = eps; a.hrf = hrf; a.ws = ws;
    return a;
}

// What one forward / backward call launches for a batch of B volumes: the path, the blocking of the factorisation and of the solves, and
// the dynamic LDS of every launch.  gain_fwd / gain_bwd and their tiled twins take grids and LDS sizes from here and vg_gp_gain_plan
// reports the same record, so the arithmetic is written down once.
struct GainPlan {
    int path;                              // 0: one workgroup, B x B matrix in LDS;  1: blocked (panel / slab in LDS);  2: tiled
    int threads;                           // threads per workgroup of the factorisation / solve kernels
    int panel, npanels, last_panel;        // columns per panel of the Cholesky, panels, columns of the last panel
    int slab, nslabs, last_slab;           // right-hand sides per slab of a solve, slabs per covariate, width of the last slab
    size_t lds_main;                       // paths 0, 1: gain_fwd_k / gain_bwd_k;  path 2: the prelude / final kernels (reduction scratch)
    size_t lds_solve;                      // path 1: gain_trsm_k;  path 2: every two-tile kernel
    size_t lds_diag, lds_p1, lds_rows;     // path 2 only: gain_potrf_diag_k, gain_bwd_p1_k, gain_bwd_rows_k
    size_t lds_fwd, lds_bwd;               // the largest request of each pass
    int launches_fwd, launches_bwd;
};

GainPlan gain_plan(int B, bool forced) {
    GainPlan p = {};
    auto mx = [](size_t a_, size_t b_) { return a_ > b_ ? a_ : b_; };
    auto blocks = [](int B_, int w, int& nblk, int& last) { nblk = (B_ + w - 1) / w; last = B_ - (nblk - 1) * w; };
    if (forced || B > GP_MAXB_BLOCKED) {
        p.path = 2; p.threads = GP_TT; p.panel = GT; p.slab = GT;
        p.lds_main = (size_t)GP_TB * sizeof(double);
        p.lds_solve = (size_t)2 * GT * GTP * sizeof(double);                                     // two 64 x 64 tiles
        p.lds_diag = (size_t)GT * GTP * sizeof(double);
        p.lds_p1 = (size_t)(B + GP_TT) * sizeof(double);
        p.lds_rows = p.lds_solve + GP_TT * sizeof(double);
        blocks(B, p.panel, p.npanels, p.last_panel); blocks(B, p.slab, p.nslabs, p.last_slab);
        p.lds_fwd = mx(p.lds_main, mx(p.lds_solve, p.lds_diag));
        p.lds_bwd = mx(mx(p.lds_main, p.lds_p1), mx(p.lds_solve, p.lds_rows));
        p.launches_fwd = 2 + p.npanels + 2 * (p.npanels - 1) + 3; p.launches_bwd = 6;
    } else if (B <= GP_LDS_MAXB) {
        p.path = 0; p.threads = GP_T; p.panel = B; p.slab = B;                                   // unblocked: the whole matrix at once
        p.lds_main = (size_t)(GP_T + (size_t)B * B) * sizeof(double);                            // reduction scratch + the matrix
        blocks(B, p.panel, p.npanels, p.last_panel); blocks(B, p.slab, p.nslabs, p.last_slab);
        p.lds_fwd = p.lds_bwd = p.lds_main;
        p.launches_fwd = 2; p.launches_bwd = 1;
    } else {
        p.path = 1; p.threads = GP_TB; p.panel = GP_NB; p.slab = gp_slab_cols(B);
        p.lds_main = (size_t)(GP_TB + (size_t)B * GP_NBP) * sizeof(double);                      // reduction scratch + one factorisation panel
        p.lds_solve = (size_t)B * (GP_NB + p.slab) * sizeof(double);                             // a block row of L + the slab
        blocks(B, p.panel, p.npanels, p.last_panel); blocks(B, p.slab, p.nslabs, p.last_slab);
        p.lds_fwd = p.lds_main; p.lds_bwd = mx(p.lds_main, p.lds_solve);
        p.launches_fwd = 2; p.launches_bwd = 4;
    }
    return p;
}

// max_b: the largest batch the caller's path takes (GP_MAXB_BLOCKED for the blocked / LDS path, GP_MAXB for the tiled one)
int check(const vg_gain_desc* d, const char* who) {
    if (!d || d->C <= 0 || d->B <= 0 || d->n < 2 || d->n > 128 || d->hrf_taps < 0 || !(d->prior_var > 0)) {
        vg_set_error("%s: bad descriptor", who); return VG_ERR_ARG;
    }
    if (d->B > GP_MAXB) {
        vg_set_error("%s: batch of %d volumes exceeds the gain block's limit of %d volumes per joint draw", who, (int)d->B, GP_MAXB);
        return VG_ERR_UNSUPPORTED;
    }
    return VG_OK;
}

int gain_fwd_tiled(const vg_gain_desc* d, const GainArgs& a, double* kl_part, float* task_var, float* gp_kl, double* bm, double* bc,
                   double* fb, double* sg, hipStream_t s) {
    const GainPlan pl = gain_plan(d->B, true);
    const int C = d->C, T = pl.npanels;
    vg_launch(gain_pre_k, dim3(C), dim3(GP_TB), pl.lds_main, s, a, kl_part, bm, fb);
    vg_launch(gain_cov_k, dim3(C * T * T), dim3(GP_TT), pl.lds_solve, s, a, bc, sg);
    int rc = vg_check_launch("gp_gain_fwd (tiled: prelude, covariance)");
    if (rc) return rc;
    for (int p = 0; p < T; ++p) {
        vg_launch(gain_potrf_diag_k, dim3(C), dim3(GP_TT), pl.lds_diag, s, a, p);
        if (p + 1 < T) {
            const int nt = T - 1 - p, per = max(nt * (nt + 1) / 2, T);
            vg_launch(gain_potrf_panel_k, dim3(C * T), dim3(GP_TT), pl.lds_solve, s, a, p);
            vg_launch(gain_potrf_update_k, dim3(C * per), dim3(GP_TT), pl.lds_solve, s, a, p, per);
        }
    }
    rc = vg_check_launch("gp_gain_fwd (tiled: Cholesky)");
    if (rc) return rc;
    vg_launch(gain_sample_k, dim3(C * T), dim3(GP_TT), 0, s, a);
    vg_launch(gain_hrf_k, dim3(C * T), dim3(GT), 0, s, a, task_var);
    vg_launch(gain_kl_sum_k, dim3(1), dim3(64), 0, s, (const double*)kl_part, C, gp_kl);
    return vg_check_launch("gp_gain_fwd (tiled: gain sample)");
}

int gain_bwd_tiled(const vg_gain_desc* d, const GainArgs& a, const float* g_tv, const float* g_kl, float* G32, hipStream_t s) {
    const GainPlan pl = gain_plan(d->B, true);
    const int C = d->C, T = pl.nslabs;
    vg_launch(gain_bwd_p1_k, dim3(C * T), dim3(GP_TT), pl.lds_p1, s, a, g_tv);
    vg_launch(gain_trsm_tiled_k, dim3(C * T), dim3(GP_TT), pl.lds_solve, s, a, 0);          // X = L^-T Phi          (column slabs)
    vg_launch(gain_trsm_tiled_k, dim3(C * T), dim3(GP_TT), pl.lds_solve, s, a, 1);          // X L^-1 = (L^-T X^T)^T (row slabs, in place)
    vg_launch(gain_sym_k, dim3(C * T * (T + 1) / 2), dim3(GP_TT), pl.lds_solve, s, a);
    vg_launch(gain_bwd_rows_k, dim3(C * T), dim3(GP_TT), pl.lds_rows, s, a);
    vg_launch(gain_bwd_fin_k, dim3(C), dim3(GP_TB), pl.lds_main, s, a, g_kl, G32);
    return vg_check_launch("gp_gain_bwd (tiled)");
}

}  // namespace

extern "C" int64_t vg_gp_gain_ws_bytes(int32_t C, int32_t B, int32_t n) {
    if (C <= 0 || B <= 0 || n < 2) return -1;
    if (B > GP_MAXB) {
        vg_set_error("vg_gp_gain_ws_bytes: batch of %d volumes exceeds the gain block's limit of %d volumes per joint draw", (int)B, GP_MAXB);
        return -1;
    }
    GpLayout w = gp_layout(B, n);
    return (int64_t)(w.total * C + C + 8) * (int64_t)sizeof(double);       // C slabs + the per-covariate KL terms
}

extern "C" int vg_gp_gain_plan(const vg_gain_desc* d, int32_t forced_tiled, int32_t* out, int32_t n_out) {
    if (!out || n_out < VG_GAIN_PLAN_LEN) { vg_set_error("vg_gp_gain_plan: out must hold %d values", VG_GAIN_PLAN_LEN); return VG_ERR_ARG; }
    const int rc = check(d, "vg_gp_gain_plan");
    if (rc) return rc;
    const GainPlan p = gain_plan(d->B, forced_tiled != 0);
    const int32_t rec[VG_GAIN_PLAN_LEN] = {p.path, p.threads, p.panel, p.npanels, p.last_panel, p.slab, p.nslabs, p.last_slab,
                                           (int32_t)p.lds_fwd, (int32_t)p.lds_bwd, p.launches_fwd, p.launches_bwd};
    for (int i = 0; i < VG_GAIN_PLAN_LEN; ++i) out[i] = rec[i];
    return VG_OK;
}

// forced = 1: the tiled path at any batch (vg_gp_gain_fwd_tiled); otherwise by batch size
static int gain_fwd(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu, const float* covariates,
                    int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws, float* task_var, float* gp_kl,
                    double* beta_mean, double* beta_cov, double* f_bar, double* Sigma, void* stream, bool forced, const char* who) {
    int rc = check(d, who);
    if (rc) return rc;
    if (!table || !params || !covariates || !eps_beta || !ws || !task_var || !gp_kl || (d->hrf_taps > 0 && !hrf_taps)) {
        vg_set_error("%s: null argument", who); return VG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    GpLayout w = gp_layout(d->B, d->n);
    double* wsd = (double*)ws;
    double* kl_part = wsd + (size_t)w.total * d->C;
    GainArgs a = mk_args(d, table, params, xu, covariates, ld_cov, eps_beta, hrf_taps, wsd);
    const GainPlan pl = gain_plan(d->B, forced);
    if (pl.path == 2) return gain_fwd_tiled(d, a, kl_part, task_var, gp_kl, beta_mean, beta_cov, f_bar, Sigma, s);
    if (pl.path == 0) vg_launch(gain_fwd_k<GP_T>, dim3(d->C), dim3(pl.threads), pl.lds_main, s, a, task_var, kl_part, beta_mean, beta_cov, f_bar, Sigma);
    else vg_launch(gain_fwd_k<GP_TB>, dim3(d->C), dim3(pl.threads), pl.lds_main, s, a, task_var, kl_part, beta_mean, beta_cov, f_bar, Sigma);
    rc = vg_check_launch("gp_gain_fwd");
    if (rc) return rc;
    vg_launch(gain_kl_sum_k, dim3(1), dim3(64), 0, s, (const double*)kl_part, (int)d->C, gp_kl);
    return vg_check_launch("gp_gain_kl_sum");
}

static int gain_bwd(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu, const float* covariates,
                    int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws, const float* g_task_var,
                    const float* g_gp_kl, float* flat_grads, void* stream, bool forced, const char* who) {
    int rc = check(d, who);
    if (rc) return rc;
    if (!table || !params || !covariates || !eps_beta || !ws || !g_task_var || !g_gp_kl || !flat_grads) {
        vg_set_error("%s: null argument", who); return VG_ERR_ARG;
    }
    GainArgs a = mk_args(d, table, params, xu, covariates, ld_cov, eps_beta, hrf_taps, (double*)ws);
    hipStream_t s = (hipStream_t)stream;
    const GainPlan pl = gain_plan(d->B, forced);
    if (pl.path == 2) return gain_bwd_tiled(d, a, g_task_var, g_gp_kl, flat_grads, s);
    if (pl.path == 0) {
        vg_launch(gain_bwd_k<GP_T, 0>, dim3(d->C), dim3(pl.threads), pl.lds_main, s, a, g_task_var, g_gp_kl, flat_grads);
        return vg_check_launch("gp_gain_bwd");
    }
    // large batches: Phi -> L^-T Phi -> (.) L^-1 -> the rest; each solve as slabs of pl.slab right-hand sides, a workgroup each
    vg_launch(gain_bwd_k<GP_TB, 1>, dim3(d->C), dim3(pl.threads), pl.lds_main, s, a, g_task_var, g_gp_kl, flat_grads);
    vg_launch(gain_trsm_k, dim3(d->C * pl.nslabs), dim3(pl.threads), pl.lds_solve, s, a, 0);   // X = L^-T Phi          (column slabs)
    vg_launch(gain_trsm_k, dim3(d->C * pl.nslabs), dim3(pl.threads), pl.lds_solve, s, a, 1);   // X L^-1 = (L^-T X^T)^T (row slabs, in place)
    vg_launch(gain_bwd_k<GP_TB, 2>, dim3(d->C), dim3(pl.threads), pl.lds_main, s, a, g_task_var, g_gp_kl, flat_grads);
    return vg_check_launch("gp_gain_bwd (large batch)");
}

extern "C" int vg_gp_gain_fwd(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                              const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                              float* task_var, float* gp_kl, double* beta_mean, double* beta_cov, double* f_bar, double* Sigma,
                              void* stream) {
    return gain_fwd(d, table, params, xu, covariates, ld_cov, eps_beta, hrf_taps, ws, task_var, gp_kl, beta_mean, beta_cov, f_bar, Sigma,
                    stream, false, "vg_gp_gain_fwd");
}

extern "C" int vg_gp_gain_bwd(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                              const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                              const float* g_task_var, const float* g_gp_kl, float* flat_grads, void* stream) {
    return gain_bwd(d, table, params, xu, covariates, ld_cov, eps_beta, hrf_taps, ws, g_task_var, g_gp_kl, flat_grads, stream, false,
                    "vg_gp_gain_bwd");
}

extern "C" int vg_gp_gain_fwd_tiled(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                                    const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                                    float* task_var, float* gp_kl, double* beta_mean, double* beta_cov, double* f_bar, double* Sigma,
                                    void* stream) {
    return gain_fwd(d, table, params, xu, covariates, ld_cov, eps_beta, hrf_taps, ws, task_var, gp_kl, beta_mean, beta_cov, f_bar, Sigma,
                    stream, true, "vg_gp_gain_fwd_tiled");
}

extern "C" int vg_gp_gain_bwd_tiled(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                                    const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                                    const float* g_task_var, const float* g_gp_kl, float* flat_grads, void* stream) {
    return gain_bwd(d, table, params, xu, covariates, ld_cov, eps_beta, hrf_taps, ws, g_task_var, g_gp_kl, flat_grads, stream, true,
                    "vg_gp_gain_bwd_tiled");
}
