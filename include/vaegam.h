/* vaegam.h -- C ABI of libvaegam_hip.so: the MI355X (gfx950) kernels under the VAE-GAM train step.
 *
 * The reference (dannyfa/VAE-GAM) is pure Python on PyTorch and has no FFI: every entry point
 * below replaces a group of ATen calls made from `VAE.forward` / `loss.backward()` /
 * `optimizer.step()`; the reference lines are cited per function.  Conventions:
 *   - every pointer is a DEVICE pointer into memory owned by the caller (PyTorch tensors);
 *     the library allocates nothing persistent and frees nothing;
 *   - every launch is asynchronous on the `stream` handed in (a hipStream_t passed as void*);
 *   - return value: 0 = OK, non-zero = vg_status; text via vg_last_error(); no exceptions;
 *   - activations are fp32, NCDHW, contiguous.  Layers store PRE-activation values; the
 *     consumer applies ReLU and the batch-norm affine when it loads them (`vg_prologue`).
 *     Rectified hand-off: a forward launch with `relu_out` set stores max(y, 0) instead.  Every
 *     consumer of such a tensor rectifies it or tests its sign (relu(relu(p)) == relu(p),
 *     relu(p) > 0 <=> p > 0), so nothing downstream changes by a bit, and a consumer without a
 *     batch-norm affine may then be launched with relu_in = 0, i.e. without any prologue.
 *     Statistics partials (stats_relu = 1) are the same with and without relu_out.
 *   - "group": the decoder runs C+1 one-hot variants in one launch (sample n -> group
 *     n / per_group); batch-norm statistics are kept per group (vae_reg_GP.py:330,343 call
 *     decode() separately per variant, each with its own batch statistics).
 */
#ifndef VAEGAM_H
#define VAEGAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vg_conv_desc {
    int32_t N;                 /* samples in this launch */
    int32_t CI, CO;            /* channels of the tensor read / written by THIS launch */
    int32_t ID, IH, IW;        /* spatial size of the tensor read */
    int32_t OD, OH, OW;        /* spatial size of the tensor written */
    int32_t KD, KH, KW;        /* kernel */
    int32_t stride;            /* 1 or 2 */
    int32_t pad_d, pad_h, pad_w; /* corr: leading zero padding of the input; tconv: ConvTranspose3d padding */
    int32_t relu_in;           /* prologue: max(x,0) on load */
    int32_t per_group;         /* samples per affine group for in_scale/in_shift ([N/per_group][CI]) */
    int32_t relu_out;          /* forward launches: store max(y, 0) instead of y (see "rectified hand-off" below); ignored with mask_src */
} vg_conv_desc;

/* library identity / errors */
int         vg_version(void);
const char* vg_last_error(void);

/* y[n][co][o] = bias[co] + sum_{ci,k} P(x)[n][ci][o*stride + k - pad] * wpk[ci][k][co]
 * (zero outside the input).  P = prologue (ReLU, then x*in_scale[g][ci]+in_shift[g][ci]).
 * Replaces F.conv3d forward (vae_reg_GP.py:238-242), ConvTranspose3d stride-1 forward with a
 * flipped repacked kernel (:260,262,264) and the data gradients of ConvTranspose3d (autograd
 * of :260-264).  If mask_src != NULL the result is multiplied by (mask_src[same index] > 0):
 * the ReLU backward of the producer layer fused into the data-gradient epilogue. */
int vg_corr3d(const vg_conv_desc* d, const float* x, const float* wpk, const float* bias,
              const float* in_scale, const float* in_shift, const float* mask_src, float* y, void* stream);

/* stride-2 transposed convolution, gather form:
 * y[n][co][o] = bias[co] + sum_{ci,k : (o+pad-k) even} P(x)[n][ci][(o+pad-k)/2] * wpk[ci][k][co].
 * Replaces ConvTranspose3d stride-2 forward (vae_reg_GP.py:261,263) and the data gradient of
 * the stride-2 Conv3d layers (autograd of :239,241). mask_src as above. */
int vg_tconv3d_s2(const vg_conv_desc* d, const float* x, const float* wpk, const float* bias,
                  const float* in_scale, const float* in_shift, const float* mask_src, float* y, void* stream);
/* vg_tconv3d_s2 that ALSO accumulates the batch statistics the NEXT layer's BatchNorm3d needs (vae_reg_GP.py:216-218,
 * 254-264: bnt3 after convt2, bnt5 after convt4) while the outputs are still in registers: per (group, channel) partial
 * [sum, sum of squares] of relu?(y), one pair per wavefront, laid out for vg_bn_stats_from_parts:
 *   stats_part[((g*CO + c)*chunks + k)*2 + {0,1}],  chunks = vg_tconv3d_s2_stats_chunks(d, stats_per_group).
 * Saves the separate full-tensor read of vg_bn_stats. */
int64_t vg_tconv3d_s2_stats_chunks(const vg_conv_desc* d, int32_t stats_per_group);
int vg_tconv3d_s2_stats(const vg_conv_desc* d, const float* x, const float* wpk, const float* bias,
                        const float* in_scale, const float* in_shift, float* y, int32_t stats_per_group,
                        int32_t stats_relu, double* stats_part, void* stream);

/* The partials vg_tconv3d_s2_stats would have written for the layer `d`, taken from its output y alone (d: N, CO, OD/OH/OW, pad_*,
 * relu_out are read): the same thread mapping, summation order and chunk layout, so they are bit for bit the fused launch's whatever
 * kernel produced y.  For a y that vg_conv_mm computed (same values, another reduction order in its own partials): the consuming
 * batch norm then sees exactly the statistics of the register-tiled engine.  stats_relu = 0 on a rectified y is VG_ERR_ARG. */
int vg_tconv3d_s2_stats_of(const vg_conv_desc* d, const float* y, int32_t stats_per_group, int32_t stats_relu,
                           double* stats_part, void* stream);

/* What vg_corr3d / vg_tconv3d_s2 (stats_per_group > 0: vg_tconv3d_s2_stats) would launch for the descriptor: nothing is launched and no
 * tensor memory is touched.  The record comes from the launchers' own planners, at the point where they would launch.
 * has_prologue: the launch would be given in_scale / in_shift (d->relu_in is read from the descriptor); a mask_src changes no choice.
 * out[0 .. VG_CONV_PLAN_LEN):
 *    0 family (0 direct: corr3d_direct_k, 1 plane: corr3d_plane_k, 2 tconv: tconv3d_s2_k)
 *    1 COT  2 KD  3 KH  4 KW  5 S  6 TDt  7 THt  8 TW  9 COC  10 NOPRO    the kernel instance (outputs per thread TDt x THt x TW x COT
 *                                                                         channels; COC: compile-time CO, 0 = run-time; tconv: S 2, brick 2x2x2)
 *   11 small                                                              the dispatcher's few-outputs switch
 *   12 BW  13 BH  14 BD                                                   threads of a block along w / h / d (TWG, TH, TD; tconv: TJW, TJH, TJD)
 *   15 tilesW  16 tilesH  17 tilesD                                       blocks per sample along w / h / d (plane: 1, nhb, tilesD)
 *   18 threads  19 grid_x  20 grid_y  21 grid_z
 *   plane only (else 0):
 *   22 LD  23 CCH  24 chunks  25 nbuf                                     input planes staged per channel, channels per chunk, chunks, buffers
 *   26 OHB  27 nhb  28 LH  29 lplane                                      output rows per row slab, slabs, staged input rows, LDS plane pitch
 *   30 ch_floats  31 lds_bytes                                            LDS floats per channel slot, dynamic LDS of the block
 *   tconv only (else 0):
 *   32 JD  33 JH  34 JW                                                   2x2x2 bricks per dimension
 *   35 stats_chunks                                                       vg_tconv3d_s2_stats_chunks(d, stats_per_group); 0 without statistics
 * n_out < VG_CONV_PLAN_LEN returns VG_ERR_ARG; every descriptor the launcher refuses returns the launcher's status (VG_ERR_ARG,
 * VG_ERR_UNSUPPORTED) with the same vg_last_error() text. */
#define VG_CONV_PLAN_LEN 36
int vg_corr3d_plan(const vg_conv_desc* d, int32_t has_prologue, int32_t* out, int32_t n_out);
int vg_tconv3d_s2_plan(const vg_conv_desc* d, int32_t has_prologue, int32_t stats_per_group, int32_t* out, int32_t n_out);

/* Table-driven implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32): the forward passes and
 * data gradients of the conv / transposed-conv layers with 8 or 16 output channels (vae_reg_GP.py:189-215; replaces F.conv3d /
 * F.conv_transpose3d and their autograd data gradients, like vg_corr3d / vg_tconv3d_s2, for the launches that are real contractions).
 * The host describes the layer as a position grid + window-offset tables (vae_gam_amd/ops.py: mm_plan):
 *   16 matrix rows = (16 / CO) replicas x CO output channels;  columns = 16 consecutive positions (pd, ph, pw) of a block's grid of
 *   PD x PH x PW positions;  class q (1 for correlations, the (rd, rh) output parities of a stride-2 transposed conv) contributes
 *   ks[q] k-steps of 4 window offsets per input channel.
 *   a_img [sum_q CI*ks[q]][64]: A operands, lane l = row (l & 15), offset 4*step + (l >> 4)  -- gathered from the weights by vg_gather_f32;
 *   tau   [sum_q ks[q]][4] int32: the window offset dd*IH*IW + dh*IW + dw of (step, kk);  dlt [sum_q ks[q]][4][3] int32: (dd, dh, dw).
 *   position (pd, ph, pw) reads input element (pd*sdi + dd, ph*shi + dh, pw*swi + dw) (zero outside the tensor) and writes output
 *   (pd*sdo + od0[q], ph*sho + oh0[q], pw*swo + ow0[q] + replica).
 *   Block (bd, bh) of a sample works on position planes [bd*PD, +PD) x rows [bh*PHB, +PHB) and stages, cc channels at a time, the rows
 *   [bh*PHB*shi + hlo, ...+ (PHB-1)*shi + hhi] of input planes [bd*PD*sdi + d0, + LD) (LDS-DMA, one contiguous span per plane; dbuf: double-buffered).
 * bias / in_scale / in_shift / mask_src / stats_*: as vg_corr3d / vg_tconv3d_s2_stats (stats chunks: vg_conv_mm_stats_chunks).
 * co_tot: 16 output channels of a stride-2 transposed conv have no free replica rows for the column pair, so such a layer runs as two
 *   halves of CO = 8 channels through the 4-class path (co_tot = 16); co_tot / CO must be 1, or 2 with CO == 8 (else VG_ERR_ARG). */
typedef struct vg_mm_desc {
    int32_t N, CI, CO;
    int32_t ID, IH, IW, OD, OH, OW;
    int32_t nq, ks[4];
    int32_t PDT, PH, PW, PD;
    int32_t sdi, shi, swi, d0, LD, cc;
    int32_t sdo, sho, swo, od0[4], oh0[4], ow0[4];
    int32_t relu_in, per_group, tpc, slack;
    int32_t dbuf;              /* 1: input planes double-buffered (copy of unit u+1 behind unit u's matrix work); 0: single buffer, half the LDS */
    int32_t PHB;               /* position rows per block (a block = PD planes x PHB rows x PW columns); 0 or >= PH: whole planes */
    int32_t hlo, hhi;          /* smallest / largest row offset dh in the window-offset table: which input rows a row slab stages */
    int32_t waves;             /* wavefronts per workgroup: 8 or 4 (4: half the tile, twice the co-resident workgroups per CU) */
    int32_t relu_out;          /* as vg_conv_desc.relu_out */
    int32_t co_tot;            /* channels of y, mask_src and the statistics; 0 = CO.  2 * CO (CO == 8 only): the launch runs the layer as
                                  two channel halves -- a_img holds the halves' images back to back, a block of the grid owns channels
                                  [8h, 8h + 8); the partials are laid out as for CO = co_tot */
} vg_mm_desc;
int64_t vg_conv_mm_stats_chunks(const vg_mm_desc* d, int32_t stats_per_group);
int vg_conv_mm(const vg_mm_desc* d, const float* x, const float* a_img, const int32_t* tau, const int32_t* dlt, const float* bias,
               const float* in_scale, const float* in_shift, const float* mask_src, float* y, int32_t stats_per_group,
               int32_t stats_relu, double* stats_part, void* stream);
/* dst[e] = idx[e] >= 0 ? src[idx[e]] : 0  -- builds every layer's A image from the flat fp32 parameter buffer in one launch per step */
int vg_gather_f32(const float* src, const int32_t* idx, float* dst, int64_t n, void* stream);

/* weight gradient:  dw[cb][ca][k] = sum_{n,p} PB(b)[n][cb][p] * PA(a)[n][ca][p*stride + k - pad]
 * b: [N][CB][PD][PH][PW], a: [N][CA][AD][AH][AW] (zero outside).  For a Conv3d layer b = dy,
 * a = layer input (prologue on a); for a ConvTranspose3d layer b = layer input (prologue on b),
 * a = dy.  dw comes out in the layer's own weight layout.  Replaces autograd's conv weight
 * gradients.  `ws` is caller workspace of vg_wgrad3d_ws_bytes() bytes.
 * Supported: CB <= 16, PW <= 128 and one of (kernel, CA, stride, padding):
 *   3x3x3, CA 1,  stride 1,      no padding
 *   3x3x3, CA 8,  stride 1 or 2, no padding
 *   3x3x3, CA 16, stride 1 or 2, no padding;  stride 2 also with padding
 *   5x3x3 or 4x4x4, CA 8, stride 2, no padding, CB == 8
 * Without padding every window must lie inside `a`: (P - 1) * stride + K <= A along each axis.  Anything else returns
 * VG_ERR_UNSUPPORTED (vg_wgrad3d_ws_bytes: -1) with vg_last_error() naming the descriptor. */
typedef struct vg_wgrad_desc {
    int32_t N, CB, CA;
    int32_t PD, PH, PW;        /* spatial size of b */
    int32_t AD, AH, AW;        /* spatial size of a */
    int32_t KD, KH, KW;
    int32_t stride;
    int32_t pad_d, pad_h, pad_w;
    int32_t pro_on_a;          /* 1: prologue applies to a, 0: to b */
    int32_t relu_in;
    int32_t per_group;
} vg_wgrad_desc;
int64_t vg_wgrad3d_ws_bytes(const vg_wgrad_desc* d);
/* accumulate != 0: dw += result (lets the caller point dw at the parameter's .grad and skip a separate add) */
int vg_wgrad3d(const vg_wgrad_desc* d, const float* a, const float* b, const float* in_scale,
               const float* in_shift, float* ws, float* dw, int32_t accumulate, void* stream);

/* The same contraction kept PER BATCH-NORM GROUP (g = n / per_group), plus one extra row: out[g][cb][ca*KVOL + tap] for cb < CB is
 * group g's share of dw; row cb == CB is the contraction of `a` with a constant-one position channel, i.e. the per-tap sums of the
 * window tensor over the positions each tap meets.  Called with in_scale = rstd, in_shift = -mean*rstd (the prologue then produces the
 * NORMALISED activation) it yields everything the batch-norm backward of the layer in front needs (vg_bn_tconv1_sums) without a pass
 * over the data.  Supported: CA == 1, 3x3x3, stride 1, no padding, CB < 16, prologue on b (the decoder's last stage); otherwise
 * VG_ERR_UNSUPPORTED.  out: float[N/per_group][CB+1][CA*KVOL], overwritten.  ws: vg_wgrad3d_grouped_ws_bytes(d) bytes. */
int64_t vg_wgrad3d_grouped_ws_bytes(const vg_wgrad_desc* d);
int vg_wgrad3d_grouped(const vg_wgrad_desc* d, const float* a, const float* b, const float* in_scale,
                       const float* in_shift, float* ws, float* out, void* stream);

/* What vg_wgrad3d (grouped != 0: vg_wgrad3d_grouped) would launch for the descriptor: nothing is launched and no tensor memory is
 * touched.  The record comes from the planner itself, at the point where the workspace queries return.  out[0 .. VG_WGRAD_PLAN_LEN):
 *    0 CA   1 KD   2 KH   3 KW   4 stride   5 PAD   6 DSH          the kernel family (DSH: plane-shift packing)
 *    7 PA   8 UG   9 RES  10 GRP  11 ONE                            the instance of the family
 *   12 TPD 13 TPH 14 nbuf                                           tile (position planes x rows), window-channel slots (CA / 2 / 1)
 *   15 pdblocks  16 nph                                             tiles per sample along depth / rows
 *   17 items  18 grid  19 wave_slabs                                work items, blocks, 1: one slab per wave, 0: one per block
 *   20 ipb  21 grp_items                                            grouped: blocks per group, items per group (else 0)
 *   22 nslabs  23 lds_bytes  24 blocks_per_cu                       slabs in the workspace, LDS per block, the occupancy answer used
 * n_out < VG_WGRAD_PLAN_LEN, a null or malformed descriptor (non-positive sizes, stride other than 1 or 2) return VG_ERR_ARG, as
 * vg_wgrad3d does (the workspace queries answer -1 for those too); for a well-formed descriptor the result is VG_ERR_UNSUPPORTED exactly
 * where the matching workspace query returns -1, and VG_OK otherwise. */
#define VG_WGRAD_PLAN_LEN 25
int vg_wgrad3d_plan(const vg_wgrad_desc* d, int32_t grouped, int32_t* out, int32_t n_out);

/* batch-norm batch statistics (BatchNorm3d(track_running_stats=False), vae_reg_GP.py:194-196,
 * 216-218): for x [N][C][P], group g = n / per_group: mean/var over (per_group samples, P) of
 * relu?(x); writes scale = gamma*rstd, shift = beta - mean*scale, mean, rstd ([G][C] each).
 * ws: caller workspace of vg_bn_ws_bytes(N, C, P, per_group) bytes.
 * If ext_sums != NULL the kernel stops after writing the raw per-(g,c) [sum, sumsq, count]
 * triples there (double[G][C][3]) so the caller can all-reduce them across ranks, and
 * vg_bn_finalize() turns reduced triples into scale/shift/mean/rstd. */
int64_t vg_bn_ws_bytes(int32_t N, int32_t C, int64_t P, int32_t per_group);
/* The launch plan of the streaming kernels behind vg_bn_stats, vg_bn_bwd_reduce, vg_bn_bwd_apply (and, with per_group = N,
 * vg_channel_sum) for these arguments, from the planner the launchers use; nothing is launched.  out = {cp, ns}: cp chunks over
 * the P positions of a sample times ns splits of a group's per_group samples = cp * ns blocks per (group, channel).  Arguments
 * that vg_bn_ws_bytes answers -1 for return VG_ERR_ARG. */
int vg_bn_plan(int32_t N, int32_t C, int64_t P, int32_t per_group, int32_t out[2]);
int vg_bn_stats(const float* x, int32_t N, int32_t C, int64_t P, int32_t per_group, int32_t relu,
                const float* gamma, const float* beta, float eps, void* ws, double* ext_sums,
                float* scale, float* shift, float* mean, float* rstd, void* stream);
int vg_bn_finalize(const double* sums, int32_t G, int32_t C, const float* gamma, const float* beta,
                   float eps, float* scale, float* shift, float* mean, float* rstd, void* stream);
/* vg_bn_stats from per-block partials another kernel produced (vg_tconv3d_s2_stats): fold + finalize.
 * count = elements per (group, channel); ext_sums != NULL: write the raw [sum, sumsq, count] triples there and stop
 * (data-parallel caller all-reduces, then vg_bn_finalize); sums_ws is unused (kept for ABI stability, may be NULL). */
int vg_bn_stats_from_parts(const double* part, int32_t G, int32_t C, int64_t chunks, double count,
                           const float* gamma, const float* beta, float eps, double* ext_sums, double* sums_ws,
                           float* scale, float* shift, float* mean, float* rstd, void* stream);

/* batch-norm backward through h = relu?(p), xe = (h-mean)*rstd*gamma+beta, given dxe (in place):
 *   dgamma_part[g][c] = sum dxe*hhat, dbeta_part[g][c] = sum dxe,
 *   dp = relu'(p) * gamma*rstd * (dxe - mean(dxe) - hhat*mean(dxe*hhat)).
 * Two entry points so a data-parallel caller can all-reduce the (double[G][C][2]) sums between.
 * vg_bn_bwd_apply optionally also returns chsum[c] (+)= sum over samples and positions of dp -- the bias gradient of the
 * layer that produced p (nn.Conv3d / ConvTranspose3d bias, vae_reg_GP.py:189-215) -- from the values it already holds
 * (ws: a vg_bn_ws_bytes workspace; chsum NULL = not wanted). */
int vg_bn_bwd_reduce(const float* dxe, const float* p, int32_t N, int32_t C, int64_t P, int32_t per_group,
                     int32_t relu, const float* mean, const float* rstd, void* ws, double* sums, void* stream);
int vg_bn_bwd_apply(float* dxe_inout, const float* p, int32_t N, int32_t C, int64_t P, int32_t per_group,
                    int32_t relu, const float* gamma, const float* mean, const float* rstd,
                    const double* sums, double count, float* dgamma_part, float* dbeta_part,
                    void* ws, float* chsum, int32_t chsum_accumulate, void* stream);

/* Batch-norm backward FUSED with the data gradient of a one-output-channel 3x3x3 stride-1 ConvTranspose3d behind it -- the
 * decoder's last stage, bnt5 -> convt5 (vae_reg_GP.py:218,264), on the largest activation of the network.  The gradient that
 * reaches the batch norm, dxe[n][c][q] = sum_k dy[n][0][q + k] * w[c][0][k] (what autograd's conv_transpose3d backward / vg_corr3d
 * would write as a C-channel tensor), is recomputed from a dy tile in LDS inside both passes instead of being stored and re-read:
 *   p   [N][C][ID][IH][IW] the stored pre-activation;  dy [N][1][ID+2][IH+2][IW+2];  w [C][27] (the layer's own weight layout);
 *   reduce: sums[g][c] = {sum dxe, sum dxe*hhat}  (double[G][C][2], as vg_bn_bwd_reduce);
 *   apply : dp[N][C][...] = relu'(p) * gamma*rstd * (dxe - mean(dxe) - hhat*mean(dxe*hhat))  (as vg_bn_bwd_apply, out of place),
 *           chsum[c] (+)= per-channel sum of dp (bias gradient of the layer that produced p; NULL = not wanted).
 * ws: vg_bn_tconv1_ws_bytes(N, C, ID, per_group) bytes.  Data-parallel callers all-reduce `sums` between the two calls. */
int64_t vg_bn_tconv1_ws_bytes(int32_t N, int32_t C, int32_t ID, int32_t per_group);
/* plan query of the pair: the LDS bytes a block stages for p [.][C][ID][IH][IW], or -1 (vg_last_error says why) where the pair refuses
 * the geometry -- nothing is launched */
int64_t vg_bn_tconv1_lds_bytes(int32_t C, int32_t ID, int32_t IH, int32_t IW);
int vg_bn_bwd_reduce_tconv1(const float* dy, const float* w, const float* p, int32_t N, int32_t C, int32_t ID, int32_t IH, int32_t IW,
                            int32_t per_group, int32_t relu, const float* mean, const float* rstd, void* ws, double* sums, void* stream);
int vg_bn_bwd_apply_tconv1(const float* dy, const float* w, const float* p, float* dp, int32_t N, int32_t C, int32_t ID, int32_t IH,
                           int32_t IW, int32_t per_group, int32_t relu, const float* gamma, const float* mean, const float* rstd,
                           const double* sums, double count, void* ws, float* chsum, int32_t chsum_accumulate, void* stream);

/* The reduce pass of the pair above WITHOUT reading p or dy again, from the grouped weight gradient of the transposed conv taken
 * against the normalised activation (q = vg_wgrad3d_grouped(...) with in_scale = rstd, in_shift = -mean*rstd; [G][C+1][K], K = 27):
 *   sums[g][c] = { sum_k w[c][k] q[g][C][k],  sum_k w[c][k] q[g][c][k] }         (= {sum dxe, sum dxe*hhat}, double[G][C][2])
 *   dw[c][k] (+)= gamma[c] * sum_g q[g][c][k] + beta[c] * sum_g q[g][C][k]       (the conv's own weight gradient, its layout)
 * (autograd of convt5(bnt5(.)), vae_reg_GP.py:218,264: conv_transpose3d's weight gradient and batch_norm's two reductions). */
int vg_bn_tconv1_sums(const float* q, const float* w, const float* gamma, const float* beta, int32_t G, int32_t C, int32_t K,
                      double* sums, float* dw, int32_t accumulate, void* stream);

/* per-channel sum of a [N][C][P] tensor (bias gradients): out[c] = sum_{n,p} x[n][c][p] */
int vg_channel_sum(const float* x, int32_t N, int32_t C, int64_t P, void* ws, float* out, int32_t accumulate, void* stream);

/* fused GAM accumulate + ELBO + GLM distance (vae_reg_GP.py:380,388-390,400-406).
 *   logits [G=C+1][B][V]: decoder pre-sigmoid outputs (group 0 = base map, group i = effect map i)
 *   gain   [C][B]: task_var per covariate;  x [B][V];  eps [V] float64 (log-precision map);
 *   glm [C][V] fp32 (GLM map of covariate i);
 * outputs: sum_log_prob[B] = sum_v log N(x | x_rec, exp(-eps)),  dist[C][B] = ||cons_ib - glm_i||_2,
 *   optional maps_out [G+1][B][V] = sigmoid(base), cons_1..C, full reconstruction (reconstruct path). */
int64_t vg_gam_ws_bytes(int32_t C, int32_t B, int64_t V);
int vg_gam_elbo_fwd(const float* logits, const float* gain, const float* x, const double* eps,
                    const float* glm, int32_t C, int32_t B, int64_t V, void* ws,
                    float* sum_log_prob, float* dist, float* maps_out, void* stream);
/* backward: given g_slp[B] = dL/dsum_log_prob and g_dist[C][B] = dL/ddist, writes
 *   d_logits[G][B][V] (sigmoid backward fused), d_gain[C][B], d_eps[V] (float64) and, if d_total != NULL,
 *   d_total[0] (+)= the sum of all of d_logits -- the bias gradient of the one-output-channel layer that produced the logits
 *   (convt5, vae_reg_GP.py:215,264), which then needs no pass of its own over the largest gradient tensor. */
int vg_gam_elbo_bwd(const float* logits, const float* gain, const float* x, const double* eps,
                    const float* glm, const float* dist, const float* g_slp, const float* g_dist,
                    int32_t C, int32_t B, int64_t V, void* ws,
                    float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream);

/* Embedded grids: the network runs on a grid G = grid[0..2] that contains the data's native grid N = nat[0..2] at its low corner
 * (nat[a] <= grid[a], row-major volumes, last axis fastest); V_N, V_G = the voxel counts.
 *
 * vg_embed_volumes: out[B][V_G] = x[B][V_N] zero-padded at the high end of each axis; every element of out is written by the one launch. */
int vg_embed_volumes(const float* x, const int32_t* nat, const int32_t* grid, int32_t B, float* out, void* stream);
/* vg_gam_elbo_fwd / _bwd with logits and d_logits [G=C+1][B][V_G] on the grid and x [B][V_N], eps [V_N], glm [C][V_N], d_eps [V_N],
 * maps_out [G+1][B][V_N] on the native grid.  The padding takes no part: sum_log_prob, dist, d_gain and d_total sum native voxels only,
 * d_logits is written as exact zeros there, and nothing of x / eps / glm outside the native tensors is addressed.  The per-voxel
 * arithmetic and the two-stage reductions are those of the plain pair (the same kernels, instantiated with the index decode).
 * ws: vg_gam_ws_bytes(C, B, V_G) bytes.  nat / grid: host arrays of three. */
int vg_gam_elbo_fwd_embed(const float* logits, const float* gain, const float* x, const double* eps,
                          const float* glm, int32_t C, int32_t B, const int32_t* nat, const int32_t* grid, void* ws,
                          float* sum_log_prob, float* dist, float* maps_out, void* stream);
int vg_gam_elbo_bwd_embed(const float* logits, const float* gain, const float* x, const double* eps,
                          const float* glm, const float* dist, const float* g_slp, const float* g_dist,
                          int32_t C, int32_t B, const int32_t* nat, const int32_t* grid, void* ws,
                          float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream);
/* The same pair restricted to a voxel mask: mask [V_N] bytes on the native grid, nonzero = the voxel counts.  A native voxel outside the
 * mask takes no part, exactly like the padding: it adds nothing to sum_log_prob, dist, d_gain or d_total, d_logits is written as exact
 * 0.f and d_eps as exact 0.0 there, and maps_out, when requested, as 0.f (every element of d_logits, d_eps and maps_out is written).
 * nat == grid runs the kernels of the plain pair, any other nat those of the _embed pair, each instantiated with the mask test.
 * ws: vg_gam_ws_bytes(C, B, V_G) bytes. */
int vg_gam_elbo_fwd_masked(const float* logits, const float* gain, const float* x, const double* eps,
                           const float* glm, const uint8_t* mask, int32_t C, int32_t B, const int32_t* nat, const int32_t* grid,
                           void* ws, float* sum_log_prob, float* dist, float* maps_out, void* stream);
int vg_gam_elbo_bwd_masked(const float* logits, const float* gain, const float* x, const double* eps,
                           const float* glm, const uint8_t* mask, const float* dist, const float* g_slp, const float* g_dist,
                           int32_t C, int32_t B, const int32_t* nat, const int32_t* grid, void* ws,
                           float* d_logits, float* d_gain, double* d_eps, float* d_total, int32_t total_accumulate, void* stream);

/* Voxel-wise statistics of the maps and of the fit (an extension; the reference re-reads every per-volume NIfTI for its averages and has
 * no second moments): per-subject running sums over the volumes of a minibatch, straight from the logits, in ONE launch.
 *   logits [C+1][B][V_G], gain [C][B], x [B][V_N]: as vg_gam_elbo_fwd_masked;  subj int32 [B]: the subject slot of each volume;
 *   mask uint8 [V_N] or NULL (every native voxel counts);  nat / grid: host arrays of three, as the _masked pair (nat == grid runs the
 *   instances without the index decode);  acc double [S][K][V_N], read and written, K = vg_gam_stats_slots(C) = 3C + 8.
 * Per volume and voxel, gam_fwd's maps by its own fp32 expressions: base = sigmoid(logit_0), cons_i = gain_i * sigmoid(logit_i),
 * rec = base + sum_i cons_i (in i order), r = x - rec.  Slots of a subject (sums over its volumes; squares and sums formed in fp64 from
 * the fp32 values):
 *   0 .. C+1        sum of base, cons_1..C, rec          C+2 .. 2C+3     sum of their squares
 *   2C+4  sum x     2C+5  sum x^2     2C+6  sum r     2C+7  sum r^2      2C+8 .. 3C+7    sum (r + cons_i)^2
 * One thread owns a voxel of one subject for the whole launch: it folds that subject's volumes in ascending b into registers that
 * start at 0 and then adds each partial to its entry of acc once.  No atomics: two runs give the same bits.  The slab of a subject with
 * no volume in the batch, and every entry of a voxel outside the mask, keep their bits (the padding has no entry).  A subj[b] outside
 * [0, S) is skipped.  Refused: null pointers, C < 0, B <= 0, B > 65535, S <= 0, S > 65535, a nat that does not fit into a grid of less
 * than 2^31 voxels (VG_ERR_ARG); C > 16 (VG_ERR_UNSUPPORTED; vg_gam_stats_slots: -1). */
int32_t vg_gam_stats_slots(int32_t C);
int vg_gam_stats_accumulate(const float* logits, const float* gain, const float* x, const int32_t* subj, const uint8_t* mask,
                            int32_t C, int32_t B, int32_t S, const int32_t* nat, const int32_t* grid, double* acc, void* stream);

/* Sign-flip permutation test with the max-statistic (an extension; host side: MapStatistics.group_permutation): family-wise-error
 * corrected inference on a one-sample map over S subjects, 2 <= S <= 64, without ever forming the [P][V] array of statistics.
 *   m double [S][V]: the subject values;  scale double [V]: 1 / sqrt(S * sum_s m[s][v]^2), formed by the caller; a voxel whose scale is
 *   not > 0 takes no part;  signs uint64 [P]: bit s of word p set flips subject s in permutation p;  tail 0: two-sided, 1: positive,
 *   2: negative;  ws: vg_signflip_ws_bytes(S, V, P) bytes of device scratch.
 * Per permutation p and voxel v, in fp64:
 *   T_p[v] = +0.0, then for s = 0 .. S-1 in that order T = T + (bit s of signs[p] ? -m[s][v] : m[s][v])   (adds only; the sign is
 *   applied exactly, as a multiplication by +-1.0: fused with the add or not, the same bits);
 *   u_p[v] = T_p[v] * scale[v]   (one multiplication; u = t / sqrt(S - 1 + t^2) is strictly increasing in the one-sample t, so ranks
 *   and p-values are those of t);  g(u) = |u| (tail 0), u (tail 1), -u (tail 2), and g' the same function applied to T itself.
 * Outputs:
 *   stat0 [V]    g(T_id[v] * scale[v]) with T_id the sum without flips (formed apart from the sign list); 0 for a voxel taking no part;
 *   maxstat [P]  max over the voxels that take part of g(u_p[v]); a -0.0 enters the maximum as +0.0, so its bits are defined; a voxel
 *                that takes no part adds nothing (not a 0 either: a one-sided maximum of negative values stays negative); with no
 *                voxel taking part at all: -inf;
 *   cnt_unc [V]  int32, the number of p with g'(T_p[v]) >= g'(T_id[v]): compared on the unscaled sums, no rounding involved; P for a
 *                voxel taking no part.
 * m and scale are expected finite.  One lane owns one voxel and keeps its S values in registers; the grid is voxel tiles x chunks of
 * permutations; per-tile maxima and per-chunk counts go to ws and a second launch folds them.  No atomics: two runs give the same bits.
 * Refused, nothing written: null pointers, S < 2, V <= 0, V >= 2^31, P <= 0, P > 2^20, tail outside 0..2 (VG_ERR_ARG); S > 64
 * (VG_ERR_UNSUPPORTED).  vg_signflip_ws_bytes answers -1 for every refused shape. */
int64_t vg_signflip_ws_bytes(int32_t S, int64_t V, int32_t P);
int vg_signflip_maxstat(const double* m, const double* scale, const uint64_t* signs, int32_t S, int64_t V, int32_t P, int32_t tail,
                        void* ws, double* stat0, double* maxstat, int32_t* cnt_unc, void* stream);
/* What vg_signflip_maxstat launches for (S, V, P), from the planner it and vg_signflip_ws_bytes use: host only, nothing is launched, no
 * memory is touched.  out[0 .. VG_SIGNFLIP_PLAN_LEN):
 *   0 SMAX          places of the register array of the instance launched: 8, 16, 32 or 64 for S <= SMAX
 *   1 lanes         lanes per block = voxels per tile (256)
 *   2 tiles         voxel tiles: ceil(V / lanes)
 *   3 chunk         permutations per chunk (a multiple of 16, at least 64; the last chunk holds the rest)
 *   4 chunks        ceil(P / chunk)
 *   5 grid_x, 6 grid_y   of the main launch (tiles, chunks)
 *   7 fold_blocks   grid of the fold launch: ceil(P / lanes) blocks for maxstat, then tiles blocks for cnt_unc
 *   8 lds_bytes     static LDS of the main kernel
 *   9 ws_lo, 10 ws_hi    the workspace bytes, ws_lo + (ws_hi << 31) = tiles * P * 8 (maxima) + chunks * V * 4 (counts)
 * n_out < VG_SIGNFLIP_PLAN_LEN (or out NULL) returns VG_ERR_ARG; a shape vg_signflip_ws_bytes answers -1 for returns the status
 * vg_signflip_maxstat would and leaves the same kind of text in vg_last_error(). */
#define VG_SIGNFLIP_PLAN_LEN 11
int vg_signflip_plan(int32_t S, int64_t V, int32_t P, int32_t* out, int32_t n_out);

/* Batch-norm parameter gradients from vg_bn_bwd_reduce's per-(group, channel) sums:
 *   dgamma[c] (+)= sum_g sums[g][c][1],  dbeta[c] (+)= sum_g sums[g][c][0]   (accumulate != 0 adds into the .grad buffers;
 *   replaces autograd's sum + add launches after torch.nn.BatchNorm3d's backward, vae_reg_GP.py:195-201,216-222). */
int vg_bn_param_grad(const double* sums, int32_t G, int32_t C, float* dgamma, float* dbeta, int32_t accumulate, void* stream);

/* Batch norm ON THE DATA (bn1, vae_reg_GP.py:187-189, 236-238) folded into conv1's backward: with dw_hat = the weight gradient taken
 * against the normalised input xhat = x*rstd + nshift (vg_data_bn_nshift: nshift = -mean*rstd) and db = the bias gradient,
 *   dw[co][ci][t] (+)= gamma[ci]*dw_hat[co][ci][t] + beta[ci]*db[co],   dbias[co] (+)= db[co],
 *   dgamma[ci] (+)= sum_{co,t} w*dw_hat,   dbeta[ci] (+)= sum_co (sum_t w[co][ci][t]) * db[co]       (accumulate != 0: add into). */
int vg_data_bn_nshift(const float* mean, const float* rstd, int32_t n, float* nshift, void* stream);
int vg_data_bn_grads(const float* dw_hat, const float* db, const float* w, const float* gamma, const float* beta,
                     int32_t CO, int32_t CI, int32_t taps, float* dw, float* dbias, float* dgamma, float* dbeta,
                     int32_t accumulate, void* stream);

/* Latent sample + KL of the low-rank Gaussian posterior in one launch (vae_reg_GP.py:321-329, 339-342, 400):
 *   d = exp(a) + 1e-6*[any(exp(a) < 1e-6)],  z = mu + w*eps_w + sqrt(d)*eps_d,
 *   kl[b] = 0.5*(-log(1 + sum w^2/d) - sum log d + sum d + sum w^2 + sum mu^2 - L),
 *   zcat[g*B + b] = [z[b], onehot_G(g)]  (the C+1 decoder inputs, row-major (G*B, L+G)).
 * mu, w, a, eps_d: [B][L]; eps_w: [B]; d_out: [B][L]; flag_out: [1] (the floor that was applied, 0 or 1e-6). */
int vg_latent_fwd(const float* mu, const float* w, const float* a, const float* eps_w, const float* eps_d,
                  int32_t B, int32_t L, int32_t G, float* zcat, float* kl, float* d_out, float* flag_out, void* stream);
/* backward of the above: g_zcat [G*B][L+G] (may be NULL), g_kl [B] (may be NULL) -> g_mu, g_w, g_a [B][L]. */
int vg_latent_bwd(const float* mu, const float* w, const float* d, const float* flag, const float* eps_w, const float* eps_d,
                  const float* g_zcat, const float* g_kl, int32_t B, int32_t L, int32_t G,
                  float* g_mu, float* g_w, float* g_a, void* stream);

/* ELBO assembly (vae_reg_GP.py:406-410): loss[0] = c_kl*sum kl[B] + c_slp*sum slp[B] + c_gp*gp_kl[0] + c_dist*sum dist[CB];
 * backward writes the four constant gradients scaled by g_loss[0].  CB = 0 (no covariates): dist / g_dist may be null. */
int vg_loss_fwd(const float* kl, const float* slp, const float* dist, const float* gp_kl, int32_t B, int32_t CB,
                double c_kl, double c_slp, double c_gp, double c_dist, float* loss, void* stream);
int vg_loss_bwd(const float* g_loss, int32_t B, int32_t CB, double c_kl, double c_slp, double c_gp, double c_dist,
                float* g_kl, float* g_slp, float* g_dist, float* g_gp, void* stream);

/* Projection of the latent means (vae_reg_GP.py:542-583 project_latent, UMAP; host side: vae_gam_amd/latent_projection.py).
 *
 * Exact k nearest neighbours, Euclidean: x [N][D] fp32 row-major, 1 <= D <= 128, 1 <= k <= min(64, N) ->
 *   idx [N][k] int32, dist [N][k] fp32.  Position 0 is the point itself at distance 0; positions 1..k-1 are the k-1 nearest
 *   OTHER points sorted by (distance, index) ascending (ties go to the lower index).  distance = sqrtf(sum_d (x_i[d] - x_j[d])^2),
 *   summed in fp32 over d = 0..D-1 in that order with fused multiply-adds (never the |a|^2 + |b|^2 - 2ab expansion).
 *   ws: vg_knn_ws_bytes(N, D, k) bytes of device scratch (may be NULL when that is 0). */
int64_t vg_knn_ws_bytes(int32_t N, int32_t D, int32_t k);
int vg_knn(const float* x, int32_t N, int32_t D, int32_t k, void* ws, int32_t* idx, float* dist, void* stream);
/* What vg_knn launches for (N, D, k), from the planner vg_knn and vg_knn_ws_bytes use: host only, nothing is launched, no memory is
 * touched.  out[0 .. VG_KNN_PLAN_LEN):
 *   KB (places of the register list of the instance launched: 8, 16, 32 or 64 for k-1 <= KB; 0 when k = 1, where only the merge
 *   kernel runs and writes position 0), S (candidate splits launched: the grid's y of the partial kernel), chunk (candidates per
 *   split, a multiple of 16), Dp (D padded to a multiple of 16), query blocks (of 256 queries: the grid's x of both kernels),
 *   candidates in the last split (N - (S-1)*chunk), dynamic LDS bytes of the partial kernel (0 when KB = 0).
 * The workspace is S*(k-1)*N*8 bytes.  n_out < VG_KNN_PLAN_LEN (or out NULL) returns VG_ERR_ARG; a shape vg_knn_ws_bytes answers -1
 * for returns VG_ERR_ARG and leaves the same kind of text in vg_last_error(). */
#define VG_KNN_PLAN_LEN 7
int vg_knn_plan(int32_t N, int32_t D, int32_t k, int32_t* out, int32_t n_out);

/* Fuzzy simplicial set of each neighbour row (umap-learn smooth_knn_dist + compute_membership_strengths, local_connectivity 1,
 * bandwidth 1), in fp64: rho_i = smallest non-zero dist in row i (0 if none); sigma_i by at most 64 bisection steps to
 * |sum_{j=1..k-1} f(d_ij - rho_i) - log2 k| < 1e-5 (f(t) = exp(-t/sigma) for t > 0, else 1; lo 0, hi inf, start 1, doubling while
 * hi = inf), floored at 1e-3 * (mean of row i if rho_i > 0, else the mean of all N*k distances: a fixed-order reduction);
 * w_ij = 0 for idx_ij = i, 1 if d_ij - rho_i <= 0 or sigma_i = 0, else exp(-(d_ij - rho_i)/sigma_i).
 * dist, idx: vg_knn's output [N][k]; ws: 256 doubles of device scratch; rho, sigma [N], w [N][k] fp32. */
int vg_umap_fuzzy(const float* dist, const int32_t* idx, int32_t N, int32_t k, double* ws, float* rho, float* sigma, float* w,
                  void* stream);

/* One synchronous (Jacobi) epoch of the 2-D UMAP layout: y_out = Y_{n+1} from y_in = Y_n ([N][2] fp32, distinct buffers).
 * Graph: symmetric CSR rowptr [N+1], col [nnz], eps [nnz] = epochs_per_sample = max(W) / w_e.  For row i, entry e = (i, j) in CSR
 * order, at epoch n = `epoch` (alpha = 1 - n/n_epochs in fp32):
 *   due iff n >= 1 and floor(n/eps_e) > floor((n-1)/eps_e)  (in fp64);
 *   attraction (d2 = |y_i - y_j|^2 > 0): c = -2ab d2^(b-1) / (a d2^b + 1); y_i += alpha*clip(c*(y_i - y_j), +-4), added TWICE (once as
 *     head of (i, j), once as the other end of (j, i): W is symmetric, so (j, i) is due at the same epochs);
 *   then negative_sample_rate (<= 31) samples s = 0, 1, ...: k = H mod N with
 *     H = splitmix64_finaliser(((uint64)n << 44 | (uint64)e << 5 | s) + seed * 0x9E3779B97F4A7C15)   (all mod 2^64),
 *     splitmix64_finaliser(z): z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; z ^ z>>31;
 *     skipped if k = i or d2 = |y_i - y_k|^2 = 0, else c = 2b / ((0.001 + d2)(a d2^b + 1)); y_i += alpha*clip(c*(y_i - y_k), +-4).
 * All arithmetic fp32 (a, b rounded to fp32, powf), no fused multiply-adds; every contribution is added to y_i in the order listed.
 * Limits: nnz < 2^39, n_epochs < 2^20, 0 <= epoch < n_epochs. */
int vg_umap_layout_epoch(const int32_t* rowptr, const int32_t* col, const float* eps, const float* y_in, int32_t N, int32_t nnz,
                         int32_t epoch, int32_t n_epochs, double a, double b, int32_t negative_sample_rate, uint64_t seed,
                         float* y_out, void* stream);

/* Fully connected layers (vae_reg_GP.py:197-210 fc1..fc8, :243-259 their use; replaces torch.nn.Linear / F.relu and what autograd
 * derives from them): one strided product on the matrix cores,
 *   C[z][m][n] (+)= epilogue( sum_k A[z](m,k) * B[z](k,n) ),   m < M, n < N, k < K, z < batch,
 * A(m,k) at A + z*a_sb + m*a_sm + k*a_sk, B(k,n) at B + z*b_sb + k*b_sk + n*b_sn (element strides; one stride of each operand must
 * be 1), C rows contiguous: C + z*c_sb + m*c_sm + n.  flags:
 *   VG_FC_A_RELU  A <- max(A, 0)                       VG_FC_A_MASK  A <- A * [amask > 0]   (amask laid out as A)
 *   VG_FC_B_RELU  B <- max(B, 0)                       VG_FC_B_ONES  B gets a column n = N of ones: sum_k A(m,k) goes to cx[z*cx_sb + m]
 *   VG_FC_C_BIAS  + bias[z*bias_sb + n]                VG_FC_C_RELU  max(., 0)
 *   VG_FC_C_MASK  * [cmask > 0]  (cmask laid out as C) VG_FC_C_ACCUM add into C / cx instead of overwriting
 * ksplit > 1 (batch must be 1): the reduction is cut into ksplit pieces of ceil(K/ksplit) rounded up to 64 indices (none may be
 * empty); partial products go to ws (vg_fc_ws_bytes) and a second launch sums them in a fixed order and applies the epilogue.
 * Forward of a layer: A = x, B(k,n) = W[n][k], BIAS (+RELU).  Data gradient: A = dy (A_MASK with the layer's output if it has a ReLU),
 * B(k,n) = W[k][n].  Weight + bias gradient: A(m,k) = dy[k][m], B(k,n) = x[k][n], B_ONES, C = dW, cx = db, C_ACCUM. */
enum { VG_FC_A_RELU = 1, VG_FC_A_MASK = 2, VG_FC_B_RELU = 4, VG_FC_B_ONES = 8, VG_FC_C_BIAS = 16, VG_FC_C_RELU = 32, VG_FC_C_MASK = 64,
       VG_FC_C_ACCUM = 128 };
typedef struct vg_fc_desc {
    int32_t M, N, K, batch;
    int64_t a_sm, a_sk, a_sb;
    int64_t b_sk, b_sn, b_sb;
    int64_t c_sm, c_sb;
    int64_t bias_sb, cx_sb;
    int32_t ksplit, flags;
} vg_fc_desc;
int64_t vg_fc_ws_bytes(const vg_fc_desc* d);
int vg_fc_gemm(const vg_fc_desc* d, const float* A, const float* amask, const float* B, const float* bias, const float* cmask,
               float* C, float* cx, float* ws, void* stream);
/* Up to 4 independent products in ONE launch (a layer's data gradient and its weight + bias gradient: these products are latency-bound,
 * a launch costs as much as the arithmetic); unused pointers NULL. */
typedef struct vg_fc_job {
    vg_fc_desc d;
    const float *A, *amask, *B, *bias, *cmask;
    float *C, *cx, *ws;
} vg_fc_job;
int vg_fc_gemm_jobs(const vg_fc_job* jobs, int32_t njobs, void* stream);

/* What vg_fc_gemm_jobs (vg_fc_gemm: njobs = 1) would launch for these jobs: nothing is launched and no memory is touched, the
 * pointers are read for their 16-byte alignment only.  The record comes from the function that builds the launch for
 * vg_fc_gemm_jobs.  out[0 .. VG_FC_PLAN_LEN):
 *    0 tile  1 grid  2 reduce_blocks  3 njobs                       tile edge (32: fc_gemm_k<1>, 64: fc_gemm_k<2>; one for all jobs),
 *                                                                   blocks of the product launch, blocks of the split-K reduction
 *                                                                   (0: no second launch), jobs
 *   per job j, from out[4 + 8*j]:
 *    0 a_vec  1 b_vec                                               load form of A / B (0 dwords, 1 16 bytes along k, 2 16 bytes
 *                                                                   along m / n): the body fc_body<W, a_vec, b_vec> the job runs
 *    2 big                                                          the job's own vote for 64 x 64 (>= 768 tiles of 32 x 32); the launch
 *                                                                   runs 64 x 64 only if every job votes for it
 *    3 kchunk                                                       reduction indices per split piece (a multiple of 64)
 *    4 gx  5 gy                                                     tiles along m and n (n counts the ones column) at the launch's tile
 *    6 first  7 blocks                                              the job's first block and block count (gx * gy * (ksplit or batch))
 *   the records of jobs >= njobs are 0.
 * n_out < VG_FC_PLAN_LEN (or out NULL) returns VG_ERR_ARG; every job list the launcher refuses returns the launcher's status and leaves
 * the launcher's text in vg_last_error(). */
#define VG_FC_PLAN_LEN 36
int vg_fc_plan(const vg_fc_job* jobs, int32_t njobs, int32_t* out, int32_t n_out);

/* Re-pack every conv / transposed-conv weight of the model into the [ci][tap][co] images vg_corr3d / vg_tconv3d_s2 read,
 * in one launch from the flat fp32 parameter buffer.  segs: device array [nseg][8] of int64
 * {src offset, dst offset, d0, d1, taps, mode, element count, 0} sorted by dst offset; w is [d0][d1][taps];
 * mode 0: out[i1][t][i0] = w[i0][i1][t]; mode 1: out[i0][t][i1] = w[i0][i1][t]; mode 2: as 1 with taps reversed
 * (replaces the permute/flip/contiguous copies that F.conv_transpose3d / autograd do internally). */
int vg_pack_weights(const float* flat_params, float* packed, const int64_t* segs, int32_t nseg, int64_t total, void* stream);

/* batched lower Cholesky factor of [batch][n][n] float64 SPD matrices (n <= 128), one workgroup per matrix
 * in LDS.  Replaces the Cholesky inside MultivariateNormal(beta_mean, beta_cov + 1e-5 I) (vae_reg_GP.py:368)
 * and MultivariateNormal(qu_m, qu_S) (gp.py:51); unlike hipSOLVER's potrf it can be captured into a hipGraph. */
int vg_cholesky_f64(const double* a, double* l, int32_t batch, int32_t n, void* stream);

/* The gain block of one minibatch: for every covariate i the sparse-GP posterior over the minibatch's query points, the gain
 * covariance, its B x B Cholesky factor, the reparameterised gain sample, the HRF along the batch axis and both KL terms
 * (vae_reg_GP.py:345-378 with gp.py:41-110: gp.GP.evaluate_posterior -- kernel build {Knu, Knn, Ku}, Ku solve --,
 * compute_GP_kl, calc_linW_KL, MultivariateNormal(beta_mean, beta_cov + 1e-5 I).rsample(), do_hrf_conv), forward and backward,
 * float64 arithmetic on fp32 inputs.
 *   Batch ranges: 1 <= B <= 1024 one workgroup per covariate (B x B matrix in LDS up to 16, beyond that the blocked Cholesky and
 *   slab solves with a panel / slab in LDS); 1024 < B <= 4096 the TILED path: the same arithmetic spread over at least
 *   C * ceil(B / 64) workgroups per O(B^2) / O(B^3) launch (64 x 64 tiles, a blocked right-looking Cholesky of three launches per
 *   64-column panel, left-looking slab solves); B > 4096 returns VG_ERR_UNSUPPORTED.  vg_gp_gain_fwd_tiled / _bwd_tiled take the
 *   tiled path at any B >= 1 (same arguments, same workspace); a backward call must use the pair of its forward call.
 *   Workspace: vg_gp_gain_ws_bytes = 8 (C (2 B^2 + 4 B n + 7 n^2 + 6 B + 16, rounded up to a multiple of 8) + C + 8) bytes, the same
 *   layout on both paths (about 268 MB per covariate at B = 4096).
 *   Determinism: every sum runs in a fixed order and no float atomics are used; both paths are run-to-run bit-reproducible and can
 *   be captured in a hipGraph (no allocation, no host synchronisation, ordering by launch boundaries only).  The tiled path agrees
 *   with the other to rounding, not bit for bit (different blocking of the same sums).
 *   table  [C][10] int64 (device): {is_gp, is_hrf, gp_index, off_sa, off_logstd, off_qu_m, off_qu_S, off_logkvar, off_log_ls, 0},
 *          offsets = element offsets of that covariate's parameters inside `params` (the flat fp32 parameter buffer);
 *   xu     [#gp][n] fp32 inducing grids (row gp_index);  covariates: element (b, i) at covariates[b*ld_cov + i], B rows (the GLOBAL
 *          batch under data parallelism);  eps_beta [C][B] fp32 standard-normal draws;  hrf_taps [hrf_taps] float64;
 *   ws     caller workspace of vg_gp_gain_ws_bytes(C, B, n) bytes: written by the forward call, read by the backward call.
 * forward outputs: task_var [C][B] fp32 (the gains), gp_kl [1] fp32 (sum over covariates of kl_lin (+ kl_gp)); optional float64
 *   copies for exports / tests (NULL = not wanted): beta_mean [C][B], beta_cov [C][B][B], f_bar [C][B], Sigma [C][B][B]
 *   (f_bar / Sigma rows of non-GP covariates are left untouched).
 * backward: given g_task_var [C][B] fp32 and g_gp_kl [1] fp32, ADDS d loss / d {sa, logstd, qu_m, qu_S, logkvar, log_ls} into
 *   flat_grads (fp32, same offsets as params).  No gradient flows to the covariates or the inducing grids (gp.py:92-101 builds
 *   the distances from Python floats). */
typedef struct vg_gain_desc {
    int32_t C, B, n;           /* covariates, minibatch, inducing points */
    int32_t hrf_taps;          /* 15 (utils.hrf(np.arange(0, 20, 1.4))); 0 = no HRF covariate */
    double jitter_b;           /* 1e-5 (vae_reg_GP.py:368) */
    double jitter_ku;          /* 0 = the reference's plain inverse of Ku (gp.py:107); > 0: Ku + jitter I (unit-variance scale) */
    double prior_var;          /* 10 (gp.py:47) */
} vg_gain_desc;
int64_t vg_gp_gain_ws_bytes(int32_t C, int32_t B, int32_t n);
int vg_gp_gain_fwd(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                   const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                   float* task_var, float* gp_kl, double* beta_mean, double* beta_cov, double* f_bar, double* Sigma, void* stream);
int vg_gp_gain_bwd(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                   const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                   const float* g_task_var, const float* g_gp_kl, float* flat_grads, void* stream);
int vg_gp_gain_fwd_tiled(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                         const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                         float* task_var, float* gp_kl, double* beta_mean, double* beta_cov, double* f_bar, double* Sigma, void* stream);
int vg_gp_gain_bwd_tiled(const vg_gain_desc* d, const int64_t* table, const float* params, const float* xu,
                         const float* covariates, int64_t ld_cov, const float* eps_beta, const double* hrf_taps, void* ws,
                         const float* g_task_var, const float* g_gp_kl, float* flat_grads, void* stream);
/* What vg_gp_gain_fwd / _bwd (forced_tiled != 0: the _tiled pair) launch for this descriptor, from the launchers' own planner: host
 * only, nothing is launched, no memory is touched.  out[0 .. VG_GAIN_PLAN_LEN):
 *   path (0 = one workgroup with the B x B matrix in LDS, 1 = blocked, 2 = tiled), threads per workgroup of the factorisation and
 *   solve kernels, panel width / panels / width of the last panel of the Cholesky, slab width / slabs per covariate / width of the
 *   last slab of the backward solves, the largest dynamic LDS request in bytes of the forward and of the backward launches, the
 *   number of launches of the forward and of the backward call.  (Path 0 is unblocked: one panel and one slab of width B.)
 * n_out < VG_GAIN_PLAN_LEN (or out NULL) returns VG_ERR_ARG; a descriptor the launchers refuse returns their status and leaves their
 * text in vg_last_error(). */
#define VG_GAIN_PLAN_LEN 12
int vg_gp_gain_plan(const vg_gain_desc* d, int32_t forced_tiled, int32_t* out, int32_t n_out);

/* fused Adam (torch.optim.Adam defaults, vae_reg_GP.py:179,429) over one flat buffer:
 * p,g,m,v: n elements of fp32 (is_f64 = 0) or fp64 (is_f64 = 1).  step_size = lr/(1-b1^t),
 * bc2_sqrt = sqrt(1-b2^t) are read from device scalars step_scalars[0..1] so a captured graph can replay
 * with a changing step count.
 * vg_adam_advance keeps that count ON THE DEVICE: state = double[3] {step_size, bc2_sqrt, t}; one launch does
 * t += 1 and refreshes the two scalars (torch.optim.Adam's per-step `step += 1` and bias corrections).  Launched
 * inside the step (and captured with it), so queued replays can never see a later step's scalars. */
int vg_adam_advance(double* state, double lr, double b1, double b2, void* stream);
int vg_adam_step(void* p, const void* g, void* m, void* v, int64_t n, int32_t is_f64,
                 double b1, double b2, double eps, const double* step_scalars, void* stream);

/* gradient guard (opt-in; an extension, the reference has none): global-norm clipping and a non-finite step skip decided ON THE
 * DEVICE, inside the (captured) step, from the optimiser's two flat gradient buffers (g32: n32 fp32 elements, g64: n64 fp64
 * elements; either may be empty: pointer NULL and count 0).
 * vg_grad_guard = two launches: (1) per-block fp64 partial sums of squares of both buffers into ws (vg_grad_guard_ws_bytes);
 * every element belongs to a fixed thread of a fixed block and the grid depends on n32 / n64 only, so the partials and (2) their
 * fixed-order sum are bit-identical from run to run and on every data-parallel rank that holds the same all-reduced buffers: all
 * ranks take the same decision with no further collective.  No floating-point atomics, no arrival counter.  A sum of squares is
 * finite exactly when every element is (squares cannot cancel; an fp64 element beyond 1e154 overflows and counts as non-finite).
 * state = double[VG_GUARD_STATE_LEN], read and written on the device only:
 *   [0] total_norm   sqrt of the last step's sum of squares (inf / nan as it comes)
 *   [1] scale        max_norm > 0: c = max_norm / (total_norm + 1e-6), c > 1 ? 1 : c  (torch.nn.utils.clip_grad_norm_; a nan norm
 *                    gives nan, an inf norm 0, as there); max_norm <= 0 (clipping off): 1
 *   [2] apply        0 when the norm is non-finite and skip_nonfinite != 0, else 1
 *   [3] seen         steps the guard has looked at
 *   [4] skipped      steps with apply = 0
 *   [5] clipped      finite steps with scale < 1
 *   [6] norm_sum     sum of total_norm over the finite steps
 *   [7] norm_max     max of total_norm over the finite steps
 * [3..7] accumulate until the caller zeroes them.  The gradient buffers are NOT scaled: vg_adam_step_guarded multiplies on load.
 * vg_adam_advance_guarded = vg_adam_advance, but t and the two scalars move only when guard[2] != 0 (a skipped step must not
 * advance the bias corrections of the later ones).  vg_adam_step_guarded = vg_adam_step with g * guard[1]; with guard[2] == 0 it
 * returns without touching p, m, v.  With scale = 1 and apply = 1 both give bit-for-bit what the plain entry points give. */
#define VG_GUARD_STATE_LEN 8
int64_t vg_grad_guard_ws_bytes(int64_t n32, int64_t n64);
int vg_grad_guard(const float* g32, int64_t n32, const double* g64, int64_t n64, double max_norm, int32_t skip_nonfinite,
                  void* ws, double* state, void* stream);
int vg_adam_advance_guarded(double* state, double lr, double b1, double b2, const double* guard, void* stream);
int vg_adam_step_guarded(void* p, const void* g, void* m, void* v, int64_t n, int32_t is_f64,
                         double b1, double b2, double eps, const double* step_scalars, const double* guard, void* stream);

/* Device-resident input path (an extension; the reference re-reads the whole 4-D NIfTI of a subject for every sample,
 * DataClass_GP.py:48-51): one launch assembles the minibatch x[B][X][Y][Z] (fp32, C-contiguous, what forward_core takes) for B rows
 * of a data set straight from the raw payloads of the subject files, kept in HBM exactly AS THEY SIT ON DISK (no host transposition,
 * no host conversion) in one byte arena.
 *   files    [#files] vg_vol_file (device): where a file's payload starts in the arena and how to read it.  Element (x, y, z, t) of
 *            the file is the `dtype` value at arena + offset + (x*sx + y*sy + z*sz + t*st) * sizeof(dtype); the only alignment assumed
 *            is that of the element itself (offset a multiple of the element size).  NIfTI is Fortran order (1, X, XY, XYZ); a C-order
 *            .npy of shape (X, Y, Z, T) is (YZT, ZT, T, 1).
 *   row_file, row_vol [N] int32 (device): the file and the volume t of data-set row i;  idx [B] int64 (device): the rows wanted.
 *   x[b] = volume row_vol[idx[b]] of file row_file[idx[b]].  Nothing is clamped: the caller validates idx, row_file and row_vol.
 *   dtype    the NIfTI datatype code every file of the table shares (2 u1, 4 i2, 8 i4, 16 f4, 64 f8, 256 i1, 512 u2, 768 u4), or 0 when
 *            the files differ and each descriptor's own code is read; any other value returns VG_ERR_ARG.
 * Arithmetic (a contract: bit for bit what the host path read_nifti1 -> FMRIDataset.__getitem__ -> ToTensor computes under numpy 2
 * promotion rules; raw = the stored value, byte-swapped first when `swap` is set):
 *   f4 files, everything in fp32:   v = raw;  if scale: v = fl32(fl32(v * (float)slope) + (float)inter)  (two roundings, never fused);
 *                                   x = fl32(v / (float)divisor)               (IEEE division, not a multiplication by a reciprocal)
 *   every other dtype, in fp64:     v = (double)raw;  if scale: v = fl64(fl64(v * slope) + inter);  x = (float)(v / divisor)
 *   `scale` is the reader's own predicate, evaluated by the caller: (slope not in {0, 1} or inter != 0) and slope != 0.
 *   Subnormal results and NaN payloads are outside the contract.
 * Files whose x axis is the faster one (x stride below z stride: NIfTI) are staged through LDS, all x and all z of a few y per workgroup, so
 * that both the loads and the stores of a wavefront are contiguous runs; other layouts (and shapes whose tile does not fit) are read
 * in output order. */
typedef struct vg_vol_file {
    int64_t offset;            /* byte offset of the payload in the arena */
    int64_t sx, sy, sz, st;    /* element strides of x, y, z, t */
    double  slope, inter;      /* scl_slope, scl_inter */
    int32_t dtype;             /* NIfTI datatype code */
    int32_t swap;              /* 1: stored big-endian */
    int32_t scale;             /* 1: apply v * slope + inter */
    int32_t reserved;
} vg_vol_file;
int vg_volume_gather(const void* arena, const vg_vol_file* files, const int32_t* row_file, const int32_t* row_vol, const int64_t* idx,
                     int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t dtype, double divisor, float* x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAEGAM_H */
