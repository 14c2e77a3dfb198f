/* libast_hip.so -- C ABI of the MI355X (gfx950) hot path.
 *
 * The reference (francescobrigante/Audio-Style-Transfer) is pure Python: it has
 * no FFI of its own.  The boundary this library replaces is the set of
 * torch/ATen operator calls made by the reference's nn.Module.forward / loss
 * functions; each entry point cites the reference call site it stands in for.
 * The host side (audio-style-transfer_amd/ast_amd) binds these with ctypes and
 * keeps the reference's Python call surface.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named h_*; the library borrows it
 *     for the duration of the enqueue, allocates nothing, never synchronises and
 *     enqueues on `stream` (a hipStream_t passed as void*), so calls are
 *     hipGraph-capturable;
 *   - return 0 on success, negative on error; ast_last_error() returns the
 *     message (thread-local);
 *   - activations are NHWC with the channel count padded to a multiple of 8;
 *     `dtype` selects their storage / MFMA operand type: AST_F32 (exact f32
 *     MFMA) or AST_BF16 (bf16 MFMA, f32 accumulate); parameters, statistics and
 *     losses are always f32;
 *   - per-clip lengths of a padded inference batch (the ast_*_len entries,
 *     ast_bign_gemm_len) are int32 DEVICE arrays that the kernels read and
 *     clamp, so one captured graph serves every mix of lengths; both decoders
 *     take them.
 */
#ifndef AST_HIP_H
#define AST_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AST_DTYPE_F32 0
#define AST_DTYPE_BF16 1
#define AST_MAX_TAPS 9

int ast_version(void);
const char* ast_last_error(void);

/* Geometry of one gathered (implicit im2col) GEMM.  Rows of the GEMM are the
 * pixels (n, hm, wm) of a logical Hm x Wm grid; tap t reads source pixel
 * (hm*sh + oh + dh[t], wm*sw + ow + dw[t]) (zero outside the tensor) and weight
 * slice wtap[t]; the result goes to destination pixel (hm*dsh + doh, wm*dsw + dow).
 * This one description covers Conv2d forward, its data gradient (one launch per
 * output-parity class for stride 2), ConvTranspose2d forward/backward and
 * nn.Linear (H = W = 1, one tap). */
typedef struct ast_gather_t {
  int32_t N, Hs, Ws, Cs;          /* source NHWC, Cs multiple of 8 */
  int32_t Hm, Wm;                 /* logical pixel grid */
  int32_t sh, sw, oh, ow;         /* source base coordinate */
  int32_t Hd, Wd, Cd;             /* destination NHWC, Cd multiple of 8 */
  int32_t dsh, dsw, doh, dow;     /* destination coordinate */
  int32_t ntaps, wtaps;           /* taps used / taps per weight row */
  int32_t tap[AST_MAX_TAPS];      /* (dh+64) | (dw+64)<<8 | wtap<<16 */
} ast_gather_t;

/* dst[pix][co] (+)= sum_{t,c} src[gather(pix,t)][c] * wgt[co][wtap[t]][c] + bias[co]
 * Replaces: nn.Conv2d fwd/bwd-data (style_encoder.py:50-67, new_decoder.py:29-61),
 * nn.ConvTranspose2d fwd/bwd-data (new_decoder.py:72-96), nn.Linear fwd/bwd-data.
 * flags: an OR of the AST_IGEMM_* bits below; every argument is checked once, before any launch, whichever kernel the plan picks. */
#define AST_IGEMM_ACCUMULATE  1      /* bit 0: add into dst */
#define AST_IGEMM_RELU        2      /* bit 1: ReLU on the stored value */
#define AST_IGEMM_WS_ZEROED   4      /* bit 2: the split-K workspace is already zero (the finish pass hands it back zeroed: a persistent one never needs a memset) */
#define AST_IGEMM_STATS       8      /* bit 3: fused forward statistics, below */
#define AST_IGEMM_BN_SUMS     16     /* bit 4: fused BatchNorm-backward sums: ast_igemm_bn only (ast_igemm clears bits 4 and 5) */
#define AST_IGEMM_BN_NO_RELU  32     /* bit 5: with BN_SUMS: the BatchNorm layer has no ReLU */
#define AST_IGEMM_PER_IMAGE   64     /* bit 6: with STATS: per-image statistics, below */
#define AST_IGEMM_SLOTS_SHIFT 8      /* bits 8-11: log2 of the number of statistics slots, 0 = 64 */
#define AST_IGEMM_SLOTS_MASK  (15 << AST_IGEMM_SLOTS_SHIFT)
#define AST_IGEMM_DET         4096   /* bit 12: the atomic-free instantiations (ast_igemm_ws_floats_det); refused with STATS, BN_SUMS or PER_IMAGE */
/* STATS: `ws` is a zeroed [slots][Cd][2] f32 table (ws_floats: its length) and every tile adds (sum, sum of squares) of the values
 * it stores into slot (tile index mod slots): nn.BatchNorm2d's batch statistics without a second pass over the output
 * (style_encoder.py:54-58, new_decoder.py:30-61).  Needs ACCUMULATE and RELU clear and a plan that does not split K
 * (ast_igemm_ws_floats == 0); reduce with ast_norm_finalize(N = slots, count = pixels).
 * STATS | PER_IMAGE: the table is [N][Cd][2] and every tile adds into the row of ITS IMAGE (tiles are laid out so that none straddles
 * two images): nn.InstanceNorm2d's per-image statistics (style_encoder.py:69); gathered and patch kernels only (ast_igemm_plan:
 * kch != 0); reduce with ast_norm_finalize(instance = 1).  PER_IMAGE without STATS is refused on every kernel path (the patch path
 * used to accept and ignore it).  A split-K plan takes neither STATS nor BN_SUMS and needs its workspace in `ws`. */
int ast_igemm(const void* src, const void* wgt, const float* bias, void* dst,
              const ast_gather_t* g, int dtype, int flags, float* ws, long ws_floats, void* stream);
/* ast_igemm as the data-gradient GEMM that PRODUCES dy of a BatchNorm2d(+ReLU) layer (AST_IGEMM_BN_SUMS; BN_NO_RELU: no ReLU):
 * bn_x is that layer's input (same geometry and dtype as dst), bn_scale/bn_shift its forward coefficients; every tile adds
 * (sum dz, sum dz*x), dz = dy*[fma(x, scale, shift) > 0], of the values it stores into the zeroed [slots][Cd][3] table `ws`,
 * so ast_norm_bwd_sums need not run (reduce with ast_norm_bwd_finalize(N = slots, count = pixels)).  Needs ACCUMULATE, RELU and
 * STATS clear, all three BatchNorm pointers and a plan without split-K. */
int ast_igemm_bn(const void* src, const void* wgt, const float* bias, void* dst, const ast_gather_t* g, int dtype, int flags,
                 float* ws, long ws_floats, const void* bn_x, const float* bn_scale, const float* bn_shift, void* stream);
/* Queries (host side, no launch; <0 on a bad geometry), all answered from the one plan ast_igemm computes per call.
 * ast_igemm_ws_floats: the f32 workspace (floats) ast_igemm needs: >0 when the launch is split over K (under-filled grids of the
 * deep, small-M layers), 0 otherwise.  ast_igemm_plan: out5 = {BM, BN, 16-byte chunks per row per barrier (kch), grid-level
 * split-K slices, in-workgroup K groups} of the gathered kernel; {-(tile rows), channel tile, -(slab bytes), -(fragments) for row
 * blocks else 1, 1} for the patch-staged kernel; {64 * pixel tiles per wave, 16 or 32, 0, 1, 1} for the LDS-free kernel of narrow
 * layers (Cd <= 16, ntaps*Cs <= 12 chunks: each lane's gather load is its MFMA fragment, the weights stay in registers).
 * ast_pconv_variant: out4 = {slab bytes, TM, TN, WALL} of the pconv_kernel instantiation and returns 1; 0 for the other two kernels. */
long ast_igemm_ws_floats(const ast_gather_t* g, int dtype);
int ast_igemm_plan(const ast_gather_t* g, int dtype, int* out5);
int ast_pconv_variant(const ast_gather_t* g, int dtype, int* out4);

/* dw[cd][wtap[t]][c] += sum_pix dy[pix][cd] * src[gather(pix,t)][c]   (f32 atomics)
 * dy is the plain operand over the logical grid (N,Hm,Wm,Cd).
 * Replaces: weight gradients of Conv2d / ConvTranspose2d / Linear. */
int ast_wgrad(const void* dy, const void* src, float* dw, const ast_gather_t* g,
              int dtype, void* stream);
/* The same with the gradient spread over `nrep` copies of dw (copy r at dw + r * Cd*wtaps*Cs; the workgroups of pixel slice z
 * use copy z % nrep): same-address f32 atomics serialise, and the reader (ast_weight_grads_flush_t with
 * ast_weight_desc_t.dwp_replicas) sums the copies.  All copies must be zeroed by the caller. */
int ast_wgrad_rep(const void* dy, const void* src, float* dw, const ast_gather_t* g, int dtype, int nrep, void* stream);
/* Slab form of the same: the launch cuts the pixels into at most `nslabs` slices, and every slice STORES (plain 256-byte-row
 * stores, no atomics) its partial gradient into its own copy of dW -- slabs[z * Cd*wtaps*Cs ...] for slice z; *slices_out = the
 * number of copies written (every one of them completely: nothing needs to be zeroed first).  ast_slab_sum adds the copies up:
 * copy 0 <- sum of the first slabs[i] copies of record i, for up to AST_MAX_SLAB_RECS weights in ONE launch (bases / floats_per_copy /
 * slabs are HOST arrays).  NOT an accumulate: a weight used twice in one backward pass must use ast_wgrad / ast_wgrad_rep.
 * (Deterministic mode routes every convolution weight gradient through these two calls.) */
#define AST_MAX_SLAB_RECS 48
int ast_wgrad_slab(const void* dy, const void* src, float* slabs, const ast_gather_t* g, int dtype, int nslabs, int* slices_out,
                   void* stream);
int ast_slab_sum(float* const* bases, const int64_t* floats_per_copy, const int* slabs, int nrec, void* stream);
/* Query (host side, no launch; <0 with ast_last_error on a bad geometry, dtype or cap), answered by the one decision the three
 * entries above launch from, with the same environment knobs read per call.  slab_cap = 0: what ast_wgrad / ast_wgrad_rep launch;
 * 1..4096: what ast_wgrad_slab launches with that many slabs.  out6 = {kernel family (0 cooperative wgrad_kernel, 1 wgrad_halo_kernel,
 * 2 wgrad_rows_kernel, 3 wgrad_tap_kernel; -1 for a geometry without taps: nothing is launched), BMW (output channels of a
 * workgroup's tile), NCT (its 16-column tiles of the (tap, channel) space; rows kernel: 64 x 12, tap kernel: 64 x 4), pixel groups
 * PG (rows kernel: ring stages; tap kernel: 1), pixel slices (what ast_wgrad_slab reports in *slices_out; pixel slice z uses copy
 * z % nrep of ast_wgrad_rep), pixels per slice (halo kernel: 8x16-pixel tiles in the layer)}.
 * With ntaps < wtaps (a parity class of a strided data gradient used as a weight-gradient geometry) no entry touches the dW slices of
 * the taps the geometry does not list: in slab form those slices of every copy keep what they held. */
int ast_wgrad_plan(const ast_gather_t* g, int dtype, int slab_cap, int* out6);

/* Token-sized nn.Linear (M <= 64 rows, f32): y = act(x W^T + b), W row pitch ldw (W may be a row slice
 * of in_proj_weight or the transposed pack for the data gradient).  One wave per output column. */
int ast_skinny_gemm(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw,
                    int ldy, int relu, void* stream);
/* ast_skinny_gemm with the fused-FFN epilogues (TransformerEncoderLayer/DecoderLayer._ff_block,
 * linear2(dropout(relu(linear1(x))))):  drop_mask != NULL draws a dropout mask (p, seed, d_offset as ast_dropout_fwd),
 * applies it and stores the COMBINED relu+dropout mask (0 or 1/(1-p)); mul_mask != NULL multiplies the result by a
 * stored mask (the backward's dh = (dy W2) * mask). */
int ast_skinny_gemm_ex(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy,
                       int relu, const float* mul_mask, float* drop_mask, float p, uint64_t seed, const int64_t* d_offset,
                       void* stream);
/* The two 2*287*513 x 256 linears of SimpleDecoder_TransformerOnly.py:16-17 on <= 64 token rows (f32, weights streamed once):
 * ast_bigk_gemm: y[M][N] = x[M][K] w[N][K]^T + bias, K huge and even (stft_to_embedding, :56-60); y is overwritten.
 * ast_bign_dgrad: dx[M][K] = dy[M][N] w[N][K], N huge, K <= 256 (data gradient of embedding_to_stft, :62-66); dx is overwritten.
 * (embedding_to_stft forward is ast_skinny_gemm with a huge N; both weight gradients are ast_linear_wgrad.) */
int ast_bigk_gemm(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldy, void* stream);
int ast_bign_dgrad(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, void* stream);
/* dW[n][k] += sum_m dy[m][n] x[m][k]; db[n] += sum_m dy[m][n]  -- straight into the parameter gradients */
int ast_linear_wgrad(const float* dy, const float* x, float* dW, float* db, int M, int N, int K, int lddy, int ldw,
                     void* stream);

/* Batched ast_linear_wgrad: table = DEVICE array of `count` records
 * {const float* dy, x; float* dW, db; int32 M, N, K, lddy, ldw, pad[3]} (64 bytes each); max_tiles >= max over
 * records of ceil(K/64)*ceil(N/64).  One launch for every linear layer of a model, after backward. */
int ast_linear_wgrad_batched(const void* table, int count, int max_tiles, void* stream);
/* The same with the records read from HOST memory at call time and passed to the kernel by value (<= 56 per launch):
 * no device table and no host-to-device copy, so the call is a plain kernel node under hipGraph capture. */
int ast_linear_wgrad_batched_host(const void* host_table, int count, int max_tiles, void* stream);

/* ---- layout conversion at the module boundary ------------------------------ */
/* x (N,C,H,W) f32, element (n,c,h,w) at n*sn + c*sc + h*sh + w  ->  NHWC dtype, Cp>=C zero padded.
 * Replaces the implicit NCHW contract of x.view(B*S,C,T,F) (style_encoder.py:213). */
int ast_nchw_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int64_t sn, int64_t sc,
                     int64_t sh, int Cp, int dtype, void* stream);
int ast_nhwc_to_nchw(const void* x, float* y, int N, int C, int H, int W, int Cp, int dtype, void* stream);
/* dtype casts of flat buffers */
int ast_cast(const void* x, int dtype_in, void* y, int dtype_out, int64_t n, void* stream);

/* ---- spectral norm + weight packing (torch spectral_norm.py:92-114) --------- */
/* KK <= 9: the pack and flush kernels stage one 32x32-channel tile with all KK taps in a fixed float[9*32*33] of LDS and a larger
 * KK writes past it.  The descriptors are read on the device, so the entry points below CANNOT check this: the caller must
 * (layers.WeightBank.add raises ValueError for a conv / conv-transpose kernel of more than 9 taps). */
typedef struct ast_weight_desc_t {
  const float* w;       /* weight_orig; element (co,ci,tap) at co*s_co + ci*s_ci + tap */
  float* u;             /* weight_u [Co] or NULL (no spectral norm) */
  float* v;             /* weight_v [Ci*KK] */
  float* sigma;         /* [1] out */
  float* scratch;       /* [ast_sn_scratch_floats(Co, Ci*KK)] = Co + Ci*KK*(1 + 32): s = W v, t = W^T u, row-chunk partials of t */
  void* wf;             /* packed [Cop][KK][Cip]  (rows = out channel) or NULL */
  void* wb;             /* packed [Cip][KK][Cop]  (rows = in channel) or NULL */
  int32_t Co, Ci, KK, s_co, s_ci, Cop, Cip;
  int32_t power_iter;   /* 1 in training, 0 in eval */
  float* dwp;           /* packed f32 gradient staging (zeroed by ast_weights_prepare_t in training) or NULL */
  float* grad;          /* gradient of `w` (same layout as w), accumulated by ast_weight_grads_flush_t */
  float* inner;         /* [1] scratch: <dWp, W/sigma> */
  int32_t dwp_from_wb;  /* 0: dwp is [Cop][KK][Cip]; 1: [Cip][KK][Cop] */
  int32_t dwp_replicas; /* dwp holds this many copies (0 = 1), Cop*KK*Cip floats apart, filled by ast_wgrad_rep; flush sums them */
} ast_weight_desc_t;
/* descs: DEVICE array of n descriptors, dtypes: DEVICE int[n] (packed dtype per weight), tiles: DEVICE array of
 * {int32 weight index, co0, ci0, pad} covering every 32x32 channel tile of every weight (padded extents).
 * prepare: power iteration (if requested), sigma = u^T W v, W/sigma written in both packed layouts and the
 * gradient staging zeroed -- five launches for all n weights; LDS-tiled so every global access is a contiguous run.
 * u, v and sigma are BIT-REPRODUCIBLE functions of (w, u): W^T u is summed over 32 row chunks through per-chunk slabs in a
 * fixed order (no float atomics), so data-parallel replicas -- which never exchange these buffers -- stay identical.
 * flush (once after backward): grad += (dWp - <dWp,W/sigma> u v^T)/sigma for every weight -- two launches. */
/* floats of ast_weight_desc_t.scratch for a (Co x ncols) weight */
long ast_sn_scratch_floats(int Co, int ncols);
int ast_weights_prepare_t(const ast_weight_desc_t* descs, const int* dtypes, int n, int max_co, int max_cols,
                          const void* tiles, int ntiles, void* stream);
int ast_weight_grads_flush_t(const ast_weight_desc_t* descs, const void* tiles, int ntiles, void* stream);
/* g_orig += (dWp - <dWp,W/sigma> u v^T)/sigma, dWp packed [Cop][KK][Cip] (from_wb=0)
 * or [Cip][KK][Cop] (from_wb=1).  u NULL => plain unpack-accumulate. */
int ast_weight_grad_unpack(const float* dwp, int from_wb, const float* w, const float* u, const float* v,
                           const float* sigma, float* g_orig, int Co, int Ci, int KK, int s_co, int s_ci,
                           int Cop, int Cip, float* scratch, void* stream);

/* ---- normalisation (nn.BatchNorm2d / nn.InstanceNorm2d / nn.LayerNorm) ------ */
/* sums[n][c][k]: k=0 sum x, k=1 sum x^2 over the H*W pixels of image n.  The buffer is zeroed inside unless
 * assume_zeroed (a persistent scratch that ast_norm_finalize(zero_sums=1) handed back clean). */
int ast_chan_stats(const void* x, float* sums, int N, int HW, int C, int dtype, int assume_zeroed, void* stream);
/* From sums -> per-channel (batch) or per-(n,c) (instance) scale/shift; updates
 * running stats when running_mean != NULL (momentum 0.1, unbiased var). eval_mode uses running stats.
 * count > 0 (batch form): the N rows of `sums` are partial-sum slots (the [64][C][2] table filled by ast_igemm's
 * flags bit 3) over `count` pixels in total; count == 0: N images of HW pixels. */
int ast_norm_finalize(float* sums, int zero_sums, int64_t* num_batches_tracked /* +1 when not NULL */,
                      int N, int HW, int C, int Creal, int instance,
                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                      int eval_mode, float eps, float* mean, float* rstd, float* scale, float* shift,
                      long count, void* stream);
/* y = act(x*scale[c] + shift[c] + r*scale2[n,c] + shift2[n,c]) ; r may be NULL.
 * flags: bit0 ReLU, bit1 scale/shift are per (n,c) instead of per c. */
int ast_affine_act(const void* x, const float* scale, const float* shift, const void* r,
                   const float* scale2, const float* shift2, void* y, int N, int HW, int C,
                   int flags, int dtype, void* stream);
/* Training-mode BatchNorm2d(+ReLU) [+ InstanceNorm2d of a second input: the ResBlock tail, style_encoder.py:76-83] in ONE
 * launch, statistics finalize included: every workgroup reduces the statistics table tab1 ([rows1][C][2] = {sum x, sum x^2} over
 * count1 pixels: the slot table of ast_igemm flags bit 3, or the [N][C][2] image sums of ast_chan_stats) into the per-channel
 * scale / shift itself, then applies y = act(x*scale + shift [+ r*scale2[n] + shift2[n]]); tab2 = [N][C][2] sums of r.  Workgroup
 * (0,0) writes out1 = [4][C] (mean, rstd, scale, shift) [out2 = [4][N*C]], updates the running statistics (momentum 0.1, unbiased
 * variance) and num_batches_tracked.  The tables are only READ: the caller clears them (one memset per step for all of them).
 * Replaces ast_norm_finalize + ast_affine_act (38 dependent single-wave launches per train step). */
int ast_bn_apply_fwd(const void* x, const void* r, void* y, const float* tab1, int rows1, long count1, const float* tab2,
                     const float* gamma1, const float* beta1, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     float eps1, const float* gamma2, const float* beta2, float eps2, float* out1, float* out2, int N, int HW, int C,
                     int Creal, int flags /* bit0 ReLU */, int dtype, void* stream);
/* Backward twin: tab3 = [rows][C][3] = {sum dz, sum dz*x, sum dz*r} (slot table of ast_igemm_bn over `count` pixels, or the
 * [N][C][3] image sums of ast_norm_bwd_sums); dx = k1[c]*(dz, x, 1), dr = k2[n][c]*(dz, r, 1) with the coefficients formed in
 * the kernel; dgamma / dbeta are ADDED by workgroup (0,0).  dz = dy * [fma(x, scale1, shift1) (+ fma(r, scale2[n], shift2[n])) > 0]
 * when flags bit0 (ReLU).  dr != NULL needs rows == N.  Replaces ast_norm_bwd_finalize + ast_norm_bwd_apply. */
int ast_bn_apply_bwd(const void* dy, const void* x, const void* r, void* dx, void* dr, const float* tab3, int rows, long count,
                     const float* gamma1, const float* mean1, const float* rstd1, float* dgamma1, float* dbeta1,
                     const float* gamma2, const float* mean2, const float* rstd2, float* dgamma2, float* dbeta2,
                     const float* scale1, const float* shift1, const float* scale2, const float* shift2, int N, int HW, int C,
                     int Creal, int flags, int dtype, void* stream);
/* backward of the above followed by the norm backward:
 * dz = dy * (y>0 if relu); sums3[n][c] = {sum dz, sum dz*x, sum dz*r} */
int ast_norm_bwd_sums(const void* dy, const void* y, const void* x, const void* r, float* sums3,
                      int N, int HW, int C, int relu, int dtype, int assume_zeroed, void* stream);
/* coefficients k[c][3] (batch branch) and j[n][c][3] (instance branch) and dgamma/dbeta accumulation */
int ast_norm_bwd_finalize(float* sums3, int zero_sums, int N, int HW, int C, int Creal,
                          const float* gamma1, const float* mean1, const float* rstd1,
                          float* dgamma1, float* dbeta1, float* k1,
                          const float* gamma2, const float* mean2, const float* rstd2,
                          float* dgamma2, float* dbeta2, float* k2, void* stream);
/* count > 0: the N rows of sums3 are partial-sum slots (the [64][C][3] table filled by ast_igemm_bn) over `count` pixels */
int ast_norm_bwd_finalize_n(float* sums3, int zero_sums, int N, int HW, int C, int Creal, const float* gamma1,
                            const float* mean1, const float* rstd1, float* dgamma1, float* dbeta1, float* k1,
                            const float* gamma2, const float* mean2, const float* rstd2, float* dgamma2,
                            float* dbeta2, float* k2, long count, void* stream);
/* dx = k1[c][0]*dz + k1[c][1]*x + k1[c][2];  dr = k2[n][c][0]*dz + k2[n][c][1]*r + k2[n][c][2] */
int ast_norm_bwd_apply(const void* dy, const void* y, const void* x, const void* r,
                       const float* k1, const float* k2, void* dx, void* dr,
                       int N, int HW, int C, int relu, int dtype, void* stream);
/* The same two passes with the ReLU mask RECOMPUTED from the pre-activation fma(x, scale1[c], shift1[c])
 * [+ fma(r, scale2[n][c], shift2[n][c])] -- bit-identical to what ast_affine_act formed in the forward pass -- so the
 * activation output y is not read (a third of each pass's HBM traffic); y may be NULL when scale1 is given. */
int ast_norm_bwd_sums_pre(const void* dy, const void* y, const void* x, const void* r, float* sums3, int N, int HW,
                          int C, int relu, int dtype, int assume_zeroed, const float* scale1, const float* shift1,
                          const float* scale2, const float* shift2, void* stream);
int ast_norm_bwd_apply_pre(const void* dy, const void* y, const void* x, const void* r, const float* k1,
                           const float* k2, void* dx, void* dr, int N, int HW, int C, int relu, int dtype,
                           const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                           void* stream);

int ast_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                      float* rstd, int rows, int D, float eps, int dtype, void* stream);
int ast_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                      const float* rstd, void* dx, float* dgamma, float* dbeta, int rows, int D,
                      int dtype, void* stream);

/* Fused residual + dropout + LayerNorm on f32 token rows (one launch for `norm(x + dropout(sub))`,
 * torch/nn/modules/transformer.py's post-norm and pre-norm blocks as style_encoder.py:181-187 and
 * new_decoder.py:111-118 instantiate them):
 *   s = x + dropout_p(sub)   (x NULL: s = dropout(sub); p == 0: mask untouched)
 *   y = LayerNorm(s)         (gamma NULL: s only)
 * mask holds 0 or 1/(1-p); seed/d_offset as ast_dropout_fwd.  Backward:
 *   ds = ds_ext + LN'(dy; s);  dx = ds (dx may be NULL);  dsub = ds * mask (mask NULL: ds). */
int ast_add_drop_ln_fwd(const float* x, const float* sub, float* mask, float* s_out, const float* gamma, const float* beta,
                        float* y, float* mean, float* rstd, int rows, int D, float eps, float p, uint64_t seed,
                        const int64_t* d_offset, void* stream);
int ast_add_drop_ln_bwd(const float* dy, const float* ds_ext, const float* s, const float* gamma, const float* mean,
                        const float* rstd, const float* mask, float* dx, float* dsub, float* dgamma, float* dbeta, int rows,
                        int D, void* stream);

/* Y[R_out][D] = A[R_out][R_in] X[R_in][D], A a small dense coefficient matrix (R_in <= 8192): class prototypes = per-class
 * means of style embeddings (style_encoder.py:243-253), per-row prototype gather, means over the section axis
 * (losses.py:88,142); the backward pass is the same call with A transposed. */
int ast_rowmix(const float* A, const float* X, float* Y, int R_out, int R_in, int D, void* stream);

/* ---- pooling / resampling ---------------------------------------------------- */
/* nn.AdaptiveAvgPool2d with bins [floor(i*In/Out), ceil((i+1)*In/Out)) (style_encoder.py:113-114, new_decoder.py:51) */
int ast_adaptive_pool_fwd(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int dtype, void* stream);
int ast_adaptive_pool_bwd(const void* dy, void* dx, int N, int H, int W, int C, int Ho, int Wo, int dtype, void* stream);
/* nn.Upsample(bilinear, align_corners=False) NHWC(Cp) -> NCHW f32 (new_decoder.py:99) */
int ast_bilinear_fwd(const void* x, float* y, int N, int C, int Cp, int H, int W, int Ho, int Wo, int dtype, void* stream);
int ast_bilinear_bwd(const float* dy, void* dx, int N, int C, int Cp, int H, int W, int Ho, int Wo, int dtype, void* stream);

/* ---- small-sequence attention core (nn.MultiheadAttention inner product part) - */
/* q:(B,Lq,ldq) k,v:(B,Lk,ldk) rows of f32 (already projected); heads of width dh; causal optional;
 * p_out (B,H,Lq,Lk) saved probabilities (after dropout mask scaling); drop_mask optional (B,H,Lq,Lk) of 0/1/(1-p)
 * Lq and Lk up to AST_ATTN_MAX_L tokens, dh <= 64.  Up to 16 x 16 tokens: one wave per (batch, head) (csrc/misc.hip).  Past
 * that (the decoder's memory is 2 S tokens, so from S = 9 sections on): tiles of 16 queries x 16 keys on
 * v_mfma_f32_16x16x4_f32 (csrc/attn.hip), which also need dh % 4 == 0, row strides that are multiples of 4 floats and 16-byte
 * aligned q / k / v / o / gradient pointers.  No float atomics on either path; the backward writes every element of dq, dk, dv
 * (and uses dq as scratch before it does). */
#define AST_ATTN_MAX_L 1024
int ast_attn_fwd(const float* q, const float* k, const float* v, float* o, float* probs,
                 int B, int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo, int causal,
                 const float* drop_mask, void* stream);
int ast_attn_bwd(const float* dout, const float* q, const float* k, const float* v, const float* probs,
                 float* dq, float* dk, float* dv, int B, int H, int Lq, int Lk, int dh, int ldq,
                 int ldk, int ldo, const float* drop_mask, void* stream);
/* The same with the attention-probability dropout DRAWN in the kernel (p, seed, d_offset as ast_dropout_fwd; element
 * index = ((b*H + h)*Lq + i)*Lk + j): forward and backward draw identical values, so no mask tensor is stored and no
 * mask kernel runs (nn.MultiheadAttention(dropout=0.1), style_encoder.py:181-187, new_decoder.py:111-118). */
int ast_attn_fwd_p(const float* q, const float* k, const float* v, float* o, float* probs, int B, int H, int Lq, int Lk,
                   int dh, int ldq, int ldk, int ldo, int causal, const float* drop_mask, float p, uint64_t seed,
                   const int64_t* d_offset, void* stream);
/* Ragged inference batches (evaluation_style_transfer.py:135-159 run on a zero-padded batch of clips of different lengths):
 * the forward core with a per-batch key mask.  Key j of batch b counts iff (j % key_period) < key_len[b]; key_len is an int32
 * (B,) DEVICE array, read by the kernel, so a captured graph serves every mix of lengths.  key_period == Lk is a plain
 * length mask (the content encoder's S section tokens, content_encoder.py:24-26); key_period == Lk / 2 masks both halves of
 * the decoder's memory [content x S | class x S] (new_decoder.py:208-229).  Checked on the host (error through
 * ast_last_error): key_len != NULL, 1 <= key_period <= Lk, Lk % key_period == 0, and everything ast_attn_fwd checks.  The
 * device values cannot be checked without a sync: the kernel clamps key_len[b] to [1, key_period], so every query has a valid
 * key and no value can produce NaN or an out-of-range access.  Masked keys contribute nothing, their probs entries are
 * written as 0, and their K / V rows are never read (NaN there does not reach o).  Every query row is computed; rows of
 * padded queries are finite and unspecified.  Same dispatch as ast_attn_fwd (csrc/misc.hip up to 16 x 16 tokens, csrc/attn.hip
 * past that, Lq = 1 included).  No dropout and no backward: those are ast_attn_fwd_len_p / ast_attn_bwd_len_p below. */
int ast_attn_fwd_len(const float* q, const float* k, const float* v, float* o, float* probs, int B, int H, int Lq, int Lk,
                     int dh, int ldq, int ldk, int ldo, int causal, const int32_t* key_len /* (B,) device */, int key_period,
                     void* stream);
int ast_attn_bwd_p(const float* dout, const float* q, const float* k, const float* v, const float* probs, float* dq, float* dk,
                   float* dv, int B, int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo, const float* drop_mask,
                   float p, uint64_t seed, const int64_t* d_offset, void* stream);
/* The key-masked core in TRAINING: zero-padded batches of clips of different lengths through the same attention calls
 * (evaluation_style_transfer.py:135-159 for the padded batch, content_encoder.py:24-26 and new_decoder.py:208-229 for the two
 * masks, style_encoder.py:181-187 and new_decoder.py:111-118 for nn.MultiheadAttention(dropout=0.1)).  key_len / key_period as
 * ast_attn_fwd_len, read from the device and clamped to [1, key_period]; drop_mask / p / seed / d_offset as ast_attn_fwd_p and
 * ast_attn_bwd_p: the element index of the draw is ((b*H + h)*Lq + i)*Lk + j whatever the mask, so with key_len[b] ==
 * key_period everywhere both entries reproduce the unmasked ones bit for bit, dropout included.  A masked key is scored
 * -inf and saved with probs == 0; its K and V rows are never read by the forward or by any backward kernel (NaN there
 * reaches none of o, dq, or the dk / dv of live keys), and its dk and dv rows are WRITTEN as exactly 0: the backward still
 * writes every element of dq, dk, dv (and uses dq as scratch before it does).  Every query row is computed from the dout it
 * is given; the caller's loss must ignore padded query rows (dout == 0 there).  Key tiles without a live key are skipped.  No
 * float atomics, one owner per output element, fixed summation order: bit-reproducible.  Checked on the host (error through
 * ast_last_error): everything ast_attn_fwd_len and ast_attn_bwd_p check (key_len != NULL, 1 <= key_period <= Lk,
 * Lk % key_period == 0, the long path's alignment and stride rules) and 0 <= p < 1. */
int ast_attn_fwd_len_p(const float* q, const float* k, const float* v, float* o, float* probs, int B, int H, int Lq, int Lk,
                       int dh, int ldq, int ldk, int ldo, int causal, const int32_t* key_len /* (B,) device */, int key_period,
                       const float* drop_mask, float p, uint64_t seed, const int64_t* d_offset, void* stream);
int ast_attn_bwd_len_p(const float* dout, const float* q, const float* k, const float* v, const float* probs, float* dq,
                       float* dk, float* dv, int B, int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo,
                       const int32_t* key_len /* (B,) device */, int key_period, const float* drop_mask, float p, uint64_t seed,
                       const int64_t* d_offset, void* stream);

/* ---- elementwise ------------------------------------------------------------- */
/* out[c] += sum_r x[r][c], c < Creal  (bias gradients of Conv2d / Linear) */
int ast_colsum_acc(const void* x, int64_t rows, int C, int Creal, float* out, int dtype, void* stream);
int ast_add(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream);
int ast_relu_bwd(const void* dy, const void* y, void* dx, int64_t n, int dtype, void* stream);
/* fused counter-based dropout: mask[i] in {0, 1/(1-p)} is generated, stored (for backward) and applied: y = x*mask */
int ast_dropout_fwd(const float* x, float* y, float* mask, int64_t n, float p, uint64_t seed, const int64_t* d_offset, void* stream);
/* counter-based dropout: mask[i] in {0, 1/(1-p)} (f32), y = x*mask */
int ast_dropout_mask(float* mask, int64_t n, float p, uint64_t seed, const int64_t* d_offset, void* stream);
int ast_mul(const void* a, const float* mask, void* y, int64_t n, int dtype, void* stream);

/* ---- losses -------------------------------------------------------------------- */
/* compute_comprehensive_loss (new_decoder.py:348-420), one pass: out (B,S,2,T,F) f32 contiguous,
 * tgt same logical shape with row stride tgt_ld (a [..., :513] view of x).  sums[5] raw sums
 * (mse, mag, phase, temporal, spectral); grad = d total / d out (may be NULL). */
int ast_recon_loss(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq,
                   float w_mse, float w_mag, float w_phase, float w_temporal, float w_spectral,
                   float* sums, float* grad, void* stream);
/* ast_recon_loss with the weighted total and the reported means formed on the device: coef5 / inv5 are HOST arrays (the five weights
 * c_mse .. c_spectral and the five 1/count factors of new_decoder.py:402-418), ws is AST_RECON_SLOTS x 5 floats of scratch (zeroed by
 * the call), res11 receives [5 raw sums][total = sum_k coef5[k] * sums[k]][5 means = inv5[k] * sums[k]].  grad as in ast_recon_loss. */
#define AST_RECON_SLOTS 64
int ast_recon_loss_total(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, const float* coef5,
                         const float* inv5, float* ws, float* res11, float* grad, void* stream);
/* compute_comprehensive_loss (new_decoder.py:348-420, SimpleDecoder_TransformerOnly.py:136-204) per clip of a zero-padded batch,
 * values only (no gradient path): row b of res is the loss of out[b, :n_b] against tgt[b, :n_b] alone,
 * n_b = clamp(n_sections[b], 1, S).  out (B,S,2,T,Fq) f32 contiguous, tgt as in ast_recon_loss; n_sections int32 (B,) ON THE DEVICE,
 * NULL = every clip holds S sections.  coef5 is a HOST array of the five weights (mse, magnitude, phase, temporal, spectral:
 * 2.0 of new_decoder.py:406 or 1.0 of SimpleDecoder_TransformerOnly.py:194, then 0.5, lambda_phase, lambda_temporal,
 * lambda_spectral).  The counts of new_decoder.py:402-418 are clip b's own and are formed on the device, without a host read:
 * mse 2 n_b T Fq; magnitude, phase n_b T Fq; temporal 2 (n_b - 1) T Fq (the term is exactly 0 at n_b == 1, new_decoder.py:387-392);
 * axis-3 difference 2 n_b (T - 1) Fq.  res (B, 11) = [5 raw sums][total = sum_k coef5[k] / count_k * sums[k]][5 means], the layout
 * of ast_recon_loss_total's res11.  Sections s >= n_b of either tensor are never read (they may hold NaN), and the last real
 * section's temporal difference does not look at section n_b.  No floating-point atomics: every workgroup stores its partials
 * into ws, a finishing launch sums them in a fixed order, so a clip's eleven numbers are bit-identical from run to run.
 * ws >= ast_recon_loss_len_ws_floats(B, S, T, Fq) floats (ws_floats is checked; ws is written completely, never zeroed); the
 * query returns < 0 for sizes the entry refuses.  Needs B <= 65535 and B*T*Fq < 2^31 (ast_recon_loss's index-width condition). */
long ast_recon_loss_len_ws_floats(int B, int S, int T, int Fq);
int ast_recon_loss_len(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, const int32_t* n_sections,
                       const float* coef5, float* ws, long ws_floats, float* res, void* stream);
/* ast_recon_loss_len with its gradient, for training on a padded batch: in one streaming pass the values of ast_recon_loss_len
 * (res (B, 11), the same layout) and grad = d loss / d out for loss = sum_b w_b * total_b, total_b = res[b][5] the loss of clip b
 * alone over its n_b = clamp(n_sections[b], 1, S) sections.  w_b = clip_weights[b] (float32 (B,) ON THE DEVICE), NULL = 1/B: at equal
 * lengths loss is then the batch value of ast_recon_loss_total and grad its gradient.  loss receives the scalar (formed on the
 * device in a fixed order by a one-wave third launch).  grad (B,S,2,T,Fq) f32 contiguous arrives uninitialised and is written
 * completely: rows s >= n_b as exactly 0.  The per-clip coefficients w_b * coef5[k] / count_k(n_b) (the counts above) are formed on
 * the device once per workgroup; a term without elements (temporal at n_b == 1, axis-3 difference at T == 1) contributes gradient
 * exactly 0, and the last real section has no successor.  Sections s >= n_b of out and tgt are never read (they may hold NaN).
 * out must be non-zero wherever the reference's phase gradient is to be finite (atan2 backward divides by re^2 + im^2, as
 * ast_recon_loss does).  No atomics, no memset, no host read: capturable, one graph serves every mix of lengths, and every
 * result is bit-identical from run to run in both modes.  ws >= ast_recon_loss_len_grad_ws_floats(B, S, T, Fq) floats (the size
 * of ast_recon_loss_len_ws_floats; checked, written completely, never zeroed; the query returns < 0 for sizes the entry refuses).
 * Checked on the host before any launch: out, tgt, coef5, ws, res, loss, grad non-null; B, S, T, Fq >= 1; tgt_ld >= Fq;
 * B <= 65535; B*T*Fq < 2^31; ws_floats. */
long ast_recon_loss_len_grad_ws_floats(int B, int S, int T, int Fq);
int ast_recon_loss_len_grad(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, const int32_t* n_sections,
                            const float* clip_weights, const float* coef5, float* ws, long ws_floats, float* res, float* loss,
                            float* grad, void* stream);
/* losses.py on (B,256) embeddings; each writes loss[0] and optional gradients.  Every row width D must be >= 1; ast_hsic and
 * ast_crosscov take ds and dc together (both or neither): one without the other is refused, since the kernels write both or none. */
int ast_infonce(const float* emb, const int32_t* labels, int B, int D, float temperature,
                float* loss, float* demb, float* ws /* 2*B*B + B floats */, void* stream);
int ast_margin(const float* cls, int C, int D, float margin, float* loss, float* dcls, void* stream);
int ast_hsic(const float* s, const float* c, int B, int D, float* loss, float* ds, float* dc,
             float* ws /* 6*B*B + 2*B + 8 floats */, void* stream);
/* cross-covariance variant of disentanglement_loss (losses.py:146-150); ws: 2*D + 2*B*B floats */
int ast_crosscov(const float* s, const float* c, int B, int D, float* loss, float* ds, float* dc, float* ws, void* stream);
/* mean cross entropy over rows of logits (R,C); dlogits optional */
int ast_cross_entropy(const float* logits, const int32_t* target, int R, int C, float* loss, float* dlogits, void* stream);
/* mean entropy with log(p+1e-8) (losses.py:118-120) */
int ast_softmax_entropy(const float* logits, int R, int C, float* loss, float* dlogits, void* stream);

/* y = (accumulate ? y : 0) + hscale * (dscale ? *dscale : 1) * x   (chain rule for scalar losses) */
int ast_scale(const float* x, const float* dscale, float hscale, float* y, int64_t n, int accumulate, void* stream);

/* ---- optimiser ------------------------------------------------------------------ */
int ast_counter_incr(int64_t* c, void* stream);
int ast_sumsq(const float* x, int64_t n, float* out /* accumulates */, void* stream);
/* Adam with bias correction; grad scaled by min(1, max_norm/(sqrt(*gnorm_sq)+1e-6)) when gnorm_sq != NULL */
int ast_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
             float eps, float wd, const int64_t* d_step, const float* gnorm_sq, float max_norm, void* stream);

/* Step scalars on the device, so that ONE captured hipGraph follows a learning-rate schedule, a ramped adversarial weight or
 * a changed clip norm (the reconstructed train2 step: `scheduler.step()` and lambda_adv(t); README.md:144-150).
 * ast_adam_dev: as ast_adam, with [lr, max_norm] read from device memory at run time (max_norm <= 0: no clipping).
 * ast_set_values: dst[i] = host_vals[i], i < n <= AST_MAX_STEP_SCALARS -- the values travel as kernel arguments (stream-ordered,
 * no pinned staging buffer to race with).
 * ast_weighted_sum: out[0] = sum_i weights[widx[i]] * terms[i][0] (widx[i] < 0: weight 1), terms added in order -- the total loss
 * `w_rec * rec + w_nce * nce + ...` of the train step in one launch; _bwd: grads[i] = g[0] * weights[widx[i]].
 * `terms` / `widx` are HOST arrays of n <= AST_MAX_STEP_SCALARS entries (device pointers / indices into `weights`). */
#define AST_MAX_STEP_SCALARS 16
int ast_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* d_hyper /* [lr, max_norm] */, float b1, float b2,
                 float eps, float wd, const int64_t* d_step, const float* gnorm_sq, void* stream);
int ast_set_values(float* dst, const float* host_vals, int n, void* stream);
int ast_weighted_sum(const float* const* terms, const int* widx, int n, const float* weights, float* out, void* stream);
int ast_weighted_sum_bwd(const float* g, const int* widx, int n, const float* weights, float* grads, void* stream);

/* ---- STFT front-end (utilityFunctions.py:12-37 + dataloader.py:9-13 + utilityFunctions.py:240-263) */
/* wave (Bc, nsamp) f32 -> x (Bc, S, 2, 287, F_total) f32: frames of a 1024-point Hann STFT (hop 256,
 * reflect padded), z-scored with mean/std (2,513), cut into S sections of 287 frames (step 191), written
 * to bins [0,513) of the F_total-wide rows. */
/* inverse_STFT (utilityFunctions.py:62-82; torch.istft defaults): spec (Bc,2,T,513) f32 -> wave (Bc, 256*(T-1));
 * frames_ws: Bc*T*1024 floats of scratch. */
int ast_istft(const float* spec, int Bc, int T, float* frames_ws, float* wave, void* stream);
/* The same for a padded batch (evaluation_style_transfer.py:154-157, one clip per row): clip b is inverted as a clip of
 * n_frames[b] frames (int32 (Bc,) DEVICE array, clamped to [2, T]): overlap-add and envelope over its frames only, samples
 * i >= 256 * (n_frames[b] - 1) of its row written as 0.  Rows of spec past n_frames[b] are never read. */
int ast_istft_len(const float* spec, int Bc, int T, float* frames_ws, float* wave, const int32_t* n_frames, void* stream);
/* sections2spectrogram (utilityFunctions.py:265-283): sections (Bc,S,2,wind,F_in) -> out (Bc,2,out_T,F_out), the
 * count-normalised overlap-average at step `hop`, bins [0,F_out) only, truncated to out_T <= hop*(S-1)+wind frames. */
/* Dataset statistics, one clip at a time (Preprocessing_Dataset/compute_unified_stats.py:34-44): per (channel, bin) mean over
 * the T frames and unbiased variance of a contiguous (C,T,F) f32 spectrogram, ADDED into mean_acc / var_acc (C*F floats). */
int ast_bin_stats_acc(const float* x, float* mean_acc, float* var_acc, int C, int T, int F, void* stream);
/* normalize (dataloader.py:9-13): out = (x - mean[c][f]) / (std[c][f] + eps) over a contiguous (C,T,F) f32 spectrogram */
int ast_zscore(const float* x, const float* mean, const float* std_, float* out, int C, int T, int F, float eps, void* stream);
int ast_sections_overlap_avg(const float* sections, float* out, int Bc, int S, int wind, int hop, int F_in, int F_out,
                             int out_T, void* stream);
/* The same for a padded batch (evaluation_style_transfer.py:154-155, one clip per row): clip b averages its sections
 * k < n_sec[b] only, in the sum and in the count (later sections are never read), and frames t >= n_frames[b] of out are
 * written as 0.  n_sec, n_frames: int32 (Bc,) DEVICE arrays, clamped to [1, S] and [1, out_T]. */
int ast_sections_overlap_avg_len(const float* sections, float* out, int Bc, int S, int wind, int hop, int F_in, int F_out,
                                 int out_T, const int32_t* n_sec, const int32_t* n_frames, void* stream);
int ast_stft_sections(const float* wave, int Bc, int nsamp, const float* mean, const float* std_,
                      float* x, int S, int win, int step, int F_total, void* stream);

/* get_CQT (utilityFunctions.py:39-60 -> librosa.cqt), all octaves in one launch.  For octave o (host arrays of n_oct
 * entries): ys[o] = device pointer to the o-times-halved signals (B rows of ns[o] floats), hops[o] its hop, los[o] its first
 * bin, nfs[o] its bin count, row0s[o] its first kernel row.  out[b][0|1][t][bin_off+los[o]+k] = Re|Im( scale[los[o]+k] *
 * sum_i y_o[b][t*hop_o - nfft/2 + i] * (w_re + i w_im)[row0s[o]+k][i] ), y = 0 outside the signal (pad_mode="constant").
 * w_* (rows, nfft), scale (n_bins), out (B, 2, T, ld) f32.  The kernels w fold librosa's rectangular-window STFT and its
 * sparsified wavelet FFT basis (built on the host, ast_amd/cqt.py). */
int ast_cqt_octaves(const float* const* ys, const int* ns, const int* hops, const int* los, const int* nfs, const int* row0s,
                    int n_oct, int B, const float* w_re, const float* w_im, const float* scale, int nfft, float* out, int T,
                    int ld, int bin_off, void* stream);
/* normalize + get_overlap_windows of the CQT planes (dataloader.py:9-18, utilityFunctions.py:240-263) into the bins behind
 * the STFT's: x[b][s][c][w][bin0+k] = (cqt[b][c][s*step+w][k] - mean[c][k]) / (std[c][k] + 1e-8), 0 past frame T-1.
 * cqt (Bc,2,T,nb), x (Bc,S,2,win,F_total) f32.  The CQT twin of ast_stft_sections. */
int ast_cqt_sections(const float* cqt, int Bc, int T, int nb, const float* mean, const float* std_, float* x, int S, int win,
                     int step, int F_total, int bin0, void* stream);
/* ---- the front end for a padded batch of clips of different sample counts (evaluation_style_transfer.py:135-159 starts from
 * one waveform per clip).  n_samples: int32 (Bc,) DEVICE array, clip b holds n_samples[b] samples inside a zero-padded row of
 * nsamp.  The values cannot be checked without a sync, so every kernel clamps them to [NS_MIN, nsamp], NS_MIN =
 * max(513, 256 * ((win + 1) / 2 - 1)): the smallest count that reflect-pads validly and yields one section (36 608 at win 287);
 * the host refuses nsamp < NS_MIN.  With ns the clamped count (csrc/ast_lengths.h, one function for host and device):
 *   T_b = 1 + ns / 256;  n_sec_b = len(section_starts(T_b)) (utilityFunctions.py:246-262) = k + (2 (T_b - k step) >= win),
 *   k = ceil(max(T_b - win, 0) / step);  n_frames_b = min(T_b, step (n_sec_b - 1) + win), the frames the kept sections cover.
 * Per output element the _len kernels run the arithmetic of the plain ones on the clip alone, in the same order. */
/* n_sections_out[b] = n_sec_b, n_frames_out[b] = n_frames_b (int32 (Bc,) device arrays), one small launch */
int ast_frontend_lengths(const int32_t* n_samples, int Bc, int nsamp, int win, int step, int32_t* n_sections_out,
                         int32_t* n_frames_out, void* stream);
/* the same function on the host for one value: out4 = {clamped ns, T_b, n_sec_b, n_frames_b} */
int ast_frontend_lengths_host(int ns, int nsamp, int win, int step, int* out4);
/* ast_stft_sections (utilityFunctions.py:12-37,240-263) with clip b transformed as a clip of n_samples[b] samples: reflected
 * at its own end; rows t >= T_b and every row of sections s >= n_sec_b (the dropped tail included) are written as 0. */
int ast_stft_sections_len(const float* wave, int Bc, int nsamp, const float* mean, const float* std_, float* x, int S, int win,
                          int step, int F_total, const int32_t* n_samples, void* stream);
/* The halving between CQT octaves (librosa audio.resample(2 -> 1); ast_resample_poly with orig = 2, nnew = 1, klen <= 4096) at
 * level o: x (B, n = ceil(nsamp / 2^o)), and input sample s of clip b counts iff s < ceil(n_samples[b] / 2^o), as the clip
 * alone ends there.  y (B, m). */
int ast_decimate2_len(const float* x, int B, int n, const float* h, int klen, int width, float* y, int m, float gain,
                      const int32_t* n_samples, int nsamp, int win, int step, int o, void* stream);
/* ast_cqt_octaves (utilityFunctions.py:39-60) where octave o is the o-times-halved signal, ns[o] = ceil(nsamp / 2^o): the span
 * of octave o reads 0 for s >= ceil(n_samples[b] / 2^o).  Frames t >= T_b are computed and unspecified (ast_cqt_sections_len
 * drops them). */
int ast_cqt_octaves_len(const float* const* ys, const int* ns, const int* hops, const int* los, const int* nfs, const int* row0s,
                        int n_oct, int B, const float* w_re, const float* w_im, const float* scale, int nfft, float* out, int T,
                        int ld, int bin_off, const int32_t* n_samples, int nsamp, int win, int step, void* stream);
/* ast_cqt_sections (dataloader.py:9-18, utilityFunctions.py:240-263) with T = 1 + nsamp / 256: 0 for t >= T_b and s >= n_sec_b */
int ast_cqt_sections_len(const float* cqt, int Bc, int T, int nb, const float* mean, const float* std_, float* x, int S, int win,
                         int step, int F_total, int bin0, const int32_t* n_samples, int nsamp, void* stream);
/* Polyphase FIR resampler: y[b][i*nnew + p] = gain * sum_k kern[p][k] * x[b][i*orig + k - width], x = 0 outside [0,n);
 * kern (nnew, klen), y (B, m).  Replaces torchaudio.functional.resample in load_audio (utilityFunctions.py:116-117;
 * kern = its sinc_interp_hann bank) and the halving resample between CQT octaves (orig=2, nnew=1). */
int ast_resample_poly(const float* x, int B, int n, const float* kern, int orig, int nnew, int klen, int width, float* y, int m,
                      float gain, void* stream);
/* load_audio's resample and stereo mean (utilityFunctions.py:116-120) for a padded batch of clips at their native rate, before
 * the ragged front end above.  x (B, C, n) f32, C = 1 or 2; the channel rows of clip b hold n_in[b] samples (int32 (B,) DEVICE
 * array, clamped on the device to [1, n]; NULL: every clip is n long).  y (B, m) mono, m == ceil(n * nnew / orig).  With nb the
 * clamped count and mb = ceil(nb * nnew / orig): y[b][j], j < mb, is ast_resample_poly's sum on x[b][c][0..nb) alone -- samples
 * s >= nb count as 0 and are never read -- in the same order (bit-equal for C = 1; for C = 2 the two channels' results are added
 * and halved, torch.mean's order); y[b][j] = 0 for j >= mb; n_out[b] = mb (int32 (B,) device array, may be NULL).
 * orig = 2, nnew = 1, klen <= 4096 runs the staged halving (one launch per channel); other ratios stage each workgroup's
 * sample span in LDS (64 rows of klen <= 638 samples), longer filters run one thread per output.  n * nnew, C * n and
 * n + 66 * orig + klen must stay below 2^31. */
int ast_resample_poly_len(const float* x, int B, int C, int n, const float* kern, int orig, int nnew, int klen, int width,
                          float* y, int m, float gain, const int32_t* n_in, int32_t* n_out, void* stream);

/* ---- spectrogram metrics of the evaluation scripts for a padded batch (csrc/metrics.hip).  |STFT| with librosa.stft's
 * documented defaults restated: frame t is centred on sample t * hop, periodic Hann window of n_fft, T(n) = 1 + n / hop frames.
 * pad_mode AST_PAD_CONSTANT: samples outside the clip are 0 (librosa >= 0.10); AST_PAD_REFLECT: reflected at the clip's own ends
 * (librosa < 0.10, get_STFT).  Per-clip sample counts are int32 (B,) DEVICE arrays, NULL: the row is full; device values are
 * clamped to [1, n] (constant) or [n_fft / 2 + 1, n] (reflect; the host refuses shorter rows), samples behind a clip's end are
 * never read.  The spectrogram is never stored: partials go to the caller's workspace ws (f32, the _ws_floats count; every slot
 * that is read is written first), a second launch sums them in a fixed order in double.  No atomics; results are bit-reproducible
 * and row b does not depend on the other rows.  B <= 65535, n + 2 n_fft < 2^31. */
#define AST_PAD_CONSTANT 0
#define AST_PAD_REFLECT 1
/* mse_spectrogram (evaluation_reconstruction.py:105-118 on the audio truncated to a common length at :193-204), n_fft 1024,
 * hop 256: original (B, n_orig), generated (B, n_gen) f32; L_b = min of the two clamped counts, both clips cut to L_b samples
 * before padding; out[b] = mean over 513 x T(L_b) of (|A| - |G|)^2.  One complex FFT per frame pair: two consecutive frames of
 * one clip in the real and the imaginary part, split by Hermitian symmetry, first for original, then for generated -- the same
 * arithmetic for both, so equal clips score exactly 0.  ws: B * ceil(T(min(n_orig, n_gen)) / 2) floats. */
long ast_spec_mse_ws_floats(int B, int n_orig, int n_gen);
int ast_spec_mse_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                     const int32_t* len_gen, int pad_mode, float* ws, long ws_floats, float* out, void* stream);
/* the band energies of instrumentation_similarity (evaluation_style_transfer.py:112-115), n_fft 2048, hop 512: waves (B, n) f32,
 * energy[b][f] = sum_{t < T(n_b)} |S_b[f][t]|, (B, 1025) f32.  A workgroup walks a run of consecutive frames of one clip (the
 * 2048-point real FFT through the 1024-point network) and stores one (1025,) partial per run.
 * ws: B * ceil((1 + n / 512) / run) * 1025 floats. */
long ast_band_energy_ws_floats(int B, int n);
int ast_band_energy_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, float* ws, long ws_floats,
                        float* energy, void* stream);
/* frames per run of the band-energy kernel (what the workspace count above is built on) */
int ast_band_energy_run_frames(void);
/* Pearson's r of rows a[b], b[b] of n >= 2 values in double (evaluation_style_transfer.py:117-119: pearsonr, nan -> 0.0):
 * out[b] is exactly 0 where r is not finite (a constant row).  a, b (B, n), out (B,) f32. */
int ast_pearson_rows(const float* a, const float* b, int B, int n, float* out, void* stream);
/* MFCC: librosa.feature.mfcc(y, sr, n_mfcc, hop_length) with every other argument at its default, restated (csrc/metrics.hip):
 * S = |STFT|^2 at n_fft 2048, M = W S with the Slaney mel filter bank (128 bands, fmin 0, fmax sr / 2, Slaney normalisation),
 * dB = 10 log10(max(1e-10, M)) clamped from below to the clip's own maximum - 80, then the first n_mfcc rows of the orthonormal
 * DCT-II along the bands.  Two passes, because the clamp needs the maximum over the whole clip: the first stores the dB rows
 * (B, T_max, 128) and one maximum per run of frames into ws, the second clamps and transforms.  The spectrogram is never stored.
 * hop is 256 or 512 (the reference's two values), n_mfcc 1 .. 128; counts, pad modes, clamps and limits as above, n_fft = 2048.
 *
 * The filter bank is a table of `ast_mel_table_words` 32-bit words that the host function below fills for a sample rate (in
 * double, no device needed); the caller copies it to the device once, outside any capture, and passes the device pointer as
 * mel_table.  Layout: 128 first bins, 129 offsets into the weights, then the bands' weights in turn as float bits (never more
 * than 2 x 1025: a bin lies inside at most two triangles).  A rate at which a band holds no bin is refused. */
int ast_mel_table_words(void);
int ast_mel_table(int sample_rate, int32_t* table);
/* frames per run of the first pass (what the workspace counts below are built on) */
int ast_mfcc_run_frames(void);
/* librosa.feature.mfcc for a padded batch (evaluation_style_transfer.py:101-102, :122-123): waves (B, n) f32 ->
 * out (B, n_mfcc, T_max) f32, T_max = 1 + n / hop, librosa's layout; frames t >= T_b = 1 + n_b / hop of clip b are exactly 0.
 * ws: B * (T_max * 128 + ceil(T_max / run)) floats. */
long ast_mfcc_ws_floats(int B, int n, int hop);
int ast_mfcc_len(const float* waves, int B, int n, const int32_t* n_samples, int n_mfcc, int hop, int pad_mode, const int32_t* mel_table,
                 float* ws, long ws_floats, float* out, void* stream);
/* mfcc_distance (evaluation_style_transfer.py:99-109): generated (B, n_gen), reference (B, n_ref) f32 -> out (B,) f32, the mean
 * over t < T = min(T_gen_b, T_ref_b) of the Euclidean norm of the difference of the two clips' coefficient columns.  Each clip
 * keeps its own length (nothing is truncated) and is clamped by its own maximum.  The DCT is taken of the difference of the
 * clamped dB rows; both clips pass through the same arithmetic, so equal clips score exactly 0.  One partial per frame, summed in
 * a fixed order in double.  ws: the two batches' counts above plus B * (1 + min(n_gen, n_ref) / hop) floats. */
long ast_mfcc_distance_ws_floats(int B, int n_gen, int n_ref, int hop);
int ast_mfcc_distance_len(const float* generated, int n_gen, const float* reference, int n_ref, int B, const int32_t* len_gen,
                          const int32_t* len_ref, int n_mfcc, int hop, int pad_mode, const int32_t* mel_table, float* ws, long ws_floats,
                          float* out, void* stream);

/* ---- chroma and pitch metrics of the evaluation scripts for a padded batch (csrc/chroma.hip).  librosa's documented chain restated
 * ("Chroma and pitch"; parity with librosa's own output is unpinned), sr = 22 050, frames, windows, pad modes, counts and
 * clamps as above.  Two settings: (n_fft 2048, hop 512), librosa's defaults, and (1024, 256); anything else is refused.
 * A clip may be cut to a partner's count first (evaluation_reconstruction.py:193-204): n_cut is the partner's int32 (B,) DEVICE
 * array or NULL, cut_max its row width, and clip b counts min(clamped n_samples[b], clamped n_cut[b]) samples; without a partner
 * pass n_cut = NULL and cut_max = n.  No float atomics; the only atomics are integer counters in LDS; results are bit-reproducible
 * and row b does not depend on the other rows. */
/* frames per run (one workgroup) of the frame passes; the candidate band of librosa.piptrack's defaults, 150 <= k sr / n_fft < 4000 */
int ast_chroma_run_frames(void);
int ast_pitch_band(int n_fft, int* k_lo, int* k_hi);
/* librosa.estimate_tuning as librosa.feature.chroma_stft calls it (S = |STFT|^2, bins_per_octave 12, resolution 0.01): piptrack's
 * peaks of the band (pitch and mag, [b][t][band], 0 where there is no peak) go to ws, 2 * B * T_max * band floats; then one
 * workgroup per clip takes the exact median of the mags by radix selection on their bit patterns (the mean of the two middle
 * values for an even count), and the 100-bin histogram (np.histogram over linspace(-0.5, 0.5, 101)) of the deviations
 * frac(12 log2(pitch / 27.5)), wrapped to [-0.5, 0.5), of the peaks with mag >= median.  tuning[b] = -0.5 + 0.01 * argmax, the
 * lowest index winning ties; 0.0 without a peak.  debug: NULL, or B * ast_tuning_debug_words() int32 on the device, per clip the
 * count of peaks, the count kept, the median as float bits and the 100 histogram counts (for the tests). */
int ast_tuning_debug_words(void);
long ast_tuning_ws_floats(int B, int n, int n_fft);
int ast_tuning_len(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int n_fft, int hop,
                   int pad_mode, float* ws, long ws_floats, float* tuning, int32_t* debug, void* stream);
/* librosa.feature.chroma_stft (evaluation_reconstruction.py:41-42, evaluation_style_transfer.py:82-83): waves (B, n) f32, tuning
 * (B,) f32 on the device (ast_tuning_len's, or the caller's) -> out (B, 12, T_max) f32, T_max = 1 + n / hop, librosa's layout, row
 * 0 = C; frames t >= T_b are exactly 0.  raw = W |STFT|^2 with librosa.filters.chroma(sr, n_fft, tuning[b])'s defaults built per
 * thread in registers, each frame divided by its maximum over the 12 rows unless that is below float32 tiny. */
int ast_chroma_len(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int n_fft, int hop,
                   int pad_mode, const float* tuning, float* out, void* stream);
/* chroma_distance (evaluation_reconstruction.py:39-52, on the audio truncated to a common length at :193-204), n_fft 2048, hop 512:
 * out[b] = mean over the T(L_b) frames of ||chroma_o[:, t] - chroma_g[:, t]||_2, each clip with its own estimated tuning.  Both
 * clips pass through the same arithmetic, so equal clips score exactly 0.
 * ws: the peaks of the wider batch + 2 B tunings + both chromas (ast_chroma_distance_ws_floats). */
long ast_chroma_distance_ws_floats(int B, int n_orig, int n_gen);
int ast_chroma_distance_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                            const int32_t* len_gen, int pad_mode, float* ws, long ws_floats, float* out, void* stream);
/* chroma_similarity (evaluation_style_transfer.py:80-96), n_fft 1024, hop 256: each clip keeps its own length; Pearson's r in
 * double over the frames t < min(T_g, T_o) for each of the 12 rows, out[b] = the mean of the finite ones, exactly 0 if none. */
long ast_chroma_similarity_ws_floats(int B, int n_gen, int n_orig);
int ast_chroma_similarity_len(const float* generated, int n_gen, const float* original, int n_orig, int B, const int32_t* len_gen,
                              const int32_t* len_orig, int pad_mode, float* ws, long ws_floats, float* out, void* stream);
/* np.mean(librosa.piptrack(y, sr)[0], axis=0) (evaluation_reconstruction.py:85-90), n_fft 2048, hop 512, S = |STFT|:
 * out[b][t] = (1 / 1025) sum_k pitch[k][t], (B, T_max) f32, summed in a fixed order; frames t >= T_b are exactly 0. */
int ast_pitch_mean_len(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int pad_mode,
                       float* out, void* stream);
/* pitch_correlation (evaluation_reconstruction.py:83-103, on the audio truncated to a common length at :193-204): Pearson's r in
 * double of the two clips' mean pitches over the T(L_b) frames, exactly 0 where r is not finite or T < 2.
 * ws: B * (T_max(n_orig) + T_max(n_gen)) floats. */
long ast_pitch_correlation_ws_floats(int B, int n_orig, int n_gen);
int ast_pitch_correlation_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                              const int32_t* len_gen, int pad_mode, float* ws, long ws_floats, float* out, void* stream);

/* ---- onsets and self-similarity: the last two of the evaluation scripts' eight metrics (csrc/metrics.hip; DESIGN 7, "Onsets and
 * self-similarity"; parity with librosa's own output is unpinned).  sr 22 050, n_fft 2048, hop 512; frames, windows, pad modes,
 * counts, clamps and limits as for the MFCC above, mel_table as there (at 22 050 Hz).  No atomics; results are bit-reproducible and
 * row b does not depend on the other rows.  Every workspace slot that is read is written first. */
/* frames per workgroup of the envelope pass and of the coefficient-distance pass (what the workspace counts are built on) */
int ast_onset_tile_frames(void);
int ast_recurrence_chunk_frames(void);
/* librosa.onset.onset_strength as onset_detect calls it (evaluation_reconstruction.py:57-58): waves (B, n) f32 -> out (B, T_max) f32,
 * T_max = 1 + n / 512.  e[t] = the mean over the 128 mel bands of max(0, dB[m][t-2] - dB[m][t-3]) for 3 <= t < T_b, with dB the
 * MFCC's clamped mel rows; exactly 0 for t < 3 and for t >= T_b.
 * ws: the MFCC's first pass at hop 512 + 2 B ceil(T_max / tile) floats (one minimum and one maximum per tile). */
long ast_onset_strength_ws_floats(int B, int n);
int ast_onset_strength_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, const int32_t* mel_table, float* ws,
                           long ws_floats, float* out, void* stream);
/* librosa.onset.onset_detect(y, sr=22050) at its defaults (evaluation_reconstruction.py:57-58), as a mask: mask (B, T_max) int32, 1
 * where frame t of clip b is an onset, 0 elsewhere and for t >= T_b.  No onsets if the envelope is all zero or not all finite;
 * else x = (e - min e) / (max e - min e + float32 tiny), frame n is a detection if x[n] >= x[n-1] and
 * x[n] >= mean(x[n-4 .. n+4]) + 0.07 (the windows cut at the clip's ends; the sizes are 0.03 sr / hop and so on), and walking up a
 * detection is kept if it lies more than 1 frame behind the last kept one.  ws: ast_onset_strength's + B T_max floats. */
long ast_onset_detect_ws_floats(int B, int n);
int ast_onset_detect_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, const int32_t* mel_table, float* ws,
                         long ws_floats, int32_t* mask, void* stream);
/* onset_accuracy (evaluation_reconstruction.py:54-81, on the audio truncated to a common length at :193-204): both clips cut to
 * L_b = min of the two clamped counts; O, G their onset sets; out[b] = 1 if both are empty, 0 if exactly one is, else
 * 2 |O and G| / (|O| + |G|), the F1 score that sklearn.metrics.f1_score gives at :78 (total_frames there only sizes the arrays).
 * Both clips pass through the same arithmetic.  ws: B + both clips' ast_onset_detect counts + B (T_max_orig + T_max_gen) floats. */
long ast_onset_accuracy_ws_floats(int B, int n_orig, int n_gen);
int ast_onset_accuracy_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                           const int32_t* len_gen, int pad_mode, const int32_t* mel_table, float* ws, long ws_floats, float* out,
                           void* stream);
/* librosa.segment.recurrence_matrix(mfcc.T) at its defaults (evaluation_style_transfer.py:122-126): the reference hands over the
 * transpose, so the matrix's points are the 20 coefficient rows c_i of librosa.feature.mfcc(y, sr) (hop 512), each a vector over
 * the clip's own T_b frames.  D[i][j] = ||c_i - c_j||_2, summed as squared differences (no Gram matrix), per chunk of frames in
 * f32 and over the chunks ascending in double, rounded to f32 once: dist2 shows exactly what is ranked.  Per column j: the min(19, k + 2) = 12 nearest other rows, ties to the lower index;
 * those at distance exactly 0 dropped; of the rest the k = 2 ceil(sqrt(19)) = 10 nearest kept.  R (B, 20, 20) int32: R[b][i][j] = 1
 * iff row i is kept for column j; the diagonal is 0, the matrix is not symmetrised.  dist2: NULL, or (B, 20, 20) f32, the squared
 * distances (for the tests).  A T x T matrix over time frames is not built.
 * ws: the MFCC's first pass at hop 512 + B 20 T_max + B ceil(T_max / chunk) 190 floats. */
long ast_recurrence_ws_floats(int B, int n);
int ast_recurrence_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, const int32_t* mel_table, float* ws,
                       long ws_floats, int32_t* R, float* dist2, void* stream);
/* self_similarity_distance (evaluation_style_transfer.py:121-133): each clip at its own length; out[b] = the mean over the 400 cells
 * of |R_a - R_b|, a multiple of 1 / 400.  Equal clips score exactly 0.  ws: both clips' ast_recurrence counts + 2 B 400 floats. */
long ast_self_similarity_distance_ws_floats(int B, int n_a, int n_b);
int ast_self_similarity_distance_len(const float* a, int n_a, const float* b, int n_b, int B, const int32_t* len_a, const int32_t* len_b,
                                     int pad_mode, const int32_t* mel_table, float* ws, long ws_floats, float* out, void* stream);

/* ---- deterministic forms (ast_amd.set_deterministic / AST_DETERMINISTIC) ---------------------------------------------------
 * The default entry points sum partials that cross workgroups with f32 atomics, in arrival order.  The forms below STORE every
 * workgroup's partial into a slot indexed by its workgroup / tile / row id (plain stores; every slot is written on every call, so
 * nothing needs to be zeroed first) and reduce the slots in ascending order, so two calls on the same inputs give bit-identical
 * results whatever the launch timing.  ws is f32 scratch owned by the caller; nslots is the caller's (fixed) number of slots,
 * 1 .. AST_DET_MAX_SLOTS.  Elsewhere in this header: ast_igemm flags bit 12 and ast_igemm_ws_floats_det (split-K slabs), and
 * ast_wgrad_slab + ast_slab_sum (weight gradients).  Every kernel these forms launch is an instantiation without float atomics
 * (compile-time DET / SLAB template parameters; tools/det_isa_audit.py checks the code objects). */
#define AST_DET_MAX_SLOTS 65536
#define AST_IGEMM_DETERMINISTIC 4096
/* out[b][i] (+)= sum_{s < nslots} parts[(b*nslots + s)*n + i], s ascending (accumulate: add to out, else overwrite) */
int ast_ordered_sum(const float* parts, int64_t n, int nslots, int batches, float* out, int accumulate, void* stream);
/* ast_igemm with flags bit 12 (on EVERY call in deterministic mode: it selects the atomic-free kernel instantiations): the split-K slices STORE into their own [M][Cd] slab of ws (nslices * M * Cd floats: this function,
 * 0 when the plan does not split K) and the finish pass sums them in slice order; fused statistics (flags 8/16/64) are refused. */
long ast_igemm_ws_floats_det(const ast_gather_t* g, int dtype);
/* ast_sumsq: out[0] += sum x^2 through nslots workgroup partials (ws >= nslots floats) */
int ast_sumsq_det(const float* x, int64_t n, float* out, float* ws, int nslots, void* stream);
/* ast_colsum_acc: out[c] += sum_r x[r][c] through nslots row-slice partials (ws >= nslots * Creal floats) */
int ast_colsum_acc_det(const void* x, int64_t rows, int C, int Creal, float* out, int dtype, float* ws, int nslots, void* stream);
/* ast_chan_stats: sums[n][c] = {sum x, sum x^2}, overwritten (no zeroing needed); ws >= N * nslots * C * 2 floats */
int ast_chan_stats_det(const void* x, float* sums, int N, int HW, int C, int dtype, float* ws, int nslots, void* stream);
/* ast_norm_bwd_sums_pre: sums3[n][c] = {sum dz, sum dz*x, sum dz*r}, overwritten; ws >= N * nslots * C * 3 floats */
int ast_norm_bwd_sums_det(const void* dy, const void* y, const void* x, const void* r, float* sums3, int N, int HW, int C, int relu,
                          int dtype, const float* scale1, const float* shift1, const float* scale2, const float* shift2, float* ws,
                          int nslots, void* stream);
/* ast_layernorm_bwd / ast_add_drop_ln_bwd: dgamma / dbeta ADDED from per-row partials (one slot per row, rows <= AST_DET_MAX_SLOTS),
 * ws >= 2 * rows * D floats */
int ast_layernorm_bwd_det(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                          float* dgamma, float* dbeta, int rows, int D, int dtype, float* ws, void* stream);
int ast_add_drop_ln_bwd_det(const float* dy, const float* ds_ext, const float* s, const float* gamma, const float* mean,
                            const float* rstd, const float* mask, float* dx, float* dsub, float* dgamma, float* dbeta, int rows,
                            int D, float* ws, void* stream);
/* ast_recon_loss_total with one slot per 256-bin workgroup: ws >= 5 * ceil(B*T*Fq / 256) floats (ws_floats checked) */
int ast_recon_loss_total_det(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, const float* coef5,
                             const float* inv5, float* ws, long ws_floats, float* res11, float* grad, void* stream);
/* ast_bigk_gemm / ast_bign_dgrad (decoder="simple"): every K chunk (n chunk) stores its partial into its own [M][N] ([M][K]) slab of
 * ws (the *_ws_floats functions; <0 on bad sizes), summed in chunk order into y / dx (overwritten; ast_bigk_gemm_det needs ldy == N) */
long ast_bigk_gemm_det_ws_floats(int M, int N, int K);
int ast_bigk_gemm_det(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, float* ws, long ws_floats, void* stream);
long ast_bign_dgrad_det_ws_floats(int M, int N, int K);
int ast_bign_dgrad_det(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, float* ws, long ws_floats, void* stream);
/* ast_weight_grads_flush_t with the <dWp, W/sigma> inner products through per-tile partials (ws >= ntiles floats) summed in tile order */
int ast_weight_grads_flush_det(const ast_weight_desc_t* descs, const void* tiles, int ntiles, float* ws, long ws_floats, void* stream);

/* ---- wide token path: 65 .. AST_WIDE_MAX_ROWS token rows (f32) ----------------------------------------------------------------
 * The entries above stop at 64 rows (one 16-row tile per workgroup, sized for B*(S+1) <= 40).  These take M in
 * 65 .. AST_WIDE_MAX_ROWS and refuse anything else; a workgroup covers 64 rows (four 16-row v_mfma_f32_16x16x4_f32 accumulator
 * tiles per wave), so a weight byte is fetched once per 64 rows.  Arguments, epilogues, alignment and K / ldw rules are those of
 * the <= 64-row entry named in each line, which runs the same kernel template with one row tile per wave (csrc/skinny.hip); only the
 * wide entries check ldw >= K, ldy >= N and lddy >= N.  Only ast_bigk_gemm_wide and ast_bign_dgrad_wide (default mode) add with f32 atomics.
 * ast_skinny_gemm_wide[_ex]: every token linear of the transformer stacks (style_encoder.py:181-191, content_encoder.py:24-26,
 *   new_decoder.py:49-51,111-119) and embedding_to_stft forward (SimpleDecoder_TransformerOnly.py:17,62-66) at a larger batch.
 *   The dropout mask of element (m, n) depends on (seed, counter, m * ldy + n) only, as in ast_skinny_gemm_ex.
 * ast_linear_wgrad_wide: dW += dy^T x, db += colsum(dy) (both linears of SimpleDecoder_TransformerOnly.py:16-17 and any token
 *   linear without a weight bank).  A wave owns its dW tile, walks the rows in ascending 64-row chunks and does one read-add-store:
 *   deterministic by construction, used in both modes.
 * ast_bigk_gemm_wide[_det]: stft_to_embedding (SimpleDecoder_TransformerOnly.py:16,56-60).  _det: one [M][N] slab per 1024-k chunk in
 *   ws (ast_bigk_gemm_wide_det_ws_floats = ceil(K/1024) * M * N; -1 on refused sizes) + ast_ordered_sum; needs ldy == N.
 * ast_bign_dgrad_wide[_det]: data gradient of embedding_to_stft (SimpleDecoder_TransformerOnly.py:17,62-66), K <= 256.  _det: one
 *   [M][K] slab per 512-n chunk (ast_bign_dgrad_wide_det_ws_floats = ceil(N/512) * M * K; -1 on refused sizes) + ast_ordered_sum. */
#define AST_WIDE_MAX_ROWS 1024
int ast_skinny_gemm_wide(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy, int relu,
                         void* stream);
int ast_skinny_gemm_wide_ex(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy,
                            int relu, const float* mul_mask, float* drop_mask, float p, uint64_t seed, const int64_t* d_offset,
                            void* stream);
int ast_linear_wgrad_wide(const float* dy, const float* x, float* dW, float* db, int M, int N, int K, int lddy, int ldw, void* stream);
int ast_bigk_gemm_wide(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldy, void* stream);
long ast_bigk_gemm_wide_det_ws_floats(int M, int N, int K);
int ast_bigk_gemm_wide_det(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, float* ws, long ws_floats,
                           void* stream);
int ast_bign_dgrad_wide(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, void* stream);
long ast_bign_dgrad_wide_det_ws_floats(int M, int N, int K);
int ast_bign_dgrad_wide_det(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, float* ws, long ws_floats,
                            void* stream);

/* ---- embedding_to_stft at inference: any row count, per-clip section counts (f32) ---------------------------------------------
 * y[m][n] = bias[n] + sum_k x[m][k] w[n][k] for the rows m = b S + s of a padded batch with s < clamp(n_valid[b], 1, S); every other
 * row is written as exactly 0 in every column n < N (no bias), and its x row is never read (NaN there reaches nothing).  Columns
 * >= N of y are not touched.  n_valid is an int32 (M / S,) DEVICE array read by the kernel, so one captured graph serves every mix
 * of lengths; the values cannot be checked without a sync, so the kernel clamps them (as ast_attn_fwd_len does).  n_valid == NULL:
 * every row counts (S must still divide M).  Replaces generate_output (SimpleDecoder_TransformerOnly.py:17,62-66) where
 * ast_skinny_gemm[_wide] cannot run: more than AST_WIDE_MAX_ROWS rows, or a padded batch.
 * Checked on the host (ast_last_error names the entry): x, w, y non-null; 1 <= M <= AST_BIGN_MAX_ROWS; S >= 1 and M % S == 0;
 * 1 <= N <= 16 * 65535; K, ldw, ldy and alignment as ast_skinny_gemm_wide (K % 4 == 0, 4 <= K <= 1024, ldw % 4 == 0, ldw >= K,
 * ldy >= N, x and w 16-byte aligned; x rows are K apart).
 * The kernel is the body of ast_skinny_gemm_wide (csrc/skinny.hip: v_mfma_f32_16x16x4_f32, 64 rows x 16 n per workgroup, no float
 * atomics) with the row mask added: each element is one dot product in a k order that depends on K alone, so a row has the same
 * bits whatever batch it sits in, repeats are bitwise equal, and with every row counting the result equals ast_skinny_gemm[_wide]
 * bit for bit.  A 16-row tile without a row that counts issues no load of x and no MFMA; a workgroup of four such tiles loads
 * nothing and only stores zeros.  Inference only: no backward. */
#define AST_BIGN_MAX_ROWS 4096          /* 8 clips x 500 sections, rounded up */
int ast_bign_gemm_len(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy, int S,
                      const int32_t* n_valid /* (M/S,) device, or NULL */, void* stream);

/* ---- backward of the length-masked output linear: training on a padded batch (f32) ----------------------------------------------
 * The row mask of ast_bign_gemm_len (row m = b S + s counts iff s < clamp(n_valid[b], 1, S); n_valid == NULL: every row counts;
 * n_valid an int32 (M / S,) DEVICE array, clamped by the kernels) for 1 <= M <= AST_WIDE_MAX_ROWS rows; M % S == 0 is checked on
 * the host, and ast_last_error names the entry.
 * ast_bign_dgrad_len[_det]: dx[m][k] = sum_n dy[m][n] w[n][k], K <= 256, lddy >= N; the entry picks the 1-row-tile (M <= 64) or the
 *   4-row-tile form of ast_bign_dgrad[_wide] itself.  A row that does not count is never read from dy (clamped address, operand
 *   selected to zero) and its dx row is exactly 0; a 16-row tile without a counting row issues no dy load and no MFMA; a
 *   workgroup all of whose tiles are such tiles leaves before any load.  The default form zeroes dx and adds with f32 atomics; _det
 *   writes one [M][K] slab per 512-n chunk into ws (ast_bign_dgrad_len_det_ws_floats = ceil(N/512) * M * K floats, -1 on refused
 *   sizes) and adds the slabs in chunk order (ast_ordered_sum): with n_valid == NULL its bits are those of ast_bign_dgrad[_wide]_det.
 * ast_linear_wgrad_len: dW[n][k] += sum_{m counts} dy[m][n] x[m][k], db[n] += sum_{m counts} dy[m][n] (db may be NULL); lddy >= N,
 *   ldw >= K, x rows are K apart, N <= 64 * 65535.  The kernels of ast_linear_wgrad[_wide] (one batch of 16 / 32 / 64 rows, 64-row
 *   chunks beyond; no atomics, both modes) with the mask, formed once per wave and batch: rows that do not count are read from
 *   neither dy nor x (NaN there reaches nothing), a 64-row chunk without a counting row is skipped.  With n_valid == NULL the result has the bits of ast_linear_wgrad[_wide].  Needed for both big linears of
 *   SimpleDecoder_TransformerOnly.py:16-17 on a padded batch: the padded target sections that stft_to_embedding reads are user
 *   data and may hold anything. */
int ast_bign_dgrad_len(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, int S,
                       const int32_t* n_valid /* (M/S,) device, or NULL */, void* stream);
long ast_bign_dgrad_len_det_ws_floats(int M, int N, int K);
int ast_bign_dgrad_len_det(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, int S, const int32_t* n_valid,
                           float* ws, long ws_floats, void* stream);
int ast_linear_wgrad_len(const float* dy, const float* x, float* dW, float* db, int M, int N, int K, int lddy, int ldw, int S,
                         const int32_t* n_valid /* (M/S,) device, or NULL */, void* stream);

/* ---- BatchNorm(+ReLU) over the live images of a padded batch: the CNN halves of new_decoder.py in ragged training -----------
 * The N = B * S NHWC images are the sections of B clips, image n = b * S + s; n_sections is an int32 (B,) DEVICE array, clamped
 * by the kernels to n_b = clamp(n_sections[b], 1, S) and never read on the host (one captured graph serves every mix of
 * lengths).  Image n is LIVE iff s < n_b.  1 <= B, S <= 65535 and B * S <= 2^24 images.  These are the separate-pass chain above (ast_chan_stats -> ast_norm_finalize ->
 * ast_affine_act; ast_norm_bwd_sums_pre -> ast_norm_bwd_finalize -> ast_norm_bwd_apply_pre) with batch statistics, backward sums
 * and the pixel count HW * sum_b n_b (formed on the device) taken over the live images only.  The launch grid is (blocks per
 * image, S, B), so liveness is one compare per workgroup; the pixel loops of live images are the bodies of the plain kernels.
 *   ast_chan_stats_len        adds {sum x, sum x^2} into the rows of live images of sums[N][C][2] (zeroed by the caller: the
 *                             shared scratch); workgroups of dead images leave before any load, and their rows are not read again.
 *   ast_norm_finalize_len     one wave per channel over the live rows: mean, rstd, scale = gamma rstd, shift = beta - mean scale
 *                             (padded channels c >= Creal: scale = shift = 0), running statistics (momentum 0.1, unbiased factor
 *                             cnt / max(cnt - 1, 1); either both or neither), *num_batches_tracked += 1 when not NULL.  EVERY row of
 *                             sums is left zero, dead ones without being read.
 *   ast_affine_act_len        live images: ast_affine_act (relu bit 0).  Dead images: zeros stored, x not loaded.
 *   ast_norm_bwd_sums_len     {sum dz, sum dz x} of the live images into sums3[N][C][3] (zeroed by the caller), dz = dy under the
 *                             ReLU mask: from y, or recomputed from fma(x, scale1, shift1) when scale1 != NULL (y may be NULL then).
 *   ast_norm_bwd_finalize_len dgamma[c] += Q, dbeta[c] += sum dz (either may be NULL), k1[C][3] the dx coefficients, all from
 *                             the live sums and the device count; every row of sums3 is left zero.
 *   ast_norm_bwd_apply_len    live images: ast_norm_bwd_apply_pre's dx = k1 (dz, x, 1).  Dead images: dx stored as exact 0, dy, y
 *                             and x not loaded (NaN there reaches nothing).
 * Atomic (default-mode) reductions only: no deterministic and no cross-rank form. */
int ast_chan_stats_len(const void* x, float* sums, int B, int S, int HW, int C, int dtype, const int32_t* n_sections, void* stream);
int ast_norm_finalize_len(float* sums, int64_t* num_batches_tracked, int B, int S, int HW, int C, int Creal, const float* gamma,
                          const float* beta, float* running_mean, float* running_var, float eps, float* mean, float* rstd,
                          float* scale, float* shift, const int32_t* n_sections, void* stream);
int ast_affine_act_len(const void* x, const float* scale, const float* shift, void* y, int B, int S, int HW, int C, int relu,
                       int dtype, const int32_t* n_sections, void* stream);
int ast_norm_bwd_sums_len(const void* dy, const void* y, const void* x, float* sums3, int B, int S, int HW, int C, int relu, int dtype,
                          const float* scale1, const float* shift1, const int32_t* n_sections, void* stream);
int ast_norm_bwd_finalize_len(float* sums3, int B, int S, int HW, int C, int Creal, const float* gamma, const float* mean,
                              const float* rstd, float* dgamma, float* dbeta, float* k1, const int32_t* n_sections, void* stream);
int ast_norm_bwd_apply_len(const void* dy, const void* y, const void* x, const float* k1, void* dx, int B, int S, int HW, int C,
                           int relu, int dtype, const float* scale1, const float* shift1, const int32_t* n_sections, void* stream);
/* The two layout ops at the decoder's ends under the same mask: ast_nchw_to_nhwc / ast_bilinear_fwd / ast_bilinear_bwd on live
 * images; a dead image's output (y, resp. dx) is exact 0 and its input is never read, so padded target sections and the
 * gradient of padded output sections may hold anything, NaN included. */
int ast_nchw_to_nhwc_len(const float* x, void* y, int B, int S, int C, int H, int W, int64_t sn, int64_t sc, int64_t sh, int Cp,
                         int dtype, const int32_t* n_sections, void* stream);
int ast_bilinear_fwd_len(const void* x, float* y, int B, int S, int C, int Cp, int H, int W, int Ho, int Wo, int dtype,
                         const int32_t* n_sections, void* stream);
int ast_bilinear_bwd_len(const float* dy, void* dx, int B, int S, int C, int Cp, int H, int W, int Ho, int Wo, int dtype,
                         const int32_t* n_sections, void* stream);

/* ---- token programs: transformer layers in one launch (csrc/tokprog.hip) ------------------------------------------------
 * Replaces, for the <= 64 token rows of the transformer stacks (style_encoder.py:181-191, content_encoder.py:24-26,
 * new_decoder.py:49-51,111-119), the per-operator launches above (ast_skinny_gemm*, ast_attn_fwd_p / ast_attn_bwd_p,
 * ast_add_drop_ln_fwd / _bwd) by ONE launch that walks a list of ops with a grid barrier between them.  All tensors are
 * f32 row-major; an op reads what earlier ops of the same launch wrote.  ast_tok_max_ops() ops per launch at most.
 *   AST_TOK_GEMM      y[M][N] = epi(x[M][K] w[N][K]^T): i = {M, N, K, ldx, ldw, ldy}; in = {x, w, bias?, mul_mask?, addend?};
 *                     out = {y, drop_mask?}; flags & 1: ReLU.  epi: +bias, ReLU, dropout (p, seed; the combined ReLU &
 *                     dropout mask goes to drop_mask), * mul_mask, + addend.  M <= 64, N % 16 == 0, K % 64 == 0.
 *   AST_TOK_ATTN_FWD  softmax(q k^T / sqrt(dh)) v per (batch, head), Lq, Lk <= 8: i = {B, H, Lq, Lk, dh, ldq, ldk, ldo}; in = {q, k, v};
 *                     out = {o, probs (B,H,Lq,Lk)}; flags & 4: causal; p, seed: dropout on the probabilities (redrawn by _BWD).
 *   AST_TOK_ATTN_BWD  same i; in = {dout, q, k, v, probs}; out = {dq, dk, dv}.
 *   AST_TOK_ADLN_FWD  s = x + dropout(sub), y = LayerNorm(s): i = {rows, 256}; in = {x?, sub, gamma?, beta?};
 *                     out = {mask?, s?, y?, mean?, rstd?}; p, seed, eps.
 *   AST_TOK_ADLN_BWD  ds = ds_ext + LayerNorm_bwd(dy; s), dx = ds, dsub = ds * mask: i = {rows, 256};
 *                     in = {dy?, ds_ext?, s, gamma, mean, rstd, mask?}; out = {dx?, dsub?, dgamma?, dbeta?} (+= for the last two).
 * flags & AST_TOK_NO_BARRIER: the next op does not depend on this one (no grid barrier between them).
 * G (<= 32) workgroups do the work (those of an 8 G grid that land on XCD xcd); sync = 32 zeroed uint32 (128-byte aligned) owned by this
 * call chain (launches that may run concurrently need their own); *status becomes 1 if a barrier wait timed out;
 * d_offset = the device step counter of the dropout draws (as ast_dropout_fwd). */
enum { AST_TOK_GEMM = 1, AST_TOK_ATTN_FWD = 2, AST_TOK_ATTN_BWD = 3, AST_TOK_ADLN_FWD = 4, AST_TOK_ADLN_BWD = 5 };
enum { AST_TOK_RELU = 1, AST_TOK_NO_BARRIER = 2, AST_TOK_CAUSAL = 4 };
typedef struct {
  int32_t type, flags;
  int32_t i[8];
  float p, eps;
  uint64_t seed;
  const float* in[7];
  float* out[5];
} ast_tok_op_t;
int ast_tok_max_ops(void);
int ast_tok_program(const ast_tok_op_t* ops, int nops, int G, int xcd, void* sync, int* status, const int64_t* d_offset,
                    void* stream);

/* ---- dataset screening: the reference's Preprocessing_Dataset scripts for a padded batch (csrc/curation.hip; DESIGN 7, "Dataset
 * screening"; parity with librosa's and pydub's own output is unpinned).  Rows, counts, clamps, pad modes and limits as for the
 * spectrogram metrics above; at any sample rate -- a rate enters only through `win` and the mel table.  No atomics; results are
 * bit-reproducible and row b does not depend on the other rows.  Every workspace slot that is read is written first. */
/* frames per workgroup of the frame-RMS pass and frames per partial of the mel-mean pass (what the workspace counts are built on) */
int ast_frame_rms_tile_frames(void);
int ast_mfcc_mean_chunk_frames(void);
/* librosa.feature.rms(y)[0] at its defaults, the silent-frame share of silent_tracks_dataset.py:20-27 and the clip level
 * sqrt(mean(y^2)) of dataset_tracks_analysis.py:27, in one pass over the samples: frame_length 2048, hop 512, centred,
 * T_b = 1 + L_b / 512.  rms (B, T_max) f32, T_max = 1 + n / 512: rms[b][t] = sqrt(mean of the padded clip's samples
 * [512 t - 1024, 512 t + 1024) squared), 0 for t >= T_b.  A frame is four hop blocks of 512 samples: a workgroup forms each
 * block's sum of squares once (a fixed tree) and adds four of them per frame in ascending block order.
 * n_frames[b] = T_b; silent[b] = the frames with rms < threshold (int32); silence_ratio[b] = silent / T_b;
 * level[b] = sqrt(S_b / L_b) with S_b the sum of squares of the clip's own L_b samples in double, rounded once; sumsq[b] = S_b
 * (double (B,), may be NULL: what ast_gain_rows_len takes).  With AST_PAD_REFLECT L_b is clamped to [1025, n] for the level too.
 * ws: 3 B ceil(T_max / tile) floats, 8-byte aligned (a double and an int32 per tile). */
long ast_frame_rms_ws_floats(int B, int n);
int ast_frame_rms_len(const float* waves, int B, int n, const int32_t* n_samples, float threshold, int pad_mode, float* ws,
                      long ws_floats, float* rms, int32_t* n_frames, int32_t* silent, float* silence_ratio, float* level,
                      double* sumsq, void* stream);
/* is_mostly_sound (split_BachViolinDataset.py:24-30) on float samples at full scale 1.0: non-overlapping windows of `win` samples
 * (the caller's sample_rate / 10 for the script's 100 ms), W_b = L_b / win of them; mask (B, W_max) int32, W_max = n / win:
 * mask[b][w] = 1 when 20 log10(rms_w) > threshold_db (an rms_w of 0 is never sound), 0 for w >= W_b; sound_ratio[b] = the clip's
 * ones / W_b, exactly 0 when W_b = 0.  One wave per window.  mask may be NULL when W_max = 0.  No workspace. */
int ast_window_sound_len(const float* waves, int B, int n, const int32_t* n_samples, int win, float threshold_db, int32_t* mask,
                         float* sound_ratio, void* stream);
/* np.mean(librosa.feature.mfcc(y, sr, n_mfcc), axis=1) (dataset_tracks_analysis.py:28-29, dataset_variety.py:13-16) without the
 * per-frame DCT: out (B, n_mfcc) f32 = the first n_mfcc <= 20 coefficients of the orthonormal DCT-II, in double, of the time-mean
 * over the clip's T_b = 1 + L_b / hop frames of its clamped mel dB rows (the DCT is linear).  The rows are ast_mfcc_len's first
 * pass, unchanged; mel_table as there, built by ast_mel_table for the clip's own sample rate.  hop 256 or 512.
 * ws: ast_mfcc_ws_floats(B, n, hop) + 128 B ceil(T_max / chunk) floats. */
long ast_mfcc_mean_ws_floats(int B, int n, int hop);
int ast_mfcc_mean_len(const float* waves, int B, int n, const int32_t* n_samples, int n_mfcc, int hop, int pad_mode,
                      const int32_t* mel_table, float* ws, long ws_floats, float* out, void* stream);
/* rms_normalize (unifies_violin_datasets.py:25-30): out[b][i] = waves[b][i] * g_b for i < L_b, 0 behind;
 * g_b = target_rms / sqrt(sumsq[b] / L_b) in double, rounded once, and 1 where the level is 0.  sumsq: ast_frame_rms_len's, taken
 * with AST_PAD_CONSTANT (the same clamp of L_b).  out may be waves.  No workspace. */
int ast_gain_rows_len(const float* waves, int B, int n, const int32_t* n_samples, const double* sumsq, double target_rms, float* out,
                      void* stream);

/* ---- state digest: what a resumable checkpoint is verified with (csrc/digest.hip; DESIGN 10, "Resuming") -------------------
 * The reference saves four state_dicts (evaluation_style_transfer.py:246-252) and has nothing that checks a restored run; this
 * is the project's own.  *out (device, 8-byte aligned) = one 64-bit digest over the exact bytes of the n device tensors
 * ptrs[e][0, nbytes[e]), in list order (ptrs and nbytes are HOST arrays):
 *   mix64(SEED + sum_e mix64((mix64(e) ^ LEN_KEY) + nbytes[e]) + sum_i mix64(mix64(i) ^ w_i))   mod 2^64,
 * w_i the i-th little-endian 32-bit word of the list (every entry starts a new word, its last word padded with zero bytes; i runs
 * on over the entries), mix64 the splitmix64 finaliser, SEED 0x4153545F44494753, LEN_KEY 0xA5A5A5A5A5A5A5A5
 * (tests/state_digest_ref.py is the same function in Python).  One flipped bit changes one term and so the digest; the word
 * index sits inside the term, so swapped words change it; the terms are combined by wrap-around integer addition, so the value
 * is the same for every launch geometry and every order in which the workgroups finish.  Any byte count, any pointer
 * alignment (16-byte loads where the entry allows them, byte loads for a pointer that is not 4-byte aligned), zero-length
 * entries (their pointer may be NULL) and n = 0.  A null list, a null out, n < 0, a negative size or a null pointer with a
 * positive size return an error before anything is launched.  2 + (entries with bytes) launches on `stream`. */
int ast_state_digest(const void* const* ptrs, const long long* nbytes, int n, unsigned long long* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
