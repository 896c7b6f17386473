// The C ABI of _madnn_kernels.so: every C-linkage entry point of the .hip files, declared once.
//
// Each .hip file includes this header, so the compiler checks its definitions against these declarations
// ("conflicting types" on a mismatch); binding.cpp and any other caller include it too, so a call is checked
// against the same text.  Grouped by defining file, in build.KERNEL_SOURCES order.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "attn.h"

extern "C" {

// ---- bucket.hip ----
hipError_t madnn_bucket_pack(void* const* srcs, const int64_t* offs, const int64_t* numels, int n, void* flat,
                             int src_dt, int flat_dt, float scale, hipStream_t stream);
hipError_t madnn_bucket_unpack(void* const* dsts, const int64_t* offs, const int64_t* numels, int n, void* flat,
                               int dst_dt, int flat_dt, float scale, hipStream_t stream);
hipError_t madnn_flat_scale_cast(const void* src, void* dst, int64_t n, int src_dt, int dst_dt, float scale,
                                 hipStream_t stream);

// ---- optim.hip ----
int madnn_optim_tune(int key, int value);
hipError_t madnn_sgd_step(float* master, const void* grad, int grad_dt, float* mom, void* model, int model_dt,
                          int64_t n, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                          int first_step, float grad_scale, const float* dscale, hipStream_t stream);
hipError_t madnn_adam_step(float* master, const void* grad, int grad_dt, float* m1, float* m2, void* model,
                           int model_dt, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                           int adamw, float bias_corr1, float bias_corr2_sqrt, float grad_scale, const float* dscale,
                           hipStream_t stream);
int madnn_sqnorm_grid(int64_t n);
hipError_t madnn_sqnorm_partial(const void* x, int dt, int64_t n, float scale, float* partial, int grid,
                                hipStream_t stream);
hipError_t madnn_norm_finalize(const float* partial, int np, float max_norm, float* out, hipStream_t stream);

// ---- norm.hip ----
int madnn_norm_tune(int key, int value);
int madnn_norm_max_h();
hipError_t madnn_norm_fwd(const void* x, const void* res, const void* w, const void* b, void* y, void* sum_out,
                          float* mean_out, float* rstd_out, int64_t rows, int H, float eps, int rms, int xdt, int wdt,
                          hipStream_t stream);
// K3 DROP forward: sum_out = res + rp * m * x, y = norm(sum_out); threshold in 1..256 (see dropout.h)
hipError_t madnn_norm_drop_fwd(const void* x, const void* res, const void* w, const void* b, void* y, void* sum_out,
                               float* mean_out, float* rstd_out, int64_t rows, int H, float eps, int rms, int xdt,
                               int wdt, uint32_t threshold, uint64_t seed, uint64_t offset, hipStream_t stream);
int64_t madnn_norm_bwd_workspace(int64_t rows, int H);
// dsum (optional, [H], bf16 if dsum_bf16 else fp32): column sums of dx over the rows (norm_bwd_kernel CS)
hipError_t madnn_norm_bwd(const void* dy, const void* x, const void* w, const float* mean_in, const float* rstd_in,
                          const void* dres, void* dx, void* dw, void* dbias, void* dsum, int dsum_bf16,
                          float* workspace, int64_t rows, int H, int rms, int xdt, int wdt, hipStream_t stream);
// K3 DROP backward: dx = dh (the residual's gradient), dx_drop = rp * m * dh; dsum: column sums of dx_drop
hipError_t madnn_norm_drop_bwd(const void* dy, const void* x, const void* w, const float* mean_in,
                               const float* rstd_in, const void* dres, void* dx, void* dx_drop, void* dw, void* dbias,
                               void* dsum, int dsum_bf16, float* workspace, int64_t rows, int H, int rms, int xdt,
                               int wdt, uint32_t threshold, uint64_t seed, uint64_t offset, hipStream_t stream);

// ---- bn.hip ----
// key 0: apply passes walk back to front (0/1), 1: apply workgroups per CU, 2: coefficient hoisting
// (0/1), 4: reduction workgroups (partial rows) per CU; value < 0 only reads.
// Key 4 sizes the partial slabs: change it only between steps (every call sizes its own workspace).
// Returns the old value (-1 for an unknown key).
int madnn_bn_tune(int key, int value);
int madnn_bn_supported(int C);
int madnn_bn_partial_rows(int64_t M, int C);
// scratch floats the producer-partial paths need to fold many partial rows (prereduce)
int madnn_bn_prereduce_floats(int C);
// Forward. training: compute batch stats (+ running update); else use running stats.
// ext_partial: [ext_rows][2][C] per-channel (sum, sum of squares) of x already produced by
// the kernel that wrote x (K9 conv1x1 epilogue); the statistics pass over x is skipped.
hipError_t madnn_bn_fwd(const void* x, const void* res, void* y, unsigned char* mask, int64_t M, int C, int xdt,
                        int relu, int training, float eps, float momentum, const float* w, const float* b,
                        float* run_mean, float* run_var, int64_t* nbt, float* save_mean, float* save_invstd,
                        float* scale, float* shift, float* workspace, const float* ext_partial, int ext_rows,
                        hipStream_t stream);
// The backward's reduction and finalize without the apply pass: dw / db and the per-channel coefficients
// coef = ca | cb | cc of dx = ca g + cb x + cc ([3][C]), for a consumer that applies them itself (K9F).
hipError_t madnn_bn_bwd_coef(const void* dy, const void* x, const unsigned char* mask, int has_res, int64_t M, int C,
                             int xdt, int relu, const float* w, const float* save_mean, const float* save_invstd,
                             const float* scale, const float* shift, float* dw, float* db, float* coef,
                             float* workspace, hipStream_t stream);
hipError_t madnn_bn_bwd(const void* dy, const void* x, const unsigned char* mask, int has_res, void* dx, void* dres,
                        int64_t M, int C, int xdt, int relu, const float* w, const float* save_mean,
                        const float* save_invstd, const float* scale, const float* shift, float* dw, float* db,
                        float* coef, float* workspace, hipStream_t stream);
// Training forward of relu(BN(x) + BN_r(r)): ResNet's last bottleneck BatchNorm with the downsample
// path's BatchNorm folded into the same apply pass (bf16 only).  Each BN's statistics come from its
// producer's epilogue (ext_partial*) or a statistics pass; both finalize into their own coefficients
// and running statistics; one pass then writes y and the ReLU bit mask.
hipError_t madnn_bn_fwd_dual(const void* x, const void* r, void* y, unsigned char* mask, int64_t M, int C, float eps,
                             float momentum, const float* w, const float* b, float* run_mean, float* run_var,
                             int64_t* nbt, float* save_mean, float* save_invstd, float* scale, float* shift,
                             const float* ext_partial, int ext_rows, float eps_r, float momentum_r, const float* w_r,
                             const float* b_r, float* run_mean_r, float* run_var_r, int64_t* nbt_r,
                             float* save_mean_r, float* save_invstd_r, float* scale_r, float* shift_r,
                             const float* ext_partial_r, int ext_rows_r, float* workspace, hipStream_t stream);
// The dual backward's reduction and its two finalizes without the apply pass: dw / db of both BatchNorms and
// coef = ca | cb | cc (dx = ca g + cb x + cc) followed by the residual BatchNorm's ca | cb | cc over r
// ([6][C]), for consumers that apply them themselves (K9F on both convolutions of a downsample block).
// workspace: bn_partial_rows(M, C) * 3 * C floats.
hipError_t madnn_bn_bwd_dual_coef(const void* dy, const void* x, const void* r, const unsigned char* mask, int64_t M,
                                  int C, const float* w, const float* save_mean, const float* save_invstd,
                                  const float* w_r, const float* save_mean_r, const float* save_invstd_r, float* dw,
                                  float* db, float* dw_r, float* db_r, float* coef, float* workspace,
                                  hipStream_t stream);
// Backward of madnn_bn_fwd_dual: one reduction pass (sum g, sum g*x, sum g*r), two finalizes, one
// apply pass writing dx and dr.  workspace: bn_partial_rows(M, C) * 3 * C floats; coef: 6 * C.
hipError_t madnn_bn_bwd_dual(const void* dy, const void* x, const void* r, const unsigned char* mask, void* dx,
                             void* dr, int64_t M, int C, const float* w, const float* save_mean,
                             const float* save_invstd, const float* w_r, const float* save_mean_r,
                             const float* save_invstd_r, float* dw, float* db, float* dw_r, float* db_r, float* coef,
                             float* workspace, hipStream_t stream);
// Training statistics + finalize only (see bn_coef in binding.cpp): the apply runs in a consumer.
hipError_t madnn_bn_coef(const void* x, int64_t M, int C, float eps, float momentum, const float* w, const float* b,
                         float* run_mean, float* run_var, int64_t* nbt, float* save_mean, float* save_invstd,
                         float* scale, float* shift, float* workspace, const float* ext_partial, int ext_rows,
                         hipStream_t stream);
// The backward finalize on its own (fused consumers with their own reduction pass: pool.hip)
hipError_t madnn_bn_bwd_finalize(const float* partial, int G, int C, int pstride, int qoff, int64_t M, const float* w,
                                 const float* mean, const float* invstd, float* dw, float* db, float* ca, float* cb,
                                 float* cc, hipStream_t stream);
// BatchNorm(+ReLU) backward whose reduction came from the producer of dy (K13's / K9's data-grad
// epilogue: partial [G][2][C] = (sum g, sum g*x)): finalize + apply only.  coef: 3 * C floats.
// scratch: madnn_bn_prereduce_floats(C) floats
hipError_t madnn_bn_bwd_ext(const void* dy, const void* x, void* dx, int64_t M, int C, int relu, const float* w,
                            const float* save_mean, const float* save_invstd, const float* scale, const float* shift,
                            float* dw, float* db, float* coef, const float* partial, int G, float* scratch,
                            hipStream_t stream);

// ---- xent.hip ----
// chunks per lane the fused kernel needs for a row of ld 16-bit elements (0 = not supported)
int madnn_xent_fused_chunks(int64_t ld);
hipError_t madnn_xent_fused(const void* logits, int dt, const int64_t* targets, int64_t n_loss_rows, int64_t seq,
                            int64_t ld, int V, int ignore_index, int64_t n_rows_all, const float* gscale, float* loss,
                            void* grad, hipStream_t stream);
hipError_t madnn_xent_rescale(void* grad, int dt, int64_t numel, const float* g, hipStream_t stream);
hipError_t madnn_xent_fwd(const void* logits, int dt, const int64_t* targets, int64_t n_loss_rows, int64_t seq,
                          int64_t ld, int V, int ignore_index, float* loss, float* lse, hipStream_t stream);
hipError_t madnn_xent_bwd(const void* logits, int dt, const int64_t* targets, const float* lse, int64_t n_loss_rows,
                          int64_t seq, int64_t ld, int V, int ignore_index, int64_t n_rows_all, const float* gscale,
                          void* grad, hipStream_t stream);

// ---- pool.hip ----
int madnn_maxpool_set_k3s2(int on);
int madnn_maxpool_supported(int64_t numel, int C, int k);
hipError_t madnn_maxpool_fwd(const void* x, void* y, void* arg, int N, int H, int W, int C, int Ho, int Wo, int k,
                             int s, int p, int xdt, hipStream_t stream);
hipError_t madnn_maxpool_bwd(const void* dy, const void* arg, void* dx, int N, int H, int W, int C, int Ho, int Wo,
                             int k, int s, int p, int xdt, hipStream_t stream);
int madnn_pool_bn_tune(int key, int value);
int madnn_pool_bn_supported(int64_t numel, int C);
// maxpool_k3s2(relu(y * scale + shift)) (bf16 NHWC): output + 1-byte argmax per element; yarg (optional,
// null = off): the raw input at each argmax, laid out as the output
hipError_t madnn_pool_bn_fwd(const void* x, const float* scale, const float* shift, void* y, void* arg, void* yarg,
                             int N, int H, int W, int C, int Ho, int Wo, int p, hipStream_t stream);
// partial rows the fused backward's reduction writes
int madnn_pool_bn_bwd_rows(int64_t pixels, int C);
// dy (and the BN weight/bias grads) from the pool output gradient dp: reduction, finalize, apply.
// workspace: madnn_pool_bn_bwd_rows * 2 * C floats; coef: 3 * C floats.
hipError_t madnn_pool_bn_bwd(const void* dp, const void* arg, const void* y, const float* w, const float* mean,
                             const float* invstd, const float* scale, const float* shift, void* dy, float* dw,
                             float* db, float* coef, float* workspace, int N, int H, int W, int C, int Ho, int Wo,
                             int p, hipStream_t stream);
// partial rows the pooled-domain reduction writes (pooled = N * Hp * Wp pooled pixels)
int madnn_pool_bn_bwd_pooled_rows(int64_t pooled, int C);
// bn's weight/bias grads and backward coefficients (coef = ca, cb, cc: 3 * C floats) from the pool output
// gradient dp and yarg, both [pooled][C] bf16: reduction + finalize.  pixels = N * H * W of bn's input.
// workspace: madnn_pool_bn_bwd_pooled_rows * 2 * C floats.
hipError_t madnn_pool_bn_bwd_pooled(const void* dp, const void* yarg, const float* w, const float* mean,
                                    const float* invstd, const float* scale, const float* shift, float* dw, float* db,
                                    float* coef, float* workspace, int64_t pooled, int64_t pixels, int C,
                                    hipStream_t stream);

// ---- attn.hip ----
int madnn_attn_supported(int D);
int madnn_attn_tune(int key, int value);
hipError_t madnn_attn_fwd(const MadnnAttnArgs* a, int D, int causal, hipStream_t st);
// rows of MadnnAttnArgs::cpart: one per (batch, 128-row sequence block)
int64_t madnn_attn_colsum_rows(int B, int S);
hipError_t madnn_attn_colsum_finalize(const float* cpart, int64_t R, int64_t C, void* out, int out_bf16,
                                      hipStream_t st);
// threshold = floor((1 - p) * 256 + 0.5): 1..256 for a usable p, 0 when p quantises to keep-nothing,
// -1 for p outside [0, 1)
int madnn_attn_dropout_threshold(double p);
hipError_t madnn_attn_dropout_mask(uint8_t* out, int B, int H, int S, uint32_t threshold, uint64_t seed,
                                   uint64_t offset, hipStream_t st);
hipError_t madnn_attn_bwd(const MadnnAttnArgs* a, int D, int causal, hipStream_t st);
// MadnnAttnArgs::seg of a batch of packed rows: ids int32 [B, S] (a document = a maximal run of equal
// consecutive ids), bounds int32 [B, 2, S] = (first token of the token's document, one past its last).
// One launch, one workgroup per row, any S.
hipError_t madnn_attn_segment_bounds(const int32_t* ids, int32_t* bounds, int B, int S, hipStream_t st);

// ---- conv.hip ----
// key 0: forward/dgrad grid target, 1: weight-grad workgroups, 2: XCD remap (0/1), 3: ring main loop (0/1),
// 4: deep forwards / plain data grad on K12P (0/1); returns the old value (value < 0: query only)
int madnn_conv1x1_tune(int key, int value);
int madnn_conv1x1_supported(int64_t cin, int64_t cout);
// partial-statistics rows the forward writes ([rows][2][cout] fp32)
int madnn_conv1x1_stat_rows(int64_t M, int64_t cin, int64_t cout);
// partial rows the BNB data grad writes ([rows][2][cin] fp32)
int madnn_conv1x1_dgrad_rows(int64_t M, int64_t cin, int64_t cout);
hipError_t madnn_conv1x1_fwd(const void* x, const void* w, void* y, float* stats, int64_t M, int64_t cin,
                             int64_t cout, hipStream_t s);
// dx = dY W (+ res: an accumulated gradient of the same layout, added in the epilogue)
// bny/bnsc/bnsh/partial (optional, all or none): dx is d relu(bn(bny)); the epilogue also writes bn's
// backward sums as partial [madnn_conv1x1_dgrad_rows][2][cin] (see BNB)
// resmask (with res): res counts only where its ReLU bit is set
hipError_t madnn_conv1x1_dgrad(const void* dy, const void* w, void* dx, const void* res, int64_t M, int64_t cin,
                               int64_t cout, const void* bny, const float* bnsc, const float* bnsh, float* partial,
                               hipStream_t s, const unsigned char* resmask);
// fp32 floats of workspace madnn_conv1x1_wgrad needs (the per-split partial slabs)
int64_t madnn_conv1x1_wgrad_ws(int64_t M, int64_t cin, int64_t cout);
// dw: [cout][cin] fp32 or (dw_bf16) bf16; ws: madnn_conv1x1_wgrad_ws floats (the per-split partial
// slabs, summed in split order into dw -- one pass that also casts)
hipError_t madnn_conv1x1_wgrad(const void* dy, const void* x, void* dw, int dw_bf16, float* ws, int64_t M, int64_t cin,
                               int64_t cout, hipStream_t s);
// K9F (bn3_conv3_bwd_kernel): the shapes it is built for
int madnn_bn3_conv3_bwd_supported(int64_t c, int64_t c4);
// workgroups = bn2 partial rows ([rows][2][C]) = dW3 slabs ([rows][4C][C] fp32 of workspace)
int madnn_bn3_conv3_bwd_groups(int64_t M);
// K9F launch.  y / coef / w / a: the BatchNorm input, its ca | cb | cc ([3][4C], bn_bwd_finalize_kernel), the
// weight and the convolution input -- bn3's set (y3, W3, a2) or the downsample path's (yd, W_ds, xf).
// y2 / sc2 / sh2 / partial all given: da is d relu(bn2(y2)) and partial gets bn2's backward sums (BNB); all
// null: da is stored plainly.  partial / slabs: madnn_bn3_conv3_bwd_groups rows;
// dw: [4C][C] fp32 or (dw_bf16) bf16, the slabs summed in workgroup order
hipError_t madnn_bn3_conv3_bwd(const void* dout, const void* y, const unsigned char* mask, const float* coef,
                               const void* w, const void* a, const void* y2, const float* sc2, const float* sh2,
                               void* da, float* partial, float* slabs, void* dw, int dw_bf16, int64_t M, int64_t c,
                               int64_t c4, hipStream_t s);

// ---- stem.hip ----
int madnn_stem_supported(int H, int W);
int madnn_stem_stat_rows(int N, int H, int W);
// x [N][H][W][3] bf16, wp packed [64][7][8][4] bf16 -> y [N][Ho][Wo][64]; stats [grid][2][64] or null
hipError_t madnn_stem_fwd(const void* x, const void* wp, void* y, float* stats, int N, int H, int W, hipStream_t s);
// fp32 workspace floats the weight gradient needs (per-workgroup partials)
int64_t madnn_stem_wgrad_ws(int N, int H, int W);
// x [N][H][W][3], dy [N][Ho][Wo][64] bf16 -> dw [64][3][7][7] fp32 (ws: madnn_stem_wgrad_ws floats)
hipError_t madnn_stem_wgrad(const void* x, const void* dy, float* ws, float* dw, int N, int H, int W, hipStream_t s);
// The weight gradient with bn1's backward apply and the 3x3 / stride-2 max-pool's backward formed on chip:
// y [N][Ho][Wo][64] the stem output, dp [N][Hp][Wp][64] the pool's output gradient, arg its argmax bytes
// (pool.hip), scale/shift bn1's forward pair, ca/cb/cc its backward coefficients ([64] fp32 each).
hipError_t madnn_stem_wgrad_bnp(const void* x, const void* y, const void* dp, const void* arg, const float* scale,
                                const float* shift, const float* ca, const float* cb, const float* cc, float* ws,
                                float* dw, int N, int H, int W, int p, hipStream_t s);

// ---- bias.hip ----
int madnn_bias_tune(int gelu, int wg_per_cu);
int madnn_bias_grad_supported(int64_t M, int N);
// partial rows R: ~wg_per_cu workgroups per CU in total, each walking >= 4 row steps
int madnn_bias_grad_rows(int64_t M, int N, int gelu);
int madnn_gelu_tune(int key, int value);
// kind: kGeluTanh (1) or kGeluErf (2)
hipError_t madnn_gelu_fwd(const void* x, void* y, int64_t n, int dt, int kind, hipStream_t stream);
// dy, pre, dp: [M, N] of dtype xdt; partial: [R, N] fp32 with R = madnn_bias_grad_rows(M, N, pre != 0);
// db: [N] of odt; kind: the GELU whose backward runs on pre (kGeluTanh / kGeluErf)
hipError_t madnn_bias_grad(const void* dy, const void* pre, void* dp, int64_t M, int N, int xdt, float* partial,
                           void* db, int odt, int kind, hipStream_t stream);

// ---- gemm.hip ----
// Shapes K12 takes: reduction % 64 == 0, output features % 8 == 0, 16-B aligned rows, and
// 32-bit-safe per-lane DMA offsets.
int madnn_gemm_supported(int64_t I, int64_t J, int64_t K, int64_t lda, int64_t ldb);
// Y[m][n] = X[m][k] W[n][k] (+ bias[n]) (-> gelu) (+ res[m][n]); aux (if given) = pre-activation
hipError_t madnn_linear_fwd(const void* x, const void* w, const void* bias, int bias_f32, const void* res, void* y,
                            void* aux, int act, int64_t M, int64_t N, int64_t K, hipStream_t s);
// dX[m][k] = dY[m][n] W[n][k] (+ res[m][k]; res may alias dX for in-place accumulation)
hipError_t madnn_linear_dgrad(const void* dy, const void* w, const void* res, void* dx, int64_t M, int64_t N,
                              int64_t K, hipStream_t s);
int madnn_wgrad_splits(int64_t M, int64_t N, int64_t K);
// dW[n][k] (+)= sum_m dY[m][n] X[m][k] (bf16 out; with accumulate the existing dW is added).
// ws: splits x N x K fp32 workspace when splits > 1 (madnn_wgrad_splits), else unused.
hipError_t madnn_linear_wgrad(const void* dy, const void* x, void* dw, float* ws, int splits, int accumulate,
                              int64_t M, int64_t N, int64_t K, hipStream_t s);
hipError_t madnn_linear_wgrad4(const void* dy, const void* x, void* dw, float* ws, int splits, int accumulate,
                               int64_t M, int64_t N, int64_t K, hipStream_t s);
hipError_t madnn_linear_wgrad4h(const void* dy, const void* x, void* dw, float* ws, int splits, int accumulate,
                                int64_t M, int64_t N, int64_t K, hipStream_t s);

// ---- gemmp.hip ----
// Shapes K12P takes: output features and tokens multiples of 256 (no edge tiles), reduction a
// multiple of 64, 32-bit-safe per-lane DMA offsets; a bias must fit the LDS bias slot.
int madnn_gemmp_supported(int64_t I, int64_t J, int64_t K, int has_bias);
// Y[m][n] = X[m][k] W[n][k] (+ bias[n]); act 1 / 2 (tanh / erf GELU): aux = that pre-activation,
// Y = gelu(aux)
hipError_t madnn_linear_fwd_p(const void* x, const void* w, const void* bias, int bias_f32, void* y, void* aux,
                              int act, int64_t M, int64_t N, int64_t K, hipStream_t s);
int madnn_conv1x1_fwd_p_rows(int64_t M, int64_t cout);
// The deep 1x1 convolution forward on NHWC rows, Y[m][co] = X[m][ci] W[co][ci] (no bias), with the
// following BatchNorm's partial statistics: stats (or null: the plain kernel) gets
// [madnn_conv1x1_fwd_p_rows][2][cout] fp32, one (sum, sum of squares) row pair per wave and tile
// over the bf16-rounded outputs -- what K9's forward writes per workgroup (conv.hip header)
hipError_t madnn_conv1x1_fwd_p(const void* x, const void* w, void* y, float* stats, int64_t M, int64_t cin,
                               int64_t cout, hipStream_t s);
// dX[m][k] = dY[m][n] W[n][k]; with pre: dX = that * gelu'(pre) (gelu_kind 1 tanh / 2 erf) and the
// fp32 column sums of dX as
// [M / 256 * 4][K] partial rows in colsum (madnn_colsum_finalize turns them into the bias grad)
hipError_t madnn_linear_dgrad_p(const void* dy, const void* w, const void* pre, void* dx, float* colsum, int64_t M,
                                int64_t N, int64_t K, int gelu_kind, hipStream_t s);
hipError_t madnn_colsum_finalize(const float* part, int R, int64_t I, void* out, int out_f32, hipStream_t s);

// ---- conv3.hip ----
int madnn_conv3x3_supported(int H, int W, int Ci, int Co);
int madnn_conv3x3_stat_rows(int64_t M);
// y = conv3x3(x, w) (stride 1, pad 1); x [N, H, W, Ci] NHWC, w [Co, 3, 3, Ci] (channels_last),
// y [N, H, W, Co]; stats (optional): [ceil(M/256)][2][Co] partial sums of y
hipError_t madnn_conv3x3_fwd(const void* x, const void* w, void* y, float* stats, int N, int H, int W, int Ci, int Co,
                             hipStream_t s);
int madnn_conv3x3_s2_supported(int H, int W, int Ci, int Co);
int madnn_conv3x3_s2_stat_rows(int N, int H, int W);
// Stride 2 (pad 1): x [N, H, W, Ci] with H, W even -> y [N, H/2, W/2, Co]; stats as above over the output.
hipError_t madnn_conv3x3_fwd_s2(const void* x, const void* w, void* y, float* stats, int N, int H, int W, int Ci,
                                int Co, hipStream_t s);
// Data grad with the BatchNorm-backward sums in the epilogue (see BNB): x = the output gradient,
// w = the flipped / transposed weight, y = dx; partial [ceil(M/256)][2][Co] = (sum g, sum g*bny)
hipError_t madnn_conv3x3_fwd_bnb(const void* x, const void* w, void* y, float* partial, const void* bny,
                                 const float* bnsc, const float* bnsh, int N, int H, int W, int Ci, int Co,
                                 hipStream_t s);
int64_t madnn_conv3x3_wgrad_ws(int N, int H, int W, int Ci, int Co);
// dw [Co][3][3][Ci] (channels_last weight layout), fp32 (out_bf16 = 0) or bf16; ws: madnn_conv3x3_wgrad_ws floats
hipError_t madnn_conv3x3_wgrad(const void* dy, const void* x, float* ws, void* dw, int out_bf16, int N, int H, int W,
                               int Ci, int Co, hipStream_t s);

// ---- xgmi.hip ----
int madnn_oneshot_max_peers();
int madnn_oneshot_handle_bytes();
// Allocate this rank's staging buffer (2 x cap bytes) and uncached flag array, and return their
// IPC handles (2 x handle_bytes into `handles`).  Returns the context id (> 0) or -hipError.
int madnn_oneshot_create(int64_t cap, int world, int rank, int device, unsigned char* handles);
// Map every peer's buffers: all_handles = world x (2 x handle_bytes), rank-major.
int madnn_oneshot_open(int id, const unsigned char* all_handles);
// out = sum over ranks of in (n elements, dtype 0 fp32 / 1 bf16; in/out may alias).  Every rank
// must call with the same n and dtype, in the same order.  Asynchronous on `stream`; a peer that
// never arrives sets the context's error word (madnn_oneshot_error) instead of hanging the GPU.
int madnn_oneshot_allreduce(int id, const void* in, void* out, int64_t n, int dtype, int spin_limit,
                            hipStream_t stream);
// error word of the context (1 = a wait timed out).  flags bit 0: clear it after reading;
// bit 1: synchronise the device first (otherwise the word reflects the kernels that have
// finished so far -- a plain host read of pinned memory, no stall)
int madnn_oneshot_error(int id, int flags);
int madnn_oneshot_destroy(int id);

// ---- probe.hip ----
hipError_t madnn_hwq_wait(const int* flag, int expect, int64_t timeout_us, int* out, hipStream_t s);
hipError_t madnn_hwq_set(int* flag, int val, hipStream_t s);
hipError_t madnn_hwq_batch(const int* kinds, const int* msgs, int nops, int* a, int* b, int epoch, int64_t timeout_us,
                           int* ok, const int* ok_index, hipStream_t s);
hipError_t madnn_hwq_spin(int64_t spin_us, hipStream_t s);
hipError_t madnn_dq_atomic_floor(float* dq, int BH, int S, int D, int kblock, int causal, hipStream_t s);

// ---- glue.hip ----
// src / dst: bf16 [rows = B*S][NH][D] contiguous (dst == src: in place, the NR rotated heads only);
// heads 0..NR-1 rotated (q then k), the rest copied; cos / sin: fp32 [>= S][D]
hipError_t madnn_rope_qkv(const void* src, void* dst, const float* cos_t, const float* sin_t, int64_t rows, int S,
                          int NH, int NR, int D, int inverse, hipStream_t st);
// gu: bf16 [M][2I], h: bf16 [M][I]; I % 8 == 0
hipError_t madnn_swiglu_fwd(const void* gu, void* h, int64_t M, int I, hipStream_t st);
hipError_t madnn_swiglu_bwd(const void* dh, const void* gu, void* dgu, int64_t M, int I, hipStream_t st);
// out = res + rp * m * x (res == nullptr: rp * m * x) on [rows][H] contiguous, dt = kF32 / kBF16, H % 8 == 0
hipError_t madnn_dropout_add(const void* x, const void* res, void* out, int64_t rows, int H, int dt,
                             uint32_t threshold, uint64_t seed, uint64_t offset, hipStream_t st);
hipError_t madnn_hidden_dropout_mask(uint8_t* out, int64_t rows, int H, int64_t row0, uint32_t threshold,
                                     uint64_t seed, uint64_t offset, hipStream_t st);

// ---- fp8.hip ----
// fmt everywhere: 0 = e4m3fn, 1 = e5m2 (OCP; torch.float8_e4m3fn / float8_e5m2)
// partial amax rows (floats of workspace) madnn_fp8_quant needs
int madnn_fp8_quant_rows(int64_t R, int64_t C);
// x: bf16 [R][C] with row stride ldx (elements) -> q: fp8 [R][C], qt (optional): fp8 [C][R];
// scales: [2] fp32 = (scale, 1 / scale), the power of two formed on the device from x's amax.
// C % 16 == 0, ldx % 8 == 0, 16-B aligned x; with qt also R % 16 == 0.
hipError_t madnn_fp8_quant(const void* x, int64_t ldx, int64_t R, int64_t C, int fmt, void* q, void* qt,
                           float* partial, float* scales, hipStream_t stream);
// K17: out[M][N] (bf16) = (a[M][K] . b[N][K]^T) * inv_a[0] * inv_b[0] (+ bias[N]) (+ res[M][N]), a / b fp8 with
// row strides lda / ldb; K % 16 == 0, N % 8 == 0, lda % 16 == 0, ldb % 16 == 0; out / res contiguous
hipError_t madnn_fp8_gemm(const void* a, int fmt_a, const void* b, int fmt_b, const float* inv_a,
                          const float* inv_b, const void* bias, int bias_f32, const void* res, void* out,
                          int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, hipStream_t stream);
// workgroups per output tile K17W would choose (its fp32 workspace is splits x N x K floats when splits > 1)
int madnn_fp8_wgrad_splits(int64_t M, int64_t N, int64_t K);
// K17W: dw[N][K] (bf16, contiguous) = (sum_m dy8[m][n] x8[m][k]) * inv_g[0] * inv_x[0], dy8 [M][N] / x8 [M][K] fp8
// with row strides ldg / ldx; any M > 0, N % 16 == 0, K % 16 == 0, ldg % 16 == 0, ldx % 16 == 0, 16-B aligned
// pointers; splits >= 1 workgroups per tile, ws: splits x N x K fp32 when splits > 1, else unused
hipError_t madnn_fp8_wgrad(const void* dy8, int fmt_g, const void* x8, int fmt_x, const float* inv_g,
                           const float* inv_x, void* dw, float* ws, int splits, int64_t M, int64_t N, int64_t K,
                           int64_t ldg, int64_t ldx, hipStream_t stream);
// MX quantiser (one launch): x bf16 [R][C] with row stride ldx -> q: fp8 [R][C] quantised in blocks of 32 along C,
// e: E8M0 scale bytes [R][lde] (byte j of a row: block j; lde % 4 == 0, lde >= 4 ceil(C / 128), 4-B aligned; pad
// bytes are unspecified).  qt (optional, with et / ldet likewise over R): fp8 [C][R] quantised along R.
// C % 32 == 0, ldx % 8 == 0, 16-B aligned x / q / qt; with qt also R % 32 == 0.
hipError_t madnn_mx_quant(const void* x, int64_t ldx, int64_t R, int64_t C, int fmt, void* q, void* e, int64_t lde,
                          void* qt, void* et, int64_t ldet, hipStream_t stream);
// K17X: out[M][N] (bf16) = sum_k a[m][k] 2^(ea[m][k / 32] - 127) b[n][k] 2^(eb[n][k / 32] - 127) (+ bias[N])
// (+ res[M][N]); a / b fp8 as in madnn_fp8_gemm, ea / eb scale bytes in the layout madnn_mx_quant writes (row
// strides ldea / ldeb >= 4 ceil(K / 128), multiples of 4, 4-B aligned; bytes of a row past K / 32 are never used).
// K % 32 == 0, N % 8 == 0.
hipError_t madnn_mx_gemm(const void* a, int fmt_a, const void* ea, int64_t ldea, const void* b, int fmt_b,
                         const void* eb, int64_t ldeb, const void* bias, int bias_f32, const void* res, void* out,
                         int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, hipStream_t stream);
// MX quantiser with the column-blocked image (one launch): q / e as madnn_mx_quant, and qc: fp8 [R][C] quantised in
// blocks of 32 ROWS per column with ec: E8M0 bytes [ceil(R / 32)][ldec] (byte c of row B: rows 32 B .. + 31 of
// column c; ldec % 4 == 0, ldec >= C, 4-B aligned).  Any R > 0 (rows past R count as zeros), C % 32 == 0.
hipError_t madnn_mx_quant_cols(const void* x, int64_t ldx, int64_t R, int64_t C, int fmt, void* q, void* e,
                               int64_t lde, void* qc, void* ec, int64_t ldec, hipStream_t stream);
// K17XW: dw[N][K] (bf16, contiguous) = sum_m dy8[m][n] 2^(eg[m / 32][n] - 127) x8[m][k] 2^(ex[m / 32][k] - 127);
// dy8 / x8 / ws / splits as madnn_fp8_wgrad (madnn_fp8_wgrad_splits gives the split count), eg / ex the
// column-blocked scale bytes madnn_mx_quant_cols writes (row strides ldeg >= N / ldex >= K, multiples of 4, 4-B
// aligned).  Any M > 0, N % 16 == 0, K % 16 == 0.
hipError_t madnn_mx_wgrad(const void* dy8, int fmt_g, const void* eg, int64_t ldeg, const void* x8, int fmt_x,
                          const void* ex, int64_t ldex, void* dw, float* ws, int splits, int64_t M, int64_t N,
                          int64_t K, int64_t ldg, int64_t ldx, hipStream_t stream);

}  // extern "C"
