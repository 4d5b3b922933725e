/*
 * mmeeg_hip.h — C ABI of libmmeeg_hip.so, the MI355X (gfx950) kernel library
 * behind multimodal_eeg_fmri_amd.
 *
 * The reference (bacon205/Multimodal_eeg_fmri) has no FFI / operator plug-in
 * interface: its only boundary is the Python nn.Module surface, whose leaf
 * arithmetic is torch.nn (ATen).  Each entry point below therefore cites the
 * reference call site(s) whose arithmetic it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.
 *
 * Contract (all entry points)
 *   - plain pointers and sizes only; device pointers are BORROWED (no
 *     allocation, free or host sync inside the library; workspaces come in);
 *   - asynchronous on `stream`; safe to capture in a hipGraph;
 *   - return 0 on success, <0 on error (-1 bad argument, -2 launch failure,
 *     -3 unsupported shape); mm_last_error() gives the thread-local message;
 *   - `void*` tensors are bf16, `float*` fp32; channels-last layouts:
 *     1-D activations [B][T][C], tokens [M][D], volumes [B][D][H][W][C];
 *   - results are BIT-REPRODUCIBLE: no floating-point atomics anywhere.  Per-channel accumulators
 *     written by many workgroups (`stats`, `sums_out`, `dbias`, dgamma/dbeta scratch, ...) are
 *     ACCUMULATOR WORKSPACES: the caller allocates and ZEROES 32 x n fp32-sized elements (written
 *     "[32][...]" below) and hands them to the consumer untouched; their content is opaque - 16 replicas
 *     of n 64-bit fixed-point sums (integer atomics are order-free; a workgroup adds rint(v * 2^k) into
 *     replica blockIdx % 16; k = 28 for activation statistics, 40 for gradient sums: csrc/common.h).
 *     mm_bn_finalize, the *_bwd_apply passes and mm_conv3d_l1_bwd read them directly;
 *     everything else goes through mm_acc_reduce / mm_reduce_many (-> fp32).  Weight gradients use
 *     per-workgroup SLOTS (one writer per element) summed in slot order by mm_wgrad_scatter;
 *   - activation codes: 0 none, 1 GELU(erf), 2 ReLU, 3 tanh, 4 sigmoid;
 *   - dropout: keep iff hash(seed, element index) >= p * 2^32, scaled 1/(1-p);
 *     the backward entry points recompute the same mask from (p, seed).
 *     `seed_epoch` (nullable device word) is mixed into the seed on the device, so
 *     a launch recorded in a hipGraph draws a new mask on every replay.
 */
#ifndef MMEEG_HIP_H
#define MMEEG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

/* what mm_abi_version() returns: bumped whenever the argument list of an entry point that remains changes
 * (removing an entry point leaves it as it is) */
#define MM_ABI_VERSION 5

const char* mm_last_error(void);
int mm_abi_version(void);

/* ---- layout packers --------------------------------------------------------
 * (B,C,T) fp32 -> (B,T,Cp) bf16, zero-padded channels.  Replaces the implicit
 * NCT layout of every nn.Conv1d input (enhanced_models_v4.py:129, 211-223). */
int mm_pack_nct_bf16(const float* x, void* y, int B, int C, int T, int Cp, hipStream_t stream);
/* inverse for the input gradient: (B,T,Cp) bf16 -> (B,C,T) fp32 */
int mm_unpack_ntc_f32(const void* g, float* dx, int B, int C, int T, int Cp, hipStream_t stream);
/* weight (Cout,Cin,k) fp32 -> forward image [Cout][k][Cinp] bf16 and (optional)
 * data-gradient image [Cinp][k flipped][Coutp] bf16 */
int mm_prep_conv_weight(const float* w, void* w_fwd, void* w_dgrad, int Cout, int Cin, int k,
                        int Cinp, int Coutp, hipStream_t stream);

/* ---- 1-D implicit GEMM (bf16 MFMA, fp32 accumulate) -----------------------
 * Y[b,t,n] = epilogue( sum_{tap,c} X[b,t+tap-pad,c] * W[n,tap,c] )
 * epilogue: v = acc*scale[n] + shift[n]; stats[0][n]+=v, stats[1][n]+=v*v;
 *           out_pre = v; v = act(v); v *= dropout; v += residual; v += pe[t][n];
 *           max over t pairs if pool == 2; store fp32 and/or bf16.
 * backward fusion: with gradz != NULL, v *= act'(gradz[idx]) before the dropout mask, so
 * the data-gradient GEMM of a Linear directly yields d(pre-activation) of the layer below.
 * Replaces nn.Conv1d (+ folded eval BatchNorm1d + GELU + MaxPool1d)
 * (enhanced_models_v4.py:128-144, 210-234; crossmodal_v4_enhancements.py:822-877)
 * and, with taps == 1, every nn.Linear / MHA projection on the path
 * (enhanced_models_v4.py:71-81, 164; bridge_utils.py:34-66). */
int mm_conv1d_fwd(const void* x, const void* w, int B, int T, int Cin, int Cout, int taps, int pad,
                  const float* scale, const float* shift, int act, const float* residual,
                  const float* pe, int pool, float* stats, float* out_f32, void* out_bf16,
                  void* out_pre, float drop_p, uint32_t drop_seed, const uint32_t* seed_epoch,
                  const void* gradz, int gradz_act, hipStream_t stream);
/* mm_conv1d_fwd with the reduction split over input-channel slices (few output tiles, long reduction: the merged
 * 192-channel k = 7 convolution of EnhancedPowerEncoder over the ~6 000 STFT channels of config #5 is 96 tiles of 98
 * chunks on 256 CUs): nsplit x the workgroups, each slice's raw fp32 tile to ws, a second launch adds the slices in order
 * (same bits every run) and runs the epilogue.  mm_conv1d_fwd_splitk_plan says when it pays (nsplit_host = 1: call
 * mm_conv1d_fwd) and how many floats ws needs; k > 1 convolutions with Cin % 64 == 0 only. */
int mm_conv1d_fwd_splitk_plan(int B, int T, int Cin, int Cout, int taps, int* nsplit_host, int64_t* ws_floats_host,
                              hipStream_t stream);
int mm_conv1d_fwd_splitk(const void* x, const void* w, int B, int T, int Cin, int Cout, int taps, int pad,
                  const float* scale, const float* shift, int act, const float* residual,
                  const float* pe, int pool, float* stats, float* out_f32, void* out_bf16,
                  void* out_pre, float drop_p, uint32_t drop_seed, const uint32_t* seed_epoch,
                  const void* gradz, int gradz_act, float* ws, int nsplit, hipStream_t stream);
/* dW[n][c][tap] (fp32, strides sn/sc/stap in elements) += sum_{b,t} dY[b,t,n]*X[b,t+tap-pad,c];
 * optional dbias[n] += sum dY.  Replaces the weight/bias gradients autograd
 * derives for the layers above (loss.backward(), run_training_lite.py:486).
 * slot_mode must be 1 (0, fp32 atomics into replicas, is gone: -1): dw is a workspace of nrep >= mm_conv1d_wgrad_slots(...) slots of rep_stride floats;
 * workgroup row-chunk x stores (no atomics, no zeroing needed) its partial dW into slot x; the caller
 * sums the slots (mm_wgrad_scatter / mm_scatter_many with nrep = slots).  dbias (nullable) is an accumulator
 * workspace [32][Cout]. */
int mm_conv1d_wgrad(const void* dy, const void* x, float* dw, float* dbias, int B, int T, int Cin,
                    int Cout, int taps, int pad, int Cin_real, int64_t sn, int64_t sc, int64_t stap,
                    int nrep, int64_t rep_stride, int slot_mode, hipStream_t stream);
/* *slots_host (HOST int) = number of slots a slot-mode launch with these dimensions writes */
int mm_conv1d_wgrad_slots(int B, int T, int Cin, int Cout, int taps, int* slots_host, hipStream_t stream);
/* several Linear weight gradients (taps 1, slot mode) in one launch: desc_host = n x 64 bytes
 * {dy, x, workspace [nslots][Cout][Cin], dbias replicas (nullable)} pointers + int B, T, Cin, Cout, Cin_real,
 * nslots (= mm_conv1d_wgrad_many_slots), 0, 0.  Same arithmetic as n mm_conv1d_wgrad(..., slot_mode = 1) calls. */
int mm_conv1d_wgrad_many(const void* desc_host, int n, hipStream_t stream);
/* slot count of one problem of such a grouped launch (fewer, longer workgroups per problem than a stand-alone
 * mm_conv1d_wgrad: the group supplies the parallelism) */
int mm_conv1d_wgrad_many_slots(int B, int T, int Cin, int Cout, int* slots_host, hipStream_t stream);
/* dw[n][c][tap] += sum_slot ws[slot][n][tap][c] (nrep = slots, summed in slot order): the wgrad kernels write
 * channel-contiguous slots; this moves the sum to the parameter layout once. */
int mm_wgrad_scatter(const float* ws, float* dw, int Cout, int Cin, int taps, int Cinp, int nrep,
                     hipStream_t stream);
/* PositionalEncoding.forward as a stand-alone op (enhanced_models_v4.py:44-55 =
 * crossmodal_v4_enhancements.py:40-50): out[b][l][d] = dropout(x[b][l][d] + pe[l][d]) on the fp32
 * stream, x (B,L,D), pe (L,D) = rows of the sinusoid buffer; fp32 and/or bf16 output.  pe == NULL is
 * the op's backward: dx = dout * the same dropout mask (same p, seed).  D % 4 == 0.
 * (Inside the encoders the add rides in the conv-3 / fusion-conv epilogue: mm_bn_act_fwd `pe`.) */
int mm_add_pe(const float* x, const float* pe, float* out_f32, void* out_bf16, int B, int L, int D,
              float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);

/* debugging: buf[idx] = 100 MHz wall clock, written in stream order (tools/ and bench --stamps) */
int mm_debug_stamp(void* buf, int idx, hipStream_t stream);
/* mm_prep_conv_weight for ndesc tensors in one launch per 64 descriptors; desc_host = HOST array
 * of {const float* w; void* w_fwd; void* w_dgrad (nullable); int32 Cout, Cin, k, Cinp, Coutp, 0}
 * (48 bytes each), copied into the kernel arguments (capturable in a hipGraph) */
int mm_prep_many(const void* desc_host, int ndesc, hipStream_t stream);
/* the same, and the launch also zeroes `nzero` floats at `zero` (16-byte aligned, nzero % 4 == 0): a training step's
 * accumulator workspaces, which would otherwise be one more fill node in front of the first kernel */
int mm_prep_many_zero(const void* desc_host, int ndesc, float* zero, int64_t nzero, hipStream_t stream);
/* mm_wgrad_scatter for ndesc workspaces in one launch per 64 descriptors; desc_host = HOST array of
 * {const float* ws; float* dw; int32 Cout, Cin, taps, Cinp, nrep, cout_all} (40 bytes each).  A descriptor may take a BLOCK
 * of a wider workspace (the three branches of EnhancedPowerEncoder's merged convolution, mm_power_merge): taps = the
 * gradient tensor's taps | first workspace tap << 8 | workspace taps << 16 (upper bits 0 = the whole kernel), ws already
 * advanced to the block's first output channel, cout_all = the workspace's output channels (0 = Cout). */
int mm_scatter_many(const void* desc_host, int ndesc, hipStream_t stream);
/* ndesc independent reductions into parameter gradients in one launch per 64 descriptors; desc_host =
 * HOST array of {const void* src; float* dst; int64 K, nrep, rep_stride} (40 bytes each), copied into the
 * kernel arguments (capturable in a hipGraph).  nrep = 16: src = a gradient accumulator workspace (8-byte
 * aligned; element e of it is at byte offset 8 e; rep_stride in 64-bit elements), dst[k] += its sum in fp32;
 * nrep = 1: src = compact fp32 vector, dst[k] += src[k];
 * nrep = -R: src = R fp32 rows rep_stride floats apart (per-sample partial rows, each written by one workgroup),
 * dst[k] += ((src[k] + src[rep_stride + k]) + ...) in ascending row order. */
int mm_reduce_many(const void* desc_host, int ndesc, hipStream_t stream);
/* mm_scatter_many(scatter_desc_host, nscatter) and mm_reduce_many(reduce_desc_host, nreduce) in ONE launch (per 48
 * descriptors of each kind): the two are independent, and a graph node costs ~5 us on the stream that flushes */
int mm_flush_many(const void* scatter_desc_host, int nscatter, const void* reduce_desc_host, int nreduce,
                  hipStream_t stream);
/* dst[k] += fp32(sum over the 16 replicas of acc[rep * rep_stride + k]),  k < K: gradient accumulator workspace
 * (64-bit elements: offset e is byte offset 8 e) -> fp32 */
int mm_acc_reduce(const float* acc, float* dst, int K, int64_t rep_stride, hipStream_t stream);
/* fp32: dst[k] += sum_rep src[rep * rep_stride + k],  k < K  (replicas summed in order) */
int mm_reduce_replicas(const float* src, float* dst, int K, int nrep, int64_t rep_stride, hipStream_t stream);

/* ---- BatchNorm / activation / pool ----------------------------------------
 * mode 0 (train): stats{sum,sumsq}/count -> out4 = {scale, shift, mean, rstd},
 * running stats updated (momentum, unbiased var);  mode 1 (eval): fold running
 * stats (+conv bias).  nn.BatchNorm1d/3d (enhanced_models_v4.py:130,135,141).
 * batches_tracked (int64 device scalar, nullable) is incremented in train mode, as
 * nn.BatchNorm's num_batches_tracked buffer is. */
int mm_bn_finalize(const float* stats, const float* gamma, const float* beta, float* run_mean,
                   float* run_var, const float* conv_bias, float* out4, int N, float count,
                   float momentum, float eps, int mode, void* batches_tracked, hipStream_t stream);
/* The train-mode finalize as the PROLOGUE of its consumer (one launch and one graph node less per BatchNorm layer): the
 * `*_fin` forms of the apply passes take, instead of scale / shift (or out4), a HOST pointer to this descriptor (read at
 * call time, like the tables of mm_prep_many); every workgroup forms scale / shift of the N <= 256 channels from the
 * statistics workspace with mm_bn_finalize's arithmetic (the same device function: same bits), workgroup 0 also writes
 * out4 [4][N] = {scale, shift, mean, rstd} (the backward reads it) and updates the running statistics / batches_tracked.
 * GELU only (the encoders' BatchNorm layers). */
typedef struct {
    const float* stats;      /* accumulator workspace [32][2][N] {sum, sumsq} */
    const float* gamma; const float* beta;
    float* run_mean; float* run_var;
    float* out4;             /* [4][N], written */
    void* batches_tracked;   /* int64 device scalar, nullable */
    float count, momentum, eps;
    int reserved;
} mm_bn_fin_t;
int mm_bn_act_fwd_fin(const float* y, const void* bn_fin_host, const float* pe, void* out_bf16, float* out_f32,
                      int R, int S, int N, int act, int pool, int drop_first, float drop_p, uint32_t seed,
                      float drop2_p, uint32_t seed2, const uint32_t* seed_epoch, hipStream_t stream);
int mm_bn_act_fwd_ln_fin(const float* y, const void* bn_fin_host, const float* pe, float* out_f32, int R, int S,
                         int act, float drop_p, uint32_t seed, float drop2_p, uint32_t seed2,
                         const uint32_t* seed_epoch, const float* ln_gamma, const float* ln_beta, float ln_eps,
                         void* ln_out_bf16, float* ln_stat, hipStream_t stream);
int mm_pool3d_bn_act_fwd_fin(const void* y, const void* bn_fin_host, void* out_bf16, void* ysel, void* arg, int B,
                             int D, int H, int W, int N, int act, float drop_p, uint32_t seed,
                             const uint32_t* seed_epoch, hipStream_t stream);
int mm_conv3d_l1_fwd_fin(const float* x, const void* wimg, const float* bias, const void* bn_fin_host, void* out,
                         int B, int D, int H, int W, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                         hipStream_t stream);
/* y fp32 [R][S][N] -> act(y*scale+shift) [-> maxpool2 over S] [-> dropout] [+pe[s][n]]
 * (BN -> GELU -> MaxPool1d -> Dropout -> PositionalEncoding add,
 *  enhanced_models_v4.py:130-143, 49-54) */
int mm_bn_act_fwd(const float* y, const float* scale, const float* shift, const float* pe,
                  void* out_bf16, float* out_f32, int R, int S, int N, int act, int pool,
                  int drop_first, float drop_p, uint32_t seed, float drop2_p, uint32_t seed2,
                  const uint32_t* seed_epoch, hipStream_t stream);
/* the same pass for the last conv block of EnhancedERPEncoder (N = 128, no pooling) with the first
 * TemporalTransformerBlock's norm1 (enhanced_models_v4.py:97-99, LayerNorm(128)) of every finished row fused in:
 * out_f32 = the transformer input, ln_out_bf16 = norm1(out) (the QKV projection's operand), ln_stat [R*S][2] =
 * mean, rstd (nullable; the backward's).  Replaces mm_bn_act_fwd + mm_layernorm_fwd. */
int mm_bn_act_fwd_ln(const float* y, const float* scale, const float* shift, const float* pe, float* out_f32,
                     int R, int S, int act, float drop_p, uint32_t seed, float drop2_p, uint32_t seed2,
                     const uint32_t* seed_epoch, const float* ln_gamma, const float* ln_beta, float ln_eps,
                     void* ln_out_bf16, float* ln_stat, hipStream_t stream);
/* drop2 = the PositionalEncoding dropout applied AFTER the table add (:55)  * mm_bn_act_bwd_apply: sums = the accumulator workspace [32][2][N] as written by mm_bn_act_bwd_reduce
 * (sums_nrep = 32: the kernel adds the replicas up itself) or a compact fp32 [2][N] (sums_nrep = 1). */
int mm_bn_act_bwd_reduce(const float* y, const float* out4, const void* dout_bf16,
                         const float* dout_f32, float* sums_out, int R, int S, int N, int act,
                         int pool, int drop_first, float drop_p, uint32_t seed, float drop2_p,
                         uint32_t seed2, const uint32_t* seed_epoch, hipStream_t stream);
int mm_bn_act_bwd_apply(const float* y, const float* out4, const void* dout_bf16,
                        const float* dout_f32, const float* sums, void* dy, float* dy_f32, int R,
                        int S, int N, int act, int pool, int drop_first, float drop_p, uint32_t seed,
                        float drop2_p, uint32_t seed2, const uint32_t* seed_epoch, int train, int sums_nrep, hipStream_t stream);

/* ---- LayerNorm (nn.LayerNorm, enhanced_models_v4.py:80-81; bridge_utils.py:36,42,62); D = a multiple of 32 up to 512, or 1024 */
int mm_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* out_bf16,
                     float* out_f32, float* stat, int M, int D, float eps, hipStream_t stream);
/* dgb_repl = zeroed accumulator workspace [32][2][D]: {dgamma, dbeta} partial sums;
 * dx_bf16 (optional) = bf16(dx * dropout_mask(drop_p, seed)): the masked GEMM operand of the
 * residual branch feeding this LayerNorm's input */
int mm_layernorm_bwd(const void* dy_bf16, const float* dy_f32, const float* x, const float* stat,
                     const float* gamma, const float* dres, float* dx, void* dx_bf16, float* dgb_repl,
                     int M, int D, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                     hipStream_t stream);
/* TemporalTransformerBlock backward (enhanced_models_v4.py:86-105, autograd of norm1/norm2 feeding
 * self_attn.in_proj / linear1): data gradient of that Linear and the LayerNorm-128 backward in one launch.
 * dy (M, K) bf16; w = the Linear's data-gradient weight image (mm_prep_conv_weight's w_dgrad: 128 x K);
 * x / stat / gamma / dres / dx / dx_bf16 / dgb_repl / dropout arguments exactly as mm_layernorm_bwd. */
int mm_linear_dgrad_ln_bwd(const void* dy, const void* w, int M, int K, const float* x, const float* stat,
                           const float* gamma, const float* dres, float* dx, void* dx_bf16, float* dgb_repl,
                           float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);

/* EnhancedERPEncoder.conv_layers backward (enhanced_models_v4.py:99-105, autograd of Conv1d -> BatchNorm1d -> GELU
 * [-> MaxPool1d(2)] -> Dropout stacked twice): the data gradient of one conv block (dy (B, T, Cin) bf16, w_dgrad = that
 * block's data-gradient weight image, dx_bf16 (B, T, Cout) bf16 = d(out) of the block BELOW) with the BatchNorm-backward
 * reduce pass of the block below as its epilogue.  y_below (B, T * pool, Cout) fp32, out4_below, sums_below (zeroed
 * [32][2][Cout] workspace) and the activation / pool / dropout arguments are those of
 * mm_bn_act_bwd_reduce(y_below, out4_below, dx_bf16, NULL, sums_below, B, T * pool, Cout, ...), whose launch this replaces
 * (drop2_p = 0).  Needs taps > 1 or Cout <= 64 (the 64 x 64 tile). */
int mm_conv1d_dgrad_bn_reduce(const void* dy, const void* w_dgrad, int B, int T, int Cin, int Cout, int taps, int pad,
                              void* dx_bf16, const float* y_below, const float* out4_below, float* sums_below, int act,
                              int pool, int drop_first, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                              hipStream_t stream);

/* mm_linear_fwd_ln (the last Linear of a TemporalTransformerBlock with the NEXT block's norm1 fused,
 * enhanced_models_v4.py:97-107) followed, inside the launch, by that next block's self_attn in_proj on the LayerNorm rows:
 * out2_bf16 (M, n2) = ln_out_bf16 @ w2^T + bias2, w2 = in_proj's forward weight image (n2 rows of 128, n2 % 128 == 0).
 * Bit-identical to mm_conv1d_fwd(ln_out_bf16, w2, 1, M, 128, n2, 1, 0, NULL, bias2, ..., out_bf16 = out2_bf16). */
int mm_linear_fwd_ln_gemm2(const void* x, const void* w, int M, int K, const float* bias, const float* residual,
                           float* out_f32, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                           const float* ln_gamma, const float* ln_beta, float ln_eps, void* ln_out_bf16, float* ln_stat,
                           const void* w2, const float* bias2, int n2, void* out2_bf16, hipStream_t stream);
/* ... and with an epilogue on the second GEMM: the attention out-projection (+ residual, dropout, norm2 fused) followed by
 * the first FFN Linear on norm2's rows - out2_bf16 (M, n2) = dropout(act2(ln_out @ w2^T + bias2)), pre2_bf16 (nullable) =
 * its bf16 pre-activation (enhanced_models_v4.py:99-105).  Bit-identical to mm_conv1d_fwd(ln_out_bf16, w2, 1, M, 128, n2,
 * 1, 0, NULL, bias2, act2, ..., out_bf16 = out2_bf16, out_pre = pre2_bf16, drop2_p, seed2, seed_epoch, ...). */
int mm_linear_fwd_ln_gemm2_act(const void* x, const void* w, int M, int K, const float* bias, const float* residual,
                               float* out_f32, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                               const float* ln_gamma, const float* ln_beta, float ln_eps, void* ln_out_bf16,
                               float* ln_stat, const void* w2, const float* bias2, int n2, void* out2_bf16,
                               void* pre2_bf16, int act2, float drop2_p, uint32_t seed2, hipStream_t stream);
/* Everything row-wise between two attention kernels of a TemporalTransformerBlock (enhanced_models_v4.py:99-107), one
 * launch: mm_linear_fwd_ln_gemm2_act (out_proj + residual + norm2, then linear1 + act1 + Dropout on norm2's rows: x1_f32,
 * ln_out_bf16, ln_stat, g_bf16, z_bf16 as its out_f32, ln_out_bf16, ln_stat, out2_bf16, pre2_bf16) followed by
 * y_f32 (M, 128) = dropout(g @ w2^T + bias2, drop2_p, seed2) + x1 (w2 = linear2's forward weight image, 128 rows of n1) and
 * ONE consumer of the finished rows y:
 *   nln_out_bf16 != NULL: LayerNorm-128 rows (+ nln_stat, nullable), as mm_linear_fwd_ln; with wq != NULL also
 *                         q_bf16 (M, nq) = nln_out @ wq^T + biasq, as mm_linear_fwd_ln_gemm2 (the next block's in_proj);
 *   pool_out != NULL:     the mean over groups of rows_per_group rows, as mm_linear_fwd_meanpool.
 * The 32 x n1 hidden tile stays in the workgroup: g_bf16 and z_bf16 may both be NULL (no backward pass: the hidden tensor
 * is never written).  K == 128, M % 32 == 0, n1 % 128 == 0, n1 <= 512 (LDS: two workgroups per CU).  Every output is
 * bit-identical to mm_linear_fwd_ln, mm_conv1d_fwd (linear1) and mm_linear_fwd_ln / _ln_gemm2 / _meanpool in a row. */
int mm_ffn_rows_fwd(const void* x, const void* w, int M, int K, const float* bias, const float* residual, float* x1_f32,
                    float drop_p, uint32_t seed, const uint32_t* seed_epoch, const float* ln_gamma, const float* ln_beta,
                    float ln_eps, void* ln_out_bf16, float* ln_stat, const void* w1, const float* bias1, int n1,
                    void* g_bf16, void* z_bf16, int act1, float drop1_p, uint32_t seed1, const void* w2, const float* bias2,
                    float* y_f32, float drop2_p, uint32_t seed2, const float* nln_gamma, const float* nln_beta, float nln_eps,
                    void* nln_out_bf16, float* nln_stat, const void* wq, const float* biasq, int nq, void* q_bf16,
                    float* pool_out, int rows_per_group, hipStream_t stream);
/* mm_linear_dgrad_ln_bwd of norm2 / linear1 with the attention out-projection's data gradient as a second GEMM in the
 * same launch (TemporalTransformerBlock backward, enhanced_models_v4.py:99-103: x1 = x0 + dropout(out_proj(attn)),
 * norm2(x1)): do_bf16 (M, 128) = dx_bf16 @ w2, w2 = out_proj's data-gradient weight image (128 x 128), dx_bf16 = the
 * rows masked with out_proj's dropout (drop_p, seed).  Bit-identical to mm_conv1d_fwd(dx_bf16, w2, 1, M, 128, 128, 1, 0,
 * ..., out_bf16 = do_bf16) after mm_linear_dgrad_ln_bwd.  dres_rows_per_sample > 0: dres holds ONE row per that many
 * consecutive rows (mm_pooled_head_bwd_rows), 0: a row per row. */
int mm_linear_dgrad_ln_bwd_gemm2(const void* dy, const void* w, int M, int K, const float* x, const float* stat,
                                 const float* gamma, const float* dres, float* dx, void* dx_bf16, float* dgb_repl,
                                 float drop_p, uint32_t seed, const uint32_t* seed_epoch, const void* w2, void* do_bf16,
                                 int dres_rows_per_sample, hipStream_t stream);
/* The row-wise backward between a TemporalTransformerBlock's output and its attention backward (enhanced_models_v4.py:99-107),
 * one launch: linear2's data gradient dz_bf16 (M, n1) = (dy2 @ w2d) * act1'(z_bf16) * dropout_mask(drop1_p, seed1) (w2d =
 * linear2's data-gradient weight image, n1 rows of 128; dy2 (M, 128) bf16 carries linear2's own dropout mask), then, on the dz
 * rows while they are still in the workgroup, mm_linear_dgrad_ln_bwd_gemm2: linear1's data gradient (w1d = its data-gradient
 * image, 128 rows of n1), norm2's backward (x1, stat2, gamma2, dres with dres_rows_per_sample -> dx1 fp32, dyo_bf16 masked
 * with (drop_p, seed), dgb_repl accumulated) and the out-projection's data gradient do_bf16 = dyo_bf16 @ wo_d.
 * dz_bf16 is written as well: linear1's weight gradient reads it.  M % 32 == 0, n1 % 128 == 0, n1 <= 512 (LDS: two
 * workgroups per CU), M * n1 < 2^32.  Every output (dz_bf16, dx1, dyo_bf16, the dgb_repl accumulator words, do_bf16) is
 * bit-identical to mm_conv1d_fwd(dy2, w2d, 1, M, 128, n1, 1, 0, ..., out_bf16 = dz_bf16, drop1_p, seed1, seed_epoch,
 * gradz = z_bf16, gradz_act = act1) followed by mm_linear_dgrad_ln_bwd_gemm2(dz_bf16, w1d, M, n1, x1, stat2, gamma2, dres,
 * dx1, dyo_bf16, dgb_repl, drop_p, seed, seed_epoch, wo_d, do_bf16, dres_rows_per_sample). */
int mm_ffn_rows_bwd(const void* dy2, const void* w2d, int M, int n1, const void* z_bf16, int act1, float drop1_p, uint32_t seed1,
                    void* dz_bf16, const void* w1d, const float* x1, const float* stat2, const float* gamma2, const float* dres,
                    int dres_rows_per_sample, float* dx1, void* dyo_bf16, float* dgb_repl, float drop_p, uint32_t seed,
                    const uint32_t* seed_epoch, const void* wo_d, void* do_bf16, hipStream_t stream);
/* mm_linear_dgrad_ln_bwd for the FIRST transformer block of EnhancedERPEncoder, whose LayerNorm input is the last conv
 * block's output (enhanced_models_v4.py:143-147: conv_layers[-1] -> pos_encoder -> transformer_layers[0].norm1): the rows dx
 * (fp32) are that block's d(out), so its BatchNorm-backward reduce pass (mm_bn_act_bwd_reduce(y_below, out4_below, NULL, dx,
 * sums_below, 1, M, 128, act, 1, 1, bn_drop_p, bn_seed, bn_drop2_p, bn_seed2, ...)) rides in the same launch.
 * y_below (M, 128) fp32; sums_below = zeroed [32][2][128] workspace; drop2 = the PositionalEncoding dropout. */
int mm_linear_dgrad_ln_bwd_bn_reduce(const void* dy, const void* w, int M, int K, const float* x, const float* stat,
                                     const float* gamma, const float* dres, float* dx, float* dgb_repl,
                                     const uint32_t* seed_epoch, const float* y_below, const float* out4_below,
                                     float* sums_below, int act, float bn_drop_p, uint32_t bn_seed, float bn_drop2_p,
                                     uint32_t bn_seed2, hipStream_t stream);

/* The two BatchNorm-backward passes for a block whose d(out) is the backward of a mean over its S positions (the voxel
 * encoder's last conv block under AdaptiveAvgPool3d(1) -> Linear): dout_rows (R, N) fp32 = ONE row per sample, every
 * position's d(out) = dout_rows[r] * scale (scale = 1 / S).  Same results as mm_bn_act_bwd_reduce / _apply on the
 * broadcast (R, S, N) tensor, which is never written or read (pool 1, no second dropout). */
int mm_bn_act_bwd_reduce_bcast(const float* y, const float* out4, const float* dout_rows, float scale, float* sums_out,
                               int R, int S, int N, int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                               hipStream_t stream);
int mm_bn_act_bwd_apply_bcast(const float* y, const float* out4, const float* dout_rows, float scale, const float* sums,
                              void* dy, int R, int S, int N, int act, float drop_p, uint32_t seed,
                              const uint32_t* seed_epoch, int train, int sums_nrep, hipStream_t stream);

/* mm_pooled_head_bwd (the backward of x.mean(dim=1) -> output_proj, enhanced_models_v4.py:161-167) without the fp32
 * (B, L, D) token gradients: rows_out (B, D) = the one row every token of a sample receives; dx_bf16 (B, L, D) = that row
 * under the consumer's dropout mask, as mm_pooled_head_bwd writes it. */
int mm_pooled_head_bwd_rows(const float* dout, const void* z_pre_bf16, const float* W, void* dz_bf16, float* rows_out,
                            void* dx_bf16, int B, int L, int D, int N, int act, float drop_p, uint32_t seed,
                            float emit_drop_p, uint32_t emit_seed, const uint32_t* seed_epoch, hipStream_t stream);

/* ---- multi-head self-attention, head_dim 32 (nn.MultiheadAttention,
 * enhanced_models_v4.py:71-73, 99).  qkv [B][L][3E] bf16 -> out [B][L][E] bf16,
 * lse [B][H][L] fp32.  drop_p = attention-probability dropout (train mode).  The
 * head-averaged weights the reference computes and discards (:99) are not produced here: mm_attn_weights /
 * mm_attn_received (below) form them from the qkv and lse a saving forward keeps.
 * attn_mask (nullable): the `mask` of TemporalTransformerBlock.forward(x, mask)
 * (enhanced_models_v4.py:88-98 -> self_attn(..., attn_mask=mask)) as an ADDITIVE fp32 (L, L)
 * matrix shared by every batch element and head (a boolean mask = 0 / -inf), or - attn_mask_per_head != 0 -
 * nn.MultiheadAttention's 3-D form: (B*H, L, L), matrix b*H + h for head h of batch element b.
 * A fully masked row yields NaN, as in PyTorch. */
int mm_attn_fwd(const void* qkv, void* out, float* lse, int B, int L, int H, int head_dim,
                float scale, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                const float* attn_mask, int attn_mask_per_head, hipStream_t stream);
int mm_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                float* delta_ws, int B, int L, int H, int head_dim, float scale, float drop_p,
                uint32_t seed, const uint32_t* seed_epoch, const float* attn_mask, int attn_mask_per_head,
                hipStream_t stream);
/* The same for every head_dim that is a multiple of 8 in [16, 64] (32 included): same arguments, layouts, mask forms
 * and dropout mask as mm_attn_fwd / mm_attn_bwd.  Any other head_dim is refused (MM_ERR_ARG, "head_dim" in
 * mm_last_error()) before anything is launched. */
int mm_attn_fwd_hd(const void* qkv, void* out, float* lse, int B, int L, int H, int head_dim,
                   float scale, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                   const float* attn_mask, int attn_mask_per_head, hipStream_t stream);
int mm_attn_bwd_hd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                   float* delta_ws, int B, int L, int H, int head_dim, float scale, float drop_p,
                   uint32_t seed, const uint32_t* seed_epoch, const float* attn_mask, int attn_mask_per_head,
                   hipStream_t stream);
/* Read-out of the attention probabilities (eval mode: no dropout) from what a forward with lse keeps (csrc/attention_readout.hip).
 * Operands as mm_attn_fwd / mm_attn_fwd_hd: qkv [B][L][3E] bf16, lse [B][H][L] fp32 (natural log), the additive mask in
 * both forms; head_dim a multiple of 8 in [16, 64], anything else is refused (MM_ERR_ARG, the entry's name and
 * "head_dim" in mm_last_error()) before a launch.
 *     P[b][h][i][j] = exp(scale * q_i . k_j + mask[i][j] - lse[b][h][i])
 * mm_attn_weights: per_head == 0: w fp32 (B, L, L) = the mean of P over the heads, summed in the order h = 0 .. H-1
 * (nn.MultiheadAttention(need_weights=True, average_attn_weights=True): the second value of the reference's self.attn
 * call, enhanced_models_v4.py:99); per_head == 1: w (B, H, L, L).  Every element is written once.
 * A fully masked row (lse = -inf) is NaN in that row of w, as in PyTorch. */
int mm_attn_weights(const void* qkv, const float* lse, float* w, int B, int L, int H, int head_dim, float scale,
                    const float* attn_mask, int attn_mask_per_head, int per_head, hipStream_t stream);
/* out[b][j] = self_weight * r[b][j] + (1 - self_weight) * sum_i r[b][i] * (1/H) sum_h P[b][h][i][j], fp32 (B, L), without
 * storing a score matrix.  r = row_w (B, L), or 1 / L everywhere when row_w is NULL.  self_weight = 0, row_w NULL: the
 * attention every time step receives; self_weight = 0.5: one step of attention rollout (Abnar & Zuidema 2020) taken as a
 * row-vector product r <- r (0.5 A + 0.5 I).  self_weight outside [0, 1] is refused.  ws: mm_attn_received_ws_floats(B, L, H)
 * floats of scratch (one slot per batch element, head and key, summed in head order by a second launch), no
 * initialisation.  No floating-point atomics: the same inputs give the same bits.  A fully masked query row is NaN in
 * EVERY column of its batch element (every key sums over that query).  Two launches on `stream`. */
int mm_attn_received(const void* qkv, const float* lse, const float* row_w, float self_weight, float* out, float* ws,
                     int B, int L, int H, int head_dim, float scale, const float* attn_mask, int attn_mask_per_head,
                     hipStream_t stream);
int mm_attn_received_ws_floats(int B, int L, int H, int* floats_host, hipStream_t stream);

/* ---- small reductions / elementwise --------------------------------------- */
int mm_colsum(const void* a_bf16, const float* a_f32, float* out, int M, int N, hipStream_t stream);
/* AdaptiveAvgPool1d(1)+Flatten (enhanced_models_v4.py:162-163) on fp32 tokens */
int mm_meanpool_fwd(const float* x, float* out_f32, void* out_bf16, int B, int L, int D, hipStream_t stream);
int mm_meanpool_bwd(const float* g, float* dx, int B, int L, int D, hipStream_t stream);
/* A training step's inputs into the static buffers a captured step reads, ONE launch: mm_pack_nct_bf16(eeg ->
 * eeg_packed_bf16) [+ an fp32 copy of the EEG batch into eeg_copy, nullable] + an fp32 copy of the fMRI batch
 * (fmri_n floats, a multiple of 4, 16-byte aligned).  The captured step then starts at the first convolution. */
int mm_stage_inputs(const float* eeg, void* eeg_packed_bf16, float* eeg_copy, int B, int C, int T, int Cp,
                    float* fmri_dst, const float* fmri_src, int64_t fmri_n, hipStream_t stream);
/* EEG augmentation in front of a training step (reference: EEGTransforms, EEG_CODE/CrossModal_EEG_scr.ipynb, handed to
 * the training datasets as transform=): per sample, with probability p_noise, Gaussian noise of noise_factor * std_b (the
 * sample's unbiased standard deviation over its C * T values); with probability p_drop, n_drop channels set to 0.  The
 * draws are counter based (csrc/augment.hip defines h(stream, index) and the five stream words the host derives from
 * (seed, step, rank)); nothing is drawn from the dropout stream and no state lives on the device.  Two launches:
 *   mm_eeg_augment_plan  fills `plan` (32-bit words, 8-byte aligned, plan_words of them): per sample S = 4 + ceil(C/32)
 *     words rounded up to even - [0] noise scale fp32 (0 = off), [1] std_b fp32, [2] noise on, [3] drop on, [4..] channel
 *     mask (bit c % 32 of word c / 32) - then, from word B * S, fp64 {sum, sum of squares} per chunk of each sample:
 *     double[B][nchunk][2], nchunk = ceil(C*T / chunk), chunk = 4096 doubled until nchunk <= 64.  So plan_words >=
 *     B * S + 4 * B * nchunk.  Words [0] and [1] are written by mm_stage_inputs_aug, which adds the partials in chunk order.
 *   mm_stage_inputs_aug  = mm_stage_inputs on the augmented batch: eeg_packed_bf16 (B, T, Cp) and / or eeg_out_f32
 *     (B, C, T) (either may be null, not both; not in place), packed == mm_pack_nct_bf16(fp32 output) bit for bit; the fMRI
 *     copy as in mm_stage_inputs, or all three of its arguments null / 0 for the EEG alone.
 * Refused before any launch: C * T < 2, B * C * ceil(T/2) >= 2^32, n_drop outside [1, C], a probability outside [0, 1]. */
int mm_eeg_augment_plan(const float* x, uint32_t* plan, int64_t plan_words, int B, int C, int T, float p_noise, float p_drop,
                        int n_drop, uint32_t s_noise, uint32_t s_drop, uint32_t s_keys, hipStream_t stream);
int mm_stage_inputs_aug(const float* eeg, uint32_t* plan, int64_t plan_words, void* eeg_packed_bf16, float* eeg_out_f32,
                        int B, int C, int T, int Cp, float noise_factor, uint32_t s_gauss_a, uint32_t s_gauss_b,
                        float* fmri_dst, const float* fmri_src, int64_t fmri_n, hipStream_t stream);
/* mm_stage_inputs_aug with the temporal EEG transforms (the reference has none): per sample an integer time
 * shift s_b in [-max_shift, max_shift] (out[t] = x[t - s_b], +0 where there is no source - and no noise there), a gain
 * g_b = (invert ? -1 : 1) * (1 + scale_range * (2u - 1)) and one window of mask_len samples set to +0 on every channel.
 * The seven per-sample draws h(stream_k, b) (decision / amount of the shift, decision / u of the scale, the inversion,
 * decision / start of the mask: purposes 19..25 of csrc/augment.hip's stream) are recomputed by every tile workgroup, so
 * the time transforms need no plan launch:
 *   plan == NULL   time transforms alone, ONE launch (plan_words, noise_factor, s_gauss_* are not read)
 *   plan != NULL   a plan mm_eeg_augment_plan has written for the same batch: its noise (indexed by the OUTPUT position,
 *                  scaled by the original sample's std_b) goes onto the gathered value before the gain, its dropped
 *                  channels are +0.
 * time_plan (nullable): 8 int32 words per sample - [0] flags (bit 0 shift, 1 scale, 2 invert, 3 mask), [1] s_b, [2] g_b
 * (fp32 bits; 1.0f when neither scale nor invert is on), [3] mask start, [4] mask length (0 when off), [5..7] 0.
 * With every time probability 0 the outputs are mm_stage_inputs_aug's (plan) / mm_stage_inputs' (no plan) bit for bit.
 * Refused before any launch: a probability outside [0, 1], max_shift outside [0, T), scale_range outside [0, 1), mask_len
 * outside [1, T], the batch and eeg_out_f32 overlapping (the shift is a gather), and - with a plan - what
 * mm_stage_inputs_aug refuses. */
int mm_stage_inputs_taug(const float* eeg, uint32_t* plan, int64_t plan_words, void* eeg_packed_bf16, float* eeg_out_f32,
                         int B, int C, int T, int Cp, float noise_factor, uint32_t s_gauss_a, uint32_t s_gauss_b,
                         float p_shift, int max_shift, float p_scale, float scale_range, float p_invert, float p_mask,
                         int mask_len, uint32_t s_shift, uint32_t s_shift_amt, uint32_t s_scale, uint32_t s_scale_u,
                         uint32_t s_invert, uint32_t s_mask, uint32_t s_mask_start, int32_t* time_plan, float* fmri_dst,
                         const float* fmri_src, int64_t fmri_n, hipStream_t stream);
/* fMRI volume augmentation in front of a training step (the reference has no volume code: the transform is defined in
 * DESIGN.md 5q and csrc/volume_augment.hip): per sample of a (B, 1, D, H, W) fp32 batch, each with its own probability, a
 * mirror of the W axis, an integer shift (dz, dy, dx) in [-max_shift, max_shift]^3, a scale by 1 + scale_range * (2u - 1),
 * Gaussian noise of noise_factor * std_b (the unbiased standard deviation of the original sample) and one ed x eh x ew
 * cuboid set to `fill`; voxels shifted in from outside are `fill` too.  The draws are h(stream, sample) of csrc/augment.hip
 * on 14 stream words of purposes 5..18 (ops.volume_augment_streams); no state on the device.  Two launches:
 *   mm_volume_augment_plan  fills `plan` (32-bit words, 8-byte aligned): per sample 16 words - [0] flags (bit 0 flip,
 *     1 shift, 2 scale, 3 noise, 4 erase), [1..3] dz, dy, dx (int32), [4] scale factor fp32 (1 when off), [5..7] erase
 *     corner z, y, x, [8..10] erase extents (0 when off), [11] noise scale fp32, [12] std_b fp32, [13..15] 0 - then, from
 *     word 16 * B, fp64 {sum, sum of squares} per chunk of each sample: double[B][nchunk][2], nchunk = ceil(V / chunk),
 *     V = D * H * W, chunk = 4096 doubled until nchunk <= 64.  So plan_words >= 16 * B + 4 * B * nchunk.
 *   mm_volume_augment  reads x and the plan, writes out (B, 1, D, H, W) and the plan's words [11] and [12].
 * Refused before any launch: V < 2, V >= 2^31, B * ceil(V / 2) >= 2^32, max_shift outside [0, min(D, H, W)), a probability
 * outside [0, 1], scale_range outside [0, 1), an extent outside [1, its axis], a noise_factor or fill that is not finite,
 * out overlapping x (the shift is a gather), the plan overlapping either. */
int mm_volume_augment_plan(const float* x, uint32_t* plan, int64_t plan_words, int B, int D, int H, int W, float p_flip,
                           float p_shift, int max_shift, float p_scale, float scale_range, float p_noise, float p_erase,
                           int ed, int eh, int ew, uint32_t s_flip, uint32_t s_shift, uint32_t s_dz, uint32_t s_dy,
                           uint32_t s_dx, uint32_t s_scale, uint32_t s_scale_u, uint32_t s_noise, uint32_t s_erase,
                           uint32_t s_ez, uint32_t s_ey, uint32_t s_ex, hipStream_t stream);
int mm_volume_augment(const float* x, uint32_t* plan, int64_t plan_words, float* out, int B, int D, int H, int W,
                      float noise_factor, float fill, uint32_t s_gauss_a, uint32_t s_gauss_b, hipStream_t stream);
/* out = bf16( g * dropout_mask * act'(z) ) */
int mm_act_bwd(const float* g_f32, const void* g_bf16, const void* z, void* out, int64_t n, int act,
               float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);

/* ---- 3-D voxel convolution, k=3 pad=1 (north-star extension: the reference has
 * no volume code; semantics = torch.nn.Conv3d / BatchNorm3d /
 * MaxPool3d(2)).  Volumes are channels-last [B][D][H][W][C] bf16. */
/* (B,1,D,H,W) fp32 -> [B][D][H][W][Cp] bf16, channel 0 = voxel value, rest 0 */
int mm_pack_volume_bf16(const float* x, void* y, int64_t nvox, int Cp, hipStream_t stream);
/* Y = X (*) W + shift; W image [Cout][27][Cin] (mm_prep_conv_weight with k=27);
 * optional accumulator workspace stats[32][2][Cout] (sum, sumsq of the fp32 results) for training BatchNorm; fp32 and/or
 * bf16 output.  Generic path: LDS-staged (TD+2)x10x10 halo block -> 27 tap-shifted A fragments -> bf16 MFMA.
 * Cin = 32, Cout = 64 with bf16 output only and >= 64 tiles of 4x8x8 voxels (layer 2 of the voxel encoder)
 * runs the weight-resident persistent kernel of csrc/conv3d_wres.hip. */
int mm_conv3d_fwd(const void* x, const void* w, int B, int D, int H, int W, int Cin, int Cout,
                  const float* shift, float* stats, float* out_f32, void* out_bf16, hipStream_t stream);
int mm_conv3d_wgrad(const void* dy, const void* x, float* dw, float* dbias, int B, int D, int H, int W,
                    int Cin, int Cout, int Cin_real, int64_t sn, int64_t sc, int64_t stap, int nrep,
                    int64_t rep_stride, int slot_mode, hipStream_t stream);
/* slot_mode as in mm_conv1d_wgrad; *slots_host (HOST int) = slots a slot-mode launch writes */
int mm_conv3d_wgrad_slots(int B, int D, int H, int W, int Cin, int Cout, int* slots_host, hipStream_t stream);
/* y bf16 [B][D][H][W][N] (the convolution's pre-BatchNorm output) -> act(BN(y)) -> MaxPool3d(2) -> dropout ->
 * bf16 [B][D/2][H/2][W/2][N] (floors, as torch: D, H, W >= 2, odd extents allowed).  N % 8 == 0.  Training also keeps, per pooled element, the winner's pre-BN
 * value (ysel bf16) and its index in the 2x2x2 window (arg, one byte: 4 d + 2 h + w); both null in eval.
 * The reduction of the BatchNorm gradient sums then reads only pooled data (gradients vanish off the
 * winners) and the apply pass (dy bf16, full volume) takes the argmax from `arg`; its `sums` is the reduce pass's
 * accumulator workspace (sums_nrep = 32) or a compact fp32 [2][N] (sums_nrep = 1), as for mm_bn_act_bwd_apply.
 * Tail rule (odd extents): the last plane / row / column that no window covers counts in the BatchNorm statistics
 * (count = B D H W) and gets no gradient through the pool; the apply pass writes every element of dy, the tail's with
 * scale * (0 - c0 - c1 xhat) in train mode and 0 under frozen BatchNorm (train == 0). */
int mm_pool3d_bn_act_fwd(const void* y, const float* out4, void* out_bf16, void* ysel, void* arg, int B, int D,
                         int H, int W, int N, int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                         hipStream_t stream);
int mm_pool3d_bn_act_bwd_reduce(const void* ysel, const float* out4, const void* dout_bf16, float* sums_out,
                                int B, int D, int H, int W, int N, int act, float drop_p, uint32_t seed,
                                const uint32_t* seed_epoch, hipStream_t stream);
int mm_pool3d_bn_act_bwd_apply(const void* y, const void* arg, const float* out4, const void* dout_bf16,
                               const float* sums, void* dy, int B, int D, int H, int W, int N, int act,
                               float drop_p, uint32_t seed, const uint32_t* seed_epoch, int train, int sums_nrep,
                               hipStream_t stream);

/* Fused first voxel layer Conv3d(1->32,k3,p1)+BatchNorm3d+GELU+MaxPool3d(2)[+Dropout]
 * on fp32 [B][D][H][W] volumes; the 32x larger pre-BN tensor is recomputed, never
 * stored.  mode 0: stats[2][32] += {sum, sumsq} of conv+bias; mode 1: forward
 * (out bf16 [B][D/2][H/2][W/2][32]); mode 2: stats += {sum dz, sum dz*xhat};
 * mode 3: dw_tapmajor[27][32] += x^T dy, dbias += sum dy.  wimg = bf16 [32][32]
 * (n, tap) from mm_prep_conv_weight(w as (32,27,1)).  D, H, W >= 2; pooled extents are floors (as torch), and the
 * tail rule of mm_pool3d_bn_act_* holds: statistics (modes 0 and the Gram kernel) and mode 3's dense dy cover all
 * B D H W conv outputs, the pooling windows (modes 1, 2 and the backward) the 2[D/2] x 2[H/2] x 2[W/2] corner. */
int mm_conv3d_l1(int mode, const float* x, const void* wimg, const float* bias, const float* out4,
                 const void* dout, const float* sums, float* stats, void* out, float* dw_tapmajor,
                 float* dbias, int B, int D, int H, int W, int train, float drop_p, uint32_t seed,
                 const uint32_t* seed_epoch, hipStream_t stream);
/* mode 1 (the forward) with one more output: arg u8 [B][D/2][H/2][W/2][32] (floors) = which member of each 2x2x2 pooling
 * window won, j = (dd << 2) | (hh << 1) | ww (the convention of mm_pool3d_bn_act_fwd's `arg`).  The training path
 * recomputes the winners in its backward and never stores them; this entry point lets a caller inspect the routing
 * (the parity tests evaluate the fp32 oracle with the HIP path's routing: an arg-max flip between two near-equal
 * window members is then not counted as a gradient error). */
int mm_conv3d_l1_fwd_winners(const float* x, const void* wimg, const float* bias, const float* out4, void* out,
                             void* arg, int B, int D, int H, int W, int train, float drop_p, uint32_t seed,
                             const uint32_t* seed_epoch, hipStream_t stream);
/* Training forward of the same layer without a statistics pass over the convolution: the Gram matrix of the im2col
 * matrix, G[t][t'] = sum over ALL B D H W output voxels (odd tails included) of xcol[v][t] * xcol[v][t'] for the 27 taps plus a column of ones (bf16-
 * rounded, zero-padded volume - what the convolution sees), holds everything the layer needs from the input:
 *   sum_v y_n = w_n . S + M b_n,  sum_v y_n^2 = w_n^T G w_n + 2 b_n w_n . S + M b_n^2   (S[t] = G[t][27], M = G[27][27])
 * and, in the backward, A3[t][n] = sum_v xcol[v][t] xhat[v][n] = rstd_n ((G w_n)[t] + (b_n - mean_n) S[t]).
 * mm_conv3d_l1_gram: gram = ZEROED accumulator workspace [32][32][32] (activation-statistics scale; G is symmetric and
 * only its upper triangle t <= t' is accumulated; kept for mm_conv3d_l1_bwd), stats = ZEROED accumulator workspace
 * [32][2][32] receiving {sum y, sum y^2} of conv + bias - every workgroup adds the sums of its own voxels (they are
 * linear in G) - i.e. the input of mm_bn_finalize, as after any other convolution.
 * Training backward in ONE recompute pass (replaces modes 2 + 3): BatchNorm's backward is linear in the two sums
 * S1 = sum dz, S2 = sum dz * xhat, so
 *   dW = scale * (A1 - (S1/M) * S - (S2/M) * A3),  A1 = x^T dz, S and A3 from the Gram workspace.
 * Zeroed accumulator workspaces: sums_out [32][2][32] (also the BatchNorm parameter gradients: dbeta = S1,
 * dgamma = S2), a1 [32][27][32].  dw (PyTorch layout [32][1][3][3][3]) and dbias are ADDED to (dbias only when
 * train == 0; it is identically 0 otherwise).  gram may be NULL when train == 0 (frozen BatchNorm: the two correction
 * terms vanish). */
int mm_conv3d_l1_gram(const float* x, const void* wimg, const float* bias, float* gram, float* stats, int B, int D,
                      int H, int W, hipStream_t stream);
int mm_conv3d_l1_bwd(const float* x, const void* wimg, const float* bias, const float* out4, const void* dout,
                     float* sums_out, float* a1, const float* gram, float* dw, float* dbias, int B, int D,
                     int H, int W, int train, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                     hipStream_t stream);

/* ---- small fp32 row kernels (projection bridge, tabular fMRI/conn MLPs) ------
 * y = dropout(act((x W^T + b) * scale + shift)) (scale/shift = folded eval
 * BatchNorm1d, may be NULL), optional pre-activation copy.  nn.Linear on
 * (B, K) feature rows: bridge_utils.py:34-45,60-66; fmri_utils.py:26-35,44-53;
 * crossmodal_v4_enhancements.py:695-723. */
int mm_small_linear_fwd(const float* x, const float* W, const float* bias, const float* scale,
                        const float* shift, float* y, float* pre, int B, int K, int N, int act,
                        float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);
/* dx = dy W ; dW += dy^T x ; db += colsum(dy)   (dy already through act') */
int mm_small_linear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db,
                        int B, int K, int N, hipStream_t stream);
int mm_act_f32(const float* z, float* y, int64_t n, int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);
int mm_act_bwd_f32(const float* g, const float* z, float* out, int64_t n, int act, float drop_p,
                   uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);
/* sum_b x and sum_b x^2 (BatchNorm1d over (B, N)) into replica 0 of the ZEROED statistics accumulator workspace
 * stats [32][2][N] (the input of mm_bn_finalize) */
int mm_colstats(const float* x, float* stats, int B, int N, hipStream_t stream);
/* Both projection heads of the contrastive bridge (bridge_utils.py:34-45 eeg_proj / fmri_proj:
 * Linear(K -> N) -> LayerNorm -> GELU -> Dropout) followed by F.normalize, one launch each way.
 * x_* fp32 [B][K_*]; W_* [N][K_*]; z packed [B][2N] = [ze | zf]; nrm [2][B].  z1 / hn / stat
 * ([2][B][N], [2][B][N], [2][B][2]; all three or none) are what the backward needs.  The
 * backward ADDS parameter gradients (any of them may be null; one writer per element, rows summed in order) and
 * writes dx. */
int mm_proj_heads_fwd(const float* x_e, const float* W_e, const float* b_e, const float* g_e, const float* be_e,
                      int K_e, const float* x_f, const float* W_f, const float* b_f, const float* g_f,
                      const float* be_f, int K_f, float* z1, float* hn, float* stat, float* z, float* nrm, int B,
                      int N, float eps, float drop_p, uint32_t seed_e, uint32_t seed_f,
                      const uint32_t* seed_epoch, hipStream_t stream);
int mm_proj_heads_bwd(const float* dz, const float* z, const float* nrm, const float* hn, const float* z1,
                      const float* stat, const float* x_e, const float* W_e, const float* g_e, int K_e,
                      const float* x_f, const float* W_f, const float* g_f, int K_f, float* dx_e, float* dW_e,
                      float* db_e, float* dg_e, float* dbe_e, float* dx_f, float* dW_f, float* db_f, float* dg_f,
                      float* dbe_f, int B, int N, float drop_p, uint32_t seed_e, uint32_t seed_f,
                      const uint32_t* seed_epoch, hipStream_t stream);
/* mm_proj_heads_bwd with one more gradient at the heads' outputs: da [2][B][N] = d loss / d (the post-GELU/dropout
 * activations a_e, a_f) from a second consumer of those rows (mm_bridge_cls_bwd).  It joins the F.normalize-backward
 * term before the dropout mask and GELU'.  Same kernel, compiled with the extra load; da = 0 gives mm_proj_heads_bwd's
 * bits. */
int mm_proj_heads_bwd_da(const float* dz, const float* da, const float* z, const float* nrm, const float* hn,
                         const float* z1, const float* stat, const float* x_e, const float* W_e, const float* g_e,
                         int K_e, const float* x_f, const float* W_f, const float* g_f, int K_f, float* dx_e,
                         float* dW_e, float* db_e, float* dg_e, float* dbe_e, float* dx_f, float* dW_f, float* db_f,
                         float* dg_f, float* dbe_f, int B, int N, float drop_p, uint32_t seed_e, uint32_t seed_f,
                         const uint32_t* seed_epoch, hipStream_t stream);
/* Classification branch of the bridge (bridge_utils.py:22-114: cross attention of the EEG token over [EEG, fMRI],
 * LearnedFusionModule, Linear -> LayerNorm -> ReLU -> Dropout -> Linear, class-weighted cross-entropy) on the rows
 * mm_proj_heads_fwd produced: hn [2][B][N] with its drop_p / seed_e / seed_f (the tokens a_e, a_f are recomputed from
 * them, not evaluated a second time).  fp32, one workgroup per sample, ONE launch.  N = bridge_dim: a multiple of 32 in
 * [32, 256]; nhead <= 16 dividing it; 2 <= C <= 16.  Weights in PyTorch layout: in_w [3N][N], out_w [N][N], g0_w [N][2N],
 * g3_w [2][N], fusion_logits [2], temperature [1], c0_w [N/2][N], ln_g / ln_b [N/2], c4_w [C][N/2].  Dropout sites
 * (own seeds; element index): attention probabilities (b * nhead + h) * 2 + key, gate hidden b * N + n, classifier
 * hidden b * (N/2) + n.  Outputs (plain stores): logits [B][C], fusion_w [B][2], attn_w [B][2] (head-averaged,
 * un-dropped), save = mm_bridge_cls_ws_floats(B, N, 0) floats for the backward.  labels int32 [B] (nullable; a label
 * outside [0, C) gives its row weight 0 and indexes nothing), class_weight [C] (nullable): loss [4] = {ce = sum_b w[y_b]
 * (lse_b - logit_b[y_b]) / sum_b w[y_b], rows with argmax == y_b, sum_b w[y_b], ce_weight * ce}, summed in row order by
 * the workgroup that finishes last (ticket: one int32 word, zero before the first launch, left zero).  Without labels
 * loss and ticket are not touched. */
int mm_bridge_cls_fwd(const float* hn, float drop_p, uint32_t seed_e, uint32_t seed_f, const float* in_w,
                      const float* in_b, const float* out_w, const float* out_b, const float* g0_w, const float* g0_b,
                      const float* g3_w, const float* g3_b, const float* fusion_logits, const float* temperature,
                      const float* c0_w, const float* c0_b, const float* ln_g, const float* ln_b, const float* c4_w,
                      const float* c4_b, const int* labels, const float* class_weight, float ce_weight, float* logits,
                      float* fusion_w, float* attn_w, float* save, float* loss, int* ticket, int B, int N, int nhead,
                      int C, float ln_eps, float attn_p, uint32_t seed_attn, float gate_p, uint32_t seed_gate,
                      float cls_p, uint32_t seed_cls, const uint32_t* seed_epoch, hipStream_t stream);
/* backward of ce_weight * ce, TWO launches, no float atomics: one call per launch with the same arguments, phase 0
 * (rows) then phase 1 (weights).  Rows (a workgroup per sample): the gradient at every
 * Linear's output and the per-row pieces of the LayerNorm / fusion_logits / temperature gradients into grad_rows
 * (mm_bridge_cls_ws_floats(B, N, 1) floats), da [2][B][N] = the gradient of a_e and a_f (plain stores; the extra input
 * of mm_proj_heads_bwd_da), and loss_total[0] = loss_in[0] + ce_weight * ce when loss_total is given (loss_in null: 0).
 * Weights: every d_* target (nullable) gets its sum over the rows, in row order, ADDED by the one thread that owns the
 * element; in_proj's q rows from a_e, its k / v rows from both tokens. */
int mm_bridge_cls_bwd(const float* save, const float* logits, const float* loss, const int* labels, float ce_weight,
                      const float* in_w, const float* out_w, const float* g0_w, const float* g3_w,
                      const float* fusion_logits, const float* temperature, const float* c0_w, const float* ln_g,
                      const float* ln_b, const float* c4_w, float* grad_rows, float* da, float* d_in_w, float* d_in_b,
                      float* d_out_w, float* d_out_b, float* d_g0_w, float* d_g0_b, float* d_g3_w, float* d_g3_b,
                      float* d_fusion_logits, float* d_temperature, float* d_c0_w, float* d_c0_b, float* d_ln_g,
                      float* d_ln_b, float* d_c4_w, float* d_c4_b, const float* loss_in, float* loss_total, int phase, int B,
                      int N, int nhead, int C, float attn_p, uint32_t seed_attn, float gate_p, uint32_t seed_gate, float cls_p,
                      uint32_t seed_cls, const uint32_t* seed_epoch, hipStream_t stream);
int mm_bridge_cls_ws_floats(int B, int N, int which, int* floats_host, hipStream_t stream);
/* Feature half of the tabular fMRI net (fMRI_CODE/fmri_utils.py:23-108: ActivationEncoder, ConnectivityEncoder, the softmax-
 * weighted concat and the `fusion` block of fMRIFusionNet; what the reference's bridge trains on, _test_bridge.py
 * extract_fmri_features) in ONE forward and ONE backward launch, no float atomics, every sum in a fixed order.  Tensors are
 * fp32; the Linear layers' sums over k, the batch statistics and the normalisation are accumulated in fp64 (a small
 * batch's 1 / deviation multiplies their rounding into every gradient).
 * x [B][A + C] = [activation | connectivity] (no alignment asked of A, C or any pointer); H = hidden_dim in {32, 64, 128}.
 * Five Linear -> BatchNorm1d -> ReLU -> Dropout layers, in this order in every argument list, seed list and buffer:
 * a1 (A -> 2H), a2 (2H -> H), c1 (C -> 2H), c2 (2H -> H), f ([wa * a2 | wc * c2] -> H), (wa, wc) = softmax of the two
 * scalars.  Per layer: w [out][in], b, BatchNorm g / be, running mean / var, num_batches_tracked (int64, nullable).
 * train = 1: batch statistics (2 <= B <= 256), running statistics updated with `momentum` (unbiased variance) and the
 * counters incremented by the one workgroup that owns the feature.  train = 0: frozen BatchNorm (running statistics), any
 * B >= 1, drop_p must be 0.  Dropout: five seeds in layer order; element index = b * width + f, the flat row-major index
 * of the layer's (B, width) output.  out [B][H] = the fused feature.  save = 13 B H + 14 H floats for the backward: per
 * layer the pre-activation (the Linear's output) and (but for f, whose output is `out`) the post-dropout output - a1 x|h
 * (2 B H each), a2 x|h (B H each), c1, c2 alike, f x - then the layers' means (2H, H, 2H, H, H) and inverse standard
 * deviations (alike) as the forward used them.
 * tickets: THREE int32 words owned by the caller, zero before the first launch and left zero: 2 x (2H / 8) workgroups each
 * own eight features of a first layer; the last arriver of a branch runs its second layer, the last of those two the
 * fusion layer.  No workgroup waits for another. */
int mm_fmri_tab_fwd(const float* x, int B, int A, int C, int H,
                    const float* a1_w, const float* a1_b, const float* a1_g, const float* a1_be, float* a1_rm,
                    float* a1_rv, int64_t* a1_nbt,
                    const float* a2_w, const float* a2_b, const float* a2_g, const float* a2_be, float* a2_rm,
                    float* a2_rv, int64_t* a2_nbt,
                    const float* c1_w, const float* c1_b, const float* c1_g, const float* c1_be, float* c1_rm,
                    float* c1_rv, int64_t* c1_nbt,
                    const float* c2_w, const float* c2_b, const float* c2_g, const float* c2_be, float* c2_rm,
                    float* c2_rv, int64_t* c2_nbt,
                    const float* f_w, const float* f_b, const float* f_g, const float* f_be, float* f_rm, float* f_rv,
                    int64_t* f_nbt,
                    const float* activation_weight, const float* connectivity_weight, float* out, float* save,
                    int* tickets, int train, float eps, float momentum, float drop_p, uint32_t seed_a1,
                    uint32_t seed_a2, uint32_t seed_c1, uint32_t seed_c2, uint32_t seed_f, const uint32_t* seed_epoch,
                    hipStream_t stream);
/* its backward from dout [B][H] = d loss / d out (same train / eps / drop_p; the ReLU and dropout masks are read off the
 * saved outputs).  fp32 but for the BatchNorm backward's sums over the batch, which run in fp64 on batch statistics formed
 * again from the saved pre-activations (where BatchNorm passes little gradient the result is a small difference of large
 * terms).  Every d_* destination (nullable) and dx [B][A + C] (nullable) is written with PLAIN stores by its only
 * writer: ceil(A / 64) + ceil(C / 64) workgroups each own 64 input columns of a first layer (d w1[:, k], dx[:, k]), three
 * more own the small matrices; each recomputes the B x (H | 2H) chain it needs in its own part of `scratch` =
 * (ceil(A / 64) + ceil(C / 64) + 3) * 4 B H floats (no initialisation).  No ticket, no workgroup waits for another. */
int mm_fmri_tab_bwd(const float* dout, const float* x, const float* out, const float* save, int B, int A, int C, int H,
                    const float* a1_w, const float* a1_g, const float* a2_w, const float* a2_g, const float* c1_w,
                    const float* c1_g, const float* c2_w, const float* c2_g, const float* f_w, const float* f_g,
                    const float* activation_weight, const float* connectivity_weight, float* scratch, float* dx,
                    float* d_a1_w, float* d_a1_b, float* d_a1_g, float* d_a1_be, float* d_a2_w, float* d_a2_b,
                    float* d_a2_g, float* d_a2_be, float* d_c1_w, float* d_c1_b, float* d_c1_g, float* d_c1_be,
                    float* d_c2_w, float* d_c2_b, float* d_c2_g, float* d_c2_be, float* d_f_w, float* d_f_b,
                    float* d_f_g, float* d_f_be, float* d_activation_weight, float* d_connectivity_weight, int train,
                    float eps, float drop_p, hipStream_t stream);
/* Lag attention pooling over the frame features of an fMRI sequence (no reference counterpart: the reference pairs an
 * epoch with one fMRI row).  x [B][F][N] fp32, q [N] and c [F] the two trained vectors:
 *   s[b][f] = (x[b][f] . q) / sqrt(N) + c[f],  attw[b] = softmax_f(s[b]) (max-subtracted),  out[b] = sum_f attw[b][f] x[b][f]
 * and from dout [B][N], with da[b][f] = dout[b] . x[b][f] and ds[b][f] = attw[b][f] (da[b][f] - sum_g attw[b][g] da[b][g]):
 *   dx[b][f] = attw[b][f] dout[b] + ds[b][f] q / sqrt(N),   dparts[b] = ( sum_f ds[b][f] x[b][f] / sqrt(N) | ds[b][.] )
 * dparts [B][N + F] are the per-sample rows (dq_b | dc_b); dq and dc are their sums in ascending b (mm_reduce_many /
 * mm_flush_many, nrep = -B).  ONE launch each, one wave per sample.  All fp32 with the accurate expf; every element of
 * out, attw [B][F], dx [B][F][N] and dparts is written with a plain store (nothing needs zeroing); no sample reads another
 * sample's data or results; the same inputs give the same bits.  The exponent is formed from differences to the row's
 * largest score, so a common offset of c of any size drops out exactly; ds is evaluated as attw[f] sum_g attw[g] (da[f] -
 * da[g]) (equal, since the weights sum to 1), which keeps its relative accuracy when the softmax is nearly one-hot.
 * 1 <= F <= 64, N % 4 == 0, 4 <= N <= 1024, B >= 1; x, out, dout and dx 16-byte aligned (q and c: parameters, any float
 * offset of a flat bucket).
 * F == 1: attw is exactly 1.0f, out is x and dx is dout bit for bit, dparts is exactly zero. */
int mm_lagpool_fwd(const float* x, const float* q, const float* c, float* out, float* attw, int B, int F, int N,
                   hipStream_t stream);
int mm_lagpool_bwd(const float* dout, const float* x, const float* attw, const float* q, float* dx, float* dparts, int B,
                   int F, int N, hipStream_t stream);
/* The encoders of the fMRI notebook's transformer model (fMRI_CODE/CrossModal_fmri_scr.ipynb, cell "# ENCODER BLOCKS":
 * ActivationEncoder / ConnectivityEncoder = Linear(in_dim -> H), nn.TransformerEncoder of L post-norm layers (nhead 4,
 * dim_feedforward 4H, ReLU) on a sequence of length ONE, LayerNorm(H)) for one or two stacks in ONE launch: replaces the
 * `self.project(x)`, `self.transformer(x)`, `self.norm(x)` calls of that cell's two forward methods.  With one key the
 * softmax is 1: per layer v = Wv h + bv, sa = Wo (keep_attn * v) + bo, h = LN1(h + drop1(sa)), h = LN2(h + drop2(W2
 * drop(relu(W1 h + b1)) + b2)), eps 1e-5.  fp32 throughout, sums over k ascending, no atomics, no workgroup waits for
 * another: grid (ceil(B / 16), stacks), a workgroup keeps 16 rows of one stack in LDS.
 * x_s [B][in_s] (no alignment asked), out_s [B][H]; H in {32, 64, 128}, 1 <= L <= 8, B >= 1; stack 1's arguments are ignored
 * when nstacks = 1.  params_host: HOST array of nstacks * (4 + 12 L) device pointers, per stack the module's parameters()
 * order: project.weight [H][in], project.bias, per layer in_proj_weight [3H][H], in_proj_bias, out_proj.weight, out_proj.bias,
 * linear1.weight [4H][H], linear1.bias, linear2.weight [H][4H], linear2.bias, norm1.weight, norm1.bias, norm2.weight,
 * norm2.bias, then norm.weight, norm.bias (copied into the launch's arguments).
 * Dropout: seeds_host = HOST array of nstacks * 4 L seeds (read only when drop_p > 0), per stack in layer order then site
 * order: attention (one draw per (row, head): element index b * 4 + head), dropout1 (b * H + f), FFN middle (b * 4H + f),
 * dropout2 (b * H + f).
 * save (nullable: eval / no_grad, then only out is written): nstacks * (1 + 9 L) B H floats for the backward, per stack
 * h0 [B][H], then per layer mv [B][H] = keep_attn * v, y1 (LN1 input), h1 (LN1 output), mid [B][4H] (post ReLU and
 * dropout), y2 (LN2 input), h2 (LN2 output). */
int mm_tab_tx_fwd(const float* x0, const float* x1, int nstacks, int B, int in0, int in1, int H, int L,
                  const void* params_host, float* out0, float* out1, float* save, float drop_p,
                  const uint32_t* seeds_host, const uint32_t* seed_epoch, hipStream_t stream);
/* its backward (replaces autograd through the same cell), TWO launches: a row-local pass with the forward's decomposition
 * that leaves the gradient at every Linear's output and every LayerNorm's dy, dy * xhat in `scratch` = nstacks *
 * (3 + 11 L) B H floats (no initialisation) and writes dx_s [B][in_s] (nullable: skipped); then a parameter pass in which
 * one workgroup owns a 64 x 64 tile of one weight gradient, or one layer's column sums, rows ascending.  grads_host: HOST
 * array of destinations in params_host's layout, each nullable; every destination is written with PLAIN stores by its only
 * writer, and the query / key rows of in_proj_weight / in_proj_bias (which never reach the output) are written as ZEROS.
 * LayerNorm has no train / eval distinction: the same call serves eval-mode attribution with drop_p = 0. */
int mm_tab_tx_bwd(const float* dout0, const float* dout1, const float* x0, const float* x1, int nstacks, int B, int in0,
                  int in1, int H, int L, const void* params_host, const void* grads_host, const float* save,
                  float* scratch, float* dx0, float* dx1, float drop_p, const uint32_t* seeds_host,
                  const uint32_t* seed_epoch, hipStream_t stream);
/* batch-pairwise cosine-similarity matrix + symmetric InfoNCE, bit-reproducible (no float atomics).
 * Embeddings are packed rows [ze (N) | zf (N)]: z_all [Bg][2N] = the all-gathered global batch, this rank's
 * pairs at rows [row0, row0+B).  C[r][j] = ze_r . zf_j; e->f = row softmax of exp(logit_scale) C, f->e =
 * column softmax.  scal4 = {mean loss, top1 e->f, top1 f->e, d loss / d logit_scale} over the rank's own rows
 * (plain stores: no zeroing needed); dz_local [B][2N] (nullable, plain stores) = d (SUM over ranks of their
 * losses) / d z_local - exactly the block a reduce-scatter-sum of every rank's d loss / d z_all would
 * deliver, so the step needs no reduce-scatter (every rank evaluates all Bg rows of the gathered batch:
 * 2 Bg^2 N MACs).  ws = scratch of mm_clip_loss_ws_floats(B, Bg) floats (log-sum-exp of every row and
 * column + per-row scalars), no initialisation needed.  N % 4 == 0.  Two launches on `stream`.
 * Extension a-X2: the reference trains a CE classifier (_test_bridge.py:858). */
int mm_clip_loss_own_rows(const float* z_all, const float* logit_scale, float* scal4, float* dz_local, float* ws,
                          int B, int Bg, int N, int row0, hipStream_t stream);
int mm_clip_loss_ws_floats(int B, int Bg, int* floats_host, hipStream_t stream);
/* the same loss with subject-grouped positives.  gid_all int32 [Bg] (gathered like z_all): pairs with equal ids are
 * positives of each other, P(r) = {j : gid_j = gid_r} (always holds r).  Per row, "log of the positive mass" (MIL-NCE):
 * l_row(r) = LSE_j(s C[r][j]) - LSE_{j in P(r)}(s C[r][j]), l_col(r) the same over column r, loss_r = (l_row + l_col) / 2.
 * dz_local and scal4 as above; top-1 counts row r when max_{j in P(r)} C[r][j] >= max_j C[r][j] (a tie FOR it).  With
 * all-distinct ids this is mm_clip_loss_own_rows' loss.  ws = mm_clip_loss_grouped_ws_floats(B, Bg) floats, no
 * initialisation.  N % 4 == 0.  Two launches on `stream`; same inputs -> bit-identical outputs. */
int mm_clip_loss_own_rows_grouped(const float* z_all, const int* gid_all, const float* logit_scale, float* scal4,
                                  float* dz_local, float* ws, int B, int Bg, int N, int row0, hipStream_t stream);
int mm_clip_loss_grouped_ws_floats(int B, int Bg, int* floats_host, hipStream_t stream);
/* the grouped loss with IGNORED keys: the ids are positions on a timeline and temporal neighbours are neither positives
 * nor negatives.  gid_all int32 [Bg] as above, radius >= 0.  For query r and key j, d = |gid_j - gid_r| computed so that it
 * cannot wrap (ids -2^31 and 2^31 - 1 are 2^32 - 1 apart):
 *   d == 0: positive, P(r) (always holds r)      0 < d <= radius: ignored      d > radius: negative
 *   A(r) = {j : d == 0 or d > radius}, the admitted keys; the relation is symmetric and serves rows and columns alike
 *   l_row(r) = LSE_{j in A(r)}(s C[r][j]) - LSE_{j in P(r)}(s C[r][j]), l_col(r) the same over column r, loss_r = (l_row + l_col) / 2
 *   dL/dC[r][j] = 0.5/B * s * ([j in A(r)] (P_row + P_col)[r][j] - [d == 0] (Q_row + Q_col)[r][j])
 * with P_row[r][j] = exp(s C[r][j] - LSE_A(row r)), P_col[r][j] = exp(s C[r][j] - LSE_A(column j)) and Q the same over the
 * positive sets.  An ignored key is in no normaliser and no positive set, its pair's coefficient is exactly 0.f (stored, not
 * computed: whatever finite values the key holds), and d loss / d logit_scale sums over A and P in the same way.  top-1 counts
 * row r when max_{j in P(r)} C[r][j] >= max_{j in A(r)} C[r][j] (a tie FOR it).  A row without an admitted negative has
 * A = P: loss, d / d logit_scale and gradient exactly 0 (stored, as for an ignored pair).  radius = 0 is mm_clip_loss_own_rows_grouped's loss.  scal4, dz_local, the own
 * rows (B, Bg, row0) and the rules (no float atomics, fixed-order sums, same inputs -> bit-identical outputs) as above.
 * ws = mm_clip_loss_masked_ws_floats(B, Bg) floats, no initialisation.  N % 4 == 0.  Two launches on `stream`.
 * Extension: the reference has no contrastive trainer. */
int mm_clip_loss_own_rows_masked(const float* z_all, const int* gid_all, const float* logit_scale, float* scal4,
                                 float* dz_local, float* ws, int B, int Bg, int N, int row0, int radius,
                                 hipStream_t stream);
int mm_clip_loss_masked_ws_floats(int B, int Bg, int* floats_host, hipStream_t stream);
/* pairwise sigmoid loss (Zhai et al., "Sigmoid Loss for Language Image Pre-Training") on the same inputs: z_all [Bg][2N]
 * L2-normalised [ze | zf] rows of the gathered batch, this rank's pairs at rows [row0, row0+B), gid_all int32 [Bg] or
 * NULL, and two device scalars logit_scale (ln s) and logit_bias (b).  Every pair is its own binary problem:
 *   C[r][j] = ze_r . zf_j        s = exp(logit_scale)        u[r][j] = s C[r][j] + b
 *   y[r][j] = +1 if (gid NULL ? r == j : gid_r == gid_j) else -1
 *   l[r][j] = softplus(-y[r][j] u[r][j])        loss_r = sum_j l[r][j]  (all Bg columns)
 *   rank loss       = (1/B) sum_{r own} loss_r
 *   G[r][j]         = -y[r][j] s sigmoid(-y[r][j] u[r][j])        (= d l[r][j] / d C[r][j])
 *   dze_r           = (1/B) sum_j G[r][j] zf_j        dzf_r = (1/B) sum_j G[j][r] ze_j        (r own; j over all Bg)
 *   d/d logit_scale = (1/B) sum_{r own} sum_j G[r][j] C[r][j]
 *   d/d logit_bias  = (1/B) sum_{r own} sum_j -y[r][j] sigmoid(-y[r][j] u[r][j])
 * dz_local [B][2N] = [dze | dzf] (nullable: scalars only; plain stores) is, as for InfoNCE, d (SUM over ranks of their
 * rank losses) / d (own rows): column r's terms G[j][r] belong to other ranks' rows and are evaluated here from the
 * gathered batch, so no reduce-scatter is needed.  scal5 = {rank loss, top1 e->f, top1 f->e, d/d logit_scale,
 * d/d logit_bias} (plain stores); the top-1 flags are mm_clip_loss_own_rows_grouped's: row r counts when its best positive
 * reaches the row maximum of C (a tie FOR it), f->e the same over column r.  All fp32; softplus(x) = max(x, 0) +
 * log1p(exp(-|x|)) with an accurate log1p, sigmoid from the same exp(-|x|).  No float atomics, every sum in a fixed order:
 * same inputs -> bit-identical outputs.  ws = mm_sigmoid_loss_ws_floats(B, Bg) floats (per-row scalars), no
 * initialisation.  N % 4 == 0.  Two launches on `stream`; no row reads another row's results.
 * Extension: the reference has no contrastive trainer. */
int mm_sigmoid_loss_own_rows(const float* z_all, const int* gid_all, const float* logit_scale, const float* logit_bias,
                             float* scal5, float* dz_local, float* ws, int B, int Bg, int N, int row0,
                             hipStream_t stream);
int mm_sigmoid_loss_ws_floats(int B, int Bg, int* floats_host, hipStream_t stream);
/* the same with IGNORED pairs (relations, gid_all (required) and radius >= 0 as mm_clip_loss_own_rows_masked): an ignored
 * pair (0 < |gid_j - gid_r| <= radius, the difference computed so that it cannot wrap) contributes l[r][j] = 0 and
 * G[r][j] = exactly 0.f to every sum above, in both directions; y = +1 where the ids are equal, -1 beyond the radius.  The
 * 1/B normalisation is unchanged; the top-1 flags are mm_clip_loss_own_rows_masked's (the maximum runs over the admitted
 * keys).  radius = 0 is mm_sigmoid_loss_own_rows with ids.  ws = mm_sigmoid_loss_masked_ws_floats(B, Bg) floats, no
 * initialisation.  N % 4 == 0.  Two launches on `stream`; same inputs -> bit-identical outputs. */
int mm_sigmoid_loss_own_rows_masked(const float* z_all, const int* gid_all, const float* logit_scale,
                                    const float* logit_bias, float* scal5, float* dz_local, float* ws, int B, int Bg,
                                    int N, int row0, int radius, hipStream_t stream);
int mm_sigmoid_loss_masked_ws_floats(int B, int Bg, int* floats_host, hipStream_t stream);
/* symmetric InfoNCE against the batch AND a cross-batch memory of earlier embeddings (csrc/clip_bank.hip; Wang et al.,
 * "Cross-Batch Memory for Embedding Learning").  All storage is the caller's device memory, allocated before any capture:
 *   bank     fp32  [K][2N]  rows [ze | zf], L2-normalised, exactly as z (keys only, constants: no loss, no gradient)
 *   bank_gid int32 [K]      the rows' group ids (nullable; required when gid is given)
 *   state    int32 [4]      {head, filled, pushes, 0}; zero them to empty the bank
 * z [B][2N] the own rows, gid int32 [B] or NULL, logit_scale one device float (ln s).  n = (state.pushes >= warmup) ?
 * state.filled : 0 is read ON THE DEVICE, so the same launch arguments (and a captured graph) serve every fill level;
 * valid bank rows are ring slots [0, n) (the ring never wraps before it is full).  For own row r, s = exp(logit_scale):
 *   e->f keys {zf_j : j < B} u {bank_k.zf : k < n}, query ze_r;   f->e keys {ze_j} u {bank_k.ze}, query zf_r
 *   P(r): gid NULL: the batch key r only (no bank row is ever a positive); else every batch or bank key whose id = gid_r
 *   l_dir(r) = LSE_{all keys}(s q.key) - LSE_{P(r)}(s q.key)        loss = (1/B) sum_r (l_e2f(r) + l_f2e(r)) / 2
 * ("log of the positive mass", as mm_clip_loss_own_rows_grouped; with n = 0 it is that kernel's loss at Bg = B).
 * dz [B][2N] (nullable, plain stores) = d loss / d z: ze_r's query term over batch and bank keys + its key term from every
 * batch fMRI query's f->e softmax, zf_r symmetric; bank rows get nothing and are never written.  scal4 = {loss, top1 e->f,
 * top1 f->e, d loss / d logit_scale} (plain stores); top-1 counts row r when its best positive reaches the maximum over
 * all keys, bank included (a tie FOR it).  All fp32, no float atomics, every sum in a fixed order (per-key-chunk partials
 * combined in chunk order): same inputs + same state -> bit-identical outputs.  Rows at or beyond n are never read (their
 * memory may hold anything, NaN included).  ws = mm_clip_bank_ws_floats(B, K, N) floats (the 2 B (B + K) scores and the
 * chunk partials), no initialisation.  N % 4 == 0, 1 <= B <= K, warmup >= 0; z, bank, dz, ws 16-byte aligned.  Two
 * launches on `stream`, both grids sized by the capacity K; no workgroup waits for another.
 * Extension: the reference has no contrastive trainer. */
int mm_clip_bank_loss(const float* z, const int* gid, const float* bank, const int* bank_gid, const int* state,
                      const float* logit_scale, float* scal4, float* dz, float* ws, int B, int K, int N, int warmup,
                      hipStream_t stream);
/* the B rows of z (and their ids, when gid is given) into ring slots (head + i) mod K, THEN head = (head + B) mod K,
 * filled = min(filled + B, K), pushes += 1.  One launch of ONE workgroup: every thread reads the words, the rows are
 * copied, and thread 0 advances the words behind the workgroup's barrier (plain stores).  Same shape rules. */
int mm_clip_bank_push(const float* z, const int* gid, float* bank, int* bank_gid, int* state, int B, int K, int N,
                      hipStream_t stream);
/* host-only: floats of mm_clip_bank_loss's workspace */
int mm_clip_bank_ws_floats(int B, int K, int N, int* floats_host, hipStream_t stream);
/* mm_clip_bank_loss with the batch's keys taken from a SECOND set of rows (a momentum key encoder's embeddings of the same
 * pairs; He et al., "Momentum Contrast"): q [B][2N] = [qe | qf] the online rows (queries only; gradients flow into them),
 * k [B][2N] = [ke | kf] the key rows of the same pairs (constants); bank, bank_gid, state, gid, logit_scale, warmup, n as
 * above.  Key index t < B is k's row t, else bank slot t - B:
 *   e->f: query qe_r over keys kf_t;   f->e: query qf_r over keys ke_t;   P(r) = {t : gid_t = gid_r} (gid NULL: {r})
 *   l_dir(r) = LSE_t(s x[r][t]) - LSE_{t in P(r)}(s x[r][t])        loss = (1/B) sum_r (l_e2f(r) + l_f2e(r)) / 2
 *   dqe_r = sum_t G_e2f[r][t] kf_t,  dqf_r = sum_t G_f2e[r][t] ke_t,  G = 0.5 s / B (softmax - [t in P] softmax over P)
 * There is no key term: neither k nor the bank receives anything or is written.  dq [B][2N] nullable (plain stores);
 * scal4 = {loss, top1 e->f, top1 f->e, d loss / d logit_scale}, top-1 as in mm_clip_bank_loss.  q and k may be the same
 * rows (the loss is then mm_clip_bank_loss's, to rounding).  All fp32, no float atomics, every sum in a fixed order: same
 * inputs + same state -> bit-identical outputs.  Rows at or beyond n are never read.  ws = mm_clip_key_ws_floats(B, K, N)
 * floats (scores, chunk partials, the folded normalisers, the key tiles' dq sums and tickets), no initialisation.  N % 4 == 0, 1 <= B <= K, warmup >= 0; q, k,
 * bank, dq, ws 16-byte aligned.  Three launches on `stream` (scores + chunk partials; the fold of the partials, once per
 * query and direction; dq, one workgroup per tile of 8 queries x 32 columns x 512 keys, a key row read once per query
 * tile - dq NULL: one workgroup for the scalars), grids sized by the capacity K.  No workgroup waits for another: with more
 * than one key tile each workgroup stores its sums and takes an integer ticket (zeroed by the second launch), and the last
 * arriver adds the tiles' sums in tile order.
 * Extension: the reference has no contrastive trainer. */
int mm_clip_key_loss(const float* q, const float* k, const int* gid, const float* bank, const int* bank_gid,
                     const int* state, const float* logit_scale, float* scal4, float* dq, float* ws, int B, int K, int N,
                     int warmup, hipStream_t stream);
/* host-only: floats of mm_clip_key_loss's workspace */
int mm_clip_key_ws_floats(int B, int K, int N, int* floats_host, hipStream_t stream);

/* ---- gallery-scale retrieval (csrc/retrieval.hip) ---------------------------
 * For each query row q of Q [Nq][D] against gallery G [Ng][D] (fp32, row-major, 16-byte aligned; callers pass
 * L2-normalised rows): s(q, j) = the ascending-d fmaf chain over d = 0..D-1 starting from +0 (what
 * v_mfma_f32_32x32x2_f32 computes bit for bit; no bf16 anywhere: a rank is a comparison).
 * ranks (nullable) int32 [Nq]: 1 + #{ j != pos[q] : s(q, j) >= s(q, pos[q]) } - ties count AGAINST the query, so an
 *        encoder that scores every pair alike ranks Ng (mm_clip_loss_own_rows' in-batch top-1 counts a tie FOR it);
 *        pos (nullable -> pos[q] = q, which needs Nq <= Ng) int32 [Nq] in [0, Ng).  A NaN s(q, pos[q]) (or a pos
 *        outside the gallery) -> rank Ng; a NaN s(q, j) never counts.
 * topk_idx int32 / topk_score fp32 [Nq][k] (k = 0: none, pointers may be NULL): the k best j by score descending,
 *        equal scores by lower j; NaN never selected; unfilled slots (-1, -inf).  k <= MM_RETRIEVAL_KMAX, k <= Ng.
 * ws = mm_retrieval_ws_floats(Nq, Ng, D, k) floats of scratch, no initialisation.  D % 4 == 0, 4 <= D <= 1024,
 * 1 <= Nq, Ng <= MM_RETRIEVAL_NMAX.  Needs ranks or k > 0.  No Nq x Ng storage: scores live in accumulators and LDS.
 * Deterministic: same inputs -> bit-identical outputs (integer counts, no float atomics).  Three launches on `stream`.
 * Extension: the reference has no retrieval evaluator. */
#define MM_RETRIEVAL_KMAX 16
#define MM_RETRIEVAL_NMAX (1 << 20)
int mm_retrieval(const float* Q, const float* G, const int* pos, int* ranks, int* topk_idx, float* topk_score,
                 float* ws, int Nq, int Ng, int D, int k, hipStream_t stream);
int mm_retrieval_ws_floats(int Nq, int Ng, int D, int k, int* floats_host, hipStream_t stream);
/* ranks with grouped positives: qgid int32 [Nq], ggid int32 [Ng] (e.g. subject ids); gallery row j is a positive of
 * query q when ggid[j] == qgid[q].  s*(q) = max over the positives of s(q, j) (NaN scores ignored), scored by the same
 * MFMA chain as mm_retrieval, and ranks[q] = 1 + #{ j : ggid[j] != qgid[q], s(q, j) >= s*(q) }: the rank of the
 * best-placed positive, the other positives never count; a tie with s* counts AGAINST the query, a NaN s(q, j) never
 * counts, a query without a positive (or with only NaN positive scores) ranks Ng.  ws =
 * mm_retrieval_grouped_ws_floats(Nq, Ng, D) floats, no initialisation; shape limits as mm_retrieval.  No Nq x Ng
 * storage, integer counts: deterministic.  Four launches on `stream`.  Top-k does not depend on groups: mm_retrieval. */
int mm_retrieval_grouped(const float* Q, const float* G, const int* qgid, const int* ggid, int* ranks, float* ws,
                         int Nq, int Ng, int D, hipStream_t stream);
int mm_retrieval_grouped_ws_floats(int Nq, int Ng, int D, int* floats_host, hipStream_t stream);
/* ranks and top-k with ignored temporal neighbours: the ids are positions on a timeline (bridge_utils.timeline_ids) and
 * d(q, j) = |ggid[j] - qgid[q]|, the unsigned difference of the larger and the smaller id (ids -2^31 and 2^31 - 1 are
 * 2^32 - 1 apart), as in mm_clip_loss_own_rows_masked.  radius >= 0.  d == 0: positive; 0 < d <= radius: IGNORED (neither a
 * positive nor a negative; what the row holds - any finite value, NaN - changes nothing for that query); d > radius:
 * negative; A(q) = {j : d == 0 or d > radius} is the admitted set.  s*(q) as mm_retrieval_grouped (same MFMA chain, NaN
 * scores skipped).
 * ranks (nullable when k > 0) int32 [Nq]: 1 + #{ j : d > radius, s(q, j) >= s*(q) }; a tie counts AGAINST the query; a
 *        query without a positive, or with only NaN positive scores, ranks Ng.
 * negatives (nullable) int32 [Nq]: #{ j : d > radius } - ids only, no score enters: the query's effective gallery minus
 *        its positives.
 * topk_idx / topk_score [Nq][k] (required when k > 0): the k best rows of A(q) - positives included, ignored rows never -
 *        in mm_retrieval's order (score descending, then index ascending; NaN never selected; unfilled (-1, -inf)).
 * radius = 0: ranks are mm_retrieval_grouped's and top-k is mm_retrieval's, bit for bit.
 * ws = mm_retrieval_masked_ws_floats(Nq, Ng, D, k) = Nq (1 + S (2 + 2 k)) floats, no initialisation, S = the number of
 * gallery slices: with QB = ceil(Nq / 128) and T = ceil(Ng / 128), W = max(1, min(T, ceil(512 / QB))), S = ceil(T /
 * ceil(T / W)).  Layout: s* [Nq] | per-slice maxima, then counts [S][Nq] | per-slice id-only counts [S][Nq] (written only
 * with negatives) | list scores [S][Nq][k] | list indices [S][Nq][k].  Shape limits, alignment and the int-overflow check
 * as mm_retrieval; null Q, G, qgid, ggid or ws, radius < 0, and ranks == NULL with k == 0 are errors before any launch.
 * At most four launches on `stream` (maxima sweep, best, counting / top-k sweep, finish; two with ranks == NULL).
 * Integer counts, no float atomics: deterministic. */
int mm_retrieval_masked(const float* Q, const float* G, const int* qgid, const int* ggid, int radius, int* ranks,
                        int* negatives, int* topk_idx, float* topk_score, float* ws, int Nq, int Ng, int D, int k,
                        hipStream_t stream);
int mm_retrieval_masked_ws_floats(int Nq, int Ng, int D, int k, int* floats_host, hipStream_t stream);

/* ---- EnhancedPowerEncoder: its three Conv1d(C -> 64, k = 3 | 5 | 7) + BatchNorm1d(64) branches
 * (enhanced_models_v4.py:210-234, forward :258-266: torch.cat of the three) as ONE Conv1d(C -> 192, k = 7, p = 3) +
 * BatchNorm1d(192).  desc_host = HOST pointer to this descriptor (read at call time, like the tables of mm_prep_many):
 *   mode 0  parts -> merged: W[o][c][t] = w_i[o % 64][c][t - (7 - k_i) / 2] inside branch i = o / 64's taps, else 0;
 *           bias / gamma / beta / running mean / running var concatenated
 *   mode 1  merged running mean / var -> the parts' (after a train-mode forward); batches_tracked[i] += 1 (nullable)
 *   mode 2  gradients: the parts' sinks (w, b, gamma, beta; null = frozen) += their slices of the merged gradients
 *           (W, B, Gamma, Beta; null = absent)
 *   mode 3  as mode 0, but W receives the merged weight as mm_conv1d_fwd's bf16 image [192][7][cinp] (what
 *           mm_prep_conv_weight makes of the fp32 merged weight, which is then never written) */
typedef struct {
    float* w[3]; float* b[3]; float* gamma[3]; float* beta[3]; float* run_mean[3]; float* run_var[3];
    void* batches_tracked[3];            /* int64 device scalars */
    float* W; float* B; float* Gamma; float* Beta; float* Run_mean; float* Run_var;
    int cin; int k[3]; int cinp; int reserved;
} mm_power_merge_t;
int mm_power_merge(const void* desc_host, int mode, hipStream_t stream);

/* ---- fused tails of the small models (forward) ------------------------------ */
/* fMRIFusionNet weighted concat (fmri_utils.py:93-96) */
int mm_softmax2_concat(const float* a, const float* c, const float* pa, const float* pc, float* out, int B,
                       int Ha, int Hc, hipStream_t stream);
/* LearnedFusionModule combine (enhanced_models_v4.py:468-484); dyn = gate_net output [B][M] */
int mm_learned_fusion(const float* f0, const float* f1, const float* f2, const float* dyn,
                      const float* logits, const float* temperature, float* fused, float* weights, int B,
                      int H, int M, hipStream_t stream);
/* nn.MultiheadAttention core for ONE query token and K <= 4 key/value tokens per sample: the
 * modality-level cross attention of the V4 classifiers (crossmodal_v4_enhancements.py:366-372 K = 3,
 * :448-456 K = 2).  p_j = in_proj(token_j) fp32 [B][3E] = [q | k | v]; the query is token 0's q.
 * backward == 0: ctx [B][E] (+ head-averaged attw [B][K], nullable);  backward == 1: dp_j [B][3E] from
 * dctx.  Attention-probability dropout by counter hash, recomputed in backward. */
int mm_attn_1xk(const float* p0, const float* p1, const float* p2, const float* p3, int K, const float* dctx,
                float* ctx, float* attw, float* dp0, float* dp1, float* dp2, float* dp3, int B, int E,
                int nhead, float drop_p, uint32_t seed, const uint32_t* seed_epoch, int backward,
                hipStream_t stream);
int mm_add_f32(const float* a, const float* b, float* out, int64_t n, hipStream_t stream);
/* bridge cross-attention core, 1 query x 2 keys (bridge_utils.py:75-82) */
int mm_attn_1x2(const float* proj_e, const float* proj_f, float* ctx, float* attw, int B, int E, int nhead,
                hipStream_t stream);
/* trainable form of the 1x2 cross-attention core (with attention-probability dropout):
 * backward == 0: ctx/attw from proj_e/proj_f;  backward == 1: dproj_e/dproj_f [B][3E] from dctx */
int mm_attn_1x2_train(const float* proj_e, const float* proj_f, const float* dctx, float* ctx, float* attw,
                      float* dproj_e, float* dproj_f, int B, int E, int nhead, float drop_p, uint32_t seed,
                      const uint32_t* seed_epoch, int backward, hipStream_t stream);
/* backward of mm_learned_fusion: df_m, ddyn, and (ADDED; rows summed in a fixed order) dlogits[M], dtemp[1] */
int mm_learned_fusion_bwd(const float* f0, const float* f1, const float* f2, const float* dyn,
                          const float* logits, const float* temperature, const float* dfused, float* df0,
                          float* df1, float* df2, float* ddyn, float* dlogits, float* dtemp, int B, int H,
                          int M, hipStream_t stream);
int mm_softmax2_concat_bwd(const float* dout, const float* a, const float* c, const float* pa,
                           const float* pc, float* da, float* dc, float* dpa, float* dpc, int B, int Ha,
                           int Hc, hipStream_t stream);
/* nn.CrossEntropyLoss(weight=class_weight) (_test_bridge.py:858; run_fmri_v11.py): loss_out[0] += loss; dlogits [B][C]
 * nullable.  Labels: the 64-bit label is compared with [0, C) before anything is indexed with it; a row whose label is
 * outside (-100, C, 2^32 + 1, ...) is dropped like torch's ignore_index: it adds nothing to the loss sum or the weight
 * sum and its gradient row is 0 (every row dropped: 0 / 0, as torch) */
int mm_weighted_ce(const float* logits, const void* target_i64, const float* class_weight, float* loss_out,
                   float* dlogits, int B, int C, hipStream_t stream);
/* FocalLoss (CrossModal_EEG_scr.ipynb cell 20; FlexibleTrainer(use_focal_loss=True), cell 23):
 * fl_b = alpha (1 - exp(-ce_b))^gamma ce_b.  loss_out[0] += scale * sum_b fl_b (zeroed by the caller),
 * per_sample[b] = fl_b (nullable), dlogits = d fl_b / d logits without the reduction's factor (nullable).
 * Labels as mm_weighted_ce: a row whose label is outside [0, C) is dropped - per_sample[b] = 0, a zero gradient row,
 * nothing added to the sum; `scale` stays the caller's */
int mm_focal_loss(const float* logits, const void* target_i64, float* loss_out, float* per_sample,
                  float* dlogits, int B, int C, float alpha, float gamma, float scale, hipStream_t stream);
/* HybridFusionModule gate + mix + conn boost (crossmodal_v4_enhancements.py:787-797) */
int mm_gate2_mix(const float* g, const float* erp, const float* pw, const float* conn, float* comb,
                 float* gate, int B, int H, float boost, hipStream_t stream);
int mm_gate2_mix_bwd(const float* dcomb, const float* g, const float* erp, const float* pw, float* derp,
                     float* dpw, float* dconn, float* dg, int B, int H, float boost, hipStream_t stream);
/* LabelSmoothingCrossEntropy (crossmodal_v4_enhancements.py:665-677): loss_out[0] += loss (zeroed by
 * the caller), dlogits = d loss / d logits (nullable); target is int64 class indices.  Labels as mm_weighted_ce: a row
 * whose label is outside [0, C) is dropped - it adds nothing, its gradient row is 0, the divisor stays B */
int mm_smoothed_ce(const float* logits, const void* target_i64, float* loss_out, float* dlogits, int B,
                   int C, float smoothing, hipStream_t stream);
/* Multi-scale STFT power front-end (extension a-X3; semantics = torch.stft(center=True,
 * pad_mode="reflect", periodic Hann) then |.|^2): x (B,C,T) fp32 -> channels-last
 * out[b][frame][ch_off + c*F + f], F = nfft/2+1, frames = T/hop+1, row width ch_total
 * (several scales write side by side into one activation tensor). */
int mm_stft_power(const float* x, void* out_bf16, float* out_f32, int B, int C, int T, int nfft, int hop,
                  int ch_off, int ch_total, hipStream_t stream);
/* normalize_modality (run_training_lite.py:48-51; applied per sample to the power features at :162):
 * out[b] = bf16((x[b] - mean(x[b])) / (std(x[b]) + eps)), population std (numpy ddof = 0), over all rows x ch_valid elements of
 * sample b; x / out [B][rows][ch_total] channels-last, channels >= ch_valid are written as zeros.
 * ws (nullable; MM_ZSCORE_WS_DOUBLES doubles per sample, 8-byte aligned): with it, big unpadded samples (ch_valid ==
 * ch_total, >= 65 536 elements) are dealt out over 32 workgroups each - per-chunk sums in double, added in chunk order by
 * every workgroup of the second launch (same bits every run); without it one workgroup per sample does it all. */
#define MM_ZSCORE_WS_DOUBLES 64
int mm_sample_zscore_bf16(const float* x, void* out_bf16, double* ws, int B, int rows, int ch_valid, int ch_total,
                          float eps, hipStream_t stream);
/* Backward of the STFT power front-end and of its z-score (gradient w.r.t. the RAW EEG: saliency / integrated
 * gradients on the config-#5 model, the protocol of bridge_utils.py:158-229 / eeg_xai_analysis.py on an end-to-end
 * path).  mm_sample_zscore_bwd: x = the fp32 spectra the forward z-scored, g_bf16 = gradient w.r.t. the z-scored
 * bf16 tensor (same [B][rows][ch_total] layout) -> dx fp32 (padding channels 0).  mm_stft_power_bwd: g_power fp32
 * [B][frames][ch_total] -> dx fp32 [B][C][T] is ADDED to (one launch per scale; zero it first).  Gathers, no atomics. */
int mm_sample_zscore_bwd(const float* x, const void* g_bf16, float* dx, int B, int rows, int ch_valid, int ch_total,
                         float eps, hipStream_t stream);
int mm_stft_power_bwd(const float* x, const float* g_power, float* dx, int B, int C, int T, int nfft, int hop,
                      int ch_off, int ch_total, hipStream_t stream);
int mm_mul_f32(const float* a, const float* b, float* out, int64_t n, hipStream_t stream);
/* Encoder tail (enhanced_models_v4.py:161-167, 186-191: mean over time -> output_proj = Linear -> GELU ->
 * Dropout).  mm_linear_fwd_meanpool is the last transformer block's linear2 (+ dropout + residual, fp32 rows
 * out_f32 (M, 128)) that also accumulates the mean over each group of rows_per_group rows (one EEG epoch's
 * tokens) into the ZEROED pool_out, an accumulator of (M / rows_per_group) x 128 64-bit elements (ONE replica:
 * 2 x that many floats).  mm_pooled_head_fwd applies the head to the pooled rows - fp32 `pooled`, or that
 * accumulator as `pooled_acc` (exactly one non-null) - in fp32 (W is the nn.Linear weight (N, D)); z_pre_bf16 / pooled_bf16 (nullable) are what the
 * backward and the weight-gradient GEMM need.  mm_pooled_head_bwd: dz = dout * dropout mask * act'(z) (bf16 copy
 * dz_bf16 for the weight gradient), d pooled = dz W, and dx[b][l][:] = d pooled / L for every token; dx_bf16
 * (nullable) = the same rows times the consumer's dropout mask (emit_drop_p, emit_seed; element index as in
 * mm_act_bwd). */
int mm_linear_fwd_meanpool(const void* x, const void* w, int M, int K, const float* bias, const float* residual,
                           float* out_f32, float drop_p, uint32_t seed, const uint32_t* seed_epoch, float* pool_out,
                           int rows_per_group, hipStream_t stream);
/* TemporalTransformerBlock forward (enhanced_models_v4.py:86-105): a sub-layer's closing Linear (attention
 * out_proj or linear2; width 128) + dropout + residual, fp32 rows out_f32 (M, 128), with the NEXT sub-layer's
 * pre-norm fused: ln_out_bf16 = LayerNorm(out rows; gamma, beta, eps) and ln_stat [M][2] = mean, rstd (nullable),
 * i.e. mm_conv1d_fwd followed by mm_layernorm_fwd without re-reading the rows. */
int mm_linear_fwd_ln(const void* x, const void* w, int M, int K, const float* bias, const float* residual,
                     float* out_f32, float drop_p, uint32_t seed, const uint32_t* seed_epoch, const float* ln_gamma,
                     const float* ln_beta, float ln_eps, void* ln_out_bf16, float* ln_stat, hipStream_t stream);
int mm_pooled_head_fwd(const float* pooled, const float* pooled_acc, const float* W, const float* bias, float* out, void* z_pre_bf16,
                       void* pooled_bf16, int B, int D, int N, int act, float drop_p, uint32_t seed,
                       const uint32_t* seed_epoch, hipStream_t stream);
int mm_pooled_head_bwd(const float* dout, const void* z_pre_bf16, const float* W, void* dz_bf16, float* dx,
                       void* dx_bf16, int B, int L, int D, int N, int act, float drop_p, uint32_t seed,
                       float emit_drop_p, uint32_t emit_seed, const uint32_t* seed_epoch, hipStream_t stream);
/* drop_path / DropPath (crossmodal_v4_enhancements.py:639-658): out[b][...] = x[b][...] * keep_b / (1 - p),
 * keep_b from the counter hash of (seed, b); calling it on the upstream gradient is the backward */
int mm_drop_path(const float* x, float* out, int64_t B, int64_t inner, float drop_p, uint32_t seed,
                 const uint32_t* seed_epoch, hipStream_t stream);
/* AdaptiveAvgPool1d(1) of the Lite encoders on bf16 [R][S][N] */
int mm_meanpool_bf16(const void* x, float* out, int R, int S, int N, hipStream_t stream);

/* ---- optimizer: clip_grad_norm_(max_norm) + AdamW.step() on one flat bucket
 * (run_training_lite.py:487-488; _test_bridge.py:784-786).  state (device, MM_OPT_STATE_FLOATS
 * = 8 + 1024 floats): [0] step count, [1] sum of squared grads of the last step, [2] lr,
 * [3] clip coefficient of the last step, [4] grad norm of the last step, [8..) per-block
 * partial sums written by mm_sumsq and added in a fixed order by mm_adamw_clip (no float
 * atomics: ranks holding the same all-reduced gradient stay bit-identical).
 * zero_grad != 0: g is cleared after use (the next step's zero_grad()); seed_epoch (nullable): the
 * device dropout-epoch word is incremented for the next step.
 * state[5]: the weight-average decay d of the last step, written by mm_adamw_clip_ema only; mm_adamw_clip never writes
 * state[5..8).
 *
 * The four mm_adamw_clip* entry points are instances of ONE update kernel body (and one finish kernel for state[0..5)),
 * so what they share they share bit for bit.
 *
 * mm_adamw_clip_ema: the same update (p, g, m, v and state[0..5) get mm_adamw_clip's bits)
 * plus an exponential moving average of the weights in `ema` (n floats, device, not NULL), in the same launch:
 *     ema[i] = fma(1 - d, p_new[i] - ema[i], ema[i])
 * with 1 - d formed in fp32, the difference rounded to fp32, then one fused multiply-add - so ema[i] keeps its bits
 * wherever it already equals p_new[i].  d comes from the step count on the device (the launch can live in a hipGraph):
 * with t = state[0] + 1, the count after this step, d = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay.
 * ema_decay must lie in [0, 1); a NULL ema or a decay outside the range is an argument error, nothing is launched.
 * No float atomics: ranks that hold the same parameters keep bit-identical averages without a collective.
 *
 * mm_adamw_clip_groups / mm_adamw_clip_groups_ema: the same step with parameter groups.  The bucket is cut into n_seg
 * (1 .. MM_OPT_MAX_SEGMENTS) contiguous segments by a table in DEVICE memory, read at launch (so a launch captured in a
 * hipGraph serves any later change of the table's values): seg_end (int64, strictly increasing, seg_end[n_seg-1] == n;
 * segment s = [seg_end[s-1], seg_end[s])), seg_lr_mult and seg_wd (fp32, n_seg values each; what lies behind them in
 * the arrays is never read).  The caller builds and validates the contents; an element past the last end takes the
 * last segment, and no element or table content forms an address outside the table.  An element of segment s is
 * updated with lr_s = fl32(state[2] * seg_lr_mult[s]) and weight decay seg_wd[s]: its p, m, v, g (and ema) bits are
 * those mm_adamw_clip (mm_adamw_clip_ema) writes on the whole bucket when called with state[2] = lr_s and
 * weight_decay = seg_wd[s] - it is the same body, the two scalars looked up per element - and state[0..5) and state[5]
 * are written by the same finish kernel.  The step count, the norm (over
 * the WHOLE bucket: clip_grad_norm_ over all groups), the clip coefficient, zero_grad and the average are unchanged.
 * A multiplier of 0 leaves p bit-unchanged while m and v move (torch's lr = 0 group).  Two launches, as the plain step. */
#define MM_OPT_STATE_FLOATS 1032
#define MM_OPT_MAX_SEGMENTS 1024
int mm_sumsq(const float* g, float* state, int64_t n, hipStream_t stream);
int mm_adamw_clip(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1,
                  float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                  int zero_grad, uint32_t* seed_epoch, hipStream_t stream);
int mm_adamw_clip_ema(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1,
                      float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                      int zero_grad, uint32_t* seed_epoch, float* ema, float ema_decay, int ema_warmup,
                      hipStream_t stream);
int mm_adamw_clip_groups(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1,
                         float beta2, float eps, float max_norm, float grad_scale, int zero_grad,
                         uint32_t* seed_epoch, const int64_t* seg_end, const float* seg_lr_mult,
                         const float* seg_wd, int n_seg, hipStream_t stream);
int mm_adamw_clip_groups_ema(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1,
                             float beta2, float eps, float max_norm, float grad_scale, int zero_grad,
                             uint32_t* seed_epoch, const int64_t* seg_end, const float* seg_lr_mult,
                             const float* seg_wd, int n_seg, float* ema, float ema_decay, int ema_warmup,
                             hipStream_t stream);

/* ---- attribution (EEG_CODE/eeg_xai_analysis.py:88-236: GradientSaliency, IntegratedGradients) ---------------
 * The reference walks its n_steps interpolation points one forward/backward at a time with a numpy round trip
 * each; here `steps` of them are one batch.  All tensors fp32, contiguous; `rows` samples of `inner` values.
 * `base` / `base_rows`: NULL / 0 = the zero baseline, 1 = one sample broadcast over the batch (the 'mean'
 * baseline), rows = one baseline per sample.
 * mm_xai_interp: out[s - s0][r][i] = base[r][i] + alpha_s * (x[r][i] - base[r][i]) for s in [s0, s0 + steps),
 * alpha_s = np.linspace(0, 1, n_steps)[s] rounded to fp32 (n_steps == 1: alpha = 0); subtraction, product and sum
 * are each rounded on their own, so the bits are torch's `base + alpha * (x - base)` (:196-198).
 * mm_xai_accum: acc[i] = ((acc[i] + grad[0][i]) + grad[1][i]) + ... over `steps` slices of n values, in that order
 * (the per-step gradient list of :217-225 without leaving the device; the order makes the sum independent of how
 * the steps were cut into chunks).
 * mm_xai_finish: attr[b][c][t] from x, base and acc (all (B, C, T)) -
 *   mode 0  |(x - base) * (acc / n_steps)|   integrated gradients (:224-229; base NULL = the connectivity rule :233-234)
 *   mode 1  |acc|                            vanilla gradient (:128-129)
 *   mode 2  |acc| * |x|                      gradient x input (:145-146)
 * and, when `chan` (B, C) is not NULL, chan[b][c] = mean_t attr[b][c][t], added in a fixed order (what
 * ChannelImportanceExtractor.extract_channel_importance averages first, :422).
 * mm_xai_pair_score: z (B, 2N) = [ze | zf] L2-normalised embeddings -> score[b] = ze_b . zf_b, the matching score
 * of pair b, and (nullable) seed (B, 2N) = [zf | ze] = d score / d z, the gradient a backward starts from. */
int mm_xai_interp(const float* x, const float* base, int base_rows, float* out, int n_steps, int s0, int steps,
                  int64_t rows, int64_t inner, hipStream_t stream);
int mm_xai_accum(const float* grad, float* acc, int steps, int64_t n, hipStream_t stream);
int mm_xai_finish(const float* x, const float* base, int base_rows, const float* acc, float* attr, float* chan,
                  int B, int C, int64_t T, int n_steps, int mode, hipStream_t stream);
int mm_xai_pair_score(const float* z, float* score, float* seed, int B, int N, hipStream_t stream);

/* ---- perturbation attribution (EEG_CODE/CrossModal_EEG_scr.ipynb, InterpretabilityAnalyzer.compute_channel_importance:
 * one clone, one zeroed channel, one forward and one .item() per channel and batch) ---------------------------------
 * All the perturbed copies of a batch are rows of one big batch instead.  fp32, contiguous.  A sample is cut into U
 * units, the things that are knocked out together:
 *   kind 0  rows     sample (n0, n1) = (C, T)                 unit of an element = c              U = n0
 *   kind 1  windows  sample (n0, n1) = (C, T), size = w       unit = t / w                        U = ceil(n1 / w)
 *   kind 2  blocks   sample (n0, n1, n2, n3) = (Cv, D, H, W)  unit = ((d/s) gh + h/s) gw + w/s    U = gd gh gw, g* = ceil(* / s)
 * (the last window / the edge blocks may be ragged; all Cv channels of a block go together; n2 = n3 = 1 for kinds 0
 * and 1; a tabular row (F,) is kind 1 with n0 = 1).  The batch must stay below 2^31 elements.
 * mm_perturb_expand: masks [M][U] int, 1 = keep, 0 = replace.  For j in [0, m):
 *   out[j * B + b][i] = masks[m0 + j][unit(i)] ? x[b][i] : base[b][i]        (mask-major rows, as mm_xai_interp's steps)
 * `base` / `base_rows` as for mm_xai_interp: NULL / 0 = zeros, 1 = one sample for all, B = one per sample.  No
 * arithmetic: every output is a copy of an input's bits or +0.0f.  U must be the unit count of the geometry (checked),
 * so a mask row is never read past its end.  m <= 65535.
 * mm_perturb_pair_scores: v[j][b] = z[j * B + b] . z_other[b] over N values, one wave per row in a fixed order: the
 * matching score of every perturbed row against the OTHER modality's embedding, which is encoded once and not per mask.
 * mm_perturb_shapley: permutation-sampled Shapley values.  v [P][U - 1][B]: v[q][k - 1] = the score of the coalition of
 * the first k units of permutation q, k = 1 .. U - 1; pos [P][U] in 1 .. U = the place of unit u in permutation q.  With
 * v(q, 0) = v_empty and v(q, U) = v_full (both (B,)):
 *   phi[b][u] = (1 / P) sum_q ( v(q, pos[q][u]) - v(q, pos[q][u] - 1) )
 * the sum over q in ascending order in fp64, rounded to fp32 once.  U == 1: v may be NULL.  A place outside 1 .. U
 * yields NaN for that unit. */
int mm_perturb_expand(const float* x, const float* base, int base_rows, const int* masks, float* out, int B, int kind,
                      int n0, int n1, int n2, int n3, int size, int U, int m0, int m, hipStream_t stream);
int mm_perturb_pair_scores(const float* z, const float* z_other, float* v, int B, int m, int N, hipStream_t stream);
int mm_perturb_shapley(const float* v, const float* v_empty, const float* v_full, const int* pos, float* phi, int B, int U,
                       int P, hipStream_t stream);

/* ---- GATv2 graph attention over one static graph (EEG_CODE/enhanced_models_v4.py:292-413: the layer of
 * GNNConnectivityEncoder; Brody et al., "How Attentive are Graph Attention Networks?") -------------------------
 * Every sample of the batch shares the graph; a layer is one launch, a workgroup per (sample, head).
 *   xl, xr   [B*N][ld] fp32, row stride ld >= H*C: the two linear images of the node features, head h in columns
 *            [h*C, (h+1)*C).  (The halves of ONE (B*N, 2*H*C) linear with W_l | W_r stacked: xr = xl + H*C, ld = 2*H*C.)
 *   att [H][C], bias [H*C] (nullable)
 *   graph    CSR by TARGET: rowptr [N+1], col [E] = source of each edge, int32 on the device, every node with at
 *            least its self-loop (E >= N); for the backward also the CSC view: colptr [N+1], row [E] = target,
 *            perm [E] = position of that edge in CSR order, sources ascending, CSR order within a source.
 *   e[i<-j] = sum_c att[h][c] * leaky_relu(xl[j][h][c] + xr[i][h][c], slope);  alpha = softmax over the edges of i;
 *   out[b][i][h*C + c] = act(sum_j alpha * keep / (1 - drop_p) * xl[j][h][c] + bias[h*C + c])      [B][N][H*C]
 *   keep: the counter-hash mask at element (b*H + h)*E + e, e the edge's CSR position (no renormalisation).
 *   alpha [B][H][E] (required): the softmax before dropout, what the backward reads; pre [B][N][H*C] (nullable): the
 *   value before `act` (the backward of an activation epilogue needs it).
 * mm_gatv2_bwd: dxl, dxr [B*N][ld] (written), datt [H][C] and dbias [H*C] (nullable, ACCUMULATED into) from dout
 *   [B][N][H*C]; same mask as the forward.  Workspaces (content opaque): ds_ws [B][H][E], part_ws [B][2][H*C], and
 *   dz_ws [B][N][H*C] when act != 0 (pre is then required too).  Sums run in a fixed order (targets of a source in
 *   CSR order, nodes, then batch): no atomics, two runs give the same bits.
 * Supported: 1 <= N <= 128, C in {16, 32, 64}, H*C <= 256, B*H*E < 2^32; anything else (or a null pointer) is
 * refused with MM_ERR_ARG before a launch. */
int mm_gatv2_fwd(const float* xl, const float* xr, int ld, const float* att, const float* bias, const int* rowptr,
                 const int* col, float* out, float* pre, float* alpha, int B, int N, int H, int C, int E,
                 float slope, int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);
int mm_gatv2_bwd(const float* dout, const float* pre, const float* xl, const float* xr, int ld, const float* att,
                 const float* alpha, const int* rowptr, const int* col, const int* colptr, const int* row,
                 const int* perm, float* dxl, float* dxr, float* datt, float* dbias, float* ds_ws, float* dz_ws,
                 float* part_ws, int B, int N, int H, int C, int E, float slope, int act, float drop_p,
                 uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);

/* ---- GATv2 with edge features (torch_geometric's GATv2Conv(edge_dim = D)): the raw attributes enter the score only,
 *   e[i<-j] = sum_c att[h][c] * leaky_relu((xl[j][h][c] + xr[i][h][c]) + sum_d w_edge[h*C + c][d] * edge_attr[e][d], slope)
 * everything else as mm_gatv2_fwd / mm_gatv2_bwd (w_edge = 0 gives their bits).
 *   w_edge     [H*C][D] = lin_edge.weight, 1 <= D <= 8
 *   edge_attr  [B][E][D] (ea_batched != 0) or [E][D] shared by the batch, in CSR order with the self-loop rows filled:
 *              the output of mm_gatv2_edge_pack.  The projection runs inside the score loop; no [B][E][H*C] image.
 * mm_gatv2_edge_bwd adds: dw_edge [H*C][D] (nullable, ACCUMULATED into, batch order), dedge_attr [B | 1][E][D]
 *   (nullable, written: the per-head partials added in head order, for shared attributes over the batch too).
 *   Workspaces: wpart_ws [B][H*C][D]; epart_ws [B][H][E][D], required when dedge_attr is given.  No atomics.
 * mm_gatv2_edge_pack: listed [Bo][El][D] (rows aligned with the listed edge_index) -> csr [Bo][E][D].  eid [E] = listed
 *   edge of each CSR position, -1 for an appended self-loop; indeg [N] = in-degree without loops.  The loop of node i
 *   gets the mean of the listed attributes into i (0 without any) when fill_mean != 0, else fill_value.
 * mm_gatv2_edge_pack_bwd: dlisted [Bo][El][D] (written) = dcsr[pos] + dcsr[loop of tgt] / indeg[tgt] (the second term
 *   only when fill_mean != 0); pos [El] = CSR position of a listed edge, -1 for a dropped self-loop (gradient 0),
 *   tgt [El] = its target. */
int mm_gatv2_edge_fwd(const float* xl, const float* xr, int ld, const float* att, const float* bias,
                      const float* w_edge, const float* edge_attr, int ea_batched, const int* rowptr, const int* col,
                      float* out, float* pre, float* alpha, int B, int N, int H, int C, int E, int D, float slope,
                      int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);
int mm_gatv2_edge_bwd(const float* dout, const float* pre, const float* xl, const float* xr, int ld, const float* att,
                      const float* w_edge, const float* edge_attr, int ea_batched, const float* alpha,
                      const int* rowptr, const int* col, const int* colptr, const int* row, const int* perm,
                      float* dxl, float* dxr, float* datt, float* dbias, float* dw_edge, float* dedge_attr,
                      float* ds_ws, float* dz_ws, float* part_ws, float* wpart_ws, float* epart_ws, int B, int N,
                      int H, int C, int E, int D, float slope, int act, float drop_p, uint32_t seed,
                      const uint32_t* seed_epoch, hipStream_t stream);
int mm_gatv2_edge_pack(const float* listed, const int* eid, const int* rowptr, const int* indeg, float* csr, int Bo,
                       int N, int El, int E, int D, int fill_mean, float fill_value, hipStream_t stream);
int mm_gatv2_edge_pack_bwd(const float* dcsr, const int* pos, const int* tgt, const int* rowptr, const int* indeg,
                           float* dlisted, int Bo, int N, int El, int E, int D, int fill_mean, hipStream_t stream);

/* ---- projection + pooling over time: the tails of the EEG notebook's single-modality baselines (PWOnlyNet, ERPOnlyNet,
 * EEG_CODE/CrossModal_EEG_scr.ipynb), csrc/timepool.hip.  x = the (B, L, K) output of the third conv block, w (P, K) /
 * bias (P) the 1 x 1 convolution; the projected (B, L, P) tensor is never written.  Sizes served: K = 128, P a multiple
 * of 16 up to 512, 1 <= L <= 64 * 65535, B >= 1, B*L*P < 2^32, bins in 1 .. 8; anything else is MM_ERR_UNSUPPORTED
 * before a launch.
 * No floating-point atomics: the same bits on every run.  dw / dbias are nullable and ACCUMULATED into (one owner per
 * element, batch order), as mm_small_linear_bwd's; dx is nullable and WRITTEN, every row, zeros included.
 *
 * max tail:  y[b][t][n] = (sum_k x[b][t][k] w[n][k] + bias[n]) * dropout_scale(mm_eff_seed(seed, epoch), (b L + t) P + n)
 *            pooled[b][n] = max_t y, arg[b][n] = the SMALLEST t that attains it (a dropped element is an exact 0 and
 *            competes as such; NaN wins).  x, w bf16 (w = the forward image of mm_prep_conv_weight, taps 1), bf16 MFMA
 *            with fp32 accumulation.
 *   bwd:     g[b][n] = dpooled[b][n] * keep-scale at (b, arg[b][n], n);  dx[b][t][:] = sum_{n: arg[b][n] = t} g[b][n] w[n][:]
 *            (bf16, n ascending);  dw[n][:] += sum_b g[b][n] x[b][arg[b][n]][:];  dbias[n] += sum_b g[b][n].
 * avg tail:  xbin[b][i][:] = mean of x[b][t][:] over t in [floor(i L / bins), ceil((i + 1) L / bins))  (AdaptiveAvgPool1d:
 *            the bins overlap when bins does not divide L);  pooled[b][p bins + i] = xbin[b][i][:] . w[p][:] + bias[p]
 *            = Flatten of AdaptiveAvgPool1d(bins)(projection) - the projection is affine, so pooling first is the same
 *            function.  fp32 throughout, sums in ascending order.
 *   bwd:     u[b][i][:] = (sum_p dpooled[b][p bins + i] w[p][:]) / len_i;  dx[b][t][:] = sum_{i holding t} u[b][i][:];
 *            dw[p][:] += sum_b sum_i dpooled[b][p bins + i] xbin[b][i][:];  dbias[p] += sum_{b,i} dpooled[b][p bins + i]. */
int mm_timepool_max_fwd(const void* x_bf16, const void* w_bf16, const float* bias, float* pooled, int* arg, int B, int L,
                        int K, int P, float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t stream);
int mm_timepool_max_bwd(const float* dpooled, const int* arg, const void* x_bf16, const void* w_bf16, void* dx_bf16,
                        float* dw, float* dbias, int B, int L, int K, int P, float drop_p, uint32_t seed,
                        const uint32_t* seed_epoch, hipStream_t stream);
int mm_timepool_avg_fwd(const float* x_f32, const float* w, const float* bias, float* xbin, float* pooled, int B, int L,
                        int K, int P, int bins, hipStream_t stream);
int mm_timepool_avg_bwd(const float* dpooled, const float* xbin, const float* w, float* dx_f32, float* dw, float* dbias,
                        int B, int L, int K, int P, int bins, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMEEG_HIP_H */
