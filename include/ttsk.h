/*
 * ttsk.h — C ABI of libttsk_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the tts-king hot path.
 *
 * The reference (diff7/tts-king) is pure Python/PyTorch and has no FFI of its own; its hot
 * path bottoms out in ATen op calls.  Every entry point below replaces one (or a fused group) of those
 * op sites; the site is cited as `reference: <file>:<lines>`.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - Plain C: raw device pointers, sizes, a hipStream_t passed as `void*`.  No torch types.
 *   - The caller owns every buffer (inputs, outputs, workspaces).  The library allocates nothing, keeps no
 *     mutable global state, never synchronises: all work is enqueued on `stream` and is graph-capturable.
 *   - Return value: 0 on success, negative TTSK_E* on a rejected call (nothing was launched);
 *     `ttsk_last_error()` returns a thread-local message.
 *   - bf16 = raw uint16 storage (round-to-nearest-even from fp32); activations are channels-last
 *     [row][channel] with row = batch * seg_len + position.
 */
#ifndef TTSK_H
#define TTSK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTSK_VERSION 1

#define TTSK_OK 0
#define TTSK_EINVAL (-1)
#define TTSK_ELAUNCH (-2)

int ttsk_version(void);
const char* ttsk_last_error(void);

/* ------------------------------------------------------------------------------------------------ GEMM
 * One tiled MFMA kernel family behind every contraction on the path:
 *   Linear fwd / dX / dW              reference: fs_two/transformer/SubLayers.py:41-63, fastspeech2.py:102
 *   attention Q·Kᵀ, P·V and backward   reference: fs_two/transformer/Modules.py:14-24
 *   Conv1d as implicit GEMM (fwd/dX/dW) reference: SubLayers.py:96 (k=9,1), model/modules.py:337-355 (k=3),
 *                                                  transformer/Layers.py:59-67 (k=5), hifi/models.py:88-95,186,198
 *   ConvTranspose1d, polyphase          reference: hifi/models.py:166-176,189
 *
 *   C[z][m][n] = epilogue( alpha * sum_{tap} sum_{k} A[z][m (+shift_tap)][tap? k] * B[z][n][tap*btap + k] )
 */
enum {
  TTSK_GEMM_A_TR      = 1 << 0,  /* A stored [k][m] (contraction index is the row)                        */
  TTSK_GEMM_B_TR      = 1 << 1,  /* B stored [k][n]                                                        */
  TTSK_GEMM_C_F32     = 1 << 2,  /* C is fp32 (default bf16)                                               */
  TTSK_GEMM_RELU      = 1 << 3,  /* v = max(v, 0) after bias/residual                                      */
  TTSK_GEMM_ADD_R     = 1 << 4,  /* v += R[m][n]                                                           */
  TTSK_GEMM_R_F32     = 1 << 5,  /* R is fp32 (default bf16)                                               */
  TTSK_GEMM_MASK_G    = 1 << 6,  /* v = (G[m][n] > 0) ? v : 0   (ReLU backward, G = saved activation bf16) */
  TTSK_GEMM_LRELU_IN  = 1 << 7,  /* A := leaky_relu(A, in_slope) while staging (conv-A mode, HiFi-GAN)     */
  TTSK_GEMM_TANH      = 1 << 8,  /* v = tanh(v) last                                                       */
  TTSK_GEMM_ACCUM_C   = 1 << 9,  /* C_F32 only: C += v  (plain read-modify-write, one writer per element)   */
  TTSK_GEMM_LRELU_OUT = 1 << 10, /* v = leaky_relu(v, out_slope) before the store                           */
  TTSK_GEMM_F16       = 1 << 11, /* 16-bit operands (A, B, C, C2, R, G) are IEEE fp16 instead of bf16           */
  TTSK_GEMM_C2_LRELU  = 1 << 12, /* the second output is leaky_relu(v, out_slope) (C keeps v): the next conv's   */
                                 /* activation is produced by this conv's epilogue instead of its operand staging */
  TTSK_GEMM_DEFER_REDUCE = 1 << 13,/* split-K: write the partial slabs only; the caller sums many GEMMs' slabs later */
                                 /* with ONE ttsk_gemm_reduce_batch launch (weight gradients: needed only by Adam)  */
  TTSK_GEMM_RAW_SLABS = 1 << 14    /* the fp32 partial tiles [splits][nz][M][N] go to `workspace` for ANY splits >= 1, no  */
                                 /* epilogue and no reducer launch: the consumer sums them (ttsk_layernorm_bwd_slabs   */
                                 /* adds the slabs and the residual while it reads its rows); C is not written         */
};

typedef struct ttsk_gemm_desc {
  const void* A;      /* bf16 */
  const void* B;      /* bf16 */
  void* C;            /* bf16 or fp32 */
  void* C2;           /* optional second output, bf16, same ldc/strides as C (NULL = none) */
  const float* bias;  /* [N] or NULL */
  const void* R;      /* residual, layout of C with ldr; bf16 or fp32 */
  const void* G;      /* ReLU gate, bf16, layout of C with ldg */
  int32_t M, N, K;    /* output M x N, K = contraction length per tap */
  int32_t lda, ldb, ldc, ldr, ldg;
  int32_t flags;
  float alpha;
  float in_slope, out_slope;
  /* batch: z = z1 * nz2 + z2 */
  int32_t nz1, nz2;
  int64_t sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2;
  /* conv-A mode (taps > 0; A not transposed): rows of A and C are (segment, position) pairs, row = s*seg_len + t.
   * Tap j reads A row (t + tap_shift0 + j*tap_dshift) of the same segment, zero outside [0, seg_len);
   * B element k of tap j sits at column j*b_tap_stride + k (B_TR: row offset j*b_tap_stride rows... see gemm.hip) */
  int32_t taps, seg_len, tap_shift0, tap_dshift;
  int64_t b_tap_stride;
  /* B_TR row shift per batch index z2 (conv dW): B row (t + bshift0 + z2*bdshift) within a segment of bseg_len rows */
  int32_t bseg_len, bshift0, bdshift;
  /* output row remap (polyphase ConvTranspose1d): C row for A row (s, t) is s*out_seg + t*out_mul + out_add,
   * skipped when outside [0, out_seg).  out_mul == 0 means identity. */
  int32_t out_seg, out_mul, out_add;
  int32_t out_add_dz;   /* out_add += z2 * out_add_dz: several polyphase phases batched into one launch */
  /* split-K: `splits` > 1 cuts the K chunks into `splits` ranges whose fp32 partial tiles go to `workspace`
   * ([splits][nz][M][N] floats); a second kernel sums them in fixed order and applies the epilogue (deterministic). */
  int32_t splits;      /* 0 = let the library choose (ttsk_gemm_plan) */
  void* workspace;
  int64_t workspace_bytes;
  /* tile configuration: 0 = let the library choose, 1 = 128x128x64 (4 waves, register staging; required by LRELU_IN),
   * 2 = 256x128x64 (8 waves, 3-stage LDS-DMA ring), 3 = 64x128x64 (4 waves, register staging, A untransposed: outputs
   * with few columns get enough workgroups to fill the chip without split-K) */
  int32_t kernel;
  /* batched problems with one bias vector per z1 (the three VariancePredictors of a training step as one launch):
   * bias of batch z1 = bias + z1 * s_bias1 (floats); 0 = one bias for all */
  int64_t s_bias1;
} ttsk_gemm_desc;

int ttsk_gemm(const ttsk_gemm_desc* d, void* stream);
/* Deferred split-K reduction.  A GEMM launched with TTSK_GEMM_DEFER_REDUCE (fp32 C, no epilogue beyond alpha / ACCUM_C,
 * nz1 == 1) leaves `splits` slabs [split][nz2][M][N] in its workspace; ttsk_gemm_reduce_batch sums the slabs of `n` such
 * GEMMs in fixed order (deterministic) into their C (C[z2*sC2 + m*ldc + n] (+)= alpha * sum) with one kernel per 64 items. */
typedef struct ttsk_reduce_item {
  const float* ws;
  float* C;
  int32_t M, N, ldc, nz, splits, accumulate;
  int64_t sC2;
  float alpha;
} ttsk_reduce_item;
int ttsk_gemm_reduce_batch(const ttsk_reduce_item* items, int n, void* stream);

/* Grouped launch of n problems with the same operand layout (A_TR / B_TR / F16 flags) and the same tile configuration
 * (desc.kernel: 1 = 128x128, also the default; 2 = 256x128) as ONE
 * grid — for the many small contractions nothing waits for individually (the weight-gradient GEMMs of a backward pass:
 * 32-256 workgroups each).  group_build validates and plans every descriptor (split-K workspaces as for ttsk_gemm) and
 * writes a table of ttsk_gemm_group_table_bytes(n) bytes into HOST memory (pageable is fine); group_launch copies it into
 * the caller's 16-byte aligned device buffer of the same size through kernel arguments (hipGraph-capturable, no pinned
 * staging), runs the grid and then the reducers of split problems that do not carry TTSK_GEMM_DEFER_REDUCE.  Results are
 * identical to n ttsk_gemm calls with the same kernel / splits. */
int64_t ttsk_gemm_group_table_bytes(int n);
int ttsk_gemm_group_build(const ttsk_gemm_desc* descs, int n, void* host_table, int32_t* total_wgs);
int ttsk_gemm_group_launch(const void* host_table, void* dev_table, void* stream);
/* The same with the grid capped at max_wgs workgroups (0 = no cap; honoured by the 256x128 configuration, kernel = 2): each
 * workgroup walks the table's tiles in steps of the grid size.  A grid of fewer workgroups than CUs (that configuration holds one
 * per CU) leaves the remaining CUs to kernels of a concurrent stream: the FS2 backward runs its weight-gradient group beside the
 * encoder-side dX chain this way. */
int ttsk_gemm_group_launch_capped(const void* host_table, void* dev_table, int max_wgs, void* stream);
/* ttsk_gemm_group_launch_capped in two parts: the table upload (kernel-argument launches; a no-op for an inline table) and the
 * grouped launch that expects the table in dev_table.  The upload may go on another stream, ordered before the launch by the caller,
 * so that it does not sit between two grouped launches on the same stream. */
int ttsk_gemm_group_upload(const void* host_table, void* dev_table, void* stream);
int ttsk_gemm_group_launch_uploaded(const void* host_table, void* dev_table, int max_wgs, void* stream);

/* The FFT block's first position-wise conv, forward: out = [relu](Conv1d(256 -> Cout, k)(x) + bias), 'same' zero padding per
 * utterance.  reference: fs_two/transformer/SubLayers.py:93-101 (w_1 + relu).  x [B*S][256] bf16 (row = utterance*S + frame), w the
 * tap-major bf16 weight (Cout, k, 256) as ttsk_gemm's conv takes it, out [B*S][Cout] bf16.  A window kernel (activation window of
 * 112 frames in LDS, weights L2 -> registers, no barrier in the tap loop) for Cin = 256, Cout % 256 == 0, odd k <= 9; same result
 * as the implicit-GEMM conv up to the order of the fp32 accumulation. */
int ttsk_ffn_conv_supported(int Cin, int Cout, int K);
int ttsk_ffn_conv_fwd(const void* x_bf16, const void* w_bf16, const float* bias, void* out_bf16, int B, int S, int Cin, int Cout, int K,
                      int relu, int packed, void* stream);
/* packed = 1: w is the fragment-major repack [k][8][Cout/16][64][8] written by ttsk_ffn_pack_weight from the tap-major weight (a
 * wave's fragment is then 1 KiB contiguous instead of 16 rows x 64 B). */
int ttsk_ffn_pack_weight(const void* w_bf16, void* packed_bf16, int Cout, int K, void* stream);
int ttsk_ffn_pack_weight_batch(const void* const* w_bf16, void* const* packed_bf16, int n /* <= 16 */, int Cout, int K, void* stream);
/* The same window kernel for Cin = 256 or 512 (the PostNet's Conv1d(512 -> 512, k = 5), fs_two/transformer/Layers.py:85-129): out =
 * [relu](conv(x) + bias), bias may be NULL, out bf16 or (out_f32 = 1, Cin = 512 only: the PostNet keeps its conv outputs in fp32 for
 * BatchNorm) fp32.  The weights are always the fragment-major pack written by ttsk_win_conv_pack_batch from the tap-major storage
 * (Cs, K, Ds): transpose = 0 packs the conv's own weights (Cout = Cs, Cin = Ds); transpose = 1 packs the weights of the conv's INPUT
 * GRADIENT seen as a forward conv on dy with flipped taps (Cout = Ds, Cin = Cs), so that ttsk_win_conv(dy, that pack) = dx. */
typedef struct ttsk_pack_item {
  const void* src;     /* tap-major bf16 weight (Cs, K, Ds) */
  void* dst;           /* fragment-major pack, Cs*K*Ds elements */
  int32_t Cs, K, Ds, transpose;
} ttsk_pack_item;
int ttsk_win_conv_supported(int Cin, int Cout, int K);
/* up to 48 packs of any shapes from a HOST item list (handed over through the kernel's arguments: capturable), one launch */
int ttsk_win_conv_pack_items(const ttsk_pack_item* items, int n, void* stream);
/* the same from an item table that already lives in DEVICE memory (8-byte aligned), any n: what a model with fixed weight and pack
 * addresses calls after every optimizer step (one launch, no upload) */
int ttsk_win_conv_pack_table(const ttsk_pack_item* dev_items, int n, void* stream);
int ttsk_win_conv_pack_batch(const void* const* w_bf16, void* const* packed_bf16, int n /* <= 16 */, int Cs, int K, int Ds, int transpose,
                             void* stream);
/* An input gradient whose contraction is wide (w_1: 1024 channels x 9 taps; q|k|v: 768), as nsplit window convs over 256-channel slices
 * of x [B*S][nsplit*256] in ONE launch: w_packed is the whole transposed pack (Cout, K, nsplit*256), slice sp takes its k-steps of every
 * tap and writes the fp32 slab slabs + sp*B*S*Cout — the raw split-K slabs that ttsk_layernorm_bwd_slabs sums (splits = nsplit,
 * stride = B*S*Cout). */
int ttsk_win_conv_split(const void* x_bf16, const void* w_packed, float* slabs, int nsplit, int B, int S, int Cin_total, int Cout, int K,
                        void* stream);
/* gate_bf16 [B*S][Cout] (may be NULL; bf16 output only): out = gate > 0 ? out : 0 — the ReLU backward of SubLayers.py:96 folded into
 * the w_2 input-gradient conv. */
/* delta_out [B*(Cout/128)][S] with delta_o32 [B*S][Cout] fp32 (both may be NULL; bf16 output, Cout = heads*128): the attention
 * backward's delta = rowsum over a head's 128 columns of out (as stored) * delta_o32, written while the rows are stored — out is then
 * the dO of ttsk_flash_attention_bwd(delta_ready = 1). */
int ttsk_win_conv(const void* x_bf16, const void* w_packed, const float* bias /* may be NULL */, const void* gate_bf16 /* may be NULL */,
                  const float* delta_o32 /* may be NULL */, float* delta_out /* may be NULL */, void* out, int out_f32, int B, int S, int Cin,
                  int Cout, int K, int relu, void* stream);
/* ttsk_win_conv (Cin = 512, fp32 output, no gate / delta) whose output's BatchNorm statistics partials come out of the same kernel:
 * stats[ttsk_win_conv_stats_rows(B, S)][2*Cout] = per-channel sum | sum of squares per (utterance, 64-frame tile) over the rows that
 * exist (t < S, t < frame_limit[0] when given) — the `partials` of ttsk_bn_train_apply, so the PostNet's 512 -> 512 layers need no
 * ttsk_bn_stats_slab launch (reference: Layers.py:133-143, Conv1d -> BatchNorm1d). */
int ttsk_win_conv_stats_rows(int B, int S);
/* Round 5: the PostNet's ends on the same kernel (reference: Layers.py:85-129, convolutions 0 and 4 = Conv1d(80 -> 512, k 5) and
 * Conv1d(512 -> 80, k 5); their input gradients are the mirrored shapes on transposed packs).  Cin = 80: rows of 80 channels, the
 * window and the pack zero-padded to three 32-channel k-steps (ttsk_win_conv_pack_* pads such a pack itself); Cout = 80: five waves
 * of 16 channels.  ttsk_win_conv / _stats / _bnb accept both.  ttsk_win_conv_resid: bf16 output = conv + resid_f32 [B*S][Cout], the
 * fp32 sum of the accumulators and the residual rounded ONCE (round 6: the residual joins the accumulators before the staging tile is
 * packed; round 5 added it to the tile's bf16 values and rounded twice) — conv 0's input gradient + the mel terms' own gradient (fastspeech2.py:104, postnet(output) + output). */
int ttsk_win_conv_resid(const void* x_bf16, const void* w_packed, const float* resid_f32, void* out_bf16, int B, int S, int Cin, int Cout,
                        int K, void* stream);
/* ttsk_win_conv with fp32 output and a bf16 copy of the same rows (round 5: mel_linear, fastspeech2.py:102, Linear(256 -> 80) as a k = 1
 * conv on the five-wave instance: the fp32 mel is what the loss reads and what the PostNet's output is added to, the copy is the PostNet's
 * input).  Shapes as ttsk_win_conv plus (Cin 256, Cout 80). */
int ttsk_win_conv_dual(const void* x_bf16, const void* w_packed, const float* bias, float* out_f32, void* out_bf16, int B, int S, int Cin,
                       int Cout, int K, void* stream);
int ttsk_win_conv_stats(const void* x_bf16, const void* w_packed, const float* bias, float* out_f32, float* stats,
                        const int32_t* frame_limit, int B, int S, int Cin, int Cout, int K, void* stream);
/* ttsk_win_conv (Cin = 512, bf16 output: the input gradient of a PostNet 512 -> 512 conv, run on the transposed pack) that also emits
 * the BatchNorm-BACKWARD statistics partials of the layer below — the layer whose upstream gradient `out` is (Layers.py:133-143
 * backwards: conv_i's input gradient is dL/d(dropout(tanh(BN_{i-1}(yc_{i-1}))))): stats[ttsk_win_conv_stats_rows(B, S)][2*Cout] =
 * per-channel sum of dy | sum of dy * xhat per (utterance, 64-frame tile) over the rows that exist, dy = out * keep / (1-p) * (1 -
 * tanh^2(gamma * xhat + beta)) (use_tanh), xhat = (bn_x - mean) * rstd — the `partials` of ttsk_bn_bwd_apply_slab, so that layer needs no
 * ttsk_bn_bwd_stats_slab launch.  keep: ttsk_bn_train_apply's keep bits (required when p > 0). */
int ttsk_win_conv_bnb(const void* x_bf16, const void* w_packed, void* out_bf16, float* stats, const float* bn_x_f32, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, const uint8_t* keep, float p, int use_tanh,
                      const int32_t* frame_limit, int B, int S, int Cin, int Cout, int K, void* stream);
/* HiFi-GAN's stride-8 upsamplers, ConvTranspose1d(Cin -> Cout, k = 16, stride 8, padding 4) (hifi/models.py:166-176,189 with
 * upsample_rates[i] = 8), on the window-conv kernel: x16 (B, T, Cin) fp16 -> out16 (B, 8T, Cout) fp16.  Output frame 8t + r reads
 * x[t] (weight tap r + 4) and x[t - 1] (r < 4: tap r + 12) or x[t + 1] (r >= 4: tap r - 4): a conv with two pseudo-taps and 8 * Cout
 * phase-major output channels whose rows are the output tensor.  w_packed: ttsk_win_conv_pack_items of the (8 * Cout, 2, Cin) tap-major
 * pseudo-weight W2[r * Cout + co][slot][ci]; bias8: the bias repeated 8 times.  Replaces the polyphase implicit GEMMs of ttsk_gemm. */
int ttsk_hifi_upsample8_supported(int Cin, int Cout);
int ttsk_hifi_upsample8(const void* x16, const void* w_packed, const float* bias8, void* out16, int f16, int B, int T, int Cin, int Cout,
                        void* stream);
/* The same for any ConvTranspose1d(kernel 2 * stride, padding stride / 2) the kernel is instantiated for: stride 8 as above, stride 2
 * (k = 4, padding 1) for 128 -> 64 channels (hifi/models.py: ups[2]).  Output frame stride * t + r reads x[t] (tap r + stride / 2) and
 * x[t - 1] (r < stride / 2: tap r + 3 * stride / 2) or x[t + 1] (tap r - stride / 2); pseudo-weight (stride * Cout, 2, Cin). */
int ttsk_hifi_upsample_win_supported(int Cin, int Cout, int stride);
int ttsk_hifi_upsample_win(const void* x16, const void* w_packed, const float* bias_rep, void* out16, int f16, int B, int T, int Cin, int Cout,
                           int stride, void* stream);
/* HiFi-GAN's conv_pre + the LeakyReLU its only reader applies (hifi/models.py:152,186,188), Conv1d(80 -> Cout, k) on fp16 rows, on the
 * window-conv kernel (96-channel instance, contraction zero-padded): out16 (B, T, Cout) = lrelu(conv(x16 (B, T, 80)) + bias, slope).
 * w_packed: ttsk_win_conv_pack_items of the (Cout, k, 80) tap-major weight.  Replaces ttsk_conv1d's implicit GEMM for this layer. */
int ttsk_hifi_conv_pre_win_supported(int Cin, int Cout, int K);
int ttsk_hifi_conv_pre_win(const void* x16, const void* w_packed, const float* bias, void* out16, int f16, int B, int T, int Cin, int Cout, int K,
                           float slope, void* stream);
/* The same operator, operands and pack (ttsk_hifi_upsample_win's) for Cin = 256, stride 8 on a kernel that loads a 96-frame window once and
 * loops over the 8 * Cout / 256 channel groups inside the workgroup, each group's stores in flight under the next group's MFMAs
 * (hifi/models.py: ups[1], 256 -> 128: one round of 256 workgroups instead of two rounds of 448 window loads).  The bias is the
 * accumulators' initial value here: results equal ttsk_hifi_upsample_win's to the last fp32 bit before the fp16 rounding. */
int ttsk_hifi_upsample_loop_supported(int Cin, int Cout, int stride);
int ttsk_hifi_upsample_loop(const void* x16, const void* w_packed, const float* bias_rep, void* out16, int f16, int B, int T, int Cin, int Cout,
                            int stride, void* stream);

/* Fused sub-layer tail of an FFT block (reference: fs_two/transformer/SubLayers.py:62-63 and :96-99 + Layers.py:29,32):
 *   out = zero_PAD_rows( LayerNorm( dropout_{p_pre, site_pre}( A[M,K] @ W[D,K]^T + bias ) + res ) ),  D = 256 only.
 * A, W, res, out, z_save bf16; z_save (may be NULL) receives the LayerNorm input, mean / rstd [M] its statistics (what
 * ttsk_layernorm_bwd needs); lens (may be NULL) marks rows t >= lens[row / seg_len] of each segment as PAD.  Same dropout
 * bits as ttsk_layernorm_fwd at the same (rng, site) — the two forms are interchangeable up to the bf16 rounding of
 * the GEMM output that the fused kernel skips. */
int ttsk_gemm_ln_fwd(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res, const float* gamma,
                     const float* beta, void* out, void* z_save, float* mean, float* rstd, const int64_t* lens, int seg_len,
                     int M, int K, int D, float eps, float p_pre, uint32_t site_pre, const void* rng, void* stream);
/* The same fused op on the window-conv data path: W_packed is the MFMA-fragment-major pack of the (256, K) weight
 * (ttsk_win_conv_pack_* with (Cs, K, Ds) = (256, 1, K), transpose = 0); K = 256 or 1024.  Same row code, same dropout mask. */
int ttsk_win_ln_supported(int K, int D);
int ttsk_win_ln_fwd(const void* A, int lda, const void* W_packed, const float* bias, const void* res, const float* gamma, const float* beta,
                    void* out, void* z_save, float* mean, float* rstd, const int64_t* lens, int seg_len, int M, int K, int D, float eps,
                    float p_pre, uint32_t site_pre, const void* rng, void* stream);
/* ttsk_win_ln_fwd whose output rows also go, inside the same kernel, through the NEXT FFTBlock's q|k|v projection
 * (reference SubLayers.py:41-43: w_qs / w_ks / w_vs on the block input): proj_out[M][768] = out · W' + proj_bias, proj_w_packed =
 * the ttsk_win_conv pack of the (768, 1, 256) weight.  One launch instead of two dependent ones; proj_out is bit-identical to
 * ttsk_win_conv on `out`. */
int ttsk_win_ln_proj_fwd(const void* A, int lda, const void* W_packed, const float* bias, const void* res, const float* gamma,
                         const float* beta, void* out, void* z_save, float* mean, float* rstd, const int64_t* lens, int seg_len, int M,
                         int K, int D, float eps, float p_pre, uint32_t site_pre, const void* rng, const void* proj_w_packed,
                         const float* proj_bias, int proj_Cout, void* proj_out, void* stream);

/* what ttsk_gemm will run for `d` (with d->kernel / d->splits as constraints when non-zero) and the workspace it needs */
int ttsk_gemm_plan(const ttsk_gemm_desc* d, int32_t* kernel, int32_t* splits, int64_t* workspace_bytes);


/* ------------------------------------------------------------------------------------ LengthRegulator
 * reference: fs_two/model/modules.py:220-252 (LengthRegulator.LR/expand) + fs_two/utils/tools.py:369-387 (pad)
 *            + fs_two/transformer/Models.py:176-178 (decoder adds the position table right after).
 * Integer-exact: di = max(trunc(d), 0); cs = inclusive wavefront prefix scan of di (64 phonemes per scan
 * step); frame t of utterance b copies phoneme #{i : cs[i] <= t} when t < cs[L-1], else it is a zero row;
 * mel_len[b] = cs[L-1] (NOT cropped to T).  `pe` (fp32 [>=T][D], may be NULL) is added to every row.
 * dur_dtype: 0 = int64, 1 = fp32, 2 = int32.
 */
int ttsk_length_regulator_fwd(const void* x_bf16, const void* dur, int dur_dtype, const float* pe, void* out_bf16,
                              int32_t* idx_out /* [B][T], -1 = zero row, may be NULL */,
                              int32_t* cumsum_out /* [B][L] */, int64_t* mel_len /* [B] */, int B, int L, int T, int D,
                              void* stream);
/* dx[b][i][:] = sum over the frames that copied phoneme i of dout[b][t][:]  (segment sum, no atomics) */
int ttsk_length_regulator_bwd(const void* dout_bf16, const int32_t* cumsum, void* dx_bf16, int B, int L, int T, int D,
                              void* stream);

/* ------------------------------------------------------------------------------ LayerNorm (fused block tail)
 * out = mask( dropout_post( LN( dropout_pre(y) + res ) ) ),  optional head_out[row] = mask(<out, head_w> + head_b)
 * reference: SubLayers.py:62-63,99-101 (LN(dropout(sublayer)+residual)), Layers.py:29,32 (masked_fill of PAD rows),
 *            model/modules.py:270-309 (VariancePredictor: ReLU -> LN -> Dropout; Linear(256,1) -> masked_fill).
 * rows are (segment, position) pairs; a row is PAD when position >= lens[segment] (lens may be NULL).
 * `rng` points at {uint64 seed, uint64 step} in device memory; masks are functions of (seed, step, site, element).
 * z_save receives the LN input (bf16) for the backward; mean/rstd are per-row fp32.
 */
int ttsk_layernorm_fwd(const void* y_bf16, const void* res_bf16, const float* gamma, const float* beta, void* out_bf16,
                       void* z_save_bf16, float* mean, float* rstd, const int64_t* lens, int seg_len, int rows, int D,
                       float eps, float p_pre, uint32_t site_pre, float p_post, uint32_t site_post, const uint64_t* rng,
                       const float* head_w, const float* head_b, float* head_out, void* stream);
int ttsk_layernorm_bwd_nblocks(int rows);
/* partials: [nblocks][3*D] = dbias(sum of dy) | dgamma | dbeta, or [nblocks][4*D + 1] with the head (| dhead_w | dhead_b)
 * — the order in which these parameters sit in the flat gradient buffer, so one ttsk_colsum_finalize call lands them all.
 * dz = grad wrt the LN input (bf16; times (z > 0) when relu_in); dy = dz through the pre-dropout mask (only if p_pre > 0). */
int ttsk_layernorm_bwd(const void* dout_bf16, const float* dhead, const float* head_w, const void* z_bf16, const float* mean,
                       const float* rstd, const float* gamma, const float* beta, const int64_t* lens, int seg_len, int rows,
                       int D, int relu_in, float p_pre, uint32_t site_pre, float p_post, uint32_t site_post,
                       const uint64_t* rng, void* dz_bf16, void* dy_bf16, float* partials, void* stream);
/* Grouped forms: rows = groups * group_rows; group g reads gamma / beta / head_w / head_b at + g * param_stride floats and
 * uses dropout sites + g * site_stride; PAD masks (lens [group_rows / seg_len], shared by the groups) and dropout element
 * indices are taken inside the group, so one grouped launch equals `groups` single launches bit for bit (the three
 * VariancePredictors of a training step: model/modules.py:158-193 with targets given are independent).  bwd partials:
 * [groups][ttsk_layernorm_bwd_nblocks(group_rows)][3*D or 4*D+1]. */
int ttsk_layernorm_fwd_grouped(const void* y_bf16, const void* res_bf16, const float* gamma, const float* beta, void* out_bf16,
                               void* z_save_bf16, float* mean, float* rstd, const int64_t* lens, int seg_len, int groups,
                               int group_rows, int64_t param_stride, uint32_t site_stride, int D, float eps, float p_pre,
                               uint32_t site_pre, float p_post, uint32_t site_post, const uint64_t* rng, const float* head_w,
                               const float* head_b, float* head_out, void* stream);
int ttsk_layernorm_bwd_grouped(const void* dout_bf16, const float* dhead, const float* head_w, const void* z_bf16,
                               const float* mean, const float* rstd, const float* gamma, const float* beta, const int64_t* lens,
                               int seg_len, int groups, int group_rows, int64_t param_stride, uint32_t site_stride, int D,
                               int relu_in, float p_pre, uint32_t site_pre, float p_post, uint32_t site_post, const uint64_t* rng,
                               void* dz_bf16, void* dy_bf16, float* partials, void* stream);
/* ttsk_layernorm_bwd whose upstream gradient is still in split-K form: dout[row] = sum_s slabs[s*slab_stride + row*D ..] (+ R[row],
 * bf16, may be NULL) — the raw partial tiles a ttsk_gemm with TTSK_GEMM_RAW_SLABS left behind (the dX GEMM that feeds this
 * LayerNorm) are summed in fixed order while the rows are read, in fp32, so neither a reducer launch nor a bf16 copy of dout
 * exists.  Other arguments as ttsk_layernorm_bwd (no head mode). */
int ttsk_layernorm_bwd_slabs(const float* slabs, int nsplit, int64_t slab_stride, const void* R_bf16, const void* z_bf16,
                             const float* mean, const float* rstd, const float* gamma, const float* beta, const int64_t* lens,
                             int seg_len, int rows, int D, int relu_in, float p_pre, uint32_t site_pre, float p_post,
                             uint32_t site_post, const uint64_t* rng, void* dz_bf16, void* dy_bf16, float* partials, void* stream);
/* ttsk_layernorm_bwd (D = 256, no head / ReLU input / post dropout; upstream gradient as dout_bf16 OR as split-K slabs + R as in
 * ttsk_layernorm_bwd_slabs) followed, in the same kernel, by the k = 1 projection that consumes dy — the sub-layer's input gradient:
 *   out[rows][Cout] = dy · W'   with w_packed = ttsk_win_conv's pack of the transposed weight (Cout = 256 or 1024, Cin = 256),
 *   gate_bf16 (may be NULL): out = gate > 0 ? out : 0  (w_2's dX through the ReLU: reference SubLayers.py:93-101 backward),
 *   delta_o32 / delta_out (may be NULL; Cout = 256 = 2 heads x 128, rows = B*seg_len): the attention backward's
 *   delta[(b*2 + h)*seg_len + t] = sum over head h's columns of out * o32  (fc's dX: SubLayers.py:62-63 backward).
 * pre_x_bf16 / pre_w_packed / pre_K (instead of dout_bf16 and slabs; pre_K = 768): the upstream gradient is itself a k = 1 projection
 * that only this LayerNorm reads, dout = pre_x · W_pre' (+ R) — the input gradient of the FOLLOWING block's q|k|v projection
 * (pre_x = dqkv [rows][768], pre_w_packed = the pack of the transposed (768, 1, 256) weight): computed per 32-row tile in fp32,
 * never written to memory (three dependent launches become one).
 * One launch instead of two dependent ones; results are bit-identical to ttsk_layernorm_bwd(_slabs) + ttsk_win_conv.
 * partials: [ttsk_layernorm_bwd_proj_nblocks(rows)][3*D] (dbias | dgamma | dbeta), a workgroup per 32 rows. */
int ttsk_layernorm_bwd_proj_nblocks(int rows);
int ttsk_layernorm_bwd_proj(const void* dout_bf16, const float* slabs, int nsplit, int64_t slab_stride, const void* R_bf16,
                            const void* z_bf16, const float* mean, const float* rstd, const float* gamma, const int64_t* lens,
                            int seg_len, int rows, int D, float p_pre, uint32_t site_pre, const uint64_t* rng, void* dz_bf16,
                            void* dy_bf16, float* partials, const void* w_packed, int Cout, const void* gate_bf16,
                            const float* delta_o32, float* delta_out, void* out_bf16, const void* pre_x_bf16,
                            const void* pre_w_packed, int pre_K, void* stream);
/* The q|k|v input gradient on its own, out[rows][256] = dqkv[rows][768] · W' (+ R_bf16, may be NULL), for the first block of a stack
 * (no LayerNorm backward in front of it to host the product: reference SubLayers.py:41-43 backward + the residual of :62): 32-row
 * tiles, one pass over the contraction, the window-conv pack of the transposed weight, no split-K slabs.  K = 768, D = 256. */
int ttsk_qkv_dx(const void* dqkv_bf16, const void* w_packed, const void* R_bf16, void* out_bf16, int rows, int K, int D, void* stream);
/* dst[c] (+)= scale * sum_b partials[b*ld + c]  in fixed order */
int ttsk_colsum_finalize(const float* partials, int nblk, int ncols, int ld, float* dst, int accumulate, float scale,
                         void* stream);
/* the same for a list of (partials, dst) pairs in one launch per 64 items (gradient column sums are needed only by Adam) */
typedef struct ttsk_finalize_item {
  const float* partials;
  float* dst;
  int32_t nblk, ncols, ld, accumulate;
  float scale;
} ttsk_finalize_item;
int ttsk_colsum_finalize_batch(const ttsk_finalize_item* items, int n, void* stream);
int ttsk_colsum_nblocks(int rows);
/* per-block column sums of x [rows][C] (bf16, or fp32 when is_f32) -> partials[nblocks][C]  (bias gradients) */
int ttsk_colsum(const void* x, int is_f32, int rows, int C, int ld, float* partials, void* stream);
/* the same for up to 64 matrices per launch; nblk must be ttsk_colsum_nblocks(rows) */
typedef struct ttsk_colsum_item {
  const void* x;
  float* partials;
  int32_t is_f32, rows, C, ld, nblk;
} ttsk_colsum_item;
int ttsk_colsum_batch(const ttsk_colsum_item* items, int n, void* stream);

/* Training-mode VarianceAdaptor embedding chain in one pass (reference: model/modules.py:158-193 with targets given;
 * fastspeech2.py:72-75): x1 = x + speaker_table[speakers[row / L]]; x2 = x1 + pitch_table[bucketize(pitch_target)];
 * x3 = x2 + energy_table[bucketize(energy_target)] (bucketize = torch.bucketize, right=False, n_bins_minus_1 edges), each
 * rounded to bf16; the bucket indices are returned for the embedding-gradient scatter-sums.  va_combine is its backward around
 * the grouped predictor backward: dxin [3][rows][D] fp32 (gradients wrt x, x1, x2 from the duration / pitch / energy
 * predictors), dx3 -> dx2 = dx3 + dxin[2], dx1 = dx2 + dxin[1], dx = dx1 + dxin[0].
 * row_limit (int64 [rows / L], may be NULL): phoneme positions l >= row_limit[u] of utterance u do not exist in the reference's
 * batch (shape-bucketed training pads L up to a multiple of 8): they are written as zero rows / carry no gradient, so that the
 * predictors' convolutions see the zero padding the reference's shorter batch has there. */
int ttsk_va_embed(const void* x_bf16, const float* speaker_table, const int64_t* speakers, int L, const float* pitch_target,
                  const float* pitch_bins, const float* pitch_table, const float* energy_target, const float* energy_bins,
                  const float* energy_table, int n_bins_minus_1, void* x1_bf16, void* x2_bf16, void* x3_bf16, int32_t* pitch_idx,
                  int32_t* energy_idx, int rows, int D, const int64_t* row_limit, void* stream);
int ttsk_va_combine(const void* dx3_bf16, const float* dxin, void* dx2_bf16, void* dx1_bf16, void* dx_bf16, int rows, int D, int L,
                    const int64_t* row_limit, void* stream);

/* ------------------------------------------------------------------------------------------ attention softmax
 * reference: fs_two/transformer/Modules.py:15-22.  scores fp32 [nz][S][Sp] (already scaled by 1/sqrt(d_k) in the
 * Q.K^T GEMM epilogue), z = b*H + h; keys >= lens[b] get -inf; probs bf16 [nz][S][Sp] with zero pad columns.
 * bwd: dscores = alpha * P o (dP - rowsum(dP o P)).
 */
int ttsk_softmax_fwd(const float* scores, void* probs_bf16, const int64_t* lens, int nz, int H, int S, int Sp, void* stream);
int ttsk_softmax_bwd(const void* probs_bf16, const float* dprobs, void* dscores_bf16, int nz, int S, int Sp, float alpha,
                     void* stream);

/* ---------------------------------------------------------------------------- flash attention (d_k = 128)
 * softmax(q k^T * scale, keys >= lens[b] masked) v per (utterance, head) on the fused projection output qkv [B*S][3*d] (q | k | v, head h =
 * columns h*128.. of each part), heads merged back in o [B*S][d] (reference: fs_two/transformer/Modules.py:14-24 + SubLayers.py:44-60)
 * without any S x S tensor in HBM: the forward keeps a running row max / sum over 64-key tiles and returns O and, for the
 * backward, lse [B*H][S] = log sum_k exp(score); the backward recomputes P = exp(score - lse) per tile.
 * bwd: delta_ws [B*H][S] fp32 scratch; writes ALL of dqkv [B*S][3*d] (dQ | dK | dV, head h at columns h*128 of each part),
 * two launches (delta = rowsum(dO o O); then the query side (dQ) and the key side (dK, dV) as one grid), no atomics.
 * o_f32 [B*S][d] (may be NULL): O before its rounding to bf16.  The backward's delta = rowsum(dO o O) is what dP is cancelled
 * against; taken from the bf16 O its 2^-9 error dominates small dQ / dK gradients, so a training forward keeps the fp32 copy.
 * Contracts at the edges (pinned by tests/test_flash_edges_gpu.py):
 *   - lens[b] is clamped to S; an utterance with lens[b] <= 0 has no keys and yields O = 0, o_f32 = 0, lse = 0 and zero dQ, dK, dV;
 *   - K and V rows at keys >= lens[b] (and < S) are read and multiplied by an exact 0: they must be FINITE (0 * Inf is NaN inside the
 *     MFMA), and whatever finite values they hold changes no output bit; their dK / dV rows are written as exact zeros. */
int ttsk_flash_attention_fwd(const void* qkv_bf16, void* o_bf16, float* o_f32 /* may be NULL */, float* lse /* may be NULL */,
                             const int64_t* lens, int B, int H, int S, int d, float scale, void* stream);
/* delta_ready = 1: delta_ws already holds delta (the producer of dout wrote it: ttsk_win_conv with delta_out), no delta launch. */
int ttsk_flash_attention_bwd(const void* qkv_bf16, const void* o_bf16, const float* o_f32 /* may be NULL */, const void* dout_bf16,
                             const float* lse, float* delta_ws, int delta_ready, void* dqkv_bf16, const int64_t* lens, int B, int H, int S,
                             int d, float scale, void* stream);

/* ------------------------------------------------------------------------------- embeddings / variance adaptor
 * bucketize: idx = #{bins < v*scale} (torch.bucketize right=False; reference: model/modules.py:95-100,134-139)
 * gather_add: out[row] = (in ? in[row] : 0) + table[idx[row / idx_div]] + (pe ? pe[row % pe_mod] : 0)
 *             reference: Models.py:101-103, fastspeech2.py:72-75 + modules.py:159, modules.py:95-100,134-139
 * scatter_sum: dtable[v] (+)= sum of dx rows whose index is v, ascending row order, no atomics; skip_row = padding_idx
 */
int ttsk_bucketize(const float* values, const float* bins, int n_bins, float scale, int32_t* idx, float* scaled_out,
                   int n, void* stream);
/* d = clamp(round(exp(logd) - 1) * d_control, min 0), fp32 — reference: model/modules.py:199-203 */
int ttsk_duration_round(const float* logd, float d_control, float* out, int n, void* stream);
/* mask[b][t] = (t >= lens[b]) as bytes (torch.bool storage) — reference: fs_two/utils/tools.py:121-131 */
int ttsk_length_mask(const int64_t* lens, uint8_t* mask, int B, int T, void* stream);
/* out = a + scale_b * b */
int ttsk_add_f32(const float* a, const float* b, float scale_b, float* out, int64_t n, void* stream);
int ttsk_gather_add(const void* in_bf16, const float* table, const void* idx, int idx_is_i64, int idx_div, const float* pe,
                    int pe_mod, void* out_bf16, int rows, int D, void* stream);
int ttsk_scatter_sum(const void* dx_bf16, const void* idx, int idx_is_i64, int idx_div, int n_idx, float* dtable,
                     int n_table_rows, int D, int skip_row, int accumulate, void* stream);
/* ---- batched synthesis: per-utterance limits and controls (tts_king_amd/synth.py `mel_ragged`)
 * Rows are (utterance, position) pairs, row = u*seg_len + l.  Positions l >= lens[u] (int64 [rows / seg_len], clamped to
 * [0, seg_len] in the kernel) exist only because the call padded its texts to a shape bucket: they are written as zero rows, the
 * zero padding the predictors' convolutions (model/modules.py:255-309) meet when utterance u runs alone.
 * gather_add_lens: out[row] = in[row] + table[idx[row / seg_len]] (the speaker add, fastspeech2.py:72-75), idx int64.
 * embed_step: the free-running embedding step (modules.py:92-101,131-140 without targets) in one launch --
 *   scaled[row] = pred[row] * control[row / seg_len]; idx[row] = #{bins < scaled[row]}; x_out[row] = x[row] + table[idx[row]].
 *   Search, NaN rule and sums are ttsk_bucketize's and ttsk_gather_add's: a control array filled with one value gives their bits.
 * duration_round_dev: ttsk_duration_round with d_control[i / L] read from a device fp32 array. */
int ttsk_gather_add_lens(const void* in_bf16, const float* table, const int64_t* idx, const int64_t* lens, int seg_len,
                         void* out_bf16, int rows, int D, void* stream);
int ttsk_embed_step(const float* pred, const float* control, const float* bins, int n_bins, const float* table,
                    const void* x_bf16, const int64_t* lens, int seg_len, void* x_out_bf16, float* scaled_out,
                    int32_t* idx_out, int rows, int D, void* stream);
int ttsk_duration_round_dev(const float* logd, const float* d_control, int L, float* out, int n, void* stream);
/* ---- per-phoneme prosody (tts_king_amd/synth.py `mel_ragged` with per-phoneme controls, explicit values or a frame budget)
 * embed_step_rows: ttsk_embed_step with control (rows,) and an explicit value per row -- scaled[row] = has[row] ? value[row] :
 *   pred[row] * control[row] (a set value is not multiplied: the reference's `target`, modules.py:92-101,131-140).  scaled_out /
 *   idx_out report what was used.  Constant control rows with has = 0 give ttsk_embed_step's bits.
 * duration_rows: v[i] = has[i] ? durations[i] : max(rint(exp(logd[i]) - 1) * d_control[i], 0)   (modules.py:195-205).
 * duration_fit: one workgroup per utterance u (seg_len <= 1024), l < lens[u] (clamped to [0, seg_len]); target[u] < 0 copies row u.
 *   Fixed phonemes (has) keep trunc(v), F = their sum; the free ones share budget = max(target[u] - F, 0): q = v * budget / S with
 *   S = the free phonemes' sum, out = floor(q) + 1 for the (budget - sum floor(q)) largest fractional parts, ties to the lower l;
 *   v = 0 stays 0; S = 0 leaves F frames.  Sums in a fixed order that depends on l only.  Positions past lens[u] are copied. */
int ttsk_embed_step_rows(const float* pred, const float* control, const float* value, const uint8_t* has, const float* bins,
                         int n_bins, const float* table, const void* x_bf16, const int64_t* lens, int seg_len, void* x_out_bf16,
                         float* scaled_out, int32_t* idx_out, int rows, int D, void* stream);
int ttsk_duration_rows(const float* logd, const float* d_control, const float* durations, const uint8_t* has, float* out, int n,
                       void* stream);
int ttsk_duration_fit(const float* v, const uint8_t* has, const int32_t* target, const int64_t* lens, int seg_len, float* out,
                      int B, void* stream);
/* the same for up to 8 independent tables per launch (all embedding-table gradients of a backward pass) */
typedef struct ttsk_scatter_item {
  const void* dx;      /* (n_idx * idx_div, D) bf16 */
  const void* idx;
  float* dtable;       /* (n_table_rows, D) fp32 */
  int32_t idx_is_i64, idx_div, n_idx, n_table_rows, D, skip_row, accumulate;
} ttsk_scatter_item;
int ttsk_scatter_sum_batch(const ttsk_scatter_item* items, int n, void* stream);

/* ------------------------------------------------------------------------------------------------ conversions */
int ttsk_cast_bf16(const float* src, void* dst_bf16, int64_t n, void* stream);
int ttsk_nct_to_ntc(const float* src, void* dst16, int f16, int B, int C, int T, void* stream);  /* f16: 0 = bf16, 1 = fp16 */
/* (x * scale) truncated toward zero to int16 — reference: hifiapi.py:50-51 */
int ttsk_to_int16(const float* src, int16_t* dst, int64_t n, float scale, void* stream);

/* ------------------------------------------------------------------------------------ windowed vocoding
 * Utterances of any length as N fixed-size windows of W mel frames (tts_king_amd/windows.py plans them on the host).  Both
 * kernels are driven by the device-resident plan table, TTSK_WIN_ROW int32 per window:
 *   [0] utterance   [1] start frame of the window in its utterance   [2],[3] kept frames [lo, hi) of the utterance
 *   [4] frame of the flat output where frame lo goes   [5] frame of the mel staging buffer where the window starts,
 *   -1 = padding window (reads zeros, keeps nothing)
 *   [6] (TTSK_WIN_VALID) valid frames of the row: 0 = all W (what a window of a long utterance holds); v in 1..W = an utterance
 *   shorter than the window as a row of its own (start 0, kept [0, v)): frames >= v of the row do not exist   [7] zero
 * so lengths are data and a captured graph holds for every call with the same N.
 * mel_windows: mel staging (fp32; frame f, channel c at src[f * stride_t + c * stride_c]: (C, frames) rows with stride_t = 1, or
 *              FastSpeech2's (frames, C) rows with stride_c = 1) -> (N, W, C) bf16 / fp16 channels-last, what ttsk_nct_to_ntc
 *              writes for a (N, C, W) batch.  W a multiple of 32, C a multiple of 8, n_src_frames = frames the staging holds.
 *              A row with v valid frames reads v frames of the staging buffer (checked against n_src_frames with v, not W) and is
 *              zero from frame v on.
 * wav_stitch:  (N, spf * W) fp32 window waveforms (spf samples per frame, a multiple of 8) -> the kept samples of every window at
 *              dst[plan[4] * spf ...]; to_i16 = 0: fp32, 1: int16 = (x * scale) truncated toward zero (ttsk_to_int16's arithmetic).
 *              n_dst_frames = frames the destination holds. */
#define TTSK_WIN_ROW 8
#define TTSK_WIN_VALID 6
int ttsk_mel_windows(const float* src, int64_t stride_t, int64_t stride_c, int64_t n_src_frames, const int32_t* plan, void* dst16,
                     int f16, int N, int W, int C, void* stream);
int ttsk_wav_stitch(const float* src, const int32_t* plan, void* dst, int64_t n_dst_frames, int to_i16, float scale, int N, int W,
                    int spf, void* stream);

/* ------------------------------------------------------------------------------------ sample-rate conversion
 * The flat waveform buffer (utterances back to back, what ttsk_wav_stitch writes with to_i16 = 0) resampled by the rational factor
 * L / M with a polyphase FIR (tts_king_amd/resample.py designs it).  Driven by the device-resident segment
 * table, TTSK_SEG_ROW int32 per utterance, 16-byte aligned:
 *   [0] src_off   first sample of the utterance in src        [1] src_len   its samples; 0 = an empty padding row
 *   [2] dst_off   first sample of the utterance in dst        [3] dst_len   samples to write (the planner: ceil(src_len * L / M))
 * so lengths are data and a captured graph holds for every call with the same n_segs and n_dst.
 * Coefficient table: fp32, tap-major: P rows (taps) of L phases, T[p][q] at table[q * L + p] (a wave reads one row per tap); C is
 * the tap that meets x[j0].  The table and C are arguments: any table runs.  Output sample m of a segment:
 *   y[m] = sum_{q = 0 .. P-1} T[p][q] * x[j0 + C - q],   u = m * M (64-bit), p = u mod L, j0 = u div L,
 * with x[j] = 0 outside [0, src_len) of its own segment (a neighbour's samples are never read as signal), accumulated in fp32 by
 * one thread in the order of q: the value depends on the segment's samples, the table and m only.
 * Exactly dst_len samples per segment are written and nothing else (gaps and the tail of dst keep their bytes); segments may start
 * anywhere.  A row that does not fit n_src / n_dst is skipped.  to_i16 = 0: fp32; 1: int16 = (int)clamp(y * scale, -32768, 32767),
 * truncated toward zero: ttsk_to_int16's arithmetic in range, saturating out of it (a resampler overshoots a near-full-scale
 * signal; the low 16 bits would wrap that into a click).
 * resample_tile (host only): samples of dst one workgroup serves for this filter, 0 for a filter ttsk_resample refuses.  Tiles may
 * straddle segments, so no planner needs it; it tells a test where the tile edges lie. */
#define TTSK_SEG_ROW 4
int ttsk_resample_tile(int L, int M, int P);
int ttsk_resample(const float* src, int64_t n_src, const int32_t* segs, int n_segs, const float* table, int L, int M, int P, int C,
                  void* dst, int64_t n_dst, int to_i16, float scale, void* stream);

/* ------------------------------------------------------------------------------------ utterances joined into one waveform
 * U utterances that lie in one flat fp32 buffer (what ttsk_wav_stitch or ttsk_resample wrote, or the rows of a padded batch) trimmed,
 * levelled, faded and laid out behind each other with pauses between, as ONE waveform (tts_king_amd/narrate.py plans it; DESIGN.md
 * section 22).  Everything that depends on a length or a setting is data: the device-resident join table, (1 + U) rows of
 * TTSK_JOIN_ROW 32-bit words, 16-byte aligned.  Row 0 holds the settings:
 *   [0] mode    TTSK_JOIN_GIVEN / _RMS / _PEAK            [1] fade    samples of the linear fade at either end of a kept range
 *   [2] keep    samples kept outside first / last          [3] lead    zeros before the first utterance
 *   [4] r       fp32: threshold as a fraction of the peak  [5] floor   fp32: the threshold's lower bound
 *   [6] target  fp32: RMS aimed at (mode _RMS)             [7] limit   fp32: peak never exceeded (modes _RMS, _PEAK)
 * and row 1 + u is utterance u:
 *   [0] src_off first sample in src   [1] src_len samples (0: an empty row, e.g. padding)   [2] pause  zeros behind it
 *   [3] flags   bit 0: trim           [4] gain    fp32, mode _GIVEN                          [5..7] zero
 * With x the row's n samples, all in fp32 and in this order: peak = max |x[i]|; with the trim flag thr = max(peak * r, floor), first /
 * last = the first / last i with |x[i]| >= thr, kept range a = max(0, first - keep), b = min(n, last + 1 + keep), empty (a = b = 0)
 * when there is no such i or peak == 0; without the flag a = 0, b = n.  ss = sum of x[i]^2 over [a, b), rms = sqrt(ss / (b - a)).
 * g = the row's gain (_GIVEN), min(target / rms, limit / peak) (_RMS), limit / peak (_PEAK); 1 when the range is empty or peak == 0.
 * F = min(fade, (b - a) / 2); w(k) = float(2k + 1) / float(2F) over the first F kept samples, mirrored over the last F, 1 between.
 * o_u = lead + sum over v < u of (b_v - a_v + pause_v);  dst[o_u + k] = (x[a + k] * g) * w(k);  total = o_U.  EVERY sample of dst
 * is written: zeros in the lead, the pauses and from `total` to n_dst.  Samples that would lie at or past n_dst are dropped.
 * to_i16 = 0: fp32; 1: int16 = (int)clamp(y * scale, -32768, 32767), ttsk_resample's rule.
 * Negative fade / keep / lead / pause count as 0; a row that does not fit n_src counts as empty (its pause stays).
 * info: (U + 1) rows of TTSK_JOIN_ROW 32-bit words, 16-byte aligned, written by the kernels for the host to read with the waveform:
 *   row u:  [0] a  [1] b  [2] o_u  [3] peak (fp32)  [4] ss (fp32)  [5] g (fp32)  [6..7] zero;     row U:  [0] total, rest zero
 * (o_u and total saturate at 2^31 - 1).  wav_join_stats: one launch, U workgroups, writes a, b, peak, ss, g.  wav_join: one launch,
 * one workgroup per tile of dst, reads what wav_join_stats left in `info`, writes o_u, total and dst.  No atomics: the same bits on
 * every run.  U <= TTSK_JOIN_MAX_ROWS, n_src and n_dst below 2^31. */
#define TTSK_JOIN_ROW 8
#define TTSK_JOIN_MAX_ROWS 4096
#define TTSK_JOIN_GIVEN 0
#define TTSK_JOIN_RMS 1
#define TTSK_JOIN_PEAK 2
int ttsk_wav_join_stats(const float* src, int64_t n_src, const int32_t* join, int U, int32_t* info, void* stream);
int ttsk_wav_join(const float* src, int64_t n_src, const int32_t* join, int U, int32_t* info, void* dst, int64_t n_dst, int to_i16,
                  float scale, void* stream);

/* ------------------------------------------------------------------------------------ device-resident training set
 * One launch builds one packed training batch (the buffer of tts_king_amd/dataset.py `packed_layout`: what the DeviceFeeder uploads
 * for the same utterances) from a training set that lives on the device (tts_king_amd/resident.py).  The
 * kernel is "gather ragged rows, zero-pad" over a table of at most TTSK_COLLATE_MAX_FIELDS fields; it knows nothing of the batch
 * tuple.  A field is one flat device array holding every utterance's rows back to back (each row `inner` elements of `elem_size`
 * bytes) plus two device tables indexed by utterance: `offsets` (int64, first ELEMENT of the utterance) and `lens` (int32, its rows).
 * In the destination the field is (B, padded_rows, inner) at byte `dst_off`; a per-utterance scalar is a field with one row.
 *   dst[dst_off + ((b * padded_rows + r) * inner + c) * elem_size ...] = src[offsets[u] + r * inner + c],  u = idx[b], r < lens[u]
 * and every other byte of dst is written as zero: the rest of a padded row, the gap between a field's end and the next field (or
 * limit, or dst_bytes), anything before the first field.  So the buffer's old content never survives and equal arguments give
 * equal bytes.  nan_to_zero (elem_size 4 only): an fp32 NaN is written as +0.  Fields must be in ascending dst_off order, 16-byte
 * aligned, not overlapping; dst 16-byte aligned, dst_bytes a multiple of 16 below 2^31.  Sources may be larger than 2^31 bytes.
 * The limits of a shape-bucketed batch come by value and follow the fields: fl_off >= 0: int32 t_true at byte fl_off; pl_off >= 0:
 * B int64 l_true from byte pl_off (fl before pl when both are present); < 0: absent.
 * idx_dev: the batch's B utterance numbers on the device (a slice of an epoch's uploaded plan); idx_host and every field's
 * lens_host are the host's copies of the same numbers, read here and never by the kernel.  Refused before the launch: an index
 * outside [0, n_utts), a row count above padded_rows, an element size other than 4 or 8.  The kernel checks again what it reads
 * from device memory (index, offset and length against n_utts / n_src / padded_rows) and writes zeros for a row that fails: wrong
 * tables give a wrong batch, never a wild access.  16-byte loads where the source piece is 16-byte aligned and lies inside one
 * utterance's rows (mel rows are 320 bytes: always, when utterances start 16-byte aligned), dword loads elsewhere; 16-byte stores
 * everywhere, each byte of dst written exactly once. */
#define TTSK_COLLATE_MAX_FIELDS 16
typedef struct ttsk_collate_field {
  const void* src;            /* device: the field's flat array */
  const int64_t* offsets;     /* device: (n_utts) first element of each utterance */
  const int32_t* lens;        /* device: (n_utts) rows of each utterance */
  const int32_t* lens_host;   /* host:   the same lengths (argument checking only) */
  int64_t n_src;              /* elements src holds */
  int64_t dst_off;            /* byte offset of the field in dst */
  int32_t elem_size, inner, padded_rows, nan_to_zero;
} ttsk_collate_field;
int ttsk_collate_batch(const ttsk_collate_field* fields, int n_fields, const int32_t* idx_dev, const int32_t* idx_host, int B,
                       int64_t n_utts, void* dst, int64_t dst_bytes, int64_t fl_off, int32_t t_true, int64_t pl_off, int64_t l_true,
                       void* stream);

/* ------------------------------------------------------------------------------------ HiFi-GAN generator
 * reference: hifi/models.py:146-210 (Generator), :12-95 (ResBlock1), hifi/vocoder/utils.py:24-37.
 * 16-bit tensors of this family are bf16 (f16 = 0) or IEEE fp16 (f16 = 1; what hifigan.py uses: the generator is
 * inference-only, fp16 has 3 more mantissa bits than bf16 at the same MFMA rate and its activations stay far inside
 * fp16's range).  The convolutions themselves run on ttsk_gemm (conv-A mode: dilation = tap_dshift, LeakyReLU fused into the
 * operand staging, ConvTranspose1d as `stride` polyphase launches with the output-row remap).
 * weight_norm_fold: w[r][:] = v[r][:] * g[r] / ||v[r][:]||  (remove_weight_norm, dim 0 — for ConvTranspose1d rows are
 *                   IN-channels, hifi/models.py:203-210).
 * pack_conv_weight: mode 0: Conv1d (Cout,Cin,k) fp32 -> (Cout,k,Cin) bf16; mode 1: ConvTranspose1d (Cin,Cout,k) fp32 ->
 *                   (k,Cout,Cin) bf16.  (d0,d1,d2) = the source shape.
 * avg3:             out = leaky_relu((a + b + c) * scale, slope) — the multi-receptive-field average, hifi/models.py:190-196,
 *                   with the consumer's LeakyReLU fused (slope 1.0 = none).
 */
int ttsk_weight_norm_fold(const float* v, const float* g, float* w, int rows, int cols, void* stream);
int ttsk_pack_conv_weight(const float* src, void* dst16, int f16, int d0, int d1, int d2, int mode, void* stream);
/* "Window" Conv1d for the C = 128 stage (one conv per launch, activation window resident in LDS, weights streamed from a
 * ttsk_pack_resblock_weight pack): out = [lrelu](conv_{K,dil}(x) + bias [+ R]); out2 (optional) = lrelu(out, slope).
 * x must already be activated (zeros outside the utterance are the conv padding).  reference: hifi/models.py:88-95. */
int ttsk_hifi_conv_window_supported(int C, int K, int dil);
int ttsk_hifi_conv_window(const void* x16, const void* w_pack, const float* bias, const void* R16, void* out16, void* out2_16,
                          int f16, int B, int len, int C, int K, int dil, int lrelu_out, float slope, void* stream);
/* The (c1 dilated -> LeakyReLU -> c2 -> + x) pair of ResBlock1 (hifi/models.py:88-95) as ONE launch at C = 128: x is the raw block
 * input, out = c2(lrelu(c1(lrelu(x)) + b1)) + b2 + x; lrelu(c1 ..) stays in LDS.  Bit-identical to two ttsk_hifi_conv_window
 * launches, a third of their HBM traffic.  w*_pack as for ttsk_hifi_conv_window; out must not alias x.
 * mode folds the MRF average (hifi/models.py:190-197) into a block's last pair, with ttsk_hifi_resblock1's meaning:
 * 0: out = y   1: out += y   2: out = lrelu((out + y) * scale, final_slope).
 * C = 128: a wave owns 32 output channels; C = 64 / 32 (the last two stages): a wave owns a quarter of the frames. */
int ttsk_hifi_conv_pair_supported(int C, int K, int dil);
int ttsk_hifi_conv_pair(const void* x16, const void* w1_pack, const float* bias1, const void* w2_pack, const float* bias2, void* out16,
                        int f16, int B, int len, int C, int K, int dil, float slope, int mode, float scale, float final_slope,
                        void* stream);
/* The same pair at C = 64 (and at C = 128 for K = 3) with the weights STATIONARY in registers (round 6, csrc/pairws.hip; hifi/models.py:88-95,
 * :190-197): one persistent 8-wave workgroup per CU walks a contiguous run of 192-frame tiles (96 at C = 128); four waves hold c1's weights and four c2's for the whole
 * launch (32 output channels x K taps x 64 input channels = 16 K registers per lane), the c1 waves produce tile s's lrelu(c1) window in LDS
 * while the c2 waves consume tile s - 1's; the next tile's x window is in flight under the MFMAs.  Arguments, modes and results as
 * ttsk_hifi_conv_pair (bit-identical to it); C = 64: K in {3, 7, 11}, C = 128: K = 3; dil in {1, 3, 5}; tensors below 2 GiB (32-bit buffer offsets);
 * max_wgs: grid cap (0 = one workgroup per CU). */
int ttsk_hifi_conv_pair_ws_supported(int C, int K, int dil);
int ttsk_hifi_conv_pair_ws(const void* x16, const void* w1_pack, const float* bias1, const void* w2_pack, const float* bias2, void* out16,
                           int f16, int B, int len, int C, int K, int dil, float slope, int mode, float scale, float final_slope,
                           int max_wgs, void* stream);
/* ResBlock2 (hifi/models.py:104-143, the block of the V3 generator) as ONE launch, csrc/resblock2.hip: x16 is the raw block input
 * (B, len, C), x1 = x + b0 + conv_{K,d0}(lrelu(x)), y = x1 + b1 + conv_{K,d1}(lrelu(x1)); x1 (rounded to the 16-bit type) and
 * lrelu(x1) stay in LDS, each conv sees zeros outside [0, len).  w*_pack: ttsk_pack_resblock_weight packs; out must not alias x.
 * mode as ttsk_hifi_conv_pair (0: out = y   1: out += y   2: out = lrelu((out + y) * scale, final_slope)): a stage of three blocks is
 * three launches.  C in {32, 64, 128}, K in {3, 5, 7}, (K-1)/2 * d0 <= 16, (K-1)/2 * d1 <= 40 (C = 128) / 48 (C = 64) / 64 (C = 32). */
int ttsk_hifi_resblock2_supported(int C, int K, int d0, int d1);
int ttsk_hifi_resblock2(const void* x16, const void* w0_pack, const float* bias0, const void* w1_pack, const float* bias1, void* out16,
                        int f16, int B, int len, int C, int K, int d0, int d1, float slope, int mode, float scale, float final_slope,
                        void* stream);
/* conv_post + tanh (hifi/models.py:198-199): x (B, len, C) 16-bit (already activated), w (1, k, C) tap-major 16-bit,
 * out (B, 1, len) fp32.  A streaming kernel: one output sample per thread. */
int ttsk_hifi_conv_post(const void* x16, const void* w16, const float* bias, float* out, int f16, int B, int len, int C, int K,
                        void* stream);
/* The stride-2, kernel-4 ConvTranspose1d upsamplers (hifi/models.py:166-176,189) as one streaming kernel: both output
 * phases from one read of the input.  x16 (B, T, Cin) 16-bit, w16 (4, Cout, Cin) tap-major (ttsk_pack_conv_weight mode 1),
 * out16 (B, 2T, Cout).  Instances: Cin -> Cout = 128 -> 64, 64 -> 32. */
int ttsk_hifi_upsample2_supported(int Cin, int Cout, int stride, int k);
int ttsk_hifi_upsample2(const void* x16, const void* w16, const float* bias, void* out16, int f16, int B, int T, int Cin,
                        int Cout, void* stream);
int ttsk_avg3(const void* a, const void* b, const void* c, void* out, int f16, int64_t n, float scale, float slope, void* stream);

/* Fused ResBlock1 (hifi/models.py:88-95): all six convs of one block for C in {32,64}, K in {3,7,11}; x/out 16-bit
 * channels-last (B, len, C); weights/biases in the order convs1[0], convs2[0], convs1[1], convs2[1], convs1[2],
 * convs2[2], each weight a fragment-major pack made by ttsk_pack_resblock_weight from the folded (C, C, K) fp32 tensor.
 * mode 0: out = y; 1: out += y; 2: out = (out + y) * scale — the MRF sum / average over the three blocks of a stage
 * (hifi/models.py:190-196); final_slope != 1 applies LeakyReLU(final_slope) to the stored value (the consumer's
 * activation, hifi/models.py:188,197, fused into the last block of the stage). */
int64_t ttsk_resblock_pack_elems(int C, int K);   /* elements of one pack (K padded to the kernel's weight stage) */
int ttsk_pack_resblock_weight(const float* src, void* dst16, int f16, int C, int K, void* stream);
int ttsk_hifi_resblock1(const void* x16, void* out16, int f16, const void* const* weights, const float* const* biases,
                        const int32_t* dilations, int B, int len, int C, int K, int mode, float scale, float slope,
                        float final_slope, void* stream);
int ttsk_hifi_resblock1_supported(int C, int K);
/* The WHOLE last stage of the generator in one launch (hifi/models.py:190-199, csrc/mrf32.hip): the three ResBlock1s of the C = 32
 * multi-receptive-field fusion (kernel sizes k0, k1, k2 = 3, 7, 11) on the same raw input x16 (B, len, 32), their sum * scale (1/3),
 * LeakyReLU(final_slope = 0.01: F.leaky_relu's default, :197), conv_post (32 -> 1, k_post = 7; w_post16 (1, 7, 32) tap-major 16-bit as
 * for ttsk_hifi_conv_post) and tanh: out (B, 1, len) fp32.  weights / biases: 18 entries, block j's six convs at [6 j ..] in
 * ttsk_hifi_resblock1's order and packs; dilations: 3 x 3.  stage_out16 (optional, (B, len, 32)): the activated average that
 * conv_post reads, for tests.  Bit-identical to three ttsk_hifi_resblock1 launches (modes 0, 1, 2) + ttsk_hifi_conv_post; one read of
 * x and one write of the waveform instead of nine tensor passes. */
int ttsk_hifi_mrf32_post_supported(int C, int k0, int k1, int k2, int k_post);
int ttsk_hifi_mrf32_post(const void* x16, float* out, void* stage_out16, int f16, const void* const* weights, const float* const* biases,
                         const int32_t* dilations, const void* w_post16, const float* b_post, int B, int len, int C, int k0, int k1, int k2,
                         int k_post, float slope, float final_slope, float scale, void* stream);

/* ---- a per-row length beside the batch stride (short utterances as rows of the windowed batch)
 * The fused generator kernels above carry one `len`: the row stride of the (B, len, C) batch AND the edge beyond which a conv reads and
 * writes zero.  The *_rowlen forms part the two.  row_frames[b * row_stride] (int32 on the device: column TTSK_WIN_VALID of the plan
 * table with row_stride = TTSK_WIN_ROW, or a compact copy with row_stride = 1) is the number of valid MEL frames of row b and spf the
 * samples per mel frame at the kernel's stage: positions >= row_frames * spf of the row are conv zero padding for every read and
 * every in-kernel intermediate, and nothing is stored there (a tile wholly past the edge returns at once), so `out16` must be ZERO
 * past the edge on entry wherever a later kernel reads it without a length (the upsamplers, conv_post): modes 1 / 2 accumulate into
 * it, mode 0 leaves it.  A value <= 0 means the whole row, a larger one is clamped to len inside the kernel (a wrong table gives
 * wrong audio, never an access outside the row); row_frames = NULL: every row full — the same results as the plain entry point, bit for
 * bit.  row_stride and spf must be positive.  Everything else as the entry point of the same name. */
int ttsk_hifi_conv_pair_rowlen(const void* x16, const void* w1_pack, const float* bias1, const void* w2_pack, const float* bias2, void* out16,
                             int f16, int B, int len, int C, int K, int dil, float slope, int mode, float scale, float final_slope,
                             const int32_t* row_frames, int row_stride, int spf, void* stream);
int ttsk_hifi_conv_pair_ws_rowlen(const void* x16, const void* w1_pack, const float* bias1, const void* w2_pack, const float* bias2,
                                void* out16, int f16, int B, int len, int C, int K, int dil, float slope, int mode, float scale,
                                float final_slope, int max_wgs, const int32_t* row_frames, int row_stride, int spf, void* stream);
int ttsk_hifi_resblock2_rowlen(const void* x16, const void* w0_pack, const float* bias0, const void* w1_pack, const float* bias1, void* out16,
                             int f16, int B, int len, int C, int K, int d0, int d1, float slope, int mode, float scale, float final_slope,
                             const int32_t* row_frames, int row_stride, int spf, void* stream);
int ttsk_hifi_resblock1_rowlen(const void* x16, void* out16, int f16, const void* const* weights, const float* const* biases,
                             const int32_t* dilations, int B, int len, int C, int K, int mode, float scale, float slope,
                             float final_slope, const int32_t* row_frames, int row_stride, int spf, void* stream);
/* (out past a row's edge is not written: those samples belong to no utterance and ttsk_wav_stitch keeps none of them) */
int ttsk_hifi_mrf32_post_rowlen(const void* x16, float* out, void* stage_out16, int f16, const void* const* weights,
                              const float* const* biases, const int32_t* dilations, const void* w_post16, const float* b_post, int B,
                              int len, int C, int k0, int k1, int k2, int k_post, float slope, float final_slope, float scale,
                              const int32_t* row_frames, int row_stride, int spf, void* stream);
/* x16 (B, len, C) 16-bit, C a multiple of 8: the positions of row b from row_frames[b * row_stride] * spf on are set to zero (same
 * clamping; NULL: nothing to do).  The short-row route's fill behind conv_pre, whose activated output the first upsampler reads. */
int ttsk_zero_rows_past(void* x16, int B, int len, int C, const int32_t* row_frames, int row_stride, int spf, void* stream);

/* rows (u, t) with t >= frame_limit[0] of x [rows][C] (elem_bytes 2 or 4, row = u*seg_len + t) are set to zero: the mel
 * frames / mel gradients past the batch's own longest utterance under shape-bucketed training (see BatchNorm below). */
int ttsk_zero_frames_from(void* x, int elem_bytes, int rows, int C, int seg_len, const int32_t* frame_limit, void* stream);

/* the per-utterance form (batched synthesis): rows (u, t) with t >= lens[u] (int64, clamped to [0, seg_len]) are set to zero. */
int ttsk_zero_frames_lens(void* x, int elem_bytes, int rows, int C, int seg_len, const int64_t* lens, void* stream);

/* ------------------------------------------------------------------------------------- PostNet BatchNorm1d
 * reference: fs_two/transformer/Layers.py:133-143 — training statistics over ALL rows (PAD rows included),
 * eps 1e-5, momentum 0.1, running_var updated with the unbiased variance; tanh (all but the last layer) and
 * F.dropout(0.5) follow; the last layer adds the mel residual (fastspeech2.py:104).
 * x (the conv output) may be fp32: channels whose batch std is far below their mean amplify a bf16 rounding of x
 * by mean/std, so the model keeps x in fp32 (x_is_f32 = 1).
 * frame_limit (device int32[1], may be NULL) + seg_len: rows are (utterance, frame) pairs, row = u*seg_len + t; frames
 * t >= frame_limit[0] do not exist in the reference's batch (shape-bucketed training pads T up to a multiple of 32 so that
 * hipGraphs repeat; the reference pads to the batch's own longest utterance): they are left out of the statistics and of
 * the row count, are written as zero rows (the next convolution's zero padding) and carry no gradient.
 */
int ttsk_bn_nblocks(int rows);
int ttsk_bn_stats(const void* x, int x_is_f32, int rows, int C, float* partials /* [nblocks][2C] */, const int32_t* frame_limit,
                  int seg_len, void* stream);
int ttsk_bn_finalize(const float* partials, int nblk, int C, int rows, float eps, float momentum, float* mean, float* rstd,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked, const int32_t* frame_limit, int seg_len,
                     void* stream);
int ttsk_rsqrt_eps(const float* var, float eps, float* rstd, int n, void* stream);
/* The training path in two launches per direction instead of three.  A workgroup owns a slab of channels (64, or all C when C is
 * not a multiple of 64; then C <= 128) and one of ttsk_bn_nchunks(rows) <= 64 row chunks, so there are few partial rows whatever
 * the grid; ttsk_bn_train_apply / ttsk_bn_bwd_apply_slab sum them for their own slab (fixed order, double) instead of waiting
 * for ttsk_bn_finalize / a column-sum launch.  ttsk_bn_train_apply = ttsk_bn_finalize (mean, rstd, running statistics,
 * num_batches_tracked: all written) + ttsk_bn_apply; ttsk_bn_bwd_apply_slab = the column sums + ttsk_bn_bwd_apply.
 * partials: [nblk][2C]; any producer of such rows will do (nblk need not be ttsk_bn_nchunks).
 * keep_out / keep (may be NULL): uint8 [rows][C/4], bit e of a byte = channel 4*q + e was kept by the dropout; written by the
 * forward and read by the two backward kernels instead of regenerating the Philox mask twice (NULL: they regenerate it). */
int ttsk_bn_nchunks(int rows);
int ttsk_bn_stats_slab(const void* x, int x_is_f32, int rows, int C, float* partials /* [nchunks][2C] */, const int32_t* frame_limit,
                       int seg_len, void* stream);
int ttsk_bn_train_apply(const void* x, int x_is_f32, const float* partials, int nblk, float eps, float momentum, float* mean,
                        float* rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* gamma,
                        const float* beta, int rows, int C, int use_tanh, float p, uint32_t site, const uint64_t* rng,
                        const float* resid_f32, void* out_bf16, float* out_f32, uint8_t* keep_out, const int32_t* frame_limit,
                        int seg_len, void* stream);
int ttsk_bn_bwd_stats_slab(const void* dout, int dout_is_f32, const void* x, int x_is_f32, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, int rows, int C, int use_tanh, float p, uint32_t site,
                           const uint64_t* rng, const uint8_t* keep, float* partials /* [nchunks][2C] */,
                           const int32_t* frame_limit, int seg_len, void* stream);
int ttsk_bn_bwd_apply_slab(const void* dout, int dout_is_f32, const void* x, int x_is_f32, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, int rows, int C, int use_tanh, float p, uint32_t site,
                           const uint64_t* rng, const uint8_t* keep, const float* partials, int nblk, void* dx_bf16, float* dgamma,
                           float* dbeta, int accumulate /* 1: dgamma / dbeta += ; 0: = */, const int32_t* frame_limit, int seg_len,
                           void* stream);
int ttsk_bn_apply(const void* x, int x_is_f32, const float* mean, const float* rstd, const float* gamma, const float* beta, int rows,
                  int C, int use_tanh, float p, uint32_t site, const uint64_t* rng, const float* resid_f32, void* out_bf16,
                  float* out_f32, const int32_t* frame_limit, int seg_len, void* stream);
/* inference BatchNorm-apply of the batched synthesis: ttsk_bn_apply's arithmetic without dropout; frames t >= lens[u] (int64
 * [rows / seg_len], clamped to [0, seg_len]) come out as zero rows, so the next PostNet convolution meets the zero padding a
 * solo run of utterance u has past its last frame (Layers.py:133-143). */
int ttsk_bn_apply_lens(const void* x, int x_is_f32, const float* mean, const float* rstd, const float* gamma, const float* beta,
                       int rows, int C, int use_tanh, const float* resid_f32, void* out_bf16, float* out_f32, const int64_t* lens,
                       int seg_len, void* stream);
int ttsk_bn_bwd_stats(const void* dout, int dout_is_f32, const void* x, int x_is_f32, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int rows, int C, int use_tanh, float p, uint32_t site,
                      const uint64_t* rng, float* partials /* [nblocks][2C]: sum dy | sum dy*xhat */, const int32_t* frame_limit,
                      int seg_len, void* stream);
int ttsk_bn_bwd_apply(const void* dout, int dout_is_f32, const void* x, int x_is_f32, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int rows, int C, int use_tanh, float p, uint32_t site,
                      const uint64_t* rng, const float* sums /* [2C] */, void* dx_bf16, float* dgamma, float* dbeta,
                      int accumulate /* 1: dgamma / dbeta += ; 0: = */, const int32_t* frame_limit, int seg_len, void* stream);

/* ------------------------------------------------------------------------------------------------- loss
 * reference: fs_two/model/loss.py:24-134 (use_cwt False).  losses[8] = {total, mel_total, pitch, energy, duration,
 * 0, 0, n_valid_phonemes}; gradients of grad_scale*total: dmel_sum = d/dmel + d/dpost (postnet adds mel back),
 * dpost, dpitch, denergy, dlogd.  partials: [ttsk_fs2_loss_nblocks()][6] fp32.
 * frame_limit (device int32[1], may be NULL): the mel terms are means over B * frame_limit[0] * n_mel elements instead of
 * B * T * n_mel — the reference's denominator when the batch was padded beyond its own longest utterance (see BatchNorm).
 */
int ttsk_fs2_loss_nblocks(void);
int ttsk_fs2_loss(const float* mel, const float* post, const float* mel_target, const int64_t* mel_lens, const float* pitch,
                  const float* energy, const float* logd, const float* pitch_target, const float* energy_target,
                  const int64_t* dur_target, const int64_t* src_lens, int B, int T, int T_target, int n_mel, int L,
                  float grad_scale, float* dmel_sum, float* dpost, float* dpitch, float* denergy, float* dlogd,
                  float* partials, float* losses, const int32_t* frame_limit, void* stream);
/* The same loss as three launches (a `partials` buffer per half: each stream writes memory of its own; they may be one buffer), for a step whose variance predictors run on a stream of their own: the
 * frame-level terms (loss.py:57-77: mel MSE + L1, postnet L1) and dmel_sum / dpost read nothing of the predictors; the phoneme-level terms
 * (loss.py:79-99) and dpitch / denergy / dlogd nothing of the decoder; ttsk_fs2_loss_finalize turns both sets of partial rows into
 * losses[8] wherever both are visible.  Same grid and per-thread order as ttsk_fs2_loss: bit-identical losses and gradients. */
int ttsk_fs2_loss_mel(const float* mel, const float* post, const float* mel_target, const int64_t* mel_lens, int B, int T, int T_target,
                      int n_mel, float grad_scale, float* dmel_sum, float* dpost, float* partials, const int32_t* frame_limit, void* stream);
int ttsk_fs2_loss_var(const float* pitch, const float* energy, const float* logd, const float* pitch_target, const float* energy_target,
                      const int64_t* dur_target, const int64_t* src_lens, int B, int L, float grad_scale, float* dpitch, float* denergy,
                      float* dlogd, float* partials, void* stream);
int ttsk_fs2_loss_finalize(const float* partials_mel, const float* partials_var, const int64_t* src_lens, int B, int T, int n_mel,
                           const int32_t* frame_limit, float* losses, void* stream);

/* ------------------------------------------------------------------------------------------- optimiser
 * reference: train.py:47-54, fs_two/model/optimizer.py:5-53, torch.optim.Adam.
 * `state` is a device block of ttsk_optim_state_bytes() bytes:
 *   { int64 sched_step; int64 adam_t; uint64 rng_seed; uint64 rng_step; float lr, bc1, bc2, clip_coef, gnorm; ... }
 * (its address + 16 is the `rng` pointer handed to the dropout kernels).
 *
 * ttsk_optim_step is the whole update as TWO launches over the flat buffers (n % 4 == 0; partials: 1024 floats), with no atomics and no
 * host synchronisation: capturable.  What it covers is given by three device tables.
 *   dev_ranges [n_ranges][3] (int64, ascending, disjoint): {start, end, sum of (end - start) / 4 over the ranges before this one}, every
 *     start / end a multiple of 4; range_floats = their total.  One range {0, n, 0} is the whole model; several are the trainable
 *     stretches when some parameter groups are frozen (speaker adaptation; torch: requires_grad_(False) on the rest — clip_grad_norm_
 *     and Adam then skip them).  n_ranges == 0 is an error.
 *   dev_items [n_items] (ttsk_adam_item, sorted by tile0): the window kernels' packed weights INSIDE the ranges — tap-major storage
 *     (Cs, K, Ds) at element offset `off` of the flat buffers, Ds % 256 == 0 and Cs % 32 == 0, its plain pack (`pack`, the weight as
 *     it is: Cout = Cs, Cin = Ds) and / or its transposed, tap-flipped pack (`pack_t`: Cout = Ds, Cin = Cs), either may be NULL; a
 *     tile = 32 storage rows x 256 storage columns of one tap, item i owns tiles [tile0, tile0 + K * (Cs/32) * (Ds/256)).
 *   dev_gaps [n_gaps][3] (int64): the layout of dev_ranges, for the parts of the ranges outside every item; gap_floats = their total,
 *     and n_tiles * 8192 + gap_floats must equal range_floats.
 *   n_items == 0 (then dev_items, dev_gaps NULL and n_tiles, n_gaps, gap_floats 0): launch 2 walks dev_ranges.
 * Launch 1 sums g^2 over the ranges only (one fixed slot of `partials` per workgroup, a fixed order: equal inputs give equal bits) and
 * advances the counters on device (graph-replay safe): ++sched_step, ++adam_t, lr / bc1 / bc2 recomputed, and ++rng_step when
 * advance_rng (ttsk_rng_advance folded in).  Launch 2 derives ||g|| -> clip_coef = min(1, max_norm / (||g|| + 1e-6)) from those partials
 * in every workgroup, applies Adam, writes the bf16 weight shadow and (zero_grad) zeroes the gradients — over the elements of the ranges
 * only: elements outside them are neither read nor written in any of the five buffers, and the bytes moved are proportional to
 * range_floats.  state.gnorm is the norm over the ranges.  The workgroup that updates a tile of an item also writes that tile's
 * fragments of the item's packs, bit-identical to ttsk_win_conv_pack_table run on the shadow afterwards; packs of weights that are no
 * item are not touched.
 */
int ttsk_optim_state_bytes(void);
int ttsk_rng_advance(void* state, void* stream);
/* The keep-mask of dropout site `site` at the state `rng` points to ({uint64 seed, uint64 step}): keep[e] = 1 iff element e (row-major
 * index into the site's [rows][C] tensor) survives with drop probability p — the very function of (seed, step, site, e) every kernel of
 * the step evaluates (masks are regenerated, never stored).  Sites of the FS2 step: encoder block i: 2 i (fc), 2 i + 1 (w_2); decoder
 * block i: 100 + 2 i, 101 + 2 i; predictor g in (duration, pitch, energy): 200 + 2 g, 201 + 2 g; PostNet layer i: 300 + i
 * (reference sites: SubLayers.py:62,98; modules.py:283,295; Layers.py:137-140).  n % 4 == 0.  For parity tests. */
int ttsk_dropout_keep_mask(const uint64_t* rng, uint32_t site, int64_t n, float p, uint8_t* keep, void* stream);
typedef struct ttsk_adam_item {
  int64_t off;
  void* pack;
  void* pack_t;
  int32_t Cs, K, Ds, tile0;
} ttsk_adam_item;
int ttsk_optim_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t n, void* state,
                    float* partials, float max_norm, float beta1, float beta2, float eps, int zero_grad, float d_model, float warmup,
                    const float* anneal_steps_host, int n_anneal, float anneal_rate, int advance_rng,
                    const int64_t* dev_ranges, int n_ranges, int64_t range_floats,
                    const ttsk_adam_item* dev_items, int n_items, int n_tiles, const int64_t* dev_gaps, int n_gaps,
                    int64_t gap_floats, void* stream);

/* Weight gradient of a Conv1d with K taps ("same" zero padding, dilation 1) as a kernel of its own (csrc/dwconv.hip):
 *   dw[co][tap][ci] (+)= sum_b sum_{t < len_b} dy[(b*S + t)*ldy + co] * x[(b*S + t + tap - K/2)*ldx + ci],   0 <= t + tap - K/2 < S
 * dy / x bf16 rows of B utterances x S rows, dw fp32 (Cout, K, Cin) — the tap-major storage of the flat gradient buffer; lens (int64
 * [B], may be NULL = S): rows t >= lens[b] of dy are not walked (PAD rows carry no gradient: fs_two/transformer/Layers.py:29,32).
 * One launch for up to 12 problems of the same K.  Replaces the K batched problems per weight that ttsk_gemm_group_* ran for
 * torch's conv weight gradient (reference call sites: SubLayers.py:96 w_1 with K = 9, Layers.py:85-129 PostNet with K = 5). */
typedef struct ttsk_dwconv_item {
  const void* dy;
  const void* x;
  float* dw;
  const int64_t* lens;
  int32_t Cout, Cin, K, ldy, ldx, B, S, accumulate;
} ttsk_dwconv_item;
int ttsk_dwconv_supported(int Cout, int Cin, int K);
int ttsk_dwconv_batch(const ttsk_dwconv_item* items, int n /* <= 12 */, void* stream);

/* The same weight gradient for Cout and Cin multiples of 256 (a Linear's or a k = 1 conv's: K = 1; or a conv with taps) on the
 * 256 x 256-tile kernel of csrc/dwgemm.hip — one workgroup per (output tile, tap, utterance range): up to 28 problems per launch.
 * splits > 1 cuts the utterances into `splits` ranges whose partial sums go to `workspace` (fp32 [splits][K][Cout][Cin],
 * ttsk_dwgemm_workspace_floats) — the slab layout of ttsk_reduce_item {ws, C = dw, M = Cout, N = Cin, ldc = K*Cin, nz = K, splits,
 * accumulate, sC2 = Cin}: run ttsk_gemm_reduce_batch behind it; splits = 1 writes / accumulates dw directly.
 * reference call sites: SubLayers.py:41-43,62 (w_qs | w_ks | w_vs, fc), :97 (w_2), Layers.py:85-129 (PostNet convs). */
typedef struct ttsk_dwgemm_item {
  const void* dy;
  const void* x;
  float* dw;
  float* workspace;
  const int64_t* lens;
  int32_t Cout, Cin, K, ldy, ldx, B, S, accumulate, splits;
} ttsk_dwgemm_item;
int ttsk_dwgemm_supported(int Cout, int Cin, int K);
int64_t ttsk_dwgemm_workspace_floats(int Cout, int Cin, int K, int splits);
/* max_wgs > 0: at most that many workgroups, each walking several tiles (one per CU on part of the chip, the rest left to a concurrent stream) */
int ttsk_dwgemm_batch(const ttsk_dwgemm_item* items, int n /* <= 28 */, int max_wgs, void* stream);

/* ------------------------------------------------------------------------------------------- CWT pitch branch
 * model_config.use_cwt: True.  reference: fs_two/model/modules.py:18-141 (get_pitch_embedding_cwt), :358-385 (CNNflat / CNNscalar),
 * fs_two/cwt/cwt_utils.py:41-66 (inverse_batch_cwt), fs_two/model/loss.py:65-124.  fp32 arithmetic in a fixed summation order
 * (no atomics): equal inputs give equal bits in every process.  Nothing here synchronises with the host.
 *
 * ttsk_layernorm_head_fwd / _bwd: the pitch predictor's tail with its 11 outputs — ttsk_layernorm_fwd's head mode
 *   (LayerNorm -> dropout_{p_post, site_post} -> Linear -> PAD mask, same dropout bits at the same (rng, site)) for
 *   Linear(256 -> 11): head_w [11][256], head_b [11], head_out [rows][11]; D = 256 and n_out = 11 only.  y is the LayerNorm input
 *   (no residual, no pre-dropout); the backward takes it again as z, gates dz with the ReLU that produced it (z > 0) and writes
 *   partials [ttsk_layernorm_head_bwd_nblocks(rows)][14 * 256 + 11] = dbias | dgamma | dbeta | dhead_w | dhead_b, the order of the
 *   flat gradient buffer (ttsk_colsum_finalize sums the blocks).
 * ttsk_cnnscalar_fwd / _bwd: BOTH CNNscalar heads (pitch_mean, pitch_std) in one launch, one workgroup per utterance:
 *   two 1x1 convs over the time axis (x [B][L][256] bf16 and cwt [B][L][11] fp32), AdaptiveAvgPool1d(30) over the padded length L
 *   (bins [floor(i L / 30), ceil((i + 1) L / 30))), LayerNorm(30), ReLU, sum, Linear(30, 1), ReLU -> out [2][B] (mean row, std row).
 *   params: the two heads' parameter blocks back to back, TTSK_CNNSCALAR_FLOATS floats each, every tensor at a multiple of 8 floats in
 *   state_dict order: flat_one.net.0.weight [256] @0, .bias @256, net.2.weight [30] @264, net.2.bias @296, flat_two.net.0.weight [11]
 *   @328, .bias @344, net.2.weight @352, net.2.bias @384, linear.weight [30] @416, linear.bias @448.
 *   Saved for the backward: pooled [B][4][30] (row = head * 2 + flat), stats [B][4][2] (mean, rstd), pre [B][2]; rowdot [B][4][L] is
 *   workspace for both directions.  The backward turns dout [2][B] into partials [B][2 * TTSK_CNNSCALAR_FLOATS] (same layout, gaps
 *   zero), one row per utterance — ttsk_colsum_finalize sums them over B in order.  No input gradients: the reference detaches both
 *   inputs.
 * ttsk_cwt_pitch: s[b][l] = sum_{i<10} cwt[b][l][i] * (i + 3.5)^-2.5; per column l over ALL B rows: z = (s - mean) / (std + 1e-12)
 *   (population std, two passes, B = 1 and all-PAD columns give exactly 0); pitch = z * heads[1][b] + heads[0][b], computed in fp64
 *   and rounded to fp32 once (1 / std amplifies fp32 rounding of s and of the mean); idx = #{bins < pitch * p_control}
 *   (ttsk_bucketize's rule).
 * ttsk_fs2_loss_cwt: runs BEHIND ttsk_fs2_loss on the same stream (which must have been given a pitch term of zero): masked
 *   11-channel MSE (mean over 11 * sum(src_lens)) and the two [B] MSEs; losses[0] += their sum, losses[2] / [5] / [6] = pitch / mean /
 *   std terms; dcwt [B][L][11] and dheads [2][B] are gradients of grad_scale * total.
 */
#define TTSK_CWT_CHANNELS 11
#define TTSK_CNNSCALAR_BINS 30
#define TTSK_CNNSCALAR_FLOATS 456
int ttsk_layernorm_head_bwd_nblocks(int rows);
int ttsk_layernorm_head_fwd(const void* y_bf16, const float* gamma, const float* beta, const int64_t* lens, int seg_len, int rows, int D,
                            int n_out, float eps, float p_post, uint32_t site_post, const uint64_t* rng, const float* head_w,
                            const float* head_b, float* mean, float* rstd, float* head_out, void* stream);
int ttsk_layernorm_head_bwd(const float* dhead, const float* head_w, const void* z_bf16, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, const int64_t* lens, int seg_len, int rows, int D, int n_out,
                            float p_post, uint32_t site_post, const uint64_t* rng, void* dz_bf16, float* partials, void* stream);
int ttsk_cnnscalar_fwd(const void* x_bf16, const float* cwt, const float* params, int B, int L, int D, float* rowdot, float* pooled,
                       float* stats, float* pre, float* out, void* stream);
int ttsk_cnnscalar_bwd(const float* dout, const void* x_bf16, const float* cwt, const float* params, const float* pooled,
                       const float* stats, const float* pre, int B, int L, int D, float* rowdot, float* partials, void* stream);
int ttsk_cwt_pitch(const float* cwt, const float* heads, const float* bins, int n_bins, float p_control, int B, int L, float* pitch,
                   int32_t* idx, void* stream);
int ttsk_fs2_loss_cwt(const float* cwt, const float* cwt_target, const float* heads, const float* mean_target, const float* std_target,
                      const int64_t* src_lens, int B, int L, float grad_scale, float* dcwt, float* dheads, float* losses, void* stream);

/* ------------------------------------------------------------------------------------------- mel extraction
 * SURVEY.md §8 row f-3.  reference: hifi/meldataset.py:49-74 (mel_spectrogram), fs_two/audio/stft.py:57-90
 * (STFT.transform: strided conv with a windowed Fourier basis), :174-193 (TacotronSTFT.mel_spectrogram).
 * The contraction is a ttsk_gemm conv (taps = n_fft/hop over rows of `hop` samples); these are the kernels around it.
 * stft_frames: wav (B, len) fp32 -> hop-block rows out16 fp16 (B, rows, 3*hop) = [hi | hi | lo]: reflect padding by `pad`
 *   samples on both sides, zeros past len + 2*pad, value*scale split as hi + lo (fp16 each); against a basis laid out
 *   [hi | lo | hi] per tap one contraction gives hi*hi + hi*lo + lo*hi.  hop % 8 == 0, pad < len.
 * mel_from_spec: spec (B*rows, ld) fp32 with Re in columns [0, nbins) and Im in [nbins, 2*nbins) ->
 *   mel (B, n_mels, T) = log(max(basis . sqrt(re^2 + im^2 + eps), clip)), energy (B, T) = sqrt(sum re^2 + im^2).
 *   The filterbank is passed packed: filter m = basis_vals[basis_off[m] .. basis_off[m+1]) applied to bins
 *   basis_start[m] ..; nnz = basis_off[n_mels].  nbins <= 1088, n_mels <= 80. */
int ttsk_stft_frames(const float* wav, void* out16, int B, int len, int pad, int rows, int hop, float scale, void* stream);
int ttsk_mel_from_spec(const float* spec, int ld, const float* basis_vals, const int32_t* basis_start,
                       const int32_t* basis_off, int nnz, float* mel, float* energy, int B, int rows, int T, int nbins,
                       int n_mels, float eps, float clip, void* stream);

/* ------------------------------------------------------------------------------- pitch and phoneme-level prosody
 * Data preparation for the FS2 trainer.  reference: fs_two/preprocessor/preprocessor.py:206-266.
 * pitch_yin: F0 per frame by YIN (de Cheveigne & Kawahara 2002, steps 1-5).  NOT DIO: the values differ from pyworld's.
 *   wav (B, ld) fp32; lens int32[B] or null (every row has ld samples); samples at or past a row's len are never read.
 *   f0 (B, T_max) fp32 with T_max = 1 + ld / hop; row b has T = 1 + len / hop frames, the others are written as 0.
 *   Frame t, S = W + tau_max: s0 = clamp(t * hop - S / 2, 0, max(len - S, 0)), x[j] = wav[s0 + j] (0 from len on), j < S;
 *   d(tau) = sum_{j < W} (x[j] - x[j + tau])^2 in fp32, direct form, in an order that depends on (W, tau_max) only;
 *   d'(tau) = d(tau) * tau / sum_{k = 1 .. tau} d(k), 1 where that sum is 0; the first tau in [tau_min, tau_max) with
 *   d'(tau) < thr, walked on while tau + 1 < tau_max and d'(tau + 1) < d'(tau); none: f0 = 0 (unvoiced);
 *   off = 0.5 (a - c) / (a - 2 b + c) over d'(tau - 1 .. tau + 1), 0 when the denominator is 0 or |off| > 1; f0 = sr / (tau + off).
 *   Needs W % 4 == 0, 2 <= tau_min, tau_min + 1 < tau_max <= 1023, W + tau_max <= 8192.
 * phoneme_prosody: one row per utterance: f0, energy (B, ldT) fp32, dur (B, ldL) int32, T[B] frames and Lp[B] phonemes.
 *   n = sum dur.  status (int32): 2 when n > T (or a duration is negative), 1 when at most one of the first n frames of f0 is
 *   non-zero, 3 when the standard deviation below is 0, else 0; a row with a non-zero status writes zeros.
 *   Unvoiced (zero) frames are interpolated linearly between their voiced neighbours; before the first voiced frame its value is
 *   held, after the last likewise.  pitch[i] = (log(mean of f0 over phoneme i's frames) - pitch_mean) / pitch_std with the mean
 *   and population standard deviation of those logs over the utterance; energy_ph[i] = mean of energy over the frames.  A phoneme
 *   with dur = 0 stores 0 for both and is left out of the statistics (the reference takes log 0 there).  Entries from Lp[b] to
 *   ldL are written as 0.  ldT <= 8192, ldL <= 1024. */
int ttsk_pitch_yin(const float* wav, const int32_t* lens, int B, int ld, int hop, int W, int tau_min, int tau_max, float sr, float thr,
                   float* f0, int T_max, void* stream);
int ttsk_phoneme_prosody(const float* f0, const float* energy, int ldT, const int32_t* dur, int ldL, const int32_t* T, const int32_t* Lp,
                         int B, float* pitch, float* energy_ph, float* pitch_mean, float* pitch_std, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------- forced alignment: dynamic time warping
 * One launch aligns B pairs of feature sequences.
 *   x (B, ldx, C) fp32 and y (B, ldy, C) fp32, contiguous; x_lens, y_lens int32[B] or null (every row is full).  Tx, Ty are the
 *   lengths clamped to [0, ld]; rows at or past a pair's length are never read.
 *   Local cost: D(i, j) = sum_c (x[i, c] - y[j, c])^2 in fp32.
 *   Cumulative cost: A(0, 0) = D(0, 0); A(i, j) = D(i, j) + min over the predecessors that exist, taken in the order (i-1, j-1),
 *   (i-1, j), (i, j-1): a later candidate replaces an earlier one only if it is strictly smaller (on a tie the earliest wins).
 *   Path: walked back from (Tx-1, Ty-1) to (0, 0) along the chosen predecessors.
 *   Outputs: path_x (B, ldy) int32: for j < Ty the largest i with (i, j) on the path, -1 from Ty on; cost[B] fp32 = A(Tx-1, Ty-1);
 *   status[B] int32.
 *   Durations, written when both x_seg and dur are given: x_seg (B, ldL) int32 are the frames of x per phoneme, n_seg int32[B] the
 *   phonemes per row (null: ldL); dur (B, ldL) int32: dur[b, l] = the number of j < Ty whose path_x[j] lies in phoneme l's span of
 *   x.  A phoneme with x_seg = 0 gets 0, entries from n_seg[b] on are 0, and sum_l dur = Ty.
 *   status: 0 good; 2: Tx < 1 or Ty < 1 (path_x = -1, dur = 0, cost = +inf); 3: x_seg has a negative entry or does not sum to Tx
 *   (dur = 0; path_x and cost are written as usual).  A non-finite cost is left for the caller to judge.
 *   Limits, refused before any launch: 1 <= C <= 128; 1 <= ldx, ldy <= 2048; 1 <= ldL <= 1024; 0 <= B <= 65535 (B = 0 launches
 *   nothing).  workspace: ttsk_dtw_workspace_bytes(B, ldx, ldy) bytes, 16-byte aligned (the local costs and one byte of
 *   back-pointer per cell, both skewed by anti-diagonal); -1 for sizes outside the limits. */
int64_t ttsk_dtw_workspace_bytes(int B, int ldx, int ldy);
int ttsk_dtw_align(const float* x, const float* y, const int32_t* x_lens, const int32_t* y_lens, int B, int ldx, int ldy, int C,
                   const int32_t* x_seg, const int32_t* n_seg, int ldL, void* workspace, int64_t workspace_bytes, int32_t* path_x,
                   float* cost, int32_t* status, int32_t* dur, void* stream);

/* ------------------------------------------------------------------------------- Griffin-Lim: STFT, inverse STFT, iteration
 * DESIGN.md section 21.  reference: fs_two/audio/stft.py:57-137 (STFT.transform / STFT.inverse),
 * fs_two/audio/audio_processing.py:66-82 (griffin_lim), fs_two/audio/tools.py:18-25 (inv_mel_spec's mel-to-linear map).
 * All fp32, an FFT in LDS.  n_fft a power of two in 64..2048, hop divides n_fft, 1 <= B <= 65535.
 * window: n_fft floats (the analysis and synthesis window, centre-padded by the caller); twiddle: n_fft / 2 pairs
 * (cos, -sin)(2 pi k / n_fft), built in fp64 and rounded once.  nbins = n_fft / 2 + 1.
 * stft_polar: wav (B, len) -> mag, phase (B, nbins, T), T = 1 + len / hop, len > n_fft / 2: reflect padding by n_fft / 2, frame t
 *   starts at padded sample t * hop, window, real FFT, phase = atan2f(im, re).  lens int32[B] or null: samples per row; a row
 *   reflects about its own end, has 1 + lens[b] / hop frames and zeros in the others (all of them when lens[b] <= n_fft / 2).
 * istft_frames: mag, phase with element (b, k, t) at b * sB + k * sk + t * st -> frames_out (B, T, n_fft): the inverse real FFT of
 *   mag * (cos, sin)(phase), imaginary parts of bins 0 and n_fft / 2 ignored, times the window.  frames int32[B] or null: frames
 *   per row; the frames past a row's count are neither read nor written.
 * istft_ola: frames_in (B, T, n_fft) -> wav (B, hop * (T - 1)): sample j = sum over the frames t < frames[b] covering padded
 *   sample p = j + n_fft / 2, in ascending t, of frames_in[t][p - t * hop], divided by sum_t window^2[p - t * hop] where that
 *   exceeds float32 tiny; zeros from hop * (frames[b] - 1) on.  A gather: no atomics, a row depends on nothing but itself.
 * istft: istft_frames into workspace (B * T * n_fft floats), then istft_ola: the reference's STFT.inverse.
 * griffinlim_step: one iteration.  Source: wav (B, ld_wav) rows of hop * (frames[b] - 1) samples, or frames_in, the previous
 *   step's frames_out, read through istft_ola's sum (exactly one of the two; frames_in != frames_out).  Z = STFT(source);
 *   A = Z - momentum / (1 + momentum) * zprev and zprev <- Z when momentum > 0 (zprev (B, T, nbins) complex pairs; momentum
 *   = 0 never touches it); bin <- mag * A / |A|, (mag, 0) where |A| == 0; inverse FFT, window -> frames_out.
 *   hop * (T - 1) > n_fft / 2; a row with hop * (frames[b] - 1) <= n_fft / 2 is skipped.
 * mel_to_spec: log-mel (B, n_mels, T) -> spec (B, nbins, T) = scale * sum_m exp(mel[m]) * fb[m][k] with the filterbank packed
 *   as for mel_from_spec (filters summed in ascending m; a bin no filter covers is exactly 0). */
int ttsk_stft_polar(const float* wav, const int32_t* lens, int B, int len, int n_fft, int hop, const float* window,
                    const float* twiddle, float* mag, float* phase, int T, void* stream);
int ttsk_istft_frames(const float* mag, const float* phase, int64_t sB, int64_t sk, int64_t st, const int32_t* frames, int B,
                      int T, int n_fft, int hop, const float* window, const float* twiddle, float* frames_out, void* stream);
int ttsk_istft_ola(const float* frames_in, const int32_t* frames, int B, int T, int n_fft, int hop, const float* window,
                   float* wav, void* stream);
int ttsk_istft(const float* mag, const float* phase, int64_t sB, int64_t sk, int64_t st, const int32_t* frames, int B, int T,
               int n_fft, int hop, const float* window, const float* twiddle, float* workspace, float* wav, void* stream);
int ttsk_griffinlim_step(const float* wav, int64_t ld_wav, const float* frames_in, const float* mag, int64_t sB, int64_t sk,
                         int64_t st, const int32_t* frames, float* zprev, float momentum, int B, int T, int n_fft, int hop,
                         const float* window, const float* twiddle, float* frames_out, void* stream);
int ttsk_mel_to_spec(const float* mel, const float* basis_vals, const int32_t* basis_start, const int32_t* basis_off, int B,
                     int n_mels, int nbins, int T, float scale, float* spec, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTSK_H */
