// cwt.hip — the CWT pitch branch of the variance adaptor (model_config.use_cwt: True).
// reference: fs_two/model/modules.py:18-141 (VariancePredictor(output_size=11), get_pitch_embedding_cwt), :358-385 (CNNflat /
// CNNscalar), fs_two/cwt/cwt_utils.py:41-66 (inverse_batch_cwt + the batch-axis standard scaler), fs_two/model/loss.py:65-124.
// Everything here is fp32 arithmetic (the column statistics of cwt_pitch: fp64, see there) in a fixed summation order (wave64
// shuffles, LDS, sequential loops): no atomics, so two processes that see the same inputs produce the same bits.
//   ln_head_fwd / ln_head_bwd   LayerNorm + dropout + Linear(256 -> 11) + PAD mask of the pitch predictor, and its backward
//   cnn_heads_fwd / _bwd        both CNNscalar heads (pitch_mean, pitch_std), one workgroup per utterance
//   cwt_pitch                   10-channel weighted sum, batch-axis standardisation, * std + mean, bucketize
//   cwt_loss                    the three loss terms of the branch, added to ttsk_fs2_loss's values on the device
#include "common.h"
#include <math.h>

namespace {

constexpr int NH = TTSK_CWT_CHANNELS;   // 11 outputs of the pitch predictor
constexpr int NBIN = TTSK_CNNSCALAR_BINS;
// offsets (floats) of the ten tensors of one CNNscalar inside its parameter block: every tensor starts at a multiple of 8
constexpr int O_W1 = 0, O_B1 = 256, O_G1 = 264, O_BE1 = 296, O_W2 = 328, O_B2 = 344, O_G2 = 352, O_BE2 = 384, O_LW = 416, O_LB = 448;
static_assert(O_LB + 8 == TTSK_CNNSCALAR_FLOATS, "CNNscalar block layout");

__device__ __forceinline__ void load4(const bf16_t* p, float v[4]) {
  const uint2 u = *(const uint2*)p;
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xFFFF0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xFFFF0000u);
}
__device__ __forceinline__ void store4(bf16_t* p, const float v[4]) {
  *(uint2*)p = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
}

// ------------------------------------------------------------------------------------------ 11-wide predictor head
struct HeadArgs {
  const bf16_t* y;        // [rows][256] LayerNorm input (the second conv's ReLU output)
  const float* gamma; const float* beta;
  const long long* lens;  // [B]
  const uint64_t* rng;
  const float* head_w;    // [11][256]
  const float* head_b;    // [11]
  float* mean; float* rstd;   // [rows]
  float* head_out;        // [rows][11]
  int rows, seg_len;
  float p_post, eps;
  unsigned site_post;
};

__global__ __launch_bounds__(256) void ln_head_fwd_kernel(const HeadArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  constexpr int D = 256;
  const uint64_t seed = a.rng ? a.rng[0] : 0, step = a.rng ? a.rng[1] : 0;
  const int c = lane * 4;
  float z[4];
  load4(a.y + (int64_t)row * D + c, z);
  const float mean = wave_sum(z[0] + z[1] + z[2] + z[3]) / D;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { const float d = z[e] - mean; q += d * d; }
  const float rstd = rsqrtf(wave_sum(q) / D + a.eps);
  if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
  const int b = row / a.seg_len, t = row - b * a.seg_len;
  const bool masked = t >= a.lens[b];
  const f32x4 g = *(const f32x4*)(a.gamma + c), bt = *(const f32x4*)(a.beta + c);
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (z[e] - mean) * rstd * g[e] + bt[e];
  if (a.p_post > 0.f)
    drop4(o, keep4(seed, step, a.site_post, (unsigned)(((int64_t)row * D + c) >> 2), keep_threshold(a.p_post)), 1.f / (1.f - a.p_post));
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const f32x4 w = *(const f32x4*)(a.head_w + k * D + c);
    const float hs = wave_sum(o[0] * w[0] + o[1] * w[1] + o[2] * w[2] + o[3] * w[3]);
    if (lane == 0) a.head_out[(int64_t)row * NH + k] = masked ? 0.f : hs + a.head_b[k];
  }
}

struct HeadBwdArgs {
  const float* dhead;     // [rows][11]
  const float* head_w;    // [11][256]
  const bf16_t* z;        // [rows][256]
  const float* mean; const float* rstd;
  const float* gamma; const float* beta;
  const long long* lens;
  const uint64_t* rng;
  bf16_t* dz;             // [rows][256] gradient of the LayerNorm input, through the ReLU that produced it
  float* partials;        // [nblk][14 * 256 + 11]: dbias | dgamma | dbeta | dhead_w [11][256] | dhead_b [11]
  int rows, seg_len;
  float p_post;
  unsigned site_post;
};

constexpr int HB_WAVES = 4;
constexpr int HB_NCOL = (3 + NH) * 256 + NH;

__global__ __launch_bounds__(HB_WAVES * 64) void ln_head_bwd_kernel(const HeadBwdArgs a) {
  __shared__ float red[HB_WAVES][256];
  __shared__ float redb[HB_WAVES][NH];
  constexpr int D = 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t seed = a.rng ? a.rng[0] : 0, step = a.rng ? a.rng[1] : 0;
  const int c = lane * 4;
  float dg[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0}, dbias[4] = {0, 0, 0, 0};
  float dhw[NH][4];
  float dhb[NH];
#pragma unroll
  for (int k = 0; k < NH; ++k) { dhb[k] = 0.f; dhw[k][0] = dhw[k][1] = dhw[k][2] = dhw[k][3] = 0.f; }
  const f32x4 gm = *(const f32x4*)(a.gamma + c), bt = *(const f32x4*)(a.beta + c);
  for (int row = blockIdx.x * HB_WAVES + wave; row < a.rows; row += gridDim.x * HB_WAVES) {
    const int b = row / a.seg_len, t = row - b * a.seg_len;
    const bool masked = t >= a.lens[b];
    const float mean = a.mean[row], rstd = a.rstd[row];
    float zz[4];
    load4(a.z + (int64_t)row * D + c, zz);
    float xh[4], o[4], d[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) { xh[e] = (zz[e] - mean) * rstd; o[e] = xh[e] * gm[e] + bt[e]; }
    // the row's keep bits once, for the recomputed output and for its gradient
    const unsigned kpost = a.p_post > 0.f ? keep4(seed, step, a.site_post, (unsigned)(((int64_t)row * D + c) >> 2), keep_threshold(a.p_post)) : 0u;
    if (a.p_post > 0.f) drop4(o, kpost, 1.f / (1.f - a.p_post));
#pragma unroll
    for (int k = 0; k < NH; ++k) {
      const float dh = masked ? 0.f : a.dhead[(int64_t)row * NH + k];
      const f32x4 w = *(const f32x4*)(a.head_w + k * D + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) { d[e] += dh * w[e]; dhw[k][e] += dh * o[e]; }
      dhb[k] += dh;           // every lane carries the same sum; lane 0's is used
    }
    if (a.p_post > 0.f) drop4(d, kpost, 1.f / (1.f - a.p_post));
    float g[4], c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dg[e] += d[e] * xh[e];
      db[e] += d[e];
      g[e] = d[e] * gm[e];
      c1 += g[e];
      c2 += g[e] * xh[e];
    }
    c1 = wave_sum(c1) / D;
    c2 = wave_sum(c2) / D;
    float dzv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dzv[e] = zz[e] > 0.f ? rstd * (g[e] - c1 - xh[e] * c2) : 0.f;      // the ReLU in front of the LayerNorm
      dbias[e] += dzv[e];
    }
    store4(a.dz + (int64_t)row * D + c, dzv);
  }
  float* P = a.partials + (int64_t)blockIdx.x * HB_NCOL;
  for (int qn = 0; qn < 3 + NH; ++qn) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v;
      if (qn == 0) v = dbias[e];
      else if (qn == 1) v = dg[e];
      else if (qn == 2) v = db[e];
      else {
        v = 0.f;
#pragma unroll
        for (int k = 0; k < NH; ++k) if (qn == 3 + k) v = dhw[k][e];      // (static indexing keeps dhw in registers)
      }
      red[wave][c + e] = v;
    }
    __syncthreads();
    {
      const int cc = threadIdx.x;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < HB_WAVES; ++w) t += red[w][cc];
      P[qn * D + cc] = t;
    }
    __syncthreads();
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NH; ++k) redb[wave][k] = dhb[k];
  }
  __syncthreads();
  if (threadIdx.x < NH) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < HB_WAVES; ++w) t += redb[w][threadIdx.x];
    P[(3 + NH) * D + threadIdx.x] = t;
  }
}

// ------------------------------------------------------------------------------------------ CNNscalar heads
// AdaptiveAvgPool1d(30) bin i over a length-L axis: [floor(i L / 30), ceil((i + 1) L / 30))
__device__ __forceinline__ int bin_start(int i, int L) { return (int)(((int64_t)i * L) / NBIN); }
__device__ __forceinline__ int bin_end(int i, int L) { return (int)((((int64_t)(i + 1)) * L + NBIN - 1) / NBIN); }

struct CnnArgs {
  const bf16_t* x;        // [B][L][256] encoder output + speaker embedding
  const float* cwt;       // [B][L][11] pitch predictor output
  const float* params;    // two CNNscalar blocks back to back (pitch_mean, pitch_std), TTSK_CNNSCALAR_FLOATS each
  float* rowdot;          // [B][4][L] workspace: the 1x1 convs' outputs (forward) / their gradients (backward); q = head * 2 + flat
  float* pooled;          // [B][4][30]
  float* stats;           // [B][4][2] LayerNorm(30) mean, rstd
  float* pre;             // [B][2] Linear(30, 1) output before the last ReLU
  float* out;             // [2][B] forward result
  const float* dout;      // [2][B] (backward)
  float* partials;        // [B][2 * TTSK_CNNSCALAR_FLOATS] (backward)
  int B, L;
};

__global__ __launch_bounds__(256) void cnn_heads_fwd_kernel(const CnnArgs a) {
  __shared__ float sp[4][NBIN];       // pooled, then ReLU(LayerNorm)
  const int b = blockIdx.x, L = a.L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* P0 = a.params;
  const float* P1 = a.params + TTSK_CNNSCALAR_FLOATS;
  float* rd = a.rowdot + (int64_t)b * 4 * L;
  // (1) the 1x1 convs: a 256-wide dot of the row with each head's flat_one weight (one wave per row) ...
  const int c = lane * 4;
  const f32x4 w0 = *(const f32x4*)(P0 + O_W1 + c), w1 = *(const f32x4*)(P1 + O_W1 + c);
  for (int l = wave; l < L; l += 4) {
    float v[4];
    load4(a.x + ((int64_t)b * L + l) * 256 + c, v);
    const float s0 = wave_sum(v[0] * w0[0] + v[1] * w0[1] + v[2] * w0[2] + v[3] * w0[3]);
    const float s1 = wave_sum(v[0] * w1[0] + v[1] * w1[1] + v[2] * w1[2] + v[3] * w1[3]);
    if (lane == 0) { rd[0 * L + l] = s0 + P0[O_B1]; rd[2 * L + l] = s1 + P1[O_B1]; }
  }
  // ... and an 11-wide dot with each head's flat_two weight (one thread per row)
  for (int l = threadIdx.x; l < L; l += 256) {
    const float* cr = a.cwt + ((int64_t)b * L + l) * NH;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < NH; ++k) { const float v = cr[k]; s0 += v * P0[O_W2 + k]; s1 += v * P1[O_W2 + k]; }
    rd[1 * L + l] = s0 + P0[O_B2]; rd[3 * L + l] = s1 + P1[O_B2];
  }
  __syncthreads();        // (global writes of this workgroup are visible to it after the barrier)
  // (2) adaptive average pool over the padded length
  if (threadIdx.x < 4 * NBIN) {
    const int q = threadIdx.x / NBIN, i = threadIdx.x - q * NBIN;
    const int s = bin_start(i, L), e = bin_end(i, L);
    float t = 0.f;
    for (int l = s; l < e; ++l) t += rd[q * L + l];
    t /= (float)(e - s);
    sp[q][i] = t;
    a.pooled[((int64_t)b * 4 + q) * NBIN + i] = t;
  }
  __syncthreads();
  // (3) LayerNorm(30) + ReLU of each of the four pooled rows: lanes 0-29 of wave q
  {
    const int q = wave;
    const float* Pq = (q >> 1) ? P1 : P0;
    const int og = (q & 1) ? O_G2 : O_G1, ob = (q & 1) ? O_BE2 : O_BE1;
    const float v = lane < NBIN ? sp[q][lane] : 0.f;
    const float mean = wave_sum(v) / NBIN;
    const float d = lane < NBIN ? v - mean : 0.f;
    const float rstd = rsqrtf(wave_sum(d * d) / NBIN + 1e-5f);
    __syncthreads();
    if (lane < NBIN) sp[q][lane] = fmaxf(d * rstd * Pq[og + lane] + Pq[ob + lane], 0.f);
    if (lane == 0) { a.stats[((int64_t)b * 4 + q) * 2] = mean; a.stats[((int64_t)b * 4 + q) * 2 + 1] = rstd; }
  }
  __syncthreads();
  // (4) Linear(30, 1) of the sum of the two rows, ReLU: wave h
  if (wave < 2) {
    const int h = wave;
    const float* Ph = h ? P1 : P0;
    const float v = lane < NBIN ? (sp[2 * h][lane] + sp[2 * h + 1][lane]) * Ph[O_LW + lane] : 0.f;
    const float pre = wave_sum(v) + Ph[O_LB];
    if (lane == 0) { a.pre[b * 2 + h] = pre; a.out[h * a.B + b] = fmaxf(pre, 0.f); }
  }
}

__global__ __launch_bounds__(256) void cnn_heads_bwd_kernel(const CnnArgs a) {
  __shared__ float dp[4][NBIN];       // gradient of the pooled values, already divided by the bin's length
  __shared__ float red[4][2][256];
  __shared__ float red2[2][NH + 1][4];
  const int b = blockIdx.x, L = a.L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* P0 = a.params;
  const float* P1 = a.params + TTSK_CNNSCALAR_FLOATS;
  float* part = a.partials + (int64_t)b * 2 * TTSK_CNNSCALAR_FLOATS;
  float* rd = a.rowdot + (int64_t)b * 4 * L;
  for (int i = threadIdx.x; i < 2 * TTSK_CNNSCALAR_FLOATS; i += 256) part[i] = 0.f;      // the alignment gaps stay zero
  __syncthreads();
  // (1) ReLU, Linear(30, 1), ReLU, LayerNorm(30) of row q = head * 2 + flat: wave q
  {
    const int q = wave, h = q >> 1, f = q & 1;
    const float* Ph = h ? P1 : P0;
    float* ph = part + h * TTSK_CNNSCALAR_FLOATS;
    const int og = f ? O_G2 : O_G1, ob = f ? O_BE2 : O_BE1;
    const float pre = a.pre[b * 2 + h];
    const float dpre = pre > 0.f ? a.dout[h * a.B + b] : 0.f;
    const float mean = a.stats[((int64_t)b * 4 + q) * 2], rstd = a.stats[((int64_t)b * 4 + q) * 2 + 1];
    const bool on = lane < NBIN;
    const float p = on ? a.pooled[((int64_t)b * 4 + q) * NBIN + lane] : 0.f;
    const float gam = on ? Ph[og + lane] : 0.f, bet = on ? Ph[ob + lane] : 0.f;
    const float xh = on ? (p - mean) * rstd : 0.f;
    const float y = xh * gam + bet;
    const float dy = (on && y > 0.f) ? dpre * Ph[O_LW + lane] : 0.f;
    const float gx = dy * gam;
    const float c1 = wave_sum(gx) / NBIN, c2 = wave_sum(gx * xh) / NBIN;
    if (on) {
      ph[og + lane] = dy * xh;
      ph[ob + lane] = dy;
      const int cnt = bin_end(lane, L) - bin_start(lane, L);
      dp[q][lane] = rstd * (gx - c1 - xh * c2) / (float)cnt;
    }
    if (f == 0) {
      // the linear layer sees ReLU(row 0) + ReLU(row 1) of its head: recompute the other row's activation
      const int q2 = q + 1;
      const float m2 = a.stats[((int64_t)b * 4 + q2) * 2], r2 = a.stats[((int64_t)b * 4 + q2) * 2 + 1];
      const float p2 = on ? a.pooled[((int64_t)b * 4 + q2) * NBIN + lane] : 0.f;
      const float y2 = on ? (p2 - m2) * r2 * Ph[O_G2 + lane] + Ph[O_BE2 + lane] : 0.f;
      if (on) ph[O_LW + lane] = dpre * (fmaxf(y, 0.f) + fmaxf(y2, 0.f));
      if (lane == 0) ph[O_LB] = dpre;
    }
  }
  __syncthreads();
  // (2) the pool's backward: row l collects from every (overlapping) bin that holds it, in bin order
  for (int l = threadIdx.x; l < L; l += 256) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < NBIN; ++i)
      if (l >= bin_start(i, L) && l < bin_end(i, L)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] += dp[q][i];
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) rd[q * L + l] = t[q];
  }
  __syncthreads();
  // (3) the 1x1 convs' weight / bias gradients: wave w walks rows l = w (mod 4), then the four waves are summed in order
  {
    const int c = lane * 4;
    float acc0[4] = {0, 0, 0, 0}, acc1[4] = {0, 0, 0, 0};
    for (int l = wave; l < L; l += 4) {
      float v[4];
      load4(a.x + ((int64_t)b * L + l) * 256 + c, v);
      const float d0 = rd[0 * L + l], d1 = rd[2 * L + l];
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc0[e] += d0 * v[e]; acc1[e] += d1 * v[e]; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[wave][0][c + e] = acc0[e]; red[wave][1][c + e] = acc1[e]; }
    // flat_two's weight (11) and both biases: thread (k, wave) sums its rows; k = 11 is the bias pair
    if (lane <= NH) {
      float s0 = 0.f, s1 = 0.f, t0 = 0.f, t1 = 0.f;
      for (int l = wave; l < L; l += 4) {
        const float d0 = rd[1 * L + l], d1 = rd[3 * L + l];
        if (lane < NH) {
          const float v = a.cwt[((int64_t)b * L + l) * NH + lane];
          s0 += d0 * v; s1 += d1 * v;
        } else {
          s0 += d0; s1 += d1; t0 += rd[0 * L + l]; t1 += rd[2 * L + l];
        }
      }
      red2[0][lane][wave] = s0; red2[1][lane][wave] = s1;
      if (lane == NH) { dp[0][wave] = t0; dp[1][wave] = t1; }      // (dp is free again: everyone passed the barrier after (2))
    }
  }
  __syncthreads();
  {
    const int cc = threadIdx.x;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      part[h * TTSK_CNNSCALAR_FLOATS + O_W1 + cc] = red[0][h][cc] + red[1][h][cc] + red[2][h][cc] + red[3][h][cc];
    if (cc < 2 * (NH + 1)) {
      const int h = cc / (NH + 1), k = cc - h * (NH + 1);
      const float t = red2[h][k][0] + red2[h][k][1] + red2[h][k][2] + red2[h][k][3];
      part[h * TTSK_CNNSCALAR_FLOATS + (k < NH ? O_W2 + k : O_B2)] = t;
    }
    if (cc < 2) part[cc * TTSK_CNNSCALAR_FLOATS + O_B1] = dp[cc][0] + dp[cc][1] + dp[cc][2] + dp[cc][3];
  }
}

// ------------------------------------------------------------------------------------------ CWT -> pitch row
// The standardisation divides by the batch std of a column, which can be 1e-4 of the values it is made from: in fp32 the result then
// carries the rounding of the 10-term sum and of the mean amplified by 1 / std (the fp32 reference itself is 1e-5 off an fp64 run of
// itself).  The column statistics are a few hundred flops per step, so they run in fp64 here and the pitch is rounded to fp32 once.
struct CwtW { double w[10]; };

__device__ __forceinline__ double cwt_sum(const float* __restrict__ c, const CwtW& w) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 10; ++i) s += (double)c[i] * w.w[i];       // channel 10 is not used (cwt_utils.py:54-58)
  return s;
}

// One column per lane; rows finish one by one (shared by both layouts below).
__device__ __forceinline__ void cwt_pitch_row(double s, double m, double sd, int b, int l, const float* __restrict__ heads, const float* __restrict__ bins,
                                              int nb, float p_control, float* __restrict__ pitch, int* __restrict__ idx, int B, int L) {
  const double z = (s - m) / sd;                                  // B = 1 or an all-PAD column: 0 / 1e-12 = 0 exactly
  const float p = (float)(z * (double)heads[B + b] + (double)heads[b]);
  pitch[(int64_t)b * L + l] = p;
  const float x = p * p_control;
  int lo = 0, hi = nb;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (bins[mid] < x) lo = mid + 1; else hi = mid; }
  idx[(int64_t)b * L + l] = (x != x) ? nb : lo;
}

// B <= CP_MAXB: 64 columns x CP_WAVES waves per workgroup.  Wave w computes the row sums of rows b = w, w + CP_WAVES, ... ONCE into
// LDS; then every wave takes the column statistics from LDS (rows in order 0 .. B - 1: the same bits in every wave) and finishes its
// own rows.  (The one-wave layout below walks the 10-term fp64 chain of every row three times, each behind dependent loads.)
constexpr int CP_WAVES = 8, CP_MAXB = 64;
__global__ __launch_bounds__(64 * CP_WAVES) void cwt_pitch_lds_kernel(const float* __restrict__ cwt, const float* __restrict__ heads,
                                                                      const float* __restrict__ bins, int nb, float p_control,
                                                                      float* __restrict__ pitch, int* __restrict__ idx, int B, int L, const CwtW w) {
  __shared__ double sdat[CP_MAXB][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l = blockIdx.x * 64 + lane;
  const bool on = l < L;
  for (int b = wave; b < B; b += CP_WAVES) sdat[b][lane] = on ? cwt_sum(cwt + ((int64_t)b * L + l) * NH, w) : 0.0;
  __syncthreads();
  if (!on) return;
  double m = 0.0;
  for (int b = 0; b < B; ++b) m += sdat[b][lane];
  m /= (double)B;
  double v = 0.0;
  for (int b = 0; b < B; ++b) { const double d = sdat[b][lane] - m; v += d * d; }
  const double sd = sqrt(v / (double)B) + 1e-12;
  for (int b = wave; b < B; b += CP_WAVES) cwt_pitch_row(sdat[b][lane], m, sd, b, l, heads, bins, nb, p_control, pitch, idx, B, L);
}

// any B: one wave per 64 columns, the row sums recomputed in each of the three passes (same arithmetic, same order, same bits)
__global__ __launch_bounds__(64) void cwt_pitch_kernel(const float* __restrict__ cwt, const float* __restrict__ heads, const float* __restrict__ bins,
                                                       int nb, float p_control, float* __restrict__ pitch, int* __restrict__ idx, int B, int L,
                                                       const CwtW w) {
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l >= L) return;
  // statistics of column l over the batch axis, PAD rows (s = 0) included: two passes, mean then population variance, rows in order
  double m = 0.0;
  for (int b = 0; b < B; ++b) m += cwt_sum(cwt + ((int64_t)b * L + l) * NH, w);
  m /= (double)B;
  double v = 0.0;
  for (int b = 0; b < B; ++b) { const double d = cwt_sum(cwt + ((int64_t)b * L + l) * NH, w) - m; v += d * d; }
  const double sd = sqrt(v / (double)B) + 1e-12;
  for (int b = 0; b < B; ++b)
    cwt_pitch_row(cwt_sum(cwt + ((int64_t)b * L + l) * NH, w), m, sd, b, l, heads, bins, nb, p_control, pitch, idx, B, L);
}

// ------------------------------------------------------------------------------------------ loss terms
// One workgroup of 16 waves, one (b, l) row of 11 channels per thread and step; per-thread sums in row order, then a wave reduction and
// the 16 wave sums in order: a fixed summation order for a given (B, L).
constexpr int CL_WAVES = 16;
__global__ __launch_bounds__(64 * CL_WAVES) void cwt_loss_kernel(const float* __restrict__ cwt, const float* __restrict__ cwt_t,
                                                                 const float* __restrict__ heads, const float* __restrict__ mean_t,
                                                                 const float* __restrict__ std_t, const long long* __restrict__ src_lens, int B, int L,
                                                                 float grad_scale, float* __restrict__ dcwt, float* __restrict__ dheads,
                                                                 float* __restrict__ losses) {
  __shared__ double red[3][CL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float nv = 0.f;
  for (int b = 0; b < B; ++b) nv += (float)src_lens[b];
  const float gv = grad_scale * 2.f / (nv * NH);
  const float gh = grad_scale * 2.f / (float)B;
  float acc = 0.f, am = 0.f, as = 0.f;
  const int rows = B * L;
  for (int r = threadIdx.x; r < rows; r += 64 * CL_WAVES) {
    const int b = r / L, l = r - b * L;
    const bool ok = l < src_lens[b];
    const float* c = cwt + (int64_t)r * NH;
    const float* t = cwt_t + (int64_t)r * NH;
    float* g = dcwt + (int64_t)r * NH;
#pragma unroll
    for (int k = 0; k < NH; ++k) {
      const float d = ok ? c[k] - t[k] : 0.f;
      acc += d * d;
      g[k] = gv * d;
    }
  }
  for (int b = threadIdx.x; b < B; b += 64 * CL_WAVES) {
    const float d0 = heads[b] - mean_t[b], d1 = heads[B + b] - std_t[b];
    am += d0 * d0; as += d1 * d1;
    dheads[b] = gh * d0; dheads[B + b] = gh * d1;
  }
  const float r0 = wave_sum(acc), r1 = wave_sum(am), r2 = wave_sum(as);
  if (lane == 0) { red[0][wave] = r0; red[1][wave] = r1; red[2][wave] = r2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double nvd = 0.0;
    for (int b = 0; b < B; ++b) nvd += (double)src_lens[b];
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int q = 0; q < CL_WAVES; ++q) { t0 += red[0][q]; t1 += red[1][q]; t2 += red[2][q]; }
    const double pl = t0 / (nvd * NH), ml = t1 / B, sl = t2 / B;
    // ttsk_fs2_loss ran in front on this stream with a pitch term of exactly 0: its slot takes the CWT term
    losses[0] = (float)((double)losses[0] + pl + ml + sl);
    losses[2] = (float)pl; losses[5] = (float)ml; losses[6] = (float)sl;
  }
}

}  // namespace

extern "C" int ttsk_layernorm_head_bwd_nblocks(int rows) {
  const int n = (rows + HB_WAVES - 1) / HB_WAVES;
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}

extern "C" int ttsk_layernorm_head_fwd(const void* y_bf16, const float* gamma, const float* beta, const int64_t* lens, int seg_len, int rows, int D,
                                       int n_out, float eps, float p_post, uint32_t site_post, const uint64_t* rng, const float* head_w,
                                       const float* head_b, float* mean, float* rstd, float* head_out, void* stream) {
  TTSK_REQUIRE(y_bf16 && gamma && beta && lens && head_w && head_b && mean && rstd && head_out, "layernorm_head_fwd: null pointer");
  TTSK_REQUIRE(rows > 0 && seg_len > 0 && rows % seg_len == 0 && D == 256 && n_out == NH, "layernorm_head_fwd: D = 256, n_out = 11, rows = B * seg_len");
  TTSK_REQUIRE(p_post >= 0.f && p_post < 1.f && (p_post == 0.f || rng), "layernorm_head_fwd: dropout needs 0 <= p < 1 and rng");
  HeadArgs a{(const bf16_t*)y_bf16, gamma, beta, (const long long*)lens, rng, head_w, head_b, mean, rstd, head_out, rows, seg_len, p_post, eps, site_post};
  hipLaunchKernelGGL(ln_head_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_layernorm_head_bwd(const float* dhead, const float* head_w, const void* z_bf16, const float* mean, const float* rstd,
                                       const float* gamma, const float* beta, const int64_t* lens, int seg_len, int rows, int D, int n_out,
                                       float p_post, uint32_t site_post, const uint64_t* rng, void* dz_bf16, float* partials, void* stream) {
  TTSK_REQUIRE(dhead && head_w && z_bf16 && mean && rstd && gamma && beta && lens && dz_bf16 && partials, "layernorm_head_bwd: null pointer");
  TTSK_REQUIRE(rows > 0 && seg_len > 0 && rows % seg_len == 0 && D == 256 && n_out == NH, "layernorm_head_bwd: D = 256, n_out = 11, rows = B * seg_len");
  TTSK_REQUIRE(p_post >= 0.f && p_post < 1.f && (p_post == 0.f || rng), "layernorm_head_bwd: dropout needs 0 <= p < 1 and rng");
  HeadBwdArgs a{dhead, head_w, (const bf16_t*)z_bf16, mean, rstd, gamma, beta, (const long long*)lens, rng, (bf16_t*)dz_bf16, partials,
                rows, seg_len, p_post, site_post};
  hipLaunchKernelGGL(ln_head_bwd_kernel, dim3(ttsk_layernorm_head_bwd_nblocks(rows)), dim3(HB_WAVES * 64), 0, (hipStream_t)stream, a);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_cnnscalar_fwd(const void* x_bf16, const float* cwt, const float* params, int B, int L, int D, float* rowdot, float* pooled,
                                  float* stats, float* pre, float* out, void* stream) {
  TTSK_REQUIRE(x_bf16 && cwt && params && rowdot && pooled && stats && pre && out, "cnnscalar_fwd: null pointer");
  TTSK_REQUIRE(B > 0 && L > 0 && D == 256, "cnnscalar_fwd: D = 256, B, L > 0");
  CnnArgs a{(const bf16_t*)x_bf16, cwt, params, rowdot, pooled, stats, pre, out, nullptr, nullptr, B, L};
  hipLaunchKernelGGL(cnn_heads_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_cnnscalar_bwd(const float* dout, const void* x_bf16, const float* cwt, const float* params, const float* pooled,
                                  const float* stats, const float* pre, int B, int L, int D, float* rowdot, float* partials, void* stream) {
  TTSK_REQUIRE(dout && x_bf16 && cwt && params && pooled && stats && pre && rowdot && partials, "cnnscalar_bwd: null pointer");
  TTSK_REQUIRE(B > 0 && L > 0 && D == 256, "cnnscalar_bwd: D = 256, B, L > 0");
  CnnArgs a{(const bf16_t*)x_bf16, cwt, params, rowdot, (float*)pooled, (float*)stats, (float*)pre, nullptr, dout, partials, B, L};
  hipLaunchKernelGGL(cnn_heads_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_cwt_pitch(const float* cwt, const float* heads, const float* bins, int n_bins, float p_control, int B, int L, float* pitch,
                              int32_t* idx, void* stream) {
  TTSK_REQUIRE(cwt && heads && bins && pitch && idx, "cwt_pitch: null pointer");
  TTSK_REQUIRE(B > 0 && L > 0 && n_bins > 0, "cwt_pitch: bad sizes");
  CwtW w;
  for (int i = 0; i < 10; ++i) w.w[i] = (double)(float)pow((double)i + 3.5, -2.5);        // cwt_utils.py:57: (i + 1 + 2.5) ** -2.5, an fp32 factor there
  if (B <= CP_MAXB)
    hipLaunchKernelGGL(cwt_pitch_lds_kernel, dim3((L + 63) / 64), dim3(64 * CP_WAVES), 0, (hipStream_t)stream, cwt, heads, bins, n_bins, p_control, pitch,
                       idx, B, L, w);
  else
    hipLaunchKernelGGL(cwt_pitch_kernel, dim3((L + 63) / 64), dim3(64), 0, (hipStream_t)stream, cwt, heads, bins, n_bins, p_control, pitch, idx, B, L, w);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_fs2_loss_cwt(const float* cwt, const float* cwt_target, const float* heads, const float* mean_target, const float* std_target,
                                 const int64_t* src_lens, int B, int L, float grad_scale, float* dcwt, float* dheads, float* losses, void* stream) {
  TTSK_REQUIRE(cwt && cwt_target && heads && mean_target && std_target && src_lens && dcwt && dheads && losses, "fs2_loss_cwt: null pointer");
  TTSK_REQUIRE(B > 0 && L > 0, "fs2_loss_cwt: bad sizes");
  hipLaunchKernelGGL(cwt_loss_kernel, dim3(1), dim3(64 * CL_WAVES), 0, (hipStream_t)stream, cwt, cwt_target, heads, mean_target, std_target,
                     (const long long*)src_lens, B, L, grad_scale, dcwt, dheads, losses);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
