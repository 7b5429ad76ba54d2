// pitch.hip — fundamental frequency per frame (YIN) and the frame-to-phoneme reduction of FS2 data preparation.
// reference: fs_two/preprocessor/preprocessor.py:206-266.  The reference takes F0 from pyworld (DIO + StoneMask); this is YIN
// (de Cheveigne & Kawahara 2002, steps 1-5), whose every step is a fixed arithmetic rule that tests/pitch_ref.py restates in fp64.
// The values are NOT pyworld's.
#include "common.h"

namespace {

constexpr int YIN_THREADS = 256;
constexpr int YIN_MAX_S = 8192;        // W + tau_max: the frame's samples live in LDS
constexpr int YIN_MAX_TAU = 1023;      // lags 0 .. 1023 = 256 groups of four, 16 per lane of the scanning wave
constexpr int YIN_FLUSH = 8;           // j-blocks (of four samples) summed in a short accumulator before they join the long one

// One workgroup per (frame, row).  The frame's S = W + tau_max samples are staged in LDS (zeros from `len` on and in eight words
// of padding).  A work item is (lag group g, part p): lags 4g .. 4g+3 over the p-th slice of the W samples, in blocks of four j.
// Per block a lane reads x[j .. j+3] (one address for all lanes: a broadcast) and x[j + 4g + 4 .. j + 4g + 7] (consecutive 16-byte
// words across lanes: conflict-free), keeps the previous such word, and does the 16 (j, lag) pairs from registers: two ds_read_b128
// per 32 VALU operations.  Sums are blocked (YIN_FLUSH blocks at a time) so that the rounding error grows with the square root
// of the slice, not with its length; the parts are added in order.  The order depends on (W, tau_max) only.
// Then one wave forms the running sum over lags (16 consecutive lags per lane, a shuffle scan across lanes), every thread the
// normalised difference d', a workgroup minimum finds the first lag under the threshold, and thread 0 walks to the local
// minimum, refines by a parabola and writes the frame.
__global__ __launch_bounds__(YIN_THREADS) void pitch_yin_kernel(const float* __restrict__ wav, const int* __restrict__ lens, int ld,
                                                                int hop, int W, int tau_min, int tau_max, float sr, float thr,
                                                                int NG, int P, int T_max, float* __restrict__ f0) {
  __shared__ __attribute__((aligned(16))) float x[YIN_MAX_S + 8];
  __shared__ __attribute__((aligned(16))) float dpart[4 * YIN_THREADS];      // [part][lag], 4 * NG * P <= 1024 floats
  __shared__ float dp[YIN_MAX_TAU + 1];                                      // d, then d'
  __shared__ int first;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int len = lens ? lens[b] : ld;
  len = len < 0 ? 0 : (len > ld ? ld : len);
  float* out = f0 + (int64_t)b * T_max + t;
  if (t >= 1 + len / hop) {          // uniform over the workgroup
    if (tid == 0) *out = 0.f;
    return;
  }
  const int S = W + tau_max;
  int s0 = t * hop - S / 2;
  const int hi = len - S > 0 ? len - S : 0;
  s0 = s0 < 0 ? 0 : (s0 > hi ? hi : s0);
  const float* w = wav + (int64_t)b * ld;
  for (int j = tid; j < S + 8; j += YIN_THREADS) x[j] = (j < S && s0 + j < len) ? w[s0 + j] : 0.f;
  if (tid == 0) first = tau_max;
  __syncthreads();

  if (tid < NG * P) {
    const int g = tid % NG, p = tid / NG;
    const int nblk = W >> 2, per = (nblk + P - 1) / P;
    const int k0 = p * per, k1 = (k0 + per < nblk) ? k0 + per : nblk;
    float tot[4] = {0.f, 0.f, 0.f, 0.f};
    const float4* xa = reinterpret_cast<const float4*>(x);          // x[j ..] : block k is xa[k]
    const float4* xb = xa + g;                                      // x[j + 4g ..]
    float4 lo = k0 < k1 ? xb[k0] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kk = k0; kk < k1; kk += YIN_FLUSH) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      const int ke = kk + YIN_FLUSH < k1 ? kk + YIN_FLUSH : k1;
      for (int k = kk; k < ke; ++k) {
        const float4 a = xa[k];
        const float4 hi4 = xb[k + 1];
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi4.x, hi4.y, hi4.z, hi4.w};
        const float aj[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int l = 0; l < 4; ++l) {
            const float df = aj[q] - v[q + l];
            acc[l] = fmaf(df, df, acc[l]);
          }
        }
        lo = hi4;
      }
#pragma unroll
      for (int l = 0; l < 4; ++l) tot[l] += acc[l];
    }
    reinterpret_cast<float4*>(dpart)[p * NG + g] = make_float4(tot[0], tot[1], tot[2], tot[3]);
  }
  __syncthreads();
  const int nlag = 4 * NG;           // > tau_max
  for (int tau = tid; tau < nlag; tau += YIN_THREADS) {
    float s = dpart[tau];
    for (int p = 1; p < P; ++p) s += dpart[p * nlag + tau];
    dp[tau] = tau == 0 ? 0.f : s;
  }
  __syncthreads();
  if (tid < 64) {                    // running sum over lags 1 .. tau_max, then d'(tau) = d(tau) * tau / sum, 1 where the sum is 0
    const int c0 = tid * 16;
    float loc[16];
    float run = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int tau = c0 + i;
      run += (tau >= 1 && tau <= tau_max) ? dp[tau] : 0.f;
      loc[i] = run;
    }
    float inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float up = __shfl_up(inc, o, 64);
      if (tid >= o) inc += up;
    }
    const float base = inc - run;    // sum of the lanes before this one
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int tau = c0 + i;
      if (tau >= 1 && tau <= tau_max) {
        const float cum = base + loc[i];
        dp[tau] = cum == 0.f ? 1.f : dp[tau] * (float)tau / cum;
      }
    }
  }
  __syncthreads();
  for (int tau = tau_min + tid; tau < tau_max; tau += YIN_THREADS)
    if (dp[tau] < thr) {
      atomicMin(&first, tau);
      break;                         // this thread's later lags are larger
    }
  __syncthreads();
  if (tid == 0) {
    int tau = first;
    float r = 0.f;
    if (tau < tau_max) {
      while (tau + 1 < tau_max && dp[tau + 1] < dp[tau]) ++tau;
      const float a = dp[tau - 1], bb = dp[tau], c = dp[tau + 1];
      const float den = a - 2.f * bb + c;
      float off = den == 0.f ? 0.f : 0.5f * (a - c) / den;
      if (!(fabsf(off) <= 1.f)) off = 0.f;
      r = sr / ((float)tau + off);
    }
    *out = r;
  }
}

constexpr int PP_THREADS = 256;
constexpr int PP_MAX_T = 8192;
constexpr int PP_MAX_L = 1024;         // four phonemes per thread
constexpr int PP_NONE = 0x7fffffff;

// inclusive scan of one int per thread over the workgroup (Hillis-Steele in LDS, buf[i] = thread i's result on return);
// OP 0: +, 1: max, 2: min.  Called by every thread.
template <int OP>
__device__ __forceinline__ int block_scan(int v, int* buf) {
  const int tid = threadIdx.x;
  __syncthreads();
  buf[tid] = v;
  __syncthreads();
  for (int o = 1; o < PP_THREADS; o <<= 1) {
    const int other = tid >= o ? buf[tid - o] : (OP == 0 ? 0 : (OP == 1 ? -1 : PP_NONE));
    __syncthreads();
    v = OP == 0 ? v + other : (OP == 1 ? (v > other ? v : other) : (v < other ? v : other));
    buf[tid] = v;
    __syncthreads();
  }
  return v;
}

// sum of one float per thread, a fixed tree in LDS; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* buf) {
  const int tid = threadIdx.x;
  __syncthreads();
  buf[tid] = v;
  __syncthreads();
  for (int o = PP_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) buf[tid] += buf[tid + o];
    __syncthreads();
  }
  return buf[0];
}

// the value interp1d(fill_value=(first, last)) gives frame t between the voiced frames pv < t < nx (-1 / PP_NONE: there is none)
__device__ __forceinline__ float interp_frame(const float* f, int t, int pv, int nx, int vfirst, int vlast) {
  if (pv < 0) return f[vfirst];
  if (nx == PP_NONE) return f[vlast];
  const float ylo = f[pv], yhi = f[nx];
  const float slope = (yhi - ylo) / (float)(nx - pv);
  return slope * (float)(t - pv) + ylo;
}

// One workgroup per utterance (preprocessor.py:215-266): totals and statuses, unvoiced frames interpolated between their voiced
// neighbours (held before the first and after the last), phoneme means of pitch and energy in frame order, log, standardisation
// by the utterance's own mean and population standard deviation.  A phoneme of no frames stores 0 and stays out of the statistics.
// Every condition that a barrier sits under is uniform over the workgroup (it comes from a scan's total).
__global__ __launch_bounds__(PP_THREADS) void phoneme_prosody_kernel(const float* __restrict__ f0, const float* __restrict__ energy, int ldT,
                                                                    const int* __restrict__ dur, int ldL, const int* __restrict__ Tn,
                                                                    const int* __restrict__ Ln, float* __restrict__ pitch,
                                                                    float* __restrict__ en, float* __restrict__ pmean,
                                                                    float* __restrict__ pstd, int* __restrict__ status) {
  __shared__ float f[PP_MAX_T];
  __shared__ int pos[PP_MAX_L + 1];
  __shared__ float lp[PP_MAX_L];
  __shared__ int ibuf[PP_THREADS];
  __shared__ int perm[PP_THREADS];
  __shared__ float fbuf[PP_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  int T = Tn[b], Lp = Ln[b];
  T = T < 0 ? 0 : (T > ldT ? ldT : T);
  Lp = Lp < 0 ? 0 : (Lp > ldL ? ldL : Lp);
  const float* fr = f0 + (int64_t)b * ldT;
  const float* er = energy + (int64_t)b * ldT;
  const int* dr = dur + (int64_t)b * ldL;
  float* po = pitch + (int64_t)b * ldL;
  float* eo = en + (int64_t)b * ldL;

  // durations: four consecutive phonemes per thread, their exclusive prefix in pos[]; a negative one, or one alone longer than any
  // row, fails the row as "more frames than T" (and keeps the total inside int32)
  int d4[4], mine = 0, bad = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ph = tid * 4 + i;
    d4[i] = ph < Lp ? dr[ph] : 0;
    if (d4[i] < 0 || d4[i] > PP_MAX_T) { bad = 1; d4[i] = 0; }
    mine += d4[i];
  }
  const int incl = block_scan<0>(mine, ibuf);
  const int n = ibuf[PP_THREADS - 1];
  block_scan<1>(bad, ibuf);
  bad = ibuf[PP_THREADS - 1];
  {
    int run = incl - mine;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pos[tid * 4 + i] = run;
      run += d4[i];
    }
    if (tid == PP_THREADS - 1) pos[PP_MAX_L] = run;
  }
  int st = (bad || n > T) ? 2 : 0;
  // a contiguous chunk of the n frames per thread: its voiced count, its first and its last voiced frame
  const int per = (n + PP_THREADS - 1) / PP_THREADS;
  const int t0 = tid * per < n ? tid * per : n, t1 = (t0 + per < n) ? t0 + per : n;
  int last = -1, firstv = PP_NONE, cnt = 0;
  if (st == 0) {
    for (int t = t0; t < t1; ++t) {
      const float v = fr[t];
      f[t] = v;
      if (v != 0.f) {
        last = t;
        if (firstv == PP_NONE) firstv = t;
        ++cnt;
      }
    }
  }
  block_scan<0>(cnt, ibuf);
  if (st == 0 && ibuf[PP_THREADS - 1] <= 1) st = 1;
  if (st == 0) {
    block_scan<1>(last, ibuf);
    const int prev_before = tid > 0 ? ibuf[tid - 1] : -1;            // the last voiced frame of the chunks before this one
    const int vlast = ibuf[PP_THREADS - 1];
    perm[tid] = firstv;
    __syncthreads();
    block_scan<2>(perm[PP_THREADS - 1 - tid], ibuf);                 // ibuf[i] = the first voiced frame of the chunks >= 255 - i
    const int next_after = tid < PP_THREADS - 1 ? ibuf[PP_THREADS - 2 - tid] : PP_NONE;
    const int vfirst = ibuf[PP_THREADS - 1];
    // fill the chunk's unvoiced runs.  Only voiced entries of f[] are read and only unvoiced ones are written, each by its owner.
    int pv = prev_before;
    for (int t = t0; t < t1;) {
      if (f[t] != 0.f) {
        pv = t++;
        continue;
      }
      int nx = PP_NONE, stop = t1;
      for (int u = t + 1; u < t1; ++u)
        if (f[u] != 0.f) {
          nx = stop = u;
          break;
        }
      if (nx == PP_NONE) nx = next_after;
      for (; t < stop; ++t) f[t] = interp_frame(f, t, pv, nx, vfirst, vlast);
    }
    __syncthreads();
    // phoneme means in frame order, log, the utterance's mean and population standard deviation over the phonemes that have frames
    float s1 = 0.f;
    int m = 0;
    for (int ph = tid; ph < Lp; ph += PP_THREADS) {
      const int a = pos[ph], d = pos[ph + 1] - a;
      float v = 0.f;
      if (d > 0) {
        float s = 0.f;
        for (int t = a; t < a + d; ++t) s += f[t];
        v = logf(s / (float)d);
        s1 += v;
        ++m;
      }
      lp[ph] = v;
    }
    block_scan<0>(m, ibuf);
    const float cntf = (float)ibuf[PP_THREADS - 1];
    const float mean = block_sum(s1, fbuf) / cntf;
    float s2 = 0.f;
    for (int ph = tid; ph < Lp; ph += PP_THREADS)
      if (pos[ph + 1] - pos[ph] > 0) {
        const float c = lp[ph] - mean;
        s2 += c * c;
      }
    const float sd = sqrtf(block_sum(s2, fbuf) / cntf);
    if (!(sd > 0.f)) st = 3;
    if (st == 0) {
      for (int ph = tid; ph < ldL; ph += PP_THREADS) {
        float pv2 = 0.f, ev = 0.f;
        if (ph < Lp) {
          const int a = pos[ph], d = pos[ph + 1] - a;
          if (d > 0) {
            pv2 = (lp[ph] - mean) / sd;
            float s = 0.f;
            for (int t = a; t < a + d; ++t) s += er[t];
            ev = s / (float)d;
          }
        }
        po[ph] = pv2;
        eo[ph] = ev;
      }
      if (tid == 0) {
        pmean[b] = mean;
        pstd[b] = sd;
        status[b] = 0;
      }
    }
  }
  if (st != 0) {
    for (int ph = tid; ph < ldL; ph += PP_THREADS) {
      po[ph] = 0.f;
      eo[ph] = 0.f;
    }
    if (tid == 0) {
      pmean[b] = 0.f;
      pstd[b] = 0.f;
      status[b] = st;
    }
  }
}

}  // namespace

extern "C" int ttsk_pitch_yin(const float* wav, const int32_t* lens, int B, int ld, int hop, int W, int tau_min, int tau_max, float sr,
                              float thr, float* f0, int T_max, void* stream) {
  TTSK_REQUIRE(wav && f0, "ttsk_pitch_yin: null wav or f0");
  TTSK_REQUIRE(B > 0 && B <= 65535 && ld > 0 && hop > 0 && W > 0 && T_max > 0, "ttsk_pitch_yin: B, ld, hop, W and T_max must be positive (B <= 65535)");
  TTSK_REQUIRE((W & 3) == 0, "ttsk_pitch_yin: the integration window must be a multiple of 4, got %d", W);
  TTSK_REQUIRE(tau_min >= 2, "ttsk_pitch_yin: tau_min %d < 2", tau_min);
  TTSK_REQUIRE(tau_max > tau_min + 1, "ttsk_pitch_yin: tau_max %d must exceed tau_min %d + 1", tau_max, tau_min);
  TTSK_REQUIRE(tau_max <= YIN_MAX_TAU && (int64_t)W + tau_max <= YIN_MAX_S,
               "ttsk_pitch_yin: tau_max %d > %d or W + tau_max %lld > %d samples of LDS", tau_max, YIN_MAX_TAU, (long long)W + tau_max,
               YIN_MAX_S);
  TTSK_REQUIRE(T_max == 1 + ld / hop, "ttsk_pitch_yin: T_max %d is not 1 + ld / hop = %d", T_max, 1 + ld / hop);
  TTSK_REQUIRE(sr > 0.f && thr > 0.f, "ttsk_pitch_yin: sample rate and threshold must be positive");
  const int NG = tau_max / 4 + 1;                 // lags 0 .. 4 NG - 1 >= tau_max
  int P = YIN_THREADS / NG;
  if (P > W / 4) P = W / 4;
  hipLaunchKernelGGL(pitch_yin_kernel, dim3(T_max, B), dim3(YIN_THREADS), 0, (hipStream_t)stream, wav, (const int*)lens, ld, hop, W,
                     tau_min, tau_max, sr, thr, NG, P, T_max, f0);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_phoneme_prosody(const float* f0, const float* energy, int ldT, const int32_t* dur, int ldL, const int32_t* T,
                                    const int32_t* Lp, int B, float* pitch, float* energy_ph, float* pitch_mean, float* pitch_std,
                                    int32_t* status, void* stream) {
  TTSK_REQUIRE(f0 && energy && dur && T && Lp && pitch && energy_ph && pitch_mean && pitch_std && status, "ttsk_phoneme_prosody: null pointer");
  TTSK_REQUIRE(B > 0 && ldT > 0 && ldT <= PP_MAX_T && ldL > 0 && ldL <= PP_MAX_L,
               "ttsk_phoneme_prosody: needs B > 0, 0 < frames per row <= %d, 0 < phonemes per row <= %d (got %d, %d, %d)", PP_MAX_T,
               PP_MAX_L, B, ldT, ldL);
  hipLaunchKernelGGL(phoneme_prosody_kernel, dim3(B), dim3(PP_THREADS), 0, (hipStream_t)stream, f0, energy, ldT, (const int*)dur, ldL,
                     (const int*)T, (const int*)Lp, pitch, energy_ph, pitch_mean, pitch_std, (int*)status);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
