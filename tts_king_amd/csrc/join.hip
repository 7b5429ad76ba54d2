// Utterances of the flat waveform buffer joined into one waveform (include/ttsk.h, tts_king_amd/narrate.py).
//   join_stats_kernel   per utterance: peak, the kept range [a, b) of the trim, the sum of squares over it, the gain
//   join_copy_kernel    the layout (a scan of the kept lengths and pauses) and the copy: gain, fade, zeros everywhere else
// Settings, offsets, lengths, pauses and gains are the join table in device memory (TTSK_JOIN_ROW words per row, row 0 the settings),
// so they are data: the stats grid is the table's rows, the copy grid one workgroup per JOIN_TILE samples of dst.  No atomics, no host
// synchronisation; every row is checked against the buffer sizes before it is used (a row that does not fit counts as empty: a wrong
// table gives wrong audio, never a wild access).
// A row's numbers depend on its samples and the settings only, not on where it lies: the reductions assign samples to threads by
// their index in the row, and an unaligned row takes the same values through 4-byte loads.
#include "common.h"

namespace {

constexpr int ST_THREADS = 1024;   // join_stats_kernel: 16 waves per row keep enough loads in flight for one workgroup to stream from L2
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int CP_THREADS = 256;
constexpr int JOIN_TILE = 4096;    // samples of dst per workgroup of join_copy_kernel (a multiple of 256 * 8)

struct JoinCfg {
  int mode, fade, keep, lead;
  float r, floor, target, limit;
};

__device__ __forceinline__ JoinCfg join_cfg(const int* __restrict__ tab) {
  JoinCfg c;
  c.mode = tab[0];
  c.fade = max(tab[1], 0);
  c.keep = max(tab[2], 0);
  c.lead = max(tab[3], 0);
  c.r = __int_as_float(tab[4]);
  c.floor = __int_as_float(tab[5]);
  c.target = __int_as_float(tab[6]);
  c.limit = __int_as_float(tab[7]);
  return c;
}

// samples of row `row` (its TTSK_JOIN_ROW words) that may be read: 0 unless the row lies inside the source
__device__ __forceinline__ int row_len(const int* __restrict__ row, int64_t n_src) {
  const int off = row[0], n = row[1];
  return (off >= 0 && n > 0 && (int64_t)off + n <= n_src) ? n : 0;
}

// x[i .. i + 4) with zeros from n on; `vec`: x is 16-byte aligned, so a whole quad is one load
__device__ __forceinline__ float4 quad_at(const float* __restrict__ x, int i, int n, bool vec) {
  if (vec && i + 4 <= n) return *reinterpret_cast<const float4*>(x + i);
  float4 v;
  v.x = i < n ? x[i] : 0.0f;
  v.y = i + 1 < n ? x[i + 1] : 0.0f;
  v.z = i + 2 < n ? x[i + 2] : 0.0f;
  v.w = i + 3 < n ? x[i + 3] : 0.0f;
  return v;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}

// One workgroup per row.  Three passes over the row (the second and third find it in L2): peak; first / last sample at or above the
// threshold; sum of squares over the kept range.  Thread t serves quads t, t + 1024, ... of the range it reduces, its four samples in
// their order; the 64 partial results of a wave meet in a butterfly, the 16 waves' in LDS, where thread 0 takes them in their order.
__global__ __launch_bounds__(ST_THREADS) void join_stats_kernel(const float* __restrict__ src, int64_t n_src, const int* __restrict__ tab,
                                                                int* __restrict__ info) {
  __shared__ float sf[ST_WAVES];
  __shared__ int si[2 * ST_WAVES];
  __shared__ float bc_f;
  __shared__ int bc_i[2];
  const int u = blockIdx.x, t = threadIdx.x, wv = t >> 6;
  const JoinCfg c = join_cfg(tab);
  const int* row = tab + (1 + u) * TTSK_JOIN_ROW;
  const int n = row_len(row, n_src);
  const float* x = src + (n ? row[0] : 0);
  const bool trim = (row[3] & 1) != 0;
  int* out = info + u * TTSK_JOIN_ROW;

  // 1. peak
  bool vec = (((uintptr_t)x) & 15) == 0;
  float pk = 0.0f;
  for (int i = 4 * t; i < n; i += 4 * ST_THREADS) {
    const float4 v = quad_at(x, i, n, vec);
    pk = fmaxf(fmaxf(pk, fabsf(v.x)), fmaxf(fmaxf(fabsf(v.y), fabsf(v.z)), fabsf(v.w)));
  }
  pk = wave_max(pk);
  if ((t & 63) == 0) sf[wv] = pk;
  __syncthreads();
  if (t == 0) {
    float m = sf[0];
    for (int w = 1; w < ST_WAVES; ++w) m = fmaxf(m, sf[w]);
    bc_f = m;
  }
  __syncthreads();
  const float peak = bc_f;

  // 2. the kept range
  int a = 0, b = n;
  if (trim) {                                             // uniform over the workgroup
    const float thr = fmaxf(peak * c.r, c.floor);
    int first = 0x7fffffff, last = -1;
    for (int i = 4 * t; i < n; i += 4 * ST_THREADS) {
      const float4 v = quad_at(x, i, n, vec);
      const float q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < n && fabsf(q[j]) >= thr) {
          first = min(first, i + j);
          last = max(last, i + j);
        }
      }
    }
    first = wave_min_i(first);
    last = wave_max_i(last);
    if ((t & 63) == 0) si[wv] = first, si[ST_WAVES + wv] = last;
    __syncthreads();
    if (t == 0) {
      int f = si[0], l = si[ST_WAVES];
      for (int w = 1; w < ST_WAVES; ++w) f = min(f, si[w]), l = max(l, si[ST_WAVES + w]);
      bc_i[0] = f, bc_i[1] = l;
    }
    __syncthreads();
    first = bc_i[0], last = bc_i[1];
    if (last < 0 || !(peak > 0.0f)) {
      a = b = 0;
    } else {
      a = first > c.keep ? first - c.keep : 0;
      b = (int)min((int64_t)n, (int64_t)last + 1 + c.keep);
    }
  }

  // 3. sum of squares over [a, b): one fma per sample, so a sample's square is not rounded on its own
  const int m = b - a;
  const float* xa = x + a;
  vec = (((uintptr_t)xa) & 15) == 0;
  float acc = 0.0f;
  for (int i = 4 * t; i < m; i += 4 * ST_THREADS) {
    const float4 v = quad_at(xa, i, m, vec);
    acc = fmaf(v.x, v.x, acc);
    acc = fmaf(v.y, v.y, acc);
    acc = fmaf(v.z, v.z, acc);
    acc = fmaf(v.w, v.w, acc);
  }
  acc = wave_sum(acc);
  if ((t & 63) == 0) sf[wv] = acc;                        // the peak's readers passed the barriers above
  __syncthreads();
  if (t == 0) {
    float ss = sf[0];
    for (int w = 1; w < ST_WAVES; ++w) ss += sf[w];
    float g = 1.0f;
    if (m > 0 && peak > 0.0f) {
      if (c.mode == TTSK_JOIN_RMS) {
        const float rms = sqrtf(ss / (float)m);
        g = fminf(c.target / rms, c.limit / peak);
      } else if (c.mode == TTSK_JOIN_PEAK) {
        g = c.limit / peak;
      } else {
        g = __int_as_float(row[4]);
      }
    } else if (m > 0 && c.mode == TTSK_JOIN_GIVEN) {
      g = __int_as_float(row[4]);
    }
    out[0] = a;
    out[1] = b;
    out[3] = __float_as_int(peak);
    out[4] = __float_as_int(ss);
    out[5] = __float_as_int(g);
    out[6] = 0;
    out[7] = 0;
  }
}

template <bool I16>
__device__ __forceinline__ float to_out(float y, float scale) {
  // int16: saturate here, truncate toward zero at the store (resample.hip's rule); a NaN gives -32768
  if constexpr (I16) return fminf(fmaxf(y * scale, -32768.0f), 32767.0f);
  return y;
}

// the fade's weight at sample k of a kept range of m samples, F = min(fade, m / 2) > 0
__device__ __forceinline__ float fade_w(int k, int m, int F) {
  if (k < F) return (float)(2 * k + 1) / (float)(2 * F);
  if (k >= m - F) return (float)(2 * (m - 1 - k) + 1) / (float)(2 * F);
  return 1.0f;
}

// One workgroup per JOIN_TILE samples of dst.  Every workgroup scans the rows' kept lengths and pauses into LDS (integers: the same
// numbers in every workgroup), then a thread serves PER samples at a time, 16 bytes of dst: it finds the row its first sample falls
// in by bisection; a piece that lies in one row's kept range takes the fast path (16-byte loads when the source is aligned to
// them, 4-byte loads otherwise), a piece of zeros is one store, and a piece that crosses an edge is served sample by sample.
template <bool I16>
__global__ __launch_bounds__(CP_THREADS) void join_copy_kernel(const float* __restrict__ src, int64_t n_src, const int* __restrict__ tab, int U,
                                                               int* __restrict__ info, void* __restrict__ dst, int n_dst, float scale) {
  constexpr int PER = I16 ? 8 : 4;
  __shared__ int so[TTSK_JOIN_MAX_ROWS + 1];             // o_u, saturated; so[U] = total
  __shared__ int sl[TTSK_JOIN_MAX_ROWS];                 // b_u - a_u
  __shared__ long long part[2][CP_THREADS];
  const int t = threadIdx.x;
  const JoinCfg c = join_cfg(tab);
  // the layout: thread t owns rows [t * per, (t + 1) * per)
  const int per = (U + CP_THREADS - 1) / CP_THREADS;
  const int u0 = min(t * per, U), u1 = min(u0 + per, U);
  long long mine = 0;
  for (int u = u0; u < u1; ++u) {
    const int* row = tab + (1 + u) * TTSK_JOIN_ROW;
    const int n = row_len(row, n_src);
    const int a = info[u * TTSK_JOIN_ROW], b = info[u * TTSK_JOIN_ROW + 1];
    const int m = (a >= 0 && a <= b && b <= n) ? b - a : 0;
    sl[u] = m;
    mine += (long long)m + max(row[2], 0);
  }
  part[0][t] = mine;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < CP_THREADS; d <<= 1) {              // inclusive scan of the threads' sums
    part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  long long o = (long long)c.lead + (t ? part[cur][t - 1] : 0);
  for (int u = u0; u < u1; ++u) {
    so[u] = (int)min(o, (long long)0x7fffffff);
    o += (long long)sl[u] + max(tab[(1 + u) * TTSK_JOIN_ROW + 2], 0);
  }
  if (t == CP_THREADS - 1) so[U] = (int)min((long long)c.lead + part[cur][CP_THREADS - 1], (long long)0x7fffffff);
  __syncthreads();
  if (blockIdx.x == 0) {
    for (int u = t; u < U; u += CP_THREADS) info[u * TTSK_JOIN_ROW + 2] = so[u];
    if (t < TTSK_JOIN_ROW) info[U * TTSK_JOIN_ROW + t] = t == 0 ? so[U] : 0;
  }

  const int t0 = blockIdx.x * JOIN_TILE;                  // n_dst < 2^31 and the grid covers it: no overflow
  const int t1 = (int)min((int64_t)t0 + JOIN_TILE, (int64_t)n_dst);
  for (int it = 0; it < JOIN_TILE / (PER * CP_THREADS); ++it) {
    const int d = t0 + (it * CP_THREADS + t) * PER;       // at most t0 + JOIN_TILE - PER
    if (d >= t1) break;
    // u = the last row with o_u <= d (-1: d lies in the lead); rows behind it start past d, rows before it end at or before o_u
    int lo = 0, hi = U;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (so[mid] <= d) lo = mid + 1; else hi = mid;
    }
    int u = lo - 1;
    const int np = min(PER, t1 - d);                      // < PER only at the end of dst
    float y[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) y[j] = 0.0f;
    const int k0 = u >= 0 ? d - so[u] : 0;
    if (u >= 0 && np == PER && k0 + PER <= sl[u]) {
      // the whole piece inside row u's kept range
      const int m = sl[u];
      const int F = min(c.fade, m >> 1);
      const float g = __int_as_float(info[u * TTSK_JOIN_ROW + 5]);
      const float* p = src + tab[(1 + u) * TTSK_JOIN_ROW] + info[u * TTSK_JOIN_ROW] + k0;
      if ((((uintptr_t)p) & 15) == 0) {
#pragma unroll
        for (int j = 0; j < PER; j += 4) {
          const float4 v = *reinterpret_cast<const float4*>(p + j);
          y[j] = v.x, y[j + 1] = v.y, y[j + 2] = v.z, y[j + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) y[j] = p[j];
      }
      const bool faded = F > 0 && (k0 < F || k0 + PER > m - F);
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        float v = y[j] * g;
        if (faded) v = v * fade_w(k0 + j, m, F);
        y[j] = to_out<I16>(v, scale);
      }
    } else if (u >= 0 && k0 >= sl[u] && (u + 1 >= U || d + np <= so[u + 1])) {
      // zeros: a pause, or past the end
    } else if (u < 0 && d + np <= so[0]) {
      // zeros: the lead
    } else {
      for (int j = 0; j < np; ++j) {
        while (u + 1 < U && so[u + 1] <= d + j) ++u;
        if (u < 0) continue;
        const int k = d + j - so[u], m = sl[u];
        if (k >= m) continue;
        const int F = min(c.fade, m >> 1);
        float v = src[(int64_t)tab[(1 + u) * TTSK_JOIN_ROW] + info[u * TTSK_JOIN_ROW] + k] * __int_as_float(info[u * TTSK_JOIN_ROW + 5]);
        if (F > 0) v = v * fade_w(k, m, F);
        y[j] = to_out<I16>(v, scale);
      }
    }
    if constexpr (I16) {
      short* q = (short*)dst + d;
      if (np == PER) {
        auto pk = [](float lo16, float hi16) { return ((unsigned)(int)lo16 & 0xFFFFu) | ((unsigned)(int)hi16 << 16); };
        *reinterpret_cast<uint4*>(q) = make_uint4(pk(y[0], y[1]), pk(y[2], y[3]), pk(y[4], y[5]), pk(y[6], y[7]));
      } else {
        for (int j = 0; j < np; ++j) q[j] = (short)(int)y[j];
      }
    } else {
      float* q = (float*)dst + d;
      if (np == PER) {
        *reinterpret_cast<float4*>(q) = make_float4(y[0], y[1], y[2], y[3]);
      } else {
        for (int j = 0; j < np; ++j) q[j] = y[j];
      }
    }
  }
}

bool join_args_ok(const float* src, int64_t n_src, const int32_t* join, int U, const int32_t* info) {
  return src && join && info && n_src > 0 && U > 0;
}

}  // namespace

#define TTSK_JOIN_COMMON(name)                                                                                                          \
  TTSK_REQUIRE(join_args_ok(src, n_src, join, U, info), name ": bad arguments");                                                        \
  TTSK_REQUIRE(U <= TTSK_JOIN_MAX_ROWS, name ": %d rows, at most %d", U, TTSK_JOIN_MAX_ROWS);                                           \
  TTSK_REQUIRE(n_src <= 0x7fffffff, name ": a source of %lld samples, must be below 2^31", (long long)n_src);                           \
  TTSK_REQUIRE((((uintptr_t)join) & 15) == 0 && (((uintptr_t)info) & 15) == 0 && (((uintptr_t)src) & 3) == 0,                           \
               name ": the join table and the info table must be 16-byte aligned, the source aligned to its element")

extern "C" int ttsk_wav_join_stats(const float* src, int64_t n_src, const int32_t* join, int U, int32_t* info, void* stream) {
  TTSK_JOIN_COMMON("wav_join_stats");
  hipLaunchKernelGGL(join_stats_kernel, dim3(U), dim3(ST_THREADS), 0, (hipStream_t)stream, src, n_src, (const int*)join, (int*)info);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_wav_join(const float* src, int64_t n_src, const int32_t* join, int U, int32_t* info, void* dst, int64_t n_dst, int to_i16,
                             float scale, void* stream) {
  TTSK_JOIN_COMMON("wav_join");
  TTSK_REQUIRE(dst && n_dst > 0, "wav_join: bad arguments");
  TTSK_REQUIRE(n_dst <= 0x7fffffff, "wav_join: a destination of %lld samples, must be below 2^31", (long long)n_dst);
  TTSK_REQUIRE((((uintptr_t)dst) & 15) == 0, "wav_join: the destination must be 16-byte aligned");
  const unsigned grid = (unsigned)((n_dst + JOIN_TILE - 1) / JOIN_TILE);
  if (to_i16)
    hipLaunchKernelGGL(join_copy_kernel<true>, dim3(grid), dim3(CP_THREADS), 0, (hipStream_t)stream, src, n_src, (const int*)join, U, (int*)info,
                       dst, (int)n_dst, scale);
  else
    hipLaunchKernelGGL(join_copy_kernel<false>, dim3(grid), dim3(CP_THREADS), 0, (hipStream_t)stream, src, n_src, (const int*)join, U, (int*)info,
                       dst, (int)n_dst, scale);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
