// Sample-rate conversion of the flat waveform buffer by a rational factor L / M (include/ttsk.h, tts_king_amd/resample.py).
//   resample_kernel   fp32 utterances back to back -> each of them resampled, fp32 or saturated int16, at its place in dst
// The work comes from the segment table in device memory (TTSK_SEG_ROW int32 per utterance), so a length is data: the grid is one
// workgroup per `tile` samples of dst (a number that depends on the filter alone) and so depends on n_dst alone.  A workgroup looks up
// the segments that cross its tile (one ballot per 64 table rows) and serves its part of each, so a segment may start anywhere and
// tiles may straddle segments.  No atomics, no host synchronisation; every row is checked against the buffer sizes before it is used
// (a row that does not fit is skipped: a wrong plan gives wrong audio, never a wild access).
// An output sample is ONE thread's sum over q = 0 .. P-1, in that order, of fma(T[p][q], x[j0 + C - q], acc) with x = 0 outside its
// own segment: the value depends on the segment's samples, the table and m only — not on the segment's place, the tile or the chunk.
#include "common.h"

namespace {

constexpr int RS_LDS = 8192;       // floats of staged input per chunk of outputs (32 KB)
constexpr int RS_R = 4;            // outputs per thread of the staged kernel, S apart: they share a phase, so a coefficient is loaded once for all
constexpr int RS_DIRECT_TILE = 1024;

struct Seg {
  int src_off, src_len, dst_off, dst_len;
};

// How a filter runs.  stride: S, a multiple of L, so that outputs S apart have the same phase; groups: how many of them (1 .. RS_R) a
// thread serves from one staged span; a chunk = S * groups outputs reads (chunk - 1) * M / L + 1 + P input samples at most, which must
// fit RS_LDS.  groups = 0: the filter is too long for that, every tap reads the source (one output per thread).  tile: outputs per workgroup.
struct RsPlan {
  int stride, groups, tile;
};

RsPlan rs_plan(int L, int M, int P) {
  RsPlan pl{0, 0, RS_DIRECT_TILE};
  if (L > 1024) return pl;
  // the multiple of L up to 1024 that leaves the fewest of the 256 threads idle in its last pass; the smallest of equals
  int best = 0, best_num = -1, best_den = 1;
  for (int s = L; s <= 1024; s += L) {
    const int den = 256 * ((s + 255) / 256);
    if (best_num < 0 || (int64_t)s * best_den > (int64_t)best_num * den) best = s, best_num = s, best_den = den;
  }
  for (int g = RS_R; g >= 1; --g) {
    if (((int64_t)best * g - 1) * M / L + 1 + P <= RS_LDS) {
      pl.stride = best, pl.groups = g, pl.tile = best * g;      // one chunk per tile: a short call still spreads over the device
      return pl;
    }
  }
  return pl;
}

__device__ __forceinline__ bool seg_fits(const Seg& s, int64_t n_src, int64_t n_dst) {
  return s.src_off >= 0 && s.src_len > 0 && (int64_t)s.src_off + s.src_len <= n_src && s.dst_off >= 0 && s.dst_len > 0 &&
         (int64_t)s.dst_off + s.dst_len <= n_dst;
}

template <bool I16>
__device__ __forceinline__ void put(void* dst, int64_t o, float y, float scale) {
  if constexpr (I16) {
    // saturate, then truncate toward zero: in range this is to_int16_kernel's arithmetic (rowops.hip); a NaN gives -32768
    ((short*)dst)[o] = (short)(int)fminf(fmaxf(y * scale, -32768.0f), 32767.0f);
  } else {
    ((float*)dst)[o] = y;
  }
}

// Outputs [m_lo, m_hi) of segment s, staged: per chunk of S * groups outputs the input span goes through LDS with the zero extension
// applied there; thread t serves outputs ma + t + i * S, i < groups.  The table is tap-major (table[q * L + p]): the threads of a wave
// read one row of L phases per tap, a few cache lines, and the whole table stays in L2 for every tile.
template <bool I16>
__device__ __forceinline__ void segment_staged(float* xs, const Seg& s, const float* __restrict__ x, const float* __restrict__ table, int L, int M,
                                               int P, int C, void* __restrict__ dst, float scale, int S, int groups, int m_lo, int m_hi) {
  const int chunk = S * groups;
  const int step = (int)((int64_t)S * M / L);             // input samples between outputs S apart (exact: L divides S)
  for (int ma = m_lo; ma < m_hi; ma += chunk) {
    const int mb = ma + chunk < m_hi ? ma + chunk : m_hi;
    const int64_t ua = (int64_t)ma * M;
    const int64_t qa = ua / L;                            // j0 of the chunk's first output
    const unsigned ra = (unsigned)(ua - qa * L);
    const int64_t jlo = qa + C - (P - 1);                 // first input sample any output of the chunk reads
    const int n = (int)(((int64_t)(mb - 1) * M) / L + C - jlo) + 1;
    __syncthreads();                                      // the previous chunk's readers are done
    for (int i = threadIdx.x; i < n; i += 256) {
      const int64_t j = jlo + i;
      xs[i] = (j >= 0 && j < s.src_len) ? x[j] : 0.0f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < S && ma + t < mb; t += 256) {
      // (ma + t) * M = ua + t * M: phase and input index from 32-bit arithmetic (t * M < 2^20)
      const unsigned v = ra + (unsigned)t * (unsigned)M;
      const unsigned dj = v / (unsigned)L;
      const float* tp = table + (v - dj * (unsigned)L);
      int xo[RS_R];
      float acc[RS_R];
#pragma unroll
      for (int i = 0; i < RS_R; ++i) {
        // x[j0 + C] of output i relative to jlo; an output past the chunk's end re-reads output 0's samples and is not stored
        xo[i] = (int)dj + (P - 1) + (ma + t + i * S < mb ? i * step : 0);
        acc[i] = 0.0f;
      }
      // eight coefficient loads in flight, then their taps in the order of q (a lone wave would otherwise wait out every load)
      int q = 0;
      for (; q + 8 <= P; q += 8) {
        float c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = tp[(int64_t)(q + k) * L];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
          for (int i = 0; i < RS_R; ++i) acc[i] = fmaf(c[k], xs[xo[i] - q - k], acc[i]);
        }
      }
      for (; q < P; ++q) {
        const float c = tp[(int64_t)q * L];
#pragma unroll
        for (int i = 0; i < RS_R; ++i) acc[i] = fmaf(c, xs[xo[i] - q], acc[i]);
      }
#pragma unroll
      for (int i = 0; i < RS_R; ++i)
        if (ma + t + i * S < mb) put<I16>(dst, (int64_t)s.dst_off + ma + t + i * S, acc[i], scale);
    }
  }
}

// The same sums with every tap read from the source under its own bounds check: one output per thread.
template <bool I16>
__device__ __forceinline__ void segment_direct(const Seg& s, const float* __restrict__ x, const float* __restrict__ table, int L, int M, int P, int C,
                                               void* __restrict__ dst, float scale, int m_lo, int m_hi) {
  for (int m = m_lo + (int)threadIdx.x; m < m_hi; m += 256) {
    const int64_t u = (int64_t)m * M;
    const int64_t j0 = u / L;
    const float* tp = table + (u - j0 * L);
    float acc = 0.0f;
    for (int q = 0; q < P; ++q) {
      const int64_t j = j0 + C - q;
      acc = fmaf(tp[(int64_t)q * L], (j >= 0 && j < s.src_len) ? x[j] : 0.0f, acc);
    }
    put<I16>(dst, (int64_t)s.dst_off + m, acc, scale);
  }
}

template <bool I16, bool STAGE>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ src, int64_t n_src, const Seg* __restrict__ segs, int n_segs,
                                                       const float* __restrict__ table, int L, int M, int P, int C, void* __restrict__ dst,
                                                       int64_t n_dst, float scale, int tile, int S, int groups) {
  __shared__ float xs[STAGE ? RS_LDS : 1];
  __shared__ unsigned long long hits[4];
  const int64_t t0 = (int64_t)blockIdx.x * tile;
  const int64_t t1 = t0 + tile < n_dst ? t0 + tile : n_dst;
  for (int base = 0; base < n_segs; base += 256) {
    const int mine = base + (int)threadIdx.x;
    bool hit = false;
    if (mine < n_segs) {
      const Seg s = segs[mine];
      hit = seg_fits(s, n_src, n_dst) && s.dst_off < t1 && (int64_t)s.dst_off + s.dst_len > t0;
    }
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0) hits[threadIdx.x >> 6] = b;
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
      unsigned long long mask = hits[w];                  // the same for every thread of the workgroup
      while (mask) {
        const int bit = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const Seg s = segs[base + 64 * w + bit];
        // outputs [m_lo, m_hi) of the segment lie in this tile
        const int m_lo = (int)(t0 > s.dst_off ? t0 - s.dst_off : 0);
        const int m_hi = (int)(t1 - s.dst_off < s.dst_len ? t1 - s.dst_off : s.dst_len);
        if constexpr (STAGE)
          segment_staged<I16>(xs, s, src + s.src_off, table, L, M, P, C, dst, scale, S, groups, m_lo, m_hi);
        else
          segment_direct<I16>(s, src + s.src_off, table, L, M, P, C, dst, scale, m_lo, m_hi);
      }
    }
    __syncthreads();                                      // `hits` is rewritten by the next 256 rows
  }
}

bool rs_factor_ok(int L, int M, int P, int C) {
  return L >= 1 && L <= 32768 && M >= 1 && M <= 32768 && P >= 1 && P <= (1 << 20) && C >= 0 && C <= (1 << 20);
}

}  // namespace

extern "C" int ttsk_resample_tile(int L, int M, int P) {
  if (!rs_factor_ok(L, M, P, 0)) return 0;
  return rs_plan(L, M, P).tile;
}

extern "C" int ttsk_resample(const float* src, int64_t n_src, const int32_t* segs, int n_segs, const float* table, int L, int M, int P, int C,
                             void* dst, int64_t n_dst, int to_i16, float scale, void* stream) {
  TTSK_REQUIRE(src && segs && table && dst && n_src > 0 && n_dst > 0 && n_segs > 0, "resample: bad arguments");
  TTSK_REQUIRE(rs_factor_ok(L, M, P, C), "resample: factor %d / %d (each 1..32768), %d taps per phase, centre %d (each up to 2^20): out of range",
               L, M, P, C);
  TTSK_REQUIRE((((uintptr_t)segs) & 15) == 0 && (((uintptr_t)src) & 3) == 0 && (((uintptr_t)table) & 3) == 0 &&
                   (((uintptr_t)dst) & (to_i16 ? 1 : 3)) == 0,
               "resample: the segment table must be 16-byte aligned, the buffers aligned to their element");
  const RsPlan pl = rs_plan(L, M, P);
  const int64_t tiles = (n_dst + pl.tile - 1) / pl.tile;
  TTSK_REQUIRE(tiles <= 0x7fffffff, "resample: destination of %lld samples is too large", (long long)n_dst);
  const Seg* sg = reinterpret_cast<const Seg*>(segs);
#define TTSK_RS_LAUNCH(I16, STAGE)                                                                                                        \
  hipLaunchKernelGGL((resample_kernel<I16, STAGE>), dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, src, n_src, sg, n_segs, table, \
                     L, M, P, C, dst, n_dst, scale, pl.tile, pl.stride, pl.groups)
  if (to_i16) {
    if (pl.groups) TTSK_RS_LAUNCH(true, true); else TTSK_RS_LAUNCH(true, false);
  } else {
    if (pl.groups) TTSK_RS_LAUNCH(false, true); else TTSK_RS_LAUNCH(false, false);
  }
#undef TTSK_RS_LAUNCH
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
