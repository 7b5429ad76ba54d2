// pairparts.h — the stages the HiFi-GAN pair kernels (convwin.hip: conv_pair_kernel, conv_pair256_kernel, conv_pair_fs_kernel) and the
// ResBlock2 kernel (resblock2.hip) have in common, each written once: the x window fill, the weight addressing of the two wave
// layouts, the plain tap nest, the t window store, the MRF finish, the copy-out of staged rows, and on the host the WithRows
// dispatch and the argument checks.  A kernel is its geometry, its tap schedule and calls of these.  Every rule they encode — zero
// padding outside [0, len), the per-row edge of rowlens.h, the three MRF modes, "weights are requested behind the window" — is
// stated here.  (pairws.hip, resblock.hip, mrf32.hip and conv_window2_kernel fill their windows with a swizzle, by
// LDS-DMA or with a second store: they keep their own.)  tests/test_pair_bits_gpu.py pins the bits of every instantiation.
#pragma once
#include <climits>
#include <type_traits>
#include "common.h"
#include "rowlens.h"

// ---- x window: lrelu(x) rows t_first .. t_first + XROWS of one batch row `xb` into LDS, zeros outside [0, len).  The window is sized
// for the widest dilation; only rows [xlo, xhi) — what the first conv reads at this dilation — are fetched, the others stay zero and
// nobody reads them.  In two halves: x_window_request puts every load in flight, x_window_store does the LeakyReLU and the LDS stores;
// BETWEEN the two calls a kernel requests its first two weight sets, BEHIND the window (loads return in order, and nothing starts
// before the window is in LDS).  (One function that took those requests as a callable cost conv_pair_kernel its loop shape: c1's tap
// loop came out rotated, with 28 register copies per trip and 0.9 % more time over the nine C = 128 pairs; profiles/pair_parts_ab.json.)
template <int C, int XROWS, int NT> constexpr int x_window_chunks() { return (XROWS * (C / 8) + NT - 1) / NT; }
template <int C, int XROWS, int NT, int NCH>
__device__ __forceinline__ void x_window_request(uint4 (&xv)[NCH], const bf16_t* __restrict__ xb, int t_first, int len, int xlo, int xhi, int tid) {
  constexpr int CH8 = C / 8;
#pragma unroll
  for (int it = 0; it < NCH; ++it) {
    const int idx = it * NT + tid;
    const int row = idx / CH8, ch = idx - row * CH8;
    const int t = t_first + row;
    xv[it] = make_uint4(0, 0, 0, 0);
    if (idx < XROWS * CH8 && t >= 0 && t < len && row >= xlo && row < xhi) xv[it] = *(const uint4*)(xb + (int64_t)t * C + ch * 8);
  }
}
template <bool F16, int C, int XROWS, int NT, int RS, int NCH>
__device__ __forceinline__ void x_window_store(unsigned char* XW, const uint4 (&xv)[NCH], float slope, int tid) {
  constexpr int CH8 = C / 8;
#pragma unroll
  for (int it = 0; it < NCH; ++it) {
    const int idx = it * NT + tid;
    const int row = idx / CH8, ch = idx - row * CH8;
    if (idx < XROWS * CH8) *(uint4*)(XW + row * RS + ch * 16) = lrelu8_fast<F16>(xv[it], slope);
  }
}

// ---- wave = 32 output channels x all frames (C = 128 / 256), rows of the A operand PERMUTED (round 6, as csrc/pairws.hip): row l15 of
// tile cc is channel 32 * wave + 8 * (l15 >> 2) + 4 * cc + (l15 & 3), so that a lane's 4 + 4 accumulator rows of the two tiles are 8
// CONSECUTIVE channels of one frame — one 16-byte LDS / global store per frame tile and lane instead of two 8-byte ones (whose rows
// collided four ways in LDS: 17 % of the kernel's LDS cycles), and the output needs no staging tile, barrier and copy-out.  Same
// products, same order: bit-identical.  woff[cc]: this lane's byte offset into a k-step of a fragment-major pack.
__device__ __forceinline__ int perm_woff(int wave, int l15, int q, int cc) {
  const int co = 32 * wave + 8 * (l15 >> 2) + 4 * cc + (l15 & 3);
  return (co >> 4) * 1024 + ((co & 15) + 16 * q) * 16;
}
__device__ __forceinline__ int perm_co8(int wave, int q) { return 32 * wave + 8 * q; }      // this lane's 8 output channels

// ---- wave = (cout group cgi of CT tiles, frame group) (C = 64 / 32, ResBlock2): tap g of the 2K-tap sequence first conv | second conv
template <int KS, int CT, int NC>
__device__ __forceinline__ void load_taps_cg(bf16x8 (&w)[KS][CT], const bf16_t* wA, const bf16_t* wB, int K, int TAP, int cgi, int lane, int g) {
  const unsigned char* src = (const unsigned char*)(g < K ? wA : wB) + (int64_t)(g < K ? g : g - K) * TAP + (cgi * CT) * 1024 + lane * 16;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int c = 0; c < CT; ++c) w[ks][c] = *(const bf16x8*)(src + (ks * NC + c) * 1024);
}

template <int CT, int NF>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[CT][NF]) {
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int i = 0; i < NF; ++i) acc[c][i] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- one tap: acc += w (x) the NF frame tiles at `inp` (this lane's fragment address at the tap's shift).  The plain nest: the
// 2-workgroup kernels measured 1 % slower with tapring.h's ring.  FIRST as there: the tap starts the sums, its first k-step multiplies
// onto the constant 0 instead of onto accumulators somebody had to zero; same sums, bit for bit.
template <bool F16, int KS, int CT, int NF, int RS, bool FIRST = false>
__device__ __forceinline__ void tap_plain(f32x4 (&acc)[CT][NF], const bf16x8 (&w)[KS][CT], const unsigned char* inp) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const bf16x8 Bf = *(const bf16x8*)(inp + i * 16 * RS + ks * 64);
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c][i] = mfma16<F16>(w[ks][c], Bf, (FIRST && ks == 0) ? zero4 : acc[c][i]);
    }
  }
}

// ---- t window (permuted layout): t = lrelu(acc + b1) as 16-bit rows t_first .. t_first + 16 NF, 16 bytes per lane and frame tile;
// frames outside [0, len) are the second conv's zero padding.  A tile whose t window lies inside the utterance has no zero padding to
// write: no compare, no select — and the conversions pack in pairs.
template <bool F16, int NF, int RS>
__device__ __forceinline__ void store_t_rows(unsigned char* TW, const f32x4 (&acc)[2][NF], const f32x4 (&bv)[2], float slope, int t_first, int len,
                                             int l15, int co8) {
  auto rows = [&](auto all_live) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int t = t_first + i * 16 + l15;
      const bool live = decltype(all_live)::value || (t >= 0 && t < len);
      unsigned o[4];
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        f32x4 v = acc[cc][i] + bv[cc];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = live ? fmaxf(v[e], v[e] * slope) : 0.f;
        o[cc * 2] = pack2<F16>(v[0], v[1]);
        o[cc * 2 + 1] = pack2<F16>(v[2], v[3]);
      }
      *(uint4*)(TW + (i * 16 + l15) * RS + co8 * 2) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  };
  if (t_first >= 0 && t_first + NF * 16 <= len) rows(std::true_type{});
  else rows(std::false_type{});
}

// ---- MRF finish of four channels of one frame: v = conv + bias comes in; + residual (two packed words), then per `mode`
// 0: y   1: out + y   2: lrelu((out + y) * scale, final_slope) with `out` as two packed words (hifi/models.py:190-197); packed.
template <bool F16>
__device__ __forceinline__ uint2 mrf_finish(f32x4 v, unsigned r01, unsigned r23, unsigned o01, unsigned o23, int mode, float scale, float final_slope) {
  float r0, r1, r2, r3;
  unpack2<F16>(r01, r0, r1); unpack2<F16>(r23, r2, r3);
  v += f32x4{r0, r1, r2, r3};
  if (mode) {
    float o0, o1, o2, o3;
    unpack2<F16>(o01, o0, o1); unpack2<F16>(o23, o2, o3);
    v += f32x4{o0, o1, o2, o3};
    if (mode == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] *= scale; v[e] = fmaxf(v[e], v[e] * final_slope); }
    }
  }
  return make_uint2(pack2<F16>(v[0], v[1]), pack2<F16>(v[2], v[3]));
}
// ... of a lane's 8 consecutive channels (the permuted layout: tile 0's four, then tile 1's)
template <bool F16>
__device__ __forceinline__ uint4 mrf_finish8(f32x4 v0, f32x4 v1, uint4 res, uint4 out, int mode, float scale, float final_slope) {
  const uint2 a = mrf_finish<F16>(v0, res.x, res.y, out.x, out.y, mode, scale, final_slope);
  const uint2 b = mrf_finish<F16>(v1, res.z, res.w, out.z, out.w, mode, scale, final_slope);
  return make_uint4(a.x, a.y, b.x, b.y);
}

// ---- the TT staged rows at SRC (LDS) -> frames t0 .. of `ob`, full-row 16-byte stores, nothing at or past `len`
template <int C, int TT, int NT, int RS>
__device__ __forceinline__ void copy_out_rows(bf16_t* __restrict__ ob, const unsigned char* SRC, int t0, int len, int tid) {
  constexpr int CH8 = C / 8, NCO = (TT * CH8 + NT - 1) / NT;
#pragma unroll
  for (int it = 0; it < NCO; ++it) {
    const int idx = it * NT + tid;
    const int rr = idx / CH8, ch = idx - rr * CH8;
    const int t = t0 + rr;
    if (idx < TT * CH8 && t < len) *(uint4*)(ob + (int64_t)t * C + ch * 8) = *(const uint4*)(SRC + rr * RS + ch * 16);
  }
}

// ---- host: fn(arguments) on the plain block (`rl` null) or on its WithRows form: one body for an entry point and its *_rowlen twin
template <typename A, typename Fn>
inline void launch_with_rows(const A& a, const RowLens* rl, Fn&& fn) {
  if (rl) {
    WithRows<A> ar;
    static_cast<A&>(ar) = a;
    ar.rl = *rl;
    fn(ar);
  } else {
    fn(a);
  }
}

// ---- host: the argument checks ttsk_hifi_conv_pair and ttsk_hifi_resblock2 share.  `name`: the entry point the error texts name;
// `inst`: what its *_supported() answered; `inst_fmt`: its whole error text, a format of C, K and up to two more conv parameters.
inline int pair_args_check(const char* name, const void* x, const void* wA, const float* bA, const void* wB, const float* bB, const void* out,
                           int B, int len, int max_len, bool inst, const char* inst_fmt, int C, int K, int p0, int p1, float slope, int mode,
                           float final_slope) {
  TTSK_REQUIRE(x && wA && bA && wB && bB && out, "%s: null pointer", name);
  TTSK_REQUIRE(B > 0 && len > 0 && B <= 65535 && len <= max_len && x != out, "%s: bad sizes / in-place output", name);
  TTSK_REQUIRE(inst, inst_fmt, C, K, p0, p1);
  TTSK_REQUIRE(mode >= 0 && mode <= 2 && (final_slope > 0.f || mode != 2), "%s: bad mode / final_slope", name);
  TTSK_REQUIRE(slope > 0.f && slope < 1.f, "%s: LeakyReLU slope %g outside (0, 1)", name, slope);
  TTSK_REQUIRE(((((uintptr_t)x) | ((uintptr_t)wA) | ((uintptr_t)wB) | ((uintptr_t)bA) | ((uintptr_t)bB) | ((uintptr_t)out)) & 15) == 0,
               "%s: 16-byte alignment", name);
  return TTSK_OK;
}
