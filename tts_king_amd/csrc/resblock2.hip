// resblock2.hip — the HiFi-GAN ResBlock2 (the block of the V3 generator) as ONE launch per block.
// reference: hifi/models.py:104-143 (ResBlock2: for c in convs: xt = c(leaky_relu(x, 0.1)); x = xt + x), :190-197 (MRF average).
//
// y = x1 + b1 + conv_{K,d1}(lrelu(x1)),  x1 = x + b0 + conv_{K,d0}(lrelu(x)).  The conv-by-conv route writes x1 and lrelu(x1) to
// HBM and reads them back, and leaves the MRF average to a separate pass; here a workgroup loads lrelu(x) for its frame tile and
// both halos once (x window in LDS), computes x1 over the tile plus conv1's halo, keeps lrelu(x1) as 16-bit rows of a second LDS
// window (zero outside [0, len): conv1's padding, not x1 values computed there) and x1 itself for the tile rows (conv1's residual),
// then runs conv1 and stores with ttsk_hifi_conv_pair's MRF modes.  x1 is rounded to the 16-bit type before both uses, where the
// conv-by-conv route stores it; lrelu(x1) is taken of the rounded value.
//
// Layout as conv_pair_fs_kernel (csrc/convwin.hip): D[cout][frame] MFMA orientation, four waves split into (32-channel cout group,
// frame group), weights streamed L2 -> registers from ttsk_pack_resblock_weight packs as one double-buffered sequence of 2K taps.
// C = 128: 4 cout groups x 96 frames (64 at the widest halo); C = 64: 2 x 2 x 96 frames; C = 32: 1 x 4 x 48 frames.  conv0 computes EW extra frame tiles
// per wave (the conv1 halo, G1 = 8 * FG * EW frames either side); an instance is picked per (C, EW) from the halo HK * d1.
// The stages it shares with them (x window fill, weight addressing, tap nest, MRF finish, copy-out, host checks) are pairparts.h's.
#include "common.h"
#include "pairparts.h"

namespace {

struct Rb2Args {
  const bf16_t* x;      // (B, len, C) 16-bit, raw block input
  const bf16_t* w0;     // fragment-major packs [Kpad][C/32][C/16][64][8] (ttsk_pack_resblock_weight)
  const bf16_t* w1;
  const float* b0;
  const float* b1;
  bf16_t* out;          // (B, len, C), stored per `mode`
  int len, K, d0, d1;
  float slope;
  int mode;             // 0: out = y   1: out += y   2: out = lrelu((out + y) * scale, final_slope)
  float scale, final_slope;
};

constexpr int RB2_H0 = 16;     // conv0 halo the x window carries on top of conv1's: HK * d0 <= 16

template <int C, int EW> struct Rb2Geom {
  static constexpr int NW = 4, NT = NW * 64;
  static constexpr int CG = C >= 64 ? C / 32 : 1, FG = NW / CG;          // cout groups x frame groups
  static constexpr int NC = C / 16, KS = C / 32, CT = NC / CG;
  // conv1 frame tiles per wave; the widest C = 128 halo takes 64-frame tiles (11 conv0 tiles of accumulators next to the residual and
  // the streamed weights went past 256 registers)
  static constexpr int NF2 = C == 32 ? 3 : (C == 128 && EW > 2 ? 4 : 6);
  static constexpr int NF1 = NF2 + EW;                                 // conv0 frame tiles per wave
  static constexpr int TT = FG * NF2 * 16;                             // frames stored per workgroup
  static constexpr int G1 = 8 * FG * EW;                               // conv1 halo covered: HK * d1 <= G1
  static constexpr int TROWS = FG * NF1 * 16;                          // = TT + 2 * G1 rows of x1
  static constexpr int XROWS = TROWS + 2 * RB2_H0;
  static constexpr int RS = C * 2 + 32;                                // 2 mod 4 sixteen-byte units: conflict-free fragment reads
  static constexpr int TAP = NC * KS * 1024;
  // the x window lives until conv0 is done; then the lrelu(x1) window (rows 0 .. TROWS) and the x1 / output rows (TT more) reuse it
  static constexpr int SMEM = (XROWS > TROWS + TT ? XROWS : TROWS + TT) * RS;
  static_assert(CT * CG == NC && FG * CG == NW, "geometry");
  static_assert(SMEM <= 80 * 1024, "two workgroups per CU");
};

template <int C, int EW, bool F16, typename A = Rb2Args>
__global__ __launch_bounds__(256, 2) void resblock2_kernel(const A a) {
  using Gm = Rb2Geom<C, EW>;
  constexpr int NT = Gm::NT, NF1 = Gm::NF1, NF2 = Gm::NF2, TT = Gm::TT, G1 = Gm::G1, TROWS = Gm::TROWS, XROWS = Gm::XROWS,
                RS = Gm::RS, NC = Gm::NC, KS = Gm::KS, CT = Gm::CT, CG = Gm::CG, TAP = Gm::TAP, H0M = RB2_H0;
  __shared__ __attribute__((aligned(16))) unsigned char smem[Gm::SMEM];
  unsigned char* XW = smem;                       // lrelu(x) rows t0 - G1 - 16 .. t0 + TT + G1 + 16 (conv0 only)
  unsigned char* TW = smem;                       // lrelu(x1) rows t0 - G1 .. t0 + TT + G1 (after conv0)
  unsigned char* RW = smem + TROWS * RS;          // x1 rows t0 .. t0 + TT, then the output rows (after conv0)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int cgi = wave % CG, fg = wave / CG;
  const int bi = blockIdx.y, t0 = blockIdx.x * TT;
  const int slen = a.len, K = a.K, d0 = a.d0, d1 = a.d1;      // slen: the batch's row stride; len: this row's edge (rowlens.h)
  const int len = edge_len(a, bi);
  if constexpr (HasRows<A>::value) {
    if (t0 >= len) return;      // a tile wholly past the row's end: nothing to read, nothing to store (`out` is zero there)
  }
  const int HK = (K - 1) / 2;
  const bf16_t* __restrict__ xb = a.x + (int64_t)bi * slen * C;

  bf16x8 wa[KS][CT], wb[KS][CT];
  auto load_w = [&](int g, bf16x8 (&w)[KS][CT]) __attribute__((always_inline)) {      // tap g of the 2K-tap sequence conv0 | conv1
    load_taps_cg<KS, CT, NC>(w, a.w0, a.w1, K, TAP, cgi, lane, g);
  };

  // ---- x window: lrelu(x), zeros outside the utterance; only the rows conv0 reads at this dilation are fetched
  uint4 xv[x_window_chunks<C, XROWS, NT>()];
  x_window_request<C, XROWS, NT>(xv, xb, t0 - G1 - H0M, len, H0M - HK * d0, H0M + TROWS + HK * d0, tid);
  load_w(0, wa);
  load_w(1, wb);
  x_window_store<F16, C, XROWS, NT, RS>(XW, xv, a.slope, tid);
  f32x4 bv0[CT], bv1[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    bv0[c] = *(const f32x4*)(a.b0 + (cgi * CT + c) * 16 + q * 4);
    bv1[c] = *(const f32x4*)(a.b1 + (cgi * CT + c) * 16 + q * 4);
  }
  __syncthreads();

  // ---- conv0: row r = fg * NF1 * 16 + i * 16 + l15 <-> frame t0 - G1 + r <-> x-window row r + 16
  f32x4 acc[CT][NF1];
  zero_acc(acc);
  auto tap0 = [&](const unsigned char* inp, const bf16x8 (&w)[KS][CT]) __attribute__((always_inline)) {
    tap_plain<F16, KS, CT, NF1, RS>(acc, w, inp);
  };
  {
    // K is odd and >= 3: taps 0 .. K-2 in pairs, tap K-1 on set a; conv1 then starts on set b
    const unsigned char* inl = XW + (fg * NF1 * 16 + l15 + H0M) * RS + q * 16;
#pragma unroll 1
    for (int g = 0; g + 1 < K; g += 2) {
      tap0(inl + (g - HK) * d0 * RS, wa);
      load_w(g + 2, wa);
      tap0(inl + (g + 1 - HK) * d0 * RS, wb);
      load_w(g + 3, wb);
    }
    tap0(inl + (K - 1 - HK) * d0 * RS, wa);
    load_w(K + 1, wa);
  }
  // raw x at this lane's conv0 rows (conv0's residual; an L2 hit: the window just read them).  Requested after the taps, not before:
  // held across them, these registers pushed the C = 128 instances into scratch
  uint2 rx[CT][NF1];
#pragma unroll
  for (int i = 0; i < NF1; ++i) {
    const int t = t0 - G1 + fg * NF1 * 16 + i * 16 + l15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      rx[c][i] = make_uint2(0u, 0u);
      if (t >= 0 && t < len) rx[c][i] = *(const uint2*)(xb + (int64_t)t * C + (cgi * CT + c) * 16 + q * 4);
    }
  }
  __syncthreads();          // every wave is done with the x window: the x1 windows overwrite it

  // x1 = conv0 + b0 + x rounded to 16 bits; lrelu(x1) rows for conv1 (zero outside [0, len)), x1 rows of the tile for its residual
#pragma unroll
  for (int i = 0; i < NF1; ++i) {
    const int r = fg * NF1 * 16 + i * 16 + l15;
    const int t = t0 - G1 + r;
    const bool live = t >= 0 && t < len;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int co = (cgi * CT + c) * 16 + q * 4;
      f32x4 v = acc[c][i] + bv0[c];
      float r0, r1, r2, r3;
      unpack2<F16>(rx[c][i].x, r0, r1); unpack2<F16>(rx[c][i].y, r2, r3);
      v += f32x4{r0, r1, r2, r3};
      uint2 x1 = make_uint2(pack2<F16>(v[0], v[1]), pack2<F16>(v[2], v[3]));
      if (!live) x1 = make_uint2(0u, 0u);
      *(uint2*)(TW + r * RS + co * 2) = make_uint2(lrelu2_fast<F16>(x1.x, a.slope), lrelu2_fast<F16>(x1.y, a.slope));
      if (r >= G1 && r < G1 + TT) *(uint2*)(RW + (r - G1) * RS + co * 2) = x1;
    }
  }
  __syncthreads();

  // the current `out` in the accumulating modes: requested now, consumed after conv1's taps
  uint2 rout[CT][NF2];
#pragma unroll
  for (int j = 0; j < NF2; ++j) {
    const int t = t0 + fg * NF2 * 16 + j * 16 + l15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      rout[c][j] = make_uint2(0u, 0u);
      if (a.mode && t < len) rout[c][j] = *(const uint2*)(a.out + ((int64_t)bi * slen + t) * C + (cgi * CT + c) * 16 + q * 4);
    }
  }
  // ---- conv1: output frame f = fg * NF2 * 16 + j * 16 + l15 <-> lrelu(x1) row f + G1; taps K .. 2K-1 of the sequence
  f32x4 acc2[CT][NF2];
  zero_acc(acc2);
  auto tap1 = [&](const unsigned char* inp, const bf16x8 (&w)[KS][CT]) __attribute__((always_inline)) {
    tap_plain<F16, KS, CT, NF2, RS>(acc2, w, inp);
  };
  {
    const unsigned char* inl = TW + (fg * NF2 * 16 + l15 + G1) * RS + q * 16;
    tap1(inl - HK * d1 * RS, wb);
    load_w(K + 2, wb);
    tap1(inl + (1 - HK) * d1 * RS, wa);
    if (3 < K) load_w(K + 3, wa);
#pragma unroll 1
    for (int g = 2; g + 1 < K; g += 2) {
      tap1(inl + (g - HK) * d1 * RS, wb);
      if (g + 2 < K) load_w(K + g + 2, wb);
      tap1(inl + (g + 1 - HK) * d1 * RS, wa);
      if (g + 3 < K) load_w(K + g + 3, wa);
    }
    tap1(inl + (K - 1 - HK) * d1 * RS, wb);
  }

  // ---- epilogue: + b1 + x1 (+ the running sum, MRF mode), written over the lane's own x1 entry, then full-row stores
#pragma unroll
  for (int j = 0; j < NF2; ++j) {
    const int f = fg * NF2 * 16 + j * 16 + l15;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int co = (cgi * CT + c) * 16 + q * 4;
      unsigned char* rp = RW + f * RS + co * 2;
      const uint2 x1 = *(const uint2*)rp;
      *(uint2*)rp = mrf_finish<F16>(acc2[c][j] + bv1[c], x1.x, x1.y, rout[c][j].x, rout[c][j].y, a.mode, a.scale, a.final_slope);
    }
  }
  __syncthreads();
  copy_out_rows<C, TT, NT, RS>(a.out + (int64_t)bi * slen * C, RW, t0, len, tid);
}

// conv1 halo G1 = 8 * FG * EW of each instance: C = 128 (FG = 1): 8 / 16 / 40; C = 64 (FG = 2): 16 / 48; C = 32 (FG = 4): 32 / 64
int rb2_max_h1(int C) { return C == 128 ? 40 : (C == 64 ? 48 : 64); }

template <int C, int EW, typename A>
void launch_rb2(const A& a, int B, int f16, hipStream_t s) {
  using Gm = Rb2Geom<C, EW>;
  dim3 grid((a.len + Gm::TT - 1) / Gm::TT, B);
  if (f16) hipLaunchKernelGGL((resblock2_kernel<C, EW, true, A>), grid, dim3(Gm::NT), 0, s, a);
  else hipLaunchKernelGGL((resblock2_kernel<C, EW, false, A>), grid, dim3(Gm::NT), 0, s, a);
}

template <typename A>
void dispatch_rb2(const A& a, int B, int f16, int C, int h1, hipStream_t s) {
  if (C == 128) {
    if (h1 <= 8) launch_rb2<128, 1>(a, B, f16, s);
    else if (h1 <= 16) launch_rb2<128, 2>(a, B, f16, s);
    else launch_rb2<128, 5>(a, B, f16, s);
  } else if (C == 64) {
    if (h1 <= 16) launch_rb2<64, 1>(a, B, f16, s);
    else launch_rb2<64, 3>(a, B, f16, s);
  } else {
    if (h1 <= 32) launch_rb2<32, 1>(a, B, f16, s);
    else launch_rb2<32, 2>(a, B, f16, s);
  }
}

}  // namespace

extern "C" int ttsk_hifi_resblock2_supported(int C, int K, int d0, int d1) {
  if (!(C == 128 || C == 64 || C == 32) || !(K == 3 || K == 5 || K == 7)) return 0;
  const int HK = (K - 1) / 2;
  return d0 >= 1 && d0 <= RB2_H0 && d1 >= 1 && d1 <= 64 && HK * d0 <= RB2_H0 && HK * d1 <= rb2_max_h1(C);
}

static int resblock2_impl(const void* x16, const void* w0_pack, const float* bias0, const void* w1_pack, const float* bias1,
                          void* out16, int f16, int B, int len, int C, int K, int d0, int d1, float slope, int mode, float scale,
                          float final_slope, const RowLens* rl, void* stream) {
  if (const int rc = pair_args_check("ttsk_hifi_resblock2", x16, w0_pack, bias0, w1_pack, bias1, out16, B, len, 1 << 30,
                                     ttsk_hifi_resblock2_supported(C, K, d0, d1), "ttsk_hifi_resblock2: no instance for C=%d K=%d d=(%d,%d)",
                                     C, K, d0, d1, slope, mode, final_slope))
    return rc;
  const Rb2Args a{(const bf16_t*)x16, (const bf16_t*)w0_pack, (const bf16_t*)w1_pack, bias0, bias1, (bf16_t*)out16, len, K, d0, d1, slope,
                  mode, scale, final_slope};
  const int h1 = (K - 1) / 2 * d1;
  launch_with_rows(a, rl, [&](const auto& args) { dispatch_rb2(args, B, f16, C, h1, (hipStream_t)stream); });
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_hifi_resblock2(const void* x16, const void* w0_pack, const float* bias0, const void* w1_pack, const float* bias1,
                                   void* out16, int f16, int B, int len, int C, int K, int d0, int d1, float slope, int mode, float scale,
                                   float final_slope, void* stream) {
  return resblock2_impl(x16, w0_pack, bias0, w1_pack, bias1, out16, f16, B, len, C, K, d0, d1, slope, mode, scale, final_slope, nullptr, stream);
}

extern "C" int ttsk_hifi_resblock2_rowlen(const void* x16, const void* w0_pack, const float* bias0, const void* w1_pack, const float* bias1,
                                        void* out16, int f16, int B, int len, int C, int K, int d0, int d1, float slope, int mode, float scale,
                                        float final_slope, const int32_t* row_frames, int row_stride, int spf, void* stream) {
  TTSK_REQUIRE_ROWS("ttsk_hifi_resblock2_rowlen", row_stride, spf);
  const RowLens rl{row_frames, row_stride, spf};
  return resblock2_impl(x16, w0_pack, bias0, w1_pack, bias1, out16, f16, B, len, C, K, d0, d1, slope, mode, scale, final_slope, &rl, stream);
}
