// Windowed vocoding: the two data movers around the HiFi-GAN generator (include/ttsk.h, tts_king_amd/windows.py).
//   mel_windows_kernel   mel staging buffer (fp32, either layout) -> (N, W, C) 16-bit channels-last windows
//   wav_stitch_kernel    (N, spf * W) fp32 window waveforms       -> the kept samples of every window in one flat buffer
// Both read their work from the plan table in device memory (TTSK_WIN_ROW int32 per window), so an utterance's length is data: a
// captured graph holds for every call with the same N.  No atomics, no host synchronisation; every row is checked against the
// buffer sizes before it is used (a row that does not fit is skipped: a wrong plan gives wrong audio, never a wild access).
#include "common.h"
#include "rowlens.h"

namespace {

constexpr int TILE_T = 32;      // frames per tile of mel_windows_kernel

// One workgroup per (window, 32-frame tile), grid-strided.  The tile goes through LDS so that both sides are coalesced whatever the
// source layout: channel-contiguous sources are read as float4 rows, frame-contiguous ones along the frames; the destination tile
// is TILE_T * C contiguous 16-bit values, written as 16-byte pieces of 8 channels.
template <bool F16>
__global__ __launch_bounds__(256) void mel_windows_kernel(const float* __restrict__ src, int64_t st, int64_t sc, int64_t n_src_frames,
                                                          const int* __restrict__ plan, bf16_t* __restrict__ dst, int N, int W, int C) {
  extern __shared__ float tile[];                       // [TILE_T][C + 1]
  const int ldt = C + 1;
  const int tiles_per_win = W / TILE_T;
  const int n_tiles = N * tiles_per_win;
  const bool vec = sc == 1 && (st & 3) == 0 && (((uintptr_t)src) & 15) == 0;
  for (int tix = blockIdx.x; tix < n_tiles; tix += gridDim.x) {
    const int n = tix / tiles_per_win, t0 = (tix - n * tiles_per_win) * TILE_T;
    const int64_t f0 = plan[n * TTSK_WIN_ROW + 5];
    // the row's valid frames (column [6]: 0 = all W): a short utterance's row reads v frames of the staging buffer, not W, and is
    // zero from frame v on — what follows it in the buffer is another utterance, or nothing
    const int vq = plan[n * TTSK_WIN_ROW + TTSK_WIN_VALID];
    const int v = (vq <= 0 || vq > W) ? W : vq;
    const bool live = f0 >= 0 && f0 + v <= n_src_frames;
    const int nt = min(TILE_T, v - t0);                 // frames of this tile that exist (<= 0: none)
    if (live && nt > 0) {
      const float* s = src + (f0 + t0) * st;
      if (vec) {
        const int q = C >> 2;
        for (int i = threadIdx.x; i < TILE_T * q; i += 256) {
          const int t = i / q, c4 = i - t * q;
          if (t >= nt) continue;
          const float4 x4 = *reinterpret_cast<const float4*>(s + (int64_t)t * st + 4 * c4);
          float* d = tile + t * ldt + 4 * c4;
          d[0] = x4.x; d[1] = x4.y; d[2] = x4.z; d[3] = x4.w;
        }
      } else if (sc == 1) {
        for (int i = threadIdx.x; i < TILE_T * C; i += 256) {
          const int t = i / C, c = i - t * C;
          if (t < nt) tile[t * ldt + c] = s[(int64_t)t * st + c];
        }
      } else {
        for (int i = threadIdx.x; i < TILE_T * C; i += 256) {
          const int c = i / TILE_T, t = i - c * TILE_T;
          if (t < nt) tile[t * ldt + c] = s[(int64_t)t * st + (int64_t)c * sc];
        }
      }
    }
    __syncthreads();
    uint4* d = reinterpret_cast<uint4*>(dst + ((int64_t)n * W + t0) * C);
    const int q8 = C >> 3;
    for (int i = threadIdx.x; i < TILE_T * q8; i += 256) {
      uint4 o = make_uint4(0u, 0u, 0u, 0u);
      const int t = i / q8, c8 = i - t * q8;
      if (live && t < nt) {
        const float* p = tile + t * ldt + 8 * c8;
        o = make_uint4(pack2<F16>(p[0], p[1]), pack2<F16>(p[2], p[3]), pack2<F16>(p[4], p[5]), pack2<F16>(p[6], p[7]));
      }
      d[i] = o;
    }
    __syncthreads();
  }
}

// One thread per 8 samples, grid-strided over every (window, frame): frames outside the window's kept range are skipped.  spf is a
// multiple of 8 and every offset a multiple of spf, so the accesses are 16-byte pieces (two float4 in; two float4 or one uint4 out).
template <bool I16>
__global__ __launch_bounds__(256) void wav_stitch_kernel(const float* __restrict__ src, const int* __restrict__ plan, void* __restrict__ dst,
                                                         int64_t n_dst_frames, float scale, int N, int W, int spf) {
  const int p8 = spf >> 3;                              // 8-sample pieces per frame
  const int64_t n = (int64_t)N * W * p8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t fr = i / p8;
    const int piece = (int)(i - fr * p8);
    const int w = (int)(fr / W), f = (int)(fr - (int64_t)w * W);
    const int* row = plan + w * TTSK_WIN_ROW;
    const int start = row[1], lo = row[2], hi = row[3], d0 = row[4];
    const int t = start + f;                            // frame of the utterance
    if (row[5] < 0 || t < lo || t >= hi) continue;
    const int64_t df = (int64_t)d0 + (t - lo);
    if (lo < start || hi > start + W || d0 < 0 || df >= n_dst_frames) continue;
    const float4* s = reinterpret_cast<const float4*>(src + fr * spf + 8 * piece);
    const float4 a = s[0], b = s[1];
    const int64_t o = df * spf + 8 * piece;
    if constexpr (I16) {
      // (x * scale) truncated toward zero, then the low 16 bits: to_int16_kernel's arithmetic (rowops.hip)
      auto cv = [scale](float x, float y) { return ((unsigned)(int)(x * scale) & 0xFFFFu) | ((unsigned)(int)(y * scale) << 16); };
      *reinterpret_cast<uint4*>((short*)dst + o) = make_uint4(cv(a.x, a.y), cv(a.z, a.w), cv(b.x, b.y), cv(b.z, b.w));
    } else {
      float4* d = reinterpret_cast<float4*>((float*)dst + o);
      d[0] = a; d[1] = b;
    }
  }
}

// (B, len, C) 16-bit: the frames of row b from its edge on (rowlens.h) are set to zero; one thread per 16 bytes, grid-strided over the
// rows' tails only.  What conv_pre leaves past a short row's end (its bias, and the taps that reach back into the row) must not
// reach the first upsampler.
__global__ __launch_bounds__(256) void zero_rows_past_kernel(uint4* __restrict__ x, int B, int len, int q8, RowLens rl) {
  const int b = blockIdx.y;
  const int e = row_edge(rl, b, len);
  uint4* row = x + (int64_t)b * len * q8;
  const int64_t n = (int64_t)(len - e) * q8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) row[(int64_t)e * q8 + i] = make_uint4(0u, 0u, 0u, 0u);
}

// workgroups for a grid-strided kernel: `per_cu` per compute unit of the current device, never more than the work needs
int grid_by_cus(int64_t work_items, int per_cu) {
  static int n_cus = 0;
  if (n_cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return -1;
    n_cus = v;
  }
  const int64_t cap = (int64_t)n_cus * per_cu;
  return (int)(work_items < cap ? (work_items < 1 ? 1 : work_items) : cap);
}

}  // namespace

extern "C" int ttsk_mel_windows(const float* src, int64_t stride_t, int64_t stride_c, int64_t n_src_frames, const int32_t* plan, void* dst16,
                                int f16, int N, int W, int C, void* stream) {
  TTSK_REQUIRE(src && plan && dst16 && N > 0 && W > 0 && C > 0 && n_src_frames > 0, "mel_windows: bad arguments");
  TTSK_REQUIRE(W % TILE_T == 0 && C % 8 == 0 && C <= 256, "mel_windows: W=%d must be a multiple of %d, C=%d a multiple of 8 (<= 256)", W, TILE_T, C);
  TTSK_REQUIRE((stride_t == 1 && stride_c >= n_src_frames) || (stride_c == 1 && stride_t >= C),
               "mel_windows: strides (%lld, %lld): one of them must be 1 and the other span a row", (long long)stride_t, (long long)stride_c);
  TTSK_REQUIRE((((uintptr_t)dst16) & 15) == 0, "mel_windows: destination must be 16-byte aligned");
  const int grid = grid_by_cus((int64_t)N * (W / TILE_T), 4);
  TTSK_REQUIRE(grid > 0, "mel_windows: cannot read the device's compute-unit count");
  const size_t lds = (size_t)TILE_T * (C + 1) * sizeof(float);
  if (f16)
    hipLaunchKernelGGL(mel_windows_kernel<true>, dim3(grid), dim3(256), lds, (hipStream_t)stream, src, stride_t, stride_c, n_src_frames,
                       (const int*)plan, (bf16_t*)dst16, N, W, C);
  else
    hipLaunchKernelGGL(mel_windows_kernel<false>, dim3(grid), dim3(256), lds, (hipStream_t)stream, src, stride_t, stride_c, n_src_frames,
                       (const int*)plan, (bf16_t*)dst16, N, W, C);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_wav_stitch(const float* src, const int32_t* plan, void* dst, int64_t n_dst_frames, int to_i16, float scale, int N, int W,
                               int spf, void* stream) {
  TTSK_REQUIRE(src && plan && dst && N > 0 && W > 0 && spf > 0 && n_dst_frames > 0, "wav_stitch: bad arguments");
  TTSK_REQUIRE(spf % 8 == 0, "wav_stitch: %d samples per frame, must be a multiple of 8", spf);
  TTSK_REQUIRE((((uintptr_t)src) & 15) == 0 && (((uintptr_t)dst) & 15) == 0, "wav_stitch: buffers must be 16-byte aligned");
  const int64_t pieces = (int64_t)N * W * (spf >> 3);
  const int grid = grid_by_cus((pieces + 255) / 256, 8);
  TTSK_REQUIRE(grid > 0, "wav_stitch: cannot read the device's compute-unit count");
  if (to_i16)
    hipLaunchKernelGGL(wav_stitch_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (const int*)plan, dst, n_dst_frames, scale,
                       N, W, spf);
  else
    hipLaunchKernelGGL(wav_stitch_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (const int*)plan, dst, n_dst_frames, scale,
                       N, W, spf);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_zero_rows_past(void* x16, int B, int len, int C, const int32_t* row_frames, int row_stride, int spf, void* stream) {
  TTSK_REQUIRE(x16 && B > 0 && len > 0 && C > 0 && B <= 65535, "zero_rows_past: bad arguments");
  TTSK_REQUIRE_ROWS("zero_rows_past", row_stride, spf);
  TTSK_REQUIRE(C % 8 == 0 && (((uintptr_t)x16) & 15) == 0, "zero_rows_past: C=%d must be a multiple of 8 and the tensor 16-byte aligned", C);
  if (!row_frames) return TTSK_OK;                      // every row full: nothing lies past an end
  const int q8 = C >> 3;
  const int64_t per_row = ((int64_t)len * q8 + 255) / 256;
  const dim3 grid((unsigned)(per_row < 64 ? per_row : 64), B);
  hipLaunchKernelGGL(zero_rows_past_kernel, grid, dim3(256), 0, (hipStream_t)stream, (uint4*)x16, B, len, q8, RowLens{row_frames, row_stride, spf});
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
