// dtw.hip — dynamic time warping of B pairs of feature sequences: forced alignment of a synthesized mel (whose frames belong to
// known phonemes) to a recording's mel (the definition is in include/ttsk.h).  Two kernels per launch:
// the local costs D, written skewed by anti-diagonal, then one workgroup per pair that walks the anti-diagonals, backtracks and
// counts the frames per phoneme.  No grid-wide barrier, no wait that spans workgroups, no atomics.
#include <math.h>
#include "common.h"

namespace {

constexpr int DTW_MAX_T = 2048;        // frames per sequence: three live diagonals of DTW_MAX_T floats sit in LDS
constexpr int DTW_MAX_C = 128;
constexpr int DTW_MAX_L = 1024;        // phonemes per row: 16 per lane of the scanning wave
constexpr int DTW_TILE = 64;           // the cost kernel's tile of D
constexpr int DTW_CK = 32;             // channels per LDS chunk
constexpr int DTW_COST_THREADS = 256;
constexpr int DTW_WIN = 64;            // the backtrack's window: DTW_WIN diagonals x DTW_WIN rows of back-pointers in LDS

__device__ __forceinline__ int clamp_len(const int* lens, int b, int ld) {
  int n = lens ? lens[b] : ld;
  return n < 0 ? 0 : (n > ld ? ld : n);
}

// Workspace: per pair (ldx + ldy) * ldx floats of D, all pairs first, then per pair as many bytes of back-pointers.  Both are
// skewed: cell (i, j) lives at (i + j) * ldx + i, so that the cells of one anti-diagonal are contiguous in i.
__device__ __forceinline__ int64_t skew_elems(int ldx, int ldy) { return (int64_t)(ldx + ldy) * ldx; }

// D(i, j) = sum_c (x[i, c] - y[j, c])^2 for one 64 x 64 tile.  The channels go through LDS in chunks of 32 (zeros past C); lane l of
// every wave owns row i0 + l and keeps its chunk of x in registers, wave w owns the tile's anti-diagonals w, w + 4, ...: on diagonal
// kk the lane's cell is column kk - l, so a wave reads 64 different rows of ys (row stride 33 words: conflict-free) and writes a
// contiguous run of the skewed D.  VEC: 16-byte global loads (C % 4 == 0 and 16-byte aligned bases).
template <bool VEC>
__global__ __launch_bounds__(DTW_COST_THREADS) void dtw_cost_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                     const int* __restrict__ x_lens, const int* __restrict__ y_lens,
                                                                     int ldx, int ldy, int C, float* __restrict__ D) {
  __shared__ float xs[DTW_TILE][DTW_CK + 1];
  __shared__ float ys[DTW_TILE][DTW_CK + 1];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int Tx = clamp_len(x_lens, b, ldx), Ty = clamp_len(y_lens, b, ldy);
  const int i0 = blockIdx.y * DTW_TILE, j0 = blockIdx.x * DTW_TILE;
  if (i0 >= Tx || j0 >= Ty) return;            // uniform over the workgroup, before any barrier
  const float* xb = x + (int64_t)b * ldx * C;
  const float* yb = y + (int64_t)b * ldy * C;
  float acc[DTW_TILE / 2];
#pragma unroll
  for (int d = 0; d < DTW_TILE / 2; ++d) acc[d] = 0.f;
  for (int c0 = 0; c0 < C; c0 += DTW_CK) {     // the trip count depends on C only
    if constexpr (VEC) {
      for (int idx = tid; idx < DTW_TILE * DTW_CK / 4; idx += DTW_COST_THREADS) {
        const int r = idx >> 3, c = c0 + 4 * (idx & 7);
        float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vy = vx;
        if (c < C && i0 + r < Tx) vx = *reinterpret_cast<const float4*>(xb + (int64_t)(i0 + r) * C + c);
        if (c < C && j0 + r < Ty) vy = *reinterpret_cast<const float4*>(yb + (int64_t)(j0 + r) * C + c);
        float* px = &xs[r][4 * (idx & 7)];
        float* py = &ys[r][4 * (idx & 7)];
        px[0] = vx.x; px[1] = vx.y; px[2] = vx.z; px[3] = vx.w;
        py[0] = vy.x; py[1] = vy.y; py[2] = vy.z; py[3] = vy.w;
      }
    } else {
      for (int idx = tid; idx < DTW_TILE * DTW_CK; idx += DTW_COST_THREADS) {
        const int r = idx >> 5, cc = idx & 31, c = c0 + cc;
        xs[r][cc] = (c < C && i0 + r < Tx) ? xb[(int64_t)(i0 + r) * C + c] : 0.f;
        ys[r][cc] = (c < C && j0 + r < Ty) ? yb[(int64_t)(j0 + r) * C + c] : 0.f;
      }
    }
    __syncthreads();
    float xr[DTW_CK];
#pragma unroll
    for (int c = 0; c < DTW_CK; ++c) xr[c] = xs[lane][c];
#pragma unroll
    for (int d = 0; d < DTW_TILE / 2; ++d) {
      const int jj = w + 4 * d - lane;
      if (jj >= 0 && jj < DTW_TILE) {
        float s = acc[d];
#pragma unroll
        for (int c = 0; c < DTW_CK; ++c) {
          const float df = xr[c] - ys[jj][c];
          s = fmaf(df, df, s);
        }
        acc[d] = s;
      }
    }
    __syncthreads();
  }
  float* Db = D + (int64_t)b * skew_elems(ldx, ldy);
  const int i = i0 + lane;
#pragma unroll
  for (int d = 0; d < DTW_TILE / 2; ++d) {
    const int jj = w + 4 * d - lane, j = j0 + jj;
    if (jj >= 0 && jj < DTW_TILE && i < Tx && j < Ty) Db[(int64_t)(i + j) * ldx + i] = acc[d];
  }
}

// One workgroup per pair.  Thread t owns rows t and t + blockDim.x of the cumulative cost A; the diagonals k, k - 1 and k - 2 rotate
// through three LDS rows indexed by i, with one barrier per diagonal, and the choice of predecessor (0: (i-1, j-1), 1: (i-1, j),
// 2: (i, j-1)) goes to the workspace at one byte per cell.  The backtrack stages windows of DTW_WIN diagonals x DTW_WIN rows of those
// bytes in LDS and thread 0 walks inside the window: a window is left only after at least DTW_WIN / 2 steps.  Then path_x is written
// by all threads, one wave forms the phonemes' start frames and every thread counts its phonemes' columns by bisection (path_x is
// non-decreasing).  Every loop that holds a barrier has a trip count that depends on (Tx, Ty) of the pair only, and no thread leaves
// before the last barrier: an empty pair walks zero diagonals and zero windows as a whole block.
__global__ __launch_bounds__(1024) void dtw_path_kernel(const float* __restrict__ D, unsigned char* __restrict__ bp,
                                                         const int* __restrict__ x_lens, const int* __restrict__ y_lens, int ldx, int ldy,
                                                         const int* __restrict__ x_seg, const int* __restrict__ n_seg, int ldL,
                                                         int* __restrict__ path_x, float* __restrict__ cost, int* __restrict__ status,
                                                         int* __restrict__ dur) {
  __shared__ float A[3][DTW_MAX_T];
  __shared__ int start[DTW_MAX_L + 1];
  __shared__ unsigned char win[DTW_WIN * DTW_WIN];
  __shared__ int at[2];
  __shared__ int seg_bad;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int Tx = clamp_len(x_lens, b, ldx), Ty = clamp_len(y_lens, b, ldy);
  const bool ok = Tx >= 1 && Ty >= 1;          // uniform over the workgroup
  const float* Db = D + (int64_t)b * skew_elems(ldx, ldy);
  unsigned char* bpb = bp + (int64_t)b * skew_elems(ldx, ldy);
  int* px = reinterpret_cast<int*>(&A[0][0]);  // path_x of the pair, once the diagonals are done

  const int nd = ok ? Tx + Ty - 1 : 0;
  const int ia = tid, ib = tid + nt;           // nt >= min(ldx, 1024) and ldx <= 2048: two rows per thread cover every i
  auto in_range = [&](int k, int i) { return i < Tx && k - i >= 0 && k - i < Ty; };
  float da = (nd > 0 && in_range(0, ia)) ? Db[ia] : 0.f, db = 0.f;
  float *cur = A[0], *p1 = A[1], *p2 = A[2];   // diagonals k, k - 1, k - 2
  for (int k = 0; k < nd; ++k) {
    float na = 0.f, nb = 0.f;                  // the next diagonal's local costs, in flight over this one's barrier
    if (k + 1 < nd) {
      if (in_range(k + 1, ia)) na = Db[(int64_t)(k + 1) * ldx + ia];
      if (in_range(k + 1, ib)) nb = Db[(int64_t)(k + 1) * ldx + ib];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = s ? ib : ia, j = k - i;
      const float d = s ? db : da;
      if (in_range(k, i)) {
        float best = 0.f;
        unsigned char c = 0;
        if (i > 0 && j > 0) {
          best = p2[i - 1];
          if (p1[i - 1] < best) { best = p1[i - 1]; c = 1; }
          if (p1[i] < best) { best = p1[i]; c = 2; }
        } else if (i > 0) {
          best = p1[i - 1];
          c = 1;
        } else if (j > 0) {
          best = p1[i];
          c = 2;
        }
        cur[i] = d + best;
        bpb[(int64_t)k * ldx + i] = c;
      }
    }
    __syncthreads();
    float* t = p2;
    p2 = p1;
    p1 = cur;
    cur = t;
    da = na;
    db = nb;
  }
  // p1 now holds the last diagonal
  if (tid == 0) {
    cost[b] = ok ? p1[Tx - 1] : INFINITY;
    at[0] = Tx - 1;
    at[1] = Ty - 1;
    seg_bad = 0;
  }
  __syncthreads();
  if (tid == 0 && ok) px[Ty - 1] = Tx - 1;
  const int rounds = ok ? (Tx + Ty - 2) / (DTW_WIN / 2) + 1 : 0;
  for (int r = 0; r < rounds; ++r) {
    const int it = at[0], jt = at[1], kt = it + jt;
    for (int idx = tid; idx < DTW_WIN * DTW_WIN; idx += nt) {
      const int k = kt - (idx >> 6), i = it - (idx & 63);
      win[idx] = (k >= 0 && i >= 0 && k - i >= 0 && k - i < Ty) ? bpb[(int64_t)k * ldx + i] : 0;
    }
    __syncthreads();
    if (tid == 0) {
      int i = it, j = jt;
      while ((i > 0 || j > 0) && kt - (i + j) < DTW_WIN && it - i < DTW_WIN) {
        const int c = win[((kt - i - j) << 6) + (it - i)];
        if (j == 0 || (i > 0 && c == 1)) {
          --i;
        } else if (i == 0 || c == 2) {
          --j;
          px[j] = i;
        } else {
          --i;
          --j;
          px[j] = i;
        }
      }
      at[0] = i;
      at[1] = j;
    }
    __syncthreads();
  }
  int* po = path_x + (int64_t)b * ldy;
  for (int j = tid; j < ldy; j += nt) po[j] = (ok && j < Ty) ? px[j] : -1;

  if (x_seg && dur) {
    const int* sg = x_seg + (int64_t)b * ldL;
    int n = n_seg ? n_seg[b] : ldL;
    n = n < 0 ? 0 : (n > ldL ? ldL : n);
    if (tid < 64) {                            // exclusive running sum of x_seg: 16 consecutive phonemes per lane, a shuffle scan across lanes
      int loc[16], run = 0, bad = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int l = tid * 16 + q;
        int v = l < n ? sg[l] : 0;
        if (v < 0 || v > DTW_MAX_T) { bad = 1; v = 0; }
        loc[q] = run;
        run += v;
      }
      int inc = run;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (tid >= o) inc += up;
      }
      const int base = inc - run;
#pragma unroll
      for (int q = 0; q < 16; ++q) start[tid * 16 + q] = base + loc[q];
      if (tid == 63) start[DTW_MAX_L] = inc;
      if (bad) seg_bad = 1;
    }
    __syncthreads();
    const bool good = ok && !seg_bad && start[DTW_MAX_L] == Tx;
    int* dout = dur + (int64_t)b * ldL;
    for (int l = tid; l < ldL; l += nt) {
      int v = 0;
      if (good && l < n) {
        int edge[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {          // the number of columns j < Ty with path_x[j] < start[l + e]
          const int lim = start[l + e];
          int lo = 0, hi = Ty;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (px[mid] < lim) lo = mid + 1; else hi = mid;
          }
          edge[e] = lo;
        }
        v = edge[1] - edge[0];
      }
      dout[l] = v;
    }
    if (tid == 0) status[b] = !ok ? 2 : (good ? 0 : 3);
  } else if (tid == 0) {
    status[b] = ok ? 0 : 2;
  }
}

bool dtw_dims_ok(int B, int ldx, int ldy) { return B >= 0 && B <= 65535 && ldx >= 1 && ldx <= DTW_MAX_T && ldy >= 1 && ldy <= DTW_MAX_T; }

}  // namespace

extern "C" int64_t ttsk_dtw_workspace_bytes(int B, int ldx, int ldy) {
  if (!dtw_dims_ok(B, ldx, ldy)) return -1;
  return (int64_t)B * (int64_t)(ldx + ldy) * ldx * 5;
}

extern "C" int ttsk_dtw_align(const float* x, const float* y, const int32_t* x_lens, const int32_t* y_lens, int B, int ldx, int ldy, int C,
                              const int32_t* x_seg, const int32_t* n_seg, int ldL, void* workspace, int64_t workspace_bytes,
                              int32_t* path_x, float* cost, int32_t* status, int32_t* dur, void* stream) {
  TTSK_REQUIRE(C >= 1 && C <= DTW_MAX_C, "ttsk_dtw_align: C %d is outside 1..%d", C, DTW_MAX_C);
  TTSK_REQUIRE(dtw_dims_ok(B, ldx, ldy), "ttsk_dtw_align: needs 0 <= B <= 65535 and 1 <= ldx, ldy <= %d (got B %d, ldx %d, ldy %d)",
               DTW_MAX_T, B, ldx, ldy);
  const bool with_dur = x_seg && dur;
  TTSK_REQUIRE(!with_dur || (ldL >= 1 && ldL <= DTW_MAX_L), "ttsk_dtw_align: ldL %d is outside 1..%d", ldL, DTW_MAX_L);
  if (B == 0) return TTSK_OK;
  TTSK_REQUIRE(x && y && path_x && cost && status, "ttsk_dtw_align: null x, y, path_x, cost or status");
  const int64_t need = ttsk_dtw_workspace_bytes(B, ldx, ldy);
  TTSK_REQUIRE(workspace && workspace_bytes >= need, "ttsk_dtw_align: the workspace holds %lld bytes, %lld are needed",
               (long long)workspace_bytes, (long long)need);
  TTSK_REQUIRE(((uintptr_t)workspace & 15) == 0, "ttsk_dtw_align: the workspace must be 16-byte aligned");
  float* D = (float*)workspace;
  unsigned char* bp = (unsigned char*)workspace + (int64_t)B * (ldx + ldy) * ldx * 4;
  const dim3 grid((ldy + DTW_TILE - 1) / DTW_TILE, (ldx + DTW_TILE - 1) / DTW_TILE, B);
  const bool vec = (C & 3) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(dtw_cost_kernel<true>, grid, dim3(DTW_COST_THREADS), 0, (hipStream_t)stream, x, y, (const int*)x_lens,
                       (const int*)y_lens, ldx, ldy, C, D);
  else
    hipLaunchKernelGGL(dtw_cost_kernel<false>, grid, dim3(DTW_COST_THREADS), 0, (hipStream_t)stream, x, y, (const int*)x_lens,
                       (const int*)y_lens, ldx, ldy, C, D);
  TTSK_CHECK_LAUNCH();
  int nt = (ldx + 63) / 64 * 64;
  nt = nt > 1024 ? 1024 : nt;
  hipLaunchKernelGGL(dtw_path_kernel, dim3(B), dim3(nt), 0, (hipStream_t)stream, (const float*)D, bp, (const int*)x_lens,
                     (const int*)y_lens, ldx, ldy, with_dur ? (const int*)x_seg : nullptr, (const int*)n_seg, ldL, (int*)path_x, cost,
                     (int*)status, with_dur ? (int*)dur : nullptr);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
