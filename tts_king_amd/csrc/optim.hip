// optim.hip — global-norm gradient clipping + Adam + LR schedule + bf16 weight shadow, over ONE flat buffer.
// reference: train.py:47-54 (clip_grad_norm_(1.0) -> step_and_update_lr -> zero_grad),
//            fs_two/model/optimizer.py:35-53 (lr = d^-0.5 * min(s^-0.5, warmup^-1.5 * s) * anneal^{#(s > a_k)}),
//            torch.optim.Adam (betas (0.95, 0.999), eps 1e-5, bias correction, no weight decay).
// The step counters, learning rate and bias corrections live in a small DEVICE state block so that a captured
// hipGraph of the train step replays with fresh values (kernel arguments are frozen at capture).
#include "common.h"

namespace {

struct OptState {          // mirrors tts_king_amd/optimizer.py: 8 x 8 bytes
  long long sched_step;    // ScheduledOptim.current_step (counts optimizer updates)
  long long adam_t;        // Adam's per-parameter step
  unsigned long long rng_seed, rng_step;   // dropout counter state (rng = &rng_seed)
  float lr, bc1, bc2, clip_coef;
  float gnorm, pad0;
  long long pad1;
};

__global__ void rng_advance_kernel(OptState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) st->rng_step += 1;
}

// ---- launch 1 of the step.  `ranges` is a device table [n_ranges][3] = {start, end, f32x4 groups in the ranges before this one} (the
// layout of AdamTables::gaps), starts / ends multiples of four floats: the elements the step covers as one compact index space — the
// whole buffer as one range, or the trainable stretches of it (speaker adaptation: FastSpeech2.set_trainable).  Sums g^2 over them
// only: every workgroup writes its partial to its own slot and a thread walks its groups in ascending order, so equal inputs give equal
// bits on every run.  Block 0 also advances the scheduler / Adam / dropout counters (it reads nothing the counters feed; the Adam
// launch after it reads the advanced state).
struct SchedArgs { float d_model, warmup, a0, a1, a2, a3, anneal_rate, b1, b2; int n_anneal, advance_rng; };

__global__ __launch_bounds__(256) void sumsq_advance_kernel(const float* __restrict__ g, int64_t n, const long long* __restrict__ ranges, int n_ranges,
                                                            long long total4, float* __restrict__ partials, OptState* st, const SchedArgs sc) {
  __shared__ float red[4];
  float s = 0.f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = blockIdx.x * 256ll + threadIdx.x;
  // Ranges that hold all n floats are the whole buffer in order: compact index = element index, and the table is not consulted (a
  // read every thread's first load would wait for: measured, about 1 us of this kernel's 28 on the shipped step).
  const bool whole = total4 * 4 == n;
  int lo = 0;
  while (i < total4) {
    long long r_start = 0, r_first = 0, r_next = total4;
    if (!whole) {
      // the range that holds compact index i (invariant: ranges[lo].first <= i < ranges[hi].first); the index only grows, so lo never
      // goes back, and the table is searched once per range a thread enters
      int hi = n_ranges;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ranges[mid * 3 + 2] <= i) lo = mid; else hi = mid;
      }
      r_start = ranges[lo * 3], r_first = ranges[lo * 3 + 2], r_next = hi < n_ranges ? ranges[hi * 3 + 2] : total4;
    }
    do {                                       // (at least one group: a thread advances whatever the table holds)
      const int64_t e = r_start + (i - r_first) * 4;
      // a table that does not fit the buffer reads nothing outside it — without a branch in front of the load: such a group reads
      // g[0..3] and adds +0, which leaves s (never -0) as it is
      const bool in = e >= 0 && e + 4 <= n;
      const f32x4 v = *(const f32x4*)(g + (in ? e : 0));
      const float q = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
      s += in ? q : 0.f;
      i += stride;
    } while (i < r_next);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long sstep = ++st->sched_step;
    const long long t = ++st->adam_t;
    double lr = fmin(pow((double)sstep, -0.5), pow((double)sc.warmup, -1.5) * (double)sstep);
    const float an[4] = {sc.a0, sc.a1, sc.a2, sc.a3};
    for (int i = 0; i < sc.n_anneal; ++i)
      if ((double)sstep > (double)an[i]) lr *= (double)sc.anneal_rate;
    st->lr = (float)(pow((double)sc.d_model, -0.5) * lr);
    st->bc1 = (float)(1.0 - pow((double)sc.b1, (double)t));
    st->bc2 = (float)(1.0 - pow((double)sc.b2, (double)t));
    if (sc.advance_rng) st->rng_step += 1;
  }
}

// ---- launch 2 of the step: clip + Adam + bf16 shadow, and the window kernels' weight packs.  Every workgroup first folds the 1024
// partials in the same fixed order (double) into the global norm and the clip coefficient; workgroup 0 records gnorm / clip_coef in
// the state block.  The packs are a pure re-layout of the bf16 shadow Adam has just written (fragment-major copies of every FFT-block /
// PostNet weight as it is and transposed with flipped taps, 140 MB; as a launch of its own, win_pack_kernel, 55 us on the step's serial
// tail).  Here the workgroup that updates a tile of a packed weight — 32 storage rows x 256 storage columns of one tap, the tile
// ffn_conv.hip:pack_one transposes through LDS — keeps the tile's bf16 values in LDS and stores the 16 fragments of the plain pack and
// the 16 of the transposed pack itself (1 KiB runs each).  Everything outside the packed weights (biases, LayerNorms, embeddings,
// predictors, the 80-channel ends: 5 % of the parameters) goes through the flat loop over the gap ranges between them — with no
// items at all, over the step's ranges themselves.  One arithmetic per element (adam4) on both walks: parameters, moments and shadow
// do not depend on which one an element takes, and the packs are bit-identical to win_pack_kernel's from that shadow.  The tables
// cover the step's ranges and nothing else: bytes moved are proportional to them, elements outside are neither read nor written.
struct AdamTables {
  const ttsk_adam_item* items;   // device, sorted by tile0
  int n_items, n_tiles;
  const long long* gaps;         // device: n_gaps x {start, end, first compact f32x4 index}
  int n_gaps;
  long long gap4;                // f32x4 groups in all gaps
};

__device__ __forceinline__ void adam4(f32x4& pp, const f32x4 gg, f32x4& mm, f32x4& vv, float coef, float b1, float b2, float step, float isb2,
                                      float eps) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float ge = gg[e] * coef;
    mm[e] = b1 * mm[e] + (1.f - b1) * ge;
    vv[e] = b2 * vv[e] + (1.f - b2) * ge * ge;
    pp[e] -= step * mm[e] / (sqrtf(vv[e]) * isb2 + eps);
  }
}

__global__ __launch_bounds__(256) void adam_pack_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, bf16_t* __restrict__ shadow, OptState* st,
                                                        const float* __restrict__ partials, int nblk, float max_norm, float b1, float b2,
                                                        float eps, int zero_grad, const AdamTables tb) {
  __shared__ double red[256];
  __shared__ __attribute__((aligned(16))) unsigned short tile[32][256 + 8];
  {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  }
  const float norm = (float)sqrt(red[0]);
  const float cc = max_norm / (norm + 1e-6f);
  const float coef = cc < 1.f ? cc : 1.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) { st->gnorm = norm; st->clip_coef = coef; }
  const float lr = st->lr, bc1 = st->bc1;
  const float isb2 = 1.f / sqrtf(st->bc2);
  const float step = lr / bc1;
  const int tid = threadIdx.x;
  // ---- the packed weights, tile by tile
  for (int t = blockIdx.x; t < tb.n_tiles; t += gridDim.x) {
    int lo = 0, hi = tb.n_items;               // invariant: items[lo].tile0 <= t < items[hi].tile0
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tb.items[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    const ttsk_adam_item it = tb.items[lo];
    const int Cs = it.Cs, K = it.K, Ds = it.Ds;
    const int ncb = Ds / 256, nks = Cs / 32;
    const int lt = t - it.tile0;
    const int cb = lt % ncb, ks = (lt / ncb) % nks, ts = lt / (ncb * nks);        // ts = storage tap
    __syncthreads();                            // the previous tile's LDS readers are done
#pragma unroll
    for (int u = 0; u < 8; ++u) {               // 32 rows x 64 groups of four floats; a wave takes a whole 1 KiB row
      const int idx = u * 256 + tid, r = idx >> 6, c4 = idx & 63;
      const int64_t e = it.off + ((int64_t)(ks * 32 + r) * K + ts) * Ds + cb * 256 + c4 * 4;
      // p, m, v and g stream through once per step (1.1 GB): nontemporal, so that they do not evict the shadow and the packs the next
      // forward reads (measured -25 us on the kernel)
      f32x4 pp = __builtin_nontemporal_load((f32x4*)(p + e)), mm = __builtin_nontemporal_load((f32x4*)(m + e)), vv = __builtin_nontemporal_load((f32x4*)(v + e));
      const f32x4 gg = __builtin_nontemporal_load((const f32x4*)(g + e));
      adam4(pp, gg, mm, vv, coef, b1, b2, step, isb2, eps);
      __builtin_nontemporal_store(pp, (f32x4*)(p + e)); __builtin_nontemporal_store(mm, (f32x4*)(m + e)); __builtin_nontemporal_store(vv, (f32x4*)(v + e));
      if (zero_grad) *(f32x4*)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
      const uint2 w = make_uint2(pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3]));
      *(uint2*)(shadow + e) = w;
      *(uint2*)&tile[r][c4 * 4] = w;
    }
    __syncthreads();
    if (it.pack) {
      // plain pack [K][Ds/32][Cs/16][64][8]: the tile's rows are couts ks*32.., its columns cins cb*256..: 8 k-steps x 2 cout tiles
      bf16_t* dst = (bf16_t*)it.pack;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pi = u * 256 + tid, f = pi >> 6, l = pi & 63;
        const int ksl = f >> 1, cl = f & 1;
        const uint4 val = *(const uint4*)&tile[cl * 16 + (l & 15)][ksl * 32 + (l >> 4) * 8];
        const int64_t piece = ((int64_t)(ts * (Ds / 32) + cb * 8 + ksl) * (Cs / 16) + 2 * ks + cl) * 64 + l;
        *(uint4*)(dst + piece * 8) = val;
      }
    }
    if (it.pack_t) {
      // transposed pack, taps flipped (ffn_conv.hip:pack_one): Cout' = Ds, Cin' = Cs; 16 contiguous fragments
      const int tap = K - 1 - ts;
      bf16_t* out = (bf16_t*)it.pack_t + ((int64_t)(tap * nks + ks) * (Ds / 16) + cb * 16) * 512;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pi = u * 256 + tid, c = pi >> 6, l = pi & 63;
        const int col = c * 16 + (l & 15), r0 = (l >> 4) * 8;
        unsigned short q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = tile[r0 + j][col];
        *(uint4*)(out + (int64_t)pi * 8) = make_uint4(q[0] | ((unsigned)q[1] << 16), q[2] | ((unsigned)q[3] << 16), q[4] | ((unsigned)q[5] << 16),
                                                      q[6] | ((unsigned)q[7] << 16));
      }
    }
  }
  // ---- everything else: the gap ranges (multiples of four floats, 16-byte aligned), as one compact index space
  for (int64_t i = blockIdx.x * 256ll + tid; i < tb.gap4; i += (int64_t)gridDim.x * 256) {
    int lo = 0, hi = tb.n_gaps;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tb.gaps[mid * 3 + 2] <= i) lo = mid; else hi = mid;
    }
    const int64_t e = tb.gaps[lo * 3] + (i - tb.gaps[lo * 3 + 2]) * 4;
    f32x4 pp = __builtin_nontemporal_load((f32x4*)(p + e)), mm = __builtin_nontemporal_load((f32x4*)(m + e)), vv = __builtin_nontemporal_load((f32x4*)(v + e));
    const f32x4 gg = __builtin_nontemporal_load((const f32x4*)(g + e));
    adam4(pp, gg, mm, vv, coef, b1, b2, step, isb2, eps);
    __builtin_nontemporal_store(pp, (f32x4*)(p + e)); __builtin_nontemporal_store(mm, (f32x4*)(m + e)); __builtin_nontemporal_store(vv, (f32x4*)(v + e));
    if (zero_grad) *(f32x4*)(g + e) = f32x4{0.f, 0.f, 0.f, 0.f};
    *(uint2*)(shadow + e) = make_uint2(pack_bf2(pp[0], pp[1]), pack_bf2(pp[2], pp[3]));
  }
}

}  // namespace

extern "C" int ttsk_optim_state_bytes(void) { return (int)sizeof(OptState); }

extern "C" int ttsk_rng_advance(void* state, void* stream) {
  TTSK_REQUIRE(state, "rng_advance: null state");
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (OptState*)state);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_optim_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t n, void* state,
                               float* partials /* >= 1024 floats */, float max_norm, float beta1, float beta2, float eps, int zero_grad,
                               float d_model, float warmup, const float* anneal_steps_host, int n_anneal, float anneal_rate, int advance_rng,
                               const int64_t* dev_ranges, int n_ranges, int64_t range_floats, const ttsk_adam_item* dev_items, int n_items,
                               int n_tiles, const int64_t* dev_gaps, int n_gaps, int64_t gap_floats, void* stream) {
  TTSK_REQUIRE(params && grads && exp_avg && exp_avg_sq && shadow_bf16 && state && partials && n > 0, "optim_step: null pointer");
  TTSK_REQUIRE((n & 3) == 0, "optim_step: n must be a multiple of 4 (pad the flat buffer)");
  TTSK_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)shadow_bf16) & 15) == 0,
               "optim_step: alignment");
  TTSK_REQUIRE(n_anneal >= 0 && n_anneal <= 4, "optim_step: at most 4 anneal steps");
  TTSK_REQUIRE(dev_ranges && n_ranges > 0, "optim_step: no trainable range (n_ranges = %d)", n_ranges);
  TTSK_REQUIRE(range_floats > 0 && (range_floats & 3) == 0 && range_floats <= n,
               "optim_step: the ranges hold %lld floats (a positive multiple of 4, at most n = %lld)", (long long)range_floats, (long long)n);
  if (n_items == 0) {
    // no packed weight among the trainable ones: the Adam launch walks the ranges themselves
    TTSK_REQUIRE(!dev_items && n_tiles == 0 && !dev_gaps && n_gaps == 0 && gap_floats == 0, "optim_step: tile / gap tables without items");
    dev_gaps = dev_ranges;
    n_gaps = n_ranges;
    gap_floats = range_floats;
  } else {
    TTSK_REQUIRE(dev_items && n_items > 0 && n_tiles > 0 && n_gaps >= 0 && (n_gaps == 0 || dev_gaps) && gap_floats >= 0 && (gap_floats & 3) == 0,
                 "optim_step: bad tables");
    TTSK_REQUIRE((int64_t)n_tiles * 8192 + gap_floats == range_floats, "optim_step: tiles (%d x 8192) + gaps (%lld) do not cover the ranges (%lld)",
                 n_tiles, (long long)gap_floats, (long long)range_floats);
  }
  float a[4] = {0, 0, 0, 0};
  for (int i = 0; i < n_anneal; ++i) a[i] = anneal_steps_host[i];
  const SchedArgs sc{d_model, warmup, a[0], a[1], a[2], a[3], anneal_rate, beta1, beta2, n_anneal, advance_rng};
  const AdamTables tb{dev_items, n_items, n_tiles, (const long long*)dev_gaps, n_gaps, (long long)(gap_floats / 4)};
  const int64_t total4 = range_floats / 4;
  // 1024 workgroups whatever the ranges hold (a workgroup without elements writes a zero; the Adam launch folds all 1024 slots)
  const int nblk = 1024;
  int64_t wgs = (gap_floats / 4 + 255) / 256;
  if (wgs < n_tiles) wgs = n_tiles;
  const int grid = (int)(wgs < 1 ? 1 : (wgs > 2048 ? 2048 : wgs));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sumsq_advance_kernel, dim3(nblk), dim3(256), 0, s, grads, n, (const long long*)dev_ranges, n_ranges,
                     (long long)total4, partials, (OptState*)state, sc);
  hipLaunchKernelGGL(adam_pack_kernel, dim3(grid), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, (bf16_t*)shadow_bf16, (OptState*)state,
                     partials, nblk, max_norm, beta1, beta2, eps, zero_grad, tb);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
