// griffinlim.hip — a phase-carrying STFT / inverse STFT pair in fp32 and the Griffin-Lim iteration around it.
// reference: fs_two/audio/stft.py:57-137 (STFT.transform / STFT.inverse), fs_two/audio/audio_processing.py:66-82 (griffin_lim),
// fs_two/audio/tools.py:18-25 (the mel-to-linear map of inv_mel_spec).
//
// One workgroup of 256 threads serves 256 / tpf frames, tpf = min(256, n_fft / 4) threads each.  A frame's real FFT of length
// n_fft runs in LDS as ONE complex FFT of M = n_fft / 2 points on z[k] = x[2k] + i x[2k+1] (radix 2, decimation in time, in place:
// the load stores to bit-reversed positions) and a split step X[k] = (Z[k] + conj Z[M-k]) / 2 - i/2 W^k (Z[k] - conj Z[M-k]),
// W = exp(-2 pi i / n_fft); the inverse runs the same steps backwards.  The twiddles W^k, k < n_fft / 2, are a table the caller
// builds in fp64 and rounds once; every stage reads it at stride n_fft / len.  Each thread owns the bin pairs (q, M - q), so the
// forward split, the projection onto the target magnitudes and the inverse split happen in registers between the two FFTs.
//
// The Griffin-Lim step keeps the signal as windowed frames F (B, T, n_fft): a step reads sample j of the previous signal as the
// overlap-add of the previous step's frames (ola_sample: a gather over the at most n_fft / hop frames that cover the sample, in
// ascending frame order, divided by the window's sum of squares) and writes its own frames to the other buffer, so an iteration is
// one launch; ttsk_istft_ola closes the loop.  Nothing is accumulated across workgroups and no row reads another row.
#include "common.h"

namespace {

constexpr int GL_THREADS = 256;
constexpr int GL_MAX_M = 1024;                 // n_fft <= 2048
constexpr float GL_TINY = 1.17549435e-38f;     // float32 tiny: the reference divides by the window sum only above it

struct GlArgs {
  const float* wav;          // POLAR, STEP: signal rows (B, ld_wav); null in STEP when frames_in is the source
  int64_t ld_wav;
  const int32_t* lens;       // POLAR: samples per row; STEP, FROM_POLAR: frames per row; null = every row is full
  const float* frames_in;    // STEP: the previous step's windowed frames (B, T, n_fft), or null
  float* frames_out;         // STEP, FROM_POLAR: (B, T, n_fft)
  const float* mag;          // STEP, FROM_POLAR: magnitudes, element (b, k, t) at b * sB + k * sk + t * st
  const float* phase;        // FROM_POLAR: phases, same strides
  int64_t sB, sk, st;
  float* mag_out;            // POLAR: (B, n_fft/2 + 1, T)
  float* phase_out;
  float2* zprev;             // STEP with momentum: (B, T, n_fft/2 + 1) complex, read and overwritten
  float mom;                 // a / (1 + a); 0: zprev is not touched
  const float* win;          // n_fft
  const float2* tw;          // n_fft / 2: (cos, -sin)(2 pi k / n_fft)
  int len, T, n_fft, hop, M, logM, tpf;
};

enum { POLAR = 0, STEP = 1, FROM_POLAR = 2 };

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// Sample p of the padded overlap-add of a row's windowed frames fr (T_row, n_fft), over the frames t with t * hop <= p < t * hop + n_fft
// in ascending order, divided by sum_t w^2[p - t * hop] where that exceeds float32 tiny.  0 <= p < n_fft + hop * (T_row - 1).
__device__ __forceinline__ float ola_sample(const float* __restrict__ fr, const float* __restrict__ win, int p, int T_row, int n_fft, int hop) {
  int t_hi = p / hop;
  if (t_hi > T_row - 1) t_hi = T_row - 1;
  const int t_lo = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;
  float acc = 0.f, ws = 0.f;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int n = p - t * hop;
    const float w = win[n];
    acc += fr[(int64_t)t * n_fft + n];
    ws = fmaf(w, w, ws);
  }
  return ws > GL_TINY ? acc / ws : acc;
}

// M-point complex FFT in place on s (input in bit-reversed order, output in natural order); every thread of the workgroup calls it.
__device__ __forceinline__ void fft_inplace(float2* s, const float2* tw, int M, int logM, int n_fft, int lane, int tpf, bool inverse) {
  for (int st = 1; st <= logM; ++st) {
    const int half = 1 << (st - 1);
    const int tstep = n_fft >> st;
    for (int j = lane; j < M / 2; j += tpf) {
      const int i = j & (half - 1);
      const int a = ((j - i) << 1) + i, b = a + half;
      float2 w = tw[i * tstep];
      if (inverse) w.y = -w.y;
      const float2 t = cmul(w, s[b]), u = s[a];
      s[a] = make_float2(u.x + t.x, u.y + t.y);
      s[b] = make_float2(u.x - t.x, u.y - t.y);
    }
    __syncthreads();
  }
}

// A / |A|, (1, 0) for A == 0; a value whose square leaves the normal range is rescaled first
__device__ __forceinline__ float2 unit(float2 a) {
  float r2 = a.x * a.x + a.y * a.y;
  if (!(r2 > 1e-30f && r2 < 1e30f)) {
    const float m = fmaxf(fabsf(a.x), fabsf(a.y));
    if (!(m > 0.f) || !(m < INFINITY)) return make_float2(1.f, 0.f);
    a.x /= m;
    a.y /= m;
    r2 = a.x * a.x + a.y * a.y;
  }
  const float r = sqrtf(r2);
  return make_float2(a.x / r, a.y / r);
}

template <int MODE>
__global__ __launch_bounds__(GL_THREADS) void gl_frames_kernel(const GlArgs a) {
  __shared__ float2 s_all[GL_MAX_M];
  __shared__ float2 s_tw[GL_MAX_M];
  const int N = a.n_fft, M = a.M, hop = a.hop, pad = N / 2, nbins = M + 1;
  const int f = threadIdx.x / a.tpf, lane = threadIdx.x - f * a.tpf;
  const int b = blockIdx.y, t = blockIdx.x * (GL_THREADS / a.tpf) + f;
  float2* s = s_all + f * M;
  for (int i = threadIdx.x; i < M; i += GL_THREADS) s_tw[i] = a.tw[i];

  // this row's frames and samples
  int T_row, rowlen;
  if (MODE == POLAR) {
    rowlen = a.lens ? min(max(a.lens[b], 0), a.len) : a.len;
    T_row = rowlen > pad ? 1 + rowlen / hop : 0;
  } else {
    T_row = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
    rowlen = T_row > 0 ? hop * (T_row - 1) : 0;
    if (MODE == STEP && rowlen <= pad) T_row = 0;      // cannot be reflect-padded: the callers refuse it, nothing is read or written
  }
  const bool active = t < T_row;
  const int64_t bt = (int64_t)b * a.T + t;

  if (MODE != FROM_POLAR) {
    const float* wrow = a.wav ? a.wav + (int64_t)b * a.ld_wav : nullptr;
    const float* frow = a.frames_in ? a.frames_in + (int64_t)b * a.T * N : nullptr;
    for (int k = lane; k < M; k += a.tpf) {
      float v[2] = {0.f, 0.f};
      if (active) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          int j = t * hop + 2 * k + e - pad;
          if (j < 0) j = -j;
          if (j >= rowlen) j = 2 * (rowlen - 1) - j;
          j = min(max(j, 0), rowlen - 1);
          const float x = (MODE == STEP && frow) ? ola_sample(frow, a.win, j + pad, T_row, N, hop) : wrow[j];
          v[e] = x * a.win[2 * k + e];
        }
      }
      s[__brev((unsigned)k) >> (32 - a.logM)] = make_float2(v[0], v[1]);
    }
    __syncthreads();
    fft_inplace(s, s_tw, M, a.logM, N, lane, a.tpf, false);
  } else {
    __syncthreads();       // the twiddles
  }

  // the bin pairs (q, M - q) of this lane: q = 0 holds bins 0 and M, q = M / 2 the one bin M / 2
  float2 z1[3], z2[3];
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int q = lane + it * a.tpf;
    z1[it] = z2[it] = make_float2(0.f, 0.f);
    if (q > M / 2) continue;
    const int k1 = q, k2 = M - q;
    const bool two = q != M / 2;
    float2 x1, x2 = make_float2(0.f, 0.f);
    if (MODE != FROM_POLAR) {
      if (q == 0) {
        const float2 z = s[0];
        x1 = make_float2(z.x + z.y, 0.f);
        x2 = make_float2(z.x - z.y, 0.f);
      } else if (!two) {
        const float2 z = s[q];
        x1 = make_float2(z.x, -z.y);
      } else {
        const float2 u = s[q], v = s[M - q];
        const float2 e = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));
        const float2 d = make_float2(0.5f * (u.x - v.x), 0.5f * (u.y + v.y));
        const float2 p = cmul(s_tw[q], d);
        x1 = make_float2(e.x + p.y, e.y - p.x);
        x2 = make_float2(e.x - p.y, -e.y - p.x);
      }
    }
    if (MODE == POLAR) {
      // the reference's (B, bins, T) layout: a frame's bins lie T apart, so these stores do not coalesce.  POLAR is the public
      // transform, not the iteration (STEP keeps its spectrum in registers and its frames frame-major).
      if (t < a.T) {
        const int64_t o = (int64_t)b * nbins * a.T + t;
        a.mag_out[o + (int64_t)k1 * a.T] = active ? sqrtf(x1.x * x1.x + x1.y * x1.y) : 0.f;
        a.phase_out[o + (int64_t)k1 * a.T] = active ? atan2f(x1.y, x1.x) : 0.f;
        if (two) {
          a.mag_out[o + (int64_t)k2 * a.T] = active ? sqrtf(x2.x * x2.x + x2.y * x2.y) : 0.f;
          a.phase_out[o + (int64_t)k2 * a.T] = active ? atan2f(x2.y, x2.x) : 0.f;
        }
      }
      continue;
    }
    float2 y1 = make_float2(0.f, 0.f), y2 = y1;
    if (active) {
      const int64_t mo = (int64_t)b * a.sB + (int64_t)t * a.st;
      const float m1 = a.mag[mo + k1 * a.sk], m2 = two ? a.mag[mo + k2 * a.sk] : 0.f;
      if (MODE == STEP) {
        if (a.mom > 0.f) {
          float2* zp = a.zprev + bt * nbins;
          const float2 p1 = zp[k1];
          zp[k1] = x1;
          x1 = make_float2(x1.x - a.mom * p1.x, x1.y - a.mom * p1.y);
          if (two) {
            const float2 p2 = zp[k2];
            zp[k2] = x2;
            x2 = make_float2(x2.x - a.mom * p2.x, x2.y - a.mom * p2.y);
          }
        }
        const float2 u1 = unit(x1), u2 = unit(x2);
        y1 = make_float2(m1 * u1.x, m1 * u1.y);
        y2 = make_float2(m2 * u2.x, m2 * u2.y);
      } else {
        float sn, cs;
        sincosf(a.phase[mo + k1 * a.sk], &sn, &cs);
        y1 = make_float2(m1 * cs, m1 * sn);
        if (two) {
          sincosf(a.phase[mo + k2 * a.sk], &sn, &cs);
          y2 = make_float2(m2 * cs, m2 * sn);
        }
      }
    }
    // inverse split: Zc[k] = E[k] + i O[k], E = Y[k] + conj Y[M-k], O = conj(W^k) (Y[k] - conj Y[M-k])
    if (q == 0) {
      z1[it] = make_float2(y1.x + y2.x, y1.x - y2.x);
    } else if (!two) {
      z1[it] = make_float2(2.f * y1.x, -2.f * y1.y);
    } else {
      const float2 e = make_float2(y1.x + y2.x, y1.y - y2.y);
      const float2 d = make_float2(y1.x - y2.x, y1.y + y2.y);
      const float2 w = s_tw[q];
      const float2 p = cmul(make_float2(w.x, -w.y), d);
      z1[it] = make_float2(e.x - p.y, e.y + p.x);
      z2[it] = make_float2(e.x + p.y, -e.y + p.x);
    }
  }
  if (MODE == POLAR) return;

  __syncthreads();         // every read of the forward spectrum is done
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int q = lane + it * a.tpf;
    if (q > M / 2) continue;
    s[__brev((unsigned)q) >> (32 - a.logM)] = z1[it];
    if (q != 0 && q != M / 2) s[__brev((unsigned)(M - q)) >> (32 - a.logM)] = z2[it];
  }
  __syncthreads();
  fft_inplace(s, s_tw, M, a.logM, N, lane, a.tpf, true);
  if (active) {
    const float inv = 1.f / (float)N;
    float2* out = reinterpret_cast<float2*>(a.frames_out + bt * N);
    for (int k = lane; k < M; k += a.tpf) {
      const float2 z = s[k];
      out[k] = make_float2(z.x * inv * a.win[2 * k], z.y * inv * a.win[2 * k + 1]);
    }
  }
}

// frames (B, T, n_fft) -> wav (B, hop * (T - 1)): the overlap-add without its n_fft / 2 ends; zeros past a row's hop * (T_row - 1)
__global__ __launch_bounds__(GL_THREADS) void gl_ola_kernel(const float* __restrict__ frames, const int32_t* __restrict__ lens,
                                                            const float* __restrict__ win, float* __restrict__ wav, int T, int n_fft, int hop) {
  const int b = blockIdx.y;
  const int T_row = lens ? min(max(lens[b], 0), T) : T;
  const int rowlen = T_row > 0 ? hop * (T_row - 1) : 0, ld = hop * (T - 1);
  const float* fr = frames + (int64_t)b * T * n_fft;
  for (int j = blockIdx.x * GL_THREADS + threadIdx.x; j < ld; j += gridDim.x * GL_THREADS)
    wav[(int64_t)b * ld + j] = j < rowlen ? ola_sample(fr, win, j + n_fft / 2, T_row, n_fft, hop) : 0.f;
}

// log-mel (B, n_mels, T) -> spec (B, nbins, T) = scale * sum_m exp(mel[m]) fb[m][k], filters in ascending order; one bin per workgroup row.
// Runs once per call, outside the iteration, so it is kept plain: every thread walks all n_mels (start, off) pairs (uniform across the
// workgroup, so scalar loads) and takes expf per covering filter per (bin, t), not once per (mel, t); a per-bin filter range in the pack
// would remove the walk.
__global__ __launch_bounds__(GL_THREADS) void mel_to_spec_kernel(const float* __restrict__ mel, const float* __restrict__ vals,
                                                                 const int32_t* __restrict__ start, const int32_t* __restrict__ off, int n_mels,
                                                                 int nbins, int T, float scale, float* __restrict__ spec) {
  const int t = blockIdx.x * GL_THREADS + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  float acc = 0.f;
  for (int m = 0; m < n_mels; ++m) {
    const int s0 = start[m], o = off[m], n = off[m + 1] - o;
    if (k >= s0 && k < s0 + n) acc = fmaf(expf(mel[((int64_t)b * n_mels + m) * T + t]), vals[o + k - s0], acc);
  }
  spec[((int64_t)b * nbins + k) * T + t] = acc * scale;
}

int log2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// the transform's geometry, or an error text
const char* gl_geometry(GlArgs& a, int B, int T, int n_fft, int hop) {
  if (B < 1 || B > 65535) return "1 <= B <= 65535";
  if (n_fft < 64 || n_fft > 2048 || (n_fft & (n_fft - 1))) return "n_fft must be a power of two in 64..2048";
  if (hop < 1 || n_fft % hop) return "hop must divide n_fft";
  if (T < 1 || (int64_t)T * hop + n_fft >= (1ll << 31)) return "1 <= T, T * hop + n_fft < 2^31";
  a.T = T;
  a.n_fft = n_fft;
  a.hop = hop;
  a.M = n_fft / 2;
  a.logM = log2_exact(a.M);
  a.tpf = a.M / 2 < GL_THREADS ? a.M / 2 : GL_THREADS;
  return nullptr;
}

dim3 gl_grid(const GlArgs& a, int B) {
  const int fpb = GL_THREADS / a.tpf;
  return dim3((a.T + fpb - 1) / fpb, B);
}

}  // namespace

extern "C" int ttsk_stft_polar(const float* wav, const int32_t* lens, int B, int len, int n_fft, int hop, const float* window,
                               const float* twiddle, float* mag, float* phase, int T, void* stream) {
  TTSK_REQUIRE(wav && window && twiddle && mag && phase, "ttsk_stft_polar: null pointer");
  GlArgs a = {};
  const char* bad = gl_geometry(a, B, T, n_fft, hop);
  TTSK_REQUIRE(!bad, "ttsk_stft_polar: %s", bad);
  TTSK_REQUIRE(len > n_fft / 2 && T == 1 + len / hop,
               "ttsk_stft_polar: reflect padding by n_fft / 2 needs a longer signal, and T = 1 + len / hop (len %d, T %d)", len, T);
  a.wav = wav;
  a.ld_wav = len;
  a.len = len;
  a.lens = lens;
  a.win = window;
  a.tw = (const float2*)twiddle;
  a.mag_out = mag;
  a.phase_out = phase;
  hipLaunchKernelGGL(gl_frames_kernel<POLAR>, gl_grid(a, B), dim3(GL_THREADS), 0, (hipStream_t)stream, a);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_istft_frames(const float* mag, const float* phase, int64_t sB, int64_t sk, int64_t st, const int32_t* frames, int B,
                                 int T, int n_fft, int hop, const float* window, const float* twiddle, float* frames_out, void* stream) {
  TTSK_REQUIRE(mag && phase && window && twiddle && frames_out, "ttsk_istft_frames: null pointer");
  GlArgs a = {};
  const char* bad = gl_geometry(a, B, T, n_fft, hop);
  TTSK_REQUIRE(!bad, "ttsk_istft_frames: %s", bad);
  TTSK_REQUIRE(sB >= 0 && sk >= 1 && st >= 1, "ttsk_istft_frames: strides must be positive");
  a.mag = mag;
  a.phase = phase;
  a.sB = sB;
  a.sk = sk;
  a.st = st;
  a.lens = frames;
  a.win = window;
  a.tw = (const float2*)twiddle;
  a.frames_out = frames_out;
  hipLaunchKernelGGL(gl_frames_kernel<FROM_POLAR>, gl_grid(a, B), dim3(GL_THREADS), 0, (hipStream_t)stream, a);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_istft_ola(const float* frames_in, const int32_t* frames, int B, int T, int n_fft, int hop, const float* window,
                              float* wav, void* stream) {
  TTSK_REQUIRE(frames_in && window && wav, "ttsk_istft_ola: null pointer");
  GlArgs a = {};
  const char* bad = gl_geometry(a, B, T, n_fft, hop);
  TTSK_REQUIRE(!bad, "ttsk_istft_ola: %s", bad);
  TTSK_REQUIRE(T >= 2, "ttsk_istft_ola: T frames give hop * (T - 1) samples, T >= 2");
  const int64_t ld = (int64_t)hop * (T - 1);
  int blocks = (int)((ld + GL_THREADS - 1) / GL_THREADS);
  if (blocks > 65535) blocks = 65535;
  hipLaunchKernelGGL(gl_ola_kernel, dim3(blocks, B), dim3(GL_THREADS), 0, (hipStream_t)stream, frames_in, frames, window, wav, T, n_fft, hop);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_istft(const float* mag, const float* phase, int64_t sB, int64_t sk, int64_t st, const int32_t* frames, int B, int T,
                          int n_fft, int hop, const float* window, const float* twiddle, float* workspace, float* wav, void* stream) {
  TTSK_REQUIRE(workspace && wav, "ttsk_istft: null pointer");
  TTSK_REQUIRE(T >= 2, "ttsk_istft: T frames give hop * (T - 1) samples, T >= 2");
  const int rc = ttsk_istft_frames(mag, phase, sB, sk, st, frames, B, T, n_fft, hop, window, twiddle, workspace, stream);
  if (rc != TTSK_OK) return rc;
  return ttsk_istft_ola(workspace, frames, B, T, n_fft, hop, window, wav, stream);
}

extern "C" int ttsk_griffinlim_step(const float* wav, int64_t ld_wav, const float* frames_in, const float* mag, int64_t sB, int64_t sk,
                                    int64_t st, const int32_t* frames, float* zprev, float momentum, int B, int T, int n_fft, int hop,
                                    const float* window, const float* twiddle, float* frames_out, void* stream) {
  TTSK_REQUIRE(mag && window && twiddle && frames_out, "ttsk_griffinlim_step: null pointer");
  TTSK_REQUIRE((wav != nullptr) != (frames_in != nullptr), "ttsk_griffinlim_step: exactly one of wav and frames_in is the source");
  TTSK_REQUIRE(frames_in != frames_out, "ttsk_griffinlim_step: frames_in and frames_out must be two buffers");
  GlArgs a = {};
  const char* bad = gl_geometry(a, B, T, n_fft, hop);
  TTSK_REQUIRE(!bad, "ttsk_griffinlim_step: %s", bad);
  TTSK_REQUIRE(sB >= 0 && sk >= 1 && st >= 1, "ttsk_griffinlim_step: strides must be positive");
  TTSK_REQUIRE(momentum >= 0.f && momentum < 1.f && (momentum == 0.f || zprev), "ttsk_griffinlim_step: momentum in [0, 1), with zprev when positive");
  TTSK_REQUIRE((int64_t)hop * (T - 1) > n_fft / 2, "ttsk_griffinlim_step: hop * (T - 1) must exceed the reflect padding n_fft / 2");
  TTSK_REQUIRE(!wav || ld_wav >= (int64_t)hop * (T - 1), "ttsk_griffinlim_step: wav rows hold hop * (T - 1) samples");
  a.wav = wav;
  a.ld_wav = ld_wav;
  a.frames_in = frames_in;
  a.mag = mag;
  a.sB = sB;
  a.sk = sk;
  a.st = st;
  a.lens = frames;
  a.zprev = (float2*)zprev;
  a.mom = momentum / (1.f + momentum);
  a.win = window;
  a.tw = (const float2*)twiddle;
  a.frames_out = frames_out;
  hipLaunchKernelGGL(gl_frames_kernel<STEP>, gl_grid(a, B), dim3(GL_THREADS), 0, (hipStream_t)stream, a);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}

extern "C" int ttsk_mel_to_spec(const float* mel, const float* basis_vals, const int32_t* basis_start, const int32_t* basis_off, int B,
                                int n_mels, int nbins, int T, float scale, float* spec, void* stream) {
  TTSK_REQUIRE(mel && basis_vals && basis_start && basis_off && spec, "ttsk_mel_to_spec: null pointer");
  TTSK_REQUIRE(B > 0 && B <= 65535 && n_mels > 0 && n_mels <= 1024 && nbins > 0 && nbins <= 65535 && T > 0,
               "ttsk_mel_to_spec: bad sizes (B, nbins <= 65535, n_mels <= 1024)");
  hipLaunchKernelGGL(mel_to_spec_kernel, dim3((T + GL_THREADS - 1) / GL_THREADS, nbins, B), dim3(GL_THREADS), 0, (hipStream_t)stream, mel,
                     basis_vals, basis_start, basis_off, n_mels, nbins, T, scale, spec);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
