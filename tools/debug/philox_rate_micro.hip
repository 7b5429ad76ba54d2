// philox_rate_micro.hip — diagnostic only (not part of the library): what does one Philox4x32-10 call (csrc/common.h, the dropout
// masks' generator) cost a wave on gfx950, with the two products of a round written
//   form 0: as the __umulhi + * pair      (v_mul_hi_u32 + v_mul_lo_u32: 36 multiplies per call)
//   form 1: as one 64-bit product         (v_mad_u64_u32: 18 per call)
// One workgroup per CU, 1 or 2 waves per SIMD; every lane runs NIT iterations of four independent calls (a lane of the row kernels
// draws four quads), each call's output feeding its next counter.  Prints cycles (s_memtime) per call and wave, and checks that the
// two forms give equal words over 6 x 2^20 counters (counter and key words of 0 and 0xFFFFFFFF, a non-zero high step word) and
// against the published known answers.
// build + run: hipcc -O3 --offload-arch=gfx950 -o philox_rate_micro philox_rate_micro.hip && ./philox_rate_micro
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include <algorithm>

template <int FORM>
__device__ __forceinline__ uint4 philox(uint2 key, uint4 ctr) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    unsigned hi0, lo0, hi1, lo1;
    if (FORM == 0) {
      hi0 = __umulhi(0xD2511F53u, ctr.x); lo0 = 0xD2511F53u * ctr.x;
      hi1 = __umulhi(0xCD9E8D57u, ctr.z); lo1 = 0xCD9E8D57u * ctr.z;
    } else {
      const uint64_t p0 = (uint64_t)0xD2511F53u * ctr.x, p1 = (uint64_t)0xCD9E8D57u * ctr.z;
      hi0 = (unsigned)(p0 >> 32); lo0 = (unsigned)p0;
      hi1 = (unsigned)(p1 >> 32); lo1 = (unsigned)p1;
    }
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

template <int FORM, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void rate_kernel(unsigned* __restrict__ out, unsigned long long* __restrict__ cyc, int nit, unsigned k0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint2 key = make_uint2(k0, k0 ^ 0x5bd1e995u);
  uint4 c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = make_uint4(blockIdx.x * WAVES * 64 + tid, j, 7u, 0u);
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
  for (int it = 0; it < nit; ++it) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = philox<FORM>(key, c[j]);
  }
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) s ^= c[j].x ^ c[j].y ^ c[j].z ^ c[j].w;
  out[blockIdx.x * WAVES * 64 + tid] = s;
  if (lane == 0) cyc[blockIdx.x * WAVES + wave] = t1 - t0;
}

// counter word 0 walks up from 0 (even i) or down from 0xFFFFFFFF (odd i); the other words come from the case
struct EqCase { unsigned kx, ky, site, step_lo, step_hi; };
__global__ __launch_bounds__(256) void equal_kernel(EqCase q, unsigned n, unsigned long long* __restrict__ bad, unsigned* __restrict__ sum) {
  unsigned acc = 0;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned e4 = (i & 1) ? 0xFFFFFFFFu - (i >> 1) : (i >> 1);
    const uint4 a = philox<0>(make_uint2(q.kx, q.ky), make_uint4(e4, q.site, q.step_lo, q.step_hi));
    const uint4 b = philox<1>(make_uint2(q.kx, q.ky), make_uint4(e4, q.site, q.step_lo, q.step_hi));
    if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) atomicAdd(bad, 1ull);
    acc ^= a.x ^ a.y ^ a.z ^ a.w;
  }
  atomicXor(sum, acc);
}
__global__ void kat_kernel(uint4* out) {
  out[0] = philox<0>(make_uint2(0u, 0u), make_uint4(0u, 0u, 0u, 0u));
  out[1] = philox<1>(make_uint2(0u, 0u), make_uint4(0u, 0u, 0u, 0u));
  out[2] = philox<0>(make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu), make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu));
  out[3] = philox<1>(make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu), make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu));
}

#define CK(x)                                                                                     \
  do {                                                                                            \
    hipError_t e__ = (x);                                                                         \
    if (e__ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e__)); return 1; }          \
  } while (0)

template <int FORM, int WAVES>
int run(const char* name, unsigned* out, unsigned long long* cyc, int nit, double* per_call) {
  const int grid = 256;
  for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL((rate_kernel<FORM, WAVES>), dim3(grid), dim3(WAVES * 64), 0, 0, out, cyc, nit, 0x12345u + rep);
  CK(hipDeviceSynchronize());
  std::vector<unsigned long long> h(grid * WAVES);
  CK(hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost));
  std::sort(h.begin(), h.end());
  const double med = (double)h[h.size() / 2], calls = (double)nit * 4;
  *per_call = med / calls;
  printf("%-44s  %7.1f cycles per call and wave, %7.1f per call and SIMD   (min %.1f, max %.1f per call and wave)\n", name, med / calls,
         med / calls / (WAVES / 4.0), (double)h.front() / calls, (double)h.back() / calls);
  return 0;
}

int main() {
  unsigned* out; unsigned long long* cyc; unsigned long long* bad; unsigned* sum; uint4* kat;
  CK(hipMalloc(&out, 256 * 512 * 4)); CK(hipMalloc(&cyc, 256 * 8 * 8)); CK(hipMalloc(&bad, 8)); CK(hipMalloc(&sum, 4)); CK(hipMalloc(&kat, 64));
  // ---- the two forms agree, and agree with the published vectors (Random123 kat_vectors: philox4x32 10)
  hipLaunchKernelGGL(kat_kernel, dim3(1), dim3(1), 0, 0, kat);
  uint4 hk[4];
  CK(hipMemcpy(hk, kat, 64, hipMemcpyDeviceToHost));
  const unsigned want0[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}, want1[4] = {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu};
  int kat_bad = 0;
  for (int f = 0; f < 2; ++f) {
    const uint4 a = hk[f], b = hk[2 + f];
    kat_bad += a.x != want0[0] || a.y != want0[1] || a.z != want0[2] || a.w != want0[3];
    kat_bad += b.x != want1[0] || b.y != want1[1] || b.z != want1[2] || b.w != want1[3];
  }
  printf("known answers (counter, key all 0 / all 0xFFFFFFFF), both forms: %s\n", kat_bad ? "MISMATCH" : "ok");
  const EqCase cases[6] = {
      {0u, 0u, 0u, 0u, 0u},
      {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
      {0u, 0xFFFFFFFFu, 30u, 1u, 0u},
      {0xFFFFFFFFu, 0u, 0u, 0u, 1u},
      {0x9E3779B9u, 0x85EBCA6Bu, 30u, 3u, 0x100u},
      {0xDEADBEEFu, 0x80000001u, 0xFFFFFFFFu, 0x7FFFFFFFu, 0x80000000u},
  };
  const unsigned n = 1u << 20;
  CK(hipMemset(bad, 0, 8)); CK(hipMemset(sum, 0, 4));
  for (int i = 0; i < 6; ++i) hipLaunchKernelGGL(equal_kernel, dim3(1024), dim3(256), 0, 0, cases[i], n, bad, sum);
  CK(hipDeviceSynchronize());
  unsigned long long hbad = 0; unsigned hsum = 0;
  CK(hipMemcpy(&hbad, bad, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&hsum, sum, 4, hipMemcpyDeviceToHost));
  printf("mul_hi + mul_lo against one 64-bit product: %llu of %u counters differ (xor of all words %08x)\n", hbad, 6 * n, hsum);
  // ---- the rates
  const int nit = 2000;
  double t[4];
  if (run<0, 4>("mul_hi + mul_lo pair, 1 wave/SIMD", out, cyc, nit, &t[0])) return 1;
  if (run<1, 4>("one 64-bit product,   1 wave/SIMD", out, cyc, nit, &t[1])) return 1;
  if (run<0, 8>("mul_hi + mul_lo pair, 2 waves/SIMD", out, cyc, nit, &t[2])) return 1;
  if (run<1, 8>("one 64-bit product,   2 waves/SIMD", out, cyc, nit, &t[3])) return 1;
  printf("64-bit product / pair: %.3f at 1 wave/SIMD, %.3f at 2 waves/SIMD\n", t[1] / t[0], t[3] / t[2]);
  return (kat_bad || hbad) ? 2 : 0;
}
