// Device-resident training set: one launch gathers one packed batch (include/ttsk.h, tts_king_amd/resident.py).
//   collate_kernel   ragged rows of up to TTSK_COLLATE_MAX_FIELDS flat fields -> the zero-padded (B, padded_rows, inner) fields of the
//                    feeder's packed layout, plus the by-value frame / phoneme limits
// The destination drives the work: the buffer is cut into 16-byte pieces, one thread per piece, grid-strided, so every byte is written
// exactly once by a 16-byte store whatever it is (a row's data, its padding, the gap behind a field) and small fields cost as many
// lanes as they have bytes.  A piece that lies inside one utterance's rows and whose source is 16-byte aligned is one 16-byte load
// (every mel piece: rows of 320 bytes from a 16-byte aligned start); any other piece is put together from dword loads.  Memory-bound
// and nearly all mel: consecutive lanes read and write consecutive 16 bytes of a row.  No atomics, no LDS, no host synchronisation.
// Everything the kernel reads from device tables (utterance number, offset, length) is checked against the sizes that came by value
// before it forms an address.
#include <string.h>
#include "common.h"

namespace {

struct Region {                 // one field as the kernel sees it
  const uint32_t* src;          // (elem_size is 4 or 8: the array as dwords)
  const int64_t* offsets;
  const int32_t* lens;
  int64_t n_src;                // elements
  uint32_t start;               // first byte of the field in dst; its region runs to the next region's start
  uint32_t row_bytes;           // inner * elem_size
  uint32_t utt_bytes;           // padded_rows * row_bytes
  int32_t padded_rows, inner, elem_size, nan_to_zero;
};

struct CollateArgs {
  Region reg[TTSK_COLLATE_MAX_FIELDS];
  int n_regions;
  int B;
  int64_t n_utts;
  const int32_t* idx;
  uint32_t n_pieces;            // dst_bytes / 16
  uint32_t fl_off, pl_off;      // byte offsets, 0xFFFFFFFF = absent
  int32_t t_true;
  int64_t l_true;
};

// rows of batch entry b that exist and may be read: (first source dword, valid bytes), (0, 0) for anything out of range
__device__ __forceinline__ void utt_span(const Region& r, const CollateArgs& a, uint32_t b, int64_t& first_dword, uint32_t& valid_bytes) {
  first_dword = 0;
  valid_bytes = 0;
  const int64_t u = a.idx[b];
  if (u < 0 || u >= a.n_utts) return;
  const int64_t off = r.offsets[u];
  const int64_t len = r.lens[u];
  if (off < 0 || len <= 0 || len > r.padded_rows || off > r.n_src || len * r.inner > r.n_src - off) return;
  first_dword = off * (r.elem_size >> 2);
  valid_bytes = (uint32_t)len * r.row_bytes;
}

__device__ __forceinline__ uint32_t clean(uint32_t w, int nan_to_zero) {
  return (nan_to_zero && (w & 0x7FFFFFFFu) > 0x7F800000u) ? 0u : w;
}

// the dword at byte p of the field's region (p a multiple of 4)
__device__ __forceinline__ uint32_t field_dword(const Region& r, const CollateArgs& a, uint32_t p) {
  const uint32_t b = p / r.utt_bytes;
  if (b >= (uint32_t)a.B) return 0u;                    // the gap behind the field
  const uint32_t q = p - b * r.utt_bytes;
  int64_t first;
  uint32_t valid;
  utt_span(r, a, b, first, valid);
  return q < valid ? clean(r.src[first + (q >> 2)], r.nan_to_zero) : 0u;
}

__global__ __launch_bounds__(256) void collate_kernel(const CollateArgs a, uint4* __restrict__ dst) {
  for (uint32_t piece = blockIdx.x * 256u + threadIdx.x; piece < a.n_pieces; piece += gridDim.x * 256u) {
    const uint32_t pos = piece << 4;                    // (dst_bytes < 2^31)
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    int ri = -1;
    for (int i = 0; i < a.n_regions; ++i) ri = pos >= a.reg[i].start ? i : ri;
    if (a.pl_off != 0xFFFFFFFFu && pos >= a.pl_off) {   // B int64 l_true, then zeros
      const uint32_t e = (pos - a.pl_off) >> 3;
      const uint32_t lo = (uint32_t)a.l_true, hi = (uint32_t)((uint64_t)a.l_true >> 32);
      if (e < (uint32_t)a.B) { o.x = lo; o.y = hi; }
      if (e + 1 < (uint32_t)a.B) { o.z = lo; o.w = hi; }
    } else if (a.fl_off != 0xFFFFFFFFu && pos >= a.fl_off) {   // int32 t_true, then zeros
      if (pos == a.fl_off) o.x = (uint32_t)a.t_true;
    } else if (ri >= 0) {
      const Region& r = a.reg[ri];
      const uint32_t p = pos - r.start;
      const uint32_t b = p / r.utt_bytes;
      const uint32_t q = p - b * r.utt_bytes;
      if (b < (uint32_t)a.B && q + 16u <= r.utt_bytes) {         // the piece lies in one utterance's padded rows
        int64_t first;
        uint32_t valid;
        utt_span(r, a, b, first, valid);
        const uint32_t* s = r.src + first + (q >> 2);
        if (q + 16u <= valid && (((uintptr_t)s) & 15) == 0) {
          o = *reinterpret_cast<const uint4*>(s);
          if (r.nan_to_zero) o = make_uint4(clean(o.x, 1), clean(o.y, 1), clean(o.z, 1), clean(o.w, 1));
        } else if (q < valid) {                                  // unaligned source, or the row's data ends inside the piece
          o.x = clean(s[0], r.nan_to_zero);
          if (q + 4u < valid) o.y = clean(s[1], r.nan_to_zero);
          if (q + 8u < valid) o.z = clean(s[2], r.nan_to_zero);
          if (q + 12u < valid) o.w = clean(s[3], r.nan_to_zero);
        }
      } else if (b < (uint32_t)a.B) {                            // the piece straddles utterances (or the field's end)
        o.x = field_dword(r, a, p);
        o.y = field_dword(r, a, p + 4u);
        o.z = field_dword(r, a, p + 8u);
        o.w = field_dword(r, a, p + 12u);
      }
    }
    dst[piece] = o;
  }
}

int n_compute_units() {
  static int n_cus = 0;
  if (n_cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return -1;
    n_cus = v;
  }
  return n_cus;
}

}  // namespace

extern "C" int ttsk_collate_batch(const ttsk_collate_field* fields, int n_fields, const int32_t* idx_dev, const int32_t* idx_host, int B,
                                  int64_t n_utts, void* dst, int64_t dst_bytes, int64_t fl_off, int32_t t_true, int64_t pl_off,
                                  int64_t l_true, void* stream) {
  TTSK_REQUIRE(fields && idx_dev && idx_host && dst && B > 0 && n_utts > 0, "collate_batch: bad arguments");
  TTSK_REQUIRE(n_fields > 0 && n_fields <= TTSK_COLLATE_MAX_FIELDS, "collate_batch: %d fields, must be 1..%d", n_fields, TTSK_COLLATE_MAX_FIELDS);
  TTSK_REQUIRE(dst_bytes > 0 && dst_bytes % 16 == 0 && dst_bytes < ((int64_t)1 << 31) && (((uintptr_t)dst) & 15) == 0,
               "collate_batch: the batch buffer must be 16-byte aligned and a multiple of 16 bytes below 2^31 (%lld)", (long long)dst_bytes);
  for (int b = 0; b < B; ++b)
    TTSK_REQUIRE(idx_host[b] >= 0 && idx_host[b] < n_utts, "collate_batch: batch entry %d is utterance %d, outside the store's %lld", b,
                 idx_host[b], (long long)n_utts);
  CollateArgs a;
  memset(&a, 0, sizeof(a));
  int64_t end = 0;                                      // first byte behind the regions checked so far
  for (int f = 0; f < n_fields; ++f) {
    const ttsk_collate_field& s = fields[f];
    TTSK_REQUIRE(s.elem_size == 4 || s.elem_size == 8, "collate_batch: field %d has element size %d, must be 4 or 8", f, s.elem_size);
    TTSK_REQUIRE(s.src && s.offsets && s.lens && s.lens_host && s.n_src > 0 && s.inner > 0 && s.padded_rows > 0, "collate_batch: field %d: bad arguments", f);
    TTSK_REQUIRE((((uintptr_t)s.src) & (uintptr_t)(s.elem_size - 1)) == 0, "collate_batch: field %d: source not aligned to its element size", f);
    TTSK_REQUIRE(!s.nan_to_zero || s.elem_size == 4, "collate_batch: field %d: nan_to_zero needs 4-byte (fp32) elements", f);
    const int64_t row_bytes = (int64_t)s.inner * s.elem_size;
    const int64_t bytes = (int64_t)B * s.padded_rows * row_bytes;
    TTSK_REQUIRE(row_bytes < ((int64_t)1 << 31) && (int64_t)s.padded_rows * row_bytes < ((int64_t)1 << 31), "collate_batch: field %d: padded rows too large", f);
    TTSK_REQUIRE(s.dst_off >= end && s.dst_off % 16 == 0 && bytes <= dst_bytes - s.dst_off,
                 "collate_batch: field %d at byte %lld (%lld bytes) overlaps its predecessor, is not 16-byte aligned or leaves the buffer of %lld",
                 f, (long long)s.dst_off, (long long)bytes, (long long)dst_bytes);
    for (int b = 0; b < B; ++b) {
      const int32_t len = s.lens_host[idx_host[b]];
      TTSK_REQUIRE(len >= 0 && len <= s.padded_rows, "collate_batch: field %d: utterance %d has %d rows, the padded length is %d", f, idx_host[b],
                   len, s.padded_rows);
    }
    end = s.dst_off + bytes;
    Region& r = a.reg[f];
    r.src = (const uint32_t*)s.src;
    r.offsets = s.offsets;
    r.lens = s.lens;
    r.n_src = s.n_src;
    r.start = (uint32_t)s.dst_off;
    r.row_bytes = (uint32_t)row_bytes;
    r.utt_bytes = (uint32_t)(s.padded_rows * row_bytes);
    r.padded_rows = s.padded_rows;
    r.inner = s.inner;
    r.elem_size = s.elem_size;
    r.nan_to_zero = s.nan_to_zero;
  }
  a.fl_off = a.pl_off = 0xFFFFFFFFu;
  if (fl_off >= 0) {
    TTSK_REQUIRE(fl_off >= end && fl_off % 16 == 0 && fl_off + 4 <= dst_bytes, "collate_batch: frame limit at byte %lld: inside a field, unaligned or outside the buffer",
                 (long long)fl_off);
    a.fl_off = (uint32_t)fl_off;
    end = fl_off + 4;
  }
  if (pl_off >= 0) {
    TTSK_REQUIRE(pl_off >= end && pl_off % 16 == 0 && pl_off + (int64_t)B * 8 <= dst_bytes,
                 "collate_batch: phoneme limits at byte %lld: inside a field or the frame limit, unaligned or outside the buffer", (long long)pl_off);
    a.pl_off = (uint32_t)pl_off;
  }
  a.n_regions = n_fields;
  a.B = B;
  a.n_utts = n_utts;
  a.idx = idx_dev;
  a.n_pieces = (uint32_t)(dst_bytes >> 4);
  a.t_true = t_true;
  a.l_true = l_true;
  const int cus = n_compute_units();
  TTSK_REQUIRE(cus > 0, "collate_batch: cannot read the device's compute-unit count");
  const int64_t want = ((int64_t)a.n_pieces + 255) / 256, cap = (int64_t)cus * 8;
  const int grid = (int)(want < cap ? want : cap);
  hipLaunchKernelGGL(collate_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, (uint4*)dst);
  TTSK_CHECK_LAUNCH();
  return TTSK_OK;
}
