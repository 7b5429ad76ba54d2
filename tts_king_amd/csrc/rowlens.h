// A per-row length beside the batch stride, for the fused HiFi-GAN kernels (include/ttsk.h: the *_rowlen entry points).
// Those kernels carry one `len` that is both the row stride of the (B, len, C) batch and the edge beyond which a conv reads and
// writes zero.  With an argument block of type WithRows<Args> the two part: the stride stays a.len, the edge of row b becomes
// frames[b * stride] * spf clamped to [1, len] (frames <= 0, or a null array: the whole row), so that a row of a windowed batch can
// hold an utterance shorter than the window and still meet the zero padding a solo run gives it.  The plain Args instantiations do
// not see any of this: edge_len() is a.len there and the early return is compiled out.
#pragma once
#include <stdint.h>

struct RowLens {
  const int32_t* frames;   // valid mel frames per row (the plan column TTSK_WIN_VALID, or a compact copy); null = every row full
  int stride;              // int32 elements between two rows' entries
  int spf;                 // samples per mel frame at the kernel's stage
};

template <typename A> struct WithRows : A { RowLens rl; };
template <typename A> struct HasRows { static constexpr bool value = false; };
template <typename A> struct HasRows<WithRows<A>> { static constexpr bool value = true; };

// the edge of row b: positions >= the result are conv zero padding.  Never more than `len`, whatever the table holds.
__device__ __forceinline__ int row_edge(const RowLens& r, int b, int len) {
  if (!r.frames) return len;
  const int v = r.frames[(int64_t)b * r.stride];
  if (v <= 0) return len;
  const int64_t e = (int64_t)v * r.spf;
  return e < len ? (int)e : len;
}
template <typename A> __device__ __forceinline__ int edge_len(const A& a, int b) {
  if constexpr (HasRows<A>::value) return row_edge(a.rl, b, a.len);
  else return a.len;
}

// host side: the checks every *_rowlen entry point makes before it launches
#define TTSK_REQUIRE_ROWS(name, row_stride, spf) \
  TTSK_REQUIRE((row_stride) > 0 && (spf) > 0, name ": row_stride=%d and spf=%d must be positive", (int)(row_stride), (int)(spf))
