// Row helpers shared by the sampler kernels (sample.hip, logprob.hip): loading a logit, the
// order-preserving integer key of the radix selects, and the 16-byte walk over a logits row.
#pragma once

#include "common.h"

namespace oamd {

template <typename T>
__device__ __forceinline__ float load_logit(const T* p, int64_t i);
template <>
__device__ __forceinline__ float load_logit<float>(const float* p, int64_t i) { return p[i]; }
template <>
__device__ __forceinline__ float load_logit<bf16_t>(const bf16_t* p, int64_t i) { return bf2f(p[i]); }

// Sign bit flipped for non-negatives, every bit for negatives: unsigned key order == float
// order, -inf lowest, +inf highest. -0 and +0 are one value. (NaN is never given a key.)
__device__ __forceinline__ uint32_t logit_key(float x) {
  uint32_t b = __float_as_uint(x);
  if (x == 0.f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Inverse of logit_key(x) >> (32 - 8 NB) for a logit whose low 32 - 8 NB bits are zero.
template <int NB>
__device__ __forceinline__ float key_logit(uint32_t kn) {
  constexpr int SH = 32 - 8 * NB;
  const uint32_t full = kn << SH;
  const uint32_t b = (full & 0x80000000u) ? (full ^ 0x80000000u) : (~full & (0xffffffffu << SH));
  return __uint_as_float(b);
}

// The 8 bf16 / 4 fp32 logits of one 16-byte row vector, in column order.
template <typename T>
__device__ __forceinline__ void unpack16(const uint4& raw, float (&x)[16 / sizeof(T)]) {
  const uint32_t wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (sizeof(T) == 2) {
      x[2 * k] = __uint_as_float(wv[k] << 16);
      x[2 * k + 1] = __uint_as_float(wv[k] & 0xffff0000u);
    } else {
      x[k] = __uint_as_float(wv[k]);
    }
  }
}

// f(x) for every column of a row, in sample_kernel's order: 16-B loads over the aligned body
// (four in flight per thread), scalar tail; a row off a 16-B boundary is all tail.
template <typename T, typename F>
__device__ __forceinline__ void walk_row(const T* __restrict__ lr, int vocab, F&& f) {
  constexpr int VEC = 16 / static_cast<int>(sizeof(T));
  const int nv = (reinterpret_cast<uintptr_t>(lr) & 15) == 0 ? vocab / VEC : 0;
  auto f16 = [&](const uint4& raw) {
    const uint32_t wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (sizeof(T) == 2) {
        f(__uint_as_float(wv[k] << 16));
        f(__uint_as_float(wv[k] & 0xffff0000u));
      } else {
        f(__uint_as_float(wv[k]));
      }
    }
  };
  constexpr int UNR = 4;
  const uint4* lv = reinterpret_cast<const uint4*>(lr);
  const int step = blockDim.x;
  int v0 = threadIdx.x;
  for (; v0 + (UNR - 1) * step < nv; v0 += UNR * step) {
    uint4 raw[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) raw[u] = lv[v0 + u * step];
#pragma unroll
    for (int u = 0; u < UNR; ++u) f16(raw[u]);
  }
  for (int v = v0; v < nv; v += step) f16(lv[v]);
  for (int i = nv * VEC + threadIdx.x; i < vocab; i += blockDim.x) f(load_logit<T>(lr, i));
}

}  // namespace oamd
