// Token sampler: temperature + Gumbel-max over the
// vocabulary (or one tensor-parallel vocab shard: col_offset + out_val let the
// caller take the max over shards, Gumbel-max being decomposable), greedy when temperature <= 0. One 1024-thread block per row;
// each thread keeps a (value, index) pair over a grid-stride of the vocab with
// 16-B loads, then a wave + LDS argmax. The noise is a counter-based hash of
// (seed[row], position[row], column), so a captured hipGraph replays to the
// same tokens and the kernel needs no RNG state on the device.
#include "common.h"
#include "kernels.h"
#include "sample_row.h"

namespace oamd {

__device__ __forceinline__ void argmax_merge(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// Filtered: only columns with x >= thr[row] take part (top-k / top-p, sample_threshold_kernel
// below). The comparison is on the raw logit, before temperature and noise: thr = -inf keeps
// every column (NaN included, which argmax_merge never picks), so such a row returns the
// token and value bits of the unfiltered instantiation.
template <typename T, bool Filtered>
__global__ void __launch_bounds__(1024) sample_kernel(const T* __restrict__ logits, int64_t stride, int vocab,
                                                      const float* __restrict__ temperature,
                                                      const int64_t* __restrict__ seeds,
                                                      const int64_t* __restrict__ positions,
                                                      int64_t* __restrict__ out_tokens, int64_t col_offset,
                                                      float* __restrict__ out_val, const float* __restrict__ thr) {
  __shared__ float sv[16];
  __shared__ int si[16];
  const int row = blockIdx.x;
  const T* lr = logits + row * stride;
  const float temp = temperature[row];
  const bool greedy = !(temp > 0.f);
  // Perturbed values are compared in base 2: x/T - ln(-ln u) = ln2 * (x log2e / T -
  // log2(-log2 u)) - ln(ln2), a monotone map, so the loop pays one FMA and two v_log_f32
  // per column and the winner is mapped back once (out_val stays in natural units).
  constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f, kNegLnLn2 = 0.36651292058166435f;
  const float inv_t = greedy ? 1.f : kLog2e / temp;
  const uint64_t key = mix64((static_cast<uint64_t>(seeds[row]) * 0x9E3779B97F4A7C15ULL) ^
                             (static_cast<uint64_t>(positions[row]) << 32));
  const uint32_t k1 = static_cast<uint32_t>(key), k2 = static_cast<uint32_t>(key >> 32);
  const uint32_t c0 = static_cast<uint32_t>(col_offset);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  float tau = -INFINITY;
  if constexpr (Filtered) tau = thr[row];
  auto visit = [&](float x, int i) {
    if constexpr (Filtered) {
      if (x < tau) return;
    }
    if (!greedy) {
      const float u = uniform01(hash_col(c0 + static_cast<uint32_t>(i), k1, k2));
      // -log2(u) >= 8.6e-8 exactly; the clamp only guards a hardware log rounding to 0
      x = x * inv_t - __builtin_amdgcn_logf(fmaxf(-__builtin_amdgcn_logf(u), 5.9604645e-8f));
    }
    argmax_merge(bv, bi, x, i);
  };
  // 16-B loads over the aligned body of the row (8 bf16 / 4 fp32 per lane), scalar tail.
  // argmax_merge is a total order (value, then smaller index), so the visiting order
  // does not change the result.
  constexpr int VEC = 16 / static_cast<int>(sizeof(T));
  const int nv = (reinterpret_cast<uintptr_t>(lr) & 15) == 0 ? vocab / VEC : 0;
  auto visit16 = [&](const uint4& raw, int v) {
    const uint32_t wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (sizeof(T) == 2) {
        visit(__uint_as_float(wv[k] << 16), VEC * v + 2 * k);
        visit(__uint_as_float(wv[k] & 0xffff0000u), VEC * v + 2 * k + 1);
      } else {
        visit(__uint_as_float(wv[k]), VEC * v + k);
      }
    }
  };
  // UNR row vectors per thread requested before any is consumed: one dependent HBM round
  // trip per UNR vectors instead of per vector (the loop was latency-bound: ~16 trips
  // of 16 B per thread for a 128k vocab row)
  constexpr int UNR = 4;
  const uint4* lv = reinterpret_cast<const uint4*>(lr);
  const int step = blockDim.x;
  int v0 = threadIdx.x;
  for (; v0 + (UNR - 1) * step < nv; v0 += UNR * step) {
    uint4 raw[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) raw[u] = lv[v0 + u * step];
#pragma unroll
    for (int u = 0; u < UNR; ++u) visit16(raw[u], v0 + u * step);
  }
  for (int v = v0; v < nv; v += step) visit16(lv[v], v);
  for (int i = nv * VEC + threadIdx.x; i < vocab; i += blockDim.x) visit(load_logit<T>(lr, i), i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, kWave);
    const int oi = __shfl_xor(bi, o, kWave);
    argmax_merge(bv, bi, ov, oi);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sv[w] = bv; si[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = sv[0];
    int id = si[0];
    for (int j = 1; j < (int)(blockDim.x >> 6); ++j) argmax_merge(v, id, sv[j], si[j]);
    out_tokens[row] = ((id == 0x7fffffff) ? 0 : id) + col_offset;
    if (out_val) out_val[row] = greedy ? v : v * kLn2 + kNegLnLn2;
  }
}

// ---------------------------------------------------------------------------------------------
// Top-k / top-p threshold (docs/PARITY.md "Sampling"): per row the logit value tau such that
// the candidate set is {x >= tau}. Radix select, 8 bits per pass, on an order-preserving
// integer key of the logit; a bf16 logit has 16 significant key bits, so two passes per
// select, an fp32 logit four.
// ---------------------------------------------------------------------------------------------

// One 1024-thread block per row. thr[row] = max(tau_k, tau_p):
//   tau_k: the top_k-th largest logit (ties at it are all kept); off for top_k <= 0 or >= vocab;
//   tau_p: the largest logit v whose mass m(v) = sum over kept x >= v of exp((x - max) / T)
//          reaches top_p * m(tau_k); off for top_p >= 1;
// -inf for a greedy row (T <= 0) or one with both off, decided from the row's three parameters
// before any logit is loaded. kept[row] (optional) = columns with x >= thr, vocab for such rows.
// NaN logits are never kept. Each select walks the row once per key digit (re-read from L2),
// building a 256-bin LDS histogram of the elements under the digits found so far, then wave 0
// scans the bins from the top to the one where the running count reaches top_k / the running
// mass reaches its target. Masses are 2^40 fixed-point integers added with integer LDS
// atomics, so the sums, and with them thr, do not depend on the order of the adds: the same
// bits on every run and every graph replay (152,064 terms <= 2^40 stay below 2^58).
template <typename T>
__global__ void __launch_bounds__(1024) sample_threshold_kernel(const T* __restrict__ logits, int64_t stride, int vocab,
                                                                const float* __restrict__ temperature,
                                                                const int* __restrict__ top_k,
                                                                const float* __restrict__ top_p,
                                                                float* __restrict__ thr, int* __restrict__ kept) {
  constexpr int NB = static_cast<int>(sizeof(T));   // key digits
  constexpr int SH = 32 - 8 * NB;
  const int row = blockIdx.x;
  const float temp = temperature[row];
  const int k_in = top_k[row];
  const float p_in = top_p[row];
  const bool use_k = k_in > 0 && k_in < vocab;
  const bool use_p = p_in < 1.f;
  if (!(temp > 0.f) || !(use_k || use_p)) {   // block-uniform
    if (threadIdx.x == 0) {
      thr[row] = -INFINITY;
      if (kept) kept[row] = vocab;
    }
    return;
  }
  __shared__ uint32_t hc[256];
  __shared__ unsigned long long hm[256];
  __shared__ float smax[16];
  __shared__ uint32_t snv[16];
  __shared__ uint32_t s_bin, s_acnt, s_bcnt;
  __shared__ unsigned long long s_amass;
  const T* lr = logits + row * stride;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;

  // the row's maximum and its number of non-NaN logits
  float mx = -INFINITY;
  uint32_t nvalid = 0;
  walk_row<T>(lr, vocab, [&](float x) {
    if (x == x) {
      mx = fmaxf(mx, x);
      ++nvalid;
    }
  });
  mx = wave_max(mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nvalid += __shfl_xor(nvalid, o, kWave);
  if (lane == 0) { smax[w] = mx; snv[w] = nvalid; }
  __syncthreads();
  mx = smax[0];
  nvalid = snv[0];
  for (int j = 1; j < (int)(blockDim.x >> 6); ++j) { mx = fmaxf(mx, smax[j]); nvalid += snv[j]; }
  if (nvalid == 0 || !(mx > -INFINITY)) {   // nothing but NaN / -inf: every mass is 0, nothing to cut
    if (threadIdx.x == 0) {
      thr[row] = -INFINITY;
      if (kept) kept[row] = static_cast<int>(nvalid);
    }
    return;
  }

  const float inv_t = 1.4426950408889634f / temp;
  auto mass_of = [&](float x) -> unsigned long long {
    if (x == mx) return 1ull << 40;   // exact, also for mx = +inf and T so small that 1 / T = inf
    // x < mx: the exponent is negative or -inf (fmaxf drops the NaN of -inf * 0 at T = inf)
    return static_cast<unsigned long long>(fmaxf(exp2f((x - mx) * inv_t), 0.f) * 1099511627776.f);
  };

  uint32_t lo = 0;        // key of tau_k: elements below it take no part in the mass select
  uint32_t prefix = 0;    // key digits found so far
  uint32_t acnt = 0, bcnt = 0;       // elements above the prefix / equal to it (after the last digit)
  unsigned long long amass = 0;      // mass above the prefix
  // by_mass false: the bin where the count from the top reaches `target`; true: where the mass
  // reaches top_p * (the whole mass), at least 1 unit so an empty bin is never chosen
  auto run_select = [&](const bool by_mass, unsigned long long target) {
    prefix = 0; acnt = 0; amass = 0;
    for (int d = 0; d < NB; ++d) {
      for (int i = threadIdx.x; i < 256; i += blockDim.x) { hc[i] = 0; hm[i] = 0; }
      __syncthreads();
      const int dsh = 8 * (NB - 1 - d);
      walk_row<T>(lr, vocab, [&](float x) {
        if (!(x == x)) return;
        const uint32_t kn = logit_key(x) >> SH;
        if (kn < lo) return;
        if (d > 0 && (kn >> (dsh + 8)) != prefix) return;
        const uint32_t b = (kn >> dsh) & 255u;
        atomicAdd(&hc[b], 1u);
        if (by_mass) {
          const unsigned long long m = mass_of(x);
          if (m) atomicAdd(&hm[b], m);
        }
      });
      __syncthreads();
      if (w == 0) {
        // lane l owns bins 255 - 4l .. 252 - 4l; inclusive scan of (count, mass) over lanes
        uint32_t c[4], lc = 0;
        unsigned long long m[4], lm = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = 255 - (4 * lane + j);
          c[j] = hc[b];
          m[j] = hm[b];
          lc += c[j];
          lm += m[j];
        }
        uint32_t ic = lc;
        unsigned long long im = lm;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t oc = __shfl_up(ic, o, kWave);
          const unsigned long long om = __shfl_up(im, o, kWave);
          if (lane >= o) { ic += oc; im += om; }
        }
        if (by_mass && d == 0) {
          const unsigned long long Z = __shfl(im, 63, kWave);   // >= 2^40: the maximum is in it
          const double t = ceil(static_cast<double>(fmaxf(p_in, 0.f)) * static_cast<double>(Z));
          target = static_cast<unsigned long long>(t);
          target = target < 1 ? 1 : (target > Z ? Z : target);
        }
        uint32_t ec = acnt + (ic - lc);
        unsigned long long em = amass + (im - lm);
        const unsigned long long ex = by_mass ? em : ec, lv = by_mass ? lm : lc;
        if (ex < target && target <= ex + lv) {   // exactly one lane
          bool found = false;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned long long cur = by_mass ? em : ec, v = by_mass ? m[j] : c[j];
            if (!found && target <= cur + v) {
              found = true;
              s_bin = 255 - (4 * lane + j);
              s_acnt = ec;
              s_amass = em;
              s_bcnt = c[j];
            }
            if (!found) { ec += c[j]; em += m[j]; }
          }
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | s_bin;
      acnt = s_acnt;
      amass = s_amass;
      bcnt = s_bcnt;
    }
  };

  if (use_k) {
    run_select(false, static_cast<uint32_t>(k_in) < nvalid ? static_cast<uint32_t>(k_in) : nvalid);
    lo = prefix;
  }
  if (use_p) run_select(true, 0);
  if (threadIdx.x == 0) {
    thr[row] = key_logit<NB>(prefix);
    if (kept) kept[row] = static_cast<int>(acnt + bcnt);
  }
}

int sample_tokens(const void* logits, bool logits_bf16, int64_t stride, int rows, int vocab,
                  const float* temperature, const int64_t* seeds, const int64_t* positions,
                  int64_t* out_tokens, int64_t col_offset, float* out_val, hipStream_t stream, const float* thr) {
  if (rows == 0) return 0;
  if (thr != nullptr) {
    if (logits_bf16)
      sample_kernel<bf16_t, true><<<rows, 1024, 0, stream>>>(static_cast<const bf16_t*>(logits), stride, vocab,
                                                             temperature, seeds, positions, out_tokens, col_offset,
                                                             out_val, thr);
    else
      sample_kernel<float, true><<<rows, 1024, 0, stream>>>(static_cast<const float*>(logits), stride, vocab,
                                                            temperature, seeds, positions, out_tokens, col_offset,
                                                            out_val, thr);
  } else if (logits_bf16) {
    sample_kernel<bf16_t, false><<<rows, 1024, 0, stream>>>(static_cast<const bf16_t*>(logits), stride, vocab,
                                                            temperature, seeds, positions, out_tokens, col_offset,
                                                            out_val, nullptr);
  } else {
    sample_kernel<float, false><<<rows, 1024, 0, stream>>>(static_cast<const float*>(logits), stride, vocab,
                                                           temperature, seeds, positions, out_tokens, col_offset,
                                                           out_val, nullptr);
  }
  OAMD_LAUNCH_CHECK();
  return 0;
}

int sample_threshold(const void* logits, bool logits_bf16, int64_t stride, int rows, int vocab,
                     const float* temperature, const int* top_k, const float* top_p, float* thr, int* kept,
                     hipStream_t stream) {
  if (rows == 0) return 0;
  if (logits_bf16)
    sample_threshold_kernel<bf16_t><<<rows, 1024, 0, stream>>>(static_cast<const bf16_t*>(logits), stride, vocab,
                                                               temperature, top_k, top_p, thr, kept);
  else
    sample_threshold_kernel<float><<<rows, 1024, 0, stream>>>(static_cast<const float*>(logits), stride, vocab,
                                                              temperature, top_k, top_p, thr, kept);
  OAMD_LAUNCH_CHECK();
  return 0;
}

}  // namespace oamd

