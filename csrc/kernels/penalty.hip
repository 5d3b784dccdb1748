// Repetition / frequency / presence penalties (docs/PARITY.md "Sampling: penalties"): the
// per-request token table on the device and the two kernels that keep and apply it.
//
// A request with a penalty owns one slot of the table (kernels.h PenaltyTable): cnt[slot][t]
// holds bit 31 = "t is in the prompt" and bits 0-30 = how often t was generated; lst[slot][0..n)
// names the tokens whose cnt word is non-zero, so a decode step touches the ~1k seen tokens of
// a row, not its 128k columns, and a slot is cleared by walking its previous occupant's list.
//
//   penalty_seed    one workgroup per request: clear the slot, then flag the prompt's tokens;
//   sample_penalty  one workgroup per logits row: count the token the step feeds in (the last
//                   sampled one), then rewrite the logits of the seen tokens in place.
//
// Both run on the engine's stream; stream order separates a slot's last use from its next
// seeding. Within a launch a slot belongs to one workgroup (the engine maps a slot to one
// request and a request to one row).
#include "common.h"
#include "kernels.h"

namespace oamd {

constexpr int kPenaltyThreads = 256;
constexpr uint32_t kPromptBit = 0x80000000u, kCountMask = 0x7fffffffu;

__global__ void __launch_bounds__(kPenaltyThreads) penalty_seed_kernel(const int* __restrict__ slots,
                                                                      const int64_t* __restrict__ ids, int64_t total,
                                                                      const int* __restrict__ cu, PenaltyTable T) {
  const int b = blockIdx.x;
  const int slot = slots[b];
  if (slot < 0 || slot >= T.slots) return;   // block-uniform
  int* cnt = T.cnt + static_cast<int64_t>(slot) * T.vocab;
  int* lst = T.lst + static_cast<int64_t>(slot) * T.cap;
  int* np = T.n + slot;
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = *np;
  __syncthreads();
  const int n0 = min(max(s_n, 0), T.cap);
  for (int i = threadIdx.x; i < n0; i += kPenaltyThreads) {
    const int t = lst[i];
    if (static_cast<uint32_t>(t) < static_cast<uint32_t>(T.vocab)) cnt[t] = 0;
  }
  if (threadIdx.x == 0) *np = 0;
  __syncthreads();   // the zeroes (cnt words, n) are in memory before any atomic below
  int64_t lo = cu[b], hi = cu[b + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > total ? total : hi;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kPenaltyThreads) {
    const int64_t t = ids[i];
    if (t < 0 || t >= T.vocab) continue;
    const uint32_t old = atomicOr(reinterpret_cast<uint32_t*>(cnt + t), kPromptBit);
    if (old != 0) continue;   // a duplicate: listed by the thread that saw 0
    const int k = atomicAdd(np, 1);
    if (k < T.cap) {
      lst[k] = static_cast<int>(t);
    } else {   // no room in the list (never for a prompt <= cap tokens): as if not seen
      atomicSub(np, 1);
      atomicAnd(reinterpret_cast<uint32_t*>(cnt + t), kCountMask);
    }
  }
}

// y of the semantics, every fp32 operation rounded on its own: no contraction into an FMA and a
// correctly rounded division, so plain fp32 torch (ops/reference.py sample_penalty) gives the
// same bits. The compiler contracts a * b + c by default, also inside the __fmul_rn / __fadd_rn
// wrappers once they are inlined, hence plain operators under the pragma.
__device__ __forceinline__ float penalised(float x, float r, float f, float p, uint32_t w) {
#pragma clang fp contract(off)
  float y = x;
  if (r != 1.f) y = (y > 0.f) ? y / r : y * r;
  const uint32_t c = w & kCountMask;
  if (c > 0) {
    const float fc = f * static_cast<float>(c);
    const float pen = fc + p;
    y = y - pen;
  }
  return y;
}

template <typename T>
__device__ __forceinline__ void store_logit(T* p, int64_t i, float v);
template <>
__device__ __forceinline__ void store_logit<float>(float* p, int64_t i, float v) { p[i] = v; }
template <>
__device__ __forceinline__ void store_logit<bf16_t>(bf16_t* p, int64_t i, float v) { p[i] = f2bf(v); }
template <typename T>
__device__ __forceinline__ float read_logit(const T* p, int64_t i);
template <>
__device__ __forceinline__ float read_logit<float>(const float* p, int64_t i) { return p[i]; }
template <>
__device__ __forceinline__ float read_logit<bf16_t>(const bf16_t* p, int64_t i) { return bf2f(p[i]); }

template <typename T>
__global__ void __launch_bounds__(kPenaltyThreads) sample_penalty_kernel(T* __restrict__ logits, int64_t stride, int vocab,
                                                                        const int* __restrict__ pslot,
                                                                        const int64_t* __restrict__ last_tok,
                                                                        const int* __restrict__ ctx,
                                                                        const float* __restrict__ rep,
                                                                        const float* __restrict__ freq,
                                                                        const float* __restrict__ pres, PenaltyTable tb) {
  const int row = blockIdx.x;
  const int slot = pslot[row];
  if (slot < 0 || slot >= tb.slots) return;        // block-uniform: no penalty on this row
  if (ctx != nullptr && ctx[row] == 0) return;     // a padding row of a decode bucket
  int* cnt = tb.cnt + static_cast<int64_t>(slot) * tb.vocab;
  int* lst = tb.lst + static_cast<int64_t>(slot) * tb.cap;
  const int nv = vocab < tb.vocab ? vocab : tb.vocab;
  __shared__ int s_n;
  if (threadIdx.x == 0) {
    int n = tb.n[slot];
    if (last_tok != nullptr) {   // count the token this step feeds in: the last sampled one
      const int64_t t = last_tok[row];
      if (t >= 0 && t < tb.vocab) {
        const uint32_t old = static_cast<uint32_t>(cnt[t]);
        if (old == 0) {
          if (n >= 0 && n < tb.cap) {   // a full list leaves both untouched
            lst[n] = static_cast<int>(t);
            tb.n[slot] = ++n;
            cnt[t] = 1;
          }
        } else if ((old & kCountMask) != kCountMask) {
          cnt[t] = static_cast<int>(old + 1u);
        }
      }
    }
    s_n = min(max(n, 0), tb.cap);
  }
  __syncthreads();   // the count and the list entry are visible to the whole workgroup
  const int n = s_n;
  const float r = rep[row], f = freq[row], p = pres[row];
  T* lr = logits + row * stride;
  // every listed token is distinct: one writer per logit, no atomics, no ordering dependence
  for (int i = threadIdx.x; i < n; i += kPenaltyThreads) {
    const int t = lst[i];
    if (static_cast<uint32_t>(t) >= static_cast<uint32_t>(nv)) continue;
    const uint32_t w = static_cast<uint32_t>(cnt[t]);
    const float x = read_logit<T>(lr, t);
    if (x != x) continue;   // NaN stays NaN, payload included
    store_logit<T>(lr, t, penalised(x, r, f, p, w));
  }
}

int penalty_seed(const int* slots, int reqs, const int64_t* ids, int64_t total, const int* cu, PenaltyTable table,
                 hipStream_t stream) {
  if (reqs == 0) return 0;
  penalty_seed_kernel<<<reqs, kPenaltyThreads, 0, stream>>>(slots, ids, total, cu, table);
  OAMD_LAUNCH_CHECK();
  return 0;
}

int sample_penalty(void* logits, bool logits_bf16, int64_t stride, int rows, int vocab, const int* pslot,
                   const int64_t* last_tok, const int* ctx, const float* rep, const float* freq, const float* pres,
                   PenaltyTable table, hipStream_t stream) {
  if (rows == 0) return 0;
  if (logits_bf16)
    sample_penalty_kernel<bf16_t><<<rows, kPenaltyThreads, 0, stream>>>(static_cast<bf16_t*>(logits), stride, vocab,
                                                                        pslot, last_tok, ctx, rep, freq, pres, table);
  else
    sample_penalty_kernel<float><<<rows, kPenaltyThreads, 0, stream>>>(static_cast<float*>(logits), stride, vocab,
                                                                       pslot, last_tok, ctx, rep, freq, pres, table);
  OAMD_LAUNCH_CHECK();
  return 0;
}

}  // namespace oamd
