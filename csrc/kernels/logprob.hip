// Log-probabilities of sampled tokens (docs/PARITY.md "Sampling: logprobs"): per row the
// log-softmax (temperature 1) of the sampled token and of the N most likely tokens, over the
// logits the sampler is handed. It sits behind the sampler in every captured decode and prefill
// graph and only reads the logits. A row whose request did not ask (nlp < 0) or that is padding
// (ctx == 0) leaves before it loads a logit.
//
// One 1024-thread block per row. A live row is walked from cache (the lm_head just wrote it):
//   1. the maximum over non-NaN logits and their number;
//   2. sum of exp(x - max): each thread adds its terms in walk order, then a 6-level wave
//      butterfly and a 4-level tree over the 16 wave sums in LDS. No floating-point atomics:
//      the same bits on every launch and every graph replay;
//   N > 0 only:
//   3. radix select (8 bits per pass, sample_row.h logit_key) of the N-th largest logit: integer
//      LDS histograms, whose counts do not depend on the order of the adds;
//   4. one pass that collects the logits above that value (fewer than N, any order) and, wave by
//      wave over contiguous pieces of the row, the smallest token ids among the logits equal to
//      it (a constant row has `vocab` of them);
//   5. wave 0 ranks the <= 20 entries by (logit descending, id ascending) and writes them.
#include "common.h"
#include "kernels.h"
#include "sample_row.h"

namespace oamd {

constexpr int kLpThreads = 1024;
constexpr int kLpWaves = kLpThreads / kWave;

template <typename T>
__global__ void __launch_bounds__(kLpThreads) sample_logprobs_kernel(const T* __restrict__ logits, int64_t stride, int vocab,
                                                                    const int* __restrict__ nlp, const int* __restrict__ ctx,
                                                                    const int64_t* __restrict__ tokens,
                                                                    const int64_t* __restrict__ step, int C,
                                                                    float* __restrict__ tok_lp, float* __restrict__ top_lp,
                                                                    int* __restrict__ top_id) {
  constexpr int NB = static_cast<int>(sizeof(T));   // key digits
  constexpr int SH = 32 - 8 * NB;
  constexpr int VEC = 16 / static_cast<int>(sizeof(T));
  const int row = blockIdx.x;
  const int n_in = nlp[row];
  if (n_in < 0) return;                            // block-uniform: the request did not ask
  if (ctx != nullptr && ctx[row] == 0) return;     // a padding row of a decode bucket
  const int N = n_in < kLogprobsMax ? n_in : kLogprobsMax;
  const int col = step != nullptr ? static_cast<int>(static_cast<uint64_t>(step[0]) % static_cast<uint64_t>(C)) : 0;
  const int64_t o1 = static_cast<int64_t>(row) * C + col;
  float* out_lp = top_lp + o1 * kLogprobsMax;
  int* out_id = top_id + o1 * kLogprobsMax;

  __shared__ float smax[kLpWaves], ssum[kLpWaves];
  __shared__ uint32_t snv[kLpWaves];
  __shared__ uint32_t hc[256];
  __shared__ uint32_t s_bin, s_acnt, s_nab;
  __shared__ float s_ex[kLogprobsMax];
  __shared__ int s_ei[kLogprobsMax];
  __shared__ int wtie[kLpWaves][kLogprobsMax];
  __shared__ int wcnt[kLpWaves];
  const T* lr = logits + row * stride;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float kNaN = __uint_as_float(0x7fc00000u);

  // 1. the row's maximum and its number of non-NaN logits
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
  if (threadIdx.x == 0) s_nab = 0;
  __syncthreads();
  mx = smax[0];
  nvalid = snv[0];
#pragma unroll
  for (int j = 1; j < kLpWaves; ++j) { mx = fmaxf(mx, smax[j]); nvalid += snv[j]; }

  // 2. lse = mx + ln(sum exp(x - mx)); a term at the maximum is exactly 1 (also for mx = +-inf)
  float part = 0.f;
  walk_row<T>(lr, vocab, [&](float x) {
    if (!(x == x)) return;
    part += (x == mx) ? 1.f : exp2f((x - mx) * 1.4426950408889634f);
  });
  part = wave_sum(part);   // xor butterfly: every lane holds the same bits
  if (lane == 0) ssum[w] = part;
  __syncthreads();
  float tr[kLpWaves];
#pragma unroll
  for (int j = 0; j < kLpWaves; ++j) tr[j] = ssum[j];
#pragma unroll
  for (int o = 1; o < kLpWaves; o <<= 1)
#pragma unroll
    for (int j = 0; j < kLpWaves; j += 2 * o) tr[j] += tr[j + o];
  // no non-NaN logit: every log-probability is NaN (mx = -inf gives NaN by itself: -inf - -inf)
  const float lse = nvalid == 0 ? kNaN : mx + logf(tr[0]);

  if (threadIdx.x == 0) {
    const int64_t t = tokens[row];
    const float xt = (t >= 0 && t < vocab) ? load_logit<T>(lr, t) : kNaN;
    tok_lp[o1] = xt - lse;
  }
  if (N == 0) return;
  const int n_eff = static_cast<uint32_t>(N) < nvalid ? N : static_cast<int>(nvalid);
  if (n_eff == 0) {
    if (static_cast<int>(threadIdx.x) < N) { out_id[threadIdx.x] = -1; out_lp[threadIdx.x] = -INFINITY; }
    return;
  }

  // 3. the key of the n_eff-th largest logit, and the number of logits above it
  uint32_t prefix = 0, acnt = 0;
  for (int d = 0; d < NB; ++d) {
    for (int i = threadIdx.x; i < 256; i += kLpThreads) hc[i] = 0;
    __syncthreads();
    const int dsh = 8 * (NB - 1 - d);
    walk_row<T>(lr, vocab, [&](float x) {
      if (!(x == x)) return;
      const uint32_t kn = logit_key(x) >> SH;
      if (d > 0 && (kn >> (dsh + 8)) != prefix) return;
      atomicAdd(&hc[(kn >> dsh) & 255u], 1u);
    });
    __syncthreads();
    if (w == 0) {
      // lane l owns bins 255 - 4l .. 252 - 4l; inclusive scan of the counts over lanes
      uint32_t c[4], lc = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = hc[255 - (4 * lane + j)];
        lc += c[j];
      }
      uint32_t ic = lc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o, kWave);
        if (lane >= o) ic += oc;
      }
      uint32_t ec = acnt + (ic - lc);
      const uint32_t target = static_cast<uint32_t>(n_eff);
      if (ec < target && target <= ec + lc) {   // exactly one lane
        bool found = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!found && target <= ec + c[j]) {
            found = true;
            s_bin = 255 - (4 * lane + j);
            s_acnt = ec;
          }
          if (!found) ec += c[j];
        }
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | s_bin;
    acnt = s_acnt;
  }
  const int need = n_eff - static_cast<int>(acnt);   // places left for the logits equal to the cut, >= 1

  // 4. wave w walks groups [g0, g1) of 64 lanes x E consecutive columns, so that (wave, group,
  // lane, column in lane) is the order of the token ids; four groups in flight per lane
  const bool al = (reinterpret_cast<uintptr_t>(lr) & 15) == 0;
  const int E = al ? VEC : 1;
  const int gsz = 64 * E;
  const int G = static_cast<int>((static_cast<int64_t>(vocab) + gsz - 1) / gsz);
  const int gpw = (G + kLpWaves - 1) / kLpWaves;
  const int g0 = w * gpw < G ? w * gpw : G;
  const int g1 = g0 + gpw < G ? g0 + gpw : G;
  const uint4* lv = reinterpret_cast<const uint4*>(lr);
  auto load_group = [&](int g, float (&x)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) x[e] = kNaN;   // out of range: skipped like a NaN logit
    if (g >= g1) return;
    const int64_t base = static_cast<int64_t>(g) * gsz + lane * E;
    if (al && base + VEC <= vocab) {
      unpack16<T>(lv[base / VEC], x);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (e < E && base + e < vocab) x[e] = load_logit<T>(lr, base + e);
    }
  };
  int run = 0;   // logits equal to the cut seen by this wave so far (wave-uniform)
  auto take_group = [&](int g, const float (&x)[VEC]) {
    const int base = static_cast<int>(static_cast<int64_t>(g) * gsz + lane * E);
    uint32_t tie = 0;
    int c = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (!(x[e] == x[e])) continue;
      const uint32_t kn = logit_key(x[e]) >> SH;
      if (kn > prefix) {   // fewer than n_eff of these in the row: the order of arrival is sorted away below
        const uint32_t slot = atomicAdd(&s_nab, 1u);
        if (slot < static_cast<uint32_t>(kLogprobsMax)) { s_ex[slot] = x[e]; s_ei[slot] = base + e; }
      } else if (kn == prefix) {
        tie |= 1u << e;
        ++c;
      }
    }
    int ic = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int oc = __shfl_up(ic, o, kWave);
      if (lane >= o) ic += oc;
    }
    int r = run + ic - c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if (tie & (1u << e)) {
        if (r < need) wtie[w][r] = base + e;
        ++r;
      }
    }
    run += __shfl(ic, 63, kWave);
  };
  constexpr int UNR = 4;
  for (int g = g0; g < g1; g += UNR) {
    float x[UNR][VEC];
#pragma unroll
    for (int u = 0; u < UNR; ++u) load_group(g + u, x[u]);
#pragma unroll
    for (int u = 0; u < UNR; ++u) take_group(g + u, x[u]);
  }
  if (lane == 0) wcnt[w] = run < need ? run : need;
  __syncthreads();
  if (threadIdx.x == 0) {   // the first `need` ties in wave order behind the acnt entries above the cut
    const float tv = key_logit<NB>(prefix);
    int k = static_cast<int>(acnt);
    for (int j = 0; j < kLpWaves; ++j)
      for (int i = 0; i < wcnt[j] && k < n_eff; ++i, ++k) { s_ex[k] = tv; s_ei[k] = wtie[j][i]; }
  }
  __syncthreads();

  // 5. rank the n_eff entries by (logit descending, id ascending); the rest of the N are empty
  if (w == 0) {
    if (lane < n_eff) {
      const float x = s_ex[lane];
      const int id = s_ei[lane];
      const uint32_t k = logit_key(x);
      int rank = 0;
      for (int j = 0; j < n_eff; ++j) {
        const uint32_t kj = logit_key(s_ex[j]);
        rank += (kj > k || (kj == k && s_ei[j] < id)) ? 1 : 0;
      }
      out_id[rank] = id;
      out_lp[rank] = x - lse;
    } else if (lane < N) {
      out_id[lane] = -1;
      out_lp[lane] = -INFINITY;
    }
  }
}

int sample_logprobs(const void* logits, bool logits_bf16, int64_t stride, int rows, int vocab, const int* nlp,
                    const int* ctx, const int64_t* tokens, const int64_t* step, int C, float* tok_lp, float* top_lp,
                    int* top_id, hipStream_t stream) {
  if (rows == 0) return 0;
  if (logits_bf16)
    sample_logprobs_kernel<bf16_t><<<rows, kLpThreads, 0, stream>>>(static_cast<const bf16_t*>(logits), stride, vocab,
                                                                    nlp, ctx, tokens, step, C, tok_lp, top_lp, top_id);
  else
    sample_logprobs_kernel<float><<<rows, kLpThreads, 0, stream>>>(static_cast<const float*>(logits), stride, vocab, nlp,
                                                                   ctx, tokens, step, C, tok_lp, top_lp, top_id);
  OAMD_LAUNCH_CHECK();
  return 0;
}

}  // namespace oamd
