// Four-wave decode GEMM for the 256-row bucket on the loop discipline of gemm_tile.hip's p5:
//   Y[256, N] = X[256, K] . W[N, K]^T, bf16 in, fp32 accumulate
// (SURVEY.md §2.4 N7 "Decode uses skinny-M split-K with nt weight streaming").
//
// gemm_pp / gemm_tn split the 256 x 128 decode tile over 8 waves (64 x 32 or 64 x 64 outputs per
// wave): 0.625 / 0.5 KB of LDS fragment reads per MFMA, and a wave never overlaps its own reads
// with its own MFMAs (profiles/decode_gemm_lds_pmc_r7.txt: the MFMA pipes are busy ~49 % of the
// time). Here:
//   * tile = 256 tokens x 128 features, BK = 64, 4 waves laid out 2 (M) x 2 (N), one per SIMD;
//     a wave holds 128 tokens x 64 features = 32 accumulator fragments in 128 tied AGPRs;
//   * per k-half (32 of K) 8 X + 4 W fragments (12 ds_read_b128) feed 32 MFMAs: 0.375 KB per
//     MFMA. The fragments are double-buffered in registers: the reads of k-half 1 ride on the
//     MFMAs of k-half 0, those of the next K-tile's k-half 0 on the MFMAs of k-half 1; the
//     waits are the compiler's lgkmcnt on the registers each MFMA takes: counted, except one
//     lgkmcnt(0) per K-tile before MFMA 8 of k-half 1, which takes the youngest fragment (read
//     about 16 MFMAs earlier; nothing younger is outstanding, so no count below it exists);
//   * three 48 KiB LDS buffers ([X 256 rows][W 128 rows] of 128 B), filled by 1 KiB LDS-DMA
//     pieces (8 rows x 128 B, 8 X + 4 W per wave per K-tile) issued TWO K-tiles ahead between
//     the MFMAs, about one per 5; counted vmcnt, never drained in the steady loop;
//   * ONE barrier per K-tile, in k-half 1 after its first 11 MFMAs have taken every fragment
//     register of the K-tile (a column of 8 + the 3 other W fragments): behind it every wave is
//     done reading this K-tile's buffer (free for the pieces of K-tile t + 3) and, by the
//     vmcnt before it, every wave's pieces of K-tile t + 1 have landed;
//   * weights stream with the non-temporal policy, X (L2-resident) with the default one;
//   * operands swapped in the MFMA (A = W) as in gemm_pp: a lane holds 4 consecutive features
//     of one token -- 16-B fp32 slab stores, 8-B bf16 stores, and the fused SwiGLU of the
//     64-row interleaved gate|up weight in registers (wave wn owns gate rows 32 wn .. and up
//     rows 64 + 32 wn .. of the 128-row tile);
//   * split-K by gemm_tn's rule: slice kz = K-steps [kz TK / S, (kz + 1) TK / S), fp32 slabs
//     P[S][256][N] summed by the consumer; block = nt * S + kz, so with S = 8 an XCD (block
//     id mod 8) sees one K slice of X only.
// Every accumulator takes its K range in ascending 32-wide MFMA steps from zero, as in
// gemm_tn / gemm_pp: the outputs are bitwise equal to theirs (tests/test_gemm_w4_gpu.py).
// LDS image: lane-linear DMA rows with the chunk ^ ((row >> 1) & 7) swizzle on the source and
// the read, fragment rows = 16-aligned base + lane % 16 as in gemm_pp (conflict-free
// ds_read_b128; SQ_LDS_BANK_CONFLICT = 0 in the profile above).
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace oamd {

namespace {

constexpr int kM = 256;          // tokens per tile = the decode bucket
constexpr int kBK = 64;
constexpr int kXBytes = 32768;   // X of a K-tile: 256 rows x 128 B
constexpr int kBuf = 49152;      // + W: 128 rows x 128 B
constexpr int kPre = 9;          // pieces of K-tile t + 2 issued before K-tile t's vmcnt

enum { kStore = 0, kPartial = 1, kSilu = 2 };
enum { kSteady = 0, kPenult = 1, kLast = 2 };

template <int N>
__device__ __forceinline__ void vmw() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void seg() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void mfma_tied(f32x4& acc, const u16x8& a, const u16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}

__device__ __forceinline__ uint2 pack4(f32x4 v) { return make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])); }

}  // namespace

template <int EPI>
__global__ void __launch_bounds__(256) gemm_w4_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                                                      bf16_t* __restrict__ Y, float* __restrict__ P, int N, int K,
                                                      int S) {
  __shared__ __attribute__((aligned(1024))) char lds[3 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int kz = blockIdx.x % S, n0 = (blockIdx.x / S) * 128;
  const int TK = K / kBK;
  const int t0 = kz * TK / S;
  const int T = (kz + 1) * TK / S - t0;   // >= 1 (host: S <= TK)

  // DMA piece q of an operand for wave w = rows 8 (w + 4q) .. +7 (X: q < 8, W: q < 4); lane l ->
  // row + l / 8, LDS slot l % 8, source chunk slot ^ ((row >> 1) & 7). Both operands are K wide:
  // one set of byte offsets into per-operand buffer resources (base = the tile's first row)
  const int lrow = lane >> 3, lslot = lane & 7;
  uint32_t vo[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int row = 8 * (w + 4 * q) + lrow;
    vo[q] = ((uint32_t)row * (uint32_t)K + (uint32_t)((lslot ^ ((row >> 1) & 7)) * 8)) * 2u;
  }
  const bf16_t* wbase = W + (int64_t)n0 * K;
  const int xbytes = kM * K * 2, wbytes = 128 * K * 2;
  // piece p of K-step kt into the buffer at byte `off`: the 4 W pieces (HBM) first, then X's
  // (scalar parameters: see the note at gemm_tile.hip's dma_ on dropped launch stubs)
  auto dma_x = [&](const bf16_t* b, int nb, int off, int kt, int q) {
    char* dst = lds + off + (w + 4 * q) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc((void*)b, (short)0, nb, 0x00020000),
                                             (__attribute__((address_space(3))) void*)dst, 16, (int)vo[q],
                                             (t0 + kt) * (kBK * 2), 0, 0);
  };
  auto dma_w = [&](const bf16_t* b, int nb, int off, int kt, int q) {
    char* dst = lds + off + kXBytes + (w + 4 * q) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc((void*)b, (short)0, nb, 0x00020000),
                                             (__attribute__((address_space(3))) void*)dst, 16, (int)vo[q],
                                             (t0 + kt) * (kBK * 2), 0, 2);
  };
  auto piece = [&](int off, int kt, int p) {
    if (p < 4) dma_w(wbase, wbytes, off, kt, p);
    else dma_x(X, xbytes, off, kt, p - 4);
  };

  // fragments: X fragment i = rows wm*128 + 16 i + l15; W fragment j (e = j / 2: gate / up half,
  // jj = j % 2) = rows 64 e + 32 wn + 16 jj + l15; k-half h reads chunk 4h + lane / 16
  const int l15 = lane & 15, lq = lane >> 4, sw = (l15 >> 1) & 7;
  const int xo0 = (wm * 128 + l15) * 128 + ((lq ^ sw) << 4);
  const int xo1 = (wm * 128 + l15) * 128 + (((4 + lq) ^ sw) << 4);
  const int wo0 = kXBytes + (wn * 32 + l15) * 128 + ((lq ^ sw) << 4);
  const int wo1 = kXBytes + (wn * 32 + l15) * 128 + (((4 + lq) ^ sw) << 4);
  // read r of a k-half: 0-3 = W fragment r, 4-11 = X fragment r - 4
  auto rd = [&](int off, int h, u16x8 (&xf)[8], u16x8 (&wf)[4], int r) {
    const int wrow = (r >> 1) * 64 + (r & 1) * 16;
    if (r < 4) wf[r] = *reinterpret_cast<const u16x8*>(lds + off + (h ? wo1 : wo0) + wrow * 128);
    else xf[r - 4] = *reinterpret_cast<const u16x8*>(lds + off + (h ? xo1 : xo0) + (r - 4) * 2048);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));
  asm volatile("s_nop 4");
  u16x8 xa[8], wa[4], xb[8], wb[4];

  // One K-tile: buffer `cur` (its k-half 0 in xa / wa), the next K-tile's buffer `nxt`, and `tgt`
  // (the previous K-tile's buffer) for the pieces of K-step kt2 = t + 2.
  //   k-half 0: 32 MFMAs in rows (X fragment m / 4); the 12 reads of k-half 1 after every second
  //     of the first 24; pieces 0-5 after MFMAs 3, 8, .. 28.
  //   k-half 1: MFMAs (m, 0) for m < 8, (0, 1..3), then rows 1-7 of columns 1-3; pieces 6-8 after
  //     MFMAs 1, 6, 11; vmcnt(kPre) + barrier; the 12 reads of the next k-half 0 after MFMAs
  //     12-23; pieces 9-11 after MFMAs 25, 28, 31.
  // kPenult / kLast (the last two K-tiles) issue nothing; kLast has no successor to wait for.
  // The K-tile is written as two halves, head (up to the barrier) and tail, so that the loop below
  // can turn around AT the barrier, where no fragment read is outstanding: every lgkmcnt hipcc
  // emits inside the loop is then counted (a loop that turns around before k-half 0 starts with
  // lgkmcnt(0) on reads issued 8 MFMAs earlier).
  auto mm_b = [&](int m) {
    const int i = m < 8 ? m : (m < 11 ? 0 : 1 + (m - 11) / 3);
    const int j = m < 8 ? 0 : (m < 11 ? m - 7 : 1 + (m - 11) % 3);
    mfma_tied(acc[i][j], wb[j], xb[i]);
  };
  auto head = [&](auto mode_c, int cur, int tgt, int kt2) {
    constexpr int MODE = decltype(mode_c)::value;
#pragma unroll
    for (int m = 0; m < 32; ++m) {
      mfma_tied(acc[m >> 2][m & 3], wa[m & 3], xa[m >> 2]);
      __builtin_amdgcn_sched_barrier(0);
      if (m < 24 && m % 2 == 0) rd(cur, 1, xb, wb, m >> 1);
      if (MODE == kSteady && m % 5 == 3) piece(tgt, kt2, m / 5);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int m = 0; m < 12; ++m) {
      mm_b(m);
      __builtin_amdgcn_sched_barrier(0);
      if (MODE == kSteady && m % 5 == 1) piece(tgt, kt2, 6 + m / 5);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (MODE != kLast) {
      if constexpr (MODE == kSteady) vmw<kPre>(); else vmw<0>();
      seg();
    }
  };
  auto tail = [&](auto mode_c, int nxt, int tgt, int kt2) {
    constexpr int MODE = decltype(mode_c)::value;
#pragma unroll
    for (int m = 12; m < 32; ++m) {
      mm_b(m);
      __builtin_amdgcn_sched_barrier(0);
      if (MODE != kLast && m < 24) {
        // the order k-half 0 takes them: W 0, X 0, W 1-3, X 1-7
        const int k = m - 12;
        rd(nxt, 0, xa, wa, k == 0 ? 0 : (k == 1 ? 4 : (k < 5 ? k - 1 : k)));
      }
      if (MODE == kSteady && m >= 25 && (m - 25) % 3 == 0) piece(tgt, kt2, 9 + (m - 25) / 3);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // prologue: K-tiles 0 and 1 in flight, tile 0 landed for every wave, its k-half 0 in registers
#pragma unroll
  for (int p = 0; p < 12; ++p) piece(0, 0, p);
  if (T > 1) {
#pragma unroll
    for (int p = 0; p < 12; ++p) piece(kBuf, 1, p);
    vmw<12>();
  } else {
    vmw<0>();
  }
  seg();
#pragma unroll
  for (int k = 0; k < 12; ++k) rd(0, 0, xa, wa, k == 0 ? 0 : (k == 1 ? 4 : (k < 5 ? k - 1 : k)));

  int cur = 0, nxt = kBuf, tgt = 2 * kBuf;
  auto rotate = [&]() {
    const int c = cur;
    cur = nxt;
    nxt = tgt;
    tgt = c;
  };
  constexpr std::integral_constant<int, kSteady> steady{};
  constexpr std::integral_constant<int, kPenult> penult{};
  constexpr std::integral_constant<int, kLast> last{};
  if (T > 2) {   // K-tiles 0 .. T - 3 issue the pieces of tiles 2 .. T - 1
    head(steady, cur, tgt, 2);
    for (int t = 0; t + 3 < T; ++t) {
      tail(steady, nxt, tgt, t + 2);
      rotate();
      head(steady, cur, tgt, t + 3);
    }
    tail(steady, nxt, tgt, T - 1);
    rotate();
  }
  if (T > 1) {
    head(penult, cur, tgt, 0);
    tail(penult, nxt, tgt, 0);
    rotate();
  }
  head(last, cur, tgt, 0);
  tail(last, nxt, tgt, 0);

  // ---- epilogue: lane holds features 4 lq .. 4 lq + 3 of W fragment j for token l15 of X fragment i
  asm volatile("s_nop 7\n s_nop 7\n s_nop 7" ::: "memory");
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int tok = wm * 128 + i * 16 + l15;
    if constexpr (EPI == kSilu) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const f32x4 gt = acc[i][jj], up = acc[i][2 + jj];
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gg = bf2f(f2bf(gt[r]));
          const float uu = bf2f(f2bf(up[r]));
          o[r] = bf2f(f2bf(gg / (1.f + __expf(-gg)))) * uu;
        }
        const int col = (n0 >> 1) + wn * 32 + jj * 16 + 4 * lq;
        *reinterpret_cast<uint2*>(Y + (int64_t)tok * (N >> 1) + col) = pack4(o);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = n0 + (j >> 1) * 64 + wn * 32 + (j & 1) * 16 + 4 * lq;
        if constexpr (EPI == kPartial)
          *reinterpret_cast<f32x4*>(P + ((int64_t)kz * kM + tok) * N + col) = acc[i][j];
        else
          *reinterpret_cast<uint2*>(Y + (int64_t)tok * N + col) = pack4(acc[i][j]);
      }
    }
  }
}

int gemm_w4(const bf16_t* X, const bf16_t* W, bf16_t* Y, float* P, int M, int N, int K, int S, bool silu_gu,
            hipStream_t stream) {
  if (M != kM || N < 128 || N % 128 != 0 || K < kBK || K % kBK != 0) return -1;
  if ((int64_t)kM * K * 2 >= (1LL << 31)) return -2;   // 32-bit buffer offsets
  if (S < 1 || S > 16 || K / kBK < S) return -3;
  if (S > 1 && P == nullptr) return -4;
  if (silu_gu && S != 1) return -5;
  if (S == 1 && Y == nullptr) return -6;
  const int grid = (N / 128) * S;
  if (silu_gu) gemm_w4_kernel<kSilu><<<grid, 256, 0, stream>>>(X, W, Y, P, N, K, S);
  else if (S > 1) gemm_w4_kernel<kPartial><<<grid, 256, 0, stream>>>(X, W, Y, P, N, K, S);
  else gemm_w4_kernel<kStore><<<grid, 256, 0, stream>>>(X, W, Y, P, N, K, S);
  OAMD_LAUNCH_CHECK();
  if (S > 1 && Y != nullptr) return splitk_reduce(P, Y, (int64_t)M * N, S, stream);
  return 0;
}

}  // namespace oamd
