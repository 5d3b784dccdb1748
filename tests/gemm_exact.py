"""Exactly computable references for the GEMM kernels (tests/test_gemm_exact_gpu.py; checked on
the CPU by tests/test_gemm_exact_ref.py).

Operands are integers in [-15, 15]: exact in bf16 and in e4m3, every product and every partial
sum up to K = MAX_K an integer below 2^24, so an fp32 accumulator is exact in ANY summation
order and a kernel has exactly one right answer. The reference is the float64 product; an fp32
split-K slab must equal its K slice of it bit for bit, a bf16 output its single
round-to-nearest-even rounding. Everything here runs on the CPU and reads no kernel."""
import functools

import torch

LO, HI = -15, 15
MAX_K = 16384   # 225 * 16384 < 2^22: partial sums stay far inside fp32's exact integers
GUARD = 32      # NaN guard rows on each side of an output
TAIL = 4096     # NaN floats after the last split-K slab

# ---- the cases: (K-steps, splits) per kernel; the step is 64 columns unless noted ----
DECODE_T = (1, 2, 5, 7, 13)                 # below the prologue depth, at it, steady loop and drain of a 6-deep ring
DECODE_TS = ((13, 2), (13, 3), (13, 5), (13, 13), (16, 16))   # even / uneven slices, one step per slice
DECODE_CFGS = tuple((bm, bn, ns) for bm in (64, 128, 256) for bn in (64, 128) for ns in (2, 3, 4, 5, 6)
                    if ns == 3 or (ns == 2 and bm <= 128) or (ns == 4 and bm + bn <= 320)
                    or (ns == 5 and bm + bn <= 256) or (ns == 6 and bm + bn <= 192))
DECODE_SILU_CFGS = ((64, 2), (64, 3), (64, 4), (128, 3), (128, 4), (256, 3))
SKINNY_M = (1, 15, 16, 17, 31, 32)
SKINNY_K = (128, 896, 1024, 1152, 2176)     # per-wave 32-deep steps K / 128 = 1, 7, 8, 9, 17
SKINNY_S = (2, 4, 8)                        # K = 128 S 9
PP_M = (1, 127, 128, 129, 255, 256, 257, 300)
PP_T = (1, 2, 3, 4, 7)
PP_TS = ((8, 2), (7, 7), (32, 32))         # gemm_pp needs K % (64 S) == 0: S = 2 at K = 512, not at K = 448
PP_CFGS = ((128, True, False), (128, False, False), (256, True, False), (256, False, False), (256, True, True),
           (256, False, True))              # (bm, nt, one_seg)
W4_T = (1, 2, 3, 4, 7, 13)
W4_TS = ((13, 3), (13, 13), (16, 16))
W4_SILU_T = (1, 3, 7)
FP8_M = (1, 63, 64, 65, 200, 256, 300)
FP8_T = (1, 2, 3, 4, 7)                     # 128-column steps
FP8_S = (1, 2, 3, 7)
TILE_M = (1, 255, 256, 257, 513)
TILE_N = (16, 272, 512)
TILE_K = (64, 128, 192, 448)
TILE_KS = ((128, 2), (256, 2), (256, 4), (512, 2), (512, 4))   # split-K needs K % (64 S) == 0: K = 256, 512 added
TILE_STRIDED_M = (257, 513)
TILE_STRIDED_K = (128, 192)

ALL_K = tuple(sorted({64 * t for t in DECODE_T + W4_T + PP_T} | {64 * t for t, _ in DECODE_TS + PP_TS + W4_TS}
                     | set(SKINNY_K) | {128 * s * 9 for s in SKINNY_S} | {128 * t for t in FP8_T} | set(TILE_K)
                     | {k for k, _ in TILE_KS}))


def ints(rows: int, cols: int, seed: int, lo: int = LO, hi: int = HI) -> torch.Tensor:
    """[rows, cols] integers uniform in [lo, hi] as float64, from a seeded CPU generator."""
    assert lo >= LO and hi <= HI and cols <= MAX_K
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, (rows, cols), generator=g).double()


def product(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x @ w^T in float64 (+0.0 for every zero)."""
    assert x.dtype == torch.float64 and w.dtype == torch.float64
    return x @ w.t() + 0.0


def even_slices(K: int, S: int, step: int) -> list[tuple[int, int]]:
    """Slice kz = steps [kz TK // S, (kz + 1) TK // S) of TK = K / step (gemm_decode, gemm_w4: step 64;
    gemm_fp8: 128): uneven by at most one step where S does not divide TK."""
    assert K % step == 0 and 1 <= S <= K // step
    TK = K // step
    return [(kz * TK // S * step, (kz + 1) * TK // S * step) for kz in range(S)]


def equal_slices(K: int, S: int) -> list[tuple[int, int]]:
    """Slice kz = columns [kz K / S, (kz + 1) K / S) (gemm_pp, gemm_skinny, gemm_tile)."""
    assert K % S == 0
    return [(kz * (K // S), (kz + 1) * (K // S)) for kz in range(S)]


def slabs(x: torch.Tensor, w: torch.Tensor, slices) -> torch.Tensor:
    """[S, M, N] float64: slab kz = x[:, a:b] @ w[:, a:b]^T of its K slice."""
    return torch.stack([product(x[:, a:b].contiguous(), w[:, a:b].contiguous()) for a, b in slices])


def f32_bits(r: torch.Tensor) -> torch.Tensor:
    """The int32 image of r (float64, exactly representable in fp32)."""
    f = r.float()
    assert torch.equal(f.double(), r), "reference not exact in fp32"
    return f.contiguous().view(torch.int32)


def bf16_bits(r: torch.Tensor) -> torch.Tensor:
    """The int16 image of r rounded ONCE to bf16, round-to-nearest-even, from the fp32 bit pattern
    (r is exact in fp32, finite): add 0x7fff + the kept lsb, drop the low 16 bits."""
    b = f32_bits(r).long() & 0xFFFFFFFF
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return (b - ((b & 0x8000) << 1)).to(torch.int16)   # the unsigned 16 bits as int16


def bf16_round(r: torch.Tensor) -> torch.Tensor:
    """r rounded once to bf16, as float64."""
    return bf16_bits(r).view(torch.bfloat16).double()


def swiglu(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """bf16(bf16(g) * bf16(u)) as int16 bits, for gate sums g >= 64: 1 + exp(-g) is 1 in fp32, so
    sigmoid(g) is exactly 1 and silu(bf16 g) = bf16 g. The product of two bf16 values is exact in fp32."""
    assert g.min().item() >= 64
    return bf16_bits(bf16_round(g) * bf16_round(u))


def interleave(g: torch.Tensor, u: torch.Tensor, block: int = 64) -> torch.Tensor:
    """[g; u] weight rows -> blocks of 64 gate rows followed by the same features' up rows."""
    inter, K = g.shape
    return torch.stack([g.reshape(inter // block, block, K), u.reshape(inter // block, block, K)], 1).reshape(
        2 * inter, K).contiguous()


def tile_w(w: torch.Tensor) -> torch.Tensor:
    """Row-major [N, K] -> the [N/64][K/64][64][64] layout gemm_decode(w_tiled=True) reads, kept as [N, K]."""
    N, K = w.shape
    return w.view(N // 64, 64, K // 64, 64).permute(0, 2, 1, 3).contiguous().view(N, K)


def untile_w(wt: torch.Tensor) -> torch.Tensor:
    N, K = wt.shape
    return wt.view(N // 64, K // 64, 64, 64).permute(0, 2, 1, 3).contiguous().view(N, K)


def fp8_scales(M: int, N: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Power-of-two scales sx[m] = 2^-(m % 4), sw[n] = 2^-(n % 3) (float64): acc * sx * sw is exact."""
    return (0.5 ** (torch.arange(M) % 4).double(), 0.5 ** (torch.arange(N) % 3).double())


def rounding_share(r: torch.Tensor) -> tuple[float, float]:
    """(share of outputs that differ between truncation and round-to-nearest-even, share that
    are exact ties) of rounding r to bf16."""
    b = f32_bits(r).long() & 0xFFFF
    odd = (f32_bits(r).long() >> 16) & 1
    differ = (b > 0x8000) | ((b == 0x8000) & (odd == 1))
    return differ.double().mean().item(), (b == 0x8000).double().mean().item()


@functools.lru_cache(maxsize=None)
def rounding_share_at(K: int) -> tuple[float, float]:
    return rounding_share(product(ints(256, K, 1000 + K), ints(256, K, 2000 + K)))


def assert_rounding_is_exercised(Ks=ALL_K) -> None:
    """On the reference alone: at M = N = 256, at least 20 % of the outputs change under truncation
    (so they need rounding) and at least 4 % are exact ties, at every K the tests use."""
    for K in Ks:
        differ, ties = rounding_share_at(K)
        assert differ >= 0.20 and ties >= 0.04, f"K={K}: {differ:.3f} need rounding, {ties:.3f} ties"
