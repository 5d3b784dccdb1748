"""Every decode GEMM kernel (gemm_decode, gemm_skinny, gemm_pp, gemm_w4, gemm_fp8) and gemm_tile,
bit for bit against an exactly computable reference (tests/gemm_exact.py): integer operands in
[-15, 15], whose fp32 accumulation is exact in any order, so each fp32 split-K slab must equal the
float64 product of its own K slice (int32 views) and each bf16 output its single
round-to-nearest-even rounding (int16 views). A truncating or double-rounding store, a slab that
holds another slice's steps, a swapped fragment or a skipped rounding point in a SwiGLU epilogue
each change bits here that atol = 2e-2 on random data does not see.

Every y is the middle M rows of a NaN-filled [M + 64, N] buffer and every slab buffer ends in a
4096-float NaN tail: a store the kernel skips leaves a NaN in the result, a store past row M - 1 or
past the last slab removes one from the guards. The parametrize lists follow the launchers'
instantiation tables (gemm.hip OAMD_GEMM2, gemm_skinny.hip MT / EPI, gemm_pp.hip OAMD_PP_E /
OAMD_PP1, gemm_fp8.hip OAMD_G8M, gemm_tile.hip variants 0-14), so every compiled instantiation is
launched at least once. The shape of SiLU itself stays with the random-data tests; stream-K gemm_pp
with test_kernels_gpu.py::test_gate_up_silu_stream_k."""
import functools

import pytest
import torch

import gemm_exact as gx
from operator_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
G = gx.GUARD


@pytest.fixture(scope="module", autouse=True)
def _reference_exercises_rounding():
    gx.assert_rounding_is_exercised()   # on the reference alone, before any kernel runs


def _bf(t):
    return t.to(DEV, torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _plain(M, N, K):
    """x [M, K], w [N, K] on the GPU, the float64 product on the CPU."""
    x, w = gx.ints(M, K, 11 * K + M), gx.ints(N, K, 13 * K + N + 1)
    return x, w, _bf(x), _bf(w)


@functools.lru_cache(maxsize=None)
def _want_y(M, N, K):
    x, w, _, _ = _plain(M, N, K)
    return gx.bf16_bits(gx.product(x, w)).to(DEV)


@functools.lru_cache(maxsize=None)
def _want_slabs(M, N, K, S, step):
    """int32 bits of the S slab references; step 0: equal K / S slices."""
    x, w, _, _ = _plain(M, N, K)
    sl = gx.equal_slices(K, S) if step == 0 else gx.even_slices(K, S, step)
    return gx.f32_bits(gx.slabs(x, w, sl)).to(DEV)


@functools.lru_cache(maxsize=None)
def _silu(M, inter, K):
    """x and gate rows in [1, 15] (every gate sum >= 64: sigmoid is exactly 1), up rows in [-15, 15]:
    (x, interleaved gate|up weight) on the GPU, bits of bf16(bf16(g) * bf16(u))."""
    x, g, u = gx.ints(M, K, 17 * K + M, 1, 15), gx.ints(inter, K, 19 * K + inter, 1, 15), gx.ints(inter, K, 23 * K + inter)
    return _bf(x), _bf(gx.interleave(g, u)), gx.swiglu(gx.product(x, g), gx.product(x, u)).to(DEV)


def _y(M, N):
    """(buffer, y): y = the middle M rows of a NaN-filled [M + 64, N] buffer."""
    buf = torch.full((M + 2 * G, N), NAN, dtype=torch.bfloat16, device=DEV)
    return buf, buf[G:G + M]


def _p(S, M, N):
    return torch.full((S * M * N + gx.TAIL,), NAN, dtype=torch.float32, device=DEV)


def _check_y(buf, want, what):
    M = want.shape[0]
    torch.cuda.synchronize()
    y = buf[G:G + M]
    assert not torch.isnan(y).any(), f"{what}: NaN left in y"
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + M:]).all(), f"{what}: guard rows written"
    bad = (y.view(torch.int16) != want).sum().item()
    assert bad == 0, f"{what}: {bad} of {want.numel()} bf16 outputs differ from the rounded float64 product"


def _check_p(p, want, what):
    S, M, N = want.shape
    torch.cuda.synchronize()
    got = p[:S * M * N].view(S, M, N)
    assert not torch.isnan(got).any(), f"{what}: NaN left in the slabs"
    assert torch.isnan(p[S * M * N:]).all(), f"{what}: the tail after the last slab was written"
    for s in range(S):
        bad = (got[s].view(torch.int32) != want[s]).sum().item()
        assert bad == 0, f"{what}: slab {s}: {bad} of {M * N} differ from its K slice"


def _slabs_then_y(launch, S, M, N, want_p, want_y, what):
    """A split-K launch twice: slabs left to the consumer (no y), then reduced into y by the launcher."""
    p = _p(S, M, N)
    launch(None, p)
    _check_p(p, want_p, f"{what} deferred")
    p, (buf, y) = _p(S, M, N), _y(M, N)
    launch(y, p)
    _check_p(p, want_p, f"{what} reduced")
    _check_y(buf, want_y, f"{what} reduced")


# ---------------------------------------------------------------- gemm_decode

@pytest.mark.parametrize("bm,bn,stages", gx.DECODE_CFGS)
def test_gemm_decode_store_and_slabs(bm, bn, stages):
    M = N = 256   # four row tiles at bm 64, four column tiles at bn 64
    C = ops.kernels()
    for T in gx.DECODE_T:
        K = 64 * T
        _, _, x, w = _plain(M, N, K)
        buf, y = _y(M, N)
        C.gemm_decode(x, w, y, None, 1, bn, bm, False, False, stages)
        _check_y(buf, _want_y(M, N, K), f"T={T}")
    for T, S in gx.DECODE_TS:
        K = 64 * T
        _, _, x, w = _plain(M, N, K)
        _slabs_then_y(lambda y, p: C.gemm_decode(x, w, y, p, S, bn, bm, False, False, stages), S, M, N,
                      _want_slabs(M, N, K, S, 64), _want_y(M, N, K), f"T={T} S={S}")


def test_gemm_decode_three_row_tiles():
    M, N, K, C = 192, 256, 320, ops.kernels()
    _, _, x, w = _plain(M, N, K)
    buf, y = _y(M, N)
    C.gemm_decode(x, w, y, None, 1, 64, 64, False, False, 3)
    _check_y(buf, _want_y(M, N, K), "store")
    _slabs_then_y(lambda y, p: C.gemm_decode(x, w, y, p, 2, 64, 64, False, False, 3), 2, M, N,
                  _want_slabs(M, N, K, 2, 64), _want_y(M, N, K), "S=2")


@pytest.mark.parametrize("bm,stages", gx.DECODE_SILU_CFGS)
def test_gemm_decode_swiglu(bm, stages):
    M, inter = 256, 128   # N = 256: two tiles of 64 gate + 64 up rows
    for T in gx.DECODE_T:
        x, wgu, want = _silu(M, inter, 64 * T)
        buf, y = _y(M, inter)
        ops.kernels().gemm_decode(x, wgu, y, None, 1, 128, bm, True, False, stages)
        _check_y(buf, want, f"T={T}")


def test_gemm_decode_tiled_weight():
    """w_tiled=True reads W as [N/64][K/64][64][64]: store, slabs and SwiGLU, one ring depth each."""
    M, N, K, C = 256, 256, 448, ops.kernels()
    _, w64, x, _ = _plain(M, N, K)
    wt = _bf(gx.tile_w(w64))
    assert not torch.equal(wt, _bf(w64))
    buf, y = _y(M, N)
    C.gemm_decode(x, wt, y, None, 1, 64, 128, False, True, 4)
    _check_y(buf, _want_y(M, N, K), "store")
    _slabs_then_y(lambda y, p: C.gemm_decode(x, wt, y, p, 3, 128, 64, False, True, 5), 3, M, N,
                  _want_slabs(M, N, K, 3, 64), _want_y(M, N, K), "S=3")
    xs, wgu, want = _silu(M, 128, K)
    buf, y = _y(M, 128)
    C.gemm_decode(xs, _bf(gx.tile_w(wgu.double().cpu())), y, None, 1, 128, 256, True, True, 3)
    _check_y(buf, want, "swiglu")


# ---------------------------------------------------------------- gemm_skinny

@pytest.mark.parametrize("M", gx.SKINNY_M)
def test_gemm_skinny(M):
    """Both MT variants (M <= 16, M <= 32) and their padded MFMA columns; per-wave step counts that run
    the remainder loop only, the 8-step main loop only, and both."""
    N, C = 48, ops.kernels()   # three blocks
    for K in gx.SKINNY_K:
        _, _, x, w = _plain(M, N, K)
        buf, y = _y(M, N)
        C.gemm_skinny(x, w, y, None, 1, False)
        _check_y(buf, _want_y(M, N, K), f"K={K}")
    for S in gx.SKINNY_S:
        K = 128 * S * 9
        _, _, x, w = _plain(M, N, K)
        _slabs_then_y(lambda y, p: C.gemm_skinny(x, w, y, p, S, False), S, M, N, _want_slabs(M, N, K, S, 0),
                      _want_y(M, N, K), f"S={S}")
    for K in gx.SKINNY_K:
        x, wgu, want = _silu(M, 128, K)   # N = 256: two gate|up groups x four 16-row sub-blocks
        buf, y = _y(M, 128)
        C.gemm_skinny(x, wgu, y, None, 1, True)
        _check_y(buf, want, f"swiglu K={K}")


# ---------------------------------------------------------------- gemm_pp

@pytest.mark.parametrize("M", gx.PP_M)
@pytest.mark.parametrize("bm,nt,one_seg", gx.PP_CFGS)
def test_gemm_pp(bm, nt, one_seg, M):
    """Rows clamped on load and skipped on store (M % bm != 0), up to three row tiles (gridDim.z)."""
    N, C = 256, ops.kernels()
    for T in gx.PP_T:
        K = 64 * T
        _, _, x, w = _plain(M, N, K)
        buf, y = _y(M, N)
        C.gemm_pp(x, w, y, None, 1, bm, False, nt, one_seg)
        _check_y(buf, _want_y(M, N, K), f"T={T}")
        xs, wgu, want = _silu(M, 128, K)
        buf, y = _y(M, 128)
        C.gemm_pp(xs, wgu, y, None, 1, bm, True, nt, one_seg)
        _check_y(buf, want, f"swiglu T={T}")
    for T, S in gx.PP_TS:
        K = 64 * T
        _, _, x, w = _plain(M, N, K)
        _slabs_then_y(lambda y, p: C.gemm_pp(x, w, y, p, S, bm, False, nt, one_seg), S, M, N,
                      _want_slabs(M, N, K, S, 0), _want_y(M, N, K), f"T={T} S={S}")


# ---------------------------------------------------------------- gemm_w4

@pytest.mark.parametrize("N", [128, 256])
def test_gemm_w4(N):
    M, C = 256, ops.kernels()
    for T in gx.W4_T:
        K = 64 * T
        _, _, x, w = _plain(M, N, K)
        buf, y = _y(M, N)
        C.gemm_w4(x, w, y, None, 1, False)
        _check_y(buf, _want_y(M, N, K), f"T={T}")
    for T, S in gx.W4_TS:
        K = 64 * T
        _, _, x, w = _plain(M, N, K)
        _slabs_then_y(lambda y, p: C.gemm_w4(x, w, y, p, S, False), S, M, N, _want_slabs(M, N, K, S, 64),
                      _want_y(M, N, K), f"T={T} S={S}")
    for T in gx.W4_SILU_T:
        x, wgu, want = _silu(M, N // 2, 64 * T)
        buf, y = _y(M, N // 2)
        C.gemm_w4(x, wgu, y, None, 1, True)
        _check_y(buf, want, f"swiglu T={T}")


# ---------------------------------------------------------------- gemm_fp8

@functools.lru_cache(maxsize=None)
def _fp8(M, N, K):
    """e4m3 operands straight from the integers (no quantize_fp8), power-of-two scales."""
    x, w, _, _ = _plain(M, N, K)
    sx, sw = gx.fp8_scales(M, N)
    x8, w8 = x.float().to(torch.float8_e4m3fn), w.float().to(torch.float8_e4m3fn)
    assert torch.equal(x8.double(), x) and torch.equal(w8.double(), w)
    return x8.to(DEV), w8.to(DEV), sx.float().to(DEV), sw.float().to(DEV)


@functools.lru_cache(maxsize=None)
def _fp8_want(M, N, K, S):
    x, w, _, _ = _plain(M, N, K)
    sx, sw = gx.fp8_scales(M, N)
    scale = sx[:, None] * sw[None, :]
    return (gx.f32_bits(gx.slabs(x, w, gx.even_slices(K, S, 128)) * scale).to(DEV),
            gx.bf16_bits(gx.product(x, w) * scale).to(DEV))


@pytest.mark.parametrize("M", gx.FP8_M)
@pytest.mark.parametrize("bm,bn", [(bm, bn) for bm in (64, 128, 256) for bn in (64, 128)])
def test_gemm_fp8(bm, bn, M):
    N, C = 256, ops.kernels()
    for T in gx.FP8_T:
        K = 128 * T
        x8, w8, sx, sw = _fp8(M, N, K)
        for S in gx.FP8_S:
            if S > T:
                continue
            want_p, want_y = _fp8_want(M, N, K, S)
            p, (buf, y) = (_p(S, M, N) if S > 1 else None), _y(M, N)
            C.gemm_fp8(x8, w8, sx, sw, y, p, S, bn, bm, True)
            _check_y(buf, want_y, f"T={T} S={S}")
            if S > 1:
                _check_p(p, want_p, f"T={T} S={S}")
            p, (buf, y) = (_p(S, M, N) if S > 1 else None), _y(M, N)
            C.gemm_fp8(x8, w8, sx, sw, y, p, S, bn, bm, False)   # reduce=False: the slabs only
            if S > 1:
                _check_p(p, want_p, f"T={T} S={S} reduce=False")
                torch.cuda.synchronize()
                assert torch.isnan(buf).all(), f"T={T} S={S} reduce=False wrote y"
            else:
                _check_y(buf, want_y, f"T={T} S=1 reduce=False")


# ---------------------------------------------------------------- gemm_tile

TILE_VARIANTS = tuple(range(15))   # 5-14 (persistent p5 and its arms) need K >= 128


@functools.lru_cache(maxsize=None)
def _bias(M, N, K):
    x, w, _, _ = _plain(M, N, K)
    b = gx.ints(1, N, 29 * N + K)[0]
    return _bf(b), gx.bf16_bits(gx.product(x, w) + b).to(DEV)


@pytest.mark.parametrize("N", gx.TILE_N)
@pytest.mark.parametrize("M", gx.TILE_M)
def test_gemm_tile_every_variant(M, N):
    C = ops.kernels()
    for K in gx.TILE_K:
        _, _, x, w = _plain(M, N, K)
        b, want_b = _bias(M, N, K)
        for v in (TILE_VARIANTS if K >= 128 else TILE_VARIANTS[:5]):
            buf, y = _y(M, N)
            C.gemm_tile(x, w, y, None, False, v)
            _check_y(buf, _want_y(M, N, K), f"K={K} variant {v}")
            buf, y = _y(M, N)
            C.gemm_tile(x, w, y, b, False, v)
            _check_y(buf, want_b, f"K={K} variant {v} bias")
            if N % 128 == 0:
                xs, wgu, want = _silu(M, N // 2, K)
                buf, y = _y(M, N // 2)
                C.gemm_tile(xs, wgu, y, None, True, v)
                _check_y(buf, want, f"K={K} variant {v} swiglu")


@pytest.mark.parametrize("N", gx.TILE_N)
@pytest.mark.parametrize("M", gx.TILE_M)
def test_gemm_tile_split_k(M, N):
    C = ops.kernels()
    for K, S in gx.TILE_KS:
        _, _, x, w = _plain(M, N, K)
        _slabs_then_y(lambda y, p: C.gemm_tile(x, w, y, None, False, 0, S, p), S, M, N, _want_slabs(M, N, K, S, 0),
                      _want_y(M, N, K), f"K={K} S={S}")


@pytest.mark.parametrize("pad", [64, 68])   # row stride N + 68 is no multiple of 8: p5 declines, the fallback runs
@pytest.mark.parametrize("N", gx.TILE_N)
@pytest.mark.parametrize("M", gx.TILE_STRIDED_M)
def test_gemm_tile_strided_output(M, N, pad):
    """y = buf[32:32 + M, 32:32 + N] of a NaN buffer (M > 256 reaches the persistent p5 path): everything
    outside the slice stays NaN."""
    C = ops.kernels()
    for K in gx.TILE_STRIDED_K:
        _, _, x, w = _plain(M, N, K)
        want = _want_y(M, N, K)
        for v in TILE_VARIANTS:
            buf = torch.full((M + 2 * G, N + pad), NAN, dtype=torch.bfloat16, device=DEV)
            y = buf[G:G + M, 32:32 + N]
            C.gemm_tile(x, w, y, None, False, v)
            torch.cuda.synchronize()
            assert not torch.isnan(y).any(), f"K={K} variant {v}: NaN left in y"
            assert (y.contiguous().view(torch.int16) == want).all(), f"K={K} variant {v}"
            outside = torch.isnan(buf)
            outside[G:G + M, 32:32 + N] = True
            assert outside.all(), f"K={K} variant {v}: wrote outside the slice"
