"""The exact GEMM references of tests/gemm_exact.py, checked on the CPU: what
tests/test_gemm_exact_gpu.py compares the kernels with must itself be right."""
import pytest
import torch

import gemm_exact as gx


def test_operands_are_exact_in_bf16_and_e4m3():
    x = gx.ints(64, 512, 1)
    assert x.min() == gx.LO and x.max() == gx.HI and torch.equal(x, x.round())
    assert torch.equal(x.to(torch.bfloat16).double(), x)
    assert torch.equal(x.float().to(torch.float8_e4m3fn).double(), x)
    assert torch.equal(gx.ints(64, 512, 1), x) and not torch.equal(gx.ints(64, 512, 2), x)
    assert 15 * 15 * gx.MAX_K < 2 ** 24 and max(gx.ALL_K) <= gx.MAX_K


def test_product_is_order_independent_in_fp32():
    x, w = gx.ints(32, 2048, 3), gx.ints(48, 2048, 4)
    r = gx.product(x, w)
    perm = torch.randperm(2048, generator=torch.Generator().manual_seed(5))
    f = torch.zeros(32, 48)
    for c in perm.view(32, 64):   # fp32, 64 columns at a time in a shuffled order
        f += x[:, c].float() @ w[:, c].float().t()
    assert torch.equal(f.double(), r)


SPLITS = sorted({(64 * t, s, 64) for t, s in gx.DECODE_TS + gx.W4_TS} | {(64 * t, s, 0) for t, s in gx.PP_TS}
                | {(128 * s * 9, s, 0) for s in gx.SKINNY_S} | {(k, s, 0) for k, s in gx.TILE_KS}
                | {(128 * t, s, 128) for t in gx.FP8_T for s in gx.FP8_S if 1 < s <= t} | {(320, 2, 64), (448, 3, 64)})


@pytest.mark.parametrize("K,S,step", SPLITS)
def test_slab_references_sum_to_the_product(K, S, step):
    sl = gx.equal_slices(K, S) if step == 0 else gx.even_slices(K, S, step)
    assert sl[0][0] == 0 and sl[-1][1] == K and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
    sizes = [b - a for a, b in sl]
    assert min(sizes) >= max(step, 1) and all(n % max(step, 1) == 0 for n in sizes)
    assert max(sizes) - min(sizes) <= step   # equal slices: 0; even slices: at most one step apart
    x, w = gx.ints(33, K, K + S), gx.ints(48, K, K + S + 1)
    p = gx.slabs(x, w, sl)
    assert p.shape == (S, 33, 48)
    assert torch.equal(p.sum(0), gx.product(x, w))
    assert torch.equal(gx.f32_bits(p).view(torch.float32).double(), p)
    if S > 1 and K // S >= 64:
        assert not torch.equal(p[0], p[1])


def test_even_slices_are_the_kernels_rule():
    assert gx.even_slices(13 * 64, 5, 64) == [(0, 128), (128, 320), (320, 448), (448, 640), (640, 832)]
    assert gx.even_slices(7 * 128, 3, 128) == [(0, 256), (256, 512), (512, 896)]
    assert gx.equal_slices(448, 7) == [(64 * i, 64 * i + 64) for i in range(7)]


def test_bf16_bits_round_to_nearest_even_once():
    # 257 -> 256 (tie to even), 259 -> 260 (tie to even, up), 258.5 -> 258 (below the tie), -259 -> -260
    r = torch.tensor([257.0, 259.0, 258.5, -259.0, 0.0, 1.0, 65535.0, 3.0 * 2 ** -5], dtype=torch.float64)
    assert gx.bf16_round(r).tolist() == [256.0, 260.0, 258.0, -260.0, 0.0, 1.0, 65536.0, 3.0 * 2 ** -5]
    big = gx.product(gx.ints(256, 2048, 6), gx.ints(256, 2048, 7))
    assert torch.equal(gx.bf16_bits(big), big.float().to(torch.bfloat16).view(torch.int16))
    trunc = (gx.f32_bits(big) >> 16).to(torch.int16)
    assert (trunc != gx.bf16_bits(big)).double().mean() > 0.2   # truncation is a different function here


def test_tiled_weight_permutation_and_inverse():
    N, K = 128, 192
    w = torch.arange(N * K, dtype=torch.float64).view(N, K)
    wt = gx.tile_w(w)
    assert wt.shape == w.shape and not torch.equal(wt, w)
    assert torch.equal(gx.untile_w(wt), w)
    flat = wt.reshape(-1)   # element (n, k) at ((n / 64) (K / 64) + k / 64) 4096 + (n % 64) 64 + k % 64
    for n, k in ((0, 0), (1, 0), (63, 63), (64, 0), (5, 64), (127, 191), (70, 130)):
        assert flat[((n // 64) * (K // 64) + k // 64) * 4096 + (n % 64) * 64 + k % 64] == w[n, k]


def test_swiglu_reference():
    M, inter, K = 16, 128, 64
    x, g, u = gx.ints(M, K, 8, 1, 15), gx.ints(inter, K, 9, 1, 15), gx.ints(inter, K, 10)
    gs, us = gx.product(x, g), gx.product(x, u)
    assert gs.min() >= 64
    # sigmoid is exactly 1 in fp32 from the smallest gate sum on
    g32 = torch.tensor([64.0, 187200.0])
    assert torch.equal(1.0 + torch.exp(-g32), torch.ones(2)) and torch.equal(g32 / (1.0 + torch.exp(-g32)), g32)
    want = gx.swiglu(gs, us)
    gb, ub = gs.float().to(torch.bfloat16), us.float().to(torch.bfloat16)
    silu = torch.nn.functional.silu(gb.float()).to(torch.bfloat16)   # the kernels' rounding points
    assert torch.equal((silu.float() * ub.float()).to(torch.bfloat16).view(torch.int16), want)
    # the interleaved weight: block b holds gate rows 64 b .. 64 b + 63, then the same features' up rows
    wgu = gx.interleave(g, u)
    assert wgu.shape == (2 * inter, K)
    assert torch.equal(wgu[0:64], g[0:64]) and torch.equal(wgu[64:128], u[0:64])
    assert torch.equal(wgu[128:192], g[64:128]) and torch.equal(wgu[192:256], u[64:128])
    with pytest.raises(AssertionError):
        gx.swiglu(us, us)   # gate sums below 64 have no exact reference


def test_fp8_scales_keep_the_product_exact():
    sx, sw = gx.fp8_scales(7, 5)
    assert sx.tolist() == [1, .5, .25, .125, 1, .5, .25] and sw.tolist() == [1, .5, .25, 1, .5]
    x, w = gx.ints(7, 896, 11), gx.ints(5, 896, 12)
    scale = sx[:, None] * sw[None, :]
    p = gx.slabs(x, w, gx.even_slices(896, 3, 128)) * scale
    gx.f32_bits(p)   # asserts exactness in fp32
    f = p[0].float()
    for s in (1, 2):
        f = f + p[s].float()   # the slab sum in fp32, in slab order
    assert torch.equal(f.double(), gx.product(x, w) * scale)


def test_reference_exercises_rounding():
    gx.assert_rounding_is_exercised()
    differ, ties = gx.rounding_share(gx.product(gx.ints(256, 256, 13, -3, 3), gx.ints(256, 256, 14, -3, 3)))
    assert differ < 0.01   # the [-3, 3] operands of the older layout test hardly round at all
