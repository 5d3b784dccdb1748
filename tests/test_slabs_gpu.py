"""The split-K slab hand-off, stated once for every consumer.

A split-K GEMM leaves S fp32 slabs [S, rows, cols]; its consumer sums them in slab order and rounds
to bf16 once (csrc/kernels/common.h slab_sum). So a consumer fed the slabs equals, bit for bit, the
same consumer fed the bf16 tensor ``a = P[0]; a += P[k]; bf16(a)`` on every output that does not
depend on a reduction order inside the kernel. S = 1, 2, 3, 4, 5, 8 reaches every compile-time arm
and the runtime arm of every kernel (3: runtime everywhere; 5: compile-time in rope_kv only; 2:
runtime in the fused decode RoPE). The fused all-reduce + RMSNorm runs the same slab counts in
tests/test_custom_ar_gpu.py.

The second half: a slab tensor that was never valid (host memory, bf16, one element short, a
non-contiguous view, splits = 0, a base off by one float, given together with the bf16 input, or
neither given) raises in the binding before any launch; the pre-filled outputs stay as they were.
"""
import functools
import math

import pytest
import torch

from operator_amd import ops
from operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLITS = [1, 2, 3, 4, 5, 8]


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _slabs(S, rows, cols):
    """(P fp32 [S, rows, cols], the bf16 tensor the hand-off promises), computed once per shape and
    shared (read-only) by the tests."""
    g = torch.Generator(device=DEV).manual_seed(1000 * S + rows + cols)
    P = torch.randn(S, rows, cols, device=DEV, generator=g) / 2
    a = P[0].clone()
    for k in range(1, S):
        a += P[k]
    return P, a.to(torch.bfloat16)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# (a) one contract, every consumer
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("hidden", [2048, 4096, 8192])   # 256 threads; the 512-thread slab path; 4 vectors a thread
def test_rmsnorm(S, hidden):
    """The updated residual is bit-equal. y is held to 2^-6 relative: the 512-thread slab path sums
    the squares in another order, which moves 1/rms by ~1e-7 relative; that can flip the inner bf16
    rounding of y = bf16(bf16(v / rms) * w) by one ulp (<= 2^-7 relative), and the outer rounding of
    each side adds half an ulp (<= 2^-8 relative each)."""
    rows = 3
    P, xb = _slabs(S, rows, hidden)
    w, r0 = _rand(hidden, seed=1), _rand(rows, hidden, seed=2)
    r1, r2 = r0.clone(), r0.clone()
    y1 = ops.rmsnorm(ops.SplitK(P.reshape(-1), S, rows, hidden), w, 1e-5, residual=r1)
    y2 = ops.rmsnorm(xb, w, 1e-5, residual=r2)
    _same(r1, r2)
    assert not torch.equal(r1, r0)
    torch.testing.assert_close(y1.float(), y2.float(), rtol=2 ** -6 * (1 + 2 ** -6), atol=1e-30)   # + the second-order term


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
def test_rope_kv(S, bias, fp8):
    """q / k / v and the cache. A bias is added in fp32 before the one rounding (bf16(x W^T + b)), so
    with a bias the bf16 tensor is bf16(slab-order sum + bias) and is fed without one."""
    T, Hq, Hkv, D = 3, 8, 2, 128
    W = (Hq + 2 * Hkv) * D
    P, xb = _slabs(S, T, W)
    b = _rand(W, seed=3) if bias else None
    if bias:
        a = P[0].clone()
        for k in range(1, S):
            a += P[k]
        xb = (a + b.float()).to(torch.bfloat16)
    cos, sin = (t.to(DEV) for t in ref.rope_tables(64, D, 500000.0))
    pos = torch.tensor([0, 5, 63], device=DEV)
    slots = torch.tensor([3, 17, 40], device=DEV)
    ks, vs = (0.5, 2.0) if fp8 else (1.0, 1.0)
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc1, vc1, kc2, vc2 = (torch.zeros(4, Hkv, 16, D, device=DEV, dtype=dt) for _ in range(4))
    got = ops.rope_kv(ops.SplitK(P.reshape(-1), S, T, W), pos, cos, sin, Hq, Hkv, kc1, vc1, slots, bias=b,
                      k_scale=ks, v_scale=vs)
    want = ops.rope_kv(xb, pos, cos, sin, Hq, Hkv, kc2, vc2, slots, k_scale=ks, v_scale=vs)
    for a, c in zip(got, want):
        _same(a, c)
    _same(kc1, kc2)
    _same(vc1, vc2)
    assert _bits(kc1).any() and _bits(vc1).any()


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("inter", [2048, 5120])   # two and four vectors a thread
def test_silu_quantize_fp8(S, inter):
    M = 3
    P, xb = _slabs(S, M, 2 * inter)
    q1, s1 = ops.silu_quantize_fp8(ops.SplitK(P.reshape(-1), S, M, 2 * inter), block=64)
    q2, s2 = ops.silu_quantize_fp8(xb, block=64)
    _same(q1, q2)
    _same(s1, s2)


def _decode_case(B=2, Hq=8, Hkv=2, page=16, ctx=40, D=128):
    g = torch.Generator(device=DEV).manual_seed(7)
    maxp = (ctx + page - 1) // page + 1
    pages = B * maxp + 1
    kc = torch.randn(pages, Hkv, page, D, device=DEV, generator=g).to(torch.bfloat16)
    vc = torch.randn(pages, Hkv, page, D, device=DEV, generator=g).to(torch.bfloat16)
    bt = torch.arange(B * maxp, device=DEV, dtype=torch.int32).reshape(B, maxp)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    pos = torch.full((B,), ctx - 1, dtype=torch.long, device=DEV)
    slots = (bt[:, (ctx - 1) // page].long() * page + (ctx - 1) % page)
    cos, sin = (t.to(DEV) for t in ref.rope_tables(64, D, 500000.0))
    return kc, vc, bt, lens, pos, slots, cos, sin


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("num_splits", [1, 2])
def test_attn_decode_rope(S, num_splits):
    """The attention output and the cache (the decode token's row is the only one written)."""
    B, Hq, Hkv, D = 2, 8, 2, 128
    ncol = (Hq + 2 * Hkv) * D
    assert B * Hkv <= ops.FUSED_ROPE_MAX_SEQ_HEADS and ops.FUSED_DECODE_ROPE   # the fused kernel runs
    P, xb = _slabs(S, B, ncol)
    kc0, vc0, bt, lens, pos, slots, cos, sin = _decode_case(B, Hq, Hkv)
    kc1, vc1, kc2, vc2 = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
    scale = 1 / math.sqrt(D)
    got = ops.attn_decode_rope(ops.SplitK(P.reshape(-1), S, B, ncol), pos, cos, sin, Hq, kc1, vc1, slots, bt, lens,
                               scale, num_splits)
    want = ops.attn_decode_rope(xb, pos, cos, sin, Hq, kc2, vc2, slots, bt, lens, scale, num_splits)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    _same(got, want)
    _same(kc1, kc2)
    _same(vc1, vc2)
    assert not torch.equal(kc1, kc0) and not torch.equal(vc1, vc0)


@pytest.mark.parametrize("S", SPLITS)
def test_linear_reduced_equals_its_deferred_slabs(S):
    """ops.linear(..., splits=S): the reduce pass over the slabs == the slabs it would have deferred,
    added in slab order and rounded once (gemm_decode, and gemm_fp8, which shares its reduce kernel)."""
    M, N, K = 64, 256, 1024
    x, w = _rand(M, K, seed=4), _rand(N, K, seed=5, scale=0.05)

    def ordered(sk):
        p = sk.p[: S * M * N].view(S, M, N)
        a = p[0].clone()
        for k in range(1, S):
            a += p[k]
        return a.to(torch.bfloat16)

    y = ops.linear(x, w, splits=S)
    sk = ops.linear(x, w, splits=S, defer_reduce=True)
    w8, sw = ops.quantize_fp8(w)
    y8 = ops.linear_fp8(x, w8, sw, plan=(64, 64, S))
    sk8 = ops.linear_fp8(x, w8, sw, plan=(64, 64, S), defer_reduce=True)
    if S == 1:
        _same(sk, y)
        _same(sk8, y8)
    else:
        assert isinstance(sk, ops.SplitK) and isinstance(sk8, ops.SplitK) and sk.S == sk8.S == S
        _same(ordered(sk), y)
        _same(ordered(sk8), y8)


# ---------------------------------------------------------------------------------------------
# (b) refusals before any launch
# ---------------------------------------------------------------------------------------------

def _bad_slabs(n):
    """name -> (slab tensor, splits) for S = 2 slabs of n / 2 floats: each was never valid."""
    good = torch.zeros(n, device=DEV)
    return {
        "host": (torch.zeros(n), 2),
        "bf16": (torch.zeros(n, dtype=torch.bfloat16, device=DEV), 2),
        "short": (torch.zeros(n - 1, device=DEV), 2),
        "strided": (torch.zeros(2 * n, device=DEV)[::2], 2),
        "splits0": (good, 0),
        "off_by_a_float": (torch.zeros(n + 1, device=DEV)[1:], 2),
    }


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _refuse(call, x, n, outs):
    """``call(x_or_None, slabs_or_None, splits)`` raises for every invalid slab tensor, for both the
    bf16 input and the slabs, and for neither; ``outs`` (pre-filled) stay untouched."""
    before = [o.clone() for o in outs]
    for name, (p, s) in _bad_slabs(n).items():
        with pytest.raises(RuntimeError):
            call(None, p, s)
    with pytest.raises(RuntimeError, match="exactly one of"):
        call(x, torch.zeros(n, device=DEV), 2)
    with pytest.raises(RuntimeError, match="exactly one of"):
        call(None, None, 2)
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        _same(o, b)


def test_rmsnorm_refuses_invalid_slabs():
    C = ops.kernels()
    rows, hidden = 3, 2048
    w, r, y = _rand(hidden, seed=1), _rand(rows, hidden, seed=2), _nan(rows, hidden)
    _refuse(lambda x, p, s: C.rmsnorm(x, r, w, y, 1e-5, p, s), _rand(rows, hidden, seed=3), 2 * rows * hidden, [r, y])


def test_rope_kv_refuses_invalid_slabs():
    C = ops.kernels()
    T, Hq, Hkv, D = 3, 8, 2, 128
    W = (Hq + 2 * Hkv) * D
    cos, sin = (t.to(DEV) for t in ref.rope_tables(64, D, 500000.0))
    pos, slots = torch.tensor([0, 5, 63], device=DEV), torch.tensor([3, 17, 40], device=DEV)
    q, k, v = _nan(T, Hq, D), _nan(T, Hkv, D), _nan(T, Hkv, D)
    kc, vc = _nan(4, Hkv, 16, D), _nan(4, Hkv, 16, D)
    _refuse(lambda x, p, s: C.rope_kv(x, pos, cos, sin, Hq, Hkv, q, k, v, kc, vc, slots, p, s),
            _rand(T, W, seed=3), 2 * T * W, [q, k, v, kc, vc])


def test_silu_quantize_fp8_refuses_invalid_slabs():
    C = ops.kernels()
    M, inter = 3, 2048
    q = torch.full((M, inter), 0x55, dtype=torch.uint8, device=DEV)
    sx = _nan(M, dtype=torch.float32)
    _refuse(lambda x, p, s: C.silu_quantize_fp8(x, q, sx, p, s), _rand(M, 2 * inter, seed=3), 2 * M * 2 * inter,
            [q, sx])


def test_attn_decode_refuses_invalid_slabs():
    C = ops.kernels()
    B, Hq, Hkv, D = 2, 8, 2, 128
    ncol = (Hq + 2 * Hkv) * D
    kc, vc, bt, lens, pos, slots, cos, sin = _decode_case(B, Hq, Hkv)
    out = _nan(B, Hq, D)
    op, ml = ops.decode_workspace(B, Hq, 1, DEV)

    def call(x, p, s):
        C.attn_decode(None, kc, vc, bt, lens, out, op, ml, 1, 1 / math.sqrt(D), 0, 1.0, 1.0, None, None, x, p, s, pos,
                      cos, sin, slots, None)

    _refuse(call, _rand(B, ncol, seed=3), 2 * B * ncol, [out, kc, vc])
    # the rotated q together with either form of the projection is refused as well
    q = _rand(B, Hq, D, seed=4)
    for x, p in ((_rand(B, ncol, seed=3), None), (None, torch.zeros(2 * B * ncol, device=DEV))):
        with pytest.raises(RuntimeError):
            C.attn_decode(q, kc, vc, bt, lens, out, op, ml, 1, 1 / math.sqrt(D), 0, 1.0, 1.0, None, None, x, p, 2,
                          pos, cos, sin, slots, None)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_all_reduce_rmsnorm_refuses_invalid_slabs():
    rows, hidden = 3, 2048
    car = ops.kernels().CustomAllReduce(1 << 20, 0, 1, 4, torch.cuda.current_device(), 0.5)   # a group of one
    try:
        w, r, y = _rand(hidden, seed=1), _rand(rows, hidden, seed=2), _nan(rows, hidden)
        _refuse(lambda x, p, s: car.all_reduce_rmsnorm(x, r, w, y, 1e-5, p, s), _rand(rows, hidden, seed=3),
                2 * rows * hidden, [r, y])
    finally:
        car.close()


def test_gemm_fp8_refuses_invalid_slab_buffer():
    """gemm_fp8's p gets the producers' output check (device, fp32, contiguity, size, alignment)."""
    C = ops.kernels()
    M, N, K = 64, 128, 256
    q, sx = ops.quantize_fp8(_rand(M, K, seed=4))
    w8, sw = ops.quantize_fp8(_rand(N, K, seed=5, scale=0.05))
    y = _nan(M, N)
    for name, (p, s) in _bad_slabs(2 * M * N).items():
        with pytest.raises(RuntimeError):
            C.gemm_fp8(q, w8, sx, sw, y, p, s, 64, 64)
    with pytest.raises(RuntimeError, match="needs a partial buffer"):
        C.gemm_fp8(q, w8, sx, sw, y, None, 2, 64, 64)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        C.gemm_fp8(q, w8, sx, sw, y.cpu(), torch.zeros(2 * M * N, device=DEV), 2, 64, 64)
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
