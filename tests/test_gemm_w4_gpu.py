"""Four-wave 256-row decode GEMM (csrc/kernels/gemm_w4.hip) against its parent kernels,
bit for bit: every accumulator takes its K range in the same ascending 32-wide MFMA steps
as gemm_decode (bm 256, bn 128) and gemm_pp (bm 256), so the bf16 outputs, the fp32 split-K
slabs and the fused SwiGLU must be identical. K = 64 T covers fewer K-steps than the three
LDS buffers (T = 1, 2), exactly three, and more (the prologue, the steady loop and the two
issue-free last K-tiles); S covers even and uneven K slices. Outputs start as NaN, so an
element the kernel does not write fails the comparison. One case per epilogue also goes
against the fp32 reference with the tolerances of tests/test_gemm_tile_gpu.py."""
import pytest
import torch

from operator_amd import ops
from operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 256


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _close(y, r, tol):
    torch.testing.assert_close(y.float(), r.float(), atol=tol, rtol=tol)


@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7])
def test_w4_store_equals_gemm_decode(N, T):
    K = 64 * T
    torch.manual_seed(N + T)
    x, w = _rand(M, K), _rand(N, K, scale=0.05)
    y, yp = _nan(M, N), _nan(M, N)
    ops.kernels().gemm_w4(x, w, y, None, 1, False)
    ops.kernels().gemm_decode(x, w, yp, None, 1, 128, 256, False, False, 3)
    assert not torch.isnan(y).any()
    assert torch.equal(y.view(torch.int16), yp.view(torch.int16))
    if (N, T) == (256, 7):
        _close(y, x.float() @ w.float().t(), 2e-2)


@pytest.mark.parametrize("T,S", [(7, 2), (7, 3), (16, 8)])
def test_w4_partial_equals_gemm_decode(T, S):
    N, K = 256, 64 * T
    torch.manual_seed(T + S)
    x, w = _rand(M, K), _rand(N, K, scale=0.05)
    p, pp = _nan(S * M * N, dtype=torch.float32), _nan(S * M * N, dtype=torch.float32)
    ops.kernels().gemm_w4(x, w, None, p, S, False)
    ops.kernels().gemm_decode(x, w, None, pp, S, 128, 256, False, False, 3)
    assert not torch.isnan(p).any()
    for s in range(S):
        a, b = p.view(S, M, N)[s], pp.view(S, M, N)[s]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"slab {s}"
    if (T, S) == (7, 3):
        _close(p.view(S, M, N).sum(0), x.float() @ w.float().t(), 1e-3)
        y = _nan(M, N)   # reduced into y by the launcher
        ops.kernels().gemm_w4(x, w, y, p, S, False)
        _close(y, x.float() @ w.float().t(), 2e-2)


@pytest.mark.parametrize("T", [1, 3, 7])
def test_w4_silu_equals_gemm_pp(T):
    inter, K = 128, 64 * T   # N = 256: two tiles of 64 gate + 64 up rows
    torch.manual_seed(T)
    x = _rand(M, K)
    g, u = _rand(inter, K, scale=0.05), _rand(inter, K, scale=0.05)
    wgu = ops.interleave_gate_up(g, u, ops.GU_BLOCK)
    y, yp = _nan(M, inter), _nan(M, inter)
    ops.kernels().gemm_w4(x, wgu, y, None, 1, True)
    ops.kernels().gemm_pp(x, wgu, yp, None, 1, 256, True, True)
    assert not torch.isnan(y).any()
    assert torch.equal(y.view(torch.int16), yp.view(torch.int16))
    if T == 7:
        gg = (x.float() @ g.float().t()).to(torch.bfloat16)
        uu = (x.float() @ u.float().t()).to(torch.bfloat16)
        _close(y, ref.silu_mul(torch.cat([gg, uu], 1), None), 3e-2)


def test_w4_rejects_bad_arguments():
    """M != 256, N % 128 != 0, more K slices than K-steps and SwiGLU with S > 1 are refused
    by the binding's checks (nothing is launched: every output and the slab buffer stay NaN)."""
    C = ops.kernels()
    K = 128
    p = _nan(4 * M * 256, dtype=torch.float32)
    ys = [_nan(128, 256), _nan(M, 192), _nan(M, 128)]
    with pytest.raises(RuntimeError):
        C.gemm_w4(_rand(128, K), _rand(256, K), ys[0], None, 1, False)
    with pytest.raises(RuntimeError):
        C.gemm_w4(_rand(M, K), _rand(192, K), ys[1], None, 1, False)
    with pytest.raises(RuntimeError):
        C.gemm_w4(_rand(M, K), _rand(256, K), None, p, 3, False)   # K / 64 = 2 K-steps
    with pytest.raises(RuntimeError):
        C.gemm_w4(_rand(M, K), _rand(256, K), ys[2], p, 2, True)
    torch.cuda.synchronize()
    assert torch.isnan(p).all() and all(torch.isnan(y).all() for y in ys)
