"""ops.linear / ops.gate_up_silu hand each back end what a direct call of its binding with the
plan's arguments would: every route's output is bit-identical to that call (deferred plans:
the fp32 slabs as int32), and one case per route also goes against the fp32 formula at the
tolerances of tests/test_gemm_w4_gpu.py. N = 256, K = 448 = 7 K-steps, the smallest count that
runs the prologue, the steady loop and the two issue-free tail tiles of every ring depth
(gemm_skinny cuts K in 128-column steps per slice and cannot take 448: its two routes use
K = 512). Plans are installed in ``ops.gemm_table()``; outputs the API lets the caller pass
start as NaN."""
import pytest
import torch
import torch.nn.functional as F

from operator_amd import ops
from operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, K = 256, 448


def _rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _close(y, r, tol):
    torch.testing.assert_close(y.float(), r.float(), atol=tol, rtol=tol)


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype and not torch.isnan(a).any()
    bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(a.view(bits), b.view(bits))


def _xw(M, k=K, seed=0):
    torch.manual_seed(1000 * M + k + seed)
    return _rand(M, k), _rand(N, k, scale=0.05)


def _xgu(M, seed=0):
    torch.manual_seed(2000 * M + seed)
    x, g, u = _rand(M, K), _rand(N // 2, K, scale=0.05), _rand(N // 2, K, scale=0.05)
    gg, uu = (x.float() @ g.float().t()).to(torch.bfloat16), (x.float() @ u.float().t()).to(torch.bfloat16)
    return x, ops.interleave_gate_up(g, u, ops.GU_BLOCK), ref.silu_mul(torch.cat([gg, uu], 1), None)


def _slabs(r, S, M):
    assert isinstance(r, ops.SplitK) and r.S == S and r.shape == (M, N)
    return r.p[: S * M * N]


def test_skinny_routes(monkeypatch):
    M, k = 8, 512
    x, w = _xw(M, k)
    C = ops.kernels()
    monkeypatch.setitem(ops.gemm_table(), ("skinny", M, N, k), 1)
    y, yd = _nan(M, N), _nan(M, N)
    assert ops.linear(x, w, out=y) is y
    C.gemm_skinny(x, w, yd, None, 1, False)
    _same(y, yd)
    _close(y, x.float() @ w.float().t(), 2e-2)
    monkeypatch.setitem(ops.gemm_table(), ("skinny", M, N, k), 2)
    p, pd = _nan(2 * M * N, dtype=torch.float32), _nan(2 * M * N, dtype=torch.float32)
    r = ops.linear(x, w, partial=p, defer_reduce=True)
    assert r.p is p
    C.gemm_skinny(x, w, None, pd, 2, False)
    _same(_slabs(r, 2, M), pd)
    _close(p.view(2, M, N).sum(0), x.float() @ w.float().t(), 1e-3)


@pytest.mark.parametrize("plan,kernel", [([128, 128, 5, 4], "decode"), ([256, 128, 3, 4, "w4"], "w4")])
def test_split_k_plan_routes(monkeypatch, plan, kernel):
    """A four-element plan on gemm_decode (5 uneven K slices) and a plan tagged "w4" on gemm_w4,
    reduced into y and deferred; explicit arguments send the tagged plan's first four elements
    to gemm_decode."""
    M, S = 256, plan[2]
    x, w = _xw(M, seed=S)
    C = ops.kernels()
    monkeypatch.setitem(ops.gemm_table(), (M, N, K), plan)

    def direct(y, p, ns=plan[3]):
        if kernel == "w4":
            C.gemm_w4(x, w, y, p, S, False)
        else:
            C.gemm_decode(x, w, y, p, S, plan[1], plan[0], False, False, ns)

    y, yd = _nan(M, N), _nan(M, N)
    p, pd = _nan(S * M * N, dtype=torch.float32), _nan(S * M * N, dtype=torch.float32)
    assert ops.linear(x, w, out=y, partial=p) is y
    direct(yd, pd)
    _same(y, yd)
    _same(p, pd)
    _close(y, x.float() @ w.float().t(), 2e-2)
    p, pd = _nan(S * M * N, dtype=torch.float32), _nan(S * M * N, dtype=torch.float32)
    r = ops.linear(x, w, partial=p, defer_reduce=True)
    assert r.p is p
    direct(None, pd)
    _same(_slabs(r, S, M), pd)
    _close(p.view(S, M, N).sum(0), x.float() @ w.float().t(), 1e-3)
    r = ops.linear(x, w, defer_reduce=True)   # no buffer given: a fresh one, same slabs
    assert r.p is not p
    _same(_slabs(r, S, M), pd)
    if kernel == "w4":
        y, yd = _nan(M, N), _nan(M, N)
        ops.linear(x, w, out=y, stages=3)
        C.gemm_decode(x, w, yd, pd, S, 128, 256, False, False, 3)
        _same(y, yd)


@pytest.mark.parametrize("M,entry", [(128, "pp128"), (256, "pp256"), (256, "w4"), (256, [128, 4])])
def test_gate_up_silu_table_routes(monkeypatch, M, entry):
    x, wgu, want = _xgu(M)
    C = ops.kernels()
    monkeypatch.setitem(ops.gemm_table(), ("silu", M, N, K), entry)
    y = ops.gate_up_silu(x, wgu, ops.GU_BLOCK)
    yd = _nan(M, N // 2)
    if entry == "w4":
        C.gemm_w4(x, wgu, yd, None, 1, True)
    elif isinstance(entry, str):
        C.gemm_pp(x, wgu, yd, None, 1, int(entry[2:]), True, True)
    else:
        C.gemm_decode(x, wgu, yd, None, 1, 128, entry[0], True, False, entry[1])
    _same(y, yd)
    _close(y, want, 3e-2)


def test_gate_up_silu_w4_entry_on_128_rows_raises(monkeypatch):
    x, wgu, _ = _xgu(128)
    monkeypatch.setitem(ops.gemm_table(), ("silu", 128, N, K), "w4")
    with pytest.raises(ValueError, match="gemm_w4 takes the 256-row bucket only"):
        ops.gate_up_silu(x, wgu, ops.GU_BLOCK)


@pytest.mark.parametrize("bias", [False, True])
def test_tile_route(bias):
    M = 40
    x, w = _xw(M)
    b = _rand(N) if bias else None
    y, yd = _nan(M, N), _nan(M, N)
    n0 = ops.BLAS_CALLS["n"]
    assert ops.linear(x, w, out=y, bias=b) is y
    ops.kernels().gemm_tile(x, w, yd, b, False)
    _same(y, yd)
    _close(y, x.float() @ w.float().t() + (b.float() if bias else 0), 2e-2)
    assert ops.BLAS_CALLS["n"] == n0


def test_tile_swiglu_route():
    M = 300
    x, wgu, want = _xgu(M)
    y = ops.gate_up_silu(x, wgu, ops.GU_BLOCK)
    yd = _nan(M, N // 2)
    ops.kernels().gemm_tile(x, wgu, yd, None, True)
    _same(y, yd)
    _close(y, want, 3e-2)


def test_blas_fallback_route(monkeypatch):
    """K = 96 is no multiple of 64: no kernel takes it, hipBLASLt does, counted as a fallback,
    and OAMD_FORBID_BLAS=1 turns the fallback into an error."""
    M = 40
    x, w = _xw(M, 96)
    monkeypatch.delenv("OAMD_FORBID_BLAS", raising=False)
    n0, p0 = ops.BLAS_CALLS["n"], ops.BLAS_PLANNED["n"]
    y = _nan(M, N)
    assert ops.linear(x, w, out=y) is y
    assert (ops.BLAS_CALLS["n"] - n0, ops.BLAS_PLANNED["n"] - p0) == (1, 0)
    _same(y, F.linear(x, w, None, out=_nan(M, N)))
    _close(y, x.float() @ w.float().t(), 2e-2)
    monkeypatch.setenv("OAMD_FORBID_BLAS", "1")
    with pytest.raises(RuntimeError, match="OAMD_FORBID_BLAS=1"):
        ops.linear(x, w)


@pytest.mark.parametrize("kernel", ["gemm_decode", "gemm_pp", "gemm_skinny"])
def test_bindings_refuse_cpu_outputs(kernel):
    """A y or a slab buffer in host memory is refused by the binding's shared output check with
    nothing launched: the GPU buffers of the same calls stay NaN."""
    C = ops.kernels()
    M = 8 if kernel == "gemm_skinny" else 256
    x, w = _xw(M, 512)   # two K slices every one of the three takes
    tail = {"gemm_decode": (128, 256, False, False, 3), "gemm_pp": (256, False, True), "gemm_skinny": (False,)}[kernel]
    y, p = _nan(M, N), _nan(2 * M * N, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        getattr(C, kernel)(x, w, y.cpu(), p, 2, *tail)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        getattr(C, kernel)(x, w, y, p.cpu(), 2, *tail)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        getattr(C, kernel)(x, w, None, p.cpu(), 2, *tail)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(p).all()
