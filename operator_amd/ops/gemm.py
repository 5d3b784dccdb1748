"""bf16 GEMMs of the model (QKV, O, gate|up + SwiGLU, down, lm_head): plan, then launch.

``route`` picks the back end from plain values (shape, facts about the tensors, the caller's
explicit arguments, the tuned table); ``_launch`` is the only code that calls one. Prefill
projections (M > 256 rows) run on gemm_tile's persistent p5 schedule, decode buckets on
gemm_skinny / gemm_decode / gemm_pp / gemm_w4, the lm_head on gemm_tile. hipBLASLt is reached only
by shapes none of them takes (K % 64 != 0, N % 16 != 0, non-bf16) or that the table measured it
fastest on (BLAS_CALLS), or by the plain prefill projections under OAMD_PREFILL_BLAS=1, an A/B
against the vendor library (BLAS_PLANNED; profiles/gemm_tile_p5_vs_hipblaslt_r6.jsonl). The table
(``gemm_tuned.json`` or OAMD_GEMM_TABLE) is the only selector among the kernels: an A/B run
installs each arm's plan in ``gemm_table()``.
"""
from __future__ import annotations

import json
import os
from typing import NamedTuple

import torch
import torch.nn.functional as F

from ._native import kernels


class SplitK:
    """A GEMM's output left as S fp32 split-K slabs [S, M, N]; the consumer (rmsnorm, rope_kv,
    silu_quantize_fp8, the fused decode RoPE, the fused all-reduce + norm) sums them in slab order
    and rounds to bf16 once, so the GEMM's separate reduction pass disappears. Not a tensor: a
    consumer tests ``isinstance`` first."""

    __slots__ = ("p", "S", "shape", "device")

    def __init__(self, p: torch.Tensor, S: int, M: int, N: int):
        self.p, self.S, self.shape, self.device = p, S, (M, N), p.device

    def materialize(self) -> torch.Tensor:
        M, N = self.shape
        return self.p[: self.S * M * N].view(self.S, M, N).sum(0).to(torch.bfloat16)


class Plan(NamedTuple):
    """One GEMM launch; p[:3] = (bm, bn, splits), bm / bn 0 where the kernel has one tile shape."""
    bm: int = 0
    bn: int = 0
    splits: int = 1
    stages: int = 3
    kernel: str = "decode"   # skinny | decode | pp | w4 | tile | blas
    planned: bool = False    # blas: by design (PREFILL_BLAS, counted in BLAS_PLANNED), else a fallback (BLAS_CALLS)


TILE = Plan(kernel="tile")
BLAS = Plan(kernel="blas")

GU_BLOCK = 64  # gate|up weight rows interleaved in 64-feature blocks (fused SwiGLU epilogue)
GEMM_DECODE_M = (64, 128, 256)  # decode buckets the gfx950 gemm_decode kernel is tuned for
SKINNY_MAX_M = 32
LM_HEAD_MIN_N = 32768   # vocab projections always run on gemm_tile (weight-streaming bound there)
PREFILL_BLAS = os.environ.get("OAMD_PREFILL_BLAS", "0") == "1"
BLAS_CALLS = {"n": 0}   # GPU GEMMs that FELL BACK to hipBLASLt (tests assert it stays 0 on model shapes)
BLAS_PLANNED = {"n": 0}   # plain prefill projections run on hipBLASLt by design (PREFILL_BLAS)

_GEMM_TABLE_PATH = os.environ.get("OAMD_GEMM_TABLE") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                     "gemm_tuned.json")
_gemm_table: dict | None = None


def gemm_table() -> dict:
    """Measured best plan per decode GEMM shape on MI355X (``tools/bench_gemm.py --write-table``): keys
    (M, N, K), ("skinny", ...), ("silu", ...), raw JSON values for ``_decode``. Tests and A/B tools install entries."""
    global _gemm_table
    if _gemm_table is None:
        try:
            with open(_GEMM_TABLE_PATH) as f:
                _gemm_table = {tuple(x if x in ("silu", "skinny") else int(x) for x in k.split(",")): v
                               for k, v in json.load(f).items()}
        except (OSError, ValueError):
            _gemm_table = {}
    return _gemm_table


def _says_blas(raw) -> bool:   # all routing asks before it knows whether the entry will be used
    return raw == "blas"


def _decode(raw, key: tuple) -> Plan | None:
    """The table value ``raw`` of ``key`` as a plan (None: no entry). The spellings:
    (M, N, K): [bm, bn, S], [bm, bn, S, stages], [bm, bn, S, stages, "w4"], "tile", "blas";
    ("skinny", ...): a split count or "blas"; ("silu", ...): "w4", "pp128" / "pp256",
    [bm] / [bm, stages], "blas" ([0] on the skinny buckets: measured, nothing to choose).
    Raises where an entry asks gemm_w4 for a shape it has no variant for."""
    if raw is None or raw == []:
        return None
    if _says_blas(raw):
        return BLAS
    M, where = key[-3], ",".join(map(str, key))
    if key[0] == "skinny":
        return Plan(splits=int(raw), kernel="skinny")
    if key[0] == "silu":
        if raw == "w4":   # four-wave 256-row kernel (gemm_w4.hip)
            if M != 256:
                raise ValueError(f"gemm table: plan 'w4' on {where}: gemm_w4 takes the 256-row bucket only")
            return Plan(kernel="w4")
        if isinstance(raw, str) and raw.startswith("pp"):   # ping-pong kernel, nt weight loads (bm 128 / 256)
            return Plan(int(raw[2:]), 128, kernel="pp")
        return Plan(raw[0], 128, 1, raw[1] if len(raw) > 1 else 3)
    if raw == "tile":
        return TILE
    plan = Plan(*raw[:4])
    if len(raw) > 4 and raw[4] == "w4":   # the plan runs on gemm_w4; the first four stay its parent gemm_decode plan
        if M != 256 or plan[:2] != (256, 128):
            raise ValueError(f"gemm table: plan {tuple(raw)} on {where}: gemm_w4 runs M = 256 as 256 x 128 tiles only")
        plan = plan._replace(kernel="w4")
    return plan


def row_tile(M: int) -> int:
    """Largest gemm_decode row tile (256, 128, 64) dividing M (M % 64 == 0): a bucket of
    192 rows runs three 64-row tiles, not one 192-row tile the kernel has no variant for."""
    return next(b for b in (256, 128, 64) if M % b == 0)


def _gemm_splits(M: int, N: int, K: int) -> int:
    """Heuristic split-K ways for gemm_decode (shapes not in the tuned table): the
    smallest S | 8 whose (N/64) x S blocks reach one block per CU (256)."""
    tiles = N // 64
    best = 1
    for S in (1, 2, 4, 8):
        if K % (64 * S):
            break
        best = S
        if tiles * S >= 256:
            return S
    return best


def gemm_plan(M: int, N: int, K: int) -> Plan | None:
    """The gemm_decode / gemm_w4 plan of a decode bucket, or None for gemm_tile / hipBLASLt."""
    if M % 64 or N % 64 or K % 64 or M > 256:
        return None
    p = _decode(gemm_table().get((M, N, K)), (M, N, K))
    if p is None:
        return Plan(row_tile(M), 64, _gemm_splits(M, N, K))
    return p if p.kernel in ("decode", "w4") else None


def skinny_plan(M: int, N: int, K: int) -> int | None:
    """Split-K count for the gfx950 gemm_skinny kernel (M <= 32 decode buckets), or None
    for hipBLASLt: tuned table entry ``skinny,M,N,K`` if present, else split K until
    the 16-row tiles give >= 512 blocks (K permitting)."""
    if M > SKINNY_MAX_M or N % 16 or K % 128:
        return None
    p = _decode(gemm_table().get(("skinny", M, N, K)), ("skinny", M, N, K))
    if p is not None:
        return p.splits if p.kernel == "skinny" else None
    S = 1
    while (N // 16) * S < 512 and S < 8 and K % (128 * S * 2) == 0:
        S *= 2
    return S


def _tile_takes(M: int, N: int, K: int, cuda: bool, bf16: bool, w_bf16: bool, contig: bool) -> bool:
    return cuda and bf16 and w_bf16 and contig and K % 64 == 0 and N % 16 == 0 and M >= 1


def route(M: int, N: int, K: int, *, silu: bool = False, block: int | None = None, bias: bool = False,
          cuda: bool = True, bf16: bool = True, w_bf16: bool = True, contig: bool = True, out_ok: bool = True,
          splits: int | None = None, bn: int | None = None, bm: int | None = None, stages: int | None = None,
          prefill_blas: bool = False) -> Plan | None:
    """The launch of y = x @ w^T, x [M, K], w [N, K] (``silu``: fused gate|up + SwiGLU, None where no fused
    kernel takes it). ``cuda`` / ``bf16`` describe x, ``w_bf16`` w, ``contig`` both, ``out_ok``: gemm_tile can
    write the caller's output. The order of the rules is behaviour (tests/test_gemm_route.py pins it)."""
    tab = gemm_table()
    fast = cuda and bf16 and contig   # what the decode kernels ask of the tensors
    tile = _tile_takes(M, N, K, cuda, bf16, w_bf16, contig)
    if silu:
        entry = tab.get(("silu", M, N, K))
        if fast and block == 64 and N % 128 == 0:
            if M <= SKINNY_MAX_M and K % 128 == 0 and skinny_plan(M, N, K) is not None and not _says_blas(entry):
                return Plan(kernel="skinny")
            if M % 64 == 0 and M <= 256 and K % 64 == 0 and not _says_blas(entry):
                return _decode(entry, ("silu", M, N, K)) or Plan(row_tile(M), 128)
        return TILE if block == 64 and tile and N % 128 == 0 else None   # prefill: SwiGLU in the tile epilogue
    if bias:
        return TILE if tile and out_ok else BLAS
    explicit = not (bm is None and bn is None and splits is None)
    if (cuda and not explicit and N < LM_HEAD_MIN_N
            and _says_blas(tab.get(("skinny", M, N, K) if M <= SKINNY_MAX_M else (M, N, K)))):
        return BLAS   # measured fastest on this decode bucket; counted as a fallback all the same
    if prefill_blas and cuda and M > 256 and N < LM_HEAD_MIN_N and splits is None and bf16:
        return BLAS._replace(planned=True)
    if fast and M <= SKINNY_MAX_M and bm is None and bn is None:
        S = splits or skinny_plan(M, N, K)
        if S is not None:
            return Plan(splits=S, kernel="skinny")
    plan = None
    if fast:
        plan = gemm_plan(M, N, K)
        if plan is None and (splits or bn or bm) and M % 64 == 0 and M <= 256 and N % 64 == 0 and K % 64 == 0:
            plan = Plan(row_tile(M), 64, 1)  # explicit request (tests / tuning)
    if plan is None:
        return TILE if tile and out_ok else BLAS
    if explicit or stages is not None:   # a tagged plan's first four elements on gemm_decode
        plan = plan._replace(kernel="decode")
    return Plan(bm or plan.bm, bn or plan.bn, splits or plan.splits, stages or plan.stages, plan.kernel)


def _blas(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None, bias: torch.Tensor | None, planned: bool):
    if x.is_cuda and planned:
        BLAS_PLANNED["n"] += 1
    elif x.is_cuda:
        BLAS_CALLS["n"] += 1
        if os.environ.get("OAMD_FORBID_BLAS") == "1":
            raise RuntimeError(f"hipBLASLt fallback for x {tuple(x.shape)} {x.dtype}, w {tuple(w.shape)} "
                               "(OAMD_FORBID_BLAS=1)")
    if out is not None:
        return F.linear(x, w, bias, out=out) if bias is None else out.copy_(F.linear(x, w, bias))
    return F.linear(x, w, bias)


def _launch(plan: Plan, x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None,
            partial: torch.Tensor | None = None, defer_reduce: bool = False, bias=None, silu: bool = False):
    """Run ``plan``: y (``out`` or a fresh tensor), or the fp32 slabs as :class:`SplitK` for a
    deferred split-K plan without ``out``. A split-K call without a large enough ``partial``
    gets a fresh slab buffer every time (captured graphs rely on that)."""
    if plan.kernel == "blas":
        return _blas(x, w, out, bias, plan.planned)
    M, N, S = x.shape[0], w.shape[0], plan.splits
    if S > 1 and (partial is None or partial.numel() < S * M * N):
        partial = torch.empty(S * M * N, dtype=torch.float32, device=x.device)
    slabs = partial if S > 1 else None
    deferred = defer_reduce and S > 1 and out is None
    y = out if out is not None or deferred else torch.empty(M, N // 2 if silu else N, dtype=x.dtype, device=x.device)
    if plan.kernel == "skinny":
        kernels().gemm_skinny(x, w, y, slabs, S, silu)
    elif plan.kernel == "decode":
        kernels().gemm_decode(x, w, y, slabs, S, plan.bn, plan.bm, silu, False, plan.stages)
    elif plan.kernel == "w4":
        kernels().gemm_w4(x, w, y, slabs, S, silu)
    elif plan.kernel == "pp":   # nt weight loads, both K segments, no stream-K workspace
        kernels().gemm_pp(x, w, y, slabs, S, plan.bm, silu, True, False, None, None)
    else:
        kernels().gemm_tile(x, w, y, bias, silu)
    return SplitK(partial, S, M, N) if deferred else y


def _facts(x: torch.Tensor, w: torch.Tensor) -> dict:
    return {"cuda": x.is_cuda, "bf16": x.dtype == torch.bfloat16, "w_bf16": w.dtype == torch.bfloat16,
            "contig": x.is_contiguous() and w.is_contiguous()}


def tile_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """Shapes the 256x256-tile gfx950 GEMM (gemm_tile) takes: bf16, K % 64, N % 16."""
    return x.dim() == 2 and _tile_takes(x.shape[0], w.shape[0], x.shape[1], **_facts(x, w))


def tile_out_ok(out: torch.Tensor | None) -> bool:
    """An explicit output gemm_tile can write: unit column stride, a row stride that is a
    multiple of 4 elements and an 8-byte-aligned base (its epilogue stores 4 bf16 at once);
    anything else falls back instead of tripping the binding's TORCH_CHECK."""
    return out is None or (out.dim() == 2 and out.stride(1) == 1 and out.stride(0) % 4 == 0
                           and out.data_ptr() % 8 == 0 and out.dtype == torch.bfloat16)


def linear_tile(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None,
                bias: torch.Tensor | None = None, silu_gu: bool = False) -> torch.Tensor:
    """Prefill / lm_head GEMM on the compute-bound gfx950 tile kernel (256 x 256 tiles,
    LDS-DMA ping-pong pipeline; fused bias or SwiGLU epilogue)."""
    return _launch(TILE, x, w, out, bias=bias, silu=silu_gu)


def linear(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None, splits: int | None = None,
           partial: torch.Tensor | None = None, bn: int | None = None, bm: int | None = None,
           defer_reduce: bool = False, stages: int | None = None, bias: torch.Tensor | None = None):
    """y = x @ w^T (+ bias) in bf16 as ``route`` plans it: M <= 32 on the weight-streaming gemm_skinny; M % 64 == 0
    up to 256 rows on the tuned table's plan (the LDS-staged split-K gemm_decode, gemm_w4 for a plan tagged "w4",
    gemm_tile / hipBLASLt where measured fastest), else gemm_decode with heuristic splits; everything else (prefill,
    the lm_head, biased projections) on the 256x256-tile gemm_tile; hipBLASLt for shapes none of them takes or under
    OAMD_PREFILL_BLAS=1; CPU tensors on torch. ``splits`` / ``bn`` / ``bm`` / ``stages`` override the plan (tests /
    tuning); ``defer_reduce`` leaves a split-K plan's fp32 slabs (:class:`SplitK`) to the consumer."""
    plan = route(x.shape[0], w.shape[0], x.shape[1], bias=bias is not None, out_ok=tile_out_ok(out),
                 splits=splits, bn=bn, bm=bm, stages=stages, prefill_blas=PREFILL_BLAS, **_facts(x, w))
    return _launch(plan, x, w, out, partial, defer_reduce, bias)


def interleave_gate_up(g: torch.Tensor, u: torch.Tensor, block: int = GU_BLOCK) -> torch.Tensor:
    """[g; u] rows -> blocks of ``block`` gate rows followed by the same features' up rows."""
    inter, H = g.shape
    return torch.stack([g.reshape(inter // block, block, H), u.reshape(inter // block, block, H)], 1).reshape(
        2 * inter, H).contiguous()


def gate_up_silu(x: torch.Tensor, wgu: torch.Tensor, block: int | None) -> torch.Tensor:
    """silu(x Wg^T) * (x Wu^T) from the interleaved gate|up weight. Decode buckets and prefill
    run one fused gfx950 kernel (GEMM + SwiGLU epilogue, no [M, 2I] intermediate);
    other shapes run the GEMM then the silu_mul kernel."""
    plan = route(x.shape[0], wgu.shape[0], x.shape[1], silu=True, block=block, **_facts(x, wgu))
    if plan is not None:
        return _launch(plan, x, wgu, silu=True)
    from . import silu_mul
    return silu_mul(linear(x, wgu), block=block)
