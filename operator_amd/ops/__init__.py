"""Device ops of the explanation model and the log scanner.

GPU tensors always go to the hand-written gfx950 kernels in ``operator_amd._C``
(loading fails loudly if the extension is missing); CPU tensors use the fp32
reference implementations in :mod:`operator_amd.ops.reference`.
"""
from __future__ import annotations

import os

import torch

from . import reference
from ._native import kernels, native_available, patterns
# the bf16 GEMMs (plan, then launch) live in ops/gemm.py
from .gemm import (BLAS_CALLS, BLAS_PLANNED, GEMM_DECODE_M, GU_BLOCK, LM_HEAD_MIN_N, PREFILL_BLAS, SKINNY_MAX_M,
                   SplitK, gate_up_silu, gemm_plan, gemm_table, interleave_gate_up, linear, linear_tile, row_tile,
                   skinny_plan, tile_ok, tile_out_ok)

__all__ = [
    "rmsnorm", "silu_mul", "embedding", "rope_kv", "attn_prefill", "attn_decode", "attn_decode_rope", "sample",
    "sample_threshold", "penalty_seed", "sample_penalty", "sample_logprobs", "LOGPROBS_MAX",
    "kernels", "patterns", "native_available", "reference", "prefill_work_list", "prefill_block_q", "prefill_variant", "decode_splits",
    "decode_workspace", "linear", "gemm_plan", "gemm_table", "gate_up_silu", "interleave_gate_up",
    "quantize_fp8", "silu_quantize_fp8", "linear_fp8", "fp8_plan", "SplitK", "linear_tile", "tile_ok", "BLAS_CALLS",
    "skinny_plan", "row_tile", "tile_out_ok", "GU_BLOCK", "GEMM_DECODE_M", "SKINNY_MAX_M", "LM_HEAD_MIN_N",
    "BLAS_PLANNED", "PREFILL_BLAS",
]

# never split a sequence into pieces shorter than this / split only while B x Hkv
# decode-attention workgroups < this (env overrides for tuning runs)
DECODE_MIN_SPLIT_TOKENS = int(os.environ.get("OAMD_DECODE_MIN_SPLIT", "256"))
# one workgroup per CU: the best split count at every measured (B, group, ctx) of
# profiles/attn_decode_splits_sweep_r5.jsonl lands at B x Hkv x splits ~ 256
DECODE_TARGET_BLOCKS = int(os.environ.get("OAMD_DECODE_TARGET_BLOCKS", "256"))
# attn_decode schedule bits (csrc/kernels/attn_decode.hip): 2 = NT 2 (two 16-token tiles per wave),
# 4 = one kv-head across all sequences first (else a sequence's kv-heads back to back)
DECODE_ATTN_VARIANT = int(os.environ.get("OAMD_DECODE_ATTN_VARIANT", "0"))


def _input_or_slabs(x):
    """``(bf16 input, slabs, splits)`` as the bindings take a consumer's input: exactly one of the
    first two (:class:`SplitK`: the slabs, summed inside the kernel)."""
    return (None, x.p, x.S) if isinstance(x, SplitK) else (x, None, 1)


def rmsnorm(x, w: torch.Tensor, eps: float, residual: torch.Tensor | None = None,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """RMSNorm; if ``residual`` is given it is updated in place to x + residual first.
    ``x`` may be a :class:`SplitK` (slabs summed inside the kernel)."""
    if isinstance(x, SplitK):
        M, N = x.shape
        y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        kernels().rmsnorm(None, residual, w, y, eps, x.p, x.S)
        return y
    if not x.is_cuda:
        y, r = reference.rmsnorm(x, w, eps, residual)
        if residual is not None:
            residual.copy_(r)
        if out is not None:
            out.copy_(y)
            return out
        return y
    y = out if out is not None else torch.empty_like(x)
    kernels().rmsnorm(x, residual, w, y, eps)
    return y


def silu_mul(gu: torch.Tensor, out: torch.Tensor | None = None, block: int | None = None) -> torch.Tensor:
    """silu(gate) * up for gate|up interleaved in ``block``-feature blocks (None: [gate | up])."""
    if not gu.is_cuda:
        r = reference.silu_mul(gu, block)
        if out is not None:
            out.copy_(r)
            return out
        return r
    inter = gu.shape[1] // 2
    o = out if out is not None else torch.empty(gu.shape[0], inter, dtype=gu.dtype, device=gu.device)
    kernels().silu_mul(gu, o, block or 0)
    return o


def embedding(ids: torch.Tensor, table: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    if not ids.is_cuda:
        r = reference.embedding(ids, table)
        if out is not None:
            out.copy_(r)
            return out
        return r
    o = out if out is not None else torch.empty(ids.numel(), table.shape[1], dtype=table.dtype, device=ids.device)
    kernels().embedding(ids, table, o)
    return o


def rope_kv(qkv: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, Hq: int, Hkv: int,
            k_cache: torch.Tensor | None = None, v_cache: torch.Tensor | None = None,
            slots: torch.Tensor | None = None, want_kv: bool = True,
            q_out: torch.Tensor | None = None, bias: torch.Tensor | None = None,
            k_scale: float = 1.0, v_scale: float = 1.0):
    """Rotate q/k of the packed qkv rows and scatter k/v into the paged cache.
    ``bias`` [(Hq + 2 Hkv) D] is added to the projection first (Qwen2); with split-K
    slabs it is added before the single bf16 rounding. An e4m3fn cache stores
    x / k_scale, x / v_scale.

    Returns (q [T,Hq,D], k [T,Hkv,D] | None, v [T,Hkv,D] | None).
    """
    slabs = isinstance(qkv, SplitK)
    if not slabs and not qkv.is_cuda:
        if bias is not None:
            qkv = (qkv.float() + bias.float()).to(qkv.dtype)
        q, k, v = reference.rope_kv(qkv, pos, cos, sin, Hq, Hkv, k_cache, v_cache, slots, k_scale, v_scale)
        if q_out is not None:
            q_out.copy_(q.reshape(q_out.shape))
            q = q_out
        return q, (k if want_kv else None), (v if want_kv else None)
    T = qkv.shape[0]
    D = cos.shape[1] * 2
    dt, dev = torch.bfloat16 if slabs else qkv.dtype, qkv.device
    q = q_out if q_out is not None else torch.empty(T, Hq, D, dtype=dt, device=dev)
    k = torch.empty(T, Hkv, D, dtype=dt, device=dev) if want_kv else None
    v = torch.empty(T, Hkv, D, dtype=dt, device=dev) if want_kv else None
    x, p, S = _input_or_slabs(qkv)
    kernels().rope_kv(x, pos, cos, sin, Hq, Hkv, q, k, v, k_cache, v_cache, slots, p, S, bias, k_scale, v_scale)
    return q, k, v


# v3 schedule options (csrc/kernels/attn_prefill.hip OPT bits): l = K/V loads after the
# S MFMAs, r = deferred rescale, d = two LDS tile buffers (one barrier per tile)
_PREFILL_VARIANTS = {"v1": 1, "v2": 2, "v3": 3, "v4": 4}


def prefill_variant(Hq: int, Hkv: int) -> int:
    """attn_prefill kernel variant: 1 = per-query-head (any G), 2 = GQA-grouped 16-row waves
    (G = Hq / Hkv in 1, 2, 4, 8), 3 = GQA-grouped swapped-operand 32x32 MFMA waves in 8-wave
    workgroups (G <= 8), 4 = the same waves in 4-wave workgroups, two per CU (G <= 4;
    profiles/prefill_attn_v3_vs_v4.jsonl: 6-9 % faster at 16x1024 and mixed lengths, equal at
    4x4096). Default: v4 where G <= 4, else v3. OAMD_PREFILL_ATTN=v1|v2|v3|v4 overrides it; a
    grouped variant that cannot take G falls back to v3, then v1."""
    G = Hq // Hkv if Hkv and Hq % Hkv == 0 else 0
    want = _PREFILL_VARIANTS.get(os.environ.get("OAMD_PREFILL_ATTN", ""), 4 if 1 <= G <= 4 else 3)
    if want == 2 and G not in (1, 2, 4, 8):
        want = 3
    if want == 4 and G > 4:
        want = 3
    return want if 1 <= G <= 8 else 1


def prefill_block_q(Hq: int, Hkv: int, variant: int | None = None) -> int:
    """Query rows per attn_prefill work item: 64 (v1), 16 x (8 / G) (v2), 32 x (8 / G) (v3),
    32 x (4 / G) (v4)."""
    v = prefill_variant(Hq, Hkv) if variant is None else variant
    if v == 1:
        return 64
    G = Hq // Hkv
    return (16 if v == 2 else 32) * ((4 if v == 4 else 8) // G)


def prefill_work_list(seq_lens: list[int], block_q: int = 64) -> tuple[list[int], list[int]]:
    """(work_seq, work_q0) for attn_prefill: one item per ``block_q``-row query block; longest first."""
    items = []
    for s, L in enumerate(seq_lens):
        for q0 in range(0, L, block_q):
            items.append((q0, s))
    items.sort(key=lambda t: -t[0])  # heavy (late, long-causal) blocks first
    return [s for _, s in items], [q0 for q0, _ in items]


def attn_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_lens: list[int], scale: float,
                 out: torch.Tensor | None = None, work: tuple[torch.Tensor, torch.Tensor, torch.Tensor] | None = None,
                 prefix: tuple | None = None):
    """Causal attention over packed sequences (q [T,Hq,D], k/v [T,Hkv,D]).

    ``prefix`` = (pk, pv, seq_pfx, pfx_lens): a shared prompt prefix (LLMEngine prefix
    sharing) whose cached K/V rows pk / pv [P, Hkv, D] come before sequence s's own keys
    for its first pfx_lens[s] keys (<= P); the own query rows sit at
    positions pfx_lens[s] + row and see every prefix key. seq_pfx: the same lengths as an
    int32 device tensor (GPU), pfx_lens: as a host list (CPU reference; may be None on
    the GPU)."""
    cu = [0]
    for L in seq_lens:
        cu.append(cu[-1] + int(L))
    if not q.is_cuda:
        r = reference.attn_prefill(q, k, v, cu, scale,
                                   prefix=None if prefix is None else (prefix[0], prefix[1], prefix[3]))
        if out is not None:
            out[:cu[-1]].copy_(r[:cu[-1]])   # like the kernels: rows past the last sequence are not written
            return out
        return r
    o = out if out is not None else torch.empty_like(q)
    if work is None:
        var = prefill_variant(q.shape[1], k.shape[1])
        ws, wq = prefill_work_list([int(x) for x in seq_lens], prefill_block_q(q.shape[1], k.shape[1], var))
        dev = q.device
        work = (torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(ws, dtype=torch.int32, device=dev),
                torch.tensor(wq, dtype=torch.int32, device=dev), var)
    # work = (cu_seqlens, work_seq, work_q0, variant); the work list must be cut at that variant's block_q
    var = work[3] if len(work) > 3 else 1
    if prefix is not None:
        if var not in (3, 4):
            raise ValueError("a shared prefix needs attn_prefill variant 3 or 4")
        kernels().attn_prefill(q, k, v, o, work[0], work[1], work[2], scale, var, prefix[0], prefix[1], prefix[2])
    else:
        kernels().attn_prefill(q, k, v, o, work[0], work[1], work[2], scale, var)
    return o


FP8_MAX = 448.0  # OCP e4m3fn


def quantize_fp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-row e4m3fn quantization: (q [M, K] float8_e4m3fn, s [M] fp32), x ~= q * s."""
    M, K = x.shape
    if x.is_cuda and x.dtype == torch.bfloat16 and K % 8 == 0:
        q = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=x.device)
        sx = torch.empty(M, dtype=torch.float32, device=x.device)
        kernels().quantize_fp8(x.contiguous(), q, sx)
        return q, sx
    xf = x.float()
    amax = xf.abs().amax(1)
    sx = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    return (xf / sx[:, None]).to(torch.float8_e4m3fn), sx


def silu_quantize_fp8(gu, block: int | None = GU_BLOCK) -> tuple[torch.Tensor, torch.Tensor]:
    """quantize_fp8(silu_mul(gu, block)) — on the GPU one kernel for 64-feature
    interleaved gate|up rows (the SwiGLU never round-trips HBM as bf16). ``gu`` may be
    the gate|up GEMM's split-K slabs (:class:`SplitK`), summed inside the kernel."""
    M, N2 = gu.shape
    inter = N2 // 2
    slabs = isinstance(gu, SplitK)
    if (slabs or (gu.is_cuda and gu.stride(1) == 1)) and block == GU_BLOCK and inter <= 16384 and N2 % 128 == 0:
        q = torch.empty(M, inter, dtype=torch.float8_e4m3fn, device=gu.device)
        sx = torch.empty(M, dtype=torch.float32, device=gu.device)
        x, p, S = _input_or_slabs(gu)
        kernels().silu_quantize_fp8(x, q, sx, p, S)
        return q, sx
    if slabs:
        gu = gu.materialize()
    return quantize_fp8(silu_mul(gu, block=block))


def _fp8_overrides() -> dict:
    """OAMD_FP8_PLANS="NxK=bm,bn,S;..." (A/B of fp8 decode plans): (N, K) -> (bm, bn, S)."""
    out = {}
    for item in filter(None, os.environ.get("OAMD_FP8_PLANS", "").split(";")):
        shape, plan = item.split("=")
        n, k = (int(v) for v in shape.split("x"))
        out[(n, k)] = tuple(int(v) for v in plan.split(","))
    return out


_FP8_OVERRIDES = _fp8_overrides()


def fp8_plan(M: int, N: int, K: int) -> tuple[int, int, int]:
    """(bm, bn, splits) for gemm_fp8: row tile by M, 128-column tiles for wide N, and
    split-K until the blocks reach one per CU (K permitting)."""
    if (N, K) in _FP8_OVERRIDES:
        return _FP8_OVERRIDES[(N, K)]
    bm = 64 if M <= 64 else 128 if M <= 128 else 256
    bn = 128 if N % 128 == 0 and N // 128 >= 192 else 64
    mt = -(-M // bm)
    S = 1
    for s in (1, 2, 4, 8):
        if K % (128 * s):
            break
        S = s
        if (N // bn) * s * mt >= 256:
            break
    return bm, bn, S


def linear_fp8(x: torch.Tensor | tuple[torch.Tensor, torch.Tensor], w8: torch.Tensor, sw: torch.Tensor,
               out: torch.Tensor | None = None, plan: tuple[int, int, int] | None = None,
               defer_reduce: bool = False):
    """y = x @ (w8 * sw)^T with x quantized per token to e4m3fn (W8A8, fp32 accumulate).
    ``x`` may already be quantized: a (q, sx) pair from quantize_fp8 / silu_quantize_fp8.
    ``defer_reduce``: a split-K plan returns its fp32 slabs (:class:`SplitK`) for a
    consumer that sums them (rope_kv, rmsnorm, the fused all-reduce + norm, SwiGLU)."""
    q, sx = x if isinstance(x, tuple) else quantize_fp8(x)
    M, K = q.shape
    N = w8.shape[0]
    if not q.is_cuda:
        y = (q.float() * sx[:, None]) @ (w8.float() * sw[:, None]).t()
        return out.copy_(y) if out is not None else y.to(torch.bfloat16 if isinstance(x, tuple) else x.dtype)
    bm, bn, S = plan or fp8_plan(M, N, K)
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=q.device)
    part = torch.empty(S * M * N, dtype=torch.float32, device=q.device) if S > 1 else None
    if defer_reduce and S > 1 and out is None:
        kernels().gemm_fp8(q, w8, sx, sw, y, part, S, bn, bm, False)
        return SplitK(part, S, M, N)
    kernels().gemm_fp8(q, w8, sx, sw, y, part, S, bn, bm)
    return y


def decode_splits(max_context: int, batch: int = 1, kv_heads: int = 8) -> int:
    """Workgroups per (sequence, kv-head) for decode attention: split only while
    ``batch * kv_heads`` workgroups cannot fill the GPU, never into pieces shorter
    than 256 tokens (measured on MI355X, B=16 ctx=1024: 1 split 25.9 us, 4 splits
    23.7 us, 16 splits 47.8 us). Powers of two, so a graph captured per value
    covers every context length with few captures."""
    want = -(-DECODE_TARGET_BLOCKS // max(1, batch * kv_heads))
    cap = -(-max(1, int(max_context)) // DECODE_MIN_SPLIT_TOKENS)
    ns = max(1, min(want, cap, 256))
    # the power of two at or BELOW: splits of 256-512 tokens, not 128-256 (B = 64, one kv-head,
    # ctx 1100: 4 splits 15.2 us vs 8 splits 19.9 us with the combine, profiles/attn_decode_tp8_splits_r5.jsonl)
    return 1 << (ns.bit_length() - 1)


def decode_workspace(B: int, Hq: int, num_splits: int, device, D: int = 128):
    """(o_part fp32, ml_part fp32) partial buffers for attn_decode (unused when num_splits == 1)."""
    n = max(1, B * Hq * num_splits) if num_splits > 1 else 1
    return (torch.empty(n * D, dtype=torch.float32, device=device),
            torch.empty(n * 2, dtype=torch.float32, device=device))


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                seq_lens: torch.Tensor, scale: float, num_splits: int, out: torch.Tensor | None = None,
                workspace: tuple[torch.Tensor, torch.Tensor] | None = None, variant: int | None = None,
                k_scale: float = 1.0, v_scale: float = 1.0, quant: bool = False):
    """Paged decode attention; ``num_splits`` workgroups per (sequence, kv-head)
    (``decode_splits``). Any value >= 1 is correct; it only changes the schedule.
    The cache is bf16, or e4m3fn holding x / k_scale and x / v_scale.
    ``quant``: return the [B, Hq*D] output rows as per-token e4m3fn ``(q, sx)`` for an
    fp8 o-projection, produced by the split-combine kernel itself (== quantize_fp8)."""
    if not q.is_cuda:
        r = reference.attn_decode(q, k_cache, v_cache, block_tables, seq_lens, scale, k_scale, v_scale)
        if out is not None:
            out.copy_(r)
            r = out
        return quantize_fp8(r.reshape(r.shape[0], -1)) if quant else r
    return _attn_decode_launch(q, q.shape, k_cache, v_cache, block_tables, seq_lens, scale, num_splits, out,
                               workspace, variant, k_scale, v_scale, quant)


def _attn_decode_launch(q, shape, k_cache, v_cache, block_tables, seq_lens, scale, num_splits, out, workspace,
                        variant, k_scale, v_scale, quant, rope=()):
    """The output / workspace / q8 allocation and the launch of ``attn_decode`` (``q`` rotated) and
    ``attn_decode_rope`` (``q`` None; ``rope``: the binding's fused-RoPE arguments)."""
    B, Hq, D = shape
    dev = k_cache.device
    variant = DECODE_ATTN_VARIANT if variant is None else variant
    o = out if out is not None else torch.empty(B, Hq, D, dtype=torch.bfloat16, device=dev)
    if workspace is None:
        workspace = decode_workspace(B, Hq, num_splits, dev)
    q8 = sx = None
    if quant:
        q8 = torch.empty(B, Hq * D, dtype=torch.float8_e4m3fn, device=dev)
        sx = torch.empty(B, dtype=torch.float32, device=dev)
    kernels().attn_decode(q, k_cache, v_cache, block_tables, seq_lens, o, workspace[0], workspace[1],
                          num_splits, scale, variant, k_scale, v_scale, q8, sx, *rope)
    return (q8, sx) if quant else o


# decode RoPE + KV-cache write folded into decode attention (OAMD_FUSED_ROPE=0: rope_kv, then attn_decode),
# for batches of at most FUSED_ROPE_MAX_SEQ_HEADS (sequence, kv-head) pairs: there attention is
# latency-bound and the fold removes a launch (TP=8 70B fp8 B=64: 6.85 -> 6.64 ms/step); at the
# 8B flagship's 256 x 8 pairs attention streams HBM and every workgroup would pay the fold's
# slab reads and store drain up front (-1.3 % analyses/s, profiles/fused_decode_rope_ab_r5.jsonl)
FUSED_DECODE_ROPE = os.environ.get("OAMD_FUSED_ROPE", "1") != "0"
FUSED_ROPE_MAX_SEQ_HEADS = int(os.environ.get("OAMD_FUSED_ROPE_MAX", "256"))


def attn_decode_rope(qkv, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, Hq: int, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, slots: torch.Tensor, block_tables: torch.Tensor, seq_lens: torch.Tensor,
                     scale: float, num_splits: int, workspace: tuple[torch.Tensor, torch.Tensor] | None = None,
                     bias: torch.Tensor | None = None, k_scale: float = 1.0, v_scale: float = 1.0,
                     quant: bool = False, variant: int | None = None):
    """One decode step's ``rope_kv`` (want_kv=False) + ``attn_decode`` as ONE kernel: every
    attention workgroup rotates its q from the QKV projection (``qkv``: bf16 rows or the
    GEMM's :class:`SplitK` slabs, + the Qwen2 bias), and the workgroup holding each
    sequence's last token writes that token's rotated K and its V into the cache before
    reading it (csrc/kernels/attn_decode.hip, ``DecRope``). Same numerics as the two
    kernels; one launch and the q round trip fewer per layer."""
    Hkv = k_cache.shape[1]
    on_gpu = isinstance(qkv, SplitK) or qkv.is_cuda
    if not (on_gpu and FUSED_DECODE_ROPE and qkv.shape[0] * Hkv <= FUSED_ROPE_MAX_SEQ_HEADS):
        q, _, _ = rope_kv(qkv, pos, cos, sin, Hq, Hkv, k_cache, v_cache, slots, want_kv=False, bias=bias,
                          k_scale=k_scale, v_scale=v_scale)
        return attn_decode(q, k_cache, v_cache, block_tables, seq_lens, scale, num_splits, workspace=workspace,
                           variant=variant, k_scale=k_scale, v_scale=v_scale, quant=quant)
    return _attn_decode_launch(None, (qkv.shape[0], Hq, cos.shape[1] * 2), k_cache, v_cache, block_tables, seq_lens,
                               scale, num_splits, None, workspace, variant, k_scale, v_scale, quant,
                               rope=(*_input_or_slabs(qkv), pos, cos, sin, slots, bias))


def sample_threshold(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                     out: torch.Tensor | None = None, out_kept: torch.Tensor | None = None) -> torch.Tensor:
    """Top-k / top-p as one fp32 threshold per row: the candidates of row r are the columns
    with logit >= thr[r] (semantics: ``reference.sample_threshold``). ``top_k`` int32 (0 = off),
    ``top_p`` fp32 (1 = off); greedy rows and rows with both off get -inf without their logits
    being read. ``out_kept`` (int32) receives the number of candidates."""
    rows = logits.shape[0]
    if not logits.is_cuda:
        thr, kept = reference.sample_threshold(logits, temperature, top_k, top_p)
        if out_kept is not None:
            out_kept.copy_(kept)
        if out is not None:
            out.copy_(thr)
            return out
        return thr
    o = out if out is not None else torch.empty(rows, dtype=torch.float32, device=logits.device)
    kernels().sample_threshold(logits, temperature, top_k, top_p, o, out_kept)
    return o


def penalty_seed(table, slots: torch.Tensor, ids: torch.Tensor, cu: torch.Tensor) -> None:
    """Clear the penalty-table slots ``slots`` (int32) and flag the tokens of their requests'
    whole prompts: ``ids`` (int64) packed, request b's at ``ids[cu[b]:cu[b + 1]]`` (``cu`` int32).
    ``table``: the ``cnt`` / ``lst`` / ``n`` tensors (models/penalty.py PenaltyTable). Slots are
    distinct; semantics: ``reference.penalty_seed``."""
    if not table.cnt.is_cuda:
        reference.penalty_seed(table.cnt, table.lst, table.n, slots, ids, cu)
        return
    kernels().penalty_seed(slots, ids, cu, table.cnt, table.lst, table.n)


def sample_penalty(logits: torch.Tensor, pslot: torch.Tensor, last_tok: torch.Tensor | None,
                   ctx: torch.Tensor | None, rep: torch.Tensor, freq: torch.Tensor, pres: torch.Tensor,
                   table) -> torch.Tensor:
    """Repetition / frequency / presence penalties on ``logits`` [rows, vocab] in place, before
    temperature and top-k / top-p (semantics: ``reference.sample_penalty``). Row i uses slot
    ``pslot[i]`` (int32; < 0: no penalty, the row is not read) of ``table``; ``rep`` / ``freq`` /
    ``pres`` fp32 per row. With ``last_tok`` (int64 per row: the last sampled token, which a
    decode step feeds in) that token is counted first; ``ctx`` (int32 per row) == 0 marks a
    padding row. Each slot appears on at most one row."""
    if not logits.is_cuda:
        reference.sample_penalty(logits, pslot, last_tok, ctx, rep, freq, pres, table.cnt, table.lst, table.n)
        return logits
    kernels().sample_penalty(logits, pslot, last_tok, ctx, rep, freq, pres, table.cnt, table.lst, table.n)
    return logits


LOGPROBS_MAX = reference.LOGPROBS_MAX   # most likely tokens reported per position (kernels.h kLogprobsMax)


def sample_logprobs(logits: torch.Tensor, nlp: torch.Tensor, ctx: torch.Tensor | None, tokens: torch.Tensor,
                    step: torch.Tensor | None, tok_lp: torch.Tensor, top_lp: torch.Tensor,
                    top_id: torch.Tensor) -> None:
    """Log-probabilities (log-softmax at temperature 1 of ``logits`` [rows, vocab] as they are:
    after the penalties, before temperature and top-k / top-p) of the sampled ``tokens`` (int64
    per row) and of each row's ``nlp[i]`` (int32; 0..LOGPROBS_MAX) most likely tokens; semantics:
    ``reference.sample_logprobs``. A row with ``nlp[i]`` < 0, or with ``ctx[i]`` (int32 per row) ==
    0, is not read. Written at column ``step[0] % C`` (``step`` int64 [1]; None: column 0) of
    ``tok_lp`` fp32 [rows, C], ``top_lp`` fp32 and ``top_id`` int32 [rows, C, LOGPROBS_MAX]: the
    token's value and the first ``nlp[i]`` list entries, nothing else. It only reads ``logits``."""
    if not logits.is_cuda:
        reference.sample_logprobs(logits, nlp, ctx, tokens, step, tok_lp, top_lp, top_id)
        return
    kernels().sample_logprobs(logits, nlp, ctx, tokens, step, tok_lp, top_lp, top_id)


def sample(logits: torch.Tensor, temperature: torch.Tensor, seeds: torch.Tensor, positions: torch.Tensor,
           out: torch.Tensor | None = None, col_offset: int = 0, out_val: torch.Tensor | None = None,
           top_k: torch.Tensor | None = None, top_p: torch.Tensor | None = None,
           thr: torch.Tensor | None = None) -> torch.Tensor:
    """Temperature / Gumbel-max sampling (greedy rows where temperature <= 0).

    For a vocab shard pass ``col_offset`` (global id of column 0) and ``out_val``
    (receives each row's winning perturbed value) and take the max over shards.

    ``top_k`` (int32, 0 = off) / ``top_p`` (fp32, 1 = off), one per row: ``sample_threshold``
    into ``thr`` (a buffer of the caller's, for graph capture, or a fresh one), then the sampler
    restricted to the columns with logit >= thr[row]. With ``thr`` alone the sampler is
    restricted by the thresholds the caller computed; that is the only filtered form a vocab
    shard can use (its own logits cannot give the global threshold), so ``top_k`` / ``top_p``
    with a ``col_offset`` raise.
    """
    rows = logits.shape[0]
    if top_k is not None or top_p is not None:
        if col_offset != 0:
            raise ValueError("top_k / top_p on a vocab shard (col_offset != 0) need a global threshold: pass thr")
        if top_k is None:
            top_k = torch.zeros(rows, dtype=torch.int32, device=logits.device)
        if top_p is None:
            top_p = torch.ones(rows, dtype=torch.float32, device=logits.device)
        thr = sample_threshold(logits, temperature, top_k, top_p, out=thr)
    if not logits.is_cuda:
        tok, val = reference.sample_shard(logits, temperature, seeds, positions, col_offset, thr=thr)
        if out_val is not None:
            out_val.copy_(val)
        if out is not None:
            out.copy_(tok)
            return out
        return tok
    o = out if out is not None else torch.empty(rows, dtype=torch.long, device=logits.device)
    if thr is None:
        kernels().sample(logits, temperature, seeds, positions, o, col_offset, out_val)
    else:
        kernels().sample(logits, temperature, seeds, positions, o, col_offset, out_val, thr)
    return o
