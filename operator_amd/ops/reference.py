"""Plain-PyTorch fp32 reference implementations of every HIP kernel.

These define the numerics each gfx950 kernel is tested against (tests/test_kernels_gpu.py)
and are what runs when a model is executed on CPU (the CPU test tier, gloo
multi-process TP tests). They are intentionally simple and unfused.
"""
from __future__ import annotations

import math

import torch


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, residual: torch.Tensor | None = None):
    """y = rmsnorm(x [+ residual]); returns (y, new_residual). HF Llama numerics."""
    if residual is not None:
        x = (x.float() + residual.float()).to(x.dtype)
        new_res = x
    else:
        new_res = None
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    y = (xf * torch.rsqrt(var + eps)).to(x.dtype)
    return (y.float() * w.float()).to(x.dtype), new_res


def silu_mul(gu: torch.Tensor, block: int | None = None) -> torch.Tensor:
    """silu(gate) * up; gate|up columns interleaved in blocks of ``block`` features
    (None: the plain [gate | up] concatenation)."""
    inter = gu.shape[-1] // 2
    if block and block != inter:
        v = gu.reshape(*gu.shape[:-1], inter // block, 2, block)
        g, u = v[..., 0, :].reshape(*gu.shape[:-1], inter), v[..., 1, :].reshape(*gu.shape[:-1], inter)
    else:
        g, u = gu[..., :inter], gu[..., inter:]
    s = torch.nn.functional.silu(g.float()).to(gu.dtype)
    return (s.float() * u.float()).to(gu.dtype)


def embedding(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    return table[ids.clamp(0, table.shape[0] - 1)]


def rope_tables(max_pos: int, head_dim: int, theta: float, scaling: dict | None = None,
                device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """fp32 cos/sin tables [max_pos, head_dim/2]; supports Llama-3.1 'llama3' scaling."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo, hi = scaling.get("low_freq_factor", 1.0), scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        mid = (wl <= lo_wl) & (wl >= hi_wl)
        inv = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def apply_rope(x: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [T, H, D] -> rotate-half RoPE at positions pos [T]."""
    half = x.shape[-1] // 2
    c = cos[pos].unsqueeze(1)
    s = sin[pos].unsqueeze(1)
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


K_TILE = 16  # tokens per K-cache tile


def k_tile_index(D: int = 128) -> torch.Tensor:
    """Physical offset inside a [16 tokens x D] K-cache tile of logical element (t, d).

    K is stored so that each MFMA fragment load of the decode-attention kernel is
    one contiguous 1 KB wave access: a tile is [ks 4][lg 4][token 16][8 dims]
    with d = 32*lg + 8*ks + j (lg = lane >> 4 group, ks = k-step) — instead of
    16 token rows x 64 B per instruction. V keeps the row layout."""
    t = torch.arange(K_TILE)[:, None]
    d = torch.arange(D)[None, :]
    lg, ks, j = d // 32, (d % 32) // 8, d % 8
    return ((ks * 4 + lg) * K_TILE + t) * 8 + j


def k_cache_logical(k_cache: torch.Tensor) -> torch.Tensor:
    """[pages, Hkv, P, D] tiled K cache -> logical (token-row) copy."""
    pages, Hkv, P, D = k_cache.shape
    idx = k_tile_index(D).flatten().to(k_cache.device)
    return k_cache.reshape(pages, Hkv, P // K_TILE, K_TILE * D)[..., idx].reshape(pages, Hkv, P, D)


def k_cache_write(k_cache: torch.Tensor, page: int, off: int, k: torch.Tensor) -> None:
    """k_cache[page, :, off] = k ([Hkv, D]) in the tiled K layout."""
    pages, Hkv, P, D = k_cache.shape
    idx = k_tile_index(D)[off % K_TILE].to(k_cache.device)
    k_cache.view(pages, Hkv, P // K_TILE, K_TILE * D)[page, :, off // K_TILE, idx] = k


FP8_KV_MAX = 448.0  # OCP e4m3fn


def kv_store(x: torch.Tensor, cache_dtype: torch.dtype, scale: float) -> torch.Tensor:
    """Value as held by a cache of ``cache_dtype``: as is, or e4m3fn(x / scale) saturated."""
    if cache_dtype == torch.float8_e4m3fn:
        return (x.float() / scale).clamp(-FP8_KV_MAX, FP8_KV_MAX).to(torch.float8_e4m3fn)
    return x.to(cache_dtype)


def kv_load(c: torch.Tensor, scale: float) -> torch.Tensor:
    """fp32 view of cache contents (fp8 caches dequantised by their scale)."""
    return c.float() * scale if c.dtype == torch.float8_e4m3fn else c.float()


def rope_kv(qkv: torch.Tensor, pos: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, Hq: int, Hkv: int,
            k_cache: torch.Tensor | None = None, v_cache: torch.Tensor | None = None,
            slots: torch.Tensor | None = None, k_scale: float = 1.0, v_scale: float = 1.0):
    """Split packed qkv, rotate q/k, optionally scatter k/v into the paged cache.

    Cache layout [pages, Hkv, page, D] (K tiled, see k_tile_index; V row-major);
    slot = page*page_size + offset; slot < 0 skips.
    Returns (q [T,Hq,D], k [T,Hkv,D], v [T,Hkv,D]).
    """
    T = qkv.shape[0]
    D = cos.shape[1] * 2
    q = qkv[:, : Hq * D].reshape(T, Hq, D)
    k = qkv[:, Hq * D: (Hq + Hkv) * D].reshape(T, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D:].reshape(T, Hkv, D)
    q = apply_rope(q, pos, cos, sin)
    k = apply_rope(k, pos, cos, sin)
    if k_cache is not None:
        P = k_cache.shape[2]
        for t in range(T):
            s = int(slots[t])
            if s < 0:
                continue
            k_cache_write(k_cache, s // P, s % P, kv_store(k[t], k_cache.dtype, k_scale))
            v_cache[s // P, :, s % P] = kv_store(v[t], v_cache.dtype, v_scale)
    return q, k.contiguous(), v.contiguous()


def attn_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens: list[int] | torch.Tensor,
                 scale: float, prefix: tuple | None = None) -> torch.Tensor:
    """Causal GQA attention over packed variable-length sequences. q [T,Hq,D], k/v [T,Hkv,D].
    ``prefix`` = (pk, pv, lens): sequence i's keys start with the rows pk[:lens[i]] /
    pv[:lens[i]] (a cached shared prompt prefix), visible to all of its query rows."""
    cu = [int(x) for x in cu_seqlens]
    Hq, Hkv = q.shape[1], k.shape[1]
    G = Hq // Hkv
    out = torch.empty_like(q)
    for i in range(len(cu) - 1):
        a, b = cu[i], cu[i + 1]
        if b == a:
            continue
        pl = int(prefix[2][i]) if prefix is not None else 0
        kk, vv = k[a:b], v[a:b]
        if pl:
            kk, vv = torch.cat([prefix[0][:pl].to(k.dtype), kk]), torch.cat([prefix[1][:pl].to(v.dtype), vv])
        qs = q[a:b].float().transpose(0, 1)                      # [Hq, L, D]
        ks = kk.float().transpose(0, 1).repeat_interleave(G, 0)
        vs = vv.float().transpose(0, 1).repeat_interleave(G, 0)
        s = torch.matmul(qs, ks.transpose(1, 2)) * scale
        L = b - a
        mask = torch.ones(L, L, dtype=torch.bool, device=q.device).triu(1)
        if pl:
            mask = torch.cat([torch.zeros(L, pl, dtype=torch.bool, device=q.device), mask], 1)
        s.masked_fill_(mask, float("-inf"))
        p = torch.softmax(s, -1)
        out[a:b] = torch.matmul(p, vs).transpose(0, 1).to(q.dtype)
    return out


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                seq_lens: torch.Tensor, scale: float, k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """One query token per sequence over a paged cache [pages, Hkv, page, D] (K tiled;
    bf16, or e4m3fn holding x / scale)."""
    B, Hq, D = q.shape
    Hkv, P = k_cache.shape[1], k_cache.shape[2]
    k_cache = k_cache_logical(k_cache)
    G = Hq // Hkv
    out = torch.zeros_like(q)
    for b in range(B):
        L = min(int(seq_lens[b]), block_tables.shape[1] * P)   # a length above the table's capacity is clamped
        if L <= 0:
            continue
        npg = (L + P - 1) // P
        pages = block_tables[b, :npg].long()
        ks = kv_load(k_cache[pages].permute(1, 0, 2, 3).reshape(Hkv, npg * P, D)[:, :L], k_scale)
        vs = kv_load(v_cache[pages].permute(1, 0, 2, 3).reshape(Hkv, npg * P, D)[:, :L], v_scale)
        ks = ks.repeat_interleave(G, 0)
        vs = vs.repeat_interleave(G, 0)
        s = torch.einsum("hd,hld->hl", q[b].float(), ks) * scale
        p = torch.softmax(s, -1)
        out[b] = torch.einsum("hl,hld->hd", p, vs).to(q.dtype)
    return out


def gumbel_noise_ref(seed: int, position: int, vocab: int, col_offset: int = 0) -> torch.Tensor:
    """Host mirror of the device counter hash (common.h mix64 / hash_col / uniform01), vectorised."""
    import numpy as np

    M = (1 << 64) - 1
    k = ((seed * 0x9E3779B97F4A7C15) & M) ^ ((position << 32) & M)
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M
    k ^= k >> 33
    k1, k2 = np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32)
    with np.errstate(over="ignore"):
        h = (np.arange(vocab, dtype=np.uint64) + np.uint64(col_offset & 0xFFFFFFFF)).astype(np.uint32) ^ k1
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15)
        h ^= k2
        h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    u = (h >> np.uint32(9)).astype(np.float64) + 0.5
    u = torch.from_numpy(u / 8388608.0)
    return -torch.log(-torch.log(u))


def sample_threshold(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor,
                     top_p: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Top-k / top-p as one threshold per row, fp64 and sort-based: (thr fp32, kept int32),
    the candidate set of row r being the columns with logit >= thr[r] (docs/PARITY.md "Sampling").

    * greedy rows (T <= 0) and rows with both filters off (top_k <= 0 or >= vocab; top_p >= 1):
      thr = -inf, kept = vocab;
    * tau_k = the top_k-th largest logit, ties at it all kept (HF TopKLogitsWarper);
    * m(v) = sum of exp((x - max) / T) over kept x >= v; tau_p = the largest logit v with
      m(v) >= top_p * m(tau_k): top-p after temperature, over the top-k survivors;
    * thr = max(tau_k, tau_p). NaN logits are never kept, -0 and +0 are one value, -inf
      logits carry mass 0.
    """
    rows, V = logits.shape
    thr = torch.full((rows,), float("-inf"), dtype=torch.float32)
    kept = torch.full((rows,), V, dtype=torch.int32)
    for r in range(rows):
        t, k, p = float(temperature[r]), int(top_k[r]), float(top_p[r])
        use_k, use_p = 0 < k < V, p < 1
        if not t > 0 or not (use_k or use_p):
            continue
        x = logits[r].double().cpu()
        s = torch.sort(x[~torch.isnan(x)], descending=True).values + 0.0   # + 0.0: -0 -> +0
        n = s.numel()
        if n == 0 or s[0] == float("-inf"):   # every mass is 0: nothing to cut
            kept[r] = n
            continue
        if use_k:
            s = s[s >= s[min(k, n) - 1]]
        tau, cnt = s[-1], s.numel()
        if use_p:
            w = torch.exp((s - s[0]) / t)
            w[s == s[0]] = 1.0                # also for max = +inf (inf - inf)
            c = torch.cumsum(torch.nan_to_num(w, nan=0.0), 0)
            vals, counts = torch.unique_consecutive(s, return_counts=True)
            ends = torch.cumsum(counts, 0) - 1
            j = int(torch.nonzero(c[ends] >= max(p, 0.0) * c[-1])[0])
            tau, cnt = vals[j], int(ends[j]) + 1
        thr[r] = float(tau)
        kept[r] = cnt
    return thr.to(logits.device), kept.to(logits.device)


def sample_shard(logits: torch.Tensor, temperature: torch.Tensor, seeds: torch.Tensor, positions: torch.Tensor,
                 col_offset: int = 0, top_k: torch.Tensor | None = None, top_p: torch.Tensor | None = None,
                 thr: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Greedy when T<=0 else Gumbel-max with the same counter hash as the kernel, over the
    columns with logit >= the row's threshold when ``top_k`` / ``top_p`` (``sample_threshold``;
    either may be None = off) or a precomputed ``thr`` is given.

    Returns (global token ids, winning perturbed values) for a vocab shard.
    """
    rows = logits.shape[0]
    if top_k is not None or top_p is not None:
        top_k = torch.zeros(rows, dtype=torch.int32) if top_k is None else top_k
        top_p = torch.ones(rows, dtype=torch.float32) if top_p is None else top_p
        thr = sample_threshold(logits, temperature, top_k, top_p)[0]
    out = torch.empty(rows, dtype=torch.long)
    val = torch.empty(rows, dtype=torch.float32)
    for r in range(rows):
        x = logits[r].double().cpu()
        t = float(temperature[r])
        cut = x < float(thr[r]) if thr is not None else None
        if t > 0:
            x = x / t + gumbel_noise_ref(int(seeds[r]), int(positions[r]), x.numel(), col_offset)
        if cut is not None and bool(cut.any()):
            x = x.masked_fill(cut, float("-inf"))
        i = int(torch.argmax(x))
        out[r] = i + col_offset
        val[r] = float(x[i])
    return out.to(logits.device), val.to(logits.device)


PROMPT_BIT = -2 ** 31      # bit 31 of a penalty-table word (int32): the token is in the prompt
COUNT_MASK = 2 ** 31 - 1    # bits 0-30: how often the token was generated


def penalty_seed(cnt: torch.Tensor, lst: torch.Tensor, n: torch.Tensor, slots: torch.Tensor, ids: torch.Tensor,
                 cu: torch.Tensor) -> None:
    """Clear the penalty-table slots ``slots`` (walking each one's list) and flag the tokens of
    the packed prompts ``ids[cu[b]:cu[b + 1]]`` with bit 31, listing each distinct one once. Ids
    outside the table's vocabulary and slots < 0 are ignored. The table is int32 ``cnt``
    [slots, vocab], ``lst`` [slots, cap], ``n`` [slots] (docs/PARITY.md "Sampling: penalties")."""
    V, cap = cnt.shape[1], lst.shape[1]
    off = [int(x) for x in cu]
    for b, s in enumerate(int(x) for x in slots):
        if not 0 <= s < cnt.shape[0]:
            continue
        k = min(max(int(n[s]), 0), cap)
        old = lst[s, :k].long()
        cnt[s, old[(old >= 0) & (old < V)]] = 0
        p = ids[max(off[b], 0):off[b + 1]].long()
        u = torch.unique(p[(p >= 0) & (p < V)])[:cap]
        cnt[s, u] = PROMPT_BIT
        lst[s, :u.numel()] = u.to(lst.dtype)
        n[s] = u.numel()


def sample_penalty(logits: torch.Tensor, pslot: torch.Tensor, last_tok: torch.Tensor | None, ctx: torch.Tensor | None,
                   rep: torch.Tensor, freq: torch.Tensor, pres: torch.Tensor, cnt: torch.Tensor, lst: torch.Tensor,
                   n: torch.Tensor) -> None:
    """Repetition / frequency / presence penalties on ``logits`` in place (vLLM / HF semantics,
    docs/PARITY.md "Sampling: penalties"). Row i uses table slot ``pslot[i]`` (< 0, or ``ctx[i]``
    == 0 when ``ctx`` is given: untouched). With ``last_tok`` the row's token is counted first
    (a new token is appended to the slot's list; a full list leaves the table as it is). Then,
    for every token t of the list with word w = cnt[slot, t] and c = w & COUNT_MASK::

        y = x (fp32);  rep != 1:  y = y / rep if y > 0 else y * rep;  c > 0:  y = y - (freq * c + pres)

    each operation rounded to fp32 on its own, the result rounded to the logits' dtype. A NaN
    logit keeps its bytes."""
    V, cap = logits.shape[1], lst.shape[1]
    for row, s in enumerate(int(x) for x in pslot):
        if not 0 <= s < cnt.shape[0] or (ctx is not None and int(ctx[row]) == 0):
            continue
        if last_tok is not None:
            t = int(last_tok[row])
            if 0 <= t < cnt.shape[1]:
                w = int(cnt[s, t])
                if w == 0:
                    k = int(n[s])
                    if 0 <= k < cap:
                        lst[s, k] = t
                        n[s] = k + 1
                        cnt[s, t] = 1
                elif (w & COUNT_MASK) != COUNT_MASK:
                    cnt[s, t] = w + 1
        k = min(max(int(n[s]), 0), cap)
        idx = lst[s, :k].long()
        idx = idx[(idx >= 0) & (idx < min(V, cnt.shape[1]))]
        c = cnt[s, idx] & COUNT_MASK
        x = logits[row, idx]
        y = x.float()
        r, f, p = rep[row].float(), freq[row].float(), pres[row].float()
        if float(r) != 1.0:
            y = torch.where(y > 0, y / r, y * r)
        y = torch.where(c > 0, y - (f * c.float() + p), y)
        logits[row, idx] = torch.where(torch.isnan(x), x, y.to(logits.dtype))


LOGPROBS_MAX = 20   # list entries per position (kernels.h kLogprobsMax)


def sample_logprobs(logits: torch.Tensor, nlp: torch.Tensor, ctx: torch.Tensor | None, tokens: torch.Tensor,
                    step: torch.Tensor | None, tok_lp: torch.Tensor, top_lp: torch.Tensor, top_id: torch.Tensor) -> None:
    """Log-probabilities of the sampled ``tokens`` and of each row's most likely tokens, fp64 and
    sort-based (docs/PARITY.md "Sampling: logprobs"). Row r with ``nlp[r]`` >= 0 (and ``ctx[r]``
    != 0 when ``ctx`` is given) writes column c = ``step[0] % C`` (0 without ``step``) of ``tok_lp``
    [rows, C] fp32 and the first N = min(nlp[r], LOGPROBS_MAX) entries of ``top_lp`` fp32 /
    ``top_id`` int32 [rows, C, LOGPROBS_MAX]; every other element keeps its value.

    * lse = mx + ln(sum over non-NaN x of exp(x - mx)), mx the maximum over non-NaN logits, a term
      with x == mx counting as exactly 1 (also for mx = +-inf); logprob(t) = x_t - lse, so NaN for a
      NaN logit, for every token of a row without a non-NaN logit or with mx = -inf, and for a
      token id outside the row;
    * the list: the first min(N, number of non-NaN logits) tokens by (logit descending, id
      ascending), -0 and +0 one value; the remaining entries are id -1, log-probability -inf."""
    V, C = logits.shape[1], tok_lp.shape[1]
    col = int(step.reshape(-1)[0]) % C if step is not None else 0
    for r in range(logits.shape[0]):
        n = int(nlp[r])
        if n < 0 or (ctx is not None and int(ctx[r]) == 0):
            continue
        n = min(n, LOGPROBS_MAX)
        x = logits[r].double().cpu()
        ok = ~torch.isnan(x)
        xv = x[ok]
        lse = torch.tensor(math.nan, dtype=torch.float64)
        if xv.numel():
            mx = xv.max()
            w = torch.exp(xv - mx)
            w[xv == mx] = 1.0                 # also for mx = +-inf (inf - inf)
            lse = mx + torch.log(w.sum())
        t = int(tokens[r])
        tok_lp[r, col] = float(x[t] - lse) if 0 <= t < V else math.nan
        if n == 0:
            continue
        ids = torch.nonzero(ok).flatten()
        order = torch.sort(-xv, stable=True).indices[:n]   # ids ascend already; -0 == +0 under the sort
        m = order.numel()
        top_id[r, col, :m] = ids[order].to(top_id.dtype)
        top_lp[r, col, :m] = (xv[order] - lse).to(top_lp.dtype)
        top_id[r, col, m:n] = -1
        top_lp[r, col, m:n] = -math.inf


def sample(logits: torch.Tensor, temperature: torch.Tensor, seeds: torch.Tensor,
           positions: torch.Tensor) -> torch.Tensor:
    return sample_shard(logits, temperature, seeds, positions)[0]
