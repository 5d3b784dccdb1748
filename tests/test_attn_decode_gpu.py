"""Paged decode attention (csrc/kernels/attn_decode.hip): every launch path, boundary token and
cache edge of the split-KV kernel, the two combines and the fused RoPE + KV-write prologue.

Inputs are built on the CPU by plain functions and properties are asserted by plain checkers.
Every test takes a device: ``hip`` (marked gpu) runs the gfx950 kernels, ``ref`` feeds the same
inputs through ``ops.attn_decode`` on CPU tensors (the fp32 torch reference) into the same
checkers, so every invariant asserted of the kernel is shown to hold for the reference first, on a
machine without a GPU. What only the binding can do (``variant``, the fused prologue, raising
before a launch) is in tests marked gpu.

Oracle and error measure. ``_oracle`` is fp64 and independent of ``reference.attn_decode``: per
sequence and head it clamps the length to the block table's capacity, gathers and dequantises the
pages, and returns ``o = sum p_i v_i`` and ``A = sum p_i |v_i|``. ``_check`` asserts for every
element

    |got - o| <= 2^-8 |o| + TAU * A

The first term is the half-ulp of the final bf16 rounding (8 significand bits). The second bounds
the fp32 accumulation and exp2 error in units that do not shrink with the context length: with
near-uniform weights |o| falls like 1/sqrt(len) while A stays at the size of a V element, and
dropping one token of a uniform softmax moves an element by about |v| / len = A-sized / len.
Where A == 0 (a padding row; a dimension in which every attended V element is 0) the output must
be exactly 0.

TAU. The largest excess ``(|got - o| - 2^-8 |o|) / A`` over all cases of this file:

    fp32 torch reference (CPU):                       1.150e-08  (randn K / V, 130 tokens)
    the kernel before this file was added (MI355X):   2.977e-08  (all e4m3 codes, G = 4, 300 tokens)

In most cases the excess is negative: the error stays inside the half-ulp term. TAU is four times
the larger of the two, 1.191e-07, rounded up to a power of two: 2^-23 (1.192e-07), far below the
ceiling of 2^-10 set for it. A one-token miscount at 1000 tokens is an excess of 7e-3 = 2^-7.

Every cache of this file is poisoned: each slot at or past a sequence's length, each page in no
block table, and the in-range page that padded block-table entries point at hold NaN (bf16 NaN /
e4m3 0x7F). Every call runs with ``out`` pre-filled with a canary, NaN-filled partial buffers with a
canary tail, and both caches compared bit for bit afterwards (``_run``).
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from operator_amd import ops
from operator_amd.ops import reference as ref

DEVS = [pytest.param("cpu", id="ref"), pytest.param("cuda", marks=pytest.mark.gpu, id="hip")]
BF16, F32, E4M3 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
D = 128
HALF_ULP = 2.0 ** -8
TAU = 2.0 ** -23
CANARY = float(torch.tensor(1e30).to(BF16))   # no output of this file comes near it
TAIL = 256                                    # canary elements behind each partial buffer
SCALE = D ** -0.5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.uint8 if t.element_size() == 1
                                     else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# cases: logical per-sequence K / V -> a poisoned paged cache; the fp64 oracle; the checkers
# ---------------------------------------------------------------------------------------------

def _store(x, fp8, scale=1.0):
    """fp32 values -> the bits a cache of that type holds (int16 bf16 / uint8 e4m3fn(x / scale))."""
    return _bits(ref.kv_store(x, E4M3 if fp8 else BF16, scale))


def _tile_k(logical):
    """[pages, Hkv, P, D] token-row K bits -> the tiled layout (inverse of ref.k_cache_logical)."""
    pages, Hkv, P, _ = logical.shape
    idx = ref.k_tile_index(D).flatten()
    out = torch.empty_like(logical)
    out.view(pages, Hkv, P // ref.K_TILE, ref.K_TILE * D)[..., idx] = logical.reshape(pages, Hkv, P // ref.K_TILE,
                                                                                      ref.K_TILE * D)
    return out


def _build(kbits, vbits, q, P, scale, k_scale=1.0, v_scale=1.0, seq_lens=None, pad_cols=1, seed=0, oracle=True):
    """kbits / vbits: per sequence the [n, Hkv, D] cache bits of its n tokens (int16: a bf16 cache,
    uint8: e4m3fn). Pages are handed out in a random order; everything no sequence holds is NaN, and
    block-table entries past a sequence's last page name an in-range all-NaN page. ``seq_lens``
    defaults to the tokens held (a larger value is a length above the table's capacity)."""
    fp8 = kbits[0].dtype == torch.uint8
    B, Hkv = len(kbits), kbits[0].shape[1]
    held = [int(k.shape[0]) for k in kbits]
    used = [(n + P - 1) // P for n in held]
    MP = max(1, max(used)) + pad_cols
    pages = sum(used) + 2
    perm = torch.randperm(pages, generator=_gen(seed)).tolist()
    nan_page, free = perm[-1], perm[:-2]          # perm[-2]: a NaN page in no table at all
    nan = 0x7F if fp8 else 0x7FC0
    kl = torch.full((pages, Hkv, P, D), nan, dtype=kbits[0].dtype)
    vl = torch.full((pages, Hkv, P, D), nan, dtype=kbits[0].dtype)
    bt = torch.full((B, MP), nan_page, dtype=torch.int32)
    at = 0
    for b in range(B):
        ids = free[at:at + used[b]]
        at += used[b]
        if not ids:
            continue
        bt[b, :used[b]] = torch.tensor(ids, dtype=torch.int32)
        for src, dst in ((kbits[b], kl), (vbits[b], vl)):
            full = torch.full((used[b] * P, Hkv, D), nan, dtype=src.dtype)
            full[:held[b]] = src
            dst[ids] = full.view(used[b], P, Hkv, D).permute(0, 2, 1, 3)
    dt = E4M3 if fp8 else BF16
    c = SimpleNamespace(q=q.to(BF16), kc=_tile_k(kl).view(dt), vc=vl.view(dt), bt=bt,
                        sl=torch.tensor(held if seq_lens is None else seq_lens, dtype=torch.int32), P=P, fp8=fp8,
                        scale=scale, k_scale=k_scale, v_scale=v_scale, Hkv=Hkv, nan_page=nan_page)
    assert _same_bits(ref.k_cache_logical(c.kc), kl.view(dt))
    if oracle:
        _oracle(c)
    return c


def _oracle(c):
    """fp64 attention over the dequantised pages: c.o, c.A [B, Hq, D] and c.p (per sequence
    [Hq, len] weights). reference.* is used for the K layout and the e4m3 decoding only."""
    B, Hq, _ = c.q.shape
    G = Hq // c.Hkv
    kl = ref.kv_load(ref.k_cache_logical(c.kc), 1.0).double() * c.k_scale
    vl = ref.kv_load(c.vc, 1.0).double() * c.v_scale
    c.o = torch.zeros(B, Hq, D, dtype=torch.float64)
    c.A = torch.zeros(B, Hq, D, dtype=torch.float64)
    c.p, c.len = [], []
    for b in range(B):
        L = min(int(c.sl[b]), c.bt.shape[1] * c.P)
        c.len.append(max(L, 0))
        if L <= 0:
            c.p.append(None)
            continue
        npg = (L + c.P - 1) // c.P
        ids = c.bt[b, :npg].long()
        ks = kl[ids].permute(1, 0, 2, 3).reshape(c.Hkv, npg * c.P, D)[:, :L]
        vs = vl[ids].permute(1, 0, 2, 3).reshape(c.Hkv, npg * c.P, D)[:, :L]
        assert torch.isfinite(ks).all() and torch.isfinite(vs).all()
        s = torch.einsum("kgd,kld->kgl", c.q[b].double().view(c.Hkv, G, D), ks) * c.scale
        p = torch.softmax(s, -1)
        c.o[b] = torch.einsum("kgl,kld->kgd", p, vs).reshape(Hq, D)
        c.A[b] = torch.einsum("kgl,kld->kgd", p, vs.abs()).reshape(Hq, D)
        c.p.append(p.reshape(Hq, L))


def _excess(got, c):
    """Per element (|got - o| - 2^-8 |o|) / A; where A == 0: 0 if got == 0 else inf."""
    got = got.double().cpu()
    err = (got - c.o).abs() - HALF_ULP * c.o.abs()
    live = c.A > 0
    return torch.where(live, err / torch.where(live, c.A, torch.ones_like(c.A)),
                       torch.where(got == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))


def _check(got, c, label, dev):
    assert got.shape == c.o.shape and torch.isfinite(got.float()).all(), label
    ex = _excess(got, c)
    worst = int(ex.argmax())
    b, h, d = worst // (ex.shape[1] * D), worst // D % ex.shape[1], worst % D
    print(f"excess dev={dev} {label}: {float(ex.max()):.3e} at row {b} (len {c.len[b]}) head {h} dim {d}")
    assert float(ex.max()) <= TAU, (label, float(ex.max()), (b, h, d), float(got[b, h, d]), float(c.o[b, h, d]))


def _run(c, dev, ns=1, variant=None, quant=False):
    """ops.attn_decode on ``dev`` with everything the call must not depend on or touch poisoned:
    ``out`` starts as a canary, the partials as NaN with a canary tail. Asserts the tails and both
    caches are intact, every row of ``out`` is written (padding rows: zero) and finite. Returns the
    bf16 output, or (q8, sx) with ``quant``."""
    B, Hq, _ = c.q.shape
    kc, vc = c.kc.to(dev), c.vc.to(dev)
    out = torch.full((B, Hq, D), CANARY, dtype=BF16, device=dev)
    n = B * Hq * ns
    ws = None
    if ns > 1:
        ws = tuple(torch.full((n * w + TAIL,), math.nan, dtype=F32) for w in (D, 2))
        for t, w in zip(ws, (D, 2)):
            t[n * w:] = CANARY
        ws = tuple(t.to(dev) for t in ws)
    r = ops.attn_decode(c.q.to(dev), kc, vc, c.bt.to(dev), c.sl.to(dev), c.scale, ns, out=out, workspace=ws,
                        variant=variant, k_scale=c.k_scale, v_scale=c.v_scale, quant=quant)
    if dev == "cuda":
        torch.cuda.synchronize()
    assert _same_bits(kc, c.kc) and _same_bits(vc, c.vc), "the call changed the cache"
    if ws is not None:
        for t, w in zip(ws, (D, 2)):
            assert (t[n * w:] == CANARY).all(), "write past the partial buffers"
    if quant:
        return r[0].cpu(), r[1].cpu()
    assert r.data_ptr() == out.data_ptr()
    o = out.cpu()
    assert torch.isfinite(o.float()).all() and (o.float().abs() < 1e29).all(), "a row of out was not written"
    dead = torch.tensor([n == 0 for n in c.len])
    assert (o[dead] == 0).all()
    return o


def _split_bounds(n, ns, chunk):
    """The kernel's schedule: at most ``ns`` pieces of a multiple of ``chunk`` tokens."""
    per = -(-(-(-n // ns)) // chunk) * chunk
    return [(s, min(n, s + per)) for s in range(0, n, per)]


def _chunk(variant, G):
    return 128 if (variant & 3) == 2 and G in (1, 2, 4) else 64


# ---------------------------------------------------------------------------------------------
# census: scale 0, one-hot V: every token counted exactly once
# ---------------------------------------------------------------------------------------------

CENSUS_LENS = [[1, 15, 16, 17, 63, 64, 65, 127, 128, 129],
               [191, 192, 193, 255, 256, 257, 319, 320, 321, 383, 384, 385]]
# (P, num_splits, variant, G, fp8): splits x variants with P, G and the cache type cycling through
# them, then the (G, NT, cache type) instantiations the cycle misses. 28 combinations x 2 batches.
CENSUS_COMBOS = [((16, 64, 256)[i % 3], ns, v, (1, 2, 3, 4, 8)[i % 5], bool(i % 2))
                 for i, (ns, v) in enumerate((ns, v) for ns in (1, 2, 3, 5, 64) for v in (0, 2, 4, 6))]
CENSUS_COMBOS += [(16, 2, 2, 2, False), (64, 3, 0, 2, True), (16, 5, 0, 1, True), (64, 2, 2, 1, False),
                  (16, 3, 0, 3, True), (64, 2, 2, 4, True), (16, 5, 6, 4, False), (256, 3, 0, 8, True)]


def _census_kv(g, n, Hkv, fp8, k_scale, v_scale):
    """K random; V[t][kvh] one-hot at dim (t + 17 kvh) % 128 (1 is exact in both cache types)."""
    v = torch.zeros(n, Hkv, D)
    t = torch.arange(n)
    for kvh in range(Hkv):
        v[t, kvh, (t + 17 * kvh) % D] = 1.0
    return _store(_randn(g, n, Hkv, D), fp8, k_scale), _store(v, fp8, v_scale)


@functools.lru_cache(maxsize=None)
def _census_case(lens, P, G, fp8, Hkv=2):
    g = _gen(100 + P + G)
    k_scale, v_scale = (0.5, 2.0) if fp8 else (1.0, 1.0)
    kv = [_census_kv(g, n, Hkv, fp8, k_scale, v_scale) for n in lens]
    c = _build([k for k, _ in kv], [v for _, v in kv], _randn(g, len(lens), G * Hkv, D), P, 0.0, k_scale, v_scale,
               seed=P + G)
    # the fp64 answer is n_d / len exactly
    for b, n in enumerate(lens):
        for kvh in range(Hkv):
            want = torch.bincount((torch.arange(n) + 17 * kvh) % D, minlength=D).double() / n
            for h in range(G):
                assert (c.o[b, kvh * G + h] - want).abs().max() < 1e-15
    assert torch.equal(c.o, c.A)
    return c


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("P,ns,variant,G,fp8", CENSUS_COMBOS,
                         ids=[f"P{p}-s{s}-v{v}-G{g}-{'fp8' if f else 'bf16'}" for p, s, v, g, f in CENSUS_COMBOS])
def test_census_every_token_counted_once(P, ns, variant, G, fp8, dev):
    """Uniform weights over one-hot V rows: element d of the output is (tokens with t % 128 == d)
    / len, so a token dropped, duplicated or double-weighted moves one element by 1 / len (at 385
    tokens: a quarter of its value; the tolerance is 0.5 %). Lengths sit on both sides of every
    chunk boundary of 1 to 5 (NT 1) / 1 to 3 (NT 2) chunks, pages are smaller than, equal to and
    larger than a chunk, and the split counts include more splits than chunks."""
    for i, lens in enumerate(CENSUS_LENS):
        c = _census_case(tuple(lens), P, G, fp8)
        _check(_run(c, dev, ns, variant), c, f"census[{i}] P={P} ns={ns} v={variant} G={G} fp8={fp8}", dev)


# ---------------------------------------------------------------------------------------------
# witness: one token takes (almost) all the weight
# ---------------------------------------------------------------------------------------------

def _witness_q(g, B, Hkv, G):
    """Heads of a group share a direction (base + 0.5 noise), so one key can win for all of them."""
    return (_randn(g, B, Hkv, 1, D) + _randn(g, B, Hkv, G, D, scale=0.5)).reshape(B, Hkv * G, D).to(BF16)


def _witness_v(Hkv):
    d = torch.arange(D)
    # [Hkv, D], bf16-exact, no element 0 (there the output would be the other tokens' ~2^-100 share,
    # below the fp32 normal range, where a half-ulp bound means nothing)
    return torch.stack([(d % 13 - 6).float() * 0.5 + 0.25 + kvh for kvh in range(Hkv)])


def _witness_kv(g, n, qb, Hkv, t, mult=6.0, second=None):
    """Keys randn * 0.25 except K[t] = mult * (mean of the group's q heads), V[t] a distinctive row;
    ``second``: a token with half that multiple (the next-largest score)."""
    k, v = _randn(g, n, Hkv, D, scale=0.25), _randn(g, n, Hkv, D)
    qm = qb.float().view(Hkv, -1, D).mean(1)
    k[t], v[t] = mult * qm, _witness_v(Hkv)
    if second is not None:
        k[second] = 0.5 * mult * qm
    return k, v


def _witness_case(lens, toks, P, G, fp8, seconds=None, seq_lens=None, pad_cols=1, Hkv=2, seed=0):
    g = _gen(200 + seed + P + G)
    k_scale, v_scale = (0.37, 1.9) if fp8 else (1.0, 1.0)
    q = _witness_q(g, len(lens), Hkv, G)
    kv = [_witness_kv(g, n, q[b], Hkv, toks[b], second=None if seconds is None else seconds[b])
          for b, n in enumerate(lens)]
    c = _build([_store(k, fp8, k_scale) for k, _ in kv], [_store(v, fp8, v_scale) for _, v in kv], q, P, SCALE,
               k_scale, v_scale, seq_lens=seq_lens, pad_cols=pad_cols, seed=seed + G)
    vl = ref.kv_load(c.vc, 1.0).double() * v_scale
    vmax = float(vl.nan_to_num().abs().max())
    for b, t in enumerate(toks):
        # CPU-side condition: the token holds 1 - 2^-12 of every head's weight, hence the fp64
        # output is its stored V row to (1 - p_t) (|V[t]| + max |v|)
        assert float(c.p[b][:, t].min()) >= 1 - 2.0 ** -12, (b, t, float(c.p[b][:, t].min()))
        row = vl[int(c.bt[b, t // P]), :, t % P]                       # [Hkv, D]
        want = row.repeat_interleave(G, 0)
        assert ((c.o[b] - want).abs() <= 2.0 ** -12 * (want.abs() + vmax)).all()
    return c


W300 = [0, 299, 63, 64, 80, 95, 127, 128, 191, 192, 255, 256]
# (P, num_splits, variant, G, fp8)
WITNESS_COMBOS = [(16, 1, 0, 4, False), (16, 2, 0, 4, False), (16, 3, 0, 4, False), (16, 1, 2, 4, False),
                  (16, 3, 2, 4, False), (16, 2, 4, 4, False), (64, 3, 0, 4, False), (16, 3, 0, 2, True),
                  (16, 2, 2, 2, True), (16, 3, 0, 8, False), (16, 3, 6, 1, True), (16, 2, 0, 3, True),
                  (16, 3, 2, 2, False), (256, 3, 2, 1, False)]


@functools.lru_cache(maxsize=None)
def _witness300(P, G, fp8):
    return _witness_case([300] * len(W300), W300, P, G, fp8)


def test_witness_positions_are_the_boundaries():
    """W300 holds token 0, len - 1, the first and last token of every split of 300 tokens in 2 and
    3 pieces (both chunk sizes), of page 5 of 16 tokens, and of chunks 0 | 1 of 64 and 128 tokens."""
    w = set(W300)
    assert {0, 299, 80, 95, 63, 64, 127, 128} <= w
    for ns in (2, 3):
        for chunk in (64, 128):
            for a, e in _split_bounds(300, ns, chunk):
                assert {a, e - 1} <= w, (ns, chunk, a, e)
    assert _split_bounds(300, 3, 64) == [(0, 128), (128, 256), (256, 300)]
    assert _split_bounds(300, 2, 64) == [(0, 192), (192, 300)]


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("P,ns,variant,G,fp8", WITNESS_COMBOS,
                         ids=[f"P{p}-s{s}-v{v}-G{g}-{'fp8' if f else 'bf16'}" for p, s, v, g, f in WITNESS_COMBOS])
def test_witness_boundary_token_carries_the_answer(P, ns, variant, G, fp8, dev):
    """Twelve sequences of 300 tokens, each with one boundary token holding >= 1 - 2^-12 of the
    weight of every head: the output row is that token's V row."""
    c = _witness300(P, G, fp8)
    _check(_run(c, dev, ns, variant), c, f"witness300 P={P} ns={ns} v={variant} G={G} fp8={fp8}", dev)


# late spikes and the capacity clamp. Rows (P = 16, capacity 44 pages = 704 tokens, no padding
# column): 700 tokens, spike at 650 (chunk 10 of 64; wave 0, lane group 2; last split of 5), the
# next-largest score at 37 (chunk 0, wave 2, lane group 1, split 0); 700 tokens, spike at 333
# (wave 0, lane group 3), next-largest at 600 (wave 1, lane group 2, another split); seq_len 804
# over 704 held tokens, the spike at the last in-capacity token.
LATE_LENS, LATE_TOKS, LATE_SECOND, LATE_SEQ_LENS = [700, 700, 704], [650, 333, 703], [37, 600, 5], [700, 700, 804]
LATE_COMBOS = [(1, 0, 4, False), (5, 0, 4, False), (1, 2, 4, False), (5, 2, 4, False), (5, 0, 4, True),
               (1, 2, 2, True), (5, 0, 8, False), (4, 4, 2, False), (5, 0, 3, True)]


@functools.lru_cache(maxsize=None)
def _late_case(G, fp8):
    c = _witness_case(LATE_LENS, LATE_TOKS, 16, G, fp8, seconds=LATE_SECOND, seq_lens=LATE_SEQ_LENS, pad_cols=0, seed=7)
    assert c.bt.shape[1] * c.P == 704 and c.len == [700, 700, 704]
    # the spike is >= 60 log2 units above every score but the planted next-largest (>= 30), which
    # itself is >= 20 above the rest
    for b, (t, u) in enumerate(zip(LATE_TOKS, LATE_SECOND)):
        s = torch.log2(c.p[b])
        noise = torch.ones(s.shape[1], dtype=torch.bool)
        noise[[t, u]] = False
        assert float((s[:, t:t + 1] - s[:, noise]).min()) >= 60 and float((s[:, t] - s[:, u]).min()) >= 30
        assert float((s[:, u:u + 1] - s[:, noise]).min()) >= 20
    return c


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("ns,variant,G,fp8", LATE_COMBOS,
                         ids=[f"s{s}-v{v}-G{g}-{'fp8' if f else 'bf16'}" for s, v, g, f in LATE_COMBOS])
def test_witness_late_spike_and_capacity_clamp(ns, variant, G, fp8, dev):
    """The running max jumps by ~100 log2 units (noise -> spike; ~50 over the planted
    next-largest score) after ten chunks: the chunk rescale (alpha), the lane-group merge, the wave
    merge and the split combine each meet a partner whose max is far below theirs. The third row's
    seq_len is 100 above the table's capacity: 5 splits of the clamped 704 tokens are 4 pieces, of
    804 they would be 5, so a combine (plain or quantising) that did not clamp reads a partial
    nobody wrote."""
    c = _late_case(G, fp8)
    o = _run(c, dev, ns, variant)
    _check(o, c, f"late ns={ns} v={variant} G={G} fp8={fp8}", dev)
    if ns > 1 and G * 2 * D <= 8192:
        q8, sx = _run(c, dev, ns, variant, quant=True)
        q0, s0 = ops.quantize_fp8(o.reshape(o.shape[0], -1).to(dev))
        assert torch.equal(sx, s0.cpu()) and _same_bits(q8, q0)


# ---------------------------------------------------------------------------------------------
# poisoned cache, padded tables, canaries, replay, the quantising combine
# ---------------------------------------------------------------------------------------------

POISON_LENS = [0, 1, 17, 64, 65, 130, 300, 517]


@functools.lru_cache(maxsize=None)
def _poison_case(fp8, G=4, Hkv=2, P=16):
    g = _gen(300 + fp8)
    k_scale, v_scale = (0.5, 2.0) if fp8 else (1.0, 1.0)
    mul = 3.0 if fp8 else 1.0
    kb = [_store(_randn(g, n, Hkv, D, scale=mul), fp8, k_scale) for n in POISON_LENS]
    vb = [_store(_randn(g, n, Hkv, D, scale=mul), fp8, v_scale) for n in POISON_LENS]
    return _build(kb, vb, _randn(g, len(POISON_LENS), G * Hkv, D), P, SCALE, k_scale, v_scale, seed=11)


def test_poison_case_is_poisoned():
    """Every slot no sequence holds is NaN, and every padded table entry is in range and names
    the all-NaN page."""
    for fp8 in (False, True):
        c = _poison_case(fp8)
        k, v = ref.k_cache_logical(c.kc).float(), c.vc.float()
        held = torch.zeros(k.shape[:3], dtype=torch.bool)
        for b, n in enumerate(POISON_LENS):
            used = (n + c.P - 1) // c.P
            assert (c.bt[b, used:] == c.nan_page).all() and c.bt.shape[1] > used
            assert int(c.bt.min()) >= 0 and int(c.bt.max()) < k.shape[0]
            for i in range(used):
                held[int(c.bt[b, i]), :, :min(c.P, n - i * c.P)] = True
        for t in (k, v):
            assert torch.equal(torch.isnan(t).all(-1), ~held) and torch.equal(torch.isfinite(t).all(-1), held)
        assert not held[c.nan_page].any()


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("ns", [1, 4])
@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_poisoned_cache_and_padded_tables(fp8, variant, ns, dev):
    """randn K / V among NaN: the output is finite and within the bound (nothing at or past a
    length, no padded table entry and no unwritten partial is read), the caches and the canary
    tails are intact (_run), a replay is bit-identical, and quant=True gives the e4m3fn rows and
    scales of ops.quantize_fp8 over the bf16 output."""
    c = _poison_case(fp8)
    o = _run(c, dev, ns, variant)
    _check(o, c, f"poison ns={ns} v={variant} fp8={fp8}", dev)
    assert _same_bits(o, _run(c, dev, ns, variant))
    q8, sx = _run(c, dev, ns, variant, quant=True)
    q0, s0 = ops.quantize_fp8(o.reshape(o.shape[0], -1).to(dev))
    assert torch.equal(sx, s0.cpu()) and _same_bits(q8, q0)
    assert _same_bits(q8, _run(c, dev, ns, variant, quant=True)[0])


# ---------------------------------------------------------------------------------------------
# more than 256 pages in one split: the strided LDS page-table fill
# ---------------------------------------------------------------------------------------------

LONG = 257 * 16 + 1


@functools.lru_cache(maxsize=None)
def _long_case(kind, fp8):
    if kind == "witness":
        return _witness_case([LONG], [256 * 16 + 5], 16, 2, fp8, seconds=[100], Hkv=1, seed=3)
    g = _gen(400)
    k_scale, v_scale = (0.5, 2.0) if fp8 else (1.0, 1.0)
    k, v = _census_kv(g, LONG, 1, fp8, k_scale, v_scale)
    return _build([k], [v], _randn(g, 1, 2, D), 16, 0.0, k_scale, v_scale, seed=5)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("kind", ["witness", "census"])
def test_long_page_table(kind, fp8, dev):
    """One sequence of 258 pages in one split: pages 256 and 257 reach the LDS table through
    the strided fill. The witness sits in page 256; the census counts every token of both."""
    c = _long_case(kind, fp8)
    assert c.bt.shape == (1, 259) and c.len == [LONG]
    for variant in (0, 2):
        _check(_run(c, dev, 1, variant), c, f"long {kind} v={variant} fp8={fp8}", dev)


# ---------------------------------------------------------------------------------------------
# every finite e4m3 code through the K (-> bf16) and V (-> fp32) widenings
# ---------------------------------------------------------------------------------------------

CODES = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)
CODES_LENS = [300, 77]
CODES_SCALE = 0.004   # not 1 / sqrt(D): the scores of these K rows spread over a few nats


@functools.lru_cache(maxsize=None)
def _codes_case(G, Hkv=2):
    """K byte (t, kvh, d) = code (t + 37 d + 57 kvh) % 254, V byte = code (3 t + 101 d + 31 kvh + 100)
    % 254: with 254 or more tokens every code appears at every d, hence in every byte of the 8-byte
    fragment (byte j holds dims d = j mod 8) of both caches."""
    assert CODES.numel() == 254 and {0x00, 0x80, 0x7E, 0xFE, 0x01, 0x07, 0x08} <= set(CODES.tolist())
    kb, vb = [], []
    for n in CODES_LENS:
        t, h, d = torch.arange(n)[:, None, None], torch.arange(Hkv)[None, :, None], torch.arange(D)[None, None, :]
        kb.append(CODES[(t + 37 * d + 57 * h) % 254])
        vb.append(CODES[(3 * t + 101 * d + 31 * h + 100) % 254])
    for x in (kb[0], vb[0]):
        for d in range(D):
            assert len(set(x[:, 0, d].tolist())) == 254
    c = _build(kb, vb, _randn(_gen(500 + G), len(CODES_LENS), G * Hkv, D), 16, CODES_SCALE, 0.37, 1.9, seed=G)
    assert float(ref.kv_load(c.vc, 1.9).nan_to_num().abs().max()) > 448 * 1.89      # +-448 is among the values
    pmax = torch.stack([p.max(1).values for p in c.p])
    assert float(pmax.max()) < 0.9 and float(pmax.min()) > 2.0 ** -7, pmax    # neither one-hot nor flat
    return c


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("G", [4, 1])
def test_all_e4m3_codes(G, dev):
    """Subnormals, +-0, +-448 and everything between, in every byte position of a fragment, with
    scales that are no powers of two: the widening is exact, so the section-1 bound holds."""
    c = _codes_case(G)
    for ns, variant in ((1, 0), (2, 0), (1, 2), (2, 6)):
        _check(_run(c, dev, ns, variant), c, f"codes G={G} ns={ns} v={variant}", dev)


# ---------------------------------------------------------------------------------------------
# the fused RoPE + KV-write prologue (gpu only)
# ---------------------------------------------------------------------------------------------

ROPE_MAXPOS = 1024
# sequence lengths; row 7: live with slot -1; row 8: pos -3; row 9: pos max_pos + 5
ROPE_LENS = [1, 17, 64, 65, 130, 700, 0, 130, 33, 200]


@functools.lru_cache(maxsize=None)
def _rope_case(G, fp8, Hkv=2, P=16):
    g = _gen(600 + G + fp8)
    k_scale, v_scale = (0.5, 2.0) if fp8 else (1.0, 1.0)
    kb = [_store(_randn(g, n, Hkv, D), fp8, k_scale) for n in ROPE_LENS]
    vb = [_store(_randn(g, n, Hkv, D), fp8, v_scale) for n in ROPE_LENS]
    nan = 0x7F if fp8 else 0x7FC0
    for b, n in enumerate(ROPE_LENS):     # the new token's slot holds NaN until the call writes it
        if n > 0 and b != 7:
            kb[b][n - 1], vb[b][n - 1] = nan, nan
    Hq = G * Hkv
    held = ROPE_LENS
    # the held slots have holes, so the oracle runs after the call that fills them
    c = _build(kb, vb, torch.zeros(len(held), Hq, D), P, SCALE, k_scale, v_scale, seed=G, oracle=False)
    c.Hq = Hq
    c.slots = torch.tensor([int(c.bt[b, (n - 1) // P]) * P + (n - 1) % P if n > 0 else -1 for b, n in enumerate(held)])
    c.slots[7] = -1
    c.pos = torch.tensor([max(n - 1, 0) for n in held])
    c.pos[8], c.pos[9] = -3, ROPE_MAXPOS + 5
    c.cos, c.sin = ref.rope_tables(ROPE_MAXPOS, D, 500000.0)
    c.qkv = _randn(g, len(held), (Hq + 2 * Hkv) * D).to(BF16)
    return c


# (G, fp8, variant, splits): variant 2 must run the NT = 1 schedule and tell the combine chunk = 64
# (65 tokens in 2 pieces: 2 splits of 64-token chunks, 1 of 128; 700 in 4: 4 and 3)
ROPE_COMBOS = [(4, False, 2, 2), (4, False, 2, 4), (4, True, 2, 2), (4, True, 2, 4), (2, False, 2, 4), (1, True, 2, 2)]
ROPE_COMBOS += [(G, fp8, 0, ns) for G in (1, 2, 3, 5, 6) for fp8, ns in ((False, 1), (True, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("G,fp8,variant,ns", ROPE_COMBOS,
                         ids=[f"G{g}-{'fp8' if f else 'bf16'}-v{v}-s{s}" for g, f, v, s in ROPE_COMBOS])
def test_fused_rope_prologue_equals_rope_kv_then_attn(G, fp8, variant, ns):
    """ops.attn_decode_rope == ops.rope_kv then ops.attn_decode (the NT = 1 schedule), bit for bit
    in the cache and in the output rows, with variant 2, the groups 1 / 2 / 3 / 5 / 6, a live row
    whose slot is -1 (nothing written; it attends over what the cache holds) and positions -3 and
    max_pos + 5 (clamped as rope_kv clamps them). Directly: the fused call changes the B x Hkv
    new-token slots and no other cache byte."""
    c = _rope_case(G, fp8)
    dev = "cuda"
    assert len(ROPE_LENS) * c.Hkv <= ops.FUSED_ROPE_MAX_SEQ_HEADS and ops.FUSED_DECODE_ROPE
    qkv, pos, cos, sin = c.qkv.to(dev), c.pos.to(dev), c.cos.to(dev), c.sin.to(dev)
    slots, bt, sl = c.slots.to(dev), c.bt.to(dev), c.sl.to(dev)
    kc_a, vc_a, kc_b, vc_b = c.kc.to(dev), c.vc.to(dev), c.kc.to(dev), c.vc.to(dev)
    kw = dict(k_scale=c.k_scale, v_scale=c.v_scale)
    q, _, _ = ops.rope_kv(qkv, pos, cos, sin, c.Hq, c.Hkv, kc_a, vc_a, slots, want_kv=False, **kw)
    want = ops.attn_decode(q, kc_a, vc_a, bt, sl, SCALE, ns, variant=variant & ~3, **kw)
    got = ops.attn_decode_rope(qkv, pos, cos, sin, c.Hq, kc_b, vc_b, slots, bt, sl, SCALE, ns, variant=variant, **kw)
    torch.cuda.synchronize()
    assert _same_bits(kc_a, kc_b) and _same_bits(vc_a, vc_b)
    live = c.sl > 0
    assert torch.isfinite(got.float().cpu()[live]).all()
    assert _same_bits(got.cpu()[live], want.cpu()[live])
    if c.Hq * D <= 8192:
        kc_q, vc_q = c.kc.to(dev), c.vc.to(dev)
        q8, sx = ops.attn_decode_rope(qkv, pos, cos, sin, c.Hq, kc_q, vc_q, slots, bt, sl, SCALE, ns, variant=variant,
                                      quant=True, **kw)
        q0, s0 = ops.quantize_fp8(got.reshape(got.shape[0], -1))
        assert torch.equal(sx[live.to(dev)], s0[live.to(dev)]) and _same_bits(q8.cpu()[live], q0.cpu()[live])
        assert _same_bits(kc_q, kc_b) and _same_bits(vc_q, vc_b)
    # the bytes that changed: exactly the rows (slot page, every kv-head, slot offset)
    allowed = torch.zeros(c.kc.shape[:3], dtype=torch.bool)
    for s in c.slots.tolist():
        if s >= 0:
            allowed[s // c.P, :, s % c.P] = True
    assert int(allowed.sum()) == 8 * c.Hkv
    for before, after in ((ref.k_cache_logical(c.kc), ref.k_cache_logical(kc_b.cpu())), (c.vc, vc_b.cpu())):
        changed = (_bits(before) != _bits(after)).any(-1)
        assert not (changed & ~allowed).any(), "a cache byte outside the new-token slots changed"
        assert torch.isfinite(after.float()[allowed]).all()
    # and the attention itself, against the fp64 oracle over the cache the call left
    o = SimpleNamespace(q=q.cpu(), kc=kc_b.cpu(), vc=vc_b.cpu(), bt=c.bt, sl=c.sl, P=c.P, Hkv=c.Hkv, scale=SCALE,
                        k_scale=c.k_scale, v_scale=c.v_scale)
    # slots past each length still hold NaN: the oracle asserts it reads none
    _oracle(o)
    _check(got.cpu(), o, f"fused rope G={G} fp8={fp8} v={variant} ns={ns}", dev)


# ---------------------------------------------------------------------------------------------
# refusals (gpu only): each raises before anything is launched
# ---------------------------------------------------------------------------------------------

def _refusal_args(B=2, Hq=8, Hkv=2, P=16, MP=4, ns=1, quant=False, ws=None):
    dev = "cuda"
    a = SimpleNamespace(
        q=torch.ones(B, Hq, D, dtype=BF16, device=dev), kc=torch.ones(B * MP + 1, Hkv, P, D, dtype=BF16, device=dev),
        bt=torch.zeros(B, MP, dtype=torch.int32, device=dev), sl=torch.full((B,), 5, dtype=torch.int32, device=dev),
        out=torch.full((B, Hq, D), CANARY, dtype=BF16, device=dev), ns=ns)
    a.vc = a.kc.clone()
    n = ws if ws is not None else max(1, B * Hq * max(ns, 1))
    a.op = torch.full((n * D,), CANARY, dtype=F32, device=dev)
    a.ml = torch.full((n * 2,), CANARY, dtype=F32, device=dev)
    a.q8 = torch.full((B, Hq * D), 0x55, dtype=torch.uint8, device=dev).view(E4M3) if quant else None
    a.sx = torch.full((B,), CANARY, dtype=F32, device=dev) if quant else None
    return a


def _call(a, variant=0):
    ops.kernels().attn_decode(a.q, a.kc, a.vc, a.bt, a.sl, a.out, a.op, a.ml, a.ns, SCALE, variant, 1.0, 1.0, a.q8, a.sx)
    torch.cuda.synchronize()


REFUSALS = {
    "page8": dict(P=8), "page48": dict(P=48), "group9": dict(Hq=9, Hkv=1), "table1025": dict(MP=1025, B=1),
    "quant_wide_row": dict(Hq=72, Hkv=9, quant=True, ns=2), "splits0": dict(ns=0), "partials_small": dict(ns=2, ws=1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_launch_nothing(name):
    """A shape the kernels do not take raises, and no buffer the call could write has changed."""
    a = _refusal_args(**REFUSALS[name])
    with pytest.raises(RuntimeError):
        _call(a)
    for t in (a.out, a.op, a.ml) + ((a.sx,) if a.sx is not None else ()):
        assert (t == CANARY).all(), name
    if a.q8 is not None:
        assert (a.q8.view(torch.uint8) == 0x55).all()


@pytest.mark.gpu
def test_accepted_neighbours_of_the_refusals_and_empty_batch():
    """The same arguments with a shape the kernels do take run (the refusals above are not
    refusals of the helper's buffers), and B = 0 returns without error."""
    for kw in (dict(), dict(ns=2), dict(Hq=64, Hkv=8, quant=True, ns=2), dict(MP=1024, B=1)):
        a = _refusal_args(**kw)
        _call(a)
        assert (a.out == 1).all()          # K = V = 1: the average of ones
    a = _refusal_args(B=0)
    _call(a)
    o = ops.attn_decode(a.q, a.kc, a.vc, a.bt, a.sl, SCALE, 1)
    assert o.shape == (0, 8, D)
