"""Prefill attention (csrc/kernels/attn_prefill.hip): every variant (v1 per query head, v2 16-row
GQA waves, v3 / v4 swapped-operand 32x32 waves in 8- / 4-wave workgroups), mask edge, shared
prefix and padded launch of the four flash-attention kernels, and the host-side work list and
variant selection.

Inputs are built on the CPU by plain functions and properties are asserted by plain checkers.
Every property test takes a device: ``hip`` (marked gpu) runs the gfx950 kernels, ``ref`` feeds the
same inputs through ``ops.attn_prefill`` on CPU tensors (the fp32 torch reference) into the same
checkers, so every invariant asserted of a kernel is shown to hold for the reference first, on a
machine without a GPU. What only the binding can do (``work=``, ``variant``, raising before a
launch, bit-identity of two launches) is asserted on the gpu only.

Oracle and error measure. ``_oracle`` is fp64 and independent of ``reference.attn_prefill``: per
sequence it concatenates the ``seq_pfx[s]`` prefix keys with the sequence's own keys, masks
causally with row r at position pl + r, and returns ``o = sum p_i v_i``, ``A = sum p_i |v_i|`` and
the weights p. ``_check`` asserts for every element of every row inside a sequence

    |got - o| <= 2^-8 |o| + TAU * A

The first term is the half-ulp of the final bf16 rounding (8 significand bits). The second is in
units that do not shrink with the row's key count: with near-uniform weights |o| falls like
1 / sqrt(keys) while A stays at the size of a V element, and one key dropped from a uniform softmax
moves an element by about |v| / keys. Where A == 0 the output must be exactly 0.

Two values of TAU, because all four kernels round the unnormalised weights P to bf16 before the
P.V MFMA while the row sum is kept in fp32:

TAU_EXACT = 2^-20, for the census cases, whose weights are exactly representable (scale 0: every
visible key has P = exp2(0) = 1). Derived, not measured: the P.V products are 1 x {0, 1} and their
fp32 sums are integers below 2^24, exact; the row sum is the exact integer key count; what is left
is one fp32 reciprocal and one fp32 multiply, 2 x 2^-24 relative, before the bf16 rounding that the
first term covers. 2^-20 leaves a factor 8. The fp32 CPU reference scores an excess of 0.0 on
every census of this file.

TAU_P, for everything else. Its derived worst case is the unit roundoff of the bf16 weights, 2^-8
(every weight off by half an ulp in the direction of its V element's sign) plus fp32 terms, too
pessimistic to fix in advance. Measured: the largest excess ``(|got - o| - 2^-8 |o|) / A`` over
all non-census cases of this file for

    (a) the fp32 torch reference (CPU):                         2.086e-07  (rescale from a prefix tile, G = 8)
    (b) ``_emulate`` (CPU: max-subtracted exp2 weights rounded
        to bf16 for P.V, normalised by their fp32 sum):         3.459e-03  (randn, G = 4, a row of 2 keys)
    (c) the kernels before this file was added (MI355X):        3.459e-03  (the same element, v1 to v4)

In (b) and (c) the largest excesses sit in rows of 2 to 8 keys, where a few roundings of one sign
do not average out; the kernels' worst per family is 1.8e-03 to 3.5e-03, that of the census 0.0.
TAU_P is twice the larger of (b) and (c), 6.92e-03, rounded up to a power of two: 2^-7 (7.81e-03),
which is also the ceiling set for it.
What follows from TAU_P being about 2^-8: a one-key miscount among n near-uniform keys is an
excess of about 1 / n, so a randn case cannot see it past a couple of hundred keys. That is why
the census (exact weights, TAU_EXACT: one key in 513 is 2000 times the tolerance) and the witness /
anti-witness cases (one key carries the whole row, so taking the wrong key is an error of the size
of V) carry this file. The randn cases check overall arithmetic only.

Every call (``_run``) is poisoned and checked:
  * q / k / v / out have PAD rows past cu[-1]; those of q / k / v hold bf16 NaN;
  * out is pre-filled with a canary: afterwards every row inside a sequence is finite and written,
    every row past cu[-1] still holds the canary bits;
  * pk / pv have rows at and past the longest seq_pfx that hold NaN (and a sequence with a
    shorter prefix must not see the valid rows between its own length and the longest: the
    anti-witness and census cases put what would be seen there);
  * on the gpu, with ``variant`` given: the work list has items with work_seq == -1 at its head,
    middle and tail, cu_seqlens is padded with repeats of cu[-1] (and seq_pfx to match), as the
    graph-captured prefill's fixed grid is; the list is then permuted: the output is bit-identical
    to that of ``ops.prefill_work_list``'s order; and a second identical call is bit-identical;
  * q, k, v, pk and pv are compared bit for bit afterwards.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from operator_amd import ops

DEVS = [pytest.param("cpu", id="ref"), pytest.param("cuda", marks=pytest.mark.gpu, id="hip")]
BF16, F32 = torch.bfloat16, torch.float32
D = 128
HKV = 2
HALF_ULP = 2.0 ** -8
TAU_EXACT = 2.0 ** -20
TAU_P = 2.0 ** -7
CANARY = float(torch.tensor(1e30).to(BF16))   # no output of this file comes near it
PAD = 5                                       # rows of q / k / v / out past cu[-1]
PFX_PAD = 3                                   # NaN rows of pk / pv past the longest prefix
SCALE = D ** -0.5
LOG2E = 1.4426950408889634

# the (variant, G) grid; Hkv = 2 (so that kvh = 1 is exercised), Hq = 2 G
GRID = ([(1, g) for g in (1, 3, 4, 16)] + [(2, g) for g in (1, 2, 4, 8)] + [(3, g) for g in range(1, 9)]
        + [(4, g) for g in (1, 2, 3, 4)])
DEFAULT_G = (1, 3, 4, 5, 8)                   # work=None: ops.prefill_variant picks (v4 to G = 4, then v3)


def _ids(combos):
    return [f"v{v}-G{g}" if v else f"default-G{g}" for v, g in combos]


def _block_q(variant, G):
    """attn_prefill_block_q of csrc/kernels/attn_prefill.hip, restated (compared with the native
    function and with ops.prefill_block_q in test_block_q_matches_the_native_function)."""
    if variant == 1:
        return 64
    if variant == 2 and G in (1, 2, 4, 8):
        return 16 * (8 // G)
    if variant == 3 and 1 <= G <= 8:
        return 32 * (8 // G)
    if variant == 4 and 1 <= G <= 4:
        return 32 * (4 // G)
    return -1


def _bq(variant, G):
    return _block_q(variant or (4 if G <= 4 else 3), G)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# a case: packed bf16 q / k / v (+ prefix); the fp64 oracle; the checkers; the poisoned call
# ---------------------------------------------------------------------------------------------

def _case(q, k, v, lens, scale, pfx=None, pk=None, pv=None, keep_p=False):
    """q / k / v: per sequence [L, H, D] fp32 values (rounded to bf16 here); pfx: per sequence
    prefix length over the shared rows pk / pv [max(pfx), Hkv, D]."""
    c = SimpleNamespace(q=torch.cat(q).to(BF16), k=torch.cat(k).to(BF16), v=torch.cat(v).to(BF16), lens=list(lens),
                        scale=scale, pfx=None if pfx is None else list(pfx), pk=None, pv=None)
    c.T, c.Hq, c.Hkv = sum(lens), c.q.shape[1], c.k.shape[1]
    c.G = c.Hq // c.Hkv
    assert c.q.shape == (c.T, c.Hq, D) and c.k.shape == c.v.shape == (c.T, c.Hkv, D)
    if pfx is not None:
        c.pk, c.pv = pk.to(BF16), pv.to(BF16)
        assert c.pk.shape == c.pv.shape == (max(pfx), c.Hkv, D) and len(pfx) == len(lens)
    _oracle(c, keep_p)
    return c


def _oracle(c, keep_p=False):
    """fp64 attention: c.o, c.A [T, Hq, D], c.lse (per sequence [Hq, L], natural log of the row's
    sum of exp scores) and, with ``keep_p``, c.p (per sequence [Hq, L, pl + L] weights)."""
    c.o = torch.zeros(c.T, c.Hq, D, dtype=torch.float64)
    c.A = torch.zeros(c.T, c.Hq, D, dtype=torch.float64)
    c.p, c.lse, c.row_keys = [], [], torch.zeros(c.T, dtype=torch.long)
    a = 0
    for s, L in enumerate(c.lens):
        pl = c.pfx[s] if c.pfx is not None else 0
        if L == 0:
            c.p.append(None)
            c.lse.append(None)
            continue
        ks, vs = c.k[a:a + L].double(), c.v[a:a + L].double()
        if pl:
            ks, vs = torch.cat([c.pk[:pl].double(), ks]), torch.cat([c.pv[:pl].double(), vs])
        assert torch.isfinite(ks).all() and torch.isfinite(vs).all()
        sc = torch.einsum("lkgd,tkd->kglt", c.q[a:a + L].double().view(L, c.Hkv, c.G, D), ks) * c.scale
        seen = torch.arange(pl + L)[None, :] <= (pl + torch.arange(L))[:, None]
        sc = sc.masked_fill(~seen, -math.inf)
        lse = torch.logsumexp(sc, -1)
        p = torch.exp(sc - lse[..., None])
        c.o[a:a + L] = torch.einsum("kglt,tkd->lkgd", p, vs).reshape(L, c.Hq, D)
        c.A[a:a + L] = torch.einsum("kglt,tkd->lkgd", p, vs.abs()).reshape(L, c.Hq, D)
        c.row_keys[a:a + L] = pl + 1 + torch.arange(L)
        c.p.append(p.reshape(c.Hq, L, pl + L) if keep_p else None)
        c.lse.append(lse.reshape(c.Hq, L))
        a += L


def _emulate(c):
    """What the kernels compute, on the CPU in fp32: scores in log2 units, weights exp2(s - max)
    rounded to bf16 for P.V, normalised by the fp32 sum of the unrounded weights."""
    out = torch.zeros(c.T, c.Hq, D, dtype=BF16)
    a = 0
    for s, L in enumerate(c.lens):
        pl = c.pfx[s] if c.pfx is not None else 0
        if L == 0:
            continue
        ks, vs = c.k[a:a + L].float(), c.v[a:a + L].float()
        if pl:
            ks, vs = torch.cat([c.pk[:pl].float(), ks]), torch.cat([c.pv[:pl].float(), vs])
        sc = torch.einsum("lkgd,tkd->kglt", c.q[a:a + L].float().view(L, c.Hkv, c.G, D), ks) * F32_SCALE(c.scale)
        seen = torch.arange(pl + L)[None, :] <= (pl + torch.arange(L))[:, None]
        sc = sc.masked_fill(~seen, -math.inf)
        p = torch.exp2(sc - sc.amax(-1, keepdim=True))
        o = torch.einsum("kglt,tkd->lkgd", p.to(BF16).float(), vs) / p.sum(-1).permute(2, 0, 1)[..., None]
        out[a:a + L] = o.reshape(L, c.Hq, D).to(BF16)
        a += L
    return out


def F32_SCALE(scale):
    """scale * log2(e) as the launcher forms it: a product of two floats."""
    return float(torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32))


def _excess(got, c):
    """Per element (|got - o| - 2^-8 |o|) / A; where A == 0: 0 if got == 0 else inf."""
    got = got.double().cpu()
    err = (got - c.o).abs() - HALF_ULP * c.o.abs()
    live = c.A > 0
    return torch.where(live, err / torch.where(live, c.A, torch.ones_like(c.A)),
                       torch.where(got == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))


def _check(got, c, tau, label, dev):
    assert got.shape == c.o.shape and torch.isfinite(got.float()).all(), label
    if c.T == 0:
        return
    ex = _excess(got, c)
    worst = int(ex.argmax())
    t, h, d = worst // (c.Hq * D), worst // D % c.Hq, worst % D
    print(f"excess dev={dev} tau={'exact' if tau == TAU_EXACT else 'p'} {label}: {float(ex.max()):.3e} at row {t} "
          f"({int(c.row_keys[t])} keys) head {h} dim {d}")
    assert float(ex.max()) <= tau, (label, float(ex.max()), (t, h, d), float(got[t, h, d]), float(c.o[t, h, d]))


def _padded_work(lens, bq, dev, order=None):
    """ops.prefill_work_list's items with work_seq == -1 items at the head, in the middle and at
    the tail (optionally permuted), and cu_seqlens with two repeats of cu[-1] behind it."""
    ws, wq = ops.prefill_work_list(list(lens), bq)
    h = len(ws) // 2
    ws = [-1] + ws[:h] + [-1, -1] + ws[h:] + [-1]
    wq = [0] + wq[:h] + [0, 0] + wq[h:] + [0]
    if order is not None:
        ws, wq = [ws[i] for i in order], [wq[i] for i in order]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    cu += [cu[-1]] * 2
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    return i32(cu), i32(ws), i32(wq)


def _run(c, dev, variant=None):
    """ops.attn_prefill on ``dev`` with everything the call must not depend on or touch poisoned
    (module docstring). ``variant`` None: work=None, the default selection. Returns the T rows
    inside sequences."""
    nan = torch.full((PAD, 1, D), math.nan, dtype=BF16)
    q, k, v = (torch.cat([t, nan.expand(PAD, t.shape[1], D)]).to(dev) for t in (c.q, c.k, c.v))
    q0, k0, v0 = q.cpu(), k.cpu(), v.cpu()
    prefix = pk0 = pv0 = None
    if c.pfx is not None:
        pnan = torch.full((PFX_PAD, c.Hkv, D), math.nan, dtype=BF16)
        pk0, pv0 = torch.cat([c.pk, pnan]), torch.cat([c.pv, pnan])
        prefix = (pk0.to(dev), pv0.to(dev), torch.tensor(c.pfx + [0, 0], dtype=torch.int32, device=dev)
                  if dev == "cuda" else None, c.pfx)

    def call(order=None):
        out = torch.full((c.T + PAD, c.Hq, D), CANARY, dtype=BF16, device=dev)
        work = None
        if dev == "cuda" and variant is not None:
            work = _padded_work(c.lens, _block_q(variant, c.G), dev, order) + (variant,)
        r = ops.attn_prefill(q, k, v, c.lens, c.scale, out=out, work=work, prefix=prefix)
        if dev == "cuda":
            torch.cuda.synchronize()
        assert r.data_ptr() == out.data_ptr()
        o = out.cpu()
        assert (_bits(o[c.T:]) == _bits(torch.tensor(CANARY, dtype=BF16))).all(), "a row past cu[-1] was written"
        assert torch.isfinite(o[:c.T].float()).all(), "a row inside a sequence is not finite"
        assert (o[:c.T].float().abs() < 1e29).all(), "a row inside a sequence was not written"
        return o[:c.T]

    o = call()
    if dev == "cuda":
        assert _same_bits(o, call()), "a second identical call differs"
        if variant is not None:
            n = len(ops.prefill_work_list(c.lens, _block_q(variant, c.G))[0]) + 4
            assert _same_bits(o, call(torch.randperm(n, generator=_gen(n)).tolist())), "the work list's order matters"
    assert _same_bits(q, q0) and _same_bits(k, k0) and _same_bits(v, v0), "the call changed q / k / v"
    if prefix is not None:
        assert _same_bits(prefix[0], pk0) and _same_bits(prefix[1], pv0), "the call changed pk / pv"
    return o


# ---------------------------------------------------------------------------------------------
# census: scale 0, one-hot V: every key counted exactly once
# ---------------------------------------------------------------------------------------------

CENSUS_BASE = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 127, 128, 129]
CENSUS_PFX = [0, 1, 16, 63, 64, 65, 130, 192]
CENSUS_COMBOS = GRID + [(None, g) for g in DEFAULT_G]
# a prefix on v3 / v4: every G once, the variants alternating where both take G; and the default
CENSUS_PFX_COMBOS = [(3, 1), (4, 2), (3, 3), (4, 4), (3, 5), (3, 6), (3, 7), (3, 8), (4, 1), (3, 2), (4, 3), (3, 4),
                     (None, 4), (None, 8)]


def _census_lens(bq):
    """Both sides of every 16 / 32-row wave edge, 64-key tile edge and block_q edge, an empty
    sequence in the middle; the longest sequence is 2 block_q + 1 <= 513 rows."""
    return tuple(CENSUS_BASE + [n for n in (bq - 1, bq, bq + 1) if n not in CENSUS_BASE] + [2 * bq + 1])


def _census_pfx_lens(bq):
    return (bq + 1, 33, 1, 2 * bq + 1, 64, 17, 65, bq - 1)


def _one_hot(n, Hkv, mul, add):
    """V[t][kvh] one-hot at dim (mul t + add + 17 kvh) % 128."""
    v = torch.zeros(n, Hkv, D)
    t = torch.arange(n)
    for kvh in range(Hkv):
        v[t, kvh, (mul * t + add + 17 * kvh) % D] = 1.0
    return v


@functools.lru_cache(maxsize=None)
def _census_case(lens, G, prefix):
    g = _gen(100 + G + len(lens) + sum(lens))
    q = [_randn(g, n, G * HKV, D) for n in lens]
    k = [_randn(g, n, HKV, D) for n in lens]
    v = [_one_hot(n, HKV, 1, 0) for n in lens]
    if prefix:
        P = max(CENSUS_PFX)
        c = _case(q, k, v, lens, 0.0, CENSUS_PFX, _randn(g, P, HKV, D), _one_hot(P, HKV, 3, 5))
    else:
        c = _case(q, k, v, lens, 0.0)
    # the fp64 answer: element d of row r is (keys of the row with a 1 at d) / (pl + r + 1), exactly
    a = 0
    for s, n in enumerate(lens):
        pl = CENSUS_PFX[s] if prefix else 0
        for kvh in range(HKV):
            cnt = v[s][:, kvh].double().cumsum(0)
            if pl:
                cnt = cnt + c.pv[:pl, kvh].double().sum(0)
            want = cnt / (pl + 1 + torch.arange(n, dtype=torch.float64))[:, None]
            for h in range(G):
                assert (c.o[a:a + n, kvh * G + h] - want).abs().max() < 1e-15 if n else True
        a += n
    assert torch.equal(c.o, c.A)
    return c


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", CENSUS_COMBOS, ids=_ids(CENSUS_COMBOS))
def test_census_every_key_counted_once(variant, G, dev):
    """Uniform weights over one-hot V rows: element d of row r is (keys t <= r with t % 128 == d)
    / (r + 1), so a key dropped, duplicated, double-weighted or leaked through the causal mask
    moves an element by 1 / (r + 1) >= 1 / 513, two thousand times the tolerance. Lengths sit on
    both sides of every wave, key-tile and block_q edge of the variant; every (variant, G) of the
    grid, the idle waves of G = 3, 5, 6, 7 included, and the default selection."""
    c = _census_case(_census_lens(_bq(variant, G)), G, False)
    _check(_run(c, dev, variant), c, TAU_EXACT, f"census v={variant} G={G}", dev)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", CENSUS_PFX_COMBOS, ids=_ids(CENSUS_PFX_COMBOS))
def test_census_with_prefix(variant, G, dev):
    """The same census over [prefix ++ own] keys, prefix lengths 0, 1, 16, 63, 64, 65, 130, 192 in
    one batch over one pk / pv of 192 rows: a sequence that read a prefix row past its own
    length, or missed one, or lost an own key behind a partial prefix tile, miscounts."""
    c = _census_case(_census_pfx_lens(_bq(variant, G)), G, True)
    _check(_run(c, dev, variant), c, TAU_EXACT, f"census+prefix v={variant} G={G}", dev)


# ---------------------------------------------------------------------------------------------
# witness / anti-witness: one key takes (almost) all of a row's weight, or would if it leaked
# ---------------------------------------------------------------------------------------------

def _hadamard():
    h = torch.ones(1, 1)
    for _ in range(7):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)])
    return h


H128 = _hadamard()       # 128 mutually orthogonal +-1 rows: one direction per (sequence, kv-head)
MULT = 6.0               # a spiked key is MULT x its direction: ~ MULT sqrt(128) nats = 98 log2 units


def _dir(s, kvh):
    return H128[(HKV * s + kvh) % D]


def _witness_v():
    d = torch.arange(D)
    # [Hkv, D], bf16-exact, no element 0
    return torch.stack([(d % 13 - 6).float() * 0.5 + 0.25 + kvh for kvh in range(HKV)])


def _spike_case(seqs, G, pfx_spikes=(), seed=0):
    """seqs: per sequence (L, pl or None, [(own key t, sequence whose direction it carries)]).
    Every query row of sequence s, head (kvh, g) is dir(s, kvh) + 0.5 noise; keys are 0.25 noise
    except the spiked ones, MULT x the direction of the sequence they are aimed at, whose V row is
    _witness_v. pfx_spikes: (prefix row j, sequence aimed at) on the shared prefix."""
    g = _gen(200 + seed + G)
    q, k, v = [], [], []
    for s, (L, _, spikes) in enumerate(seqs):
        base = torch.stack([_dir(s, kvh) for kvh in range(HKV)])                      # [Hkv, D]
        q.append((base[None, :, None] + _randn(g, L, HKV, G, D, scale=0.5)).reshape(L, HKV * G, D))
        ks, vs = _randn(g, L, HKV, D, scale=0.25), _randn(g, L, HKV, D)
        for t, aim in spikes:
            ks[t] = MULT * torch.stack([_dir(aim, kvh) for kvh in range(HKV)])
            vs[t] = _witness_v()
        k.append(ks)
        v.append(vs)
    lens = [L for L, _, _ in seqs]
    if seqs[0][1] is None:
        return _case(q, k, v, lens, SCALE, keep_p=True)
    pfx = [pl for _, pl, _ in seqs]
    pk, pv = _randn(g, max(pfx), HKV, D, scale=0.25), _randn(g, max(pfx), HKV, D)
    for j, aim in pfx_spikes:
        pk[j] = MULT * torch.stack([_dir(aim, kvh) for kvh in range(HKV)])
        pv[j] = _witness_v()
    return _case(q, k, v, lens, SCALE, pfx, pk, pv, keep_p=True)


def _assert_witness(c, s, key, rows):
    """CPU-side condition: key ``key`` (index into [prefix ++ own]) holds >= 1 - 2^-12 of the weight
    of every head in rows ``rows`` of sequence s, so the fp64 output is its V row to 2^-12."""
    p = c.p[s][:, rows, key]
    assert float(p.min()) >= 1 - 2.0 ** -12, (s, key, float(p.min()))
    a = sum(c.lens[:s])
    pl = c.pfx[s] if c.pfx is not None else 0
    vrow = (c.pv[key] if key < pl else c.v[a + key - pl]).double().repeat_interleave(c.G, 0)
    vmax = max(float(c.v.abs().max()), float(c.pv.abs().max()) if c.pv is not None else 0.0)
    o = c.o[a:a + c.lens[s]][rows]
    assert ((o - vrow).abs() <= 2.0 ** -12 * (vrow.abs() + vmax)).all()


def _assert_would_dominate(c, s, rows, kvec):
    """The key vector kvec [Hkv, D], which rows ``rows`` of sequence s must not see, would take
    >= 1 - 2^-12 of their weight if they did: its score is 12 log2 units above the row's
    log-sum-exp over the keys it does see."""
    a = sum(c.lens[:s])
    L = c.lens[s]
    sc = torch.einsum("lkgd,kd->kgl", c.q[a:a + L].double().view(L, c.Hkv, c.G, D), kvec.to(BF16).double()) * c.scale
    margin = (sc.reshape(c.Hq, L) - c.lse[s])[:, rows] / math.log(2)
    assert float(margin.min()) >= 12, (s, float(margin.min()))


def _witness_positions(bq):
    """Own-key positions of the witness, one sequence each: key 0; both sides of the 16- and 32-row
    wave edges, of the 64-key tile edges 63 | 64 and 127 | 128 and of the block_q edge; the last
    key. With the witness at t, row t has it on the diagonal, row t + 1 at key r - 1, and row
    t - 1 must not see it (the causal anti-witness)."""
    L = max(bq, 128) + 34
    return sorted({0, 15, 16, 31, 32, 63, 64, 127, 128, bq - 1, bq, bq + 1, L - 1}), L


@functools.lru_cache(maxsize=None)
def _witness_case(bq, G):
    pos, L = _witness_positions(bq)
    c = _spike_case([(L, None, [(t, s)]) for s, t in enumerate(pos)], G)
    for s, t in enumerate(pos):
        _assert_witness(c, s, t, slice(t, L))
        if t > 0:       # rows before t: the key after their diagonal would dominate them
            _assert_would_dominate(c, s, slice(0, t), c.k[sum(c.lens[:s]) + t].float())
    del c.p
    return c


def test_witness_positions_are_the_boundaries():
    """For every (variant, G) of the grid the witness sits on both sides of the variant's wave
    edge (16 rows: v1 / v2, 32 rows: v3 / v4), of the key-tile edges and of its block_q edge, with
    at least two rows behind every position but the last."""
    for variant, G in GRID:
        bq = ops.prefill_block_q(2 * G, 2, variant)
        assert bq == _block_q(variant, G) and bq in (16, 32, 64, 128, 256)
        pos, L = _witness_positions(bq)
        wave = 16 if variant <= 2 else 32
        assert {0, wave - 1, wave, 63, 64, 127, 128, bq - 1, bq, L - 1} <= set(pos)
        assert all(t + 2 < L for t in pos[:-1]) and L > bq + 2 and L <= 513


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", CENSUS_COMBOS, ids=_ids(CENSUS_COMBOS))
def test_witness_boundary_key_carries_the_answer(variant, G, dev):
    """One sequence per boundary position t, whose key t holds >= 1 - 2^-12 of the weight of
    every row r >= t: those rows are V[t]; rows r < t, which key t would dominate as thoroughly if
    the mask let it through, are the near-uniform average of their own keys. A mask off by one
    replaces a whole row (error ~ |V|, four hundred times the tolerance). The max of a row jumps
    by ~98 log2 units where the witness enters."""
    c = _witness_case(_bq(variant, G), G)
    _check(_run(c, dev, variant), c, TAU_P, f"witness v={variant} G={G}", dev)


# sequence ends: the first key of the next packed sequence carries a spike aimed at this one, whose
# last key tile is partly filled (70, 33, 1, 129, 65, 300 keys) or exactly full (64, 128)
ENDS_LENS = [70, 0, 33, 1, 64, 129, 65, 128, 300, 5]


@functools.lru_cache(maxsize=None)
def _ends_case(G):
    seqs, prev = [], None
    for s, L in enumerate(ENDS_LENS):
        seqs.append((L, None, [(0, prev)] if prev is not None and L else []))
        prev = s if L else prev
    c = _spike_case(seqs, G, seed=1)
    prev = None
    for s, L in enumerate(ENDS_LENS):
        if prev is not None and L:
            _assert_would_dominate(c, prev, slice(0, ENDS_LENS[prev]), c.k[sum(ENDS_LENS[:s])].float())
        prev = s if L else prev
    del c.p
    return c


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", CENSUS_COMBOS, ids=_ids(CENSUS_COMBOS))
def test_anti_witness_next_sequence_does_not_leak(variant, G, dev):
    """The row of k / v right behind each sequence (the next one's first key; behind an empty
    sequence too) would take every row of this sequence if a partly filled last tile let it in."""
    c = _ends_case(G)
    _check(_run(c, dev, variant), c, TAU_P, f"ends v={variant} G={G}", dev)


# a shared prefix of 192 rows. Per sequence (own length, prefix length, what is spiked):
#   0: pl 130, witness = prefix key 129, the last key of a partial last prefix tile
#   1: pl  64, witness = prefix key 63, the last key of a whole prefix tile
#   2: pl  65, witness = own key 0, right behind a one-key prefix tile
#   3: pl 192, witness = prefix key 191
#   4: pl   1, witness = prefix key 0
#   5: pl 100, anti-witness: prefix row 100 (in its partial tile) is aimed at it
#   6: pl 128, anti-witness: prefix row 128 (the first row of the next tile) is aimed at it
#   7: pl   0, anti-witness: prefix row 0 is sequence 4's witness, rows 1.. belong to others
#   8: pl  63, witness = own key 1 behind a 63-key prefix tile; row 0 must not see it
PFX_SEQS = [(70, 130), (33, 64), (97, 65), (40, 192), (65, 1), (66, 100), (34, 128), (35, 0), (64, 63)]
PFX_SPIKES = [(129, 0), (63, 1), (191, 3), (0, 4), (100, 5), (128, 6)]
PFX_OWN = {2: 0, 8: 1}


@functools.lru_cache(maxsize=None)
def _pfx_witness_case(G):
    c = _spike_case([(L, pl, [(PFX_OWN[s], s)] if s in PFX_OWN else []) for s, (L, pl) in enumerate(PFX_SEQS)], G,
                    PFX_SPIKES, seed=2)
    for j, s in PFX_SPIKES:
        L, pl = PFX_SEQS[s]
        if j < pl:
            _assert_witness(c, s, j, slice(0, L))
        else:
            assert j == pl       # the row just past this sequence's prefix, valid for a longer one
            _assert_would_dominate(c, s, slice(0, L), c.pk[j].float())
    for s, t in PFX_OWN.items():
        _assert_witness(c, s, PFX_SEQS[s][1] + t, slice(t, PFX_SEQS[s][0]))
    _assert_would_dominate(c, 8, slice(0, 1), c.k[sum(L for L, _ in PFX_SEQS[:8]) + 1].float())
    del c.p
    return c


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", CENSUS_PFX_COMBOS, ids=_ids(CENSUS_PFX_COMBOS))
def test_witness_and_anti_witness_in_the_prefix(variant, G, dev):
    """The witness on the last prefix key (whole and partial last tile), on the first own key
    behind a prefix, on prefix keys 0 and 191; and prefix rows just past seq_pfx[s], valid for
    the longer-prefix sequences of the batch, that would take every row of s if it saw them."""
    c = _pfx_witness_case(G)
    _check(_run(c, dev, variant), c, TAU_P, f"prefix witness v={variant} G={G}", dev)


# ---------------------------------------------------------------------------------------------
# the deferred rescale of v3 / v4 (run on every variant): controlled scores
# ---------------------------------------------------------------------------------------------
# q and k lie along dim 0 with bf16-exact magnitudes and scale = ln 2, so a raw dot product IS
# the score in log2 units (exact in fp32: one non-zero product). Head g multiplies its rows by
# 1 + g / 8 and every third row by 1 / 2, so the planted rises of 7.9375 / 8 / 8.0625 (just under,
# on and just over the `mnew > mrow + 8` threshold for head 0) land on both sides of it across
# heads and rows. Unplanted keys score 0, -0.25, .. -1.
RESCALE_L = 300          # five key tiles
RESCALE_OWN = {
    "under": {70: 7.9375}, "on": {70: 8.0}, "over": {70: 8.0625},
    "under_then_over": {70: 7.9375, 140: 16.0},               # 16 is 8.0625 over 7.9375 but 16 over the kept 0
    "stairs": {74: 7.0, 138: 14.0, 202: 21.0, 266: 28.0},      # +7 a tile: kept 0, 0, 14, 14, 28
    "drop": {3: 100.0},                                        # every later tile ~100 below the kept max
    "leap": {200: 160.0},                                      # one rise of 160: rescaled, or exp2 overflows
    "short": {64: 8.0625, 129: 16.125},
}
RESCALE_COMBOS = [(1, 1), (1, 4), (2, 2), (2, 8), (3, 1), (3, 2), (3, 3), (3, 5), (3, 8), (4, 1), (4, 3), (4, 4),
                  (None, 2), (None, 7)]
# with a prefix: the rises start in the prefix tiles (pk: 7.9375 at row 70, 14 at row 130) and go
# on in the own tiles; (own length, prefix length, own spikes)
RESCALE_PFX = [(140, 64, {5: 8.0625}), (140, 100, {5: 8.0625, 70: 16.0}), (140, 128, {5: 14.0, 70: 21.0}),
               (200, 192, {5: 21.0, 70: 28.0, 140: 160.0}), (70, 130, {5: 7.0}), (70, 1, {}), (33, 0, {40 - 8: 8.0}),
               (130, 131, {5: 100.0})]
RESCALE_PFX_PK = {70: 7.9375, 130: 14.0}
RESCALE_PFX_COMBOS = [(3, 1), (3, 3), (3, 6), (3, 8), (4, 2), (4, 4), (None, 1)]
# the largest score sits in prefix tile 0, everything after it ~100 below
DROP_PFX = [(70, 1, {}), (70, 6, {}), (130, 64, {}), (140, 130, {60: 50.0})]
DROP_PFX_PK = {5: 100.0}


def _axis_rows(n, H, mags):
    x = torch.zeros(n, H, D)
    x[:, :, 0] = mags
    return x


def _axis_case(G, seqs, pk_spikes=None, seed=0):
    """seqs: (L, pl or None, {own key: score for head 0 of an unhalved row})."""
    g = _gen(300 + G + seed)
    head = (1 + torch.arange(G) / 8.0).repeat(HKV)                                     # [Hq]
    jitter = lambda n: -0.25 * (torch.arange(n) % 5).float()  # noqa: E731
    q, k, v = [], [], []
    for L, _, spikes in seqs:
        row = torch.where(torch.arange(L) % 3 == 2, 0.5, 1.0)
        q.append(_axis_rows(L, G * HKV, row[:, None] * head[None, :]))
        b = jitter(L)
        for t, x in spikes.items():
            b[t] = x
        k.append(_axis_rows(L, HKV, b[:, None].expand(L, HKV)))
        v.append(_randn(g, L, HKV, D))
    lens = [L for L, _, _ in seqs]
    for t in q + k:
        assert torch.equal(t.to(BF16).float(), t)
    if pk_spikes is None:
        return _case(q, k, v, lens, math.log(2))
    pfx = [pl for _, pl, _ in seqs]
    b = jitter(max(pfx))
    for j, x in pk_spikes.items():
        b[j] = x
    return _case(q, k, v, lens, math.log(2), pfx, _axis_rows(max(pfx), HKV, b[:, None].expand(-1, HKV)),
                 _randn(g, max(pfx), HKV, D))


@functools.lru_cache(maxsize=None)
def _rescale_case(G, kind):
    if kind == "own":
        return _axis_case(G, [(130 if n == "short" else RESCALE_L, None, sp) for n, sp in RESCALE_OWN.items()])
    if kind == "prefix":
        return _axis_case(G, RESCALE_PFX, RESCALE_PFX_PK, seed=1)
    return _axis_case(G, DROP_PFX, DROP_PFX_PK, seed=2)


def test_rescale_cases_straddle_the_threshold():
    """What the patterns promise, from the case's own bf16 inputs: ln 2 * log2(e) is 1 to a float
    ulp, head 0's unhalved rows see tile maxima that rise by 7.9375, 8 and 8.0625, the staircase
    rises by 7 per tile, and with the other heads' factors the rises cover both sides of 8."""
    assert abs(F32_SCALE(math.log(2)) - 1) < 2e-7
    c = _rescale_case(4, "own")
    names = list(RESCALE_OWN)
    rises = set()
    for s, n in enumerate(names):
        a = sum(c.lens[:s])
        b = c.k[a:a + c.lens[s], 0, 0].float()
        tiles = [float(b[i:i + 64].max()) for i in range(0, c.lens[s], 64)]
        if n in ("under", "on", "over"):
            assert tiles[0] == 0 and tiles[1] == {"under": 7.9375, "on": 8.0, "over": 8.0625}[n]
        if n == "stairs":
            assert tiles == [0.0, 7.0, 14.0, 21.0, 28.0]
        if n == "drop":
            assert tiles[0] == 100 and max(tiles[1:]) == 0
        for h in range(4):
            f = float(c.q[a, h, 0])
            rises |= {f * (y - x) for x, y in zip(tiles, tiles[1:]) if y > x}
    assert min(rises) < 8 < max(rises) and any(7.9 < r < 8 for r in rises) and any(8 < r < 8.1 for r in rises)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", RESCALE_COMBOS, ids=_ids(RESCALE_COMBOS))
def test_deferred_rescale(variant, G, dev):
    """A row's kept max against tile maxima that rise by just under, exactly and just over 8, by
    7 a tile over four tiles (each below the threshold against the kept max until two add up), that
    drop by 100 after tile 0, and that leap by 160 (not rescaled, exp2 overflows fp32)."""
    c = _rescale_case(G, "own")
    _check(_run(c, dev, variant), c, TAU_P, f"rescale v={variant} G={G}", dev)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("kind", ["prefix", "prefix_drop"])
@pytest.mark.parametrize("variant,G", RESCALE_PFX_COMBOS, ids=_ids(RESCALE_PFX_COMBOS))
def test_deferred_rescale_from_a_prefix_tile(variant, G, kind, dev):
    """The same patterns starting in the prefix tiles (whole and partial) and continuing into
    the sequence's own tiles; and the largest score in prefix tile 0 with all else 100 below."""
    c = _rescale_case(G, kind)
    _check(_run(c, dev, variant), c, TAU_P, f"rescale {kind} v={variant} G={G}", dev)


# ---------------------------------------------------------------------------------------------
# randn sanity: overall arithmetic
# ---------------------------------------------------------------------------------------------

RANDN_LENS = [[1, 33, 64, 200, 97, 0, 5, 40], [300, 17, 129, 64, 2, 255]]
RANDN_PFX = [[64, 0, 192, 96, 128, 7, 0, 112], [130, 1, 63, 0, 65, 16]]


@functools.lru_cache(maxsize=None)
def _randn_case(i, G, prefix):
    g = _gen(400 + i + G)
    lens = RANDN_LENS[i]
    q = [_randn(g, n, G * HKV, D) for n in lens]
    k, v = [_randn(g, n, HKV, D) for n in lens], [_randn(g, n, HKV, D) for n in lens]
    if not prefix:
        return _case(q, k, v, lens, SCALE)
    P = max(RANDN_PFX[i])
    return _case(q, k, v, lens, SCALE, RANDN_PFX[i], _randn(g, P, HKV, D), _randn(g, P, HKV, D))


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", CENSUS_COMBOS, ids=_ids(CENSUS_COMBOS))
def test_randn(variant, G, dev):
    """Two batches of mixed lengths. With TAU_P ~ 2^-8 this sees a wrong scale, a wrong head
    mapping or a wrong softmax, not a one-key miscount (module docstring)."""
    for i in range(2):
        c = _randn_case(i, G, False)
        _check(_run(c, dev, variant), c, TAU_P, f"randn[{i}] v={variant} G={G}", dev)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("variant,G", CENSUS_PFX_COMBOS, ids=_ids(CENSUS_PFX_COMBOS))
def test_randn_with_prefix(variant, G, dev):
    for i in range(2):
        c = _randn_case(i, G, True)
        _check(_run(c, dev, variant), c, TAU_P, f"randn+prefix[{i}] v={variant} G={G}", dev)


def test_bf16_weight_emulation_is_within_tau_p():
    """Figure (b) of the module docstring: the kernels' arithmetic emulated on the CPU, over one
    case of every non-census family."""
    cases = {"witness": _witness_case(64, 4), "ends": _ends_case(4), "prefix witness": _pfx_witness_case(4),
             "rescale": _rescale_case(4, "own"), "rescale prefix": _rescale_case(4, "prefix"),
             "rescale prefix_drop": _rescale_case(4, "prefix_drop"), "randn[0]": _randn_case(0, 4, False),
             "randn[1]": _randn_case(1, 4, False), "randn+prefix[0]": _randn_case(0, 4, True),
             "randn+prefix[1]": _randn_case(1, 4, True)}
    for name, c in cases.items():
        _check(_emulate(c), c, TAU_P, name, "emu")
    c = _census_case(_census_lens(64), 4, False)
    _check(_emulate(c), c, TAU_EXACT, "census", "emu")


# ---------------------------------------------------------------------------------------------
# the binding (gpu only): block_q, refusals and their accepted neighbours
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_block_q_matches_the_native_function():
    native = ops.kernels().attn_prefill_block_q
    for variant, G in GRID:
        assert ops.prefill_block_q(2 * G, 2, variant) == native(2 * G, 2, variant) == _block_q(variant, G)
    for G in DEFAULT_G:
        assert ops.prefill_block_q(2 * G, 2) == native(2 * G, 2, ops.prefill_variant(2 * G, 2)) == _bq(None, G)
    for variant in range(0, 6):
        for G in (1, 2, 3, 4, 5, 8, 9, 16):
            assert native(2 * G, 2, variant) == _block_q(variant, G)
    assert native(7, 2, 3) == -1 and native(7, 2, 1) == 64


def _refusal_args(T=40, Hq=8, Hkv=2, Dh=D, lens=(17, 23), q_dtype=BF16, k_strided=False, wq_extra=0, P=0, pfx_n=None,
                  pk_hkv=None, ws=None):
    dev = "cuda"
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    a = SimpleNamespace(q=torch.ones(T, Hq, Dh, dtype=q_dtype, device=dev),
                        k=torch.ones(T, Hkv, Dh, dtype=BF16, device=dev),
                        v=torch.ones(T, Hkv, Dh, dtype=BF16, device=dev),
                        out=torch.full((T, Hq, Dh), CANARY, dtype=BF16, device=dev), cu=i32(cu), lens=list(lens))
    if k_strided:
        a.k = torch.ones(T, Hkv, 2 * Dh, dtype=BF16, device=dev)[:, :, ::2]
    work = ops.prefill_work_list(list(lens), 32) if ws is None else (ws, [0] * len(ws))
    a.ws, a.wq = i32(work[0]), i32(work[1] + [0] * wq_extra)
    a.prefix = ()
    if P:
        pk = torch.ones(P, pk_hkv or Hkv, Dh, dtype=BF16, device=dev)
        a.prefix = (pk, pk.clone(), i32([P] * (len(lens) if pfx_n is None else pfx_n)))
    return a


def _call(a, variant):
    ops.kernels().attn_prefill(a.q, a.k, a.v, a.out, a.cu, a.ws, a.wq, SCALE, variant, *a.prefix)
    torch.cuda.synchronize()


# name: (arguments, variant). Hq = 8, Hkv = 2 (G = 4) unless the arguments say otherwise
REFUSALS = {
    "v2_G3": (dict(Hq=6), 2), "v4_G8": (dict(Hq=16), 4), "v3_G16": (dict(Hq=32), 3), "variant0": (dict(), 0),
    "variant5": (dict(), 5), "prefix_v1": (dict(P=16), 1), "prefix_v2": (dict(P=16), 2),
    "q_fp16": (dict(q_dtype=torch.float16), 4), "k_strided": (dict(k_strided=True), 4), "head_dim64": (dict(Dh=64), 4),
    "Hq_not_multiple": (dict(Hq=7), 1), "work_lengths_differ": (dict(wq_extra=1), 4),
    "seq_pfx_short": (dict(P=16, pfx_n=1), 4), "pk_wrong_Hkv": (dict(P=16, pk_hkv=1), 4),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_launch_nothing(name):
    """What the kernels do not take raises, and ``out`` is still all canary."""
    kw, variant = REFUSALS[name]
    a = _refusal_args(**kw)
    with pytest.raises(RuntimeError):
        _call(a, variant)
    assert (a.out == CANARY).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2])
def test_ops_refuses_a_prefix_on_v1_v2(variant):
    a = _refusal_args(P=16)
    with pytest.raises(ValueError):
        ops.attn_prefill(a.q, a.k, a.v, a.lens, SCALE, out=a.out, work=(a.cu, a.ws, a.wq, variant),
                         prefix=a.prefix + (None,))
    torch.cuda.synchronize()
    assert (a.out == CANARY).all()


@pytest.mark.gpu
def test_accepted_neighbours_of_the_refusals():
    """The same arguments with what the kernels do take run (the refusals above are not refusals
    of the helper's buffers): K = V = 1 gives rows of ones. An empty work list and one that is all
    -1 return with ``out`` untouched; a single sequence of length 1 succeeds."""
    for kw, variant in ((dict(), 4), (dict(), 3), (dict(Hq=6), 3), (dict(Hq=16), 3), (dict(P=16), 4), (dict(P=16), 3),
                        (dict(Hq=32), 1), (dict(P=16, pfx_n=3), 4)):
        a = _refusal_args(**kw)
        ws, wq = ops.prefill_work_list(a.lens, _block_q(variant, kw.get("Hq", 8) // 2))
        a.ws = torch.tensor(ws, dtype=torch.int32, device="cuda")
        a.wq = torch.tensor(wq, dtype=torch.int32, device="cuda")
        _call(a, variant)
        assert (a.out == 1).all(), (kw, variant)
    for ws in ([], [-1, -1, -1]):
        for variant in (1, 2, 3, 4):
            a = _refusal_args(ws=ws)
            _call(a, variant)
            assert (a.out == CANARY).all(), (ws, variant)
    for variant in (None, 1, 2, 3, 4):
        a = _refusal_args(T=1, lens=(1,))
        work = None if variant is None else (a.cu, torch.zeros(1, dtype=torch.int32, device="cuda"),
                                             torch.zeros(1, dtype=torch.int32, device="cuda"), variant)
        o = ops.attn_prefill(a.q, a.k, a.v, [1], SCALE, out=a.out, work=work)
        assert (o == 1).all()


# ---------------------------------------------------------------------------------------------
# host side (CPU): the work list and the variant selection
# ---------------------------------------------------------------------------------------------

def test_work_list_tiles_every_row_once():
    """For random length lists and every block_q of the grid: the items cover every row of every
    sequence exactly once, an empty sequence yields no item, q0 is a multiple of block_q and
    non-increasing down the list (the long-causal blocks first)."""
    g = _gen(7)
    for bq in (16, 32, 64, 128, 256):
        for trial in range(20):
            n = int(torch.randint(0, 9, (1,), generator=g))
            lens = [int(x) for x in torch.randint(0, 3 * bq + 2, (n,), generator=g)]
            if trial % 4 == 0 and n:
                lens[n // 2] = 0
            ws, wq = ops.prefill_work_list(lens, bq)
            assert len(ws) == len(wq) == sum(-(-L // bq) for L in lens)
            assert all(a >= b for a, b in zip(wq, wq[1:]))
            seen = [torch.zeros(L, dtype=torch.int32) for L in lens]
            for s, q0 in zip(ws, wq):
                assert 0 <= s < n and q0 % bq == 0 and q0 < lens[s]
                seen[s][q0:q0 + bq] += 1
            assert all((t == 1).all() for t in seen)
    assert ops.prefill_work_list([], 64) == ([], []) and ops.prefill_work_list([0, 0], 64) == ([], [])
    assert ops.prefill_work_list([5]) == ([0], [0])


@pytest.mark.parametrize("env", [None, "v1", "v2", "v3", "v4", "v9"])
def test_variant_selection_and_fallback(env, monkeypatch):
    """ops.prefill_variant under each OAMD_PREFILL_ATTN: the asked variant where it takes G, a
    grouped variant that cannot falls back to v3, then v1 (G > 8, or Hq no multiple of Hkv); never
    a variant whose block_q the kernel refuses, and ops.prefill_block_q agrees with the kernel's."""
    if env is None:
        monkeypatch.delenv("OAMD_PREFILL_ATTN", raising=False)
    else:
        monkeypatch.setenv("OAMD_PREFILL_ATTN", env)
    for G in list(range(1, 9)) + [16]:
        got = ops.prefill_variant(2 * G, 2)
        asked = {None: 4 if G <= 4 else 3, "v9": 4 if G <= 4 else 3}.get(env) or int(env[1])
        want = asked if _block_q(asked, G) > 0 else 3 if _block_q(3, G) > 0 else 1
        if G > 8:
            want = 1
        assert got == want, (env, G, got, want)
        assert _block_q(got, G) > 0 and ops.prefill_block_q(2 * G, 2) == _block_q(got, G)
    assert ops.prefill_variant(7, 2) == 1 and ops.prefill_block_q(7, 2) == 64
    assert ops.prefill_variant(8, 0) == 1
