"""Row-wise kernels (sample, rmsnorm, silu_mul, embedding, quantize_fp8, silu_quantize_fp8, the
fp8 store of rope_kv): every launch path, stride and numeric edge.

Each case's inputs are built on the CPU by a plain function and each property is asserted by a
plain checker. Every test takes a device: ``hip`` (marked gpu) runs the gfx950 kernels, ``ref``
feeds the same inputs through the torch fallbacks (``ops.*`` on CPU tensors) into the same
checkers, so every invariant asserted of a kernel is shown to hold for the reference first, on
a machine without a GPU. What only a binding can do (raising before a launch, behaviour the
reference does not share) is in tests marked gpu.
"""
import functools
import math

import pytest
import torch

from operator_amd import ops
from operator_amd.ops import reference as ref

DEVS = [pytest.param("cpu", id="ref"), pytest.param("cuda", marks=pytest.mark.gpu, id="hip")]
BF16, F32, E4M3 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
CANARY = 7.0          # bf16-exact; no kernel here writes it by accident into a whole region
TOL = dict(atol=2e-2, rtol=2e-2)   # the project's tolerance for rmsnorm / silu_mul


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0, dtype=BF16):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _strided(t, dev, pad_left, pad_right, fill=CANARY):
    """``t`` [rows, cols] as a column slice of a wider ``fill``-ed buffer on ``dev``:
    returns (view, buffer, column mask of the view)."""
    rows, cols = t.shape
    buf = torch.full((rows, pad_left + cols + pad_right), fill, dtype=t.dtype)
    buf[:, pad_left:pad_left + cols] = t
    buf = buf.to(dev)
    inside = torch.zeros(buf.shape[1], dtype=torch.bool)
    inside[pad_left:pad_left + cols] = True
    return buf[:, pad_left:pad_left + cols], buf, inside


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.uint8 if t.element_size() == 1
                                     else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# sample
# ---------------------------------------------------------------------------------------------

SAMPLE_PATH_SHAPES = [(BF16, 41003), (F32, 20503)] + [(dt, v) for v in (1, 7, 8, 1003) for dt in (BF16, F32)]
SAMPLE_TEMPS = [0.0, 0.3, 1.0, 0.0, 2.0, 1.0]


@functools.lru_cache(maxsize=None)
def _sample_case(dtype, V):
    """6 rows mixing greedy and T in {0.3, 1, 2}, with the fp64 reference tokens and values."""
    g = _gen(1000 + V)
    logits = _randn(g, 6, V, scale=3.0, dtype=dtype)
    temp = torch.tensor(SAMPLE_TEMPS)
    seeds = torch.arange(6) * 7 + 1
    pos = torch.arange(6) + 100
    tok, val = ref.sample_shard(logits, temp, seeds, pos)
    return logits, temp, seeds, pos, tok, val


def _sample_layout(logits, layout, dev):
    """aligned: a [:, :V] slice of rows whose stride is a multiple of 8 (vector body + scalar
    tail); unaligned: a [:, 1:V+1] slice of the same (every row off a 16-B boundary: all
    scalar); contig: [rows, V] as is (alignment changes from row to row when V is odd)."""
    rows, V = logits.shape
    if layout == "contig":
        return logits.to(dev)
    stride = (V + 1 + 7) // 8 * 8 + 8
    buf = torch.full((rows, stride), 1e4, dtype=logits.dtype)   # a canary that would win any row
    c0 = 0 if layout == "aligned" else 1
    buf[:, c0:c0 + V] = logits
    view = buf.to(dev)[:, c0:c0 + V]
    assert (view.data_ptr() % 16 == 0) == (layout == "aligned")
    return view


def _run_sample(logits, temp, seeds, pos, dev, col_offset=0):
    rows = logits.shape[0]
    out = torch.full((rows,), -7, dtype=torch.long, device=dev)
    val = torch.full((rows,), float("nan"), dtype=F32, device=dev)
    tok = ops.sample(logits, temp.to(dev), seeds.to(dev), pos.to(dev), out=out, col_offset=col_offset, out_val=val)
    assert tok.data_ptr() == out.data_ptr()
    return out.cpu(), val.cpu()


def _check_sample_matches_ref(case, tok, val, col_offset=0):
    """The reference token, or (fp32 vs fp64 near-ties only) one whose perturbed value is within
    1e-3 of the reference's; the winning value within 1e-3 of the reference's."""
    logits, temp, seeds, pos, tok_r, val_r = case
    V = logits.shape[1]
    assert ((tok >= col_offset) & (tok < col_offset + V)).all(), tok
    for r in range(logits.shape[0]):
        if tok[r] != tok_r[r]:
            x = logits[r].double()
            if float(temp[r]) > 0:
                x = x / float(temp[r]) + ref.gumbel_noise_ref(int(seeds[r]), int(pos[r]), V, col_offset)
            assert abs(float(x[tok[r] - col_offset] - x[tok_r[r] - col_offset])) < 1e-3, (r, tok[r], tok_r[r])
    torch.testing.assert_close(val, val_r, atol=1e-3, rtol=0)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("layout", ["aligned", "unaligned", "contig"])
@pytest.mark.parametrize("dtype,V", SAMPLE_PATH_SHAPES, ids=lambda p: str(p).replace("torch.", ""))
def test_sample_paths(dtype, V, layout, dev):
    """41003 bf16 / 20503 fp32: 5125 vectors + 3 scalars per aligned row: one four-way unrolled
    round, a remainder round taken by every thread, one taken by five, then the scalar tail;
    unaligned rows take the all-scalar fallback. 1 / 7 / 8 / 1003: no vector, one vector, no
    unrolled round."""
    case = _sample_case(dtype, V)
    logits, temp, seeds, pos = case[:4]
    x = _sample_layout(logits, layout, dev)
    tok, val = _run_sample(x, temp, seeds, pos, dev)
    _check_sample_matches_ref(case, tok, val)
    tok2, val2 = _run_sample(x, temp, seeds, pos, dev)   # replay
    assert torch.equal(tok, tok2) and _same_bits(val, val2)


def _sample_regions(dtype, V):
    """One column in each region an aligned row is visited by: column 0, the unrolled body,
    the remainder rounds, the scalar tail (V - 1)."""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    nv = V // vec
    unrolled = nv // 4096 * 4096 * vec
    assert 0 < unrolled < nv * vec < V
    return [0, unrolled // 3 + 1, (unrolled + nv * vec) // 2 + 1, V - 1]


@functools.lru_cache(maxsize=None)
def _sample_planted_case(dtype, V):
    cols = _sample_regions(dtype, V)
    pairs = [(a, b) for i, a in enumerate(cols) for b in cols[i + 1:]] + [(V - 4, V - 3)]   # last vector | tail
    plant = [(c,) for c in cols] + pairs
    logits = _randn(_gen(7), len(plant), V, scale=3.0, dtype=dtype)
    for r, cs in enumerate(plant):
        for c in cs:
            logits[r, c] = 100.0
    want = torch.tensor([min(cs) for cs in plant])
    assert torch.equal(torch.argmax(logits.float(), 1), want)
    return logits, want


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
@pytest.mark.parametrize("dtype,V", SAMPLE_PATH_SHAPES[:2], ids=lambda p: str(p).replace("torch.", ""))
def test_sample_greedy_planted_maxima_and_ties(dtype, V, layout, dev):
    """Greedy rows with the maximum planted in each region, and equal maxima in two regions:
    exactly argmax, the smaller index on a tie (argmax_merge is a total order)."""
    logits, want = _sample_planted_case(dtype, V)
    n = logits.shape[0]
    tok, val = _run_sample(_sample_layout(logits, layout, dev), torch.zeros(n), torch.arange(n), torch.arange(n), dev)
    assert torch.equal(tok, want)
    assert torch.equal(val, torch.full((n,), 100.0))   # greedy: the raw logit


@pytest.mark.parametrize("dev", DEVS)
def test_sample_masked_logits(dev):
    """All but three columns at -inf and T > 0: the token is one of the three over 256 seeds
    (one of them in the scalar tail); an all -inf row returns col_offset + 0."""
    V, R, keep = 1003, 256, [0, 500, 1002]
    row = torch.full((V,), float("-inf"))
    row[keep] = torch.tensor([0.5, -1.0, 1.0])
    for dtype in (BF16, F32):
        logits = row.to(dtype).expand(R, V).contiguous()
        temp = torch.tensor([0.3, 1.0, 2.0, 0.7]).repeat(R // 4)
        tok, val = _run_sample(logits.to(dev), temp, torch.arange(R) * 2654435761 % (1 << 40), torch.full((R,), 17), dev)
        assert set(tok.tolist()) <= set(keep), sorted(set(tok.tolist()))
        assert len(set(tok.tolist())) == 3   # and all three occur in 256 draws
        assert torch.isfinite(val).all()
        dead = torch.full((4, V), float("-inf"), dtype=dtype)
        tok, val = _run_sample(dead.to(dev), torch.tensor([0.0, 1.0, 0.0, 0.3]), torch.arange(4), torch.arange(4), dev,
                               col_offset=77)
        assert tok.tolist() == [77] * 4 and (val == float("-inf")).all()


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("dtype,V", SAMPLE_PATH_SHAPES[:2], ids=lambda p: str(p).replace("torch.", ""))
def test_sample_shard_decomposition(dtype, V, dev):
    """The vocab-sharded form of models/llama.py: shards cut at unaligned columns, each called
    with its col_offset and an out_val; per row the shard with the largest value (ties: lower
    token) gives exactly the unsharded token and its value bit for bit, greedy rows (value =
    raw logit) included: a column's value depends on the logit and the global column only."""
    case = _sample_case(dtype, V)
    logits, temp, seeds, pos = case[:4]
    x = _sample_layout(logits, "aligned", dev)
    tok, val = _run_sample(x, temp, seeds, pos, dev)
    _check_sample_matches_ref(case, tok, val)
    cuts = [0, 5, 13000, 13001, V]
    best_tok = best_val = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        t, v = _run_sample(x[:, a:b], temp, seeds, pos, dev, col_offset=a)
        assert ((t >= a) & (t < b)).all()
        tr, vr = ref.sample_shard(logits[:, a:b], temp, seeds, pos, a)
        torch.testing.assert_close(v, vr, atol=1e-3, rtol=0)
        if best_tok is None:
            best_tok, best_val = t.clone(), v.clone()
        else:
            take = (v > best_val) | ((v == best_val) & (t < best_tok))
            best_tok, best_val = torch.where(take, t, best_tok), torch.where(take, v, best_val)
    assert torch.equal(best_tok, tok)
    assert _same_bits(best_val, val)


# ---------------------------------------------------------------------------------------------
# rmsnorm
# ---------------------------------------------------------------------------------------------

RMS_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _rms_case(rows, hidden, fused, std=1.0):
    g = _gen(2000 + hidden + rows)
    x = _randn(g, rows, hidden, scale=std)
    w = (torch.randn(hidden, generator=g) * 0.5 + 1).to(BF16)
    r = _randn(g, rows, hidden, scale=std) if fused else None
    y_ref, r_ref = ref.rmsnorm(x, w, RMS_EPS, r)
    return x, w, r, y_ref, r_ref


def _run_rmsnorm(x, w, r, dev):
    y = torch.full(x.shape, float("nan"), dtype=BF16, device=dev)
    rd = r.clone().to(dev) if r is not None else None
    got = ops.rmsnorm(x.to(dev) if torch.is_tensor(x) else x, w.to(dev), RMS_EPS, residual=rd, out=y)
    assert got.data_ptr() == y.data_ptr()
    return y.cpu(), (rd.cpu() if r is not None else None)


def _check_rmsnorm(y, r_new, y_ref, r_ref):
    assert torch.isfinite(y.float()).all()
    torch.testing.assert_close(y.float(), y_ref.float(), **TOL)
    if r_ref is not None:
        assert _same_bits(r_new, r_ref)   # a bf16 add: exact


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("hidden", [8, 72, 2056, 4096, 4104, 8192, 8200, 16384])
def test_rmsnorm_widths(hidden, rows, fused, dev):
    """8 / 72: rows shorter than a wave / a block; 2056, 4104, 8200: the last vector round of
    the 2-, 4- and 8-vector instantiations filled by a few threads only; 8200 / 16384: the
    8-vectors-per-thread instantiation up to its limit."""
    x, w, r, y_ref, r_ref = _rms_case(rows, hidden, fused)
    y, r_new = _run_rmsnorm(x, w, r, dev)
    _check_rmsnorm(y, r_new, y_ref, r_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [16392, 12])
def test_rmsnorm_binding_rejects_width(hidden):
    """Wider than 16384 or not a multiple of 8: raised before anything is launched."""
    x, w, r = torch.ones(3, hidden, dtype=BF16), torch.ones(hidden, dtype=BF16), torch.ones(3, hidden, dtype=BF16)
    y = torch.full((3, hidden), float("nan"), dtype=BF16, device="cuda")
    rd = r.cuda()
    with pytest.raises(RuntimeError, match="hidden must be|16-B aligned rows"):   # 12: the row-stride check fires first
        ops.rmsnorm(x.cuda(), w.cuda(), RMS_EPS, residual=rd, out=y)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.equal(rd.cpu(), r)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("hidden", [72, 4104])
def test_rmsnorm_strides(hidden, dev):
    """x, residual and y as column slices of wider canary-filled buffers with three different
    row strides: bit-equal to the contiguous call, canary columns untouched."""
    x, w, r, y_ref, r_ref = _rms_case(5, hidden, True)
    y0, r0 = _run_rmsnorm(x, w, r, dev)
    xv, xbuf, _ = _strided(x, dev, 8, 16)
    rv, rbuf, rin = _strided(r, dev, 16, 24)
    yv, ybuf, yin = _strided(torch.full_like(x, float("nan")), dev, 24, 32)
    assert len({xv.stride(0), rv.stride(0), yv.stride(0), hidden}) == 4
    xbuf0 = xbuf.clone()
    ops.rmsnorm(xv, w.to(dev), RMS_EPS, residual=rv, out=yv)
    assert _same_bits(yv, y0) and _same_bits(rv, r0)
    _check_rmsnorm(yv.cpu(), rv.cpu(), y_ref, r_ref)
    assert _same_bits(xbuf, xbuf0)
    assert (rbuf.cpu()[:, ~rin] == CANARY).all() and (ybuf.cpu()[:, ~yin] == CANARY).all()


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("hidden", [72, 4096])
def test_rmsnorm_eps(hidden, fused, dev):
    """Rows at standard deviation 3e-3 (fused: the sum's), so the mean square is about eps = 1e-5:
    a norm that dropped eps would be off by about 1.4x, far outside the tolerance."""
    std = 3e-3 / math.sqrt(2) if fused else 3e-3
    x, w, r, y_ref, r_ref = _rms_case(5, hidden, fused, std)
    xs = (x.float() + r.float()) if fused else x.float()
    ms = xs.pow(2).mean(-1)
    assert ((ms > 0.3 * RMS_EPS) & (ms < 3 * RMS_EPS)).all()
    no_eps = (xs * torch.rsqrt(ms)[:, None]).to(BF16).float() * w.float()
    assert ((no_eps - y_ref.float()).abs() > 0.1).float().mean() > 0.5   # the case can tell the two apart
    y, r_new = _run_rmsnorm(x, w, r, dev)
    _check_rmsnorm(y, r_new, y_ref, r_ref)


def _slab_sum(P):
    """The bf16 row a split-K consumer sees: slabs added in slab order in fp32, rounded once."""
    a = P[0].clone()
    for k in range(1, P.shape[0]):
        a += P[k]
    return a.to(BF16)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("N", [2048, 2056, 4096, 4104])
@pytest.mark.parametrize("S", [2, 3, 4, 8])
def test_rmsnorm_slabs(S, N, fused, dev):
    """Split-K slabs summed inside rmsnorm. The 512-thread instantiation takes nvec in
    (256, 512]: 2048 is the last width below it, 2056 and 4096 its two ends, 4104 the first
    above; S = 2, 4, 8 are compiled slab counts, 3 the runtime loop. The updated residual is
    the same arithmetic on every path and must be bit-equal. y is compared at the project
    tolerance only: the 512-thread path reduces the sum of squares in another order than the
    256-thread one, so y is not promised bitwise."""
    g = _gen(3000 + S + N)
    M = 5
    P = torch.randn(S, M, N, generator=g)
    w = (torch.randn(N, generator=g) * 0.5 + 1).to(BF16)
    r = _randn(g, M, N) if fused else None
    xb = _slab_sum(P)
    y_ref, r_ref = ref.rmsnorm(xb, w, RMS_EPS, r)
    x = ops.SplitK(P.reshape(-1).to(dev), S, M, N) if dev == "cuda" else xb
    y, r_new = _run_rmsnorm(x, w, r, dev)
    _check_rmsnorm(y, r_new, y_ref, r_ref)


# ---------------------------------------------------------------------------------------------
# silu_mul
# ---------------------------------------------------------------------------------------------

def _run_silu_mul(gu, block, dev):
    out = torch.full((gu.shape[0], gu.shape[1] // 2), float("nan"), dtype=BF16, device=dev)
    got = ops.silu_mul(gu.to(dev), out=out, block=block)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu()


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("rows,inter,block", [(2056, 4104, None), (3, 8, None), (3, 8, 8), (5, 192, None), (5, 192, 8),
                                              (5, 192, 64), (5, 192, 192)])
def test_silu_mul_shapes_and_blocks(rows, inter, block, dev):
    """2056 x 4104: 1,054,728 vectors, more than the 1,048,576 the capped grid covers in one
    trip of its grid-stride loop; inter 8: one vector per row; every interleave block."""
    gu = _randn(_gen(4000 + inter), rows, 2 * inter, scale=2.0)
    out = _run_silu_mul(gu, block, dev)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.float(), ref.silu_mul(gu, block).float(), **TOL)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("block", [None, 64])
def test_silu_mul_strides(block, dev):
    """Input and output as column slices of wider canary-filled buffers: bit-equal to the
    contiguous call, canary columns untouched."""
    rows, inter = 5, 192
    gu = _randn(_gen(4100), rows, 2 * inter, scale=2.0)
    out0 = _run_silu_mul(gu, block, dev)
    gv, gbuf, _ = _strided(gu, dev, 8, 16)
    ov, obuf, oin = _strided(torch.full((rows, inter), float("nan"), dtype=BF16), dev, 16, 24)
    gbuf0 = gbuf.clone()
    ops.silu_mul(gv, out=ov, block=block)
    assert _same_bits(ov, out0)
    assert _same_bits(gbuf, gbuf0) and (obuf.cpu()[:, ~oin] == CANARY).all()


def _silu_edge_case():
    gates = [0.0, 1e-30, 20.0, 88.0, 89.0, 100.0, 1e4]
    g = torch.tensor([s * v for v in gates for s in (1.0, -1.0)] + [1.0, -1.0]).to(BF16)   # 16 gates
    u = torch.tensor([1.5, -2.0]).to(BF16)
    gate = g.repeat(2)
    up = u.repeat_interleave(16)
    gu = torch.cat([gate, up])[None, :].contiguous()           # [1, 2 * 32], plain [gate | up]
    gd, ud = gate.double(), up.double()
    s = (gd / (1 + torch.exp(-gd))).to(BF16)                    # fp64 SiLU, the kernel's two bf16 roundings
    want = (s.double() * ud).to(BF16)
    return gu, gate, up, want[None, :]


@pytest.mark.parametrize("dev", DEVS)
def test_silu_mul_gate_extremes(dev):
    """Gates where exp(-g) overflows (g <= -89), underflows (g >= 89) or is exactly 1 (+-0):
    every output finite, large negative gates give a signed zero (never -g / inf = NaN), large
    positive gates give gate * up exactly."""
    gu, gate, up, want = _silu_edge_case()
    out = _run_silu_mul(gu, None, dev)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.float(), want.float(), **TOL)
    o, g, u = out[0].float(), gate.float(), up.float()
    big = g >= 20
    assert _same_bits(out[0][big], (g[big] * u[big]).to(BF16))
    neg = g <= -100
    assert neg.sum() == 4 and (o[neg] == 0).all()
    assert torch.equal(torch.signbit(o[neg]), torch.signbit(-u[neg]))
    zero = g == 0
    assert (o[zero] == 0).all() and torch.equal(torch.signbit(o[zero]), torch.signbit(g[zero] * u[zero]))


# ---------------------------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------------------------

EMB_VOCAB = 50


def _run_embedding(ids, table, dev):
    out = torch.full((ids.numel(), table.shape[1]), float("nan"), dtype=BF16, device=dev)
    ops.embedding(ids.to(dev), table.to(dev), out=out)
    return out.cpu()


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("hidden", [8, 2056, 4096])
def test_embedding_widths_and_edge_ids(hidden, dev):
    """hidden 8: one lane copies; 2056: 257 vectors, the per-thread loop's second trip taken by
    one thread; 4096: by all. In-range ids (0 and vocab - 1 among them) equal
    reference.embedding; out-of-range ids (-1, vocab, 2^40) read row 0 in the kernel, as it
    documents (the reference clamps to the nearest row instead, so that part is asserted of
    the kernel alone)."""
    table = _randn(_gen(5000 + hidden), EMB_VOCAB, hidden)
    ids = torch.tensor([0, EMB_VOCAB - 1, 7, -1, EMB_VOCAB, 1 << 40, 3, 3, 0])
    ok = (ids >= 0) & (ids < EMB_VOCAB)
    out = _run_embedding(ids, table, dev)
    assert _same_bits(out[ok], ref.embedding(ids[ok], table))
    if dev == "cuda":
        assert _same_bits(out[~ok], table[:1].expand(int((~ok).sum()), hidden))
    else:
        assert torch.isfinite(out[~ok].float()).all()
    empty = _run_embedding(torch.empty(0, dtype=torch.long), table, dev)   # zero tokens: no launch
    assert empty.shape == (0, hidden)


# ---------------------------------------------------------------------------------------------
# quantize_fp8, silu_quantize_fp8, the fused decode output quantisation
# ---------------------------------------------------------------------------------------------

BF16_MAX = torch.finfo(BF16).max


def _check_fp8_rows(x, q, sx, zero_rows_exact=True):
    """Invariants of a per-row e4m3fn quantisation of ``x`` (the values the kernel quantised):
    no NaN byte, a finite positive scale equal to amax / 448 (1 for an all-zero row), a non-zero
    row's largest byte at +-448, zero bytes for an all-zero row, and |q * s - x| within one e4m3
    step of q, times s, in fp64 (the step formula of test_quantize_fp8_matches_torch)."""
    x, q, sx = x.cpu().float(), q.cpu(), sx.cpu()
    by = q.view(torch.uint8)
    mag = by & 0x7F
    assert (mag != 0x7F).all(), f"{int((mag == 0x7F).sum())} NaN bytes; row maxima {mag.amax(1).tolist()}"
    assert (torch.isfinite(sx) & (sx > 0)).all(), sx
    amax = x.abs().amax(1)
    want_s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    torch.testing.assert_close(sx, want_s, rtol=1.3e-6, atol=0)   # atol = 0: the scales go down to 1e-43
    nz = amax > 0
    assert (mag[nz].amax(1) == 0x7E).all(), mag.amax(1).tolist()
    assert (sx[~nz] == 1).all()
    assert ((by[~nz] if zero_rows_exact else mag[~nz]) == 0).all()
    qd, sd = q.double(), sx.double()[:, None]
    step = torch.clamp(qd.abs(), min=2.0 ** -6) * 2.0 ** -3
    err = (qd * sd - x.double()).abs()
    assert (err <= step * sd).all(), f"worst error / step: {float((err / (step * sd)).max()):.3g}"


@functools.lru_cache(maxsize=None)
def _quant_case(K, scale):
    """Rows at ``scale`` with a few exact zeros, one row with a single non-zero element, an
    all-zero row and (for contrast) one ordinary row."""
    g = _gen(6000 + K)
    x = torch.randn(6, K, generator=g) * scale
    x = x.clamp(-BF16_MAX, BF16_MAX)
    x[:, ::97] = 0
    x[3] = 0
    x[3, K // 2 + 1] = -scale
    x[4] = 0
    x[5] = torch.randn(K, generator=g) * 3
    return x.to(BF16)


QUANT_SCALES = [1e-37, 2.0 ** -126, 7.5e37]


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("scale", QUANT_SCALES, ids=["1e-37", "2^-126", "7.5e37"])
@pytest.mark.parametrize("K", [1024, 8192, 20480])   # register paths (2 / 4 vectors) and the streaming kernel
def test_quantize_fp8_extreme_rows(K, scale, dev):
    """Rows whose scale amax / 448 is subnormal (1 / s overflows below amax ~ 1.3e-36) and rows
    near the bf16 maximum."""
    x = _quant_case(K, scale)
    if scale < 1e-30:
        assert (x[:4].float().abs().amax(1) < 1.3e-36).all()
    q, sx = ops.quantize_fp8(x.to(dev))
    _check_fp8_rows(x, q, sx)


def _silu_quant_case(inter):
    """64-interleaved gate|up rows whose SwiGLU output is all zero (silu underflows; gate and up
    both zero), all tiny (~1e-37) or ordinary."""
    g = _gen(6100 + inter)
    gate = torch.randn(5, inter, generator=g) * 2
    up = torch.randn(5, inter, generator=g) * 2
    gate[0] = -1e4                 # silu = -0: an all-zero row of signed zeros
    gate[1], up[1] = gate[1] * 1e-18, up[1] * 1e-20
    gate[2], up[2] = 0.0, 0.0
    gate[3] = gate[3].abs() * 1e-18 + 1e-19
    up[3] = 1e-20                  # every element tiny and non-zero... or rounded to zero
    gu = torch.stack([gate.reshape(5, inter // 64, 64), up.reshape(5, inter // 64, 64)], 2).reshape(5, 2 * inter)
    return gu.to(BF16)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("inter", [1024, 8192])
def test_silu_quantize_fp8_zero_and_tiny_rows(inter, dev):
    gu = _silu_quant_case(inter).to(dev)
    x = ops.silu_mul(gu, block=64)          # the values the fused kernel quantises
    amax = x.float().abs().amax(1).cpu()
    assert amax[0] == 0 and amax[2] == 0 and 0 < amax[1] < 1.3e-36 and amax[4] > 1
    q, sx = ops.silu_quantize_fp8(gu, block=64)
    _check_fp8_rows(x, q, sx, zero_rows_exact=False)   # row 0 holds -0: byte 0x80
    if dev == "cuda":   # the fused kernel against the two kernels it replaces
        q0, s0 = ops.quantize_fp8(x)
        assert torch.equal(sx, s0)
        assert (q.view(torch.uint8) == q0.view(torch.uint8)).float().mean() > 0.99


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("splits", [1, 4])
def test_attn_decode_fused_quant_tiny_rows(splits, dev):
    """The decode split-combine's fused output quantisation on rows whose attention output is
    ~1e-37 (a V cache of tiny values): the same invariants, and the bytes and scales of
    quantize_fp8 over the bf16 output."""
    g = _gen(6200)
    B, Hq, Hkv, D, page = 3, 8, 1, 128, 16
    lens = torch.tensor([1, 17, 300], dtype=torch.int32)
    pages = (int(lens.max()) + page - 1) // page
    kc = _randn(g, B * pages, Hkv, page, D)
    vc = _randn(g, B * pages, Hkv, page, D, scale=1e-37)
    vc[pages:2 * pages] = 0                      # sequence 1: an all-zero output row
    bt = torch.arange(B * pages, dtype=torch.int32).view(B, pages)
    q = _randn(g, B, Hq, D)
    args = (q.to(dev), kc.to(dev), vc.to(dev), bt.to(dev), lens.to(dev), D ** -0.5, splits)
    o = ops.attn_decode(*args).reshape(B, Hq * D)
    amax = o.float().abs().amax(1).cpu()
    assert 0 < amax[0] < 1.3e-36 and amax[1] == 0, amax    # one key: the row is that token's V
    q8, sx = ops.attn_decode(*args, quant=True)
    _check_fp8_rows(o, q8, sx, zero_rows_exact=False)
    q0, s0 = ops.quantize_fp8(o)
    assert torch.equal(sx, s0) and _same_bits(q8, q0)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1024, 20480])
def test_quantize_fp8_binding_row_stride(K):
    """The binding on a 16-B aligned column slice of a wider buffer equals the contiguous call;
    a row stride that is not a multiple of 8 elements or a base off a 16-B boundary is rejected
    before a launch (the kernels issue 16-B loads)."""
    C = ops.kernels()
    x = _quant_case(K, 1e-37).clone()
    x[:3] = _randn(_gen(1), 3, K, scale=3.0)
    q0, s0 = ops.quantize_fp8(x.cuda())
    xv, _, _ = _strided(x, "cuda", 8, 16)
    q = torch.full((6, K), 0x55, dtype=torch.uint8, device="cuda").view(E4M3)
    sx = torch.full((6,), float("nan"), device="cuda")
    C.quantize_fp8(xv, q, sx)
    assert _same_bits(q, q0) and torch.equal(sx, s0)
    _check_fp8_rows(x, q, sx)
    odd_stride, _, _ = _strided(x, "cuda", 0, 4)      # row stride K + 4
    off_base, _, _ = _strided(x, "cuda", 4, 20)       # stride K + 24, base 8 bytes in
    for bad in (odd_stride, off_base):
        q = torch.full((6, K), 0x55, dtype=torch.uint8, device="cuda")
        sx = torch.full((6,), float("nan"), device="cuda")
        with pytest.raises(RuntimeError, match="16-B aligned"):
            C.quantize_fp8(bad, q, sx)
        torch.cuda.synchronize()
        assert (q == 0x55).all() and torch.isnan(sx).all()


@pytest.mark.gpu
def test_silu_quantize_fp8_binding_row_stride():
    """The same for the fused SwiGLU form, which reads gate|up rows 16 B per lane."""
    C = ops.kernels()
    gu = _silu_quant_case(1024)
    q0, s0 = ops.silu_quantize_fp8(gu.cuda(), block=64)
    gv, _, _ = _strided(gu, "cuda", 8, 16)
    q, sx = ops.silu_quantize_fp8(gv, block=64)
    assert _same_bits(q, q0) and torch.equal(sx, s0)
    odd_stride, _, _ = _strided(gu, "cuda", 0, 4)
    off_base, _, _ = _strided(gu, "cuda", 4, 20)
    for bad in (odd_stride, off_base):
        q = torch.full((5, 1024), 0x55, dtype=torch.uint8, device="cuda")
        sx = torch.full((5,), float("nan"), device="cuda")
        with pytest.raises(RuntimeError, match="16-B aligned"):
            C.silu_quantize_fp8(bad, q, sx)
        torch.cuda.synchronize()
        assert (q == 0x55).all() and torch.isnan(sx).all()


# ---------------------------------------------------------------------------------------------
# rope_kv and the fused decode form
# ---------------------------------------------------------------------------------------------

ROPE_D, ROPE_MAXPOS = 128, 64
KV_CANARY = 0x3A       # a finite e4m3 byte


@functools.lru_cache(maxsize=None)
def _rope_tables():
    return ref.rope_tables(ROPE_MAXPOS, ROPE_D, 500000.0)


def _rope_decode_case(lens, Hq, Hkv, P=16, seed=0):
    """A decode step: one new token per sequence at position len - 1, its slot the last token
    of the sequence's pages."""
    g = _gen(7000 + seed + len(lens))
    B = len(lens)
    maxp = (max(lens) + P - 1) // P + 1
    pages = B * maxp + 2
    bt = torch.randperm(pages, generator=g)[: B * maxp].reshape(B, maxp).int()
    pos = torch.tensor([n - 1 for n in lens])
    slots = torch.tensor([int(bt[b, (n - 1) // P]) * P + (n - 1) % P for b, n in enumerate(lens)])
    qkv = _randn(g, B, (Hq + 2 * Hkv) * ROPE_D)
    return dict(qkv=qkv, pos=pos, slots=slots, bt=bt, sl=torch.tensor(lens, dtype=torch.int32), Hq=Hq, Hkv=Hkv, P=P,
                pages=pages)


def _fresh_caches(c, dtype, dev):
    shape = (c["pages"], c["Hkv"], c["P"], ROPE_D)
    if dtype == E4M3:
        k = torch.full(shape, KV_CANARY, dtype=torch.uint8).view(E4M3)
    else:
        k = torch.full(shape, CANARY, dtype=BF16)
    return k.to(dev), k.clone().to(dev)


def _run_rope_kv(c, dev, cache_dtype, k_scale=1.0, v_scale=1.0, qkv=None, pos=None, slots=None):
    cos, sin = _rope_tables()
    kc, vc = _fresh_caches(c, cache_dtype, dev)
    q, k, v = ops.rope_kv((c["qkv"] if qkv is None else qkv).to(dev), (c["pos"] if pos is None else pos).to(dev),
                          cos.to(dev), sin.to(dev), c["Hq"], c["Hkv"], kc, vc,
                          (c["slots"] if slots is None else slots).to(dev), k_scale=k_scale, v_scale=v_scale)
    return q.cpu(), k.cpu(), v.cpu(), kc.cpu(), vc.cpu()


def _check_fp8_caches(c, kc8, vc8, kcb, v, k_scale, v_scale):
    """V bytes == kv_store(v); K bytes == kv_store of what the bf16-cache run stored (exact for
    a power-of-two scale); every other byte still the canary; no NaN byte."""
    P = c["P"]
    k8 = ref.k_cache_logical(kc8.view(torch.uint8))
    kb = ref.k_cache_logical(kcb)
    v8 = vc8.view(torch.uint8)
    want_k = torch.full_like(k8, KV_CANARY)
    want_v = torch.full_like(v8, KV_CANARY)
    for t, s in enumerate(c["slots"].tolist()):
        want_k[s // P, :, s % P] = ref.kv_store(kb[s // P, :, s % P].float(), E4M3, k_scale).view(torch.uint8)
        want_v[s // P, :, s % P] = ref.kv_store(v[t], E4M3, v_scale).view(torch.uint8)
    assert torch.equal(k8, want_k)
    assert torch.equal(v8, want_v)
    assert ((k8 & 0x7F) != 0x7F).all() and ((v8 & 0x7F) != 0x7F).all()
    return want_k, want_v


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("lens", [[1], [1, 17, 33, 48, 20]], ids=["T1", "T5"])
def test_rope_kv_fp8_store_saturates(lens, dev):
    """Scales 2^-10: most of x / scale lies beyond +-448 and must store as +-448 (0x7E / 0xFE),
    never NaN; the fused decode form (ops.attn_decode_rope) writes the same bytes."""
    c = _rope_decode_case(lens, Hq=8, Hkv=2)
    scale = 2.0 ** -10
    q8, k8, v8, kc8, vc8 = _run_rope_kv(c, dev, E4M3, scale, scale)
    qb, kb, vb, kcb, vcb = _run_rope_kv(c, dev, BF16)
    assert _same_bits(q8, qb) and _same_bits(k8, kb) and _same_bits(v8, vb)
    want_k, _ = _check_fp8_caches(c, kc8, vc8, kcb, c["qkv"][:, (8 + 2) * ROPE_D:].reshape(-1, 2, ROPE_D), scale, scale)
    written = want_k != KV_CANARY
    assert ((want_k[written] & 0x7F) == 0x7E).float().mean() > 0.5    # the case does saturate
    cos, sin = _rope_tables()
    kcf, vcf = _fresh_caches(c, E4M3, dev)
    ops.attn_decode_rope(c["qkv"].to(dev), c["pos"].to(dev), cos.to(dev), sin.to(dev), 8, kcf, vcf, c["slots"].to(dev),
                         c["bt"].to(dev), c["sl"].to(dev), ROPE_D ** -0.5, 1, k_scale=scale, v_scale=scale)
    assert _same_bits(kcf, kc8) and _same_bits(vcf, vc8)


@pytest.mark.parametrize("dev", DEVS)
def test_rope_kv_position_clamp(dev):
    """Positions 0, max_pos - 1, max_pos and max_pos + 1000 rotate as positions clamped to
    max_pos - 1 (the kernel clamps; the reference is given the clamped positions)."""
    c = _rope_decode_case([3, 9, 20, 31], Hq=8, Hkv=2)
    raw = torch.tensor([0, ROPE_MAXPOS - 1, ROPE_MAXPOS, ROPE_MAXPOS + 1000])
    clamped = raw.clamp(max=ROPE_MAXPOS - 1)
    cos, sin = _rope_tables()
    q_r, k_r, v_r = ref.rope_kv(c["qkv"], clamped, cos, sin, 8, 2)
    want = _run_rope_kv(c, dev, BF16, pos=clamped)
    torch.testing.assert_close(want[0].float(), q_r.float(), **TOL)
    torch.testing.assert_close(want[1].float(), k_r.float(), **TOL)
    assert _same_bits(want[2], v_r)
    if dev == "cuda":
        got = _run_rope_kv(c, dev, BF16, pos=raw)
        assert all(_same_bits(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("cache_dtype", [BF16, E4M3], ids=["bf16", "fp8"])
def test_rope_kv_strided_qkv_and_dead_slots(cache_dtype, dev):
    """qkv as a column slice of a wider buffer (row stride a multiple of 8): bit-equal to the
    contiguous call. All slots -1: both caches stay byte-identical."""
    c = _rope_decode_case([1, 17, 33, 48, 20], Hq=8, Hkv=2)
    want = _run_rope_kv(c, dev, cache_dtype, 0.5, 2.0)
    qv, qbuf, _ = _strided(c["qkv"], "cpu", 8, 16)
    assert qv.stride(0) % 8 == 0 and qv.stride(0) != c["qkv"].shape[1]
    got = _run_rope_kv(c, dev, cache_dtype, 0.5, 2.0, qkv=qbuf.to(dev)[:, 8:8 + qv.shape[1]])
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    dead = _run_rope_kv(c, dev, cache_dtype, 0.5, 2.0, slots=torch.full((5,), -1))
    kc0, vc0 = _fresh_caches(c, cache_dtype, "cpu")
    assert _same_bits(dead[3], kc0) and _same_bits(dead[4], vc0)
    assert all(_same_bits(a, b) for a, b in zip(dead[:3], want[:3]))
