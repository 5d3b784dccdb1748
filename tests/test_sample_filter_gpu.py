"""Top-k / top-p on the GPU: the sample_threshold kernel and the filtered sampler
(csrc/kernels/sample.hip) against the fp64 reference (ops/reference.py sample_threshold), on
every path of the row walk (16-B vector body, remainder rounds, scalar tail, unaligned
fallback; strided rows with a canary outside them), and the engine's captured prefill and
decode graphs with filtered and default requests in one batch.

Top-k selects by count, so thr and kept must equal the reference exactly. Top-p compares
masses the kernel sums in 2^40 fixed point from fp32 exponents, so on random rows its threshold
must be sufficient and minimal within EPS of the fp64 masses, and on planted rows whose
cumulative edges lie >= 1e-3 from top_p it must be exact.
"""
import functools
import math

import pytest
import torch

from operator_amd import ops
from operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NEG_INF = float("-inf")
# 1e-4 of the total mass: about ten times the worst-case error of the kernel's own arithmetic
# (fp32 rounding of (x - max) / T at magnitudes up to ~100: <= 8e-6 relative per term; the 2^-40
# fixed point: < 1e-7)
EPS = 1e-4
LAYOUTS = ["contig", "aligned", "unaligned"]
SHAPES = [(BF16, 1), (BF16, 7), (BF16, 8), (BF16, 1003), (BF16, 41003), (F32, 1), (F32, 7), (F32, 1003), (F32, 20503)]
ROWS = 14


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _layout(logits, layout, dev="cuda"):
    """aligned: a [:, :V] slice of rows whose stride is a multiple of 8 (vector body + scalar
    tail); unaligned: a [:, 1:V+1] slice of the same (every row off a 16-B boundary: all
    scalar); contig: [rows, V] as is. Outside the rows the buffer holds 1e4, which would be
    the maximum, the k-th value and nearly all the mass of any row that read it."""
    rows, V = logits.shape
    if layout == "contig":
        return logits.to(dev)
    stride = (V + 1 + 7) // 8 * 8 + 8
    buf = torch.full((rows, stride), 1e4, dtype=logits.dtype)
    c0 = 0 if layout == "aligned" else 1
    buf[:, c0:c0 + V] = logits
    view = buf.to(dev)[:, c0:c0 + V]
    assert (view.data_ptr() % 16 == 0) == (layout == "aligned")
    return view


def _params(V):
    """Greedy (row 0, its filters ignored), default (1), top-k only (2-7), top-p only (8-10),
    both (11-13)."""
    temp = torch.tensor([0.0, 1.0, 0.3, 1.5, 1.0, 0.3, 1.5, 0.7, 1.0, 0.3, 1.5, 1.0, 0.3, 1.5])
    top_k = torch.tensor([5, 0, 1, 2, 40, V - 1, V, V + 5, 0, 0, 0, 40, 2, 40], dtype=torch.int32)
    top_p = torch.tensor([0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1e-6, 0.5, 0.9, 0.97, 0.9, 0.5])
    return temp, top_k, top_p


@functools.lru_cache(maxsize=None)
def _case(dtype, V, rows=ROWS):
    """Random rows at scale 3 with -inf, +0 and -0 planted, and three more copies of the k-th
    largest value in every row with top_k in (1, V); the fp64 reference's thresholds, counts
    and tokens."""
    g = _gen(500 + V)
    logits = (torch.randn(rows, V, generator=g) * 3).to(dtype)
    temp, top_k, top_p = (t[:rows] for t in _params(V))
    for r in range(rows):
        if V < 8:
            continue
        c = torch.randperm(V, generator=g)[:6].tolist()
        logits[r, c[0]], logits[r, c[1]], logits[r, c[2]] = NEG_INF, 0.0, -0.0
        k = int(top_k[r])
        if 1 < k < V:
            kth = torch.sort(logits[r].float(), descending=True).values[k - 1]
            lower = [x for x in c[3:] if float(logits[r, x]) < float(kth)]
            logits[r, lower] = kth.to(dtype)
    seeds = torch.arange(rows) * 7 + 1
    pos = torch.arange(rows) + 100
    thr, kept = ref.sample_threshold(logits, temp, top_k, top_p)
    tok, val = ref.sample_shard(logits, temp, seeds, pos, thr=thr)
    return dict(logits=logits, temp=temp, top_k=top_k, top_p=top_p, seeds=seeds, pos=pos, thr=thr, kept=kept,
                tok=tok, val=val)


def _run_threshold(x, c):
    n = x.shape[0]
    thr = torch.full((n,), float("nan"), device="cuda")
    kept = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    got = ops.sample_threshold(x, c["temp"].cuda(), c["top_k"].cuda(), c["top_p"].cuda(), out=thr, out_kept=kept)
    assert got.data_ptr() == thr.data_ptr()
    return thr.cpu(), kept.cpu()


def _run_sample(x, c, **kw):
    n = x.shape[0]
    out = torch.full((n,), -7, dtype=torch.long, device="cuda")
    val = torch.full((n,), float("nan"), device="cuda")
    ops.sample(x, c["temp"].cuda(), c["seeds"].cuda(), c["pos"].cuda(), out=out, out_val=val,
               **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
    return out.cpu(), val.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _masses(row, t, k):
    """The row's kept values after top-k, descending, and their fp64 masses."""
    x = row.double()
    s = torch.sort(x[~torch.isnan(x)], descending=True).values + 0.0
    if 0 < k < row.numel():
        s = s[s >= s[min(k, s.numel()) - 1]]
    w = torch.exp((s - s[0]) / t)
    w[s == s[0]] = 1.0
    return s, w


def _check_threshold(c, thr, kept):
    logits, temp, top_k, top_p = c["logits"], c["temp"], c["top_k"], c["top_p"]
    for r in range(logits.shape[0]):
        t, k, p = float(temp[r]), int(top_k[r]), float(top_p[r])
        got = float(thr[r])
        print(f"row {r}: T={t} top_k={k} top_p={p}: thr {got!r} (ref {float(c['thr'][r])!r}) "
              f"kept {int(kept[r])} (ref {int(c['kept'][r])})")
        x = logits[r].double()
        if not (t > 0 and p < 1):
            # unfiltered or top-k only: selection by count, no tolerance
            assert _bits(thr[r:r + 1]).item() == _bits(c["thr"][r:r + 1]).item(), r
            assert int(kept[r]) == int(c["kept"][r]), r
            continue
        s, w = _masses(logits[r], t, k)
        Z = float(w.sum())
        assert bool((s == got).any()), (r, got)                 # a value of the row, at or above tau_k
        assert int(kept[r]) == int((x >= got).sum()), r
        m = float(w[s >= got].sum())
        above = s[s > got]
        m_next = float(w[s >= above[-1]].sum()) if above.numel() else 0.0
        print(f"   m(thr)/Z = {m / Z:.9f}, m(next above)/Z = {m_next / Z:.9f}")
        assert m / Z >= p - EPS, (r, m / Z, p)                  # sufficient
        assert m_next / Z < p + EPS, (r, m_next / Z, p)         # minimal


def _check_tokens(c, x, thr, kept, tok, val):
    """The reference token (or, on an fp32-vs-fp64 near-tie, one whose perturbed value is within
    1e-3 of the reference's), always inside the kernel's own kept set; top_k = 1 rows give the
    argmax; thr = -inf rows the token and value bits of the unfiltered sampler."""
    logits, temp, seeds, pos = c["logits"], c["temp"], c["seeds"], c["pos"]
    V = logits.shape[1]
    assert ((tok >= 0) & (tok < V)).all(), tok
    plain_tok, plain_val = _run_sample(x, c)
    for r in range(logits.shape[0]):
        xr = logits[r].double()
        assert not float(xr[tok[r]]) < float(thr[r]), (r, int(tok[r]))
        if tok[r] != c["tok"][r]:
            y = xr
            if float(temp[r]) > 0:
                y = xr / float(temp[r]) + ref.gumbel_noise_ref(int(seeds[r]), int(pos[r]), V)
            assert abs(float(y[tok[r]] - y[c["tok"][r]])) < 1e-3, (r, int(tok[r]), int(c["tok"][r]))
        if int(c["top_k"][r]) == 1 and float(temp[r]) > 0 and V > 1:
            assert int(tok[r]) == int(torch.argmax(logits[r].float())), r
        if float(thr[r]) == NEG_INF:
            assert tok[r] == plain_tok[r] and _bits(val[r:r + 1]).item() == _bits(plain_val[r:r + 1]).item(), r
    torch.testing.assert_close(val, c["val"], atol=1e-3, rtol=0)


def _check_all(c, x):
    thr, kept = _run_threshold(x, c)
    _check_threshold(c, thr, kept)
    buf = torch.full((x.shape[0],), float("nan"), device="cuda")
    tok, val = _run_sample(x, c, top_k=c["top_k"], top_p=c["top_p"], thr=buf)
    assert torch.equal(_bits(buf.cpu()), _bits(thr))            # ops.sample filled the caller's buffer
    _check_tokens(c, x, thr, kept, tok, val)
    own_tok, own_val = _run_sample(x, c, thr=buf)               # the caller's own thresholds
    assert torch.equal(own_tok, tok) and torch.equal(_bits(own_val), _bits(val))
    thr2, kept2 = _run_threshold(x, c)                           # a second call: the same bits
    tok2, val2 = _run_sample(x, c, top_k=c["top_k"], top_p=c["top_p"])
    assert torch.equal(_bits(thr2), _bits(thr)) and torch.equal(kept2, kept)
    assert torch.equal(tok2, tok) and torch.equal(_bits(val2), _bits(val))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype,V", SHAPES, ids=lambda p: str(p).replace("torch.", ""))
def test_threshold_and_filtered_sampler_paths(dtype, V, layout):
    """41003 bf16 / 20503 fp32: 5125 vectors + 3 scalars per aligned row (one four-way unrolled
    round, two remainder rounds, the scalar tail); 1 / 7 / 8 / 1003: no vector, one vector, no
    unrolled round. 14 rows mixing greedy, default, top-k only (1, 2, 40, V - 1, V, V + 5),
    top-p only (1e-6, 0.5, 0.9) and both, at T in {0.3, 0.7, 1, 1.5}."""
    c = _case(dtype, V)
    _check_all(c, _layout(c["logits"], layout))


def test_llama_vocab_rows():
    """4 rows x 128256 bf16: the row length of the flagship model."""
    V = 128256
    g = _gen(11)
    logits = (torch.randn(4, V, generator=g) * 3).to(BF16)
    c = dict(logits=logits, temp=torch.tensor([1.0, 0.3, 1.5, 0.7]),
             top_k=torch.tensor([40, 0, V - 1, 0], dtype=torch.int32), top_p=torch.tensor([0.9, 0.9, 1.0, 1.0]),
             seeds=torch.arange(4) + 3, pos=torch.arange(4) + 900)
    c["thr"], c["kept"] = ref.sample_threshold(logits, c["temp"], c["top_k"], c["top_p"])
    c["tok"], c["val"] = ref.sample_shard(logits, c["temp"], c["seeds"], c["pos"], thr=c["thr"])
    _check_all(c, logits.cuda())


PLANT_N = 40
PLANT_P = [(0.5, 4), (0.9, 11), (0.97, 16)]
# T ln(0.8) = -0.25, -0.5, -1: the planted logits -s i are exact in bf16, so the probabilities
# are 0.8^i in both dtypes
PLANT_STEPS = [0.25, 0.5, 1.0]


def _plant_columns(dtype, V, g):
    """40 columns: column 0, the scalar tail, the remainder rounds and the unrolled body of an
    aligned row, ordered so that the first ranks (the ones top_p = 0.5 keeps) take one of each."""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    nv = V // vec
    unrolled = nv // 4096 * 4096 * vec
    assert 0 < unrolled < nv * vec < V
    tail = list(range(V - 1, nv * vec - 1, -1))
    rem = (unrolled + torch.randperm(nv * vec - unrolled, generator=g)[:14]).tolist() + [unrolled, nv * vec - 1]
    body = (1 + torch.randperm(unrolled - 1, generator=g)[:PLANT_N]).tolist()
    groups = [tail, [0], rem, body]
    cols = []
    while len(cols) < PLANT_N:
        for grp in groups:
            if grp and len(cols) < PLANT_N:
                cols.append(grp.pop(0))
    assert len(set(cols)) == PLANT_N
    return cols


@functools.lru_cache(maxsize=None)
def _planted_case(dtype, V):
    g = _gen(77 + V)
    rows = len(PLANT_P) * len(PLANT_STEPS)
    logits = torch.empty(rows, V, dtype=dtype)
    temp, top_p, want = [], [], []
    for j, (step, (p, n)) in enumerate((s, pn) for s in PLANT_STEPS for pn in PLANT_P):
        T = step / -math.log(0.8)
        cols = _plant_columns(dtype, V, g)
        logits[j] = -30.0 * T
        logits[j, cols] = (-step * torch.arange(PLANT_N, dtype=torch.float64)).to(dtype)
        temp.append(T)
        top_p.append(p)
        want.append(n)
    c = dict(logits=logits, temp=torch.tensor(temp), top_k=torch.zeros(rows, dtype=torch.int32),
             top_p=torch.tensor(top_p), seeds=torch.arange(rows) + 1, pos=torch.arange(rows) + 7)
    c["thr"], c["kept"] = ref.sample_threshold(logits, c["temp"], c["top_k"], c["top_p"])
    c["tok"], c["val"] = ref.sample_shard(logits, c["temp"], c["seeds"], c["pos"], thr=c["thr"])
    return c, want


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype,V", [(BF16, 41003), (F32, 20503)], ids=lambda p: str(p).replace("torch.", ""))
def test_top_p_planted_rows_are_exact(dtype, V, layout):
    """40 columns with probabilities proportional to 0.8^i scattered over every region of the
    row walk, every other column 30 T lower: top_p 0.5 / 0.9 / 0.97 keep exactly 4 / 11 / 16
    columns (cumulative 0.488 | 0.590, 0.893 | 0.914, 0.965 | 0.972). An off-by-one bin or a
    dropped tail element changes the count, which the EPS check alone would let through."""
    c, want = _planted_case(dtype, V)
    for r in range(c["logits"].shape[0]):   # the reference first: every edge >= 1e-3 from top_p
        s, w = _masses(c["logits"][r], float(c["temp"][r]), 0)
        edges = torch.cumsum(w, 0) / w.sum()
        assert float((edges - float(c["top_p"][r])).abs().min()) >= 1e-3, r
    assert c["kept"].tolist() == want
    thr, kept = _run_threshold(_layout(c["logits"], layout), c)
    print("kept", kept.tolist(), "want", want, "thr", thr.tolist(), "ref", c["thr"].tolist())
    assert kept.tolist() == want
    assert torch.equal(_bits(thr), _bits(c["thr"]))
    tok, val = _run_sample(_layout(c["logits"], layout), c, top_k=c["top_k"], top_p=c["top_p"])
    for r in range(len(want)):
        assert float(c["logits"][r, tok[r]]) >= float(thr[r]), r


def test_binding_rejects_bad_arguments():
    x = torch.zeros(3, 16, dtype=BF16, device="cuda")
    t, k, p = torch.ones(3, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"), torch.ones(3, device="cuda")
    thr = torch.full((3,), 5.0, device="cuda")
    C = ops.kernels()
    with pytest.raises(RuntimeError):
        C.sample_threshold(x, t, k.long(), p, thr)          # top_k must be int32
    with pytest.raises(RuntimeError):
        C.sample_threshold(x, t, k, p, thr[:2])             # one threshold per row
    with pytest.raises(RuntimeError):
        C.sample_threshold(x, t, k.cpu(), p, thr)           # device tensors only
    torch.cuda.synchronize()
    assert (thr == 5.0).all()
    with pytest.raises(ValueError, match="col_offset"):
        ops.sample(x, t, torch.zeros(3, dtype=torch.long, device="cuda"), torch.zeros(3, dtype=torch.long, device="cuda"),
                   col_offset=16, top_k=k)


def test_engine_graphs_filter_prefill_and_decode_tokens():
    """One batch through the captured prefill and decode graphs: a default request, T = 1 with
    top_k = 1, T = 5 with top_p = 1e-6, T = 0, and T = 5 unfiltered, all on one prompt. The
    filtered two equal the greedy one from the first (prefill-sampled) token on, the
    unfiltered T = 5 request does not, and the default request's tokens are those it gets
    when it runs alone."""
    from operator_amd.engine.llm import GenRequest, LLMEngine
    from operator_amd.models.config import get_config
    from operator_amd.models.kv_cache import PagedKVCache
    from operator_amd.models.llama import LlamaModel

    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=5)
    prompt = list(range(3, 40))

    def run(specs):
        kv = PagedKVCache(cfg.layers, 128, cfg.kv_heads, 128, 16, device="cuda")
        eng = LLMEngine(m, kv, max_batch=8, max_prefill_tokens=512, max_context=512, use_graphs=True, multi_step=4)
        reqs = [GenRequest(list(prompt), max_tokens=10, seed=9, ignore_eos=True, **kw) for kw in specs]
        eng.generate(reqs)
        assert eng.stats.prefill_graph_replays >= 1 and eng.stats.prefill_eager == 0 and eng.stats.graph_replays > 0
        assert all(r.error is None and len(r.output) == 10 for r in reqs)
        return [r.output for r in reqs]

    default, k1, p0, greedy, hot = run([{}, {"temperature": 1.0, "top_k": 1}, {"temperature": 5.0, "top_p": 1e-6},
                                        {"temperature": 0.0}, {"temperature": 5.0}])
    print("default", default, "\ntop_k=1", k1, "\ntop_p=1e-6", p0, "\ngreedy", greedy, "\nT=5", hot)
    assert k1 == greedy and p0 == greedy
    assert hot[0] != greedy[0] and hot != greedy
    alone, = run([{}])
    print("default alone", alone)
    assert default == alone
