"""Repetition / frequency / presence penalties on the GPU: penalty_seed and sample_penalty
(csrc/kernels/penalty.hip) against the plain-torch reference (ops/reference.py), and the
engine's captured prefill and decode graphs with penalised and plain requests in one batch.

Every comparison is bit-exact: the semantics round each fp32 operation on its own (no fused
multiply-add, a correctly rounded division), so fp32 torch on the CPU gives the kernel's bits.
Logits are compared as integers, whole buffers at a time (canaries outside strided rows and
NaN payloads included), and so is the whole table.
"""
from collections import Counter

import pytest
import torch

from operator_amd import ops
from operator_amd.models.penalty import PenaltyTable
from operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
I32 = torch.int32
LAYOUTS = ["contig", "aligned", "unaligned"]
SHAPES = [(BF16, 1), (BF16, 7), (BF16, 8), (BF16, 1003), (BF16, 41003), (F32, 7), (F32, 1003)]
# (r, f, p): each penalty alone at both of its values, then combined, then all off
PARAMS = [(1.3, 0.0, 0.0), (0.5, 0.0, 0.0), (1.0, 0.7, 0.0), (1.0, -1.5, 0.0), (1.0, 0.0, 1.1), (1.0, 0.0, -2.0),
          (1.3, 0.7, 1.1), (0.5, -1.5, -2.0), (1.3, -1.5, 1.1), (0.5, 0.7, -2.0), (1.0, 0.7, 1.1), (1.0, 0.0, 0.0)]
CANARY = 12345.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else I32)


def _buffer(logits, layout):
    """(host buffer, column of the rows' first element): contig: the rows as they are; aligned:
    rows at a stride that is a multiple of 8 elements; unaligned: the same, one element in.
    Outside the rows the buffer holds CANARY."""
    rows, V = logits.shape
    if layout == "contig":
        return logits.clone(), 0
    stride = (V + 1 + 7) // 8 * 8 + 8
    buf = torch.full((rows, stride), CANARY, dtype=logits.dtype)
    c0 = 0 if layout == "aligned" else 1
    buf[:, c0:c0 + V] = logits
    return buf, c0


def _to_gpu(tb):
    g = PenaltyTable(tb.slots, tb.vocab, tb.cap, device="cuda")
    g.cnt.copy_(tb.cnt)
    g.lst.copy_(tb.lst)
    g.n.copy_(tb.n)
    return g


def _clone(tb):
    c = PenaltyTable(tb.slots, tb.vocab, tb.cap, device="cpu")
    c.cnt.copy_(tb.cnt)
    c.lst.copy_(tb.lst)
    c.n.copy_(tb.n)
    return c


def _same_table(g, c):
    torch.cuda.synchronize()
    assert torch.equal(g.n.cpu(), c.n)
    assert torch.equal(g.cnt.cpu(), c.cnt)
    assert torch.equal(g.lst.cpu(), c.lst)


def _fill_slot(tb, slot, n, g):
    """``n`` distinct random tokens in ``slot``'s list; their words cycle through prompt-only,
    generated once, both (c = 2) and c = 3000."""
    V = tb.vocab
    toks = torch.randperm(V, generator=g)[:n]
    kinds = torch.tensor([ref.PROMPT_BIT, 1, ref.PROMPT_BIT + 2, 3000], dtype=torch.long)
    tb.cnt[slot, toks] = kinds[torch.arange(n) % 4].to(I32)
    tb.lst[slot, :n] = toks.to(I32)
    tb.n[slot] = n
    return toks


def _apply_case(dtype, V, seed=0):
    """Rows: 0 no slot (NaN payloads, must keep its bytes); 1-6 a list of 0, 1, 255, 256, 257,
    min(V, 3000) tokens (the edges of a 256-thread stride); 7 every token seen; 8.. one row
    per PARAMS entry. Rows map to slots by a permutation; NaN, +-inf and +-0 are planted on
    seen tokens."""
    g = _gen(seed + V)
    sizes = [None, 0, 1, 255, 256, 257, min(V, 3000), V] + [min(V, 300)] * len(PARAMS)
    rows = len(sizes)
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    nan_bits = torch.tensor([0x7FC1, 0xFFC2 - 0x10000, 0x7F81], dtype=torch.int16)
    if dtype == BF16:
        logits[0, :min(V, 3)] = nan_bits[:min(V, 3)].view(BF16)
    else:
        logits[0, :min(V, 3)] = (nan_bits[:min(V, 3)].to(I32) << 16 | 5).view(F32)
    slots = rows + 2
    perm = torch.randperm(slots, generator=g)[:rows].to(I32)
    tb = PenaltyTable(slots, V, V + 3, device="cpu")
    pslot = perm.clone()
    pslot[0] = -1
    _fill_slot(tb, int(perm[0]), min(V, 50), g)   # a live slot that row 0 must not use
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0])
    for r in range(1, rows):
        n = min(sizes[r], V)
        toks = _fill_slot(tb, int(perm[r]), n, g)
        if n >= 6:
            logits[r, toks[:5]] = special.to(dtype)
    par = torch.tensor([PARAMS[(r + 3) % len(PARAMS)] if r < 8 else PARAMS[r - 8] for r in range(rows)], dtype=F32)
    return logits, pslot, par[:, 0].contiguous(), par[:, 1].contiguous(), par[:, 2].contiguous(), tb


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype,V", SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_apply_matches_reference(dtype, V, layout):
    logits, pslot, rep, freq, pres, tb = _apply_case(dtype, V)
    want = logits.clone()
    tb_ref = _clone(tb)
    ref.sample_penalty(want, pslot, None, None, rep, freq, pres, tb_ref.cnt, tb_ref.lst, tb_ref.n)
    assert torch.equal(_bits(want[0]), _bits(logits[0]))                 # no slot: untouched by the reference too
    assert not torch.equal(_bits(want[8:]), _bits(logits[8:]))           # the case does penalise
    buf, c0 = _buffer(logits, layout)
    exp = buf.clone()
    exp[:, c0:c0 + V] = want
    dbuf = buf.cuda()
    view = dbuf[:, c0:c0 + V]
    assert layout == "contig" or (view.data_ptr() % 16 == 0) == (layout == "aligned")
    gt = _to_gpu(tb)
    out = ops.sample_penalty(view, pslot.cuda(), None, None, rep.cuda(), freq.cuda(), pres.cuda(), gt)
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    got = dbuf.cpu()
    bad = torch.nonzero(_bits(got) != _bits(exp))
    assert bad.numel() == 0, f"{bad.shape[0]} logits differ, first (row, col) {bad[0].tolist()}"
    _same_table(gt, tb)                                                  # last_tok null: the table is read only


def test_count_then_apply_in_one_call():
    V, cap = 1003, 40
    g = _gen(7)
    rows = 8
    tb = PenaltyTable(rows + 1, V, cap, device="cpu")
    slot_of = [3, 0, 5, 1, 2, 6, 7, 4]                                  # row -> slot
    for s in range(rows + 1):
        _fill_slot(tb, s, 12 if s != 4 else cap, g)                      # slot 4 (row 7): its list is full
    free = lambda s: next(t for t in range(V) if int(tb.cnt[s, t]) == 0)   # noqa: E731
    listed = lambda s, w: next(int(t) for t in tb.lst[s, :12] if int(tb.cnt[s, t]) == w)   # noqa: E731
    shared = next(t for t in range(V) if int(tb.cnt[6, t]) == 0 and int(tb.cnt[7, t]) == 0)
    last = [free(3), listed(0, 1), listed(5, ref.PROMPT_BIT), free(1), free(2), shared, shared, free(4)]
    pslot = torch.tensor(slot_of, dtype=I32)
    pslot[4] = -1                                                        # row 4: no slot
    ctx = torch.tensor([9, 9, 9, 0, 9, 9, 9, 9], dtype=I32)              # row 3: padding
    last_tok = torch.tensor(last)
    par = torch.tensor([PARAMS[r] for r in (6, 7, 8, 9, 6, 7, 8, 9)], dtype=F32)
    rep, freq, pres = (par[:, i].contiguous() for i in range(3))
    logits = (torch.randn(rows, V, generator=g) * 4).to(BF16)
    before = _clone(tb)
    want, tb_ref = logits.clone(), _clone(tb)
    ref.sample_penalty(want, pslot, last_tok, ctx, rep, freq, pres, tb_ref.cnt, tb_ref.lst, tb_ref.n)
    gt = _to_gpu(tb)
    dl = logits.cuda()
    ops.sample_penalty(dl, pslot.cuda(), last_tok.cuda(), ctx.cuda(), rep.cuda(), freq.cuda(), pres.cuda(), gt)
    _same_table(gt, tb_ref)
    assert torch.equal(_bits(dl.cpu()), _bits(want))                     # the reference applied after counting
    t = gt
    n, cnt, lst = t.n.cpu(), t.cnt.cpu(), t.lst.cpu()
    assert int(n[3]) == 13 and int(lst[3, 12]) == last[0] and int(cnt[3, last[0]]) == 1        # new: appended, c = 1
    assert int(n[0]) == 12 and int(cnt[0, last[1]]) == 2                                       # generated before: c + 1
    assert int(n[5]) == 12 and int(cnt[5, last[2]]) == ref.PROMPT_BIT + 1                      # prompt only: bit kept
    for s in (1, 2, 4, 8):                                                                     # ctx 0, no slot, full, unused
        assert torch.equal(cnt[s], before.cnt[s]) and torch.equal(lst[s], before.lst[s]) and n[s] == before.n[s]
    assert int(cnt[6, shared]) == 1 and int(cnt[7, shared]) == 1 and int(n[6]) == int(n[7]) == 13
    assert torch.equal(_bits(dl.cpu()[[3, 4]]), _bits(logits[[3, 4]]))                         # those rows' logits too


def test_seed_matches_reference():
    V, cap, S = 1003, 4200, 7
    g = _gen(11)
    tb = PenaltyTable(S, V, cap, device="cpu")
    for s in range(S):
        _fill_slot(tb, s, 100 + 30 * s, g)                               # previous occupants / a planted pattern
    prompts = [[V - 1], [0, 0], (torch.randint(0, 90, (257,), generator=g)).tolist(),
               torch.randint(0, V + 40, (4096,), generator=g).tolist()]   # duplicates; ids >= V in the last
    prompts[2][5], prompts[2][200] = 0, V - 1
    prompts[3][17], prompts[3][18], prompts[3][19] = V, V - 1, 0
    named = [5, 0, 3, 1]
    cu = torch.tensor([0] + torch.tensor([len(p) for p in prompts]).cumsum(0).tolist(), dtype=I32)
    ids = torch.tensor([t for p in prompts for t in p])
    slots = torch.tensor(named, dtype=I32)
    want = _clone(tb)
    ref.penalty_seed(want.cnt, want.lst, want.n, slots, ids, cu)
    gt = _to_gpu(tb)
    ops.penalty_seed(gt, slots.cuda(), ids.cuda(), cu.cuda())
    torch.cuda.synchronize()

    def check(gt, want, named):
        cnt, lst, n = gt.cnt.cpu(), gt.lst.cpu(), gt.n.cpu()
        assert torch.equal(n, want.n) and torch.equal(cnt, want.cnt)
        for s in range(S):
            k = int(n[s])
            if s in named:
                assert sorted(lst[s, :k].tolist()) == sorted(want.lst[s, :k].tolist())
            else:
                assert torch.equal(lst[s], tb.lst[s]) and torch.equal(cnt[s], tb.cnt[s])   # not named: the pattern

    check(gt, want, named)
    for p, s in zip(prompts, named):
        u = sorted({t for t in p if t < V})
        assert int(want.n[s]) == len(u) and torch.nonzero(want.cnt[s]).flatten().tolist() == u
    # seeded twice: slots 5 and 0 swap prompts; both equal a fresh seeding
    cu2 = torch.tensor([0, len(prompts[3]), len(prompts[3]) + len(prompts[2])], dtype=I32)
    ids2 = torch.tensor(prompts[3] + prompts[2])
    slots2 = torch.tensor([5, 0], dtype=I32)
    ops.penalty_seed(gt, slots2.cuda(), ids2.cuda(), cu2.cuda())
    fresh = PenaltyTable(S, V, cap, device="cpu")
    ref.penalty_seed(fresh.cnt, fresh.lst, fresh.n, slots2, ids2, cu2)
    torch.cuda.synchronize()
    for s in (5, 0):
        k = int(fresh.n[s])
        assert int(gt.n[s]) == k and torch.equal(gt.cnt[s].cpu(), fresh.cnt[s])
        assert sorted(gt.lst[s, :k].tolist()) == sorted(fresh.lst[s, :k].tolist())
    assert torch.equal(gt.cnt[[3, 1]].cpu(), want.cnt[[3, 1]])           # the other two are as they were


def test_graph_replay_counts_on_the_device():
    """Count-and-apply captured once, last_tok fed back on the device: three replays equal three
    reference steps. The warm-up and the capture hold pslot at -1, as the engine's do."""
    V, rows = 1003, 4
    g = _gen(3)
    base = torch.randn(rows, V, generator=g) * 2    # fp32: no ties for the argmax that feeds last_tok
    tb = PenaltyTable(6, V, 64, device="cpu")
    for s in range(6):
        _fill_slot(tb, s, 20, g)
    pslot = torch.tensor([4, -1, 0, 2], dtype=I32)
    ctx = torch.tensor([5, 5, 5, 5], dtype=I32)
    par = torch.tensor([PARAMS[3], PARAMS[6], PARAMS[7], PARAMS[9]], dtype=F32)   # negative f: repeats are rewarded
    rep, freq, pres = (par[:, i].contiguous() for i in range(3))
    tok0 = torch.tensor([1, 2, 3, 4])
    d = {k: v.cuda() for k, v in dict(base=base, ctx=ctx, rep=rep, freq=freq, pres=pres).items()}
    gt = _to_gpu(tb)
    dps = torch.full((rows,), -1, dtype=I32, device="cuda")
    last = tok0.cuda()
    work = torch.empty_like(d["base"])

    def step():
        work.copy_(d["base"])
        ops.sample_penalty(work, dps, last, d["ctx"], d["rep"], d["freq"], d["pres"], gt)
        last.copy_(work.float().argmax(1))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    _same_table(gt, tb)                                                  # neither touched the table
    dps.copy_(pslot)
    last.copy_(tok0)
    want_tb, tok = _clone(tb), tok0.clone()
    for _ in range(3):
        graph.replay()
        w = base.clone()
        ref.sample_penalty(w, pslot, tok, ctx, rep, freq, pres, want_tb.cnt, want_tb.lst, want_tb.n)
        tok = w.float().argmax(1)
    _same_table(gt, want_tb)
    assert torch.equal(_bits(work.cpu()), _bits(w)) and torch.equal(last.cpu(), tok)
    assert int(want_tb.n.sum()) > int(tb.n.sum())                        # tokens were appended


def test_bindings_reject_bad_operands():
    C = ops.kernels()
    V, rows = 64, 3
    tb = PenaltyTable(4, V, 16, device="cuda")
    tb.cnt.fill_(7)
    tb.lst.fill_(7)
    tb.n.fill_(7)
    x = torch.full((rows, V), 5.0, dtype=BF16, device="cuda")
    ps = torch.zeros(rows, dtype=I32, device="cuda")
    one = torch.ones(rows, device="cuda")
    last = torch.zeros(rows, dtype=torch.long, device="cuda")
    ok = (x, ps, last, None, one, one, one, tb.cnt, tb.lst, tb.n)

    def bad(i, v):
        a = list(ok)
        a[i] = v
        with pytest.raises(RuntimeError):
            C.sample_penalty(*a)

    bad(1, ps.long())                    # pslot must be int32
    bad(1, ps[:2])                       # one slot per row
    bad(1, ps.cpu())                     # device tensors only
    bad(4, one.double())                 # rep must be fp32
    bad(4, one[:2])
    bad(4, one.cpu())
    bad(2, last.to(I32))                 # last_tok must be int64
    bad(3, ps.long())                    # ctx must be int32
    bad(7, tb.cnt.long())                # the table is int32 ...
    bad(7, tb.cnt[:3])                   # ... its tensors agree in slots ...
    bad(7, tb.cnt[:, :V - 1])            # ... contiguous, and as wide as the logits
    bad(8, tb.lst.cpu())
    bad(9, tb.n[:2])
    bad(0, x.cpu())
    bad(0, x.half())
    sl = torch.zeros(1, dtype=I32, device="cuda")
    ids = torch.zeros(4, dtype=torch.long, device="cuda")
    cu = torch.tensor([0, 4], dtype=I32, device="cuda")
    for args in ((sl.long(), ids, cu), (sl, ids.to(I32), cu), (sl, ids, cu.long()), (sl, ids, cu[:1]),
                 (sl.cpu(), ids, cu), (sl, ids.cpu(), cu)):
        with pytest.raises(RuntimeError):
            C.penalty_seed(*args, tb.cnt, tb.lst, tb.n)
    with pytest.raises(RuntimeError):
        C.penalty_seed(sl, ids, cu, tb.cnt, tb.lst.long(), tb.n)
    torch.cuda.synchronize()
    assert (x == 5.0).all() and (tb.cnt == 7).all() and (tb.lst == 7).all() and (tb.n == 7).all()


# ---------------------------------------------------------------------------------------------
# the engine: captured prefill and decode graphs
# ---------------------------------------------------------------------------------------------

def _slot_state(eng, slot):
    tb = eng.penalties
    n = int(tb.n[slot])
    lst = tb.lst[slot, :n].tolist()
    assert len(set(lst)) == n
    w = tb.cnt[slot].cpu().long()
    nz = torch.nonzero(w).flatten().tolist()
    assert sorted(lst) == nz                                             # the list names exactly the non-zero words
    prompt = set(torch.nonzero(w < 0).flatten().tolist())
    counts = {t: int(w[t]) & ref.COUNT_MASK for t in nz if int(w[t]) & ref.COUNT_MASK}
    return prompt, counts


def _check_engine(eng, prompt):
    from operator_amd.engine.llm import GenRequest

    slots = {}
    release = eng._release

    def spy(r):
        if r.pslot >= 0:
            slots[id(r)] = r.pslot
        release(r)

    eng._release = spy
    try:
        mk = lambda n=10, **kw: GenRequest(list(prompt), max_tokens=n, temperature=0.0, ignore_eos=True, **kw)   # noqa: E731
        alone = mk()
        eng.generate([alone])
        t0 = alone.output[0]
        # the 3-token request finishes first: a load renumbers the other rows mid-run
        plain, short, freq, pres, rep = reqs = [mk(), mk(3, presence_penalty=100.0), mk(frequency_penalty=-100.0),
                                                mk(presence_penalty=100.0), mk(repetition_penalty=1.5)]
        eng.generate(reqs)
        print("alone", alone.output, "\nplain", plain.output, "\nfreq -100", freq.output, "\npres 100", pres.output,
              "\nrep 1.5", rep.output)
        assert eng.stats.prefill_graph_replays >= 1 and eng.stats.prefill_eager == 0 and eng.stats.graph_replays > 0
        assert all(r.error is None and r.done for r in reqs)
        assert plain.output == alone.output
        assert freq.output == [t0] * 10       # the first decode step counts the prefill-sampled token; counts add up across windows
        assert len(set(pres.output)) == 10 and len(short.output) == 3
        assert len({slots[id(r)] for r in reqs[1:]}) == 4 and id(plain) not in slots
        for r in reqs[1:]:
            seen, counts = _slot_state(eng, slots[id(r)])
            assert seen == set(prompt), "bit 31 on exactly the prompt's tokens"
            assert counts == dict(Counter(r.output[:-1])), "c = the histogram of output[:-1]"
        assert eng.penalties.free == eng.penalties.slots
        return alone.output
    finally:
        eng._release = release


def _gpu_engine(prefix_sharing):
    from operator_amd.engine.llm import LLMEngine
    from operator_amd.models.config import get_config
    from operator_amd.models.kv_cache import PagedKVCache
    from operator_amd.models.llama import LlamaModel

    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=5)
    kv = PagedKVCache(cfg.layers, 128, cfg.kv_heads, 128, 16, device="cuda")
    return LLMEngine(m, kv, max_batch=8, max_prefill_tokens=512, max_context=512, use_graphs=True, multi_step=4,
                     prefix_sharing=prefix_sharing)


PROMPT = [7, 8, 9, 7, 8, 9, 7, 8, 30, 31, 7, 8]


def test_engine_graphs_count_and_penalise():
    eng = _gpu_engine(prefix_sharing=False)
    _check_engine(eng, PROMPT)
    assert eng.penalties.cnt.is_cuda and eng.penalties.cnt.shape == (8, 2048)


def test_engine_graphs_with_a_shared_prefix_and_reused_slots():
    eng = _gpu_engine(prefix_sharing=True)
    prompt = list(range(40, 40 + 37)) + PROMPT
    _check_engine(eng, prompt)
    hits = eng.stats.prefix_hits
    _check_engine(eng, prompt)      # slots reused; the prompts now sit on the shared prefix
    assert eng.stats.prefix_hits > hits
