"""ac_scan v2, scan_fixup, the scorer and the line index on the paths that whole synthetic batches
reach only by chance (cases, references and censuses: tests/scan_cases.py, checked on the CPU by
tests/test_scan_cases_ref.py): streams that start inside a segment, matches that lie in a stream's
look-back, cold walks through chain bytes in LDS, through chain bytes in global memory and through
the table at every class-count, the rank cap and every tie of the event order."""
import numpy as np
import pytest
import scan_cases as sc
import torch

from operator_amd.engine.match import MatchEngine
from operator_amd.patterns import oracle

pytestmark = pytest.mark.gpu


def _engine(case, profile_bytes):
    eng = MatchEngine(case.patset, device="cuda", seg_bytes=case.seg, grid_blocks=case.grid_blocks,
                      profile_bytes=profile_bytes)
    eng.SCAN_LANES = 0        # keep the requested segment size (the engine halves it for small batches)
    assert eng.cp.factors == case.factors
    return eng


def _rows(a):
    return sorted(map(tuple, np.asarray(a).tolist()))


def _scan_and_check(case, eng):
    """Rows (all four columns) and per-document newlines equal the reference, twice on the same
    engine (buffer reuse, the launcher's memset of the totals and heads). Returns the head half of
    the per-segment newline counts."""
    n_segs = case.total // case.seg
    heads = None
    for rep in range(2):
        got = _rows(eng.scan_gpu(case.docs))
        assert eng.last_seg == case.seg
        assert len(got) == len(case.rows), (case.name, rep)
        assert got == case.rows, (case.name, rep)
        docs, nls = eng._doc_newlines
        assert docs is case.docs and nls == case.newlines, (case.name, rep)
        h = eng._seg_nl[n_segs:2 * n_segs].cpu().tolist()
        assert heads is None or h == heads
        heads = h
        totals = eng._seg_nl[:n_segs].cpu().tolist()
        assert totals == [case.text.count(b"\n", g * case.seg, (g + 1) * case.seg) for g in range(n_segs)]
    return heads


def _uploaded(eng):
    return dict(table=eng.table.cpu().numpy().view(np.uint16), cls_map=eng.cls_map.cpu().numpy().tobytes(),
                log2c=eng.log2c, states=eng.dfa_states, chain=eng.chain.cpu().numpy().tobytes(), H=eng.hot_states)


@pytest.mark.parametrize("case", sc.split_cases(), ids=lambda c: c.name)
def test_streams_that_start_inside_a_segment(case):
    """L % seg != 0: matches after a mid-segment stream start carry bit 31 and scan_fixup adds the
    segment's head count. The heads the device wrote are non-zero where the case says, and the
    reference has rows behind them, so the path ran here whatever the device's CU count."""
    eng = _engine(case, 0)
    heads = _scan_and_check(case, eng)
    assert any(heads)
    assert heads == sc.seg_heads(case)
    n = sc.check_split(case, heads)       # mid_rows counted with the DEVICE's heads
    assert n["mid_rows"] > 0


@pytest.mark.parametrize("profiled", [False, True], ids=["bfs", "profiled"])
@pytest.mark.parametrize("case", sc.scan_path_cases(), ids=lambda c: c.name)
def test_cold_walks(case, profiled):
    """The exact re-walk through cold states: by the table (breadth-first numbering) and by chain
    bytes (profiled numbering), ends on every byte of a chunk, walks held cold across chunks and
    across a stream's look-back, 3 / 6 / 7 / 8-bit class indices, chain bytes past the LDS."""
    eng = _engine(case, case.profile_bytes if profiled else 0)
    heads = _scan_and_check(case, eng)
    assert eng._profiled == profiled
    t = _uploaded(eng)
    n = sc.check_census(case, t, profiled)          # on the tables this engine uploaded
    ref = case.tables(case.profile_bytes if profiled else 0)
    assert np.array_equal(t["table"].reshape(-1), ref["table"]) and t["chain"] == ref["chain"]
    if case.name == "big-dfa":
        assert n["beyond_lds"] > 0 and t["states"] > sc.lds_chain_states() + 256
    if case.L % case.seg:
        assert heads == sc.seg_heads(case) and any(heads)


# ------------------------------------------------------------------------------------------ scorer
def _score(eng, docs):
    """score_events on hand-made hits, driven as MatchEngine._events_gpu drives it. Returns
    (hits, per-document (score, pattern, line, order), summary)."""
    from operator_amd.ops import kernels

    hits = np.asarray([(d, m, l) for d, hs in enumerate(docs) for m, l in hs], np.int64).reshape(-1, 3)
    T, dev, n_docs, n = eng._gpu_tables(), eng.device, len(docs), hits.shape[0]
    doc, mat, line = hits[:, 0], hits[:, 1], hits[:, 2]
    doc_ptr = np.zeros(n_docs + 1, np.int64)
    doc_ptr[1:] = np.cumsum(np.bincount(doc, minlength=n_docs))
    nm = T["npat"].shape[0]
    ev_ptr = np.zeros(n + 1, np.int64)
    ev_ptr[1:] = np.cumsum(np.where(mat < nm, T["npat"][np.minimum(mat, nm - 1)], 0))
    ev_doc_ptr = ev_ptr[doc_ptr]
    E = int(ev_ptr[-1])
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32).to(dev)  # noqa: E731
    keys = torch.as_tensor((mat << 32) | line, dtype=torch.long).to(dev)
    ev_score = torch.full((E,), float("nan"), dtype=torch.float64, device=dev)
    ev_pat, ev_line, order = (torch.full((E,), -7, dtype=torch.int32, device=dev) for _ in range(3))
    summary = torch.full((3 * n_docs,), -7, dtype=torch.int32, device=dev)
    kernels().score_events(keys, i32(doc), i32(doc_ptr), T["prim_ptr"], T["prim_pat"], i32(ev_ptr), i32(ev_doc_ptr),
                           T["sec_ptr"], T["sec_matcher"], T["sec_w"], T["sec_win"], T["conf"], T["severity"],
                           float(eng.significance), ev_score, ev_pat, ev_line, order, summary)
    torch.cuda.synchronize()
    s, p, l, o = (x.cpu().numpy() for x in (ev_score, ev_pat, ev_line, order))
    per = [(s[a:b], p[a:b], l[a:b], o[a:b] - a) for a, b in zip(ev_doc_ptr[:-1], ev_doc_ptr[1:])]
    return hits, per, summary.cpu().numpy().reshape(n_docs, 3)


def _want_summary(cp, evs, significance):
    sev = [cp.patset.patterns[e.pattern].severity_rank for e in evs]
    return [max(sev, default=-1), sum(e.score >= significance for e in evs), len(evs)]


def test_scorer_exact_scores_full_order_and_rank_cap():
    """Dyadic inputs: every score is one correctly rounded division of exact operands, so it must
    equal the fp64 formula bit for bit, and the ranking the full four-level order: ties at every
    level, 0 .. 2048 events a document (around the bitonic padding, at the cap), window edges, a
    score equal to the significance threshold, matcher ids past the compiled set."""
    c = sc.score_exact_case()
    eng = MatchEngine(c.patset, device="cuda")
    hits, per, summary = _score(eng, c.docs)
    seen = []
    for d, (hs, (s, p, l, o)) in enumerate(zip(c.docs, per)):
        want = oracle.score_doc(eng.cp, set(hs))
        assert summary[d].tolist() == _want_summary(eng.cp, want, eng.significance), d
        seen.append(len(want))
        assert len(s) == len(want)
        got = {(int(p[i]), int(l[i])): float(s[i]) for i in range(len(s))}
        assert got == {(e.pattern, e.line): e.score for e in want}, d          # bit-equal scores
        if len(want) <= sc.RANK_CAP:
            assert sorted(o.tolist()) == list(range(len(want))), d             # a permutation
            assert [(int(p[i]), int(l[i])) for i in o] == [(e.pattern, e.line) for e in want], d
    assert seen[1:1 + len(sc.RANK_COUNTS)] == list(sc.RANK_COUNTS) and seen[-1] == sc.RANK_CAP + 1
    assert summary[0, 1] > 0 and any(e.score == eng.significance for e in oracle.score_doc(eng.cp, set(c.docs[0])))
    # past the cap the engine ranks on the host, with the same key
    evs = eng._events_gpu(hits, len(c.docs))
    for d, hs in enumerate(c.docs):
        assert evs[d] == oracle.score_doc(eng.cp, set(hs)), d


def test_scorer_random_scores_within_the_rounding_bound():
    """Non-dyadic inputs: each score within (2 n_sec + 3) fp64 roundings of the plain formula;
    events of one document are >= 1e-6 apart, so the order cannot hinge on that."""
    c = sc.score_random_case()
    eng = MatchEngine(c.patset, device="cuda")
    _, per, summary = _score(eng, c.docs)
    bound = sc.score_bound(c.n_sec)
    worst = 0.0
    for d, (hs, (s, p, l, o)) in enumerate(zip(c.docs, per)):
        want = oracle.score_doc(eng.cp, set(hs))
        sc.check_score_gap(want)
        assert summary[d].tolist() == _want_summary(eng.cp, want, eng.significance), d
        assert [(int(p[i]), int(l[i])) for i in o] == [(e.pattern, e.line) for e in want], d
        for i, e in zip(o, want):
            worst = max(worst, abs(float(s[i]) - e.score) / e.score)
            assert abs(float(s[i]) - e.score) <= bound * e.score, (d, e, float(s[i]))
    print(f"worst relative distance {worst:.3e} (bound {bound:.3e})")
    assert summary[0].tolist() == [-1, 0, 0]


# ------------------------------------------------------------------------------------------ line index
@pytest.mark.parametrize("n", [4095, 4096, 4097, 9000])
def test_line_prefix_counts_are_unsigned_and_sums_64_bit(n):
    """Counts 0xffffffff (int32 -1) and 0x7fffffff: the prefix is the int64 cumsum of the values
    read as uint32, on both sides of a tile boundary and over three tiles; twice on one state."""
    from operator_amd.ops import kernels

    C = kernels()
    g = torch.Generator(device="cpu").manual_seed(n)
    pick = torch.randint(0, 2, (n,), generator=g)
    pick[0], pick[-1] = 0, 1
    cnt = torch.where(pick == 0, torch.tensor(-1, dtype=torch.int32), torch.tensor(0x7FFFFFFF, dtype=torch.int32))
    ref = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt.to(torch.int64) & 0xFFFFFFFF, 0)])
    assert int(ref[-1]) > n * 0x7FFFFFFF and int(ref[1]) == 0xFFFFFFFF
    excl = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((C.line_prefix_state_words(n),), -1, dtype=torch.int64, device="cuda")
    first = torch.tensor(sorted({min(x, n) for x in (0, 1, 4095, 4096, 4097, n)}), dtype=torch.int64)
    dn = torch.empty(len(first) - 1, dtype=torch.int64, device="cuda")
    for _ in range(2):
        C.line_prefix(cnt.cuda(), excl, st)
        assert torch.equal(excl.cpu(), ref)
        assert int(st[1]) == 0            # error word: no look-back gave up
        C.doc_lines(excl, first.cuda(), dn)
        assert dn.cpu().tolist() == [int(ref[b] - ref[a]) for a, b in zip(first[:-1], first[1:])]
