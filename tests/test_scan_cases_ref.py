"""The cases of tests/scan_cases.py, checked without a GPU: the reference scan against a second one
written differently, every case against the path it was built to reach, the scorer cases against
rational arithmetic."""
import re
from fractions import Fraction

import numpy as np
import pytest
import scan_cases as sc

from operator_amd.patterns import oracle
from operator_amd.patterns.compiler import compile_patterns

SCAN = {c.name: c for c in sc.split_cases() + sc.scan_path_cases()}


def _regex_scan(factors, docs):
    """Every occurrence by a zero-width lookahead (so overlapping ones are found), ignoring case;
    the line of a match end is the newlines before it."""
    rows = []
    for di, d in enumerate(docs):
        for fi, f in enumerate(factors):
            for m in re.finditer(b"(?=" + re.escape(f) + b")", d, re.I):
                end = m.start() + len(f) - 1
                rows.append((di, fi, d.count(b"\n", 0, end), end))
    return sorted(rows)


@pytest.mark.parametrize("name", list(SCAN))
def test_ref_scan_equals_regex_scan(name):
    c = SCAN[name]
    assert len(c.rows) > 0
    assert c.rows == _regex_scan(c.factors, c.docs)
    assert len({f for f in c.factors}) == len(c.factors) and all(f == f.lower() for f in c.factors)
    total, first = c.layout
    assert total % c.seg == 0 and len(c.text) == total
    for d, f in zip(c.docs, first):
        assert c.text[f * c.seg:f * c.seg + len(d)] == d and c.text[f * c.seg + len(d)] == 0


def test_stream_len_is_the_launchers_rule():
    assert sc.stream_len(1, 64, 1) == 64
    assert sc.stream_len(1024 * 128, 128, 1) == 128
    assert sc.stream_len(1024 * 128 + 1, 128, 1) == 192          # 129 bytes a stream, in whole chunks
    assert sc.stream_len(1024 * 192, 128, 1) == 192
    assert sc.stream_len(1024 * 192, 1024, 1) == 1024            # never below a segment
    assert sc.stream_len(2048 * 192 + 1, 128, 2) == 256
    assert sc.lds_chain_states(258) == 31488


@pytest.mark.parametrize("case", sc.split_cases(), ids=lambda c: c.name)
def test_split_cases_start_streams_inside_segments(case):
    n = sc.check_split(case)
    assert (case.seg, case.L, case.grid_blocks, case.total // case.seg) in sc.SPLIT_GEOMETRY
    heads = sc.seg_heads(case)
    assert any(heads) and len(heads) == case.total // case.seg
    if case.total // case.seg in (1499, 2345):
        assert n["short_last"] and n["idle_lanes"] > 0
    if case.grid_blocks == 2:
        assert 1024 < -(-case.total // case.L) < 2048           # a partly filled second block


@pytest.mark.parametrize("profiled", [False, True], ids=["bfs", "profiled"])
@pytest.mark.parametrize("case", sc.scan_path_cases(), ids=lambda c: c.name)
def test_walk_cases_reach_their_paths(case, profiled):
    t = case.tables(case.profile_bytes if profiled else 0)
    n = sc.check_census(case, t, profiled)
    assert n["via_chain"] + n["via_table"] == n["cold_steps"]
    if case.name == "big-dfa":
        assert sc.lds_chain_states() + 256 < t["states"] <= 32768 and n["beyond_lds"] > 0
    else:
        assert n["beyond_lds"] == 0


def test_cold_literals_have_the_lengths_prefixes_and_suffixes():
    sweep, extra = sc.cold_literals()
    assert sorted({len(f) for f in sweep}) == [16, 17, 33, 63, 64]
    a64, a63, b64, c64 = sweep[0], sweep[1], sweep[5], sweep[6]
    assert b64[:40] == a64[:40] and b64[40] != a64[40] and c64[:56] == a64[:56]
    assert sum(a64.endswith(f) for f in extra) == 3 and sum(a63.endswith(f) for f in extra) == 1
    for c in sc.cold_cases():
        d = c.cp.dfa
        off = np.frombuffer(d["out_off"], np.uint32)
        assert int(np.diff(off).max()) >= 4                        # a64's end state: itself and three suffixes
        assert d["num_states"] > sc.HOT


@pytest.mark.parametrize("case", sc.class_cases(), ids=lambda c: c.name)
def test_class_cases_compile_to_their_class_count(case):
    d = case.cp.dfa
    assert d["log2_classes"] == case.want["log2c"]
    lo = 0 if case.want["log2c"] == 3 else 1 << (case.want["log2c"] - 1)
    assert lo < d["num_classes_used"] <= 1 << d["log2_classes"]
    if case.want["log2c"] >= 7:
        assert any(b >= 0x80 for f in case.factors for b in f)
    if case.want["log2c"] == 6:
        assert 33 <= d["num_classes_used"] <= 64


# ------------------------------------------------------------------------------------------ scorer
def test_exact_score_case_is_exact_and_covers_its_edges():
    c = sc.score_exact_case()
    cp = compile_patterns(c.patset, build_dfa=False)
    assert [m.literal for m in cp.matchers] == [b"p-a", b"s-near", b"s-far", b"p-b", b"p-c", b"s-gone"]
    counts = []
    for hits in c.docs:
        evs = oracle.score_doc(cp, set(hits))
        exact = sc.exact_scores(cp, hits)
        assert len(evs) == len(exact)
        for e in evs:
            q = exact[e.pattern, e.line]
            assert float(q) == e.score                      # the fp64 formula rounded once
            den = 1 + sum(Fraction(s.weight) for s in cp.patset.patterns[e.pattern].secondary)
            assert float(q * den) == q * den and float(den) == den   # numerator and denominator exact in fp64
        counts.append(len(evs))
    assert counts[1:2 + len(sc.RANK_COUNTS) - 1] == list(sc.RANK_COUNTS) and counts[-1] == sc.RANK_CAP + 1
    evs = oracle.score_doc(cp, set(c.docs[0]))
    sc_of = {(e.pattern, e.line): e.score for e in evs}
    base = 0.5 / 1.75
    assert sc_of[0, 100] == 0.5 * (1 + 0.5 + 0.25 * 0.25) / 1.75         # dist 0; dist == window on both sides
    assert sc_of[0, 200] == 0.5 * (1 + 0.5 * 0.125) / 1.75               # dist == window counts, window + 1 does not
    assert sc_of[0, 300] == base                                          # both one past their window
    assert sc_of[0, 400] == 0.5 * (1 + 0.5 * 0.125) / 1.75               # equally far on both sides
    assert sc_of[3, 5] == 0.5                                             # == significance
    assert sc_of[4, 500] == 0.625 / 1.5 and sc_of[5, 100] == 0.875 and sc_of[5, 208] == 0.875 / 2
    # ties at every level of the order, next to each other in the ranking
    rank = [(e.pattern, e.line) for e in evs]
    assert rank.index((1, 200)) + 1 == rank.index((2, 200))               # score, severity equal: pattern
    assert rank.index((2, 400)) < rank.index((0, 200))                    # score equal: severity
    assert rank.index((3, 5)) + 1 == rank.index((3, 6))                   # same pattern: line
    assert any(m >= cp.num_matchers for m, _ in c.docs[0])


def test_random_score_case_keeps_events_apart():
    c = sc.score_random_case()
    cp = compile_patterns(c.patset, build_dfa=False)
    assert max(len(s) for s in cp.pattern_secondary) == c.n_sec == 4
    assert c.docs[0] == [] and sum(len(oracle.score_doc(cp, set(h))) for h in c.docs) > 50
    bonus = 0
    for hits in c.docs:
        evs = oracle.score_doc(cp, set(hits))
        sc.check_score_gap(evs)
        exact = sc.exact_scores(cp, hits)
        for e in evs:
            q = float(exact[e.pattern, e.line])
            assert abs(e.score - q) <= sc.score_bound(c.n_sec) * q
            bonus += e.score > cp.patset.patterns[e.pattern].primary.confidence / \
                (1 + sum(s.weight for s in cp.patset.patterns[e.pattern].secondary)) * (1 + 1e-9)
    assert bonus > 10
    assert sc.score_bound(4) == 11 * 2.0 ** -52
