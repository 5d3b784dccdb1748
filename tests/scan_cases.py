"""Cases and CPU references for the log scan, the scorer and the line index (tests/test_scan_paths_gpu.py;
checked on the CPU by tests/test_scan_cases_ref.py).

ac_scan v2 (csrc/kernels/scan.hip) cuts the packed text into `grid x 1024` equal streams and walks
each in 64-byte chunks: a branch-free walk over the 256 hot states in LDS, and an exact re-walk of
every 16-byte sub-chunk that touched a cold or an output state (chain bytes from LDS or, past
`chain_lds` states, from global memory; the full table otherwise). Which of these paths a batch
reaches follows from its size, its DFA and the state numbering, so every case here is built FOR one
path and carries the census that proves it got there: `stream_len` is the launcher's stream rule,
`walk_census` a CPU walk of the tables the engine uploads that counts the steps of each kind, and
the `check_*` functions assert the counts. A case that stops reaching its path fails; none passes
empty. The reference of every scan is `ref_scan`: `bytes.find` on the lower-cased document.

Nothing here touches a GPU; the DFA compiler and the renumbering are the host's (operator_amd._patterns)."""
import bisect
import functools
import random
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from operator_amd.patterns.schema import PatternSet

HOT = 256                 # ac_scan v2's hot set: states below it never leave the LDS rows
SCAN_LDS = 160 * 1024     # LDS of one CU: class map, hot rows, then as many chain bytes as fit
RANK_CAP = 2048           # events per document ranked on the GPU (score.hip kRankCap)


def hot_stride() -> int:
    from operator_amd.ops import kernels

    return int(kernels().SCAN_HOT_STRIDE)


def lds_chain_states(stride: int | None = None) -> int:
    """States whose chain byte is staged in LDS: what the 160 KB leave after the class map (256 B)
    and the hot rows (256 bytes x stride entries x 2 B), in whole 16-byte vectors."""
    stride = hot_stride() if stride is None else stride
    return (SCAN_LDS - 256 - 256 * stride * 2) // 16 * 16


def stream_len(total: int, seg: int, grid_blocks: int) -> int:
    """Bytes per stream: ceil(total / (grid_blocks * 1024)), in whole 64-byte chunks, at least seg."""
    streams = grid_blocks * 1024
    length = -(-total // streams)
    length = -(-length // 64) * 64
    return max(length, seg)


def plan(docs, seg: int):
    """(total bytes, first segment of each document + the end): a document takes its bytes plus at
    least one NUL, in whole segments."""
    first = [0]
    for d in docs:
        first.append(first[-1] + (len(d) + seg) // seg)
    return first[-1] * seg, first


def packed(docs, seg: int) -> bytes:
    total, first = plan(docs, seg)
    buf = bytearray(total)
    for d, f in zip(docs, first):
        buf[f * seg:f * seg + len(d)] = d
    return bytes(buf)


def ref_scan(factors, docs):
    """Sorted (doc, factor, line, end_offset) of every occurrence of every factor in the lower-cased
    documents (the contract of MatchEngine.scan_cpu / scan_gpu)."""
    rows = []
    for di, d in enumerate(docs):
        low = d.lower()
        nls = [i for i, b in enumerate(low) if b == 10]
        for fi, f in enumerate(factors):
            i = low.find(f)
            while i >= 0:
                end = i + len(f) - 1
                rows.append((di, fi, bisect.bisect_left(nls, end), end))
                i = low.find(f, i + 1)
    rows.sort()
    return rows


def walk_census(table, cls_map, log2c: int, chain, text: bytes, H: int = HOT, chain_lds: int | None = None,
                stream_len: int = 0) -> dict:
    """Walk the uploaded DFA over the packed text as the kernel's exact re-walk does and count its
    cold steps (state >= H) by kind. Also checks every chain byte it follows against the table."""
    tab = np.ascontiguousarray(np.asarray(table)).view(np.uint16).reshape(-1).tolist()
    cls = list(bytes(np.asarray(cls_map, dtype=np.uint8).tobytes()) if not isinstance(cls_map, bytes) else cls_map)
    ch = list(bytes(np.asarray(chain, dtype=np.uint8).tobytes()) if not isinstance(chain, bytes) else chain)
    lds = lds_chain_states() if chain_lds is None else chain_lds
    n = dict(cold_steps=0, via_chain=0, via_table=0, beyond_lds=0, cold_chunk_starts=0, cold_stream_starts=0,
             cold_outputs=0)
    s = 0
    for i, b in enumerate(text):
        cold = s >= H
        if cold and not i & 63:
            n["cold_chunk_starts"] += 1
            if stream_len and i % stream_len == 0:
                n["cold_stream_starts"] += 1   # the 64-byte look-back alone brought the walk here
        c = cls[b]
        e = tab[(s << log2c) | c]
        if cold:
            n["cold_steps"] += 1
            x = ch[s]
            if x & 0x40 and (x & 0x3F) == c:
                n["via_chain"] += 1
                assert e == (s + 1) | ((x & 0x80) << 8), f"chain byte of state {s} disagrees with the table"
            else:
                n["via_table"] += 1
            n["beyond_lds"] += s >= lds
            n["cold_outputs"] += e >> 15
        s = e & 0x7FFF
    return n


# ------------------------------------------------------------------------------------------ cases
@dataclass
class ScanCase:
    name: str
    factors: list
    docs: list
    seg: int
    grid_blocks: int = 1
    profile_bytes: int = 1 << 20          # of the profiled run (every case also runs with 0: breadth-first)
    want: dict = field(default_factory=dict)   # what the case is for: checked by check_split / check_census

    @functools.cached_property
    def patset(self) -> PatternSet:
        return PatternSet.from_dicts([{"id": f"f{i}", "primary_pattern": {"literal": f}}
                                      for i, f in enumerate(self.factors)])

    @functools.cached_property
    def cp(self):
        from operator_amd.patterns.compiler import compile_patterns

        cp = compile_patterns(self.patset)
        assert cp.factors == self.factors
        return cp

    @functools.cached_property
    def layout(self):
        return plan(self.docs, self.seg)

    @property
    def total(self) -> int:
        return self.layout[0]

    @property
    def L(self) -> int:
        return stream_len(self.total, self.seg, self.grid_blocks)

    @functools.cached_property
    def text(self) -> bytes:
        return packed(self.docs, self.seg)

    @functools.cached_property
    def rows(self):
        return ref_scan(self.factors, self.docs)

    @functools.cached_property
    def newlines(self):
        return [d.count(b"\n") for d in self.docs]

    def tables(self, profile_bytes: int) -> dict:
        """The DFA as MatchEngine uploads it: breadth-first, or renumbered by the visits of the first
        `profile_bytes` of the packed text; with its chain bytes."""
        from operator_amd.ops import patterns

        d = self.cp.dfa
        S, l2c = int(d["num_states"]), int(d["log2_classes"])
        table = d["table"]
        if profile_bytes > 0:
            table = patterns().reorder_dfa(table, d["out_off"], d["out_ids"], l2c, S, d["cls_map"],
                                           self.text[:profile_bytes], min(S, HOT))["table"]
        return dict(table=np.frombuffer(table, np.uint16), cls_map=d["cls_map"], log2c=l2c, states=S,
                    chain=patterns().dfa_chain(table, l2c, S), H=min(S, HOT))

    def census(self, t: dict) -> dict:
        return walk_census(t["table"], t["cls_map"], t["log2c"], t["chain"], self.text, t["H"], lds_chain_states(),
                           self.L)


def _words(rng, alphabet: bytes, n: int, lo: int = 2, hi: int = 9):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def _lines(rng, words, n: int, specials=()):
    out = []
    for _ in range(n):
        k = rng.choice([0, 1, 2, 4, 7, 12])
        ws = [rng.choice(words) for _ in range(k)]
        if specials and rng.random() < 0.3:
            ws.insert(rng.randint(0, len(ws)), rng.choice(specials))
        out.append(b" ".join(ws) + b"\n")
    return out


def _fill(rng, pool, n: int) -> bytes:
    out, have = [], 0
    while have < n:
        ln = rng.choice(pool)
        out.append(ln)
        have += len(ln)
    return b"".join(out)[:n]


def _doc_lengths(rng, n_segs: int, seg: int, sizes):
    """Document lengths that pack into exactly n_segs segments: empty documents, documents that
    leave a single NUL of padding, and everything between."""
    lens = []
    while n_segs > 0:
        k = min(rng.choice(sizes), n_segs)
        r = rng.random()
        lens.append((k - 1) * seg if r < 0.1 else k * seg - 1 if r < 0.25 else rng.randint((k - 1) * seg, k * seg - 1))
        n_segs -= k
    return lens


def _cut(text: bytearray, lens, seg: int):
    docs, f = [], 0
    for n in lens:
        docs.append(bytes(text[f * seg:f * seg + n]))
        f += (n + seg) // seg
    return docs


class _Canvas:
    """The packed text of a batch while it is being written: a write lands only where it lies
    inside ONE document's bytes (never in the padding, never across two documents)."""

    def __init__(self, lens, seg: int):
        self.lens, self.seg = lens, seg
        self.start = []
        f = 0
        for n in lens:
            self.start.append(f * seg)
            f += (n + seg) // seg
        self.buf = bytearray(f * seg)

    def put(self, pos: int, data: bytes) -> bool:
        if pos < 0:
            return False
        d = bisect.bisect_right(self.start, pos) - 1
        if pos + len(data) > self.start[d] + self.lens[d]:
            return False
        self.buf[pos:pos + len(data)] = data
        return True

    def put_end(self, end: int, data: bytes) -> bool:
        """data with its LAST byte at `end`."""
        return self.put(end - len(data) + 1, data)

    def docs(self):
        return _cut(self.buf, self.lens, self.seg)


SPLIT_FACTORS = [b"error", b"rror", b"oom", b"timeout", b"fail", b"xy"]
SPLIT_GEOMETRY = (           # (seg, L, grid_blocks, segments)
    (128, 192, 1, 1536),     # 1024 full streams of 1.5 segments
    (128, 320, 1, 2560),
    (256, 320, 1, 1280),
    (1024, 1088, 1, 1088),
    (128, 192, 1, 1499),     # 999 1/3 streams: a 64-byte last stream, 24 idle lanes
    (128, 192, 2, 2345),     # 1563 1/3 streams: the second block 540 of 1024 lanes
)


def split_case(seg: int, L: int, grid_blocks: int, n_segs: int, seed: int = 0) -> ScanCase:
    """Streams that start inside a segment, inside documents, with newlines and match ends on
    both sides of every such start."""
    rng = random.Random(1000 * seed + n_segs + seg)
    total = n_segs * seg
    words = _words(rng, b"abcdefghilmnorstuxy", 60) + [b"ERROR", b"Timeout", b"oom", b"xyxy", b"failfail"]
    pool = _lines(rng, words, 150, specials=SPLIT_FACTORS) + [b"errorerrorERRORerror xyxyxyxy oomoom\n", b"\n", b"\n\n"]
    lens = _doc_lengths(rng, n_segs, seg, [1, 1, 2, 3, 5, 8, 13, 21, 34])
    cv = _Canvas(lens, seg)
    for st, n in zip(cv.start, lens):
        cv.buf[st:st + n] = _fill(rng, pool, n)
    fs = [f if i % 3 else f.upper() for i, f in enumerate(SPLIT_FACTORS)]
    for k in range(1, -(-total // L)):
        p, f = k * L, fs[k % len(fs)]
        kind = k % 7                      # 7 kinds: every kind meets every alignment of a start in its segment
        if kind == 0:
            cv.put(p - 1, b"\n")
        elif kind == 1:
            cv.put(p, b"\n")
        elif kind == 2:
            cv.put_end(p, f)              # ends on the stream's first byte: all but one byte in the look-back
        elif kind == 3:
            cv.put_end(p - 1, f)          # ends one byte before it: the previous stream's match
        elif kind == 4:
            cv.put(p - 1, b"\n" + f)
        elif kind == 5:
            cv.put_end(p + 1, f + b"\n")
        elif kind == 6:
            cv.put(p - 9, b"\nerrorERRORerror xyxy\n")
    c = ScanCase(f"split-seg{seg}-L{L}-g{grid_blocks}-n{n_segs}", list(SPLIT_FACTORS), cv.docs(), seg, grid_blocks,
                 want=dict(split=True, L=L))
    assert c.total == total
    return c


@functools.cache
def split_cases():
    return tuple(split_case(*g) for g in SPLIT_GEOMETRY)


def split_points(total: int, seg: int, L: int) -> dict:
    """{segment: first byte of the stream that starts inside it}."""
    return {p // seg: p for p in range(L, total, L) if p % seg}


def seg_heads(case: ScanCase):
    """Per segment, the newlines of its part before the stream start inside it (0 where no stream
    starts inside): what the kernel leaves in the head half of seg_nl."""
    heads = [0] * (case.total // case.seg)
    for g, p in split_points(case.total, case.seg, case.L).items():
        heads[g] = case.text.count(b"\n", g * case.seg, p)
    return heads


def split_census(case: ScanCase, heads=None) -> dict:
    """What a split case holds, from the reference rows: `mid_rows` are the matches found after a
    mid-segment stream start whose segment head has newlines (their line number needs seg_head)."""
    seg, L, total = case.seg, case.L, case.total
    _, first = case.layout
    heads = seg_heads(case) if heads is None else heads
    cut = split_points(total, seg, L)
    n = dict(mid_rows=0, end_on_first=0, end_before_first=0, nl_before_start=0, nl_on_start=0,
             starts_in_doc=0, doc_ends_in_stream=0, max_line_matches=0,
             short_last=int(total % L != 0), idle_lanes=case.grid_blocks * 1024 - -(-total // L))
    per_line: dict = {}
    for d, _, line, off in case.rows:
        p = first[d] * seg + off
        g = p // seg
        if g in cut and p >= cut[g] and heads[g]:
            n["mid_rows"] += 1
        n["end_on_first"] += p % L == 0 and p > 0 and p % seg != 0
        n["end_before_first"] += p % L == L - 1 and (p + 1) % seg != 0
        per_line[d, line] = per_line.get((d, line), 0) + 1
    n["max_line_matches"] = max(per_line.values(), default=0)
    ends = [first[i] * seg + len(d) for i, d in enumerate(case.docs)]
    for p in cut.values():
        n["nl_before_start"] += case.text[p - 1] == 10
        n["nl_on_start"] += case.text[p] == 10
        i = bisect.bisect_right(first, p // seg) - 1
        n["starts_in_doc"] += first[i] * seg < p < ends[i]
    n["doc_ends_in_stream"] = sum(1 for e in ends if e % L)
    return n


def check_split(case: ScanCase, heads=None) -> dict:
    assert case.L == case.want["L"] == stream_len(case.total, case.seg, case.grid_blocks)
    assert case.L % case.seg != 0, "streams start on segment boundaries only"
    n = split_census(case, heads)
    for k in ("mid_rows", "end_on_first", "end_before_first", "nl_before_start", "nl_on_start", "starts_in_doc",
              "doc_ends_in_stream"):
        assert n[k] > 0, (case.name, k, n)
    assert n["max_line_matches"] >= 8, (case.name, n)
    return n


LIT_ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789-_./:"      # 41 classes + "other": log2_classes 6


def _lit(rng, n: int, alphabet: bytes = LIT_ALPHABET) -> bytes:
    return bytes(rng.choice(alphabet) for _ in range(n))


def cold_literals(seed: int = 0, scale: int = 1):
    """(sweep, extra): `sweep` are the long literals whose end is placed on every byte of a chunk;
    `extra` their suffixes (several outputs on one cold state) and more 64-byte literals.
    `scale` > 1 divides every length (the liveness check of the census preconditions)."""
    rng = random.Random(77 + seed)
    n = lambda x: max(2, x // scale)   # noqa: E731
    a64, a63, a33, a17, a16 = (_lit(rng, n(k)) for k in (64, 63, 33, 17, 16))
    b64 = a64[:n(40)] + _lit(rng, n(64) - n(40))      # shares 40 bytes with a64, then diverges in cold territory
    c64 = a64[:n(56)] + _lit(rng, n(64) - n(56))
    b33 = a33[:n(20)] + _lit(rng, n(33) - n(20))
    sweep = [a64, a63, a33, a17, a16, b64, c64, b33]
    extra = [a64[-n(16):], a64[-n(17):], a64[-n(33):], a63[-n(16):]] + [_lit(rng, n(64)) for _ in range(6)]
    assert len(set(sweep + extra)) == len(sweep + extra)
    return sweep, extra


def cold_case(seg: int, seed: int = 0, scale: int = 1) -> ScanCase:
    """One long document (global offset == document offset) of 192-byte streams, then three short
    ones. First part: every sweep literal ending on every offset 0..63 of a chunk, every fourth in
    upper case. Second part, per stream seam in turn: a 64-byte literal ending on the stream's
    first byte, on its byte 63, one byte before its start; a near miss (40 bytes of a literal) over
    the seam; literals back to back over the seam."""
    rng = random.Random(5 + seed)
    sweep, extra = cold_literals(seed, scale)
    a64, a16, a17 = sweep[0], sweep[4], sweep[3]
    words = _words(rng, LIT_ALPHABET[:26], 80)
    pool = _lines(rng, words, 120) + [b"\n"]
    n0 = 170000 - (170000 % seg) - 1                # one NUL of padding
    lens = [n0, len(a64), 0, len(sweep[1]) + 1 + len(a16)]
    cv = _Canvas(lens, seg)
    cv.buf[0:n0] = _fill(rng, pool, n0)
    cv.buf[cv.start[1]:cv.start[1] + lens[1]] = a64                       # a document that IS the literal
    cv.buf[cv.start[3]:cv.start[3] + lens[3]] = sweep[1] + b"\n" + a16
    L = stream_len(len(cv.buf), seg, 1)
    assert L == 192
    slot = 0
    for li, lit in enumerate(sweep):
        for r in range(64):
            assert cv.put_end(slot * 192 + 128 + r, lit.upper() if (li + r) % 4 == 0 else lit)
            slot += 1
    k = -(-slot * 192 // L) + 1
    more = extra[4:]
    while (k + 1) * L < n0:
        p, kind, j = k * L, k % 9, k // 9          # 9 kinds: each meets aligned and mid-segment starts
        if kind == 0:
            cv.put_end(p, a64)                     # all but its last byte in the look-back
        elif kind == 1:
            cv.put_end(p + 63, a64)
        elif kind == 2:
            cv.put_end(p - 1, a64)
        elif kind == 3:                            # near misses: 40 bytes of a literal, over the seam
            cv.put_end(p + 20, (a64 if j % 2 else more[j % len(more)])[:max(2, 40 // scale)] + b"#")
        elif kind == 4:
            cv.put_end(p + 40, a64 + a64 + a16 + a17 + a16 + a16)
        elif kind == 5:
            cv.put_end(p, sweep[j % len(sweep)])
        elif kind == 6:
            cv.put_end(p + 5, sweep[5] + sweep[6])
        elif kind == 7:                            # the rarely seen literals: cold under the profiled numbering
            cv.put_end(p, more[j % len(more)])
        elif kind == 8:
            cv.put_end(p + 63, more[j % len(more)] + more[(j + 1) % len(more)])
        k += 1
    return ScanCase(f"cold-seg{seg}" + (f"-scale{scale}" if scale > 1 else ""), sweep + extra, cv.docs(), seg, 1,
                    want=dict(states_above=HOT, sweep=len(sweep), census_profiled=("via_chain",),
                              census=("cold_steps", "via_table", "cold_chunk_starts", "cold_stream_starts",
                                      "cold_outputs")))


@functools.cache
def cold_cases():
    return (cold_case(64), cold_case(128))   # seg 128: 192-byte streams start inside segments as well


def sweep_census(case: ScanCase) -> dict:
    """Per sweep literal, the chunk offsets (0..63) on which an occurrence ends; and the 64-byte
    matches that end on a stream's first byte / its byte 63."""
    _, first = case.layout
    ends = {fi: set() for fi in range(case.want["sweep"])}
    on_first = on_63 = 0
    for d, fi, _, off in case.rows:
        p = first[d] * case.seg + off
        if fi in ends:
            ends[fi].add(p % 64)
        if len(case.factors[fi]) == 64:
            on_first += p % case.L == 0 and p > 0
            on_63 += p % case.L == 63
    return dict(ends=ends, on_first=on_first, on_63=on_63)


def check_census(case: ScanCase, tables: dict, profiled: bool) -> dict:
    """The census preconditions of a cold / class / big-DFA case on the given tables."""
    w = case.want
    assert tables["log2c"] == w.get("log2c", tables["log2c"]), (case.name, tables["log2c"])
    if "states_above" in w:
        assert tables["states"] > w["states_above"], (case.name, tables["states"])
    assert tables["states"] <= 32768
    n = case.census(tables)
    for k in w.get("census", ()) + (w.get("census_profiled", ()) if profiled else w.get("census_bfs", ())):
        assert n[k] > 0, (case.name, "profiled" if profiled else "bfs", k, n)
    for k in w.get("census_zero", ()):
        assert n[k] == 0, (case.name, k, n)
    if "sweep" in w:
        s = sweep_census(case)
        for fi, e in s["ends"].items():
            assert e == set(range(64)), (case.name, fi, sorted(set(range(64)) - e))
        assert s["on_first"] > 0 and s["on_63"] > 0, (case.name, s["on_first"], s["on_63"])
    return n


def _class_alphabet(n: int) -> bytes:
    """n distinct bytes, no NUL, newline or upper case; bytes >= 0x80 first."""
    pool = list(range(0x80, 0x100)) + [b for b in range(0x7E, 0x20, -1) if not 65 <= b <= 90] + [0x7F, 0x20, 9] + \
        list(range(1, 9)) + list(range(11, 32))
    return bytes(pool[:n])


def class_case(log2c: int, n_bytes: int, seed: int = 0, lit_len=(12, 40), n_lits: int = 30) -> ScanCase:
    rng = random.Random(31 * log2c + seed)
    alpha = b"abcde"[:n_bytes] if n_bytes <= 5 else _class_alphabet(n_bytes)
    lits = []
    while len(lits) < n_lits:
        f = _lit(rng, rng.randint(*lit_len), alpha)
        if f not in lits:
            lits.append(f)
    lits[0] = (bytes(alpha) * 64)[:64] if n_bytes <= 64 else bytes(alpha[:64])
    lits[1] = bytes(alpha[-64:]) if n_bytes > 64 else lits[1]
    if n_bytes > 128:
        lits[2], lits[3] = bytes(alpha[64:128]), bytes(alpha[100:164])
    assert len(set(lits)) == len(lits)
    seg = 64
    noise = bytes(alpha) + (b"" if n_bytes <= 5 else b" \t~") + b"\n"
    n0 = 60000 - 1
    body = bytearray(rng.choice(noise) for _ in range(n0))
    for i in range(0, n0 - 200, 150):
        f = rng.choice(lits)
        at = i + rng.randint(0, 80)
        body[at:at + len(f)] = f.upper() if i % 600 == 0 else f
    docs = [bytes(body), b"", lits[0], lits[-1] + b"\n" + lits[0][:-1]]
    used = len({b for f in lits for b in f.lower()}) + 1
    assert (1 << (log2c - 1) if log2c > 3 else 0) < used <= 1 << log2c
    return ScanCase(f"classes{log2c}", lits, docs, seg, 1,
                    want=dict(log2c=log2c, states_above=HOT, census=("cold_steps", "via_table", "cold_chunk_starts"),
                              # above 64 classes dfa_chain is all zeros: every cold step reads the table
                              **({"census_zero": ("via_chain",)} if log2c > 6 else
                                 {"census_profiled": ("via_chain",)})))


@functools.cache
def class_cases():
    return (class_case(3, 5), class_case(6, 40), class_case(7, 100), class_case(8, 200))


BIG_PROFILE = 64 * 1024


@functools.cache
def big_dfa_case(n_lits: int = 515, seed: int = 0) -> ScanCase:
    """More states than chain bytes fit in LDS. The profiled numbering puts the visited literals'
    states first, so the states past `chain_lds` belong to literals the profile sample (the first
    64 KB) does NOT hold: the text after it holds those, picked by walking each literal through the
    renumbered table."""
    from operator_amd.ops import patterns
    from operator_amd.patterns.compiler import compile_patterns

    rng = random.Random(909 + seed)
    lits = []
    while len(lits) < n_lits:
        f = _lit(rng, 64)
        if f not in lits:
            lits.append(f)
    seg = 64
    words = _words(rng, LIT_ALPHABET[:26], 80)
    pool = _lines(rng, words, 120) + [b"\n"]
    lens = [rng.randint(9000, 30000) for _ in range(11)]
    lens[3] = 0
    cv = _Canvas(lens, seg)
    for st, n in zip(cv.start, lens):
        cv.buf[st:st + n] = _fill(rng, pool, n)

    def place(lo: int, hi: int, which):
        slots = list(range(lo, hi - 1024, 1024))
        rng.shuffle(slots)
        done = 0
        for f in which:
            while slots and not cv.put(slots.pop() + rng.randint(0, 900), f):
                pass
            done += 1
        return done

    place(0, BIG_PROFILE, lits[:50])
    case = ScanCase("big-dfa", lits, cv.docs(), seg, 1, profile_bytes=BIG_PROFILE)
    d = compile_patterns(case.patset).dfa
    S, l2c = int(d["num_states"]), int(d["log2_classes"])
    t = np.frombuffer(patterns().reorder_dfa(d["table"], d["out_off"], d["out_ids"], l2c, S, d["cls_map"],
                                             bytes(cv.buf[:BIG_PROFILE]), HOT)["table"], np.uint16).reshape(S, -1)
    cls, lds = d["cls_map"], lds_chain_states()

    def beyond(f):
        s = n = 0
        for b in f:
            s = int(t[s, cls[b]]) & 0x7FFF
            n += s >= lds
        return n

    rest = sorted(range(50, n_lits), key=lambda i: -beyond(lits[i]))
    late = [lits[i] for i in rest[:30]] + [lits[i] for i in rng.sample(rest[30:], 20)] if len(rest) >= 50 else \
        [lits[i] for i in rest]
    place(BIG_PROFILE + 1024, len(cv.buf), late)
    return ScanCase("big-dfa" if n_lits == 515 else f"big-dfa-{n_lits}", lits, cv.docs(), seg, 1,
                    profile_bytes=BIG_PROFILE,
                    want=dict(log2c=6, states_above=lds_chain_states() + 256,
                              census=("cold_steps", "via_table", "beyond_lds", "cold_chunk_starts"),
                              census_profiled=("via_chain",)))


def scan_path_cases():
    """Every case whose path is a property of the DFA walk (census-checked)."""
    return cold_cases() + class_cases() + (big_dfa_case(),)


# ------------------------------------------------------------------------------------------ scorer
@dataclass
class ScoreCase:
    patset: PatternSet
    docs: list          # per document: sorted unique (matcher, line); matcher ids of the compiled set
    n_sec: int          # most secondaries of any pattern


def _pat(pid, lit, conf, sev="MEDIUM", sec=()):
    return {"id": pid, "severity": sev, "primary_pattern": {"literal": lit, "confidence": conf},
            "secondary_patterns": [{"literal": s, "weight": w, "proximity_window": win} for s, w, win in sec]}


RANK_COUNTS = (0, 1, 2, 3, 255, 256, 257, 2047, 2048)


@functools.cache
def score_exact_case() -> ScoreCase:
    """Dyadic confidences and weights, every window + 1 a power of two: the numerator and the
    denominator of every score are exact in fp64, so the score is ONE correctly rounded division
    and any right implementation gives the same bits. Matcher ids (compile order):
    0 p-a, 1 s-near (window 7), 2 s-far (window 3), 3 p-b, 4 p-c, 5 s-gone (in no document)."""
    ps = PatternSet.from_dicts([
        _pat("a-high", "p-a", 0.5, "HIGH", [("s-near", 0.5, 7), ("s-far", 0.25, 3)]),
        _pat("a-crit", "p-a", 0.5, "CRITICAL", [("s-near", 0.5, 7), ("s-far", 0.25, 3)]),   # ties a-high: severity
        _pat("a-crit-2", "p-a", 0.5, "CRITICAL", [("s-near", 0.5, 7), ("s-far", 0.25, 3)]),  # ties a-crit: pattern
        _pat("b-plain", "p-b", 0.5, "LOW"),                          # score == significance exactly; ties by line
        _pat("c-gone", "p-c", 0.625, "INFO", [("s-gone", 0.5, 0)]),  # its secondary matches nowhere: 0.625 / 1.5
        _pat("c-zero", "p-c", 0.875, "MEDIUM", [("s-near", 1.0, 0)]),  # window 0: only a hit on the same line counts
    ])
    A, NEAR, FAR, B, C = 0, 1, 2, 3, 4
    docs = []
    # window edges of s-near (7) and s-far (3) around p-a on line 100: dist 0, win, win + 1, and a
    # nearest hit equally far on both sides; p-c with s-near on its line and one line off
    docs.append([(A, 100), (NEAR, 100), (FAR, 97), (FAR, 103),
                 (A, 200), (NEAR, 207), (FAR, 204),
                 (A, 300), (NEAR, 308), (FAR, 296), (FAR, 304),
                 (A, 400), (NEAR, 393), (NEAR, 407),
                 (B, 5), (B, 6), (B, 700), (C, 100), (C, 208), (C, 500),
                 (6, 100), (11, 3)])                                 # matcher ids past the compiled set: ignored
    docs.append([])
    # event counts around the bitonic padding and at the rank cap: p-b on n lines, s-near here and
    # there (no event of its own); for n >= 255 p-a on the first n // 3 lines gives 3 events a line
    for n in RANK_COUNTS[1:]:
        if n < 255:
            docs.append([(B, 3 * i) for i in range(n)] + [(NEAR, 4)])
        else:
            k = n // 3
            docs.append([(A, 2 * i) for i in range(k)] + [(B, 2 * i + 1) for i in range(n - 3 * k)] +
                        [(NEAR, 16 * i) for i in range(k // 8)] + [(FAR, 50 * i + 1) for i in range(k // 25)])
    # one past the cap: the kernel returns after the summary, the engine ranks on the host
    docs.append([(A, 2 * i) for i in range(683)] + [(NEAR, 16 * i) for i in range(80)] + [(FAR, 7), (FAR, 1200)])
    return ScoreCase(ps, [sorted(set(d)) for d in docs], 2)


@functools.cache
def score_random_case(seed: int = 3) -> ScoreCase:
    """Non-dyadic inputs. Each primary matcher belongs to one pattern and hits one line per
    document at most, so no two events of a document are equal by construction; the seed is one
    for which they also differ by >= 1e-6 (asserted by check_score_gap)."""
    rng = random.Random(seed)
    n_pat, n_secm, n_sec = 24, 10, 4
    pats = []
    for p in range(n_pat):
        sec = [(f"sec-{m}", rng.uniform(0.05, 1.5), rng.choice([0, 1, 2, 4, 5, 9, 12, 20, 30]))
               for m in rng.sample(range(n_secm), rng.randint(0, n_sec))]
        if p == 0:
            sec = [(f"sec-{m}", rng.uniform(0.05, 1.5), 6 + m) for m in range(n_sec)]
        pats.append(_pat(f"r{p}", f"prim-{p}", rng.uniform(0.1, 1.0), rng.choice(["INFO", "LOW", "MEDIUM", "HIGH",
                                                                                 "CRITICAL"]), sec))
    ps = PatternSet.from_dicts(pats)
    from operator_amd.patterns.compiler import compile_patterns

    cp = compile_patterns(ps, build_dfa=False)
    secm = sorted({m for ms in cp.pattern_secondary for m in ms})
    docs = [[]]
    for _ in range(12):
        hits = {(cp.pattern_primary[p], rng.randint(0, 60)) for p in rng.sample(range(n_pat), rng.randint(1, 16))}
        hits |= {(rng.choice(secm), rng.randint(0, 60)) for _ in range(rng.randint(0, 40))}
        docs.append(sorted(hits))
    return ScoreCase(ps, docs, n_sec)


def exact_scores(cp, hits):
    """{(pattern, line): score} of one document by the formula in rational arithmetic: the value a
    correctly rounded fp64 evaluation must round to when numerator and denominator are exact."""
    by_m: dict = {}
    for m, l in hits:
        by_m.setdefault(m, []).append(l)
    out = {}
    for pi, p in enumerate(cp.patset.patterns):
        for line in by_m.get(cp.pattern_primary[pi], []):
            bonus = wsum = Fraction(0)
            for j, sm in enumerate(cp.pattern_secondary[pi]):
                w, win = Fraction(p.secondary[j].weight), p.secondary[j].window
                wsum += w
                d = min((abs(l - line) for l in by_m.get(sm, [])), default=None)
                if d is not None and d <= win:
                    bonus += w * (1 - Fraction(d, win + 1))
            out[pi, line] = Fraction(p.primary.confidence) * (1 + bonus) / (1 + wsum)
    return out


def check_score_gap(events, gap: float = 1e-6) -> float:
    """Smallest score difference of two events of one document (>= gap, asserted)."""
    s = sorted(e.score for e in events)
    g = min((b - a for a, b in zip(s, s[1:])), default=1.0)
    assert g >= gap, g
    return g


def score_bound(n_sec: int) -> float:
    """Relative distance allowed between two fp64 evaluations of the score formula: a division, a
    subtraction, a product and a sum per secondary, which a fused multiply-add evaluation rounds
    once less and in which the terms are all positive (2 n_sec roundings apart at most), plus the
    three of 1 + bonus, the product with the confidence and the final division."""
    return (2 * n_sec + 3) * float(np.finfo(np.float64).eps)
