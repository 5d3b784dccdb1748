"""Which kernel every bf16 GEMM runs on, and with which arguments, pinned without a GPU.

``ops.linear`` / ``ops.gate_up_silu`` are driven with storage-less tensors that claim to be on
the GPU, the ``kernels`` hook is replaced by a recorder, and every launch (kernel name, tensor
shapes, scalars), the kind of result, the hipBLASLt counters and any exception are compared with
``tests/golden/gemm_route/decisions.json``. That fixture is written by this file run as a script
on the commit whose behaviour is to be kept::

    python tests/test_gemm_route.py --write

The recorder uses only ``ops.linear``, ``ops.gate_up_silu``, the ``kernels`` hook, the
``PREFILL_BLAS`` flag and the table dict, so the same file runs on either side of a change to
the routing code.
"""
from __future__ import annotations

import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from operator_amd import ops  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_route", "decisions.json")

MS = (1, 2, 8, 16, 17, 32, 33, 40, 64, 128, 192, 200, 256, 257, 512, 32768)
VARIANT_MS = (8, 64, 256, 512)
NKS = ((6144, 4096), (4096, 4096), (4096, 14336), (28672, 4096), (128256, 4096),    # Llama-3-8B
       (768, 4096), (4096, 512), (3584, 4096), (4096, 1792),                        # tabled TP shards
       (640, 2048), (256, 448), (128, 4096), (1024, 14336),                         # off the table
       (136, 4096), (256, 96), (40, 128))                                           # no kernel takes these
WGUS = ((28672, 4096), (1280, 1024), (256, 448))
BLOCKS = (64, 32, None)

# every spelling of a table value, on shapes of the grid (laid over the shipped table)
SYNTHETIC = {
    (64, 640, 2048): [64, 64, 2],
    (256, 256, 448): [128, 128, 5, 4],
    (256, 640, 2048): [256, 128, 3, 4, "w4"],
    (128, 640, 2048): [128, 128, 2, 3, "w4"],          # gemm_w4 on 128 rows: raises
    (256, 1024, 14336): [128, 128, 4, 3, "w4"],        # gemm_w4 as 128 x 128 tiles: raises
    (64, 1024, 14336): "tile",
    (128, 1024, 14336): "blas",
    (512, 640, 2048): "blas",                          # read although no decode plan has 512 rows
    (64, 128256, 4096): "blas",                        # the lm_head never takes "blas"
    ("skinny", 8, 128256, 4096): "blas",
    ("skinny", 8, 640, 2048): "blas",
    ("skinny", 8, 28672, 4096): "blas",
    ("skinny", 16, 640, 2048): "tile",
    ("skinny", 8, 1024, 14336): 4,
    ("skinny", 2, 128, 4096): 8,
    ("silu", 256, 1280, 1024): "w4",
    ("silu", 128, 1280, 1024): "pp128",
    ("silu", 256, 256, 448): "pp256",
    ("silu", 128, 256, 448): [128, 4],
    ("silu", 64, 256, 448): [64],
    ("silu", 192, 1280, 1024): "blas",
    ("silu", 8, 1280, 1024): "blas",
    ("silu", 16, 1280, 1024): "w4",
    ("silu", 32, 256, 448): [0],
    ("silu", 128, 28672, 4096): "w4",                  # gemm_w4 on 128 rows: raises
}


class FakeGpu(torch.Tensor):
    """A meta tensor (shape, strides and dtype, no storage) that says it is on the GPU."""

    @property
    def is_cuda(self):
        return True

    def data_ptr(self):
        return 0


def fake(*shape, dtype=torch.bfloat16):
    return torch.empty(*shape, dtype=dtype, device="meta").as_subclass(FakeGpu)


class FakeAlloc(torch.overrides.TorchFunctionMode):
    """Buffers the code under test allocates on a fake GPU tensor's device are fake GPU tensors
    too, so the kernels that consume a GEMM's output (silu_mul after an unfused gate|up) are
    recorded as well."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        r = func(*args, **(kwargs or {}))
        if func is torch.empty and r.device.type == "meta":
            return r.as_subclass(FakeGpu)
        return r


def _desc(v):
    if isinstance(v, torch.Tensor):
        return list(v.shape)
    return v


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self):   # stands in for ops.kernels
        return self

    def __getattr__(self, name):
        def launch(*args, **kw):
            self.calls.append([name] + [_desc(a) for a in args] + [[k, _desc(v)] for k, v in sorted(kw.items())])
        return launch


def _modules():
    """The modules that hold the ``kernels`` hook and read ``PREFILL_BLAS``."""
    return [m for m in (ops, getattr(ops, "gemm", None)) if m is not None and hasattr(m, "kernels")]


def _table() -> dict:
    return (getattr(ops, "gemm_table", None) or ops._gemm_table_get)()


def _linear_variants(M, N, K):
    """name -> thunk, the non-default forms of ops.linear."""
    x, w = fake(M, K), fake(N, K)
    return {
        "out": lambda: ops.linear(x, w, out=fake(M, N)),
        "out_strided": lambda: ops.linear(x, w, out=fake(M, N + 8)[:, :N]),
        "out_unwritable": lambda: ops.linear(x, w, out=fake(M, N + 2)[:, :N]),
        "bias": lambda: ops.linear(x, w, bias=fake(N)),
        "bias_out_unwritable": lambda: ops.linear(x, w, bias=fake(N), out=fake(M, N + 2)[:, :N]),
        "splits": lambda: ops.linear(x, w, splits=2),
        "explicit": lambda: ops.linear(x, w, splits=2, bn=128, bm=64, stages=2),
        "explicit_defer": lambda: ops.linear(x, w, splits=2, bn=128, bm=64, stages=2, defer_reduce=True),
        "stages": lambda: ops.linear(x, w, stages=2),
        "partial_small": lambda: ops.linear(x, w, partial=fake(M * N, dtype=torch.float32), defer_reduce=True),
        "partial_large": lambda: ops.linear(x, w, partial=fake(16 * M * N, dtype=torch.float32), defer_reduce=True),
        "fp16": lambda: ops.linear(fake(M, K, dtype=torch.float16), fake(N, K, dtype=torch.float16)),
        "x_strided": lambda: ops.linear(fake(M, 2 * K)[:, :K], w),
        "w_strided": lambda: ops.linear(x, fake(N, 2 * K)[:, :K]),
        "prefill_blas": lambda: ops.linear(x, w),
    }


def _cases():
    """(key, thunk, PREFILL_BLAS) for the whole grid."""
    for M in MS:
        for N, K in NKS:
            x, w = fake(M, K), fake(N, K)
            yield f"linear,{M},{N},{K}", (lambda x=x, w=w: ops.linear(x, w)), False
            yield f"linear,{M},{N},{K},defer", (lambda x=x, w=w: ops.linear(x, w, defer_reduce=True)), False
            if M in VARIANT_MS:
                for name, fn in _linear_variants(M, N, K).items():
                    yield f"linear,{M},{N},{K},{name}", fn, name == "prefill_blas"
        for N, K in WGUS:
            for block in BLOCKS:
                x, w = fake(M, K), fake(N, K)
                yield f"silu,{M},{N},{K},{block}", (lambda x=x, w=w, b=block: ops.gate_up_silu(x, w, b)), False


def record(synthetic: bool) -> dict:
    """key -> [launches, result, BLAS_CALLS delta, BLAS_PLANNED delta]."""
    rec, mods, tab = Recorder(), _modules(), _table()
    saved = [(m, m.kernels, m.PREFILL_BLAS) for m in mods]
    saved_tab, saved_env = dict(tab), os.environ.pop("OAMD_FORBID_BLAS", None)
    log = {}
    try:
        for m in mods:
            m.kernels = rec
        if synthetic:
            tab.update(SYNTHETIC)
        for key, fn, prefill_blas in _cases():
            for m in mods:
                m.PREFILL_BLAS = prefill_blas
            rec.calls = []
            n0, p0 = ops.BLAS_CALLS["n"], ops.BLAS_PLANNED["n"]
            try:
                with FakeAlloc():
                    r = fn()
                res = ["S", r.S, *r.shape] if isinstance(r, ops.SplitK) else ["T", *r.shape]
            except Exception as e:   # the routing code's own refusals are part of its behaviour
                res = ["E", type(e).__name__, str(e)]
            log[key] = [rec.calls, res, ops.BLAS_CALLS["n"] - n0, ops.BLAS_PLANNED["n"] - p0]
    finally:
        for m, k, pb in saved:
            m.kernels, m.PREFILL_BLAS = k, pb
        tab.clear()
        tab.update(saved_tab)
        if saved_env is not None:
            os.environ["OAMD_FORBID_BLAS"] = saved_env
    return log


def _pack(logs: dict) -> dict:
    """Entries stored once, cases as indices into them."""
    entries, index, cases = [], {}, {}
    for table, log in logs.items():
        cases[table] = {}
        for key, entry in log.items():
            s = json.dumps(entry)
            if s not in index:
                index[s] = len(entries)
                entries.append(entry)
            cases[table][key] = index[s]
    return {"entries": entries, "cases": cases}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("table", ["shipped", "synthetic"])
def test_same_launches_as_recorded(golden, table):
    """Every case of the grid launches the recorded kernels with the recorded arguments, returns
    the recorded kind of result, moves the hipBLASLt counters as recorded and raises what was
    recorded."""
    got = json.loads(json.dumps(record(table == "synthetic")))
    want = {k: golden["entries"][i] for k, i in golden["cases"][table].items()}
    assert got.keys() == want.keys()
    diff = [(k, want[k], got[k]) for k in want if got[k] != want[k]]
    assert not diff, f"{len(diff)} of {len(want)} cases differ, first: {diff[:3]}"


def test_fixture_reaches_every_kernel_and_refusal(golden):
    """The grid is worth its name: every back end, both result kinds, both counters and both
    gemm_w4 refusals are in the fixture."""
    entries = golden["entries"]
    kernels = {c[0] for e in entries for c in e[0]}
    assert {"gemm_skinny", "gemm_decode", "gemm_pp", "gemm_w4", "gemm_tile", "silu_mul"} <= kernels
    assert {e[1][0] for e in entries} == {"T", "S", "E"}
    assert any(e[2] for e in entries) and any(e[3] for e in entries)
    msgs = {e[1][2] for e in entries if e[1][0] == "E"}
    assert any("gemm_w4 runs M = 256 as 256 x 128 tiles only" in m for m in msgs)
    assert any("gemm_w4 takes the 256-row bucket only" in m for m in msgs)


def test_route_is_callable_from_plain_values(monkeypatch):
    """The routing function needs no tensor: the quirks of its order of precedence, from shapes,
    flags and table entries alone."""
    from operator_amd.ops.gemm import BLAS, TILE, Plan, route

    tab = ops.gemm_table()
    # the shipped table: tuned decode plan, skinny split count, lm_head on the tile kernel
    assert route(256, 6144, 4096) == Plan(256, 128, 5, 3, "decode")
    assert route(256, 6144, 4096)[:3] == (256, 128, 5)
    assert route(1, 4096, 4096) == Plan(splits=2, kernel="skinny")
    assert route(64, 128256, 4096) == TILE
    assert route(256, 28672, 4096, silu=True, block=64) == Plan(kernel="w4")
    assert route(128, 28672, 4096, silu=True, block=64) == Plan(128, 128, kernel="pp")
    assert route(128, 28672, 4096, silu=True, block=32) is None        # unfused: GEMM, then silu_mul
    assert route(192, 1280, 1024, silu=True, block=64) == Plan(64, 128, 1, 3, "decode")
    # a "blas" entry is a FALLBACK, unless tile / split arguments are explicit or N is a vocabulary
    monkeypatch.setitem(tab, (128, 640, 2048), "blas")
    assert route(128, 640, 2048) == BLAS and not BLAS.planned
    assert route(128, 640, 2048, splits=2) == Plan(128, 64, 2, 3, "decode")
    monkeypatch.setitem(tab, (64, 128256, 4096), "blas")
    assert route(64, 128256, 4096) == TILE
    # PREFILL_BLAS plans hipBLASLt past 256 rows only, and not for the lm_head
    assert route(512, 4096, 4096, prefill_blas=True) == Plan(kernel="blas", planned=True)
    assert route(256, 4096, 4096, prefill_blas=True).kernel == "decode"
    assert route(512, 128256, 4096, prefill_blas=True) == TILE
    # a bias goes to the tile kernel or falls back, whatever the table says
    assert route(256, 6144, 4096, bias=True) == TILE
    assert route(256, 6144, 4096, bias=True, out_ok=False) == BLAS
    assert route(512, 4096, 4096, out_ok=False) == BLAS
    # a plan tagged "w4" runs on gemm_w4 only untouched; a tag gemm_w4 cannot honour raises at the call
    monkeypatch.setitem(tab, (256, 640, 2048), [256, 128, 3, 4, "w4"])
    assert route(256, 640, 2048) == Plan(256, 128, 3, 4, "w4")
    assert route(256, 640, 2048, stages=2) == Plan(256, 128, 3, 2, "decode")
    assert route(256, 640, 2048, bf16=False) == BLAS
    monkeypatch.setitem(tab, (128, 640, 2048), [128, 128, 2, 3, "w4"])
    with pytest.raises(ValueError, match="gemm table: plan .* gemm_w4 runs M = 256 as 256 x 128 tiles only"):
        route(128, 640, 2048)
    assert route(128, 640, 2048, contig=False) == BLAS      # the entry is not used: nothing raised
    # off-plan shapes: explicit arguments get (row_tile, 64, 1); nothing explicit, the tile kernel
    assert route(192, 256, 448, cuda=False) == BLAS
    assert route(40, 256, 448) == TILE and route(40, 256, 96) == BLAS
    assert route(8, 256, 448) == TILE                       # K % 128 != 0: not skinny
    assert route(8, 256, 448, splits=1) == Plan(splits=1, kernel="skinny")   # explicit splits are not second-guessed


def test_table_value_decoder(monkeypatch):
    from operator_amd.ops.gemm import BLAS, TILE, Plan, _decode

    assert _decode(None, (64, 640, 2048)) is None
    assert _decode([64, 64, 2], (64, 640, 2048)) == Plan(64, 64, 2, 3, "decode")
    assert _decode([128, 128, 5, 4], (256, 256, 448)) == Plan(128, 128, 5, 4, "decode")
    assert _decode([256, 128, 3, 4, "w4"], (256, 640, 2048)) == Plan(256, 128, 3, 4, "w4")
    assert _decode("tile", (64, 640, 2048)) == TILE and _decode("blas", (64, 640, 2048)) == BLAS
    assert _decode(4, ("skinny", 8, 640, 2048)) == Plan(splits=4, kernel="skinny")
    assert _decode("blas", ("skinny", 8, 640, 2048)) == BLAS
    assert _decode("w4", ("silu", 256, 1280, 1024)) == Plan(kernel="w4")
    assert _decode("pp256", ("silu", 256, 1280, 1024)) == Plan(256, 128, kernel="pp")
    assert _decode([128, 4], ("silu", 256, 1280, 1024)) == Plan(128, 128, 1, 4, "decode")
    assert _decode([64], ("silu", 64, 1280, 1024)) == Plan(64, 128, 1, 3, "decode")
    with pytest.raises(ValueError, match="plan 'w4' on silu,128,1280,1024: gemm_w4 takes the 256-row bucket only"):
        _decode("w4", ("silu", 128, 1280, 1024))
    # the shipped table decodes whole, and gemm_plan's first three elements stay (bm, bn, splits)
    for key, raw in ops.gemm_table().items():
        _decode(raw, key)
    assert ops.gemm_plan(256, 4096, 4096)[:3] == (128, 128, 4) and ops.gemm_plan(256, 4096, 4096).stages == 4


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gemm_route.py --write")
    packed = _pack({"shipped": record(False), "synthetic": record(True)})
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        json.dump(packed, f, separators=(",", ":"))
        f.write("\n")
    print(f"{FIXTURE}: {sum(len(c) for c in packed['cases'].values())} cases, {len(packed['entries'])} entries")
