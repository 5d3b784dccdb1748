"""Repetition / frequency / presence penalties on the CPU tier: the reference semantics
(ops/reference.py penalty_seed / sample_penalty, docs/PARITY.md "Sampling: penalties"), the
per-request table through the CPU engine (slots that follow the request across recompositions
and prefix sharing), and the parameters' way from the HTTP bodies, an AIProvider's
additionalConfig, the CLI and a GenRequest down to the engine, including the refusals on a
tensor-parallel replica and on an engine built without a table."""
import os
import socket
from collections import Counter

import httpx
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from operator_amd import ops
from operator_amd.models.penalty import PenaltyTable
from operator_amd.ops import reference as ref

F32 = torch.float32
V = 16


def _table(prompt, generated=(), slots=2, slot=1, cap=32):
    """A table whose slot ``slot`` was seeded with ``prompt`` and then counted ``generated``."""
    tb = PenaltyTable(slots, V, cap, device="cpu")
    ops.penalty_seed(tb, torch.tensor([slot], dtype=torch.int32), torch.tensor(prompt, dtype=torch.long),
                     torch.tensor([0, len(prompt)], dtype=torch.int32))
    x = torch.zeros(1, V)
    one = lambda v: torch.tensor([v], dtype=F32)   # noqa: E731
    for t in generated:
        ops.sample_penalty(x, torch.tensor([slot], dtype=torch.int32), torch.tensor([t]), None, one(1.0), one(0.0),
                           one(0.0), tb)
    assert not x.any()   # the off values: counting alone changes no logit
    return tb


def _apply(row, tb, r=1.0, f=0.0, p=0.0, slot=1, dtype=F32):
    x = torch.tensor([row], dtype=torch.float64).to(dtype)
    one = lambda v: torch.tensor([v], dtype=F32)   # noqa: E731
    out = ops.sample_penalty(x, torch.tensor([slot], dtype=torch.int32), None, None, one(r), one(f), one(p), tb)
    assert out is x
    return x[0]


ROW = [2.0, -2.0, 3.0, -3.0, 1.5, -1.5, 4.0, 0.0] + [1.0] * 8


def test_seed_flags_the_prompt_and_clears_the_previous_occupant():
    tb = _table([3, 3, 0, V - 1, V, V + 7, 5], generated=[5, 9, 9])
    assert int(tb.n[1]) == 5 and set(tb.lst[1, :5].tolist()) == {0, 3, 5, 9, V - 1}
    want = torch.zeros(V, dtype=torch.int32)
    want[[0, 3, V - 1]] = ref.PROMPT_BIT
    want[5] = ref.PROMPT_BIT + 1
    want[9] = 2
    assert torch.equal(tb.cnt[1], want) and not tb.cnt[0].any() and int(tb.n[0]) == 0
    ops.penalty_seed(tb, torch.tensor([1], dtype=torch.int32), torch.tensor([7, 7]), torch.tensor([0, 2], dtype=torch.int32))
    want = torch.zeros(V, dtype=torch.int32)
    want[7] = ref.PROMPT_BIT
    assert torch.equal(tb.cnt[1], want) and int(tb.n[1]) == 1 and tb.lst[1, 0] == 7


def test_repetition_divides_positive_and_multiplies_negative_logits():
    y = _apply(ROW, _table([0, 1]), r=2.0)
    assert y[0] == 1.0 and y[1] == -4.0                       # x > 0: x / r; x <= 0: x * r
    assert torch.equal(y[2:], torch.tensor(ROW[2:]))          # tokens not seen are not touched
    y = _apply(ROW, _table([0, 1, 7]), r=0.5)
    assert y[0] == 4.0 and y[1] == -1.0 and y[7] == 0.0


def test_the_prompt_counts_for_repetition_but_not_for_frequency_and_presence():
    tb = _table([0, 1], generated=[2, 3, 3])
    y = _apply(ROW, tb, f=0.5, p=0.25)
    assert y[0] == 2.0 and y[1] == -2.0                       # prompt only: c = 0
    assert y[2] == 3.0 - (0.5 * 1 + 0.25) and y[3] == -3.0 - (0.5 * 2 + 0.25)
    y = _apply(ROW, tb, r=2.0)
    assert y.tolist()[:4] == [1.0, -4.0, 1.5, -6.0]           # generated tokens are seen as well


def test_repetition_is_applied_before_frequency_and_presence():
    tb = _table([], generated=[4, 4, 5])
    y = _apply(ROW, tb, r=2.0, f=0.5, p=1.0)
    assert y[4] == 1.5 / 2.0 - (0.5 * 2 + 1.0) == -1.25       # not (1.5 - 2) * 2 = -1
    assert y[5] == -1.5 * 2.0 - (0.5 * 1 + 1.0) == -4.5
    y = _apply(ROW, tb, f=-1.0, p=-0.5)                       # negative penalties reward repeats
    assert y[4] == 1.5 + 2.5 and y[5] == -1.5 + 1.5


def test_off_values_and_rows_without_a_slot_leave_the_bytes_unchanged():
    tb = _table([0, 1, 7], generated=[2, 2])
    nan = float("nan")
    row = [nan, -0.0, 3.0, float("inf"), float("-inf")] + [0.1] * (V - 5)
    for dt in (F32, torch.bfloat16):
        x0 = torch.tensor([row], dtype=torch.float64).to(dt)[0]
        bits = lambda t: t.view(torch.int32 if dt == F32 else torch.int16)   # noqa: E731
        assert torch.equal(bits(_apply(row, tb, dtype=dt)), bits(x0))                              # r 1, f 0, p 0
        assert torch.equal(bits(_apply(row, tb, r=3.0, f=1.0, p=1.0, slot=-1, dtype=dt)), bits(x0))  # no slot
    y = _apply(row, tb, r=2.0, f=1.0)
    assert torch.isnan(y[0]) and y[1] == 0 and torch.signbit(y[1]) and y[3] == float("inf") and y[4] == float("-inf")


def test_each_operation_is_rounded_to_fp32_on_its_own():
    """x / r, f * c, (f * c) + p and y - pen, each fp32: values whose fused or double-precision
    evaluation differs in the last bit."""
    tb = _table([], generated=[0] * 3)
    x, r, f, p = 1.1, 1.3, 0.7, 1.1
    t = lambda v: torch.tensor(v, dtype=F32)   # noqa: E731
    want = t(x) / t(r) - (t(f) * t(3.0) + t(p))
    y = _apply([x] + [0.0] * (V - 1), tb, r=r, f=f, p=p)
    assert y[0].item() == want.item()
    yb = _apply([x] + [0.0] * (V - 1), tb, r=r, f=f, p=p, dtype=torch.bfloat16)
    xb = t(x).to(torch.bfloat16).float()
    assert yb[0].item() == (xb / t(r) - (t(f) * t(3.0) + t(p))).to(torch.bfloat16).item()


def test_count_ignores_padding_rows_and_a_full_list():
    tb = PenaltyTable(3, V, 2, device="cpu")
    ops.penalty_seed(tb, torch.tensor([0, 2], dtype=torch.int32), torch.tensor([1, 2, 1]),
                     torch.tensor([0, 2, 3], dtype=torch.int32))
    assert tb.n.tolist() == [2, 0, 1]
    x = torch.zeros(3, V)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    ones, zeros = torch.ones(3), torch.zeros(3)
    # row 0 -> slot 0, full: token 9 is dropped, token 1 would still count; row 1: ctx 0; row 2: no slot
    ops.sample_penalty(x, i32([0, 2, -1]), torch.tensor([9, 5, 5]), i32([4, 0, 4]), ones, zeros, zeros, tb)
    assert tb.n.tolist() == [2, 0, 1] and int(tb.cnt[0, 9]) == 0 and not tb.cnt[2, 5]
    ops.sample_penalty(x, i32([0, 2, -1]), torch.tensor([1, 5, 5]), i32([4, 3, 4]), ones, zeros, zeros, tb)
    assert int(tb.cnt[0, 1]) == ref.PROMPT_BIT + 1 and tb.n.tolist() == [2, 0, 2] and int(tb.cnt[2, 5]) == 1


# ---------------------------------------------------------------------------------------------
# the CPU engine
# ---------------------------------------------------------------------------------------------

def _engine(**kw):
    from operator_amd.engine.llm import LLMEngine
    from operator_amd.models.config import get_config
    from operator_amd.models.kv_cache import PagedKVCache
    from operator_amd.models.llama import LlamaModel

    cfg = get_config("tiny")
    m = LlamaModel(cfg, device="cpu", dtype=F32).init_random(seed=5)
    kv = PagedKVCache(cfg.layers, 128, m.hkv, cfg.head_dim, 16, device="cpu", dtype=F32)
    return LLMEngine(m, kv, **{"max_batch": 8, "max_context": 512, "use_graphs": False, "multi_step": 4, **kw})


def _slot_state(eng, slot):
    tb = eng.penalties
    n = int(tb.n[slot])
    lst = tb.lst[slot, :n].tolist()
    assert len(set(lst)) == n
    nz = torch.nonzero(tb.cnt[slot]).flatten().tolist()
    assert sorted(lst) == nz                                   # the list names exactly the non-zero words
    w = tb.cnt[slot].long()
    prompt = set(torch.nonzero(w < 0).flatten().tolist())
    counts = {t: int(w[t]) & ref.COUNT_MASK for t in nz if int(w[t]) & ref.COUNT_MASK}
    return prompt, counts


def check_engine_penalties(eng, prompt, GenRequest):
    """The engine properties of the issue, on whatever device ``eng`` runs: returns the outputs."""
    slots = {}
    release = eng._release

    def spy(r):
        if r.pslot >= 0:
            slots[id(r)] = r.pslot
        release(r)

    eng._release = spy
    mk = lambda n=10, **kw: GenRequest(list(prompt), max_tokens=n, temperature=0.0, ignore_eos=True, **kw)   # noqa: E731
    alone = mk()
    eng.generate([alone])
    t0 = alone.output[0]
    # the 3-token request finishes first: the others' rows are renumbered mid-run
    plain, short, freq, pres, rep = reqs = [mk(), mk(3, presence_penalty=100.0), mk(frequency_penalty=-100.0),
                                            mk(presence_penalty=100.0), mk(repetition_penalty=1.5)]
    eng.generate(reqs)
    assert all(r.error is None and r.done for r in reqs)
    assert plain.output == alone.output
    assert freq.output == [t0] * 10
    assert len(set(pres.output)) == 10 and len(short.output) == 3
    assert len({slots[id(r)] for r in reqs[1:]}) == 4 and id(plain) not in slots
    for r in reqs[1:]:
        seen, counts = _slot_state(eng, slots[id(r)])
        assert seen == set(prompt), "bit 31 on exactly the prompt's tokens"
        assert counts == dict(Counter(r.output[:-1])), "c = the histogram of output[:-1]"
        assert r.pslot == -1
    assert eng.penalties.free == eng.penalties.slots
    return {"alone": alone.output, "freq": freq.output, "pres": pres.output, "rep": rep.output}


PROMPT = [7, 8, 9, 7, 8, 9, 7, 8, 30, 31, 7, 8]


def test_engine_counts_follow_the_request():
    from operator_amd.engine.llm import GenRequest

    eng = _engine(prefix_sharing=False)
    check_engine_penalties(eng, PROMPT, GenRequest)
    assert eng.penalties.cnt.shape == (8, 1024) and eng.penalties.lst.shape == (8, 512 + 4)


def test_engine_flags_shared_prefix_tokens_and_reuses_slots():
    from operator_amd.engine.llm import GenRequest

    eng = _engine(prefix_sharing=True)
    prompt = list(range(40, 40 + 37)) + PROMPT
    check_engine_penalties(eng, prompt, GenRequest)
    hits = eng.stats.prefix_hits
    check_engine_penalties(eng, prompt, GenRequest)            # slots reused; prompts now on the shared prefix
    assert eng.stats.prefix_hits > hits


def test_check_sampling_ranges():
    from operator_amd.engine.llm import GenRequest

    eng = _engine()
    nan, inf = float("nan"), float("inf")
    for kw in ({"repetition_penalty": 0.0}, {"repetition_penalty": -1.0}, {"repetition_penalty": nan},
               {"repetition_penalty": inf}, {"repetition_penalty": True}, {"repetition_penalty": "1.1"},
               {"repetition_penalty": 1e-60}, {"frequency_penalty": nan}, {"frequency_penalty": inf},
               {"frequency_penalty": 1e39}, {"frequency_penalty": None}, {"presence_penalty": -inf},
               {"presence_penalty": False}, {"presence_penalty": [1]}):
        with pytest.raises(ValueError, match="_penalty must be"):
            eng.submit(GenRequest([3, 4, 5], max_tokens=2, **kw))
    assert not eng.waiting
    for kw in ({"repetition_penalty": 1}, {"frequency_penalty": -5}, {"presence_penalty": 7.5},
               {"repetition_penalty": 0.25, "frequency_penalty": 2.0}):
        eng.check_sampling(GenRequest([3, 4, 5], max_tokens=2, **kw))


def test_penalty_slots_0_refuses_and_allocates_nothing():
    from operator_amd.config import load_settings
    from operator_amd.engine.llm import GenRequest

    assert load_settings(env={}, overrides={}).engine.penalty_slots is None        # None: max_batch
    assert load_settings(env={}, overrides={"engine.penalty_slots": 0}).engine.penalty_slots == 0
    eng = _engine(penalty_slots=0)
    assert eng.penalties is None
    for kw in ({"repetition_penalty": 1.1}, {"frequency_penalty": 0.5}, {"presence_penalty": -0.5}):
        with pytest.raises(ValueError, match="penalties are not supported with engine.penalty_slots = 0"):
            eng.submit(GenRequest([3, 4, 5], max_tokens=2, **kw))
    r = GenRequest(list(PROMPT), max_tokens=6, temperature=0.0, ignore_eos=True)
    eng.generate([r])
    ref_eng = _engine()
    assert ref_eng.penalties.slots == 8
    r2 = GenRequest(list(PROMPT), max_tokens=6, temperature=0.0, ignore_eos=True)
    ref_eng.generate([r2])
    assert r.error is None and r.output == r2.output


def test_fewer_slots_than_rows_wait_for_a_free_slot():
    from operator_amd.engine.llm import GenRequest

    eng = _engine(penalty_slots=1)
    reqs = [GenRequest(list(PROMPT), max_tokens=5, temperature=0.0, ignore_eos=True, presence_penalty=100.0)
            for _ in range(3)]
    eng.generate(reqs)
    assert all(r.error is None and len(set(r.output)) == 5 for r in reqs)
    assert reqs[0].output == reqs[1].output == reqs[2].output and eng.penalties.free == 1


# ---------------------------------------------------------------------------------------------
# HTTP, AIProvider additionalConfig, CLI
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def server():
    from operator_amd.config import load_settings
    from operator_amd.engine.factory import build_explain_service
    from operator_amd.engine.server import CompatServer

    s = load_settings(env={}, overrides={"engine.model": "tiny", "engine.extra_models": ["tiny-gqa4"],
                                         "engine.device": "cpu", "engine.dtype": "float32",
                                         "engine.kv_cache_gb": 0.04, "engine.use_graphs": False,
                                         "engine.max_batch": 4, "engine.max_context": 512,
                                         "engine.max_prompt_tokens": 256, "engine.ignore_eos": True})
    svc = build_explain_service(s)
    srv = CompatServer(None, svc, "127.0.0.1", 0).start()
    llm = svc.services["tiny"].ee.llm
    seen = []
    submit = llm.submit
    llm.submit = lambda req: seen.append(req) or submit(req)
    yield srv, svc, seen
    srv.stop()
    svc.close()


def _post(srv, path, body):
    return httpx.post(f"http://127.0.0.1:{srv.port}{path}", json=body, timeout=120)


MSGS = [{"role": "user", "content": "why did my pod crash?"}]


def _chat(server, **kw):
    srv, _, seen = server
    r = _post(srv, "/v1/chat/completions", {"model": "tiny", "max_tokens": 8, "temperature": 0, "messages": MSGS, **kw})
    assert r.status_code == 200, r.text
    return r.json()["choices"][0]["message"]["content"], seen[-1]


def _generate(server, **options):
    srv, _, seen = server
    r = _post(srv, "/api/generate", {"model": "tiny", "prompt": "CrashLoopBackOff means", "stream": False,
                                     "options": {"num_predict": 8, "temperature": 0, **options}})
    assert r.status_code == 200, r.text
    return r.json()["response"], seen[-1]


def test_http_openai_penalties_reach_the_engine(server):
    base, req0 = _chat(server)
    assert (req0.repetition_penalty, req0.frequency_penalty, req0.presence_penalty) == (1.0, 0.0, 0.0)
    assert req0.pslot == -1 and len(set(req0.output)) > 1
    text, req = _chat(server, frequency_penalty=-2)
    assert req.frequency_penalty == -2.0 and req.output == [req0.output[0]] * 8 and text != base
    text, req = _chat(server, presence_penalty=2, repetition_penalty=1.5)
    assert (req.presence_penalty, req.repetition_penalty) == (2.0, 1.5)
    text, req = _chat(server, frequency_penalty=None, presence_penalty=None, repetition_penalty=None)
    assert text == base and not req.penalised                       # null = off
    srv = server[0]
    r = _post(srv, "/v1/completions", {"model": "tiny", "prompt": "CrashLoopBackOff means", "max_tokens": 8,
                                       "temperature": 0, "frequency_penalty": -2})
    assert r.status_code == 200 and server[2][-1].frequency_penalty == -2.0 and server[2][-1].pslot == -1


def _ollama_chat(server, **options):
    srv, _, seen = server
    r = _post(srv, "/api/chat", {"model": "tiny", "messages": MSGS, "stream": False,
                                 "options": {"num_predict": 8, "temperature": 0, **options}})
    assert r.status_code == 200, r.text
    return r.json()["message"]["content"], seen[-1]


def test_http_ollama_penalties_reach_the_engine(server):
    # the chat prompt: a bonus of 2 per repeat locks the greedy path onto the first token only
    # where that token is within 2 of the best logit at the second step, which holds for this
    # prompt on the tiny model (and is no property of the penalty code)
    cbase, creq0 = _ollama_chat(server)
    text, req = _ollama_chat(server, frequency_penalty=-2)
    assert req.frequency_penalty == -2.0 and req.output == [creq0.output[0]] * 8 and text != cbase
    base, req0 = _generate(server)
    assert not req0.penalised and len(set(req0.output)) > 1
    text, req = _generate(server, frequency_penalty=-2)
    assert req.frequency_penalty == -2.0 and req.output[0] == req0.output[0] and req.output != req0.output
    text, req = _generate(server, repeat_penalty=1.3, presence_penalty=0.5, repeat_last_n=-1)
    assert (req.repetition_penalty, req.presence_penalty, req.frequency_penalty) == (1.3, 0.5, 0.0)
    text, req = _generate(server, repeat_penalty=1.3, repeat_last_n=0)
    assert text == base and not req.penalised                       # repeat_last_n 0: repeat_penalty off
    text, req = _generate(server, repeat_penalty=None)
    assert text == base and not req.penalised
    srv = server[0]
    r = _post(srv, "/api/chat", {"model": "tiny", "messages": MSGS, "stream": False,
                                 "options": {"num_predict": 8, "temperature": 0, "repeat_penalty": 1.25}})
    assert r.status_code == 200 and server[2][-1].repetition_penalty == 1.25


BAD_OPENAI = [{"frequency_penalty": 2.5}, {"frequency_penalty": -2.01}, {"frequency_penalty": "high"},
              {"frequency_penalty": True}, {"presence_penalty": 3}, {"presence_penalty": [1]},
              {"presence_penalty": False}, {"repetition_penalty": 0}, {"repetition_penalty": -1.5},
              {"repetition_penalty": "1.1"}, {"repetition_penalty": True}]
BAD_OLLAMA = [{"repeat_penalty": 0}, {"repeat_penalty": -1}, {"repeat_penalty": "1.1"}, {"repeat_penalty": True},
              {"presence_penalty": "x"}, {"presence_penalty": True}, {"frequency_penalty": {}},
              {"frequency_penalty": False}, {"repeat_last_n": 64}, {"repeat_last_n": 1.5}, {"repeat_last_n": True},
              {"repeat_last_n": "all"}]
_ids = lambda b: "-".join(f"{k}={v}" for k, v in b.items())   # noqa: E731


@pytest.mark.parametrize("bad", BAD_OPENAI, ids=_ids)
def test_http_openai_bad_penalties_are_400(server, bad):
    n = len(server[2])
    r = _post(server[0], "/v1/chat/completions", {"model": "tiny", "max_tokens": 2, "messages": MSGS, **bad})
    err = r.json()["error"]
    assert r.status_code == 400 and err["type"] == "invalid_request_error" and next(iter(bad)) in err["message"], r.text
    assert len(server[2]) == n


@pytest.mark.parametrize("bad", BAD_OLLAMA, ids=_ids)
def test_http_ollama_bad_penalties_are_400(server, bad):
    n = len(server[2])
    r = _post(server[0], "/api/generate", {"model": "tiny", "prompt": "x", "options": {"num_predict": 2, **bad}})
    err = r.json()["error"]
    assert r.status_code == 400 and err["type"] == "invalid_request_error" and next(iter(bad)) in err["message"], r.text
    assert len(server[2]) == n


def test_http_engine_refusals_are_400(server, monkeypatch):
    """An engine that cannot apply a penalty (a TP replica, penalty_slots = 0) says so with a 400."""
    srv, svc, _ = server
    llm = svc.services["tiny"].ee.llm
    monkeypatch.setattr(llm, "penalties", None)
    for path, body in (("/v1/chat/completions", {"model": "tiny", "max_tokens": 2, "messages": MSGS,
                                                 "presence_penalty": 1}),
                       ("/api/generate", {"model": "tiny", "prompt": "x", "options": {"repeat_penalty": 1.1}})):
        r = _post(srv, path, body)
        assert r.status_code == 400 and r.json()["error"]["type"] == "invalid_request_error"
        assert "penalties are not supported with engine.penalty_slots = 0" in r.json()["error"]["message"]


def test_explain_reads_additional_config(server):
    from operator_amd.api.models import AIProviderConfig, AnalysisResult, AnalysisSummary
    from operator_amd.engine.explain import ExplainError

    _, svc, seen = server
    ee = svc.services["tiny"].ee
    res = AnalysisResult(pod_name="p", pod_namespace="default",
                         summary=AnalysisSummary(highest_severity="HIGH", significant_events=1))
    cfg = lambda extra=None: AIProviderConfig(model_id="tiny", max_tokens=8, temperature=0.0,   # noqa: E731
                                              caching_enabled=False, additional_headers=extra)
    base = ee.explain(res, cfg()).explanation
    first = seen[-1].output[0]
    assert ee.explain(res, cfg({"frequency_penalty": " -50 "})).explanation != base
    assert seen[-1].frequency_penalty == -50.0 and seen[-1].output == [first] * 8
    ee.explain(res, cfg({"repetition_penalty": "1.2", "presence_penalty": "0.5"}))
    assert (seen[-1].repetition_penalty, seen[-1].presence_penalty) == (1.2, 0.5)
    ids = ee.build_prompt(res, cfg())
    k0 = ee._key(ids, cfg())
    assert ee._key(ids, cfg({"x-other": "1"})) == k0                       # unset: the key is what it was
    assert ee._key(ids, cfg({"repetition_penalty": "1.0", "frequency_penalty": "0", "presence_penalty": "0.0"})) == k0
    keys = {k0, ee._key(ids, cfg({"repetition_penalty": "1.1"})), ee._key(ids, cfg({"frequency_penalty": "0.1"})),
            ee._key(ids, cfg({"presence_penalty": "0.1"})), ee._key(ids, cfg({"presence_penalty": "0.1", "top_k": "5"}))}
    assert len(keys) == 5
    for extra, name in (({"repetition_penalty": "strong"}, "repetition_penalty"), ({"repetition_penalty": "0"}, "repetition_penalty"),
                        ({"frequency_penalty": "nan"}, "frequency_penalty"), ({"presence_penalty": "inf"}, "presence_penalty"),
                        ({"presence_penalty": ""}, "presence_penalty")):
        with pytest.raises(ExplainError, match=f"additionalConfig.*{name}"):
            ee.explain(res, cfg(extra))


def test_cli_explain_takes_the_penalties(monkeypatch):
    from operator_amd import cli

    seen = {}
    monkeypatch.setattr(cli, "cmd_explain", lambda args: seen.update(vars(args)) or 0)
    assert cli.main(["explain", "pod.log", "--repetition-penalty", "1.1", "--frequency-penalty", "0.4",
                     "--presence-penalty", "-0.2"]) == 0
    assert (seen["repetition_penalty"], seen["frequency_penalty"], seen["presence_penalty"]) == (1.1, 0.4, -0.2)
    assert cli.main(["explain", "pod.log"]) == 0
    assert (seen["repetition_penalty"], seen["frequency_penalty"], seen["presence_penalty"]) == (1.0, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------
# tensor parallelism: refused at submit, a plain request still served
# ---------------------------------------------------------------------------------------------

def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from operator_amd.engine.llm import GenRequest
    from operator_amd.engine.tp import TPLLMEngine, control_group
    from operator_amd.models.config import get_config
    from operator_amd.models.kv_cache import PagedKVCache
    from operator_amd.models.llama import LlamaModel
    from operator_amd.parallel.comm import init_from_env, split_groups

    init_from_env(backend="gloo")
    tp, _ = split_groups(world)
    cfg = get_config("tiny-tp8")
    m = LlamaModel(cfg, device="cpu", tp=tp, dtype=torch.float32).init_random(seed=21)
    kv = PagedKVCache(cfg.layers, 64, m.hkv, cfg.head_dim, 16, device="cpu", dtype=torch.float32)
    eng = TPLLMEngine(m, kv, tp_group=tp, ctrl_group=control_group(tp), max_batch=4, max_context=256,
                      use_graphs=False)
    if tp.rank == 0:
        errs = []
        for kw in ({"repetition_penalty": 1.1}, {"frequency_penalty": 0.5}, {"presence_penalty": 0.5}):
            try:
                eng.submit(GenRequest([5, 6, 7, 8], max_tokens=4, temperature=0.8, **kw))
                errs.append(None)
            except ValueError as e:
                errs.append(str(e))
        ok = GenRequest([5, 6, 7, 8], max_tokens=4, temperature=0.8, seed=11, ignore_eos=True)
        eng.submit(ok)
        while not ok.done:
            eng.step()
        eng.close()
        torch.save({"errs": errs, "out": ok.output, "error": ok.error, "table": eng.penalties is None},
                   os.path.join(out_dir, "tp.pt"))
    else:
        eng.follow()
    dist.barrier()
    dist.destroy_process_group()


def test_tp_engine_rejects_penalised_requests(tmp_path):
    mp.start_processes(_tp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    got = torch.load(tmp_path / "tp.pt", weights_only=True)
    assert got["errs"] == ["penalties are not supported with engine.tp > 1"] * 3
    assert got["error"] is None and len(got["out"]) == 4 and got["table"]
