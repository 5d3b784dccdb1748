"""Log-probabilities of sampled tokens (docs/PARITY.md "Sampling: logprobs") on the CPU tier: the
reference semantics on hand-made rows, the engine on the small CPU model against a plain forward
over prompt + output, and the four HTTP endpoints' shapes.

The engine's values are compared with log_softmax (fp64) of the logits of one prefill-shaped
forward over prompt + output. Both are fp32 forwards of the same weights that differ only in the
order of the attention sums (decode steps against one prefill), a few ulp of logits of magnitude
< 16 (2^-20 each), and the log-sum-exp adds less than that again: TOL = 1e-4 is more than ten
times what either can contribute.
"""
import math
import os
import socket

import httpx
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from operator_amd import ops

F32, I32 = torch.float32, torch.int32
NMAX = 20
TOL = 1e-4
INF, NAN = math.inf, math.nan


# ---------------------------------------------------------------------------------------------
# the reference on hand-made rows
# ---------------------------------------------------------------------------------------------

def _lp(rows, nlp, tokens, ctx=None, step=None, C=1, dtype=F32):
    x = torch.tensor(rows, dtype=dtype)
    R = x.shape[0]
    tok_lp = torch.full((R, C), 77.0)
    top_lp = torch.full((R, C, NMAX), 77.0)
    top_id = torch.full((R, C, NMAX), -7, dtype=I32)
    ops.sample_logprobs(x, torch.tensor(nlp, dtype=I32), None if ctx is None else torch.tensor(ctx, dtype=I32),
                        torch.tensor(tokens), None if step is None else torch.tensor([step]), tok_lp, top_lp, top_id)
    return tok_lp, top_lp, top_id


def test_reference_orders_by_logit_then_id_and_matches_log_softmax():
    row = [1.0, 3.0, 2.0, 3.0, -1.0, 2.0]
    tok_lp, top_lp, top_id = _lp([row], [4], [2])
    want = torch.log_softmax(torch.tensor(row, dtype=torch.float64), 0)
    assert top_id[0, 0, :4].tolist() == [1, 3, 2, 5]                     # ties by id
    assert torch.allclose(top_lp[0, 0, :4].double(), want[[1, 3, 2, 5]], atol=1e-6)
    assert abs(float(tok_lp[0, 0]) - float(want[2])) < 1e-6
    assert top_id[0, 0, 4:].tolist() == [-7] * (NMAX - 4) and bool((top_lp[0, 0, 4:] == 77.0).all())


def test_reference_signed_zeros_are_one_value():
    _, top_lp, top_id = _lp([[-1.0, -0.0, 0.0, -0.0, 0.0, -2.0]], [5], [0])
    assert top_id[0, 0, :5].tolist() == [1, 2, 3, 4, 0]
    assert len(set(top_lp[0, 0, :4].tolist())) == 1


def test_reference_nan_takes_no_part_and_short_rows_are_padded():
    tok_lp, top_lp, top_id = _lp([[NAN, 2.0, NAN, 1.0]] * 2, [5, 5], [0, 3])
    want = torch.log_softmax(torch.tensor([2.0, 1.0], dtype=torch.float64), 0)
    assert math.isnan(float(tok_lp[0, 0])) and abs(float(tok_lp[1, 0]) - float(want[1])) < 1e-6
    assert top_id[0, 0, :5].tolist() == [1, 3, -1, -1, -1]
    assert torch.allclose(top_lp[0, 0, :2].double(), want, atol=1e-6)
    assert top_lp[0, 0, 2:5].tolist() == [-INF] * 3 and float(top_lp[0, 0, 5]) == 77.0
    # no non-NaN logit: an empty list, the token's value NaN; all -inf: every value NaN
    tok_lp, top_lp, top_id = _lp([[NAN] * 3, [-INF] * 3], [2, 2], [1, 1])
    assert top_id[:, 0, :2].tolist() == [[-1, -1], [0, 1]]
    assert top_lp[0, 0, :2].tolist() == [-INF, -INF] and bool(torch.isnan(top_lp[1, 0, :2]).all())
    assert bool(torch.isnan(tok_lp[:, 0]).all())


def test_reference_infinities():
    # a term at the maximum counts as exactly 1, also at +inf: lse = +inf, finite logits get -inf
    tok_lp, top_lp, top_id = _lp([[1.0, INF, 2.0, INF, -INF]], [3], [0])
    assert top_id[0, 0, :3].tolist() == [1, 3, 2]
    assert float(tok_lp[0, 0]) == -INF and float(top_lp[0, 0, 2]) == -INF
    # -inf logits get -inf under a finite maximum
    tok_lp, top_lp, top_id = _lp([[0.0, -INF, -INF]], [3], [1])
    assert float(tok_lp[0, 0]) == -INF and top_id[0, 0, :3].tolist() == [0, 1, 2]
    assert top_lp[0, 0, :3].tolist() == [0.0, -INF, -INF]


def test_reference_leaves_other_rows_columns_and_entries_alone():
    rows = [[0.5, 1.5, 2.5]] * 4
    tok_lp, top_lp, top_id = _lp(rows, [-1, 0, 2, 2], [0, 1, 2, 0], ctx=[5, 5, 5, 0], step=6, C=4)   # column 6 % 4
    assert bool((tok_lp[[0, 3]] == 77.0).all()) and bool((top_id[[0, 1, 3]] == -7).all())
    assert bool((tok_lp[:, [0, 1, 3]] == 77.0).all()) and bool((top_id[:, [0, 1, 3]] == -7).all())
    assert float(tok_lp[1, 2]) != 77.0 and top_id[2, 2, :3].tolist() == [2, 1, -7]
    assert float(top_lp[2, 2, 0]) == float(tok_lp[2, 2])


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


def _forward_logits(model, ids):
    """fp32 logits [len(ids), vocab] of one plain forward over ``ids``: row j predicts token j + 1."""
    from operator_amd.models.kv_cache import PagedKVCache
    from operator_amd.models.llama import ForwardBatch

    n, cfg = len(ids), model.cfg
    kv = PagedKVCache(cfg.layers, (n + 15) // 16 + 1, model.hkv, cfg.head_dim, 16, device="cpu", dtype=F32)
    ar = torch.arange(n)
    fb = ForwardBatch(torch.tensor(ids), ar, ar.clone(), True, ar.clone(), seq_lens=[n])
    return model.forward(fb, kv).float()


def _check_against_forward(model, r, adjust=None):
    """``r``'s lists against log_softmax of the forward logits (after ``adjust(logits, i)``, the
    penalty on the logits of output position i)."""
    assert len(r.token_logprobs) == len(r.top_logprobs) == len(r.output)
    logits = _forward_logits(model, r.prompt + r.output)
    worst = 0.0
    for i, t in enumerate(r.output):
        x = logits[len(r.prompt) - 1 + i].clone()
        if adjust is not None:
            x = adjust(x, i)
        ls = torch.log_softmax(x.double(), 0)
        worst = max(worst, abs(r.token_logprobs[i] - float(ls[t])))
        top = r.top_logprobs[i]
        assert len(top) == r.logprobs
        assert [a for a, _ in top] == torch.sort(-x, stable=True).indices[:r.logprobs].tolist()
        worst = max([worst] + [abs(b - float(ls[a])) for a, b in top])
        assert all(top[j][1] >= top[j + 1][1] for j in range(len(top) - 1))
    print(f"max abs error against the forward: {worst:.3g}")
    assert worst <= TOL
    return worst


PROMPT = [7, 8, 9, 7, 8, 9, 7, 8, 30, 31, 7, 8]


@pytest.fixture(scope="module")
def eng():
    return _engine()


def _req(n=11, **kw):
    from operator_amd.engine.llm import GenRequest

    return GenRequest(list(PROMPT), **{"max_tokens": n, "temperature": 0.0, "ignore_eos": True, **kw})


def test_engine_logprobs_only_observe_and_match_a_plain_forward(eng):
    """11 tokens at multi_step 4: the first from the prefill, then windows whose columns come round again."""
    plain, on = _req(), _req(logprobs=5)
    eng.generate([plain])
    eng.generate([on])
    assert on.output == plain.output and len(on.output) == 11
    assert plain.token_logprobs == [] and plain.top_logprobs == []
    _check_against_forward(eng.model, on)
    for t, lp, top in zip(on.output, on.token_logprobs, on.top_logprobs):   # greedy: the token is entry 0
        assert top[0] == (t, lp)


def test_engine_sampled_rows_and_zero_alternatives(eng):
    hot, hot0 = _req(logprobs=3, temperature=0.9, seed=3), _req(logprobs=0, temperature=0.9, seed=3)
    eng.generate([hot])
    eng.generate([hot0])
    assert hot.output == hot0.output
    assert hot0.token_logprobs == hot.token_logprobs and hot0.top_logprobs == [[]] * 11
    _check_against_forward(eng.model, hot)
    assert any(t != top[0][0] for t, top in zip(hot.output, hot.top_logprobs)), "T = 0.9 never left the greedy path"


def test_engine_mixed_batch_leaves_the_off_rows_alone(eng):
    mk = lambda **kw: [_req(temperature=0.7, seed=1, **kw), _req(7, **kw), _req(temperature=0.7, seed=2, **kw)]   # noqa: E731
    solo = mk()
    for r in solo:
        eng.generate([r])
    a, b, c = batch = [_req(temperature=0.7, seed=1), _req(7, logprobs=20), _req(temperature=0.7, seed=2, logprobs=0)]
    eng.generate(batch)
    assert [r.output for r in batch] == [r.output for r in solo]
    assert a.token_logprobs == [] and len(b.top_logprobs) == 7 and len(c.token_logprobs) == 11
    _check_against_forward(eng.model, b)
    _check_against_forward(eng.model, c)


def test_engine_eos_inside_a_window_keeps_the_lists_in_step(eng):
    base = _req(logprobs=2)
    eng.generate([base])
    stop = base.output[6]                      # the second token of the second window
    first = base.output.index(stop)
    eos = eng.eos
    eng.eos = {stop}
    try:
        r = _req(logprobs=2, ignore_eos=False)
        eng.generate([r])
    finally:
        eng.eos = eos
    assert r.output == base.output[:first + 1] and first >= 1
    assert len(r.token_logprobs) == len(r.top_logprobs) == len(r.output)
    assert r.token_logprobs == base.token_logprobs[:first + 1]


def test_engine_penalised_request_reports_the_penalised_distribution(eng):
    f, p = 0.7, 0.3
    r = _req(logprobs=4, frequency_penalty=f, presence_penalty=p)
    eng.generate([r])

    def adjust(x, i):
        for t in set(r.output[:i]):
            x[t] = x[t] - (torch.tensor(f) * r.output[:i].count(t) + torch.tensor(p))
        return x

    _check_against_forward(eng.model, r, adjust)
    raw = _req(logprobs=4)
    eng.generate([raw])
    assert raw.token_logprobs[0] == r.token_logprobs[0] and raw.token_logprobs != r.token_logprobs


def test_engine_without_the_kernel_refuses():
    e = _engine(logprobs=False)
    assert e._state(1).tok_lp is None
    with pytest.raises(ValueError, match="logprobs are not supported with engine.logprobs = false"):
        e.submit(_req(logprobs=0))
    ok = _req(4)
    e.generate([ok])
    assert len(ok.output) == 4 and ok.error is None


@pytest.mark.parametrize("bad", [-2, 21, 1.0, True, "5", None])
def test_logprobs_range_errors_raise(eng, bad):
    with pytest.raises(ValueError, match="logprobs must be an integer in -1..20"):
        eng.submit(_req(logprobs=bad))
    assert not eng.waiting


def test_config_reaches_the_engine():
    from operator_amd.config import load_settings

    assert load_settings(env={}, overrides={}).engine.logprobs is True
    assert load_settings(env={}, overrides={"engine.logprobs": False}).engine.logprobs is False


# ---------------------------------------------------------------------------------------------
# HTTP
# ---------------------------------------------------------------------------------------------

def _service(**over):
    from operator_amd.config import load_settings
    from operator_amd.engine.factory import build_explain_service

    s = load_settings(env={}, overrides={"engine.model": "tiny", "engine.device": "cpu", "engine.dtype": "float32",
                                         "engine.kv_cache_gb": 0.04, "engine.use_graphs": False,
                                         "engine.max_batch": 4, "engine.max_context": 512,
                                         "engine.max_prompt_tokens": 256, "engine.ignore_eos": True, **over})
    return build_explain_service(s)


@pytest.fixture(scope="module")
def server():
    from operator_amd.engine.server import CompatServer

    svc = _service()
    srv = CompatServer(None, svc, "127.0.0.1", 0).start()
    llm = svc.ee.llm
    seen = []
    submit = llm.submit
    llm.submit = lambda req: seen.append(req) or submit(req)
    yield srv, svc, seen
    srv.stop()
    svc.ee.close()


def _post(srv, path, body):
    return httpx.post(f"http://127.0.0.1:{srv.port}{path}", json=body, timeout=120)


MSGS = [{"role": "user", "content": "why did my pod crash?"}]
OPENAI_CHAT = ("/v1/chat/completions", {"model": "tiny", "max_tokens": 6, "temperature": 0, "messages": MSGS})
OPENAI_TEXT = ("/v1/completions", {"model": "tiny", "max_tokens": 6, "temperature": 0, "prompt": "CrashLoopBackOff means"})
OLLAMA_GEN = ("/api/generate", {"model": "tiny", "prompt": "CrashLoopBackOff means", "stream": False,
                                "options": {"num_predict": 6, "temperature": 0}})
OLLAMA_CHAT = ("/api/chat", {"model": "tiny", "messages": MSGS, "stream": False,
                             "options": {"num_predict": 6, "temperature": 0}})


def _check_chat_entries(entries, n_tokens, n_top):
    assert len(entries) == n_tokens
    for e in entries:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert bytes(e["bytes"]).decode("utf-8", "replace") == e["token"] and e["logprob"] <= 0
        assert len(e["top_logprobs"]) == n_top
        for t in e["top_logprobs"]:
            assert set(t) == {"token", "logprob", "bytes"} and bytes(t["bytes"]).decode("utf-8", "replace") == t["token"]
        assert sum(math.exp(t["logprob"]) for t in e["top_logprobs"]) <= 1 + 1e-4


def test_http_openai_chat_matches_the_models_logits(server):
    srv, svc, seen = server
    path, body = OPENAI_CHAT
    r = _post(srv, path, {**body, "logprobs": True, "top_logprobs": 5})
    assert r.status_code == 200, r.text
    b = r.json()
    _check_chat_entries(b["choices"][0]["logprobs"]["content"], b["usage"]["completion_tokens"], 5)
    req = seen[-1]
    assert req.logprobs == 5
    model = svc.ee.llm.model
    logits = _forward_logits(model, req.prompt + req.output)
    for i, e in enumerate(b["choices"][0]["logprobs"]["content"]):
        ls = torch.log_softmax(logits[len(req.prompt) - 1 + i].double(), 0)
        want = torch.topk(ls, 5).values.tolist()
        assert max(abs(t["logprob"] - w) for t, w in zip(e["top_logprobs"], want)) <= TOL
        assert abs(e["logprob"] - float(ls[req.output[i]])) <= TOL
    # logprobs alone: the tokens' values, no alternatives; the single SSE chunk carries the object too
    r = _post(srv, path, {**body, "logprobs": True})
    _check_chat_entries(r.json()["choices"][0]["logprobs"]["content"], 6, 0)
    r = _post(srv, path, {**body, "logprobs": True, "top_logprobs": 2, "stream": True})
    chunk = __import__("json").loads(r.text.split("data: ")[1])
    _check_chat_entries(chunk["choices"][0]["logprobs"]["content"], 6, 2)


def test_http_openai_completions_shape(server):
    srv, _, seen = server
    path, body = OPENAI_TEXT
    r = _post(srv, path, {**body, "logprobs": 3})
    assert r.status_code == 200, r.text
    b = r.json()
    lp, n = b["choices"][0]["logprobs"], b["usage"]["completion_tokens"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"} and seen[-1].logprobs == 3
    assert all(len(lp[k]) == n for k in lp) and n == 6
    assert lp["text_offset"] == [sum(len(t) for t in lp["tokens"][:i]) for i in range(n)]
    for tok, v, top in zip(lp["tokens"], lp["token_logprobs"], lp["top_logprobs"]):
        assert 1 <= len(top) <= 3 and all(isinstance(k, str) for k in top)
        assert sum(math.exp(x) for x in top.values()) <= 1 + 1e-4
        assert top.get(tok) == v                                        # greedy: the token is the most likely
    r = _post(srv, path, {**body, "logprobs": 0})
    assert r.json()["choices"][0]["logprobs"]["top_logprobs"] == [{}] * 6 and seen[-1].logprobs == 0


@pytest.mark.parametrize("path,body", [OLLAMA_GEN, OLLAMA_CHAT], ids=["generate", "chat"])
def test_http_ollama_shape(server, path, body):
    srv, _, seen = server
    r = _post(srv, path, {**body, "logprobs": True, "top_logprobs": 4})
    assert r.status_code == 200, r.text
    b = r.json()
    _check_chat_entries(b["logprobs"], b["eval_count"], 4)
    assert seen[-1].logprobs == 4
    r = _post(srv, path, {**body, "logprobs": True, "stream": True})       # one NDJSON line
    _check_chat_entries(__import__("json").loads(r.text)["logprobs"], 6, 0)


def test_http_without_the_field_the_bodies_are_todays(server):
    srv, _, seen = server
    for path, body in (OPENAI_CHAT, OPENAI_TEXT):
        for extra in ({}, {"logprobs": None}, {"logprobs": False} if path == OPENAI_CHAT[0] else {}):
            b = _post(srv, path, {**body, **extra}).json()
            assert b["choices"][0]["logprobs"] is None and seen[-1].logprobs == -1
            assert set(b["choices"][0]) == {"index", "message" if "chat" in path else "text", "logprobs", "finish_reason"}
    for path, body in (OLLAMA_GEN, OLLAMA_CHAT):
        for extra in ({}, {"logprobs": False}):
            b = _post(srv, path, {**body, **extra}).json()
            assert "logprobs" not in b and seen[-1].logprobs == -1
            assert set(b) == {"model", "created_at", "done", "done_reason", "prompt_eval_count", "eval_count",
                              "total_duration", "message" if path.endswith("chat") else "response"}


BAD = [(OPENAI_CHAT, {"logprobs": 1}), (OPENAI_CHAT, {"logprobs": "true"}), (OPENAI_CHAT, {"top_logprobs": 3}),
       (OPENAI_CHAT, {"logprobs": False, "top_logprobs": 3}), (OPENAI_CHAT, {"logprobs": True, "top_logprobs": 21}),
       (OPENAI_CHAT, {"logprobs": True, "top_logprobs": -1}), (OPENAI_CHAT, {"logprobs": True, "top_logprobs": True}),
       (OPENAI_CHAT, {"logprobs": True, "top_logprobs": 2.5}), (OPENAI_CHAT, {"logprobs": True, "top_logprobs": "3"}),
       (OPENAI_TEXT, {"logprobs": True}), (OPENAI_TEXT, {"logprobs": 21}), (OPENAI_TEXT, {"logprobs": -1}),
       (OPENAI_TEXT, {"logprobs": "2"}), (OLLAMA_GEN, {"logprobs": 1}), (OLLAMA_GEN, {"top_logprobs": 2}),
       (OLLAMA_GEN, {"logprobs": True, "top_logprobs": 21}), (OLLAMA_CHAT, {"logprobs": True, "top_logprobs": False}),
       (OLLAMA_CHAT, {"logprobs": "yes"})]


@pytest.mark.parametrize("case,bad", BAD, ids=lambda v: str(v) if isinstance(v, dict) else v[0])
def test_http_bad_logprobs_are_400(server, case, bad):
    srv, _, seen = server
    n = len(seen)
    r = _post(srv, case[0], {**case[1], **bad})
    assert r.status_code == 400 and r.json()["error"]["type"] == "invalid_request_error", r.text
    assert "logprobs" in r.json()["error"]["message"] and len(seen) == n


def test_http_engine_refusals_are_400():
    """engine.logprobs = false travels from the settings to the engine, whose refusal is a 400."""
    from operator_amd.engine.server import CompatServer

    svc = _service(**{"engine.logprobs": False})
    srv = CompatServer(None, svc, "127.0.0.1", 0).start()
    try:
        assert svc.ee.llm.logprobs is False
        for (path, body), extra in ((OPENAI_CHAT, {"logprobs": True}), (OPENAI_TEXT, {"logprobs": 1}),
                                    (OLLAMA_GEN, {"logprobs": True})):
            r = _post(srv, path, {**body, **extra})
            assert r.status_code == 400 and r.json()["error"]["type"] == "invalid_request_error"
            assert "logprobs are not supported with engine.logprobs = false" in r.json()["error"]["message"]
        assert _post(srv, *OPENAI_TEXT).status_code == 200
    finally:
        srv.stop()
        svc.ee.close()


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
        for n in (0, 5):
            try:
                eng.submit(GenRequest([5, 6, 7, 8], max_tokens=4, temperature=0.8, logprobs=n))
                errs.append(None)
            except ValueError as e:
                errs.append(str(e))
        ok = GenRequest([5, 6, 7, 8], max_tokens=4, temperature=0.8, seed=11, ignore_eos=True)
        eng.submit(ok)
        while not ok.done:
            eng.step()
        eng.close()
        torch.save({"errs": errs, "out": ok.output, "error": ok.error, "kernel": eng.logprobs},
                   os.path.join(out_dir, "tp.pt"))
    else:
        eng.follow()
    dist.barrier()
    dist.destroy_process_group()


def test_tp_engine_rejects_logprob_requests(tmp_path):
    mp.start_processes(_tp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    got = torch.load(tmp_path / "tp.pt", weights_only=True)
    assert got["errs"] == ["logprobs are not supported with engine.tp > 1"] * 2
    assert got["error"] is None and len(got["out"]) == 4 and got["kernel"] is False
