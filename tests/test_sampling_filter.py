"""Top-k / top-p (nucleus) sampling on the CPU tier: the fp64 reference semantics
(ops/reference.py sample_threshold, docs/PARITY.md "Sampling"), the filtered sampler, and the
parameters' way from the HTTP bodies, an AIProvider's additionalConfig and a GenRequest down to
the engine (a tiny model on the CPU), including the rejection on a tensor-parallel replica."""
import math
import os
import socket

import httpx
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from operator_amd import ops
from operator_amd.ops import reference as ref

NEG_INF = float("-inf")


def _thr(rows, temp, top_k, top_p, dtype=torch.float32):
    logits = torch.tensor(rows, dtype=torch.float64).to(dtype)
    n = logits.shape[0]
    bc = lambda v, dt: torch.tensor(v if isinstance(v, list) else [v] * n, dtype=dt)   # noqa: E731
    kept = torch.full((n,), -1, dtype=torch.int32)
    thr = ops.sample_threshold(logits, bc(temp, torch.float32), bc(top_k, torch.int32), bc(top_p, torch.float32),
                               out_kept=kept)
    assert thr.dtype == torch.float32 and thr.shape == (n,)
    return thr.tolist(), kept.tolist()


# probabilities 0.5 / 0.3 / 0.15 / 0.05 at T = 1, in an order that is not sorted
P_ROW = [math.log(0.15), math.log(0.5), math.log(0.05), math.log(0.3)]


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def test_top_k_keeps_ties_at_the_kth_value():
    row = [1.0, 3.0, 2.0, 2.0, 2.0, 0.5, 3.0]
    thr, kept = _thr([row] * 4, 1.0, [1, 2, 3, 6], 1.0)
    assert thr == [3.0, 3.0, 2.0, 1.0] and kept == [2, 2, 5, 6]   # k = 1: both 3.0 are kept


def test_top_p_on_a_hand_written_row():
    thr, kept = _thr([P_ROW] * 4, 1.0, 0, [0.7, 0.81, 0.5, 1e-6])
    assert kept == [2, 3, 1, 1]                                    # 0.5 + 0.3 >= 0.7; 0.95 >= 0.81; 0.5 >= 0.5
    assert thr == [_f32(math.log(0.3)), _f32(math.log(0.15)), _f32(math.log(0.5)), _f32(math.log(0.5))]


def test_top_p_is_taken_over_the_renormalised_top_k_set():
    """top_k = 2 leaves {0.5, 0.3}, renormalised 0.625 / 0.375: top_p = 0.7 needs both. At
    top_p = 0.6 the order decides: after top-k the first token alone reaches it (0.625 >= 0.6),
    over the whole row it would not (0.5 < 0.6) and two would be kept."""
    thr, kept = _thr([P_ROW] * 2, 1.0, 2, [0.7, 0.6])
    assert kept == [2, 1]
    assert thr == [_f32(math.log(0.3)), _f32(math.log(0.5))]


def test_temperature_applies_before_top_p():
    # at T = 0.5 the probabilities are proportional to p^2: 0.25 / 0.09 / 0.0225 / 0.0025 -> 0.685 of the mass on the first
    thr, kept = _thr([P_ROW] * 2, [1.0, 0.5], 0, 0.6)
    assert kept == [2, 1]


def test_greedy_and_default_rows_are_unfiltered():
    thr, kept = _thr([P_ROW] * 5, [0.0, -1.0, 1.0, 1.0, 1.0], [2, 2, 0, 4, 9], [0.5, 0.5, 1.0, 1.0, 1.0])
    assert thr == [NEG_INF] * 5 and kept == [4] * 5                # T <= 0; off; top_k >= vocab


def test_special_values():
    inf, nan = float("inf"), float("nan")
    # -inf logits carry no mass and are cut by any finite threshold; kept when nothing is cut
    thr, kept = _thr([[NEG_INF, 1.0, NEG_INF, 0.0]] * 3, 1.0, [0, 3, 2], [0.99, 1.0, 1.0])
    assert thr == [0.0, NEG_INF, 0.0] and kept == [2, 4, 2]   # k = 3: the third value is -inf, a tie of two
    # -0.0 and +0.0 are one value: a tie at the k-th value, and the threshold is +0.0
    thr, kept = _thr([[-0.0, 0.0, -1.0, 1.0]], 1.0, 2, 1.0)
    assert kept == [3] and thr == [0.0] and math.copysign(1.0, thr[0]) == 1.0
    # NaN is never kept and never counted
    thr, kept = _thr([[nan, 2.0, 1.0, nan, 0.0]], 1.0, 2, 1.0)
    assert thr == [1.0] and kept == [2]
    # an all -inf row: every mass is 0, nothing to cut
    thr, kept = _thr([[NEG_INF] * 4], 1.0, 2, 0.5)
    assert thr == [NEG_INF] and kept == [4]
    # +inf maximum: all the mass
    thr, kept = _thr([[1.0, inf, 2.0]], 1.0, 0, 0.9)
    assert thr == [inf] and kept == [1]


def _rand_case(rows=6, V=500, seed=3):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, V, generator=g) * 3
    return logits, torch.arange(rows) * 5 + 2, torch.arange(rows) + 40


def test_top_k_1_is_greedy_and_full_k_is_unfiltered():
    logits, seeds, pos = _rand_case()
    n, V = logits.shape
    ones = torch.ones(n)
    greedy = ops.sample(logits, torch.zeros(n), seeds, pos)
    for p in (1.0, 0.9):
        tok = ops.sample(logits, ones, seeds, pos, top_k=torch.ones(n, dtype=torch.int32), top_p=torch.full((n,), p))
        assert torch.equal(tok, greedy)
    tok = ops.sample(logits, ones, seeds, pos, top_p=torch.full((n,), 1e-6))
    assert torch.equal(tok, greedy)
    plain_tok, plain_val = ref.sample_shard(logits, ones, seeds, pos)
    assert not torch.equal(plain_tok, greedy)   # T = 1 alone does sample
    for k in (V, V + 5, 0):
        tok, val = ref.sample_shard(logits, ones, seeds, pos, top_k=torch.full((n,), k, dtype=torch.int32),
                                    top_p=torch.ones(n))
        assert torch.equal(tok, plain_tok) and torch.equal(val, plain_val)
    thr = torch.full((n,), 123.0)
    val = torch.empty(n)
    tok = ops.sample(logits, ones, seeds, pos, out_val=val, top_k=torch.full((n,), V, dtype=torch.int32), thr=thr)
    assert torch.equal(tok, plain_tok) and torch.equal(val, plain_val) and (thr == NEG_INF).all()   # caller's buffer


def test_sampled_tokens_stay_in_the_kept_set():
    """200 positions of one row at top_k = 5: every token is one of the reference's five, and
    more than one of them occurs."""
    g = torch.Generator().manual_seed(9)
    row = torch.randn(1, 300, generator=g)
    n = 200
    logits = row.expand(n, 300).contiguous()
    k = torch.full((n,), 5, dtype=torch.int32)
    thr, kept = ref.sample_threshold(logits, torch.ones(n), k, torch.ones(n))
    assert kept.tolist() == [5] * n
    allowed = set(torch.nonzero(row[0] >= thr[0]).flatten().tolist())
    assert allowed == set(torch.topk(row[0], 5).indices.tolist())
    tok = ops.sample(logits, torch.ones(n), torch.full((n,), 7), torch.arange(n), top_k=k)
    assert set(tok.tolist()) <= allowed and len(set(tok.tolist())) > 1


def test_shard_filtering_needs_the_callers_threshold():
    logits, seeds, pos = _rand_case()
    n, V = logits.shape
    ones = torch.ones(n)
    k = torch.full((n,), 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="col_offset"):
        ops.sample(logits[:, 100:], ones, seeds, pos, col_offset=100, top_k=k)
    # a global threshold applied per shard and a max over shards: the unsharded filtered token
    thr = ops.sample_threshold(logits, ones, k, ones)
    want = ops.sample(logits, ones, seeds, pos, top_k=k)
    best_t = best_v = None
    for a, b in ((0, 100), (100, V)):
        v = torch.empty(n)
        t = ops.sample(logits[:, a:b], ones, seeds, pos, col_offset=a, out_val=v, thr=thr)
        if best_t is None:
            best_t, best_v = t, v
        else:
            take = v > best_v
            best_t, best_v = torch.where(take, t, best_t), torch.where(take, v, best_v)
    assert torch.equal(best_t, want)


# ---------------------------------------------------------------------------------------------
# engine, HTTP, AIProvider additionalConfig
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
                                         "engine.max_prompt_tokens": 256})
    svc = build_explain_service(s)
    srv = CompatServer(None, svc, "127.0.0.1", 0).start()
    yield srv, svc
    srv.stop()
    svc.close()


def _post(srv, path, body):
    return httpx.post(f"http://127.0.0.1:{srv.port}{path}", json=body, timeout=120)


MSGS = [{"role": "user", "content": "why did my pod crash?"}]


def _chat(srv, **kw):
    r = _post(srv, "/v1/chat/completions", {"model": "tiny", "max_tokens": 12, "seed": 5, "messages": MSGS, **kw})
    assert r.status_code == 200, r.text
    return r.json()["choices"][0]["message"]["content"]


def _generate(srv, **options):
    r = _post(srv, "/api/generate", {"model": "tiny", "prompt": "CrashLoopBackOff means", "stream": False,
                                     "options": {"num_predict": 12, "seed": 5, **options}})
    assert r.status_code == 200, r.text
    return r.json()["response"]


def test_http_top_k_1_and_tiny_top_p_equal_greedy(server):
    srv, _ = server
    greedy = _chat(srv, temperature=0)
    assert _chat(srv, temperature=1.0) != greedy            # the prompt and seed do sample at T = 1
    assert _chat(srv, temperature=1.0, top_k=1) == greedy
    assert _chat(srv, temperature=1.0, top_p=1e-6) == greedy
    assert _chat(srv, temperature=1.0, top_k=None, top_p=None) == _chat(srv, temperature=1.0)   # null = off
    greedy = _generate(srv, temperature=0)
    assert _generate(srv, temperature=1.0) != greedy
    assert _generate(srv, temperature=1.0, top_k=1) == greedy
    assert _generate(srv, temperature=1.0, top_p=1e-6) == greedy
    r = _post(srv, "/v1/completions", {"model": "tiny", "prompt": "CrashLoopBackOff means", "max_tokens": 12,
                                       "seed": 5, "temperature": 1.0, "top_k": 1})
    r0 = _post(srv, "/v1/completions", {"model": "tiny", "prompt": "CrashLoopBackOff means", "max_tokens": 12,
                                        "temperature": 0})
    assert r.status_code == 200 and r.json()["choices"][0]["text"] == r0.json()["choices"][0]["text"]


@pytest.mark.parametrize("bad", [{"top_p": 0}, {"top_p": -0.1}, {"top_p": 1.5}, {"top_p": "most"}, {"top_p": True},
                                 {"top_k": -1}, {"top_k": 2.5}, {"top_k": "forty"}, {"top_k": [40]}, {"top_k": 2 ** 40}],
                         ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_http_bad_filter_values_are_400(server, bad):
    srv, _ = server
    r = _post(srv, "/v1/chat/completions", {"model": "tiny", "max_tokens": 2, "messages": MSGS, **bad})
    assert r.status_code == 400 and "bad sampling parameter" in r.json()["error"]["message"], r.text
    r = _post(srv, "/api/generate", {"model": "tiny", "prompt": "x", "options": {"num_predict": 2, **bad}})
    assert r.status_code == 400 and "bad sampling parameter" in r.json()["error"]["message"], r.text


def test_engine_submit_validates(server):
    from operator_amd.engine.llm import GenRequest

    _, svc = server
    llm = svc.services["tiny"].ee.llm
    for kw in ({"top_k": -1}, {"top_p": 0.0}, {"top_p": 1.01}, {"top_k": 1.5}, {"top_p": float("nan")}):
        with pytest.raises(ValueError, match="top_k|top_p"):
            llm.submit(GenRequest([3, 4, 5], max_tokens=2, **kw))
    assert not llm.waiting


def test_explain_reads_additional_config(server):
    from operator_amd.api.models import AIProviderConfig, AnalysisResult, AnalysisSummary
    from operator_amd.engine.explain import ExplainError

    _, svc = server
    ee = svc.services["tiny"].ee
    res = AnalysisResult(pod_name="p", pod_namespace="default",
                         summary=AnalysisSummary(highest_severity="HIGH", significant_events=1))
    cfg = lambda t, extra=None: AIProviderConfig(model_id="tiny", max_tokens=10, temperature=t,   # noqa: E731
                                                 caching_enabled=False, additional_headers=extra)
    greedy = ee.explain(res, cfg(0.0)).explanation
    assert ee.explain(res, cfg(1.0)).explanation != greedy
    assert ee.explain(res, cfg(1.0, {"top_k": "1"})).explanation == greedy
    assert ee.explain(res, cfg(1.0, {"top_p": "0.000001"})).explanation == greedy
    ids = ee.build_prompt(res, cfg(1.0))
    k0 = ee._key(ids, cfg(1.0))
    assert ee._key(ids, cfg(1.0, {"x-other": "1"})) == k0                  # unset: the key is what it was
    assert ee._key(ids, cfg(1.0, {"top_k": "0", "top_p": "1.0"})) == k0    # the off values too
    assert len({k0, ee._key(ids, cfg(1.0, {"top_k": "1"})), ee._key(ids, cfg(1.0, {"top_p": "0.9"}))}) == 3
    for extra in ({"top_k": "many"}, {"top_p": "2"}, {"top_k": "-3"}):
        with pytest.raises(ExplainError, match="additionalConfig"):
            ee.explain(res, cfg(1.0, extra))


def test_cli_explain_takes_top_k_and_top_p(monkeypatch):
    from operator_amd import cli

    seen = {}
    monkeypatch.setattr(cli, "cmd_explain", lambda args: seen.update(vars(args)) or 0)
    assert cli.main(["explain", "pod.log", "--temperature", "0.8", "--top-k", "40", "--top-p", "0.9"]) == 0
    assert (seen["top_k"], seen["top_p"], seen["temperature"]) == (40, 0.9, 0.8)
    assert cli.main(["explain", "pod.log"]) == 0
    assert (seen["top_k"], seen["top_p"]) == (0, 1.0)


# ---------------------------------------------------------------------------------------------
# tensor parallelism: rejected at submit, defaults still served
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
        for kw in ({"top_p": 0.9}, {"top_k": 40}):
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
        torch.save({"errs": errs, "out": ok.output, "error": ok.error}, os.path.join(out_dir, "tp.pt"))
    else:
        eng.follow()
    dist.barrier()
    dist.destroy_process_group()


def test_tp_engine_rejects_filtered_requests(tmp_path):
    mp.start_processes(_tp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    got = torch.load(tmp_path / "tp.pt", weights_only=True)
    assert got["errs"] == ["top_k / top_p are not supported with engine.tp > 1"] * 2
    assert got["error"] is None and len(got["out"]) == 4
