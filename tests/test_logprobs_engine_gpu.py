"""Log-probabilities through the engine's captured prefill and decode graphs on the GPU
(docs/PARITY.md "Sampling: logprobs"): one batch with a row that asks for 20 alternatives, one that
asks for its tokens' values only and one that does not ask, 2 x multi_step + 1 tokens each, so the
first token comes from a prefill graph and the columns of the decode state come round twice.
The kernel is reproducible, so the graphs must give the bytes of the same engine run eagerly.
"""
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

MULTI_STEP = 4
TOKENS = 2 * MULTI_STEP + 1
PROMPTS = [[7, 8, 9, 7, 8, 9, 7, 8, 30, 31, 7, 8], list(range(40, 55)), [5, 6, 7, 8, 9, 10, 11]]


def _engine(use_graphs):
    from operator_amd.engine.llm import LLMEngine
    from operator_amd.models.config import get_config
    from operator_amd.models.kv_cache import PagedKVCache
    from operator_amd.models.llama import LlamaModel

    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=5)
    kv = PagedKVCache(cfg.layers, 128, cfg.kv_heads, 128, 16, device="cuda")
    return LLMEngine(m, kv, max_batch=8, max_prefill_tokens=512, max_context=512, use_graphs=use_graphs,
                     multi_step=MULTI_STEP)


def _run(eng, nlps):
    from operator_amd.engine.llm import GenRequest

    reqs = [GenRequest(list(p), max_tokens=TOKENS, temperature=t, seed=11 + i, ignore_eos=True, logprobs=n)
            for i, (p, t, n) in enumerate(zip(PROMPTS, (0.0, 0.8, 0.8), nlps))]
    eng.generate(reqs)
    torch.cuda.synchronize()
    assert all(r.error is None and len(r.output) == TOKENS for r in reqs)
    return reqs


def _bits(v):
    return struct.pack("<d", v)   # a float of a request's lists holds an fp32 exactly; NaN payloads included


@pytest.fixture(scope="module")
def runs():
    g = _engine(True)
    graphs = _run(g, (20, 0, -1))
    plain = _run(g, (-1, -1, -1))
    assert g.stats.graph_replays > 0 and g.stats.prefill_graph_replays >= 2 and g.stats.prefill_eager == 0
    e = _engine(False)
    eager = _run(e, (20, 0, -1))
    assert e.stats.graph_replays == 0 and e.stats.prefill_graph_replays == 0
    return graphs, plain, eager


def test_lists_are_in_step_with_the_output(runs):
    a, b, c = runs[0]
    assert len(a.token_logprobs) == len(a.top_logprobs) == TOKENS and all(len(t) == 20 for t in a.top_logprobs)
    assert len(b.token_logprobs) == TOKENS and b.top_logprobs == [[]] * TOKENS
    assert c.token_logprobs == [] and c.top_logprobs == []
    for t, lp, top in zip(a.output, a.token_logprobs, a.top_logprobs):   # the greedy row: its token is entry 0
        assert top[0] == (t, lp) and lp <= 0
        assert all(top[j][1] >= top[j + 1][1] for j in range(19))
        assert sum(torch.tensor([v for _, v in top], dtype=torch.float64).exp()) <= 1 + 1e-4


def test_graphs_give_the_bytes_of_the_eager_engine(runs):
    graphs, _, eager = runs
    for g, e in zip(graphs, eager):
        assert g.output == e.output
        assert [_bits(v) for v in g.token_logprobs] == [_bits(v) for v in e.token_logprobs]
        assert [[(i, _bits(v)) for i, v in top] for top in g.top_logprobs] == \
               [[(i, _bits(v)) for i, v in top] for top in e.top_logprobs]


def test_the_off_row_is_the_row_of_a_run_without_logprobs(runs):
    graphs, plain, _ = runs
    assert [r.output for r in graphs] == [r.output for r in plain]   # logprobs only observe: the asking rows too
