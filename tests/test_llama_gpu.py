"""Explanation model on the GPU kernels: parity with the CPU fp32 reference path,
hipGraph decode == eager decode, and an 8B-architecture smoke step."""
import pytest
import torch

from operator_amd.engine.llm import GenRequest, LLMEngine
from operator_amd.models.config import get_config
from operator_amd.models.kv_cache import PagedKVCache
from operator_amd.models.llama import ForwardBatch, LlamaModel

pytestmark = pytest.mark.gpu


def _cpu_copy(m: LlamaModel) -> LlamaModel:
    c = LlamaModel(m.cfg, device="cpu", dtype=torch.float32)
    c.embed, c.final_norm, c.lm_head = m.embed.float().cpu(), m.final_norm.float().cpu(), m.lm_head.float().cpu()
    from operator_amd.models.llama import LayerWeights
    c.layers = [LayerWeights(*(t.float().cpu() for t in (l.wqkv, l.wo, l.wgu, l.wd, l.attn_norm, l.mlp_norm)),
                             bqkv=None if l.bqkv is None else l.bqkv.float().cpu())
                for l in m.layers]
    return c


@pytest.mark.parametrize("name", ["tiny-gqa4", "tiny-qwen"])
def test_prefill_logits_match_cpu_reference(name):
    cfg = get_config(name)
    g = LlamaModel(cfg, device="cuda").init_random(seed=3)
    c = _cpu_copy(g)
    kv_g = PagedKVCache(cfg.layers, 32, cfg.kv_heads, 128, 16, device="cuda")
    kv_c = PagedKVCache(cfg.layers, 32, cfg.kv_heads, 128, 16, device="cpu", dtype=torch.float32)
    lens = [33, 70]
    ids = torch.randint(0, cfg.vocab_size, (sum(lens),))
    pos = torch.cat([torch.arange(L) for L in lens])
    last = torch.tensor([lens[0] - 1, sum(lens) - 1])
    slots = torch.full((sum(lens),), -1, dtype=torch.long)
    fb_g = ForwardBatch(ids.cuda(), pos.cuda(), slots.cuda(), True, last.cuda(), seq_lens=lens)
    fb_c = ForwardBatch(ids, pos, slots, True, last, seq_lens=lens)
    lg = g.forward(fb_g, kv_g).float().cpu()
    lc = c.forward(fb_c, kv_c)
    # bf16 weights/activations vs fp32: compare with a relative-to-scale tolerance
    err = (lg - lc).abs().max() / lc.abs().max()
    assert err < 0.05, float(err)
    assert (lg.argmax(-1) == lc.argmax(-1)).float().mean() >= 0.5


def test_graph_decode_equals_eager_decode():
    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=5)
    outs = []
    for graphs in (False, True):
        kv = PagedKVCache(cfg.layers, 128, cfg.kv_heads, 128, 16, device="cuda")
        eng = LLMEngine(m, kv, max_batch=8, max_context=1024, use_graphs=graphs)
        reqs = [GenRequest(list(range(1, 1 + n)), max_tokens=20, temperature=t, seed=s, ignore_eos=True)
                for n, t, s in [(5, 0.0, 0), (300, 0.7, 1), (17, 0.3, 2)]]
        eng.generate(reqs)
        outs.append([r.output for r in reqs])
        assert kv.allocator.free + eng.prefix_pages == kv.num_pages
    assert outs[0] == outs[1]


def test_llama3_8b_architecture_smoke():
    cfg = get_config("llama3-8b")
    m = LlamaModel(cfg, device="cuda").init_random(seed=0)
    assert abs(m.weight_bytes() - 2 * cfg.param_count()) < 1e6
    kv = PagedKVCache(cfg.layers, 256, cfg.kv_heads, 128, 64, device="cuda")
    eng = LLMEngine(m, kv, max_batch=4, max_context=2048, use_graphs=True)
    reqs = [GenRequest(list(range(100, 100 + n)), max_tokens=6, temperature=0.3, seed=n, ignore_eos=True)
            for n in (64, 200)]
    eng.generate(reqs)
    for r in reqs:
        assert len(r.output) == 6 and all(0 <= t < cfg.vocab_size for t in r.output)


def test_llama3_8b_prefill_and_greedy_decode_track_fp32_reference():
    """SURVEY.md §4.2 'Model end-to-end, GPU' at the flagship size: Llama-3-8B
    random-init on the gfx950 kernels (hipBLASLt prefill GEMMs, MFMA flash prefill,
    paged decode attention, decode GEMMs, hipGraph decode) against the fp32 PyTorch
    reference path of the same weights on the host.
      * prefill logits: max error within 5 % of the logit scale, argmax agreement;
      * 32 greedy decode steps: every token the engine picks is the reference's argmax
        at that position, or within a bf16-sized gap of it (a near-tie), and nearly all
        are exact."""
    cfg = get_config("llama3-8b")
    torch.manual_seed(0)
    g = LlamaModel(cfg, device="cuda").init_random(seed=1)
    prompt = torch.randint(0, cfg.vocab_size, (48,)).tolist()
    kv = PagedKVCache(cfg.layers, 16, cfg.kv_heads, 128, 64, device="cuda")
    eng = LLMEngine(g, kv, max_batch=4, max_context=256, use_graphs=True)
    req = GenRequest(list(prompt), max_tokens=32, temperature=0.0, ignore_eos=True)
    eng.generate([req])
    assert len(req.output) == 32 and eng.stats.graph_replays > 0
    # GPU prefill logits of the whole prompt + generated sequence (every position)
    seq = prompt + req.output
    T = len(seq)
    ids = torch.tensor(seq)
    fb = ForwardBatch(ids.cuda(), torch.arange(T).cuda(), torch.full((T,), -1, dtype=torch.long).cuda(), True,
                      torch.arange(T).cuda(), seq_lens=[T])
    kv_g = PagedKVCache(cfg.layers, 8, cfg.kv_heads, 128, 64, device="cuda")
    lg = g.forward(fb, kv_g).float().cpu()
    del kv, kv_g, eng
    c = _cpu_copy(g)
    del g
    torch.cuda.empty_cache()
    kv_c = PagedKVCache(cfg.layers, 8, cfg.kv_heads, 128, 64, device="cpu", dtype=torch.float32)
    fb_c = ForwardBatch(ids, torch.arange(T), torch.full((T,), -1, dtype=torch.long), True, torch.arange(T),
                        seq_lens=[T])
    with torch.inference_mode():
        lc = c.forward(fb_c, kv_c)
    scale = lc.abs().max()
    assert float((lg - lc).abs().max() / scale) < 0.05
    assert (lg.argmax(-1) == lc.argmax(-1)).float().mean() >= 0.9
    # decode: the token chosen after position p is judged by the reference logits at p
    pos = torch.arange(len(prompt) - 1, T - 1)
    chosen = torch.tensor(req.output)
    ref_rows = lc[pos]
    gap = ref_rows.max(-1).values - ref_rows.gather(1, chosen[:, None])[:, 0]
    exact = (ref_rows.argmax(-1) == chosen).float().mean()
    assert float(gap.max() / scale) < 0.02, gap.tolist()
    assert exact >= 0.85, float(exact)
    del c, kv_c, lc, lg
    import gc

    gc.collect()


def test_graph_capture_with_dead_cycles_holding_multi_stream_tensors():
    """Regression: a Python GC pass inside a hipGraph capture that frees a dead cycle's
    tensor last used on another stream records an event on that stream mid-capture
    (a process abort). The engine collects before capturing and holds GC off during
    it; here collection is forced to run on almost every allocation."""
    import gc

    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=7)
    side = torch.cuda.Stream()

    class Node:
        pass

    for _ in range(64):   # dead cycles, each holding a tensor with a use on `side`
        a, b = Node(), Node()
        a.o, b.o = b, a
        a.t = torch.ones(1 << 16, device="cuda")
        with torch.cuda.stream(side):
            a.t.mul_(2)
        a.t.record_stream(side)
    del a, b
    old = gc.get_threshold()
    gc.set_threshold(1, 1, 1)
    try:
        kv = PagedKVCache(cfg.layers, 64, cfg.kv_heads, 128, 16, device="cuda")
        eng = LLMEngine(m, kv, max_batch=4, max_context=512, use_graphs=True, multi_step=2)
        reqs = [GenRequest(list(range(2, 2 + n)), max_tokens=6, temperature=0.0, ignore_eos=True) for n in (7, 30)]
        eng.generate(reqs)
    finally:
        gc.set_threshold(*old)
    torch.cuda.synchronize()
    assert all(len(r.output) == 6 for r in reqs) and eng.stats.graph_replays > 0


def test_pipelined_windows_eos_and_arrivals():
    """Pipelined multi-step decode windows (graphs) must produce exactly the eager
    engine's tokens with staggered lengths, EOS inside a window and requests that
    arrive while others decode."""
    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=6)

    def run(graphs, eos):
        kv = PagedKVCache(cfg.layers, 256, cfg.kv_heads, 128, 16, device="cuda")
        eng = LLMEngine(m, kv, max_batch=8, max_context=1024, use_graphs=graphs, multi_step=4)
        if eos is not None:
            eng.eos = {eos}
        first = [GenRequest(list(range(3, 3 + n)), max_tokens=mt, temperature=0.8, seed=s)
                 for n, mt, s in [(9, 30, 0), (40, 7, 1), (120, 19, 2)]]
        late = [GenRequest(list(range(50, 50 + n)), max_tokens=mt, temperature=0.8, seed=s)
                for n, mt, s in [(33, 11, 3), (5, 26, 4)]]
        for r in first:
            eng.submit(r)
        for _ in range(3):
            eng.step()
        for r in late:
            eng.submit(r)
        while any(not r.done for r in first + late):
            eng.step()
        assert kv.allocator.free + eng.prefix_pages == kv.num_pages
        return [r.output for r in first + late]

    base = run(False, None)
    assert run(True, None) == base
    eos = base[0][12]  # a token request 0 samples mid-stream: EOS inside a window
    ref = run(False, eos)
    assert len(ref[0]) == 13
    assert run(True, eos) == ref


def test_fp8_weights_model_runs_and_tracks_bf16():
    cfg = get_config("tiny-gqa4")
    outs = {}
    for wd in ("bfloat16", "fp8"):
        m = LlamaModel(cfg, device="cuda", weight_dtype=wd).init_random(seed=11)
        kv = PagedKVCache(cfg.layers, 64, cfg.kv_heads, 128, 16, device="cuda")
        T = 48
        fb = ForwardBatch(torch.arange(T, device="cuda"), torch.arange(T, device="cuda"),
                          torch.full((T,), -1, dtype=torch.long, device="cuda"), True, None, seq_lens=[T],
                          prefill_work=None)
        outs[wd] = m.forward(fb, kv).float()
        eng = LLMEngine(m, kv, max_batch=4, max_context=512, use_graphs=True)
        reqs = [GenRequest(list(range(2, 40)), max_tokens=9, temperature=0.5, seed=1, ignore_eos=True)]
        eng.generate(reqs)
        assert len(reqs[0].output) == 9
    cos = torch.nn.functional.cosine_similarity(outs["fp8"].flatten(), outs["bfloat16"].flatten(), dim=0)
    assert cos > 0.98, float(cos)


@pytest.mark.parametrize("wd", ["bfloat16", "fp8"])
def test_weight_cache_maps_shard_onto_the_gpu(tmp_path, wd):
    """A model started from the weight cache (safetensors mmapped straight to the device)
    computes exactly what the freshly built one does."""
    from operator_amd.models import weight_cache

    cfg = get_config("tiny-gqa4")
    outs = []
    for expect in ("miss", "hit"):
        m = LlamaModel(cfg, device="cuda", weight_dtype=wd)
        assert weight_cache.load_or_build(m, str(tmp_path), None, 11) == expect
        assert m.embed.is_cuda and m.layers[0].wqkv.is_cuda
        kv = PagedKVCache(cfg.layers, 64, cfg.kv_heads, 128, 16, device="cuda")
        T = 40
        fb = ForwardBatch(torch.arange(T, device="cuda"), torch.arange(T, device="cuda"),
                          torch.full((T,), -1, dtype=torch.long, device="cuda"), True, None, seq_lens=[T],
                          prefill_work=None)
        outs.append(m.forward(fb, kv))
    assert torch.equal(outs[0], outs[1])


def test_graph_prefill_equals_eager_prefill():
    """A prefill replayed from a captured bucket graph (tokens padded to the bucket,
    padding slots -1, padding attention items -1) writes the same KV cache and samples
    the same tokens as the eager prefill; a 3-token batch replays the smallest (512) bucket."""
    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=7)
    lens = [400, 350, 30, 170]          # 950 tokens: bucket 1024 (7 % padding)
    outs, caches, replays = [], [], []
    for pg in (False, True):
        kv = PagedKVCache(cfg.layers, 256, cfg.kv_heads, 128, 16, device="cuda")
        eng = LLMEngine(m, kv, max_batch=8, max_prefill_tokens=1024, max_context=1024, use_graphs=True,
                        prefill_graphs=pg)
        eng.warmup([8])
        reqs = [GenRequest(list(range(3, 3 + n)), max_tokens=12, temperature=t, seed=i, ignore_eos=True)
                for i, (n, t) in enumerate(zip(lens, (0.0, 0.5, 0.0, 1.0)))]
        for r in reqs:
            eng.submit(r)
        eng.step()                       # the one prefill of all four
        caches.append(torch.stack([kv.layer(i)[0].float() for i in range(cfg.layers)]).cpu())
        while any(not r.done for r in reqs):
            eng.step()
        outs.append([r.output for r in reqs])
        replays.append(eng.stats.prefill_graph_replays)
        small = [GenRequest([5, 6, 7], max_tokens=2, ignore_eos=True)]   # 3 tokens: bucket 512
        eng.generate(small)
        assert eng.stats.prefill_graph_replays == replays[-1] + pg
        assert eng.stats.prefill_eager == (0 if pg else 2)
    assert replays == [0, 1]
    assert outs[0] == outs[1]
    assert torch.equal(caches[0], caches[1])


@pytest.mark.parametrize("B", [3, 64])
def test_qwen_decode_step_matches_cpu_reference(B):
    """Qwen2-shaped decode (q/k/v bias, GQA group 7): one paged decode step after a
    prefill, GPU kernels vs the fp32 CPU path. B = 64 takes the split-K decode GEMM
    whose slabs carry the bias into rope_kv; B = 3 the skinny bf16 path."""
    cfg = get_config("tiny-qwen")
    g = LlamaModel(cfg, device="cuda").init_random(seed=9)
    c = _cpu_copy(g)
    P, per = 16, 4
    lens = [(7 * i) % 50 + 3 for i in range(B)]
    out = []
    for m, dev, dt in ((g, "cuda", torch.bfloat16), (c, "cpu", torch.float32)):
        kv = PagedKVCache(cfg.layers, B * per, cfg.kv_heads, 128, P, device=dev, dtype=dt)
        bt = torch.arange(B * per, dtype=torch.int32).reshape(B, per)
        ids = [torch.randint(0, cfg.vocab_size, (L,), generator=torch.Generator().manual_seed(i))
               for i, L in enumerate(lens)]
        pos = torch.cat([torch.arange(L) for L in lens])
        slots = torch.cat([bt[i, torch.arange(L) // P].long() * P + torch.arange(L) % P for i, L in enumerate(lens)])
        fb = ForwardBatch(torch.cat(ids).to(dev), pos.to(dev), slots.to(dev), True,
                          torch.tensor([0]).to(dev), seq_lens=lens)
        m.forward(fb, kv)
        nxt = torch.tensor([int(x[-1]) for x in ids])
        dpos = torch.tensor(lens)
        dslots = torch.stack([bt[i, L // P].long() * P + L % P for i, L in enumerate(lens)])
        fb = ForwardBatch(nxt.to(dev), dpos.to(dev), dslots.to(dev), False, None, block_tables=bt.to(dev),
                          context_lens=(dpos + 1).int().to(dev), num_splits=1)
        out.append(m.forward(fb, kv).float().cpu())
    err = (out[0] - out[1]).abs().max() / out[1].abs().max()
    assert err < 0.05, float(err)


def test_fp8_kv_cache_engine_tracks_bf16_cache():
    """Llama decode with an e4m3fn KV cache through the graph engine: the first decode
    logits track the bf16 cache's and the engine runs windows with graphs."""
    cfg = get_config("tiny-gqa4")
    m = LlamaModel(cfg, device="cuda").init_random(seed=13)
    lens = [37, 210, 5]
    outs, toks = {}, {}
    for dt in (torch.bfloat16, torch.float8_e4m3fn):
        kv = PagedKVCache(cfg.layers, 64, cfg.kv_heads, 128, 16, device="cuda", dtype=dt)
        P, per = 16, 16
        B = len(lens)
        bt = torch.arange(B * per, dtype=torch.int32).reshape(B, per)
        ids = [torch.arange(3, 3 + L) for L in lens]
        pos = torch.cat([torch.arange(L) for L in lens])
        slots = torch.cat([bt[i, torch.arange(L) // P].long() * P + torch.arange(L) % P for i, L in enumerate(lens)])
        m.forward(ForwardBatch(torch.cat(ids).cuda(), pos.cuda(), slots.cuda(), True, torch.tensor([0]).cuda(),
                               seq_lens=lens), kv)
        dpos = torch.tensor(lens)
        dslots = torch.stack([bt[i, L // P].long() * P + L % P for i, L in enumerate(lens)])
        fb = ForwardBatch(torch.tensor([7, 8, 9]).cuda(), dpos.cuda(), dslots.cuda(), False, None,
                          block_tables=bt.cuda(), context_lens=(dpos + 1).int().cuda(), num_splits=1)
        outs[dt] = m.forward(fb, kv).float()
        kv2 = PagedKVCache(cfg.layers, 128, cfg.kv_heads, 128, 16, device="cuda", dtype=dt)
        eng = LLMEngine(m, kv2, max_batch=4, max_context=1024, use_graphs=True)
        r = eng.generate([GenRequest(list(range(2, 90)), max_tokens=20, temperature=0.0, ignore_eos=True)])[0]
        assert len(r.output) == 20 and eng.stats.graph_replays > 0
        toks[dt] = r.output
    cos = torch.nn.functional.cosine_similarity(outs[torch.bfloat16].flatten(), outs[torch.float8_e4m3fn].flatten(),
                                                dim=0)
    assert cos > 0.99, float(cos)


@pytest.mark.parametrize("prefill_blas", [False, True])
def test_llama3_8b_shapes_never_fall_back_to_hipblaslt(monkeypatch, prefill_blas):
    """Every GEMM of the Llama-3-8B shapes runs where it is planned to: with
    OAMD_FORBID_BLAS=1 any hipBLASLt FALLBACK raises. Two layers of the real architecture,
    prefill batches of 1k and 4k packed tokens (tails included) and the M = 64 / 256
    decode buckets. With ops.gemm.PREFILL_BLAS the plain prefill projections (QKV, O, down:
    3 per layer and batch) are planned hipBLASLt calls and nothing else is; without it
    every GEMM runs on the gfx950 kernels."""
    from dataclasses import replace

    from operator_amd import ops

    monkeypatch.setenv("OAMD_FORBID_BLAS", "1")
    monkeypatch.setattr(ops.gemm, "PREFILL_BLAS", prefill_blas)
    cfg = replace(get_config("llama3-8b"), layers=2)
    m = LlamaModel(cfg, device="cuda").init_random(seed=3)
    kv = PagedKVCache(cfg.layers, 128, cfg.kv_heads, 128, 64, device="cuda")
    n0, p0 = ops.BLAS_CALLS["n"], ops.BLAS_PLANNED["n"]
    for lens in ([1024], [700, 1300, 2096]):
        T = sum(lens)
        ids = torch.randint(0, cfg.vocab_size, (T,), device="cuda")
        pos = torch.cat([torch.arange(n) for n in lens]).cuda()
        last = torch.tensor(lens).cumsum(0).cuda() - 1
        fb = ForwardBatch(ids, pos, torch.full((T,), -1, dtype=torch.long, device="cuda"), True, last, seq_lens=lens)
        lg = m.forward(fb, kv)
        assert lg.shape == (len(lens), cfg.vocab_size) and torch.isfinite(lg.float()).all()
    assert ops.BLAS_PLANNED["n"] - p0 == (2 * 2 * 3 if prefill_blas else 0)
    eng = LLMEngine(m, kv, max_batch=256, max_context=512, use_graphs=False)
    p1 = ops.BLAS_PLANNED["n"]
    for B in (64, 256):
        reqs = [GenRequest(list(range(1, 17)), max_tokens=2, temperature=0.0, ignore_eos=True) for _ in range(B)]
        eng.generate(reqs)
        assert all(len(r.output) == 2 for r in reqs)
    assert ops.BLAS_CALLS["n"] == n0
    # decode never plans hipBLASLt; the engine's prefills (64 x 16 and 256 x 16 tokens: > 256
    # rows) do, 3 projections x 2 layers per prefill batch
    d = ops.BLAS_PLANNED["n"] - p1
    assert (d >= 2 * 6 and d % 6 == 0) if prefill_blas else d == 0
