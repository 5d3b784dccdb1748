"""What top-k / top-p cost on the decode step's sampler: 256 rows x 128256 bf16 logits
(Llama-3 lm_head output), four arms interleaved round by round in one process, median and
minimum of the rounds' microseconds per call.

  plain         ops.sample as before the filter existed (what a step used to launch)
  defaults      sample_threshold + filtered sampler, every row at top_k 0 / top_p 1: what
                every decode step launches now (the threshold kernel leaves at once)
  top_p         every row top_p = 0.9
  top_k+top_p   every row top_k = 40, top_p = 0.9

defaults - plain is what an existing decode step pays; the last two are the price of the
feature. One JSON line per arm on stdout (and appended to --out).

--penalties measures the repetition / frequency / presence penalty kernel the same way, three
arms: the defaults step; the same behind sample_penalty with no row holding a slot (what every
decode step launches now); the same with every row penalised over --seen distinct tokens.

--logprobs measures the log-probability kernel behind the sampler the same way, four arms: the
defaults step; the same followed by sample_logprobs with every row off (what every decode step
launches now); with every row asking for its token's value only (N = 0); with every row asking
for 20 alternatives.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from operator_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--vocab", type=int, default=128256)
ap.add_argument("--scale", type=float, default=3.0, help="logit std (a trained model's rows are peaked)")
ap.add_argument("--temperature", type=float, default=0.8)
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--calls", type=int, default=20, help="calls per arm per round")
ap.add_argument("--out", default=None)
ap.add_argument("--penalties", action="store_true",
                help="the penalty arms in place of the filter arms: the defaults step, the same behind the "
                     "penalty kernel with every row off, and with every row on")
ap.add_argument("--logprobs", action="store_true",
                help="the log-probability arms in place of the filter arms: the defaults step, the same followed by "
                     "the logprob kernel with every row off, every row at N = 0, every row at N = 20")
ap.add_argument("--seen", type=int, default=1100, help="distinct seen tokens per row of the rows-on arm")
a = ap.parse_args()

B = a.batch
x = (torch.randn(B, a.vocab, device="cuda") * a.scale).to(torch.bfloat16)
t = torch.full((B,), a.temperature, device="cuda")
sd = torch.arange(B, device="cuda")
ps = torch.arange(B, device="cuda")
out = torch.empty(B, dtype=torch.long, device="cuda")
thr = torch.empty(B, dtype=torch.float32, device="cuda")


def filt(k, p):
    return dict(top_k=torch.full((B,), k, dtype=torch.int32, device="cuda"),
                top_p=torch.full((B,), p, dtype=torch.float32, device="cuda"), thr=thr)


def penalty_arm(on: bool):
    """The decode step's count-and-apply kernel in front of the defaults step: every row
    without a slot (what a step with no penalised request pays), or every row with its own
    slot holding --seen distinct tokens (the flagship's context) at r 1.1, f 0.2, p 0.3. The
    token fed in is one already listed, so every call walks a list of the same length."""
    from operator_amd.models.penalty import PenaltyTable

    tb = PenaltyTable(B, a.vocab, a.seen + 64, device="cuda")
    g = torch.Generator().manual_seed(1)
    for s in range(B):
        toks = torch.randperm(a.vocab, generator=g)[:a.seen].to(torch.int32).cuda()
        tb.lst[s, :a.seen] = toks
        tb.cnt[s, toks.long()] = 3
    tb.n.fill_(a.seen)
    pslot = (torch.arange(B, dtype=torch.int32) if on else torch.full((B,), -1, dtype=torch.int32)).cuda()
    last = tb.lst[:, 0].long().contiguous()
    ctx = torch.full((B,), 1100, dtype=torch.int32, device="cuda")
    rep, freq, pres = (torch.full((B,), v, dtype=torch.float32, device="cuda") for v in (1.1, 0.2, 0.3))
    return lambda: ops.sample_penalty(x, pslot, last, ctx, rep, freq, pres, tb)


def logprob_arm(n: int):
    """sample_logprobs behind the defaults step as a decode graph runs it (the device step counter,
    eight columns, every row live by its context length), every row asking for ``n``."""
    C, L = 8, ops.LOGPROBS_MAX
    nlp = torch.full((B,), n, dtype=torch.int32, device="cuda")
    ctx = torch.full((B,), 1100, dtype=torch.int32, device="cuda")
    step = torch.full((1,), 3, dtype=torch.long, device="cuda")
    tok_lp = torch.zeros(B, C, dtype=torch.float32, device="cuda")
    top_lp = torch.zeros(B, C, L, dtype=torch.float32, device="cuda")
    top_id = torch.zeros(B, C, L, dtype=torch.int32, device="cuda")
    return lambda: ops.sample_logprobs(x, nlp, ctx, out, step, tok_lp, top_lp, top_id)


post = {}   # arm -> what runs behind the sampler
if a.logprobs:
    bench = "sampler_logprobs"
    arms = {n: (None, filt(0, 1.0)) for n in ("defaults", "logprob_kernel_rows_off", "logprob_rows_n0", "logprob_rows_n20")}
    post = {"logprob_kernel_rows_off": logprob_arm(-1), "logprob_rows_n0": logprob_arm(0),
            "logprob_rows_n20": logprob_arm(20)}
elif a.penalties:
    bench = "sampler_penalty"
    arms = {"defaults": (None, filt(0, 1.0)), "penalty_kernel_rows_off": (penalty_arm(False), filt(0, 1.0)),
            f"penalty_rows_on_{a.seen}_seen": (penalty_arm(True), filt(0, 1.0))}
else:
    bench = "sampler_filter"
    arms = {"plain": (None, {}), "defaults": (None, filt(0, 1.0)), "top_p": (None, filt(0, 0.9)),
            "top_k+top_p": (None, filt(40, 0.9))}


def call(pre, kw, after=None):
    if pre is not None:
        pre()
    ops.sample(x, t, sd, ps, out=out, **kw)
    if after is not None:
        after()


for n, (pre, kw) in arms.items():
    for _ in range(3):
        call(pre, kw, post.get(n))
torch.cuda.synchronize()
us = {n: [] for n in arms}
for _ in range(a.rounds):
    for n, (pre, kw) in arms.items():
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(a.calls):
            call(pre, kw, post.get(n))
        e1.record()
        torch.cuda.synchronize()
        us[n].append(e0.elapsed_time(e1) / a.calls * 1e3)
for n, v in us.items():
    line = json.dumps({"bench": bench, "arm": n, "batch": B, "vocab": a.vocab, "scale": a.scale,
                       "temperature": a.temperature, "rounds": a.rounds, "calls_per_round": a.calls,
                       "us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1),
                       "us_max": round(max(v), 1)})
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
