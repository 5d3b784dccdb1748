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


arms = {"plain": {}, "defaults": filt(0, 1.0), "top_p": filt(0, 0.9), "top_k+top_p": filt(40, 0.9)}
for kw in arms.values():
    for _ in range(3):
        ops.sample(x, t, sd, ps, out=out, **kw)
torch.cuda.synchronize()
us = {n: [] for n in arms}
for _ in range(a.rounds):
    for n, kw in arms.items():
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(a.calls):
            ops.sample(x, t, sd, ps, out=out, **kw)
        e1.record()
        torch.cuda.synchronize()
        us[n].append(e0.elapsed_time(e1) / a.calls * 1e3)
for n, v in us.items():
    line = json.dumps({"bench": "sampler_filter", "arm": n, "batch": B, "vocab": a.vocab, "scale": a.scale,
                       "temperature": a.temperature, "rounds": a.rounds, "calls_per_round": a.calls,
                       "us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1),
                       "us_max": round(max(v), 1)})
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
