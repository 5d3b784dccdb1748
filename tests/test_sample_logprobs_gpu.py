"""sample_logprobs (csrc/kernels/logprob.hip) against the fp64, sort-based reference
(ops/reference.py sample_logprobs) on the semantics of docs/PARITY.md "Sampling: logprobs".

Token ids are compared as integers. Every output element the semantics leave alone (list entries
from nlp up to 20, the other columns, rows that are off or padding) is compared bit for bit with
the canary the buffers were filled with. Log-probabilities: infinities and NaNs equal as classes,
finite values within TOL = 1e-4 absolute of the reference, which is computed from the same
rounded logits.

Where the 1e-4 comes from: x_t and the maximum are exact, so the error is that of ln(sum). A
thread of the 1024 adds its terms in walk order, at most about 150 of them at a 128k vocabulary
(at most 48 at the largest shape here), then the sum goes through a 6-level wave butterfly and a
4-level tree over the 16 wave sums: about 170 roundings, a relative error of about 170 * 2^-24
~ 1e-5 on the sum. Add 1 ulp per hardware exp2 / log and the 2e-6 spacing of an fp32 near 30:
about 2e-5 in all, and the tolerance is 5 x that.
"""
import functools
import math

import pytest
import torch

from operator_amd import ops
from operator_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
LAYOUTS = ["contig", "aligned", "unaligned"]
SHAPES = [(BF16, 1), (BF16, 7), (BF16, 8), (BF16, 1003), (BF16, 41003), (F32, 7), (F32, 1003)]
NMAX = 20
C = 4
TOL = 1e-4
CANARY = 12345.0
CANARY_ID = -777
NLP = [-1, 0, 1, 5, 20]
STEPS = [None, 0, C - 1, C + 3]
TIE_SEED = 3   # the bf16 row of 41003 normals whose N = 20 cut falls inside a group of equal logits
KINDS = ["normal", "constant", "ties", "inf1", "inf2", "neginf_tail", "nans", "zeros", "all_nan", "all_neginf"]


def _rows(dtype, V):
    """One row per entry of KINDS."""
    g = torch.Generator().manual_seed(1000 + V)
    inf, nan = math.inf, math.nan
    x = (torch.randn(len(KINDS), V, generator=g) * 4).to(dtype)
    x[1] = 1.5
    x[2] = torch.randn(V, generator=torch.Generator().manual_seed(TIE_SEED)).to(dtype)
    x[3, V // 2] = inf
    x[4, V // 3] = inf
    x[4, V - 1] = inf
    x[5, (V + 2) // 3:] = -inf
    x[6, ::3] = nan                       # column 0 among them
    if V > 4:
        x[6, V - 2] = nan
    x[7] = (torch.randn(V, generator=g) - 30).to(dtype)   # all negative: the zeros are the maximum
    for i, z in zip(range(V // 2, V), [-0.0, 0.0, -0.0, 0.0]):
        x[7, i] = z
    if V > 2:
        x[7, 0] = 0.0
    x[8] = nan
    x[9] = -inf
    return x


@functools.lru_cache(maxsize=None)
def _case(dtype, V):
    """The launches of one shape, shared by the layouts: (rows of _rows, nlp, ctx | None, tokens,
    step | None) and what the reference leaves in canary-filled outputs."""
    x = _rows(dtype, V)
    K = len(KINDS)
    launches = []

    def add(kinds, nlp, ctx, tokens, step):
        R = len(kinds)
        lg = x[kinds].clone()
        nlp_t = torch.tensor(nlp, dtype=I32)
        ctx_t = None if ctx is None else torch.tensor(ctx, dtype=I32)
        tok_t = torch.tensor(tokens, dtype=torch.long)
        step_t = None if step is None else torch.tensor([step], dtype=torch.long)
        tok_lp = torch.full((R, C), CANARY, dtype=F32)
        top_lp = torch.full((R, C, NMAX), CANARY, dtype=F32)
        top_id = torch.full((R, C, NMAX), CANARY_ID, dtype=I32)
        ref.sample_logprobs(lg, nlp_t, ctx_t, tok_t, step_t, tok_lp, top_lp, top_id)
        col = 0 if step is None else step % C
        touched = torch.zeros(R, C, NMAX + 1, dtype=torch.bool)   # [..., 0]: tok_lp, [..., 1:]: the list
        for r in range(R):
            if nlp[r] >= 0 and (ctx is None or ctx[r] != 0):
                touched[r, col, :1 + nlp[r]] = True
        launches.append((lg, nlp_t, ctx_t, tok_t, step_t, tok_lp, top_lp, top_id, touched))

    n = 0
    for grp in (list(range(0, 5)), list(range(5, K))):
        for rot in range(5):     # every kind meets every nlp value
            nlp = [NLP[(i + rot) % 5] for i in range(5)]
            ctx = None
            if rot in (1, 3):    # a padding row that asks for 20 (rot 1) / 5 (rot 3) entries
                ctx = [7] * 5
                ctx[(rot + 2) % 5] = 0
            tokens = [(rot * 7919 + k * 31 + 1) % V for k in grp]
            if rot == 0:
                tokens = [int(torch.argmax(torch.nan_to_num(x[k].float(), nan=-math.inf))) for k in grp]   # the greedy token
            if rot == 2 and 6 in grp:
                tokens[grp.index(6)] = 0   # a NaN logit
            add(grp, nlp, ctx, tokens, STEPS[n % 4])
            n += 1
    for k in range(K):           # one row per launch, N = 20 (> vocab at the small shapes)
        add([k], [20], None if k % 2 else [3], [(k * 131 + 5) % V], STEPS[(k + 1) % 4])
    add([0], [-1], None, [0], 1)
    add([0], [7], [0], [0], None)
    return launches


def _place(logits, layout):
    """The rows on the GPU: as they are, at a stride that is a multiple of 16 bytes, or the same
    one element in. Outside the rows the buffer holds CANARY."""
    R, V = logits.shape
    if layout == "contig":
        return logits.cuda()
    stride = (V + 1 + 7) // 8 * 8 + 8
    buf = torch.full((R, stride), CANARY, dtype=logits.dtype)
    c0 = 0 if layout == "aligned" else 1
    buf[:, c0:c0 + V] = logits
    view = buf.cuda()[:, c0:c0 + V]
    assert (view.data_ptr() % 16 == 0) == (layout == "aligned")
    return view


def _run(view, nlp, ctx, tok, step):
    R = view.shape[0]
    tok_lp = torch.full((R, C), CANARY, dtype=F32, device="cuda")
    top_lp = torch.full((R, C, NMAX), CANARY, dtype=F32, device="cuda")
    top_id = torch.full((R, C, NMAX), CANARY_ID, dtype=I32, device="cuda")
    ops.sample_logprobs(view, nlp.cuda(), None if ctx is None else ctx.cuda(), tok.cuda(),
                        None if step is None else step.cuda(), tok_lp, top_lp, top_id)
    torch.cuda.synchronize()
    return tok_lp.cpu(), top_lp.cpu(), top_id.cpu()


def _check_lp(got, want, touched, what):
    same_bits = got.view(I32) == want.view(I32)
    assert bool(same_bits[~touched].all()), f"{what}: an element outside the written ones lost its canary"
    g, w = got[touched].double(), want[touched].double()
    fin = torch.isfinite(w)
    assert torch.equal(torch.isfinite(g), fin), f"{what}: finite / non-finite classes differ: {g} vs {w}"
    assert torch.equal(torch.isnan(g), torch.isnan(w)), f"{what}: NaN classes differ: {g} vs {w}"
    assert torch.equal(g[~fin & ~torch.isnan(w)], w[~fin & ~torch.isnan(w)]), f"{what}: infinities differ"
    err = (g[fin] - w[fin]).abs()
    print(f"{what}: {int(fin.sum())} finite, max abs error {float(err.max()) if err.numel() else 0.0:.3g}")
    assert bool((err <= TOL).all()), f"{what}: max abs error {float(err.max()):.3g} > {TOL}"


def test_tie_row_cut_is_inside_a_tie_group():
    """The seed of the "ties" row is chosen so that its 20th and 21st largest bf16 logits are equal."""
    s = torch.sort(_rows(BF16, 41003)[2].float(), descending=True).values
    assert s[19] == s[20]
    assert s[0] > s[19]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype,V", SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_matches_reference(dtype, V, layout):
    for i, (lg, nlp, ctx, tok, step, w_tok, w_lp, w_id, touched) in enumerate(_case(dtype, V)):
        view = _place(lg, layout)
        g_tok, g_lp, g_id = _run(view, nlp, ctx, tok, step)
        what = f"launch {i} (nlp {nlp.tolist()}, step {None if step is None else int(step)})"
        assert torch.equal(g_id, w_id), f"{what}: top_id differs:\n{g_id[g_id != w_id]}\n{w_id[g_id != w_id]}"
        _check_lp(g_lp, w_lp, touched[..., 1:], what + " top_lp")
        _check_lp(g_tok, w_tok, touched[..., 0], what + " tok_lp")


@pytest.mark.parametrize("dtype,V", SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_two_launches_give_the_same_bytes(dtype, V):
    for lg, nlp, ctx, tok, step, *_ in _case(dtype, V)[:10]:
        view = _place(lg, "contig")
        a = _run(view, nlp, ctx, tok, step)
        b = _run(view, nlp, ctx, tok, step)
        for u, v in zip(a, b):
            assert torch.equal(u.view(I32), v.view(I32))


def test_greedy_token_is_entry_zero():
    """A row with a single maximum: the greedy token is entry 0 and carries the same value."""
    lg = _rows(BF16, 1003)[:1]
    top = int(torch.argmax(lg[0].float()))
    assert int((lg[0] == lg[0, top]).sum()) == 1
    g_tok, g_lp, g_id = _run(lg.cuda(), torch.tensor([5], dtype=I32), None, torch.tensor([top]), None)
    assert int(g_id[0, 0, 0]) == top
    assert torch.equal(g_tok[0, 0].view(I32), g_lp[0, 0, 0].view(I32))


def test_list_length_is_one_constant():
    assert ops.kernels().LOGPROBS_MAX == ops.LOGPROBS_MAX == ref.LOGPROBS_MAX == NMAX
