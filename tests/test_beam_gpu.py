"""GPU: beam search (DESIGN.md "Beam search").  rwkv7_beam_select bit for bit against the plain reference of tests/beam_ref.py (the
hand-made tables, random tables for one group and for three groups of different W and S in one launch); rwkv7_beam_copy_states bit
for bit against torch indexing (NaN payloads, infinities, -0; every slot that is no destination unchanged; the 7.2B geometry); then
the real Worker on the L2/C128 golden model and the 0.1B synthetic model, graph and eager, run-ahead and in-step: the contract
replayed on the host from each step's downloaded candidate tables reproduces the worker's parents, ids, scores, finished records and
hypotheses exactly; children of one parent hold identical states; a neighbouring greedy request is not disturbed; and the returned
hypotheses are re-scored through the prompt-logprobs path.

Run as a program it prints the measurement behind tests/golden/beam_bars.json (profiles/r08_beam_rescoring.txt)."""
import json
import os
import queue
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import beam_ref  # noqa: E402
from chirrup_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB = {"L2C128": 320, "0.1B": 65536}
SPECIAL = [0x7E01, 0xFE7F, 0x7C00, 0xFC00, 0x8000, 0x0000, 0xFFFF, 0x7C01, 0x0001]     # NaN payloads, +-inf, -0, 0, a subnormal


# ------------------------------------------------------------------------------------------------------------ the select kernel
def _select(cases, **kw):
    from test_beam_cpu import _run_select, assert_bits_equal

    nxt = [0]

    def slots_of(g, W):                                     # distinct slots over all groups of the launch
        nxt[0] += W
        return list(range(nxt[0] - W, nxt[0]))

    got, want = _run_select(cases, device="cuda", slots_of=slots_of, **kw)
    torch.cuda.synchronize()
    assert_bits_equal(got, want)
    return got


def test_beam_select_kernel_on_the_hand_made_tables():
    cases = beam_ref.hand_cases()
    for c in cases:                                         # each alone ...
        _select([c])
    _select(cases, k_cols=20)                               # ... and all of them as one launch


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_beam_select_kernel_on_random_tables(seed):
    rng = np.random.default_rng(seed)
    for W, S in ((2, 1), (3, 3), (8, 12), (8, 1), (2, 18)):                                  # one group
        _select([beam_ref.random_case(rng, W, S)])
    groups = [beam_ref.random_case(rng, W, S) for W, S in ((3, 2), (8, 5), (2, 7))]          # three groups, different W and S
    got = _select(groups, k_cols=20)
    assert got[1][39] == 123.0 and (got[2] == -5).sum() == 3   # slots and ids elements of no group are untouched


def test_beam_select_kernel_equals_the_cpu_form_and_skips_bad_groups():
    from test_beam_cpu import _run_select

    rng = np.random.default_rng(9)
    cases = [beam_ref.random_case(rng, W, S) for W, S in ((4, 3), (8, 12), (5, 5), (2, 1))]
    dev, _ = _run_select(cases, device="cuda", k_cols=20)
    host, _ = _run_select(cases, device="cpu", k_cols=20)
    torch.cuda.synchronize()
    for a, b in zip(dev, host):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    lp, ids = torch.zeros((2, 5), device="cuda"), torch.zeros((2, 5), dtype=torch.int32, device="cuda")
    scores, ids_out = torch.full((4,), 1.5, device="cuda"), torch.full((2,), -5, dtype=torch.int32, device="cuda")
    out = torch.full((1, ops.BEAM_OUT_WORDS), 99, dtype=torch.int32, device="cuda")
    for bad in (dict(slots=[0, 4]), dict(rows=[0, 2]), dict(outs=[0, 2]), dict(slots=[-1, 0])):
        d = ops.beam_desc(2, [1], bad.get("rows", [0, 1]), bad.get("outs", [0, 1]), bad.get("slots", [0, 1]))
        ops.beam_select(lp, ids, torch.tensor([d], dtype=torch.int32).cuda(), scores, ids_out, out)
        torch.cuda.synchronize()
        assert bool((out == 99).all()) and bool((scores == 1.5).all()) and bool((ids_out == -5).all())


# ------------------------------------------------------------------------------------------------------------ the copy kernel
def _tables(L, C, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shift = torch.randint(-32768, 32768, (L, 2, S, C), dtype=torch.int32, device="cuda", generator=g).to(torch.int16)
    wkv = torch.randint(-32768, 32768, (L, S, C // 64, 64, 64), dtype=torch.int32, device="cuda", generator=g).to(torch.int16)
    sp = torch.tensor(SPECIAL, dtype=torch.int32).to(torch.int16).cuda()
    shift[:, :, :, :len(SPECIAL)] = sp                     # in every slot and layer
    wkv[:, :, 0, 0, :len(SPECIAL)] = sp
    wkv[:, :, -1, -1, -len(SPECIAL):] = sp
    elapsed = torch.randint(-(1 << 31), (1 << 31) - 1, (S,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    return shift, wkv, elapsed


def _pad(xs):
    return list(xs) + [-1] * (8 - len(xs))


# (copy_src [G][<= 8], dst [G][<= 8]) over 9 slots
COPY_CASES = {
    "one_group_of_3_one_copy": ([[-1, -1, 2]], [[2, 5, 7]]),
    "one_group_of_8_seven_copies": ([[4, 4, 4, -1, 4, 4, 4, 4]], [[0, 1, 2, 4, 5, 6, 7, 8]]),
    "two_groups": ([[-1, 0, -1], [6, -1, 6, -1]], [[0, 1, 2], [3, 6, 7, 8]]),
    "nothing_to_copy": ([[-1, -1, -1], [-1, -1]], [[0, 1, 2], [5, 6]]),
    "out_of_range_sources_are_skipped": ([[9, 3, -2, 1 << 20]], [[0, 1, 2, 4]]),
    "out_of_range_destinations_are_skipped": ([[3, 3, 3]], [[9, -1, 5]]),
}


def _check_copy(L, C, S, copy_src, dst, seed):
    shift, wkv, elapsed = _tables(L, C, S, seed)
    got = [t.clone() for t in (shift, wkv, elapsed)]
    cs = torch.tensor([_pad(r) for r in copy_src], dtype=torch.int32).cuda()
    ds = torch.tensor([_pad(r) for r in dst], dtype=torch.int32).cuda()
    ops.beam_copy_states([got[0].view(torch.float16), got[1].view(torch.float16), got[2]], cs, ds)
    # ... and read through a strided view, as the worker passes the select kernel's output records
    rec = torch.full((len(copy_src), ops.BEAM_OUT_WORDS), -1, dtype=torch.int32, device="cuda")
    rec[:, ops.BEAM_OUT_COPY:ops.BEAM_OUT_COPY + 8] = cs
    got2 = [t.clone() for t in (shift, wkv, elapsed)]
    ops.beam_copy_states([got2[0].view(torch.float16), got2[1].view(torch.float16), got2[2]], rec[:, ops.BEAM_OUT_COPY:ops.BEAM_OUT_COPY + 8], ds)
    torch.cuda.synchronize()
    pairs = [(s, d) for rs, rd in zip(copy_src, dst) for s, d in zip(rs, rd) if 0 <= s < S and 0 <= d < S and s != d]
    src_of = {d: s for s, d in pairs}
    want = [t.clone() for t in (shift, wkv, elapsed)]
    if pairs:
        s = torch.tensor([p[0] for p in pairs], dtype=torch.long, device="cuda")
        d = torch.tensor([p[1] for p in pairs], dtype=torch.long, device="cuda")
        want[0][:, :, d] = shift[:, :, s]
        want[1][:, d] = wkv[:, s]
        want[2][d] = elapsed[s]
    for g in (got, got2):
        for name, a, b in zip(("shift", "wkv", "elapsed"), g, want):
            assert torch.equal(a, b), name
        keep = torch.tensor([x for x in range(S) if x not in src_of], dtype=torch.long, device="cuda")
        assert torch.equal(g[0].index_select(2, keep), shift.index_select(2, keep))          # every other slot bit-unchanged
        assert torch.equal(g[1].index_select(1, keep), wkv.index_select(1, keep)) and torch.equal(g[2][keep], elapsed[keep])
    return len(pairs)


@pytest.mark.parametrize("case", list(COPY_CASES))
def test_beam_copy_states_kernel_matches_torch_indexing(case):
    n = _check_copy(2, 128, 9, *COPY_CASES[case], seed=len(case))
    assert n == {"one_group_of_3_one_copy": 1, "one_group_of_8_seven_copies": 7, "two_groups": 3, "nothing_to_copy": 0,
                 "out_of_range_sources_are_skipped": 1, "out_of_range_destinations_are_skipped": 1}[case]


def test_beam_copy_states_kernel_at_the_7b_geometry():
    assert _check_copy(32, 4096, 9, [[-1, 0, 0], [5, -1, 5, 5]], [[0, 1, 2], [3, 5, 6, 8]], seed=72) == 5
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ the worker
def _model(name):
    from test_decode_sampling_gpu import _model as model

    return model(name)


class _Sink:
    def __init__(self):
        self.items = []

    def put_nowait(self, x):
        self.items.append(x)


class _Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "".join(chr(65 + i % 26) for i in ids)


def _worker(m, V, run_ahead=True, use_graph=True, batch_size=9):
    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=batch_size, model=m, tokenizer=_Tok(), run_ahead=run_ahead)
    w._init_worker()
    assert w.use_graph
    w.use_graph = use_graph
    w.max_prefill_count = batch_size
    return w, tq


def _task(prompt, **kw):
    from chirrup_amd.core_structure import Task

    g = dict(temperature=0.0, top_p=0.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_decay=1.0, stop_tokens=[])
    g.update(kw)
    return Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **g)


def _drain(w, tasks, after_step=None):
    for _ in range(4000):
        busy = w.step()
        if after_step is not None:
            after_step()
        if not busy and all(any(k == "task_completed" for k, _ in t.output_queue.items) for t in tasks):
            return
    raise AssertionError("worker did not drain")


def _spy_beam_records(w):
    """Copies of every step's beam record at the moment the host handles it (the pinned buffers are reused two steps later)."""
    seen = []
    real = w._handle_results

    def spy(rec):
        if isinstance(rec, dict) and rec.get("beam") is not None:
            if rec["event"] is not None:
                rec["event"].synchronize()
            part = rec["beam"]
            seen.append({"group": part["groups"][0], "spans": list(part["spans"]), "out": part["out"].clone().numpy(),
                         "lp": part["lp"].clone().numpy(), "ids": part["ids"].clone().numpy()})
        return real(rec)

    w._handle_results = spy
    return seen


def _hyps(t):
    (payload,) = [p for k, p in t.output_queue.items if k == "beams"]
    return [{k: h[k] for k in ("token_ids", "cumulative_logprob", "score", "finish_reason")} for h in payload["hypotheses"]]


def _stops(V):
    return [0, 7, V - 1]


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
@pytest.mark.parametrize("model", list(VOCAB))
def test_worker_follows_the_contract_replayed_from_its_candidate_tables(model, run_ahead, use_graph, W):
    """A 23-token prompt (chunked and single-token prefill), max_tokens 12, a greedy request beside it.  Every step's output record
    equals the reference selection on that step's downloaded W x K tables; so do the hypotheses.  In-step: right after each step
    the slots of two children of one parent hold bit-identical states."""
    V = VOCAB[model]
    m = _model(model)
    prompt = np.random.default_rng(V + W).integers(1, V, 23).tolist()
    w, tq = _worker(m, V, run_ahead, use_graph)
    w.beam_trace = True
    seen = _spy_beam_records(w)
    stops = _stops(V)
    b = _task(prompt, beam_width=W, beam_n_best=W, length_penalty=1.0, max_tokens=12, stop_tokens=stops, temperature=1.0, top_p=0.5,
              frequency_penalty=0.4, presence_penalty=0.3)
    other = _task(prompt[:9], max_tokens=12)
    twins = [0]

    def after_step():
        if run_ahead or not seen:
            return
        rec, group = seen[-1], seen[-1]["group"]
        if group["done"]:
            return
        torch.cuda.synchronize()
        parents = rec["out"][0][:W].tolist()
        s0, s1, s2 = w.batch_state
        for p in range(W):
            for q in range(p + 1, W):
                if parents[p] == parents[q] and parents[p] >= 0:
                    a, c = group["slots"][p], group["slots"][q]
                    assert torch.equal(s0[:, :, a].view(torch.int16), s0[:, :, c].view(torch.int16)), (p, q)
                    assert torch.equal(s1[:, a].view(torch.int16), s1[:, c].view(torch.int16)), (p, q)
                    assert int(s2[a]) == int(s2[c])
                    twins[0] += 1

    tq.put(b)
    tq.put(other)
    _drain(w, [b, other], after_step)
    steps = []
    for rec in seen:
        (r0, W_, K), = rec["spans"]
        assert (W_, K) == (W, W + len(stops))
        steps.append((rec["lp"][r0:r0 + W, :K], rec["ids"][r0:r0 + W, :K]))
    trace, hyps = beam_ref.replay(steps, W, stops, 12, 1.0, W)
    assert len(trace) >= 1 and len(seen) - len(trace) in ((0, 1) if run_ahead else (0,))     # (one speculative step may follow the end)
    slots = seen[0]["group"]["slots"]
    for t, (rec, (parents, ids, scores, finished, copy_from)) in enumerate(zip(seen, trace)):
        row = rec["out"][0]
        assert row[:W].tolist() == parents and row[24:24 + W].tolist() == ids, t
        assert row[32:32 + W].tolist() == scores, t
        assert row[16:16 + W].tolist() == [slots[c] if c >= 0 else -1 for c in copy_from], t
        assert row[40] == len(finished) and [(row[41 + j], row[49 + j], row[57 + j]) for j in range(row[40])] == finished, t
    assert _hyps(b) == hyps and len(hyps) >= 1
    assert len(other.generated_tokens) == 12
    if not run_ahead:
        assert twins[0] >= 1                                 # the first step alone: every beam is a child of position 0


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
@pytest.mark.parametrize("model", list(VOCAB))
def test_a_neighbouring_greedy_request_is_not_disturbed(model, run_ahead, use_graph):
    """The same greedy n = 1 request beside a beam request of width 4 and beside a sampled n = 4 group of the same prompt: both runs
    have the same batch width at every step (the forward is not batch-invariant across row counts), so the streams are equal."""
    V = VOCAB[model]
    m = _model(model)
    rng = np.random.default_rng(V + 5)
    prompt, near = rng.integers(1, V, 23).tolist(), rng.integers(1, V, 23).tolist()
    runs = []
    for beam in (True, False):
        w, tq = _worker(m, V, run_ahead, use_graph)
        n1 = _task(near, max_tokens=12, return_logits=True, frequency_penalty=0.3, presence_penalty=0.2, penalty_decay=0.98)
        if beam:
            lead = _task(prompt, beam_width=4, max_tokens=12, stop_tokens=[V - 1])
            group = [lead]
        else:
            kw = dict(temperature=1.0, top_p=0.9, seed=4, max_tokens=12)
            others = [_task(prompt, choice_index=j, **kw) for j in range(1, 4)]
            lead = _task(prompt, siblings=others, **kw)
            group = [lead] + others
        tq.put(lead)
        tq.put(n1)
        _drain(w, group + [n1])
        items = [p for k, p in n1.output_queue.items if k == "token_generated"]
        runs.append(([p[0] for p in items], [p[2].numpy().view(np.uint16) for p in items]))
        if beam:
            assert len(_hyps(lead)) == 1
        else:
            assert all(len(t.generated_tokens) == 12 for t in group)
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) == 12
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ------------------------------------------------------------------------------------------------------------ re-scoring
RESCORE_STOP = 319                                          # the one stop id of the re-scoring runs (L2/C128, V 320)


def _prompt_lps(task):
    lps = []
    for k, p in task.output_queue.items:
        if k == "prompt_logprobs":
            assert p["start"] == len(lps)
            lps += p["logprobs"]
    return lps


def _score(m, V, sequences):
    """Σ of the prompt-path logprobs of the last n positions of each (tokens, n): one scoring request each (max_tokens = 0)."""
    w, tq = _worker(m, V)
    tasks = [_task(toks, max_tokens=0, prompt_logprobs=0) for toks, _ in sequences]
    for t in tasks:
        tq.put(t)
    _drain(w, tasks)
    out = []
    for t, (toks, n) in zip(tasks, sequences):
        lps = _prompt_lps(t)
        assert len(lps) == len(toks)
        out.append(float(sum(lps[len(toks) - n:])) if n else 0.0)
    return out


def greedy_rescoring_differences(m, V, n_new=12, batches=8, width=4):
    """|decode-path sum - prompt-path sum| of the logprobs of n_new greedy tokens: n = 1 requests, `width` of them side by side (the
    width a beam request of that width decodes at) and one alone per batch.  The decode-path sum is accumulated in binary32, one
    addition per token, like a beam's cumulative score."""
    rng = np.random.default_rng(2024)
    diffs = []
    for _ in range(batches):
        for n in (width, 1):
            prompts = [rng.integers(1, V - 1, 23).tolist() for _ in range(n)]
            w, tq = _worker(m, V)
            tasks = [_task(p, max_tokens=n_new, logprobs=True) for p in prompts]
            for t in tasks:
                tq.put(t)
            _drain(w, tasks)
            seqs, sums = [], []
            for p, t in zip(prompts, tasks):
                items = [x for k, x in t.output_queue.items if k == "token_generated"]
                acc = np.float32(0.0)
                for it in items:
                    acc = np.float32(acc + np.float32(it[3]["logprob"]))
                seqs.append((p + [it[0] for it in items], len(items)))
                sums.append(float(acc))
            diffs += [abs(a - b) for a, b in zip(sums, _score(m, V, seqs))]
    return diffs


def beam_rescoring_differences(m, V, n_new=12):
    """|cumulative_logprob - prompt-path sum| of every hypothesis of beam requests of width 2 and 4 (the stop token's position is
    part of a hypothesis that ended "stop")."""
    rng = np.random.default_rng(77)
    diffs = []
    for W in (2, 4, 4):
        prompt = rng.integers(1, V - 1, 23).tolist()
        w, tq = _worker(m, V)
        b = _task(prompt, beam_width=W, beam_n_best=W, max_tokens=n_new, stop_tokens=[RESCORE_STOP])
        tq.put(b)
        _drain(w, [b])
        hyps = _hyps(b)
        assert hyps
        seqs = [(prompt + h["token_ids"] + ([RESCORE_STOP] if h["finish_reason"] == "stop" else []),
                 len(h["token_ids"]) + (h["finish_reason"] == "stop")) for h in hyps]
        diffs += [abs(h["cumulative_logprob"] - s) for h, s in zip(hyps, _score(m, V, seqs))]
    return diffs


def test_hypotheses_rescore_through_the_prompt_logprobs_path():
    """The bar is 1.25 x the largest difference the same comparison shows for greedy n = 1 requests of the same length on the same
    model -- code that predates beam search -- measured once and committed (profiles/r08_beam_rescoring.txt, tests/golden/beam_bars.json)."""
    bars = json.load(open(os.path.join(G, "beam_bars.json")))
    m = _model("L2C128")
    diffs = beam_rescoring_differences(m, 320)
    print(json.dumps({"case": "beam hypotheses re-scored", "n": len(diffs), "max_abs_diff": max(diffs), "bar": bars["rescoring_abs"]}))
    assert len(diffs) >= 3 and max(diffs) <= bars["rescoring_abs"], (diffs, bars)


if __name__ == "__main__":
    model = _model("L2C128")
    greedy = greedy_rescoring_differences(model, 320)
    print(json.dumps({"case": "greedy n=1, 12 tokens: |decode-path sum (binary32) - prompt-path sum|", "requests": len(greedy),
                      "max_abs_diff": max(greedy), "mean_abs_diff": float(np.mean(greedy)), "bar_1.25x": 1.25 * max(greedy)}))
    beam = beam_rescoring_differences(model, 320)
    print(json.dumps({"case": "beam hypotheses (W 2, 4, 4; 12 tokens): |cumulative_logprob - prompt-path sum|", "hypotheses": len(beam),
                      "max_abs_diff": max(beam), "mean_abs_diff": float(np.mean(beam))}))
