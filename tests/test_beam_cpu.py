"""Beam search without a GPU (DESIGN.md "Beam search"): the fake-backend worker against a plain reference search (tests/beam_ref.py),
the CPU form of ops.beam_select on hand-made tables, scheduling and lifecycle, the refusals at Task and on both routes, the
process-mode wire, and the compiler's resource report of the two kernels."""
import asyncio
import os
import queue
import re
import subprocess

import httpx
import numpy as np
import pytest
import torch

import beam_ref
from chirrup_amd import ops
from chirrup_amd.core_structure import ModelLoadConfig, RequestStatus, Task
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.web_service import chat_prompt, create_app
from chirrup_amd.worker import StateCategory, Worker
from test_engine_cpu import _Tok
from test_worker_cpu import V, FakeModel, FakeTok, Sink, cpu_penalize_argmax, expected_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
STOPS1, STOPS3 = [0], [0, 5, 9]


def logits_of(h: int) -> np.ndarray:
    """A full row of logits with many ties; the stop token 0 is the favourite after a third of all histories."""
    v = np.arange(V)
    x = (((h * 37 + v * v * 11 + v * 5) % 23).astype(np.float32)) / 2
    if h % 3 == 0:
        x[0] = 12.0
    return x.astype(np.float16)


class BeamModel(FakeModel):
    """FakeModel with full rows of logits; counts the tokens it is fed."""

    def __init__(self):
        self.fed = 0

    def forward_slots(self, tokens, pool, slot_idx, full_output=False):
        out = torch.zeros((len(tokens), V), dtype=torch.float16)
        for b, (toks, s) in enumerate(zip(tokens, slot_idx.tolist())):
            h = int(pool[1][0, s, 0, 0, 0])
            for t in toks:
                h = self.advance(h, int(t))
            self.fed += len(toks)
            pool[1][0, s, 0, 0, 0] = h
            pool[2][s] += len(toks)
            out[b] = torch.from_numpy(logits_of(h))
        return out


def hist(tokens, h=0):
    for t in tokens:
        h = FakeModel.advance(h, t)
    return h


def candidates_of(tokens, K):
    """The K most likely ids after `tokens` and their float32 log-softmax (the definition of rwkv7_token_logprobs)."""
    x = torch.from_numpy(logits_of(hist(tokens))).float().view(1, V)
    m = x.max(dim=1, keepdim=True).values
    lpr = ((x - m) - torch.log(torch.exp(x - m).sum(dim=1, keepdim=True))).numpy()[0]
    order = np.argsort(-x.numpy()[0], kind="stable")[:K]
    return lpr[order], order


def _worker(run_ahead, batch_size=10, model=None):
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [], cfg, tq, queue.Queue(), queue.Queue(), batch_size=batch_size, model=model or BeamModel(), tokenizer=FakeTok(),
               penalize_argmax=cpu_penalize_argmax, run_ahead=run_ahead)
    w._init_worker()
    return w, tq


def _task(prompt, **kw):
    for k, v in (("temperature", 0.0), ("top_p", 0.0), ("frequency_penalty", 0.0), ("presence_penalty", 0.0), ("penalty_decay", 1.0),
                 ("stop_tokens", list(STOPS1)), ("max_tokens", 10)):
        kw.setdefault(k, v)
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **kw)


def _drain(w, max_iter=3000):
    for _ in range(max_iter):
        if not w.step():
            return
    raise AssertionError("worker did not drain")


def _msgs(t, kind):
    return [p for k, p in t.output_queue.items if k == kind]


def _hyps(t):
    (payload,) = _msgs(t, "beams")
    return [{k: h[k] for k in ("token_ids", "cumulative_logprob", "score", "finish_reason")} for h in payload["hypotheses"]]


def _all_empty(w):
    return all(td["state_category"] == StateCategory.EMPTY for td in w.state_slot.values())


# --------------------------------------------------------------------------------------------------- streams against the reference
@MODES
@pytest.mark.parametrize("stops", [STOPS1, STOPS3], ids=["S1", "S3"])
@pytest.mark.parametrize("lam", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_hypotheses_equal_the_reference_search(run_ahead, W, lam, stops):
    prompt = [3, 1, 4, 1, 5, 9, 2, 6]
    for n_best in (1, W):
        w, tq = _worker(run_ahead)
        t = _task(prompt, beam_width=W, length_penalty=lam, beam_n_best=n_best, stop_tokens=list(stops), max_tokens=9,
                  temperature=1.0, top_p=0.9, frequency_penalty=0.7, presence_penalty=0.4, seed=5)       # accepted and ignored
        tq.put(t)
        _drain(w)
        want, _ = beam_ref.search(candidates_of, prompt, W, stops, 9, lam, n_best)
        assert _hyps(t) == want and 1 <= len(want) <= n_best
        (payload,) = _msgs(t, "beams")
        assert payload["prompt_tokens"] == len(prompt)
        assert [h["text"] for h in payload["hypotheses"]] == ["".join(f"<{i}>" for i in h["token_ids"]) for h in want]
        assert t.output_queue.items[-1] == ("task_completed", t) and len(_msgs(t, "task_completed")) == 1
        assert not _msgs(t, "token_generated")                    # nothing streams
        assert t.generated_tokens == want[0]["token_ids"] and "".join(t.decoded_texts) == payload["hypotheses"][0]["text"]
        assert t.request_status == (RequestStatus.FINISHED_STOPPED if want[0]["finish_reason"] == "stop"
                                    else RequestStatus.FINISHED_LENGTH_CAPPED)
        assert _all_empty(w) and not t.siblings


@MODES
def test_a_best_first_candidate_that_is_a_stop_token_gives_an_empty_hypothesis(run_ahead):
    prompt = next([k, 1, 2] for k in range(1, 60) if hist([k, 1, 2]) % 3 == 0)
    assert int(candidates_of(prompt, 1)[1][0]) == 0
    w, tq = _worker(run_ahead)
    t = _task(prompt, beam_width=3, beam_n_best=3, max_tokens=6, length_penalty=0.0)
    tq.put(t)
    _drain(w)
    want, _ = beam_ref.search(candidates_of, prompt, 3, STOPS1, 6, 0.0, 3)
    assert _hyps(t) == want
    empty = [h for h in want if h["token_ids"] == []]
    assert len(empty) == 1 and empty[0]["finish_reason"] == "stop" and empty[0]["score"] == empty[0]["cumulative_logprob"]


@MODES
def test_a_max_tokens_cut_ends_every_hypothesis_with_length(run_ahead):
    prompt = next([k, 7] for k in range(1, 60) if beam_ref.search(candidates_of, [k, 7], 4, STOPS1, 3, 1.0, 4)[1] == "length"
                  and all(h["finish_reason"] == "length" for h in beam_ref.search(candidates_of, [k, 7], 4, STOPS1, 3, 1.0, 4)[0]))
    w, tq = _worker(run_ahead)
    t = _task(prompt, beam_width=4, beam_n_best=4, max_tokens=3)
    tq.put(t)
    _drain(w)
    want, _ = beam_ref.search(candidates_of, prompt, 4, STOPS1, 3, 1.0, 4)
    assert _hyps(t) == want and len(want) == 4
    assert all(h["finish_reason"] == "length" and len(h["token_ids"]) == 3 for h in want)
    assert t.request_status == RequestStatus.FINISHED_LENGTH_CAPPED


@MODES
def test_a_request_ends_once_W_hypotheses_have_finished(run_ahead):
    prompt = next([k, 2, 8] for k in range(1, 60) if beam_ref.search(candidates_of, [k, 2, 8], 2, STOPS3, 200, 1.0, 2)[1] == "finished")
    m = BeamModel()
    w, tq = _worker(run_ahead, model=m)
    t = _task(prompt, beam_width=2, beam_n_best=2, max_tokens=200, stop_tokens=list(STOPS3))
    tq.put(t)
    _drain(w)
    want, ended = beam_ref.search(candidates_of, prompt, 2, STOPS3, 200, 1.0, 2)
    assert ended == "finished" and _hyps(t) == want and all(h["finish_reason"] == "stop" for h in want)
    assert m.fed < 2 * 150                                        # it did not run on to max_tokens


# --------------------------------------------------------------------------------------------------- ops.beam_select, CPU form
def _run_select(cases, slots_of=None, k_cols=None, select=ops.beam_select, device="cpu"):
    """Runs the cases as ONE launch (one group each) and returns (out records, scores, ids_out) with the expectations."""
    n_slots, R = 40, sum(c["W"] for c in cases)
    k_cols = k_cols or max(c["W"] + len(c["stops"]) for c in cases)
    lp = torch.full((R, k_cols + 1), float("nan"), dtype=torch.float32)       # (column 0: the target column of token_logprobs)
    ids = torch.full((R, k_cols), -7, dtype=torch.int32)
    scores = torch.full((n_slots,), 123.0, dtype=torch.float32)
    ids_out = torch.full((R + 3,), -5, dtype=torch.int32)
    desc, want, r0 = [], [], 0
    want_scores, want_ids = scores.clone().numpy(), ids_out.clone().numpy()
    for g, c in enumerate(cases):
        W, K = c["W"], c["W"] + len(c["stops"])
        slots = slots_of(g, W) if slots_of else [(7 * g + 3 * p + 1) % n_slots for p in range(W)]
        out_rows = [R + 2 - (r0 + p) for p in range(W)]                      # (not the identity)
        lp[r0:r0 + W, 1:1 + K] = torch.from_numpy(c["lp"])
        ids[r0:r0 + W, :K] = torch.from_numpy(c["ids"])
        scores[torch.tensor(slots)] = torch.from_numpy(c["scores"])
        desc.append(ops.beam_desc(W, c["stops"], list(range(r0, r0 + W)), out_rows, slots))
        rec, new_scores, new_ids = beam_ref.expected_record(c["lp"], c["ids"], c["scores"], W, set(c["stops"]), slots)
        want.append(rec)
        for p in range(W):
            want_scores[slots[p]] = new_scores[p]
            if new_ids[p] is not None:
                want_ids[out_rows[p]] = new_ids[p]
        r0 += W
    out = torch.full((len(cases), ops.BEAM_OUT_WORDS), 99, dtype=torch.int32)
    dev = [t.to(device) for t in (lp, ids, torch.tensor(desc, dtype=torch.int32), scores, ids_out, out)]
    select(dev[0][:, 1:], dev[1], dev[2], dev[3], dev[4], dev[5])
    return (dev[5].cpu().numpy(), dev[3].cpu().numpy(), dev[4].cpu().numpy()), (np.stack(want), want_scores, want_ids)


def assert_bits_equal(got, want):
    for g, w_, name in zip(got, want, ("records", "scores", "ids")):
        gb = g.view(np.int32) if g.dtype == np.float32 else g
        wb = w_.view(np.int32) if w_.dtype == np.float32 else w_
        assert np.array_equal(gb, wb), (name, gb.tolist(), wb.tolist())


@pytest.mark.parametrize("case", beam_ref.hand_cases(), ids=lambda c: c["name"])
def test_beam_select_cpu_form_on_hand_made_tables(case):
    got, want = _run_select([case])
    assert_bits_equal(got, want)
    rec, W = got[0][0], case["W"]
    parent, rank, copy = rec[0:W].tolist(), rec[8:8 + W].tolist(), rec[16:16 + W].tolist()
    name = case["name"]
    if name == "equal_cum":
        assert [(parent[p], rec[24 + p]) for p in np.argsort(rank)] == [(0, 10), (0, 11)]         # b = 0 first, then k
    if name == "first_step":
        assert parent == [0, 0, 0] and copy[0] == -1 and copy[1] == copy[2] and copy[1] >= 0
    if name == "stop_at_W_minus_1":
        assert rec[40] == 1 and (rec[41], rec[49]) == (0, 1)
    if name == "stop_at_W":
        assert rec[40] == 0
    if name == "non_finite_stop":
        assert rec[40] == 0
    if name == "one_parent_takes_all":
        assert parent == [2, 2, 2, 2] and copy[2] == -1 and sorted(rank[p] for p in (0, 1, 3)) == [1, 2, 3]
        assert [rank[p] for p in (0, 1, 3)] == [1, 2, 3] and len({copy[0], copy[1], copy[3]}) == 1       # ascending positions
    if name == "all_survive":
        assert copy == [-1, -1, -1] and parent == [0, 1, 2]
    if name == "nan_lp":
        assert not np.isnan(got[1]).any()


def test_beam_select_cpu_form_leaves_other_entries_and_bad_groups_alone():
    rng = np.random.default_rng(3)
    cases = [beam_ref.random_case(rng, W, S) for W, S in ((2, 1), (8, 12), (3, 4))]
    got, want = _run_select(cases, k_cols=20)
    assert_bits_equal(got, want)
    # a descriptor out of range writes nothing at all
    lp, ids = torch.zeros((2, 5)), torch.zeros((2, 5), dtype=torch.int32)
    scores, ids_out = torch.full((4,), 1.5), torch.full((2,), -5, dtype=torch.int32)
    out = torch.full((1, ops.BEAM_OUT_WORDS), 99, dtype=torch.int32)
    for bad in (dict(slots=[0, 4]), dict(rows=[0, 2]), dict(outs=[0, 2])):
        d = ops.beam_desc(2, [1], bad.get("rows", [0, 1]), bad.get("outs", [0, 1]), bad.get("slots", [0, 1]))
        ops.beam_select(lp, ids, torch.tensor([d], dtype=torch.int32), scores, ids_out, out)
        assert (out == 99).all() and (scores == 1.5).all() and (ids_out == -5).all()
    with pytest.raises(Exception):
        ops.beam_desc(9, [1], [0] * 9, [0] * 9, [0] * 9)
    with pytest.raises(Exception):
        ops.beam_desc(8, list(range(13)), [0] * 8, [0] * 8, [0] * 8)


def test_beam_copy_states_cpu_form():
    rng = np.random.default_rng(11)
    S = 9
    shift = torch.from_numpy(rng.standard_normal((2, 2, S, 8)).astype(np.float16))
    wkv = torch.from_numpy(rng.standard_normal((2, S, 1, 4, 4)).astype(np.float32))
    elapsed = torch.arange(S, dtype=torch.int32) * 3
    before = [t.clone() for t in (shift, wkv, elapsed)]
    copy_src = torch.tensor([[-1, 2, 2, -1, -1, -1, -1, -1], [-1, 40, -1, -1, -1, -1, -1, -1]], dtype=torch.int32)
    dst = torch.tensor([[2, 3, 5, -1, -1, -1, -1, -1], [0, 1, -1, -1, -1, -1, -1, -1]], dtype=torch.int32)
    ops.beam_copy_states([shift, wkv, elapsed], copy_src, dst)
    for s in range(S):
        src = 2 if s in (3, 5) else s
        assert torch.equal(shift[:, :, s], before[0][:, :, src]) and torch.equal(wkv[:, s], before[1][:, src])
        assert int(elapsed[s]) == int(before[2][src])


# --------------------------------------------------------------------------------------------------- scheduling and lifecycle
@MODES
@pytest.mark.parametrize("plen", [1, 6, 37])
def test_the_prompt_is_fed_once(run_ahead, plen):
    """(P - 1) + W prompt tokens; then W rows per step.  Run-ahead adds one speculative step of W rows."""
    prompt = list(range(3, 3 + plen))
    W, steps = 4, 1
    m = BeamModel()
    w, tq = _worker(run_ahead, model=m)
    t = _task(prompt, beam_width=W, max_tokens=steps, stop_tokens=[63])
    tq.put(t)
    _drain(w)
    assert len(_hyps(t)) == 1
    spec = W if run_ahead else 0
    assert m.fed - spec == (plen - 1) + W, m.fed


@MODES
def test_beam_and_ordinary_requests_side_by_side(run_ahead):
    plain = [([5, 7, 11], 14), ([2, 2, 9, 4], 9)]
    alone = []
    for prompt, n in plain:
        w, tq = _worker(run_ahead)
        t = _task(prompt, max_tokens=n, stop_tokens=[])
        tq.put(t)
        _drain(w)
        alone.append(t.generated_tokens)
    w, tq = _worker(run_ahead)
    a = _task(plain[0][0], max_tokens=plain[0][1], stop_tokens=[])
    b = _task([3, 1, 4, 1, 5], beam_width=3, beam_n_best=3, max_tokens=8, stop_tokens=list(STOPS3))
    c = _task(plain[1][0], max_tokens=plain[1][1], stop_tokens=[])
    for t in (a, b, c):
        tq.put(t)
    _drain(w)
    assert [a.generated_tokens, c.generated_tokens] == alone                # the ordinary streams are unchanged
    assert [p[0] for p in _msgs(a, "token_generated")] == alone[0]
    assert _hyps(b) == beam_ref.search(candidates_of, [3, 1, 4, 1, 5], 3, STOPS3, 8, 1.0, 3)[0]
    assert _all_empty(w)


@MODES
def test_a_beam_request_waits_for_W_free_slots_and_nothing_overtakes_it(run_ahead, monkeypatch):
    w, tq = _worker(run_ahead, batch_size=5)              # 4 slots
    order = []
    real = w._install
    monkeypatch.setattr(w, "_install", lambda task, slot: (order.append(task), real(task, slot))[1])
    busy = [_task([3 + k, 1], max_tokens=12 + 4 * k, stop_tokens=[]) for k in range(3)]
    b = _task([8, 9, 10], beam_width=3, beam_n_best=2, max_tokens=6)
    late = _task([4, 4], max_tokens=5, stop_tokens=[])
    for t in busy + [b, late]:
        tq.put(t)
    held_seen = False
    for _ in range(3000):
        if w._held is b:
            held_seen = True
            assert late not in order
        if not w.step():
            break
    assert held_seen and order == busy + [b, late]
    assert _hyps(b) == beam_ref.search(candidates_of, [8, 9, 10], 3, STOPS1, 6, 1.0, 2)[0]
    assert len(late.generated_tokens) == 5 and _all_empty(w)


def test_a_beam_wider_than_the_worker_ends_at_once():
    w, tq = _worker(True, batch_size=3)                   # 2 slots
    b = _task([1, 2], beam_width=3)
    tq.put(b)
    _drain(w)
    assert b.request_status == RequestStatus.FINISHED_ABORTED and len(_msgs(b, "task_completed")) == 1 and not _msgs(b, "beams")


PROMPT = list(range(2, 50))                               # 48 tokens: chunked prefill over several steps


@MODES
def test_abort_before_the_fork_frees_W_slots(run_ahead):
    w, tq = _worker(run_ahead)
    b = _task(PROMPT, beam_width=4, max_tokens=8)
    tq.put(b)
    w.step()
    assert [w.state_slot[s]["state_category"] for s in (1, 2, 3)] == [StateCategory.FORWARD_ONE_SUSPENDED] * 3
    b.task_event_queue.put(("abort", None))
    _drain(w)
    assert b.request_status == RequestStatus.FINISHED_ABORTED and len(_msgs(b, "task_completed")) == 1 and not _msgs(b, "beams")
    assert _all_empty(w) and not w._groups and not b.siblings
    after = _task([4, 5], beam_width=2, max_tokens=4)     # the slots are free again
    tq.put(after)
    _drain(w)
    assert _hyps(after) == beam_ref.search(candidates_of, [4, 5], 2, STOPS1, 4, 1.0, 1)[0]


@MODES
def test_abort_after_the_fork_frees_W_slots(run_ahead):
    w, tq = _worker(run_ahead)
    b = _task(PROMPT, beam_width=4, max_tokens=10 ** 6, stop_tokens=[63])
    tq.put(b)
    for _ in range(500):
        w.step()
        if w.state_slot[0]["beam"] is not None and len(w.state_slot[0]["beam"][0]["ids"]) >= 3:
            break
    assert [w.state_slot[s]["beam"][1] for s in range(4)] == [0, 1, 2, 3]
    b.task_event_queue.put(("abort", None))
    _drain(w)
    assert b.request_status == RequestStatus.FINISHED_ABORTED and len(_msgs(b, "task_completed")) == 1 and not _msgs(b, "beams")
    assert _all_empty(w)


@MODES
def test_the_prefix_cache_export_happens_once_and_a_hit_forks(run_ahead, monkeypatch):
    forks = []
    real = ops.fork_states
    monkeypatch.setattr(ops, "fork_states", lambda pool, groups: (forks.append([(int(s), list(d)) for s, d in groups]), real(pool, groups))[1])
    w, tq = _worker(run_ahead)
    prompt = list(range(1, 31))
    b = _task(prompt, beam_width=3, beam_n_best=3, max_tokens=6, cache_prefill=True, cache_prefill_padding=3)
    tq.put(b)
    _drain(w)
    exports = _msgs(b, "cache_prefill")
    assert len(exports) == 1
    seen = list(exports[0]["prefilled_tokens"])
    assert seen == prompt[:len(seen)]
    hit = _task(prompt[len(seen):], beam_width=3, beam_n_best=3, max_tokens=6)
    hit.state = [x.clone() for x in exports[0]["state"]]
    tq.put(hit)
    _drain(w)
    want = beam_ref.search(candidates_of, prompt, 3, STOPS1, 6, 1.0, 3)[0]
    assert _hyps(b) == want and _hyps(hit) == want
    assert forks == [[(0, [1, 2])], [(0, [1, 2])]]


@MODES
def test_beam_trace_carries_the_candidate_tables(run_ahead):
    w, tq = _worker(run_ahead)
    w.beam_trace = True
    recs = []
    real = w._handle_results

    def spy(rec):
        if isinstance(rec, dict) and rec.get("beam") is not None:
            recs.append(rec["beam"])
        return real(rec)

    w._handle_results = spy
    b = _task([3, 1, 4], beam_width=3, beam_n_best=3, max_tokens=5, stop_tokens=list(STOPS3))
    tq.put(b)
    _drain(w)
    steps = []
    for part in recs:
        (r0, W, K), = part["spans"]
        steps.append((part["lp"][r0:r0 + W, :K].numpy(), part["ids"][r0:r0 + W, :K].numpy()))
    _, hyps = beam_ref.replay(steps, 3, STOPS3, 5, 1.0, 3)
    assert _hyps(b) == hyps


# --------------------------------------------------------------------------------------------------- refusals
REFUSED = [dict(logprobs=True), dict(return_logits=True), dict(prompt_logprobs=2), dict(max_tokens=0), dict(max_tokens=None),
           dict(guide=type("G", (), {"next": 1, "accept": 1, "key": 1})()), dict(logit_bias={3: 1.0}), dict(forbidden_tokens=[4]),
           dict(embed="mean"), dict(choice_index=1), dict(beam_width=1), dict(beam_width=9), dict(beam_width=-2),
           dict(beam_width=True), dict(beam_n_best=0), dict(beam_n_best=5), dict(length_penalty=float("nan")),
           dict(length_penalty=float("inf")), dict(length_penalty="x"), dict(stop_tokens=[]), dict(stop_tokens=list(range(17)))]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: ",".join(f"{k}={v}" if not hasattr(v, "key") else k for k, v in d.items()))
def test_task_refuses(bad):
    kw = dict(beam_width=4, beam_n_best=2)
    kw.update(bad)
    with pytest.raises(ValueError):
        _task([1, 2, 3], **kw)


def test_task_refuses_siblings_and_accepts_the_rest():
    with pytest.raises(ValueError):
        _task([1], beam_width=2, siblings=[_task([1], choice_index=1)])
    with pytest.raises(ValueError):
        _task([1], beam_n_best=2)                          # beam_n_best without beam_width
    t = _task([1, 2], beam_width=8, beam_n_best=8, length_penalty=0, stop_tokens=list(range(12)), temperature=1.3, top_p=0.2,
              top_k=5, seed=9, frequency_penalty=1.0, presence_penalty=1.0)
    assert (t.beam_width, t.beam_n_best, t.length_penalty) == (8, 8, 0.0)
    plain = _task([1, 2])
    assert (plain.beam_width, plain.length_penalty, plain.beam_n_best) == (0, 1.0, 1)


# --------------------------------------------------------------------------------------------------- the process-mode wire
def test_the_process_mode_wire_carries_the_beam_fields_and_the_beams_message():
    from chirrup_amd.engine_process import RemoteTaskQueue, task_to_wire

    t = _task([3, 1, 4], beam_width=5, length_penalty=0.25, beam_n_best=3, max_tokens=7, stop_tokens=[0, 9])
    d = task_to_wire(t)
    assert (d["beam_width"], d["length_penalty"], d["beam_n_best"]) == (5, 0.25, 3) and "siblings" not in d
    task_q, result_q = queue.Queue(), queue.Queue()
    task_q.put(d)
    rq = RemoteTaskQueue(task_q, result_q, "w1")
    got = rq.get_nowait()
    assert (got.beam_width, got.length_penalty, got.beam_n_best, got.max_tokens, got.stop_tokens) == (5, 0.25, 3, 7, [0, 9])
    assert result_q.get_nowait() == (t.task_id, ("__accepted__", "w1"))
    payload = {"hypotheses": [{"token_ids": [7], "text": "<7>", "cumulative_logprob": -0.5, "score": -0.5, "finish_reason": "stop"}],
               "prompt_tokens": 3}
    got.output_queue.put_nowait(("beams", payload))
    assert result_q.get_nowait() == (t.task_id, ("beams", payload))


def _process_factory(**kw):
    return Worker(model=BeamModel(), tokenizer=_Tok(), penalize_argmax=cpu_penalize_argmax, **kw)


def test_process_mode_beam_end_to_end():
    async def main():
        eng = AsyncEngineCore(worker_factory=_process_factory, tokenizer=_Tok(), worker_mode="process")
        cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
        await asyncio.wait_for(eng.init(worker_num=1, model_config=cfg, batch_size=6), 120)
        prompt = [3, 1, 4, 1, 5, 9, 2, 6]
        c = eng.completion("", prefill_tokens=prompt, beam_width=4, beam_n_best=2, length_penalty=1.0, max_tokens=7,
                           stop_tokens=list(STOPS3))
        events = await asyncio.wait_for(_events(c), 60)
        assert [e[0] for e in events] == ["beams"]
        want, _ = beam_ref.search(candidates_of, prompt, 4, STOPS3, 7, 1.0, 2)
        assert [{k: h[k] for k in want[0]} for h in events[0][1]["hypotheses"]] == want
        assert c.task.generated_tokens == want[0]["token_ids"] and c.is_finished       # the best hypothesis, on the task that came back
        with pytest.raises(ValueError):
            eng.completion("", prefill_tokens=prompt, beam_width=6)             # more beams than a worker has slots
        eng.shutdown()

    asyncio.run(main())


async def _events(c):
    return [ev async for ev in c]


# --------------------------------------------------------------------------------------------------- the routes
def _thread_factory(**kw):
    return Worker(model=BeamModel(), tokenizer=_Tok(), penalize_argmax=cpu_penalize_argmax, **kw)


class _VocabTok(_Tok):
    idx2token = {i: f"t{i}".encode() for i in range(V)}


async def _client(batch_size=6):
    eng = AsyncEngineCore(worker_factory=_thread_factory, tokenizer=_VocabTok())
    await eng.init(worker_num=1, model_config=ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64),
                   batch_size=batch_size)
    return eng, httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(eng, state_cache_size=0)), base_url="http://t")


CHAT = {"model": "rwkv-latest:no-thinking", "messages": [{"role": "user", "content": "three ways"}], "max_tokens": 7}
TEXT = {"prompt": "three ways", "max_tokens": 7}
ROUTE_STOPS = [0, 261, 24281]


def _chat_tokens():
    prompt, _ = chat_prompt([type("M", (), {"role": "user", "content": "three ways"})()], CHAT["model"])
    return [0] + _Tok().encode(prompt)


def test_chat_route_returns_n_hypotheses_in_rank_order():
    async def main():
        eng, cl = await _client()
        async with cl:
            r = await cl.post("/v1/chat/completions", json=dict(CHAT, use_beam_search=True, beam_width=4, n=2, length_penalty=0.5,
                                                                temperature=1.5, seed=3))
            assert r.status_code == 200, r.text
            body = r.json()
            plain = await cl.post("/v1/chat/completions", json=dict(CHAT, temperature=0.0))
            assert plain.status_code == 200 and len(plain.json()["choices"]) == 1
        want, _ = beam_ref.search(candidates_of, _chat_tokens(), 4, ROUTE_STOPS, 7, 0.5, 2)
        assert len(want) == 2 and [c["index"] for c in body["choices"]] == [0, 1]
        # (the route's content rules cut an answer at a blank line; the fake vocabulary has none)
        assert [c["message"]["content"] for c in body["choices"]] == ["".join(f"<{t}>" for t in h["token_ids"]) for h in want]
        assert [c["finish_reason"] for c in body["choices"]] == [h["finish_reason"] for h in want]
        n_out = sum(len(h["token_ids"]) for h in want)
        n_in = len(_chat_tokens())
        assert body["usage"] == {"prompt_tokens": n_in, "completion_tokens": n_out, "total_tokens": n_in + n_out}
        assert body["object"] == "chat.completion" and body["id"].startswith("chatcmpl-")
        eng.shutdown()

    asyncio.run(main())


def test_completions_route_returns_the_best_hypothesis_and_echoes_the_prompt():
    async def main():
        eng, cl = await _client()
        async with cl:
            r = await cl.post("/v1/completions", json=dict(TEXT, use_beam_search=True, beam_width=3))
            e = await cl.post("/v1/completions", json=dict(TEXT, use_beam_search=True, beam_width=3, echo=True))
            d = await cl.post("/v1/completions", json=dict(TEXT, use_beam_search=True))              # the default width
            two = await cl.post("/v1/completions", json=dict(TEXT, use_beam_search=True, beam_width=3, n=2))
            assert r.status_code == e.status_code == d.status_code == 200, (r.text, e.text, d.text)
            assert two.status_code == 400                                                        # untouched: n stays 1 here
        toks = [0] + _Tok().encode(TEXT["prompt"])
        (best,), _ = beam_ref.search(candidates_of, toks, 3, ROUTE_STOPS, 7, 1.0, 1)
        text = "".join(f"<{t}>" for t in best["token_ids"])
        for resp, want_text in ((r, text), (e, TEXT["prompt"] + text)):
            body = resp.json()
            assert len(body["choices"]) == 1 and body["choices"][0]["text"] == want_text
            assert body["choices"][0]["finish_reason"] == best["finish_reason"] and body["choices"][0]["logprobs"] is None
            assert body["usage"]["completion_tokens"] == len(best["token_ids"])
        (best4,), _ = beam_ref.search(candidates_of, toks, 4, ROUTE_STOPS, 7, 1.0, 1)
        assert d.json()["choices"][0]["text"] == "".join(f"<{t}>" for t in best4["token_ids"])
        eng.shutdown()

    asyncio.run(main())


def test_both_routes_answer_400_to_every_refused_combination():
    async def main():
        eng, cl = await _client()
        beam = dict(use_beam_search=True, beam_width=3)
        chat_bad = [(dict(beam, stream=True), "stream"), (dict(beam, logprobs=True), "logprobs"),
                    (dict(beam, logit_bias={"5": 1.0}), "logit_bias"), (dict(beam, guided_regex="a+"), "guided_regex"),
                    (dict(beam, guided_choice=["a", "b"]), "guided_choice"),
                    (dict(beam, response_format={"type": "json_schema", "json_schema": {"schema": {"type": "boolean"}}}), "response_format"),
                    (dict(beam_width=3), "use_beam_search"), (dict(beam, model="rwkv-latest:thinking"), "thinking"),
                    (dict(use_beam_search=True, beam_width=6), "slots"), (dict(beam, n=4), "n = 4"),
                    (dict(beam, stop=[chr(40 + k) for k in range(16)]), "stop tokens")]
        text_bad = [(dict(beam, stream=True), "stream"), (dict(beam, logprobs=2), "logprobs"),
                    (dict(beam, echo=True, logprobs=1, max_tokens=0), "logprobs"), (dict(beam, echo=True, max_tokens=0), "max_tokens"),
                    (dict(beam, logit_bias={"5": 1.0}), "logit_bias"), (dict(beam, guided_regex="a+"), "guided_regex"),
                    (dict(beam_width=3), "use_beam_search"), (dict(use_beam_search=True, beam_width=6), "slots"),
                    (dict(beam, stop=[chr(40 + k) for k in range(16)]), "stop tokens")]
        async with cl:
            for extra, word in chat_bad:
                r = await cl.post("/v1/chat/completions", json=dict(CHAT, **extra))
                assert r.status_code == 400 and word in r.text, (extra, r.status_code, r.text)
            for extra, word in text_bad:
                r = await cl.post("/v1/completions", json=dict(TEXT, **extra))
                assert r.status_code == 400 and word in r.text, (extra, r.status_code, r.text)
            for route, base in (("/v1/chat/completions", CHAT), ("/v1/completions", TEXT)):
                for w_ in (1, 9):
                    assert (await cl.post(route, json=dict(base, use_beam_search=True, beam_width=w_))).status_code == 422
        eng.shutdown()

    asyncio.run(main())


# --------------------------------------------------------------------------------------------------- the kernels' resource report
VGPR_BUDGET = {"beam_select_kernel": 28, "beam_copy_states_kernel": 60}      # the compiler's figures (DESIGN.md "Beam search")


def test_beam_kernels_have_no_scratch_and_no_spills():
    from test_kernel_budget_cpu import CSRC, FLAGS, HIPCC

    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "beam.hip"), "-o", os.devnull], capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    report, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = next((k for k in VGPR_BUDGET if k in m.group(1)), None)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs): (\d+)", line)
        if m and cur is not None:
            report.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    assert set(report) == set(VGPR_BUDGET), report
    for name, r in report.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] <= VGPR_BUDGET[name], (name, r)


def test_beam_entry_points_check_their_arguments():
    import ctypes

    import chirrup_amd
    from chirrup_amd import lib

    hdr = open(os.path.join(ROOT, "include", "chirrup_amd.h")).read()
    assert "int rwkv7_beam_select(int n_groups, int n_lp_rows, int k_cols, const float *lp" in hdr
    assert "int rwkv7_beam_copy_states(int n_groups, int L, int S, int C, int H, const int32_t *copy_src" in hdr
    assert "#define CHIRRUP_ABI_VERSION 4" in hdr and lib.ABI_VERSION == 4
    assert (ops.BEAM_MAX_W, ops.BEAM_DESC_WORDS, ops.BEAM_OUT_WORDS) == tuple(
        int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in ("CHIRRUP_BEAM_MAX_W", "CHIRRUP_BEAM_DESC_WORDS", "CHIRRUP_BEAM_OUT_WORDS"))
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    L = chirrup_amd.load()
    p = ctypes.c_void_p(4096)                             # never dereferenced: validation fails first (or nothing to do)
    sel, cp = L.rwkv7_beam_select, L.rwkv7_beam_copy_states
    assert len(lib.SIGNATURES["rwkv7_beam_select"][1]) == 14 and len(lib.SIGNATURES["rwkv7_beam_copy_states"][1]) == 12
    assert sel(0, 0, 0, None, 0, None, 0, None, None, 0, None, 0, None, None) == 0
    assert sel(-1, 4, 5, p, 5, p, 5, p, p, 4, p, 4, p, None) == -1
    for bad in ((70000, 4, 5, 5, 5, 4, 4), (1, 0, 5, 5, 5, 4, 4), (1, 4, 2, 5, 5, 4, 4), (1, 4, 21, 21, 21, 4, 4), (1, 4, 5, 4, 5, 4, 4),
                (1, 4, 5, 5, 4, 4, 4), (1, 4, 5, 5, 5, 0, 4), (1, 4, 5, 5, 5, 4, 0)):
        G, R, k, ls, is_, ns, ni = bad
        assert sel(G, R, k, p, ls, p, is_, p, p, ns, p, ni, p, None) == -1, bad
    for miss in range(6):
        a = [p] * 6
        a[miss] = None
        assert sel(1, 4, 5, a[0], 5, a[1], 5, a[2], a[3], 4, a[4], 4, a[5], None) == -2, miss
    assert cp(0, 0, 0, 0, 0, None, 0, None, None, None, None, None) == 0
    assert cp(-1, 2, 4, 128, 2, p, 8, p, p, p, p, None) == -1
    for bad in ((9000, 2, 4, 128, 2, 8), (1, 0, 4, 128, 2, 8), (1, 2, 0, 128, 2, 8), (1, 2, 4, 100, 2, 8), (1, 2, 4, 128, 1, 8), (1, 2, 4, 128, 2, 7)):
        assert cp(*bad[:5], p, bad[5], p, p, p, p, None) == -1, bad
    for miss in range(5):
        a = [p] * 5
        a[miss] = None
        assert cp(1, 2, 4, 128, 2, a[0], 8, a[1], a[2], a[3], a[4], None) == -2, miss
    assert cp(1, 2, 4, 128, 2, p, 8, p, ctypes.c_void_p(4104), p, p, None) == -3
    assert cp(1, 2, 4, 128, 2, p, 8, p, p, ctypes.c_void_p(4104), p, None) == -3
    assert cp(1, 2, 4, 128, 2, p, 8, p, p, p, ctypes.c_void_p(4098), None) == -3
