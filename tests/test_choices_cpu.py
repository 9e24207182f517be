"""Parallel choices (n) without a GPU: the fake-backend worker (the prompt fed once, greedy and seeded choices, admission of a group,
aborts before and after the fork, the prefix-cache export), the CPU form of ops.fork_states, the seeded host form with a stream,
the fork kernel's resource report, the process-mode wire, AsyncEngineCore.completions and the chat route's `n`."""
import asyncio
import json
import os
import queue
import re
import subprocess

import httpx
import numpy as np
import pytest
import torch

from chirrup_amd import ChirrupAmdError, ops
from chirrup_amd.core_structure import ModelLoadConfig, RequestStatus, Task
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.web_service import chat_prompt, create_app
from chirrup_amd.worker import StateCategory, Worker
from test_engine_cpu import _factory, _Tok
from test_worker_cpu import V, FakeModel, FakeTok, Sink, cpu_penalize_argmax, expected_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])


class CountingModel(FakeModel):
    """FakeModel that counts the tokens it is fed."""

    def __init__(self):
        self.fed = 0

    def forward_slots(self, tokens, pool, slot_idx, full_output=False):
        self.fed += sum(len(t) for t in tokens)
        return super().forward_slots(tokens, pool, slot_idx, full_output)


def _worker(run_ahead, batch_size=6, model=None):
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [], cfg, tq, queue.Queue(), queue.Queue(), batch_size=batch_size, model=model or FakeModel(), tokenizer=FakeTok(),
               penalize_argmax=cpu_penalize_argmax, run_ahead=run_ahead)
    w._init_worker()
    return w, tq


def _task(prompt, **kw):
    for k, v in (("temperature", 0.0), ("top_p", 0.0), ("frequency_penalty", 0.0), ("presence_penalty", 0.0), ("penalty_decay", 1.0),
                 ("stop_tokens", []), ("max_tokens", 10)):
        kw.setdefault(k, v)
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **kw)


def _group(prompt, n, **kw):
    """n choices of one prompt as AsyncEngineCore.completions assembles them: choice 0 carries choices 1..n-1."""
    others = [_task(prompt, choice_index=j, **kw) for j in range(1, n)]
    return [_task(prompt, siblings=others, **kw)] + others


def _drain(w, max_iter=3000):
    for _ in range(max_iter):
        if not w.step():
            return
    raise AssertionError("worker did not drain")


def _tokens(t):
    return [p[0] for kind, p in t.output_queue.items if kind == "token_generated"]


def _completed(t):
    return [p for kind, p in t.output_queue.items if kind == "task_completed"]


def _spy_forks(monkeypatch):
    calls = []
    real = ops.fork_states

    def spy(pool, groups):
        calls.append([(int(s), list(d)) for s, d in groups])
        return real(pool, groups)

    monkeypatch.setattr(ops, "fork_states", spy)
    return calls


def _seeded_stream(prompt, n, seed, stream, T=1.0, stop=()):
    """Host computation of a seeded, unpenalised, top_p = 1 choice over FakeModel with the Philox uniforms of `stream`."""
    h = 0
    for t in prompt:
        h = FakeModel.advance(h, t)
    out = []
    for i in range(n):
        lg = np.zeros(V, np.float16)
        lg[h % V], lg[(h + 1) % V] = 5.0, 4.0
        x = lg.astype(np.float64)
        w = np.exp(x - x.max())
        w = (w / w.sum()) ** (1.0 / float(np.float16(T)))
        cum = np.cumsum(w)
        tok = int(np.searchsorted(cum, float(ops.philox_uniform(seed, i, stream)) * cum[-1], side="right"))
        if tok in stop:
            break
        out.append(tok)
        h = FakeModel.advance(h, tok)
    return out


# --------------------------------------------------------------------------------------------------- the worker
@MODES
@pytest.mark.parametrize("plen", [1, 6, 37])
def test_the_prompt_is_fed_once(run_ahead, plen):
    """(P - 1) + n prompt tokens for n choices instead of n * P.  max_tokens = 1: every choice feeds the last prompt token, samples
    one id and ends; run-ahead adds one speculative row per choice, measured on the n = 1 request."""
    prompt = list(range(3, 3 + plen))
    m1 = CountingModel()
    w, tq = _worker(run_ahead, model=m1)
    one = _task(prompt, max_tokens=1)
    tq.put(one)
    _drain(w)
    spec = m1.fed - plen                                  # rows behind the last sampled token (run-ahead: 1, in-step: 0)
    assert spec == (1 if run_ahead else 0)
    for n in (2, 5):
        m = CountingModel()
        w, tq = _worker(run_ahead, model=m)
        g = _group(prompt, n, max_tokens=1)
        tq.put(g[0])
        _drain(w)
        assert [_tokens(t) for t in g] == [_tokens(one)] * n
        assert m.fed - n * spec == (plen - 1) + n, (n, m.fed)


@MODES
def test_greedy_choices_equal_the_single_stream(run_ahead, monkeypatch):
    forks = _spy_forks(monkeypatch)
    w, tq = _worker(run_ahead)
    prompt = [5, 7, 11, 13] * 8
    g = _group(prompt, 4, max_tokens=12, frequency_penalty=0.5, presence_penalty=0.25, penalty_decay=0.99)
    tq.put(g[0])
    _drain(w)
    want = expected_stream(prompt, 12, freq=0.5, pres=0.25, decay=0.99)
    for j, t in enumerate(g):
        assert _tokens(t) == want and t.generated_tokens == want, j
        assert t.request_status == RequestStatus.FINISHED_LENGTH_CAPPED and len(_completed(t)) == 1
        assert t.output_queue.items[-1] == ("task_completed", t) and t.prefill_tokens == []
    assert len(forks) == 1 and len(forks[0]) == 1 and len(forks[0][0][1]) == 3
    assert all(td["state_category"] == StateCategory.EMPTY for td in w.state_slot.values()) and not w._groups


@MODES
def test_seeded_choices_draw_their_own_streams(run_ahead):
    prompt, seed = [9, 2, 4, 4, 1], -4242
    w, tq = _worker(run_ahead)
    single = _task(prompt, temperature=1.0, top_p=1.0, seed=seed, max_tokens=16)
    tq.put(single)
    _drain(w)
    assert single.generated_tokens == _seeded_stream(prompt, 16, seed, 0)
    w, tq = _worker(run_ahead)
    g = _group(prompt, 4, temperature=1.0, top_p=1.0, seed=seed, max_tokens=16)
    tq.put(g[0])
    _drain(w)
    assert g[0].generated_tokens == single.generated_tokens                  # choice 0 reproduces the n = 1 request
    streams = [t.generated_tokens for t in g]
    for j, got in enumerate(streams):
        assert got == _seeded_stream(prompt, 16, seed, j), j
    assert len({tuple(s) for s in streams}) == 4                             # choices differ from each other
    assert w.seeded.tolist()[:4] == [1, 2, 3, 4]


@MODES
def test_unseeded_sampled_choices_and_their_own_tables(run_ahead):
    """Sampled choices without a seed take torch.rand; every choice has its own penalty tables and bias list (all from the request)."""
    torch.manual_seed(3)
    w, tq = _worker(run_ahead)
    prompt = [1, 2, 3]
    g = _group(prompt, 3, temperature=1.0, top_p=1.0, max_tokens=20, logit_bias={40: 3.0}, frequency_penalty=0.3, penalty_decay=0.9)
    tq.put(g[0])
    _drain(w)
    assert all(len(t.generated_tokens) == 20 for t in g)
    assert len({tuple(t.generated_tokens) for t in g}) == 3
    assert w._bias_n[:3] == [1, 1, 1] and w.bias_ids[:3, 0].tolist() == [40] * 3


# --------------------------------------------------------------------------------------------------- admission and aborts
@MODES
def test_a_group_waits_for_n_free_slots_and_nothing_overtakes_it(run_ahead, monkeypatch):
    w, tq = _worker(run_ahead, batch_size=5)              # 4 slots
    order = []
    real = w._install
    monkeypatch.setattr(w, "_install", lambda task, slot: (order.append(task), real(task, slot))[1])
    busy = [_task([3 + k, 1], max_tokens=12 + 4 * k) for k in range(3)]
    g = _group([8, 9, 10], 3, max_tokens=6)
    late = _task([4, 4], max_tokens=5)
    for t in busy + [g[0], late]:
        tq.put(t)
    held_seen = False
    for _ in range(3000):
        if w._held is g[0]:
            held_seen = True
            assert late not in order                      # the free slot is not given to the request behind the group
        if not w.step():
            break
    assert held_seen
    assert order == busy + [g[0], late]
    for t in g:
        assert t.generated_tokens == expected_stream([8, 9, 10], 6)
    assert late.generated_tokens == expected_stream([4, 4], 5)


@MODES
def test_a_group_larger_than_the_worker_ends_at_once(run_ahead):
    w, tq = _worker(run_ahead, batch_size=3)              # 2 slots
    g = _group([1, 2], 3)
    after = _task([5], max_tokens=3)
    tq.put(g[0])
    tq.put(after)
    _drain(w)
    assert all(t.request_status == RequestStatus.FINISHED_ABORTED and len(_completed(t)) == 1 and not _tokens(t) for t in g)
    assert after.generated_tokens == expected_stream([5], 3)


PROMPT = list(range(2, 50))                               # 48 tokens: chunked prefill over several steps


def _steps_until(w, cond, limit=500):
    for _ in range(limit):
        if cond():
            return
        w.step()
    raise AssertionError("condition never met")


@MODES
def test_abort_one_choice_before_the_fork(run_ahead, monkeypatch):
    forks = _spy_forks(monkeypatch)
    w, tq = _worker(run_ahead)
    g = _group(PROMPT, 3, max_tokens=8)
    tq.put(g[0])
    w.step()
    assert [w.state_slot[s]["state_category"] for s in (1, 2)] == [StateCategory.FORWARD_ONE_SUSPENDED] * 2
    g[1].task_event_queue.put(("abort", None))
    _drain(w)
    want = expected_stream(PROMPT, 8)
    assert g[1].request_status == RequestStatus.FINISHED_ABORTED and not _tokens(g[1]) and len(_completed(g[1])) == 1
    assert _tokens(g[0]) == _tokens(g[2]) == want
    assert forks == [[(0, [2])]]                          # the aborted choice gets no state


@MODES
def test_abort_one_choice_after_the_fork(run_ahead):
    w, tq = _worker(run_ahead)
    g = _group(PROMPT, 3, max_tokens=30)
    tq.put(g[0])
    _steps_until(w, lambda: len(_tokens(g[1])) >= 3)
    g[1].task_event_queue.put(("abort", None))
    _drain(w)
    want = expected_stream(PROMPT, 30)
    assert g[1].request_status == RequestStatus.FINISHED_ABORTED and 3 <= len(_tokens(g[1])) < 30
    assert _tokens(g[1]) == want[:len(_tokens(g[1]))]
    assert _tokens(g[0]) == _tokens(g[2]) == want


@MODES
def test_choice_0_aborted_before_the_fork_leaves_the_prefill_to_the_others(run_ahead, monkeypatch):
    forks = _spy_forks(monkeypatch)
    w, tq = _worker(run_ahead)
    g = _group(PROMPT, 3, max_tokens=8, cache_prefill=True, cache_prefill_padding=3)
    tq.put(g[0])
    w.step()
    g[0].task_event_queue.put(("abort", None))
    w.step()
    assert g[0].request_status == RequestStatus.FINISHED_ABORTED and len(_completed(g[0])) == 1
    assert w.state_slot[0]["task"] is g[0] and w.state_slot[0]["orphan"]           # its slot prefills on
    g[0].task_event_queue.put(("abort", None))                                    # (a second abort changes nothing)
    _drain(w)
    assert len(_completed(g[0])) == 1 and not _tokens(g[0])
    assert not [1 for t in g for kind, _ in t.output_queue.items if kind == "cache_prefill"]     # no export for a choice that left
    assert _tokens(g[1]) == _tokens(g[2]) == expected_stream(PROMPT, 8)
    assert forks == [[(0, [1, 2])]]
    assert all(td["state_category"] == StateCategory.EMPTY for td in w.state_slot.values())


@MODES
def test_all_choices_aborted_before_the_fork_stop_the_prefill(run_ahead, monkeypatch):
    forks = _spy_forks(monkeypatch)
    m = CountingModel()
    w, tq = _worker(run_ahead, model=m)
    w.max_forward_seq_len_per_forward = 10
    g = _group(list(range(1, 60)) * 3, 3, max_tokens=8)
    tq.put(g[0])
    w.step()
    w.step()
    for t in g:
        t.task_event_queue.put(("abort", None))
    fed = m.fed
    _drain(w)
    assert m.fed - fed <= 20 and not forks                # at most the chunks already under way
    for t in g:
        assert t.request_status == RequestStatus.FINISHED_ABORTED and len(_completed(t)) == 1 and not _tokens(t)
    assert all(td["state_category"] == StateCategory.EMPTY for td in w.state_slot.values()) and not w._groups
    after = _task([4, 5], max_tokens=4)                   # the slots are free again
    tq.put(after)
    _drain(w)
    assert after.generated_tokens == expected_stream([4, 5], 4)


@MODES
def test_the_prefix_cache_export_happens_once_and_a_hit_forks(run_ahead, monkeypatch):
    forks = _spy_forks(monkeypatch)
    w, tq = _worker(run_ahead)
    prompt = list(range(1, 31))
    g = _group(prompt, 3, max_tokens=6, cache_prefill=True, cache_prefill_padding=3)
    tq.put(g[0])
    _drain(w)
    exports = [[p for kind, p in t.output_queue.items if kind == "cache_prefill"] for t in g]
    assert [len(e) for e in exports] == [1, 0, 0]
    seen = list(exports[0][0]["prefilled_tokens"])
    assert seen == prompt[:len(seen)]
    hit = _group(prompt[len(seen):], 3, max_tokens=6)
    hit[0].state = [x.clone() for x in exports[0][0]["state"]]
    tq.put(hit[0])
    _drain(w)
    want = expected_stream(prompt, 6)
    assert [_tokens(t) for t in g + hit] == [want] * 6
    assert len(forks) == 2


# --------------------------------------------------------------------------------------------------- ops
def _tables(S, dtype, rng):
    L, C = 3, 16
    bits = {torch.float16: np.uint16, torch.float32: np.uint32}[dtype]
    shift = torch.from_numpy(rng.integers(0, np.iinfo(bits).max, (L, 2, S, C), dtype=np.uint64).astype(bits).view(
        np.float16 if dtype == torch.float16 else np.float32))
    wkv = torch.from_numpy(rng.integers(0, np.iinfo(bits).max, (L, S, 2, 4, 4), dtype=np.uint64).astype(bits).view(
        np.float16 if dtype == torch.float16 else np.float32))
    shift.view(-1)[:4] = torch.tensor([float("nan"), -0.0, float("inf"), -float("inf")], dtype=dtype)
    elapsed = torch.from_numpy(rng.integers(-(1 << 31), (1 << 31) - 1, S, dtype=np.int64).astype(np.int32))
    return [shift, wkv, elapsed]


def _bits(t):
    return t.numpy().view({2: np.uint16, 4: np.uint32}[t.element_size()])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_fork_states_cpu_form_copies_bits(dtype):
    rng = np.random.default_rng(7)
    S = 12
    pool = _tables(S, dtype, rng)
    before = [t.clone() for t in pool]
    groups = [(0, [3, 5]), (7, [1]), (2, []), (9, [4, 6, 8, 10, 11])]
    ops.fork_states(pool, groups)
    dst_of = {d: s for s, ds in groups for d in ds}
    for s in range(S):
        src = dst_of.get(s, s)
        assert np.array_equal(_bits(pool[0][:, :, s]), _bits(before[0][:, :, src])), s
        assert np.array_equal(_bits(pool[1][:, s]), _bits(before[1][:, src])), s
        assert int(pool[2][s]) == int(before[2][src]), s
    ops.fork_states(pool, [])
    for bad in ([(0, [1, 1])], [(0, [1]), (2, [1])], [(0, [2]), (2, [3])], [(0, [0])], [(0, [S])], [(-1, [2])], [(S, [2])]):
        with pytest.raises(ChirrupAmdError):
            ops.fork_states([t.clone() for t in before], bad)
    with pytest.raises(ChirrupAmdError):
        ops.fork_states([before[0][:, 0], before[1], before[2]], [(0, [1])])


def test_seeded_uniform_host_form_with_streams():
    seeds = torch.tensor([5, 5, 5, -9, 5], dtype=torch.int64)
    seeded = torch.tensor([1, 2, 16, 4, 0], dtype=torch.int32)
    counters = torch.tensor([0, 0, 7, -1, 0], dtype=torch.int32)
    slot_idx = torch.arange(5, dtype=torch.int32)
    u = torch.full((5,), 0.5, dtype=torch.float32)
    ops.seeded_uniform(slot_idx, slot_idx, seeds, seeded, counters, u)
    assert u.tolist() == [float(ops.philox_uniform(5, 0)), float(ops.philox_uniform(5, 0, 1)), float(ops.philox_uniform(5, 7, 15)),
                          float(ops.philox_uniform(-9, 0xFFFFFFFF, 3)), 0.5]
    assert counters.tolist() == [1, 1, 8, 0, 0]
    assert len(set(u.tolist()[:2])) == 2
    i = np.arange(64, dtype=np.uint64)
    assert np.array_equal(ops.philox_uniform(77, i), ops.philox_uniform(77, i, 0))          # stream 0 is the single request's
    x = ops.philox4x32_10(np.stack([i, np.full_like(i, 3), 0 * i, 0 * i], -1), np.array([77, 0], np.uint64))[:, 0]
    assert np.array_equal(ops.philox_uniform(77, i, 3).astype(np.float64), (x >> 8).astype(np.float64) / 2 ** 24)


def test_fork_kernel_has_no_scratch_and_no_spills():
    from test_kernel_budget_cpu import CSRC, FLAGS, HIPCC

    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "elementwise.hip"), "-o", os.devnull], capture_output=True, text=True,
                         cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    report, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs): (\d+)", line)
        if m and cur is not None and "fork_states_kernel" in cur:
            report[m.group(1)] = int(m.group(2))
    assert report.get("ScratchSize [bytes/lane]") == 0 and report.get("VGPRs Spill") == 0 and report.get("SGPRs Spill") == 0, report
    assert report["VGPRs"] <= 128, report


def test_fork_states_entry_point_checks_its_arguments():
    import ctypes

    import chirrup_amd
    from chirrup_amd import lib

    hdr = open(os.path.join(ROOT, "include", "chirrup_amd.h")).read()
    assert re.search(r"int rwkv7_fork_states\(int n_groups, int L, int S, int C, int H, const int32_t \*src, const int32_t \*dst_offs", hdr)
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    f = chirrup_amd.load().rwkv7_fork_states
    assert len(lib.SIGNATURES["rwkv7_fork_states"][1]) == 12
    p = ctypes.c_void_p(4096)                             # never dereferenced: validation fails first (or nothing to do)
    assert f(-1, 2, 4, 128, 2, p, p, p, p, p, p, None) == -1
    assert f(0, 0, 0, 0, 0, None, None, None, None, None, None, None) == 0
    for bad in ((1, 0, 4, 128, 2), (1, 2, 0, 128, 2), (1, 2, 4, 100, 2), (1, 2, 4, 128, 1), (70000, 2, 4, 128, 2)):
        assert f(*bad, p, p, p, p, p, p, None) == -1, bad
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert f(1, 2, 4, 128, 2, *args, None) == -2, k
    assert f(1, 2, 4, 128, 2, p, p, p, ctypes.c_void_p(4104), p, p, None) == -3
    assert f(1, 2, 4, 128, 2, p, p, p, p, ctypes.c_void_p(4104), p, None) == -3
    assert f(1, 2, 4, 128, 2, p, p, p, p, p, ctypes.c_void_p(4098), None) == -3


# --------------------------------------------------------------------------------------------------- task, wire, engine
def test_task_validates_groups():
    with pytest.raises(ValueError):
        _task([1], siblings=[_task([1], choice_index=2)])
    with pytest.raises(ValueError):
        _task([1], siblings=[_task([1], choice_index=1)], prompt_logprobs=2)
    with pytest.raises(ValueError):
        _task([1], siblings=[_task([1], choice_index=1, max_tokens=0)])
    with pytest.raises(ValueError):
        _task([1], choice_index=1, siblings=[_task([1], choice_index=1)])
    with pytest.raises(ValueError):
        _task([1], choice_index=-1)
    g = _group([1, 2], 3)
    assert [t.choice_index for t in g] == [0, 1, 2] and g[0].siblings == g[1:]


def test_the_process_mode_wire_carries_a_group_whole():
    from chirrup_amd.engine_process import RemoteTaskQueue, task_to_wire

    g = _group([3, 1, 4], 3, seed=11, logit_bias={5: 1.0}, max_tokens=7)
    d = task_to_wire(g[0])
    assert "siblings" not in task_to_wire(_task([1]))      # a single choice travels as before
    task_q, result_q = queue.Queue(), queue.Queue()
    task_q.put(d)
    rq = RemoteTaskQueue(task_q, result_q, "w3")
    rq.deliver_abort(g[2].task_id)                         # an abort that arrives before the pull
    t = rq.get_nowait()
    assert [x.task_id for x in [t] + t.siblings] == [x.task_id for x in g]
    assert [x.choice_index for x in [t] + t.siblings] == [0, 1, 2]
    for x, y in zip([t] + t.siblings, g):
        assert (x.prefill_tokens, x.seed, x.logit_bias, x.max_tokens, x.state) == (y.prefill_tokens, y.seed, y.logit_bias, y.max_tokens, None)
    accepted = [result_q.get_nowait() for _ in range(3)]
    assert sorted(a[0] for a in accepted) == sorted(x.task_id for x in g) and all(a[1] == ("__accepted__", "w3") for a in accepted)
    assert set(rq.local_events) == {x.task_id for x in g}
    assert t.siblings[1].task_event_queue.get_nowait() == ("abort", None) and t.siblings[0].task_event_queue.empty()
    t.siblings[0].output_queue.put_nowait(("token_generated", (7, "<7>")))
    assert result_q.get_nowait() == (g[1].task_id, ("token_generated", (7, "<7>")))


def _engine(loop_batch=4, **kw):
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=_VocabTok(), **kw)
    return eng, eng.init(worker_num=1, model_config=ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64),
                         batch_size=loop_batch)


def test_engine_completions():
    async def main():
        eng, init = _engine()
        await init
        kw = dict(temperature=1.0, top_p=1.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, stop_tokens=[],
                  max_tokens=9, seed=123)
        prompt = [2, 7, 1, 8]
        for bad in (dict(n=0), dict(n=4), dict(n=True), dict(n=2, prompt_logprobs=1), dict(n=2, max_tokens=0)):
            with pytest.raises(ValueError):
                eng.completions("", prefill_tokens=prompt, **dict(kw, **bad))
        single = eng.completions("", prefill_tokens=prompt, n=1, **kw)
        assert len(single) == 1 and not single[0].task.siblings
        cs = eng.completions("", prefill_tokens=prompt, n=3, **kw)
        assert [c.task.choice_index for c in cs] == [0, 1, 2] and cs[0].task.siblings == [c.task for c in cs[1:]]
        streams = await asyncio.gather(*[_collect(c) for c in reversed(cs)])       # any choice may start first: one submission
        assert streams[::-1] == [_seeded_stream(prompt, 9, 123, j) for j in range(3)]
        assert [t async for t in _agen(single[0])] == _seeded_stream(prompt, 9, 123, 0)
        assert eng.task_queue.empty()
        eng.shutdown()

    asyncio.run(main())


async def _collect(c):
    return [ev[1] async for ev in c if ev[0] == "token"]


async def _agen(c):
    async for ev in c:
        if ev[0] == "token":
            yield ev[1]


def _process_factory(**kw):
    return Worker(model=FakeModel(), tokenizer=_Tok(), penalize_argmax=cpu_penalize_argmax, **kw)


def test_process_mode_group_end_to_end():
    async def main():
        eng = AsyncEngineCore(worker_factory=_process_factory, tokenizer=_Tok(), worker_mode="process")
        cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
        await asyncio.wait_for(eng.init(worker_num=2, model_config=cfg, batch_size=5), 120)
        kw = dict(temperature=0.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, stop_tokens=[])
        prompt = [3, 1, 4, 1, 5, 9, 2, 6]
        cs = eng.completions("", prefill_tokens=prompt, n=4, max_tokens=6, **kw)
        got = await asyncio.wait_for(asyncio.gather(*[_collect(c) for c in cs]), 60)
        assert got == [expected_stream(prompt, 6)] * 4
        cs = eng.completions("", prefill_tokens=prompt, n=3, max_tokens=10 ** 6, **kw)
        it = cs[1].__aiter__()
        for _ in range(3):
            await asyncio.wait_for(it.__anext__(), 60)
        cs[1].abort()
        rest = [ev async for ev in it]
        assert str(cs[1].task.request_status) == "FINISHED_ABORTED" and len(rest) < 10 ** 5
        for c in (cs[0], cs[2]):
            c.abort()
            [ev async for ev in c]
            assert str(c.task.request_status) == "FINISHED_ABORTED"
        assert not eng._router.owner                        # every choice has left the router's books
        eng.shutdown()

    asyncio.run(main())


# --------------------------------------------------------------------------------------------------- the chat route
class _VocabTok(_Tok):
    idx2token = {i: f"t{i}".encode() for i in range(V)}


async def _client(record):
    eng, init = _engine()
    await init
    real = eng.completions

    def completions(*a, **kw):
        cs = real(*a, **kw)
        record.append(cs)
        return cs

    eng.completions = completions
    return eng, httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(eng, state_cache_size=0)), base_url="http://t")


REQ = {"model": "rwkv-latest:no-thinking", "messages": [{"role": "user", "content": "three ways"}], "temperature": 1.0, "top_p": 1.0,
       "presence_penalty": 0.0, "frequency_penalty": 0.0, "penalty_decay": 1.0, "max_tokens": 7, "seed": 99}


def _chat_tokens():
    prompt, _ = chat_prompt([type("M", (), {"role": "user", "content": "three ways"})()], REQ["model"])
    return [0] + _Tok().encode(prompt)


def _chat_stream(j):
    return _seeded_stream(_chat_tokens(), REQ["max_tokens"], REQ["seed"], j, stop=(0, 261, 24281))


def test_chat_n_streamed():
    async def main():
        record = []
        eng, cl = await _client(record)
        async with cl:
            r = await cl.post("/v1/chat/completions", json=dict(REQ, n=3, stream=True))
            assert r.status_code == 200
            events = [e[len("data: "):] for e in r.text.split("\n\n") if e.startswith("data: ")]
        assert events[-1] == "[DONE]" and events.count("[DONE]") == 1
        chunks = [json.loads(e) for e in events[:-1]]
        assert all(len(c["choices"]) == 1 for c in chunks)
        by = {j: [c["choices"][0] for c in chunks if c["choices"][0]["index"] == j] for j in range(3)}
        assert sorted({c["choices"][0]["index"] for c in chunks}) == [0, 1, 2]
        for j, cs in by.items():
            finish = [c for c in cs if c["finish_reason"] is not None]
            assert len(finish) == 1 and finish[0] is cs[-1] and finish[0]["finish_reason"] == "stop" and finish[0]["delta"] == {}
            text = "".join(c["delta"].get("content", "") for c in cs)
            assert text == "".join(f"<{t}>" for t in _chat_stream(j)), j
        assert len({tuple(_chat_stream(j)) for j in range(3)}) == 3
        assert len(record) == 1 and len(record[0]) == 3
        eng.shutdown()

    asyncio.run(main())


def test_chat_n_whole_body():
    async def main():
        record = []
        eng, cl = await _client(record)
        async with cl:
            r = await cl.post("/v1/chat/completions", json=dict(REQ, n=3, logprobs=True, top_logprobs=2))
            assert r.status_code == 200, r.text
            body = r.json()
        assert [c["index"] for c in body["choices"]] == [0, 1, 2]
        n_out = 0
        for j, c in enumerate(body["choices"]):
            want = _chat_stream(j)
            assert c["message"]["content"] == "".join(f"<{t}>" for t in want) and c["finish_reason"] == "stop"
            assert [e["token"] for e in c["logprobs"]["content"]] == [f"t{t}" for t in want]
            n_out += len(want)
        assert body["usage"] == {"prompt_tokens": len(_chat_tokens()), "completion_tokens": n_out, "total_tokens": len(_chat_tokens()) + n_out}
        eng.shutdown()

    asyncio.run(main())


def test_chat_n_1_is_todays_body_and_bad_n_is_refused():
    async def main():
        record = []
        eng, cl = await _client(record)
        async with cl:
            plain = await cl.post("/v1/chat/completions", json=REQ)
            one = await cl.post("/v1/chat/completions", json=dict(REQ, n=1))
            assert plain.status_code == one.status_code == 200
            a, b = plain.json(), one.json()
            for x in (a, b):
                assert x.pop("id").startswith("chatcmpl-") and isinstance(x.pop("created"), int)
            want = "".join(f"<{t}>" for t in _chat_stream(0))
            n = len(_chat_stream(0))
            assert a == b == {"object": "chat.completion", "model": REQ["model"],
                              "choices": [{"index": 0, "finish_reason": "stop",
                                           "message": {"role": "assistant", "content": want, "reasoning_content": ""}}],
                              "usage": {"prompt_tokens": len(_chat_tokens()), "completion_tokens": n, "total_tokens": len(_chat_tokens()) + n}}
            assert list(b) == ["object", "model", "choices", "usage"]
            s1 = await cl.post("/v1/chat/completions", json=dict(REQ, stream=True))
            s2 = await cl.post("/v1/chat/completions", json=dict(REQ, stream=True, n=1))
            strip = lambda t: re.sub(r'"(id|created)": ("[^"]*"|\d+)', "", t)
            assert strip(s1.text) == strip(s2.text) and s1.text.count("[DONE]") == 1
            assert not record                                # n = 1 never goes through completions()
            big = await cl.post("/v1/chat/completions", json=dict(REQ, n=4))
            assert big.status_code == 400 and "n = 4" in big.text
            for bad in (0, -1, 129, "x", 1.5):
                r = await cl.post("/v1/chat/completions", json=dict(REQ, n=bad))
                assert r.status_code == 422, bad
            assert not record
        eng.shutdown()

    asyncio.run(main())
