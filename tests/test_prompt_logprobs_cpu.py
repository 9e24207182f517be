"""Prompt logprobs without a GPU: the worker's bookkeeping of prompt rows (chunked prefill, single-token prefill, scoring-only
requests) over a fake model that honours ``logit_rows`` and the torch form of ops.token_logprobs, and POST /v1/completions over the
fake-backend engine."""
import asyncio
import json
import math
import queue

import httpx
import pytest
import torch

from chirrup_amd.core_structure import ModelLoadConfig, RequestStatus, Task
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.web_service import CompletionRequest, create_app, legacy_top
from chirrup_amd.worker import Worker
from test_engine_cpu import _Tok
from test_worker_cpu import V, FakeModel, FakeTok, Sink, cpu_penalize_argmax, expected_stream


def _row(h):
    out = torch.zeros((V,), dtype=torch.float16)
    out[h % V], out[(h + 1) % V] = 5.0, 4.0
    return out


class RowModel(FakeModel):
    """FakeModel with forward_slots(logit_rows=..., row_sink=...): the logits after every token of a chunk."""

    def __init__(self, block=7):
        self.block, self.calls = block, []

    def forward_slots(self, tokens, pool, slot_idx, full_output=False, logit_rows=None, row_sink=None):
        if logit_rows is None:
            return super().forward_slots(tokens, pool, slot_idx, full_output)
        T = len(tokens[0])
        per_row = []
        for toks, s in zip(tokens, slot_idx.tolist()):
            h = int(pool[1][0, s, 0, 0, 0])
            for t in toks:
                h = self.advance(h, int(t))
                per_row.append(_row(h))
        out = super().forward_slots(tokens, pool, slot_idx)
        rows = torch.stack(per_row)[logit_rows.long()]
        self.calls.append((len(tokens), T, logit_rows.tolist()))
        if row_sink is None:
            return out, rows
        for r0 in range(0, rows.shape[0], self.block):
            row_sink(r0, rows[r0:r0 + self.block].contiguous())
        return out, None


def make_worker(run_ahead=True, batch_size=6, model=None):
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    w = Worker("w0", [], cfg, queue.Queue(), queue.Queue(), queue.Queue(), batch_size=batch_size,
               model=model if model is not None else RowModel(), tokenizer=FakeTok(), penalize_argmax=cpu_penalize_argmax,
               run_ahead=run_ahead)
    w._init_worker()
    return w


def new_task(prompt, **kw):
    for key, v in (("temperature", 0.0), ("frequency_penalty", 0.0), ("presence_penalty", 0.0), ("penalty_decay", 1.0),
                   ("stop_tokens", [])):
        kw.setdefault(key, v)
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **kw)


def run_until_idle(w, max_iter=5000):
    for _ in range(max_iter):
        if not w.step():
            return
    raise AssertionError("worker did not drain")


def expected_prompt(prompt, k):
    """Host recomputation: position i >= 1 = log_softmax(logits after prompt[:i])[prompt[i]], and the k most likely ids."""
    lps, tops, h = [None], [None], 0
    for i in range(1, len(prompt)):
        h = FakeModel.advance(h, prompt[i - 1])
        x = [float(v) for v in _row(h).tolist()]
        m = max(x)
        z = math.log(sum(math.exp(v - m) for v in x))
        lp = [(v - m) - z for v in x]
        lps.append(lp[prompt[i]])
        order = sorted(range(V), key=lambda j: (-x[j], j))[:k]
        tops.append([(j, lp[j]) for j in order])
    return lps, tops


def prompt_messages(task):
    return [p for kind, p in task.output_queue.items if kind == "prompt_logprobs"]


def joined(task):
    msgs = prompt_messages(task)
    pos = 0
    ids, lps, tops = [], [], []
    for m in msgs:
        assert m["start"] == pos, "prompt_logprobs out of position order"
        pos += len(m["logprobs"])
        ids += m["token_ids"]
        lps += m["logprobs"]
        tops += m["top_logprobs"]
    return ids, lps, tops


def check_prompt(task, prompt, k):
    ids, lps, tops = joined(task)
    want_lp, want_top = expected_prompt(prompt, k)
    assert ids == list(prompt) and len(lps) == len(prompt)
    assert lps[0] is None and tops[0] is None
    for got, want in zip(lps[1:], want_lp[1:]):
        assert abs(got - want) < 1e-5
    for got, want in zip(tops[1:], want_top[1:]):
        assert [i for i, _ in got] == [i for i, _ in want]
        assert all(abs(a - b) < 1e-5 for (_, a), (_, b) in zip(got, want))
    kinds = [kind for kind, _ in task.output_queue.items]
    if "token_generated" in kinds:           # every prompt message before the first token
        first = kinds.index("token_generated")
        assert all(i < first for i, kind in enumerate(kinds) if kind == "prompt_logprobs")


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, V, (n,), generator=g).tolist()


LENGTHS = [1, 2, 9, 10, 101, 250]


@pytest.mark.parametrize("run_ahead", [True, False])
@pytest.mark.parametrize("padding", [0, 3])
def test_positions_and_targets_match_host_recomputation(run_ahead, padding):
    w = make_worker(run_ahead)
    tasks = []
    for i, n in enumerate(LENGTHS):
        p = _prompt(n, 10 + i)
        t = new_task(p, max_tokens=4, prompt_logprobs=[0, 3, 20, 1, 5, 2][i], cache_prefill=padding > 0,
                     cache_prefill_padding=padding)
        plain = new_task(_prompt(n + 5, 50 + i), max_tokens=3)          # non-asking neighbours in the same batches
        tasks.append((t, p, plain))
        w.task_queue.put(t)
        w.task_queue.put(plain)
    run_until_idle(w)
    for t, p, plain in tasks:
        check_prompt(t, p, t.prompt_logprobs)
        gen = [x[1][0] for x in t.output_queue.items if x[0] == "token_generated"]
        assert gen == expected_stream(p, 4)
        assert prompt_messages(plain) == []
    assert any(T > 1 for _, T, _ in w.model.calls)          # chunks were scored (and blocks went through the sink)


def _stream(run_ahead, with_neighbour):
    w = make_worker(run_ahead)
    asks = [new_task(_prompt(n, 100 + n), max_tokens=3, prompt_logprobs=2, logprobs=True, top_logprobs=1) for n in (2, 9, 37, 130)]
    score = [new_task(_prompt(n, 200 + n), max_tokens=0, prompt_logprobs=1) for n in (1, 5, 64)]
    plain = new_task(_prompt(120, 7), max_tokens=5, logprobs=True)
    for t in ([plain] + (asks + score if with_neighbour else [])):
        w.task_queue.put(t)
    run_until_idle(w)
    return strip(plain.output_queue.items), [strip(t.output_queue.items) for t in asks + score] if with_neighbour else None


def strip(items):
    """A task's messages with consecutive prompt_logprobs messages merged: how a prompt is cut into forwards depends on when the
    slots of other requests free up, which differs between the two scheduling modes; what each position carries does not."""
    out = []
    for k, p in items:
        if k == "prompt_logprobs" and out and out[-1][0] == k:
            prev = out[-1][1]
            out[-1] = (k, {key: prev[key] + p[key] if key != "start" else prev[key] for key in p})
        else:
            out.append((k, p[:2] if k == "token_generated" else (p.request_status if k == "task_completed" else dict(p))))
    return out


def test_run_ahead_and_in_step_give_identical_streams():
    a_plain, a = _stream(True, True)
    b_plain, b = _stream(False, True)
    assert a == b and a_plain == b_plain


def test_non_asking_request_unchanged_by_asking_neighbours():
    for ra in (True, False):
        alone, _ = _stream(ra, False)
        mixed, _ = _stream(ra, True)
        assert alone == mixed


@pytest.mark.parametrize("run_ahead", [True, False])
@pytest.mark.parametrize("n", [1, 2, 9, 10, 101, 250])
def test_scoring_only_feeds_no_last_token_and_samples_nothing(run_ahead, n):
    w = make_worker(run_ahead)
    p = _prompt(n, 300 + n)
    t = new_task(p, max_tokens=0, prompt_logprobs=3)
    w.task_queue.put(t)
    run_until_idle(w)
    kinds = [k for k, _ in t.output_queue.items]
    assert "token_generated" not in kinds and kinds[-1] == "task_completed"
    assert t.request_status == RequestStatus.FINISHED_LENGTH_CAPPED and t.generated_tokens == []
    check_prompt(t, p, 3)
    if n == 1:
        assert prompt_messages(t) == [{"start": 0, "token_ids": p, "logprobs": [None], "top_logprobs": [None]}]
    # every prompt token but the last was fed (the fake counts fed tokens in the slots' step counters)
    assert int(w.batch_state[2].sum()) == n - 1
    assert all(td["task"] is None for td in w.state_slot.values())


def test_scoring_only_after_abort_and_max_tokens_zero_without_prompt_logprobs():
    w = make_worker(True)
    t = new_task(_prompt(150, 1), max_tokens=0, prompt_logprobs=0)
    w.task_queue.put(t)
    w.step()
    t.task_event_queue.put(("abort", None))
    run_until_idle(w)
    assert t.request_status == RequestStatus.FINISHED_ABORTED
    assert all(m["start"] + len(m["logprobs"]) <= 150 for m in prompt_messages(t))
    # max_tokens=0 without prompt_logprobs keeps its old behaviour (one token)
    t0 = new_task(_prompt(12, 2), max_tokens=0)
    w.task_queue.put(t0)
    run_until_idle(w)
    assert len(t0.generated_tokens) == 1 and prompt_messages(t0) == []


def test_task_validates_prompt_logprobs():
    for bad in (-1, 21, 2.5, True):
        with pytest.raises(ValueError):
            new_task([1, 2], prompt_logprobs=bad)
    assert new_task([1, 2], prompt_logprobs=20).prompt_logprobs == 20 and new_task([1]).prompt_logprobs is None


def test_legacy_top_keeps_the_higher_of_two_ids_with_one_string():
    table = {1: b"a", 2: b"a", 3: b"\xff"}
    assert legacy_top(table, [(1, -2.0), (2, -1.0), (3, -3.0)]) == {"a": -1.0, "\\xff": -3.0}
    assert legacy_top(table, None) is None


# ---------------------------------------------------------------------------------------------- POST /v1/completions
class _VocabTok(_Tok):
    idx2token = {i: f"t{i}".encode() for i in range(V)}


def _factory(**kw):
    return Worker(model=RowModel(), tokenizer=_VocabTok(), penalize_argmax=cpu_penalize_argmax, **kw)


async def _client(state_cache_size=0):
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=_VocabTok())
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    await eng.init(worker_num=1, model_config=cfg, batch_size=6)
    app = create_app(eng, state_cache_size=state_cache_size)
    return eng, httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t")


GREEDY = {"temperature": 0.0, "top_p": 0.0, "presence_penalty": 0.0, "frequency_penalty": 0.0, "penalty_decay": 1.0}


def test_completions_request_defaults_and_validation():
    r = CompletionRequest(prompt="hi")
    assert (r.max_tokens, r.echo, r.logprobs, r.stream, r.pad_zero, r.n) == (16, False, None, False, True, 1)
    assert CompletionRequest(prompt=[1, 2]).prompts() == [[1, 2]]
    assert CompletionRequest(prompt=["a", [3]]).prompts() == ["a", [3]]
    for bad in ({"prompt": "x", "max_tokens": 0}, {"prompt": "x", "logprobs": 21}, {"prompt": []},
                {"prompt": "x", "logit_bias": {"a": 1}}, {"prompt": "x", "temperature": 3}):
        with pytest.raises(Exception):
            CompletionRequest(**bad)


def test_completions_echo_logprobs_scoring_and_generation():
    async def main():
        eng, cl = await _client()
        async with cl:
            text = "scored text"
            ids = _VocabTok().encode(text)
            toks = [0] + ids
            # scoring only: echo + logprobs + max_tokens=0
            r = await cl.post("/v1/completions", json=dict(GREEDY, prompt=text, echo=True, logprobs=2, max_tokens=0))
            assert r.status_code == 200
            j = r.json()
            assert j["object"] == "text_completion" and j["id"].startswith("cmpl-")
            c = j["choices"][0]
            want_lp, want_top = expected_prompt(toks, 2)
            assert c["text"] == text and c["finish_reason"] == "length" and c["index"] == 0
            lp = c["logprobs"]
            assert lp["tokens"] == [f"t{i}" for i in ids]
            assert all(abs(a - b) < 1e-5 for a, b in zip(lp["token_logprobs"], want_lp[1:]))   # the first echoed token: given token 0
            assert lp["text_offset"] == [sum(len(f"t{i}") for i in ids[:n]) for n in range(len(ids))]
            assert all(set(d) == {f"t{i}" for i, _ in w} for d, w in zip(lp["top_logprobs"], want_top[1:]))
            assert j["usage"] == {"prompt_tokens": len(toks), "completion_tokens": 0, "total_tokens": len(toks)}
            # token-list prompt without pad_zero: the first position is null
            r = await cl.post("/v1/completions", json=dict(GREEDY, prompt=ids, echo=True, logprobs=0, max_tokens=0, pad_zero=False))
            lp = r.json()["choices"][0]["logprobs"]
            assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None and len(lp["tokens"]) == len(ids)
            # echo + generation + logprobs, stop -> finish_reason
            gen = expected_stream(toks, 5, stop=(0,))          # (the route keeps the default stop tokens, 0 among them)
            r = await cl.post("/v1/completions", json=dict(GREEDY, prompt=text, echo=True, logprobs=1, max_tokens=5))
            c = r.json()["choices"][0]
            assert c["text"] == text + "".join(f"<{t}>" for t in gen) and c["finish_reason"] == "length"
            assert c["logprobs"]["tokens"] == [f"t{i}" for i in ids + gen]
            assert r.json()["usage"]["completion_tokens"] == 5
            assert len(gen) == 5
            cut = gen.index(gen[2])                              # _Tok encodes chr(t - 1) as token t
            r = await cl.post("/v1/completions", json=dict(GREEDY, prompt=text, max_tokens=5, stop=[chr(gen[2] - 1)]))
            c = r.json()["choices"][0]
            assert c["finish_reason"] == "stop" and c["text"] == "".join(f"<{t}>" for t in gen[:cut])
            assert c["logprobs"] is None
            # batched prompts: one choice each, in order; usage sums
            r = await cl.post("/v1/completions", json=dict(GREEDY, prompt=["ab", [5, 6, 7]], max_tokens=3))
            j = r.json()
            assert [c["index"] for c in j["choices"]] == [0, 1]
            g0, g1 = expected_stream([0] + _VocabTok().encode("ab"), 3, stop=(0,)), expected_stream([0, 5, 6, 7], 3, stop=(0,))
            assert j["choices"][0]["text"] == "".join(f"<{t}>" for t in g0)
            assert j["choices"][1]["text"] == "".join(f"<{t}>" for t in g1)
            assert j["usage"] == {"prompt_tokens": 3 + 4, "completion_tokens": len(g0) + len(g1), "total_tokens": 7 + len(g0) + len(g1)}
            # echo without logprobs and max_tokens=0: answered without running anything
            r = await cl.post("/v1/completions", json=dict(prompt="xyz", echo=True, max_tokens=0))
            assert r.json()["choices"][0] == {"text": "xyz", "index": 0, "logprobs": None, "finish_reason": "length"}
            # errors
            assert (await cl.post("/v1/completions", json=dict(prompt="x", n=2))).status_code == 400
            assert (await cl.post("/v1/completions", json=dict(prompt="x", best_of=3))).status_code == 400
            assert (await cl.post("/v1/completions", json=dict(prompt=[1, V + 5]))).status_code == 400
            assert (await cl.post("/v1/completions", json=dict(prompt="x", logit_bias={str(V): 1}))).status_code == 400
            assert (await cl.post("/v1/completions", json=dict(prompt="x", max_tokens=0))).status_code == 422
            assert (await cl.post("/v1/completions", json=dict(prompt="x", logprobs=25))).status_code == 422
        eng.shutdown()

    asyncio.run(main())


def test_completions_streamed_echo_first_chunk_carries_the_prompt():
    async def main():
        eng, cl = await _client(state_cache_size=4)
        async with cl:
            text = "stream me"
            ids = _VocabTok().encode(text)
            gen = expected_stream([0] + ids, 4, stop=(0,))
            assert len(gen) == 4
            r = await cl.post("/v1/completions", json=dict(GREEDY, prompt=text, echo=True, logprobs=1, max_tokens=4, stream=True))
            assert r.headers["content-type"].startswith("text/event-stream")
            lines = [x[len("data: "):] for x in r.text.split("\n\n") if x.startswith("data: ")]
            assert lines[-1] == "[DONE]"
            chunks = [json.loads(x)["choices"][0] for x in lines[:-1]]
            assert chunks[0]["text"] == text and chunks[0]["logprobs"]["tokens"] == [f"t{i}" for i in ids]
            assert [c["text"] for c in chunks[1:-1]] == [f"<{t}>" for t in gen]
            assert all(c["logprobs"]["tokens"] == [f"t{t}"] for c, t in zip(chunks[1:-1], gen))
            assert chunks[-1]["finish_reason"] == "length" and all(c["finish_reason"] is None for c in chunks[:-1])
            # same request, one body: the same tokens and logprobs
            r2 = await cl.post("/v1/completions", json=dict(GREEDY, prompt=text, echo=True, logprobs=1, max_tokens=4))
            body = r2.json()["choices"][0]["logprobs"]
            assert body["token_logprobs"] == chunks[0]["logprobs"]["token_logprobs"] + [c["logprobs"]["token_logprobs"][0] for c in chunks[1:-1]]
        eng.shutdown()

    asyncio.run(main())
