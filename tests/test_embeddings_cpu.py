"""Text embeddings without a GPU: Task validation, the host form of ops.pool_rows against a plain numpy loop, embeddings.finish, the
worker's embedding requests over a fake backend (alone, beside generating requests, slot reuse, abort; both run-ahead modes), the
engine's embed() and POST /v1/embeddings on the fake backend, and the C ABI of rwkv7_pool_rows."""
import asyncio
import base64
import ctypes
import os
import queue
import re

import numpy as np
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import ModelLoadConfig, RequestStatus, Task
from chirrup_amd.embeddings import finish
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.worker import StateCategory, Worker
from test_worker_cpu import FakeModel, FakeTok, Sink, V, cpu_penalize_argmax, expected_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 8
LENGTHS = (1, 2, 3, 9, 17, 40)


def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------- Task
def new_task(prompt, **kw):
    kw.setdefault("temperature", 0.0)
    kw.setdefault("frequency_penalty", 0.0)
    kw.setdefault("presence_penalty", 0.0)
    kw.setdefault("penalty_decay", 1.0)
    kw.setdefault("stop_tokens", [])
    kw.setdefault("state", None)
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), **kw)


def test_task_embedding_fields_and_refusals():
    t = new_task([1, 2, 3])
    assert (t.embed, t.embed_skip, t.embed_normalize) == (None, 0, True)
    t = new_task([0, 1, 2], embed="mean", embed_skip=1, embed_normalize=False)
    assert (t.embed, t.embed_skip, t.embed_normalize) == ("mean", 1, False)
    assert new_task([5], embed="last").embed == "last"
    from chirrup_amd.guided import compile_regex

    state = [torch.zeros(1), torch.zeros(1), torch.zeros(1)]
    pairs = {"logprobs": dict(logprobs=True), "prompt_logprobs": dict(prompt_logprobs=0), "return_logits": dict(return_logits=True),
             "guide": dict(guide=compile_regex("a+"), stop_tokens=[0]), "siblings": dict(siblings=[new_task([1], choice_index=1)]),
             "choice_index": dict(choice_index=1), "cache_prefill": dict(cache_prefill=True), "state": dict(state=state)}
    for name, kw in pairs.items():
        with pytest.raises(ValueError, match=f"embed.*{name}"):
            new_task([1, 2], embed="mean", **kw)
        new_task([1, 2], **kw)                               # the same fields without embed are fine
    with pytest.raises(ValueError, match="pooling"):
        new_task([1, 2], embed="max")
    for prompt, skip in (([], 0), ([0], 1), ([1, 2], 2), ([1, 2], 5), ([1, 2], -1)):
        with pytest.raises((ValueError, IndexError)):
            new_task(prompt, embed="mean", embed_skip=skip)
    # sampling fields are ignored
    assert new_task([1], embed="mean", temperature=1.5, top_p=0.2, top_k=3, max_tokens=0, seed=4, logit_bias={1: 2.0}).embed == "mean"
    # a group assembled afterwards is refused too
    t = new_task([1, 2], embed="mean")
    t.siblings = [new_task([1, 2], choice_index=1)]
    with pytest.raises(ValueError, match="embed"):
        t.check_group()


# ---------------------------------------------------------------------------------------------- ops.pool_rows, host form
def numpy_pool(xo, seq, t0, slot, acc_sum, acc_last, acc_count):
    """The contract as a plain loop: one np.float32 addition per channel and token, in token order."""
    B, T, C_ = xo.shape
    for b, a, s in zip(seq, t0, slot):
        if not 0 <= b < B or not 0 <= s < acc_count.shape[0]:
            continue
        for t in range(a, T):
            for c in range(C_):
                acc_sum[s, c] = np.float32(acc_sum[s, c] + np.float32(xo[b, t, c]))
        if a < T:
            acc_last[s] = xo[b, T - 1]
            acc_count[s] += T - a


def special_rows(rng, B, T, C_):
    x = (rng.standard_normal((B, T, C_)) * 8).astype(np.float16)
    flat = x.reshape(-1)
    vals = np.array([-0.0, 0.0, 6e-8, -6e-8, 5.96e-8, 65504.0, -65504.0, 6.1e-5], np.float16)
    flat[rng.choice(flat.size, size=min(flat.size, 3 * len(vals)), replace=False)] = np.resize(vals, min(flat.size, 3 * len(vals)))
    return x


def sentinel_tables(n, C_):
    return (np.full((n, C_), 1234.5, np.float32), np.full((n, C_), -7.25, np.float16), np.full((n,), 77, np.int32))


@pytest.mark.parametrize("T", [1, 2, 7])
def test_pool_rows_host_equals_the_numpy_loop(T):
    rng = np.random.default_rng(T)
    B, n = 5, 9
    x = special_rows(rng, B, T, C)
    for t0 in sorted({0, min(1, T), T - 1, T}):
        seq, slot, t0s = [3, 0, 4], [7, 2, 5], [t0, 0, T if t0 == 0 else t0]
        want = sentinel_tables(n, C)
        for s in slot:                                       # a listed slot continues ITS running values
            want[0][s], want[1][s], want[2][s] = rng.standard_normal(C).astype(np.float32), 0, 3
        got = [torch.from_numpy(w.copy()) for w in want]
        numpy_pool(x, seq, t0s, slot, *want)
        ops.pool_rows(torch.from_numpy(x), i32(*seq), i32(*t0s), i32(*slot), *got)
        assert np.array_equal(got[0].numpy().view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[1].numpy().view(np.uint16), want[1].view(np.uint16))
        assert np.array_equal(got[2].numpy(), want[2])
        unlisted = [s for s in range(n) if s not in slot]
        assert (got[0].numpy()[unlisted] == 1234.5).all() and (got[1].numpy()[unlisted] == -7.25).all() and (got[2].numpy()[unlisted] == 77).all()
        if t0 == T or t0s[2] == T:                           # t0 = T: nothing of that slot is written
            s = slot[0] if t0 == T else slot[2]
            assert got[2][s] == 3 and (got[1].numpy()[s] == 0).all()


def test_pool_rows_host_edge_cases():
    rng = np.random.default_rng(0)
    x = torch.from_numpy(special_rows(rng, 2, 7, C))
    # n_seq = 0: nothing happens
    tabs = [torch.from_numpy(t) for t in sentinel_tables(3, C)]
    ops.pool_rows(x, i32(), i32(), i32(), *tabs)
    assert (tabs[0] == 1234.5).all() and (tabs[2] == 77).all()
    # a sequence or slot out of range is skipped
    ops.pool_rows(x, i32(2, -1, 0), i32(0, 0, 0), i32(0, 1, 3), *tabs)
    assert (tabs[0] == 1234.5).all() and (tabs[2] == 77).all()
    # 7 tokens in one call, and as 3 + 4: identical bits
    one = [torch.zeros(2, C), torch.zeros(2, C, dtype=torch.float16), torch.zeros(2, dtype=torch.int32)]
    two = [t.clone() for t in one]
    ops.pool_rows(x, i32(1), i32(0), i32(1), *one)
    ops.pool_rows(x[:, :3].contiguous(), i32(1), i32(0), i32(1), *two)
    ops.pool_rows(x[:, 3:].contiguous(), i32(1), i32(0), i32(1), *two)
    for a, b in zip(one, two):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16) if a.dtype == torch.float16 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16) if b.dtype == torch.float16 else b)
    assert int(one[2][1]) == 7
    # wrong dtypes and shapes are refused
    with pytest.raises(RuntimeError):
        ops.pool_rows(x.float(), i32(0), i32(0), i32(0), *one)
    with pytest.raises(RuntimeError):
        ops.pool_rows(x, i32(0), i32(0, 1), i32(0), *one)
    with pytest.raises(RuntimeError):
        ops.pool_rows(x, i32(0), i32(0), i32(0), one[0][:, :4].contiguous(), one[1], one[2])


# ---------------------------------------------------------------------------------------------- finish()
def test_finish_mean_last_normalised_zero_and_one_rounding():
    rng = np.random.default_rng(1)
    s = (rng.standard_normal(16) * 100).astype(np.float32)
    last = rng.standard_normal(16).astype(np.float16)
    m = finish(s, last, 7, "mean", False)
    assert m.dtype == np.float32 and np.array_equal(m, (s.astype(np.float64) / 7.0).astype(np.float32))
    la = finish(s, last, 7, "last", False)
    assert la.dtype == np.float32 and np.array_equal(la, last.astype(np.float32))
    for pooling, raw in (("mean", s.astype(np.float64) / 7.0), ("last", last.astype(np.float64))):
        e = finish(s, last, 7, pooling, True)
        assert np.array_equal(e, (raw / np.sqrt((raw * raw).sum())).astype(np.float32))
        assert abs(float(np.linalg.norm(e.astype(np.float64))) - 1.0) <= 1e-6
    z = finish(np.zeros(4, np.float32), np.zeros(4, np.float16), 3, "mean", True)
    assert z.dtype == np.float32 and not z.any() and np.isfinite(z).all()
    assert not finish(np.ones(4, np.float32), np.zeros(4, np.float16), 3, "last", True).any()
    # binary64 arithmetic with ONE rounding: binary32 division followed by binary32 normalisation differs on this input
    s3 = np.array([1.0, 2.0, 4.0], np.float32)
    want = s3.astype(np.float64) / 3.0
    want = (want / np.sqrt((want * want).sum())).astype(np.float32)
    assert np.array_equal(finish(s3, np.zeros(3, np.float16), 3), want)
    big = np.array([3e38, 3e38], np.float32)                 # the squared norm overflows binary32, not binary64
    assert np.allclose(finish(big, np.zeros(2, np.float16), 1), np.float32(np.sqrt(0.5)))
    with pytest.raises(ValueError):
        finish(s, last, 7, "max")
    with pytest.raises(ValueError):
        finish(s, last, 0)


# ---------------------------------------------------------------------------------------------- worker over a fake backend
def hidden_row(h):
    """The fake model's "ln_out row" after a token: a deterministic binary16 function of the slot's token history."""
    return np.array([((h * (c + 3) + c) % 251 - 125) / 16.0 for c in range(C)], np.float16)


class EmbModel(FakeModel):
    """FakeModel with hidden rows of C channels and the pool_rows exit; records the keywords of every call."""

    def __init__(self):
        self.calls = []

    def generate_zero_state(self, n):
        return [torch.zeros((1, 2, n, C), dtype=torch.float16), torch.zeros((1, n, 1, 1, 1), dtype=torch.float32),
                torch.zeros((n,), dtype=torch.int32)]

    def forward_slots(self, tokens, pool, slot_idx, full_output=False, pool_rows=None):
        slots = slot_idx.tolist()
        self.calls.append({"slots": slots, "T": len(tokens[0]), "pool_rows": pool_rows is not None})
        if pool_rows is not None:
            xo = np.zeros((len(tokens), len(tokens[0]), C), np.float16)
            for b, (toks, s) in enumerate(zip(tokens, slots)):
                h = int(pool[1][0, s, 0, 0, 0])
                for t, tok in enumerate(toks):
                    h = self.advance(h, int(tok))
                    xo[b, t] = hidden_row(h)
            ops.pool_rows(torch.from_numpy(xo), *pool_rows)
        return super().forward_slots(tokens, pool, slot_idx)


def expected_embedding(prompt, skip=0, pooling="mean", normalize=True):
    h, rows = 0, []
    for t in prompt:
        h = FakeModel.advance(h, t)
        rows.append(hidden_row(h))
    acc = np.zeros(C, np.float32)
    for r in rows[skip:]:
        acc = acc + r.astype(np.float32)
    return finish(acc, rows[-1], len(rows) - skip, pooling, normalize)


def make_worker(batch_size=6, run_ahead=True, model=None):
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    tq, mq, wq = queue.Queue(), queue.Queue(), queue.Queue()
    w = Worker("w0", [], cfg, tq, mq, wq, batch_size=batch_size, model=model if model is not None else EmbModel(), tokenizer=FakeTok(),
               penalize_argmax=cpu_penalize_argmax, run_ahead=run_ahead)
    w._init_worker()
    w.max_forward_seq_len_per_forward = 8
    return w, tq


def run_until_idle(w, max_iter=3000):
    for _ in range(max_iter):
        if not w.step():
            return
    raise AssertionError("the worker did not go idle")


def prompt_of(n, seed):
    return np.random.default_rng(seed).integers(1, V, n).tolist()


def messages(task, kind):
    return [p for k, p in task.output_queue.items if k == kind]


def check_embedding(task, prompt, skip, pooling="mean", normalize=True):
    kinds = [k for k, _ in task.output_queue.items]
    assert kinds == ["embedding", "task_completed"], kinds
    payload = messages(task, "embedding")[0]
    want = expected_embedding(prompt, skip, pooling, normalize)
    assert payload["embedding"].dtype == np.float32 and payload["embedding"].shape == (C,)
    assert np.array_equal(payload["embedding"].view(np.uint32), want.view(np.uint32)), (len(prompt), payload["embedding"], want)
    assert payload["pooled_tokens"] == len(prompt) - skip and payload["prompt_tokens"] == len(prompt)
    assert task.request_status == RequestStatus.FINISHED_LENGTH_CAPPED and task.generated_tokens == []


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_worker_embeddings_alone(run_ahead):
    w, tq = make_worker(batch_size=9, run_ahead=run_ahead)
    tasks = []
    for i, n in enumerate(LENGTHS):
        prompt = prompt_of(n, i)
        for pooling, normalize in (("mean", True), ("last", False)):
            t = new_task([0] + prompt, embed=pooling, embed_skip=1, embed_normalize=normalize)
            tasks.append((t, [0] + prompt, 1, pooling, normalize))
            tq.put(t)
    tasks.append((new_task(prompt_of(5, 99), embed="mean"), prompt_of(5, 99), 0, "mean", True))     # no padding token
    tq.put(tasks[-1][0])
    run_until_idle(w)
    for t, prompt, skip, pooling, normalize in tasks:
        check_embedding(t, prompt, skip, pooling, normalize)
    calls = w.model.calls
    assert all(c["pool_rows"] for c in calls) and max(c["T"] for c in calls) <= 8      # chunks only, never a single-token row path
    assert all(td["state_category"] == StateCategory.EMPTY for td in w.state_slot.values())


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_worker_embeddings_beside_generating_requests(run_ahead):
    gen_prompts = [prompt_of(n, 50 + n) for n in (4, 13, 30)]

    def streams(with_embeddings):
        w, tq = make_worker(batch_size=8, run_ahead=run_ahead)
        gens = [new_task(p, max_tokens=12) for p in gen_prompts]
        embs = [(new_task([0] + prompt_of(n, i), embed="mean", embed_skip=1), [0] + prompt_of(n, i)) for i, n in enumerate(LENGTHS)]
        order = [gens[0]] + [e for e, _ in embs[:3]] + [gens[1]] + [e for e, _ in embs[3:]] + [gens[2]] if with_embeddings else gens
        for t in order:
            tq.put(t)
        run_until_idle(w)
        if with_embeddings:
            for t, prompt in embs:
                check_embedding(t, prompt, 1)
        # an embedding never rides in a single-token forward (no graph, no sampler kernel sees it)
        return [[p[0] for p in messages(g, "token_generated")] for g in gens], w.model.calls

    alone, calls0 = streams(False)
    mixed, calls1 = streams(True)
    want = [expected_stream(p, 12) for p in gen_prompts]
    assert alone == want and mixed == want
    assert not any(c["pool_rows"] for c in calls0) and any(c["pool_rows"] for c in calls1)
    # the chunk rule: a forward that carries an ordinary sequence is never shorter than it would be without the embeddings
    assert all(c["T"] >= 8 or c["pool_rows"] for c in calls1 if c["T"] > 1)


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_short_embedding_remainder_does_not_shorten_a_neighbours_chunk(run_ahead):
    """A 30-token prompt prefills in chunks of 8 while a 3-token embedding sits in the next slot: the long prompt's chunks stay 8 long
    (the embedding runs in a forward of its own)."""
    w, tq = make_worker(batch_size=17, run_ahead=run_ahead)          # two prefill slots
    g = new_task(prompt_of(30, 1), max_tokens=3)
    e = new_task(prompt_of(3, 2), embed="mean")
    tq.put(g)
    tq.put(e)
    run_until_idle(w)
    check_embedding(e, prompt_of(3, 2), 0)
    assert [p[0] for p in messages(g, "token_generated")] == expected_stream(prompt_of(30, 1), 3)
    long_chunks = [c["T"] for c in w.model.calls if c["T"] > 1 and not c["pool_rows"]]
    assert long_chunks[:2] == [8, 8]
    assert [c["T"] for c in w.model.calls if c["pool_rows"]] == [3]


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_two_embeddings_through_one_slot_do_not_leak(run_ahead):
    w, tq = make_worker(batch_size=2, run_ahead=run_ahead)           # one usable slot
    a, b = prompt_of(17, 1), prompt_of(9, 2)
    ta, tb, tc = new_task(a, embed="mean"), new_task(b, embed="last", embed_normalize=False), new_task(a, embed="mean")
    for t in (ta, tb, tc):
        tq.put(t)
    run_until_idle(w)
    check_embedding(ta, a, 0)
    check_embedding(tb, b, 0, "last", False)
    check_embedding(tc, a, 0)
    assert np.array_equal(messages(ta, "embedding")[0]["embedding"], messages(tc, "embedding")[0]["embedding"])


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_abort_during_prefill_frees_the_slot(run_ahead):
    w, tq = make_worker(batch_size=2, run_ahead=run_ahead)
    t = new_task(prompt_of(40, 3), embed="mean")
    tq.put(t)
    assert w.step() and w.state_slot[0]["task"] is t and w.state_slot[0]["state_category"] == StateCategory.FORWARD_SEQ
    t.task_event_queue.put(("abort", None))
    nxt = new_task(prompt_of(9, 4), embed="mean")
    tq.put(nxt)
    run_until_idle(w)
    assert t.request_status == RequestStatus.FINISHED_ABORTED and [k for k, _ in t.output_queue.items] == ["task_completed"]
    check_embedding(nxt, prompt_of(9, 4), 0)                         # the freed slot, zeroed accumulators
    # ... and an abort that arrives after the last chunk, before the vector was finished
    w, tq = make_worker(batch_size=2, run_ahead=True)
    t = new_task(prompt_of(5, 5), embed="mean")
    tq.put(t)
    assert w.step()
    t.task_event_queue.put(("abort", None))
    run_until_idle(w)
    assert t.request_status == RequestStatus.FINISHED_ABORTED and not messages(t, "embedding")
    assert w.state_slot[0]["state_category"] == StateCategory.EMPTY


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_without_embeddings_the_backend_never_sees_the_keyword(run_ahead):
    """test_worker_cpu.FakeModel.forward_slots takes no pool_rows: any call with it would raise."""
    w, tq = make_worker(batch_size=6, run_ahead=run_ahead, model=FakeModel())
    prompts = [prompt_of(n, n) for n in (3, 12, 40)]
    tasks = [new_task(p, max_tokens=6) for p in prompts]
    for t in tasks:
        tq.put(t)
    run_until_idle(w)
    assert [[p[0] for p in messages(t, "token_generated")] for t in tasks] == [expected_stream(p, 6) for p in prompts]
    assert w._emb is None


# ---------------------------------------------------------------------------------------------- engine and route
class _Tok(FakeTok):
    idx2token = {i: f"t{i}".encode() for i in range(V)}

    def encode(self, s):
        return [ord(c) % (V - 1) + 1 for c in s]


def _factory(**kw):
    w = Worker(model=EmbModel(), tokenizer=_Tok(), penalize_argmax=cpu_penalize_argmax, **kw)
    w.max_forward_seq_len_per_forward = 8
    return w


async def _engine(worker_num=2, **kw):
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=_Tok(), **kw)
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    await asyncio.wait_for(eng.init(worker_num=worker_num, model_config=cfg, batch_size=4), 120)
    return eng


def test_engine_embed():
    async def main():
        eng = await _engine()
        ids = _Tok().encode("embed me, please")
        got = await eng.embed("embed me, please")
        assert np.array_equal(got["embedding"], expected_embedding([0] + ids, 1)) and got["prompt_tokens"] == len(ids) + 1
        assert got["pooled_tokens"] == len(ids)
        got = await eng.embed(prefill_tokens=ids, pooling="last", normalize=False, pad_zero=False)
        assert np.array_equal(got["embedding"], expected_embedding(ids, 0, "last", False)) and got["prompt_tokens"] == len(ids)
        many = await asyncio.gather(*[eng.embed(prefill_tokens=prompt_of(n, n)) for n in (1, 2, 3, 9, 17, 40, 5, 6, 7)])
        for n, r in zip((1, 2, 3, 9, 17, 40, 5, 6, 7), many):
            assert np.array_equal(r["embedding"], expected_embedding([0] + prompt_of(n, n), 1))
        # an ordinary completion beside it is what it is without
        c = eng.completion("", prefill_tokens=[3, 1, 4], max_tokens=5, temperature=0.0, frequency_penalty=0.0, presence_penalty=0.0,
                           penalty_decay=1.0, stop_tokens=[])
        e, text = await asyncio.gather(eng.embed(prefill_tokens=[3, 1, 4]), c.get_full_completion())
        assert text == "".join(f"<{t}>" for t in expected_stream([3, 1, 4], 5))
        for bad in (dict(prefill_tokens=[]), dict(prompt_str=""), dict(prefill_tokens=[1], pooling="max"), dict(prefill_tokens=[V])):
            with pytest.raises(ValueError):
                eng.embed(**bad)
        eng.shutdown()
        with pytest.raises(RuntimeError):
            eng.embed("x")

    asyncio.run(main())


def _process_factory(**kw):
    return _factory(**kw)


def test_engine_embed_in_process_mode():
    """The new Task fields and the ("embedding", ...) message cross the process boundary; the vector arrives as a numpy array."""
    async def main():
        eng = AsyncEngineCore(worker_factory=_process_factory, tokenizer=_Tok(), worker_mode="process")
        cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
        await asyncio.wait_for(eng.init(worker_num=1, model_config=cfg, batch_size=4), 120)
        ids = prompt_of(17, 3)
        got = await asyncio.wait_for(eng.embed(prefill_tokens=ids, pooling="mean", normalize=False), 60)
        assert isinstance(got["embedding"], np.ndarray) and got["embedding"].dtype == np.float32
        assert np.array_equal(got["embedding"], expected_embedding([0] + ids, 1, "mean", False))
        got = await asyncio.wait_for(eng.embed(prefill_tokens=ids, pooling="last", pad_zero=False), 60)
        assert np.array_equal(got["embedding"], expected_embedding(ids, 0, "last", True)) and got["pooled_tokens"] == 17
        eng.shutdown()

    asyncio.run(main())
    assert not torch.cuda.is_initialized()


def test_embeddings_route():
    import httpx

    from chirrup_amd.web_service import EmbeddingRequest, create_app

    assert EmbeddingRequest(input="a").inputs() == ["a"] and EmbeddingRequest(input=[1, 2]).inputs() == [[1, 2]]
    assert EmbeddingRequest(input=["a", "b"]).inputs() == ["a", "b"] and EmbeddingRequest(input=[[1], [2, 3]]).inputs() == [[1], [2, 3]]

    async def main():
        eng = await _engine()
        app = create_app(eng, state_cache_size=4)
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
            models_before = (await cl.get("/v1/models")).json()["data"]
            enc = _Tok().encode

            def want(ids, **kw):
                return [float(v) for v in expected_embedding([0] + ids, 1, **kw)]

            # a string
            r = await cl.post("/v1/embeddings", json={"input": "hello world", "model": "rwkv-latest:thinking"})
            assert r.status_code == 200, r.text
            j = r.json()
            assert j["object"] == "list" and j["model"] == "rwkv-latest:thinking" and len(j["data"]) == 1
            assert j["data"][0]["object"] == "embedding" and j["data"][0]["index"] == 0
            assert j["data"][0]["embedding"] == want(enc("hello world"))
            n = len(enc("hello world")) + 1
            assert j["usage"] == {"prompt_tokens": n, "total_tokens": n}
            # a list of strings: index order, usage sums
            texts = ["first", "the second one is longer than a chunk", "3"]
            j = (await cl.post("/v1/embeddings", json={"input": texts})).json()
            assert [d["index"] for d in j["data"]] == [0, 1, 2]
            assert [d["embedding"] for d in j["data"]] == [want(enc(t)) for t in texts]
            n = sum(len(enc(t)) + 1 for t in texts)
            assert j["usage"] == {"prompt_tokens": n, "total_tokens": n}
            # one tokenised input, and a list of them
            j = (await cl.post("/v1/embeddings", json={"input": [5, 6, 7]})).json()
            assert len(j["data"]) == 1 and j["data"][0]["embedding"] == want([5, 6, 7])
            lists = [[5, 6, 7], [9], prompt_of(20, 1)]
            j = (await cl.post("/v1/embeddings", json={"input": lists})).json()
            assert [d["embedding"] for d in j["data"]] == [want(x) for x in lists]
            # base64 decodes to the float answer
            jb = (await cl.post("/v1/embeddings", json={"input": lists, "encoding_format": "base64"})).json()
            for d, f in zip(jb["data"], j["data"]):
                vec = np.frombuffer(base64.b64decode(d["embedding"]), dtype="<f4")
                assert vec.shape == (C,) and [float(v) for v in vec] == f["embedding"]
            # the extension fields
            j = (await cl.post("/v1/embeddings", json={"input": [5, 6, 7], "pooling": "last", "normalize": False, "pad_zero": False})).json()
            assert j["data"][0]["embedding"] == [float(v) for v in expected_embedding([5, 6, 7], 0, "last", False)]
            assert j["usage"] == {"prompt_tokens": 3, "total_tokens": 3}
            # 400 with a reason
            for body in ({"input": []}, {"input": ""}, {"input": ["a", ""]}, {"input": [[1], []]}, {"input": [[1]] * 2049},
                         {"input": [1, V]}, {"input": [[1], [2, -1]]}, {"input": "x", "dimensions": 4}, {"input": "x", "pooling": "max"}):
                r = await cl.post("/v1/embeddings", json=body)
                assert r.status_code == 400 and r.json()["detail"], (body if len(str(body)) < 99 else "2049 inputs", r.status_code)
            # 422 for malformed bodies
            for body in ({}, {"input": 5}, {"input": "x", "encoding_format": "hex"}, {"input": {"a": 1}}, {"input": [[1.5]]}):
                assert (await cl.post("/v1/embeddings", json=body)).status_code == 422, body
            assert (await cl.get("/v1/models")).json()["data"] == models_before
            # the prefix-state cache is bypassed in both directions
            assert len(app.state.state_cache) == 0
            eng.shutdown()
            assert (await cl.post("/v1/embeddings", json={"input": "x"})).status_code == 503

    asyncio.run(main())


# ---------------------------------------------------------------------------------------------- C ABI
def test_cabi_exports_pool_rows_with_the_documented_prototype():
    import chirrup_amd
    from chirrup_amd import lib

    header = open(os.path.join(ROOT, "include", "chirrup_amd.h")).read()
    proto = re.search(r"int rwkv7_pool_rows\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    assert " ".join(proto.split()) == ("int n_seq, int B, int T, int C, const void *xo, const int32_t *seq, const int32_t *t0, "
                                       "const int32_t *slot, int n_slots, float *acc_sum, void *acc_last, int32_t *acc_count, void *stream")
    assert int(re.search(r"#define\s+CHIRRUP_ABI_VERSION\s+(\d+)", header).group(1)) == lib.ABI_VERSION == 4
    L = chirrup_amd.load()
    assert L.chirrup_abi_version() == 4 and hasattr(L, "rwkv7_pool_rows")
    res, args = lib.SIGNATURES["rwkv7_pool_rows"]
    assert res is ctypes.c_int and len(args) == 13
    # bad arguments are refused on the host, before any launch
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    f = L.rwkv7_pool_rows
    assert f(0, 1, 1, 64, None, None, None, None, 1, None, None, None, None) == 0       # n_seq = 0: nothing to do
    assert f(1, 1, 1, 60, p, p, p, p, 1, p, p, p, None) == -1                            # C % 8
    assert f(-1, 1, 1, 64, p, p, p, p, 1, p, p, p, None) == -1
    assert f(1, 1, 0, 64, p, p, p, p, 1, p, p, p, None) == -1
    for k in (4, 5, 6, 7, 9, 10, 11):                                                    # every pointer is required
        a = [1, 1, 1, 64, p, p, p, p, 1, p, p, p, None]
        a[k] = None
        assert f(*a) == -2, k
    for k in (4, 9, 10):                                                                 # xo, acc_sum, acc_last: 16-byte aligned
        a = [1, 1, 1, 64, p, p, p, p, 1, p, p, p, None]
        a[k] = odd
        assert f(*a) == -3, k
