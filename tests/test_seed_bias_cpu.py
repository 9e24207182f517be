"""Per-request seed and logit_bias without a GPU: the Philox4x32-10 host form (known-answer vectors), the uniform mapping, the CPU
forms of ops.seeded_uniform / ops.apply_logit_bias, Task validation, the fake-backend worker (seeded draws that do not depend on
the slot or the neighbours, counters that restart with a slot's next request, unseeded draws left alone), the chat route and the
C ABI's declarations and argument checks."""
import asyncio
import ctypes
import os
import queue
import re

import httpx
import numpy as np
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import LOGIT_BIAS_MAX, ModelLoadConfig, Task
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.samplers import sample_inverse_cdf
from chirrup_amd.web_service import ChatCompletionRequest, ChatMessage, chat_prompt, create_app
from chirrup_amd.worker import Worker
from test_engine_cpu import _factory, _Tok
from test_worker_cpu import V, FakeModel, FakeTok, Sink, cpu_penalize_argmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------- Philox and the uniform
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = ops.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
    assert tuple(int(x) for x in got) == want
    batch = ops.philox4x32_10(np.array([c for c, _, _ in KAT], np.uint64), np.array([k for _, k, _ in KAT], np.uint64))
    assert [tuple(int(x) for x in r) for r in batch] == [w for _, _, w in KAT]


def test_uniform_mapping_and_seed_reinterpretation():
    seed = 0x0123456789ABCDEF
    i = np.arange(1000, dtype=np.uint64)
    ctr = np.stack([i, 0 * i, 0 * i, 0 * i], -1)
    x0 = ops.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))[:, 0]
    u = ops.philox_uniform(seed, i)
    assert u.dtype == np.float32
    assert np.array_equal(u.astype(np.float64), (x0 >> 8).astype(np.float64) / 2 ** 24)     # exact in binary32
    assert u.min() >= 0 and u.max() <= 1 - 2 ** -24 and len(set(u.tolist())) > 990
    # the key is (lo32, hi32) of the uint64: counter 0 of key (0, 0) is the first known answer
    assert float(ops.philox_uniform(0, 0)) == (0x6627E8D5 >> 8) / 2 ** 24
    # an int64 seed is its two's complement uint64
    for neg in (-1, -2, -(1 << 63), -123456789):
        assert np.array_equal(ops.philox_uniform(neg, i[:16]), ops.philox_uniform(neg + (1 << 64), i[:16]))
        assert ops.seed_bits(neg) == neg + (1 << 64) and ops.seed_int64(neg + (1 << 64)) == neg
    assert ops.seed_int64(5) == 5 and ops.seed_bits((1 << 64) - 1) == (1 << 64) - 1
    for bad in (1 << 64, -(1 << 63) - 1):
        with pytest.raises(ValueError):
            ops.seed_bits(bad)
    assert not np.array_equal(ops.philox_uniform(1, i[:8]), ops.philox_uniform(2, i[:8]))


def test_seeded_uniform_host_form():
    """Row indirection, counter advance, unseeded rows untouched."""
    S = 6
    seeds = torch.tensor([0, 11, -5, 0, 1 << 40, 7], dtype=torch.int64)
    seeded = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32)
    counters = torch.tensor([0, 0, 3, 9, -1, 0], dtype=torch.int32)             # -1: uint32 0xffffffff, wraps to 0
    slot_idx = torch.tensor([4, 3, 1, 2, 0], dtype=torch.int32)                   # batch row -> slot
    rows = torch.tensor([2, 1, 3, 0], dtype=torch.int32)                          # the sampled batch rows
    u = torch.tensor([0.5, 0.25, 0.125, 0.75], dtype=torch.float32)
    ops.seeded_uniform(rows, slot_idx, seeds, seeded, counters, u)
    assert u[0].item() == float(ops.philox_uniform(11, 0))                        # row 2 -> slot 1
    assert u[1].item() == 0.25                                                    # row 1 -> slot 3: not seeded
    assert u[2].item() == float(ops.philox_uniform(-5, 3))                        # row 3 -> slot 2
    assert u[3].item() == float(ops.philox_uniform(1 << 40, 0xFFFFFFFF))          # row 0 -> slot 4
    assert counters.tolist() == [0, 1, 4, 9, 0, 0]
    ops.seeded_uniform(rows[:1], slot_idx, seeds, seeded, counters, u[:1])
    assert u[0].item() == float(ops.philox_uniform(11, 1)) and counters[1].item() == 2
    empty = torch.zeros((0,), dtype=torch.float32)
    ops.seeded_uniform(rows[:0], slot_idx, seeds, seeded, counters, empty)
    assert counters.tolist() == [0, 2, 4, 9, 0, 0]


def test_apply_logit_bias_host_form():
    lg = torch.tensor([[1.0, -2.0, 0.5, 3.0, 65504.0, -65504.0, float("-inf"), 0.1],
                       [0.0] * 8, [2.0] * 8], dtype=torch.float16)
    cap = 5
    ids = torch.zeros((3, cap), dtype=torch.int32)
    vals = torch.zeros((3, cap), dtype=torch.float32)
    ids[0] = torch.tensor([0, 1, 7, 9, -1])
    vals[0] = torch.tensor([100.0, -100.0, 1e-3, 5.0, 5.0])
    ids[2] = torch.tensor([4, 5, 6, 2, 3])
    vals[2] = torch.tensor([100.0, -100.0, -100.0, 0.3, 1.0])
    counts = torch.tensor([4, 0, 5], dtype=torch.int32)                           # slot 0: the 5th entry is past its count
    raw = lg.clone()
    b = lg[[0, 2]].contiguous()                                                   # batch row 0 -> slot 2, row 1 -> slot 0
    ops.apply_logit_bias(b, torch.tensor([2, 0], dtype=torch.int32), counts, ids, vals)
    f = lambda l, v: float(np.float16(np.clip(np.float32(l) + np.float32(v), -65504, 65504)))
    want1 = raw[2].clone()                                                        # slot 0's list; id 9 >= V is skipped
    want1[0], want1[1], want1[7] = f(2.0, 100.0), f(2.0, -100.0), f(2.0, 1e-3)
    assert torch.equal(b[1], want1) and b[1, 7].item() != 2.0
    row = b[0].tolist()                                                           # slot 2's list on the edge row
    assert row[4] == 65504.0 and row[5] == -65504.0 and row[6] == float("-inf")   # clamp, finite stays finite, -inf stays
    assert row[2] == f(0.5, 0.3) and row[3] == f(3.0, 1.0) and row[0] == 1.0 and row[7] == float(raw[0, 7])
    lg2 = lg.clone()
    ops.apply_logit_bias(lg2[1:2].contiguous(), torch.tensor([1], dtype=torch.int32), counts, ids, vals)   # empty list
    e = raw[4:4]
    ops.apply_logit_bias(torch.zeros((0, 8), dtype=torch.float16), None, counts, ids, vals)
    assert torch.equal(lg2, raw) and e.numel() == 0
    # the edges of the clamp: finite + 100 never becomes +inf, -inf + 100 stays -inf
    edge = torch.tensor([[65504.0, -65504.0, float("-inf"), 65472.0]], dtype=torch.float16)
    ops.apply_logit_bias(edge, None, torch.tensor([4], dtype=torch.int32), torch.tensor([[0, 1, 2, 3]], dtype=torch.int32),
                         torch.tensor([[100.0, -100.0, 100.0, 1000.0]]))
    assert edge.tolist() == [[65504.0, -65504.0, float("-inf"), 65504.0]]


def test_inverse_cdf_draw_rule():
    lg = torch.tensor([[0.0, float("-inf"), 0.0, 0.0]], dtype=torch.float16)
    T, P, K = torch.ones((1, 1)), torch.ones((1, 1)), torch.zeros((1, 1), dtype=torch.int32)
    for u, want in ((0.0, 0), (0.3, 0), (1 / 3 + 1e-6, 2), (0.5, 2), (0.7, 3), (1 - 2 ** -24, 3)):
        assert int(sample_inverse_cdf(lg, T, P, K, torch.tensor([u]))[0]) == want, u


# --------------------------------------------------------------------------------------------------- Task
def _task(**kw):
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=[1, 2], state=None, **kw)


def test_task_validates_seed_and_logit_bias():
    assert _task().seed is None and _task().logit_bias == {}
    assert _task(seed=-(1 << 63)).seed == -(1 << 63) and _task(seed=(1 << 64) - 1).seed == (1 << 64) - 1
    assert _task(logit_bias={np.int64(3): 1, 5: -2.5}).logit_bias == {3: 1.0, 5: -2.5}
    assert len(_task(logit_bias={i: 0.0 for i in range(LOGIT_BIAS_MAX)}).logit_bias) == LOGIT_BIAS_MAX == 1024
    for bad in (dict(seed=1 << 64), dict(seed=-(1 << 63) - 1), dict(seed=1.5), dict(seed="7"), dict(seed=True),
                dict(logit_bias={-1: 1.0}), dict(logit_bias={1: float("inf")}), dict(logit_bias={1: float("nan")}),
                dict(logit_bias={"1": 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={1: "x"}),
                dict(logit_bias={i: 0.0 for i in range(LOGIT_BIAS_MAX + 1)})):
        with pytest.raises(ValueError):
            _task(**bad)


# --------------------------------------------------------------------------------------------------- the fake-backend worker
def _worker(run_ahead, batch_size=6):
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [], cfg, tq, queue.Queue(), queue.Queue(), batch_size=batch_size, model=FakeModel(), tokenizer=FakeTok(),
               penalize_argmax=cpu_penalize_argmax, run_ahead=run_ahead)
    w._init_worker()
    return w, tq


def _new(prompt, **kw):
    kw.setdefault("temperature", 1.0)
    kw.setdefault("top_p", 1.0)
    for k, v in (("frequency_penalty", 0.0), ("presence_penalty", 0.0), ("penalty_decay", 1.0), ("stop_tokens", []), ("max_tokens", 12)):
        kw.setdefault(k, v)
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **kw)


def _drain(w):
    for _ in range(2000):
        if not w.step():
            return
    raise AssertionError("worker did not drain")


def _seeded_stream(prompt, n, seed, T=1.0, bias=None):
    """An independent host computation of a seeded, unpenalised, top_p = 1 request over FakeModel: the model's two-peak logits,
    the bias, softmax ** (1/T) in float64, the inverse-CDF walk in token order with the request's Philox uniforms."""
    h = 0
    for t in prompt:
        h = FakeModel.advance(h, t)
    out = []
    for i in range(n):
        lg = np.zeros(V, np.float16)
        lg[h % V], lg[(h + 1) % V] = 5.0, 4.0
        for t, b in (bias or {}).items():
            lg[t] = np.float16(np.clip(np.float32(lg[t]) + np.float32(b), -65504, 65504))
        x = lg.astype(np.float64)
        w = np.exp(x - x.max())
        w = (w / w.sum()) ** (1.0 / float(np.float16(T)))
        cum = np.cumsum(w)
        tok = int(np.searchsorted(cum, float(ops.philox_uniform(seed, i)) * cum[-1], side="right"))
        out.append(tok)
        h = FakeModel.advance(h, tok)
    return out


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_seeded_request_ids_do_not_depend_on_slot_or_neighbours(run_ahead):
    prompt, seed = [5, 9, 2], 424242
    want = _seeded_stream(prompt, 12, seed, T=1.3)
    assert len(set(want)) > 4                                         # the draws really spread over the vocabulary
    w, tq = _worker(run_ahead)
    alone = _new(prompt, seed=seed, temperature=1.3)
    tq.put(alone)
    _drain(w)
    assert alone.generated_tokens == want
    torch.manual_seed(99)
    w, tq = _worker(run_ahead)
    others = [_new([3 + k, 1], temperature=0.8 + 0.1 * k, max_tokens=9 + k) for k in range(3)]
    busy = _new(prompt, seed=seed, temperature=1.3)
    for t in others + [busy]:                                         # the seeded request lands in slot 3 behind three others
        tq.put(t)
    _drain(w)
    assert busy.generated_tokens == want
    assert _new(prompt, seed=seed).seed == seed


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_counters_restart_when_a_slot_is_reused(run_ahead):
    w, tq = _worker(run_ahead, batch_size=2)                          # one decode slot: every request reuses slot 0
    seed = -77
    first, plain, second = _new([4, 4], seed=seed, max_tokens=10), _new([8], max_tokens=6), _new([4, 4], seed=seed, max_tokens=10)
    other = _new([4, 4], seed=seed + 1, max_tokens=10)
    for t in (first, plain, second, other):
        tq.put(t)
    _drain(w)
    assert first.generated_tokens == second.generated_tokens == _seeded_stream([4, 4], 10, seed)
    assert other.generated_tokens == _seeded_stream([4, 4], 10, seed + 1) != first.generated_tokens
    assert w._seeded == [True, False] and int(w.counters[0]) >= 10


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_a_seed_leaves_the_other_requests_draws_unchanged(run_ahead):
    def run(seed_of_1):
        torch.manual_seed(1234)
        w, tq = _worker(run_ahead)
        ts = [_new([2 + k, 7], temperature=1.0 + 0.2 * k, max_tokens=10, seed=(seed_of_1 if k == 1 else None)) for k in range(4)]
        for t in ts:
            tq.put(t)
        _drain(w)
        return [t.generated_tokens for t in ts]

    base, with_seed = run(None), run(31337)
    assert with_seed[1] == _seeded_stream([3, 7], 10, 31337, T=1.2)
    assert [with_seed[k] for k in (0, 2, 3)] == [base[k] for k in (0, 2, 3)]


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_logit_bias_moves_greedy_and_sampled_rows(run_ahead):
    from test_worker_cpu import expected_stream

    w, tq = _worker(run_ahead)
    g = dict(temperature=0.0, top_p=0.0)
    plain = _new([5, 9], max_tokens=8, **g)
    up = _new([5, 9], max_tokens=8, logit_bias={17: 100.0}, **g)
    down_tok = expected_stream([5, 9], 1)[0]
    down = _new([5, 9], max_tokens=8, logit_bias={down_tok: -100.0, 63: 0.5}, **g)
    sampled = _new([5, 9], max_tokens=8, seed=5, logit_bias={30: 8.0, 31: -3.0})
    for t in (plain, up, down, sampled):
        tq.put(t)
    _drain(w)
    assert plain.generated_tokens == expected_stream([5, 9], 8)
    assert up.generated_tokens == [17] * 8
    assert down_tok not in down.generated_tokens
    assert sampled.generated_tokens == _seeded_stream([5, 9], 8, 5, bias={30: 8.0, 31: -3.0})
    assert w._bias_n[:4] == [0, 1, 2, 2]


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_steps_without_seed_or_bias_never_call_the_kernels(run_ahead, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("seed / bias kernel called in a step where no row asked")

    monkeypatch.setattr(ops, "seeded_uniform", boom)
    monkeypatch.setattr(ops, "apply_logit_bias", boom)
    w, tq = _worker(run_ahead)
    ts = [_new([1, 2, 3]), _new([4], temperature=0.0, top_p=0.0), _new([6], seed=3, temperature=0.0, top_p=0.0)]   # greedy: no draw
    for t in ts:
        tq.put(t)
    _drain(w)
    assert all(len(t.generated_tokens) == 12 for t in ts)
    assert int(w.counters[2]) == 0
    tq.put(_new([1, 2, 3], logit_bias={3: 1.0}))
    with pytest.raises(AssertionError, match="no row asked"):
        _drain(w)


# --------------------------------------------------------------------------------------------------- engine and chat route
class _VocabTok(_Tok):
    idx2token = {i: f"t{i}".encode() for i in range(V)}


async def _app_client(record):
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=_VocabTok())
    await eng.init(worker_num=1, model_config=ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64),
                   batch_size=4)
    real = eng.completion

    def completion(*a, **kw):
        c = real(*a, **kw)
        record.append(c.task)
        return c

    eng.completion = completion
    return eng, httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(eng, state_cache_size=0)), base_url="http://t")


def test_engine_completion_rejects_ids_outside_the_vocabulary():
    async def main():
        eng = AsyncEngineCore(worker_factory=_factory, tokenizer=_Tok())
        await eng.init(worker_num=1, model_config=ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64),
                       batch_size=4)
        with pytest.raises(ValueError):
            eng.completion("x", prefill_tokens=[1, 2], logit_bias={V: 1.0})
        c = eng.completion("x", prefill_tokens=[1, 2], logit_bias={V - 1: 100.0}, seed=-9, temperature=0.0, top_p=0.0, max_tokens=4,
                           presence_penalty=0.0, frequency_penalty=0.0)
        assert c.task.seed == -9 and c.task.logit_bias == {V - 1: 100.0}
        assert [ev[1] async for ev in c if ev[0] == "token"] == [V - 1] * 4
        eng.shutdown()

    asyncio.run(main())


def test_process_mode_carries_both_fields():
    from chirrup_amd.engine_process import _TASK_FIELDS, task_to_wire

    assert {"seed", "logit_bias"} <= set(_TASK_FIELDS)
    d = task_to_wire(_task(seed=3, logit_bias={4: 2.0}))
    assert d["seed"] == 3 and d["logit_bias"] == {4: 2.0}


def test_chat_passes_seed_and_logit_bias_and_rejects_bad_values():
    async def main():
        record = []
        eng, cl = await _app_client(record)
        msgs = [{"role": "user", "content": "seeded"}]
        req = {"model": "rwkv-latest:no-thinking", "messages": msgs, "temperature": 0.0, "top_p": 0.0, "presence_penalty": 0.0,
               "frequency_penalty": 0.0, "penalty_decay": 1.0, "max_tokens": 5}
        async with cl:
            plain = await cl.post("/v1/chat/completions", json=req)
            assert plain.status_code == 200 and record[-1].seed is None and record[-1].logit_bias == {}
            pj = plain.json()
            assert list(pj) == ["id", "object", "created", "model", "choices", "usage"]
            assert list(pj["choices"][0]) == ["index", "finish_reason", "message"]
            r = await cl.post("/v1/chat/completions", json=dict(req, seed=-12, logit_bias={"17": 100, "018": -2.5}))
            assert r.status_code == 200, r.text
            assert record[-1].seed == -12 and record[-1].logit_bias == {17: 100.0, 18: -2.5}
            assert record[-1].generated_tokens == [17] * 5 and r.json()["choices"][0]["message"]["content"] == "<17>" * 5
            assert list(r.json()) == list(pj) and list(r.json()["choices"][0]) == list(pj["choices"][0])
            s1 = await cl.post("/v1/chat/completions", json=dict(req, temperature=1.0, top_p=1.0, seed=(1 << 64) - 1, max_tokens=8))
            s2 = await cl.post("/v1/chat/completions", json=dict(req, temperature=1.0, top_p=1.0, seed=-1, max_tokens=8))
            assert s1.status_code == s2.status_code == 200
            assert record[-1].generated_tokens == record[-2].generated_tokens           # the same uint64 seed
            n = len(record)
            for bad in ({"logit_bias": {"abc": 1}}, {"logit_bias": {"-1": 1}}, {"logit_bias": {"1.0": 1}}, {"logit_bias": {" 1": 1}},
                        {"logit_bias": {"1": 100.5}}, {"logit_bias": {"1": -101}}, {"logit_bias": {"1": "x"}},
                        {"logit_bias": {"1": 1, "01": 2}}, {"logit_bias": {str(i): 0 for i in range(LOGIT_BIAS_MAX + 1)}},
                        {"seed": 1 << 64}, {"seed": -(1 << 63) - 1}, {"seed": "abc"}, {"seed": 1.5}):
                rb = await cl.post("/v1/chat/completions", json=dict(req, **bad))
                assert rb.status_code == 422, (bad, rb.status_code)
            for bad in ({"logit_bias": {str(V): 1}}, {"logit_bias": {"3": 1, "99999": -1}}):
                rb = await cl.post("/v1/chat/completions", json=dict(req, **bad))
                assert rb.status_code == 400 and "vocabulary" in rb.text, (bad, rb.status_code)
            assert len(record) == n                                                     # none reached the engine
        eng.shutdown()

    asyncio.run(main())


def test_chat_request_fields():
    r = ChatCompletionRequest(messages=[{"role": "user", "content": "hi"}])
    assert r.seed is None and r.logit_bias is None and r.token_bias() == {}
    r = ChatCompletionRequest(messages=[], seed=5, logit_bias={"7": -100, "0": 100})
    assert r.token_bias() == {7: -100.0, 0: 100.0}
    assert chat_prompt([ChatMessage(role="user", content="x")], "rwkv-latest")[0]


# --------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_exports_and_checks_arguments():
    import chirrup_amd
    from chirrup_amd import lib

    hdr = open(os.path.join(ROOT, "include", "chirrup_amd.h")).read()
    assert re.search(r"int rwkv7_seeded_uniform\(int n_rows, const int32_t \*rows, const int32_t \*slot_idx, const uint64_t \*seeds", hdr)
    assert re.search(r"int rwkv7_apply_logit_bias\(int n_rows, int V, int cap, void \*logits, const int32_t \*slot_idx", hdr)
    assert int(re.search(r"#define\s+CHIRRUP_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    L = chirrup_amd.load()
    assert L.chirrup_abi_version() == 4
    assert len(lib.SIGNATURES["rwkv7_seeded_uniform"][1]) == 8 and len(lib.SIGNATURES["rwkv7_apply_logit_bias"][1]) == 9
    su, lb = L.rwkv7_seeded_uniform, L.rwkv7_apply_logit_bias
    p = ctypes.c_void_p(4096)                                  # never dereferenced: validation fails first (or n == 0)
    assert su(-1, p, p, p, p, p, p, None) == -1
    assert su(0, None, None, None, None, None, None, None) == 0          # nothing to do, nothing launched
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert su(1, *args, None) == -2, k
    assert su(1, p, p, ctypes.c_void_p(4100), p, p, p, None) == -3       # seeds: 8-byte aligned
    assert lb(-1, 8, 4, p, None, p, p, p, None) == -1
    assert lb(1, 0, 4, p, None, p, p, p, None) == -1
    assert lb(1, 8, 0, p, None, p, p, p, None) == -1
    assert lb(0, 8, 4, None, None, None, None, None, None) == 0
    assert lb(1, 8, 4, None, None, p, p, p, None) == -2
    assert lb(1, 8, 4, p, None, None, p, p, None) == -2
    assert lb(1, 8, 4, p, None, p, None, p, None) == -2
    assert lb(1, 8, 4, p, None, p, p, None, None) == -2
    assert lb(1, 8, 4, ctypes.c_void_p(4097), None, p, p, p, None) == -3
