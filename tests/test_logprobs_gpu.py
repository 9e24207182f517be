"""GPU: token log-probabilities (include/chirrup_amd.h: rwkv7_token_logprobs) against a float64 host reference from the same binary16
values, their determinism, and the worker / process-mode engine that carry them to a client.

Error ceiling ("Token logprobs"): lp = (l_t - m) - log Z with l_t - m exact, Z a binary32 sum of <= 65 536 terms in
[0, 1] -- 64 sequential terms per lane, a 64-lane tree, 16 wave sums in order: relative error <= (63 + 6 + 15) u (u = 2^-24) plus the
few-ulp exp, i.e. about 5.3e-6 on log Z -- and the final subtraction rounds once (|lp| u <= 1.8e-6 at lp >= -30).  Ceiling 2e-5
for lp >= -30."""
import asyncio
import json
import os
import queue

import numpy as np
import pytest
import torch

from chirrup_amd import ops

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CEIL = 2e-5
KS = (0, 1, 5, 20)
_MEASURED = []


def _ref(l16, k):
    """float64 log_softmax, top-k ids by logit descending then id ascending."""
    x = l16.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    lp = (x - m) - np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    order = np.lexsort((np.broadcast_to(np.arange(x.shape[1]), x.shape), -x), axis=1)[:, :k]
    return lp, order


def _cases():
    rng = np.random.default_rng(11)
    V = 65536
    yield "normal_n200", (rng.standard_normal((200, V)) * 3).astype(np.float16)
    yield "heavy_ties", (np.round(rng.standard_normal((8, V)) * 1.5) * 2).astype(np.float16)
    yield "all_equal", np.full((2, V), 1.25, np.float16)
    dom = (rng.standard_normal((3, V)) * 0.1).astype(np.float16)
    dom[np.arange(3), [5, 60000, 65535]] = 40.0
    yield "dominant", dom
    ext = np.zeros((2, V), np.float16)
    ext[0, ::7] = 65504
    ext[0, 3::11] = -65504
    ext[1, ::5] = -65504
    ext[1, 17] = 65504
    yield "pm65504", ext
    yield "small_V", (rng.standard_normal((5, 200)) * 2).astype(np.float16)


def _check(name, l16, k, lp, ids, targets):
    want, order = _ref(l16, k)
    assert np.array_equal(ids, order.astype(np.int32)), f"{name} K={k}: top ids"
    n = l16.shape[0]
    got_t, want_t = lp[:, 0].astype(np.float64), want[np.arange(n), targets]
    got_k, want_k = lp[:, 1:].astype(np.float64), np.take_along_axis(want, order, axis=1)
    errs = []
    for g, w in ((got_t, want_t), (got_k, want_k)):
        sel = w >= -30
        if sel.any():
            errs.append(float(np.abs(g[sel] - w[sel]).max()))
    err = max(errs) if errs else 0.0
    _MEASURED.append({"case": name, "K": k, "max_abs_err_lp_ge_-30": err})
    assert err <= CEIL, f"{name} K={k}: {err}"


@pytest.mark.parametrize("k", KS)
def test_token_logprobs_matches_float64_reference(k):
    rng = np.random.default_rng(k)
    for name, l16 in _cases():
        n, V = l16.shape
        targets = rng.integers(0, V, n).astype(np.int32)
        targets[0] = int(l16[0].astype(np.float32).argmax())
        t_l = torch.from_numpy(l16).cuda()
        t_t = torch.from_numpy(targets).cuda()
        lp, ids = ops.token_logprobs(t_l, k, targets=t_t)
        lp2, ids2 = ops.token_logprobs(t_l, k, targets=t_t)
        lp, ids, lp2, ids2 = (x.cpu().numpy() for x in (lp, ids, lp2, ids2))
        assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(ids, ids2), f"{name}: two launches differ"
        _check(name, l16, k, lp, ids, targets)
        if name == "all_equal" and k:
            assert ids[0].tolist() == list(range(k)) and abs(lp[0, 1] + np.log(V)) <= CEIL
    print(json.dumps(_MEASURED))                                 # the measured errors (profiles/r05_token_logprobs.json)
    _MEASURED.clear()


def test_token_logprobs_row_independent_of_batch_indirection_and_k():
    """A row's bits are the same alone, in a batch of 200, through row indirection, and at another K (a prefix); bad targets: NaN."""
    rng = np.random.default_rng(3)
    V = 65536
    l16 = (rng.standard_normal((200, V)) * 2).astype(np.float16)
    l16[17, rng.integers(0, V, 300)] = 7.5                    # ties at the top
    t_l = torch.from_numpy(l16).cuda()
    tg = torch.from_numpy(rng.integers(0, V, 200).astype(np.int32)).cuda()
    lp_all, ids_all = ops.token_logprobs(t_l, 20, targets=tg)
    rows = torch.tensor([17, 3, 17], dtype=torch.int32, device="cuda")
    lp_ind, ids_ind = ops.token_logprobs(t_l, 20, targets=tg, rows=rows, target_rows=rows)
    lp_one, ids_one = ops.token_logprobs(t_l[17:18].contiguous(), 20, targets=tg[17:18].contiguous())
    lp_k5, ids_k5 = ops.token_logprobs(t_l, 5, targets=tg)
    b = lambda x: x.cpu().numpy().view(np.uint32) if x.dtype == torch.float32 else x.cpu().numpy()
    for lp, ids, r in ((lp_ind, ids_ind, 0), (lp_ind, ids_ind, 2), (lp_one, ids_one, 0)):
        assert np.array_equal(b(lp[r]), b(lp_all[17])) and np.array_equal(b(ids[r]), b(ids_all[17]))
    assert np.array_equal(b(lp_ind[1]), b(lp_all[3]))
    assert np.array_equal(b(lp_k5), b(lp_all[:, :6])) and np.array_equal(b(ids_k5), b(ids_all[:, :5]))
    bad = torch.tensor([-1, V, 5], dtype=torch.int32, device="cuda")
    lp_bad, _ = ops.token_logprobs(t_l[:3].contiguous(), 2, targets=bad)
    v = lp_bad[:, 0].cpu().numpy()
    assert np.isnan(v[0]) and np.isnan(v[1]) and np.isfinite(v[2])


def _tiny_model():
    import types

    from chirrup_amd.rwkv7 import RWKV_x070

    d = np.load(os.path.join(G, "model_L2_C128.npz"))
    zd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}
    return RWKV_x070(types.SimpleNamespace(vocab_size=320, head_size=64, MODEL_NAME="unused"), state_dict=zd, device="cuda:0")


class _Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "".join(chr(65 + i % 26) for i in ids)


class _Sink:
    def __init__(self):
        self.items = []

    def put_nowait(self, x):
        self.items.append(x)


def _run_worker(m, reqs, use_graph):
    from chirrup_amd.core_structure import ModelLoadConfig, Task
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=320, head_size=64)
    tq, mq = queue.Queue(), queue.Queue()
    w = Worker("w0", [0], cfg, tq, mq, None, batch_size=6, model=m, tokenizer=_Tok())
    w._init_worker()
    w.use_graph = use_graph and w.use_graph
    sinks = []
    for prompt, kw in reqs:
        s = _Sink()
        sinks.append(s)
        tq.put(Task(output_queue=s, task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None,
                    max_tokens=12, stop_tokens=[], **kw))
    for _ in range(400):
        if not w.step() and all(any(k == "task_completed" for k, _ in s.items) for s in sinks):
            break
    return [[p for k, p in s.items if k == "token_generated"] for s in sinks]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_worker_logprobs_are_those_of_the_raw_logits(use_graph):
    m = _tiny_model()
    rng = np.random.default_rng(9)
    prompts = [rng.integers(1, 320, n).tolist() for n in (3, 12, 30, 5)]
    greedy = dict(temperature=0.0, top_p=0.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_decay=1.0)
    pen = dict(temperature=1.0, top_p=0.7, presence_penalty=0.5, frequency_penalty=0.5, penalty_decay=0.996, forbidden_tokens=[1, 2])
    lpkw = dict(logprobs=True, top_logprobs=20, return_logits=True)
    reqs = [(prompts[0], dict(greedy, **lpkw)), (prompts[1], dict(pen, **lpkw)), (prompts[2], dict(greedy, logprobs=True, top_logprobs=3)),
            (prompts[3], dict(greedy))]
    out = _run_worker(m, reqs, use_graph)
    assert all(len(o) == 12 for o in out)
    for o in out[:2]:                                         # lp == log_softmax(float64(raw))[id], top ids exact
        for tok, _text, raw, lp in o:
            want, order = _ref(raw.numpy()[None], 20)
            assert abs(lp["logprob"] - want[0, tok]) <= CEIL
            assert [i for i, _ in lp["top_logprobs"]] == order[0].tolist()
            assert max(abs(v - want[0, i]) for i, v in lp["top_logprobs"]) <= CEIL
    for o in (out[0], out[2]):                                # greedy, no penalties: the token is the top entry
        for p in o:
            assert p[3]["top_logprobs"][0][0] == p[0]
    assert all(p[2] is None and len(p[3]["top_logprobs"]) == 3 for p in out[2])
    assert all(len(p) == 2 for p in out[3])
    # greedy ids do not depend on whether logprobs were asked for
    off = _run_worker(m, [(prompts[0], dict(greedy)), (prompts[2], dict(greedy))], use_graph)
    assert [p[0] for p in off[0]] == [p[0] for p in out[0]] and [p[0] for p in off[1]] == [p[0] for p in out[2]]


def test_process_mode_engine_carries_logprobs(tmp_path):
    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.engine_core import AsyncEngineCore

    d = np.load(os.path.join(G, "model_L2_C128.npz"))
    zd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}
    ckpt = os.path.join(tmp_path, "tiny.pth")
    torch.save(zd, ckpt)
    vocab = os.path.join(G, "mini_vocab.txt")
    kw = dict(temperature=0.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, stop_tokens=[])

    async def run(mode):
        eng = AsyncEngineCore(worker_mode=mode)
        cfg = ModelLoadConfig(model_path=ckpt, vocab_path=vocab, vocab_size=320, head_size=64)
        await asyncio.wait_for(eng.init(worker_num=1, model_config=cfg, batch_size=4), 300)
        c = eng.completion("hello world", max_tokens=8, logprobs=True, top_logprobs=5, **kw)
        evs = [ev for ev in [e async for e in c] if ev[0] == "token"]
        c = eng.completion("hello world", max_tokens=8, **kw)
        plain = [ev for ev in [e async for e in c] if ev[0] == "token"]
        eng.shutdown()
        return evs, plain

    evs_t, plain_t = asyncio.run(run("thread"))
    evs_p, plain_p = asyncio.run(run("process"))
    assert len(evs_p) == 8 and all(len(e) == 5 and e[3] is None for e in evs_p)
    assert [(e[1], e[4]) for e in evs_p] == [(e[1], e[4]) for e in evs_t]
    assert all(e[4]["top_logprobs"][0][0] == e[1] and len(e[4]["top_logprobs"]) == 5 for e in evs_p)
    assert all(len(e) == 3 for e in plain_p) and [e[1] for e in plain_p] == [e[1] for e in evs_p]
