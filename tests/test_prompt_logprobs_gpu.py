"""GPU: prompt logprobs -- forward_slots(logit_rows=...) against the same forward's full_output rows, the worker's prompt positions
against a float64 log-softmax of the numpy oracle's full_output logits, scoring against the decode path, independence of the chunk
length, and POST /v1/completions through a process-mode engine.

Bar of a prompt logprob against the oracle: lp = l_t - logsumexp(l), so |d lp| <= |d l_t| + max |d l| <= 2 max |d l|: twice the
committed logit parity bar (3e-3 relative to the largest logit, tests/test_model_gpu.py) plus the logprob kernel's 2e-5 ceiling
("Token logprobs").  The synthetic V = 65 536 model (C = 256, random weights) is held to 1e-2 relative: its largest logit
is ~5.4, where one binary16 ulp is 4e-3, and its measured worst top-5 entry was 0.039 (about 5 ulp of a logit).  The measured
errors are printed beside the bars."""
import asyncio
import json
import os
import queue
import types

import numpy as np
import pytest
import torch

from chirrup_amd import ops
from oracle import rwkv7_np as M

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CEIL = 2e-5
LOGIT_REL = 3e-3


def _golden_sd():
    d = np.load(os.path.join(G, "model_L2_C128.npz"))
    return {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}, 320


def _synth_sd():
    from chirrup_amd.synth import make_state_dict

    return make_state_dict(2, 256, vocab_size=65536, seed=7), 65536


def _model(sd, V, **kw):
    from chirrup_amd.rwkv7 import RWKV_x070

    return RWKV_x070(types.SimpleNamespace(vocab_size=V, head_size=64, MODEL_NAME="unused"), state_dict=dict(sd), device="cuda:0", **kw)


def _pool(m, n, seed=0):
    pool = m.generate_zero_state(n)
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool[0].copy_((torch.randn(pool[0].shape, generator=g, device="cuda") * 0.5).half())
    pool[1].copy_((torch.randn(pool[1].shape, generator=g, device="cuda") * 0.1).to(pool[1].dtype))
    return pool


def _clone(pool):
    return [t.clone() for t in pool]


@pytest.mark.parametrize("B,T,form", [(2, 100, "ring"), (3, 100, "library"), (2, 100, "mm8")])
def test_logit_rows_bit_identical_to_full_output_rows(B, T, form):
    """<= 256 rows: the ring kernel on both sides; above: one library call on both sides (resident row-major head); a uint8 head:
    one mm8t_linear call of <= 256 rows on both sides."""
    sd, V = _golden_sd()
    m = _model(sd, V, **({"att_dtype": torch.int8, "ffn_dtype": torch.int8} if form == "mm8" else {}))
    rng = np.random.default_rng(B)
    toks = rng.integers(1, V, (B, T)).tolist()
    slots = torch.tensor([4, 1, 6][:B], dtype=torch.int32, device="cuda")
    base = _pool(m, 8)
    p_full, p_rows = _clone(base), _clone(base)
    full = m.forward_slots(toks, p_full, slots, full_output=True).reshape(B * T, V)
    rows = torch.arange(B * T, dtype=torch.int32, device="cuda")
    last, got = m.forward_slots(toks, p_rows, slots, logit_rows=rows)
    assert got.shape == (rows.numel(), V)
    assert torch.equal(got, full[rows.long()]), form
    for a, b in zip(p_full, p_rows):
        assert torch.equal(a, b)
    # a sparse row list (the rows of the last sequence) and the sink form give the same bits, block by block
    sub = torch.arange((B - 1) * T, B * T, dtype=torch.int32, device="cuda")
    if form != "library":
        _, got2 = m.forward_slots(toks, _clone(base), slots, logit_rows=sub)
        assert torch.equal(got2, full[sub.long()])
    blocks = []
    m.forward_slots(toks, _clone(base), slots, logit_rows=rows, row_sink=lambda r0, blk: blocks.append((r0, blk.clone())))
    assert [r0 for r0, _ in blocks] == list(range(0, rows.numel(), 512))
    assert torch.equal(torch.cat([b for _, b in blocks]), got)
    # (the last-token logits are those of the plain forward's head form on the same ln_out rows)
    assert last.shape == (B, V)


def test_tile_only_model_above_256_rows_uses_ring_blocks():
    """keep_row_major=False: the head exists only as tile images -- 300 rows go through the ring kernel in 256-row blocks; bit for bit
    against ops.skinny_linear on the same gathered rows in the same blocks, and within the bar of the row-major model."""
    sd, V = _synth_sd()
    m_rm = _model(sd, V)
    m_t = _model(sd, V, keep_row_major=False)
    B, T = 3, 100
    toks = np.random.default_rng(1).integers(1, V, (B, T)).tolist()
    slots = torch.tensor([0, 2, 5], dtype=torch.int32, device="cuda")
    rows = torch.arange(B * T, dtype=torch.int32, device="cuda")
    _, got = m_t.forward_slots(toks, _pool(m_t, 6), slots, logit_rows=rows)
    # ln_out rows of the same forward, through the model's own full_output route, then the ring kernel in the same blocks
    xo_cap = {}
    orig = ops.add_ln_mix

    def spy(*a, **k):
        orig(*a, **k)
        xo_cap["xo"] = a[12]

    ops.add_ln_mix = spy
    try:
        m_t.forward_slots(toks, _pool(m_t, 6), slots, logit_rows=rows)
    finally:
        ops.add_ln_mix = orig
    x2 = xo_cap["xo"].reshape(B * T, -1)
    want = torch.cat([ops.skinny_linear(x2[r0:r0 + 256].contiguous(), m_t._head_ring(), splits=1) for r0 in range(0, B * T, 256)])
    assert torch.equal(got, want)
    _, ref = m_rm.forward_slots(toks, _pool(m_rm, 6), slots, logit_rows=rows)
    err = (got.float() - ref.float()).abs().max().item()
    bar = LOGIT_REL * max(1.0, ref.float().abs().max().item())
    print(json.dumps({"case": "tile-only vs row-major head, 300 rows", "max_abs_logit_diff": err, "bar": bar}))
    assert err <= bar


def _worker(m, V, batch_size=6, chunk=100, run_ahead=True):
    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.worker import Worker

    class _Tok:
        def decode(self, ids, utf8_errors="strict"):
            return "".join(chr(65 + i % 26) for i in ids)

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V, head_size=64)
    w = Worker("w0", [0], cfg, queue.Queue(), queue.Queue(), None, batch_size=batch_size, model=m, tokenizer=_Tok(), run_ahead=run_ahead)
    w._init_worker()
    w.max_forward_seq_len_per_forward = chunk
    return w


class _Sink:
    def __init__(self):
        self.items = []

    def put_nowait(self, x):
        self.items.append(x)


def _task(prompt, **kw):
    from chirrup_amd.core_structure import Task

    g = dict(temperature=0.0, top_p=0.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_decay=1.0, stop_tokens=[])
    g.update(kw)
    return Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **g)


def _drain(w, tasks):
    for _ in range(3000):
        if not w.step() and all(any(k == "task_completed" for k, _ in t.output_queue.items) for t in tasks):
            return
    raise AssertionError("worker did not drain")


def _prompt_lp(task):
    lps, tops = [], []
    for k, p in task.output_queue.items:
        if k == "prompt_logprobs":
            assert p["start"] == len(lps)
            lps += p["logprobs"]
            tops += p["top_logprobs"]
    return lps, tops


def _oracle_lp(sd, V, prompt):
    z = M.prepare_weights({k: v.numpy() for k, v in sd.items()})
    L = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    C = sd["emb.weight"].shape[1]
    st = [np.zeros((L, 2, 1, C), np.float16), np.zeros((L, 1, C // 64, 64, 64), np.float16), np.zeros((1,), np.int32)]
    lg = M.forward_seq_batch(z, [prompt], st, L, full_output=True)[0].astype(np.float64)     # [T, V]
    m = lg.max(axis=1, keepdims=True)
    return (lg - m) - np.log(np.exp(lg - m).sum(axis=1, keepdims=True)), np.abs(lg).max()


@pytest.mark.parametrize("which", ["L2_C128", "synth_V65536"])
def test_worker_prompt_logprobs_match_oracle(which):
    sd, V = _golden_sd() if which == "L2_C128" else _synth_sd()
    m = _model(sd, V)
    rng = np.random.default_rng(21)
    lens = (2, 9, 40, 130) if which == "L2_C128" else (9, 130)
    prompts = [rng.integers(1, V, n).tolist() for n in lens]
    w = _worker(m, V)
    asks = [_task(p, max_tokens=0 if i % 2 else 2, prompt_logprobs=5) for i, p in enumerate(prompts)]
    plain = _task(rng.integers(1, V, 50).tolist(), max_tokens=4)
    for t in asks + [plain]:
        w.task_queue.put(t)
    _drain(w, asks + [plain])
    worst, bar_used = 0.0, 0.0
    for p, t in zip(prompts, asks):
        lps, tops = _prompt_lp(t)
        assert len(lps) == len(p) and lps[0] is None
        want, lmax = _oracle_lp(sd, V, p)
        bar = 2 * (LOGIT_REL if V == 320 else 1e-2) * max(1.0, lmax) + CEIL
        for i in range(1, len(p)):
            worst = max(worst, abs(lps[i] - want[i - 1, p[i]]))
            assert abs(lps[i] - want[i - 1, p[i]]) <= bar, (len(p), i)
            assert len(tops[i]) == 5 and max(abs(v - want[i - 1, j]) for j, v in tops[i]) <= bar
        bar_used = max(bar_used, bar)
        if t.max_tokens == 0:
            assert not any(k == "token_generated" for k, _ in t.output_queue.items)
    assert not any(k == "prompt_logprobs" for k, _ in plain.output_queue.items)
    print(json.dumps({"case": f"worker prompt logprobs vs oracle ({which})", "max_abs_err": worst, "bar": bar_used}))


def test_scoring_matches_decode_logprobs_and_chunk_length():
    sd, V = _golden_sd()
    m = _model(sd, V)
    rng = np.random.default_rng(3)
    P = rng.integers(1, V, 57).tolist()
    w = _worker(m, V)
    gen = _task(P, max_tokens=1, logprobs=True)
    w.task_queue.put(gen)
    _drain(w, [gen])
    (x, _text, _raw, lp), = [p for k, p in gen.output_queue.items if k == "token_generated"]
    res = {}
    for chunk in (100, 16):
        w = _worker(m, V, chunk=chunk)
        sc = _task(P + [x], max_tokens=0, prompt_logprobs=0)
        w.task_queue.put(sc)
        _drain(w, [sc])
        res[chunk], _ = _prompt_lp(sc)
    st = m.generate_zero_state(1)
    lmax = m.forward_seq_batch_seperate([P], st).float().abs().max().item()
    bar = 2 * LOGIT_REL * max(1.0, lmax) + CEIL
    d_dec = abs(res[100][-1] - lp["logprob"])
    d_chunk = max(abs(a - b) for a, b in zip(res[100][1:], res[16][1:]))
    print(json.dumps({"case": "scoring vs decode logprob; chunk 100 vs 16", "decode_diff": d_dec, "chunk_diff": d_chunk, "bar": bar}))
    assert d_dec <= bar and d_chunk <= bar


def test_process_mode_completions_echo_logprobs(tmp_path):
    import httpx

    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.engine_core import AsyncEngineCore
    from chirrup_amd.web_service import create_app

    sd, V = _golden_sd()
    ckpt = os.path.join(tmp_path, "tiny.pth")
    torch.save(sd, ckpt)
    vocab = os.path.join(G, "mini_vocab.txt")

    async def run():
        eng = AsyncEngineCore(worker_mode="process")
        cfg = ModelLoadConfig(model_path=ckpt, vocab_path=vocab, vocab_size=V, head_size=64)
        await asyncio.wait_for(eng.init(worker_num=1, model_config=cfg, batch_size=4), 300)
        try:
            app = create_app(eng, state_cache_size=0)
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=120) as cl:
                r = await cl.post("/v1/completions", json={"prompt": "hello world", "echo": True, "logprobs": 3, "max_tokens": 0})
                r2 = await cl.post("/v1/completions", json={"prompt": "hello world", "echo": True, "logprobs": 3, "max_tokens": 3,
                                                            "temperature": 0.0, "top_p": 0.0})
            return r.status_code, r.json(), r2.json()
        finally:
            eng.shutdown()

    code, j, j2 = asyncio.run(run())
    assert code == 200
    c = j["choices"][0]
    n = j["usage"]["prompt_tokens"] - 1
    assert c["text"] == "hello world" and c["finish_reason"] == "length" and j["usage"]["completion_tokens"] == 0
    lp = c["logprobs"]
    assert len(lp["tokens"]) == n and all(isinstance(v, float) and v <= 0 for v in lp["token_logprobs"])
    assert all(len(d) <= 3 and d for d in lp["top_logprobs"])
    lp2 = j2["choices"][0]["logprobs"]
    assert len(lp2["tokens"]) == n + j2["usage"]["completion_tokens"]
    # the same prompt positions, computed in batches of another composition
    assert max(abs(a - b) for a, b in zip(lp2["token_logprobs"][:n], lp["token_logprobs"])) <= 0.05
