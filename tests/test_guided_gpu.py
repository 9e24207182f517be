"""GPU: guided decoding.  The three kernels (rwkv7_guide_build / _apply / _advance) bit for bit against their CPU forms -- the build
for every pattern of the CPU list with the real vocabulary (V = 65 536; tests/golden/rwkv_vocab_v20230424.txt.gz is a gzip of the
vocabulary file, byte for byte) and the mini vocabulary (V = 320) --, then the real Worker on the L2/C128 golden model and the
0.1B synthetic model: greedy, sampled and seeded requests under bounded patterns all end "stop" with a matching text, the same
prompts unguided do not match, greedy rows equal a host replay from the raw logits; and one request through the engine and the
chat route with response_format json_schema."""
import asyncio
import gzip
import json
import os
import queue
import re

import numpy as np
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.guided import compile_regex, schema_to_regex, token_table
from chirrup_amd.tokenizer import TRIE_TOKENIZER
from guided_cases import ALL_PATTERNS, validate
from test_decode_sampling_gpu import _model, _Sink
from util import replay_decode

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB = {"L2C128": 320, "0.1B": 65536}
_TOK = {}


def _tokenizer(model, tmp_path_factory):
    if model not in _TOK:
        path = os.path.join(G, "mini_vocab.txt")
        if model == "0.1B":
            path = str(tmp_path_factory.mktemp("vocab") / "rwkv_vocab_v20230424.txt")
            with gzip.open(os.path.join(G, "rwkv_vocab_v20230424.txt.gz"), "rb") as src, open(path, "wb") as dst:
                dst.write(src.read())
        _TOK[model] = TRIE_TOKENIZER(path)
    return _TOK[model]


# ------------------------------------------------------------------------------------------------------------ the kernels
def _filled_pool(dfas, V, tok, stops, device):
    """Every dfa one behind the other (gaps between them) in a pool on `device`, built by ops.guide_build there."""
    off, data = token_table(tok.idx2token, V)
    P = sum(d.n_states + 3 for d in dfas) + 5
    nxt = torch.full((P, 256), -1, dtype=torch.int32)
    rows, at = [], 2
    for d in dfas:
        nxt[at:at + d.n_states] = torch.from_numpy(np.where(d.next >= 0, d.next + at, -1).astype(np.int32))
        rows.append(at)
        at += d.n_states + 3
    nxt = nxt.to(device)
    allow = torch.full((P, V // 32), 0x5A5A5A5A, dtype=torch.int32, device=device)        # rows outside the guides must stay as they are
    tok_off, tok_bytes = torch.from_numpy(off).to(device), torch.from_numpy(data).to(device)
    special = torch.tensor(stops, dtype=torch.int32, device=device)
    for d, r0 in zip(dfas, rows):
        ops.guide_build(d.n_states, r0, nxt, tok_off, tok_bytes, special, torch.from_numpy(d.accept.astype(np.uint8)).to(device), allow)
    return nxt, allow, tok_off, tok_bytes, rows


@pytest.mark.parametrize("model", ["0.1B", "L2C128"])
def test_guide_build_kernel_matches_host_form_for_every_pattern(model, tmp_path_factory):
    V, tok = VOCAB[model], _tokenizer(model, tmp_path_factory)
    if model == "0.1B":
        assert len(tok.idx2token) == 65530 and max(len(b) for b in tok.idx2token.values()) == 128
    dfas = [compile_regex(p) for p, _ in ALL_PATTERNS]
    stops = [0, 261, 24281, V + 5]
    h = _filled_pool(dfas, V, tok, stops, "cpu")
    d = _filled_pool(dfas, V, tok, stops, "cuda")
    torch.cuda.synchronize()
    got, want = d[1].cpu().numpy(), h[1].numpy()
    assert np.array_equal(got, want), [p for (p, _), r0, x in zip(ALL_PATTERNS, h[4], dfas)
                                       if not np.array_equal(got[r0:r0 + x.n_states], want[r0:r0 + x.n_states])][:3]
    used = np.zeros(len(want), bool)
    for r0, x in zip(h[4], dfas):
        used[r0:r0 + x.n_states] = True
    assert (got[~used] == 0x5A5A5A5A).all() and (got[used] != 0).any(axis=1).all() == (model == "0.1B")
    # spot checks of the meaning, on the first pattern ("a"): its start state allows exactly the tokens that spell "a"
    bits = np.unpackbits(want[h[4][0]].view(np.uint8), bitorder="little")
    assert [tok.idx2token[i] for i in np.nonzero(bits)[0]] == [b"a"]
    acc = np.unpackbits(want[h[4][0] + 1].view(np.uint8), bitorder="little")
    assert sorted(np.nonzero(acc)[0]) == sorted(s for s in stops if s < V)       # the accepting state: only the stop ids


@pytest.mark.parametrize("V", [65536, 320])
def test_guide_apply_kernel_matches_host_form(V):
    rng = np.random.default_rng(V)
    P, S, n = 37, 260, 200
    allow = torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, (P, V // 32), dtype=np.int64).astype(np.int32))
    allow[0], allow[1] = 0, -1                                                       # nothing allowed / everything allowed
    allow[2, ::2] = -1                                                               # whole groups allowed: never read
    allow[3] = torch.from_numpy(np.where(rng.random(V // 32) < 0.9, 0, 1 << rng.integers(0, 31, V // 32)).astype(np.int32))
    lg = (rng.standard_normal((n, V)) * 4).astype(np.float16)
    lg[rng.random((n, V)) < 0.01] = -np.inf
    lg[rng.random((n, V)) < 0.01] = np.nan
    lg[:, 0], lg[:, 1] = np.inf, -65504
    lg = torch.from_numpy(lg)
    state = torch.from_numpy(rng.integers(-1, P, S).astype(np.int32))
    state[:6] = torch.tensor([0, 1, 2, 3, -1, P - 1], dtype=torch.int32)
    slot_idx = torch.from_numpy(rng.permutation(S)[:n].astype(np.int32))
    slot_idx[:6] = torch.arange(6, dtype=torch.int32)
    rows = torch.from_numpy(np.sort(rng.permutation(n)[:150]).astype(np.int32))
    rows[:6] = torch.arange(6, dtype=torch.int32)
    for si in (slot_idx, None):
        h, d = lg.clone(), lg.cuda()
        st = state if si is not None else state[:n].contiguous()
        ops.guide_apply(h, rows, si, st, allow)
        ops.guide_apply(d, rows.cuda(), si.cuda() if si is not None else None, st.cuda(), allow.cuda())
        torch.cuda.synchronize()
        got, want, raw = d.cpu().numpy().view(np.uint16), h.numpy().view(np.uint16), lg.numpy().view(np.uint16)
        assert np.array_equal(got, want)
        assert (got[0] == 0xFC00).all() and np.array_equal(got[1], raw[1]) and np.array_equal(got[4], raw[4])
        unlisted = np.setdiff1d(np.arange(n), rows.numpy())
        assert np.array_equal(got[unlisted], raw[unlisted]) and not np.array_equal(got, raw)
    ops.guide_apply(lg.cuda(), rows[:0].cuda(), slot_idx.cuda(), state.cuda(), allow.cuda())


@pytest.mark.parametrize("model", ["0.1B", "L2C128"])
def test_guide_advance_kernel_matches_host_form(model, tmp_path_factory):
    V, tok = VOCAB[model], _tokenizer(model, tmp_path_factory)
    rng = np.random.default_rng(7)
    dfas = [compile_regex(p) for p, _ in ALL_PATTERNS]
    nxt, allow, tok_off, tok_bytes, starts = _filled_pool(dfas, V, tok, [0], "cpu")
    P, S, n = nxt.shape[0], 300, 256
    live = torch.nonzero((nxt >= 0).any(dim=1)).view(-1)
    for trial in range(3):
        state = live[torch.from_numpy(rng.integers(0, len(live), S))].to(torch.int32)
        state[rng.random(S) < 0.2] = -1
        slot_idx = torch.from_numpy(rng.permutation(S)[:n].astype(np.int32))
        rows = torch.from_numpy(rng.permutation(n)[:200].astype(np.int32))
        ids = rng.integers(0, V, n)
        # half of the listed rows get a token their state allows (the walk survives); the others are random: dying, undefined
        # (ids past the vocabulary file), the stop id, out of range
        for r in rows.tolist()[::2]:
            s = int(state[slot_idx[r]])
            if s >= 0:
                ok = np.nonzero(np.unpackbits(allow[s].numpy().view(np.uint8), bitorder="little")[:V])[0]
                if len(ok):
                    ids[r] = ok[rng.integers(0, len(ok))]
        ids[rows[1].item()], ids[rows[3].item()], ids[rows[5].item()], ids[rows[7].item()] = 0, V - 1, V + 3, -2
        ids = torch.from_numpy(ids.astype(np.int32))
        h, d = state.clone(), state.cuda()
        ops.guide_advance(rows, slot_idx, ids, tok_off, tok_bytes, nxt, h)
        ops.guide_advance(rows.cuda(), slot_idx.cuda(), ids.cuda(), tok_off.cuda(), tok_bytes.cuda(), nxt.cuda(), d)
        torch.cuda.synchronize()
        assert torch.equal(d.cpu(), h), trial
        moved = int((h != state).sum())
        assert 20 <= moved <= 200 and torch.equal(h[state < 0], state[state < 0]), moved


# ------------------------------------------------------------------------------------------------------------ the worker
# bounded patterns (no * / + / {m,}): the longest match is shorter than max_tokens
BOUNDED = {
    "0.1B": [r"(yes|no|maybe)", r"\d{3}-\d{4}", r"[A-Z][a-z]{2,8} [A-Z][a-z]{2,8}", r"(19|20)\d\d-(0[1-9]|1[0-2])-(0[1-9]|[12]\d|3[01])",
             r"héllo|wörld", r"[éü中]{1,3}!", r"-?(0|[1-9]\d{0,5})(\.\d{1,3})?",
             schema_to_regex({"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "integer"},
                                                               "tags": {"type": "array", "items": {"enum": ["a", "b"]}, "maxItems": 3}}})],
    "L2C128": [r"(yes|no|maybe)", r"\d{3}-\d{4}", r"[a-z]{2,8} (the|then|here)", r"0x[0-9a-f]{1,8}",
               schema_to_regex({"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "integer"}}})],
}
MAX_TOKENS = 96


def _specs(model, V):
    rng = np.random.default_rng(V + 1)
    z = dict(frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0)
    pen = dict(frequency_penalty=0.5, presence_penalty=0.5, penalty_decay=0.996)
    specs = []
    for k, p in enumerate(BOUNDED[model]):
        P = lambda n: rng.integers(1, V, n).tolist()
        specs += [(p, P(4), dict(temperature=0.0, top_p=0.0, top_k=0, **(pen if k % 2 else z))),
                  (p, P(7), dict(temperature=1.0, top_p=0.9, top_k=0, **(z if k % 2 else pen))),
                  (p, P(3), dict(temperature=1.2, top_p=1.0, top_k=0, seed=100 + k, **z))]
    return specs


def _run(m, V, tok, specs, guided, run_ahead, use_graph, batch_size=7):
    from chirrup_amd.core_structure import ModelLoadConfig, Task
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=batch_size, model=m, tokenizer=tok, run_ahead=run_ahead)
    w._init_worker()
    assert w.use_graph
    w.use_graph = use_graph
    tasks = [Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(p), state=None,
                  stop_tokens=[0], return_logits=True, max_tokens=MAX_TOKENS, guide=compile_regex(pat) if guided else None, **kw)
             for pat, p, kw in specs]
    torch.manual_seed(11)
    for t in tasks:
        tq.put(t)
    for _ in range(6000):
        if not w.step():
            break
    assert all(t.output_queue.items[-1][0] == "task_completed" for t in tasks)
    return w, tasks


def _masked(dfa, tok, V, raw_steps, emitted, stops=(0,)):
    """Each step's raw logits masked by the host form, the automaton's state followed along the emitted ids on the host."""
    off, data = token_table(tok.idx2token, V)
    nxt = torch.from_numpy(dfa.next.copy())
    allow = torch.zeros((dfa.n_states, V // 32), dtype=torch.int32)
    tok_off, tok_bytes = torch.from_numpy(off), torch.from_numpy(data)
    ops.guide_build(dfa.n_states, 0, nxt, tok_off, tok_bytes, torch.tensor(stops, dtype=torch.int32),
                    torch.from_numpy(dfa.accept.astype(np.uint8)), allow)
    state = torch.zeros((1,), dtype=torch.int32)
    out, one = [], torch.zeros((1,), dtype=torch.int32)
    for raw, t in zip(raw_steps, emitted):
        lg = torch.from_numpy(np.array(raw, np.float16).reshape(1, V).copy())
        ops.guide_apply(lg, one, None, state, allow)
        out.append(lg.numpy()[0])
        ops.guide_advance(one, None, torch.tensor([t], dtype=torch.int32), tok_off, tok_bytes, nxt, state)
    return out, int(state[0])


@pytest.mark.parametrize("mode", [(True, True), (False, False)], ids=["graph-run_ahead", "eager-in_step"])
@pytest.mark.parametrize("model", ["L2C128", "0.1B"])
def test_guided_requests_on_the_gpu_stop_with_matching_text_and_equal_the_host_replay(model, mode, tmp_path_factory):
    from chirrup_amd.core_structure import RequestStatus

    V, tok, m = VOCAB[model], _tokenizer(model, tmp_path_factory), _model(model)
    specs = _specs(model, V)
    w, tasks = _run(m, V, tok, specs, True, *mode)
    replayed = ties = 0
    for (pat, _, kw), t in zip(specs, tasks):
        text = tok.decodeBytes(t.generated_tokens).decode("utf-8")
        assert t.request_status == RequestStatus.FINISHED_STOPPED and t.error is None, (pat, kw, t.request_status, text)
        assert re.fullmatch(pat, text, re.ASCII) is not None, (pat, text)
        assert 0 < len(t.generated_tokens) < MAX_TOKENS
        if kw["temperature"] == 0:                  # greedy: mask (host form) -> penalties -> arg-max must give the emitted ids
            raw = [p[2].numpy() for k, p in t.output_queue.items if k == "token_generated"]
            dfa = compile_regex(pat)
            masked, end = _masked(dfa, tok, V, raw, t.generated_tokens)
            assert dfa.accept[end]
            want, pen = replay_decode(masked, t.generated_tokens, kw["frequency_penalty"], kw["presence_penalty"], kw["penalty_decay"])
            for k, (a, b) in enumerate(zip(t.generated_tokens, want)):
                replayed += 1
                if a != b:                          # a tie of the top two masked logits: either id counts
                    ties += 1
                    assert pen[k][a] == pen[k][b] == np.nanmax(pen[k]), (pat, k, a, b)
    print(f"{model}: {replayed} greedy steps replayed, {ties} ties")
    assert replayed >= 20
    assert all(e["refs"] == 0 for e in w._guides.entries.values()) and w._guides.builds == len(BOUNDED[model])
    # the control: the same prompts without a guide do not produce matching texts
    _, plain = _run(m, V, tok, specs, False, *mode)
    hits = sum(re.fullmatch(pat, tok.decodeBytes([i for i in t.generated_tokens if i in tok.idx2token]).decode("utf-8", "replace"), re.ASCII)
               is not None for (pat, _, _), t in zip(specs, plain))
    assert hits == 0


def test_chat_route_with_a_json_schema_on_the_gpu(tmp_path):
    import httpx

    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.engine_core import AsyncEngineCore
    from chirrup_amd.web_service import create_app

    d = np.load(os.path.join(G, "model_L2_C128.npz"))
    ckpt = os.path.join(tmp_path, "tiny.pth")
    torch.save({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}, ckpt)
    schema = {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "integer"}, "kind": {"enum": ["abc", "the"]}}}

    async def main():
        eng = AsyncEngineCore()
        cfg = ModelLoadConfig(model_path=ckpt, vocab_path=os.path.join(G, "mini_vocab.txt"), vocab_size=320, head_size=64)
        await eng.init(worker_num=1, model_config=cfg, batch_size=4)
        c = eng.completion("hello", guided_json=schema, stop_tokens=[0], max_tokens=80, temperature=1.0, top_p=0.8, seed=5)
        direct = await c.get_full_completion()
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(eng, state_cache_size=0)), base_url="http://t") as cl:
            r = await cl.post("/v1/chat/completions", json={
                "model": "rwkv-latest:no-thinking", "messages": [{"role": "user", "content": "give me json"}], "max_tokens": 80,
                "response_format": {"type": "json_schema", "json_schema": {"name": "answer", "schema": schema}}})
        eng.shutdown()
        return c.task, direct, r

    task, direct, r = asyncio.run(main())
    assert str(task.request_status) == "FINISHED_STOPPED" and validate(schema, json.loads(direct)), direct
    assert r.status_code == 200, r.text
    content = r.json()["choices"][0]["message"]["content"]
    assert validate(schema, json.loads(content)), content
