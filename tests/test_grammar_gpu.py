"""GPU: grammar-guided decoding.  The four kernels (rwkv7_grammar_build / _apply / _advance / _reset) bit for bit against their CPU
forms (which test_grammar_cpu.py holds to StackDFA.walk): the build for every case grammar with the real vocabulary (V = 65 536)
and with a synthetic vocabulary of V = 384 whose tokens cross bracket levels; apply and advance on hand-made stacks up to depth
32.  Then the real Worker on the L2/C128 golden model (ASCII list grammar, mini vocabulary) and the 0.1B synthetic model
(JSON_OBJECT_GRAMMAR, real vocabulary): greedy, sampled, seeded and n = 3 requests end "stop" with an accepted text, the same
prompts without the grammar do not, greedy rows equal a host replay without a tie, and a DFA row, a grammar row and a plain row
share steps and emit what each emits alone.

The models have random weights and would never close a string or a list of their own accord, so every worker request carries a
logit_bias towards the structural single-byte tokens; the bias is applied before the mask and the replay applies it too."""
import asyncio
import json
import os
import queue

import numpy as np
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.guided import JSON_OBJECT_GRAMMAR, compile_grammar, compile_regex, pack_stack, unpack_stack
from grammar_cases import CASES, synthetic_vocab
from test_decode_sampling_gpu import _model, _Sink
from test_grammar_cpu import HostPool, compiled, outcome_bits
from test_guided_gpu import VOCAB, _tokenizer
from util import replay_decode

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("vocab", ["real", "synthetic"])
def test_build_kernel_matches_host_form_in_every_word_of_both_bitmaps(vocab, tmp_path_factory):
    if vocab == "real":
        V_, table = 65536, _tokenizer("0.1B", tmp_path_factory).idx2token
        stops = [0, 261, 24281, V_ + 5]
    else:
        V_, table, stops = 384, synthetic_vocab(), [0, 258, 380]
        assert max(len(b) for b in table.values()) == 128 and all(t in table.values() for t in (b"}}", b"]}", b"}]}", b"[[[", b'{"a":[', b"[]", b"{}"))
    guides = [compiled(name, 32 if k % 2 else 5) for k, name in enumerate(sorted(CASES))]
    h = HostPool(guides, table, V_, stops).build()
    d = HostPool(guides, table, V_, stops, device="cuda").build()
    torch.cuda.synchronize()
    used = np.zeros(h.P, bool)
    for g, r0 in zip(guides, h.rows):
        used[r0:r0 + g.n_states] = True
    for name, got, want in (("allow", d.allow.cpu().numpy(), h.allow.numpy()), ("maybe", d.maybe.cpu().numpy(), h.maybe.numpy())):
        assert np.array_equal(got, want), (name, [n for n, g, r0 in zip(sorted(CASES), guides, h.rows)
                                                  if not np.array_equal(got[r0:r0 + g.n_states], want[r0:r0 + g.n_states])])
        assert (got[~used] == FILL).all() and (got[used] != FILL).any()
    # the meaning, on the JSON grammar: the start state takes exactly tokens that begin an object; inside a string (nearly) no
    # token depends on the stack, behind a complete value of a nested list (nearly) every live one does
    j = sorted(CASES).index("json")
    g = guides[j]
    allow, maybe = h.bits(h.allow, h.rows[j]), h.bits(h.maybe, h.rows[j])
    assert allow.any() and all(table[t][:1] == b"{" for t in np.nonzero(allow | maybe)[0].tolist())
    inside, behind = g.walk(0, (), b'{"ab')[0], g.walk(0, (), b'{"a":[[1')[0]
    counts = [(int(h.bits(h.allow, h.rows[j] + s).sum()), int(h.bits(h.maybe, h.rows[j] + s).sum())) for s in (inside, behind)]
    print(vocab, "allow / maybe bits inside a string and behind a nested value:", counts)
    assert counts[0][0] > 100 * counts[0][1] and counts[1][1] > counts[1][0]


def _json_setup(tmp_path_factory, device):
    table = _tokenizer("0.1B", tmp_path_factory).idx2token
    g = compiled("json")
    return g, table, HostPool([compiled("mixed"), g], table, 65536, [0, 261], device=device).build()


def _configs(g):
    """(state, stack) for 16 rows: the three kinds of state under the stacks the issue lists."""
    at = lambda text: g.walk(0, (), text)[0]
    start, string, value = 0, at(b'{"ab'), at(b'{"a":[1')
    deep = g.walk(0, (), b'{"a":[' + b"[" * 31)
    assert len(deep[1]) == 31 and g.walk(deep[0], deep[1], b"[") is not None and g.walk(deep[0], deep[1], b"[[") is None
    n = g.n_sites
    alt = tuple(1 + k % n for k in range(20))
    full = tuple(1 + (k * 3) % n for k in range(32))
    out = [(start, ()), (string, ()), (value, ())] + [(value, (c,)) for c in range(1, n + 1)] + [(string, (1,)), deep, (value, deep[1]),
           (value, full), (deep[0], full), (string, full), (value, alt), (start, alt), g.walk(0, (), b'{"a":[[{"b":[2')]
    return out[:16]


def test_apply_kernel_matches_host_form_bit_for_bit(tmp_path_factory):
    g, table, h = _json_setup(tmp_path_factory, "cpu")
    r0, V_ = h.rows[1], 65536
    configs = _configs(g)
    assert len(configs) == 16
    rng = np.random.default_rng(3)
    n_slots, n = 24, 20
    state = np.full(n_slots, -1, np.int32)
    stack = np.zeros((n_slots, 4), np.uint64)
    slot_of = rng.permutation(n_slots)[:n].astype(np.int32)
    for i, (st, sk) in enumerate(configs):
        state[slot_of[i]], stack[slot_of[i]] = r0 + st, pack_stack(sk)
    stack[slot_of[16]] = pack_stack((1, 2))                                        # row 16: a slot without a grammar (its stack is ignored)
    state[slot_of[17]] = h.P + 3                                                   # row 17: a state outside the pool
    slot_of[18], slot_of[19] = -1, n_slots                                         # rows 18, 19: slots outside the table
    lg = (rng.standard_normal((n, V_)) * 4).astype(np.float16)
    lg[rng.random((n, V_)) < 0.01] = -np.inf
    lg[rng.random((n, V_)) < 0.01] = np.nan
    lg = torch.from_numpy(lg)
    rows = torch.tensor(list(range(n)) + [-1, n], dtype=torch.int32)                # and rows outside the logits
    st_t, sk_t, sl_t = torch.from_numpy(state), torch.from_numpy(stack.view(np.int64)), torch.from_numpy(slot_of)
    want = lg.clone()
    ops.grammar_apply(want, rows, sl_t, st_t, sk_t, h.next, h.meta, h.allow, h.maybe, h.tok_off, h.tok_bytes)
    d = HostPool([compiled("mixed"), g], table, 65536, [0, 261], device="cuda")
    d.allow, d.maybe = h.allow.cuda(), h.maybe.cuda()                                # the bitmaps of the host form: apply alone is under test
    got = lg.cuda()
    ops.grammar_apply(got, rows.cuda(), sl_t.cuda(), st_t.cuda(), sk_t.cuda(), d.next, d.meta, d.allow, d.maybe, d.tok_off, d.tok_bytes)
    torch.cuda.synchronize()
    got, want, raw = got.cpu().numpy().view(np.uint16), want.numpy().view(np.uint16), lg.numpy().view(np.uint16)
    assert np.array_equal(got, want), [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert np.array_equal(got[16:], raw[16:]) and all(not np.array_equal(got[i], raw[i]) for i in range(16))
    for i in (2, 9, 11):                                                 # and the meaning, against the automaton itself
        bits = outcome_bits(g, table, V_, [0, 261], *configs[i])
        assert np.array_equal(got[i], np.where(bits, raw[i], 0xFC00)), i
    full = got[11] != 0xFC00                                                       # depth 32: every push is refused
    assert not any(table[t][:1] in (b"[", b"{") for t in np.nonzero(full)[0].tolist() if t in table and t not in (0, 261))


def test_advance_and_reset_kernels_match_host_form(tmp_path_factory):
    g, table, h = _json_setup(tmp_path_factory, "cpu")
    assert all(table[1 + b] == bytes([b]) for b in range(256))
    d = HostPool([compiled("mixed"), g], table, 65536, [0, 261], device="cuda").build()
    r0, V_ = h.rows[1], 65536
    configs = _configs(g)
    rng = np.random.default_rng(9)
    n_slots = n = 256
    pick = rng.integers(0, len(configs), n_slots)
    state = np.array([r0 + configs[k][0] for k in pick], np.int32)
    stack = np.stack([pack_stack(configs[k][1]) for k in pick])
    state[rng.random(n_slots) < 0.1] = -1
    slot_idx = rng.permutation(n_slots).astype(np.int32)
    rows = rng.permutation(n)[:200].astype(np.int32)
    ids = rng.integers(0, V_, n)
    for r in rows[::2].tolist():                                                   # half of the rows: a token the configuration allows
        st, sk = configs[pick[slot_idx[r]]]
        alive = [1 + b for b in range(256) if g.token_outcome(st, sk, bytes([b])) is not None]     # (the single bytes are ids 1..256)
        ids[r] = alive[int(rng.integers(len(alive)))]
    ids[rows[1]], ids[rows[3]], ids[rows[5]], ids[rows[7]], ids[rows[9]] = 0, V_ - 1, V_ + 3, -2, 261      # stop, undefined, outside
    slot_idx[rows[11]] = n_slots + 1
    args = [torch.from_numpy(x) for x in (rows, slot_idx, ids.astype(np.int32))]
    hs, hk = torch.from_numpy(state.copy()), torch.from_numpy(stack.view(np.int64).copy())
    ds, dk = hs.cuda(), hk.cuda()
    ops.grammar_advance(*args, h.tok_off, h.tok_bytes, h.next, h.meta, hs, hk)
    ops.grammar_advance(*[a.cuda() for a in args], d.tok_off, d.tok_bytes, d.next, d.meta, ds, dk)
    torch.cuda.synchronize()
    assert torch.equal(ds.cpu(), hs) and torch.equal(dk.cpu(), hk)
    moved = 0
    for r in rows.tolist():
        s = int(slot_idx[r])
        if not 0 <= s < n_slots or state[s] < 0:
            continue
        st, sk = configs[pick[s]]
        at = g.token_outcome(st, sk, table[int(ids[r])]) if int(ids[r]) in table else None
        want = (r0 + at[0], at[1]) if at is not None else (r0 + st, sk)              # a dying walk leaves state and stack
        assert (int(hs[s]), unpack_stack(hk[s].numpy().view(np.uint64))) == want, (r, st, sk, int(ids[r]))
        moved += at is not None
    assert 60 <= moved <= 200
    untouched = np.setdiff1d(np.arange(n_slots), slot_idx[rows][(slot_idx[rows] >= 0) & (slot_idx[rows] < n_slots)])
    assert np.array_equal(hs.numpy()[untouched], state[untouched])
    # reset, in stream order against a following apply: the row is masked as the start state under the empty stack masks it
    slots = torch.tensor([5, 7, -1, n_slots, 9], dtype=torch.int32)
    start = torch.tensor([r0, -1, r0, r0, h.rows[0]], dtype=torch.int32)
    ops.grammar_reset(slots, start, hs, hk)
    ops.grammar_reset(slots.cuda(), start.cuda(), ds, dk)
    lg = torch.from_numpy((rng.standard_normal((3, V_)) * 4).astype(np.float16))
    got = lg.cuda()
    sl = torch.tensor([5, 7, 9], dtype=torch.int32)
    ops.grammar_apply(got, torch.arange(3, dtype=torch.int32).cuda(), sl.cuda(), ds, dk, d.next, d.meta, d.allow, d.maybe, d.tok_off, d.tok_bytes)
    torch.cuda.synchronize()
    assert torch.equal(ds.cpu(), hs) and torch.equal(dk.cpu(), hk) and hs[5] == r0 and hs[7] == -1 and (hk[[5, 7, 9]] == 0).all()
    got, raw = got.cpu().numpy().view(np.uint16), lg.numpy().view(np.uint16)
    assert np.array_equal(got[0], np.where(outcome_bits(g, table, V_, [0, 261], 0, ()), raw[0], 0xFC00)) and np.array_equal(got[1], raw[1])
    assert not np.array_equal(got[2], raw[2])


# ------------------------------------------------------------------------------------------------------------ the worker
GRAMMAR = {"L2C128": CASES["ascii_list"][0], "0.1B": JSON_OBJECT_GRAMMAR}
# logit_bias per single-byte token.  The models' logits have a standard deviation of 1, so these decide the kind of token and the
# model's own logits decide among equals; the quote outranks what a string may contain, so strings close; penalties wear every
# biased token down, so lists and objects close.
# (not the digits of the mini vocabulary: their ids are among the worker's no-penalty ids, so nothing would end a run of them)
BIAS = {"L2C128": {b"[": 12.0, b",": 12.0, b"a": 12.0, b"b": 12.0, b"]": 10.0},
        "0.1B": {b'"': 20.0, b"[": 17.0, b"{": 14.0, b",": 12.0, b"1": 12.0, b"}": 13.0, b"]": 13.0}}
MAX_TOKENS = 320
Z = dict(frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0)
PEN = dict(frequency_penalty=0.6, presence_penalty=0.4, penalty_decay=0.996)


def _bias(model, tok):
    ids = {bytes(b): i for i, b in tok.idx2token.items()}
    return {ids[c]: v for c, v in BIAS[model].items()}


def _specs(model, V_):
    rng = np.random.default_rng(V_ + 7)
    P = lambda n: rng.integers(1, min(V_, 65000), n).tolist()
    return [(P(4), dict(temperature=0.0, top_p=0.0, top_k=0, **PEN)), (P(6), dict(temperature=0.0, top_p=0.0, top_k=0, **PEN)),
            (P(7), dict(temperature=1.0, top_p=0.9, top_k=0, **PEN)), (P(3), dict(temperature=1.2, top_p=1.0, top_k=0, seed=104, **PEN)),
            (P(5), dict(temperature=1.0, top_p=1.0, top_k=0, seed=7, n=3, **PEN))]


def _run(m, V_, tok, model, specs, guides, run_ahead, use_graph, batch_size=9):
    """One worker, every spec as a request (a spec with n: a group of n choices) under guides[k] (one guide: for all)."""
    from chirrup_amd.core_structure import ModelLoadConfig, Task
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V_, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=batch_size, model=m, tokenizer=tok, run_ahead=run_ahead)
    w._init_worker()
    assert w.use_graph
    w.use_graph = use_graph
    w.max_prefill_count = batch_size
    bias = _bias(model, tok)
    new = lambda p, **kw: Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(p), state=None,
                               stop_tokens=[0], return_logits=True, max_tokens=MAX_TOKENS, logit_bias=dict(bias), **kw)
    tasks, heads = [], []
    for k, (p, kw) in enumerate(specs):
        kw = dict(kw)
        n = kw.pop("n", 1)
        guide = guides[k] if isinstance(guides, (list, tuple)) else guides
        others = [new(p, guide=guide, choice_index=j, **kw) for j in range(1, n)]
        heads.append(new(p, guide=guide, siblings=others, **kw))
        tasks += [heads[-1]] + others
    torch.manual_seed(11)
    for t in heads:
        tq.put(t)
    for _ in range(8000):
        if not w.step():
            break
    assert all(t.output_queue.items[-1][0] == "task_completed" for t in tasks)
    return w, tasks, bias


class _Host:
    """A guide on the host for the replay: start, step(at, bytes) -> at | None, ends(at).  None: no guide."""

    def __init__(self, guide):
        self.g, self.grammar = guide, hasattr(guide, "site_start")
        self.start = (0, ()) if self.grammar else 0

    def step(self, at, data):
        if self.grammar:
            return self.g.token_outcome(at[0], at[1], data)
        s = self.g.walk(at, data)
        return s if s >= 0 and len(data) else None

    def ends(self, at):
        return self.g.ends(*at) if self.grammar else bool(self.g.accept[at])


def _replay_masked(guide, tok, V_, raw_steps, emitted, bias, stops=(0,)):
    """Each step's raw logits with the bias, then masked by the automaton itself (StackDFA.token_outcome for a grammar); the
    position follows the emitted ids.  Returns the masked logits and the last position."""
    table = tok.idx2token
    by_first = {}
    for t, b in table.items():
        if t < V_ and t not in stops and len(b):
            by_first.setdefault(b[0], []).append(t)
    h = _Host(guide) if guide is not None else None
    cache, at, out = {}, h.start if h else None, []
    ids, vals = np.array(list(bias), np.int64), np.array(list(bias.values()), np.float32)
    for raw, t in zip(raw_steps, emitted):
        lg = np.array(raw, np.float16).reshape(V_).copy()
        lv = lg[ids].astype(np.float32)
        fin = np.isfinite(lv)
        lg[ids[fin]] = np.clip(lv[fin] + vals[fin], np.float32(-65504), np.float32(65504)).astype(np.float16)
        if h is not None:
            if at not in cache:
                ok = np.zeros(V_, bool)
                for b, toks in by_first.items():
                    if h.step(at, bytes([b])) is not None:                          # (a token whose first byte dies is masked)
                        for x in toks:
                            ok[x] = h.step(at, table[x]) is not None
                for s in stops:
                    ok[s] = h.ends(at)
                cache[at] = ok
            assert cache[at].any(), at                                              # a guided row always has an allowed token
            lg.view(np.uint16)[~cache[at]] = 0xFC00
            if t not in stops:
                at = h.step(at, table[t])
                assert at is not None
        out.append(lg)
    return out, at


def _check_replay(guide, tok, V_, t, bias):
    """The greedy request t against its host replay: bias -> mask -> penalties -> arg-max gives the emitted ids.  Returns the steps
    replayed, how many of them were ties (the emitted id differs from the replay's, their penalised logits equal and the largest:
    the callers assert there are none) and the automaton's last position; any other difference fails here."""
    raw = [p[2].numpy() for k, p in t.output_queue.items if k == "token_generated"]
    masked, end = _replay_masked(guide, tok, V_, raw, t.generated_tokens, bias)
    want, pen = replay_decode(masked, t.generated_tokens, t.frequency_penalty, t.presence_penalty, t.penalty_decay)
    ties = 0
    for k, (a, b) in enumerate(zip(t.generated_tokens, want)):
        if a != b:
            ties += 1
            assert pen[k][a] == pen[k][b] == np.nanmax(pen[k]), (k, a, b)
    return len(want), ties, end


@pytest.mark.parametrize("mode", [(True, True), (False, False)], ids=["graph-run_ahead", "eager-in_step"])
@pytest.mark.parametrize("model", ["L2C128", "0.1B"])
def test_grammar_requests_on_the_gpu_stop_with_accepted_text_and_equal_the_host_replay(model, mode, tmp_path_factory):
    from chirrup_amd.core_structure import RequestStatus

    V_, tok, m = VOCAB[model], _tokenizer(model, tmp_path_factory), _model(model)
    g = compile_grammar(GRAMMAR[model])
    specs = _specs(model, V_)
    w, tasks, bias = _run(m, V_, tok, model, specs, g, *mode)
    replayed = ties = 0
    for t in tasks:
        text = tok.decodeBytes(t.generated_tokens)
        print(model, t.temperature, len(t.generated_tokens), text[:100])
        assert t.request_status == RequestStatus.FINISHED_STOPPED and t.error is None, (t.request_status, text)
        assert g.matches(text) and 0 < len(t.generated_tokens) < MAX_TOKENS, text
        if model == "0.1B":
            assert isinstance(json.loads(text.decode("utf-8")), dict), text
        if t.temperature == 0:
            n, k, end = _check_replay(g, tok, V_, t, bias)
            assert g.ends(*end)
            replayed, ties = replayed + n, ties + k
    print(f"{model}: {replayed} greedy steps replayed, {ties} ties")
    assert replayed >= 4                                                            # two greedy requests, at least "[]" / "{}" each
    assert ties == 0                                                                # (a tie would call for another prompt)
    assert all(e["refs"] == 0 for e in w._grammars.entries.values()) and w._grammars.builds == 1 and w._guides is None
    # the control: the same prompts, with the same bias, without the grammar are not accepted
    _, plain, _ = _run(m, V_, tok, model, specs, None, *mode)
    assert not any(g.matches(tok.decodeBytes([i for i in t.generated_tokens if i in tok.idx2token])) for t in plain)


@pytest.mark.parametrize("model", ["L2C128", "0.1B"])
def test_a_dfa_row_a_grammar_row_and_a_plain_row_share_steps_and_match_their_solo_runs(model, tmp_path_factory):
    """Three greedy requests of one prompt in the same steps, one under a grammar, one under a DFA guide, one without: each emits
    the ids it emits in a worker of its own (same batch size, so the same decode graph), and each equals the host replay of its
    own kind of mask, without a tie."""
    V_, tok, m = VOCAB[model], _tokenizer(model, tmp_path_factory), _model(model)
    kinds = [compile_grammar(GRAMMAR[model]), compile_regex(r"\[(a|b|1)(,(a|b|1)){0,3}\]"), None]
    prompt, kw = _specs(model, V_)[0]
    solo = [_run(m, V_, tok, model, [(prompt, kw)], kind, True, True, batch_size=5)[1][0].generated_tokens for kind in kinds]
    w, tasks, bias = _run(m, V_, tok, model, [(prompt, kw)] * 3, kinds, True, True, batch_size=5)
    for guide, t, alone in zip(kinds, tasks, solo):
        n, ties, end = _check_replay(guide, tok, V_, t, bias)
        text = tok.decodeBytes([i for i in t.generated_tokens if i in tok.idx2token])
        print(model, "grammar" if guide is kinds[0] else "dfa" if guide is kinds[1] else "plain", n, ties, text[:80])
        assert n == len(t.generated_tokens) > 0 and ties == 0
        assert guide is None or (guide.matches(text) and str(t.request_status) == "FINISHED_STOPPED"), text
        assert t.generated_tokens == alone, (text, tok.decodeBytes([i for i in alone if i in tok.idx2token]))
    assert not kinds[0].matches(tok.decodeBytes([i for i in tasks[2].generated_tokens if i in tok.idx2token]))
    assert w._guides.builds == w._grammars.builds == 1 and w._guided.count(True) <= 1 and w._grammared.count(True) <= 1
    assert [a and b for a, b in zip(w._guided, w._grammared)] == [False] * 5         # a slot is in at most one pool


def test_chat_route_with_a_grammar_on_the_gpu(tmp_path):
    import httpx

    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.engine_core import AsyncEngineCore
    from chirrup_amd.web_service import create_app

    d = np.load(os.path.join(G, "model_L2_C128.npz"))
    ckpt = os.path.join(tmp_path, "tiny.pth")
    torch.save({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}, ckpt)
    text = "root ::= \\[<v>(,<v>){0,2}\\]\nv ::= a|the|1|\\[<v>\\]\n"       # a finite language of short texts: the request ends by itself

    async def main():
        eng = AsyncEngineCore()
        cfg = ModelLoadConfig(model_path=ckpt, vocab_path=os.path.join(G, "mini_vocab.txt"), vocab_size=320, head_size=64)
        await eng.init(worker_num=1, model_config=cfg, batch_size=4)
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=create_app(eng, state_cache_size=0)), base_url="http://t") as cl:
            r = await cl.post("/v1/chat/completions", json={
                "model": "rwkv-latest:no-thinking", "messages": [{"role": "user", "content": "give me a list"}], "max_tokens": 400,
                "guided_grammar": text, "temperature": 1.0, "top_p": 0.9, "seed": 5})
        eng.shutdown()
        return r

    r = asyncio.run(main())
    assert r.status_code == 200, r.text
    ch = r.json()["choices"][0]
    assert ch["finish_reason"] == "stop" and compile_grammar(text).matches(ch["message"]["content"]), ch["message"]["content"]
