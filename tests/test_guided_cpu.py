"""Guided decoding without a GPU: the pattern compiler against Python's ``re`` (the subset defines ``\\d \\w \\s`` and their negations
over ASCII, so the patterns are compiled with ``re.ASCII``: the negated escapes, ``.`` and negated classes then accept every other
code point, as the byte automaton does), schema_to_regex against a validator of the subset, the CPU forms of ops.guide_build /
guide_apply / guide_advance on hand-made automata, the fake-backend worker (finish reasons, neighbours, slot reuse, parallel
choices, no call and no pool without a guided request, the guide cache, a pattern the vocabulary cannot spell), the engine and both
routes, and the C ABI's declarations and argument checks."""
import asyncio
import ctypes
import json
import os
import pickle
import queue
import re

import httpx
import numpy as np
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import GUIDE_MAX_STATES, ModelLoadConfig, RequestStatus, Task
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.guided import (ByteDFA, GuideError, compile_choice, compile_regex, escape_literal, schema_to_regex, token_table)
from chirrup_amd.tokenizer import TRIE_TOKENIZER
from chirrup_amd.web_service import create_app
from chirrup_amd.worker import GuidePool, Worker
from guided_cases import (ALL_PATTERNS, FAKE_VOCAB, PATTERNS, SCHEMAS, distance_to_accept, mutate, random_member, validate)
from test_engine_cpu import _Tok
from test_worker_cpu import V, FakeModel, FakeTok, Sink, cpu_penalize_argmax, expected_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# --------------------------------------------------------------------------------------------------- the compiler
def test_the_pattern_list_covers_the_subset():
    assert len(ALL_PATTERNS) >= 30 and len(SCHEMAS) >= 5
    assert sum(any(ord(c) > 127 for c in p) for p, _ in PATTERNS) >= 4               # non-ASCII literals
    assert GUIDE_MAX_STATES == 4096


@pytest.mark.parametrize("k", range(len(ALL_PATTERNS)))
def test_compiler_agrees_with_re_on_members_and_single_edit_mutations(k):
    pattern, states = ALL_PATTERNS[k]
    dfa = compile_regex(pattern)
    assert dfa.n_states == states < GUIDE_MAX_STATES, (pattern, dfa.n_states)
    assert dfa.next.dtype == np.int32 and dfa.next.shape == (states, 256) and dfa.accept.shape == (states,)
    assert dfa.next.min() >= -1 and dfa.next.max() < states
    assert (distance_to_accept(dfa) < 1 << 30).all()                                 # every state has a completion
    want = re.compile(pattern, re.ASCII)
    rng = np.random.default_rng(1000 + k)
    dist = distance_to_accept(dfa)
    members = 0
    for i in range(200):
        data = random_member(dfa, rng, dist, wander=int(rng.integers(0, 24)))
        text = data.decode("utf-8")                                                  # an accepted byte string is well-formed UTF-8
        members += 1
        assert dfa.matches(text) and want.fullmatch(text) is not None, (pattern, text)
        m = mutate(text, rng)
        assert dfa.matches(m) == (want.fullmatch(m) is not None), (pattern, text, m)
    assert members == 200


def test_equal_languages_share_a_key_and_the_dfa_pickles():
    a, b = compile_regex(r"(a|b)*abb"), compile_regex(r"(?:[ab])*a(b{2})")
    assert a.key == b.key and np.array_equal(a.next, b.next)
    assert a.key != compile_regex(r"(a|b)*ab").key
    c = pickle.loads(pickle.dumps(a))
    assert isinstance(c, ByteDFA) and c.key == a.key and np.array_equal(c.next, a.next) and np.array_equal(c.accept, a.accept)
    assert compile_regex("é").next[0, 0xC3] == 1 and compile_regex("é").n_states == 3       # a non-ASCII literal: its bytes


UNSUPPORTED = [r"a*?", r"a+?", r"a??", r"a{2}?", r"a*+", r"a++", r"(?=a)b", r"(?!a)b", r"(?<=a)b", r"(?<!a)b", r"^a", r"a$", r"a^b",
               r"\bword", r"\Bx", r"\Aa", r"a\Z", r"(a)\1", r"(?P<n>a)", r"(?P=n)", r"(?i)a", r"(?s:a)", r"(?#c)a", r"a{2", r"a{,3}",
               r"a{x}", r"a}", r"{2}", r"*a", r"a**", r"a{2}{3}", r"a{3,2}", r"[a", r"[z-a]", r"[\d-z]", r"(a", r"a)", r"\q", r"\x4",
               r"\0", "a\\", r"a{1001}", r"(?(1)a|b)"]


@pytest.mark.parametrize("pattern", UNSUPPORTED)
def test_constructs_outside_the_subset_raise_with_an_offset(pattern):
    with pytest.raises(GuideError, match=r"at offset \d+"):
        compile_regex(pattern)


def test_state_bound_and_empty_language():
    with pytest.raises(GuideError, match="GUIDE_MAX_STATES"):
        compile_regex(r"(a|b)*a(a|b){12}")                                            # 2^13 states, minimal
    with pytest.raises(GuideError, match="GUIDE_MAX_STATES"):
        compile_regex(r"[a-z]{1000}[0-9]{1000}[a-z]{1000}[0-9]{1000}x{100}")
    assert compile_regex(r"(a|b)*a(a|b){10}").n_states == 2048
    with pytest.raises(GuideError, match="matches nothing"):
        compile_regex("a[^\\x00-" + chr(0x10FFFF) + "]")
    with pytest.raises(GuideError):
        compile_regex(None)
    assert isinstance(GuideError("x"), ValueError)


def test_compile_choice_is_built_from_the_strings():
    nasty = ["a.b", "a|b", "(x)*", "[z]", "\\d", "^$", "{2}", "é+", "", "日本", "a.b"]
    dfa = compile_choice(nasty)
    for c in nasty:
        assert dfa.matches(c), c
    for c in ("axb", "a", "b", "x", "xx", "z", "5", "é", "éé", "{2", "日"):
        assert not dfa.matches(c), c
    assert dfa.key == compile_regex("|".join(escape_literal(c) for c in nasty)).key       # the same language, two routes
    assert compile_choice(["yes", "no"]).n_states == 5
    for bad in ([], "yes", [1, 2], None, ["ok", b"bytes"], ["\ud800"]):
        with pytest.raises(GuideError):
            compile_choice(bad)


# --------------------------------------------------------------------------------------------------- schemas
@pytest.mark.parametrize("k", range(len(SCHEMAS)))
def test_schema_members_parse_and_satisfy_the_schema(k):
    schema, _ = SCHEMAS[k]
    dfa = compile_regex(schema_to_regex(schema))
    rng = np.random.default_rng(k)
    dist = distance_to_accept(dfa)
    for _ in range(150):
        text = random_member(dfa, rng, dist, wander=int(rng.integers(0, 60))).decode("utf-8")
        value = json.loads(text)
        assert validate(schema, value), (schema, text)
        assert not re.search(r"[\x00-\x1f]", text)                                   # compact, no raw control bytes
    ok = {0: ['"a\\n\\u00e9 é"', '""'], 1: ["0", "-7", "123456789012345678"], 2: ["-0.5e+10", "3", "1E3"],
          7: ['{"name":"x","age":-1,"ok":true}'], 8: ["[1]", "[1,2,3]"], 9: ["[]", '["a","b","a"]'], 13: ["{}"]}
    no = {0: ['"a\nb"', '"\\x"', "'a'", '"a'], 1: ["01", "1234567890123456789", "+1", "1.0", "-"], 2: ["1.", ".5", "1e", "0x1"],
          7: ['{"age":1,"name":"x","ok":true}', '{"name":"x","age":1}', '{"name": "x","age":1,"ok":true}'], 8: ["[]", "[1,2,3,4]", "[1,]"],
          9: ['["c"]'], 13: ["{ }"]}
    for t in ok.get(k, []):
        assert dfa.matches(t) and validate(schema, json.loads(t)), t
    for t in no.get(k, []):
        assert not dfa.matches(t), t


@pytest.mark.parametrize("schema", [{"$ref": "#/x"}, {"type": "string", "pattern": "a+"}, {"type": "string", "format": "date"},
                                    {"type": "object", "properties": {}, "additionalProperties": True}, {"oneOf": [{"type": "null"}]},
                                    {"allOf": [{"type": "null"}]}, {"type": "array"}, {"type": "string", "minLength": 2},
                                    {"type": "integer", "minimum": 0}, {"enum": [[1]]}, {"const": {"a": 1}}, {"type": "tuple"}, {},
                                    {"type": "array", "items": {"type": "null"}, "minItems": 3, "maxItems": 2}, "string", {"enum": []},
                                    {"type": "object", "properties": {"a": {"type": "null"}}, "required": ["b"]}])
def test_schema_features_outside_the_subset_raise(schema):
    with pytest.raises(GuideError):
        schema_to_regex(schema)


def test_recursive_schema_raises():
    s = {"type": "array"}
    s["items"] = s
    with pytest.raises(GuideError, match="recursion"):
        schema_to_regex(s)


# --------------------------------------------------------------------------------------------------- host forms of the ops
def _pool(dfas, P, V_, vocab, stops=(0,)):
    """A CPU guide pool holding `dfas` one behind the other; returns (next, allow, tok_off, tok_bytes, start rows)."""
    off, data = token_table(vocab, V_)
    nxt = torch.full((P, 256), -1, dtype=torch.int32)
    allow = torch.zeros((P, V_ // 32), dtype=torch.int32)
    tok_off, tok_bytes = torch.from_numpy(off), torch.from_numpy(data)
    rows, at = [], 3                                                               # (not at row 0: entries are absolute)
    for d in dfas:
        S = d.n_states
        nxt[at:at + S] = torch.from_numpy(np.where(d.next >= 0, d.next + at, -1).astype(np.int32))
        ops.guide_build(S, at, nxt, tok_off, tok_bytes, torch.tensor(stops, dtype=torch.int32),
                        torch.from_numpy(d.accept.astype(np.uint8)), allow)
        rows.append(at)
        at += S + 2
    return nxt, allow, tok_off, tok_bytes, rows


def _bits(allow, row, V_):
    return np.unpackbits(allow[row].numpy().view(np.uint8), bitorder="little")[:V_].astype(bool)


def test_guide_build_host_form():
    d1, d2 = compile_regex(r"(yes|no)"), compile_regex(r"ab*c?")
    nxt, allow, tok_off, tok_bytes, (r1, r2) = _pool([d1, d2], 40, V, FAKE_VOCAB, stops=(0, 46, 99, -4))
    # an independent walk per (state, token)
    for d, r0 in ((d1, r1), (d2, r2)):
        for s in range(d.n_states):
            bits = _bits(allow, r0 + s, V)
            for t in range(V):
                if t in (0, 46):                                                   # special ids follow accept, bytes never walked
                    want = bool(d.accept[s])
                elif t not in FAKE_VOCAB:                                          # undefined ids are never allowed
                    want = False
                else:
                    want = d.walk(s, FAKE_VOCAB[t]) >= 0
                assert bits[t] == want, (d.pattern, s, t)
    start = _bits(allow, r1, V)
    assert sorted(np.nonzero(start)[0]) == [24, 35, 45]                            # n, y, yes -- "no" (46) is a stop id here
    assert not _bits(allow, r2, V)[[60, 61]].any()
    assert (allow[:3] == 0).all() and (allow[r1 + d1.n_states:r2] == 0).all()      # rows outside the guides are untouched
    assert (nxt[r1:r1 + d1.n_states][nxt[r1:r1 + d1.n_states] >= 0] >= r1).all()
    with pytest.raises(ops._lib.ChirrupAmdError):
        ops.guide_build(5, 38, nxt, tok_off, tok_bytes, torch.zeros(0, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8), allow)


def test_guide_apply_host_form():
    d = compile_regex(r"(yes|no)")
    nxt, allow, tok_off, tok_bytes, (r0,) = _pool([d], 16, V, FAKE_VOCAB)
    rng = np.random.default_rng(0)
    lg = torch.from_numpy(rng.standard_normal((4, V)).astype(np.float16))
    lg[0, 24], lg[0, 5], lg[2, 35], lg[2, 7] = float("-inf"), float("nan"), float("nan"), float("-inf")
    raw = lg.clone()
    state = torch.tensor([-1, r0, r0 + int(d.next[0, ord("y")]), -1, r0], dtype=torch.int32)
    slot_idx = torch.tensor([4, 0, 2, 1], dtype=torch.int32)                        # rows 0 and 2 are guided, 1 is not, 3 not listed
    ops.guide_apply(lg, torch.tensor([0, 1, 2], dtype=torch.int32), slot_idx, state, allow)
    u = lambda t: t.numpy().view(np.uint16)
    assert np.array_equal(u(lg[1]), u(raw[1])) and np.array_equal(u(lg[3]), u(raw[3]))      # unguided / unlisted rows untouched
    keep0 = _bits(allow, r0, V)
    assert np.array_equal(u(lg[0])[keep0], u(raw[0])[keep0]) and (u(lg[0])[~keep0] == 0xFC00).all()
    assert lg[0, 24].item() == float("-inf") and lg[0, 5].item() == float("-inf")  # -inf stays, a masked NaN becomes -inf
    keep2 = _bits(allow, int(state[2]), V)
    assert sorted(np.nonzero(keep2)[0]) == [15] and lg[2, 35].item() == float("-inf") and (u(lg[2])[~keep2] == 0xFC00).all()
    assert u(lg[2])[15] == u(raw[2])[15]
    ops.guide_apply(lg, torch.zeros(0, dtype=torch.int32), slot_idx, state, allow)
    ops.guide_apply(raw, torch.tensor([1], dtype=torch.int32), None, state, allow)   # without slot_idx: row 1 -> slot 1
    assert (u(raw[1])[~keep0] == 0xFC00).all()


def test_guide_advance_host_form():
    d = compile_regex(r"(yes|no)")
    nxt, allow, tok_off, tok_bytes, (r0,) = _pool([d], 16, V, FAKE_VOCAB)
    y = r0 + int(d.next[0, ord("y")])
    state = torch.tensor([r0, r0, r0, r0, -1, y, r0], dtype=torch.int32)
    slot_idx = torch.tensor([0, 1, 2, 3, 4, 5, 6], dtype=torch.int32)
    ids = torch.tensor([35, 45, 11, 60, 35, 0, 99], dtype=torch.int32)              # y, yes, a (dies), undefined, -, stop, out of range
    ops.guide_advance(torch.tensor([0, 1, 2, 3, 4, 5, 6], dtype=torch.int32), slot_idx, ids, tok_off, tok_bytes, nxt, state)
    assert state.tolist() == [y, r0 + d.walk(0, b"yes"), r0, r0, -1, y, r0]
    assert d.accept[d.walk(0, b"yes")]
    before = state.clone()
    ops.guide_advance(torch.tensor([1], dtype=torch.int32), torch.tensor([3, 0], dtype=torch.int32),
                      torch.tensor([0, 15], dtype=torch.int32), tok_off, tok_bytes, nxt, state)     # row 1 -> slot 0, id 'e'
    assert state[0].item() == r0 + d.walk(0, b"ye") and torch.equal(state[1:], before[1:])


# --------------------------------------------------------------------------------------------------- the fake-backend worker
class GuideTok(_Tok):
    idx2token = FAKE_VOCAB

    def decode(self, ids, utf8_errors="strict"):
        return b"".join(FAKE_VOCAB[i] for i in ids).decode("utf-8", errors=utf8_errors)


def _text(task) -> str:
    return b"".join(FAKE_VOCAB[t] for t in task.generated_tokens).decode("utf-8")


def _worker(run_ahead, batch_size=6, **kw):
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [], cfg, tq, queue.Queue(), queue.Queue(), batch_size=batch_size, model=FakeModel(), tokenizer=GuideTok(),
               penalize_argmax=cpu_penalize_argmax, run_ahead=run_ahead, **kw)
    w._init_worker()
    return w, tq


def _new(prompt, **kw):
    for k, v in (("temperature", 0.0), ("top_p", 0.0), ("frequency_penalty", 0.0), ("presence_penalty", 0.0), ("penalty_decay", 1.0),
                 ("stop_tokens", [0]), ("max_tokens", 40)):
        kw.setdefault(k, v)
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **kw)


def _drain(w):
    for _ in range(4000):
        if not w.step():
            return
    raise AssertionError("worker did not drain")


BOUNDED = [r"(yes|no)", r"[ab]{3}c", r"\d{3}-\d{2}", r"true|false|null", r"\"[a-c]{1,4}\"", r"é中", r"\{\"k\":(12|ab)\}"]
SAMPLED = dict(temperature=1.0, top_p=1.0)


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_guided_requests_end_stop_and_their_text_matches(run_ahead):
    torch.manual_seed(3)
    w, tq = _worker(run_ahead, batch_size=9)
    ts = []
    for k, p in enumerate(BOUNDED):
        g = compile_regex(p)
        ts += [(p, _new([3 + k, 1], guide=g)), (p, _new([5, k], guide=g, **SAMPLED)), (p, _new([k, 9, 2], guide=g, seed=k, **SAMPLED)),
               (p, _new([k + 1], guide=g, frequency_penalty=0.5, presence_penalty=0.5, penalty_decay=0.99, **SAMPLED))]
    for _, t in ts:
        tq.put(t)
    _drain(w)
    texts = set()
    for p, t in ts:
        assert t.request_status == RequestStatus.FINISHED_STOPPED and t.error is None, (p, t.request_status)
        assert re.fullmatch(p, _text(t)) is not None, (p, _text(t))
        assert t.output_queue.items[-1][0] == "task_completed" and 0 not in t.generated_tokens
        texts.add(_text(t))
    assert len(texts) > len(BOUNDED)                                               # the sampled rows really vary
    cut = _new([1, 2], guide=compile_regex(r"[ab]{30}"), max_tokens=7)              # max_tokens may cut a guided text short
    tq.put(cut)
    _drain(w)
    assert cut.request_status == RequestStatus.FINISHED_LENGTH_CAPPED and re.fullmatch(r"[ab]+", _text(cut)) and len(cut.generated_tokens) == 7
    assert w._guides.builds == len(BOUNDED) + 1 and all(e["refs"] == 0 for e in w._guides.entries.values())


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_unguided_neighbour_and_the_slots_next_request_are_unconstrained(run_ahead):
    w, tq = _worker(run_ahead, batch_size=3)                                        # two decode slots
    plain, guided = _new([5, 9], stop_tokens=[], max_tokens=12), _new([5, 9], guide=compile_regex(r"[ab]{3}c"))
    after = _new([7, 7], stop_tokens=[], max_tokens=12)                             # takes the guided request's slot when it ends
    for t in (plain, guided, after):
        tq.put(t)
    _drain(w)
    assert plain.generated_tokens == expected_stream([5, 9], 12)                   # what it emits without any neighbour
    assert after.generated_tokens == expected_stream([7, 7], 12)
    assert re.fullmatch(r"[ab]{3}c", _text(guided)) and guided.request_status == RequestStatus.FINISHED_STOPPED
    assert w._guided == [False, False, False] and w._guides.state.tolist() == [-1, -1, -1]
    assert not re.fullmatch(r"[ab]{3}c", "".join(FAKE_VOCAB.get(t, b"?").decode("utf-8", "replace") for t in plain.generated_tokens))


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_three_parallel_choices_each_match(run_ahead):
    w, tq = _worker(run_ahead)
    g = compile_regex(r"\d{3}-\d{2}")
    kw = dict(guide=g, seed=11, **SAMPLED)
    others = [_new([4, 2, 6], choice_index=j, **kw) for j in (1, 2)]
    first = _new([4, 2, 6], siblings=others, **kw)
    tq.put(first)
    _drain(w)
    texts = [_text(t) for t in [first] + others]
    for t, text in zip([first] + others, texts):
        assert t.request_status == RequestStatus.FINISHED_STOPPED and re.fullmatch(r"\d{3}-\d{2}", text), text
    assert len(set(texts)) > 1                                                      # each choice draws from its own stream
    assert w._guides.builds == 1 and [e["refs"] for e in w._guides.entries.values()] == [0]


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_without_a_guided_request_no_op_is_called_and_no_pool_exists(run_ahead, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("guide op called in a step where no row is guided")

    for name in ("guide_build", "guide_apply", "guide_advance"):
        monkeypatch.setattr(ops, name, boom)
    w, tq = _worker(run_ahead)
    ts = [_new([1, 2, 3], stop_tokens=[], max_tokens=12), _new([4], stop_tokens=[], max_tokens=12, **SAMPLED)]
    for t in ts:
        tq.put(t)
    _drain(w)
    assert all(len(t.generated_tokens) == 12 for t in ts) and w._guides is None and w._guided == [False] * 6
    tq.put(_new([1], guide=compile_regex("a")))
    with pytest.raises(AssertionError, match="no row is guided"):
        _drain(w)


def test_guide_cache_refcounts_and_evicts_least_recently_used():
    pool = GuidePool(32, 4, V, torch.device("cpu"), FAKE_VOCAB)
    a, b, c, d = (compile_regex(p) for p in (r"\d{3}-\d{4}", r"[ab]{19}", r"[a-c]{8}", r"[b-d]{9}"))
    assert [x.n_states for x in (a, b, c, d)] == [9, 20, 9, 10]
    ka, ra = pool.acquire(a, [0])
    assert (ra, pool.acquire(a, [0]), pool.builds) == (0, (ka, 0), 1) and pool.entries[ka]["refs"] == 2
    ka2, ra2 = pool.acquire(a, [0, 5])                                             # other stop tokens: other bitmaps, another entry
    assert ka2 != ka and ra2 == 9 and pool.builds == 2
    for k in (ka, ka, ka2):
        pool.release(k)
    kb, rb = pool.acquire(b, [0])                                                  # 18 rows used, 14 free: both idle guides must go
    assert rb == 0 and list(pool.entries) == [kb] and pool.builds == 3
    kc, rc = pool.acquire(c, [0])
    assert rc == 20 and pool.builds == 4
    with pytest.raises(GuideError, match="no room"):                               # 3 rows free, nothing idle
        pool.acquire(d, [0])
    pool.release(kc)
    with pytest.raises(GuideError, match="no room"):                               # dropping c frees 12 rows at the end: 13 do not fit
        pool.acquire(compile_regex(r"[ab]{12}"), [0])
    assert list(pool.entries) == [kb]                                              # (c was dropped in the attempt)
    kd, rd = pool.acquire(d, [0])
    assert rd == 20
    pool.release(kb)
    ka3, ra3 = pool.acquire(a, [0])                                                # first fit: b (idle, least recently used) makes room
    assert ra3 == 0 and set(pool.entries) == {kd, ka3}
    want = np.where(a.next >= 0, a.next, -1)
    assert np.array_equal(pool.next[:9].numpy(), want) and (pool.next[30:] == -1).all()


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_a_guide_that_cannot_be_placed_fails_its_request_only(run_ahead):
    w, tq = _worker(run_ahead, guide_pool_rows=12)
    big, small, plain = _new([1], guide=compile_regex(r"[ab]{19}")), _new([2], guide=compile_regex(r"(yes|no)")), _new([3], stop_tokens=[], max_tokens=5)
    for t in (big, small, plain):
        tq.put(t)
    _drain(w)
    assert big.request_status == RequestStatus.FINISHED_ABORTED and "no room" in big.error and big.generated_tokens == []
    assert [k for k, _ in big.output_queue.items] == ["error", "task_completed"]
    assert small.request_status == RequestStatus.FINISHED_STOPPED and _text(small) in ("yes", "no") and small.error is None
    assert plain.generated_tokens == expected_stream([3], 5)


class _MiniModel(FakeModel):
    def forward_slots(self, tokens, pool, slot_idx, full_output=False):
        small = super().forward_slots(tokens, pool, slot_idx)
        out = torch.zeros((small.shape[0], 320), dtype=torch.float16)
        out[:, :V] = small
        return out


def test_a_pattern_the_mini_vocabulary_cannot_realise_is_refused():
    tok = TRIE_TOKENIZER(os.path.join(G, "mini_vocab.txt"))
    single = {b[0] for b in tok.idx2token.values() if len(b) == 1}
    assert len(single) == 139
    missing = next(bytes([b]) for b in range(0x80, 0xC0) if b not in single)        # a continuation byte that is no token
    ch = next(c for c in map(chr, range(0xA0, 0x800)) if c.encode()[1:] == missing
              and not any(len(t) > 1 and t.startswith(c.encode()[:1]) for t in tok.idx2token.values()))
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=320, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [], cfg, tq, queue.Queue(), queue.Queue(), batch_size=4, model=_MiniModel(), tokenizer=tok,
               penalize_argmax=cpu_penalize_argmax)
    w._init_worker()
    bad, good = _new([1], guide=compile_regex("x" + ch)), _new([1], guide=compile_regex(r"ab|cd"))
    tq.put(bad)
    tq.put(good)
    _drain(w)
    assert bad.request_status == RequestStatus.FINISHED_ABORTED and "vocabulary cannot realise" in bad.error
    assert good.request_status == RequestStatus.FINISHED_STOPPED and tok.decode(good.generated_tokens) in ("ab", "cd")
    assert len(w._guides.entries) == 1


def test_task_validation():
    g = compile_regex("a")
    for bad in (dict(guide=g, stop_tokens=[]), dict(guide=g, stop_tokens=None), dict(guide="a+"), dict(guide=g, max_tokens=0, prompt_logprobs=1),
                dict(guide=g, prompt_logprobs=2)):
        with pytest.raises(ValueError):
            _new([1, 2], **bad)
    assert _new([1], guide=g).guide is g and _new([1]).guide is None
    from chirrup_amd.engine_process import _RESULT_FIELDS, _TASK_FIELDS, task_to_wire

    assert "guide" in _TASK_FIELDS and "error" in _RESULT_FIELDS
    wire = pickle.loads(pickle.dumps(task_to_wire(_new([1], guide=g))))
    assert wire["guide"].key == g.key


# --------------------------------------------------------------------------------------------------- engine and routes
def _factory(**kw):
    return Worker(model=FakeModel(), tokenizer=GuideTok(), penalize_argmax=cpu_penalize_argmax, **kw)


async def _engine():
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=GuideTok())
    await eng.init(worker_num=1, model_config=ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64), batch_size=6)
    return eng


GREEDY = dict(temperature=0.0, top_p=0.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_decay=1.0)
SCHEMA = {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "integer"}, "t": {"enum": ["ab", "ba"]}}}


def test_engine_compiles_on_the_callers_side():
    async def main():
        eng = await _engine()
        with pytest.raises(GuideError, match="offset"):
            eng.completion("x", prefill_tokens=[1], guided_regex="a*?")
        with pytest.raises(GuideError, match="at most one"):
            eng.completion("x", prefill_tokens=[1], guided_regex="a", guided_choice=["a"])
        with pytest.raises(GuideError):
            eng.completion("x", prefill_tokens=[1], guided_json={"$ref": "#"})
        with pytest.raises(ValueError, match="stop tokens"):
            eng.completion("x", prefill_tokens=[1], guided_regex="a", stop_tokens=[])
        assert eng.task_queue.empty()
        c1 = eng.completion("x", prefill_tokens=[1, 2], guided_regex=r"[ab]{3}c", stop_tokens=[0], max_tokens=20, **GREEDY)
        c2 = eng.completion("x", prefill_tokens=[1, 2], guided_regex=r"[ab]{3}c", stop_tokens=[0], max_tokens=20, **GREEDY)
        assert c1.task.guide is c2.task.guide and list(eng._guide_cache) == [("regex", "a"), ("regex", r"[ab]{3}c")]      # the small LRU keyed by the source
        assert re.fullmatch(r"[ab]{3}c", await c1.get_full_completion()) and c1.task.request_status == RequestStatus.FINISHED_STOPPED
        c3 = eng.completion("x", prefill_tokens=[3], guided_choice=["yes", "no"], stop_tokens=[0], max_tokens=20, **GREEDY)
        assert await c3.get_full_completion() in ("yes", "no")
        c4 = eng.completion("x", prefill_tokens=[3], guided_json=SCHEMA, stop_tokens=[0], max_tokens=60, **GREEDY)
        assert validate(SCHEMA, json.loads(await c4.get_full_completion()))
        cs = eng.completions("x", prefill_tokens=[5, 6], n=3, guided_regex=r"\d{3}-\d{2}", stop_tokens=[0], max_tokens=20, seed=4,
                             temperature=1.0, top_p=1.0)
        texts = await asyncio.gather(*[c.get_full_completion() for c in cs])
        assert all(re.fullmatch(r"\d{3}-\d{2}", t) for t in texts)
        eng.shutdown()

    asyncio.run(main())


def test_routes_accept_each_field_and_answer_400_for_each_refusal():
    async def main():
        eng = await _engine()
        app = create_app(eng, state_cache_size=0)
        msgs = [{"role": "user", "content": "answer"}]
        chat = dict(model="rwkv-latest:no-thinking", messages=msgs, max_tokens=60, **GREEDY)
        legacy = dict(prompt="answer", max_tokens=60, **GREEDY)
        rf = {"type": "json_schema", "json_schema": {"name": "x", "schema": SCHEMA}}
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
            async def content(route, body):
                r = await cl.post(route, json=body)
                assert r.status_code == 200, r.text
                ch = r.json()["choices"][0]
                assert ch["finish_reason"] == "stop"
                return ch["message"]["content"] if "message" in ch else ch["text"]

            for route, base in (("/v1/chat/completions", chat), ("/v1/completions", legacy)):
                assert re.fullmatch(r"[ab]{3}c", await content(route, dict(base, guided_regex=r"[ab]{3}c")))
                assert await content(route, dict(base, guided_choice=["yes", "no"])) in ("yes", "no")
                assert validate(SCHEMA, json.loads(await content(route, dict(base, response_format=rf))))
                plain = await content(route, dict(base, max_tokens=6))
                assert await content(route, dict(base, max_tokens=6, response_format={"type": "text"})) == plain
                for bad, word in ((dict(guided_regex="a*?"), "lazy"), (dict(guided_regex="(?=a)"), "look-ahead"),
                                  (dict(guided_choice=[]), "non-empty"), (dict(response_format={"type": "json_object"}), "regular language"),
                                  (dict(response_format={"type": "json_schema", "json_schema": {"schema": {"$ref": "#"}}}), "$ref"),
                                  (dict(response_format={"type": "json_schema"}), "response_format"), (dict(response_format={"type": "xml"}), "response_format"),
                                  (dict(guided_regex="a", guided_choice=["a"]), "at most one"), (dict(guided_regex="a", response_format=rf), "at most one"),
                                  (dict(guided_choice=["a"], response_format=rf), "at most one")):
                    r = await cl.post(route, json=dict(base, **bad))
                    assert r.status_code == 400 and word in r.json()["detail"], (route, bad, r.status_code, r.text)
            r = await cl.post("/v1/chat/completions", json=dict(chat, model="rwkv-latest:thinking", guided_regex="a"))
            assert r.status_code == 400 and "thinking" in r.json()["detail"]
            # streaming is unchanged: the guided text arrives as content deltas
            r = await cl.post("/v1/chat/completions", json=dict(chat, stream=True, guided_choice=["yes", "no"]))
            chunks = [json.loads(ln[6:]) for ln in r.text.split("\n\n") if ln.startswith("data: ") and ln != "data: [DONE]"]
            assert "".join(c["choices"][0]["delta"].get("content", "") for c in chunks) in ("yes", "no")
            # a request without the new fields: the body the fake backend's stream pins (as test_web_service_cpu.py computes it)
            from chirrup_amd.web_service import ChatMessage, chat_prompt

            toks = [0] + GuideTok().encode(chat_prompt([ChatMessage(**m) for m in msgs], chat["model"])[0])
            r = await cl.post("/v1/chat/completions", json=dict(chat, max_tokens=6))
            j = r.json()
            want = "".join(FAKE_VOCAB.get(t, b"").decode("utf-8", "ignore") for t in expected_stream(toks, 6, stop=(0,)))
            assert list(j) == ["id", "object", "created", "model", "choices", "usage"] and list(j["choices"][0]) == ["index", "finish_reason", "message"]
            assert j["choices"][0]["message"] == {"role": "assistant", "content": want.split("\n\n")[0], "reasoning_content": ""}
        eng.shutdown()

    asyncio.run(main())


# --------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_exports_and_checks_arguments():
    import chirrup_amd
    from chirrup_amd import lib

    hdr = open(os.path.join(ROOT, "include", "chirrup_amd.h")).read()
    assert re.search(r"int rwkv7_guide_build\(int S, int row0, int P, int V, const int32_t \*guide_next, const int32_t \*tok_off", hdr)
    assert re.search(r"int rwkv7_guide_apply\(int n_rows, int n_logit_rows, int V, int P, void \*logits, const int32_t \*rows", hdr)
    assert re.search(r"int rwkv7_guide_advance\(int n_rows, int n_ids, int V, int P, const int32_t \*rows, const int32_t \*slot_idx", hdr)
    assert [len(lib.SIGNATURES[n][1]) for n in ("rwkv7_guide_build", "rwkv7_guide_apply", "rwkv7_guide_advance")] == [12, 11, 13]
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    L = chirrup_amd.load()
    gb, ga, gv = L.rwkv7_guide_build, L.rwkv7_guide_apply, L.rwkv7_guide_advance
    p = ctypes.c_void_p(4096)                                  # never dereferenced: validation fails first (or there is nothing to do)
    ok_b = [4, 0, 16, 64, p, p, p, 1, p, p, p, None]
    assert gb(*[0] + ok_b[1:]) == 0                            # S == 0: nothing launched
    for k, v in ((0, -1), (1, -1), (1, 13), (2, 0), (3, 0), (3, 96), (7, -1), (0, 65536)):
        args = list(ok_b)
        args[k] = v
        if (k, v) == (0, 65536):
            args[2] = 1 << 20
        assert gb(*args) == -1, (k, v)
    for k in (4, 5, 6, 8, 9, 10):
        args = list(ok_b)
        args[k] = None
        assert gb(*args) == -2, k
    assert gb(4, 0, 16, 64, p, p, p, 0, None, p, ctypes.c_void_p(4100), None) == -3      # guide_allow: 8-byte aligned
    ok_a = [2, 4, 64, 16, p, p, None, 8, p, p, None]
    assert ga(*[0] + ok_a[1:]) == 0
    for k, v in ((0, -1), (1, -1), (2, 0), (2, 48), (3, 0), (7, 0)):
        args = list(ok_a)
        args[k] = v
        assert ga(*args) == -1, (k, v)
    for k in (4, 5, 8, 9):
        args = list(ok_a)
        args[k] = None
        assert ga(*args) == -2, k
    assert ga(*ok_a[:4] + [ctypes.c_void_p(4104)] + ok_a[5:]) == -3                       # logits: 16-byte aligned
    ok_v = [2, 4, 64, 16, p, None, 8, p, p, p, p, p, None]
    assert gv(*[0] + ok_v[1:]) == 0
    for k, v in ((0, -1), (1, -1), (2, 0), (3, 0), (6, 0)):
        args = list(ok_v)
        args[k] = v
        assert gv(*args) == -1, (k, v)
    for k in (4, 7, 8, 9, 10, 11):
        args = list(ok_v)
        args[k] = None
        assert gv(*args) == -2, k
