"""Grammar-guided decoding without a GPU: compile_grammar against the independent recognisers of grammar_cases.py (members, single
byte edits, the depth cut, no dead ends under it, every GuideError), the StackDFA's key and pickling, the CPU forms of the four
ops.grammar_* against StackDFA.walk, the fake-backend worker and engine, both routes, and the C ABI's argument checks."""
import asyncio
import ctypes
import json
import os
import pickle
import re

import httpx
import numpy as np
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import GUIDE_CALL_SITES_MAX, GUIDE_MAX_STATES, GUIDE_STACK_DEPTH_MAX, ModelLoadConfig, RequestStatus
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.guided import GuideError, StackDFA, compile_grammar, compile_regex, pack_stack, token_table, unpack_stack
from chirrup_amd.web_service import create_app
from chirrup_amd.worker import GrammarPool, Worker
from grammar_cases import CASES, SINGLE_RULE, edit, json_loads_dict, member, synthetic_vocab
from guided_cases import FAKE_VOCAB
from test_guided_cpu import GREEDY, SAMPLED, GuideTok, _drain, _new, _text, _worker
from test_worker_cpu import V, FakeModel, cpu_penalize_argmax, expected_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMPILED = {}


def compiled(name: str, max_depth: int = 32) -> StackDFA:
    if (name, max_depth) not in _COMPILED:
        _COMPILED[name, max_depth] = compile_grammar(CASES[name][0], max_depth)
    return _COMPILED[name, max_depth]


# --------------------------------------------------------------------------------------------------- the compiler
def test_constants_and_the_shipped_grammar():
    assert (GUIDE_STACK_DEPTH_MAX, GUIDE_CALL_SITES_MAX, ops.GRAMMAR_STACK_DEPTH) == (32, 255, 32) and len(CASES) >= 6
    g = compiled("json")
    assert g.n_states <= GUIDE_MAX_STATES and 1 <= g.n_sites <= 8 and g.next.shape == (g.n_states, 256) and g.max_depth == 32
    assert len(set(g.site_start[1:].tolist())) == 1                                 # one recursive rule: `value`
    for text in ('{}', '{"a":1}', '{"a":[1,2,{"b":null}],"c":{"d":[[],[{}]]}}', '{"é":"\\u00e9\\n","n":-1.5e+3}'):
        assert g.matches(text) and json_loads_dict(text.encode()), text
    for text in ('', '[]', '[1]', '1', '{"a":}', '{"a":1,}', '{"a":[1,]}', '{"a":1} ', '{ }', '{"a":01}', '{"a":NaN}', '{a:1}', '{"a":[}'):
        assert not g.matches(text), text


@pytest.mark.parametrize("name", sorted(CASES))
def test_members_are_accepted_and_single_byte_edits_are_judged_as_the_recogniser_judges(name):
    text, _, recognise, structural = CASES[name]
    g = compiled(name)
    rng = np.random.default_rng(sorted(CASES).index(name))
    judged = accepted_edits = 0
    for _ in range(200):
        m = member(name, rng)
        assert recognise(m) and g.matches(m), (name, m)
        if name == "json":
            assert json_loads_dict(m), m
        e = edit(m, rng, structural)
        want = recognise(e)                                                         # total: every edit is judged
        judged += 1
        accepted_edits += want
        if want and name == "json":
            assert json_loads_dict(e), e
        assert g.matches(e) == want, (name, m, e, want)
    assert judged == 200 and 0 < accepted_edits < 200, (name, accepted_edits)        # both verdicts occur


@pytest.mark.parametrize("name", sorted(SINGLE_RULE))
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_the_depth_bound_is_exact(name, depth):
    g = compiled(name, depth)
    for n in range(depth + 1):
        assert g.matches(SINGLE_RULE[name](n)), (name, depth, n)
    assert not g.matches(SINGLE_RULE[name](depth + 1)) and not g.matches(SINGLE_RULE[name](depth + 5))


def test_anbn_is_exact_to_depth_32():
    g = compiled("anbn")
    for n in range(0, 41):
        for m in range(max(0, n - 1), n + 2):
            assert g.matches("a" * n + "b" * m) == (1 <= n == m <= 33), (n, m)          # a^n b^n takes n - 1 pushes
    assert not g.matches("a" * 40 + "b" * 40) and compile_grammar(CASES["anbn"][0], 8).matches("a" * 9 + "b" * 9)


def _explore(g: StackDFA):
    """Every (state, stack) reachable from the start, and for each whether a completion exists (backwards fixed point)."""
    cols = np.unique(g.next, axis=1, return_index=True)[1].tolist()                # one byte per class of equal columns
    seen, order, edges = {(0, ()): 0}, [(0, ())], []
    k = 0
    while k < len(order):
        st, sk = order[k]
        for b in cols:
            at = g.walk(st, sk, bytes([b]))
            if at is not None:
                if at not in seen:
                    seen[at] = len(order)
                    order.append(at)
                edges.append((seen[at], k))
        k += 1
    good = [g.ends(st, sk) for st, sk in order]
    rev = {}
    for dst, src in edges:
        rev.setdefault(dst, []).append(src)
    todo = [i for i, ok in enumerate(good) if ok]
    while todo:
        for src in rev.get(todo.pop(), ()):
            if not good[src]:
                good[src] = True
                todo.append(src)
    return order, good


@pytest.mark.parametrize("name,depth", [(n, d) for n in sorted(CASES) for d in (1, 2, 3)])
def test_every_reachable_state_and_stack_has_a_completion(name, depth):
    g = compiled(name, depth)
    order, good = _explore(g)
    assert all(good), (name, depth, [order[i] for i, ok in enumerate(good) if not ok][:3])
    assert max(len(sk) for _, sk in order) == depth and all(len(sk) + int(g.need[st]) <= depth for st, sk in order)


ERRORS = [
    ("root ::= a<item>b", "undefined rule <item>"),
    ("root ::= a\nroot ::= b", "defined twice"),
    ("start ::= a", "no rule named 'root'"),
    ("root ::= <root>a|b", "left recursive"),
    ("root ::= x<p>\np ::= <q>a|b\nq ::= <p>c|d", "left recursive"),
    ("root ::= (a<root>b)?", "matches the empty text"),
    ("root ::= a<root>b|ab|aab", "claimed twice, by a plain edge and by a call"),
    ("root ::= x(<p>|<q>)y\np ::= a<p>?b\nq ::= a<q>?c", "claimed twice, by a call of <p> and by a call of <q>"),
    ("root ::= a(<root>)*|b", "FIRST/FOLLOW"),
    ("root ::= \\(<root>\\)", "matches nothing"),
    ("root ::= z|" + "|".join(f"{a}{b}<root>{a}{b}" for a in "abcdefghijklmnop" for b in "abcdefghijklmnop"), "more than 255 call sites"),
    ("root ::= \\(<root>\\)|[ab]{1000}[cd]{1000}[ef]{1000}[gh]{1000}[ij]{200}", "GUIDE_MAX_STATES"),
    ("root ::= a<root", "opens no <rule> reference"),
    ("root ::= a*?", "lazy"),
    ("root = a", "no rule 'name ::= body'"),
]


@pytest.mark.parametrize("k", range(len(ERRORS)))
def test_each_violation_raises_with_the_rule(k):
    text, word = ERRORS[k]
    with pytest.raises(GuideError, match=re.escape(word)) as e:
        compile_grammar(text)
    assert "rule" in str(e.value) or "root" in str(e.value)
    if word in ("undefined rule <item>", "opens no <rule> reference", "lazy"):
        assert "offset" in str(e.value)


@pytest.mark.parametrize("links", [12, 30, 60])
def test_references_that_multiply_a_rule_are_refused_before_they_are_expanded(links):
    """Expansion in place copies a body at every reference: r0 ::= <r1><r1>, r1 ::= <r2><r2>, ... doubles per link.  The expansion is
    held to the NFA's bound while it is made (12 links stay under it and are refused by the state bound instead), so a grammar of
    a few hundred bytes cannot occupy the caller."""
    import time

    text = "root ::= x<r0>\n" + "".join(f"r{i} ::= <r{i + 1}><r{i + 1}>\n" for i in range(links)) + f"r{links} ::= a|\\[<root>\\]\n"
    t0 = time.perf_counter()
    with pytest.raises(GuideError, match="GUIDE_MAX_STATES" if links == 12 else "more than 400000 nodes") as e:
        compile_grammar(text)
    assert "rule 'root'" in str(e.value) and time.perf_counter() - t0 < 30
    assert compile_grammar("root ::= x<r0>\n" + "".join(f"r{i} ::= <r{i + 1}><r{i + 1}>\n" for i in range(8)) + "r8 ::= a\n").matches("x" + "a" * 256)


def test_empty_language_and_bad_depth():
    with pytest.raises(GuideError, match="matches nothing"):
        compile_grammar("root ::= \\(<root>\\)|x<root>")
    for bad in (0, 33, -1, 1.5, True, None):
        with pytest.raises(GuideError, match="max_depth"):
            compile_grammar("root ::= a", bad)
    with pytest.raises(GuideError, match="string"):
        compile_grammar(b"root ::= a")
    g = compile_grammar("root ::= ab|cd")                                           # a grammar without recursion is a plain DFA
    assert g.n_sites == 0 and g.matches("ab") and not g.matches("abc") and int(g.need.max()) == 0


def test_key_ignores_rule_names_and_depends_on_the_depth():
    a = compile_grammar(CASES["arith"][0])
    b = compile_grammar("# the same language\nroot ::= <sum>\nsum ::= <prod>([+\\-]<prod>)*\nprod ::= <atom>([*/]<atom>)*\natom ::= [0-9]+|\\(<sum>\\)\n")
    assert a.key == b.key and a.key != compile_grammar(CASES["arith"][0], 31).key and a.key != compiled("mixed").key
    assert len(a.key) == 64 and all(hasattr(a, f) for f in ("next", "accept", "key", "need", "site_start", "site_after", "site_need"))


def test_pickle_round_trip_and_stack_packing():
    g = compiled("json")
    h = pickle.loads(pickle.dumps(g))
    assert isinstance(h, StackDFA) and h.key == g.key and np.array_equal(h.next, g.next) and h.max_depth == 32
    assert h.matches('{"a":[{"b":[]}]}') and h.walk(0, (), b'{"a":[') == g.walk(0, (), b'{"a":[')
    for stack in ((), (1,), (3, 1, 2), tuple(range(1, 33)), (255,) * 32):
        w = pack_stack(stack)
        assert w.dtype == np.uint64 and w.shape == (4,) and unpack_stack(w) == stack
    assert int(pack_stack((7, 9))[0]) == 0x0709                                     # the top in the low byte
    with pytest.raises(GuideError):
        pack_stack((1,) * 33)


# --------------------------------------------------------------------------------------------------- the CPU forms of the ops
class HostPool:
    """A grammar pool on the CPU (or another device): guides placed one after another from `first`, rows outside them keep a fill."""

    def __init__(self, guides, vocab, V_, stops=(0,), first=3, P=None, device="cpu", fill=0x5A5A5A5A):
        off, data = token_table(vocab, V_)
        self.V, self.stops, self.vocab, self.rows = V_, list(stops), vocab, []
        at = first
        for g in guides:
            self.rows.append(at)
            at += ops.grammar_guide_rows(g, len(stops)) + 2
        self.P = P or at + 1
        nxt = np.full((self.P, 256), -1, np.int32)
        meta = np.full((self.P, 8), -1, np.int32)
        for g, r in zip(guides, self.rows):
            a, b = ops.grammar_guide_tables(g, r, stops)
            nxt[r:r + len(a)], meta[r:r + len(a)] = a, b
        dev = torch.device(device)
        self.next, self.meta = torch.from_numpy(nxt).to(dev), torch.from_numpy(meta).to(dev)
        self.allow = torch.full((self.P, V_ // 32), fill, dtype=torch.int32, device=dev)
        self.maybe = torch.full((self.P, V_ // 32), fill, dtype=torch.int32, device=dev)
        self.tok_off, self.tok_bytes = torch.from_numpy(off).to(dev), torch.from_numpy(data).to(dev)
        self.special = torch.tensor(self.stops, dtype=torch.int32, device=dev)
        self.guides = guides

    def build(self):
        for g, r in zip(self.guides, self.rows):
            ops.grammar_build(g.n_states, r, self.next, self.meta, self.tok_off, self.tok_bytes, self.special, self.allow, self.maybe)
        return self

    def bits(self, which, row):
        return np.unpackbits(which[row].cpu().numpy().view(np.uint8), bitorder="little")[:self.V].astype(bool)


def reachable(g: StackDFA, rng, n: int, texts):
    """(state, stack) configurations met while walking members, n of them, deepest stacks included."""
    seen = {(0, ())}
    for t in texts:
        at = (0, ())
        for b in t:
            at = g.walk(at[0], at[1], bytes([b]))
            if at is None:
                break
            seen.add(at)
    seen = sorted(seen, key=lambda c: (-len(c[1]), c))
    keep = seen[:n // 2] + [seen[int(i)] for i in rng.integers(0, len(seen), n - n // 2)]
    return keep


def outcome_bits(g, vocab, V_, stops, st, sk):
    want = np.zeros(V_, bool)
    for t, b in vocab.items():
        if t < V_ and t not in stops:
            want[t] = g.token_outcome(st, sk, b) is not None
    for t in stops:
        want[t] = g.ends(st, sk)
    return want


@pytest.mark.parametrize("name", ["json", "mixed", "anbn", "arith"])
def test_build_and_apply_host_forms_agree_with_the_walk(name):
    vocab, V_ = synthetic_vocab(), 384
    g = compiled(name, 4)
    other = compiled("markup", 4)
    pool = HostPool([other, g], vocab, V_).build()
    r0 = pool.rows[1]
    rng = np.random.default_rng(5)
    assert (pool.allow[:pool.rows[0]] == 0x5A5A5A5A).all() and (pool.maybe[r0 + g.n_states:] == 0x5A5A5A5A).all()     # only state rows are written
    for s in range(g.n_states):
        allow, maybe = pool.bits(pool.allow, r0 + s), pool.bits(pool.maybe, r0 + s)
        assert not (allow & maybe).any() and not allow[300:].any() and not maybe[300:].any()
        for t in np.nonzero(allow)[0].tolist():                                    # allowed under every stack: the empty and a full one
            if t != 0:
                for sk in ((), (1,) * (4 - int(g.need[s]))):
                    assert g.token_outcome(s, sk, vocab[t]) is not None, (s, t)
        dead = ~(allow | maybe)
        for t in np.nonzero(dead[:300])[0].tolist():                               # neither bit: dead under every stack
            if t in vocab and t != 0:
                assert all(g.token_outcome(s, sk, vocab[t]) is None for sk in ((), (1,), (1, 1, 1, 1))), (s, t)
        assert allow[0] == bool(g.accept[s] and not g.called[s]) and maybe[0] == bool(g.accept[s] and g.called[s])
    texts = [member(name, rng, 5) for _ in range(60)]
    configs = reachable(g, rng, 24, texts)
    n = len(configs)
    state = torch.tensor([r0 + st for st, _ in configs] + [-1], dtype=torch.int32)
    stack = torch.from_numpy(np.stack([pack_stack(sk) for _, sk in configs] + [pack_stack(())]).view(np.int64))
    base = torch.from_numpy(rng.standard_normal((n + 1, V_)).astype(np.float16))
    base[0, 5], base[1, 7] = float("nan"), float("-inf")
    logits = base.clone()
    rows = torch.tensor(list(range(n + 1)) + [-1, n + 5], dtype=torch.int32)
    ops.grammar_apply(logits, rows, None, state, stack, pool.next, pool.meta, pool.allow, pool.maybe, pool.tok_off, pool.tok_bytes)
    got, was = logits.numpy().view(np.uint16), base.numpy().view(np.uint16)
    for i, (st, sk) in enumerate(configs):
        want = outcome_bits(g, vocab, V_, [0], st, sk)
        assert want.any(), (st, sk)                                                # a guided row always has an allowed token
        assert np.array_equal(got[i], np.where(want, was[i], 0xFC00)), (name, st, sk)
    assert np.array_equal(got[n], was[n])                                          # the slot without a grammar
    # advance: every token from every configuration, against the walk
    ids = list(range(0, 300))
    for st, sk in configs[:6]:
        S = torch.full((len(ids),), r0 + st, dtype=torch.int32)
        K = torch.from_numpy(np.tile(pack_stack(sk).view(np.int64), (len(ids), 1)).copy())
        ops.grammar_advance(torch.arange(len(ids), dtype=torch.int32), None, torch.tensor(ids, dtype=torch.int32), pool.tok_off, pool.tok_bytes,
                            pool.next, pool.meta, S, K)
        for t in ids:
            at = g.token_outcome(st, sk, vocab[t]) if t in vocab else None
            want = (r0 + at[0], at[1]) if at is not None else (r0 + st, sk)        # a dying walk leaves both
            assert (int(S[t]), unpack_stack(K[t].numpy().view(np.uint64))) == want, (st, sk, t)
    # reset
    S, K = torch.tensor([5, 6, 7], dtype=torch.int32), torch.full((3, 4), -1, dtype=torch.int64)
    ops.grammar_reset(torch.tensor([2, 0, 9], dtype=torch.int32), torch.tensor([r0, -1, 4], dtype=torch.int32), S, K)
    assert S.tolist() == [-1, 6, r0] and K.tolist() == [[0] * 4, [-1] * 4, [0] * 4]


# --------------------------------------------------------------------------------------------------- the fake-backend worker
# finite languages the fake vocabulary can spell (its single bytes: digits, a-z, - " { } : , space . [ ]), so every request ends
NESTED = "root ::= \\[<v>(,<v>){0,2}\\]\nv ::= [a-c]{1,2}|[0-9]|\\[(<v>(,<v>)?)?\\]\n"
OBJECT = 'root ::= \\{"[a-c]":<v>\\}\nv ::= true|null|12|\\{("[a-c]":<v>)?\\}|\\[<v>?\\]\n'
PAIRS = "root ::= a<root>b|ab|c"


def _accepts(text, *grammars):
    return any(g.matches(text) for g in grammars)


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_grammar_requests_end_stop_with_an_accepted_text(run_ahead):
    torch.manual_seed(4)
    w, tq = _worker(run_ahead, batch_size=9)
    assert w._grammars is None
    ts = []
    for k, (text, depth) in enumerate(((NESTED, 3), (OBJECT, 3), (PAIRS, 5))):
        g = compile_grammar(text, depth)
        ts += [(g, _new([3 + k, 1], guide=g, max_tokens=400)), (g, _new([5, k], guide=g, max_tokens=400, **SAMPLED)),
               (g, _new([k, 9, 2], guide=g, max_tokens=400, seed=k, **SAMPLED)),
               (g, _new([k + 1], guide=g, max_tokens=400, frequency_penalty=0.5, presence_penalty=0.5, penalty_decay=0.99, **SAMPLED))]
    for _, t in ts:
        tq.put(t)
    _drain(w)
    texts = set()
    for g, t in ts:
        assert t.request_status == RequestStatus.FINISHED_STOPPED and t.error is None, (g, t.request_status, _text(t))
        assert g.matches(_text(t)), (g, _text(t))
        assert 0 not in t.generated_tokens
        texts.add(_text(t))
    assert len(texts) > 4 and any(t.count("[") + t.count("{") + t.count("a") > 2 for t in texts)      # the rows vary, and some nest
    assert w._grammars.builds == 3 and all(e["refs"] == 0 for e in w._grammars.entries.values()) and w._guides is None
    plain = [_new([k, 3], stop_tokens=[], max_tokens=5) for k in range(8)]           # the slots' next requests are unconstrained again
    for t in plain:
        tq.put(t)
    _drain(w)
    assert [t.generated_tokens for t in plain] == [expected_stream([k, 3], 5) for k in range(8)]
    state = w._grammars.state.tolist()
    assert w._grammared == [r >= 0 for r in state] and state.count(-1) >= 6         # a slot a plain request took was reset on the device


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_a_dfa_row_a_grammar_row_and_a_plain_row_share_a_step(run_ahead):
    g, d = compile_grammar(NESTED, 3), compile_regex(r"[ab]{3}c")
    solo = []
    for kw in (dict(guide=g, max_tokens=300), dict(guide=d), dict(stop_tokens=[], max_tokens=12)):
        w, tq = _worker(run_ahead, batch_size=4)
        t = _new([5, 9], **kw)
        tq.put(t)
        _drain(w)
        solo.append(t.generated_tokens)
    w, tq = _worker(run_ahead, batch_size=4)
    mixed = [_new([5, 9], guide=g, max_tokens=300), _new([5, 9], guide=d), _new([5, 9], stop_tokens=[], max_tokens=12)]
    for t in mixed:
        tq.put(t)
    _drain(w)
    after = _new([7, 7], stop_tokens=[], max_tokens=12)                             # takes the slot the grammar request had
    tq.put(after)
    _drain(w)
    assert [t.generated_tokens for t in mixed] == solo and solo[2] == expected_stream([5, 9], 12)
    assert after.generated_tokens == expected_stream([7, 7], 12)
    assert g.matches(_text(mixed[0])) and re.fullmatch(r"[ab]{3}c", _text(mixed[1])) and not g.matches(_text(mixed[2]))
    assert w._grammars.state.tolist() == [-1] * 4 and (w._grammars.stack == 0).all() and w._grammared == [False] * 4


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_three_parallel_choices_each_accepted(run_ahead, monkeypatch):
    resets, reset = [], ops.grammar_reset
    monkeypatch.setattr(ops, "grammar_reset", lambda slots, *a: (resets.append(slots.numel()), reset(slots, *a))[1])
    w, tq = _worker(run_ahead)
    g = compile_grammar(OBJECT, 3)
    kw = dict(guide=g, seed=11, max_tokens=300, **SAMPLED)
    others = [_new([4, 2, 6], choice_index=j, **kw) for j in (1, 2)]
    first = _new([4, 2, 6], siblings=others, **kw)
    tq.put(first)
    _drain(w)
    for t in [first] + others:
        assert t.request_status == RequestStatus.FINISHED_STOPPED and g.matches(_text(t)), _text(t)
    assert len({_text(t) for t in [first] + others}) > 1
    assert w._grammars.builds == 1 and [e["refs"] for e in w._grammars.entries.values()] == [0]
    assert sorted(resets) == [1, 2]                                                # admission: one slot; the fork: both siblings in one launch


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_without_a_grammar_request_no_op_is_called_and_no_pool_exists(run_ahead, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("grammar op called in a step where no row has a grammar")

    for name in ("grammar_build", "grammar_apply", "grammar_advance", "grammar_reset"):
        monkeypatch.setattr(ops, name, boom)
    w, tq = _worker(run_ahead)
    ts = [_new([1, 2, 3], stop_tokens=[], max_tokens=12), _new([4], guide=compile_regex("(yes|no)"))]
    for t in ts:
        tq.put(t)
    _drain(w)
    assert len(ts[0].generated_tokens) == 12 and _text(ts[1]) in ("yes", "no") and w._grammars is None
    tq.put(_new([1], guide=compile_grammar(PAIRS)))
    with pytest.raises(AssertionError, match="no row has a grammar"):
        _drain(w)


def test_pool_placement_refcounts_eviction_and_a_vocabulary_that_cannot_spell():
    a, b, c = compile_grammar(NESTED, 3), compile_grammar(OBJECT, 3), compile_grammar(PAIRS)
    pool = GrammarPool(ops.grammar_guide_rows(a, 1) + ops.grammar_guide_rows(b, 2) + ops.grammar_guide_rows(c, 1), 4, V, torch.device("cpu"), FAKE_VOCAB)
    ka, ra = pool.acquire(a, [0])
    assert (ra, pool.acquire(a, [0]), pool.builds) == (0, (ka, 0), 1) and pool.entries[ka]["refs"] == 2
    assert pool.entries[ka]["S"] == ops.grammar_guide_rows(a, 1) >= a.n_states
    kb, rb = pool.acquire(b, [0, 5])
    assert rb == pool.entries[ka]["S"] and pool.builds == 2
    with pytest.raises(GuideError, match="no room"):
        pool.acquire(compile_grammar("root ::= \\[<root>?\\]|[ab]{80}"), [0])
    for k in (ka, ka):
        pool.release(k)
    kc, rc = pool.acquire(c, [0])                                                   # fits behind b: nothing is dropped
    assert set(pool.entries) == {ka, kb, kc}
    with pytest.raises(GuideError, match="is no token by itself"):                  # '(' is not in the fake vocabulary
        pool.acquire(compile_grammar(CASES["sexp"][0]), [0])
    w, tq = _worker(True)
    bad, good = _new([1], guide=compile_grammar(CASES["sexp"][0])), _new([2], guide=c, max_tokens=200)
    tq.put(bad)
    tq.put(good)
    _drain(w)
    assert bad.request_status == RequestStatus.FINISHED_ABORTED and "cannot realise the grammar" in bad.error and bad.generated_tokens == []
    assert good.request_status == RequestStatus.FINISHED_STOPPED and c.matches(_text(good))


def test_task_validation_treats_a_grammar_as_any_guide():
    g = compile_grammar(PAIRS)
    for bad in (dict(guide=g, stop_tokens=[]), dict(guide=g, max_tokens=0, prompt_logprobs=1), dict(guide=g, prompt_logprobs=2),
                dict(guide=g, beam_width=2)):
        with pytest.raises(ValueError):
            _new([1, 2], **bad)
    from chirrup_amd.engine_process import task_to_wire

    wire = pickle.loads(pickle.dumps(task_to_wire(_new([1], guide=g))))
    assert isinstance(wire["guide"], StackDFA) and wire["guide"].key == g.key


# --------------------------------------------------------------------------------------------------- engine and routes
def _factory(**kw):
    return Worker(model=FakeModel(), tokenizer=GuideTok(), penalize_argmax=cpu_penalize_argmax, **kw)


async def _engine():
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=GuideTok())
    await eng.init(worker_num=1, model_config=ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64), batch_size=6)
    return eng


def test_engine_compiles_grammars_on_the_callers_side():
    async def main():
        eng = await _engine()
        with pytest.raises(GuideError, match="left recursive"):
            eng.completion("x", prefill_tokens=[1], guided_grammar="root ::= <root>a|b")
        with pytest.raises(GuideError, match="at most one of guided_regex, guided_choice, guided_json and guided_grammar"):
            eng.completion("x", prefill_tokens=[1], guided_regex="a", guided_grammar=PAIRS)
        with pytest.raises(GuideError, match="at most one of guided_regex, guided_choice and guided_json may"):      # the old wording stays
            eng.completion("x", prefill_tokens=[1], guided_regex="a", guided_choice=["a"])
        with pytest.raises(GuideError, match="string"):
            eng.compile_guide(guided_grammar=["root ::= a"])
        with pytest.raises(ValueError, match="stop tokens"):
            eng.completion("x", prefill_tokens=[1], guided_grammar=PAIRS, stop_tokens=[])
        assert eng.task_queue.empty() and eng.compile_guide() is None
        c1 = eng.completion("x", prefill_tokens=[1, 2], guided_grammar=OBJECT, stop_tokens=[0], max_tokens=300, **GREEDY)
        c2 = eng.completion("x", prefill_tokens=[1, 2], guided_grammar=OBJECT, stop_tokens=[0], max_tokens=300, **GREEDY)
        assert c1.task.guide is c2.task.guide is eng.compile_guide(guided_grammar=OBJECT) and ("grammar", OBJECT) in eng._guide_cache
        g = c1.task.guide
        assert isinstance(g, StackDFA) and g.max_depth == 32
        text = await c1.get_full_completion()
        assert g.matches(text) and isinstance(json.loads(text), dict) and c1.task.request_status == RequestStatus.FINISHED_STOPPED
        cs = eng.completions("x", prefill_tokens=[5, 6], n=3, guided_grammar=OBJECT, stop_tokens=[0], max_tokens=300, seed=4, temperature=1.0, top_p=1.0)
        texts = await asyncio.gather(*[c.get_full_completion() for c in cs])
        assert all(g.matches(t) for t in texts)
        eng.shutdown()

    asyncio.run(main())


def test_both_routes_accept_the_field_and_answer_each_400():
    async def main():
        eng = await _engine()
        app = create_app(eng, state_cache_size=0)
        msgs = [{"role": "user", "content": "answer"}]
        chat = dict(model="rwkv-latest:no-thinking", messages=msgs, max_tokens=300, **GREEDY)
        legacy = dict(prompt="answer", max_tokens=300, **GREEDY)
        g = compile_grammar(OBJECT)
        rf = {"type": "json_schema", "json_schema": {"name": "x", "schema": {"type": "boolean"}}}
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
            for route, base in (("/v1/chat/completions", chat), ("/v1/completions", legacy)):
                r = await cl.post(route, json=dict(base, guided_grammar=OBJECT))
                assert r.status_code == 200, r.text
                ch = r.json()["choices"][0]
                text = ch["message"]["content"] if "message" in ch else ch["text"]
                assert ch["finish_reason"] == "stop" and g.matches(text) and isinstance(json.loads(text), dict)
                for bad, word in ((dict(guided_grammar="root ::= <root>a|b"), "left recursive"), (dict(guided_grammar="x ::= a"), "no rule named 'root'"),
                                  (dict(guided_grammar="root ::= a*?"), "lazy"),
                                  (dict(guided_grammar=PAIRS, guided_regex="a"), "at most one"), (dict(guided_grammar=PAIRS, guided_choice=["a"]), "at most one"),
                                  (dict(guided_grammar=PAIRS, response_format=rf), "at most one"),
                                  (dict(response_format={"type": "json_object"}), "regular language"),
                                  (dict(guided_grammar=PAIRS, use_beam_search=True), "guided_grammar")):
                    r = await cl.post(route, json=dict(base, **bad))
                    assert r.status_code == 400 and word in r.json()["detail"], (route, bad, r.status_code, r.text)
                r = await cl.post(route, json=dict(base, guided_grammar=17))
                assert r.status_code == 422
            r = await cl.post("/v1/chat/completions", json=dict(chat, model="rwkv-latest:thinking", guided_grammar=PAIRS))
            assert r.status_code == 400 and "thinking" in r.json()["detail"]
            # a request without the field: the body the fake backend's stream pins
            from chirrup_amd.web_service import ChatMessage, chat_prompt

            toks = [0] + GuideTok().encode(chat_prompt([ChatMessage(**m) for m in msgs], chat["model"])[0])
            j = (await cl.post("/v1/chat/completions", json=dict(chat, max_tokens=6))).json()
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
    for name in ("build", "apply", "advance", "reset"):
        assert re.search(rf"int rwkv7_grammar_{name}\(int ", hdr) and f"rwkv7_grammar_{name}" in lib.SIGNATURES
    assert [len(lib.SIGNATURES["rwkv7_grammar_" + n][1]) for n in ("build", "apply", "advance", "reset")] == [13, 17, 15, 7]
    assert "#define CHIRRUP_GRAMMAR_STACK_DEPTH 32" in hdr and "#define CHIRRUP_GRAMMAR_CALL_SITES 255" in hdr
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    L = chirrup_amd.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)       # never dereferenced: validation fails first (or there is nothing to do)
    ok_b = [4, 0, 16, 64, p, p, p, p, 1, p, p, p, None]
    assert L.rwkv7_grammar_build(*[0] + ok_b[1:]) == 0          # S == 0: nothing launched
    for k, v in ((0, -1), (1, -1), (1, 13), (2, 0), (3, 0), (3, 96), (8, -1)):
        args = list(ok_b)
        args[k] = v
        assert L.rwkv7_grammar_build(*args) == -1, (k, v)
    for k in (4, 5, 6, 7, 9, 10, 11):
        args = list(ok_b)
        args[k] = None
        assert L.rwkv7_grammar_build(*args) == -2, k
    for k in (10, 11):
        args = list(ok_b)
        args[k] = odd
        assert L.rwkv7_grammar_build(*args) == -3, k
    ok_a = [2, 4, 64, 16, p, p, None, 8, p, p, p, p, p, p, p, p, None]
    assert L.rwkv7_grammar_apply(*[0] + ok_a[1:]) == 0
    for k, v in ((0, -1), (1, -1), (2, 0), (2, 48), (3, 0), (7, 0)):
        args = list(ok_a)
        args[k] = v
        assert L.rwkv7_grammar_apply(*args) == -1, (k, v)
    for k in (4, 5, 8, 9, 10, 11, 12, 13, 14, 15):
        args = list(ok_a)
        args[k] = None
        assert L.rwkv7_grammar_apply(*args) == -2, k
    assert L.rwkv7_grammar_apply(*ok_a[:4] + [ctypes.c_void_p(4104)] + ok_a[5:]) == -3      # logits: 16-byte aligned
    assert L.rwkv7_grammar_apply(*ok_a[:9] + [odd] + ok_a[10:]) == -3                       # the stacks: 8-byte aligned
    ok_v = [2, 4, 64, 16, p, None, 8, p, p, p, p, p, p, p, None]
    assert L.rwkv7_grammar_advance(*[0] + ok_v[1:]) == 0
    for k, v in ((0, -1), (1, -1), (2, 0), (3, 0), (6, 0)):
        args = list(ok_v)
        args[k] = v
        assert L.rwkv7_grammar_advance(*args) == -1, (k, v)
    for k in (4, 7, 8, 9, 10, 11, 12, 13):
        args = list(ok_v)
        args[k] = None
        assert L.rwkv7_grammar_advance(*args) == -2, k
    assert L.rwkv7_grammar_advance(*ok_v[:13] + [odd, None]) == -3
    ok_r = [2, 8, p, p, p, p, None]
    assert L.rwkv7_grammar_reset(*[0] + ok_r[1:]) == 0
    assert L.rwkv7_grammar_reset(-1, 8, p, p, p, p, None) == -1 and L.rwkv7_grammar_reset(2, 0, p, p, p, p, None) == -1
    for k in (2, 3, 4, 5):
        args = list(ok_r)
        args[k] = None
        assert L.rwkv7_grammar_reset(*args) == -2, k
    assert L.rwkv7_grammar_reset(2, 8, p, p, p, odd, None) == -3
