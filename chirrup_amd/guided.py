"""Guided decoding, host side: a pattern becomes a byte-level DFA (DESIGN.md "Guided decoding").

    compile_regex(pattern)   full-match regular expression over the subset below -> ByteDFA
    compile_choice(choices)  one of the given strings (built from the strings, never through regex text) -> ByteDFA
    schema_to_regex(schema)  a non-recursive JSON-Schema subset -> a pattern of the same subset (compact JSON)
    compile_grammar(text)    rules `name ::= body` over the same patterns that may refer to each other and recurse -> StackDFA, a
                             deterministic call/return automaton with a bounded stack (DESIGN.md "Grammar-guided decoding")

The automaton runs over UTF-8 bytes: the worker walks a token's vocabulary bytes through it, so a token is allowed in a state
exactly when its bytes keep a completion possible.  Pipeline: recursive-descent parser -> Thompson NFA whose edges are byte ranges
(code point sets are split into UTF-8 byte-range sequences) -> subset construction over the byte classes the NFA distinguishes ->
removal of the states no accepting state is reachable from ("live" means "has a completion") -> Hopcroft minimisation -> renumbering
in breadth-first byte order from the start state.  The result is the canonical minimal DFA of the language, so ``key`` (a hash of
its tables) is the same for every pattern of that language.

Supported: literals; escapes ``\\d \\w \\s \\D \\W \\S`` (ASCII classes, as under Python's ``re.ASCII``; the negated ones accept
every other code point), ``\\n \\t \\r \\f \\v \\xHH`` and escaped punctuation; ``.`` (any code point but ``\\n``); classes ``[...]``
with ranges and negation; groups ``(...)`` / ``(?:...)``; alternation; ``* + ? {m} {m,} {m,n}``.  Everything else -- anchors,
backreferences, look-around, named groups, flags, lazy and possessive quantifiers, braces that are no quantifier -- raises
GuideError with the construct and its offset.  Pure Python and numpy.
"""
import hashlib
import json
import re as _re
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .core_structure import GUIDE_CALL_SITES_MAX, GUIDE_MAX_STATES, GUIDE_STACK_DEPTH_MAX

MAX_CP = 0x10FFFF
MAX_REPEAT = 1000                 # largest count of a {m,n}; the state bound is what really limits a pattern
_NFA_MAX = 400_000
_SUBSET_MAX = 8 * GUIDE_MAX_STATES
Ranges = List[Tuple[int, int]]


class GuideError(ValueError):
    """A pattern, choice list or schema outside the supported subset, or one the state bound / the vocabulary cannot hold."""


class ByteDFA:
    """next int32 [S, 256] (-1: dead), accept bool [S], start state 0; every state has a completion.  Picklable (numpy arrays)."""

    def __init__(self, next_table: np.ndarray, accept: np.ndarray, pattern: str = ""):
        nxt = np.ascontiguousarray(next_table, dtype=np.int32)
        acc = np.ascontiguousarray(accept, dtype=np.bool_)
        if nxt.ndim != 2 or nxt.shape[1] != 256 or acc.shape != (nxt.shape[0],) or nxt.shape[0] < 1:
            raise GuideError("ByteDFA: next must be [S, 256] and accept [S], S >= 1")
        if nxt.shape[0] > GUIDE_MAX_STATES:
            raise GuideError(f"the automaton has {nxt.shape[0]} states, more than GUIDE_MAX_STATES = {GUIDE_MAX_STATES}")
        if int(nxt.min()) < -1 or int(nxt.max()) >= nxt.shape[0]:
            raise GuideError("ByteDFA: a transition leaves the table")
        self.next, self.accept, self.pattern = nxt, acc, pattern
        self.key = hashlib.sha256(nxt.tobytes() + acc.tobytes()).hexdigest()

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    def walk(self, state: int, data: bytes) -> int:
        """The state after `data` from `state`; -1 once the walk has died."""
        for b in data:
            if state < 0:
                return -1
            state = int(self.next[state, b])
        return state

    def matches(self, text) -> bool:
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        s = self.walk(0, data)
        return s >= 0 and bool(self.accept[s])

    def __repr__(self):
        return f"ByteDFA({self.n_states} states, key {self.key[:12]}, pattern {self.pattern[:40]!r})"


# ------------------------------------------------------------------------------------------------ code point sets and UTF-8
def _norm(rs: Ranges) -> Ranges:
    out: Ranges = []
    for lo, hi in sorted(rs):
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def _negate(rs: Ranges) -> Ranges:
    out, at = [], 0
    for lo, hi in _norm(rs):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= MAX_CP:
        out.append((at, MAX_CP))
    return out


def _scalar_values(rs: Ranges) -> Ranges:
    """Without the surrogates U+D800..U+DFFF: well-formed UTF-8 does not encode them."""
    out = []
    for lo, hi in _norm(rs):
        if lo < 0xD800:
            out.append((lo, min(hi, 0xD7FF)))
        if hi > 0xDFFF:
            out.append((max(lo, 0xE000), hi))
    return [(lo, hi) for lo, hi in out if lo <= hi]


_DIGIT: Ranges = [(48, 57)]
_WORD: Ranges = [(48, 57), (65, 90), (95, 95), (97, 122)]
_SPACE: Ranges = [(9, 13), (32, 32)]
_DOT: Ranges = _negate([(10, 10)])
_CLASS_ESCAPES = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _negate(_DIGIT), "W": _negate(_WORD), "S": _negate(_SPACE)}
_CHAR_ESCAPES = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11}


def _utf8_sequences(lo: int, hi: int):
    """Code points [lo, hi] (no surrogates inside) as sequences of byte ranges: every sequence accepts exactly the encodings of a
    sub-range, and the sub-ranges partition [lo, hi]."""
    stack = [(lo, hi)]
    while stack:
        lo, hi = stack.pop()
        split = next((m for m in (0x7F, 0x7FF, 0xFFFF) if lo <= m < hi), None)
        if split is not None:                            # the two sides encode to different lengths
            stack += [(split + 1, hi), (lo, split)]
            continue
        if hi <= 0x7F:
            yield [(lo, hi)]
            continue
        n = 2 if hi <= 0x7FF else (3 if hi <= 0xFFFF else 4)
        for i in range(1, n):
            m = (1 << (6 * i)) - 1
            if (lo & ~m) != (hi & ~m):
                if lo & m:
                    stack += [((lo | m) + 1, hi), (lo, lo | m)]
                    break
                if (hi & m) != m:
                    stack += [(hi & ~m, hi), (lo, (hi & ~m) - 1)]
                    break
        else:
            yield list(zip(chr(lo).encode("utf-8"), chr(hi).encode("utf-8")))


# ------------------------------------------------------------------------------------------------ parser
class _Parser:
    """Pattern text -> ("set", ranges) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)."""

    def __init__(self, pattern: str):
        self.p, self.i, self.depth = pattern, 0, 0

    def fail(self, what: str, at: Optional[int] = None):
        raise GuideError(f"{what} at offset {self.i if at is None else at} of the pattern {self.p!r}")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.quantified(self.atom()))
        return ("cat", items)

    def atom(self):
        c, at = self.p[self.i], self.i
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                if not self.p.startswith("?:", self.i):
                    rest = self.p[self.i + 1:self.i + 3]
                    what = ("look-ahead" if rest[:1] in ("=", "!") else "look-behind" if rest in ("<=", "<!") else
                            "a named group or backreference" if rest[:1] == "P" or rest[:1] == "<" else
                            "a comment group" if rest[:1] == "#" else "a conditional group" if rest[:1] == "(" else "inline flags")
                    self.fail(f"unsupported group ({what})", at)
                self.i += 2
            self.depth += 1
            if self.depth > 64:
                self.fail("groups nested deeper than 64", at)
            node = self.alt()
            self.depth -= 1
            if self.peek() != ")":
                self.fail("missing ')' for the group opened", at)
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            self.i += 1
            return ("set", _DOT)
        if c in "^$":
            self.fail(f"unsupported anchor {c!r} (patterns are full-match)")
        if c in "*+?":
            self.fail(f"quantifier {c!r} with nothing to repeat")
        if c in "{}":
            self.fail(f"unescaped {c!r} that is not part of a {{m}}, {{m,}} or {{m,n}} quantifier")
        if c == "\\":
            self.i += 1
            return ("set", self.escape(False))
        self.i += 1
        return ("set", [(ord(c), ord(c))])

    def escape(self, in_class: bool) -> Ranges:
        """The character(s) after a backslash (self.i stands on it)."""
        at = self.i - 1
        if self.i >= len(self.p):
            self.fail("a backslash at the end of the pattern", at)
        e = self.p[self.i]
        self.i += 1
        if e in _CLASS_ESCAPES:
            return _CLASS_ESCAPES[e]
        if e in _CHAR_ESCAPES:
            return [(_CHAR_ESCAPES[e],) * 2]
        if e == "x":
            h = self.p[self.i:self.i + 2]
            if not _re.fullmatch(r"[0-9a-fA-F]{2}", h):
                self.fail("\\x needs two hexadecimal digits", at)
            self.i += 2
            return [(int(h, 16),) * 2]
        if e.isascii() and e.isalnum():
            what = ("a backreference or octal escape" if e.isdigit() else
                    "an anchor or word-boundary escape" if e in "bBAZ" else "an unsupported escape")
            self.fail(f"{what} \\{e}", at)
        return [(ord(e), ord(e))]                        # escaped punctuation (and any non-ASCII character): itself

    def klass(self):
        at = self.i
        self.i += 1
        negated = self.peek() == "^"
        self.i += negated
        items: Ranges = []
        first = True
        while True:
            if self.i >= len(self.p):
                self.fail("unterminated character class opened", at)
            if self.p[self.i] == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_member()
            if self.peek() == "-" and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                r_at = self.i
                self.i += 1
                hi = self.class_member()
                if len(lo) != 1 or lo[0][0] != lo[0][1] or len(hi) != 1 or hi[0][0] != hi[0][1]:
                    self.fail("a class escape as the end of a range", r_at)
                if hi[0][0] < lo[0][0]:
                    self.fail("a reversed range in a character class", r_at)
                items.append((lo[0][0], hi[0][0]))
            else:
                items.extend(lo)
        rs = _norm(items)
        return ("set", _negate(rs) if negated else rs)

    def class_member(self) -> Ranges:
        c = self.p[self.i]
        self.i += 1
        if c == "\\":
            return self.escape(True)
        return [(ord(c), ord(c))]

    def quantified(self, node):
        c, at = self.peek(), self.i
        if c == "*":
            m, n = 0, None
        elif c == "+":
            m, n = 1, None
        elif c == "?":
            m, n = 0, 1
        elif c == "{":
            q = _re.compile(r"\{([0-9]+)(,([0-9]*))?\}").match(self.p, self.i)
            if q is None:
                self.fail("unescaped '{' that is not a {m}, {m,} or {m,n} quantifier")
            m = int(q.group(1))
            n = m if q.group(2) is None else (int(q.group(3)) if q.group(3) else None)
            self.i = q.end() - 1
        else:
            return node
        self.i += 1
        if n is not None and n < m:
            self.fail("a {m,n} quantifier with n < m", at)
        if m > MAX_REPEAT or (n or 0) > MAX_REPEAT:
            self.fail(f"a repeat count above {MAX_REPEAT}", at)
        nxt = self.peek()
        if nxt == "?":
            self.fail("unsupported lazy quantifier")
        if nxt == "+":
            self.fail("unsupported possessive quantifier")
        if nxt in ("*", "{"):
            self.fail("a quantifier applied to a quantifier")
        return ("rep", node, m, n)


# ------------------------------------------------------------------------------------------------ NFA
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.trans: List[List[Tuple[int, int, int]]] = []     # (byte lo, byte hi, target)

    def new(self) -> int:
        if len(self.eps) >= _NFA_MAX:
            raise GuideError(f"the pattern needs more than {_NFA_MAX} NFA states")
        self.eps.append([])
        self.trans.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            for lo, hi in _scalar_values(node[1]):
                for seq in _utf8_sequences(lo, hi):
                    cur = s
                    for k, (b0, b1) in enumerate(seq):
                        nxt = e if k == len(seq) - 1 else self.new()
                        self.trans[cur].append((b0, b1, nxt))
                        cur = nxt
            return s, e
        if kind == "call":                                  # a grammar's call of rule node[1]: one symbol past the bytes
            s, e = self.new(), self.new()
            self.trans[s].append((256 + node[1], 256 + node[1], e))
            return s, e
        if kind == "cat":
            s = cur = self.new()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[cur].append(a)
                cur = b
            return s, cur
        if kind == "alt":
            s, e = self.new(), self.new()
            for br in node[1]:
                a, b = self.build(br)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, m, n = node
        s = cur = self.new()
        for _ in range(m):
            a, b = self.build(sub)
            self.eps[cur].append(a)
            cur = b
        if n is None:
            loop = self.new()
            a, b = self.build(sub)
            self.eps[cur].append(loop)
            self.eps[loop].append(a)
            self.eps[b].append(loop)
            return s, loop
        e = self.new()
        for _ in range(n - m):
            self.eps[cur].append(e)
            a, b = self.build(sub)
            self.eps[cur].append(a)
            cur = b
        self.eps[cur].append(e)
        return s, e


def _subset_construction(nfa: _NFA, start: int, final: int, width: int = 256) -> Tuple[np.ndarray, np.ndarray]:
    cuts = {0, width}
    for ts in nfa.trans:
        for b0, b1, _ in ts:
            cuts.add(b0)
            cuts.add(b1 + 1)
    cuts = sorted(cuts)
    reps = cuts[:-1]                                      # one representative byte per class
    class_of = np.zeros(width, np.int64)
    for c, (b0, b1) in enumerate(zip(cuts[:-1], cuts[1:])):
        class_of[b0:b1] = c

    def closure(states) -> frozenset:
        seen, stack = set(states), list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(s for s in seen if nfa.trans[s] or s == final)    # the states that matter from here on

    first = closure([start])
    index: Dict[frozenset, int] = {first: 0}
    order, rows = [first], []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        edges = [t for s in cur for t in nfa.trans[s]]
        row = []
        for b in reps:
            tgt = {t for b0, b1, t in edges if b0 <= b <= b1}
            if not tgt:
                row.append(-1)
                continue
            cl = closure(tgt)
            j = index.get(cl)
            if j is None:
                if len(order) >= _SUBSET_MAX:
                    raise GuideError(f"the automaton needs more than GUIDE_MAX_STATES = {GUIDE_MAX_STATES} states")
                j = index[cl] = len(order)
                order.append(cl)
            row.append(j)
        rows.append(row)
    table = np.asarray(rows, np.int32).reshape(len(order), len(reps))[:, class_of]
    accept = np.fromiter((final in st for st in order), np.bool_, len(order))
    return table, accept


def _hopcroft(cols: np.ndarray, accept: np.ndarray, live: np.ndarray) -> Tuple[np.ndarray, int]:
    """Coarsest partition of the live states of the partial DFA `cols` [S, C] (-1 dead) that separates accepting from other states
    and is stable under every column: Hopcroft's refinement with the dead state as a block of its own (index S).  Returns the
    block of every state (-1 for states that are not live) and the number of blocks of live states."""
    S, C = cols.shape
    ids = np.nonzero(live)[0]
    tgt = np.where(cols >= 0, cols, S)
    inverse = []                                          # per column: target -> the live states that go there
    for c in range(C):
        col = tgt[ids, c]
        order = np.argsort(col, kind="stable")
        keys, first = np.unique(col[order], return_index=True)
        inverse.append(dict(zip(keys.tolist(), np.split(ids[order], first[1:]))))
    parts = [p for p in (set(ids[accept[ids]].tolist()), set(ids[~accept[ids]].tolist())) if p] + [{S}]
    block_of = {s: b for b, p in enumerate(parts) for s in p}
    work = set(range(len(parts)))
    while work:
        splitter = list(parts[work.pop()])
        for inv in inverse:
            hit: Dict[int, List[int]] = {}
            for t in splitter:
                for s in inv.get(t, ()):
                    hit.setdefault(block_of[s], []).append(s)
            for b, members in hit.items():
                if len(members) == len(parts[b]):
                    continue
                moved = set(int(s) for s in members)
                parts[b] -= moved
                nb = len(parts)
                parts.append(moved)
                for s in moved:
                    block_of[s] = nb
                work.add(nb if (b in work or len(moved) <= len(parts[b])) else b)
    block = np.full(S, -1, np.int64)
    n = 0
    for p in parts:
        if S not in p:
            block[list(p)] = n
            n += 1
    return block, n


def _finish(table: np.ndarray, accept: np.ndarray, pattern: str) -> ByteDFA:
    """A deterministic table [S, 256] (start 0, -1 dead) -> the trimmed, minimal, canonically numbered ByteDFA."""
    return ByteDFA(*_minimise(table, accept, pattern), pattern)


def _minimise(table: np.ndarray, accept: np.ndarray, pattern: str) -> Tuple[np.ndarray, np.ndarray]:
    """The trimmed, minimal, canonically numbered form of a deterministic table [S, W] (start 0, -1 dead; W = 256, or wider for a
    grammar rule, whose symbols past the bytes are its calls)."""
    S = table.shape[0]
    cols, col_of = np.unique(table, axis=1, return_inverse=True)          # byte classes: equal columns
    col_of = np.asarray(col_of).reshape(-1)
    # states with a completion: backwards from the accepting states
    src, c = np.nonzero(cols >= 0)
    dst = cols[src, c]
    by_dst = np.argsort(dst, kind="stable")
    src_sorted, starts = src[by_dst], np.searchsorted(dst[by_dst], np.arange(S + 1))
    live = accept.copy()
    stack = list(np.nonzero(accept)[0])
    while stack:
        t = stack.pop()
        for s in src_sorted[starts[t]:starts[t + 1]]:
            if not live[s]:
                live[s] = True
                stack.append(s)
    if not live[0]:
        raise GuideError(f"the pattern {pattern!r} matches nothing")
    ext_live = np.append(live, False)
    cols = np.where(ext_live[cols], cols, -1)                              # (index -1 reads the appended False)
    block, n_blocks = _hopcroft(cols, accept, live)
    rep_state = np.zeros(n_blocks, np.int64)
    rep_state[block[live]] = np.nonzero(live)[0]
    ext = np.append(block, -1)
    q = ext[cols[rep_state]]                                              # quotient over the classes [n_blocks, C]
    # canonical numbering: breadth first from the start's block, bytes in ascending order
    first_byte = np.full(cols.shape[1], table.shape[1], np.int64)
    np.minimum.at(first_byte, col_of, np.arange(table.shape[1]))
    class_order = np.argsort(first_byte, kind="stable")
    number = {int(block[0]): 0}
    order = [int(block[0])]
    k = 0
    while k < len(order):
        for t in q[order[k], class_order]:
            t = int(t)
            if t >= 0 and t not in number:
                number[t] = len(order)
                order.append(t)
        k += 1
    if len(order) > GUIDE_MAX_STATES:
        raise GuideError(f"the minimal automaton has {len(order)} states, more than GUIDE_MAX_STATES = {GUIDE_MAX_STATES}")
    renum = np.full(n_blocks + 1, -1, np.int64)
    for b, i in number.items():
        renum[b] = i
    out = renum[q[order]][:, col_of].astype(np.int32)                     # (q == -1 reads renum[-1] == -1)
    return out, accept[rep_state[order]]


def token_table(idx2token: Dict[int, bytes], V: int) -> Tuple[np.ndarray, np.ndarray]:
    """The vocabulary as the kernels read it: tok_off int32 [V + 1] (ascending offsets) and tok_bytes uint8; an id below V without
    an entry has an empty range (the model's vocabulary is padded past the file)."""
    lens = np.zeros(V, np.int64)
    for i, b in idx2token.items():
        if 0 <= i < V:
            lens[i] = len(b)
    off = np.zeros(V + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] >= 1 << 31:
        raise GuideError("the vocabulary's bytes do not fit int32 offsets")
    data = np.zeros(max(int(off[-1]), 1), np.uint8)
    for i, b in idx2token.items():
        if 0 <= i < V and len(b):
            data[off[i]:off[i + 1]] = np.frombuffer(bytes(b), np.uint8)
    return off.astype(np.int32), data


# ------------------------------------------------------------------------------------------------ public compilers
def compile_regex(pattern: str) -> ByteDFA:
    if not isinstance(pattern, str):
        raise GuideError(f"a pattern must be a string, got {type(pattern).__name__}")
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    start, final = nfa.build(ast)
    table, accept = _subset_construction(nfa, start, final)
    return _finish(table, accept, pattern)


def compile_choice(choices: Sequence[str]) -> ByteDFA:
    """One of `choices`, as the trie of their UTF-8 bytes (then minimised): no regular-expression text is involved."""
    if isinstance(choices, (str, bytes)) or not choices or not all(isinstance(c, str) for c in choices):
        raise GuideError("guided_choice must be a non-empty list of strings")
    rows: List[Dict[int, int]] = [{}]
    accept = [False]
    for c in choices:
        try:
            data = c.encode("utf-8")
        except UnicodeEncodeError as e:
            raise GuideError(f"choice {c!r} is not encodable as UTF-8: {e}") from None
        s = 0
        for b in data:
            t = rows[s].get(b)
            if t is None:
                if len(rows) >= _SUBSET_MAX:
                    raise GuideError(f"the choices need more than GUIDE_MAX_STATES = {GUIDE_MAX_STATES} states")
                t = rows[s][b] = len(rows)
                rows.append({})
                accept.append(False)
            s = t
        accept[s] = True
    table = np.full((len(rows), 256), -1, np.int32)
    for s, row in enumerate(rows):
        for b, t in row.items():
            table[s, b] = t
    return _finish(table, np.asarray(accept, np.bool_), "choice:" + json.dumps(list(choices), ensure_ascii=False))


_META = set("\\.[](){}*+?|^$-")


def escape_literal(text: str) -> str:
    """`text` as a pattern of the subset that matches exactly it."""
    out = []
    for ch in text:
        if ch in _META:
            out.append("\\" + ch)
        elif ord(ch) < 0x20 or ord(ch) == 0x7F:
            out.append(f"\\x{ord(ch):02x}")
        else:
            out.append(ch)
    return "".join(out)


# compact JSON (RFC 8259): no optional whitespace; strings without raw control bytes; numbers by the JSON grammar, bounded
JSON_STRING = r'"([^"\\\x00-\x1f]|\\(["\\/bfnrt]|u[0-9a-fA-F]{4}))*"'
JSON_INTEGER = r"-?(0|[1-9][0-9]{0,17})"
JSON_NUMBER = JSON_INTEGER + r"(\.[0-9]{1,18})?([eE][+\-]?[0-9]{1,3})?"
_TYPES = {"string": JSON_STRING, "integer": JSON_INTEGER, "number": JSON_NUMBER, "boolean": "(true|false)", "null": "null"}
_ANNOTATIONS = {"title", "description", "default", "examples", "$schema", "$id", "$comment", "required", "additionalProperties"}
_REFUSED = ("$ref", "$defs", "definitions", "pattern", "format", "oneOf", "allOf", "not", "if", "patternProperties",
            "prefixItems", "dependentSchemas")


def _json_literal(v: Any, where: str) -> str:
    if isinstance(v, float) and v != v or v in (float("inf"), float("-inf")):
        raise GuideError(f"{where}: a non-finite number is not JSON")
    if v is not None and not isinstance(v, (str, bool, int, float)):
        raise GuideError(f"{where}: enum / const values must be scalars, got {type(v).__name__}")
    return escape_literal(json.dumps(v, ensure_ascii=False, separators=(",", ":")))


def _schema(schema: Any, where: str, depth: int) -> str:
    if depth > 32:
        raise GuideError(f"{where}: schemas nested deeper than 32 (recursion is not supported)")
    if not isinstance(schema, dict):
        raise GuideError(f"{where}: a schema must be an object, got {type(schema).__name__}")
    for k in _REFUSED:
        if k in schema:
            raise GuideError(f"{where}: '{k}' is not supported")
    if schema.get("additionalProperties") not in (None, False):
        raise GuideError(f"{where}: additionalProperties other than false is not supported")
    known = _ANNOTATIONS | {"type", "enum", "const", "properties", "items", "minItems", "maxItems", "anyOf"}
    extra = sorted(set(schema) - known)
    if extra:
        raise GuideError(f"{where}: '{extra[0]}' is not supported")
    if "const" in schema:
        return _json_literal(schema["const"], where + ".const")
    if "enum" in schema:
        if not isinstance(schema["enum"], list) or not schema["enum"]:
            raise GuideError(f"{where}.enum: must be a non-empty list")
        return "(" + "|".join(_json_literal(v, where + ".enum") for v in schema["enum"]) + ")"
    if "anyOf" in schema:
        if not isinstance(schema["anyOf"], list) or not schema["anyOf"]:
            raise GuideError(f"{where}.anyOf: must be a non-empty list")
        return "(" + "|".join(_schema(s, f"{where}.anyOf[{i}]", depth + 1) for i, s in enumerate(schema["anyOf"])) + ")"
    t = schema.get("type")
    if isinstance(t, list) and t:
        return "(" + "|".join(_schema(dict(schema, type=x), where, depth + 1) for x in t) + ")"
    if t in _TYPES:
        return _TYPES[t]
    if t == "object":
        props = schema.get("properties", {})
        if not isinstance(props, dict):
            raise GuideError(f"{where}.properties: must be an object")
        missing = [r for r in schema.get("required", []) if r not in props]
        if missing:
            raise GuideError(f"{where}.required: '{missing[0]}' is not among the properties")
        parts = [_json_literal(str(name), where) + ":" + _schema(sub, f"{where}.{name}", depth + 1) for name, sub in props.items()]
        return r"\{" + ",".join(parts) + r"\}"
    if t == "array":
        if "items" not in schema:
            raise GuideError(f"{where}: an array needs 'items'")
        item = "(" + _schema(schema["items"], where + ".items", depth + 1) + ")"
        lo, hi = schema.get("minItems", 0), schema.get("maxItems")
        for name, v in (("minItems", lo), ("maxItems", hi)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0 or v > MAX_REPEAT):
                raise GuideError(f"{where}.{name}: must be an integer in [0, {MAX_REPEAT}]")
        if hi is not None and hi < lo:
            raise GuideError(f"{where}: maxItems < minItems")
        if hi == 0:
            return r"\[\]"
        more = f"(,{item}){{{max(lo - 1, 0)},{'' if hi is None else hi - 1}}}"
        return rf"\[{item}{more}\]" if lo > 0 else rf"\[({item}{more})?\]"
    raise GuideError(f"{where}: type {t!r} is not supported (string, integer, number, boolean, null, object, array; enum, const, anyOf)")


def schema_to_regex(schema: Dict[str, Any]) -> str:
    """The pattern of the compact JSON texts that satisfy `schema` (the subset in the module docstring of DESIGN.md's section):
    objects hold exactly the listed properties, all required, in the listed order."""
    return _schema(schema, "schema", 0)


# ------------------------------------------------------------------------------------------------ grammars (DESIGN.md "Grammar-guided decoding")
_RULE_LINE = _re.compile(r"([A-Za-z_][A-Za-z0-9_]*)\s*::=(.*)$", _re.S)
_REF = _re.compile(r"<([A-Za-z_][A-Za-z0-9_]*)>")
_GRAMMAR_WIDTH = 256 + GUIDE_CALL_SITES_MAX               # a rule's alphabet: the bytes, then one symbol per called rule
_NEED_INF = 255


class _GrammarParser(_Parser):
    """A rule body: the pattern dialect plus the atom <name> -> ("ref", name, offset)."""

    def __init__(self, body: str, rule: str):
        super().__init__(body)
        self.rule = rule

    def fail(self, what: str, at: Optional[int] = None):
        raise GuideError(f"rule {self.rule!r}: {what} at offset {self.i if at is None else at} of its body {self.p!r}")

    def atom(self):
        if self.p[self.i] == "<":
            m = _REF.match(self.p, self.i)
            if m is None:
                self.fail("'<' that opens no <rule> reference (a literal '<' is written '\\<')")
            at, self.i = self.i, m.end()
            return ("ref", m.group(1), at)
        return super().atom()


def pack_stack(stack: Sequence[int]) -> np.ndarray:
    """A stack (call-site ids, bottom first) as the device holds it: uint64 [4], the top in the low byte of word 0, 0 below the bottom."""
    if len(stack) > GUIDE_STACK_DEPTH_MAX or any(not 1 <= c <= GUIDE_CALL_SITES_MAX for c in stack):
        raise GuideError(f"a stack holds at most {GUIDE_STACK_DEPTH_MAX} call sites in 1..{GUIDE_CALL_SITES_MAX}")
    v = 0
    for c in stack:
        v = (v << 8) | int(c)
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], np.uint64)


def unpack_stack(words) -> Tuple[int, ...]:
    """The inverse of pack_stack: the call-site ids, bottom first."""
    v = 0
    for k in range(4):
        v |= (int(words[k]) & 0xFFFFFFFFFFFFFFFF) << (64 * k)
    out = []
    while v:
        out.append(v & 0xFF)
        v >>= 8
    return tuple(reversed(out))


class StackDFA:
    """A deterministic call/return automaton over bytes: the minimal DFAs of the compiled rules in one state numbering (start 0).

        next       int32 [S, 256]  >= 0: plain edge (the only move that consumes the byte); -1: no move of the state's own;
                                   -(c + 1), c in 1..n_sites: call site c -- push c, go on with the same byte at site_start[c]
        accept     bool  [S]       final state of its rule; ``called`` bool [S]: its rule is called from somewhere, so a final
                                   state returns (pop c, go on with the same byte at site_after[c]) on a byte it has no move for
        need       uint8 [S]       the least further stack depth a completion from the state requires
        site_start / site_after int32 [n_sites + 1], site_need uint8 [n_sites + 1] = max(1 + need[start], need[after]); entry 0 unused

    A move into a state (or through a call site) whose need exceeds the room left under max_depth is refused, so every reachable
    (state, stack) has a completion.  The text is accepted when the returns at its end reach an accepting state with an empty
    stack.  A stack is a tuple of call-site ids, bottom first.  ``key`` hashes all tables and max_depth.  Picklable."""

    def __init__(self, next_table, accept, called, need, site_start, site_after, site_need, max_depth: int, pattern: str = ""):
        self.next = np.ascontiguousarray(next_table, dtype=np.int32)
        self.accept = np.ascontiguousarray(accept, dtype=np.bool_)
        self.called = np.ascontiguousarray(called, dtype=np.bool_)
        self.need = np.ascontiguousarray(need, dtype=np.uint8)
        self.site_start = np.ascontiguousarray(site_start, dtype=np.int32)
        self.site_after = np.ascontiguousarray(site_after, dtype=np.int32)
        self.site_need = np.ascontiguousarray(site_need, dtype=np.uint8)
        self.max_depth, self.pattern = int(max_depth), pattern
        S, n = self.next.shape[0], self.site_start.shape[0]
        if self.next.ndim != 2 or self.next.shape[1] != 256 or S < 1 or any(a.shape != (S,) for a in (self.accept, self.called, self.need)):
            raise GuideError("StackDFA: next must be [S, 256] and accept, called, need [S], S >= 1")
        if not 1 <= n <= GUIDE_CALL_SITES_MAX + 1 or self.site_after.shape != (n,) or self.site_need.shape != (n,):
            raise GuideError(f"StackDFA: at most {GUIDE_CALL_SITES_MAX} call sites")
        if S > GUIDE_MAX_STATES:
            raise GuideError(f"the automaton has {S} states, more than GUIDE_MAX_STATES = {GUIDE_MAX_STATES}")
        if not 1 <= self.max_depth <= GUIDE_STACK_DEPTH_MAX:
            raise GuideError(f"max_depth must be in 1..{GUIDE_STACK_DEPTH_MAX}, got {max_depth}")
        if int(self.next.min()) < -n or int(self.next.max()) >= S or (n > 1 and (
                int(min(self.site_start[1:].min(), self.site_after[1:].min())) < 0 or int(max(self.site_start.max(), self.site_after.max())) >= S)):
            raise GuideError("StackDFA: a transition leaves the tables")
        h = hashlib.sha256()
        for a in (self.next, self.accept, self.called, self.need, self.site_start, self.site_after, self.site_need):
            h.update(a.tobytes())
            h.update(b"|")
        h.update(str(self.max_depth).encode())
        self.key = h.hexdigest()

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    @property
    def n_sites(self) -> int:
        return self.site_start.shape[0] - 1

    def edge_bytes(self) -> List[int]:
        """The bytes that label an edge (plain, or the first byte of a call): each must be a token of the vocabulary by itself."""
        return np.nonzero((self.next != -1).any(axis=0))[0].tolist()

    def walk(self, state: int, stack: Sequence[int], data: bytes):
        """(state, stack) after `data` from (state, stack), or None once the walk has died."""
        st, D = list(stack), self.max_depth
        for b in data:
            for _ in range(2 * GUIDE_STACK_DEPTH_MAX + 2):
                v = int(self.next[state, b])
                if v >= 0:
                    if len(st) + int(self.need[v]) > D:
                        return None
                    state = v
                    break
                if v < -1:
                    c = -v - 1
                    if len(st) + int(self.site_need[c]) > D:
                        return None
                    st.append(c)
                    state = int(self.site_start[c])
                elif st and self.accept[state] and self.called[state]:
                    state = int(self.site_after[st.pop()])
                else:
                    return None
            else:
                return None
        return state, tuple(st)

    def ends(self, state: int, stack: Sequence[int]) -> bool:
        """Whether the text may end at (state, stack): the returns at its end reach an accepting state with an empty stack."""
        st = list(stack)
        while st and self.accept[state] and self.called[state]:
            state = int(self.site_after[st.pop()])
        return not st and bool(self.accept[state])

    def token_outcome(self, state: int, stack: Sequence[int], token_bytes: bytes):
        """What the worker's mask decides for a token with these bytes: the (state, stack) it leads to, None when it is masked
        (an id without bytes is always masked)."""
        return self.walk(state, stack, token_bytes) if len(token_bytes) else None

    def matches(self, text) -> bool:
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        at = self.walk(0, (), data)
        return at is not None and self.ends(*at)

    def __repr__(self):
        return (f"StackDFA({self.n_states} states, {self.n_sites} call sites, max_depth {self.max_depth}, key {self.key[:12]}, "
                f"grammar {self.pattern[:40]!r})")


def compile_grammar(text: str, max_depth: int = GUIDE_STACK_DEPTH_MAX) -> StackDFA:
    """Grammar text -> StackDFA.  One rule per line, ``name ::= body``; ``#`` lines and blank lines are ignored; ``root`` is the
    start.  A body is a pattern of the dialect above (whitespace around it stripped) plus ``<name>``, a reference to a rule (a
    literal ``<`` is ``\\<``).  This is not GBNF: the pattern parser, its UTF-8 handling and its error offsets are reused.

    Expansion policy (what max_depth counts): rules are expanded from root, depth first; a reference to a rule that is not under
    expansion is expanded in place, a reference to a rule that is under expansion (an ancestor, or the rule itself) becomes a
    call, and a called rule is compiled on its own by the same policy.  Each call is one push; texts that need more than max_depth
    pushes are not members.  The grammar must be deterministic with one byte of look-ahead: every violation raises GuideError."""
    if not isinstance(text, str):
        raise GuideError(f"a grammar must be a string, got {type(text).__name__}")
    if isinstance(max_depth, bool) or not isinstance(max_depth, int) or not 1 <= max_depth <= GUIDE_STACK_DEPTH_MAX:
        raise GuideError(f"max_depth must be an integer in 1..{GUIDE_STACK_DEPTH_MAX}, got {max_depth!r}")
    asts: Dict[str, Any] = {}
    for ln, line in enumerate(text.split("\n"), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        m = _RULE_LINE.match(line)
        if m is None:
            raise GuideError(f"line {ln} of the grammar is no rule 'name ::= body': {line[:60]!r}")
        name = m.group(1)
        if name in asts:
            raise GuideError(f"rule {name!r} is defined twice (line {ln})")
        asts[name] = _GrammarParser(m.group(2).strip(), name).parse()
    if "root" not in asts:
        raise GuideError("the grammar has no rule named 'root'")

    called: Dict[str, int] = {}                            # called rule -> its symbol 256 + k, in order of the first call

    budget = [0]                                           # nodes of the rule under compilation, expansions in place included

    def expand(node, under: Tuple[str, ...]):
        # expansion in place copies a rule's body at every reference, so a chain of rules can double at each link: the nodes are
        # counted as they are made and held to the NFA's own bound (every node becomes at least one NFA state)
        budget[0] += 1
        if budget[0] > _NFA_MAX:
            raise GuideError(f"rule {under[0]!r}: expanded in place (through {' -> '.join(under)}) it has more than {_NFA_MAX} nodes; "
                             f"the grammar's references multiply its size")
        kind = node[0]
        if kind == "set":
            return node
        if kind in ("cat", "alt"):
            return (kind, [expand(n, under) for n in node[1]])
        if kind == "rep":
            return ("rep", expand(node[1], under), node[2], node[3])
        _, name, at = node
        if name not in asts:
            raise GuideError(f"rule {under[-1]!r}: undefined rule <{name}> at offset {at} of its body")
        if name in under:
            if name not in called:
                if len(called) >= GUIDE_CALL_SITES_MAX:
                    raise GuideError(f"rule {under[-1]!r}: more than {GUIDE_CALL_SITES_MAX} call sites (<{name}> at offset {at})")
                called[name] = len(called)
            return ("call", called[name])
        return expand(asts[name], under + (name,))

    # the compiled rules ("units"): root, then the called rules in order of their first call; each a minimal DFA over bytes + calls
    units: List[str] = ["root"]
    tables: List[Tuple[np.ndarray, np.ndarray]] = []
    u = 0
    while u < len(units):
        name = units[u]
        nfa = _NFA()
        budget[0] = 0
        start, final = nfa.build(expand(asts[name], (name,)))
        t, a = _subset_construction(nfa, start, final, _GRAMMAR_WIDTH)
        try:
            tables.append(_minimise(t, a, f"rule {name}"))
        except GuideError as e:
            raise GuideError(f"rule {name!r}: {e}") from None
        for r in sorted(called, key=called.get):
            if r not in units:
                units.append(r)
        u += 1
    base = np.cumsum([0] + [t.shape[0] for t, _ in tables])
    S = int(base[-1])
    if S > GUIDE_MAX_STATES:
        raise GuideError(f"the grammar's rules have {S} states in total, more than GUIDE_MAX_STATES = {GUIDE_MAX_STATES}")
    start_of = {name: int(base[i]) for i, name in enumerate(units)}
    k_name = sorted(called, key=called.get)                # k -> rule
    k_start = [start_of[r] for r in k_name]
    plain = np.full((S, 256), -1, np.int32)
    accept, is_called, unit_of = np.zeros(S, np.bool_), np.zeros(S, np.bool_), np.zeros(S, np.int64)
    calls: List[List[Tuple[int, int]]] = [[] for _ in range(S)]          # per state: (k, state after the call)
    for i, (t, a) in enumerate(tables):
        lo, hi = int(base[i]), int(base[i + 1])
        plain[lo:hi] = np.where(t[:, :256] >= 0, t[:, :256] + lo, -1)
        accept[lo:hi], is_called[lo:hi], unit_of[lo:hi] = a, units[i] in called, i
        for s, k in zip(*np.nonzero(t[:, 256:] >= 0)):
            calls[lo + int(s)].append((int(k), lo + int(t[s, 256 + k])))
    where = lambda s: f"rule {units[int(unit_of[s])]!r} (state {s - int(base[unit_of[s]])} of its automaton)"
    for k, r in enumerate(k_name):
        if accept[k_start[k]]:
            raise GuideError(f"rule {r!r} is called and matches the empty text: a call must consume a byte")

    # need, level by level: the states that complete with L further pushes, backwards from the final states
    src, b = np.nonzero(plain >= 0)
    rev: List[set] = [set() for _ in range(S)]
    for s_, t_ in set(zip(src.tolist(), plain[src, b].tolist())):
        rev[t_].add(s_)
    need = np.full(S, _NEED_INF, np.int64)
    for level in range(len(k_name) + 2):
        ok = need <= level
        ok |= accept
        stack_ = list(np.nonzero(ok)[0])
        call_in: List[List[int]] = [[] for _ in range(S)]               # after-state -> callers whose callee fits the level
        for s_ in range(S):
            for k, t_ in calls[s_]:
                if level >= 1 and need[k_start[k]] <= level - 1:
                    call_in[t_].append(s_)
        while stack_:
            t_ = int(stack_.pop())
            for s_ in list(rev[t_]) + call_in[t_]:
                if not ok[s_]:
                    ok[s_] = True
                    stack_.append(s_)
        need[ok & (need == _NEED_INF)] = level
    if (need == _NEED_INF).any():
        s_ = int(np.nonzero(need == _NEED_INF)[0][0])
        raise GuideError(f"{where(s_)} has no completion: a rule it calls matches nothing (a recursion without a way out)")
    if need[0] > max_depth:
        raise GuideError(f"the grammar matches nothing within max_depth = {max_depth}: its shortest text needs {int(need[0])} pushes")

    # FIRST of the called rules (left recursion is a cycle among the calls made at a start state)
    first: List[Optional[np.ndarray]] = [None] * len(k_name)
    visiting: List[int] = []

    def first_of(k: int) -> np.ndarray:
        if first[k] is not None:
            return first[k]
        if k in visiting:
            cyc = " -> ".join(k_name[j] for j in visiting[visiting.index(k):] + [k])
            raise GuideError(f"rule {k_name[k]!r} is left recursive: it can call itself before a byte is consumed ({cyc})")
        visiting.append(k)
        f = plain[k_start[k]] >= 0
        for j, _ in calls[k_start[k]]:
            f = f | first_of(j)
        visiting.pop()
        first[k] = f
        return f

    for k in range(len(k_name)):
        first_of(k)
    # call sites and the edge table: a byte is claimed once per state
    site_of: Dict[Tuple[int, int], int] = {}
    site_start, site_after, site_need = [0], [0], [0]
    nxt = plain.copy()
    for s_ in range(S):
        for k, t_ in calls[s_]:
            c = site_of.get((k, t_))
            if c is None:
                if len(site_of) >= GUIDE_CALL_SITES_MAX:
                    raise GuideError(f"{where(s_)}: the grammar has more than {GUIDE_CALL_SITES_MAX} call sites")
                c = site_of[(k, t_)] = len(site_of) + 1
                site_start.append(k_start[k])
                site_after.append(t_)
                site_need.append(max(1 + int(need[k_start[k]]), int(need[t_])))
            clash = first[k] & (nxt[s_] != -1)
            if clash.any():
                bb = int(np.nonzero(clash)[0][0])
                other = "a plain edge" if nxt[s_, bb] >= 0 else f"a call of <{k_name[k_start.index(site_start[-int(nxt[s_, bb]) - 1])]}>"
                raise GuideError(f"{where(s_)}: the byte {bytes([bb])!r} is claimed twice, by {other} and by a call of <{k_name[k]}>")
            nxt[s_, first[k]] = -(c + 1)
    claimed = nxt != -1
    # FOLLOW of the called rules, to a fixed point; a final state of a called rule must not claim a byte that may follow the rule
    follow = np.zeros((len(k_name), 256), np.bool_)
    unit_k = [called.get(name, -1) for name in units]
    changed = True
    while changed:
        changed = False
        for (k, t_) in site_of:
            f = follow[k] | claimed[t_]
            j = unit_k[int(unit_of[t_])]
            if accept[t_] and j >= 0:
                f = f | follow[j]
            if (f != follow[k]).any():
                follow[k], changed = f, True
    for s_ in range(S):
        k = unit_k[int(unit_of[s_])]
        if accept[s_] and k >= 0 and (claimed[s_] & follow[k]).any():
            bb = int(np.nonzero(claimed[s_] & follow[k])[0][0])
            raise GuideError(f"{where(s_)}: a final state of the called rule can take the byte {bytes([bb])!r}, which may also "
                             f"follow the rule (FIRST/FOLLOW conflict)")
    return StackDFA(nxt, accept, is_called, need.astype(np.uint8), site_start, site_after, site_need, max_depth, text)


_JSON_MEMBERS = "(" + JSON_STRING + ":<value>(," + JSON_STRING + ":<value>)*)?"
# compact JSON with an object at the top, as schema_to_regex emits it; the one recursive rule is `value`, so one level of value
# nesting is exactly one push
JSON_OBJECT_GRAMMAR = ("root  ::= \\{" + _JSON_MEMBERS + "\\}\n"
                       "value ::= \\{" + _JSON_MEMBERS + "\\}|\\[(<value>(,<value>)*)?\\]|" + JSON_STRING + "|" + JSON_NUMBER
                       + "|true|false|null\n")



__all__ = ["ByteDFA", "GuideError", "compile_regex", "compile_choice", "schema_to_regex", "escape_literal", "token_table", "JSON_STRING",
           "JSON_INTEGER", "JSON_NUMBER", "StackDFA", "compile_grammar", "pack_stack", "unpack_stack", "JSON_OBJECT_GRAMMAR"]
