"""Grammars for the grammar-guided decoding tests.  Each case has the grammar text, a hand-written random member generator and an
independent recogniser (plain recursive descent or counters over bytes; nothing of chirrup_amd.guided is used here except the
shipped grammar text, which is the thing under test).
A recogniser is total: it answers True or False for every byte string.  SINGLE_RULE builds, for the grammars with one recursive
rule, the text that needs exactly n pushes under the compiler's expansion policy (a reference to a rule under expansion is a
call), so the depth tests can be written down."""
import json

from chirrup_amd.guided import JSON_OBJECT_GRAMMAR

_HEX = b"0123456789abcdefABCDEF"


def _json_string(d: bytes, i: int) -> int:
    """The offset behind the JSON string at d[i:] (RFC 8259, no raw control bytes), -1 when there is none."""
    if d[i:i + 1] != b'"':
        return -1
    i += 1
    while i < len(d):
        c = d[i]
        if c == 0x22:
            return i + 1
        if c < 0x20:
            return -1
        if c == 0x5C:
            e = d[i + 1:i + 2]
            if e == b"u":
                if len(d) < i + 6 or any(h not in _HEX for h in d[i + 2:i + 6]):
                    return -1
                i += 6
            elif e and e in b'"\\/bfnrt':
                i += 2
            else:
                return -1
        else:
            i += 1
    return -1


def _digits(d: bytes, i: int) -> int:
    n = 0
    while i + n < len(d) and 0x30 <= d[i + n] <= 0x39:
        n += 1
    return n


def _json_number(d: bytes, i: int) -> int:
    """The offset behind the longest number at d[i:] that the package's compact JSON admits: -?(0|[1-9] and up to 17 more digits),
    an optional fraction of 1..18 digits, an optional exponent of 1..3 digits; -1 when there is none.  (An optional part that does
    not fit is left where it is: the caller then finds a byte that cannot follow a value.)"""
    if d[i:i + 1] == b"-":
        i += 1
    n = _digits(d, i)
    if n == 0:
        return -1
    i += 1 if d[i] == 0x30 else min(n, 18)
    if d[i:i + 1] == b".":
        n = _digits(d, i + 1)
        if n >= 1:
            i += 1 + min(n, 18)
    if d[i:i + 1] in (b"e", b"E"):
        j = i + 1 + (d[i + 1:i + 2] in (b"+", b"-"))
        n = _digits(d, j)
        if n >= 1:
            i = j + min(n, 3)
    return i


def _utf8(data: bytes) -> bool:
    try:
        data.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


# ------------------------------------------------------------------------------------------------ compact JSON, an object on top
def _json_value(d: bytes, i: int, top: bool = False) -> int:
    """The offset behind the value at d[i:], -1 when there is none."""
    if i >= len(d):
        return -1
    c = d[i:i + 1]
    if c == b"{":
        i += 1
        if d[i:i + 1] == b"}":
            return i + 1
        while True:
            i = _json_string(d, i)
            if i < 0 or d[i:i + 1] != b":":
                return -1
            i = _json_value(d, i + 1)
            if i < 0:
                return -1
            if d[i:i + 1] == b"}":
                return i + 1
            if d[i:i + 1] != b",":
                return -1
            i += 1
    if top:
        return -1
    if c == b"[":
        i += 1
        if d[i:i + 1] == b"]":
            return i + 1
        while True:
            i = _json_value(d, i)
            if i < 0:
                return -1
            if d[i:i + 1] == b"]":
                return i + 1
            if d[i:i + 1] != b",":
                return -1
            i += 1
    if c == b'"':
        return _json_string(d, i)
    for lit in (b"true", b"false", b"null"):
        if d.startswith(lit, i):
            return i + len(lit)
    return _json_number(d, i)


def json_recognise(d: bytes) -> bool:
    return _utf8(d) and _json_value(d, 0, top=True) == len(d)


def _raise(_):
    raise ValueError("a constant outside JSON")


def json_loads_dict(d: bytes) -> bool:
    return isinstance(json.loads(d.decode("utf-8"), parse_constant=_raise), dict)


_WORDS = ["a", "key", "x y", "é", "中文", "q\\n", "\\u00e9", "\\\"", "", "[]", "{", "},"]


def _json_scalar(rng) -> str:
    k = int(rng.integers(0, 7))
    if k == 0:
        return '"' + _WORDS[int(rng.integers(len(_WORDS)))] + '"'
    if k == 1:
        return str(int(rng.integers(-1000, 1000)))
    if k == 2:
        return f"{int(rng.integers(0, 99))}.{int(rng.integers(0, 999))}e{'+-'[int(rng.integers(2))]}{int(rng.integers(0, 99))}"
    return ["true", "false", "null", "0"][k - 3]


def _json_gen(rng, depth: int, obj: bool) -> str:
    n = int(rng.integers(0, 4))
    items = []
    for _ in range(n):
        k = int(rng.integers(0, 4)) if depth > 0 else 0
        v = _json_scalar(rng) if k < 2 else _json_gen(rng, depth - 1, k == 2)
        items.append(('"' + _WORDS[int(rng.integers(len(_WORDS)))] + '":' if obj else "") + v)
    return ("{%s}" if obj else "[%s]") % ",".join(items)


# ------------------------------------------------------------------------------------------------ bracket languages by descent
class _Descent:
    """Recursive descent over bytes: self.d, self.i; eat(b) consumes a literal; rules return False when they fail."""

    def __init__(self, d: bytes):
        self.d, self.i = d, 0

    def eat(self, lit: bytes) -> bool:
        if self.d.startswith(lit, self.i):
            self.i += len(lit)
            return True
        return False

    def run(self, lo: int, hi: int) -> int:
        n = 0
        while self.i < len(self.d) and lo <= self.d[self.i] <= hi:
            self.i += 1
            n += 1
        return n

    def peek(self) -> int:
        return self.d[self.i] if self.i < len(self.d) else -1


def sexp_recognise(d: bytes) -> bool:
    p = _Descent(d)

    def lst():
        if not p.eat(b"("):
            return False
        if p.eat(b")"):
            return True
        while True:
            if not (p.run(97, 122) or p.run(48, 57) or (p.peek() == 40 and lst())):
                return False
            if p.eat(b")"):
                return True
            if not p.eat(b" "):
                return False

    return lst() and p.i == len(d)


def _sexp_gen(rng, depth):
    items = []
    for _ in range(int(rng.integers(0, 4))):
        k = int(rng.integers(0, 3)) if depth > 0 else int(rng.integers(0, 2))
        items.append(["ab", "x", "lambda"][int(rng.integers(3))] if k == 0 else str(int(rng.integers(0, 500))) if k == 1 else _sexp_gen(rng, depth - 1))
    return "(" + " ".join(items) + ")"


def arith_recognise(d: bytes) -> bool:
    p = _Descent(d)

    def factor():
        if p.eat(b"("):
            return expr() and p.eat(b")")
        return p.run(48, 57) > 0

    def term():
        if not factor():
            return False
        while p.peek() in (42, 47):
            p.i += 1
            if not factor():
                return False
        return True

    def expr():
        if not term():
            return False
        while p.peek() in (43, 45):
            p.i += 1
            if not term():
                return False
        return True

    return expr() and p.i == len(d)


def _arith_gen(rng, depth):
    def factor(dep):
        if dep > 0 and rng.integers(0, 3) == 0:
            return "(" + expr(dep - 1) + ")"
        return str(int(rng.integers(0, 100)))

    def term(dep):
        return "".join(factor(dep) + "*/"[int(rng.integers(2))] for _ in range(int(rng.integers(0, 3)))) + factor(dep)

    def expr(dep):
        return "".join(term(dep) + "+-"[int(rng.integers(2))] for _ in range(int(rng.integers(0, 3)))) + term(dep)

    return expr(depth)


def anbn_recognise(d: bytes) -> bool:
    n = len(d) // 2
    return n >= 1 and d == b"a" * n + b"b" * n


def mixed_recognise(d: bytes) -> bool:
    p = _Descent(d)

    def lst():
        for o, c, sep in ((b"[", b"]", b","), (b"(", b")", b";")):
            if p.eat(o):
                if p.eat(c):
                    return True
                while True:
                    if not (p.eat(b"x") or (p.peek() in (40, 91) and lst())):
                        return False
                    if p.eat(c):
                        return True
                    if not p.eat(sep):
                        return False
        return False

    return lst() and p.i == len(d)


def _mixed_gen(rng, depth):
    sq = bool(rng.integers(2))
    items = ["x" if depth == 0 or rng.integers(0, 3) else _mixed_gen(rng, depth - 1) for _ in range(int(rng.integers(0, 4)))]
    return ("[%s]" if sq else "(%s)") % (",;"[not sq]).join(items)


def markup_recognise(d: bytes) -> bool:
    p = _Descent(d)

    def node():
        if not (p.eat(b"<a:") or p.eat(b"<b:")):
            return False
        while True:
            if p.eat(b">"):
                return True
            if not (p.eat(b"t") or (p.peek() == 60 and node())):
                return False

    return node() and p.i == len(d)


def _markup_gen(rng, depth):
    body = "".join("t" if depth == 0 or rng.integers(0, 3) else _markup_gen(rng, depth - 1) for _ in range(int(rng.integers(0, 5))))
    return "<%s:%s>" % ("ab"[int(rng.integers(2))], body)


def ascii_list_recognise(d: bytes) -> bool:
    p = _Descent(d)

    def lst():
        if not p.eat(b"["):
            return False
        if p.eat(b"]"):
            return True
        while True:
            if not (p.run(97, 122) or p.run(48, 57) or (p.peek() == 91 and lst())):
                return False
            if p.eat(b"]"):
                return True
            if not p.eat(b","):
                return False

    return lst() and p.i == len(d)


def _ascii_list_gen(rng, depth):
    items = []
    for _ in range(int(rng.integers(0, 4))):
        k = int(rng.integers(0, 3)) if depth > 0 else int(rng.integers(0, 2))
        items.append(["ab", "x", "list"][int(rng.integers(3))] if k == 0 else str(int(rng.integers(0, 500))) if k == 1 else _ascii_list_gen(rng, depth - 1))
    return "[" + ",".join(items) + "]"


SEXP = "# S-expressions\nroot ::= \\((<item>( <item>)*)?\\)\nitem ::= [a-z]+|[0-9]+|<root>\n"
ARITH = "root   ::= <expr>\nexpr   ::= <term>([+\\-]<term>)*\nterm   ::= <factor>([*/]<factor>)*\n\nfactor ::= [0-9]+|\\(<expr>\\)\n"
ANBN = "root ::= a<root>b|ab"
MIXED = "root ::= <list>\nlist ::= \\[(<elem>(,<elem>)*)?\\]|\\((<elem>(;<elem>)*)?\\)\nelem ::= x|<list>\n"
MARKUP = "root ::= <node>\nnode ::= \\<a:(t|<node>)*>|\\<b:(t|<node>)*>\n"
ASCII_LIST = "root ::= \\[(<v>(,<v>)*)?\\]\nv    ::= [a-z]+|[0-9]+|\\[(<v>(,<v>)*)?\\]\n"

# name -> (grammar text, generator(rng, nesting), recogniser(bytes), structural bytes the edits favour)
CASES = {
    "json": (JSON_OBJECT_GRAMMAR, lambda rng, dep: _json_gen(rng, dep, True), json_recognise, b'{}[],:"\\0-e.tn'),
    "sexp": (SEXP, _sexp_gen, sexp_recognise, b"() a1"),
    "arith": (ARITH, _arith_gen, arith_recognise, b"()+-*/7"),
    "anbn": (ANBN, lambda rng, dep: "a" * (dep + 1) + "b" * (dep + 1), anbn_recognise, b"ab"),
    "mixed": (MIXED, _mixed_gen, mixed_recognise, b"[](),;x"),
    "markup": (MARKUP, _markup_gen, markup_recognise, b"<>ab:t"),
    "ascii_list": (ASCII_LIST, _ascii_list_gen, ascii_list_recognise, b"[],a1"),
}
# the grammars written with one rule that calls itself (ANBN) or one called rule beside root: a level of nesting is one push
SINGLE_RULE = {"anbn": lambda n: "a" * (n + 1) + "b" * (n + 1),                 # n pushes
               "sexp": lambda n: "(" * (n + 1) + ")" * (n + 1),
               "ascii_list": lambda n: "[" * (n + 2) + "]" * (n + 2)}           # the list inside root's list is expanded in place


def member(name: str, rng, nesting: int = 8) -> bytes:
    return CASES[name][1](rng, int(rng.integers(0, nesting + 1))).encode("utf-8")


def edit(data: bytes, rng, structural: bytes) -> bytes:
    """One single-byte insert, delete or replace, biased to the structural bytes."""
    pick = lambda: structural[int(rng.integers(len(structural)))] if rng.integers(0, 4) else int(rng.integers(0, 256))
    kind = int(rng.integers(0, 3)) if data else 0
    at = int(rng.integers(0, len(data) + (kind == 0)))
    if kind == 0:
        return data[:at] + bytes([pick()]) + data[at:]
    if kind == 1:
        return data[:at] + data[at + 1:]
    return data[:at] + bytes([pick()]) + data[at + 1:]


def synthetic_vocab() -> dict:
    """An in-memory vocabulary of V = 384: every single byte (ids 1..256), multi-byte tokens that cross bracket levels, a 128-byte
    token, and ids left undefined (0 is the stop id and has no bytes; 300..383 do not exist)."""
    v = {1 + b: bytes([b]) for b in range(256)}
    extra = [b"}}", b"]}", b"}]}", b"[[[", b'{"a":[', b"[]", b"{}", b'"a":', b",[", b"],[", b"]]", b"]]]", b"1,2", b'"}', b'":{"', b"true", b"null]",
             b"((", b"))", b"(()", b"ab", b"aabb", b"<a:", b"t>", b">>", b"1+(", b")*(", b" (", b") ", b"x,[", b"[x", b"x]", b'"' + b"k" * 126 + b'"']
    for i, t in enumerate(extra):
        v[257 + i] = t
    assert len(extra[-1]) == 128 and max(v) < 300
    return v


__all__ = ["CASES", "SINGLE_RULE", "member", "edit", "synthetic_vocab", "json_loads_dict", "JSON_OBJECT_GRAMMAR"]
