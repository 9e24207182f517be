"""Shared cases of the guided-decoding tests (test_guided_cpu.py, test_guided_gpu.py): the pattern list with each pattern's minimal
state count, the schemas, a validator for the supported JSON-Schema subset, random members of a ByteDFA's language, single-edit
mutations, and a 64-entry vocabulary for the fake-backend worker."""
import numpy as np

from chirrup_amd.guided import schema_to_regex

# (pattern, states of its minimal byte DFA).  The counts are those of the minimal automaton over UTF-8 bytes with the states
# that have no completion removed: e.g. `.` needs 8 states per position (lead bytes of 2, 3 and 4-byte encodings with their
# restricted second bytes), a literal one state per byte plus the start.
PATTERNS = [
    (r"a", 2), (r"abc|abd|b", 4), (r"(yes|no|maybe)", 9), (r"[abc]+", 2), (r"a*b+c?", 3), (r"(ab|cd)*ef", 5), (r"x{3}", 4),
    (r"x{2,}", 3), (r"x{1,4}y{0,2}", 7), (r"\d{3}-\d{4}", 9), (r"-?(0|[1-9]\d{0,5})(\.\d{1,3})?", 12), (r"[A-Za-z_]\w{0,15}", 17),
    (r"\w+@\w+\.(com|org|net)", 12), (r"\s*\S+\s*", 10), (r"[^abc]{2}", 17), (r"[^\d\s]+", 9), (r"\D\W\S", 25), (r".{0,5}", 41),
    (r"a.c", 11), (r"(?:na){2,3} batman", 14), (r"\(\d+\)\[x\]\{y\}\|\*\+\?\.\^\$\\", 18), (r"[\]\-\^a]+", 2), (r"[a\-z]{2}", 3),
    (r"\x41\x7e\t\n", 5), (r"héllo|wörld", 12), (r"[éü中]+!", 6), (r"日本語(テキスト)?", 22), (r"😀{1,3}[^😀]", 23), (r"caf\xe9", 6),
    (r"(a|b)*abb", 4), (r"((a|b)(c|d)){2}|", 5), (r"\"(\\.|[^\"\\\n])*\"", 11), (r"0x[0-9a-fA-F]{1,8}", 11),
    (r"(19|20)\d\d-(0[1-9]|1[0-2])-(0[1-9]|[12]\d|3[01])", 15), (r"[€-₿]x", 5), (r"[^\x00-\x7f]{1,2}", 17),
]

# (schema, states of the minimal DFA of schema_to_regex(schema))
SCHEMAS = [
    ({"type": "string"}, 15), ({"type": "integer"}, 20), ({"type": "number"}, 44), ({"type": "boolean"}, 8), ({"type": "null"}, 5),
    ({"enum": ["red", "green", 3, 2.5, True, None, "a\"b\\c", "naïve {x}"]}, 33),
    ({"const": "only.this|one"}, 16),
    ({"type": "object", "properties": {"name": {"type": "string"}, "age": {"type": "integer"}, "ok": {"type": "boolean"}}}, 63),
    ({"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 3}, 62),
    ({"type": "array", "items": {"enum": ["a", "b"]}}, 7),
    ({"anyOf": [{"type": "null"}, {"type": "number"}, {"type": "array", "items": {"type": "boolean"}, "maxItems": 2}]}, 63),
    ({"type": "object", "properties": {"id": {"type": "integer"}, "tags": {"type": "array", "items": {"type": "string"}, "maxItems": 2},
                                       "pos": {"type": "object", "properties": {"x": {"type": "number"}, "y": {"type": "number"}}},
                                       "kind": {"enum": ["a", "b"]}}, "required": ["id"], "additionalProperties": False}, 181),
    ({"type": ["string", "null"]}, 18),
    ({"type": "object", "properties": {}}, 3),
]

ALL_PATTERNS = PATTERNS + [(schema_to_regex(s), n) for s, n in SCHEMAS]


def validate(schema, value) -> bool:
    """`value` (parsed JSON) against the supported subset: objects hold exactly the listed properties, in the listed order."""
    if "const" in schema:
        return type(value) is type(schema["const"]) and value == schema["const"]
    if "enum" in schema:
        return any(type(value) is type(v) and value == v for v in schema["enum"])
    if "anyOf" in schema:
        return any(validate(s, value) for s in schema["anyOf"])
    t = schema["type"]
    if isinstance(t, list):
        return any(validate(dict(schema, type=x), value) for x in t)
    if t == "string":
        return isinstance(value, str)
    if t == "integer":
        return isinstance(value, int) and not isinstance(value, bool)
    if t == "number":
        return isinstance(value, (int, float)) and not isinstance(value, bool)
    if t == "boolean":
        return isinstance(value, bool)
    if t == "null":
        return value is None
    if t == "object":
        props = schema.get("properties", {})
        return isinstance(value, dict) and list(value) == list(props) and all(validate(props[k], v) for k, v in value.items())
    if t == "array":
        return (isinstance(value, list) and schema.get("minItems", 0) <= len(value) <= schema.get("maxItems", 1 << 30)
                and all(validate(schema["items"], v) for v in value))
    raise AssertionError(t)


def distance_to_accept(dfa) -> np.ndarray:
    S = dfa.n_states
    dist = np.where(dfa.accept, 0, 1 << 30).astype(np.int64)
    for _ in range(S):
        nxt = np.where(dfa.next >= 0, dist[np.maximum(dfa.next, 0)], 1 << 30).min(axis=1) + 1
        new = np.minimum(dist, nxt)
        if np.array_equal(new, dist):
            break
        dist = new
    return dist


def random_member(dfa, rng, dist, wander: int) -> bytes:
    """A member of the language: a random walk of about `wander` steps (uniform over the distinct successor states, then over the
    bytes that lead there, so rare multi-byte paths are taken as often as ASCII ones), then downhill to an accepting state."""
    s, out = 0, bytearray()
    while True:
        if dfa.accept[s] and (len(out) >= wander or rng.random() < 0.15 or not (dfa.next[s] >= 0).any()):
            return bytes(out)
        row = dfa.next[s]
        targets = np.unique(row[row >= 0])
        if len(out) >= wander:
            targets = targets[dist[targets] < dist[s]] if (dist[targets] < dist[s]).any() else targets
        t = int(rng.choice(targets))
        out.append(int(rng.choice(np.nonzero(row == t)[0])))
        s = t


EDIT_ALPHABET = list("abcxyz019 -_.@\"\\{}[](),:\n\t!|*+?^$") + ["é", "ü", "中", "😀", "€", "\x7f", "\x00", "語", "ß"]


def mutate(text: str, rng) -> str:
    """One edit: a character inserted, removed or replaced (characters of the text itself and of EDIT_ALPHABET)."""
    pool = EDIT_ALPHABET + list(text)
    kind = rng.integers(0, 3) if text else 0
    at = int(rng.integers(0, len(text) + (1 if kind == 0 else 0))) if text else 0
    ch = pool[int(rng.integers(0, len(pool)))]
    if kind == 0:
        return text[:at] + ch + text[at:]
    if kind == 1:
        return text[:at] + text[at + 1:]
    return text[:at] + ch + text[at + 1:]


# a vocabulary for the fake backend (V = 64): id 0 is the end-of-text literal (the stop token), 60 and 61 have no entry; 58, 59 and 62
# are the three bytes of one character, 63 the second byte of another (every state of a guide must allow some token, also a state
# in the middle of a character)
FAKE_VOCAB = {0: b"<|endoftext|>"}
FAKE_VOCAB.update({1 + i: str(i).encode() for i in range(10)})
FAKE_VOCAB.update({11 + i: bytes([97 + i]) for i in range(26)})
FAKE_VOCAB.update({37: b"-", 38: b'"', 39: b"{", 40: b"}", 41: b":", 42: b",", 43: b"ab", 44: b"abc", 45: b"yes", 46: b"no", 47: b"12",
                   48: b" ", 49: b".", 50: b"tr", 51: b"ue", 52: b"true", 53: b"false", 54: b"null", 55: b"[", 56: b"]",
                   57: "é".encode(), 58: b"\xe4", 59: b"\xb8", 62: b"\xad", 63: b"\xa9"})
