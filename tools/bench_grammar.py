"""Cost of grammar-guided decoding at the bench shape (7.2B synthetic model, bsz 200, V 65 536, the real vocabulary), under
guided.JSON_OBJECT_GRAMMAR:
  * each kernel alone (device events over many launches): rwkv7_grammar_apply and rwkv7_grammar_advance at 200 rows in three
    situations -- inside a JSON string (no maybe bit: the cost of a DFA guide), at a structural position (behind a complete value
    of a nested list: `,` `]` `}` and nearly every other live token are maybe bits, each resolved by a walk with the slot's stack),
    and at depth 31 --, beside rwkv7_guide_apply / _advance of a DFA guide inside a string; rwkv7_grammar_build per state, and
    what GrammarPool.acquire adds on the host for a new grammar (table upload and the build; nothing synchronises);
  * the Worker's decode iteration with no guided row, with all 200 rows under the grammar, and with all 200 rows under a DFA
    guide of similar size, legs alternated A B C A B C.
usage: python tools/bench_grammar.py [--model 7.2B] [--bsz 200] [--new 48] [--reps 2] [--vocab FILE] [--no-worker] [--out FILE]"""
import argparse
import gzip
import json
import os
import queue
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import ModelLoadConfig, Task
from chirrup_amd.guided import JSON_OBJECT_GRAMMAR, JSON_STRING, compile_grammar, compile_regex, pack_stack
from chirrup_amd.tokenizer import TRIE_TOKENIZER
from chirrup_amd.worker import GrammarPool, GuidePool, Worker

V = 65536
DFA_OF_SIMILAR_SIZE = r"\{(" + JSON_STRING + ":" + JSON_STRING + r",){0,6}" + JSON_STRING + ":" + JSON_STRING + r"\}"


def _time(fn, iters=200, warm=10):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _bits(t, row):
    return np.unpackbits(t[row].cpu().numpy().view(np.uint8), bitorder="little")


def kernels_alone(n, tok):
    dev = torch.device("cuda", 0)
    out = []
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    raw = (torch.randn((n, V), generator=gen, device=dev) * 3).half()
    lg = raw.clone()
    us_copy = _time(lambda: lg.copy_(raw))
    g = compile_grammar(JSON_OBJECT_GRAMMAR)
    pool = GrammarPool(2048, n, V, dev, tok.idx2token)
    t0 = time.perf_counter()
    key, row0 = pool.acquire(g, [0])
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    sp = torch.tensor([0], dtype=torch.int32, device=dev)
    us = _time(lambda: ops.grammar_build(g.n_states, row0, pool.next, pool.meta, pool.tok_off, pool.tok_bytes, sp, pool.allow, pool.maybe), iters=10, warm=2)
    out.append({"kernel": "rwkv7_grammar_build", "states": g.n_states, "call_sites": g.n_sites, "us_per_launch": round(us, 1),
                "us_per_state": round(us / g.n_states, 2), "acquire_new_grammar_host_ms": round(host_ms, 2)})
    print(json.dumps(out[-1]), flush=True)
    single = {b[0]: i for i, b in tok.idx2token.items() if len(b) == 1}
    for name, text, byte in (("in_string", b'{"ab', b"c"), ("structural", b'{"a":[[1', b","), ("depth_31", b'{"a":[' + b"[" * 31, b"1")):
        st, sk = g.walk(0, (), text)
        pool.state.fill_(row0 + st)
        words = torch.from_numpy(np.tile(pack_stack(sk).view(np.int64), (n, 1)).copy()).to(dev)
        pool.stack.copy_(words)
        allow, maybe = int(_bits(pool.allow, row0 + st).sum()), int(_bits(pool.maybe, row0 + st).sum())
        us = _time(lambda: (lg.copy_(raw), ops.grammar_apply(lg, rows, rows, pool.state, pool.stack, pool.next, pool.meta, pool.allow, pool.maybe,
                                                             pool.tok_off, pool.tok_bytes)))
        out.append({"kernel": "rwkv7_grammar_apply", "rows": n, "situation": name, "depth": len(sk), "allow_bits": allow, "maybe_bits": maybe,
                    "us_per_launch": round(us - us_copy, 2), "us_of_the_logits_reset_subtracted": round(us_copy, 2)})
        ids = torch.full((n,), single[byte[0]], dtype=torch.int32, device=dev)
        reset = lambda: (pool.state.fill_(row0 + st), pool.stack.copy_(words))
        us = _time(lambda: (reset(), ops.grammar_advance(rows, rows, ids, pool.tok_off, pool.tok_bytes, pool.next, pool.meta, pool.state, pool.stack)))
        out.append({"kernel": "rwkv7_grammar_advance", "rows": n, "situation": name, "us_per_launch": round(us - _time(reset), 2)})
        print(json.dumps(out[-2:]), flush=True)
    dfa = compile_regex(DFA_OF_SIMILAR_SIZE)
    dpool = GuidePool(16384, n, V, dev, tok.idx2token)
    _, d0 = dpool.acquire(dfa, [0])
    inner = d0 + dfa.walk(0, b'{"ab')
    dpool.state.fill_(inner)
    us = _time(lambda: (lg.copy_(raw), ops.guide_apply(lg, rows, rows, dpool.state, dpool.allow)))
    out.append({"kernel": "rwkv7_guide_apply", "rows": n, "situation": "in_string", "states": dfa.n_states,
                "allowed_tokens": int(_bits(dpool.allow, inner).sum()), "us_per_launch": round(us - us_copy, 2)})
    ids = torch.full((n,), single[ord("c")], dtype=torch.int32, device=dev)
    us = _time(lambda: (dpool.state.fill_(inner), ops.guide_advance(rows, rows, ids, dpool.tok_off, dpool.tok_bytes, dpool.next, dpool.state)))
    out.append({"kernel": "rwkv7_guide_advance", "rows": n, "situation": "in_string", "us_per_launch": round(us - _time(lambda: dpool.state.fill_(inner)), 2)})
    print(json.dumps(out[-2:]), flush=True)
    return out


class Sink:
    def __init__(self):
        self.n = 0

    def put_nowait(self, x):
        self.n += x[0] == "token_generated"


_GUIDES = {}


def worker_leg(model, tok, n, new, kind):
    cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
    tq, mq = queue.Queue(), queue.Queue()
    w = Worker("w0", [0], cfg, tq, mq, None, batch_size=n + 1, model=model, tokenizer=tok)
    w.max_prefill_count = n
    w._init_worker()
    gen = torch.Generator().manual_seed(1234)
    if kind not in _GUIDES:
        _GUIDES[kind] = {"none": lambda: None, "grammar": lambda: compile_grammar(JSON_OBJECT_GRAMMAR),
                         "dfa": lambda: compile_regex(DFA_OF_SIMILAR_SIZE)}[kind]()
    guide = _GUIDES[kind]
    tasks = []
    for k in range(n):
        t = Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="",
                 prefill_tokens=torch.randint(1, V, (4,), generator=gen).tolist(), state=None, frequency_penalty=0.0,
                 presence_penalty=0.0, penalty_decay=0.996, stop_tokens=[0] if guide is not None else [],
                 max_tokens=new, guide=guide, temperature=1.0, top_p=0.9)
        tasks.append(t)
        tq.put(t)
    for _ in range(8):
        w.step()
    torch.cuda.synchronize()
    n0 = sum(t.output_queue.n for t in tasks)
    t0 = time.perf_counter()
    steps = 0
    while w.step():
        steps += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    toks = sum(t.output_queue.n for t in tasks) - n0
    del w
    torch.cuda.empty_cache()
    # rows_per_iteration: guided rows may end "stop" before `new` tokens, so a leg's later steps hold fewer than n rows
    return {"rows_under": kind, "ms_per_iteration": round(dt / steps * 1e3, 4), "tok_per_s": round(toks / dt, 1), "iterations": steps, "tokens": toks,
            "rows_per_iteration": round(toks / steps, 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="7.2B")
    p.add_argument("--bsz", type=int, default=200)
    p.add_argument("--new", type=int, default=48)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--vocab", default=None, help="vocabulary file (default: the gzip under tests/golden)")
    p.add_argument("--no-worker", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_grammar needs a GPU"
    vocab = a.vocab
    if vocab is None:
        fd, vocab = tempfile.mkstemp(suffix=".txt")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "rwkv_vocab_v20230424.txt.gz"), "rb") as src, os.fdopen(fd, "wb") as dst:
            dst.write(src.read())
    try:
        tok = TRIE_TOKENIZER(vocab)
    finally:
        if a.vocab is None:
            os.remove(vocab)                               # the decompressed copy: the tokenizer has read it
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels_alone(a.bsz, tok)}
    if not a.no_worker:
        from chirrup_amd.rwkv7 import RWKV_x070, model_args
        from chirrup_amd.synth import CONFIGS, make_state_dict

        L, C = CONFIGS[a.model]
        zd = make_state_dict(L, C, V, seed=42, device=torch.device("cuda", 0))
        model = RWKV_x070(model_args("synthetic"), state_dict=zd, device=torch.device("cuda", 0))
        del zd
        legs = []
        for _ in range(a.reps):
            for kind in ("none", "grammar", "dfa"):
                legs.append(worker_leg(model, tok, a.bsz, a.new, kind))
                print(json.dumps(legs[-1]), flush=True)
        best = lambda k: min(x["ms_per_iteration"] for x in legs if x["rows_under"] == k)
        spread = lambda k: round(max(x["ms_per_iteration"] for x in legs if x["rows_under"] == k) - best(k), 4)
        res.update(model=a.model, bsz=a.bsz, worker_legs=legs,
                   best_ms={k: best(k) for k in ("none", "grammar", "dfa")}, spread_ms={k: spread(k) for k in ("none", "grammar", "dfa")},
                   grammar_added_us_per_step=round((best("grammar") - best("none")) * 1e3, 1),
                   dfa_added_us_per_step=round((best("dfa") - best("none")) * 1e3, 1))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
