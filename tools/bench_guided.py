"""Cost of guided decoding at the bench shape (7.2B synthetic model, bsz 200, V 65 536, the real vocabulary):
  * each kernel alone (device events over many launches): rwkv7_guide_apply and rwkv7_guide_advance at 200 rows, under a
    restrictive guide (digits: nearly every token masked) and a permissive one (a JSON string: most tokens allowed);
    rwkv7_guide_build for guides of 64, 512 and 4096 states, and what GuidePool.acquire adds on the host for a new guide
    (table upload, the build, the one synchronising check) -- the time a new guide costs the step it is admitted in;
  * the Worker's decode iteration with no guided row and with all 200 rows guided, sampled (T 1, top_p 0.9) and greedy, legs
    alternated A B A B.
usage: python tools/bench_guided.py [--model 7.2B] [--bsz 200] [--new 48] [--reps 2] [--vocab FILE] [--no-worker] [--out FILE]"""
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
from chirrup_amd.guided import JSON_STRING, compile_regex
from chirrup_amd.tokenizer import TRIE_TOKENIZER
from chirrup_amd.worker import GuidePool, Worker

V = 65536


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


def kernels_alone(n, tok):
    dev = torch.device("cuda", 0)
    out = []
    pool = GuidePool(16384, n, V, dev, tok.idx2token)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    raw = (torch.randn((n, V), generator=gen, device=dev) * 3).half()
    for name, pattern in (("digits", r"\d{1,18}"), ("json_string", JSON_STRING)):
        g = compile_regex(pattern)
        key, row0 = pool.acquire(g, [0])
        inner = row0 + int(g.next[0, ord('"')]) if name == "json_string" else row0      # inside the string: most tokens allowed
        pool.state.fill_(inner)
        bits = np.unpackbits(pool.allow[inner].cpu().numpy().view(np.uint8), bitorder="little")
        allowed = int(bits.sum())
        lg = raw.clone()
        us = _time(lambda: (lg.copy_(raw), ops.guide_apply(lg, rows, rows, pool.state, pool.allow)))
        us_copy = _time(lambda: lg.copy_(raw))
        out.append({"kernel": "rwkv7_guide_apply", "rows": n, "guide": name, "allowed_tokens": allowed,
                    "us_per_launch": round(us - us_copy, 2), "us_of_the_logits_reset_subtracted": round(us_copy, 2)})
        ok = torch.from_numpy(np.nonzero(bits)[0]).to(dev)
        ok = ok[ok != 0][:4096]
        ids = ok[torch.randint(0, len(ok), (n,), generator=gen, device=dev)].to(torch.int32)
        us = _time(lambda: (pool.state.fill_(inner), ops.guide_advance(rows, rows, ids, pool.tok_off, pool.tok_bytes, pool.next, pool.state)))
        us_fill = _time(lambda: pool.state.fill_(inner))
        out.append({"kernel": "rwkv7_guide_advance", "rows": n, "guide": name, "us_per_launch": round(us - us_fill, 2)})
        pool.release(key)
        print(json.dumps(out[-2:]), flush=True)
    for S in (64, 512, 4096):
        g = compile_regex("[a-z]{%d}" % (S - 1) if S <= 1000 else "([a-z]{819}){5}")      # (a repeat count is at most 1000)
        assert g.n_states == S
        t0 = time.perf_counter()
        key, row0 = pool.acquire(g, [0, S])                     # a new guide: upload + build + the synchronising check
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        acc = torch.from_numpy(g.accept.astype(np.uint8)).to(dev)
        sp = torch.tensor([0, S], dtype=torch.int32, device=dev)
        us = _time(lambda: ops.guide_build(S, row0, pool.next, pool.tok_off, pool.tok_bytes, sp, acc, pool.allow), iters=10, warm=2)
        pool.release(key)
        out.append({"kernel": "rwkv7_guide_build", "states": S, "us_per_launch": round(us, 1), "us_per_state": round(us / S, 2),
                    "acquire_new_guide_host_ms": round(host_ms, 2)})
        print(json.dumps(out[-1]), flush=True)
    return out


class Sink:
    def __init__(self):
        self.n = 0

    def put_nowait(self, x):
        self.n += x[0] == "token_generated"


_GUIDE = []


def worker_leg(model, tok, n, new, guided, greedy):
    cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
    tq, mq = queue.Queue(), queue.Queue()
    w = Worker("w0", [0], cfg, tq, mq, None, batch_size=n + 1, model=model, tokenizer=tok)
    w.max_prefill_count = n
    w._init_worker()
    gen = torch.Generator().manual_seed(1234)
    # long enough that no row reaches the accepting state (and with it the stop token) within `new` tokens
    if guided and not _GUIDE:
        _GUIDE.append(compile_regex(r"([a-z ,.]{1000}){2}"))
    guide = _GUIDE[0] if guided else None
    samp = dict(temperature=0.0, top_p=0.0) if greedy else dict(temperature=1.0, top_p=0.9)
    tasks = []
    for k in range(n):
        t = Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="",
                 prefill_tokens=torch.randint(1, V, (4,), generator=gen).tolist(), state=None, frequency_penalty=0.0,
                 presence_penalty=0.0, penalty_decay=0.996, stop_tokens=[0] if guided else [],
                 max_tokens=new, guide=guide, **samp)
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
    return {"guided": bool(guided), "greedy": bool(greedy), "ms_per_iteration": round(dt / steps * 1e3, 4), "tok_per_s": round(toks / dt, 1),
            "iterations": steps, "tokens": toks}


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
    assert torch.cuda.is_available(), "bench_guided needs a GPU"
    vocab = a.vocab
    if vocab is None:
        fd, vocab = tempfile.mkstemp(suffix=".txt")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "rwkv_vocab_v20230424.txt.gz"), "rb") as src, os.fdopen(fd, "wb") as dst:
            dst.write(src.read())
    tok = TRIE_TOKENIZER(vocab)
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
            for guided, greedy in ((False, False), (True, False), (False, True), (True, True)):
                legs.append(worker_leg(model, tok, a.bsz, a.new, guided, greedy))
                print(json.dumps(legs[-1]), flush=True)
        best = lambda g, gr: min(x["ms_per_iteration"] for x in legs if x["guided"] == g and x["greedy"] == gr)
        res.update(model=a.model, bsz=a.bsz, worker_legs=legs,
                   sampled={"unguided_ms": best(False, False), "guided_ms": best(True, False),
                            "added_us_per_step": round((best(True, False) - best(False, False)) * 1e3, 1)},
                   greedy={"unguided_ms": best(False, True), "guided_ms": best(True, True),
                           "added_us_per_step": round((best(True, True) - best(False, True)) * 1e3, 1)})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
