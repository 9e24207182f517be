"""Cost of prompt logprobs at the bench shape (7.2B synthetic model, V 65 536):
  * one 25 x 100 chunked-prefill forward (forward_slots) with 0, 1 and 25 sequences asking for the logprobs of their rows
    (logit_rows + the logprob kernel through the row sink, K = 5), legs alternated, device events around each forward;
  * scoring throughput: prompt tokens/s of max_tokens=0 requests with prompt_logprobs=5 through the Worker, 512-token prompts.
usage: python tools/bench_prompt_logprobs.py [--model 7.2B] [--reps 5] [--requests 100] [--prompt 512] [--out FILE]"""
import argparse
import json
import os
import queue
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import ModelLoadConfig, Task
from chirrup_amd.rwkv7 import RWKV_x070, model_args
from chirrup_amd.synth import CONFIGS, make_state_dict
from chirrup_amd.worker import Worker

V = 65536
K = 5


def chunk_leg(model, pool, slots, toks, n_ask):
    B, T = len(toks), len(toks[0])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if n_ask == 0:
        a.record()
        model.forward_slots(toks, pool, slots)
        b.record()
    else:
        rows = torch.arange((B - n_ask) * T, B * T, dtype=torch.int32, device="cuda")
        targets = torch.randint(0, V, (rows.numel(),), dtype=torch.int32, device="cuda")
        lp = torch.empty((rows.numel(), K + 1), dtype=torch.float32, device="cuda")

        def sink(r0, blk):
            v, _ = ops.token_logprobs(blk, K, targets=targets[r0:r0 + blk.shape[0]])
            lp[r0:r0 + blk.shape[0]].copy_(v)

        a.record()
        model.forward_slots(toks, pool, slots, logit_rows=rows, row_sink=sink)
        b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "x"


class Sink:
    def put_nowait(self, x):
        pass


def scoring_leg(model, n_req, plen, batch_size=201):
    cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
    w = Worker("w0", [0], cfg, queue.Queue(), queue.Queue(), None, batch_size=batch_size, model=model, tokenizer=Tok())
    w._init_worker()
    g = torch.Generator().manual_seed(7)
    tasks = [Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", state=None,
                  prefill_tokens=torch.randint(1, V, (plen,), generator=g).tolist(), max_tokens=0, prompt_logprobs=K)
             for _ in range(n_req)]
    for t in tasks:
        w.task_queue.put(t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while w.step() or not all(t.is_finished() for t in tasks):
        pass
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"requests": n_req, "prompt_tokens": n_req * plen, "seconds": round(dt, 3), "prompt_tokens_per_s": round(n_req * plen / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7.2B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--requests", type=int, default=100)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L, C = CONFIGS[a.model]
    model = RWKV_x070(model_args("synthetic", V, 64), state_dict=make_state_dict(L, C, V), device="cuda:0")
    B, T = 25, 100
    g = torch.Generator().manual_seed(3)
    toks = torch.randint(1, V, (B, T), generator=g).tolist()
    pool = model.generate_zero_state(B + 1)
    slots = torch.arange(B, dtype=torch.int32, device="cuda")
    legs = (0, 1, 25)
    for n in legs:                                           # warm-up: library set-up, _mm_nt's one-time measurement, allocator
        chunk_leg(model, pool, slots, toks, n)
    times = {n: [] for n in legs}
    for _ in range(a.reps):
        for n in legs:
            times[n].append(chunk_leg(model, pool, slots, toks, n))
    res = {"model": a.model, "chunk": f"{B}x{T}", "K": K,
           "chunk_ms_median": {str(n): round(sorted(v)[len(v) // 2], 3) for n, v in times.items()},
           "chunk_ms_all": {str(n): [round(x, 3) for x in v] for n, v in times.items()}}
    base = res["chunk_ms_median"]["0"]
    res["added_ms"] = {str(n): round(res["chunk_ms_median"][str(n)] - base, 3) for n in legs[1:]}
    del pool
    torch.cuda.empty_cache()
    scoring_leg(model, 4, a.prompt)                          # warm-up
    res["scoring"] = scoring_leg(model, a.requests, a.prompt)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
