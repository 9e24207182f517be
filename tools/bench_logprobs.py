"""Cost of token logprobs at the bench shape (7.2B synthetic model, bsz 200, V 65 536):
  * the rwkv7_token_logprobs kernel alone, 200 rows, K = 20 (device events over many launches), beside its HBM bytes;
  * the Worker's decode iteration with no row asking and with all 200 rows asking for logprobs + top_logprobs=20, legs alternated.
usage: python tools/bench_logprobs.py [--model 7.2B] [--bsz 200] [--new 48] [--reps 2] [--out FILE]"""
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


def kernel_alone(n, k, iters=200):
    g = torch.Generator(device="cuda").manual_seed(0)
    lg = (torch.randn((n, V), generator=g, device="cuda") * 3).half()
    tg = torch.randint(0, V, (n,), generator=g, device="cuda", dtype=torch.int32)
    for _ in range(10):
        ops.token_logprobs(lg, k, targets=tg)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        ops.token_logprobs(lg, k, targets=tg)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / iters
    nbytes = n * V * 2 + n * (k + 1) * 4 + n * k * 4 + n * 4
    return {"rows": n, "K": k, "us_per_launch": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}


class Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "x"


class Sink:
    def __init__(self):
        self.n = 0

    def put_nowait(self, x):
        self.n += x[0] == "token_generated"


def worker_leg(model, n, new, lp):
    cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
    tq, mq = queue.Queue(), queue.Queue()
    w = Worker("w0", [0], cfg, tq, mq, None, batch_size=n + 1, model=model, tokenizer=Tok())
    w.max_prefill_count = n
    w._init_worker()
    g = torch.Generator().manual_seed(1234)
    tasks = []
    for _ in range(n):
        t = Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="",
                 prefill_tokens=torch.randint(1, V, (4,), generator=g).tolist(), state=None, temperature=0.0, top_p=0.0,
                 frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=0.996, stop_tokens=[], max_tokens=new,
                 **({"logprobs": True, "top_logprobs": 20} if lp else {}))
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
    return {"logprobs": bool(lp), "ms_per_iteration": round(dt / steps * 1e3, 4), "tok_per_s": round(toks / dt, 1), "iterations": steps}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="7.2B")
    p.add_argument("--bsz", type=int, default=200)
    p.add_argument("--new", type=int, default=48)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_logprobs needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "kernel": [kernel_alone(a.bsz, k) for k in (20, 5, 0)]}
    res["kernel"].append(kernel_alone(1, 20))
    L, C = CONFIGS[a.model]
    zd = make_state_dict(L, C, V, seed=42, device=torch.device("cuda", 0))
    model = RWKV_x070(model_args("synthetic"), state_dict=zd, device=torch.device("cuda", 0))
    del zd
    legs = []
    for _ in range(a.reps):
        for lp in (False, True):
            legs.append(worker_leg(model, a.bsz, a.new, lp))
            print(json.dumps(legs[-1]), flush=True)
    off = min(x["ms_per_iteration"] for x in legs if not x["logprobs"])
    on = min(x["ms_per_iteration"] for x in legs if x["logprobs"])
    res.update(model=a.model, bsz=a.bsz, worker_legs=legs, best_ms_off=off, best_ms_on=on, added_us_per_step=round((on - off) * 1e3, 1))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
