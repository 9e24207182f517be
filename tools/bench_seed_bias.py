"""Cost of per-request seeds and logit_bias at the bench shape (7.2B synthetic model, bsz 200, V 65 536):
  * each kernel alone at 200 rows (device events over many launches): rwkv7_seeded_uniform with every row seeded,
    rwkv7_apply_logit_bias with 64 and 1024 entries per row;
  * the Worker's decode iteration with all 200 rows sampled (T 1, top_p 0.9) and none asking, and with all 200 rows seeded plus a
    64-entry logit_bias each, legs alternated.
usage: python tools/bench_seed_bias.py [--model 7.2B] [--bsz 200] [--new 48] [--reps 2] [--out FILE]"""
import argparse
import json
import os
import queue
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import LOGIT_BIAS_MAX, ModelLoadConfig, Task
from chirrup_amd.rwkv7 import RWKV_x070, model_args
from chirrup_amd.synth import CONFIGS, make_state_dict
from chirrup_amd.worker import Worker

V = 65536


def _time(fn, iters=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernels_alone(n):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    seeds = torch.randint(-(1 << 62), 1 << 62, (n,), generator=g, device=dev, dtype=torch.int64)
    seeded = torch.ones((n,), dtype=torch.int32, device=dev)
    counters = torch.zeros((n,), dtype=torch.int32, device=dev)
    u = torch.rand((n,), generator=g, device=dev)
    out = [{"kernel": "rwkv7_seeded_uniform", "rows": n,
            "us_per_launch": round(_time(lambda: ops.seeded_uniform(rows, rows, seeds, seeded, counters, u)), 2)}]
    lg = (torch.randn((n, V), generator=g, device=dev) * 3).half()
    for k in (64, LOGIT_BIAS_MAX):
        ids = torch.stack([torch.randperm(V, device=dev)[:LOGIT_BIAS_MAX] for _ in range(n)]).to(torch.int32)
        vals = (torch.rand((n, LOGIT_BIAS_MAX), generator=g, device=dev) * 200 - 100)
        cnt = torch.full((n,), k, dtype=torch.int32, device=dev)
        us = _time(lambda: ops.apply_logit_bias(lg, rows, cnt, ids, vals))
        out.append({"kernel": "rwkv7_apply_logit_bias", "rows": n, "entries": k, "us_per_launch": round(us, 2),
                    "bytes": n * k * (4 + 4 + 2 + 2) + n * 4})
    return out


class Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "x"


class Sink:
    def __init__(self):
        self.n = 0

    def put_nowait(self, x):
        self.n += x[0] == "token_generated"


def worker_leg(model, n, new, ask):
    cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
    tq, mq = queue.Queue(), queue.Queue()
    w = Worker("w0", [0], cfg, tq, mq, None, batch_size=n + 1, model=model, tokenizer=Tok())
    w.max_prefill_count = n
    w._init_worker()
    g = torch.Generator().manual_seed(1234)
    tasks = []
    for k in range(n):
        extra = {}
        if ask:
            extra = {"seed": 1000 + k, "logit_bias": {int(t): 0.5 for t in torch.randperm(V, generator=g)[:64].tolist()}}
        t = Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="",
                 prefill_tokens=torch.randint(1, V, (4,), generator=g).tolist(), state=None, temperature=1.0, top_p=0.9,
                 frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=0.996, stop_tokens=[], max_tokens=new, **extra)
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
    return {"seed_and_bias": bool(ask), "ms_per_iteration": round(dt / steps * 1e3, 4), "tok_per_s": round(toks / dt, 1),
            "iterations": steps}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="7.2B")
    p.add_argument("--bsz", type=int, default=200)
    p.add_argument("--new", type=int, default=48)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_seed_bias needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels_alone(a.bsz)}
    print(json.dumps(res["kernels"]), flush=True)
    L, C = CONFIGS[a.model]
    zd = make_state_dict(L, C, V, seed=42, device=torch.device("cuda", 0))
    model = RWKV_x070(model_args("synthetic"), state_dict=zd, device=torch.device("cuda", 0))
    del zd
    legs = []
    for _ in range(a.reps):
        for ask in (False, True):
            legs.append(worker_leg(model, a.bsz, a.new, ask))
            print(json.dumps(legs[-1]), flush=True)
    off = min(x["ms_per_iteration"] for x in legs if not x["seed_and_bias"])
    on = min(x["ms_per_iteration"] for x in legs if x["seed_and_bias"])
    res.update(model=a.model, bsz=a.bsz, worker_legs=legs, best_ms_off=off, best_ms_on=on, added_us_per_step=round((on - off) * 1e3, 1))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
