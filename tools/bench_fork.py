"""Cost of parallel choices (n) at the bench shape (7.2B synthetic model, bsz 200: 201 state slots):
  * rwkv7_fork_states alone (device events over many launches, index tables already on the device): one group with n = 2, 4, 8, 16
    and 8 groups of n = 4 in one launch, beside the torch form (an index_select and an index_copy_ per table and group).  Bytes per group: one slot's
    state read once and written n - 1 times.  The slot sets rotate over disjoint slots so that the footprint of the timed launches
    exceeds the 256 MiB Infinity Cache;
  * end to end in the Worker: a 2 000-token prompt with n = 8 and max_tokens 64, against 8 independent requests of the same prompt
    (no prefix cache), legs alternated: prompt tokens fed and wall time from submission to the last completion.
usage: python tools/bench_fork.py [--model 7.2B] [--bsz 200] [--prompt 2000] [--n 8] [--new 64] [--reps 2] [--out FILE]"""
import argparse
import json
import os
import queue
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from chirrup_amd import lib, ops
from chirrup_amd.core_structure import ModelLoadConfig, Task
from chirrup_amd.rwkv7 import RWKV_x070, model_args
from chirrup_amd.synth import CONFIGS, make_state_dict
from chirrup_amd.worker import Worker

V = 65536
COPY_RATE = 6.3e12                                        # bytes/s: the achievable HBM rate of a streaming copy on an MI355X


def _time(fn, iters=100):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernel_legs(L, C, S):
    H = C // 64
    dev = "cuda"
    shift = torch.zeros((L, 2, S, C), dtype=torch.float16, device=dev)
    wkv = torch.zeros((L, S, H, 64, 64), dtype=torch.float16, device=dev)
    elapsed = torch.zeros((S,), dtype=torch.int32, device=dev)
    slot_bytes = L * (2 * C + H * 64 * 64) * 2 + 4
    L_ = lib.load()
    out = []
    for n_groups, n in ((1, 2), (1, 4), (1, 8), (1, 16), (8, 4)):
        per = n_groups * n
        sets = []                                        # disjoint slot sets, cycled
        for r in range((S - 1) // per):
            base = r * per
            groups = [(base + g * n, list(range(base + g * n + 1, base + (g + 1) * n))) for g in range(n_groups)]
            srcs, offs, dsts = ops._fork_groups(groups, S)
            tab = torch.tensor(srcs + offs + dsts, dtype=torch.int32, device=dev)
            torch_idx = [(torch.full((len(ds),), s, dtype=torch.long, device=dev), torch.tensor(ds, dtype=torch.long, device=dev))
                         for s, ds in groups]
            sets.append((tab, torch_idx))
        k = [0]

        def kern():
            tab = sets[k[0] % len(sets)][0]
            k[0] += 1
            rc = L_.rwkv7_fork_states(n_groups, L, S, C, H, tab.data_ptr(), tab.data_ptr() + 4 * n_groups,
                                      tab.data_ptr() + 4 * (2 * n_groups + 1), shift.data_ptr(), wkv.data_ptr(), elapsed.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
            lib.check(rc, "rwkv7_fork_states")

        def torch_form():
            idx = sets[k[0] % len(sets)][1]
            k[0] += 1
            for s, d in idx:
                for t, dim in ((shift, 2), (wkv, 1), (elapsed, 0)):
                    t.index_copy_(dim, d, t.index_select(dim, s))

        nbytes = n_groups * slot_bytes * n
        us_k = _time(kern)
        us_t = _time(torch_form, iters=30)
        footprint = len(sets) * nbytes
        out.append({"groups": n_groups, "n": n, "bytes_per_launch": nbytes, "rotation_footprint_MB": round(footprint / 1e6, 1),
                    "kernel_us": round(us_k, 2), "kernel_TBps": round(nbytes / us_k / 1e6, 3),
                    "kernel_fraction_of_6.3TBps": round(nbytes / (us_k * 1e-6) / COPY_RATE, 3),
                    "torch_us": round(us_t, 2), "torch_TBps": round(nbytes / us_t / 1e6, 3)})
        print(json.dumps(out[-1]), flush=True)
    del shift, wkv
    torch.cuda.empty_cache()
    return out


class Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "x"


class Sink:
    def __init__(self):
        self.n = 0
        self.done = False

    def put_nowait(self, x):
        self.n += x[0] == "token_generated"
        self.done |= x[0] == "task_completed"


class CountingWorker(Worker):
    """Counts the prompt tokens the forwards feed: chunk tokens, single-token prefill rows and a request's first decode row."""

    prompt_fed = 0

    def _run_forward_one(self, decode_slots, prefill_slots):
        self.prompt_fed += len(prefill_slots) + sum(1 for s in decode_slots if not self.state_slot[s]["feedback"])
        return super()._run_forward_one(decode_slots, prefill_slots)

    def _run_forward_seq(self, seq_slots):
        lens = [len(self.state_slot[s]["task"].prefill_tokens) - max(self.state_slot[s]["task"].cache_prefill_padding - 1, 0)
                for s in seq_slots]
        self.prompt_fed += min(self.max_forward_seq_len_per_forward, *lens) * len(seq_slots)
        return super()._run_forward_seq(seq_slots)


def e2e_leg(model, bsz, prompt, n, new, grouped):
    cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = CountingWorker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=bsz + 1, model=model, tokenizer=Tok())
    w._init_worker()
    kw = dict(temperature=1.0, top_p=0.9, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=0.996, stop_tokens=[], max_tokens=new,
              seed=7)
    mk = lambda **x: Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None,
                          **dict(kw, **x))
    if grouped:
        others = [mk(choice_index=j) for j in range(1, n)]
        tasks = [mk(siblings=others)] + others
        submit = tasks[:1]
    else:
        tasks = submit = [mk() for _ in range(n)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in submit:
        tq.put(t)
    while w.step():
        pass
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert all(t.output_queue.done and t.output_queue.n == new for t in tasks)
    res = {"leg": f"n={n} group" if grouped else f"{n} independent requests", "prompt_tokens_fed": w.prompt_fed, "wall_s": round(dt, 4),
           "iterations": w.iterations}
    del w
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="7.2B")
    p.add_argument("--bsz", type=int, default=200)
    p.add_argument("--prompt", type=int, default=2000)
    p.add_argument("--n", type=int, default=8)
    p.add_argument("--new", type=int, default=64)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--skip-e2e", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_fork needs a GPU"
    L, C = CONFIGS[a.model]
    res = {"device": torch.cuda.get_device_name(0), "model": a.model, "slots": a.bsz + 1, "kernel": kernel_legs(L, C, a.bsz + 1)}
    if not a.skip_e2e:
        zd = make_state_dict(L, C, V, seed=42, device=torch.device("cuda", 0))
        model = RWKV_x070(model_args("synthetic"), state_dict=zd, device=torch.device("cuda", 0))
        del zd
        prompt = torch.randint(1, V, (a.prompt,), generator=torch.Generator().manual_seed(5)).tolist()
        for grouped in (True, False):                     # warm-up: graph captures and the prefill GEMM plans of both legs
            e2e_leg(model, a.bsz, prompt, a.n, 4, grouped)
        legs = []
        for _ in range(a.reps):
            for grouped in (True, False):
                legs.append(e2e_leg(model, a.bsz, prompt, a.n, a.new, grouped))
                print(json.dumps(legs[-1]), flush=True)
        res.update(e2e=legs, prompt=a.prompt, n=a.n, max_tokens=a.new,
                   best_wall_s_group=min(x["wall_s"] for x in legs if "group" in x["leg"]),
                   best_wall_s_independent=min(x["wall_s"] for x in legs if "group" not in x["leg"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
