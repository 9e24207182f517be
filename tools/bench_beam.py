"""Cost of beam search at the bench shape (7.2B synthetic model, bsz 200: 201 state slots):
  * rwkv7_beam_select alone at 25 groups x W 8 (200 rows, K = 11), device events over many launches;
  * rwkv7_beam_copy_states alone: 1 group with 7 copies, and 25 groups x W 8 with 4 copies each; the slot sets rotate so that the
    footprint of the timed launches exceeds the 256 MiB Infinity Cache (as tools/bench_fork.py does); each is reported as a fraction
    of the 6.3 TB/s streaming-copy rate bench_fork.py measures against, and beside rwkv7_fork_states at 1 group of n = 8;
  * the Worker's decode step with 0 beam rows (200 greedy requests) and with 200 beam rows (25 requests of W 8);
  * end to end: a 2 000-token prompt with W 8 and max_tokens 64 against n = 8 sampled choices, legs alternated.
usage: python tools/bench_beam.py [--model 7.2B] [--bsz 200] [--prompt 2000] [--new 64] [--reps 2] [--skip-worker] [--out FILE]"""
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


def select_leg(G=25, W=8, S=3, n_slots=201):
    dev, K = "cuda", W + S
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.randn((G * W, V), device=dev, generator=g).half()
    lp, ids = ops.token_logprobs(logits, K)
    desc = torch.tensor([ops.beam_desc(W, [0, 1, 2][:S], list(range(i * W, i * W + W)), list(range(i * W, i * W + W)),
                                       list(range(i * W, i * W + W))) for i in range(G)], dtype=torch.int32, device=dev)
    scores = torch.zeros((n_slots,), dtype=torch.float32, device=dev)
    ids_out = torch.zeros((G * W,), dtype=torch.int32, device=dev)
    out = torch.zeros((G, ops.BEAM_OUT_WORDS), dtype=torch.int32, device=dev)

    def kern():
        scores.zero_()                                    # (the scores would run off to -inf over 100 launches; the fill is ~2 us)
        ops.beam_select(lp[:, 1:], ids, desc, scores, ids_out, out)

    us = _time(kern)
    us_fill = _time(lambda: scores.zero_())
    return {"groups": G, "W": W, "K": K, "rows": G * W, "select_plus_fill_us": round(us, 2), "fill_us": round(us_fill, 2),
            "select_us": round(us - us_fill, 2)}


def copy_legs(L, C, S):
    H, dev = C // 64, "cuda"
    shift = torch.zeros((L, 2, S, C), dtype=torch.float16, device=dev)
    wkv = torch.zeros((L, S, H, 64, 64), dtype=torch.float16, device=dev)
    elapsed = torch.zeros((S,), dtype=torch.int32, device=dev)
    pool = [shift, wkv, elapsed]
    slot_bytes = L * (2 * C + H * 64 * 64) * 2 + 4
    out = []
    for G, copies in ((1, 7), (25, 4)):
        sets = []
        for r in range((S - 1) // (8 * G) if G == 1 else 8):
            src, dst = [], []
            for g in range(G):
                base = (r * 8 if G == 1 else g * 8)
                slots = list(range(base, base + 8))
                keep = (r + g) % 8 if G > 1 else 0            # the surviving parent's position; the copies rotate with r
                cs = [-1] * 8
                for j in range(copies):
                    cs[(keep + 1 + j) % 8] = slots[keep]
                src.append(cs)
                dst.append(slots)
            sets.append((torch.tensor(src, dtype=torch.int32, device=dev), torch.tensor(dst, dtype=torch.int32, device=dev)))
        k = [0]

        def kern():
            cs, ds = sets[k[0] % len(sets)]
            k[0] += 1
            ops.beam_copy_states(pool, cs, ds)

        us = _time(kern)
        nbytes = 2 * G * copies * slot_bytes                 # every copy reads its source's state and writes it once ...
        hbm = G * (1 + copies) * slot_bytes                  # ... but the copies of one source share its lines in the caches
        out.append({"groups": G, "copies_per_group": copies, "bytes_per_launch": nbytes, "rotation_sets": len(sets),
                    "kernel_us": round(us, 2), "kernel_TBps": round(nbytes / us / 1e6, 3),
                    "fraction_of_6.3TBps": round(nbytes / (us * 1e-6) / COPY_RATE, 3), "hbm_bytes_per_launch": hbm,
                    "hbm_TBps": round(hbm / us / 1e6, 3), "hbm_fraction_of_6.3TBps": round(hbm / (us * 1e-6) / COPY_RATE, 3)})
        print(json.dumps(out[-1]), flush=True)
    # rwkv7_fork_states at 1 group of n = 8 (7 destinations), the same rotation: the host-listed copy of the same bytes
    fsets = [(r * 8, list(range(r * 8 + 1, r * 8 + 8))) for r in range((S - 1) // 8)]
    tabs = []
    for s, ds in fsets:
        srcs, offs, dsts = ops._fork_groups([(s, ds)], S)
        tabs.append(torch.tensor(srcs + offs + dsts, dtype=torch.int32, device=dev))
    L_, k = lib.load(), [0]

    def fork():
        tab = tabs[k[0] % len(tabs)]
        k[0] += 1
        lib.check(L_.rwkv7_fork_states(1, L, S, C, H, tab.data_ptr(), tab.data_ptr() + 4, tab.data_ptr() + 12, shift.data_ptr(),
                                       wkv.data_ptr(), elapsed.data_ptr(), torch.cuda.current_stream().cuda_stream), "rwkv7_fork_states")

    us = _time(fork)
    out.append({"fork_states_1_group_n8_us": round(us, 2), "bytes_per_launch": 8 * slot_bytes,
                "fraction_of_6.3TBps": round(8 * slot_bytes / (us * 1e-6) / COPY_RATE, 3)})
    print(json.dumps(out[-1]), flush=True)
    del shift, wkv, pool
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


def _worker(model, bsz):
    cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=bsz + 1, model=model, tokenizer=Tok())
    w._init_worker()
    w.max_prefill_count = bsz
    return w, tq


def _mk(prompt, **kw):
    base = dict(temperature=0.0, top_p=0.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=0.996, stop_tokens=[0], max_tokens=64)
    return Task(output_queue=Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None,
                **dict(base, **kw))


def step_leg(model, bsz, beams: bool, steps=60, W=8):
    """Mean wall time of a full-width decode step: bsz greedy requests, or bsz / W beam requests of width W."""
    w, tq = _worker(model, bsz)
    g = torch.Generator().manual_seed(9)
    n = bsz // W if beams else bsz
    tasks = [_mk(torch.randint(1, V, (4,), generator=g).tolist(), max_tokens=10 ** 6, **({"beam_width": W} if beams else {}))
             for _ in range(n)]
    for t in tasks:
        tq.put(t)
    for _ in range(40):                                   # admission, forks, graph capture, warm-up
        w.step()
    width = sum(1 for td in w.state_slot.values() if td["task"] is not None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        w.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    for t in tasks:
        t.task_event_queue.put(("abort", None))
    while w.step():
        pass
    del w
    torch.cuda.empty_cache()
    return {"leg": f"{n} beam requests of W {W}" if beams else f"{n} greedy requests", "rows": width, "step_ms": round(dt * 1e3, 3)}


def e2e_leg(model, bsz, prompt, n, new, beam: bool):
    w, tq = _worker(model, bsz)
    if beam:
        tasks = submit = [_mk(prompt, beam_width=n, beam_n_best=n, max_tokens=new)]
    else:
        kw = dict(temperature=1.0, top_p=0.9, seed=7, stop_tokens=[], max_tokens=new)
        others = [_mk(prompt, choice_index=j, **kw) for j in range(1, n)]
        tasks = [_mk(prompt, siblings=others, **kw)] + others
        submit = tasks[:1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in submit:
        tq.put(t)
    while w.step():
        pass
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert all(t.output_queue.done for t in tasks)
    res = {"leg": f"beam W={n}" if beam else f"n={n} sampled", "wall_s": round(dt, 4), "iterations": w.iterations}
    del w
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="7.2B")
    p.add_argument("--bsz", type=int, default=200)
    p.add_argument("--prompt", type=int, default=2000)
    p.add_argument("--new", type=int, default=64)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--skip-worker", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_beam needs a GPU"
    L, C = CONFIGS[a.model]
    res = {"device": torch.cuda.get_device_name(0), "model": a.model, "slots": a.bsz + 1, "select": select_leg(a.bsz // 8, 8, 3, a.bsz + 1)}
    print(json.dumps(res["select"]), flush=True)
    res["copy"] = copy_legs(L, C, a.bsz + 1)
    if not a.skip_worker:
        zd = make_state_dict(L, C, V, seed=42, device=torch.device("cuda", 0))
        model = RWKV_x070(model_args("synthetic"), state_dict=zd, device=torch.device("cuda", 0))
        del zd
        steps = []
        for _ in range(a.reps):
            for beams in (False, True):
                steps.append(step_leg(model, a.bsz, beams))
                print(json.dumps(steps[-1]), flush=True)
        prompt = torch.randint(1, V, (a.prompt,), generator=torch.Generator().manual_seed(5)).tolist()
        for beam in (True, False):                        # warm-up: graph captures and the prefill GEMM plans of both legs
            e2e_leg(model, a.bsz, prompt, 8, 4, beam)
        legs = []
        for _ in range(a.reps):
            for beam in (True, False):
                legs.append(e2e_leg(model, a.bsz, prompt, 8, a.new, beam))
                print(json.dumps(legs[-1]), flush=True)
        res.update(worker_step=steps, e2e=legs, prompt=a.prompt, max_tokens=a.new)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
