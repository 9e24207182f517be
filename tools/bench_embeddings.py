"""Cost of text embeddings (DESIGN.md "Embeddings") at the bench shape (7.2B synthetic model, chunks of 25 sequences x 100 tokens):
  * rwkv7_pool_rows alone at 25 x 100 x 4096 (device events over many launches, index tables already on the device; the launches
    rotate over 16 row buffers, 328 MB, so that the rows come from HBM and not from the 256 MiB Infinity Cache): 20.5 MB read once;
  * one prefill chunk of 25 x 100 tokens through forward_slots with 0 and with 25 sequences pooling, legs alternated -- the leg
    without pooling is the forward as it was before embeddings existed;
  * embeddings per second for 200 inputs of 64 tokens through the engine (one worker thread, 201 slots: 25 sequences per chunk).
usage: python tools/bench_embeddings.py [--model 7.2B] [--bsz 200] [--inputs 200] [--tokens 64] [--reps 3] [--out FILE]"""
import argparse
import asyncio
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from chirrup_amd import lib
from chirrup_amd.core_structure import ModelLoadConfig
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.rwkv7 import RWKV_x070, model_args
from chirrup_amd.synth import CONFIGS, make_state_dict
from chirrup_amd.worker import Worker

V = 65536
B, T = 25, 100


def _time(fn, iters, warm=3):
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


def kernel_leg(C, n_slots):
    dev = "cuda"
    bufs = [torch.randn((B, T, C), device=dev).half() for _ in range(16)]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    seq, t0, slot = i32(list(range(B))), i32([0] * B), i32(list(range(0, 2 * B, 2)))
    acc = (torch.zeros((n_slots, C), device=dev), torch.zeros((n_slots, C), dtype=torch.float16, device=dev),
           torch.zeros((n_slots,), dtype=torch.int32, device=dev))
    k = [0]

    L_, stream = lib.load(), torch.cuda.current_stream().cuda_stream
    tail = (seq.data_ptr(), t0.data_ptr(), slot.data_ptr(), n_slots, acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), stream)

    def kern():                                            # the raw entry point: ops.pool_rows' host checks cost more than the kernel
        lib.check(L_.rwkv7_pool_rows(B, B, T, C, bufs[k[0] % len(bufs)].data_ptr(), *tail), "rwkv7_pool_rows")
        k[0] += 1

    us = _time(kern, 200, warm=10)
    nbytes = B * T * C * 2
    return {"shape": [B, T, C], "bytes_read": nbytes, "rotation_footprint_MB": round(len(bufs) * nbytes / 1e6, 1), "kernel_us": round(us, 2),
            "kernel_TBps": round(nbytes / us / 1e6, 3)}


def chunk_legs(model, n_slots, reps):
    dev = model.device
    C = model.n_embd
    pool = model.generate_zero_state(n_slots)
    slots = torch.arange(B, dtype=torch.int32, device=dev)
    toks = torch.randint(1, V, (B, T), generator=torch.Generator().manual_seed(3)).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    acc = (torch.zeros((n_slots, C), device=dev), torch.zeros((n_slots, C), dtype=torch.float16, device=dev),
           torch.zeros((n_slots,), dtype=torch.int32, device=dev))
    pooling = (i32(list(range(B))), i32([0] * B), i32(list(range(B))), *acc)
    plain = lambda: model.forward_slots(toks, pool, slots)
    pooled = lambda: model.forward_slots(toks, pool, slots, pool_rows=pooling)
    legs = []
    for _ in range(reps):                                  # alternated: drift of the clocks hits both legs alike
        legs.append({"pooling_sequences": 0, "chunk_ms": round(_time(plain, 10) / 1e3, 3)})
        legs.append({"pooling_sequences": B, "chunk_ms": round(_time(pooled, 10) / 1e3, 3)})
    return legs


class Tok:
    def encode(self, s):
        return [1]

    def decode(self, ids, utf8_errors="strict"):
        return "x"


def engine_leg(model, bsz, inputs, tokens, reps):
    def factory(**kw):
        return Worker(model=model, tokenizer=Tok(), **kw)

    async def run():
        eng = AsyncEngineCore(worker_factory=factory, tokenizer=Tok())
        cfg = ModelLoadConfig(model_path="synthetic", vocab_path="none", vocab_size=V, head_size=64)
        await eng.init(worker_num=1, model_config=cfg, batch_size=bsz + 1)
        g = torch.Generator().manual_seed(11)
        prompts = [torch.randint(1, V, (tokens - 1,), generator=g).tolist() for _ in range(inputs)]      # + the token 0 in front
        out = []
        try:
            await asyncio.gather(*[eng.embed(prefill_tokens=p) for p in prompts[:bsz // 8]])             # warm-up: GEMM plans
            for _ in range(reps):
                t0 = time.perf_counter()
                res = await asyncio.gather(*[eng.embed(prefill_tokens=p) for p in prompts])
                dt = time.perf_counter() - t0
                assert all(r["prompt_tokens"] == tokens for r in res)
                out.append({"inputs": inputs, "tokens_each": tokens, "wall_s": round(dt, 4), "embeddings_per_s": round(inputs / dt, 1),
                            "prompt_tokens_per_s": round(inputs * tokens / dt)})
        finally:
            eng.shutdown()
        return out

    return asyncio.run(run())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="7.2B")
    p.add_argument("--bsz", type=int, default=200)
    p.add_argument("--inputs", type=int, default=200)
    p.add_argument("--tokens", type=int, default=64)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_embeddings needs a GPU"
    L, C = CONFIGS[a.model]
    res = {"device": torch.cuda.get_device_name(0), "model": a.model, "slots": a.bsz + 1, "kernel": kernel_leg(4096, a.bsz + 1)}
    print(json.dumps(res["kernel"]), flush=True)
    zd = make_state_dict(L, C, V, seed=42, device=torch.device("cuda", 0))
    model = RWKV_x070(model_args("synthetic"), state_dict=zd, device=torch.device("cuda", 0))
    del zd
    res["chunk"] = chunk_legs(model, a.bsz + 1, a.reps)
    for leg in res["chunk"]:
        print(json.dumps(leg), flush=True)
    best = lambda n: min(x["chunk_ms"] for x in res["chunk"] if x["pooling_sequences"] == n)
    res["best_chunk_ms_plain"], res["best_chunk_ms_pooling"] = best(0), best(B)
    res["engine"] = engine_leg(model, a.bsz, a.inputs, a.tokens, a.reps)
    for leg in res["engine"]:
        print(json.dumps(leg), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
