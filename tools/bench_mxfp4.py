"""MXFP4 (w4a16) channel-mix weights against binary16 and uint8 (mm8) on the same box, in one process:

  1. the GEMM alone at the 7.2B ffn.key (N 16384, K 4096; relu^2 epilogue) and ffn.value (N 4096, K 16384; the partial-planes form the
     model uses) shapes at 1, 32 and 200 rows: ops.skinny_linear / skinny_linear_partial, ops.mm8t_linear / mm8t_gemm_partial,
     ops.mxfp4_linear / mxfp4_linear_partial.  Every format rotates over enough weight copies (> 600 MB together) that no launch finds
     its matrix in the L2 or the memory-side cache, as in a model step where every layer has its own; the three formats alternate
     inside each round, HIP-event time over 20 launches, median and range over the rounds.
  2. the model step (HIP-graph replay of the decode step, logits out) at 7.2B bsz 200, 7.2B bsz 32 and 13.3B bsz 64 with the
     channel-mix as binary16 / uint8 / MXFP4: the three models of a size are resident together and their timed regions alternate.
  3. resident weight bytes: the channel-mix matrices and the whole model, per format.

    python tools/bench_mxfp4.py [--steps 48] [--regions 5] [--configs 7.2B:200,7.2B:32,13.3B:64] [--no-gemm] [--no-step]

No speed is asserted anywhere; this prints what it measures."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chirrup_amd import ops                                                     # noqa: E402
from chirrup_amd.quant import quantize_linear, quantize_linear_mxfp4             # noqa: E402

DEV = "cuda:0"


def event_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def gemm_section(rounds=7, n=20):
    C = 4096
    print("== 1. GEMM alone, 7.2B channel-mix shapes; us per launch: median [min .. max] over the rounds; weights rotate over > 600 MB of copies")
    print(f"{'product':10s} {'rows':>4s}  {'binary16 (ring GEMM)':>26s}  {'uint8 (mm8 ring GEMM)':>26s}  {'MXFP4':>26s}   weight bytes f16 / u8 / mxfp4")
    for name, N, K in (("ffn.key", 4 * C, C), ("ffn.value", C, 4 * C)):
        torch.manual_seed(1)
        w16 = (torch.randn(N, K, device=DEV) / K ** 0.5).half()
        q8 = quantize_linear(w16)
        q4 = quantize_linear_mxfp4(w16)
        t16, t8, t4 = ops.tile_weight(w16), q8._replace(qT=ops.tile_weight_u8(q8.qT)), ops.tile_weight_mxfp4(q4)
        nbytes = (t16.data.numel() * 2, t8.qT.numel(), t4.data.numel())
        copies = [max(2, -(-600 * 2 ** 20 // b)) for b in nbytes]
        W16 = [t16] + [ops.TiledWeight(t16.data.clone(), N, K) for _ in range(copies[0] - 1)]
        W8 = [t8] + [t8._replace(qT=t8.qT.clone()) for _ in range(copies[1] - 1)]
        W4 = [t4] + [ops.TiledMxfp4(t4.data.clone(), N, K) for _ in range(copies[2] - 1)]
        del w16
        for M in (1, 32, 200):
            x = torch.randn(M, K, device=DEV).half()
            y = torch.empty(M, N, device=DEV, dtype=torch.float16)
            parts = torch.empty(16 * M * N, device=DEV, dtype=torch.float32)
            halves = M >= 128
            if name == "ffn.key":                   # relu^2 in the epilogue, as the model calls them
                forms = (lambda i: ops.skinny_linear(x, W16[i % len(W16)], act=1, out=y, row_halves=halves),
                         lambda i: ops.mm8t_linear(x, *W8[i % len(W8)], act=1, out=y, tiled=True),
                         lambda i: ops.mxfp4_linear(x, W4[i % len(W4)], act=1, out=y))
            else:                                   # binary32 planes for the next LN kernel (uint8: the core product of the prologue's xs)
                forms = (lambda i: ops.skinny_linear_partial(x, W16[i % len(W16)], 0, parts),
                         lambda i: ops.mm8t_gemm_partial(x, W8[i % len(W8)].qT, N, 0, parts, tiled=True),
                         lambda i: ops.mxfp4_linear_partial(x, W4[i % len(W4)], 0, parts))
            for f in forms:
                for i in range(2 * max(copies)):
                    f(i)
            torch.cuda.synchronize()
            times = [[], [], []]
            for _ in range(rounds):
                for j, f in enumerate(forms):
                    times[j].append(event_us(f, n))
            cells = [f"{statistics.median(t):8.1f} [{min(t):6.1f} .. {max(t):6.1f}]" for t in times]
            splits = (ops.gemm_splits(N, K, 1, 0), ops.mxfp4_gemm_splits(M, N, K, 0))
            print(f"{name:10s} {M:4d}  {cells[0]:>26s}  {cells[1]:>26s}  {cells[2]:>26s}   {nbytes[0] / 1e6:.1f} / {nbytes[1] / 1e6:.1f} / {nbytes[2] / 1e6:.1f} MB"
                  f"   (K-slices: ring {splits[0]}, mxfp4 {splits[1]})", flush=True)
        del W16, W8, W4, t16, t8, t4
        torch.cuda.empty_cache()


def weight_bytes(model):
    groups = model.get_gpu_parameter_groups()
    total = sum(g["size"] for g in groups)
    z, ffn = model.z, 0
    for i in range(model.n_layer):
        for n in ("key", "value"):
            k = f"blocks.{i}.ffn.{n}.weight"
            t = z[k] if k in z else z[k + ".mm8"] if k + ".mm8" in z else z[k + ".mxfp4"].data
            ffn += sum(x.numel() * x.element_size() for x in (t if isinstance(t, tuple) else (t,)))
    return ffn, total


def step_section(configs, steps, regions):
    from chirrup_amd.rwkv7 import RWKV_x070, model_args
    from chirrup_amd.synth import CONFIGS, make_state_dict

    print("\n== 2. model step (HIP-graph replay of one decode step), ms per step: median [min .. max] over alternating regions;  3. resident weight bytes")
    by_model = {}
    for name, bsz in configs:
        by_model.setdefault(name, []).append(bsz)
    for name, bszs in by_model.items():
        L, C = CONFIGS[name]
        models = {}
        for label, dt in (("binary16", torch.float16), ("uint8", torch.int8), ("mxfp4", "mxfp4")):
            before = torch.cuda.memory_allocated()
            zd = make_state_dict(L, C, 65536, seed=42, device=DEV)
            models[label] = RWKV_x070(model_args("synthetic"), state_dict=zd, device=DEV, ffn_dtype=dt)
            del zd
            torch.cuda.empty_cache()
            ffn, total = weight_bytes(models[label])
            print(f"{name} ffn {label:8s}: channel-mix matrices {ffn / 1e9:6.2f} GB, all weights {total / 1e9:6.2f} GB, allocated on the device incl. the "
                  f"ring GEMM's tile-image copies {(torch.cuda.memory_allocated() - before) / 1e9:6.2f} GB", flush=True)
        for B in bszs:
            graphs = {}
            for label, m in models.items():
                st = m.generate_zero_state(B)
                g = torch.Generator(device=DEV)
                g.manual_seed(7)
                st[0].copy_((torch.randn(st[0].shape, generator=g, device=DEV) * 0.5).half())
                st[1].copy_((torch.randn(st[1].shape, generator=g, device=DEV) * 0.1).half())
                graphs[label] = m.capture_decode_graph(st)
            tok = torch.randint(1, 65536, (B, 1), device=DEV)
            for gr in graphs.values():
                for _ in range(8):
                    gr.step(tok)
            torch.cuda.synchronize()
            times = {label: [] for label in graphs}
            for _ in range(regions):
                for label, gr in graphs.items():
                    times[label].append(event_us(lambda i: gr.step(tok), steps) / 1e3)
            base = statistics.median(times["binary16"])
            for label, t in times.items():
                med = statistics.median(t)
                print(f"{name} bsz {B:3d} ffn {label:8s}: {med:7.3f} ms/step [{min(t):7.3f} .. {max(t):7.3f}]  {med / base - 1:+7.1%} vs binary16   "
                      f"{B / med * 1e3:9.0f} tok/s", flush=True)
            del graphs
            torch.cuda.empty_cache()
        del models
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=48)
    p.add_argument("--regions", type=int, default=5)
    p.add_argument("--configs", default="7.2B:200,7.2B:32,13.3B:64")
    p.add_argument("--no-gemm", action="store_true")
    p.add_argument("--no-step", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mxfp4.py measures on the GPU: none found")
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    if not a.no_gemm:
        gemm_section()
    if not a.no_step:
        step_section([(c.split(":")[0], int(c.split(":")[1])) for c in a.configs.split(",")], a.steps, a.regions)


if __name__ == "__main__":
    main()
