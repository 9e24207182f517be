"""One export (slot -> arena row) and one install (arena row -> slot) of a whole request state through a plain HbmStateArena
(strided copies, 2 x the state bytes each) and through a packed one (wkv_format="mxint8": ops.state_pack / state_unpack, about
1.5 x), at the 7.2B and 13.3B state geometries, in ONE process with the forms alternating round by round.  HIP-event times, the
median of the rounds; rows and slots rotate so that no round finds its bytes in the Infinity Cache.  Two times per form: "call",
the events around one call as a worker thread issues it (three launches: the device waits for the host in between), and "device",
the same behind a 1-GiB fill that keeps the device busy while the host enqueues the three launches -- the time the device itself
needs.  Also bytes per state and rows per 100 GB of each format.

usage: python tools/bench_state_codec.py [rounds=40] [out.txt]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from chirrup_amd.state_cache import HbmStateArena
from chirrup_amd.synth import CONFIGS

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 40
out_path = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
ROWS = SLOTS = 16                      # 16 x 17-33 MB per table: more than the 256 MiB Infinity Cache
WARM = 4
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


filler = torch.empty(1 << 30, dtype=torch.uint8, device=dev)


def timed(fn, behind_fill=False):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if behind_fill:
        filler.fill_(1)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3     # microseconds


say(f"# state codec on {torch.cuda.get_device_name(0)}: export / install of one state, plain arena vs MXINT8 arena, {rounds} rounds "
    f"after {WARM} warm-up rounds, forms alternating, HIP events, median (min) in microseconds; 'call' = as one host thread issues it, "
    f"'device' = with the three launches already queued behind a fill")
for name in ("7.2B", "13.3B"):
    L, C = CONFIGS[name]
    H = C // 64
    g = torch.Generator(device=dev).manual_seed(1)
    pool = [torch.randn((L, 2, SLOTS, C), device=dev, generator=g).half(),
            (torch.randn((L, SLOTS, H, 64, 64), device=dev, generator=g) * 0.3).half(), torch.arange(SLOTS, dtype=torch.int32, device=dev)]
    arenas = {"plain": HbmStateArena(L, C, ROWS, dev), "mxint8": HbmStateArena(L, C, ROWS, dev, wkv_format="mxint8")}
    refs = {k: [a.export_slot(pool, r % SLOTS) for r in range(ROWS)] for k, a in arenas.items()}       # every row filled once
    t = {(k, op): [] for k in arenas for op in ("export", "install", "export device", "install device")}
    for it in range(WARM + 2 * rounds):
        fill = it >= WARM and (it - WARM) % 2 == 1
        sfx = " device" if fill else ""
        for k, a in arenas.items():
            r = it % ROWS
            refs[k][r].release()                                       # the row goes back to the free list ...
            box = {}

            def export(k=k, a=a, it=it, box=box):
                box["ref"] = a.export_slot(pool, (it * 5 + 1) % SLOTS)  # ... and is the one this export takes

            us = timed(export, fill)
            refs[k][r] = box["ref"]
            if it >= WARM:
                t[(k, "export" + sfx)].append(us)
        for k, a in arenas.items():
            ref = refs[k][(it + 7) % ROWS]
            us = timed(lambda ref=ref, it=it: ref.install_into(pool, (it * 3 + 2) % SLOTS), fill)
            if it >= WARM:
                t[(k, "install" + sfx)].append(us)
    torch.cuda.synchronize()
    say(f"{name} (L={L}, C={C}, H={H}):")
    for k, a in arenas.items():
        say(f"  {k:7s} {a.bytes_per_state / 1e6:7.3f} MB per state, {int(100e9 // a.bytes_per_state)} rows per 100 GB "
            f"(head states {a.wkv[0].numel() * a.wkv.element_size() / 1e6:.3f} MB)")
    for op in ("export", "install", "export device", "install device"):
        mp, mq = statistics.median(t[("plain", op)]), statistics.median(t[("mxint8", op)])
        moved_p = 2 * arenas["plain"].bytes_per_state
        moved_q = arenas["plain"].bytes_per_state + arenas["mxint8"].bytes_per_state
        say(f"  {op:14s} plain {mp:8.1f} ({min(t[('plain', op)]):8.1f}) us = {moved_p / mp / 1e6:6.2f} TB/s moved;  "
            f"mxint8 {mq:8.1f} ({min(t[('mxint8', op)]):8.1f}) us = {moved_q / mq / 1e6:6.2f} TB/s moved;  mxint8 / plain = {mq / mp:.3f}")
    del pool, arenas, refs
    torch.cuda.empty_cache()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
