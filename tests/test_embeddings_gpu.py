"""GPU: text embeddings -- the pooling kernel bit for bit against a numpy loop, forward_slots(pool_rows=...) against the same forward
without it (bits) and against the numpy oracle's ln_out rows (bar), the worker's embedding requests on a real small model, and
engine.embed() through a process-mode engine.

Bar against the oracle (on the un-normalised mean, L-inf relative to max(1, max|want|), tests/util.parity_stats): the ceiling is 3e-3,
the bar tests/test_model_gpu.py holds the LOGITS of multi-token forwards of these models to -- ln_out is one GEMM earlier, and a mean
of rows cannot err more than its worst row.  Per case the bar is 1.25 x the error measured on an MI355X (tests/golden/
embedding_bars.json, profiles/r05_embedding_parity.txt), never above the ceiling.  The oracle's ln_out rows: oracle.rwkv7_np.
forward_seq_batch(full_output=True) on a copy of the weights whose head.weight is the C x C identity (x . I in binary32 is x)."""
import asyncio
import ctypes
import json
import os
import queue
import types

import numpy as np
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.embeddings import finish
from oracle import rwkv7_np as M
from util import parity_stats

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CEILING = 3e-3
_BARS = json.load(open(os.path.join(G, "embedding_bars.json"))) if os.path.exists(os.path.join(G, "embedding_bars.json")) else {}


def held(case, got, want):
    """Prints the measured error beside its bar, then asserts it."""
    stats = parity_stats(got, want)
    bar = min(CEILING, _BARS.get(case, CEILING))
    print(json.dumps({"case": case, "rel_linf": stats["rel_linf"], "max_abs_want": stats["max_abs_want"], "bar": bar}))
    assert stats["rel_linf"] <= bar, (case, stats["rel_linf"], bar)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- the kernel
def numpy_pool(xo, seq, t0, slot, acc_sum, acc_last, acc_count):
    """The contract: per channel sum = sum + float32(row), strictly in token order (a row of channels per numpy addition)."""
    B, T, _ = xo.shape
    for b, a, s in zip(seq, t0, slot):
        if not 0 <= b < B or not 0 <= s < acc_count.shape[0]:
            continue
        for t in range(a, T):
            acc_sum[s] = acc_sum[s] + xo[b, t].astype(np.float32)
        if a < T:
            acc_last[s] = xo[b, T - 1]
            acc_count[s] += T - a


def rows_with_specials(rng, B, T, C):
    x = (rng.standard_normal((B, T, C)) * 8).astype(np.float16)
    flat = x.reshape(-1)
    vals = np.array([-0.0, 0.0, 6e-8, -6e-8, 5.96e-8, 6.1e-5, 65504.0, -65504.0, 65504.0], np.float16)      # -0, subnormals, +-max
    at = rng.choice(flat.size, size=min(flat.size, 4 * len(vals)), replace=False)
    flat[at] = np.resize(vals, at.size)
    return x


def bits_equal(t, want):
    got = t.cpu().numpy()
    view = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16, np.dtype(np.int32): np.int32}[want.dtype]
    return np.array_equal(got.view(view), want.view(view))


@pytest.mark.parametrize("T", [1, 2, 7, 64])
@pytest.mark.parametrize("C", [64, 128, 768, 4096])
def test_pool_rows_kernel_bit_exact(C, T):
    rng = np.random.default_rng(C * 100 + T)
    B, n = 5, 9
    x = rows_with_specials(rng, B, T, C)
    x_dev = cuda(x)
    starts = [0, min(1, T), T - 1, T]
    for r in range(4):
        seq, slot = [3, 0, 4], [7, 2, 5]                    # shuffled sequences, non-contiguous slots
        t0 = [starts[(r + i) % 4] for i in range(3)]
        want = [np.full((n, C), 1234.5, np.float32), np.full((n, C), -7.25, np.float16), np.full((n,), 77, np.int32)]   # sentinels
        for s in slot:                                      # a listed slot continues its own running values
            want[0][s] = (rng.standard_normal(C) * 50).astype(np.float32)
            want[2][s] = int(rng.integers(0, 1000))
        got = [cuda(w.copy()) for w in want]
        numpy_pool(x, seq, t0, slot, *want)
        ops.pool_rows(x_dev, cuda(np.array(seq, np.int32)), cuda(np.array(t0, np.int32)), cuda(np.array(slot, np.int32)), *got)
        for g, w, name in zip(got, want, ("sum", "last", "count")):
            assert bits_equal(g, w), (name, C, T, t0)       # the unlisted rows (sentinels) included


def test_pool_rows_one_launch_equals_two_and_skips():
    rng = np.random.default_rng(7)
    C = 768
    x = rows_with_specials(rng, 2, 7, C)
    idx = lambda *v: cuda(np.array(v, np.int32))
    new = lambda: [torch.zeros((3, C), device="cuda"), torch.zeros((3, C), dtype=torch.float16, device="cuda"),
                   torch.zeros((3,), dtype=torch.int32, device="cuda")]
    one, two = new(), new()
    ops.pool_rows(cuda(x), idx(1), idx(0), idx(2), *one)
    ops.pool_rows(cuda(x[:, :3]), idx(1), idx(0), idx(2), *two)
    ops.pool_rows(cuda(x[:, 3:]), idx(1), idx(0), idx(2), *two)
    for a, b in zip(one, two):
        assert bits_equal(a, b.cpu().numpy())
    assert one[2].tolist() == [0, 0, 7]
    # a sequence or a slot out of range is skipped; n_seq = 0 launches nothing (the raw entry point: no pointer is looked at)
    before = [t.clone() for t in one]
    ops.pool_rows(cuda(x), idx(2, -1, 0), idx(0, 0, 0), idx(0, 1, 3), *one)
    L = ops._lib.load()
    assert L.rwkv7_pool_rows(0, 2, 7, C, None, None, None, None, 3, None, None, None, None) == 0
    ops.pool_rows(cuda(x), idx(), idx(), idx(), *one)
    torch.cuda.synchronize()
    for a, b in zip(one, before):
        assert torch.equal(a, b)


def test_pool_rows_error_codes():
    L = ops._lib.load()
    C = 64
    x = torch.zeros((1, 2, C + 8), dtype=torch.float16, device="cuda")
    i = torch.zeros((4,), dtype=torch.int32, device="cuda")
    s, l, c = torch.zeros((2, C + 8), device="cuda"), torch.zeros((2, C + 8), dtype=torch.float16, device="cuda"), torch.zeros((2,), dtype=torch.int32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = lambda: [1, 1, 2, C, p(x), p(i), p(i), p(i), 2, p(s), p(l), p(c), st]
    assert L.rwkv7_pool_rows(*good()) == 0
    a = good()
    a[3] = 60
    assert L.rwkv7_pool_rows(*a) == -1                       # CHIRRUP_E_SHAPE: C % 8
    for k in (4, 5, 6, 7, 9, 10, 11):
        a = good()
        a[k] = None
        assert L.rwkv7_pool_rows(*a) == -2, k                # CHIRRUP_E_NULL
    for k, t in ((4, x), (9, s), (10, l)):
        a = good()
        a[k] = p(t, 8)
        assert L.rwkv7_pool_rows(*a) == -3, k                # CHIRRUP_E_ALIGN
    torch.cuda.synchronize()
    with pytest.raises(ops._lib.ChirrupAmdError):
        ops.pool_rows(x[:, :, :60].contiguous(), i[:1], i[:1], i[:1], s[:, :60].contiguous(), l[:, :60].contiguous(), c)


# ---------------------------------------------------------------------------------------------- the model
_MODELS = {}


def synth(L, C, V=320):
    """(state dict, GPU model, oracle weights with the identity head), built once per shape and shared."""
    if (L, C) not in _MODELS:
        from chirrup_amd.rwkv7 import RWKV_x070
        from chirrup_amd.synth import make_state_dict

        sd = make_state_dict(L, C, vocab_size=V, seed=11, varied_norms=True)
        m = RWKV_x070(types.SimpleNamespace(vocab_size=V, head_size=64, MODEL_NAME="unused"), state_dict=dict(sd), device="cuda:0")
        z = M.prepare_weights({k: v.numpy() for k, v in sd.items()})
        z["head.weight"] = np.eye(C, dtype=np.float16)
        _MODELS[(L, C)] = (sd, m, z)
    return _MODELS[(L, C)]


def oracle_rows(z, L, C, tokens, state=None):
    """binary16 ln_out rows [B, T, C] of the numpy oracle (state: numpy tables, updated in place; zero without)."""
    B = len(tokens)
    if state is None:
        state = [np.zeros((L, 2, B, C), np.float16), np.zeros((L, B, C // 64, 64, 64), np.float16), np.zeros((B,), np.int32)]
    return M.forward_seq_batch(z, tokens, state, L, full_output=True)


@pytest.mark.parametrize("T", [1, 5, 12])
@pytest.mark.parametrize("L,C", [(2, 128), (3, 768)])
def test_forward_slots_pool_rows(L, C, T):
    sd, m, z = synth(L, C)
    V, B, n = 320, 3, 6
    rng = np.random.default_rng(L * 1000 + T)
    toks = rng.integers(1, V, (B, T)).tolist()
    slots = torch.tensor([4, 1, 5], dtype=torch.int32, device="cuda")
    base = m.generate_zero_state(n)
    g = torch.Generator(device="cuda").manual_seed(T)
    base[0].copy_((torch.randn(base[0].shape, generator=g, device="cuda") * 0.5).half())
    base[1].copy_((torch.randn(base[1].shape, generator=g, device="cuda") * 0.1).to(base[1].dtype))
    base[2].copy_(torch.arange(n, dtype=torch.int32) * 3)
    plain, pooled, both = ([t.clone() for t in base] for _ in range(3))
    seq, t0, slot = [2, 0, 1], [0, min(1, T - 1), 0], [7, 2, 5]
    acc = [torch.zeros((9, C), device="cuda"), torch.zeros((9, C), dtype=torch.float16, device="cuda"),
           torch.zeros((9,), dtype=torch.int32, device="cuda")]
    args = tuple(cuda(np.array(v, np.int32)) for v in (seq, t0, slot))
    lg_plain = m.forward_slots(toks, plain, slots)
    lg_pool = m.forward_slots(toks, pooled, slots, pool_rows=args + tuple(acc))
    assert torch.equal(lg_plain, lg_pool)
    for a, b in zip(plain, pooled):
        assert torch.equal(a, b)
    # combined with logit_rows: the pair that call returns without pool_rows, and the same pooled tables
    rows = torch.arange(B * T, dtype=torch.int32, device="cuda")
    acc2 = [torch.zeros_like(t) for t in acc]
    lg_rows, head_rows = m.forward_slots(toks, both, slots, logit_rows=rows, pool_rows=args + tuple(acc2))
    lg_ref, head_ref = m.forward_slots(toks, [t.clone() for t in base], slots, logit_rows=rows)
    assert torch.equal(lg_rows, lg_ref) and torch.equal(head_rows, head_ref)
    for a, b in zip(acc, acc2):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        m.forward_slots(toks, [t.clone() for t in base], slots, full_output=True, pool_rows=args + tuple(acc))
    # the pooled means against the oracle's ln_out rows (binary64 mean)
    sl = slots.long()
    st = [base[0][:, :, sl].cpu().numpy(), np.ascontiguousarray(base[1][:, sl].cpu().numpy()), base[2][sl].cpu().numpy()]
    want_rows = oracle_rows(z, L, C, toks, st).astype(np.float64)
    sums, lasts, counts = (t.cpu().numpy() for t in acc)
    for b, a, s in zip(seq, t0, slot):
        assert counts[s] == T - a
        held(f"model L{L}_C{C} T={T}", sums[s].astype(np.float64) / (T - a), want_rows[b, a:].mean(axis=0))
    assert sorted(np.nonzero(counts)[0].tolist()) == sorted(slot)


def test_pool_rows_keeps_the_plain_logits_where_the_two_exits_differ():
    """C = 2048, B = 3, T = 5: the plain exit (ln_out over the last rows, their split-K partials summed on its own) and the all-rows
    exit that logit_rows takes differ in the last binary16 place of some logits there.  A pooling forward must return the PLAIN
    call's bits, and with logit_rows the logit_rows call's."""
    sd, m, _ = synth(2, 2048)
    B, T, C = 3, 5, 2048
    toks = np.random.default_rng(T).integers(1, 320, (B, T)).tolist()
    slots = torch.arange(B, dtype=torch.int32, device="cuda")
    acc = [torch.zeros((B, C), device="cuda"), torch.zeros((B, C), dtype=torch.float16, device="cuda"),
           torch.zeros((B,), dtype=torch.int32, device="cuda")]
    args = tuple(cuda(np.array(v, np.int32)) for v in ([0, 1, 2], [0, 0, 0], [0, 1, 2]))
    pools = [m.generate_zero_state(B) for _ in range(4)]
    rows = torch.arange(B * T, dtype=torch.int32, device="cuda")
    plain = m.forward_slots(toks, pools[0], slots)
    pooled = m.forward_slots(toks, pools[1], slots, pool_rows=args + tuple(acc))
    with_rows, _ = m.forward_slots(toks, pools[2], slots, logit_rows=rows)
    both, _ = m.forward_slots(toks, pools[3], slots, logit_rows=rows, pool_rows=args + tuple(torch.zeros_like(t) for t in acc))
    assert torch.equal(plain, pooled) and torch.equal(with_rows, both)
    for p in pools[1:]:
        for a, b in zip(pools[0], p):
            assert torch.equal(a, b)
    assert acc[2].tolist() == [T] * B and torch.isfinite(acc[0]).all()


# ---------------------------------------------------------------------------------------------- the worker
class _Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "".join(chr(65 + i % 26) for i in ids)


class _Sink:
    def __init__(self):
        self.items = []

    def put_nowait(self, x):
        self.items.append(x)


def _worker(m, V, batch_size=9, chunk=8, run_ahead=True):
    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V, head_size=64)
    w = Worker("w0", [0], cfg, queue.Queue(), queue.Queue(), None, batch_size=batch_size, model=m, tokenizer=_Tok(), run_ahead=run_ahead)
    w._init_worker()
    w.max_forward_seq_len_per_forward = chunk
    return w


def _task(prompt, **kw):
    from chirrup_amd.core_structure import Task

    g = dict(temperature=0.0, top_p=0.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_decay=1.0, stop_tokens=[])
    g.update(kw)
    return Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=None, **g)


def _drain(w, tasks):
    for _ in range(3000):
        if not w.step() and all(any(k == "task_completed" for k, _ in t.output_queue.items) for t in tasks):
            return
    raise AssertionError("worker did not drain")


def _vector(task):
    (payload,) = [p for k, p in task.output_queue.items if k == "embedding"]
    return payload


_ORACLE_MEANS = {}


def oracle_mean(n):
    """binary64 mean of the oracle's ln_out rows of the n-token test prompt behind the token 0 (computed once)."""
    if n not in _ORACLE_MEANS:
        _, _, z = synth(2, 128)
        prompt = np.random.default_rng(100 + n).integers(1, 320, n).tolist()
        rows = oracle_rows(z, 2, 128, [[0] + prompt]).astype(np.float64)[0]
        _ORACLE_MEANS[n] = (prompt, rows[1:].mean(axis=0))
    return _ORACLE_MEANS[n]


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_worker_embeddings_match_oracle(run_ahead):
    sd, m, z = synth(2, 128)
    V, lens = 320, (1, 2, 9, 33)
    w = _worker(m, V, run_ahead=run_ahead)
    rng = np.random.default_rng(2)
    gens = [_task(rng.integers(1, V, n).tolist(), max_tokens=k) for n, k in ((20, 6), (5, 9))]
    raw = [_task([0] + oracle_mean(n)[0], embed="mean", embed_skip=1, embed_normalize=False) for n in lens]
    unit = [_task([0] + oracle_mean(n)[0], embed="mean", embed_skip=1) for n in lens]
    last = _task([0] + oracle_mean(9)[0], embed="last", embed_skip=1, embed_normalize=False)
    order = [gens[0]] + raw[:2] + [gens[1]] + raw[2:] + unit + [last]
    for t in order:
        w.task_queue.put(t)
    _drain(w, order)
    for n, t, u in zip(lens, raw, unit):
        p = _vector(t)
        assert p["embedding"].dtype == np.float32 and p["embedding"].shape == (128,)
        assert p["pooled_tokens"] == n and p["prompt_tokens"] == n + 1
        held(f"worker L2_C128 n={n}", p["embedding"], oracle_mean(n)[1])
        e = _vector(u)["embedding"].astype(np.float64)
        assert abs(np.sqrt((e * e).sum()) - 1.0) <= 1e-6
        assert str(t.request_status) == "FINISHED_LENGTH_CAPPED" and not t.generated_tokens
    assert np.isfinite(_vector(last)["embedding"]).all() and _vector(last)["pooled_tokens"] == 9
    for g_, k in zip(gens, (6, 9)):                          # the generating neighbours still finish with their max_tokens tokens
        assert len(g_.generated_tokens) == k and str(g_.request_status) == "FINISHED_LENGTH_CAPPED"


@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
def test_worker_same_request_twice_gives_identical_bits(run_ahead):
    sd, m, z = synth(2, 128)
    w = _worker(m, 320, batch_size=3, run_ahead=run_ahead)
    prompt = [0] + oracle_mean(33)[0]
    got = []
    for _ in range(2):                                       # one after the other, through an otherwise idle worker
        t = _task(prompt, embed="mean", embed_skip=1)
        w.task_queue.put(t)
        _drain(w, [t])
        got.append(_vector(t)["embedding"])
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    # the host's half of the same vector: finish() on the device tables is what the worker sent (slot 0, not zeroed since)
    sums, lasts, counts = (t.cpu().numpy() for t in w._emb)
    assert np.array_equal(finish(sums[0], lasts[0], counts[0], "mean", True).view(np.uint32), got[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------- process mode
def test_process_mode_embed_equals_thread_mode_worker(tmp_path):
    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.engine_core import AsyncEngineCore
    from chirrup_amd.worker import Worker

    sd, _, _ = synth(2, 128)
    ckpt = os.path.join(tmp_path, "tiny.pth")
    torch.save(sd, ckpt)
    cfg = ModelLoadConfig(model_path=ckpt, vocab_path=os.path.join(G, "mini_vocab.txt"), vocab_size=320, head_size=64)
    ids = np.random.default_rng(9).integers(1, 320, 41).tolist()

    async def run():
        eng = AsyncEngineCore(worker_mode="process")
        await asyncio.wait_for(eng.init(worker_num=1, model_config=cfg, batch_size=4), 300)
        try:
            return await asyncio.wait_for(eng.embed(prefill_tokens=ids), 120), await asyncio.wait_for(eng.embed(prefill_tokens=ids, pooling="last"), 120)
        finally:
            eng.shutdown()

    mean, last = asyncio.run(run())
    assert isinstance(mean["embedding"], np.ndarray) and mean["embedding"].dtype == np.float32
    assert mean["prompt_tokens"] == 42 and mean["pooled_tokens"] == 41
    # the thread-mode worker: the same checkpoint loaded the same way, the same input, the same chunking (one chunk of 42 tokens)
    w = Worker("w0", [0], cfg, queue.Queue(), queue.Queue(), None, batch_size=4)
    w._init_worker()
    tasks = [_task([0] + ids, embed=p, embed_skip=1, max_tokens=0) for p in ("mean", "last")]
    for t in tasks:
        w.task_queue.put(t)
        _drain(w, [t])
    for got, t in zip((mean, last), tasks):
        assert np.array_equal(got["embedding"].view(np.uint32), _vector(t)["embedding"].view(np.uint32))
