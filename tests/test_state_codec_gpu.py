"""GPU: the MXINT8 state codec kernels against the host codec bit for bit (csrc/state_codec.hip, ops.state_pack / state_unpack),
the packed HbmStateArena on the device, a worker whose prefix hit comes out of a packed arena, and process mode with every hit
installed out of the OTHER process's packed arena.  The host codec itself is held to its definition in test_state_codec_cpu.py."""
import asyncio
import os
import queue
import types

import numpy as np
import pytest
import torch

import state_codec_cases as cases

pytestmark = pytest.mark.gpu
G = cases.G
SENT16, SENT8 = 0x5A5B, 0xC3          # what surrounds the targets: a finite binary16 pattern, a byte that is no scale of the inputs


@pytest.fixture(scope="module")
def reference():
    """Every input head, its packed form and its round trip by the HOST codec -- computed once, read by every test."""
    from chirrup_amd import quant

    x = torch.from_numpy(cases.all_inputs())
    p = quant.pack_state_mxint8(x)
    return types.SimpleNamespace(x=x, packed=p, tilde=quant.unpack_state_mxint8(p))


def _i16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape,slots", [((1, 1, 1), (0,)), ((2, 3, 2), (1,)), ((3, 5, 12), (0, 4))], ids=["1x1x1", "2x3x2_mid", "3x5x12_ends"])
def test_kernels_equal_the_host_codec_bit_for_bit(reference, shape, slots):
    """Both directions, every input family (all finite binary16 patterns with random partners, the scale rule's boundary blocks,
    zero / subnormal-only / 65504 / non-finite blocks, the fixture states) at every shape, walked through the target slot L * H
    heads at a time (314, 79 and 9 rounds of two launches);
    the pool and the packed buffer are full of sentinel bytes and every byte outside the target slot or row must stay as it was."""
    from chirrup_amd import ops

    L, S, H = shape
    n = L * H
    x, packed, tilde = reference.x, reference.packed, reference.tilde
    assert x.shape[0] == 62 + 4 + 248                       # all finite patterns, the special heads, the fixture states
    rounds = 0
    for k, lo in enumerate(range(0, len(x), n)):
        idx = torch.arange(lo, lo + n) % len(x)
        slot = slots[k % len(slots)]
        # pack: slot -> row 1 of a three-row buffer
        pool = torch.full((L, S, H, 64, 64), SENT16, dtype=torch.int16).view(torch.float16)
        pool[:, slot] = x[idx].reshape(L, H, 64, 64)
        d_pool = pool.cuda()
        buf = torch.full((3, L, H, 4224), SENT8, dtype=torch.uint8, device="cuda")
        ops.state_pack(d_pool, slot, buf[1])
        got = buf.cpu()
        assert torch.equal(got[1], packed[idx].reshape(L, H, 4224)), (shape, slot, lo)
        assert bool((got[0] == SENT8).all()) and bool((got[2] == SENT8).all())
        assert torch.equal(_i16(d_pool.cpu()), _i16(pool))                      # the table is only read
        # unpack: row 1 -> slot of a table full of sentinels
        d_out = torch.full((L, S, H, 64, 64), SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
        src = torch.full((3, L, H, 4224), SENT8, dtype=torch.uint8)
        src[1] = packed[idx].reshape(L, H, 4224)
        d_src = src.cuda()
        ops.state_unpack(d_src[1], d_out, slot)
        out = d_out.cpu()
        assert torch.equal(_i16(out[:, slot]), _i16(tilde[idx].reshape(L, H, 64, 64))), (shape, slot, lo)
        others = [s for s in range(S) if s != slot]
        assert bool((_i16(out[:, others]) == SENT16).all())
        assert torch.equal(d_src.cpu(), src)                                    # the row is only read
        rounds += 1
    assert rounds == -(-len(x) // n)


def test_unpack_reads_every_code_and_exponent_exactly():
    """All 255 codes x 34 exponents and the 0xFF scale straight into the unpack kernel: equal to the host codec's values."""
    from chirrup_amd import ops, quant

    b = np.arange(3 * 128)                                   # block b: scale number (b // 8) % 35, codes 32 * (b % 8) + j - 127
    idx = 32 * (b % 8)[:, None] + np.arange(32)[None, :]
    codes = np.where(idx < 255, idx - 127, 0).astype(np.int8)
    scales = (b // 8) % 35 + 109
    scales[scales == 109 + 34] = 0xFF
    assert len({(int(c), int(s)) for c, s in zip(codes.reshape(-1), np.repeat(scales, 32))}) == 255 * 35
    p = np.concatenate([codes.view(np.uint8).reshape(3, 4096), scales.astype(np.uint8).reshape(3, 128)], -1)
    host = torch.from_numpy(p).reshape(3, 1, 4224)
    out = torch.zeros((3, 2, 1, 64, 64), dtype=torch.float16, device="cuda")
    ops.state_unpack(host.cuda(), out, 1)
    assert torch.equal(_i16(out[:, 1].cpu()), _i16(quant.unpack_state_mxint8(host)))
    assert not bool(out[:, 0].any())


def test_ops_refuse_bad_arguments_on_the_device():
    from chirrup_amd import ChirrupAmdError, ops

    pool = torch.zeros((2, 3, 2, 64, 64), dtype=torch.float16, device="cuda")
    row = torch.zeros((2, 2, 4224), dtype=torch.uint8, device="cuda")
    for args in ((pool, 3, row), (pool, -1, row), (pool, 0, row.cpu()), (pool.float(), 0, row), (pool, 0, row[:1]),
                 (pool.transpose(0, 1), 0, row), (pool, 0, torch.zeros((2, 2, 4225), dtype=torch.uint8, device="cuda")[..., :4224])):
        with pytest.raises(ChirrupAmdError):
            ops.state_pack(*args)
        with pytest.raises(ChirrupAmdError):
            ops.state_unpack(args[2], args[0], args[1])


def test_device_arena_export_then_install_gives_the_host_round_trip(reference):
    from chirrup_amd import quant
    from chirrup_amd.state_cache import HbmStateArena

    L, C, S = 3, 768, 4
    H = C // 64
    arena = HbmStateArena(L, C, capacity=2, device="cuda:0", wkv_format="mxint8")
    assert arena.wkv.dtype == torch.uint8 and tuple(arena.wkv.shape) == (2, L, H, 4224) and arena.wkv.is_cuda
    g = torch.Generator().manual_seed(3)
    heads = reference.x[torch.randperm(len(reference.x), generator=g)[: L * S * H]].reshape(L, S, H, 64, 64)
    pool = [torch.randn((L, 2, S, C), generator=g).half().cuda(), heads.cuda(), torch.tensor([3, 5, 8, 13], dtype=torch.int32).cuda()]
    before = [t.clone() for t in pool]
    ref = arena.export_slot(pool, 2)
    want = quant.roundtrip_state_mxint8(heads[:, 2])
    got = ref.tensors()
    assert torch.equal(_i16(got[1][:, 0].cpu()), _i16(want)) and torch.equal(_i16(got[0][:, :, 0]), _i16(before[0][:, :, 2])) and int(got[2]) == 8
    ref.install_into(pool, 0)
    torch.cuda.synchronize()
    assert torch.equal(_i16(pool[1][:, 0].cpu()), _i16(want))                                  # S~, bit for bit
    assert torch.equal(_i16(pool[0][:, :, 0]), _i16(before[0][:, :, 2])) and int(pool[2][0]) == 8      # shift and elapsed: the source's bits
    for s in (1, 2, 3):
        assert torch.equal(_i16(pool[1][:, s]), _i16(before[1][:, s])) and torch.equal(_i16(pool[0][:, :, s]), _i16(before[0][:, :, s]))
    assert pool[2].tolist() == [8, 5, 8, 13]
    ref.release()
    row = arena.put([before[0][:, :, [1]].cpu(), heads[:, [1]], torch.tensor([5], dtype=torch.int32)])     # host tensors into the device arena
    assert torch.equal(_i16(arena.get(row)[1].cpu()), _i16(quant.roundtrip_state_mxint8(heads[:, [1]])))
    assert arena.bytes_per_state == L * 2 * C * 2 + L * H * 4224 + 4


# ---------------------------------------------------------------------------------------------------------------- the worker
class _Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "".join(chr(65 + i % 26) for i in ids)


class _Sink:
    def __init__(self):
        self.items = []

    def put_nowait(self, x):
        self.items.append(x)


def _tiny_model():
    from chirrup_amd.rwkv7 import RWKV_x070

    d = np.load(os.path.join(G, "model_L2_C128.npz"))
    zd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}
    return RWKV_x070(types.SimpleNamespace(vocab_size=320, head_size=64, MODEL_NAME="unused"), state_dict=zd, device="cuda:0")


@pytest.fixture(scope="module")
def tiny_model():
    return _tiny_model()


CASES = [(40, 3, 3), (13, 1, 4), (101, 3, 5), (230, 2, 6)]          # prompt length, cache_prefill_padding, seed


@pytest.mark.parametrize("plen,pad,seed", CASES, ids=[f"len{c[0]}_pad{c[1]}" for c in CASES])
def test_a_hit_on_a_packed_arena_continues_like_a_request_given_the_round_trip(tiny_model, plen, pad, seed):
    """Greedy, return_logits.  A prefix is cached through a packed arena and hit: ids equal and logits bit-identical to a request
    handed state=[shift, S~, elapsed], S~ the HOST round trip of what a plain arena exports for the same prefix.  Also printed (not
    bounded): how far the first continuation logits after the packed hit are from those after the plain hit."""
    from chirrup_amd import quant
    from chirrup_amd.core_structure import ModelLoadConfig, Task
    from chirrup_amd.state_cache import ArenaRef, HbmStateArena, SimpleStateCache
    from chirrup_amd.worker import Worker

    m = tiny_model
    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=320, head_size=64)
    prompt = np.random.default_rng(seed).integers(1, 320, plen).tolist()
    mk = lambda toks, state=None, **kw: Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(toks),
                                             state=state, temperature=0.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0,
                                             stop_tokens=[], max_tokens=8, return_logits=True, **kw)

    def serve(fmt):
        arena = HbmStateArena.for_model(m, capacity=3, wkv_format=fmt)
        cache = SimpleStateCache(max_size=2, arena=arena)
        tq = queue.Queue()
        w = Worker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=4, model=m, tokenizer=_Tok(), state_arena=arena)
        w._init_worker()

        def run(task):
            tq.put(task)
            for _ in range(2000):
                if not w.step():
                    break
            items = [x[1] for x in task.output_queue.items if x[0] == "token_generated"]
            assert len(items) == 8
            return [p[0] for p in items], [p[2] for p in items]

        t1 = mk(prompt, cache_prefill=True, cache_prefill_padding=pad)
        run(t1)
        ex = [x[1] for x in t1.output_queue.items if x[0] == "cache_prefill"]
        assert len(ex) == 1 and isinstance(ex[0]["state"], ArenaRef)
        seen = tuple(ex[0]["prefilled_tokens"])
        assert len(seen) == plen - pad
        exported = ex[0]["state"].tensors()
        cache.cache(seen, ex[0]["state"])
        return arena, cache, run, seen, exported

    arena_p, cache_p, run_p, seen, exported_plain = serve(None)
    s_tilde = quant.roundtrip_state_mxint8(exported_plain[1].cpu())
    assert not torch.equal(_i16(s_tilde), _i16(exported_plain[1].cpu()))          # the format does round this state
    # the reference request: tensors in, no arena involved in its install
    want_ids, want_lg = run_p(mk(prompt[len(seen):], state=[exported_plain[0], s_tilde.cuda(), exported_plain[2]]))
    rest, hit, n = cache_p.check(list(prompt))
    plain_ids, plain_lg = run_p(mk(rest, state=hit))
    # the packed arena
    arena_q, cache_q, run_q, seen_q, exported_packed = serve("mxint8")
    assert seen_q == seen and arena_q.wkv.dtype == torch.uint8
    assert torch.equal(_i16(exported_packed[1].cpu()), _i16(s_tilde))              # what the packed arena holds IS the host round trip
    assert torch.equal(_i16(exported_packed[0]), _i16(exported_plain[0])) and torch.equal(exported_packed[2], exported_plain[2])
    rest, hit, n = cache_q.check(list(prompt))
    assert n == len(seen) and rest == prompt[n:] and isinstance(hit, ArenaRef)
    got_ids, got_lg = run_q(mk(rest, state=hit))
    assert not hit._live and arena_q.free_rows == 2
    assert got_ids == want_ids
    for a, b in zip(got_lg, want_lg):
        assert torch.equal(_i16(a), _i16(b))                                       # bit-identical logits, every step
    # recorded, not barred: the first continuation logits, packed hit vs plain hit, in units of the logit scale (their standard
    # deviation over the vocabulary); an untrained random-weight model, so this says nothing about a trained one
    a, b = got_lg[0].double().flatten(), plain_lg[0].double().flatten()
    scale = float(b.std())
    print(f"packed vs plain hit, prompt {plen} pad {pad}: first logits max |d| = {float((a - b).abs().max()):.4e} "
          f"= {float((a - b).abs().max()) / scale:.4e} x std(logits) ({scale:.3f}), rms {float((a - b).pow(2).mean().sqrt()) / scale:.4e} x std; "
          f"ids equal for {next((i for i, (u, v) in enumerate(zip(got_ids, plain_ids)) if u != v), 8)} of 8 tokens")


# ---------------------------------------------------------------------------------------------------------------- process mode
def test_process_mode_installs_every_hit_out_of_the_other_process_packed_arena(tmp_path):
    """Two worker processes on cuda:0 with packed arenas, hits queued for the process that does NOT own the row ("avoid"): every
    hit is unpacked straight out of the owner's arena through its IPC handle, is counted as a peer install, and gives the ids of
    the same requests served by one thread-mode worker with a packed arena."""
    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.engine_core import AsyncEngineCore
    from chirrup_amd.remote_arena import RemoteStateRef
    from chirrup_amd.state_cache import ArenaRef, SimpleStateCache

    d = np.load(os.path.join(G, "model_L2_C128.npz"))
    zd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}
    ckpt = os.path.join(tmp_path, "tiny.pth")
    torch.save(zd, ckpt)
    vocab = os.path.join(G, "mini_vocab.txt")
    kw = dict(temperature=0.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, stop_tokens=[])
    texts = ["abc abc abc abc abc abc abc abc", "the quick brown fox jumps over the lazy dog"]
    cfg = ModelLoadConfig(model_path=ckpt, vocab_path=vocab, vocab_size=320, head_size=64)

    async def run(mode):
        if mode == "process":
            eng = AsyncEngineCore(worker_mode="process", state_arena_rows=4, state_arena_format="mxint8", prefix_affinity="avoid",
                                  gpu_ids=[0, 0])
            await asyncio.wait_for(eng.init(worker_num=2, model_config=cfg, batch_size=4), 300)
            arena, handle = eng.state_arena, RemoteStateRef
        else:
            eng = AsyncEngineCore(worker_kwargs=dict(state_arena_rows=4, state_arena_format="mxint8"))
            await asyncio.wait_for(eng.init(worker_num=1, model_config=cfg, batch_size=4), 300)
            arena, handle = None, ArenaRef                 # the worker thread builds its arena after it reports "loaded"
        cache, first, resumed = None, {}, {}
        for text in texts:
            toks = eng.tokenizer.encode(text)
            c = eng.completion("", prefill_tokens=list(toks), max_tokens=8, cache_prefill=True, cache_prefill_padding=2, **kw)
            evs = [ev async for ev in c]
            hit = [e[1] for e in evs if e[0] == "cache_prefill"]
            assert len(hit) == 1 and isinstance(hit[0]["state"], handle)
            if arena is None:
                arena = hit[0]["state"].arena
                assert arena is eng.workers[0].state_arena and arena.wkv_format == "mxint8" and arena.wkv.dtype == torch.uint8
            cache = cache or SimpleStateCache(max_size=2, arena=arena)
            cache.cache(hit[0]["prefilled_tokens"], hit[0]["state"])
            first[text] = [e[1] for e in evs if e[0] == "token"]
        for _ in range(2):
            cs = []
            for text in texts * 2:
                toks = eng.tokenizer.encode(text)
                rest, state, n_hit = cache.check(list(toks))
                assert isinstance(state, handle) and n_hit == len(toks) - 2
                cs.append((text, eng.completion("", prefill_tokens=rest, state=state, max_tokens=8, **kw)))
            for text, c in cs:
                ids = [ev[1] async for ev in c if ev[0] == "token"]
                assert resumed.setdefault(text, ids) == ids                       # every hit on a prefix gives the same ids
        inst = dict(eng._router.installs) if mode == "process" else None
        eng.shutdown()
        return first, resumed, inst

    first_t, resumed_t, _ = asyncio.run(run("thread"))
    first_p, resumed_p, inst = asyncio.run(run("process"))
    print("installs", inst, "resumed", resumed_p, "uncached", first_p)
    assert first_p == first_t
    assert resumed_p == resumed_t                                                  # the thread-mode packed run's ids
    assert inst == {"local": 0, "peer": 8}                                         # all 8 hits came out of the OTHER process's arena
