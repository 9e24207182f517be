"""The MXINT8 state codec on the host (chirrup_amd.quant.pack_state_mxint8 / unpack_state_mxint8), the packed HbmStateArena on
CPU tensors, a PeerArenas rehearsal over shared memory, and the C ABI / resource report of the two kernels.  The codec is held
to tests/state_codec_cases.py, which writes the format down a second time from its definition.  No GPU."""
import ctypes
import os
import queue
import shutil

import numpy as np
import pytest
import torch

import state_codec_cases as cases
from test_kernel_budget_cpu import HIPCC, _report

from chirrup_amd import quant
from chirrup_amd.state_cache import ArenaRef, HbmStateArena, SimpleStateCache


def _pack(x16: np.ndarray) -> np.ndarray:
    return quant.pack_state_mxint8(torch.from_numpy(np.ascontiguousarray(x16))).numpy()


def _unpack(p: np.ndarray) -> np.ndarray:
    return quant.unpack_state_mxint8(torch.from_numpy(np.ascontiguousarray(p))).numpy()


def _head_with_block(block: np.ndarray, at: int = 0) -> np.ndarray:
    h = np.zeros((128, 32), np.float16)
    h[at] = block
    return h.reshape(64, 64)


# ---------------------------------------------------------------------------------------------------------------- the scale rule
def test_scale_rule_for_every_finite_amax():
    """Every non-negative finite binary16 value as a block's amax: the exponent equals the definition's (smallest e with
    amax <= 127 * 2^(e-6), held to [-18, 15]), through mxint8_block_exponent and through the scale byte pack() writes."""
    amax = np.arange(0x7C00, dtype=np.uint16).view(np.float16)
    want = cases.exponent_by_definition(amax.astype(np.float64))
    assert want.min() == -18 and want.max() == 15 and want[0] == -18
    got = quant.mxint8_block_exponent(torch.from_numpy(amax)).numpy()
    assert np.array_equal(got, want)
    # the same through pack(): one block per value, the amax at a varying position with a varying sign
    blocks = np.zeros((0x7C00, 32), np.float16)
    pos = np.arange(0x7C00) % 32
    blocks[np.arange(0x7C00), pos] = np.where(np.arange(0x7C00) % 3 == 0, -amax, amax)
    p = _pack(blocks.reshape(-1, 64, 64))
    assert np.array_equal(p[:, 4096:].reshape(-1).astype(np.int64) - 127, want)
    # f * 2^p form of the rule: e = p when f <= 127/64, else p + 1
    f, p2 = np.frexp(amax[1:].astype(np.float64))                    # amax = f * 2^p2, f in [0.5, 1)
    rule = np.clip(np.where(2 * f <= 127 / 64, p2 - 1, p2), -18, 15)
    assert np.array_equal(rule, want[1:])


def test_scale_rule_at_and_around_every_threshold():
    for e in range(cases.E_MIN, cases.E_MAX + 1):
        t = np.float16(127.0 * 2.0 ** (e - 6))
        assert float(t) == 127.0 * 2.0 ** (e - 6)
        below, above = np.nextafter(t, np.float16(0)), np.nextafter(t, np.float16(np.inf))
        got = quant.mxint8_block_exponent(torch.from_numpy(np.array([below, t, above]))).tolist()
        assert float(below) > 127.0 * 2.0 ** (e - 7)                  # one binary16 ulp below a threshold is still above the previous one
        assert got == [e, e, min(e + 1, cases.E_MAX)], (e, got)


# ---------------------------------------------------------------------------------------------------------------- round trip
def test_pack_of_unpack_is_the_identity_for_every_code_and_exponent():
    """All 255 codes x 34 exponents: a block that holds a 127 keeps its exponent, so the packed bytes come back unchanged, and
    every decoded value is exactly code * 2^(e-6) as a binary16 number."""
    codes = np.arange(-127, 128, dtype=np.int64)
    blocks_c, blocks_s = [], []
    for e in range(cases.E_MIN, cases.E_MAX + 1):
        for i in range(0, 255, 31):
            c = np.zeros(32, np.int64)
            chunk = codes[i: i + 31]
            c[0], c[1: 1 + len(chunk)] = (127 if (i // 31) % 2 else -127), chunk
            blocks_c.append(c)
            blocks_s.append(e + 127)
    n = len(blocks_c)
    n_heads = -(-n // 128)
    c = np.zeros((n_heads * 128, 32), np.int8)
    s = np.full((n_heads * 128,), 127 + cases.E_MIN, np.uint8)       # the padding blocks are zero blocks: e = -18
    c[:n], s[:n] = np.array(blocks_c, np.int8), np.array(blocks_s, np.uint8)
    packed = np.concatenate([c.view(np.uint8).reshape(n_heads, 4096), s.reshape(n_heads, 128)], -1)
    x = _unpack(packed)
    want = c.astype(np.float64) * 2.0 ** (s.astype(np.int64) - 133)[:, None]
    assert np.array_equal(x.reshape(-1, 32).astype(np.float64), want)           # exact: nothing was rounded
    assert not np.signbit(x[x == 0]).any()
    assert np.array_equal(cases.bits(x), cases.bits(cases.unpack_by_definition(packed)))
    assert np.array_equal(_pack(x), packed)
    seen = {(int(cc), int(ss)) for cc, ss in zip(c[:n].reshape(-1), np.repeat(s[:n], 32))}
    assert all((int(k), e + 127) in seen for k in codes for e in range(cases.E_MIN, cases.E_MAX + 1))


def test_host_codec_equals_the_definition_on_every_input_family():
    x = cases.all_inputs()
    p = _pack(x)
    assert np.array_equal(p, cases.pack_by_definition(x))
    assert np.array_equal(cases.bits(_unpack(p)), cases.bits(cases.unpack_by_definition(p)))
    assert not (p[..., :4096] == 0x80).any()                        # -128 is never written
    assert np.array_equal(_pack(_unpack(p)), p)                     # a second trip changes nothing


# ---------------------------------------------------------------------------------------------------------------- special blocks
def test_special_blocks():
    def trip(block):
        p = _pack(_head_with_block(np.asarray(block, np.float16)))
        return p[:32].view(np.int8).tolist(), int(p[4096]), _unpack(p).reshape(128, 32)[0]

    # ties to the even integer: e = 6 (amax 100), so the code is RNE(x)
    c, s, _ = trip([100, 0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 63.5, -126.5] + [0] * 22)
    assert s == 133 and c[:10] == [100, 0, 2, 2, 4, 0, -2, -2, 64, -126]
    # the zero block, with either sign of zero: e = -18, codes 0, +0 back
    for z in (0.0, -0.0):
        c, s, x = trip([z] * 32)
        assert s == 109 and c == [0] * 32 and not cases.bits(x).any()
    c, s, x = trip([-0.0] + [1.0] * 31)
    assert c[0] == 0 and cases.bits(x)[0] == 0                      # -0 packs to code 0
    # 2^-24, the smallest subnormal, alone: e = -18, code 1, exact
    c, s, x = trip([2.0 ** -24] + [0] * 31)
    assert s == 109 and c[0] == 1 and float(x[0]) == 2.0 ** -24
    c, s, x = trip([-1023 * 2.0 ** -24, 5 * 2.0 ** -24] + [0] * 30)      # subnormals only: amax 1023 * 2^-24 <= 127 * 2^-17
    assert s == 127 - 14 and c[:2] == [-64, 0] and x[:2].astype(np.float64).tolist() == [-2.0 ** -14, 0.0]      # -63.94 -> -64, 0.31 -> 0
    # 65504 saturates to 65024 (the clamp at e = 15), both signs
    c, s, x = trip([65504, -65504, 65024, 256] + [0] * 28)
    assert s == 142 and c[:4] == [127, -127, 127, 0] and x[:4].astype(np.float64).tolist() == [65024.0, -65024.0, 65024.0, 0.0]
    c, s, x = trip([65504, 768] + [0] * 30)
    assert c[1] == 2 and float(x[1]) == 1024.0                      # 1.5 -> 2 (even)
    # a NaN or an infinity poisons its block, and only its block
    for bad in (np.nan, np.inf, -np.inf):
        h = np.ones((128, 32), np.float16)
        h[5, 17] = bad
        p = _pack(h.reshape(64, 64))
        assert p[4096 + 5] == 0xFF and not p[5 * 32: 6 * 32].any()
        x = _unpack(p).reshape(128, 32)
        assert (cases.bits(x[5]) == 0x7E00).all()
        assert np.array_equal(np.delete(x, 5, 0), np.delete(h, 5, 0)) and (np.delete(p[4096:], 5) == 127).all()


# ---------------------------------------------------------------------------------------------------------------- the error bound
def test_error_bound_on_random_blocks():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((64 * 128, 32)) * 2.0 ** rng.integers(-20, 14, (64 * 128, 1))).astype(np.float16)
    p = _pack(x.reshape(-1, 64, 64))
    y = _unpack(p).reshape(-1, 32).astype(np.float64)
    e = p[:, 4096:].reshape(-1).astype(np.int64) - 127
    amax = np.abs(x.astype(np.float64)).max(-1)
    err = np.abs(x.astype(np.float64) - y).max(-1)
    assert e.min() == -18 and e.max() >= 13 and (e < 15).all()
    assert (err <= 2.0 ** (e - 7)).all()
    assert (err[amax > 0] < amax[amax > 0] / 127).all()


def test_error_bound_on_the_fixture_states():
    for name, a in cases.fixture_states():
        x = a.astype(np.float64).reshape(-1, 32)
        y = _unpack(_pack(a)).astype(np.float64).reshape(-1, 32)
        amax = np.abs(x).max(-1)
        live = amax > 0
        ratio = (np.abs(x - y).max(-1)[live] / amax[live]).max()
        rms = np.sqrt(((x - y) ** 2).sum() / (x ** 2).sum())
        print(f"{name}: max |err| / block amax {ratio:.3e}, relative RMS error {rms:.3e}")
        assert ratio < 1 / 127


# ---------------------------------------------------------------------------------------------------------------- layout
def test_layout_byte_offsets_and_determinism():
    assert quant.MXINT8_HEAD_BYTES == cases.HEAD_BYTES == 4096 + 128
    for r, c in ((0, 0), (0, 31), (0, 32), (17, 45), (63, 63)):
        h = np.zeros((64, 64), np.float16)
        h[r, c] = -3.0                                              # amax 3 = 1.5 * 2^1: e = 1, code -3 * 2^5 = -96
        p = _pack(h)
        i, b = 64 * r + c, (64 * r + c) // 32
        assert p.shape == (4224,) and p[i] == 0xA0 and p[4096 + b] == 128
        assert not np.delete(p[:4096], i).any() and (np.delete(p[4096:], b) == 109).all()
    x = torch.from_numpy(cases.special_heads()).reshape(2, 2, 64, 64)
    p = quant.pack_state_mxint8(x)
    assert p.shape == (2, 2, 4224) and p.dtype == torch.uint8 and p.is_contiguous()
    assert torch.equal(p, quant.pack_state_mxint8(x.clone())) and torch.equal(p[1, 0], quant.pack_state_mxint8(x[1, 0]))
    assert torch.equal(quant.pack_state_mxint8(x.transpose(0, 1)), p.transpose(0, 1))          # strided input
    assert quant.unpack_state_mxint8(p).shape == (2, 2, 64, 64)
    for bad in (x.float(), x.reshape(2, 2, 4096), x[..., :32]):
        with pytest.raises(ValueError):
            quant.pack_state_mxint8(bad)
    for bad in (p[..., :4096], p.to(torch.int8)):
        with pytest.raises(ValueError):
            quant.unpack_state_mxint8(bad)


# ---------------------------------------------------------------------------------------------------------------- the arena, on the host
L_, C_, S_ = 2, 128, 3


def _pool(seed=0):
    """A worker's state tables on the CPU, every slot different: [L, 2, S, C], [L, S, H, 64, 64], [S]."""
    g = torch.Generator().manual_seed(seed)
    heads = np.concatenate([cases.special_heads(seed + 2), cases.all_finite_patterns_heads(seed + 2)[: L_ * S_ * 2 - 4]], 0)
    heads = torch.from_numpy(heads).reshape(L_, S_, 2, 64, 64).clone()
    return [torch.randn((L_, 2, S_, C_), generator=g).half(), heads, torch.tensor([7, 11, 13], dtype=torch.int32)]


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def test_packed_host_arena_export_install_get_put_and_bookkeeping():
    arena = HbmStateArena(L_, C_, capacity=3, device="cpu", wkv_format="mxint8")
    plain = HbmStateArena(L_, C_, capacity=3, device="cpu")
    assert arena.wkv.dtype == torch.uint8 and tuple(arena.wkv.shape) == (3, L_, 2, 4224) and arena.wkv_format == "mxint8"
    assert tuple(arena.shift.shape) == (3, L_, 2, C_) and arena.shift.dtype == torch.float16 and arena.elapsed.dtype == torch.int32
    assert arena.bytes_per_state == L_ * 2 * C_ * 2 + L_ * 2 * 4224 + 4
    assert plain.bytes_per_state == L_ * 2 * C_ * 2 + L_ * 2 * 8192 + 4
    pool = _pool()
    tilde = quant.roundtrip_state_mxint8(pool[1])
    assert not _same_bits(tilde, pool[1])                           # the round trip is not the identity on this input
    before = [t.clone() for t in pool]
    ref = arena.export_slot(pool, 1)
    assert isinstance(ref, ArenaRef) and arena.free_rows == 2 and all(_same_bits(a, b) for a, b in zip(pool[:2], before))
    assert torch.equal(arena.wkv[ref.row], quant.pack_state_mxint8(pool[1][:, 1]))
    got = ref.tensors()                                             # binary16 in the reference's layout
    assert [tuple(t.shape) for t in got] == [(L_, 2, 1, C_), (L_, 1, 2, 64, 64), (1,)] and got[1].dtype == torch.float16
    assert _same_bits(got[1][:, 0], tilde[:, 1]) and _same_bits(got[0][:, :, 0], pool[0][:, :, 1]) and int(got[2]) == 11
    dst = _pool(5)
    keep = [t.clone() for t in dst]
    ref.install_into(dst, 2)
    assert _same_bits(dst[1][:, 2], tilde[:, 1])                    # S~, bit for bit
    assert _same_bits(dst[0][:, :, 2], pool[0][:, :, 1]) and int(dst[2][2]) == 11      # shift and elapsed unchanged by the format
    for s in (0, 1):                                                # the other slots are untouched
        assert _same_bits(dst[1][:, s], keep[1][:, s]) and _same_bits(dst[0][:, :, s], keep[0][:, :, s]) and dst[2][s] == keep[2][s]
    # an unadopted export goes back on release; an adopted one lives until the cache gives it up AND the last pin is gone
    ref.release()
    assert arena.free_rows == 3
    cache = SimpleStateCache(max_size=2, arena=arena)
    cache.cache((1, 2, 3), arena.export_slot(pool, 0))
    assert arena.free_rows == 2
    _, hit, n = cache.check([1, 2, 3, 4])
    assert n == 3 and isinstance(hit, ArenaRef)
    cache.remove([1, 2, 3])
    assert arena.free_rows == 2                                     # doomed, still pinned by the hit
    dst2 = _pool(6)
    hit.install_into(dst2, 0)
    assert _same_bits(dst2[1][:, 0], tilde[:, 0])
    hit.release()
    assert arena.free_rows == 3
    # put: tensors in the exported layout, packed on the way in; get gives the round trip
    state = [pool[0][:, :, [2]], pool[1][:, [2]], pool[2][[2]]]
    row = arena.put(state)
    back = arena.get(row)
    assert _same_bits(back[1], tilde[:, [2]]) and _same_bits(back[0], state[0]) and int(back[2]) == 13
    cache.cache((9, 9), state)                                      # tensors into an arena-backed cache: put()
    assert _same_bits(cache.check([9, 9, 1])[1].tensors()[1], tilde[:, [2]])
    with pytest.raises(ValueError):
        arena.put([state[0], state[1].float(), state[2]])
    with pytest.raises(ValueError):
        arena.export_slot([pool[0], pool[1].float(), pool[2]], 0)
    assert arena.free_rows == 1                                     # the refused calls took no row


def test_packed_format_is_refused_for_other_state_shapes():
    with pytest.raises(ValueError, match="mxint8"):
        HbmStateArena(2, 128, 2, "cpu", wkv_shape=(2, 8), wkv_dtype=torch.float32, wkv_format="mxint8")     # a fake backend's state
    with pytest.raises(ValueError, match="mxint8"):
        HbmStateArena(2, 128, 2, "cpu", dtype=torch.float32, wkv_format="mxint8")
    with pytest.raises(ValueError, match="mxint8"):
        HbmStateArena(2, 128, 2, "cpu", wkv_shape=(2, 32, 64), wkv_format="mxint8")
    with pytest.raises(ValueError, match="wkv_format"):
        HbmStateArena(2, 128, 2, "cpu", wkv_format="mxfp8")


def test_worker_and_engine_pass_the_format_on():
    """The knobs: Worker(state_arena_format=) reaches the arena it builds from state_arena_rows -- with a fake backend, whose state[1]
    is not [H, 64, 64] binary16, that is the refusal -- and AsyncEngineCore(state_arena_format=) is checked and kept for its workers."""
    from test_worker_cpu import FakeModel, FakeTok, V, cpu_penalize_argmax

    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.engine_core import AsyncEngineCore
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    mk = lambda **kw: Worker("w0", [], cfg, queue.Queue(), queue.Queue(), None, batch_size=3, model=FakeModel(), tokenizer=FakeTok(),
                             penalize_argmax=cpu_penalize_argmax, state_arena_rows=2, **kw)
    w = mk()
    w._init_worker()
    assert w.state_arena.wkv_format is None and w.state_arena.wkv.dtype == w.batch_state[1].dtype
    with pytest.raises(ValueError, match="mxint8"):
        mk(state_arena_format="mxint8")._init_worker()
    assert AsyncEngineCore(state_arena_format="mxint8").state_arena_format == "mxint8" and AsyncEngineCore().state_arena_format is None
    with pytest.raises(ValueError):
        AsyncEngineCore(state_arena_format="fp8")


def test_default_arena_is_what_it_was():
    a = HbmStateArena(3, 768, capacity=2, device="cpu")
    assert a.wkv_format is None
    assert (a.shift.dtype, a.wkv.dtype, a.elapsed.dtype) == (torch.float16, torch.float16, torch.int32)
    assert (tuple(a.shift.shape), tuple(a.wkv.shape), tuple(a.elapsed.shape)) == ((2, 3, 2, 768), (2, 3, 12, 64, 64), (2,))
    assert a.bytes_per_state == (3 * 2 * 768 + 3 * 12 * 4096) * 2 + 4
    f = HbmStateArena(2, 128, 2, "cpu", dtype=torch.float32, wkv_shape=(2, 8), wkv_dtype=torch.float64)
    assert f.wkv.dtype == torch.float64 and tuple(f.wkv.shape) == (2, 2, 2, 8)
    pool = _pool()
    ref = HbmStateArena(L_, C_, 1, "cpu").export_slot(pool, 1)
    dst = _pool(5)
    ref.install_into(dst, 0)
    assert _same_bits(dst[1][:, 0], pool[1][:, 1])                  # a plain arena hands back the bits it was given
    ref.release()


# ---------------------------------------------------------------------------------------------------------------- PeerArenas rehearsal
def _peer_owner(inbox, outboxes, done):
    """The OTHER process: builds a packed host arena, publishes it (shared memory standing in for the HIP IPC handle), exports one
    slot into it and says which row."""
    from chirrup_amd.remote_arena import PeerArenas

    torch.set_num_threads(1)
    arena = HbmStateArena(L_, C_, capacity=2, device="cpu", wkv_format="mxint8")
    peers = PeerArenas("w1", inbox, outboxes)
    peers.publish(arena)
    ref = arena.export_slot(_pool(), 1)                             # after the publication: the row is written through the share
    outboxes["w0"].put(("row", ref.row))
    done.wait(60)


def test_peer_arenas_rehearsal_with_a_packed_arena_over_shared_memory():
    """remote_arena.PeerArenas.install out of ANOTHER process's packed arena: the three tensors travel once as shared-memory
    handles (uint8 wkv among them), the row is unpacked straight out of the owner's memory into this process's slot."""
    import torch.multiprocessing as mp

    from chirrup_amd.remote_arena import PeerArenas

    ctx = mp.get_context("spawn")
    q0, q1, done = ctx.Queue(), ctx.Queue(), ctx.Event()
    boxes = {"w0": q0, "w1": q1}
    p = ctx.Process(target=_peer_owner, args=(q1, boxes, done), daemon=True)
    p.start()
    try:
        mine = PeerArenas("w0", q0, boxes)
        mine.publish(HbmStateArena(L_, C_, capacity=1, device="cpu", wkv_format="mxint8"))
        items = [q0.get(timeout=120), q0.get(timeout=120)]
        row = [m[1] for m in items if m[0] == "row"][0]
        for m in items:
            if m[0] != "row":
                q0.put(m)                                           # the publication goes back for PeerArenas to pick up
        shift, wkv, elapsed = mine.tensors_of("w1", wait_s=30.0)
        assert wkv.dtype == torch.uint8 and tuple(wkv.shape) == (2, L_, 2, 4224) and wkv.is_shared()
        src, dst = _pool(), _pool(5)
        keep = [t.clone() for t in dst]
        mine.install("w1", row, dst, 0)
        assert _same_bits(dst[1][:, 0], quant.roundtrip_state_mxint8(src[1][:, 1]))
        assert _same_bits(dst[0][:, :, 0], src[0][:, :, 1]) and int(dst[2][0]) == 11
        assert _same_bits(dst[1][:, 1:], keep[1][:, 1:])
        # this process's own row takes the same path
        own = mine.local.export_slot(src, 2)
        mine.install("w0", own.row, dst, 1)
        assert _same_bits(dst[1][:, 1], quant.roundtrip_state_mxint8(src[1][:, 2]))
    finally:
        done.set()
        p.join(30)
    assert p.exitcode == 0


# ---------------------------------------------------------------------------------------------------------------- ABI and budget
def test_the_two_symbols_and_their_signatures():
    import chirrup_amd
    from chirrup_amd import lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chirrup_amd.h")).read()
    assert "int rwkv7_state_pack(int L, int S, int H, int slot, const void *wkv, void *packed, void *stream);" in header
    assert "int rwkv7_state_unpack(int L, int S, int H, int slot, const void *packed, void *wkv, void *stream);" in header
    assert "#define CHIRRUP_MXINT8_HEAD_BYTES 4224" in header
    i, vp = ctypes.c_int, ctypes.c_void_p
    for name in ("rwkv7_state_pack", "rwkv7_state_unpack"):
        assert lib.SIGNATURES[name] == (i, [i, i, i, i, vp, vp, vp])
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    L = chirrup_amd.load()
    p = ctypes.c_void_p(4096)                                       # never dereferenced: validation fails first
    for fn in (L.rwkv7_state_pack, L.rwkv7_state_unpack):
        assert fn(0, 1, 1, 0, p, p, None) == -1 and fn(1, 0, 1, 0, p, p, None) == -1 and fn(1, 1, 0, 0, p, p, None) == -1
        assert fn(1, 2, 1, 2, p, p, None) == -1 and fn(1, 2, 1, -1, p, p, None) == -1       # slot outside [0, S)
        assert fn(1, 1, 1, 0, None, p, None) == -2 and fn(1, 1, 1, 0, p, None, None) == -2
        assert fn(1, 1, 1, 0, ctypes.c_void_p(4104), p, None) == -3 and fn(1, 1, 1, 0, p, ctypes.c_void_p(4100), None) == -3


def test_ops_check_shapes_and_take_the_host_codec_for_cpu_tensors():
    from chirrup_amd import ChirrupAmdError, ops

    pool = _pool()
    row = torch.full((L_, 2, 4224), 0xAB, dtype=torch.uint8)
    ops.state_pack(pool[1], 1, row)
    assert torch.equal(row, quant.pack_state_mxint8(pool[1][:, 1]))
    out = _pool(5)[1]
    keep = out.clone()
    ops.state_unpack(row, out, 2)
    assert _same_bits(out[:, 2], quant.roundtrip_state_mxint8(pool[1][:, 1])) and _same_bits(out[:, :2], keep[:, :2])
    for args in ((pool[1], 3, row), (pool[1], -1, row), (pool[1].float(), 0, row), (pool[1], 0, row[:, :1]), (pool[1], 0, row.to(torch.int8)),
                 (pool[1].transpose(0, 1), 0, row), (pool[1][:, :, 0], 0, row), (pool[1], True, row)):
        with pytest.raises(ChirrupAmdError):
            ops.state_pack(*args)
        with pytest.raises(ChirrupAmdError):
            ops.state_unpack(args[2], args[0], args[1])


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_the_codec_kernels_use_no_scratch_and_no_lds():
    kernels = _report("state_codec.hip")
    for sub in ("state_pack_kernel", "state_unpack_kernel"):
        hits = {n: r for n, r in kernels.items() if sub in n}
        assert len(hits) == 1, f"state_codec.hip: no single kernel matching {sub}"
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0, (name, r)
