"""MXFP4 (w4a16) on the GPU: csrc/mxfp4.hip against exact references, and the ffn_dtype="mxfp4" model against the numpy oracle fed the
DEQUANTISED matrices.

Dequantisation: bit equality with quant.dequantize_mxfp4 for every code, every accepted exponent and every nibble position of a tile
image -- what settles on hardware what v_cvt_scalef32_pk_f16_fp4 does with the nibble order and the scale.
GEMM: the cases of tests/mxfp4_cases.py (the exact-sum lemma, proved per case by tests/test_mxfp4_cpu.py): ONE admissible binary16
pattern per output, every assertion is bit equality.  x is a view inside a NaN parent, codes and scales views inside 0xFF parents (0xFF
is the scale format's NaN), outputs and planes views inside sentinel parents."""
import os
import queue
import types

import numpy as np
import pytest
import torch

import gemm_ref as G
import mxfp4_cases as X
from test_gemm_exact_gpu import SENT16, SENT32, Guarded, T, note, operand, output

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tiled(case):
    """The case's weights as a TiledMxfp4, tiled from views inside 0xFF parents."""
    from chirrup_amd import ops
    from chirrup_amd.quant import Mxfp4Weight

    codes, scales = X.packed(case)
    return ops.tile_weight_mxfp4(Mxfp4Weight(Guarded(codes, np.uint8(255)).view, Guarded(scales, np.uint8(255)).view))


# ---------------------------------------------------------------------------------------------------------------------
# dequantisation

def test_dequant_every_code_exponent_and_nibble_position():
    """Four 128 x 64 tiles (two tile rows, two K-blocks).  Pass p = 0..15 puts code (i + p) % 16 at element i of every row, so every
    nibble position of a tile image sees all 16 codes; the exponent of (row, block) walks all 27 values along the rows, offset per
    block, so both k-steps of a tile and every row residue see different scales."""
    from chirrup_amd import ops, quant as Q

    M, K = 256, 128
    i = np.arange(K)[None, :] + 3 * np.arange(M)[:, None]
    eb = (np.arange(M)[:, None] + 5 * np.arange(K // 32)[None, :]) % 27 - 13
    out = output((M, K), pad_rows=2, pad_cols=8)
    n = 0
    for p in range(16):
        case = dict(codes=((i + p) % 16).astype(np.uint8), eblk=eb)
        codes, scales = X.packed(case)
        w = Q.Mxfp4Weight(T(codes), T(scales))
        tw = ops.tile_weight_mxfp4(w)
        back = Q.untile_mxfp4(tw.data, M, K)
        assert torch.equal(back.codes, w.codes) and torch.equal(back.scales, w.scales)
        want = Q.dequantize_mxfp4(Q.Mxfp4Weight(torch.from_numpy(codes), torch.from_numpy(scales))).numpy()
        assert np.array_equal(want.astype(F64), X.dequantised(case))
        out.poison()
        ops.mxfp4_dequant(tw, out=out.view)
        got = out.get()
        bad = got.view(np.uint16) != want.view(np.uint16)
        if bad.any():
            r, c = (int(a[0]) for a in np.nonzero(bad))
            raise AssertionError(f"pass {p}: {int(bad.sum())} of {bad.size} wrong; first ({r}, {c}): code {int(case['codes'][r, c])} e {int(eb[r, c // 32])} "
                                 f"got {got[r, c]!r} want {want[r, c]!r}; wrong per k % 16: {bad.reshape(M, -1, 16).sum((0, 1)).tolist()}")
        n += bad.size
    assert out.intact()
    note("mxfp4_dequant[codes x exponents x positions]", dict(n=n, bad=0))


def test_dequant_random_matrix_and_scratch_form():
    from chirrup_amd import ops, quant as Q

    rng = np.random.default_rng(2)
    w = torch.from_numpy((rng.standard_normal((256, 128)) * 2.0 ** rng.integers(-10, 6, (256, 1))).astype(F16))
    q = Q.quantize_linear_mxfp4(w)
    want = Q.dequantize_mxfp4(q).numpy()
    tw = ops.tile_weight_mxfp4(Q.Mxfp4Weight(q.codes.cuda(), q.scales.cuda()))
    out = output((256, 128))
    ops.mxfp4_dequant(tw, out=out.view)
    assert np.array_equal(out.get().view(np.uint16), want.view(np.uint16)) and out.intact()
    assert np.array_equal(ops.mxfp4_dequant(tw).cpu().numpy().view(np.uint16), want.view(np.uint16))
    flat = torch.full((256 * 128 + 64,), float(SENT16), device="cuda", dtype=torch.float16)      # the model's scratch form
    got = ops.mxfp4_dequant(tw, out=flat[:256 * 128 + 32])
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16)) and bool((flat[256 * 128:] == float(SENT16)).all())
    note("mxfp4_dequant[random 256x128]", dict(n=3 * want.size, bad=0))


def test_tile_weight_refuses_on_the_host():
    from chirrup_amd import ChirrupAmdError, ops, quant as Q

    ok = Q.quantize_linear_mxfp4(torch.ones(128, 64))
    for bad in (113, 141, 255):
        s = ok.scales.clone()
        s[77, 1] = bad
        with pytest.raises(ValueError):
            ops.tile_weight_mxfp4(Q.Mxfp4Weight(ok.codes.cuda(), s.cuda()))
    for shape in ((64, 64), (128, 96)):
        q = Q.quantize_linear_mxfp4(torch.ones(shape))
        with pytest.raises(ChirrupAmdError):
            ops.tile_weight_mxfp4(Q.Mxfp4Weight(q.codes.cuda(), q.scales.cuda()))
    with pytest.raises(ChirrupAmdError):
        ops.tile_weight_mxfp4(ok)                                                 # CPU tensors


# ---------------------------------------------------------------------------------------------------------------------
# GEMM

def run_linear(name, case, splits, K):
    """act 0 / 1 x splits 0 / 1 / 2 / 4 / 16 (where K allows) of mxfp4_linear, then every plane of mxfp4_linear_partial."""
    from chirrup_amd import ops

    M, N = case["xi"].shape[0], case["codes"].shape[0]
    q = 2.0 ** (case["ex"] + case["ew"])
    x, wt = operand(X.x_half(case)), tiled(case)
    ex = G.exact_pre(case)
    out = output((M, N))
    n = 0
    for act in (0, 1):
        lo = G.expected(case, act)[0]
        for s in (0, 1, 2, 4, 16):
            if s and (K // 64) % s:
                continue
            out.poison()
            ops.mxfp4_linear(x, wt, act=act, splits=s, out=out.view)
            G.assert_bits(out.get(), lo, lo, ex, q, f"{name} s={s} act={act}")
            n += lo.size
    assert out.intact()
    y = ops.mxfp4_linear(x, wt)                                                   # (no out given)
    G.assert_bits(y.cpu().numpy(), *G.expected(case)[:1] * 2, ex, q, f"{name} fresh out")
    room, pad = 16 * M * N, 64
    buf = torch.empty(room + 2 * pad, device="cuda", dtype=torch.float32)
    for s in tuple(splits) + (0,):
        buf.fill_(float(SENT32))
        got = ops.mxfp4_linear_partial(x, wt, s, buf[pad:pad + room])
        s_used = got.shape[0]
        assert tuple(got.shape) == (s_used, M, N) and s_used == ops.mxfp4_gemm_splits(M, N, K, s) and (s == 0 or s_used == s)
        n += G.assert_planes(got.cpu().numpy(), G.expected_planes(case, s_used), f"{name} planes s={s}")
        flat = buf.cpu().numpy()
        assert (flat[:pad] == SENT32).all() and (flat[pad + s_used * M * N:] == SENT32).all(), "written past the planes in use"
    return n


@pytest.mark.parametrize("name", list(X.CASES))
def test_mxfp4_linear_exact(name):
    M, N, K, splits = X.CASES[name]
    n = run_linear(name, X.named(name), splits, K)
    note(f"mxfp4_linear[{name}]", dict(n=n, bad=0))


@pytest.mark.parametrize("name", list(X.SCALED))
def test_mxfp4_linear_scaled(name):
    """Outputs in the binary16 subnormal range (from subnormal x), and sums past 65504 (inf)."""
    case, splits = X.scaled_named(name)
    lo = G.expected(case)[0]
    assert (np.abs(lo.astype(F64)) < 2.0 ** -14).mean() > 0.95 if name == "subnormal" else 0.05 < np.isinf(lo).mean() < 0.95
    n = run_linear(name, case, splits, case["xi"].shape[1])
    note(f"mxfp4_linear[{name}]", dict(n=n, bad=0))


def test_mxfp4_linear_extreme_exponents():
    """Block exponents -13 and +13 (scale bytes 114 and 140), mixed inside every 16-row MFMA tile."""
    from chirrup_amd import ops

    case, subs = X.extreme_case()
    M, N = case["xi"].shape[0], case["codes"].shape[0]
    x, wt = operand(X.x_half(case)), tiled(case)
    out = output((M, N))
    buf = torch.empty(4 * M * N, device="cuda", dtype=torch.float32)
    n = 0
    for act in (0, 1):
        for s in (0, 1, 2, 4):
            out.poison()
            ops.mxfp4_linear(x, wt, act=act, splits=s, out=out.view)
            got = out.get()
            for e, (cols, sub) in subs.items():
                lo = G.expected(sub, act)[0]
                G.assert_bits(got[:, cols], lo, lo, G.exact_pre(sub), 2.0 ** (sub["ex"] + sub["ew"]), f"extreme e={e} s={s} act={act}")
                n += lo.size
    for s in (1, 2, 4):
        planes = ops.mxfp4_linear_partial(x, wt, s, buf).cpu().numpy()
        for e, (cols, sub) in subs.items():
            n += G.assert_planes(planes[:, :, cols], G.expected_planes(sub, s), f"extreme e={e} planes s={s}")
    assert out.intact()
    note("mxfp4_linear[extreme exponents]", dict(n=n, bad=0))


def test_non_finite_x_stays_in_its_row():
    from chirrup_amd import ops

    name = "M17-N128-K192"
    case = X.named(name)
    x16 = X.x_half(case).copy()
    x16[5, 70], x16[11, 10] = np.nan, np.inf
    w = X.dequantised(case)
    with np.errstate(invalid="ignore", over="ignore"):
        want11 = G.h(x16[11].astype(F64) @ w.T)                       # inf * 0 = NaN, inf * w = +-inf, in binary64 as in binary32
    assert np.isnan(want11).any() and np.isinf(want11).any()
    wt = tiled(case)
    clean = np.ones(17, bool)
    clean[[5, 11]] = False
    for s in (1, 3):
        for act in (0, 1):
            lo = G.expected(case, act)[0]
            got = ops.mxfp4_linear(operand(x16), wt, act=act, splits=s).cpu().numpy()
            G.assert_bits(got[clean], lo[clean], lo[clean], name=f"clean rows s={s} act={act}")
            assert np.isnan(got[5]).all()
            w11 = G.apply_act(want11.astype(F64), act)[0]
            G.assert_bits(got[11:12], w11[None], w11[None], name=f"inf row s={s} act={act}")
    planes = ops.mxfp4_linear_partial(operand(x16), wt, 3, torch.empty(3 * 17 * 128, device="cuda", dtype=torch.float32)).cpu().numpy()
    want = G.expected_planes(case, 3)
    assert np.array_equal(planes[:, clean].view(np.uint32), want[:, clean].view(np.uint32))
    assert np.isnan(planes[1, 5]).all() and np.isfinite(planes[[0, 2], 5]).all()          # k = 70 lies in the second slice


# ---------------------------------------------------------------------------------------------------------------------
# model

def rel_linf(got, want):
    w = np.asarray(want).astype(F32)
    return float(np.abs(np.asarray(got).astype(F32) - w).max() / max(1.0, float(np.abs(w).max())))


def bar(floor):
    """tests/test_model_gpu.py's bar for the fused binary16 model: within twice a second CPU evaluation's distance (+5e-4), 5e-3 at most."""
    return min(5e-3, 2 * floor + 5e-4)


GREEDY_SEED = 5        # chosen on the CPU (oracle and CPU model alone): the oracle's top-two gap stays above twice the logit bar at all 24 steps


@pytest.fixture(scope="module")
def models(oracle):
    """The fixture model three ways on the same DEQUANTISED channel-mix matrices: the MXFP4 model on the GPU (it quantises itself), the
    numpy oracle, and this package's torch-op path on the CPU (the floor); plus the unquantised binary16 GPU model."""
    from chirrup_amd import quant as Q
    from chirrup_amd.rwkv7 import RWKV_x070
    from oracle import rwkv7_np as M

    d = np.load(os.path.join(GOLD, "model_L2_C128.npz"))
    zd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}
    zq, quantised = dict(zd), {}
    for i in range(2):
        for n in ("key", "value"):
            k = f"blocks.{i}.ffn.{n}.weight"
            quantised[k] = Q.quantize_linear_mxfp4(zd[k].to(torch.float16))      # (checkpoint layout: the Linear weight [M_out, N_in])
            zq[k] = Q.dequantize_mxfp4(quantised[k]).to(zd[k].dtype)
    z_np = M.prepare_weights({k: v.numpy() for k, v in zq.items()})
    args = lambda: types.SimpleNamespace(vocab_size=320, head_size=64, MODEL_NAME="unused")

    def wkv_cpu(B_, T_, C_, H, S, r, w, k, v, a, b, y, et, slot_idx=None):
        y.copy_(torch.from_numpy(oracle.wkv7_seq(S.numpy(), r.numpy(), w.numpy(), k.numpy(), v.numpy(), a.numpy(), b.numpy(), et.numpy())))

    return types.SimpleNamespace(
        d=d, zd=zd, quantised=quantised, z_np=z_np, M=M,
        m4=RWKV_x070(args(), state_dict=zd, device="cuda:0", ffn_dtype="mxfp4"),
        m16=RWKV_x070(args(), state_dict=zd, device="cuda:0"),
        cpu=RWKV_x070(args(), state_dict=zq, device="cpu", fused=False, wkv_impl=wkv_cpu))


def test_model_keeps_tile_images_only(models):
    from chirrup_amd import ops, quant as Q

    m4 = models.m4
    for i in range(2):
        for n, (mo, ni) in (("key", (512, 128)), ("value", (128, 512))):
            k = f"blocks.{i}.ffn.{n}.weight"
            assert k not in m4.z and isinstance(m4.z[k + ".mxfp4"], ops.TiledMxfp4) and m4.z[k + ".mxfp4"].shape == (mo, ni)
            back = Q.untile_mxfp4(m4.z[k + ".mxfp4"].data, mo, ni)
            assert np.array_equal(back.codes.cpu().numpy(), models.quantised[k].codes.numpy())           # the quantiser's bytes
            assert np.array_equal(back.scales.cpu().numpy(), models.quantised[k].scales.numpy())
        assert m4._layers[i].f_K is None and m4._layers[i].f_V is None
    assert not m4.sparse_bsz1
    groups = m4.get_gpu_parameter_groups()
    ffn16 = 2 * 2 * 512 * 128 * 2
    assert sum(g["size"] for g in models.m16.get_gpu_parameter_groups()) - sum(g["size"] for g in groups) == ffn16 - ffn16 * 17 // 64


@pytest.mark.parametrize("tag", ["b3t1", "b3t5"])
def test_model_vs_oracle_on_the_dequantised_weights(models, tag):
    d, M = models.d, models.M
    toks = d[f"{tag}:tokens"].tolist()
    st_np = [d[f"{tag}:{n}_in"].copy() for n in ("s0", "s1", "s2")]
    lg_np = M.forward_seq_batch(models.z_np, toks, st_np, 2)
    st_cpu = [torch.from_numpy(d[f"{tag}:{n}_in"].copy()) for n in ("s0", "s1", "s2")]
    lg_cpu = models.cpu.forward_seq_batch_seperate(toks, st_cpu)
    st4 = [torch.from_numpy(d[f"{tag}:{n}_in"].copy()).cuda() for n in ("s0", "s1", "s2")]
    st16 = [t.clone() for t in st4]
    lg4 = models.m4.forward_seq_batch_seperate(toks, st4)
    lg16 = models.m16.forward_seq_batch_seperate(toks, st16)
    for name, got, cpu, want in (("logits", lg4, lg_cpu, lg_np), ("wkv state", st4[1], st_cpu[1], st_np[1]), ("shift state", st4[0], st_cpu[0], st_np[0])):
        floor, err = rel_linf(cpu.numpy(), want), rel_linf(got.cpu().numpy(), want)
        print(f"MXFP4MODEL {tag} {name}: rel-Linf {err:.2e} floor {floor:.2e} bar {bar(floor):.2e}")
        assert err <= bar(floor), (tag, name, err, floor)
    assert st4[2].cpu().tolist() == st_np[2].tolist()
    print(f"MXFP4MODEL {tag} distance to the unquantised binary16 model's logits (recorded, not barred): rel-Linf "
          f"{rel_linf(lg4.cpu().numpy(), lg16.cpu().numpy()):.3e}")


def test_model_prefill_chunk_takes_the_dequant_path(models):
    """3 x 100 rows: above 256, the dequantised matrices through the library GEMM -- the same matrix as the decode path's."""
    from chirrup_amd.rwkv7 import plan_forward

    m4, M = models.m4, models.M
    assert plan_forward(m4, 300, 100, 128, m4._layers[0]).ffn_value == "mxfp4_dequant"
    toks = np.random.default_rng(11).integers(1, 320, (3, 100)).tolist()
    st_np = [np.zeros_like(models.d[f"b3t1:{n}_in"]) for n in ("s0", "s1", "s2")]
    lg_np = M.forward_seq_batch(models.z_np, toks, st_np, 2)
    st_cpu = models.cpu.generate_zero_state(3)
    lg_cpu = models.cpu.forward_seq_batch_seperate(toks, st_cpu)
    st4 = m4.generate_zero_state(3)
    lg4 = m4.forward_seq_batch_seperate(toks, st4)
    for name, got, cpu, want in (("logits", lg4, lg_cpu, lg_np), ("wkv state", st4[1], st_cpu[1], st_np[1]), ("shift state", st4[0], st_cpu[0], st_np[0])):
        floor, err = rel_linf(cpu.numpy(), want), rel_linf(got.cpu().numpy(), want)
        print(f"MXFP4MODEL prefill 3x100 {name}: rel-Linf {err:.2e} floor {floor:.2e} bar {bar(floor):.2e}")
        assert err <= bar(floor), (name, err, floor)


def greedy_run(models, forward, state, prompt, steps=8):
    """Teacher-forced on the oracle's ids: per step the oracle's ids, its top-two gaps, the logit bar in logit units, forward's ids."""
    M = models.M
    st_np = [np.zeros_like(models.d[f"b3t1:{n}_in"]) for n in ("s0", "s1", "s2")]
    st_cpu = models.cpu.generate_zero_state(3)
    toks, rows = prompt, []
    for _ in range(steps + 1):
        lg_np = M.forward_seq_batch(models.z_np, toks, st_np, 2).astype(F32)
        lg_cpu = models.cpu.forward_seq_batch_seperate(toks, st_cpu)
        got = forward(toks, state) if forward is not None else None
        top2 = np.sort(lg_np, -1)[:, -2:]
        rows.append((lg_np.argmax(-1), top2[:, 1] - top2[:, 0], bar(rel_linf(lg_cpu.numpy(), lg_np)) * max(1.0, float(np.abs(lg_np).max())),
                     None if got is None else got.float().argmax(-1).cpu().numpy()))
        toks = [[int(t)] for t in rows[-1][0]]
    return rows[1:]                                                       # (the prompt's own step is the prefill)


def test_model_greedy_decode_gives_the_oracles_ids(models):
    m4 = models.m4
    prompt = np.random.default_rng(GREEDY_SEED).integers(1, 320, (3, 6)).tolist()
    rows = greedy_run(models, m4.forward_seq_batch_seperate, m4.generate_zero_state(3), prompt)
    left_out = 0
    for step, (want, gap, lbar, got) in enumerate(rows):
        for b in range(3):
            if gap[b] < 2 * lbar:
                left_out += 1
                continue
            assert got[b] == want[b], (step, b, int(got[b]), int(want[b]), float(gap[b]), lbar)
    print(f"MXFP4MODEL greedy: 24 steps, {left_out} left out (top-two gap below twice the logit bar), smallest gap {min(float(r[1].min()) for r in rows):.3f}")
    assert left_out <= 1


# ---------------------------------------------------------------------------------------------------------------------
# worker

class _Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "".join(chr(65 + i % 26) for i in ids)


class _Sink:
    def __init__(self):
        self.items = []

    def put_nowait(self, x):
        self.items.append(x)


def test_worker_with_dtype_mxfp4(models, tmp_path):
    """ModelLoadConfig(dtype="mxfp4") through the worker's own model load: two greedy requests give the ids of the model-level run.
    The worker batches the requests and prefills in chunks -- the same matrices in another summation order -- so the two prompts are the
    first of a fixed candidate list whose model-level run keeps its top-two margin above binary16 noise at every step (0.02, the margin
    of tests/test_worker_gpu.py); for those the ids must be equal outright."""
    from chirrup_amd.core_structure import ModelLoadConfig, Task
    from chirrup_amd.worker import Worker

    path = str(tmp_path / "fixture.pth")
    torch.save(models.zd, path)
    cfg = ModelLoadConfig(model_path=path, vocab_path="unused", vocab_size=320, head_size=64, dtype="mxfp4")
    tq, mq = queue.Queue(), queue.Queue()
    w = Worker("w0", [0], cfg, tq, mq, None, batch_size=4, tokenizer=_Tok())
    w._init_worker()
    assert w.model.ffn_dtype == "mxfp4" and "blocks.0.ffn.key.weight.mxfp4" in w.model.z
    m4, n_new = models.m4, 8

    def solo(p):
        st = m4.generate_zero_state(1)
        lg = m4.forward_seq_batch_seperate([p], st)
        ids, margins = [], []
        for _ in range(n_new):
            top2 = torch.topk(lg.float(), 2, dim=-1).values[0]
            margins.append(float(top2[0] - top2[1]))
            ids.append(int(lg.float().argmax(-1)))
            lg = m4.forward_seq_batch_seperate([[ids[-1]]], st)
        return ids, min(margins)

    rng = np.random.default_rng(5)
    candidates = [models.d["greedy:prompt"][0].tolist(), models.d["greedy:prompt"][1].tolist()] + [rng.integers(1, 320, n).tolist() for n in (4, 14, 37, 9, 21, 6)]
    chosen = []
    for p in candidates:
        ids, margin = solo(p)
        print(f"MXFP4WORKER candidate of {len(p)} tokens: model-level margin {margin:.3f}")
        if margin >= 0.02:
            chosen.append((p, ids))
        if len(chosen) == 2:
            break
    assert len(chosen) == 2
    tasks = []
    for p, _ in chosen:
        t = Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(p), state=None,
                 temperature=0.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, stop_tokens=[], max_tokens=n_new)
        tasks.append(t)
        tq.put(t)
    for _ in range(2000):
        if not w.step():
            break
    for t, (p, want) in zip(tasks, chosen):
        got = [x[1][0] for x in t.output_queue.items if x[0] == "token_generated"]
        assert got == want, (len(p), got, want)
