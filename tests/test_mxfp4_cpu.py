"""MXFP4 (w4a16) without a GPU: the host quantiser (chirrup_amd/quant.py), plan_forward's forms for ffn_dtype="mxfp4", the C ABI of
csrc/mxfp4.hip, and the exact-sum lemma for every GEMM case that tests/test_mxfp4_gpu.py runs (a checked condition, not a belief)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import gemm_ref as G
import mxfp4_cases as X
from chirrup_amd import quant as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = torch.tensor(Q.E2M1_VALUES + tuple(-v for v in Q.E2M1_VALUES), dtype=torch.float64)
E_RANGE = range(Q.MXFP4_E_MIN, Q.MXFP4_E_MAX + 1)


def block_e(q):
    return q.scales.to(torch.int64) - 127


def nibbles(q):
    return torch.stack([q.codes & 15, q.codes >> 4], -1).reshape(q.codes.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------------
# quantiser

def test_round_trip_of_every_code_and_exponent():
    """A block that holds every grid value at exponent e (and 6 * 2^e, so that e is the block's exponent) comes back unchanged:
    27 exponents x 16 codes; -0 is stored as +0."""
    rows = []
    for e in E_RANGE:
        blk = torch.zeros(32, dtype=torch.float64)
        blk[:16] = VALUES * 2.0 ** e
        blk[16] = 6.0 * 2.0 ** e
        rows.append(blk)
    w = torch.stack(rows)
    q = Q.quantize_linear_mxfp4(w)
    assert block_e(q)[:, 0].tolist() == list(E_RANGE)
    want = list(range(8)) + [0] + list(range(9, 16)) + [7] + [0] * 15
    assert all(nibbles(q)[i].tolist() == want for i in range(len(rows)))
    d = Q.dequantize_mxfp4(q)
    assert d.dtype == torch.float16 and torch.equal(d.double(), w)
    assert torch.equal(Q.dequantize_mxfp4(Q.quantize_linear_mxfp4(w.half())), d)            # binary16 input, the model's


def test_error_bound_and_scale_rule():
    """|w - w~| <= 2^e per element (no saturation; the grid's widest step is 2 * 2^e) and 6 * 2^(e-1) < amax <= 6 * 2^e for every
    block whose exponent was not clamped -- over magnitudes from 2^-20 to 2^15, block boundaries 6 * 2^e exactly and one ulp either side."""
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(64, 256, generator=g, dtype=torch.float64) * 2.0 ** torch.randint(-20, 12, (64, 8), generator=g).repeat_interleave(32, 1).double())
    edge = torch.zeros(81, 32, dtype=torch.float64)
    for i, e in enumerate(E_RANGE):
        for j, f in enumerate((1.0, 1.0 + 2.0 ** -10, 1.0 - 2.0 ** -11)):
            edge[3 * i + j, 5] = -6.0 * 2.0 ** e * f
            edge[3 * i + j, 6:] = torch.rand(26, generator=g, dtype=torch.float64) * 2.0 ** e
    for m in (w.half().double(), edge.half().double()):
        m = m.clamp(-49152.0, 49152.0)                                    # (beyond 6 * 2^13 a block saturates: tested below)
        q = Q.quantize_linear_mxfp4(m)
        e = block_e(q)
        d = Q.dequantize_mxfp4(q).double()
        amax = m.abs().reshape(m.shape[0], -1, 32).amax(-1)
        err = (m - d).abs().reshape(m.shape[0], -1, 32).amax(-1)
        assert bool((err <= 2.0 ** e.double()).all()), float((err / 2.0 ** e.double()).max())
        free = (e > Q.MXFP4_E_MIN) & (e < Q.MXFP4_E_MAX)
        assert int(free.sum()) > 20
        assert bool((amax[free] <= 6.0 * 2.0 ** e[free].double()).all()) and bool((amax[free] > 3.0 * 2.0 ** e[free].double()).all())
        low = e == Q.MXFP4_E_MIN
        assert bool((amax[low] <= 6.0 * 2.0 ** -13).all())
    e_edge = block_e(Q.quantize_linear_mxfp4(edge))[:, 0].reshape(27, 3)
    ee = torch.tensor(list(E_RANGE))
    assert torch.equal(e_edge[:, 0], ee) and torch.equal(e_edge[:, 2], ee)          # amax = 6 * 2^e and just below: e
    assert torch.equal(e_edge[:-1, 1], ee[:-1] + 1) and int(e_edge[-1, 1]) == 13      # just above: e + 1 (clamped at 13)


def test_rounding_is_nearest_with_ties_to_the_even_code():
    pts = [0.2, 0.25, 0.26, 0.74, 0.75, 1.2, 1.25, 1.3, 1.75, 2.4, 2.5, 2.6, 3.5, 4.9, 5.0, 5.1, 6.0]
    want = [0, 0, 1, 1, 2, 2, 2, 3, 4, 4, 4, 5, 6, 6, 6, 7, 7]
    blk = torch.zeros(2, 32, dtype=torch.float64)
    blk[0, :len(pts)] = torch.tensor(pts)
    blk[1, :len(pts)] = -torch.tensor(pts)
    blk[:, 31] = 6.0
    q = Q.quantize_linear_mxfp4(blk)
    n = nibbles(q)
    assert block_e(q).flatten().tolist() == [0, 0]
    assert n[0, :len(pts)].tolist() == want
    assert n[1, :len(pts)].tolist() == [c | 8 if c else 0 for c in want]


def test_zero_tiny_and_saturating_blocks():
    w = torch.zeros(4, 64, dtype=torch.float16)
    w[1, :32] = 2.0 ** -24                         # the smallest binary16 subnormal: below half a grid step at 2^-13 -> 0
    w[1, 32:] = 2.0 ** -15                         # 0.25 * 2^-13: a tie -> the even code 0
    w[2, 0], w[2, 1] = 2.0 ** -14, -1.5 * 2.0 ** -14      # 0.5 and -0.75 grid units at 2^-13: code 1, tie -> -1.0 (code 2)
    w[3, 0], w[3, 40] = 65504.0, -60000.0          # past 6 * 2^13: clamped to +-6 * 2^13
    q = Q.quantize_linear_mxfp4(w)
    assert block_e(q).tolist() == [[-13, -13], [-13, -13], [-13, -13], [13, 13]]
    d = Q.dequantize_mxfp4(q)
    assert not d[0].any() and not d[1].any()
    assert float(d[2, 0]) == 2.0 ** -14 and float(d[2, 1]) == -(2.0 ** -13)
    assert float(d[3, 0]) == 49152.0 and float(d[3, 40]) == -49152.0
    assert int(q.codes[0].max()) == 0 and int(q.codes[1].max()) == 0


def test_refusals():
    ok = Q.quantize_linear_mxfp4(torch.ones(4, 64))
    Q.check_mxfp4(ok)
    for bad in (113, 141, 0, 255):
        s = ok.scales.clone()
        s[2, 1] = bad
        with pytest.raises(ValueError):
            Q.check_mxfp4(ok._replace(scales=s))
        with pytest.raises(ValueError):
            Q.dequantize_mxfp4(ok._replace(scales=s))
    for s in (114, 140):
        Q.check_mxfp4(ok._replace(scales=torch.full_like(ok.scales, s)))
    with pytest.raises(ValueError):
        Q.check_mxfp4(ok._replace(scales=ok.scales[:, :1]))
    with pytest.raises(ValueError):
        Q.check_mxfp4(ok._replace(codes=ok.codes[:3]))
    with pytest.raises(ValueError):
        Q.check_mxfp4(ok._replace(codes=ok.codes.to(torch.int32)))
    for shape in ((4, 48), (4, 0), (0, 64), (64,)):
        with pytest.raises(ValueError):
            Q.quantize_linear_mxfp4(torch.ones(shape))
    with pytest.raises(ValueError):
        Q.quantize_linear_mxfp4(torch.ones(4, 64, dtype=torch.int32))
    w = torch.ones(4, 64)
    w[1, 3] = float("nan")
    with pytest.raises(ValueError):
        Q.quantize_linear_mxfp4(w)
    w[1, 3] = float("inf")
    with pytest.raises(ValueError):
        Q.quantize_linear_mxfp4(w)


def test_determinism_and_packing_order():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(128, 192, generator=g).half()
    a, b = Q.quantize_linear_mxfp4(w), Q.quantize_linear_mxfp4(w.clone())
    assert torch.equal(a.codes, b.codes) and torch.equal(a.scales, b.scales)
    c = Q.quantize_linear_mxfp4(w.t().contiguous().t())                      # a strided view of the same values
    assert torch.equal(a.codes, c.codes) and torch.equal(a.scales, c.scales)
    assert a.codes.shape == (128, 96) and a.scales.shape == (128, 6) and a.codes.dtype == a.scales.dtype == torch.uint8
    blk = torch.zeros(1, 32, dtype=torch.float64)
    blk[0, 0], blk[0, 1], blk[0, 2], blk[0, 31] = 1.0, -6.0, 0.5, 3.0
    q = Q.quantize_linear_mxfp4(blk)
    assert int(q.codes[0, 0]) == 2 | (15 << 4)                                # k = 0 in the low nibble, k = 1 in the high one
    assert int(q.codes[0, 1]) == 1 and int(q.codes[0, 15]) == 5 << 4


def test_tile_image_inverse_matches_the_documented_layout():
    """untile_mxfp4 against the layout written out by hand (include/chirrup_amd.h): tile (g, b) at 4352 (g K/64 + b); code byte position
    8 q + 4 s + j of row r holds logical byte 16 s + 4 q + j of the K-block; scale byte 2 r + s."""
    M, K = 256, 192
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 256, (M, K // 2)).astype(np.uint8)
    scales = rng.integers(114, 141, (M, K // 32)).astype(np.uint8)
    flat = np.zeros(Q.mxfp4_tiled_bytes(M, K), np.uint8)
    assert flat.size == M * K // 2 + M * K // 32 == 2 * 3 * 4352
    for g in range(M // 128):
        for b in range(K // 64):
            base = (g * (K // 64) + b) * 4352
            for r in range(128):
                for p in range(32):
                    q_, s, j = p >> 3, (p >> 2) & 1, p & 3
                    flat[base + 32 * r + p] = codes[128 * g + r, 32 * b + 16 * s + 4 * q_ + j]
                for s in range(2):
                    flat[base + 4096 + 2 * r + s] = scales[128 * g + r, 2 * b + s]
    w = Q.untile_mxfp4(torch.from_numpy(flat), M, K)
    assert np.array_equal(w.codes.numpy(), codes) and np.array_equal(w.scales.numpy(), scales)


# ---------------------------------------------------------------------------------------------------------------------
# plan_forward

def test_plan_forward_forms():
    from test_forward_plan_cpu import layer, plan

    for att in (torch.float16, torch.int8):
        lw = layer(att8=att == torch.int8)
        for rows, T in ((1, 1), (16, 1), (16, 4), (200, 1), (256, 1), (255, 5)):
            p = plan(4096, rows, T=T, lw=lw, ffn_dtype="mxfp4", att_dtype=att)
            assert (p.ffn_key, p.ffn_value) == ("mxfp4", "mxfp4_parts"), (rows, T)
            assert not p.use_parts                   # (the binary16 FFN's ring launches are not part of this plan)
        for rows, T in ((257, 1), (2500, 100)):
            p = plan(4096, rows, T=T, lw=lw, ffn_dtype="mxfp4", att_dtype=att)
            assert (p.ffn_key, p.ffn_value) == ("mxfp4_dequant", "mxfp4_dequant"), rows
        for rows, T in ((1, 1), (16, 1), (200, 1), (256, 1), (257, 1), (2500, 100)):
            p = plan(4096, rows, T=T, lw=lw, ffn_dtype="mxfp4", att_dtype=att)
            assert "mm8" not in p.ffn_key and "mm8" not in p.ffn_value
            base = plan(4096, rows, T=T, lw=lw, att_dtype=att)       # everything but the channel-mix: the binary16-FFN plan's
            assert (p.hw, p.fuse_core, p.row_halves, p.rkv, p.lora, p.side, p.att_out, p.head) == \
                   (base.hw, base.fuse_core, base.row_halves, base.rkv, base.lora, base.side, base.att_out, base.head)
    # a knob that takes the binary16 FFN off the hand-written kernels does not move the MXFP4 forms (there is no library form of them)
    assert plan(4096, 16, ffn_dtype="mxfp4", skinny_ffn_value=False).ffn_value == "mxfp4_parts"


def test_model_refuses_what_it_cannot_run():
    from chirrup_amd import rwkv7
    from chirrup_amd.synth import make_state_dict

    args = lambda: types.SimpleNamespace(vocab_size=256, head_size=64, MODEL_NAME="unused")
    zd = make_state_dict(1, 128, 256, seed=0)
    with pytest.raises(Exception, match="MXFP4"):
        rwkv7.RWKV_x070(args(), state_dict=zd, device="cpu", ffn_dtype="mxfp4")        # no CPU form: the HIP kernels or nothing
    with pytest.raises(ValueError):
        rwkv7.RWKV_x070(args(), state_dict=zd, device="cpu", ffn_dtype="fp4")
    with pytest.raises(ValueError):
        rwkv7.RWKV_x070(args(), state_dict=zd, device="cpu", att_dtype="mxfp4")        # att_dtype keeps its two values


# ---------------------------------------------------------------------------------------------------------------------
# ABI

NEW = ["mxfp4_tiled_bytes", "mxfp4_tile_weight", "mxfp4_dequant_f16", "mxfp4_gemm_splits", "mxfp4_gemm_workspace_bytes", "mxfp4_gemm",
       "mxfp4_gemm_partial"]


def test_abi_header_signatures_and_symbols():
    import chirrup_amd
    from chirrup_amd import lib

    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    L = chirrup_amd.load()
    header = open(os.path.join(ROOT, "include", "chirrup_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;{]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/chirrup_amd.h"
        res, args = lib.SIGNATURES[name]
        assert res is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int)
        decl = [a.strip() for a in m.group(2).split(",")]
        assert len(decl) == len(args), name
        for a, t in zip(decl, args):
            want = ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int
            assert t is want, (name, a)
        assert hasattr(L, name)
    assert int(re.search(r"#define\s+CHIRRUP_ABI_VERSION\s+(\d+)", header).group(1)) == lib.ABI_VERSION == L.chirrup_abi_version() == 4


def test_abi_argument_validation_needs_no_gpu():
    import chirrup_amd

    L = chirrup_amd.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert L.mxfp4_tiled_bytes(128, 64) == 4352 and L.mxfp4_tiled_bytes(256, 192) == 6 * 4352
    assert L.mxfp4_tiled_bytes(64, 64) == 0 and L.mxfp4_tiled_bytes(128, 32) == 0 and L.mxfp4_tiled_bytes(0, 64) == 0
    assert L.mxfp4_tile_weight(100, 64, p, 32, p, 2, p, None) == -1                  # M_out % 128
    assert L.mxfp4_tile_weight(128, 96, p, 48, p, 3, p, None) == -1                  # N_in % 64
    assert L.mxfp4_tile_weight(128, 64, p, 16, p, 2, p, None) == -1                  # ld_codes < N_in / 2
    assert L.mxfp4_tile_weight(128, 64, p, 32, p, 1, p, None) == -1                  # ld_scales < N_in / 32
    assert L.mxfp4_tile_weight(128, 64, None, 32, p, 2, p, None) == -2
    assert L.mxfp4_tile_weight(128, 64, p, 32, p, 2, odd, None) == -3
    assert L.mxfp4_dequant_f16(128, 64, p, p, 60, None) == -1                        # ld_out < N_in
    assert L.mxfp4_dequant_f16(128, 64, p, None, 64, None) == -2
    assert L.mxfp4_dequant_f16(128, 64, p, odd, 64, None) == -3
    assert L.mxfp4_gemm(257, 128, 64, p, 64, p, p, 128, 0, 0, None, None) == -1      # more than 256 rows
    assert L.mxfp4_gemm(0, 128, 64, p, 64, p, p, 128, 0, 0, None, None) == -1
    assert L.mxfp4_gemm(4, 132, 64, p, 64, p, p, 132, 0, 0, None, None) == -1        # N % 128
    assert L.mxfp4_gemm(4, 128, 96, p, 96, p, p, 128, 0, 0, None, None) == -1        # K % 64
    assert L.mxfp4_gemm(4, 128, 64, p, 60, p, p, 128, 0, 0, None, None) == -1        # ldx < K
    assert L.mxfp4_gemm(4, 128, 64, p, 64, p, p, 126, 0, 0, None, None) == -1        # ldy < N
    assert L.mxfp4_gemm(4, 128, 64, p, 64, p, p, 128, 2, 0, None, None) == -4        # act
    assert L.mxfp4_gemm(4, 128, 64, None, 64, p, p, 128, 0, 0, None, None) == -2
    assert L.mxfp4_gemm(4, 128, 64, odd, 64, p, p, 128, 0, 0, None, None) == -3
    assert L.mxfp4_gemm(4, 128, 128, p, 128, p, p, 128, 0, 2, None, None) == -2      # two slices and no workspace
    assert L.mxfp4_gemm_partial(4, 128, 64, p, 64, p, 1, None, None) == -1000 + 2
    assert L.mxfp4_gemm_partial(300, 128, 64, p, 64, p, 1, p, None) == -1000 + 1
    # split counts: as asked for when they divide the K-block count, else cut back; 0: the library's choice, a divisor too
    assert [L.mxfp4_gemm_splits(17, 128, 1024, s) for s in (1, 2, 4, 16)] == [1, 2, 4, 16]
    assert L.mxfp4_gemm_splits(17, 128, 192, 2) == 1 and L.mxfp4_gemm_splits(17, 128, 192, 3) == 3 and L.mxfp4_gemm_splits(17, 128, 64, 16) == 1
    for M, N, K in ((1, 128, 64), (17, 128, 192), (200, 256, 4096), (200, 16384, 4096), (200, 4096, 16384), (1, 4096, 16384)):
        s = L.mxfp4_gemm_splits(M, N, K, 0)
        assert 1 <= s <= 16 and (K // 64) % s == 0, (M, N, K, s)
        assert L.mxfp4_gemm_workspace_bytes(M, N, K, 0) == (s * M * N * 4 if s > 1 else 0)
    assert L.mxfp4_gemm_splits(17, 100, 1024, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the lemma, for every case of tests/test_mxfp4_gpu.py

def test_case_recipe_is_the_library_format():
    """The cases' integer weights are what the library's own dequantisation gives for their codes and scale bytes."""
    for name in ("M17-N128-K192", "M33-N256-K1024"):
        c = X.named(name)
        codes, scales = X.packed(c)
        d = Q.dequantize_mxfp4(Q.Mxfp4Weight(torch.from_numpy(codes), torch.from_numpy(scales))).double().numpy()
        assert np.array_equal(d, c["wi"] * 2.0 ** c["ew"]) and np.array_equal(d, X.dequantised(c))
        assert (c["eblk"][:, 0::2] != c["eblk"][:, 1::2]).mean() > 0.5          # the two halves of a K-block differ
        assert set(np.unique(c["codes"])) == set(range(16)) and set(np.unique(c["eblk"])) == set(range(-12, -5))
    c, _ = X.scaled_named("overflow")
    codes, scales = X.packed(c)
    d = Q.dequantize_mxfp4(Q.Mxfp4Weight(torch.from_numpy(codes), torch.from_numpy(scales))).double().numpy()
    assert np.array_equal(d, c["wi"] * 2.0 ** c["ew"])


@pytest.mark.parametrize("name", list(X.CASES))
def test_lemma_holds_for_every_gpu_case(name):
    M, N, K, splits = X.CASES[name]
    margin, rounded = G.prove_exact(X.named(name), splits)
    print(f"MXFP4REF {name}: splits {splits} margin {margin:.4f} outputs needing the final rounding {rounded:.2f}")
    assert margin < 1.0 and rounded > 0.1           # (a case whose outputs were all binary16 numbers already would not test the final rounding)


def test_lemma_holds_for_the_scaled_and_extreme_cases():
    for name in X.SCALED:
        c, splits = X.scaled_named(name)
        margin, rounded = G.prove_exact(c, splits)
        lo = G.expected(c)[0]
        sub = float(((np.abs(lo.astype(np.float64)) < 2.0 ** -14) & (lo != 0)).mean())
        inf = float(np.isinf(lo).mean())
        print(f"MXFP4REF {name}: margin {margin:.4f} rounded {rounded:.2f} subnormal outputs {sub:.2f} infinite {inf:.2f}")
        assert margin < 1.0
        assert (sub > 0.95) if name == "subnormal" else (0.05 < inf < 0.95)
        if name == "subnormal":
            x16 = X.x_half(c)
            assert ((np.abs(x16.astype(np.float64)) < 2.0 ** -14) & (x16 != 0)).mean() > 0.5       # x itself is made of subnormals
    case, subs = X.extreme_case()
    codes, scales = X.packed(case)
    assert set(np.unique(scales)) == {114, 140}
    d = Q.dequantize_mxfp4(Q.Mxfp4Weight(torch.from_numpy(codes), torch.from_numpy(scales))).double().numpy()
    for e, (cols, sub) in subs.items():
        assert np.array_equal(d[cols], sub["wi"] * 2.0 ** sub["ew"])
        margin, rounded = G.prove_exact(sub, (1, 2, 4))
        lo = G.expected(sub)[0]
        print(f"MXFP4REF extreme e={e}: {len(cols)} columns margin {margin:.4f} rounded {rounded:.2f} finite {float(np.isfinite(lo).mean()):.2f} "
              f"subnormal {float((np.abs(lo.astype(np.float64)) < 2.0 ** -14).mean()):.2f}")
        assert margin < 1.0 and np.isfinite(lo).mean() > 0.9
