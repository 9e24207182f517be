"""CPU tests of the exact reference of the skinny GEMMs (tests/gemm_ref.py): what shows, without a GPU, that the GPU tests of
tests/test_gemm_exact_gpu.py can fail and that they hide nothing.  Every case those tests use satisfies the exact-sum lemma's
condition (prove_exact: a condition, not a measurement); binary32 evaluations in several orders give the expected bits; numpy
emulations of wrong kernels are rejected."""
import numpy as np
import pytest

import gemm_ref as G
from tmix_ref import bits

F16, F32, F64 = np.float16, np.float32, np.float64


@pytest.mark.parametrize("name", list(G.F16_CASES))
def test_f16_cases_are_exact_in_any_order(name):
    M, N, K, bias, splits = G.F16_CASES[name]
    case = G.f16_named(name)
    margin, rounded = G.prove_exact(case, splits)
    print(f"{name}: sum|terms| / 2^24 q = {margin:.5f}, outputs that needed rounding {rounded:.3f}")
    big = M * N * K > 1 << 28                                   # the wide cases: the orders on 2048 rows of W
    sub = case if not big else dict(case, wi=case["wi"][:2048], bi=None if case["bi"] is None else case["bi"][:2048])
    for act in (None, "relu_sq"):
        lo, hi = G.expected(sub, act)
        assert np.array_equal(bits(lo), bits(hi))
        evals = [("permuted", 1), ("slices", 2), ("slices", 3), ("slices", 4), ("blocks", splits[-1])]
        for order, s in evals:
            got = G.emulate_f16(sub, act, order, s)
            G.assert_bits(got, lo, hi, G.exact_pre(sub), 2.0 ** (case["ex"] + case["ew"]), f"{name} {order} {s}")
    if not big:
        for s in splits:
            p = G.expected_planes(case, s)
            x32, w32 = (a.astype(F32) for a in G.halves(case)[:2])
            got = np.stack([x32[:, i * K // s:(i + 1) * K // s] @ w32[:, i * K // s:(i + 1) * K // s].T for i in range(s)])
            G.assert_planes(got, p)


@pytest.mark.parametrize("name", list(G.SCALED_CASES))
def test_scaled_cases_are_exact(name):
    case, splits = G.scaled_named(name)
    margin, rounded = G.prove_exact(case, splits)
    x, _, _ = G.halves(case)
    lo, _ = G.expected(case)
    v = G.exact_pre(case)
    sub = float((np.abs(lo.astype(F64)) < 2.0 ** -14).mean())
    inf = float(np.isinf(lo).mean())
    edge = (np.abs(v) > 65504) & (np.abs(v) < 65520)
    past = np.abs(v) >= 65520
    print(f"{name}: margin {margin:.5f} rounded {rounded:.3f} subnormal outputs {sub:.3f} inf {inf:.3f} in (65504, 65520): {int(edge.sum())} "
          f"at or past 65520: {int(past.sum())}")
    if name.startswith("subnormal"):
        assert float(np.abs(x.astype(F64)).max()) < 2.0 ** -14 and sub > 0.99 and float((lo != 0).mean()) > 0.5
    else:
        assert 0.01 < inf < 0.5 and past.sum() > 0 and np.isinf(lo[past]).all()
    if name.startswith("overflow-edge"):                        # both thresholds, both signs
        for sign in (1, -1):
            assert (edge & (v * sign > 0)).sum() >= 10 and (past & (v * sign > 0)).sum() >= 10
        assert (np.abs(lo[edge].astype(F64)) == 65504).all()
        # an epilogue that saturates at the wrong threshold (everything above 65504 to inf) is rejected on exactly the edge elements
        wrong = np.where(np.abs(v) > 65504, np.sign(v) * np.inf, lo.astype(F64)).astype(F16)
        assert G.report(wrong, lo, lo)["bad"] == int(edge.sum())
    for order, s in (("permuted", 1), ("slices", 3), ("blocks", splits[-1])):
        G.assert_bits(G.emulate_f16(case, None, order, s), lo, lo, v, 2.0 ** (case["ex"] + case["ew"]), f"{name} {order}")


@pytest.mark.parametrize("name", list(G.MM8_CASES))
def test_mm8_cases_are_exact_in_any_order(name):
    B, K, N, splits = G.MM8_CASES[name]
    c = G.mm8_named(name)
    margin = G.mm8_prove_exact(c, splits)
    print(f"{name}: core sum|terms| / 2^19 = {margin:.4f}")
    for act in (0, 1):
        y, xs2 = G.mm8_expected(c, act)
        for order, s in (("permuted", 1), ("slices", 2), ("slices", 3), ("slices", 4)):
            gy, gx = G.emulate_mm8(c, act, order, s)
            G.assert_bits(gy, y, y, name=f"{name} y {order} {s}")
            G.assert_bits(gx, xs2, xs2, name=f"{name} xs2 {order} {s}")
    for s in splits:
        hv = G.mm8_halves(c)
        xs, wq = hv["xs"].astype(F32), F32(1024) + hv["q"].astype(F32)
        got = np.stack([xs[:, i * K // s:(i + 1) * K // s] @ wq[:, i * K // s:(i + 1) * K // s].T for i in range(s)])
        G.assert_planes(got, G.mm8_planes(c, s))


# mutant -> the cases it is run on (act, split count, k_of); rejected on at least 10 elements of at least one of them
MUT_F16 = {
    "block_dropped": [("M17-N132-K1024", None, 4, None)],
    "slice_boundary_off": [("M17-N132-K1024", None, 4, None)],
    "chunks_swapped": [("M16-N128-K192", None, 1, None)],
    "half_boundary_off": [("M113-N260-K64", None, 1, None)],
    "bias_after_rounding": [("M33-N1000-K192", None, 1, None), ("M24-N1024-K4096", None, 1, None)],
    "relu_sq_unrounded": [("M33-N1000-K192", "relu_sq", 1, None)],
    "round_toward_zero": [("M33-N1000-K192", None, 1, None)],
    "f16_block_accumulation": [("M200-N1000-K1024", None, 1, None), ("M24-N1024-K4096", None, 1, None)],
    "k_of_ignored": [("M17-N132-K1024", None, 1, 128)],
}


@pytest.mark.parametrize("mutant", G.F16_MUTANTS)
def test_f16_mutants_are_rejected(mutant):
    worst = 0
    for name, act, s, k in MUT_F16[mutant]:
        case = G.f16_named(name)
        lo, hi = G.expected(case, act, k)
        ok = G.report(G.emulate_f16(case, act, "blocks", s, None, k), lo, hi)
        assert ok["bad"] == 0, ok["msg"]
        res = G.report(G.emulate_f16(case, act, "blocks", s, mutant, k), lo, hi, G.exact_pre(case, k), 2.0 ** -12)
        print(f"{mutant} on {name}: rejected on {res['bad']} of {res['n']} ({res['bad'] / res['n']:.4f})")
        if res["bad"]:
            print("   ", res["msg"][:300])
        worst = max(worst, res["bad"])
    assert worst >= 10


@pytest.mark.parametrize("mutant", G.MM8_MUTANTS)
def test_mm8_mutants_are_rejected(mutant):
    c = G.mm8_named("B33-K256-N1000")
    y, xs2 = G.mm8_expected(c, 0)
    gy, _ = G.emulate_mm8(c, 0, "slices", 2, mutant)
    res = G.report(gy, y, y)
    print(f"{mutant}: rejected on {res['bad']} of {res['n']} ({res['bad'] / res['n']:.4f})")
    assert res["bad"] >= 10


def test_old_bar_misses_what_bit_equality_sees():
    """The 2e-3 * max(1, |want|) bar of test_skinny_linear_matches_fp64 against bit equality, on the defects it cannot see."""
    case = G.f16_named("M24-N1024-K4096")
    lo, _ = G.expected(case)
    want = G.exact_pre(case)
    for mutant in ("bias_after_rounding", "round_toward_zero"):
        got = G.emulate_f16(case, None, "blocks", 1, mutant)
        old = int((np.abs(got.astype(F64) - want) > 2e-3 * np.maximum(1.0, np.abs(want))).sum())
        new = G.report(got, lo, lo)["bad"]
        print(f"{mutant}: old bar flags {old}, bit equality {new} of {got.size}")
        assert old == 0 and new >= 0.05 * got.size


def test_guards_and_report():
    t = np.arange(12, dtype=F16).reshape(3, 4)
    parent, idx = G.embed(t, 2, 8, np.nan)
    assert parent.shape == (7, 20) and np.array_equal(parent[idx], t) and np.isnan(parent).sum() == 7 * 20 - 12
    out, oidx = G.embed(np.zeros((2, 3, 4), F32), 1, 4, -7777.0)
    assert out.shape == (2, 5, 12) and G.guards_intact(out, oidx, -7777.0)
    out[1, 0, 0] = 0
    assert not G.guards_intact(out, oidx, -7777.0)
    b, bidx = G.embed(np.ones(8, F16), pad_cols=8)
    assert b.shape == (24,) and np.isnan(b[:8]).all() and (b[bidx] == 1).all()
    # a wrong 16-row x 128-column tile shows as one in the report
    case = G.f16_named("M33-N1000-K192")
    lo, _ = G.expected(case)
    got = lo.copy()
    got[16:32, 128:256] += F16(1)
    res = G.report(got, lo, lo, G.exact_pre(case), 2.0 ** -12)
    assert "first (16, 128)" in res["msg"] and "1 of 24 tiles" in res["msg"] and "(1.00, 1, 1)" in res["msg"], res["msg"]
    x = np.array([1.0009765625 + 2.0 ** -12, -(1.0009765625 + 2.0 ** -12), 65519.0, 3.0])
    assert G.rtz16(x).tolist() == [1.0009765625, -1.0009765625, 65504.0, 3.0]


@pytest.mark.parametrize("M", list(G.BMM_KOF))
def test_bmm_k_of_cases_are_exact(M):
    cases, ks = G.bmm_kof_named(M)
    for z, (c, k) in enumerate(zip(cases, ks)):
        margin, rounded = G.prove_exact(c, (1,), k)
        print(f"bmm k_of M={M} z={z} k={k}: margin {margin:.5f} rounded {rounded:.3f}")
        lo, _ = G.expected(c, None, k)
        for order, s in (("permuted", 1), ("slices", 2), ("slices", 3), ("slices", 4)):
            G.assert_bits(G.emulate_f16(c, None, order, s, k=k), lo, lo, G.exact_pre(c, k), 2.0 ** -12, f"bmm k_of M={M} z={z} {order} {s}")


@pytest.mark.parametrize("M,act", sorted({(M, act) for M, act, _ in G.BMM_PLANES}))
def test_bmm_plane_cases_are_exact(M, act):
    """Every split count a launch may use (the library picks among 1, 2, 4, 8, 16 at K = 1024); tanh / sigmoid of the exact half from the table."""
    for z, c in enumerate(G.bmm_planes_named(M, act)):
        margin, rounded = G.prove_exact(c, (1, 2, 4, 8, 16))
        print(f"bmm planes M={M} act={act} z={z}: margin {margin:.5f} rounded {rounded:.3f}")
        kind = {1: "tanh", 3: "sigmoid"}.get(z + act - 4)
        lo, hi = G.expected(c, kind)
        for order, s in (("permuted", 1), ("slices", 2), ("slices", 3), ("slices", 4)):
            pre = G.emulate_f16(c, None, order, s)
            G.assert_bits(pre, *G.expected(c), name=f"bmm planes M={M} z={z} {order} {s}")
            if kind:                                            # the table is entered with the exact half
                assert np.array_equal(bits(lo), bits(G.act_table(kind)[0][bits(pre)]))


@pytest.mark.parametrize("which,M", [("group", M) for M in G.GROUP_LAYERS] + [("tmix", M) for M in G.TMIX_LAYERS])
def test_layer_launch_cases_are_exact(which, M):
    """R/K/V, the four down-projections and the v and a up-projections (fed by an exact hidden plane) of every layer launch."""
    layer = G.layer_problem(*(G.GROUP_LAYERS if which == "group" else G.TMIX_LAYERS)[M])
    res = G.layer_prove_exact(layer)
    print(f"{which} layer M={M}: worst margin {max(m for m, _ in res):.5f}, rounded {min(r for _, r in res):.3f}..{max(r for _, r in res):.3f}")
    main, _, down, _, _ = layer
    ups = [G.layer_up_case(layer, j) for j in range(4) if G.ACTS[j] is None]
    for i, c in enumerate(main + down + ups):
        lo, _ = G.expected(c)
        for order, s in (("permuted", 1), ("slices", 2), ("slices", 3), ("slices", 4)):
            G.assert_bits(G.emulate_f16(c, None, order, s), lo, lo, name=f"{which} layer M={M} problem {i} {order} {s}")


@pytest.mark.parametrize("M", list(G.TMIX_LAYERS))
def test_tmix_mm8_cases_are_exact(M):
    for j, c in enumerate(G.tmix_mm8_cases(M)):
        margin = G.mm8_prove_exact(c, (1, 2, 4))
        print(f"tmix mm8 M={M} problem {j}: core sum|terms| / 2^19 = {margin:.4f}")
        y, _ = G.mm8_expected(c)
        for order, s in (("permuted", 1), ("slices", 2), ("slices", 3), ("slices", 4)):
            G.assert_bits(G.emulate_mm8(c, 0, order, s)[0], y, y, name=f"tmix mm8 M={M} problem {j} {order} {s}")
