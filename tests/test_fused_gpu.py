"""Unit parity of the fused element-wise HIP kernels (csrc/elementwise.hip) against the numpy
oracle's per-op restatement (oracle/rwkv7_np.py).  Element-wise parts must be bit-identical; the
binary32 reductions (norms, head sums) may differ in summation order, which can move a result by
one binary16 ulp on a small fraction of elements."""
import numpy as np
import pytest
import torch

from oracle import rwkv7_np as M
from util import bits

pytestmark = pytest.mark.gpu
F16, F32 = np.float16, np.float32


def ulp_diff(a, b):
    def key(x):
        u = bits(x).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.abs(key(a) - key(b))


def assert_close_ulps(got, want, max_ulp=1, max_frac=0.01, name="", atol=1e-3):
    """Every element within max_ulp binary16 ulps of the oracle, or -- where operands of magnitude
    ~1 cancel to a result near zero, so that an ulp of the RESULT is far below the rounding of its
    inputs -- within atol (= one ulp at magnitude 1); and at most max_frac of elements differ at all."""
    d = ulp_diff(got, want)
    ad = np.abs(got.astype(F32) - want.astype(F32))
    bad = (d > max_ulp) & ~(ad <= atol)
    assert not bad.any(), f"{name}: {int(bad.sum())} elements off, worst {d[bad].max()} ulps / {ad[bad].max()} abs"
    assert (d > 0).mean() <= max_frac, f"{name}: {(d > 0).mean():.4f} of elements differ"


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("B,T,C,n_mix,with_delta", [(3, 1, 128, 6, True), (2, 4, 768, 6, True), (5, 1, 4096, 1, True),
                                                    (2, 3, 256, 1, False), (4, 1, 2048, 0, True), (200, 1, 4096, 6, True)])
def test_add_ln_mix(B, T, C, n_mix, with_delta):
    from chirrup_amd import ops

    rng = np.random.default_rng(B * 7 + T + C)
    x = rng.standard_normal((B, T, C)).astype(F16)
    delta = (rng.standard_normal((B, T, C)) * 0.5).astype(F16) if with_delta else None
    w = (1 + 0.1 * rng.standard_normal(C)).astype(F16)
    b = (0.1 * rng.standard_normal(C)).astype(F16)
    prev = rng.standard_normal((B, C)).astype(F16)
    mix = rng.uniform(0, 1, (max(n_mix, 1), C)).astype(F16)
    # oracle
    xn = x + delta if with_delta else x
    cur = M.layer_norm(xn, w, b)
    if n_mix:
        dx = np.concatenate([prev[:, None], cur[:, :-1]], 1) - cur
        want = np.stack([cur + dx * mix[m] for m in range(n_mix)])
    else:
        want = cur[None]
    tx, tprev = cu(x), cu(prev)
    out = torch.empty((max(n_mix, 1), B, T, C), dtype=torch.float16, device="cuda")
    prev_out = tprev if T == 1 else torch.empty_like(tprev)
    x_new = tx if T == 1 else torch.empty_like(tx)       # in place only for T == 1 (T > 1: rows re-read their predecessor)
    ops.add_ln_mix(B, T, C, tx, cu(delta) if with_delta else None, x_new if with_delta else None, cu(w), cu(b), 1e-5,
                   tprev if n_mix else None, prev_out if n_mix else None, cu(mix[:n_mix]) if n_mix else None, out)
    got = out.cpu().numpy()
    if with_delta:
        assert np.array_equal(bits(x_new.cpu().numpy()), bits(xn))       # residual add is exact
    # LN outputs reach |x| ~ 4-5 (ulp 3.9e-3); a one-ulp flip there can survive a cancelling lerp
    assert_close_ulps(got, want, 2, 0.02, "mixed", atol=4e-3)
    if n_mix:
        assert_close_ulps(prev_out.cpu().numpy(), cur[:, -1], 1, 0.01, "carry")


@pytest.mark.parametrize("regime,B,T,C", [("offset", 3, 1, 768), ("offset", 5, 5, 4096), ("outlier", 4, 5, 768), ("outlier", 200, 1, 4096)])
def test_add_ln_mix_offset_and_outlier_rows(regime, B, T, C):
    """LayerNorm + token shift on rows whose mean is 20-50 x their spread and on rows with three channels at 100 x the rest, with
    slot_idx and the side carry table, against the binary64 interval reference (tests/tmix_ref.ln_mix_reference): the residual
    sum is exact, the six mixed planes and the carried row lie in their intervals (bit-equal where those are one half), carry rows
    of other slots are untouched."""
    import tmix_ref as R
    from chirrup_amd import ops

    li = R.ln_inputs(B, T, C, regime, seed=B + T + C)
    ref = R.ln_mix_reference(li["x"], li["delta"], li["w"], li["b"], li["prev"], li["mix"], slot_idx=li["slot_idx"])
    tx, tprev = cu(li["x"]), cu(li["prev"])
    n_mix = li["mix"].shape[0]
    out = torch.full((n_mix, B, T, C), float("nan"), dtype=torch.float16, device="cuda")
    prev_out = tprev if T == 1 else tprev.clone()
    x_new = tx if T == 1 else torch.empty_like(tx)
    ops.add_ln_mix(B, T, C, tx, cu(li["delta"]), x_new, cu(li["w"]), cu(li["b"]), 1e-5, tprev, prev_out, cu(li["mix"]), out,
                   slot_idx=cu(li["slot_idx"]))
    torch.cuda.synchronize()
    assert np.array_equal(bits(x_new.cpu().numpy()), bits(ref["x_new"]))
    res = R.assert_check(out.cpu().numpy(), *ref["out"], name="mixed", group=C)
    carry = prev_out.cpu().numpy()
    rc = R.assert_check(carry, *ref["carry"], name="carry", group=C)
    others = np.setdiff1d(np.arange(carry.shape[0]), li["slot_idx"])
    assert np.array_equal(bits(carry[others]), bits(li["prev"][others]))
    print(f"LN {regime} B{B} T{T} C{C}: mixed {res['single']} of {res['n']} single-pattern, carry {rc['single']} of {rc['n']}; 0 outside")
    _record_ref(f"add_ln_mix|{regime}|B{B}-T{T}-C{C}", out_bad=0, out_n=res["n"], out_single=res["single"])


@pytest.mark.parametrize("rows,C,layer0", [(3, 128, True), (7, 768, False), (200, 4096, False)])
def test_tmix_mid(rows, C, layer0):
    from chirrup_amd import ops

    rng = np.random.default_rng(rows + C)
    H = C // 64
    k = rng.standard_normal((rows, C)).astype(F16)
    v = rng.standard_normal((rows, C)).astype(F16)
    a_pre = rng.standard_normal((rows, C)).astype(F16)
    vg_pre = rng.standard_normal((rows, C)).astype(F16)
    v_first = rng.standard_normal((rows, C)).astype(F16)
    k_k = (0.85 + 0.05 * rng.standard_normal(C)).astype(F16)
    k_a = (1 + 0.05 * rng.standard_normal(C)).astype(F16)
    # oracle: oracle/rwkv7_np.tmix lines for rwkv7.py:629-637
    a = M.sigmoid_h(a_pre)
    kk_in = (k * k_k).reshape(rows, H, 64)
    nrm = np.sqrt((kk_in.astype(F32) ** 2).sum(-1, keepdims=True, dtype=F32)).astype(F16)
    kk = (kk_in / np.maximum(nrm, F16(1e-12))).reshape(rows, C)
    k_want = k * (F16(1.0) + (a - F16(1.0)) * k_a)
    kka_want = kk * a
    v_want = v if layer0 else v + (v_first - v) * M.sigmoid_h(vg_pre)
    tk, tv = cu(k), cu(v)
    nk, kka = torch.empty_like(tk), torch.empty_like(tk)
    ops.tmix_mid(rows, C, tk, tv, cu(a_pre), None if layer0 else cu(vg_pre), None if layer0 else cu(v_first), cu(k_k),
                 cu(k_a), nk, kka)
    assert_close_ulps(tk.cpu().numpy(), k_want, 1, 0.005, "k")          # sigmoid: device expf vs numpy
    assert_close_ulps(nk.cpu().numpy(), -kk, 1, 0.01, "neg_kk")
    assert_close_ulps(kka.cpu().numpy(), kka_want, 2, 0.02, "kka")
    assert_close_ulps(tv.cpu().numpy(), v_want, 1, 0.005, "v")
    # ... and against the binary64 interval reference: bit-equal wherever sigmoid and norm are unambiguous
    import tmix_ref as R
    iv = R.mid_interval(k, v, a_pre, vg_pre, v_first, k_k, k_a, layer0)
    for name, got in (("k", tk), ("neg_kk", nk), ("kka", kka), ("v", tv)):
        R.assert_check(got.cpu().numpy(), *iv[name], name=name)


@pytest.mark.parametrize("rows,C", [(3, 128), (7, 768), (200, 4096)])
def test_tmix_post(rows, C):
    from chirrup_amd import ops

    rng = np.random.default_rng(rows * 3 + C)
    H = C // 64
    y = (rng.standard_normal((rows, C)) * 2).astype(F16)
    r, k, v, g = (rng.standard_normal((rows, C)).astype(F16) for _ in range(4))
    r_k = (0.1 * rng.standard_normal(C)).astype(F16)
    w = (1 + 0.1 * rng.standard_normal(C)).astype(F16)
    b = (0.1 * rng.standard_normal(C)).astype(F16)
    gn = M.group_norm_heads(y, H, w, b)
    bonus = ((r * k * r_k).reshape(rows, H, 64).astype(F32).sum(-1, keepdims=True, dtype=F32)).astype(F16)
    want = (gn + (bonus * v.reshape(rows, H, 64)).reshape(rows, C)) * g
    out = torch.empty((rows, C), dtype=torch.float16, device="cuda")
    ops.tmix_post(rows, C, cu(y), cu(r), cu(k), cu(v), cu(g), cu(r_k), cu(w), cu(b), 64e-5, out)
    assert_close_ulps(out.cpu().numpy(), want, 2, 0.03, "out")
    import tmix_ref as R
    lo, hi = R.post_interval(y, r, k, v, g, r_k, w, b, H)[:2]
    R.assert_check(out.cpu().numpy(), lo, hi)


def test_relu_sq_exact():
    from chirrup_amd import ops

    rng = np.random.default_rng(0)
    x = (rng.standard_normal((200, 16384)) * 3).astype(F16)
    x[0, :4] = [F16(-0.0), F16(0.0), F16(250.0), F16(300.0)]          # 300^2 overflows to inf like torch
    t = cu(x)
    ops.relu_sq_(t)
    with np.errstate(over="ignore"):
        want = np.maximum(x, F16(0)) * np.maximum(x, F16(0))
    assert np.array_equal(bits(t.cpu().numpy()), bits(want))


@pytest.mark.parametrize("B,T,C,layer0", [(3, 1, 128, True), (4, 3, 256, False), (200, 1, 4096, False)])
def test_fused_tmix_core_equals_three_kernel_path(oracle, B, T, C, layer0):
    """rwkv7_tmix_wkv7_fused (gating + WKV7 + group-norm/bonus/gate in one kernel) against tmix_mid ->
    wkv7_fwd_seq -> tmix_post.  Same per-op roundings; only the order of the binary32 head reductions
    differs (8-lane partials vs a 64-lane butterfly), so outputs and state may differ by an ulp on a
    small fraction of elements, never more."""
    from chirrup_amd import ops
    from util import wkv7_inputs

    rng = np.random.default_rng(B + T + C)
    H, rows = C // 64, B * T
    state, r, w, k, v, _, _, et = wkv7_inputs(B, T, C, seed=B * 3 + C)
    mk = lambda s=1.0: (rng.standard_normal((B, T, C)) * s).astype(F16)
    a_pre, vg_pre, v_first, g = mk(), mk(), mk(), mk()
    k_k = (0.85 + 0.05 * rng.standard_normal(C)).astype(F16)
    k_a = (1 + 0.05 * rng.standard_normal(C)).astype(F16)
    r_k = (0.1 * rng.standard_normal(C)).astype(F16)
    lw = (1 + 0.1 * rng.standard_normal(C)).astype(F16)
    lb = (0.1 * rng.standard_normal(C)).astype(F16)
    # three-kernel path
    tk, tv = cu(k), cu(v)
    nk, kka = torch.empty_like(tk), torch.empty_like(tk)
    ops.tmix_mid(rows, C, tk, tv, cu(a_pre), None if layer0 else cu(vg_pre), None if layer0 else cu(v_first), cu(k_k), cu(k_a), nk, kka)
    S3 = cu(state)
    y = torch.empty((B, T, C), dtype=torch.float16, device="cuda")
    ops.forward_seq(B, T, C, H, S3, cu(r), cu(w), tk, tv, nk, kka, y, cu(et))
    out3 = torch.empty_like(y)
    ops.tmix_post(rows, C, y, cu(r), tk, tv, cu(g), cu(r_k), cu(lw), cu(lb), 64e-5, out3)
    # fused
    S1 = cu(state)
    out1 = torch.empty((B, T, C), dtype=torch.float16, device="cuda")
    ops.tmix_wkv7_fused(B, T, C, H, S1, cu(r), cu(w), cu(k), cu(v), cu(a_pre), None if layer0 else cu(vg_pre),
                        None if layer0 else cu(v_first), cu(g), cu(k_k), cu(k_a), cu(r_k), cu(lw), cu(lb), 64e-5, out1, cu(et))
    s_a, s_b = S1.cpu().numpy(), S3.cpu().numpy()
    scale = max(1.0, float(np.abs(s_b.astype(F32)).max()))
    assert (bits(s_a) != bits(s_b)).mean() < 0.02
    assert float(np.abs(s_a.astype(F32) - s_b.astype(F32)).max()) <= 2e-3 * scale
    assert_close_ulps(out1.cpu().numpy(), out3.cpu().numpy(), 2, 0.05, "out", atol=4e-3 * max(1.0, float(out3.abs().max())))


@pytest.mark.parametrize("B,T,C,layer0", [(3, 1, 128, True), (4, 3, 256, False), (64, 1, 4096, False)])
def test_fused_tmix_core_with_the_mm8_prologue_is_the_same_kernel(B, T, C, layer0):
    """The mm8 prologue of the fused time-mix core is a template form of its own (as a run-time branch it cost the binary16 form
    a wave per SIMD).  With ry = 1 the prologue's xs = binary16(o * ry) IS o: both forms must write the same output
    and state bits, and the prologue's third row sum must be the sum of o over the head."""
    from chirrup_amd import ops
    from util import wkv7_inputs

    rng = np.random.default_rng(B + T + C + 7)
    H = C // 64
    state, r, w, k, v, _, _, et = wkv7_inputs(B, T, C, seed=B * 5 + C)
    mk = lambda s=1.0: (rng.standard_normal((B, T, C)) * s).astype(F16)
    a_pre, vg_pre, v_first, g = mk(), mk(), mk(), mk()
    k_k = (0.85 + 0.05 * rng.standard_normal(C)).astype(F16)
    k_a = (1 + 0.05 * rng.standard_normal(C)).astype(F16)
    r_k = (0.1 * rng.standard_normal(C)).astype(F16)
    lw = (1 + 0.1 * rng.standard_normal(C)).astype(F16)
    lb = (0.1 * rng.standard_normal(C)).astype(F16)
    res = []
    for prologue in (False, True):
        S = cu(state)
        out = torch.empty((B, T, C), dtype=torch.float16, device="cuda")
        mm8_out = None
        if prologue:
            sums = torch.full((B * T, H, 3), float("nan"), dtype=torch.float32, device="cuda")
            mm8_out = (torch.ones(C, dtype=torch.float16, device="cuda"), torch.zeros(C, dtype=torch.float16, device="cuda"), sums)
        ops.tmix_wkv7_fused(B, T, C, H, S, cu(r), cu(w), cu(k), cu(v), cu(a_pre), None if layer0 else cu(vg_pre),
                            None if layer0 else cu(v_first), cu(g), cu(k_k), cu(k_a), cu(r_k), cu(lw), cu(lb), 64e-5, out, cu(et),
                            mm8_out=mm8_out)
        torch.cuda.synchronize()
        res.append((out, S, mm8_out[2] if prologue else None))
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))
    assert torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16))
    sums = res[1][2]
    want = res[0][0].float().view(B * T, H, 64).sum(-1)
    assert torch.allclose(sums[..., 0], want, rtol=1e-5, atol=1e-3) and torch.allclose(sums[..., 2], want, rtol=1e-5, atol=1e-3)
    assert float(sums[..., 1].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------
# The fused time-mix core against the binary64 interval reference of tests/tmix_ref.py: state bit for bit over the WHOLE pool
# (untouched slots included), out bit for bit where the reference is unambiguous and inside its interval of halves elsewhere.
# tests/test_tmix_ref_cpu.py shows on the CPU that this check rejects defective evaluations and accepts legitimate ones.

def _record_ref(case, **fields):
    """One JSON line per case in the file $CHIRRUP_TMIX_REF_LOG names, when it is set: the figures of DESIGN.md's table."""
    import json
    import os

    path = os.environ.get("CHIRRUP_TMIX_REF_LOG")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, **fields}, sort_keys=True) + "\n")
    except OSError:
        pass


def _launch_fused(inp, S, mm8_out=None):
    """One launch of ops.tmix_wkv7_fused on the inputs of tmix_ref.make_inputs; S: the cuda state (a pool or a view of one)."""
    from chirrup_amd import ops

    B, T, C = inp["k"].shape
    out = torch.full((B, T, C), float("nan"), dtype=torch.float16, device="cuda")
    l0 = inp["layer0"]
    ops.tmix_wkv7_fused(B, T, C, C // 64, S, cu(inp["r"]), cu(inp["w"]), cu(inp["k"]), cu(inp["v"]), cu(inp["a_pre"]),
                        None if l0 else cu(inp["vg_pre"]), None if l0 else cu(inp["v_first"]), cu(inp["g"]), cu(inp["k_k"]), cu(inp["k_a"]),
                        cu(inp["r_k"]), cu(inp["lnx_w"]), cu(inp["lnx_b"]), inp["eps"], out, cu(inp["et"]),
                        slot_idx=None if inp["slot_idx"] is None else cu(inp["slot_idx"]), mm8_out=mm8_out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_state_and_out(case, got_state, got_out, ref):
    import tmix_ref as R

    n_state = int((bits(got_state) != bits(ref["state"])).sum())
    res = R.check(got_out, ref["lo"], ref["hi"], ref["mid"])
    print(f"{case}: state elements differing {n_state} of {got_state.size}; out: {res['bad']} outside, {res['single']} of {res['n']} "
          f"single-pattern, {res['off_nearest']} admissible but not the nearest half")
    _record_ref(case, state_diff=n_state, state_n=int(got_state.size), out_bad=res["bad"], out_n=res["n"], out_single=res["single"],
                out_off_nearest=res["off_nearest"])
    assert n_state == 0, f"{case}: {n_state} state elements differ from the reference"
    assert res["bad"] == 0, f"{case}: {res['msg']}"


def _fused_case_names():
    import tmix_ref as R
    return list(R.CASES)


@pytest.mark.parametrize("name", _fused_case_names())
def test_fused_tmix_core_against_interval_reference(oracle, name):
    import tmix_ref as R

    inp, _ = R.case_inputs(name)
    ref = R.reference(inp)
    assert ref["amb_gate"] == 0 and ref["amb_norm"] == 0
    S = cu(inp["state"])
    out = _launch_fused(inp, S)
    _assert_state_and_out(name, S.cpu().numpy(), out, ref)


def test_fused_tmix_core_view_into_layer_pool(oracle):
    """state = pool[layer][lo:hi], a contiguous view of [L, n, H, 64, 64], with slot_idx into the view: the other layers, the
    slots outside the view and the slots of the view that slot_idx does not name stay bit-identical."""
    import tmix_ref as R

    L_, n, C, lo, hi = 3, 9, 128, 2, 8
    rng = np.random.default_rng(9)
    pool = (rng.standard_normal((L_, n, C // 64, 64, 64)) * 0.5).astype(F16)
    inp, _ = R.make_inputs(3, 2, C, layer0=False, regime="plain", seed=21, n_slots=hi - lo, state=pool[1, lo:hi].copy())
    assert sorted(inp["slot_idx"].tolist()) != list(range(3))
    ref = R.reference(inp)
    t_pool = cu(pool)
    out = _launch_fused(inp, t_pool[1][lo:hi])
    want = pool.copy()
    want[1, lo:hi] = ref["state"]
    touched = np.zeros(pool.shape[:2], bool)
    touched[1, lo + inp["slot_idx"]] = True
    assert np.array_equal(bits(want[~touched]), bits(pool[~touched]))          # (the reference itself leaves them alone)
    got = t_pool.cpu().numpy()
    assert np.array_equal(bits(got[~touched]), bits(pool[~touched])), "a slot outside slot_idx was written"
    ref = dict(ref, state=want)
    _assert_state_and_out("view-into-layer-pool", got, out, ref)


def test_fused_tmix_core_edge_values(oracle):
    """Zero / subnormal / -0.0 state, w = +-60000, a_pre / vg_pre = +-60000 (sigmoid exactly 1 / 0), g = +-0, v_first == v,
    elapsed_t that wraps the int32 multiply, and one head with k = 0: F.normalize gives 0/0 there (clamp_min(1e-12) is 0 in
    binary16), so exactly that head's state rows and output channels of that slot are NaN -- compared by mask, not by payload."""
    import tmix_ref as R

    inp, _ = R.make_inputs(**R.EDGE_CASE)
    ref = R.reference(inp)
    S = cu(inp["state"])
    out = _launch_fused(inp, S)
    got = S.cpu().numpy()
    b, hd = inp["zero_head"]
    want_nan = np.zeros(got.shape, bool)
    want_nan[b, hd] = True
    assert np.array_equal(np.isnan(ref["state"]), want_nan)
    assert np.array_equal(np.isnan(got), want_nan), "NaN outside (or missing inside) the k = 0 head's state"
    out_nan = np.zeros(out.shape, bool)
    out_nan[b, :, hd * 64:(hd + 1) * 64] = True
    assert np.array_equal(np.isnan(out), out_nan), "NaN outside (or missing inside) the k = 0 head's outputs"
    n_state = int((bits(got)[~want_nan] != bits(ref["state"])[~want_nan]).sum())
    res = R.check(out, ref["lo"], ref["hi"], ref["mid"])
    print(f"edge values: state elements differing {n_state}; out: {res['bad']} outside, {res['off_nearest']} not the nearest half")
    _record_ref("edge-values", state_diff=n_state, state_n=int(got.size), out_bad=res["bad"], out_n=res["n"], out_single=res["single"],
                out_off_nearest=res["off_nearest"])
    assert n_state == 0
    assert res["bad"] == 0, res["msg"]


def test_fused_tmix_core_64_chained_steps(oracle):
    """64 T = 1 launches on one state with fresh guarded inputs and an advancing elapsed_t: out checked at every step, the state
    bit-equal at the end (and, since the reference's state feeds the next step's reference, at every step)."""
    import tmix_ref as R

    S = None
    worst = dict(bad=0, off_nearest=0, n=0, single=0)
    for step, (inp, ref) in enumerate(R.chain_inputs(steps=64)):
        if S is None:
            S = cu(inp["state"])
        out = _launch_fused(inp, S)
        res = R.check(out, ref["lo"], ref["hi"], ref["mid"])
        assert res["bad"] == 0, f"step {step}: {res['msg']}"
        for k_ in worst:
            worst[k_] += res[k_]
        assert np.array_equal(bits(S.cpu().numpy()), bits(ref["state"])), f"state differs after step {step}"
    assert np.isfinite(ref["state"].astype(F32)).all()
    print(f"64 chained steps: state equal at every step; out: {worst['single']} of {worst['n']} single-pattern, {worst['off_nearest']} not the nearest half")
    _record_ref("chained-64-steps", state_diff=0, state_n=int(ref["state"].size), out_bad=0, out_n=worst["n"], out_single=worst["single"],
                out_off_nearest=worst["off_nearest"])


@pytest.mark.parametrize("name", ["plain-B3-T2-C128", "plain-B1-T31-C768", "offset-B200-T1-C4096-layer0", "outlier-B256-T1-C128",
                                  "plain-B256-T1-C2048-layer0"])
def test_fused_tmix_core_mm8_prologue_against_reference(oracle, name):
    """MODE 2 with ry, my of a quantised att.output-shaped matrix (chirrup_amd.quant.quantize_linear): the state is MODE 1's and the
    reference's bit for bit, xs == h(out1 * ry) bit for bit for MODE 1's out1 of the same inputs, and each of the three row sums per
    head is within gamma_64 * sum|terms| of the binary64 sum of exactly those halves."""
    import tmix_ref as R
    from chirrup_amd.quant import quantize_linear

    inp, _ = R.case_inputs(name)
    B, T, C = inp["k"].shape
    H = C // 64
    torch.manual_seed(C + B)
    W8 = quantize_linear((torch.randn(C, C, device="cuda") / C ** 0.5).half())
    ry, my = W8.ry.contiguous(), W8.my.contiguous()
    ref = R.reference(inp, ry=ry.cpu().numpy())
    assert float((ry.float() - 1).abs().min()) > 0 and float(my.float().abs().max()) > 0       # not the trivial ry = 1, my = 0
    S1 = cu(inp["state"])
    out1 = _launch_fused(inp, S1)
    _assert_state_and_out(name + "|mode1", S1.cpu().numpy(), out1, ref)
    S2 = cu(inp["state"])
    sums = torch.full((B * T, H, 3), float("nan"), dtype=torch.float32, device="cuda")
    xs = _launch_fused(inp, S2, mm8_out=(ry, my, sums))
    assert np.array_equal(bits(S2.cpu().numpy()), bits(ref["state"]))
    R.assert_check(xs, ref["xs_lo"], ref["xs_hi"], name="xs")                 # ... inside the reference's own corners
    xs_want, S_want, bound = R.mm8_reference(out1, ry.cpu().numpy(), my.cpu().numpy())
    assert np.array_equal(bits(xs), bits(xs_want)), f"{int((bits(xs) != bits(xs_want)).sum())} xs elements differ from h(out1 * ry)"
    err = np.abs(sums.cpu().numpy().astype(np.float64) - S_want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{name}: mm8 row sums: worst error / bound {ratio:.3f} (columns: {[float((err[..., j] / np.maximum(bound[..., j], 1e-300)).max()) for j in range(3)]})")
    _record_ref(name + "|mm8", sums_err_over_bound=ratio, xs_diff=0)
    assert (err <= bound).all(), f"row sums outside gamma_64 * sum|terms|: worst ratio {ratio}"


@pytest.mark.parametrize("name", ["plain-B3-T2-C128", "plain-B3-T5-C64-layer0", "offset-B3-T1-C768", "offset-B3-T5-C2048",
                                  "outlier-B3-T2-C768-layer0", "outlier-B256-T1-C128", "offset-B200-T1-C4096-layer0"])
def test_three_kernel_path_against_interval_reference(oracle, name):
    """tmix_mid -> wkv7_fwd_seq -> tmix_post held to the same reference, in the plain, offset and outlier regimes: the gating
    outputs k', -kk, kk*a, v' are observable here and must equal the reference bit for bit (guarded inputs), so must the state
    and y; out by the interval check."""
    import tmix_ref as R
    from chirrup_amd import ops

    inp, _ = R.case_inputs(name)
    ref = R.reference(inp)
    B, T, C = inp["k"].shape
    rows, l0 = B * T, inp["layer0"]
    tk, tv = cu(inp["k"]), cu(inp["v"])
    nk, kka = torch.empty_like(tk), torch.empty_like(tk)
    ops.tmix_mid(rows, C, tk, tv, cu(inp["a_pre"]), None if l0 else cu(inp["vg_pre"]), None if l0 else cu(inp["v_first"]), cu(inp["k_k"]),
                 cu(inp["k_a"]), nk, kka)
    for nm, got, want in (("k'", tk, ref["k2"]), ("-kk", nk, ref["neg_kk"]), ("kk*a", kka, ref["kka"]), ("v'", tv, ref["v2"])):
        nd = int((bits(got.cpu().numpy()) != bits(want)).sum())
        assert nd == 0, f"{name}: {nd} elements of {nm} differ from the reference"
    S = cu(inp["state"])
    y = torch.empty((B, T, C), dtype=torch.float16, device="cuda")
    ops.forward_seq(B, T, C, C // 64, S, cu(inp["r"]), cu(inp["w"]), tk, tv, nk, kka, y, cu(inp["et"]),
                    slot_idx=None if inp["slot_idx"] is None else cu(inp["slot_idx"]))
    assert np.array_equal(bits(y.cpu().numpy()), bits(ref["y"]))
    out = torch.empty_like(y)
    ops.tmix_post(rows, C, y, cu(inp["r"]), tk, tv, cu(inp["g"]), cu(inp["r_k"]), cu(inp["lnx_w"]), cu(inp["lnx_b"]), inp["eps"], out)
    _assert_state_and_out(name + "|three-kernel", S.cpu().numpy(), out.cpu().numpy(), ref)


def test_lora_act_exhaustive():
    """rwkv7_lora_act on all 65 536 binary16 bit patterns as one plane each of [v, w, a, g] (plus 40 padding elements, so that the
    plane is not a multiple of the 256-lane block's 2048 elements): v and a planes unchanged bit for bit (NaN payloads included),
    w = the correctly rounded tanh and g = the correctly rounded sigmoid on every input whose result is unambiguous under the
    4-binary32-ulp assumption of tests/tmix_ref.py, inside the two-half interval on the others; NaN in, NaN out."""
    import tmix_ref as R
    from chirrup_amd import ops

    allbits = np.arange(65536, dtype=np.uint16)
    plane = np.concatenate([allbits, allbits[15360:15400]]).view(F16)          # 65 576 elements = 8197 chunks of 8
    xf = plane.astype(np.float64)
    names = ["v", "w", "a", "g"]
    for first, n in ((0, 4), (1, 3), (3, 1), (1, 1), (0, 1)):
        hbuf = cu(np.stack([plane] * n).reshape(n, 1, -1))
        ops.lora_act_(hbuf, first)
        torch.cuda.synchronize()
        got = hbuf.cpu().numpy().reshape(n, -1)
        for j in range(n):
            which = names[first + j]
            if which in ("v", "a"):
                assert np.array_equal(bits(got[j]), bits(plane)), f"plane {which} (first_plane {first}) was modified"
                continue
            kind = "tanh" if which == "w" else "sigmoid"
            lo, hi = R.act_table(kind)
            lo, hi = lo[bits(plane)], hi[bits(plane)]
            res = R.check(got[j], lo, hi)
            with np.errstate(over="ignore", invalid="ignore"):
                exact = np.tanh(xf) if kind == "tanh" else 1.0 / (1.0 + np.exp(-xf))
            near = exact.astype(F16)
            not_cr = int(((bits(got[j]) != bits(near)) & ~np.isnan(plane))[:65536].sum())
            print(f"lora_act {kind} first_plane {first} nplanes {n}: {res['bad']} outside, {not_cr} of 63488 finite inputs not the correctly rounded half")
            if first == 0 or n == 1:
                _record_ref(f"lora_act|{kind}|first{first}|n{n}", out_bad=res["bad"], not_correctly_rounded=not_cr)
            if res["bad"]:
                # distance of the binary64 value from the rounding boundary it would have to cross, in binary32 ulps: a lower bound
                # on the device function's error at that input
                bad = np.flatnonzero(((R.key(np.nan_to_num(got[j])) < R.key(np.nan_to_num(lo))) | (R.key(np.nan_to_num(got[j])) > R.key(np.nan_to_num(hi)))) & ~np.isnan(plane))
                for i in bad[:20]:
                    step = np.nextafter(near[i], got[j][i], dtype=F16)             # the neighbour of the correct half towards the device's
                    boundary = (float(step) + float(near[i])) / 2
                    print(f"   input {plane[i]!r} (bits {bits(plane)[i]:#06x}): device {got[j][i]!r}, binary64 {exact[i]!r}, "
                          f"{abs(exact[i] - boundary) / R.ulp32(exact[i]):.2f} binary32 ulps from the boundary")
            assert res["bad"] == 0, f"lora_act {kind} (first_plane {first}): {res['msg']}"


@pytest.mark.parametrize("rows,C", [(5, 128), (200, 1024)])
def test_mm8_chain_folded_into_neighbouring_kernels_equals_mm8t_linear(rows, C):
    """Decode-regime mm8 FFN: the activation prologue of ffn.key written by the LN kernel, corrections + relu^2 of ffn.key
    and the prologue of ffn.value in ONE row kernel, corrections of ffn.value in the next LN kernel -- the same operations
    and rounding points as the stand-alone mm8t_linear calls (bit-identical up to the order of the binary32 row sums)."""
    from chirrup_amd import ops
    from chirrup_amd.quant import quantize_linear

    torch.manual_seed(rows + C)
    dev = "cuda"
    K8 = quantize_linear((torch.randn(4 * C, C, device=dev) / C ** 0.5).half())
    V8 = quantize_linear((torch.randn(C, 4 * C, device=dev) / (4 * C) ** 0.5).half())
    x = torch.randn(rows, 1, C, device=dev).half()
    att = (torch.randn(rows, 1, C, device=dev) * 0.3).half()
    w, b = (1 + 0.1 * torch.randn(C, device=dev)).half(), (0.1 * torch.randn(C, device=dev)).half()
    prev, mix = torch.randn(rows, C, device=dev).half(), torch.rand(1, C, device=dev).half()
    # reference: separate launches
    x_ref, prev_ref = x.clone(), prev.clone()
    kin_ref = torch.empty(1, rows, 1, C, dtype=torch.float16, device=dev)
    ops.add_ln_mix(rows, 1, C, x_ref, att, x_ref, w, b, 1e-5, prev_ref, prev_ref, mix, kin_ref)
    kf_ref = ops.mm8t_linear(kin_ref[0].view(rows, C), *K8, act=1)
    d_ref = ops.mm8t_linear(kf_ref, *V8)
    x2_ref, out_ref = x_ref.clone(), torch.empty(1, rows, 1, C, dtype=torch.float16, device=dev)
    ops.add_ln_mix(rows, 1, C, x2_ref, d_ref.view(rows, 1, C), x2_ref, w, b, 1e-5, None, None, None, out_ref)
    # fused chain
    f32 = dict(dtype=torch.float32, device=dev)
    x_f, prev_f = x.clone(), prev.clone()
    kin = torch.empty(1, rows, 1, C, dtype=torch.float16, device=dev)
    xs_k, S_k = torch.empty(rows, C, dtype=torch.float16, device=dev), torch.empty(rows, 3, **f32)
    xs_v, S_v = torch.empty(rows, 4 * C, dtype=torch.float16, device=dev), torch.empty(rows, ops.mm8_row_parts(4 * C), 3, **f32)
    ops.add_ln_mix(rows, 1, C, x_f, att, x_f, w, b, 1e-5, prev_f, prev_f, mix, kin, mm8_out=(K8.ry, K8.my, xs_k, S_k))
    assert torch.equal(kin, kin_ref) and torch.equal(prev_f, prev_ref)
    pk = torch.empty(16, rows, 4 * C, **f32)
    kparts = ops.mm8t_gemm_partial(xs_k, K8.qT, 4 * C, 0, pk)
    kf = torch.empty(rows, 4 * C, dtype=torch.float16, device=dev)
    ops.mm8_reduce_rows(kparts, K8.rx, K8.mx, S_k, act=1, y=kf, nxt=(V8.ry, V8.my, xs_v, S_v))
    assert torch.equal(kf, kf_ref)
    pv = torch.empty(16, rows, C, **f32)
    vparts = ops.mm8t_gemm_partial(xs_v, V8.qT, C, 0, pv)
    out = torch.empty(1, rows, 1, C, dtype=torch.float16, device=dev)
    ops.add_ln_mix(rows, 1, C, x_f, None, x_f, w, b, 1e-5, None, None, None, out, delta_partials=vparts.view(-1, rows, C),
                   mm8_in=(V8.rx, V8.mx, S_v))
    # the row sums S of ffn.value's prologue are binary32 sums in another order here (1024-lane row kernel vs the
    # stand-alone prologue kernel): a delta may move by one binary16 ulp on a few elements, never more
    dx = (x_f.float() - x2_ref.float()).abs()
    assert float(dx.max()) <= 4e-3 and float((dx > 0).float().mean()) < 0.10      # (the 1024*S0 term of the u8 offset makes delta that sensitive to the order of the S0 sum)
    assert float((out.float() - out_ref.float()).abs().max()) <= 8e-3


@pytest.mark.parametrize("B,T,C,V", [(5, 1, 128, 1000), (3, 4, 768, 65536), (200, 1, 4096, 65536)])
def test_embed_rows_and_advance_elapsed_equal_the_torch_ops(B, T, C, V):
    """The two ends of a decode step as one launch each (include/chirrup_amd.h: rwkv7_embed_rows, rwkv7_advance_elapsed) against
    the torch statements they replace: the embedding gather with fed-back ids for negative tokens (rwkv7.py:503-517 + the worker's
    id feedback), the slots' step counters in row order, the zeroing of the launch-sync words, and state[2] += T over a slot list."""
    from chirrup_amd import ops

    g = torch.Generator(device="cpu").manual_seed(B + T + C)
    dev = "cuda"
    emb = torch.randn(V, C, generator=g).half().to(dev)
    n_slots = B + 7
    slots = torch.randperm(n_slots, generator=g)[:B].to(torch.int32).to(dev)
    tokens = torch.randint(0, V, (B, T), generator=g).to(dev)
    tokens[::2, 0] = -1                                    # these rows take the id fed back for their slot
    feedback = torch.randint(0, V, (n_slots,), generator=g).to(torch.int32).to(dev)
    pool = torch.randint(0, 1000, (n_slots,), generator=g).to(torch.int32).to(dev)
    arena, _ = ops._sync_arena(emb.device)
    arena.fill_(7)
    x, rows = ops.embed_rows(emb, tokens, slots, feedback, zero_sync=True, elapsed_pool=pool)
    want_tok = torch.where(tokens < 0, feedback[slots.long()].long().view(B, 1), tokens)
    assert torch.equal(x.view(torch.int16), emb[want_tok].view(torch.int16))
    assert torch.equal(rows, pool[slots.long()])
    assert int(arena.abs().sum()) == 0
    # without slots / feedback / extras: the plain gather; an id outside the table gives a zero row
    tok2 = torch.randint(0, V, (B, T), generator=g).to(dev)
    assert torch.equal(ops.embed_rows(emb, tok2).view(torch.int16), emb[tok2].view(torch.int16))
    tok2[0, 0] = V + 5
    assert float(ops.embed_rows(emb, tok2)[0, 0].abs().max()) == 0.0
    # state[2] += T
    before = pool.clone()
    ops.advance_elapsed(pool, T, slots)
    want = before.clone()
    want[slots.long()] += T
    assert torch.equal(pool, want)
    flat = torch.arange(B, dtype=torch.int32, device=dev)
    ops.advance_elapsed(flat, 3)
    assert torch.equal(flat, torch.arange(B, dtype=torch.int32, device=dev) + 3)


def test_copy_slot_rows_equals_index_copy():
    from chirrup_amd import ops

    g = torch.Generator(device="cpu").manual_seed(3)
    for n_slots, B, C in ((9, 4, 128), (201, 200, 4096)):
        src = torch.randn(n_slots, C, generator=g).half().cuda()
        dst = torch.randn(n_slots, C, generator=g).half().cuda()
        slots = torch.randperm(n_slots, generator=g)[:B].to(torch.int32).cuda()
        want = dst.clone()
        want.index_copy_(0, slots.long(), src.index_select(0, slots.long()))
        ops.copy_slot_rows(src, dst, slots)
        assert torch.equal(dst.view(torch.int16), want.view(torch.int16))
