"""Every skinny GEMM entry point (csrc/skinny_gemm.hip) against the exact reference of tests/gemm_ref.py: operands on a coarse dyadic
grid make every binary32 sum exact in any order (the exact-sum lemma; proved per case on the CPU by tests/test_gemm_ref_cpu.py), so
each output has ONE admissible binary16 pattern and every assertion here is bit equality -- except the tanh / sigmoid planes (the
table of tmix_ref.act_table) and the up-projections they feed (an interval around the binary64 product of the kernel's own hidden
plane).  Operands are views inside NaN parents (a read past M, N, K or k_of poisons the result), outputs and partial buffers views
inside sentinel parents (a write past them shows).  Each test prints one line per check: elements compared, mismatches (asserted 0),
table-ambiguous / undecided elements."""
import numpy as np
import pytest
import torch

import gemm_ref as G
from tmix_ref import bits

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64
SENT16, SENT32 = F16(-1234.0), F32(-7777.0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """A tensor as a strided view inside a parent filled with `fill`."""

    def __init__(self, arr, fill, pad_rows=2, pad_cols=8):
        parent, self.idx = G.embed(arr, pad_rows, pad_cols, fill)
        self.fill, self.parent = fill, T(parent)
        self.view = self.parent[self.idx]

    def get(self):
        return self.view.cpu().numpy()

    def intact(self):
        return G.guards_intact(self.parent.cpu().numpy(), self.idx, self.fill)

    def poison(self):
        self.view.fill_(float("nan"))


def operand(a, **kw):
    return None if a is None else Guarded(a, np.nan, **kw).view


def rows_operand(a):
    """A CONTIGUOUS operand (the entry point asks for one) between NaN rows: 1-D, or 2-D with whole guard rows above and below."""
    return Guarded(a, np.nan, pad_rows=4, pad_cols=8 if np.ndim(a) == 1 else 0).view


class FlatGuarded:
    """A contiguous tensor of `shape` filled with NaN, between two runs of a sentinel in one flat parent."""

    def __init__(self, shape, pad=64):
        self.n, self.pad = int(np.prod(shape)), pad
        self.parent = torch.full((self.n + 2 * pad,), float(SENT16), device="cuda", dtype=torch.float16)
        self.view = self.parent[pad:pad + self.n].view(*shape)

    def poison(self):
        self.view.fill_(float("nan"))

    def intact(self):
        p = self.parent.cpu().numpy()
        return bool((p[:self.pad] == SENT16).all() and (p[self.pad + self.n:] == SENT16).all())


def output(shape, dtype=F16, **kw):
    return Guarded(np.full(shape, np.nan, dtype), SENT16 if dtype == F16 else SENT32, **kw)


def note(name, res, extra=""):
    print(f"GEMMREF {name}: n={res['n']} bad={res['bad']} ambiguous={res.get('ambiguous', 0)}{extra}")


def operands(case, k=None):
    x, w, b = G.halves(case)
    if k is not None:                                       # beyond the reduction length: NaN
        x, w = x.copy(), w.copy()
        x[:, k:], w[:, k:] = np.nan, np.nan
    return operand(x), operand(w), operand(b)


NARROW = [n for n in G.F16_CASES if not n.startswith("wide")]


@pytest.mark.parametrize("name", NARROW)
def test_skinny_linear(name):
    """splits 0 / 1 / 2 / 4 / 16, bias on and off, act 0 and 1, row halves, tile images, the in-launch reduction on and off."""
    from chirrup_amd import ops

    M, N, K, bias, splits = G.F16_CASES[name]
    case = G.f16_named(name)
    q = 2.0 ** (case["ex"] + case["ew"])
    x, w, b = operands(case)
    wt = ops.tile_weight(w) if N % 128 == 0 else None
    out = output((M, N))
    nobias = dict(case, bi=None)
    want = {(a, bb): (G.expected(case if bb else nobias, a)[0], G.exact_pre(case if bb else nobias)) for a in (0, 1) for bb in (False, True)}
    n = 0
    for s in (0, 1, 2, 4, 16):
        for act in (0, 1):
            for use_bias in ((True, False) if bias and s in (1, 4) else (bias,)):
                for halves in ((False, True) if M > 32 else (False,)):
                    for weight in ((w, wt) if wt is not None else (w,)):
                        for pair in ((True, False) if M <= 32 and s in (2, 4) and weight is w and not halves else (True,)):
                            out.poison()
                            ops.PAIR_REDUCE = pair
                            try:
                                ops.skinny_linear(x, weight, b if use_bias else None, act=act, splits=s, out=out.view, row_halves=halves)
                            finally:
                                ops.PAIR_REDUCE = True
                            lo, ex = want[(act, bool(use_bias))]
                            G.assert_bits(out.get(), lo, lo, ex, q, f"{name} s={s} act={act} bias={use_bias} halves={halves} tiled={weight is wt} pair={pair}")
                            n += lo.size
    assert out.intact()
    assert int(ops._tile_counters(x.device).abs().sum()) == 0
    note(f"skinny_linear[{name}]", dict(n=n, bad=0))


@pytest.mark.parametrize("name", ["M16-N128-K192", "M17-N132-K1024", "M113-N260-K64", "M200-N1000-K1024", "M24-N1024-K4096"])
def test_skinny_linear_partial(name):
    """Every plane exactly; planes beyond the split count and the buffer's surroundings untouched."""
    from chirrup_amd import ops

    M, N, K, _, splits = G.F16_CASES[name]
    case = G.f16_named(name)
    x, w, _ = operands(case)
    wt = ops.tile_weight(w) if N % 128 == 0 else None
    room, pad = 16 * M * N, 64
    buf = torch.empty(room + 2 * pad, device="cuda", dtype=torch.float32)
    n = 0
    for s in tuple(splits) + (0,):
        for halves in ((False, True) if M > 32 else (False,)):
            for weight in ((w, wt) if wt is not None else (w,)):
                buf.fill_(float(SENT32))
                got = ops.skinny_linear_partial(x, weight, s, buf[pad:pad + room], row_halves=halves)
                s_used = got.shape[0]                       # (the library's own choice, s = 0, depends on row_halves)
                assert tuple(got.shape) == (s_used, M, N) and (s == 0 or s_used == ops.gemm_splits(N, K, 1, s))
                want = G.expected_planes(case, s_used)
                n += G.assert_planes(got.cpu().numpy(), want, f"{name} s={s} halves={halves} tiled={weight is wt}")
                flat = buf.cpu().numpy()
                assert (flat[:pad] == SENT32).all() and (flat[pad + s_used * M * N:] == SENT32).all(), "written past the planes in use"
    note(f"skinny_linear_partial[{name}]", dict(n=n, bad=0))


@pytest.mark.parametrize("name", [n for n in G.F16_CASES if n.startswith("wide")])
def test_wide_kernel(name):
    """N = 32768 selects the 256-column kernel."""
    from chirrup_amd import ops

    M, N, K, bias, splits = G.F16_CASES[name]
    case = G.f16_named(name)
    x, w, b = operands(case)
    out = output((M, N))
    n = 0
    ex = G.exact_pre(case)
    for act in (0, 1):
        lo, _ = G.apply_act(ex, act)
        for s in ((0,) + tuple(splits) if act == 0 else (0,)):
            out.poison()
            ops.skinny_linear(x, w, b, act=act, splits=s, out=out.view)
            G.assert_bits(out.get(), lo, lo, ex, 2.0 ** -12, f"{name} s={s} act={act}")
            n += lo.size
    wt = ops.tile_weight(w)
    out.poison()
    ops.skinny_linear(x, wt, b, act=0, splits=1, out=out.view)
    lo, _ = G.apply_act(ex, 0)
    G.assert_bits(out.get(), lo, lo, ex, 2.0 ** -12, f"{name} tiled")
    assert out.intact()
    note(f"wide[{name}]", dict(n=n + lo.size, bad=0))


@pytest.mark.parametrize("M", list(G.BMM_KOF))
def test_skinny_bmm_k_of(M):
    """The LoRA up-projection launch: per-problem reduction lengths (NaN beyond them), tile images, row halves."""
    from chirrup_amd import ops

    cases, ks = G.bmm_kof_named(M)
    (N, K, _), Z, ks = G.BMM_KOF[M], len(ks), list(ks)
    hv = [G.halves(c) for c in cases]
    xs, ws = np.stack([v[0] for v in hv]), np.stack([v[1] for v in hv])
    for z, k in enumerate(ks):
        xs[z, :, k:], ws[z, :, k:] = np.nan, np.nan
    x, w, b = operand(xs), operand(ws), operand(np.stack([v[2] for v in hv]))
    out = output((Z, M, N))
    lo = np.stack([G.expected(c, None, k)[0] for c, k in zip(cases, ks)])
    n = 0
    weights = [w] + ([ops.tile_weight_batch(w)] if N % 128 == 0 else [])
    for weight in weights:
        for halves in (False, True):
            out.poison()
            ops.skinny_bmm(x, weight, b, splits=1, out=out.view, k_of=ks, row_halves=halves)
            got = out.get()
            for z in range(Z):
                G.assert_bits(got[z], lo[z], lo[z], G.exact_pre(cases[z], ks[z]), 2.0 ** -12, f"bmm M={M} z={z} halves={halves} tiled={weight is not w}")
                n += lo[z].size
    assert out.intact()
    note(f"skinny_bmm_k_of[M={M}]", dict(n=n, bad=0))


@pytest.mark.parametrize("M,act,splits", G.BMM_PLANES)
def test_skinny_bmm_lora_planes(M, act, splits):
    """act 4 + p: tanh on plane w, sigmoid on plane g, in the GEMM epilogue (unsplit) and in the reduce kernel (split)."""
    from chirrup_amd import ops

    Z, (N, K) = 8 - act, G.BMM_PLANES_NK
    cases = G.bmm_planes_named(M, act)
    assert ops.gemm_splits(N, K, Z, splits) in (1, 2, 4, 8, 16)         # the split counts test_gemm_ref_cpu.py proves these cases for
    hv = [G.halves(c) for c in cases]
    x, w = operand(np.stack([v[0] for v in hv])), operand(np.stack([v[1] for v in hv]))
    out = output((Z, M, N))
    ops.skinny_bmm(x, w, None, act=act, splits=splits, out=out.view)
    got = out.get()
    n = amb = 0
    for z in range(Z):
        kind = {1: "tanh", 3: "sigmoid"}.get(z + act - 4)
        lo, hi = G.expected(cases[z], kind)
        res = G.assert_bits(got[z], lo, hi, name=f"bmm planes M={M} act={act} s={splits} z={z} ({kind})")
        n, amb = n + res["n"], amb + res["ambiguous"]
    assert out.intact()
    note(f"skinny_bmm_lora_planes[M={M},act={act},s={splits}]", dict(n=n, bad=0, ambiguous=amb))


RANKS, ACTS = G.RANKS, G.ACTS


@pytest.mark.parametrize("M,splits,halves,tiled", [(200, 1, True, True), (200, 2, False, False), (33, 0, False, True), (32, 2, False, True),
                                                     (32, 4, False, False), (17, 1, False, False), (113, 4, True, False)])
def test_skinny_group_layer_launch(M, splits, halves, tiled):
    """The seven-problem layer launch (R/K/V + four LoRA down-projections of ranks 64/128/64/192, tanh / sigmoid on two of them): epilogue
    form, reduce-kernel form and the in-launch reduction at <= 32 rows."""
    from chirrup_amd import ops

    _, C, K, _ = G.GROUP_LAYERS[M]
    main, mixed, down, _, _ = G.layer_problem(*G.GROUP_LAYERS[M])
    mx = operand(np.stack([G.h(m * 2.0 ** -3) for m in mixed]))
    rkv = operand(np.stack([G.halves(c)[1] for c in main]))
    l1 = np.full((4, 192, K), np.nan, F16)
    for j in range(4):
        l1[j, :RANKS[j]] = G.halves(down[j])[1]
    l1 = operand(l1)
    bias = G.h(np.random.default_rng(M).integers(-255, 256, C) * 2.0 ** -6)
    bias_d = operand(bias)
    out_rkv, hid = output((3, M, C)), output((4, M, 192))
    probs = [(mx[j], ops.tile_weight(rkv[j]) if tiled else rkv[j], out_rkv.view[j], bias_d if j == 1 else None, None) for j in range(3)]
    probs += [(mx[2 + j], l1[j, :RANKS[j]], hid.view[j, :, :RANKS[j]], None, ACTS[j]) for j in range(4)]
    n = amb = 0
    for it in range(3):
        out_rkv.poison(), hid.poison()
        ops.skinny_group(probs, splits=splits, row_halves=halves)
        got_r, got_h = out_rkv.get(), hid.get()
        for j in range(3):
            c = dict(main[j], bi=bias.astype(F64) * 64, eb=-6) if j == 1 else main[j]
            lo, _ = G.expected(c)
            n += G.assert_bits(got_r[j], lo, lo, G.exact_pre(c), 2.0 ** -12, f"group M={M} s={splits} rkv {j} launch {it}")["n"]
        for j in range(4):
            lo, hi = G.expected(down[j], ACTS[j])
            res = G.assert_bits(got_h[j][:, :RANKS[j]], lo, hi, name=f"group M={M} s={splits} hidden {j} ({ACTS[j]}) launch {it}")
            n, amb = n + res["n"], amb + res["ambiguous"]
            assert np.isnan(got_h[j][:, RANKS[j]:]).all(), "written past N"
        assert int(ops._tile_counters(mx.device).abs().sum()) == 0
    assert out_rkv.intact() and hid.intact()
    note(f"skinny_group[M={M},s={splits},halves={halves},tiled={tiled}]", dict(n=n, bad=0, ambiguous=amb))


@pytest.mark.parametrize("M,halves,mm8", [(1, False, False), (17, False, False), (64, False, False), (64, True, False), (200, True, False),
                                          (1, False, True), (17, False, True), (64, True, True), (64, False, True), (200, True, True)])
def test_tmix_gemms_chain(M, halves, mm8):
    """rwkv7_tmix_gemms / _mm8: R/K/V exact; hidden planes exact or inside the table; up-projections of the v and a planes exact, of the
    w and g planes inside the interval around the binary64 product of the kernel's own hidden plane.  NaN-poisoned outputs, three launches,
    status word and hand-off words zero after each."""
    from chirrup_amd import ops

    _, C, K, _ = G.TMIX_LAYERS[M]
    dmax = 192
    layer = main, mixed, down, up_w, up_b = G.layer_problem(*G.TMIX_LAYERS[M])
    mx = operand(np.stack([G.h(m * 2.0 ** -3) for m in mixed]))
    l1 = np.full((4, dmax, K), np.nan, F16)
    l2 = np.full((4, C, dmax), np.nan, F16)
    for j in range(4):
        l1[j, :RANKS[j]] = G.halves(down[j])[1]
        l2[j, :, :RANKS[j]] = G.h(up_w[j])
    l1 = operand(l1)
    l2_t = ops.tile_weight_batch(T(l2))
    lbias = operand(np.stack([G.h(b) for b in up_b]))
    rkv, up = output((3, M, C)), output((4, M, C))
    hid = FlatGuarded((4, M, dmax))                             # (the launch asks for a contiguous scratch)
    if mm8:
        m8 = G.tmix_mm8_cases(M)
        m8h = [G.mm8_halves(c) for c in m8]
        xs = operand(np.stack([v["xs"] for v in m8h]))
        main_p = [(xs[j], (ops.tile_weight_u8(T(m8h[j]["q"])), True), rkv.view[j], rows_operand(m8h[j]["rx"]), rows_operand(m8h[j]["mx"]),
                   rows_operand(m8h[j]["S"])) for j in range(3)]
        want_rkv = [G.mm8_expected(c)[0] for c in m8]
    else:
        rkv_w = operand(np.stack([G.halves(c)[1] for c in main]))
        main_p = [(mx[j], ops.tile_weight(rkv_w[j]), rkv.view[j]) for j in range(3)]
        want_rkv = [G.expected(c)[0] for c in main]
    lora_p = [(mx[2 + j], l1[j, :RANKS[j]], j, lbias[j], up.view[j], ACTS[j], RANKS[j]) for j in range(4)]
    want_hid = [G.expected(down[j], ACTS[j]) for j in range(4)]
    n = amb = und = n_int = 0
    for it in range(3):
        rkv.poison(), up.poison(), hid.poison()
        ops.tmix_gemms(main_p, lora_p, l2_t, hid.view, row_halves=halves, mm8=mm8)
        torch.cuda.synchronize()
        assert ops.chain_status() == 0
        assert all(int(t.abs().sum()) == 0 for t in ops._chain_sync.values())
        got_r, got_u, got_h = rkv.get(), up.get(), hid.view.cpu().numpy()
        for j in range(3):
            n += G.assert_bits(got_r[j], want_rkv[j], want_rkv[j], name=f"tmix M={M} mm8={mm8} rkv {j} launch {it}")["n"]
        for j in range(4):
            r = RANKS[j]
            res = G.assert_bits(got_h[j][:, :r], *want_hid[j], name=f"tmix M={M} hidden {j} ({ACTS[j]}) launch {it}")
            n, amb = n + res["n"], amb + res["ambiguous"]
            assert np.isnan(got_h[j][:, r:]).all(), "hidden plane written past its rank"
            if ACTS[j] is None:
                c = G.layer_up_case(layer, j)
                lo, _ = G.expected(c)
                n += G.assert_bits(got_u[j], lo, lo, G.exact_pre(c), 2.0 ** (c["ex"] + c["ew"]), f"tmix M={M} up {j} launch {it}")["n"]
            else:
                lo, hi = G.up_interval(got_h[j], G.h(up_w[j]), G.h(up_b[j]), r)
                res = G.assert_bits(got_u[j], lo, hi, name=f"tmix M={M} up {j} (interval) launch {it}")
                n_int, und = n_int + res["n"], und + res["ambiguous"]
    assert rkv.intact() and up.intact() and hid.intact()
    note(f"tmix_gemms[M={M},halves={halves},mm8={mm8}]", dict(n=n + n_int, bad=0, ambiguous=amb), f" interval_elements={n_int} undecided={und / max(n_int, 1):.4f}")


def mm8_dev(c):
    hv = G.mm8_halves(c)
    return {k: (operand(v) if k in ("x", "xs") else T(v) if k == "q" else rows_operand(v)) for k, v in hv.items()}


@pytest.mark.parametrize("name", list(G.MM8_CASES))
def test_mm8t_linear(name):
    """splits, tile images, act; B = 257 and 600 run as 256-row blocks."""
    from chirrup_amd import ops

    B, K, N, splits = G.MM8_CASES[name]
    c = G.mm8_named(name)
    d = mm8_dev(c)
    qt = ops.tile_weight_u8(d["q"]) if N % 128 == 0 else None
    out = output((B, N))
    n = 0
    for act in (0, 1):
        want, _ = G.mm8_expected(c, act)
        for s in (0,) + tuple(splits):
            for tiled in ((False, True) if qt is not None else (False,)):
                out.poison()
                ops.mm8t_linear(d["x"], qt if tiled else d["q"], d["mx"], d["rx"], d["my"], d["ry"], act=act, splits=s, out=out.view, tiled=tiled)
                n += G.assert_bits(out.get(), want, want, name=f"mm8t_linear {name} act={act} s={s} tiled={tiled}")["n"]
    assert out.intact()
    note(f"mm8t_linear[{name}]", dict(n=n, bad=0))


@pytest.mark.parametrize("name", [n for n in G.MM8_CASES if G.MM8_CASES[n][0] <= 256])
def test_mm8_partial_reduce_and_fused(name):
    """mm8t_gemm_partial planes exactly; mm8_reduce_rows and mm8t_gemm_fused (unsplit, and split inside the launch where it applies):
    y and the next product's xs2 exactly."""
    from chirrup_amd import ops

    B, K, N, splits = G.MM8_CASES[name]
    c = G.mm8_named(name)
    d = mm8_dev(c)
    tiled = N % 128 == 0
    qt = ops.tile_weight_u8(d["q"]) if tiled else d["q"]
    room, pad = 16 * B * N, 64
    buf = torch.empty(room + 2 * pad, device="cuda", dtype=torch.float32)
    n = 0
    for act in (0, 1):
        want_y, want_xs2 = G.mm8_expected(c, act)
        for s in splits:
            s_used = ops.gemm_splits(N, K, 1, s)
            buf.fill_(float(SENT32))
            parts = ops.mm8t_gemm_partial(d["xs"], qt, N, s, buf[pad:pad + room], tiled=tiled, row_halves=B > 32 and s == 1)
            n += G.assert_planes(parts.cpu().numpy(), G.mm8_planes(c, s_used), f"{name} mm8 planes s={s}")
            flat = buf.cpu().numpy()
            assert (flat[:pad] == SENT32).all() and (flat[pad + s_used * B * N:] == SENT32).all()
            y, xs2 = output((B, N), pad_rows=2, pad_cols=0), output((B, N), pad_rows=2, pad_cols=0)
            S2 = torch.empty(B, ops.mm8_row_parts(N), 3, device="cuda")
            ops.mm8_reduce_rows(parts, d["rx"], d["mx"], d["S"], act=act, y=y.view, nxt=(d["ry2"], d["my2"], xs2.view, S2))
            n += G.assert_bits(y.get(), want_y, want_y, name=f"{name} reduce_rows y act={act} s={s}")["n"]
            n += G.assert_bits(xs2.get(), want_xs2, want_xs2, name=f"{name} reduce_rows xs2 act={act} s={s}")["n"]
            assert y.intact() and xs2.intact()
            forms = []
            if s == 1 and N % 8 == 0:
                forms += [dict(row_halves=False)] + ([dict(row_halves=True)] if B > 32 else [])
            if s > 1 and ops.mm8_fused_split_ok(B, K, N, s):
                forms += [dict(splits=s, partials=buf[pad:pad + room])]
            for kw in forms:
                y, xs2 = output((B, N), pad_rows=2, pad_cols=0), output((B, N), pad_rows=2, pad_cols=0)
                S2 = torch.empty(B, ops.mm8_tile_parts(N), 3, device="cuda")
                ops.mm8t_gemm_fused(d["xs"], qt, N, d["rx"], d["mx"], d["S"], act=act, y=y.view, nxt=(d["ry2"], d["my2"], xs2.view, S2), tiled=tiled, **kw)
                n += G.assert_bits(y.get(), want_y, want_y, name=f"{name} fused y act={act} {sorted(kw)}")["n"]
                n += G.assert_bits(xs2.get(), want_xs2, want_xs2, name=f"{name} fused xs2 act={act} {sorted(kw)}")["n"]
                assert y.intact() and xs2.intact()
                assert int(ops._tile_counters(d["rx"].device).abs().sum()) == 0
    note(f"mm8_partial_reduce_fused[{name}]", dict(n=n, bad=0))


@pytest.mark.parametrize("name", ["B17-K1024-N1024", "B200-K512-N1024"])
def test_mm8_seq_on_the_matrix_cores(name):
    """ops.mm8_seq (two exact passes) and ops.mm8_seq_opt (the split form) through the packed MFMA kernel."""
    from chirrup_amd import ops

    B, K, N, _ = G.MM8_CASES[name]
    c = G.mm8_named(name)
    hv = G.mm8_halves(c)
    w = T(np.ascontiguousarray(hv["q"].T))                       # the reference op's [N_in, M_out]
    assert ops._mm8_packed(w, K, N) is not None
    x, mx, rx, my, ry = (operand(hv["x"]),) + tuple(rows_operand(hv[k]) for k in ("mx", "rx", "my", "ry"))
    out = output((B, N))
    want, _ = G.mm8_expected(c)
    n = 0
    for fn in (ops.mm8_seq, ops.mm8_seq_opt):
        out.poison()
        fn(B, K, N, x, w, mx, rx, my, ry, out.view)
        n += G.assert_bits(out.get(), want, want, name=f"{fn.__name__} {name}")["n"]
    assert out.intact()
    note(f"mm8_seq[{name}]", dict(n=n, bad=0))


def _all_finite_halves():
    pat = np.concatenate([np.arange(0, 0x7C00), np.arange(0x8001, 0xFC00), [0]]).astype(np.uint16)     # every finite half but -0
    return pat.view(F16).reshape(992, 64)


def test_epilogue_on_every_finite_half():
    """x = one-hot rows, W = every finite binary16 pattern except -0, 64 per row: y[m, n] = W[n, m] exactly, so the epilogue sees every
    finite half.  Plain, bias, relu^2 (exact); tanh / sigmoid (the table) through skinny_bmm act 4 and 5 and skinny_group, in the epilogue form
    (unsplit) and the reduce-kernel form (K = 128 split in two), which must give each other's bits."""
    from chirrup_amd import ops

    W = _all_finite_halves()
    N = W.shape[0]
    rng = np.random.default_rng(7)
    bias = (rng.standard_normal(N) * 4).astype(F16)
    with np.errstate(over="ignore"):
        want = {None: (W.T.copy(),) * 2, "bias": (G.h(W.T.astype(F32) + bias.astype(F32)),) * 2, "relu_sq": G.apply_act(W.T.astype(F64), 1),
                "tanh": G.apply_act(W.T.astype(F64), "tanh"), "sigmoid": G.apply_act(W.T.astype(F64), "sigmoid")}
    stats, forms = {}, {}
    for K, s in ((64, 1), (128, 2)):
        x16 = np.zeros((64, K), F16)
        x16[np.arange(64), np.arange(64)] = 1
        W16 = np.ones((N, K), F16)
        W16[:, :64] = W
        x, w, b = operand(x16), operand(W16), operand(bias)
        got = {None: ops.skinny_linear(x, w, None, splits=s), "bias": ops.skinny_linear(x, w, b, splits=s), "relu_sq": ops.skinny_linear(x, w, None, act=1, splits=s)}
        assert all(ops.gemm_splits(N, K, Z, s) == s for Z in (1, 3, 4))      # the request is not cut back: s = 2 is the reduce-kernel form
        xb, wb = x.expand(4, 64, K), w.expand(4, N, K)
        yb = ops.skinny_bmm(xb, wb, None, act=4, splits=s)
        yb5 = ops.skinny_bmm(xb[:3], wb[:3], None, act=5, splits=s)           # act 4 + p: plane z is LoRA plane z + p
        outs = [torch.full((64, N), float("nan"), device="cuda", dtype=torch.float16) for _ in range(4)]
        ops.skinny_group([(x, w, o, None, a) for o, a in zip(outs, (None, "relu_sq", "tanh", "sigmoid"))], splits=s)
        got.update({("bmm", "tanh"): yb[1], ("bmm", "sigmoid"): yb[3], ("bmm", None): yb[0], ("bmm5", "tanh"): yb5[0], ("bmm5", None): yb5[1],
                    ("bmm5", "sigmoid"): yb5[2], ("group", None): outs[0],
                    ("group", "relu_sq"): outs[1], ("group", "tanh"): outs[2], ("group", "sigmoid"): outs[3]})
        forms[s] = {k: v.cpu().numpy() for k, v in got.items()}
        for k, v in forms[s].items():
            kind = k[1] if isinstance(k, tuple) else k
            res = G.report(v, *want[kind])
            stats[(s, k)] = res
            print(f"GEMMREF epilogue_every_half[s={s},{k}]: n={res['n']} bad={res['bad']} ambiguous={res['ambiguous']}" + (" " + res["msg"] if res["bad"] else ""))
    bad = {k: r["msg"] for k, r in stats.items() if r["bad"]}
    assert not bad, bad
    for k in forms[1]:
        assert np.array_equal(bits(forms[1][k]), bits(forms[2][k])), f"epilogue form and reduce-kernel form differ: {k}"


@pytest.mark.parametrize("name", list(G.SCALED_CASES))
def test_scaled_cases(name):
    """Subnormal inputs and outputs; overflow to +-inf."""
    from chirrup_amd import ops

    case, _ = G.scaled_named(name)
    x, w, b = operands(case)
    lo, _ = G.expected(case)
    M, N = lo.shape
    out = output((M, N))
    for s in (1, 4):
        out.poison()
        ops.skinny_linear(x, w, b, splits=s, out=out.view)
        G.assert_bits(out.get(), lo, lo, G.exact_pre(case), 2.0 ** (case["ex"] + case["ew"]), f"{name} s={s}")
    assert out.intact()
    note(f"scaled[{name}]", dict(n=2 * lo.size, bad=0), f" subnormal={float((np.abs(lo.astype(F64)) < 2.0 ** -14).mean()):.3f} inf={float(np.isinf(lo).mean()):.3f}")


@pytest.mark.parametrize("name,s", [("M33-N1000-K192", 1), ("M17-N132-K1024", 4), ("M200-N1000-K1024", 2)])
def test_non_finite_values_stay_in_their_row_and_column(name, s):
    """A NaN and an inf in one row of x change only that output row, a NaN in one row of W only that column; every other element keeps
    its exact bits."""
    from chirrup_amd import ops

    M, N, K, _, _ = G.F16_CASES[name]
    case = G.f16_named(name)
    x16, w16, b16 = G.halves(case)
    x16, w16 = x16.copy(), w16.copy()
    m0, n0 = M // 2, N - 3
    x16[m0, 5], x16[m0, K - 1], w16[n0, K // 2] = np.nan, np.inf, np.nan
    lo, _ = G.expected(case)
    lo = lo.copy()
    lo[m0, :], lo[:, n0] = np.nan, np.nan
    y = ops.skinny_linear(operand(x16), operand(w16), operand(b16), splits=s).cpu().numpy()
    res = G.assert_bits(y, lo, lo, name=f"non-finite {name}")
    note(f"non_finite[{name}]", res)
