"""Every launch form of rwkv7_add_ln_mix / rwkv7_add_ln_mix_mm8 (csrc/elementwise.hip) against the binary64 interval reference of
tests/tmix_ref.py (ln_form_reference / ln_form_check): rows grouped R to a workgroup, delta from split-K planes in batches of PL,
the mm8 correction of those planes (in_*), the mm8 prologue of the mixed planes (out_*), 8 to 1024 lanes inside the row, the forced
512- and 1024-lane instantiations, and the argument rejections.

Every case checks: x_new bit-exact (family "real" of the mm8 correction: inside its candidates, the rest staged on the kernel's own
x_new); every mixed plane and the carry rows inside their intervals, bit-equal where an interval holds one pattern; carry rows of
slots outside slot_idx untouched; xs exact and S inside its any-order bound, planes past out_planes untouched.  Outputs are
pre-filled with NaN or a canary.  tests/test_tmix_ref_cpu.py shows which defects this check rejects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F16, F32 = np.float16, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cu(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


GAP = 4096                  # elements of canary between two operands of an arena


class Arena:
    """Operands as slices of ONE buffer filled with a canary, with canary gaps between them (the layout of
    test_ln_kernel_lanes_past_the_row_touch_nothing): a lane that writes past its row or its plane lands in a gap."""

    def __init__(self, dtype, sizes):
        import tmix_ref as R
        import torch

        self.sizes = {k: (n + 7) // 8 * 8 for k, n in sizes.items() if n}
        self.buf = torch.full((sum(self.sizes.values()) + GAP * (len(self.sizes) + 1),), R.CANARY, dtype=dtype, device="cuda")
        self.views, pos = {}, GAP
        for k, n in self.sizes.items():
            self.views[k] = self.buf[pos:pos + sizes[k]]
            pos += n + GAP

    def get(self, k, fill=None, shape=None):
        v = self.views.get(k)
        if v is None:
            return None
        if fill is not None:
            v.copy_(cu(fill).view(-1)) if isinstance(fill, np.ndarray) else v.fill_(fill)
        return v if shape is None else v.view(*shape)

    def gaps_intact(self):
        import tmix_ref as R
        import torch

        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for v in self.views.values():
            off = v.data_ptr() - self.buf.data_ptr()
            mask[off // self.buf.element_size():off // self.buf.element_size() + v.numel()] = False
        return bool((self.buf[mask] == R.CANARY).all())


def launch(li):
    """One ops.add_ln_mix launch of the form li (tmix_ref.ln_form_inputs) selects; in place where the model runs it in place
    (T == 1).  Every output starts as NaN (xs and S: the canary) and every operand lies between canary gaps.  Returns the dict
    tmix_ref.ln_form_check takes."""
    import tmix_ref as R
    import torch
    from chirrup_amd import ops

    B, T, C = li["x"].shape
    n_mix, rows, nan = li["n_mix"], B * T, float("nan")
    has_delta = li["delta"] is not None or li["planes"] is not None
    P = 0 if li["out_ry"] is None else li["out_ry"].shape[0]
    n_slots = li["prev"].shape[0]
    a16 = Arena(torch.float16, dict(x=rows * C, delta=rows * C if li["delta"] is not None else 0, x_out=rows * C if has_delta and T > 1 else 0,
                                    prev_in=n_slots * C if n_mix else 0, prev_out=n_slots * C if n_mix and T > 1 else 0,
                                    out=max(n_mix, 1) * rows * C, xs=3 * rows * C if P else 0))
    a32 = Arena(torch.float32, dict(planes=0 if li["planes"] is None else li["planes"].size, S_in=0 if li["in_S"] is None else li["in_S"].size,
                                    S_out=3 * rows * 3 if P else 0))
    tx = a16.get("x", li["x"], (B, T, C))
    x_out = None if not has_delta else (tx if T == 1 else a16.get("x_out", nan, (B, T, C)))
    out = a16.get("out", nan, (max(n_mix, 1), B, T, C))
    prev_in = prev_out = mix = slot = None
    if n_mix:
        prev_in, mix, slot = a16.get("prev_in", li["prev"], (n_slots, C)), cu(li["mix"]), cu(li["slot_idx"])
        prev_out = prev_in if T == 1 else a16.get("prev_out", li["prev"], (n_slots, C))
    dp = a32.get("planes", li["planes"], (-1, rows, C)) if li["planes"] is not None else None
    mm8_in = None if li["in_S"] is None else (cu(li["in_rx"]), cu(li["in_mx"]), a32.get("S_in", li["in_S"], li["in_S"].shape))
    mm8_out = xs_all = S_all = None
    if P:
        xs_all, S_all = a16.get("xs", None, (3, rows * C)), a32.get("S_out", None, (3, rows, 3))
        mm8_out = (cu(li["out_ry"]), cu(li["out_my"]), xs_all[:P], S_all[0] if P == 1 else S_all[:P])
    ops.add_ln_mix(B, T, C, tx, a16.get("delta", li["delta"], (B, T, C)), x_out, cu(li["w"]), cu(li["b"]), 1e-5, prev_in, prev_out,
                   mix, out, slot_idx=slot, delta_partials=dp, mm8_in=mm8_in, mm8_out=mm8_out)
    torch.cuda.synchronize()
    assert a16.gaps_intact() and a32.gaps_intact(), "a lane wrote outside its operand"
    got = dict(out=out.cpu().numpy())
    if has_delta:
        got["x_new"] = x_out.cpu().numpy()
        if T > 1:
            assert np.array_equal(R.bits(tx.cpu().numpy()), R.bits(li["x"])), "x was written"
    if li["planes"] is not None:
        assert np.array_equal(dp.cpu().numpy().reshape(li["planes"].shape), li["planes"]), "the planes were written"
    if n_mix:
        got["carry"] = prev_out.cpu().numpy()
    if P:
        got.update(xs=xs_all.view(3, B, T, C).cpu().numpy(), S=S_all.cpu().numpy())
    return got


def run_case(case, li, record=True):
    import tmix_ref as R

    got = launch(li)
    res = R.ln_form_check(li, got)
    print(f"LN form {case}: {res['single']} of {res['n']} single-pattern, {res['bad']} outside, multi-candidate x_new {res['multi']:.5f}")
    if record:
        from test_fused_gpu import _record_ref

        fields = dict(n=res["n"], single=res["single"], outside=res["bad"])
        if li["family"] == "real":
            fields["x_new_multi_share"] = res["multi"]
        _record_ref(f"ln_form|{case}", **fields)
    assert res["bad"] == 0 and not res["fails"], f"{case}: " + "; ".join(res["fails"])
    assert res["multi"] <= 0.05 and (li["family"] == "real" or res["multi"] == 0.0)
    return got, res


def _seed(*a):
    return sum((i + 1) * 131 * int(v) for i, v in enumerate(a)) % 100003


# ---------------------------------------------------------------------------------------------------------------------
# rows grouped R to a workgroup (binary16 delta).  The R each shape reaches:
#   (5, 7)     T < 8: R = 1, one row per workgroup, every row with t > 0 recomputes its predecessor
#   (1, 8)     R = 2, four even groups
#   (2, 9)     R = 2, ragged: the last group of a sequence has one row
#   (3, 701)   R = 5, the last group has one row
#   (2, 1803)  R = 8 (the cap), the last group has three rows
# C = 64: 8 of 256 lanes inside the row; 2048: all 256; 2112: 264 of 1024; 8192: all 1024.
GROUPED = [(64, 5, 7), (64, 1, 8), (64, 2, 9), (64, 3, 701), (64, 2, 1803), (2048, 2, 9), (2112, 2, 9), (8192, 1, 8)]
GROUPED_CASES = [(C, B, T, n) for C, B, T in GROUPED for n in (6, 1)] + [(64, 2, 9, 0), (2048, 2, 9, 0), (2112, 2, 9, 0), (8192, 1, 8, 0)]


@pytest.mark.parametrize("C,B,T,n_mix", GROUPED_CASES)
def test_row_groups(C, B, T, n_mix):
    import tmix_ref as R

    li = R.ln_form_inputs(B, T, C, n_mix=n_mix, seed=_seed(C, B, T, n_mix))
    run_case(f"grouped|C{C}-B{B}-T{T}-n{n_mix}", li)


@pytest.mark.parametrize("C,B,T", [(64, 2, 9), (2048, 2, 9), (2112, 2, 9), (8192, 1, 8)])
def test_same_bits_however_rows_are_grouped(C, B, T):
    """The prefill launch (rows grouped, predecessor recomputed or carried in registers) and T decode launches of the same rows with
    the carry table threaded through give the same bits: each row's arithmetic is the same code at the same lane count."""
    import tmix_ref as R

    li = R.ln_form_inputs(B, T, C, n_mix=6, seed=_seed(C, B, T, 6))
    got = launch(li)
    prev = li["prev"]
    for t in range(T):
        step = dict(li, x=li["x"][:, t:t + 1], delta=li["delta"][:, t:t + 1], prev=prev)
        g1 = launch(step)
        assert np.array_equal(R.bits(g1["out"][:, :, 0]), R.bits(got["out"][:, :, t])), f"row {t}"
        assert np.array_equal(R.bits(g1["x_new"][:, 0]), R.bits(got["x_new"][:, t])), f"row {t}"
        prev = g1["carry"]
    assert np.array_equal(R.bits(prev), R.bits(got["carry"]))


# ---------------------------------------------------------------------------------------------------------------------
# delta from split-K planes: PL = 8 planes per batch with 256 lanes (C = 192), PL = 4 with 1024 lanes (C = 2112); one plane, one
# short of a batch, a full batch, one past it, several batches.  Decode (in place) and prefill (R = 2, ragged).
PLANES = [(192, s) for s in (1, 7, 8, 9, 16, 17)] + [(2112, s) for s in (1, 3, 4, 5, 8, 12)]
PLANES_CASES = [(C, s, B, T, (6, 1, 0)[(i + j) % 3]) for i, (C, s) in enumerate(PLANES) for j, (B, T) in enumerate([(5, 1), (2, 9)])]
PLANES_CASES += [(192, 9, 3, 4, 6), (2112, 5, 3, 4, 1)]         # R = 1 with T > 1: every row recomputes its predecessor from the planes


@pytest.mark.parametrize("C,splits,B,T,n_mix", PLANES_CASES)
def test_delta_from_partial_planes(C, splits, B, T, n_mix):
    import tmix_ref as R

    li = R.ln_form_inputs(B, T, C, n_mix=n_mix, splits=splits, seed=_seed(C, splits, B, T))
    run_case(f"planes|C{C}-B{B}-T{T}-n{n_mix}-splits{splits}", li)


# ---------------------------------------------------------------------------------------------------------------------
# mm8 in_*: the correction rx (core - 1023.5 S0) + S1 + mx S2 with the row sums added up from in_S_parts parts (lane-strided by 64:
# 1, 3, 64, 65, 130 parts = below, at and past one and two trips).  n_mix 0 and 1 as in the model (LN1 of the next layer / ln_out
# after ffn.value, and LN2 after att.output).  9 planes at C = 192 and 5 at C = 2112: more than one batch in both.
MM8_IN_CASES = [(fam, C, parts, 5, 1, (i + k) % 2) for fam in ("grid", "real") for k, C in enumerate((192, 2112))
                for i, parts in enumerate((1, 3, 64, 65, 130))] + \
               [(fam, C, 65, 2, 9, n) for fam in ("grid", "real") for C, n in ((192, 1), (2112, 0))]


@pytest.mark.parametrize("family,C,parts,B,T,n_mix", MM8_IN_CASES)
def test_mm8_in_correction(family, C, parts, B, T, n_mix):
    import tmix_ref as R

    li = R.ln_form_inputs(B, T, C, n_mix=n_mix, splits=9 if C == 192 else 5, mm8_in=family, parts=parts, seed=_seed(C, parts, B, T, n_mix))
    run_case(f"mm8_in|{family}|C{C}-B{B}-T{T}-n{n_mix}-parts{parts}", li)


# ---------------------------------------------------------------------------------------------------------------------
# mm8 out_*: the prologues of the first out_planes mixed planes, ry / my distinct per plane
MM8_OUT_CASES = [(C, B, T, n, P) for C in (192, 2112) for B, T in ((5, 1), (2, 9)) for n, P in ((1, 1), (6, 1), (6, 2), (6, 3))]


@pytest.mark.parametrize("C,B,T,n_mix,planes", MM8_OUT_CASES)
def test_mm8_out_prologue(C, B, T, n_mix, planes):
    import tmix_ref as R

    li = R.ln_form_inputs(B, T, C, n_mix=n_mix, out_planes=planes, seed=_seed(C, B, T, n_mix, planes))
    run_case(f"mm8_out|C{C}-B{B}-T{T}-n{n_mix}-planes{planes}", li)


def test_mm8_in_and_out_together():
    import tmix_ref as R

    li = R.ln_form_inputs(2, 9, 2112, n_mix=6, splits=5, mm8_in="real", parts=65, out_planes=3, seed=77)
    run_case("mm8_in_out|real|C2112-B2-T9-n6-parts65-planes3", li)


# ---------------------------------------------------------------------------------------------------------------------
# the forced lane counts: CHIRRUP_LN_THREADS is read once per process, so each value gets one fresh child

def child_cases(C):
    import tmix_ref as R

    return {f"delta|C{C}": R.ln_form_inputs(2, 9, C, n_mix=6, seed=_seed(C, 1)),                                     # R = 2
            f"planes9|C{C}": R.ln_form_inputs(2, 9, C, n_mix=1, splits=9, seed=_seed(C, 2)),
            f"mm8_in_out|C{C}": R.ln_form_inputs(2, 9, C, n_mix=6, splits=5, mm8_in="real", parts=65, out_planes=3, seed=_seed(C, 3))}


def child_main(widths):
    import tmix_ref as R

    results = {}
    for C in widths:
        for name, li in child_cases(C).items():
            res = R.ln_form_check(li, launch(li))
            results[name] = {k: res[k] for k in ("n", "single", "bad", "multi", "fails")}
    print("LN_FORMS_CHILD " + json.dumps(results, sort_keys=True))


@pytest.mark.parametrize("threads,widths", [(512, (64, 4096)), (1024, (64,))])
def test_forced_lane_counts(threads, widths):
    env = dict(os.environ, CHIRRUP_LN_THREADS=str(threads))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(c) for c in widths], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("LN_FORMS_CHILD ")]
    assert len(line) == 1, r.stdout[-2000:]
    results = json.loads(line[0].split(" ", 1)[1])
    assert len(results) == 3 * len(widths)
    from test_fused_gpu import _record_ref

    for name, res in sorted(results.items()):
        print(f"LN form TH{threads} {name}: {res['single']} of {res['n']} single-pattern, {res['bad']} outside")
        _record_ref(f"ln_form|lanes{threads}|{name}", n=res["n"], single=res["single"], outside=res["bad"],
                    **({"x_new_multi_share": res["multi"]} if name.startswith("mm8") else {}))
        assert res["n"] > 0 and res["bad"] == 0 and not res["fails"], f"{name}: {res['fails']}"
        assert res["multi"] <= 0.05


# ---------------------------------------------------------------------------------------------------------------------
# argument rejections: all return before any launch

def test_rejections_return_the_documented_code_and_touch_nothing():
    import ctypes

    import torch
    from chirrup_amd import lib, ops

    L = lib.load()
    E = {v: k for k, v in lib.E_NAMES.items()}
    B, T, CMAX = 2, 3, 8256
    # every buffer is large enough for every shape named below
    h16 = lambda n, v: torch.full((n,), v, dtype=torch.float16, device="cuda")
    x, delta, x_out, prev_in, prev_out = h16(B * T * CMAX + 8, 1.0), h16(B * T * CMAX, 0.5), h16(B * T * CMAX, 7.0), h16(B * CMAX, 1.0), h16(B * CMAX, 7.0)
    w, b, mix, out = h16(CMAX, 1.0), h16(CMAX, 0.0), h16(6 * CMAX, 0.5), h16(6 * B * T * CMAX, 7.0)
    planes = torch.zeros(2 * B * T * CMAX, dtype=torch.float32, device="cuda")
    ry, my, xs = h16(3 * CMAX, 1.0), h16(3 * CMAX, 0.0), h16(3 * B * T * CMAX, 7.0)
    S_in = torch.zeros(B * T * 3, dtype=torch.float32, device="cuda")
    S_out = torch.full((3 * B * T * 3,), 7.0, dtype=torch.float32, device="cuda")
    base = dict(B=B, T=T, C=64, n_mix=6, x=x.data_ptr(), delta=delta.data_ptr(), x_out=x_out.data_ptr(), prev_in=prev_in.data_ptr(),
                prev_out=prev_out.data_ptr(), mix=mix.data_ptr(), dpart=None, dsplits=0, fuse=None)

    def call(**kw):
        a = dict(base, **kw)
        fz = a["fuse"]
        st = None
        if fz is not None:
            st = ops._Mm8Fuse()
            for k, v in fz.items():
                setattr(st, k, v)
        return L.rwkv7_add_ln_mix_mm8(a["B"], a["T"], a["C"], a["n_mix"], a["x"], a["delta"], a["x_out"], w.data_ptr(), b.data_ptr(), 1e-5,
                                      a["prev_in"], a["prev_out"], a["mix"], out.data_ptr(), a["B"] * a["T"] * a["C"], None, a["dpart"],
                                      a["dsplits"], None if st is None else ctypes.addressof(st), ops._stream())
    out_fuse = dict(out_ry=ry.data_ptr(), out_my=my.data_ptr(), out_xs=xs.data_ptr(), out_S=S_out.data_ptr())
    cases = [
        ("T > 1 with prev_out == prev_in", dict(prev_out=prev_in.data_ptr()), "CHIRRUP_E_UNSUPPORTED"),
        ("T > 1, n_mix > 0, x_out == x with a delta", dict(x_out=x.data_ptr()), "CHIRRUP_E_UNSUPPORTED"),
        ("T > 1, n_mix > 0, x_out == x with partials", dict(x_out=x.data_ptr(), delta=None, dpart=planes.data_ptr(), dsplits=2), "CHIRRUP_E_UNSUPPORTED"),
        ("delta and delta_partials together", dict(dpart=planes.data_ptr(), dsplits=2), "CHIRRUP_E_UNSUPPORTED"),
        ("delta_splits == 0 with partials", dict(delta=None, dpart=planes.data_ptr(), dsplits=0), "CHIRRUP_E_UNSUPPORTED"),
        ("delta_splits < 0 with partials", dict(delta=None, dpart=planes.data_ptr(), dsplits=-1), "CHIRRUP_E_UNSUPPORTED"),
        ("n_mix = 3", dict(n_mix=3), "CHIRRUP_E_UNSUPPORTED"),
        ("C = 72", dict(C=72), "CHIRRUP_E_SHAPE"),
        ("C = 8256", dict(C=8256), "CHIRRUP_E_SHAPE"),
        ("out_xs with n_mix = 0", dict(n_mix=0, fuse=dict(out_fuse, out_planes=1)), "CHIRRUP_E_UNSUPPORTED"),
        ("out_planes = 2 with n_mix = 1", dict(n_mix=1, fuse=dict(out_fuse, out_planes=2)), "CHIRRUP_E_SHAPE"),
        ("in_S without partials", dict(fuse=dict(in_rx=ry.data_ptr(), in_mx=my.data_ptr(), in_S=S_in.data_ptr(), in_S_parts=1)), "CHIRRUP_E_NULL"),
        ("x 8 bytes off alignment", dict(x=x.data_ptr() + 8), "CHIRRUP_E_ALIGN"),
    ]
    for what, kw, code in cases:
        rc = call(**kw)
        assert rc == E[code], f"{what}: returned {lib.E_NAMES.get(rc, rc)}, documented {code}"
    torch.cuda.synchronize()
    for name, t in (("x_out", x_out), ("prev_out", prev_out), ("out", out), ("xs", xs), ("S", S_out)):
        assert bool((t == 7.0).all()), f"{name} was written by a rejected call"
    assert bool((prev_in == 1.0).all()) and bool((x == 1.0).all())
    # ... and through the wrapper, which turns the code into an exception that names it
    with pytest.raises(lib.ChirrupAmdError, match="UNSUPPORTED"):
        v = lambda t, *s: t[:int(np.prod(s))].view(*s)
        ops.add_ln_mix(B, T, 64, v(x, B, T, 64), v(delta, B, T, 64), v(x_out, B, T, 64), w[:64], b[:64], 1e-5, v(prev_in, B, 64), v(prev_in, B, 64),
                       v(mix, 6, 64), v(out, 6, B, T, 64))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((x_out == 7.0).all())


if __name__ == "__main__":
    for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert sys.argv[1] == "--child"
    child_main([int(c) for c in sys.argv[2:]])
