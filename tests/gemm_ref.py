"""Exact binary64 reference of the skinny GEMM entry points (csrc/skinny_gemm.hip: binary16 and uint8 / mm8 weights, every
epilogue, split-K partial planes, the LoRA chain of the time-mix launch).  TEST INFRASTRUCTURE ONLY, CPU only.

The exact-sum lemma (tmix_ref.py): a binary32 sum, in any order, of multiples of q is EXACT while sum|terms| < 2^24 q.  The
operands here lie on a coarse dyadic grid (x = i 2^-3, w = j 2^-9, bias = b 2^-6 with |i|, |j| <= 31, |b| <= 255), so every
product is a multiple of 2^-12, exact in binary32 (at most 10 significant bits), and every MFMA chain, K split, partial plane,
in-launch reduction and bias addition is exact in binary32 whatever its order.  There is then exactly ONE admissible binary16
pattern per output, h(exact value): nothing is assumed about the matrix core's summation order or internal rounding.
prove_exact() asserts the lemma's condition per case -- a condition of the test, not a measurement of a kernel.

What stays an interval, and why:
  tanh / sigmoid planes   h(tanhf(h(v))) / h(1 / (1 + expf(-h(v)))): v and h(v) are exact, the transcendental is not; the pair
                          act_table(kind)[bits(h(v))] of tmix_ref.py (4 binary32 ulps) -- one pattern where lo == hi.
  up-projections of them  their inputs are arbitrary halves, so the lemma does not apply: [h(e - d), h(e + d)] around the binary64
                          product e of the kernel's OWN hidden plane (checked against the table first),
                          d = gamma_(rank+2) sum|h w| + 2^-46 slack.

mm8 (uint8 weights, the split form y = rx (sum xs (1024 + q) - 1023.5 S0) + S1 + mx S2): x integers in +-4, ry in 2^-3..2^-5,
rx in 2^-5..2^-7, mx / my integers in +-8 times 2^-7.  xs = h(x ry) is exact, the core is a sum of multiples of 2^-5, every step
of the epilogue is exact in binary32 and the result equals the as-coded sum x ((q + 0.5) rx ry + mx + my) in binary64.
"""
import numpy as np

from tmix_ref import SLACK, U, act_table, bits, from_key, gamma, h, key

F16, F32, F64 = np.float16, np.float32, np.float64
KB = 64                  # the kernels' K-block
TILE_M, TILE_N = 16, 128


# ---------------------------------------------------------------------------------------------------------------------
# operand recipes

def _grid(rng, shape, sigma, clip):
    return np.clip(np.rint(rng.normal(0.0, sigma, shape)), -clip, clip) + 0.0          # (+ 0.0: no negative zeros)


def f16_case(M, N, K, seed=0, bias=True, ex=-3, ew=-9, eb=-6):
    """x [M,K] = i 2^ex, w [N,K] = j 2^ew, bias [N] = b 2^eb as integer arrays (binary64) with their exponents."""
    rng = np.random.default_rng(seed)
    return dict(xi=_grid(rng, (M, K), 8.0, 31), wi=_grid(rng, (N, K), 8.0, 31),
                bi=rng.integers(-255, 256, N).astype(F64) if bias else None, ex=ex, ew=ew, eb=eb)


def scaled(case, sx, sw=0, sb=0):
    """The case with x, w, bias multiplied by 2^sx, 2^sw, 2^sb: the lemma is scale-free.  Puts outputs into the binary16 subnormal
    range (x made of subnormal halves) or past 65504."""
    c = dict(case)
    c["ex"], c["ew"], c["eb"] = case["ex"] + sx, case["ew"] + sw, case["eb"] + sb
    return c


def halves(case):
    """(x, w, bias) as binary16 arrays."""
    x, w = case["xi"] * 2.0 ** case["ex"], case["wi"] * 2.0 ** case["ew"]
    b = None if case["bi"] is None else case["bi"] * 2.0 ** case["eb"]
    out = []
    for name, v in (("x", x), ("w", w), ("bias", b)):
        if v is None:
            out.append(None)
            continue
        v16 = h(v)
        assert np.array_equal(v16.astype(F64), v), f"{name} is not made of binary16 numbers"
        out.append(v16)
    return out


def exact_sum(case, k0=0, k1=None):
    """The exact value (binary64) of sum_{k0 <= k < k1} x[m,k] w[n,k]: integer arithmetic below 2^53."""
    k1 = case["xi"].shape[1] if k1 is None else k1
    s = case["xi"][:, k0:k1] @ case["wi"][:, k0:k1].T
    assert np.abs(s).max(initial=0.0) < 2.0 ** 53
    return s * 2.0 ** (case["ex"] + case["ew"])


def exact_pre(case, k=None):
    v = exact_sum(case, 0, k)
    return v if case["bi"] is None else v + case["bi"] * 2.0 ** case["eb"]


def prove_exact(case, splits=(1,), k=None):
    """Assert the lemma's condition for every binary32 quantity the kernels form from this case: each partial plane of each
    split count in `splits`, the full sum, sum + bias.  Returns (margin = max sum|terms| / (2^24 q), share of outputs that are not
    binary16 numbers before the final rounding)."""
    K = case["xi"].shape[1] if k is None else k
    halves(case)
    eq = case["ex"] + case["ew"]
    assert eq >= -126, "products below the binary32 normal range"
    xa, wa = np.abs(case["xi"][:, :K]), np.abs(case["wi"][:, :K])
    assert (xa * wa.max(initial=0.0)).max(initial=0.0) < 2.0 ** 24          # every product fits binary32
    for s in splits:
        assert K % (KB * s) == 0, (K, s)
        for i in range(s):
            a = xa[:, i * K // s:(i + 1) * K // s] @ wa[:, i * K // s:(i + 1) * K // s].T
            assert a.max(initial=0.0) < 2.0 ** 24, f"slice {i} of {s}: sum|terms| = {a.max()} q"
    a = xa @ wa.T                                                            # in units of q = 2^eq
    if case["bi"] is not None:
        e = min(eq, case["eb"])
        a = a * 2.0 ** (eq - e) + np.abs(case["bi"]) * 2.0 ** (case["eb"] - e)
        assert np.abs(case["bi"]).max() < 2.0 ** 24
    margin = float(a.max(initial=0.0)) / 2.0 ** 24
    assert margin < 1.0, f"sum|terms| = {margin} * 2^24 q"
    v = exact_pre(case, k)
    with np.errstate(over="ignore"):
        rounded = float((h(v).astype(F64) != v).mean())
    return margin, rounded


def apply_act(v, act):
    """(lo, hi) binary16 of the epilogue on the exact pre-activation value v.  act: None / 0, "relu_sq" / 1, "tanh", "sigmoid"."""
    v16 = h(v)
    if act in (None, 0):
        return v16, v16
    if act in ("relu_sq", 1):
        with np.errstate(over="ignore"):
            r = h(np.maximum(v16.astype(F64), 0.0) ** 2)                     # the square of a half is exact in binary32
        r[np.isnan(v16)] = np.nan
        return r, r
    lo, hi = act_table(act)
    return lo[bits(v16)], hi[bits(v16)]


def expected(case, act=None, k=None):
    return apply_act(exact_pre(case, k), act)


def expected_planes(case, s):
    """[s, M, N] binary32: plane i is the exact sum over columns [i K / s, (i + 1) K / s)."""
    K = case["xi"].shape[1]
    p = np.stack([exact_sum(case, i * K // s, (i + 1) * K // s) for i in range(s)])
    p32 = p.astype(F32)
    assert np.array_equal(p32.astype(F64), p)
    return p32


def up_interval(hid16, w16, bias16, rank):
    """An up-projection whose input is a tanh / sigmoid plane: [h(e - d), h(e + d)], e the binary64 product of the given hidden
    plane, d = gamma_(rank+2) (sum|h w| + |bias|) + slack."""
    hd, w = hid16[:, :rank].astype(F64), w16[:, :rank].astype(F64)
    e, a = hd @ w.T, np.abs(hd) @ np.abs(w).T
    if bias16 is not None:
        e, a = e + bias16.astype(F64), a + np.abs(bias16.astype(F64))
    d = (gamma(rank + 2) + SLACK) * a
    return h(e - d), h(e + d)


# ---------------------------------------------------------------------------------------------------------------------
# mm8

def mm8_case(B, K, N, seed=0):
    """x [B,K] integers in +-4, q [N,K] uint8 (K-contiguous, the layout of mm8t_linear), rx / mx [N], ry / my [K], and the next
    product's ry2 (powers of two) / my2 [N]."""
    rng = np.random.default_rng(seed)
    p2 = lambda n, es: 2.0 ** rng.choice(es, n)
    return dict(x=_grid(rng, (B, K), 1.5, 4), q=rng.integers(0, 256, (N, K)).astype(np.uint8),
                ry=p2(K, [-3, -4, -5]), rx=p2(N, [-5, -6, -7]), mx=rng.integers(-8, 9, N) * 2.0 ** -7, my=rng.integers(-8, 9, K) * 2.0 ** -7,
                ry2=p2(N, [-3, -4, -5]), my2=rng.integers(-8, 9, N) * 2.0 ** -7)


def mm8_halves(c):
    out = {}
    for name in ("x", "ry", "rx", "mx", "my", "ry2", "my2"):
        v16 = h(c[name])
        assert np.array_equal(v16.astype(F64), c[name]), name
        out[name] = v16
    out["q"] = c["q"]
    xs = c["x"] * c["ry"]
    out["xs"] = h(xs)
    assert np.array_equal(out["xs"].astype(F64), xs)
    S = np.stack([xs.sum(1), (c["x"] * c["my"]).sum(1), c["x"].sum(1)], 1)
    out["S"] = S.astype(F32)
    assert np.array_equal(out["S"].astype(F64), S)
    return out


def _fits(v, q, what):
    """v: multiples of q that a binary32 operation produces: representable while |v| < 2^24 q."""
    v = np.asarray(v, dtype=F64)
    assert np.array_equal(np.rint(v / q), v / q), f"{what}: not a multiple of 2^{int(np.log2(q))}"
    m = float(np.abs(v).max(initial=0.0)) / (2.0 ** 24 * q)
    assert m < 1.0, f"{what}: {m} * 2^24 q"
    return m


def mm8_core(c, k0=0, k1=None):
    k1 = c["x"].shape[1] if k1 is None else k1
    xs = (c["x"] * c["ry"])[:, k0:k1]
    return xs @ (1024.0 + c["q"][:, k0:k1].astype(F64)).T


def mm8_prove_exact(c, splits=(1,)):
    """Every binary32 quantity of the mm8 path: xs, the core (each partial plane, the full sum), S0 / S1 / S2 and each step of the
    epilogue.  Returns the core's margin sum|terms| / (2^24 2^-5)."""
    mm8_halves(c)
    K = c["x"].shape[1]
    xs = c["x"] * c["ry"]
    axs, aw = np.abs(xs), 1024.0 + c["q"].astype(F64)
    for s in splits:
        assert K % (KB * s) == 0
        for i in range(s):
            sl = slice(i * K // s, (i + 1) * K // s)
            _fits(axs[:, sl] @ aw[:, sl].T, 2.0 ** -5, f"core slice {i} of {s}")
    margin = _fits(axs @ aw.T, 2.0 ** -5, "core")
    _fits(axs.sum(1), 2.0 ** -5, "S0")
    _fits(np.abs(c["x"] * c["my"]).sum(1), 2.0 ** -7, "S1")
    _fits(np.abs(c["x"]).sum(1), 1.0, "S2")
    S0, S1, S2 = xs.sum(1)[:, None], (c["x"] * c["my"]).sum(1)[:, None], c["x"].sum(1)[:, None]
    core = mm8_core(c)
    _fits(1023.5 * S0, 2.0 ** -6, "1023.5 S0")
    _fits(np.abs(core) + np.abs(1023.5 * S0), 2.0 ** -6, "core - 1023.5 S0")
    t = c["rx"] * (core - 1023.5 * S0)
    _fits(c["mx"] * S2, 2.0 ** -7, "mx S2")
    _fits(np.abs(t) + np.abs(S1) + np.abs(c["mx"] * S2), 2.0 ** -13, "rx t + S1 + mx S2")      # in any association, fused or not
    y = t + S1 + c["mx"] * S2
    wd = (c["q"].astype(F64) + 0.5) * c["rx"][:, None] * c["ry"][None] + c["mx"][:, None] + c["my"][None]      # the as-coded weight [N, K]
    rows = max(1, (1 << 24) // wd.size)
    for m in range(0, y.shape[0], rows):                                         # row chunks: [rows, N, K] products at a time
        coded = (c["x"][m:m + rows, None, :] * wd[None]).sum(-1)
        assert np.array_equal(coded, y[m:m + rows]), "the split form differs from the as-coded expression"
    return margin


def mm8_expected(c, act=0):
    """(y, xs2) binary16: the product and the next product's prologue xs2 = h(y ry2)."""
    xs = c["x"] * c["ry"]
    S0, S1, S2 = xs.sum(1)[:, None], (c["x"] * c["my"]).sum(1)[:, None], c["x"].sum(1)[:, None]
    v = c["rx"] * (mm8_core(c) - 1023.5 * S0) + S1 + c["mx"] * S2
    y = apply_act(v, act)[0]
    return y, h(y.astype(F64) * c["ry2"])


def mm8_planes(c, s):
    K = c["x"].shape[1]
    p = np.stack([mm8_core(c, i * K // s, (i + 1) * K // s) for i in range(s)])
    p32 = p.astype(F32)
    assert np.array_equal(p32.astype(F64), p)
    return p32


# ---------------------------------------------------------------------------------------------------------------------
# guards

def embed(t, pad_rows=2, pad_cols=8, fill=np.nan):
    """(parent, index): parent[index] is a strided view holding t, surrounded by `fill` -- pad_rows rows above and below and
    pad_cols columns left and right of the last two dimensions (1-D: pad_cols either side).  Operands take NaN (a read past
    M, N or K poisons the result), outputs and partial buffers a sentinel (a write past them shows).  pad_cols a multiple of 8
    keeps 16-byte alignment."""
    t = np.asarray(t)
    if t.ndim == 1:
        shape, idx = (t.shape[0] + 2 * pad_cols,), (slice(pad_cols, pad_cols + t.shape[0]),)
    else:
        shape = t.shape[:-2] + (t.shape[-2] + 2 * pad_rows, t.shape[-1] + 2 * pad_cols)
        idx = (slice(None),) * (t.ndim - 2) + (slice(pad_rows, pad_rows + t.shape[-2]), slice(pad_cols, pad_cols + t.shape[-1]))
    parent = np.full(shape, fill, dtype=t.dtype)
    parent[idx] = t
    return parent, idx


def guards_intact(parent, idx, fill):
    """Every element of parent outside parent[idx] still holds the bit pattern of `fill`."""
    p = np.array(parent, copy=True)
    f = np.array(fill, dtype=p.dtype)
    p[idx] = f
    u = {2: np.uint16, 4: np.uint32, 1: np.uint8}[p.dtype.itemsize]
    return bool((p.view(u) == f.view(u)).all())


# ---------------------------------------------------------------------------------------------------------------------
# the check and its failure report

def report(got, lo, hi, exact=None, q=None):
    """Where an [M, N] result leaves its admissible patterns: the first bad (m, n), its 16-row x 128-column tile, the difference in
    units of q, the share of bad elements per tile (an indexing bug shows as a pattern)."""
    got, lo, hi = (np.asarray(a).reshape(-1, np.shape(got)[-1]) for a in (got, lo, hi))
    nan_w, nan_g = np.isnan(lo), np.isnan(got)
    z = lambda a: np.where(nan_w | nan_g, 0, a).astype(F16)
    ko, kl, kh = key(z(got)), key(z(lo)), key(z(hi))
    bad = (nan_w != nan_g) | (ko < kl) | (ko > kh)          # the rule of tmix_ref.check: NaN masks equal, lo <= got <= hi in half order
    res = dict(n=got.size, bad=int(bad.sum()), mask=bad, ambiguous=int(((bits(lo) != bits(hi)) & ~nan_w).sum()), msg="")
    if res["bad"]:
        M, N = got.shape
        m, n = (int(a[0]) for a in np.nonzero(bad))
        tm, tn = (M + TILE_M - 1) // TILE_M, (N + TILE_N - 1) // TILE_N
        cnt, tot = np.zeros((tm, tn)), np.zeros((tm, tn))
        mi, ni = np.arange(M)[:, None] // TILE_M + 0 * np.arange(N)[None], 0 * np.arange(M)[:, None] + np.arange(N)[None] // TILE_N
        np.add.at(cnt, (mi, ni), bad)
        np.add.at(tot, (mi, ni), 1)
        share = cnt / tot
        worst = sorted(((float(share[i, j]), i, j) for i, j in zip(*np.nonzero(cnt))), reverse=True)[:8]
        diff = ""
        if exact is not None and q:
            ex = np.asarray(exact).reshape(got.shape)
            with np.errstate(invalid="ignore", over="ignore"):
                diff = f", got - exact = {(float(got[m, n]) - float(ex[m, n])) / q:.3f} q (q = 2^{int(np.log2(q))})"
        res["msg"] = (f"{res['bad']} of {got.size} elements wrong; first ({m}, {n}) in tile (rows {m // TILE_M * TILE_M}.., cols "
                      f"{n // TILE_N * TILE_N}..): got {got[m, n]!r} (0x{int(bits(got)[m, n]):04x}) want [{lo[m, n]!r}, {hi[m, n]!r}]{diff}; "
                      f"{len(np.nonzero(cnt)[0])} of {tm * tn} tiles affected, worst shares (share, row tile, col tile): "
                      + ", ".join(f"({s:.2f}, {i}, {j})" for s, i, j in worst))
    return res


def assert_bits(got, lo, hi, exact=None, q=None, name="y"):
    res = report(got, lo, hi, exact, q)
    assert res["bad"] == 0, f"{name}: {res['msg']}"
    return res


def assert_planes(got32, want32, name="partials"):
    """Partial planes [s, M, N] binary32: bit equality."""
    got32, want32 = np.asarray(got32), np.asarray(want32)
    assert got32.shape == want32.shape, (got32.shape, want32.shape)
    bad = got32.view(np.uint32) != want32.view(np.uint32)
    if bad.any():
        i, m, n = (int(a[0]) for a in np.nonzero(bad))
        per = bad.reshape(bad.shape[0], -1).mean(1)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} wrong; first plane {i} ({m}, {n}) tile (rows {m // TILE_M * TILE_M}.., cols "
                             f"{n // TILE_N * TILE_N}..): got {got32[i, m, n]!r} want {want32[i, m, n]!r}; share per plane {np.round(per, 3).tolist()}")
    return int(bad.size)


# ---------------------------------------------------------------------------------------------------------------------
# binary32 evaluations on the CPU in a chosen order, with optional defects: what tests/test_gemm_ref_cpu.py holds the checker to

def rtz16(v):
    """binary64 -> binary16 rounded toward zero."""
    y = h(v)
    with np.errstate(invalid="ignore"):
        over = np.abs(y.astype(F64)) > np.abs(v)
    k = key(np.where(np.isnan(y), 0, y).astype(F16))
    stepped = from_key(np.where(k >= 0, k - 1, k + 1))
    return np.where(over, stepped, y).astype(F16)


F16_MUTANTS = ["block_dropped", "slice_boundary_off", "chunks_swapped", "half_boundary_off", "bias_after_rounding", "relu_sq_unrounded",
               "round_toward_zero", "f16_block_accumulation", "k_of_ignored"]
MM8_MUTANTS = ["offset_1024", "mx_my_exchanged", "bytes_23_for_01"]


def emulate_f16(case, act=None, order="blocks", s=1, mutant=None, k=None, seed=0):
    """y [M,N] binary16 from binary32 arithmetic.  order: "blocks" (64-column blocks added in order inside each of s slices, slices
    added in slice order), "permuted" (K permuted, one sum), "slices" (s column slices, any boundaries, added in slice order).
    k: the reduction length (k_of); columns beyond it hold NaN in x and w."""
    x16, w16, b16 = halves(case)
    M, K = x16.shape
    x, w = x16.astype(F32), w16.astype(F32)
    if k is not None:
        x, w = x.copy(), w.copy()
        x[:, k:], w[:, k:] = np.nan, np.nan
        if mutant != "k_of_ignored":
            x, w, K = x[:, :k], w[:, :k], k
    if mutant == "chunks_swapped":                       # two 16-byte chunks of every odd row of W, in the first K-block
        w = w.copy()
        w[1::2, 0:8], w[1::2, 8:16] = w[1::2, 8:16].copy(), w[1::2, 0:8].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if order == "permuted":
            p = np.random.default_rng(seed).permutation(K)
            acc = x[:, p] @ w[:, p].T
        elif order == "slices":
            cuts = np.linspace(0, K, s + 1).astype(int)
            acc = np.zeros((M, w.shape[0]), F32)
            for i in range(s):
                acc = acc + x[:, cuts[i]:cuts[i + 1]] @ w[:, cuts[i]:cuts[i + 1]].T
        else:
            nb = K // KB
            per = nb // s
            acc = np.zeros((M, w.shape[0]), F32)
            for i in range(s):
                blocks = list(range(i * per, (i + 1) * per))
                if mutant == "block_dropped" and i == s - 1:
                    blocks = blocks[:-1]
                if mutant == "slice_boundary_off" and i == 0 and s > 1:
                    blocks = blocks + [per]                  # slice 0 runs one block into slice 1
                part = np.zeros_like(acc)
                for b in blocks:
                    xb, wb = x[:, b * KB:(b + 1) * KB], w[:, b * KB:(b + 1) * KB]
                    if mutant == "f16_block_accumulation":
                        a16 = np.zeros(acc.shape, F16)
                        for j in range(KB):
                            a16 = h(a16.astype(F32) + xb[:, j:j + 1] * wb[:, j][None])
                        part = part + a16.astype(F32)
                    else:
                        part = part + xb @ wb.T
                acc = acc + part
        v = acc
        if b16 is not None and mutant != "bias_after_rounding":
            v = v + b16.astype(F32)
        if mutant == "bias_after_rounding" and b16 is not None:
            v = h(v).astype(F32) + b16.astype(F32)
        if act in ("relu_sq", 1):
            r = v if mutant == "relu_sq_unrounded" else h(v).astype(F32)
            v = np.where(r > 0, r * r, F32(0))
        y = rtz16(v.astype(F64)) if mutant == "round_toward_zero" else h(v)
    if mutant == "half_boundary_off" and M > 32:             # the lower half starts 16 rows late: those rows are never written
        half = (M + 31) // 32 * 16
        y = y.copy()
        y[half:half + 16] = 0
    return y


def emulate_mm8(c, act=0, order="blocks", s=1, mutant=None, seed=0):
    """(y, xs2) binary16 from binary32 arithmetic of the mm8 split form."""
    hv = mm8_halves(c)
    f = lambda a: a.astype(F32)
    xs, q = f(hv["xs"]), hv["q"]
    if mutant == "bytes_23_for_01":
        q = q.copy()
        q[:, 0::4], q[:, 1::4] = q[:, 2::4].copy(), q[:, 3::4].copy()
    wq = F32(1024.0) + q.astype(F32)
    K = xs.shape[1]
    if order == "permuted":
        p = np.random.default_rng(seed).permutation(K)
        core = xs[:, p] @ wq[:, p].T
    else:
        cuts = np.linspace(0, K, s + 1).astype(int)
        core = np.zeros((xs.shape[0], wq.shape[0]), F32)
        for i in range(s):
            core = core + xs[:, cuts[i]:cuts[i + 1]] @ wq[:, cuts[i]:cuts[i + 1]].T
    S = hv["S"]
    S0, S1, S2 = S[:, 0:1], S[:, 1:2], S[:, 2:3]
    if mutant == "mx_my_exchanged":
        # mx [N] and my [K] act only through the rank-1 terms mx S2 (S2 = sum x) and S1 = sum x my; they differ in length, so "mx and
        # my exchanged" is emulated as each term taking the other's row sum: mx S1 + S2
        S1, S2 = S2, S1
    off = F32(1024.0 if mutant == "offset_1024" else 1023.5)
    v = f(hv["rx"]) * (core - off * S0) + S1 + f(hv["mx"]) * S2
    if act:
        r = f(h(v))
        v = np.where(r > 0, r * r, F32(0))
    y = h(v)
    return y, h(f(y) * f(hv["ry2"]))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gemm_exact_gpu.py, proved by tests/test_gemm_ref_cpu.py: id -> (M, N, K, bias, split counts whose planes
# are formed).  M: MT = ceil(M / 16) sets the ring depth, halves above 32 rows, the in-launch reduction at <= 32; N: last tile
# partial, 16-byte and 8-byte stores; K: one block, three blocks (a split of 2 is cut back to 1), 16 blocks (the ring wraps twice
# at every depth), 4096 (the library's own split); N = 32768 selects the wide kernel.

F16_CASES = {
    "M1-N4-K64": (1, 4, 64, True, (1,)),
    "M16-N128-K192": (16, 128, 192, True, (1, 3)),
    "M17-N132-K1024": (17, 132, 1024, True, (1, 2, 4, 8, 16)),
    "M32-N260-K1024": (32, 260, 1024, False, (1, 2, 4, 16)),
    "M33-N1000-K192": (33, 1000, 192, True, (1, 3)),
    "M112-N128-K1024": (112, 128, 1024, True, (1, 2, 4, 16)),
    "M113-N260-K64": (113, 260, 64, True, (1,)),
    "M200-N1000-K1024": (200, 1000, 1024, True, (1, 2, 4, 8, 16)),
    "M209-N132-K4096": (209, 132, 4096, False, (1, 2, 4, 16)),
    "M256-N260-K1024": (256, 260, 1024, True, (1, 2, 4, 16)),
    "M24-N1024-K4096": (24, 1024, 4096, True, (1, 2, 4, 16)),
    "wide-M17-N32768-K128": (17, 32768, 128, True, (1, 2)),
    "wide-M64-N32768-K1024": (64, 32768, 1024, False, (1, 2, 4)),
}


def case_seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


_F16 = {}


def f16_named(name):
    if name not in _F16:
        M, N, K, bias, _ = F16_CASES[name]
        _F16[name] = f16_case(M, N, K, case_seed(name), bias)
    return _F16[name]


# scaled cases: (base case, sx, sw, sb, bias override) -- subnormal x and outputs; part of the outputs past 65504.  "overflow": the sums
# themselves pass 65504 (q = 2^4, so nothing lies strictly between 65504 = 4094 q and 65520 = 4095 q).  "overflow-edge": q = 2^-6, sums
# of a few tens, and the bias +-65504 / +-65472 (2047 and 2046 times 2^5) puts sum + bias on both sides of the two thresholds: values in
# (65504, 65520) must round to 65504, values from 65520 on to inf, both asserted to occur by tests/test_gemm_ref_cpu.py.
EDGE_BIAS = (2047.0, -2047.0, 2046.0, -2046.0)
SCALED_CASES = {
    "subnormal": ("M33-N1000-K192", -21, 4, -18, None),
    "subnormal-K1024": ("M17-N132-K1024", -21, 4, -18, None),
    "overflow": ("M17-N132-K1024", 12, 4, 10, None),
    "overflow-M200": ("M200-N1000-K1024", 12, 4, 10, None),
    "overflow-edge": ("M17-N132-K1024", 3, 3, 11, EDGE_BIAS),
    "overflow-edge-M200": ("M200-N1000-K1024", 3, 3, 11, EDGE_BIAS),
}


def scaled_named(name):
    base, sx, sw, sb, edge = SCALED_CASES[name]
    c = scaled(f16_named(base), sx, sw, sb)
    if edge is not None:
        c["bi"] = np.resize(np.array(edge), c["wi"].shape[0])
    return c, F16_CASES[base][4]


def bmm_case(Z, M, N, K, seed, bias=True):
    """Z problems [M,K] x [N,K] of a batched launch."""
    return [f16_case(M, N, K, seed + 17 * z, bias) for z in range(Z)]


# skinny_bmm with per-problem reduction lengths (the LoRA up-projection launch): M -> (N, K, k_of)
BMM_KOF = {17: (256, 192, (64, 128, 64, 192)), 33: (260, 192, (64, 128, 64, 192)), 200: (256, 192, (64, 128, 64, 192))}
# skinny_bmm act 4 / 5 (tanh on plane w, sigmoid on plane g): (M, act, splits asked for); Z = 8 - act problems of N = 132, K = 1024
BMM_PLANES = [(17, 4, 1), (200, 4, 2), (33, 5, 1), (113, 5, 4), (32, 4, 0)]
BMM_PLANES_NK = (132, 1024)


def bmm_kof_named(M):
    N, K, ks = BMM_KOF[M]
    return bmm_case(len(ks), M, N, K, 100 + M), ks


def bmm_planes_named(M, act):
    return bmm_case(8 - act, M, *BMM_PLANES_NK, 200 + M, bias=False)


# the layer launch: R/K/V plus four LoRA down-projections of these ranks, tanh on plane w and sigmoid on plane g
RANKS = [64, 128, 64, 192]
ACTS = [None, "tanh", None, "sigmoid"]
GROUP_LAYERS = {M: (M, 384, 1024, 300 + M) for M in (17, 32, 33, 113, 200)}           # skinny_group: (M, C, K, seed)
TMIX_LAYERS = {M: (M, 1024, 1024, 400 + M) for M in (1, 17, 64, 200)}                 # tmix_gemms
_LAYER = {}


def layer_problem(M, C, K, seed):
    """The operands of a layer's seven-problem launch: main (three R/K/V cases), mixed (six [M,K] integer planes, x = mixed 2^-3), down
    (four LoRA down-projection cases of RANKS[j] rows, fed by mixed[2 + j]), LoRA up weights [C, RANKS[j]] and biases [C] as values."""
    if (M, C, K, seed) not in _LAYER:
        main = [f16_case(M, C, K, seed + j, bias=False) for j in range(3)]
        rng = np.random.default_rng(seed + 50)
        mixed = [c["xi"] for c in main] + [_grid(rng, (M, K), 8.0, 31) for _ in range(3)]
        down = [dict(xi=mixed[2 + j], wi=_grid(rng, (RANKS[j], K), 8.0, 31), bi=None, ex=-3, ew=-9, eb=-6) for j in range(4)]
        up_w = [_grid(rng, (C, RANKS[j]), 8.0, 31) * 2.0 ** -9 for j in range(4)]
        up_b = [rng.integers(-63, 64, C) * 2.0 ** -6 for j in range(4)]      # (|bias| < 1: the up-projections' products are multiples of 2^-21)
        _LAYER[(M, C, K, seed)] = (main, mixed, down, up_w, up_b)
    return _LAYER[(M, C, K, seed)]


def dyadic_case(x16, w16, b16):
    """A case dict from binary16 arrays: the coarsest power-of-two grids they lie on."""
    def grid(a):
        a = np.asarray(a, F64)
        for e in range(8, -25, -1):
            if np.array_equal(np.rint(a / 2.0 ** e), a / 2.0 ** e):
                return e
        raise AssertionError("not binary16")
    ex, ew = grid(x16), grid(w16)
    c = dict(xi=x16.astype(F64) / 2.0 ** ex, wi=w16.astype(F64) / 2.0 ** ew, bi=None, ex=ex, ew=ew, eb=0)
    if b16 is not None:
        c["eb"] = grid(b16)
        c["bi"] = b16.astype(F64) / 2.0 ** c["eb"]
    return c


def layer_up_case(layer, j):
    """The up-projection of plane j (v or a: no activation), fed by the exact hidden plane h(down-projection)."""
    _, _, down, up_w, up_b = layer
    assert ACTS[j] is None
    return dyadic_case(expected(down[j])[0], h(up_w[j]), h(up_b[j]))


def layer_prove_exact(layer, splits=(1, 2, 4)):
    """prove_exact for every exact problem of a layer launch: R/K/V, the four down-projections, the v and a up-projections."""
    main, _, down, _, _ = layer
    return [prove_exact(c, splits) for c in main + down] + [prove_exact(layer_up_case(layer, j), (1,)) for j in range(4) if ACTS[j] is None]


def tmix_mm8_cases(M):
    """The uint8 R/K/V problems of the time-mix launch with mm8=True."""
    _, C, K, _ = TMIX_LAYERS[M]
    return [mm8_named_case(M, K, C, 500 + M + j) for j in range(3)]


MM8_CASES = {
    "B1-K256-N384": (1, 256, 384, (1, 2, 4)),
    "B17-K1024-N1024": (17, 1024, 1024, (1, 2, 4, 16)),
    "B33-K256-N1000": (33, 256, 1000, (1, 2, 4)),
    "B64-K2048-N256": (64, 2048, 256, (1, 2, 4)),
    "B200-K512-N1024": (200, 512, 1024, (1, 2, 4)),
    "B256-K64-N136": (256, 64, 136, (1,)),
    "B257-K256-N128": (257, 256, 128, (1, 2)),
    "B600-K128-N256": (600, 128, 256, (1, 2)),
}

_MM8 = {}


def mm8_named_case(B, K, N, seed):
    if (B, K, N, seed) not in _MM8:
        _MM8[(B, K, N, seed)] = mm8_case(B, K, N, seed)
    return _MM8[(B, K, N, seed)]


def mm8_named(name):
    B, K, N, _ = MM8_CASES[name]
    return mm8_named_case(B, K, N, case_seed(name))
