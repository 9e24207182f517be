"""Float64 interval reference of the fused time-mix core (rwkv7_tmix_wkv7_fused, csrc/wkv7.hip MODE 1 / 2), of the
three-kernel path (tmix_mid -> wkv7 -> tmix_post) and of rwkv7_lora_act.  TEST INFRASTRUCTURE ONLY, CPU only.

"Exact where the reference is unambiguous, an interval where it is not".  Every operation of the chain is one correctly
rounded binary32 operation on binary16 values followed by one rounding to binary16 (numpy's half arithmetic does the
same; the WKV7 recurrence is oracle/oracle.c bit for bit) EXCEPT four: expf inside the sigmoids, the L2 norm of k*k_k
over a head, the group-norm moments of y over a head and the bonus sum over a head.  Those are evaluated in binary64
with a bound `delta` on what ANY binary32 evaluation of them can be off by; h(x - delta) and h(x + delta) (h = round to
binary16) either agree -- then the kernel must give that bit pattern -- or span a closed interval of halves.

Margins (u = 2^-24, gamma_n = n u / (1 - n u); nothing here is fitted to a kernel's output):

  sigmoid   s = 1 / (1 + expf(-x)): 4 binary32 ulps of s for the whole chain.  ASSUMPTION: no accuracy figure for the
            device expf / tanhf is documented in the ROCm tree this was written against; a device expf good to E ulps
            gives (2E + 2) u relative <= 2E + 2 ulps, so 4 ulps allows E = 1.  test_lora_act_exhaustive tests it on
            every binary16 input.  tanh: 4 binary32 ulps of tanhf, the same assumption.
  exact-sum lemma  a binary32 sum, in any order, of numbers that are all multiples of q is EXACT while sum|terms| < 2^24 q
            (every partial sum is a multiple of q below 2^24 q, hence representable).  q = the smallest binary16 ulp
            among a head's 64 terms (q^2 for squares of halves, whose products are exact in binary32).
  sum       of 64 terms: 0 by the lemma, else gamma_63 * sum|terms|.
  L2 norm   ss = sum (k k_k)^2 has relative error g in {0, gamma_63}; sqrtf is correctly rounded:
            sqrt(ss (1 + g))(1 + u) is within g/2 + 1.5 u relative of sqrt(ss) (0.5 u swallows the second-order terms).
  group norm  mean: E_m = sum error / 64.  d_i = fl(y_i - mean): e_i = E_m (1 + u) + u |y_i - m|; 0 when the mean is exact and
            the difference is a multiple of q/64 below 2^24 q/64.  var: |var - V| <= eV = (2 sum D_i e_i + sum e_i^2)/64 *
            (1 + gamma_64) + gamma_64 V  (D_i = |y_i - m|; squares rounded once, 63 additions).  rstd = 1/sqrtf(var + eps)
            (three roundings): relative rho = r / (2 (1 - r)) + 3 u, r = eV / (V + eps).  A group size n that is not a power
            of two (LayerNorm over C = 768) rounds sum / n once more: E_m (1 + u) + u |m|, no exact differences, 4 u in rho.  gn32 = fl(fl(fl(d rstd) w) + b):
            eP = |w| R (e_i (1 + rho') + D_i rho'), rho' = (1 + rho)(1 + u)^2 - 1;  eG = eP + u (|G| + eP).
  bonus     sum of 64 known halves h(h(r k') r_k): the sum bound above.
  out       h(h(gn + h(bonus v')) g) is monotone in gn and in bonus: the four corners bound it.
  mm8 sums  S0 = sum xs, S1 = sum o my, S2 = sum o over a head, of known halves (products of two halves are exact in
            binary32): gamma_64 * sum|terms|.
  binary64  the binary64 evaluation itself is given 2^-46 relative slack on every margin.

The INPUTS keep ambiguity out of the state: pre-sigmoid values are drawn only from the halves whose sigmoid is
unambiguous (an ambiguous one is replaced by its neighbouring half), a head whose norm is ambiguous gets its k redrawn.
Then k', v', -kk, kk*a are determined bit for bit, and so are the state and y.
"""
import numpy as np

from oracle import native

F16, F32, F64 = np.float16, np.float32, np.float64
U = 2.0 ** -24
SLACK = 2.0 ** -46
EPS = 64e-5
ACT_ULPS = 4.0          # binary32 ulps granted to 1/(1+expf(-x)) and to tanhf (assumption, see above)


def gamma(n):
    return n * U / (1 - n * U)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint16)


def key(x):
    """Total order on binary16 bit patterns of non-NaN values: ... < -0 < +0 < ...; consecutive halves differ by 1."""
    b = bits(x).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF) - 1, b)


def h(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(F16)


def ulp32(x):
    """The binary32 ulp at |x| (binary64 array)."""
    ax = np.abs(np.asarray(x, dtype=F64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    return np.where(ax > 0, 2.0 ** (np.maximum(e, -126.0) - 23.0), 2.0 ** -149)


def ulp16(x):
    """The binary16 ulp at |x| of a binary16 array (2^-24 in the subnormal range and at zero)."""
    ax = np.abs(np.asarray(x).astype(F64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    return np.where(ax > 0, 2.0 ** (np.maximum(e, -14.0) - 10.0), 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------------------
# sigmoid / tanh of every binary16 input

_TABLES = {}


def act_table(kind):
    """(lo, hi) binary16 arrays indexed by the input's bit pattern: the admissible results of h(sigmoid_f(x)) / h(tanhf(x)).
    lo == hi: unambiguous.  NaN inputs give NaN in both."""
    if kind not in _TABLES:
        x = np.arange(65536, dtype=np.uint16).view(F16).astype(F64)
        with np.errstate(over="ignore", invalid="ignore"):
            s = 1.0 / (1.0 + np.exp(-x)) if kind == "sigmoid" else np.tanh(x)
            d = ACT_ULPS * ulp32(s) + SLACK * np.abs(s)
            d = np.where((s == 0.0) | (np.abs(s) == 1.0) & (np.abs(x) > 40), 0.0, d)    # saturated: expf gives 0 / inf, exactly
            lo = h(np.maximum(s - d, 0.0) if kind == "sigmoid" else s - d)       # 1 / (1 + e) is never below +0
            hi = h(s + d)
        _TABLES[kind] = (lo, hi)
    return _TABLES[kind]


def act_ambiguous(kind):
    lo, hi = act_table(kind)
    return (bits(lo) != bits(hi)) & ~np.isnan(lo)


def guard_preact(x):
    """Replace every half whose sigmoid is ambiguous by the nearest half (in bit order) whose sigmoid is not.
    Returns (guarded copy, number replaced)."""
    amb = act_ambiguous("sigmoid")
    b = bits(x).copy()
    bad = amb[b]
    n = int(bad.sum())
    flat = b.reshape(-1)
    for i in np.flatnonzero(bad):
        for step in range(1, 64):
            cands = [c for c in (int(flat[i]) + step, int(flat[i]) - step) if (c & 0x7C00) != 0x7C00 and (c & 0x7FFF) and not amb[c]]
            if cands:
                flat[i] = cands[0]
                break
    return flat.view(F16).reshape(np.shape(x)), n


def sigmoid_exact(x):
    """(h(sigmoid(x)) of guarded inputs, number of inputs that are still ambiguous)."""
    lo, hi = act_table("sigmoid")
    b = bits(x)
    return lo[b], int((bits(lo[b]) != bits(hi[b])).sum())


# ---------------------------------------------------------------------------------------------------------------------
# sums of 64 known halves

def sum_err(abs_sum, q, n=64):
    """Bound on a binary32 sum of n multiples of q in any order: 0 by the exact-sum lemma, else gamma_(n-1) sum|terms|."""
    return np.where(abs_sum < 2.0 ** 24 * q, 0.0, gamma(n - 1) * abs_sum) + SLACK * abs_sum


def head_sum(t16):
    """t16 [..., 64] binary16 terms -> (binary64 sum, bound of a binary32 evaluation)."""
    t = t16.astype(F64)
    q = ulp16(t16).min(-1)
    return t.sum(-1), sum_err(np.abs(t).sum(-1), q)


def norm_interval(kk_in):
    """kk_in [..., 64] binary16 -> (lo, hi) halves of h(sqrtf(sum kk_in^2))."""
    t = kk_in.astype(F64) ** 2
    ss = t.sum(-1)
    q = ulp16(kk_in).min(-1) ** 2
    g = np.where(ss < 2.0 ** 24 * q, 0.0, gamma(63))
    rel = g / 2 + 1.5 * U + SLACK
    n = np.sqrt(ss)
    return h(n * (1 - rel)), h(n * (1 + rel))


def group_norm_interval(y, lw, lb, eps=EPS, group=64):
    """y [rows, C] binary16 (known exactly), groups of `group` channels -> (lo, hi, nearest) halves of the binary16 group norm."""
    rows, C = y.shape
    G = C // group
    yf = y.astype(F64).reshape(rows, G, group)
    w = lw.astype(F64).reshape(1, G, group)
    b = lb.astype(F64).reshape(1, G, group)
    eps = float(F32(eps))
    n = group
    q = ulp16(y).reshape(rows, G, group).min(-1, keepdims=True)
    asum = np.abs(yf).sum(-1, keepdims=True)
    m = yf.mean(-1, keepdims=True)
    pow2 = (n & (n - 1)) == 0                         # sum / n is exact for a power of two, one more rounding otherwise
    E_m = sum_err(asum, q, n) / n
    exact_sub = (E_m <= SLACK * asum) & (np.abs(yf - m) < 2.0 ** 24 * q / n) & pow2
    if not pow2:
        E_m = E_m * (1 + U) + U * np.abs(m)
    D = np.abs(yf - m)
    e = np.where(exact_sub, 0.0, E_m * (1 + U) + U * D) + SLACK * (D + np.abs(m))
    V = (D ** 2).mean(-1, keepdims=True)
    eV = (2 * (D * e).sum(-1, keepdims=True) + (e ** 2).sum(-1, keepdims=True)) / n * (1 + gamma(n)) + gamma(n) * V + SLACK * (V + eps)
    x = V + eps
    r = eV / x
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(r < 1, r / (2 * (1 - np.minimum(r, 0.999999))) + (3 if pow2 else 4) * U, np.inf)
    R = 1.0 / np.sqrt(x)
    rho1 = (1 + rho) * (1 + U) ** 2 - 1
    Gv = (yf - m) * R * w + b
    eP = np.abs(w) * R * (e * (1 + rho1) + D * rho1)
    eG = eP + U * (np.abs(Gv) + eP) + SLACK * (np.abs(Gv) + np.abs(b)) + 2.0 ** -140       # (+ binary32 underflow of the products)
    return h(Gv - eG).reshape(rows, C), h(Gv + eG).reshape(rows, C), h(Gv).reshape(rows, C)


def _minmax(cands):
    ks = np.stack([key(c) for c in cands])
    st = np.stack(cands)
    lo = np.take_along_axis(st, ks.argmin(0)[None], 0)[0]
    hi = np.take_along_axis(st, ks.argmax(0)[None], 0)[0]
    nan = np.isnan(st).any(0)
    lo, hi = lo.copy(), hi.copy()
    lo[nan] = np.nan
    hi[nan] = np.nan
    return lo, hi


def post_interval(y, r, k2, v2, g, r_k, lw, lb, H, eps=EPS):
    """Everything behind the recurrence (rwkv7.py:647-649) from known halves: y, r, k' (after the a gate), v' (after the v gate),
    g [rows, C].  Returns (lo, hi, mid, gn_lo, gn_hi, bonus_lo, bonus_hi); mid: the chain from the binary64 values rounded once."""
    rows, C = y.shape
    with np.errstate(over="ignore", invalid="ignore"):
        gn_lo, gn_hi, gn_mid = group_norm_interval(y, lw, lb, eps)
        t = ((r * k2) * r_k).reshape(rows, H, 64)
        s, e = head_sum(t)
        b_lo, b_hi = h(s - e)[..., None], h(s + e)[..., None]
        v3, g3 = v2.reshape(rows, H, 64), g.reshape(rows, H, 64)
        tail = lambda gn, bo: ((gn.reshape(rows, H, 64) + bo * v3) * g3).reshape(rows, C)
        cands = [tail(gn, bo) for gn in (gn_lo, gn_hi) for bo in (b_lo, b_hi)]
        mid = tail(gn_mid, h(s)[..., None])
    lo, hi = _minmax(cands)
    return lo, hi, mid, gn_lo, gn_hi, b_lo[..., 0], b_hi[..., 0]


# ---------------------------------------------------------------------------------------------------------------------
# the reference

def gating(inp):
    """rwkv7.py:629-637 from guarded inputs: k', v', -kk, kk*a as exact halves, and how many sigmoid inputs / head norms
    are still ambiguous (the generator brings both to zero)."""
    k, v = inp["k"], inp["v"]
    B, T, C = k.shape
    H = C // 64
    a, amb_a = sigmoid_exact(inp["a_pre"])
    kk_in = (k * inp["k_k"]).reshape(B, T, H, 64)
    n_lo, n_hi = norm_interval(kk_in)
    amb_n = int((bits(n_lo) != bits(n_hi)).sum())
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        kk = (kk_in / n_lo[..., None]).reshape(B, T, C)        # 0/0 = NaN for a head with k = 0 (clamp_min(1e-12) is 0 in binary16)
        k2 = k * (F16(1.0) + (a - F16(1.0)) * inp["k_a"])
        kka = kk * a
        amb_g = 0
        if inp["layer0"]:
            v2 = v
        else:
            gate, amb_g = sigmoid_exact(inp["vg_pre"])
            v2 = v + (inp["v_first"] - v) * gate
    return dict(k2=k2, v2=v2, neg_kk=-kk, kka=kka, amb_gate=amb_a + amb_g, amb_norm=amb_n)


def mid_interval(k, v, a_pre, vg_pre, v_first, k_k, k_a, layer0):
    """rwkv7.py:629-637 for ANY inputs [rows, C] (not guarded): (lo, hi) halves of k', -kk, kk*a, v'.  Each is monotone in the
    sigmoid's half and in the norm's half, so the corners of those two intervals bound it; lo == hi wherever both are unambiguous."""
    rows, C = k.shape
    H = C // 64
    s_lo, s_hi = act_table("sigmoid")
    a_c = [s_lo[bits(a_pre)], s_hi[bits(a_pre)]]
    kk_in = (k * k_k).reshape(rows, H, 64)
    n_c = norm_interval(kk_in)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k2 = _minmax([k * (F16(1.0) + (a - F16(1.0)) * k_a) for a in a_c])
        kk_c = [(kk_in / n[..., None]).reshape(rows, C) for n in n_c]
        nkk = _minmax([-kk for kk in kk_c])
        kka = _minmax([kk * a for kk in kk_c for a in a_c])
        if layer0:
            v2 = (v, v)
        else:
            v2 = _minmax([v + (v_first - v) * gt for gt in (s_lo[bits(vg_pre)], s_hi[bits(vg_pre)])])
    return dict(k=k2, neg_kk=nkk, kka=kka, v=v2)


def reference(inp, ry=None):
    """inp: the dict make_inputs returns.  Returns state (the whole pool after the launch, exact), y (exact), lo / hi
    (binary16 [B,T,C], equal where out is unambiguous), mid (the half the binary64 values round to), the exact gating outputs
    and the ambiguity counts.  ry [C] (MODE 2): also xs_lo / xs_hi, the corners of xs = h(out * ry); the row sums are those of
    whatever admissible halves the kernel wrote: mm8_reference."""
    B, T, C = inp["k"].shape
    H = C // 64
    gt = gating(inp)
    S = np.ascontiguousarray(inp["state"]).copy()
    y = native.wkv7_seq(S, inp["r"], inp["w"], gt["k2"], gt["v2"], gt["neg_kk"], gt["kka"], inp["et"], slot_idx=inp["slot_idx"])
    rs = lambda x: x.reshape(B * T, C)
    lo, hi, mid, gn_lo, gn_hi, b_lo, b_hi = post_interval(rs(y), rs(inp["r"]), rs(gt["k2"]), rs(gt["v2"]), rs(inp["g"]), inp["r_k"],
                                                     inp["lnx_w"], inp["lnx_b"], H, inp["eps"])
    width = interval_width(lo, hi)
    out = dict(gt)
    if ry is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            out["xs_lo"], out["xs_hi"] = (x.reshape(B, T, C) for x in _minmax([lo * ry, hi * ry]))
    out.update(state=S, y=y, lo=lo.reshape(B, T, C), hi=hi.reshape(B, T, C), mid=mid.reshape(B, T, C), gn_lo=gn_lo, gn_hi=gn_hi, bonus_lo=b_lo, bonus_hi=b_hi,
               single=float((width == 1).mean()), wide=float((width > 2).mean()), widest=int(width.max()))
    return out


def interval_width(lo, hi):
    """Number of admissible bit patterns per element (1 where NaN is the one admissible result)."""
    nan = np.isnan(lo)
    return np.where(nan, 1, key(np.where(nan, 0, hi)) - key(np.where(nan, 0, lo)) + 1)


def mm8_reference(out1, ry, my):
    """The mm8 prologue of att.output from known halves out1 [B,T,C]: xs = h(out1 * ry) exact, S [B*T,H,3] the binary64 sums
    {sum xs, sum out1*my, sum out1} per head, and the bound of a binary32 evaluation, gamma_64 * sum|terms|."""
    B, T, C = out1.shape
    H = C // 64
    with np.errstate(over="ignore", invalid="ignore"):
        xs = out1 * ry
        terms = [xs.astype(F64), out1.astype(F64) * my.astype(F64), out1.astype(F64)]
        S = np.stack([t.reshape(B * T, H, 64).sum(-1) for t in terms], -1)
        bound = np.stack([np.abs(t).reshape(B * T, H, 64).sum(-1) for t in terms], -1) * (gamma(64) + SLACK)
    return xs, S, bound


def check(out, lo, hi, mid=None, group=64):
    """Bit equality where lo == hi, lo <= out <= hi elsewhere, NaN masks equal.  Returns counts; "bad" == 0 is a pass.
    mid (optional): the value the binary64 evaluation rounds to; "off_nearest" counts admissible elements that differ from it."""
    out, lo, hi = (np.asarray(x).reshape(-1) for x in (out, lo, hi))
    nan_w, nan_g = np.isnan(lo), np.isnan(out)
    z = lambda x: np.where(nan_w | nan_g, 0, x).astype(F16)
    ko, kl, kh = key(z(out)), key(z(lo)), key(z(hi))
    below, above = kl - ko, ko - kh
    dist = np.maximum(np.maximum(below, above), 0)
    bad = (nan_w != nan_g) | (dist > 0)
    res = dict(n=out.size, bad=int(bad.sum()), nan_mismatch=int((nan_w != nan_g).sum()), single=int(((kl == kh) & ~nan_w).sum()),
               worst=int(dist.max()) if out.size else 0,
               off_nearest=None if mid is None else int(((ko != key(z(np.asarray(mid).reshape(-1)))) & ~bad & ~nan_w).sum()), msg="")
    if res["bad"]:
        i = int(np.flatnonzero(bad)[np.argmax(np.where(nan_w != nan_g, 1 << 20, dist)[bad])])
        heads = np.unique(np.flatnonzero(bad) // group)
        res["msg"] = (f"{res['bad']} of {out.size} elements outside their interval ({res['nan_mismatch']} NaN mismatches), worst {res['worst']} "
                      f"halves at flat index {i} (group {i // group}, lane {i % group}): got {out[i]!r} want [{lo[i]!r}, {hi[i]!r}]; "
                      f"{len(heads)} groups affected, first {heads[:8].tolist()}")
    return res


def assert_check(out, lo, hi, mid=None, name="out", group=64):
    res = check(out, lo, hi, mid, group)
    assert res["bad"] == 0, f"{name}: {res['msg']}"
    return res


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm + token shift (rwkv7_add_ln_mix): the group norm's interval with one group of C channels, then
# out[m] = h(cur + h(h(shifted - cur) * mix[m])).  That tail is NOT monotone in cur once rounded, so the admissible halves of cur
# and of shifted are enumerated where their intervals hold at most ENUM patterns each; elsewhere (a normalised value next to
# zero) the real-arithmetic lerp cur (1 - mix) + shifted mix, monotone in both for 0 <= mix <= 1, bounds the result with the
# three roundings' error 2^-11 (2 |d mix| + |f|) (1 + 2^-10) + 3 * 2^-25 and one half of slack either side.

ENUM = 3


def from_key(kx):
    kx = np.asarray(kx, dtype=np.int32)
    return np.where(kx < 0, 0x8000 | (-kx - 1), kx).astype(np.uint16).view(F16)


def ln_mix_reference(x, delta, w, b, prev, mix, eps=1e-5, slot_idx=None):
    """x, delta [B,T,C] (delta may be None), prev [n_slots,C] the carry table, mix [n_mix,C] with 0 <= mix <= 1, n_mix 1 or 6, or
    None (n_mix = 0: out is the interval of cur, one plane, and there is no carry: carry = None).
    Returns x_new (exact), cur (lo, hi, mid) [B,T,C], out (lo, hi) [n_mix,B,T,C], carry (lo, hi) [n_slots,C]."""
    B, T, C = x.shape
    xn = x if delta is None else x + delta
    c_lo, c_hi, c_mid = (a.reshape(B, T, C) for a in group_norm_interval(xn.reshape(B * T, C), w, b, eps, group=C))
    if mix is None:
        return dict(x_new=xn, cur=(c_lo, c_hi, c_mid), out=(c_lo[None], c_hi[None]), carry=None)
    slots = np.arange(B) if slot_idx is None else np.asarray(slot_idx)
    p0 = prev[slots][:, None]
    s_lo = np.concatenate([p0, c_lo[:, :-1]], 1)
    s_hi = np.concatenate([p0, c_hi[:, :-1]], 1)
    carry_lo, carry_hi = prev.copy(), prev.copy()
    carry_lo[slots], carry_hi[slots] = c_lo[:, -1], c_hi[:, -1]
    kcl, kch, ksl, ksh = key(c_lo), key(c_hi), key(s_lo), key(s_hi)
    narrow = (kch - kcl < ENUM) & (ksh - ksl < ENUM)
    los, his = [], []
    for m in range(mix.shape[0]):
        mv = mix[m]
        assert (mv >= 0).all() and (mv <= 1).all()
        cands = []
        for i in range(ENUM):
            c = from_key(np.minimum(kcl + i, kch))
            for j in range(ENUM):
                sh = from_key(np.minimum(ksl + j, ksh))
                cands.append(c + (sh - c) * mv)
        lo, hi = _minmax(cands)
        if not narrow.all():
            m64 = mv.astype(F64)
            f = lambda c, sh: c.astype(F64) * (1 - m64) + sh.astype(F64) * m64
            dmax = np.maximum(np.abs(s_hi.astype(F64) - c_lo.astype(F64)), np.abs(s_lo.astype(F64) - c_hi.astype(F64))) * m64
            f_lo, f_hi = f(c_lo, s_lo), f(c_hi, s_hi)
            err = 2.0 ** -11 * (2 * dmax + np.maximum(np.abs(f_lo), np.abs(f_hi))) * (1 + 2.0 ** -10) + 3 * 2.0 ** -25
            wl, wh = from_key(key(h(f_lo - err)) - 1), from_key(key(h(f_hi + err)) + 1)
            lo, hi = np.where(narrow, lo, wl), np.where(narrow, hi, wh)
        los.append(lo)
        his.append(hi)
    return dict(x_new=xn, cur=(c_lo, c_hi, c_mid), out=(np.stack(los), np.stack(his)), carry=(carry_lo, carry_hi))


def ln_inputs(B, T, C, regime, seed=0, n_slots=None, n_mix=6):
    """Rows for rwkv7_add_ln_mix.  "plain": N(0,1) (as test_add_ln_mix); "offset": rows whose mean is 20-50 x their spread;
    "outlier": three channels at 100 x the rest."""
    rng = np.random.default_rng(seed)
    n_slots = B + 3 if n_slots is None else n_slots
    x = rng.standard_normal((B, T, C))
    if regime == "offset":
        x = x + rng.uniform(20, 50, (B, T, 1)) * rng.choice([-1.0, 1.0], (B, T, 1))
    elif regime == "outlier":
        x[..., rng.choice(C, 3, replace=False)] *= 100.0
    return dict(x=x.astype(F16), delta=(rng.standard_normal((B, T, C)) * 0.5).astype(F16), w=(1 + 0.1 * rng.standard_normal(C)).astype(F16),
                b=(0.1 * rng.standard_normal(C)).astype(F16), prev=rng.standard_normal((n_slots, C)).astype(F16),
                mix=rng.uniform(0, 1, (n_mix, C)).astype(F16), slot_idx=rng.permutation(n_slots)[:B].astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# The launch forms of rwkv7_add_ln_mix / rwkv7_add_ln_mix_mm8: n_mix 0 / 1 / 6, rows grouped R to a workgroup, delta from split-K
# planes, the mm8 correction of those planes (in_*), the mm8 prologue of the mixed planes (out_*).
#
#   planes    acc = ((0 + p_0) + p_1) + ...: binary32, plane order (the kernel adds the planes of a batch of PL loads in order and
#             the batches in order; -ffp-contract=off), delta = h(acc), x_new = h(x + delta): EXACT.
#   mm8 in_*  acc' = ((rx (acc - 1023.5 S0)) + S1) + mx S2 with S0, S1, S2 the sums of in_S_parts parts.  The inputs keep the PART
#             sums exact in any order (S0 parts even integers, S1 parts multiples of 2^-6, S2 parts of 2^-4, all small: the
#             exact-sum lemma), and 1023.5 S0 and mx S2 exact (asserted).  Every one of the four remaining operations contributes
#             its rounding u |result| only where its operands are exact and its binary64 result is not a binary32 number -- so
#             family "grid" (integer planes with acc - 1023.5 S0 an integer below 2^11, rx and |mx| powers of two) is exact from end
#             to end, and family "real" (any rx, mx, planes) is bounded by four roundings.  delta lies between h(D - e) and
#             h(D + e), x_new between h(x + h(D - e)) and h(x + h(D + e)) (both monotone).
#   after     the LayerNorm / lerp intervals are computed from the x_new the evaluation under test produced (the staged check): an
#             x_new inside its candidates with a wrong row behind it still fails.
#   mm8 out_* xs[m] = h(out[m] ry[m]) from the produced out[m] bits: exact.  S[m][row] = {sum xs, sum out my, sum out} over C terms
#             (the products of two halves are exact in binary32): binary64 sums, bound gamma(C) sum|terms| + SLACK in any order.
#             Planes >= out_planes of xs and S keep their canary.

CANARY = 7.0


def _is_f32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return v.astype(F32).astype(F64) == v


def ln_form_inputs(B, T, C, n_mix=6, splits=0, mm8_in=None, parts=1, out_planes=0, seed=0, regime="plain"):
    """ln_inputs plus what selects a launch form.  splits > 0: delta comes from `planes` (binary32 [splits,B,T,C]) and li["delta"] is
    None.  mm8_in "grid" / "real" (needs splits): the planes are core sums, with in_rx, in_mx [C] and in_S [B*T,parts,3] (see above).
    out_planes > 0: out_ry, out_my [out_planes,C], distinct per plane."""
    li = ln_inputs(B, T, C, regime, seed=seed, n_mix=max(n_mix, 1))
    rng = np.random.default_rng(seed + 7919)
    rows = B * T
    li.update(n_mix=n_mix, planes=None, family=mm8_in, in_rx=None, in_mx=None, in_S=None, out_ry=None, out_my=None)
    if n_mix == 0:
        li["mix"] = None
    if mm8_in is not None:
        assert splits > 0 and mm8_in in ("grid", "real")
        amp = max(1, int(round(24 / np.sqrt(parts))))
        nz = lambda: rng.integers(1, amp + 1, (rows, parts)) * rng.choice([-1, 1], (rows, parts))     # never 0: every part counts
        S = np.stack([2.0 * nz(), nz() * 2.0 ** -6, nz() * 2.0 ** -4], -1)
        t = 1023.5 * S[..., 0].sum(1)[:, None]
        if mm8_in == "grid":
            rx = 2.0 ** -rng.integers(10, 14, C)                              # rx A: multiples of 2^-10 .. 2^-13 below 2
            mx = rng.choice([-1.0, 1.0], C) * 2.0 ** -rng.integers(6, 9, C)        # mx S2: multiples of 2^-12, so h() rounds
            core = t + rng.integers(-2047, 2048, (rows, C))
            pl = rng.integers(-4096, 4097, (splits, rows, C)).astype(F64)
        else:
            rx = 2.0 ** -10 * rng.uniform(0.5, 2.0, C)
            mx = 0.1 * rng.standard_normal(C)
            core = t + 400.0 * rng.standard_normal((rows, C))
            pl = (2000.0 * rng.standard_normal((splits, rows, C))).astype(F32).astype(F64)
        pl[-1] = core - pl[:-1].sum(0)
        li.update(planes=pl.astype(F32).reshape(splits, B, T, C), delta=None, in_rx=rx.astype(F16), in_mx=mx.astype(F16), in_S=S.astype(F32))
    elif splits:
        li.update(planes=(rng.standard_normal((splits, B, T, C)) * 0.5 / np.sqrt(splits)).astype(F32), delta=None)
    if out_planes:
        li.update(out_ry=rng.uniform(0.5, 2.0, (out_planes, C)).astype(F16), out_my=(0.1 * rng.standard_normal((out_planes, C))).astype(F16))
    return li


def planes_sum(planes, dtype=F32):
    """((0 + p_0) + p_1) + ... in `dtype`, one rounding per addition."""
    acc = np.zeros(planes.shape[1:], dtype)
    for p in planes:
        acc = (acc + p.astype(dtype)).astype(dtype)
    return acc


def ln_delta_interval(li):
    """(d_lo, d_hi) binary16 [B,T,C]: the admissible deltas (equal bits: exact); (None, None) without a delta."""
    if li["planes"] is None:
        return li["delta"], li["delta"]
    B, T, C = li["x"].shape
    with np.errstate(over="ignore", invalid="ignore"):
        acc = planes_sum(li["planes"])
        if li["in_S"] is None:
            return h(acc), h(acc)
        S = li["in_S"].astype(F64)
        q = np.array([2.0, 2.0 ** -6, 2.0 ** -4])
        assert (S / q == np.round(S / q)).all() and (np.abs(S).sum(1) < 2.0 ** 24 * q).all(), "in_S parts off their grid: sums not exact"
        S = S.sum(1).reshape(B, T, 1, 3)
        S0, S1, S2 = S[..., 0], S[..., 1], S[..., 2]
        rx, mx = li["in_rx"].astype(F64), li["in_mx"].astype(F64)
        t, m = 1023.5 * S0, mx * S2
        assert _is_f32(t).all() and _is_f32(m).all(), "1023.5 S0 or mx S2 rounds: more than four roundings"
        A = acc.astype(F64) - t
        e = np.where(_is_f32(A), 0.0, U * np.abs(A))
        step = lambda v, e: np.where((e == 0) & _is_f32(v), 0.0, e + U * (np.abs(v) + e))      # one rounding, unless nothing rounds
        A, e = rx * A, np.abs(rx) * e
        e = step(A, e)
        A = A + S1
        e = step(A, e)
        A = A + m
        e = step(A, e)
        e = e + SLACK * np.abs(A) * (e > 0)
        return h(A - e), h(A + e)


def ln_form_reference(li, x_out=None, eps=1e-5):
    """The reference of one launch.  x_out: the x_new bits of the evaluation under test (needed where x_new has more than one
    candidate: the LN intervals are then those of x_out's rows); None: the lower candidate.
    Returns x_new (lo, hi), multi (the share of elements with more than one admissible x_new), and ln_mix_reference's cur / out /
    carry computed from x_out."""
    d_lo, d_hi = ln_delta_interval(li)
    x = li["x"]
    with np.errstate(over="ignore", invalid="ignore"):
        x_lo, x_hi = (x, x) if d_lo is None else (x + d_lo, x + d_hi)
    swap = key(x_lo) > key(x_hi)
    x_lo, x_hi = np.where(swap, x_hi, x_lo), np.where(swap, x_lo, x_hi)
    xn = x_lo if x_out is None else np.asarray(x_out).reshape(x.shape)
    ref = ln_mix_reference(xn, None, li["w"], li["b"], li["prev"], li["mix"], eps, li["slot_idx"])
    ref.update(x_new=(x_lo, x_hi), multi=float((bits(x_lo) != bits(x_hi)).mean()))
    return ref


def ln_mm8_out_reference(out, ry, my):
    """out [P,B,T,C] known halves (the first P mixed planes), ry, my [P,C] -> xs [P,B,T,C] exact, S [P,B*T,3] binary64 and its bound."""
    P, B, T, C = out.shape
    with np.errstate(over="ignore", invalid="ignore"):
        xs = out * ry[:, None, None, :]
        o64 = out.astype(F64)
        terms = [xs.astype(F64), o64 * my.astype(F64)[:, None, None, :], o64]
        S = np.stack([t.reshape(P, B * T, C).sum(-1) for t in terms], -1)
        bound = np.stack([np.abs(t).reshape(P, B * T, C).sum(-1) for t in terms], -1) * (gamma(C) + SLACK)
    return xs, S, bound


def ln_form_check(li, got, eps=1e-5):
    """got: x_new [B,T,C] (absent without a delta), out [max(n_mix,1),B,T,C], carry [n_slots,C] (n_mix > 0), and with out_planes: xs
    [3,B,T,C], S [3,B*T,3], both pre-filled with CANARY.  Returns counts: n / single / bad over x_new, the mixed planes and the carry
    rows; multi (the share of x_new with more than one candidate); fails: one line per property that does not hold (empty: pass)."""
    B, T, C = li["x"].shape
    n_mix = li["n_mix"]
    ref = ln_form_reference(li, got.get("x_new"), eps)
    res = dict(n=0, single=0, bad=0, multi=ref["multi"], fails=[])

    def add(name, r):
        res["n"] += r["n"]
        res["single"] += r["single"]
        res["bad"] += r["bad"]
        if r["bad"]:
            res["fails"].append(f"{name}: {r['msg']}")

    def same_bits(name, a, b):
        d = int((bits(np.asarray(a)) != bits(np.asarray(b))).sum()) if np.asarray(a).dtype == F16 else int((np.asarray(a) != np.asarray(b)).sum())
        if d:
            res["bad"] += d
            res["fails"].append(f"{name}: {d} of {np.asarray(a).size} elements differ")
    if "x_new" in got:
        add("x_new", check(got["x_new"], *ref["x_new"], group=C))
    add("out", check(got["out"], *ref["out"], group=C))
    if n_mix:
        add("carry", check(got["carry"], *ref["carry"], group=C))
        others = np.setdiff1d(np.arange(li["prev"].shape[0]), li["slot_idx"])
        same_bits("carry rows of other slots", got["carry"][others], li["prev"][others])
    if li["out_ry"] is not None:
        P = li["out_ry"].shape[0]
        xs, S, bound = ln_mm8_out_reference(np.asarray(got["out"])[:P], li["out_ry"], li["out_my"])
        same_bits("xs", got["xs"][:P], xs)
        with np.errstate(invalid="ignore"):
            off = ~(np.abs(got["S"][:P].astype(F64) - S) <= bound)
        res["n"] += off.size
        if off.any():
            res["bad"] += int(off.sum())
            r = np.argwhere(off)[0]
            res["fails"].append(f"S: {int(off.sum())} of {off.size} sums outside their bound, first [plane, row, k] = {r.tolist()}: got "
                                f"{got['S'][tuple(r)]!r} want {S[tuple(r)]!r} +- {bound[tuple(r)]:.3g}")
        same_bits("xs planes >= out_planes", got["xs"][P:], np.full_like(got["xs"][P:], CANARY))
        same_bits("S planes >= out_planes", got["S"][P:], np.full_like(got["S"][P:], CANARY))
    return res


def ln_emulate(li, order="pairwise", mutant=None, eps=1e-5, R=1, PL=8, full=False):
    """A binary32 evaluation of add_ln_mix on ln_inputs / ln_form_inputs.  order: "pairwise" (numpy) or "lanes" (per-lane partial sums
    added in order, then a sequential combine; the in_S parts lane-strided by 64).  R: rows per workgroup, PL: planes per batch
    (both only change what the mutants do).  mutant: one of LN_MUTANTS, "one_pass_variance" or "no_round_lerp".
    Returns (out [n_mix,B,T,C], cur), or with full=True the dict ln_form_check takes."""
    f = lambda a: np.asarray(a).astype(F32)
    x = li["x"]
    B, T, C = x.shape
    W = 128 if C % 128 == 0 else 64

    def rsum(a):
        if order == "pairwise":
            return a.sum(-1, keepdims=True, dtype=F32)
        part = a.reshape(a.shape[:-1] + (a.shape[-1] // W, W))
        acc = part[..., 0, :].copy()
        for i in range(1, part.shape[-2]):
            acc = acc + part[..., i, :]
        tot = acc[..., 0].copy()
        for j in range(1, W):
            tot = tot + acc[..., j]
        return tot[..., None]
    got = {}
    planes = li.get("planes")
    with np.errstate(over="ignore", invalid="ignore"):
        if planes is not None:
            if mutant == "planes_beyond_PL_dropped":
                planes = planes[:PL]
            acc = f(planes_sum(planes, F16 if mutant == "planes_summed_in_binary16" else F32))
            if li["in_S"] is not None:
                Sp = li["in_S"][:, :64] if mutant == "S_parts_beyond_64_dropped" else li["in_S"]
                if order == "pairwise":
                    S = Sp.sum(1, dtype=F32)
                else:
                    lanes = np.zeros((Sp.shape[0], 64, 3), F32)
                    for pp in range(Sp.shape[1]):
                        lanes[:, pp % 64] = lanes[:, pp % 64] + Sp[:, pp]
                    S = lanes[:, 0].copy()
                    for j in range(1, 64):
                        S = S + lanes[:, j]
                S = S.reshape(B, T, 1, 3)
                s0, s1, s2 = S[..., 0], S[..., 2 if mutant == "S1_S2_swapped" else 1], S[..., 1 if mutant == "S1_S2_swapped" else 2]
                off = F32(1024.0 if mutant == "offset_1024" else 1023.5)
                acc = f(li["in_rx"]) * (acc - off * s0) + s1 + f(li["in_mx"]) * s2
            xn = h(f(x) + (acc if mutant == "delta_added_unrounded" else f(h(acc))))
            got["x_new"] = xn
        elif li["delta"] is not None:
            xn = x + li["delta"]
            got["x_new"] = xn
        else:
            xn = x
        xf = f(xn)
        mean = rsum(xf) / F32(C)
        d = xf - mean
        var = rsum(xf * xf) / F32(C) - mean * mean if mutant == "one_pass_variance" else rsum(d * d) / F32(C)
        cur = h(d * (F32(1.0) / np.sqrt(var + F32(eps))) * f(li["w"]) + f(li["b"]))
        mix = li["mix"]
        if mix is None:
            got["out"] = cur[None]
            return got if full else (got["out"], cur)
        p0 = li["prev"][li["slot_idx"]]
        sh = np.concatenate([p0[:, None], cur[:, :-1]], 1)
        if mutant == "group_shift_from_carry":                   # a group's first row (t0 > 0) shifts against the carry table
            sh[:, R::R] = p0[:, None]
        outs = []
        for m in range(mix.shape[0]):
            dx = f(h(f(sh) - f(cur))) * f(mix[m])
            if mutant != "no_round_lerp":
                dx = f(h(dx))
            outs.append(h(f(cur) + dx))
        out = np.stack(outs)
        carry = li["prev"].copy()
        last = (T // R) * R - 1 if mutant == "carry_from_last_full_group" and T % R and T >= R else T - 1
        carry[li["slot_idx"]] = cur[:, last]
        got.update(out=out, carry=carry)
        if li.get("out_ry") is not None:
            P = li["out_ry"].shape[0]
            xs_all = np.full((3, B, T, C), CANARY, F16)
            S_all = np.full((3, B * T, 3), CANARY, F32)
            for m in range(P):
                ry = li["out_ry"][0 if mutant == "prologue_ry_of_plane_0" else m]
                xs = h(f(out[m]) * f(ry))
                S = np.concatenate([rsum(f(xs)), rsum(f(out[m]) * f(li["out_my"][m])), rsum(f(out[m]))], -1).reshape(B * T, 3)
                xs_all[m] = xs
                if mutant == "out_S_rows_by_t":
                    for row in range(B * T):
                        S_all[m, row % T] = S[row]
                else:
                    S_all[m] = S
            got.update(xs=xs_all, S=S_all)
    return got if full else (out, cur)


# Defects of a launch form that the reference must reject (tests/test_tmix_ref_cpu.py), each the counterpart of one line of the kernel
LN_MUTANTS = ["group_shift_from_carry", "carry_from_last_full_group", "planes_summed_in_binary16", "planes_beyond_PL_dropped",
              "delta_added_unrounded", "offset_1024", "S_parts_beyond_64_dropped", "S1_S2_swapped", "prologue_ry_of_plane_0",
              "out_S_rows_by_t"]


# ---------------------------------------------------------------------------------------------------------------------
# the guarded input generator

def make_inputs(B, T, C, layer0, regime="plain", seed=0, n_slots=None, elapsed="arange", edges=False, state=None):
    """Seeded inputs of one launch of the fused time-mix core.  regime: "plain" (util.wkv7_inputs' distributions), "offset"
    (heads of y with a mean far above their spread: a state of nearly equal positive entries read by a nearly constant
    positive r, slow decay, small k), "outlier" (four channels of k, v, r at 50-100x the rest; the rest scaled down so that
    k*v*r stays finite over T).  edges (needs B >= 8, C >= 128): the edge values of test_fused_edge_values.
    Returns (inp, stats): stats = sigmoid inputs replaced / total, heads redrawn / total."""
    rng = np.random.default_rng(seed)
    H = C // 64
    n_slots = B if n_slots is None else n_slots
    N = lambda *s: rng.standard_normal(s)
    if regime == "plain":
        st = N(n_slots, H, 64, 64) * 0.5
        r, k, v = N(B, T, C), N(B, T, C), N(B, T, C)
        w = rng.uniform(-8.0, 4.0, (B, T, C))
    elif regime == "offset":
        st = 0.5 + 0.004 * N(n_slots, H, 64, 64)
        r = 1.0 + 0.05 * N(B, T, C)
        k, v = 0.02 * N(B, T, C), 0.5 * N(B, T, C)
        w = rng.uniform(-9.0, -7.0, (B, T, C))
    elif regime == "outlier":
        st = N(n_slots, H, 64, 64) * 0.1
        ch = rng.choice(C, 4, replace=False)
        r, k, v = (0.05 * N(B, T, C) for _ in range(3))
        for x in (r, k, v):
            x[..., ch] *= rng.uniform(50, 100, 4)
        w = rng.uniform(-8.0, 4.0, (B, T, C))
    else:
        raise ValueError(regime)
    st = st.astype(F16) if state is None else state
    r, k, v, w = (x.astype(F16) for x in (r, k, v, w))
    a_pre, vg_pre, v_first, g = (N(B, T, C).astype(F16) for _ in range(4))
    k_k = (0.85 + 0.05 * N(C)).astype(F16)
    k_a = (1 + 0.05 * N(C)).astype(F16)
    r_k = (0.1 * N(C)).astype(F16)
    lw = (1 + 0.1 * N(C)).astype(F16)
    lb = (0.1 * N(C)).astype(F16)
    if elapsed == "arange":
        et = (np.arange(B) * 7 + 3).astype(np.int32)
    elif elapsed == "big":                                  # elapsed + t wraps the int32 multiply
        et = rng.integers(2 ** 30, 2 ** 31 - 1 - T, size=B).astype(np.int32)
        et[0] = 2 ** 31 - 1 - T
    elif elapsed == "zero":
        et = np.zeros(B, np.int32)
    else:
        et = np.asarray(elapsed, dtype=np.int32)
    slot_idx = rng.permutation(n_slots)[:B].astype(np.int32) if n_slots != B else None     # a permutation into a larger pool
    zero_head = None
    if edges:
        assert B >= 8 and C >= 128 and slot_idx is None
        st[0] = 0
        st[1] = F16(6e-8)                    # subnormal state
        st[2, :, ::2] = F16(-0.0)
        w[0] = F16(60000.0)                  # sigmoid -> 1
        w[1] = F16(-60000.0)                 # sigmoid -> 0: w~ is the dither alone
        a_pre[2] = F16(60000.0)              # a = 1 exactly
        a_pre[3] = F16(-60000.0)             # a = 0 exactly
        vg_pre[4] = F16(60000.0)
        vg_pre[5] = F16(-60000.0)
        g[6] = 0
        g[6, :, ::3] = F16(-0.0)
        v_first[7] = v[7]
        k[3, :, 64:128] = 0                  # one head with k = 0: NaN, by 0/0 in F.normalize, in that head's state rows and outputs
        zero_head = (3, 1)
        et = np.array([0, 2 ** 31 - 3, 1, 123456789, 2 ** 31 - 1 - T, 5, 2 ** 30, 77], np.int32)[:B] if B == 8 else et
    a_pre, n1 = guard_preact(a_pre)
    n_gate = a_pre.size
    n2 = 0
    if not layer0:
        vg_pre, n2 = guard_preact(vg_pre)
        n_gate += vg_pre.size
    # heads whose norm is ambiguous: redraw k
    redrawn = 0
    k4 = k.reshape(B, T, H, 64)
    for _ in range(20):
        n_lo, n_hi = norm_interval((k * k_k).reshape(B, T, H, 64))
        amb = bits(n_lo) != bits(n_hi)
        if not amb.any():
            break
        redrawn += int(amb.sum())
        scale = np.abs(k4[amb].astype(F64)).max(-1, keepdims=True) / 3
        k4[amb] = (k4[amb].astype(F64) + 0.3 * scale * N(int(amb.sum()), 64)).astype(F16)
    inp = dict(state=st, slot_idx=slot_idx, r=r, w=w, k=k, v=v, a_pre=a_pre, vg_pre=vg_pre, v_first=v_first, g=g, k_k=k_k, k_a=k_a,
               r_k=r_k, lnx_w=lw, lnx_b=lb, et=et, layer0=bool(layer0), eps=EPS, zero_head=zero_head)
    stats = dict(replaced=n1 + n2, gates=n_gate, redrawn=redrawn, heads=B * T * H)
    return inp, stats


# ---------------------------------------------------------------------------------------------------------------------
# binary32 evaluations of the kernel's chain in a chosen reduction order, with optional defects: what the CPU tests hold the
# checker to (legitimate orders pass, mutants are rejected)

_XOR = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def sum32(x, order):
    """x [..., 64] binary32 -> [..., 1] binary32 sum in the given order."""
    x = np.ascontiguousarray(x, dtype=F32)
    if order == "pairwise":
        return x.sum(-1, keepdims=True, dtype=F32)
    if order == "butterfly":                 # wave_sum: o = 32 .. 1, every lane ends with the same total
        for idx in _XOR:
            x = x + x[..., idx]
        return x[..., :1]
    if order == "sequential":
        acc = x[..., 0].copy()
        for j in range(1, 64):
            acc = acc + x[..., j]
        return acc[..., None]
    raise ValueError(order)


def emulate(inp, order="butterfly", mutant=None):
    """The fused kernel's arithmetic on the CPU in binary32 / binary16, the four reductions in `order`.  mutant: one of MUTANTS.
    Returns (out [B,T,C] binary16, state pool after the launch)."""
    f = lambda x: np.asarray(x).astype(F32)
    B, T, C = inp["k"].shape
    H = C // 64
    k, v, r = inp["k"], inp["v"], inp["r"]
    k_k, k_a = inp["k_k"], inp["k_a"]
    if mutant == "ka_kk_swapped":
        k_k, k_a = k_a, k_k
    sig = lambda x: h(F32(1.0) / (F32(1.0) + np.exp(-f(x))))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a = sig(inp["a_pre"])
        kk_in = h(f(k) * f(k_k)).reshape(B, T, H, 64)
        sq = f(kk_in) * f(kk_in)
        ss = sum32(sq, order)
        if mutant == "half_wave":            # head 0 of every row reduced over 32 lanes only
            ss[:, :, 0] = sum32(np.concatenate([sq[:, :, 0, :32], np.zeros_like(sq[:, :, 0, :32])], -1), order)
        nrm = h(np.sqrt(ss))
        kk = h(f(kk_in) / f(nrm)).reshape(B, T, C)
        t1 = f(a) - F32(1.0)
        if mutant != "no_round_a_minus_1":
            t1 = f(h(t1))
        k2 = h(f(k) * f(h(F32(1.0) + f(h(t1 * f(k_a))))))
        kka = h(f(kk) * f(a))
        v2 = v
        if not inp["layer0"] or mutant == "v_gate_at_layer0":
            d = f(h(f(inp["v_first"]) - f(v))) * f(sig(inp["vg_pre"]))
            if mutant != "no_round_vgate":
                d = f(h(d))
            v2 = h(f(v) + d)
        S = np.ascontiguousarray(inp["state"]).copy()
        et = inp["et"] + 1 if mutant == "elapsed_off_by_one" else inp["et"]
        y = native.wkv7_seq(S, r, inp["w"], k2, v2, h(-f(kk)), kka, et, slot_idx=inp["slot_idx"])
        yf = f(y).reshape(B, T, H, 64)
        mean = sum32(yf, order) * F32(1.0 / 64.0)
        dlt = yf - mean
        if mutant == "one_pass_variance":
            var = sum32(yf * yf, order) * F32(1.0 / 64.0) - mean * mean
        else:
            dsq = dlt * dlt
            var = sum32(dsq, order) * F32(1.0 / 64.0)
            if mutant == "half_wave":
                var[:, :, 0] = sum32(np.concatenate([dsq[:, :, 0, :32], np.zeros_like(dsq[:, :, 0, :32])], -1), order) * F32(1.0 / 64.0)
        eps = F32(1e-5) if mutant == "eps_1e-5" else F32(inp["eps"])
        rstd = F32(1.0) / np.sqrt(var + eps)
        gn = h(dlt * rstd * f(inp["lnx_w"]).reshape(H, 64) + f(inp["lnx_b"]).reshape(H, 64))
        bt = f(h(f(h(f(r) * f(k2))) * f(inp["r_k"]))).reshape(B, T, H, 64)
        bonus = h(sum32(bt, order))
        bv = f(bonus) * f(v2).reshape(B, T, H, 64)
        if mutant != "no_round_bonus_v":
            bv = f(h(bv))
        out = h(f(h(f(gn) + bv)) * f(inp["g"]).reshape(B, T, H, 64)).reshape(B, T, C)
    slots = np.arange(B) if inp["slot_idx"] is None else inp["slot_idx"]
    if mutant == "heads_swapped_between_slots" and B >= 2:
        s0, s1 = int(slots[0]), int(slots[1])
        S[[s0, s1], 0] = S[[s1, s0], 0]
    if mutant == "untouched_slot_overwritten":
        free = sorted(set(range(S.shape[0])) - set(int(s) for s in slots))
        S[free[0], 0, 0, :8] = F16(1.0)
    return out, S


MUTANTS = ["eps_1e-5", "no_round_bonus_v", "no_round_a_minus_1", "no_round_vgate", "one_pass_variance", "ka_kk_swapped", "half_wave",
           "heads_swapped_between_slots", "v_gate_at_layer0", "elapsed_off_by_one", "untouched_slot_overwritten"]


# The cases of the GPU test of the fused kernel (tests/test_fused_gpu.py) and of the CPU tests of this reference
# (tests/test_tmix_ref_cpu.py): id -> make_inputs arguments.  Each of C in {64, 128, 768, 2048, 4096}, B in {1, 3, 200, 256},
# T in {1, 2, 5, 31}, both layer kinds, the three regimes and the three elapsed_t kinds appears at least once.
CASES = {
    "plain-B200-T1-C4096": dict(B=200, T=1, C=4096, layer0=False, regime="plain", n_slots=208),
    "plain-B1-T31-C768": dict(B=1, T=31, C=768, layer0=False, regime="plain", elapsed="zero", n_slots=3),
    "plain-B25-T31-C4096": dict(B=25, T=31, C=4096, layer0=False, regime="plain", n_slots=32),
    "plain-B256-T1-C2048-layer0": dict(B=256, T=1, C=2048, layer0=True, regime="plain", elapsed="big"),
    "plain-B3-T5-C64-layer0": dict(B=3, T=5, C=64, layer0=True, regime="plain", n_slots=7),
    "plain-B3-T2-C128": dict(B=3, T=2, C=128, layer0=False, regime="plain", elapsed="big", n_slots=5),
    "offset-B3-T1-C768": dict(B=3, T=1, C=768, layer0=False, regime="offset", n_slots=6),
    "offset-B200-T1-C4096-layer0": dict(B=200, T=1, C=4096, layer0=True, regime="offset"),
    "offset-B3-T5-C2048": dict(B=3, T=5, C=2048, layer0=False, regime="offset", elapsed="big", n_slots=4),
    "outlier-B3-T2-C768-layer0": dict(B=3, T=2, C=768, layer0=True, regime="outlier", n_slots=9),
    "outlier-B25-T31-C4096": dict(B=25, T=31, C=4096, layer0=False, regime="outlier", elapsed="zero", n_slots=26),
    "outlier-B256-T1-C128": dict(B=256, T=1, C=128, layer0=False, regime="outlier", n_slots=300),
}


def case_inputs(name):
    kw = dict(CASES[name])
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003
    return make_inputs(seed=seed, **kw)


# Edge values in one launch (make_inputs(edges=True)): zero / subnormal / -0.0 state, w = +-60000, a_pre / vg_pre = +-60000,
# g = +-0, v_first == v, one head with k = 0, elapsed_t that wraps the int32 multiply.
EDGE_CASE = dict(B=8, T=2, C=128, layer0=False, regime="plain", edges=True, seed=5)


def chain_inputs(steps=64, B=4, C=256, n_slots=6, seed=1000):
    """`steps` chained T = 1 launches on one state pool: fresh guarded inputs every step, the reference's state of step i is the
    input state of step i + 1, elapsed_t advances by one per step.  Yields (inp, reference(inp))."""
    state, slot_idx, et0 = None, None, None
    for i in range(steps):
        inp, _ = make_inputs(B, 1, C, layer0=False, regime="plain", seed=seed + i, n_slots=n_slots, state=state)
        if i == 0:
            slot_idx, et0 = inp["slot_idx"], inp["et"]
        inp["slot_idx"], inp["et"] = slot_idx, (et0 + i).astype(np.int32)
        ref = reference(inp)
        state = ref["state"]
        yield inp, ref
