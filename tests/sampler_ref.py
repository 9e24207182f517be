"""Binary64 admissible-set reference of the top-p / top-k / temperature draw (csrc/sampler.hip: sample_topp_kernel), its input
families and its sets of uniforms.  TEST INFRASTRUCTURE ONLY, CPU only, plain numpy; nothing here comes from the kernel.

The operation, for one row of binary16 logits x, T and top_p as the binary16 values the kernel reads, top_k, one binary32 u:
    m_i = exp(x_i - max x),  Z = sum m_i
    cutoff   the distinct values in descending order v_1 > v_2 > ..., M_j = mass of the tokens >= v_j: the smallest prefix whose
             mass reaches top_p Z is kept, ties at its last value included (top_p = 0: the maxima)
    top-k    the K-th largest value, ties kept; the effective threshold is the larger of the two
    weights  w_i = (m_i / Z)^(1/T) for kept tokens, 0 otherwise;  C_i = sum_{k <= i} w_k in id order,  W = C_{V-1}
    draw     the first token of positive weight whose C_i exceeds u W
A kernel evaluates the masses and weights with a fast binary32 exponential and adds them in binary32 in an order of its own, so
for some inputs more than one id is a correct answer.  admissible() returns ALL of them; a kernel is right when its id is one.

Bounds.  With u24 = 2^-24 (half a binary32 ulp, the relative error of one rounding):

  any-order summation   a binary32 sum of n non-negative terms, in any order and association, differs from the exact sum S of
                        the terms it was given by at most (n - 1) u24 S to first order: each addition rounds a partial sum <= S
                        once.  Only terms that can move a partial sum need counting: n_sig = the number of terms above 2^-40 S;
                        a smaller term, added or lost to rounding, changes the result by at most itself, so the terms below
                        2^-40 S contribute their own total.
  fast exponential      exp(a) evaluated as exp2(a log2 e): the product rounds once and log2 e is itself a rounded constant
                        (together 1.5 |a| u24 on the result, an absolute error of the exponent being a relative error of the
                        power), the exp2 instruction is good to one ulp (2 u24); the round figure (|a| + 2) 2^-23 = (2 |a| +
                        4) u24 covers these with one further rounding (the division by Z, the conversion of the argument).  For
                        T != 1 the argument itself is computed, a = (x - max - ln Z) / T: two subtractions (<= 2 T |a| u24 <= 3 |a|
                        u24 for T <= 1.5), the rounding of 1 / T and the product with it (2 |a| u24).  An error common to all
                        tokens (ln Z, Z) scales every weight alike and cancels in u W against C.  In all: (7 |a| + 4) u24 per
                        term, used for every T; in a sum the terms' errors enter weighted by the terms,
                        c_exp = sum t_i (7 |a_i| + 4) / S   [units of u24].
  e, delta / W          (n_sig + c_exp) u24 + (total of the terms below 2^-40 S) / S, DOUBLED: both sides of each comparison
                        carry the bound -- M_j against top_p Z (two sums), the lane's partial sum C against u W (W is a sum of
                        the same terms) -- and the doubling also covers the second-order terms and the product's own rounding.
  Nothing here is fitted to a kernel's output.

Cutoff.  j is admissible unless it is excluded for certain, M_j (1 + e) < top_p Z (1 - e), or its predecessor holds for certain,
M_{j-1} (1 - e) >= top_p Z (1 + e).  With top_p = 1 no prefix is certain, so the last j, "keep everything", is admissible with
every j whose mass is within the bound of Z.  top_p = 0 leaves j = 1: the maxima.  Top-k works on counts and is exact.
(The contiguity of a draw's admissible ids is by construction: per kept set they are a run of its positive-weight ids, and the
kept sets are nested.)
Draw.  Per admissible cutoff, a kept token of positive weight is admissible when [C_{i-1} - delta, C_i + delta] contains u W.  A
token whose binary32 weight may flush to zero (below 2^-125) has an interval narrower than delta: it is admissible only
together with its neighbours, never alone (never required).  A weight below 2^-151 is 0 in binary32 whatever the denormal mode
(the smallest denormal is 2^-149): such a token has no positive weight and is never admissible.

Inputs (section "cases"): sparse-significant rows -- at most N_SIG logits drawn N(0, 2.5^2), the rest at a floor, -inf (a
forbidden token) or max - 120 (a mass that underflows or is negligible) -- so that n_sig, and with it the bound, does not grow
with V.  The significant logits sit at ids 0 and V - 1, at the first and last id of lanes' chunks, on both sides of wave
boundaries, in every 8192-token load stride and in the ragged last group of eight.  Two properties of the REFERENCE are
conditions of the tests (test_sampler_ref_cpu.py asserts them on the reference alone): at least 95 % of random draws have one
admissible id, and no draw of the boundary sweep has more than three, contiguous in kept order.  Two choices of the inputs serve
them: (1) a kept token narrower than 2.5 delta is placed between two wider ones (three ids at most share a point then); the
narrow tokens that cannot be separated that way are left at the floor; (2) the top_p = 1 / top_k = 0 cases take the -inf floor: a
kept max - 120 floor would put hundreds of negligible ids of positive weight between two significant tokens."""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
U24 = 2.0 ** -24
TINY = 2.0 ** -40            # terms below TINY * sum cannot be counted on to move a binary32 partial sum
ZERO = 2.0 ** -151           # a weight below this is 0 in binary32 for certain
LANES, STRIDE = 1024, 8192   # the kernel's lanes per row and tokens per load stride
N_SIG = 96


def sum_bound(terms, args):
    """Relative bound (module docstring: e, delta / W) of a binary32 any-order sum of the positive binary64 `terms`, each the fast
    exponential of `args`."""
    S = float(terms.sum())
    if S <= 0.0:
        return 0.0
    sig = terms > TINY * S
    c_exp = float((terms[sig] * (7.0 * np.abs(args[sig]) + 4.0)).sum()) / S
    return 2.0 * ((int(sig.sum()) + c_exp) * U24 + float(terms[~sig].sum()) / S)


class Prepared:
    """One row with one (T, top_p, top_k): the admissible kept sets, each with its positive-weight ids, CDF, W and delta."""

    def __init__(self, x16, T, top_p, top_k):
        x16 = np.asarray(x16, F16)
        self.V = V = x16.size
        x = x16.astype(F64)
        Tq, Pq, K = float(F16(T)), float(F16(top_p)), int(top_k)
        a = x - x.max()
        with np.errstate(under="ignore"):
            m = np.exp(a)
        Z = float(m.sum())
        nz = m > 0
        self.e = e = sum_bound(m[nz], a[nz])
        order = np.argsort(-x, kind="stable")
        sx = x[order]
        cm = np.cumsum(m[order])
        last = np.nonzero(np.append(sx[1:] != sx[:-1], True))[0]         # last index of every run of equal values
        vj, Mj = sx[last], cm[last]
        target = Pq * Z
        prev = np.concatenate([[-1.0], Mj[:-1]])
        ok = ~(Mj * (1 + e) < target * (1 - e)) & ~(prev * (1 - e) >= target * (1 + e))
        ok[0] |= target == 0
        kth = sx[min(K, V) - 1] if K > 0 else -np.inf
        self.cut_values = vj[ok]                                          # the admissible top-p cutoffs (before top-k)
        self.alts, seen = [], set()
        lnZ = np.log(Z)
        for v in self.cut_values:
            kept = x >= max(v, kth)
            b = (a - lnZ) / Tq
            with np.errstate(under="ignore"):
                w = np.where(kept, np.exp(b), 0.0)
            pos = np.nonzero(w >= ZERO)[0]
            if pos.tobytes() in seen:
                continue
            seen.add(pos.tobytes())
            wp = w[pos]
            C = np.cumsum(wp)
            W = float(C[-1])
            delta = W * sum_bound(wp, b[pos])
            self.alts.append(dict(thr=max(v, kth), kept=kept, pos=pos, w=wp, C=C, Cprev=np.concatenate([[0.0], C[:-1]]), W=W, delta=delta))

    def ranges(self, us):
        """Per admissible kept set: (pos, lo, hi) -- the ids pos[lo[i]..hi[i]] are admissible for us[i]."""
        us = np.asarray(us, F32).astype(F64)
        out = []
        for alt in self.alts:
            want = us * alt["W"]
            n = len(alt["pos"])
            lo = np.minimum(np.searchsorted(alt["C"], want - alt["delta"], side="left"), n - 1)
            hi = np.maximum(np.searchsorted(alt["Cprev"], want + alt["delta"], side="right") - 1, 0)
            out.append((alt["pos"], lo, np.maximum(hi, lo)))
        return out

    def accepts(self, us, ids):
        """bool per draw: ids[i] is admissible for us[i]."""
        ids = np.asarray(ids).astype(np.int64)
        ok = np.zeros(ids.shape, bool)
        for pos, lo, hi in self.ranges(us):
            k = np.minimum(np.searchsorted(pos, ids), len(pos) - 1)
            ok |= (pos[k] == ids) & (lo <= k) & (k <= hi)
        return ok

    def sets(self, us):
        """Per draw: the length of the shortest run, in the kept order of the widest kept set, that holds every admissible id (the
        number of admissible ids when there is one kept set; an upper bound of it otherwise: the kept sets are nested)."""
        wide = max(self.alts, key=lambda alt: len(alt["pos"]))["pos"]
        first = last = None
        for pos, lo, hi in self.ranges(us):
            a, b = np.searchsorted(wide, pos[lo]), np.searchsorted(wide, pos[hi])
            first, last = (a, b) if first is None else (np.minimum(first, a), np.maximum(last, b))
        size = last - first + 1
        if len(self.alts) > 1:                                 # the exact count where the run is long
            rs = self.ranges(us)
            for i in np.nonzero(size > 1)[0]:
                size[i] = len(set().union(*[pos[lo[i]:hi[i] + 1].tolist() for pos, lo, hi in rs]))
        return size


def admissible(x16, T, top_p, top_k, u):
    """The set of ids a correct kernel may return for one row and one uniform."""
    out = set()
    for pos, lo, hi in Prepared(x16, T, top_p, top_k).ranges([u]):
        out.update(int(t) for t in pos[lo[0]:hi[0] + 1])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases

VS = (8, 1000, 1024, 8192, 8200, 50304, 65536)
TS = (0.5, 0.7, 1.0, 1.5)
SETTINGS = ("p0.3", "p0.9", "p1.0", "k1", "k5", "k20", "ktie", "ptie", "allneg", "big", "slots", "underflow")


def _placement(V, rng):
    """Ids in priority order: the deliberate places first, then random ones, N_SIG at most."""
    per = -(-V // LANES)
    nl = -(-V // per)
    ids = [0, V - 1, V - 8, V - 5, V - 2]
    for w in (1, 2, 8, 15):                                 # both sides of a wave boundary
        if 64 * w < nl:
            ids += [min(64 * w * per, V) - 1, 64 * w * per]
    for t in rng.choice(nl, size=min(3, nl), replace=False):  # first and last id of a lane's chunk
        ids += [int(t) * per, min(int(t) * per + per, V) - 1]
    for s in range(-(-V // STRIDE)):                        # every load stride
        ids += [s * STRIDE, min(s * STRIDE + STRIDE, V) - 1]
    for i in rng.choice(V // 4, size=min(4, V // 4), replace=False):    # four neighbours in one lane's group of eight: the kernel
        ids += [4 * int(i) + k for k in range(4)]                       # adds them pair by pair in Z and one by one in the cutoff,
                                                                        # so with top_p = 1 its mass{all} can miss Z by an ulp
    ids = [i for i in dict.fromkeys(ids) if 0 <= i < V]
    rest = rng.permutation(V)
    taken = set(ids)
    for i in rest:
        if len(ids) >= min(V, N_SIG):
            break
        if int(i) not in taken:
            ids.append(int(i))
    return np.array(ids[:min(V, N_SIG)], np.int64)


def _variants(setting, T):
    T2 = TS[(TS.index(T) + 1) % len(TS)]
    return {"p0.3": [(T, 0.3, 0)], "p0.9": [(T, 0.9, 0)], "p1.0": [(T, 1.0, 0)], "k1": [(T, 1.0, 1)], "k5": [(T, 1.0, 5)],
            "k20": [(T, 1.0, 20)], "ktie": [(T, 1.0, 5)], "ptie": [(T, 0.6, 0)], "allneg": [(T, 0.9, 0)], "big": [(T, 0.9, 0)],
            "slots": [(T, 0.9, 0), (T2, 1.0, 5), (T, 0.3, 0), (T2, 1.0, 20)],
            # beside the T list: kept tokens whose weight is 0 in binary32 FOR CERTAIN.  With T >= 0.5 there are none (a mass
            # large enough to be kept for certain has p^(1/T) >= 1e-14), so this setting runs at T = 0.1 whatever the T of the loop
            "underflow": [(0.1, 1.0, 0)]}[setting]


def _values(setting, n, rng, P):
    v = (rng.standard_normal(n) * 2.5).astype(F16)
    if setting == "allneg":
        v = (v.astype(F32) - 20.0).astype(F16)
        v = np.minimum(v, F16(-0.5))
    elif setting == "big":
        v = np.where(np.arange(n) % 3 == 0, F16(65504), np.where(np.arange(n) % 3 == 1, F16(65472), F16(-65504))).astype(F16)
        v = v[rng.permutation(n)]
    elif setting == "underflow":                             # logits 0 .. -3/8, and -8: p ~ 5e-6 each, kept for certain by
        v = (-0.125 * rng.integers(0, 4, n)).astype(F16)     # top_p = 1 as a group; p^10 < 2^-151
        v[rng.permutation(n)[:n // 4]] = F16(-8.0)
        v[0] = F16(0.0)
    elif setting == "ktie" and n >= 8:                       # four tokens tied at the K-th value (K = 5): ranks 4..7
        s = np.sort(v)[::-1].copy()
        s[3:7] = s[6]
        v = s[rng.permutation(n)]
    elif setting == "ptie" and n >= 8:                       # the top-p crossing inside a group of four tied values
        s = np.sort(v)[::-1].copy()
        for r in range(0, n - 4):
            t = s.copy()
            t[r:r + 4] = t[r + 3]
            m = np.exp(t.astype(F64) - float(t[0]))
            cm, z = np.cumsum(m), m.sum()
            above = cm[r - 1] if r else 0.0
            if above + 0.5 * m[r] < P * z < cm[r + 3] - 0.5 * m[r]:
                s = t
                break
        v = s[rng.permutation(n)]
    return v


def make_case(V, setting, T, seed=0):
    """dict(x = binary16 [V], variants = [(T, top_p, top_k), ...], preps = their Prepared references, name, floor)."""
    iv, ist, it = VS.index(V), SETTINGS.index(setting), TS.index(T)
    variants = _variants(setting, T)
    neg_inf_floor = setting in ("p1.0", "underflow") or V == 8 or (iv + ist + it) % 2 == 0
    for attempt in range(50):
        rng = np.random.default_rng(1000003 * seed + 10007 * iv + 101 * ist + 7 * it + 7919 * attempt)
        ids = _placement(V, rng)
        vals = _values(setting, len(ids), rng, float(F16(variants[0][1])))
        floor = F16(-np.inf) if neg_inf_floor else F16(np.float32(vals.max()) - 120.0)

        def row(ids_, vals_):
            x = np.full(V, floor, F16)
            x[ids_] = vals_
            return x

        # the variant that keeps the most tokens decides which kept tokens are narrow (module docstring, choice 1)
        preps = [Prepared(row(ids, vals), *v) for v in variants]
        alt = max((max(p.alts, key=lambda a_: len(a_["pos"])) for p in preps), key=lambda a_: len(a_["pos"]))
        wfull = np.zeros(V)
        wfull[alt["pos"]] = alt["w"]
        wv = wfull[ids]
        wide = np.nonzero(wv >= 2.5 * alt["delta"])[0]
        narrow = np.nonzero((wv > 0) & (wv < 2.5 * alt["delta"]))[0]
        other = np.nonzero(wv <= 0)[0]
        narrow = narrow[np.argsort(-wv[narrow])][:max(len(wide) - 1, 0)]           # the surplus stays at the floor
        seq = []                                                                   # wide narrow wide narrow ... wide wide
        wide = list(rng.permutation(wide))
        for k, b in enumerate(wide):
            seq.append(b)
            if k < len(narrow):
                seq.append(narrow[k])
        for o in other:                                                            # tokens outside the kept set: anywhere
            seq.insert(int(rng.integers(0, len(seq) + 1)), o)
        seq = np.array(seq, np.int64)
        use = np.sort(ids[:len(seq)])
        x = row(use, vals[seq])
        preps = [Prepared(x, *v) for v in variants]
        # a cutoff the bound cannot decide would make most draws of the case ambiguous: such a draw of the inputs is not used
        # (top_p = 1 always has a tail of admissible cutoffs; its kept sets differ by tokens of mass below the bound)
        # (top_p = 1: a draw of the inputs whose nested kept sets put a fourth id within the bound of a lane boundary is not used)
        if all((len(p.alts) == 1 or (v[1] == 1.0 and p.sets(boundary_uniforms(p, V, 30 if V > 8200 else None)).max() <= 3))
               for p, v in zip(preps, variants)):
            return dict(x=x, variants=variants, name=f"V{V}-{setting}-T{T}", floor=float(floor), preps=preps)
    raise AssertionError(f"no decidable inputs for V{V}-{setting}-T{T}")


def _ulps(c, k):
    """The binary32 values c[i] + j ulps, j = -k .. k (c >= 0)."""
    b = np.asarray(c, F32).view(np.int32).astype(np.int64)[:, None] + np.arange(-k, k + 1)[None, :]
    b = np.unique(b[b >= 0])
    return b.astype(np.int32).view(F32)


def boundary_uniforms(prep, V, max_boundaries=None, k=16):
    """Every binary32 u within +-k ulps of C(boundary) / W for the lane boundaries with positive weight on their left: lane t
    owns ids [t per, (t + 1) per), per = ceil(V / 1024).  (The hardware's sums differ from any emulation's by an ulp here and
    there, so the sweep covers the neighbourhood.)"""
    alt = max(prep.alts, key=lambda a_: len(a_["pos"]))
    per = -(-V // LANES)
    ends = np.minimum((np.arange(-(-V // per)) + 1) * per, V) - 1
    idx = np.searchsorted(alt["pos"], ends, side="right")
    has = idx > np.concatenate([[0], idx[:-1]])
    idx = idx[has]
    if max_boundaries is not None and len(idx) > max_boundaries:
        idx = idx[np.unique(np.linspace(0, len(idx) - 1, max_boundaries).round().astype(int))]
    us = _ulps((alt["C"][idx - 1] / alt["W"]).astype(F32), k)
    return us[(us >= 0) & (us < 1)]


def uniforms(case, kind, n_random=2000, max_rows=None, seed=0):
    """(us binary32 [n], variant index [n]) of a case: kind "random" (n_random draws, u = 0 and 1 - 2^-24 among them) or
    "boundary" (max_rows caps the sweep: it then takes evenly spaced boundaries)."""
    nv = len(case["variants"])
    us, vi = [], []
    for v, prep in enumerate(case["preps"]):
        if kind == "random":
            rng = np.random.default_rng(seed + 17 * v + 1)
            u = rng.random(n_random // nv, dtype=F32)
            u[:2] = [0.0, 1.0 - 2.0 ** -24]
        else:
            cap = None if max_rows is None else max(1, max_rows // nv // 33)
            u = boundary_uniforms(prep, case["x"].size, cap)
        us.append(u)
        vi.append(np.full(len(u), v))
    return np.concatenate(us).astype(F32), np.concatenate(vi)
