"""CPU: the binary64 admissible-set reference of the sampler (tests/sampler_ref.py) is sharp enough and not too sharp.

A numpy binary32 emulation of sample_topp_kernel's algorithm, written from the kernel's header comment (csrc/sampler.hip), runs
with two different summation orders: the reference must accept every draw of both.  Ten wrong kernels (the emulation with one
defect each) must each be rejected on at least one case.  The conditions set on the reference itself -- at least 95 %
of random draws decided (one admissible id), no boundary-sweep draw with more than three ids -- are asserted for every case at
every V.  The host form of the draw (chirrup_amd.samplers.sample_inverse_cdf) is held to the same reference."""
import numpy as np
import pytest

import sampler_ref as R

F16, F32, F64 = np.float16, np.float32, np.float64
SMALL_VS = (8, 1000, 1024, 8200)                # every walk form below two load strides; the GPU file runs all of R.VS
MUTANTS = ("gap_fallback", "wave_base", "per_floor", "drop_ties", "topk_off", "temp_first", "norm_target", "zero_drawable",
           "descending", "skip_strides")


# ---------------------------------------------------------------------------------------------------------------------
# the emulation

def _key(x16):
    b = np.ascontiguousarray(x16).view(np.uint16).astype(np.uint32)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


def _exp32(a):
    """binary32 exponential; results below the smallest normal flush to 0 as the hardware instruction's do."""
    with np.errstate(under="ignore", over="ignore"):
        r = np.exp(a.astype(F32)).astype(F32)
    r[r < F32(2.0 ** -126)] = 0
    return r


def _block_sum(q, order, pairs=False):
    """Sum of a per-token binary32 array over the workgroup.  order 0: the kernel's -- lane tid holds the groups of eight
    tid + 1024 it and adds them in (it, element) order (pairs: each two neighbours first, as Z is added; the cutoff's masses are
    added one by one, so mass{all} and Z may differ by an ulp and top_p = 1 may keep everything, -inf logits included), a xor
    butterfly over the wave's 64 lanes, the 16 wave sums in wave order.  order 1: numpy's pairwise sum."""
    if order == 1:
        return F32(np.sum(q, dtype=F32))
    n_it = -(-q.size // R.STRIDE)
    p = np.zeros(n_it * R.STRIDE, F32)
    p[:q.size] = q
    p = p.reshape(n_it, R.LANES, 8)
    z = np.zeros(R.LANES, F32)
    for it in range(n_it):
        for e in range(0, 8, 2 if pairs else 1):
            z = z + ((p[it, :, e] + p[it, :, e + 1]) if pairs else p[it, :, e])
    z = z.reshape(16, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        z = z + z[:, lane ^ o]
    t = F32(0)
    for w in range(16):
        t = t + z[w, 0]
    return t


def emulate(x16, T, top_p, top_k, us, order=0, mutant=None):
    """ids [len(us)] of the kernel's algorithm in binary32 (header comment of sample_topp_kernel): masses exp(x - max) and Z;
    c_key = the largest occurring key whose mass{key >= c_key} reaches top_p Z; k_key = the K-th largest key; kept = key >=
    max(c_key, k_key); weights (m / Z)^(1/T) as one exponential; lane t owns ids [t per, (t + 1) per), per = ceil(V / 1024), and
    adds its kept weights (local); an inclusive scan over the wave, the wave sums in order -> before_t; want = u total; the
    HIGHEST lane with local > 0 and before <= want walks its chunk and takes the first token of positive weight whose running sum
    exceeds want, its last such token when none does; when no lane has weight, the last kept token."""
    x16 = np.asarray(x16, F16)
    V = x16.size
    Tq, Pq, K = F32(F16(T)), F32(F16(top_p)), int(top_k)
    x = x16.astype(F32)
    key = _key(x16)
    mx = x.max()
    invT = F32(1.0) / Tq
    m = _exp32((x - mx) * invT) if mutant == "temp_first" else _exp32(x - mx)
    img = np.ones(V, bool)                                    # the tokens in the register image
    if mutant == "skip_strides":
        img[R.STRIDE:] = False
    Z0 = _block_sum(np.where(img, m, F32(0)), order, pairs=True)
    target = Pq if mutant == "norm_target" else Pq * Z0
    kmax = int(key.max())
    cand = np.unique(key[img])[::-1]                          # occurring keys, descending; mass{key >= k} falls as k grows
    c_key = 0
    lo, hi = 0, len(cand) - 1                                 # the largest key that still holds the target (monotone: bisect)
    mass = lambda k: _block_sum(np.where(img & (key >= k), m, F32(0)), order)
    if mass(cand[hi]) >= target:
        while lo < hi:
            mid = (lo + hi) // 2
            if mass(cand[mid]) >= target:
                hi = mid
            else:
                lo = mid + 1
        c_key = int(cand[lo])
    c_key = min(c_key, kmax)
    k_key = 0
    Ke = K + 1 if (mutant == "topk_off" and K > 0) else K
    if Ke > 0:
        ks = np.sort(key[img])[::-1]
        k_key = int(ks[Ke - 1]) if Ke <= len(ks) else 0
    if mutant == "drop_ties" and c_key > 0:
        kept = key > c_key
        kept[np.nonzero(key == c_key)[0][0]] = True
        kept &= key >= k_key
    else:
        kept = key >= max(c_key, k_key)
    if Tq != 1.0:
        lnZ = F32(np.log(Z0))
        wt = _exp32(((x - mx) - lnZ) * invT)
    else:
        with np.errstate(under="ignore"):
            wt = (_exp32(x - mx) / Z0).astype(F32)
        wt[wt < F32(2.0 ** -126)] = 0
    wt = np.where(kept, wt, F32(0)).astype(F32)

    per = V // R.LANES if mutant == "per_floor" else -(-V // R.LANES)
    chunk = np.zeros((R.LANES, max(per, 1)), F32)
    keptc = np.zeros((R.LANES, max(per, 1)), bool)
    n_cov = min(V, R.LANES * per)
    if per > 0:
        chunk.reshape(-1)[:n_cov] = wt[:n_cov]
        keptc.reshape(-1)[:n_cov] = kept[:n_cov]
    local = np.zeros(R.LANES, F32)
    for j in (range(per) if order == 0 else range(per - 1, -1, -1)):
        local = local + chunk[:, j]
    if order == 0:
        incl = local.reshape(16, 64).copy()
        for o in (1, 2, 4, 8, 16, 32):
            nxt = incl.copy()
            nxt[:, o:] = incl[:, o:] + incl[:, :-o]
            incl = nxt
        red = incl[:, 63]
        base, total = np.zeros(16, F32), F32(0)
        for w in range(16):
            base[w] = total
            total = total + red[w]
        if mutant == "wave_base":
            base = np.concatenate([[F32(0)], base[:-1]]).astype(F32)
        before = ((base[:, None] + incl) - local.reshape(16, 64)).reshape(-1).astype(F32)
    else:
        incl = np.cumsum(local, dtype=F32)
        total = incl[-1]
        before = (incl - local).astype(F32)
    us = np.asarray(us, F32)
    want = (us * total).astype(F32)
    live = keptc.any(1) if mutant == "zero_drawable" else local > 0
    if mutant == "gap_fallback":                               # the parent: a lane claims want inside its own interval only
        elig = live[None, :] & (want[:, None] >= before[None, :]) & (want[:, None] < (before + local)[None, :])
    else:
        elig = live[None, :] & (before[None, :] <= want[:, None])
    winner = np.where(elig.any(1), R.LANES - 1 - np.argmax(elig[:, ::-1], axis=1), -1)
    wl = np.maximum(winner, 0)
    acc, pick, done = before[wl].copy(), np.full(len(us), -1, np.int64), winner < 0
    for j in (range(per - 1, -1, -1) if mutant == "descending" else range(per)):
        wj = chunk[wl, j]
        act = ~done & (keptc[wl, j] if mutant == "zero_drawable" else wj > 0)
        acc = np.where(act, acc + wj, acc).astype(F32)
        pick = np.where(act, wl * per + j, pick)
        done |= act & (acc > want)
    posw = np.nonzero(kept if mutant == "zero_drawable" else wt > 0)[0]
    fallback = int(posw[-1]) if len(posw) else int(np.nonzero(kept)[0][-1])
    return np.where(pick < 0, fallback, pick)


# ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(V, setting, T):
    k = (V, setting, T)
    if k not in _CASES:
        c = R.make_case(V, setting, T)
        cap = 1000 if V > 8200 else None
        c["us"] = {kind: R.uniforms(c, kind, max_rows=cap) for kind in ("random", "boundary")}
        _CASES[k] = c
    return _CASES[k]


def _rejected(case, order, mutant):
    """Number of draws of the emulation that the reference rejects, over both sets of uniforms."""
    bad = n = 0
    for kind in ("random", "boundary"):
        us, vi = case["us"][kind]
        for v, (prep, (T, P, K)) in enumerate(zip(case["preps"], case["variants"])):
            u = us[vi == v]
            ids = emulate(case["x"], T, P, K, u, order, mutant)
            bad += int((~prep.accepts(u, ids)).sum())
            n += len(u)
    return bad, n


@pytest.mark.parametrize("V", R.VS)
def test_reference_decides_almost_every_draw(V):
    """Conditions on the reference alone: >= 95 % of each case's random draws have ONE admissible id; no draw of a boundary sweep
    has more than three (counted as the run of kept order that holds them: contiguous)."""
    for setting in R.SETTINGS:
        for T in R.TS:
            c = _case(V, setting, T)
            for kind in ("random", "boundary"):
                us, vi = c["us"][kind]
                assert len(us) > 0, (c["name"], kind)
                for v, prep in enumerate(c["preps"]):
                    size = prep.sets(us[vi == v])
                    assert size.min() >= 1
                    if kind == "random":
                        assert (size == 1).mean() >= 0.95, (c["name"], v, float((size == 1).mean()))
                    else:
                        assert size.max() <= 3, (c["name"], v, int(size.max()))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("V", SMALL_VS)
def test_both_emulations_are_accepted(V, order):
    for setting in R.SETTINGS:
        for T in R.TS:
            bad, n = _rejected(_case(V, setting, T), order, None)
            assert bad == 0 and n > 0, (V, setting, T, order, bad, n)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_is_rejected(mutant):
    hits = []
    for V in (1000, 1024, 8200):
        for setting in R.SETTINGS:
            for T in R.TS:
                bad, n = _rejected(_case(V, setting, T), 0, mutant)
                if bad:
                    hits.append((V, setting, T, bad, n))
    print(f"{mutant}: rejected on {len(hits)} cases, e.g. {hits[:3]}")
    assert hits, mutant


def test_reference_corners():
    x = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, 0.0, -1.0, 3.0], F16)
    assert R.admissible(x, 1.0, 0.0, 0, 0.0) == {1} and R.admissible(x, 1.0, 0.0, 0, 1 - 2.0 ** -24) == {7}      # top_p 0: the maxima
    assert R.admissible(x, 0.7, 1.0, 1, 0.5) == {2}                                                           # top_k 1, ties kept
    assert R.admissible(x, 1.0, 1.0, 4, 0.0) == {1} and R.admissible(x, 1.0, 1.0, 4, 1 - 2.0 ** -24) == {7}     # {1, 2, 4, 7}
    assert R.admissible(x, 1.0, 1.0, 0, 1 - 2.0 ** -24) == {7}                                                # -inf is never drawn
    p = np.exp(x.astype(F64) - 3.0)
    c = np.cumsum(p) / p.sum()
    assert R.admissible(x, 1.0, 1.0, 0, F32(c[4] * 0.999)) == {4}
    assert R.admissible(x, 1.0, 1.0, 0, F32(c[4])) == {4, 5}                                                   # on a boundary: both


@pytest.mark.parametrize("V", (8, 1000, 1024))
def test_host_inverse_cdf_is_admissible(V):
    """samplers.sample_inverse_cdf (fake backends, V > 65 536) against the same reference: u = 0, 1 - 2^-24, random u and both
    sides of every token boundary.  Its top-k keeps exactly K tokens, so the cases with ties at the K-th value are left out."""
    import torch

    from chirrup_amd.samplers import sample_inverse_cdf

    for setting in R.SETTINGS:
        if setting == "ktie":
            continue
        for T in R.TS:
            c = _case(V, setting, T)
            for prep, (Tv, P, K) in zip(c["preps"], c["variants"]):
                alt = max(prep.alts, key=lambda a_: len(a_["pos"]))
                edges = (alt["C"][:-1] / alt["W"]).astype(F32)
                us = np.concatenate([[0.0, 1 - 2.0 ** -24], np.nextafter(edges, F32(0)), edges, np.nextafter(edges, F32(1)),
                                     np.random.default_rng(V).random(200, dtype=F32)]).astype(F32)
                us = us[(us >= 0) & (us < 1)]
                n = len(us)
                lg = torch.from_numpy(c["x"]).expand(n, V)
                ids = sample_inverse_cdf(lg, torch.full((n, 1), float(F16(Tv))), torch.full((n, 1), float(F16(P))),
                                         torch.full((n, 1), K, dtype=torch.int64), torch.from_numpy(us)).numpy()
                ok = prep.accepts(us, ids)
                assert ok.all(), (c["name"], (Tv, P, K), int((~ok).sum()), us[~ok][:4], ids[~ok][:4])
