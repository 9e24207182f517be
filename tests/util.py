"""Shared input generators for the parity tests (seeded, no reference access at run time)."""
import numpy as np


def wkv7_inputs(B, T, C, seed=0, n_slots=None, state_scale=0.5, elapsed="arange"):
    """Inputs shaped like what RWKV_x070_TMix_seq_batch hands the kernel (rwkv7.py:625-645):
    a = -kk with kk unit-norm per head, b = kk * sigmoid-range gate, w a pre-activation."""
    rng = np.random.default_rng(seed)
    H = C // 64
    n_slots = B if n_slots is None else n_slots
    f16 = np.float16
    state = (rng.standard_normal((n_slots, H, 64, 64)) * state_scale).astype(f16)
    r = rng.standard_normal((B, T, C)).astype(f16)
    k = rng.standard_normal((B, T, C)).astype(f16)
    v = rng.standard_normal((B, T, C)).astype(f16)
    w = rng.uniform(-8.0, 4.0, (B, T, C)).astype(f16)
    kk = rng.standard_normal((B, T, H, 64)).astype(np.float32)
    kk /= np.linalg.norm(kk, axis=-1, keepdims=True)
    gate = rng.uniform(0.0, 1.0, (B, T, H, 64)).astype(np.float32)
    a = (-kk).reshape(B, T, C).astype(f16)
    b = (kk * gate).reshape(B, T, C).astype(f16)
    if elapsed == "arange":
        et = (np.arange(B) * 7 + 3).astype(np.int32)
    elif elapsed == "big":
        et = rng.integers(0, 2**31 - 1 - T, size=B).astype(np.int32)
    else:
        et = np.zeros(B, np.int32)
    return state, r, w, k, v, a, b, et


def bits(x):
    return np.ascontiguousarray(x).view(np.uint16)


def c768_fixture():
    """(fixture, checkpoint dict) of tests/golden/model_L3_C768.npz: outputs of the REFERENCE's
    forward_seq_batch_seperate (tests/golden/make_golden.py::gen_model_c768) on seed-generated weights that are
    rebuilt here and proven identical through the stored sha256."""
    import hashlib
    import os

    from chirrup_amd.synth import make_state_dict

    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_L3_C768.npz"))
    L, C, V, B, seed = (int(v) for v in d["config"])
    zd = make_state_dict(L, C, V, seed=seed, varied_norms=True)
    h = hashlib.sha256()
    for k in sorted(zd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(zd[k].numpy()).tobytes())
    assert h.hexdigest() == d["weights_sha256"].tobytes().decode(), "synthetic weights differ from the fixture's (torch RNG changed?)"
    return d, zd


def c768_inputs(d, tag):
    """The seeded inputs of case `tag` (state tensors are regenerated, not stored)."""
    L, C, V, B, _ = (int(v) for v in d["config"])
    rng = np.random.default_rng(int(d[f"{tag}:seed"][0]))
    s0 = (rng.standard_normal((L, 2, B, C)) * 0.5).astype(np.float16)
    s1 = (rng.standard_normal((L, B, C // 64, 64, 64)) * 0.1).astype(np.float16)
    s2 = (np.arange(B) * 7 + 3).astype(np.int32)
    toks = rng.integers(1, V, size=d[f"{tag}:tokens"].shape).tolist()
    assert toks == d[f"{tag}:tokens"].tolist()
    return toks, [s0, s1, s2]


def parity_stats(got, want):
    """The error figures the parity bars are written in: absolute L-inf, L-inf relative to max(1, max|want|) (the bar form of
    DESIGN.md section 2), max|want|, and the absolute error in units in the last place of binary16 at the tensor's TOP binade."""
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    d = float(np.abs(g - w).max()) if w.size else 0.0
    m = float(np.abs(w).max()) if w.size else 0.0
    top_ulp = float(2.0 ** (np.floor(np.log2(max(m, 2.0 ** -14))) - 10))
    return {"abs_linf": d, "rel_linf": d / max(1.0, m), "max_abs_want": m, "top_binade_ulps": d / top_ulp}


def record_parity(case, **fields):
    """Append one measured-error record to the parity log (JSON lines; gpurun_out/parity/r04_parity_errors.jsonl, or
    $CHIRRUP_PARITY_LOG): VERDICT r3 item 2 -- every bar of the fixture / full-size / smoke tests sits beside the error that was
    measured against it; tools/parity_report.py turns the log into profiles/r04_parity_errors.txt."""
    import json
    import os

    path = os.environ.get("CHIRRUP_PARITY_LOG") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                "gpurun_out", "parity", "r04_parity_errors.jsonl")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, **fields}, sort_keys=True) + "\n")
    except OSError:
        pass


_BARS = None


def tight_bar(case, name, ceiling):
    """The bar a measurement is held to: tests/golden/parity_bars.json holds, per (case, tensor), 1.25 x the error measured on an
    MI355X with this round's kernels (written by `python tools/parity_report.py --write-bars` from the log of a full -m gpu run;
    the same log is committed as profiles/r04_parity_errors.txt) -- never above `ceiling`, the bar the test's own argument gives
    (north_star's 1e-3, a noise floor of two CPU evaluations, ...).  VERDICT r3 item 2: every bar <= 1.25 x its measurement."""
    global _BARS
    if _BARS is None:
        import json
        import os

        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parity_bars.json")
        _BARS = json.load(open(path)) if os.path.exists(path) else {}
    b = _BARS.get(f"{case}|{name}")
    return ceiling if b is None else min(ceiling, b)


def check_bar(case, name, stats, bar, key="rel_linf"):
    """Record (measurement, bar) and assert measurement <= bar (bar = tight_bar(...): 1.25 x the committed measurement, at most `bar`)."""
    bar = tight_bar(case, name, bar)
    record_parity(case, tensor=name, bar=bar, bar_on=key, **stats)
    assert stats[key] <= bar, (case, name, key, stats[key], bar)


# ----------------------------------------------------------------------------------------------------------------------------
# Host replay of the reference worker's decode step (chirrup/worker.py:720-728 and :527-547), which the worker end-to-end tests
# hold the real kernels to.

NO_PENALTY_IDS = frozenset({10, 33, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58})     # occurrence is not incremented for these ids


def kept_sets(prob, top_p, top_k):
    """The kept sets of the reference's top-p / top-k rule for one row of probabilities (float32, CPU;
    chirrup/utils/samplers.py:171-255): cutoff by value at the first index where the descending cumulative sum reaches
    fp16(top_p), ties at the cutoff kept; then top-k, ties at the k-th value kept.  A kernel adds the same masses in another
    order, so where the cumulative sum crosses top_p within 1e-5 the crossing may fall one token either way: one bool mask per
    admissible crossing index, the exact crossing first."""
    import torch

    V = prob.numel()
    sp, _ = torch.sort(prob, descending=True)
    cs = torch.cumsum(sp, 0)
    tpv = float(torch.tensor(top_p).half())
    j = min(int(torch.searchsorted(cs, torch.tensor(tpv))), V - 1)
    near = [j] + [jj for jj in (j - 1, j + 1) if 0 <= jj < V and min(abs(float(cs[max(jj, j) - 1]) - tpv), abs(float(cs[min(jj, j)]) - tpv)) < 1e-5]
    sets = []
    for jj in near:
        keep = prob >= sp[jj]
        if top_k > 0:
            keep &= prob >= sp[top_k - 1]
        sets.append(keep)
    return sets


def replay_decode(raw_logits, emitted, frequency_penalty, presence_penalty, penalty_decay, forbidden_tokens=(),
                  no_penalty_ids=NO_PENALTY_IDS, greedy=True):
    """Replays one request's decode steps on the host from the raw fp16 logits of each step (Task(return_logits=True): the
    model output before any edit) and the ids it emitted.  Per step:
      1. forbidden ids -> -inf (what `fp16 -= 1e10` gives);
      2. occurrence *= decay (fp32 * fp16 -> fp32);
      3. logits = fp16(float(logits) - (alpha + occurrence * freq))   (oracle.rwkv7_np.apply_penalties);
      4. greedy rows: the arg-max, lowest id on ties;
      5. with the emitted id: occurrence[id] += 0 for the no-penalty ids else 1, alpha[id] = presence.
    Returns (ids, penalised): the replay's greedy id per step (None for sampled rows) and the penalised fp16 logits per step
    (what a sampled row draws from)."""
    from oracle import rwkv7_np as M

    f16, f32 = np.float16, np.float32
    V = len(raw_logits[0])
    occ, alpha = np.zeros(V, f32), np.zeros(V, f32)
    decay, freq, pres = f16(penalty_decay), f16(frequency_penalty), f32(presence_penalty)
    forbidden = sorted(set(int(t) for t in forbidden_tokens))
    ids, penalised = [], []
    for raw, tok in zip(raw_logits, emitted):
        lg = np.array(raw, dtype=f16).reshape(V)
        if forbidden:
            with np.errstate(over="ignore"):
                lg[forbidden] = (lg[forbidden].astype(f32) - f32(1e10)).astype(f16)
        lg, occ = M.apply_penalties(lg, occ, alpha, decay, freq)
        penalised.append(lg)
        ids.append(int(M.greedy_sample(lg)) if greedy else None)
        tok = int(tok)
        occ[tok] += f32(0.0 if tok in no_penalty_ids else 1.0)
        alpha[tok] = pres
    return ids, penalised


def check_sampled_step(penalised, tok, top_p, top_k, forbidden_tokens=()):
    """A sampled row's id at one step: not forbidden, a finite penalised logit, inside one of the kept sets of the penalised
    logits (kept_sets).  Returns a description of the failure, or None."""
    import torch

    tok = int(tok)
    if tok in set(int(t) for t in forbidden_tokens):
        return f"forbidden id {tok}"
    if not 0 <= tok < len(penalised) or not np.isfinite(float(penalised[tok])):
        return f"id {tok} has no finite logit"
    prob = torch.softmax(torch.from_numpy(penalised.astype(np.float32)), -1)
    if not any(bool(k[tok]) for k in kept_sets(prob, top_p, top_k)):
        return f"id {tok} is outside the kept set (top_p {top_p}, top_k {top_k})"
    return None
