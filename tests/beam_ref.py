"""Reference beam search for the tests (DESIGN.md "Beam search"): the contract written out in plain Python / numpy, over explicit
token sequences rather than a trellis, sharing no code with ops.beam_select or the worker.  Also the hand-made candidate tables that
the CPU form and the kernel are both held to."""
import functools
import math

import numpy as np

NEG_INF = np.float32(-np.inf)


def f32_bits(x) -> int:
    return int(np.array([x], np.float32).view(np.int32)[0])


def _cmp(a, b):
    """Total order of candidates (cum, b, k): cum descending, then b ascending, then k ascending."""
    if a[0] > b[0]:
        return -1
    if a[0] < b[0]:
        return 1
    return -1 if (a[1], a[2]) < (b[1], b[2]) else 1


def select(lp, ids, scores, W, stops):
    """One step of one group.  lp / ids: W rows of K = W + len(stops) candidates (logit descending, id ascending); scores: W old
    scores.  Returns {"parent", "rank", "copy_from" (old position or -1), "id", "score"} per new position (None entries where no beam
    was left) and the finished records [(parent, id, cum)]."""
    K = W + len(stops)
    cands = []
    with np.errstate(invalid="ignore"):
        for b in range(W):
            for k in range(K):
                cum = np.float32(scores[b]) + np.float32(lp[b][k])          # one binary32 addition
                cands.append((NEG_INF if np.isnan(cum) else cum, b, k))
    cands.sort(key=functools.cmp_to_key(_cmp))
    chosen, finished = [], []
    for pos, (cum, b, k) in enumerate(cands):
        tok = int(ids[b][k])
        if tok in stops:
            if pos < W and np.isfinite(cum):
                finished.append((b, tok, cum))
            continue
        chosen.append((b, tok, cum))
        if len(chosen) == W:
            break
    survivors = {b for b, _, _ in chosen}
    free = [p for p in range(W) if p not in survivors]                       # dead parents' positions, ascending
    new = [None] * W
    stayed = set()
    for r, (b, tok, cum) in enumerate(chosen):
        if b not in stayed:
            stayed.add(b)
            new[b] = {"parent": b, "rank": r, "copy_from": -1, "id": tok, "score": cum}
        else:
            new[free.pop(0)] = {"parent": b, "rank": r, "copy_from": b, "id": tok, "score": cum}
    return new, finished


def expected_record(lp, ids, scores, W, stops, slots):
    """The int32 output record (ops.BEAM_OUT_WORDS) rwkv7_beam_select writes for a group, its new scores and its ids."""
    new, finished = select(lp, ids, scores, W, stops)
    rec = np.full(65, -1, np.int32)
    rec[32:40] = f32_bits(NEG_INF)
    rec[57:65] = 0
    rec[40] = len(finished)
    for j, (b, tok, cum) in enumerate(finished):
        rec[41 + j], rec[49 + j], rec[57 + j] = b, tok, f32_bits(cum)
    for p, n in enumerate(new):
        if n is not None:
            rec[p], rec[8 + p], rec[24 + p], rec[32 + p] = n["parent"], n["rank"], n["id"], f32_bits(n["score"])
            rec[16 + p] = slots[n["copy_from"]] if n["copy_from"] >= 0 else -1
    return rec, [NEG_INF if n is None else n["score"] for n in new], [None if n is None else n["id"] for n in new]


def rank(hyps, lam, n_best):
    """hyps: dicts with tokens, cum, reason, step, order.  Score cum / max(T, 1) ** lam in binary64; ties: earlier step, lower order."""
    for h in hyps:
        h["score"] = float(h["cum"]) / (float(max(len(h["tokens"]), 1)) ** float(lam))
    return sorted(hyps, key=lambda h: (-h["score"], h["step"], h["order"]))[:n_best]


def search(candidates_of, prompt, W, stops, max_tokens, lam=1.0, n_best=1):
    """candidates_of(tokens) -> (lp [K], ids [K]) of the model after `tokens`.  Returns (hypotheses, ended_by)."""
    stops = set(stops)
    K = W + len(stops)
    beams = [list() for _ in range(W)]
    scores = [np.float32(0.0)] + [NEG_INF] * (W - 1)
    hyps, ended = [], None
    for t in range(1, max_tokens + 1):
        rows = [candidates_of(list(prompt) + beams[p], K) for p in range(W)]
        new, finished = select([r[0] for r in rows], [r[1] for r in rows], scores, W, stops)
        for j, (b, tok, cum) in enumerate(finished):
            hyps.append({"tokens": list(beams[b]), "cum": float(cum), "reason": "stop", "step": t, "order": j})
        beams = [beams[n["parent"]] + [n["id"]] if n is not None else [] for n in new]
        scores = [n["score"] if n is not None else NEG_INF for n in new]
        if t >= max_tokens:
            for p, n in enumerate(new):
                if n is not None and math.isfinite(float(n["score"])):
                    hyps.append({"tokens": list(beams[p]), "cum": float(n["score"]), "reason": "length", "step": t, "order": W + n["rank"]})
            ended = "length" if len([h for h in hyps if h["reason"] == "stop"]) < W else "both"
            break
        if len(hyps) >= W:
            ended = "finished"
            break
    return [{"token_ids": h["tokens"], "cumulative_logprob": h["cum"], "score": h["score"], "finish_reason": h["reason"]}
            for h in rank(hyps, lam, n_best)], ended


def replay(steps, W, stops, max_tokens, lam, n_best):
    """The contract replayed from a worker's per-step candidate tables: steps = [(lp [W][K], ids [W][K])] in step order.  Returns
    (per-step (parents, ids, scores, finished), hypotheses)."""
    stops = set(stops)
    beams = [list() for _ in range(W)]
    scores = [np.float32(0.0)] + [NEG_INF] * (W - 1)
    hyps, trace = [], []
    for t, (lp, ids) in enumerate(steps, start=1):
        new, finished = select(lp, ids, scores, W, stops)
        for j, (b, tok, cum) in enumerate(finished):
            hyps.append({"tokens": list(beams[b]), "cum": float(cum), "reason": "stop", "step": t, "order": j})
        beams = [beams[n["parent"]] + [n["id"]] if n is not None else [] for n in new]
        scores = [n["score"] if n is not None else NEG_INF for n in new]
        trace.append(([n["parent"] for n in new], [n["id"] for n in new], [f32_bits(s) for s in scores],
                      [(b, tok, f32_bits(cum)) for b, tok, cum in finished], [n["copy_from"] for n in new]))
        if t >= max_tokens:
            for p, n in enumerate(new):
                if math.isfinite(float(n["score"])):
                    hyps.append({"tokens": list(beams[p]), "cum": float(n["score"]), "reason": "length", "step": t, "order": W + n["rank"]})
            break
        if len(hyps) >= W:
            break
    return trace, [{"token_ids": h["tokens"], "cumulative_logprob": h["cum"], "score": h["score"], "finish_reason": h["reason"]}
                   for h in rank(hyps, lam, n_best)]


# --------------------------------------------------------------------------------------------------- hand-made tables
def _case(name, W, stops, scores, lp, ids):
    K = W + len(stops)
    lp = np.asarray(lp, np.float32)
    ids = np.asarray(ids, np.int32)
    assert lp.shape == ids.shape == (W, K), (name, lp.shape, K)
    return {"name": name, "W": W, "stops": list(stops), "scores": np.asarray(scores, np.float32), "lp": lp, "ids": ids}


def _ids(W, K, base=10):
    return [[base + 20 * b + k for k in range(K)] for b in range(W)]


def hand_cases():
    inf, nan = float("inf"), float("nan")
    cases = []
    # equal cum in two beams: b, then k, decides
    cases.append(_case("equal_cum", 2, [1], [-1.0, -1.0], [[-0.5, -0.5, -2.0], [-0.5, -0.5, -3.0]], _ids(2, 3)))
    # the first step: only position 0 is alive, so it takes every place (W - 1 copies from one source)
    cases.append(_case("first_step", 3, [1], [0.0, -inf, -inf], [[-0.1, -1.0, -2.0, -3.0]] * 3, _ids(3, 4)))
    # a stop candidate at pos = W - 1 is recorded ...
    ids = _ids(3, 4)
    ids[0][1] = 1
    cases.append(_case("stop_at_W_minus_1", 3, [1], [-0.1, -0.2, -9.0], [[-0.1, -0.6, -5.0, -6.0], [-0.1, -4.0, -5.0, -6.0],
                                                                        [-0.1, -1.0, -2.0, -3.0]], ids))
    # ... and one at pos = W is skipped (two better candidates in front of it now come from beam 1)
    cases.append(_case("stop_at_W", 3, [1], [-0.1, -0.2, -9.0], [[-0.1, -0.6, -5.0, -6.0], [-0.1, -0.2, -5.0, -6.0],
                                                                [-0.1, -1.0, -2.0, -3.0]], ids))
    # a stop candidate that is not finite (its beam is dead) is not recorded, whatever its place
    ids = _ids(2, 4)
    ids[0][0] = ids[1][0] = 2
    cases.append(_case("non_finite_stop", 2, [1, 2], [-inf, -inf], [[-0.1, -1.0, -2.0, -3.0]] * 2, ids))
    # one parent takes all W places: W - 1 copies into the dead parents' positions, ascending
    cases.append(_case("one_parent_takes_all", 4, [1], [-50.0, -50.0, -1.0, -50.0],
                       [[-0.1, -0.2, -0.3, -0.4, -0.5]] * 4, _ids(4, 5)))
    # every parent survives: nothing is copied
    cases.append(_case("all_survive", 3, [1], [-1.0, -1.5, -2.0], [[-0.01, -30.0, -31.0, -32.0]] * 3, _ids(3, 4)))
    # a NaN log-prob orders as -inf
    cases.append(_case("nan_lp", 2, [1], [-1.0, -2.0], [[nan, -0.5, -0.7], [-0.1, nan, -9.0]], _ids(2, 3)))
    # widest: W 8 with 12 stop ids, several finished among the first W
    rng = np.random.default_rng(5)
    lp = -np.sort(rng.random((8, 20)).astype(np.float32) * 4, axis=1)
    ids = np.stack([rng.permutation(40)[:20] for _ in range(8)]).astype(np.int32)
    cases.append(_case("widest", 8, list(range(12)), -rng.random(8).astype(np.float32), lp, ids))
    return cases


def random_case(rng, W, S, V=97):
    """lp from a float32 log-softmax of random binary16 logits (the top K by logit descending, id ascending), with planted ties and
    -inf; some old scores equal, one -inf."""
    K = W + S
    x = rng.integers(-12, 13, (W, V)).astype(np.float16).astype(np.float32) / 2          # many equal logits
    x[rng.integers(0, W), rng.integers(0, V, 5)] = -np.inf
    m = x.max(axis=1, keepdims=True)
    lpr = (x - m) - np.log(np.exp(x - m).sum(axis=1, keepdims=True, dtype=np.float32))
    order = np.argsort(-x, axis=1, kind="stable")[:, :K]
    lp = np.take_along_axis(lpr, order, axis=1).astype(np.float32)
    scores = -(rng.integers(0, 6, W).astype(np.float32)) / 2
    scores[rng.integers(0, W)] = -np.inf
    if not np.isfinite(scores).any():
        scores[0] = 0.0
    if W > 2:
        lp[1] = lp[0]                                                                   # planted ties across beams
        scores[1] = scores[0]
    stops = [int(t) for t in rng.choice(V, S, replace=False)]
    stops[0] = int(order[rng.integers(0, W), 0])                                        # a stop id among the top candidates
    stops = list(dict.fromkeys(stops))
    while len(stops) < S:
        t = int(rng.integers(0, V))
        if t not in stops:
            stops.append(t)
    return _case(f"random_W{W}_S{S}", W, stops, scores, lp, order.astype(np.int32))
