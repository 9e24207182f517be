"""GPU: per-request seeds and logit_bias.  The two kernels (rwkv7_seeded_uniform, rwkv7_apply_logit_bias) bit for bit against
their CPU forms; then the real Worker on the L2/C128 golden model (V = 320) and the 0.1B synthetic model (V = 65 536), graph and
eager, run-ahead and in-step: seeded sampled ids against a host replay that draws with the Philox uniforms, determinism across
slots and neighbours, bias on greedy rows, logprobs that stay those of the raw output, and slot reuse."""
import queue

import numpy as np
import pytest
import torch

from chirrup_amd import ops
from oracle import rwkv7_np as M
from test_decode_sampling_gpu import _model, _Sink, _Tok
from util import kept_sets, replay_decode

pytestmark = pytest.mark.gpu
MODELS = ["L2C128", "0.1B"]
VOCAB = {"L2C128": 320, "0.1B": 65536}


# ------------------------------------------------------------------------------------------------------------ the kernels
def _seed_tables(S, rng):
    seeds = torch.from_numpy(rng.integers(-(1 << 63), (1 << 63) - 1, S, dtype=np.int64))
    seeds[:4] = torch.tensor([0, -1, -(1 << 63), (1 << 63) - 1])
    seeded = torch.from_numpy((rng.random(S) < 0.7).astype(np.int32))
    counters = torch.from_numpy(rng.integers(-(1 << 31), (1 << 31) - 1, S, dtype=np.int64).astype(np.int32))
    counters[:3] = torch.tensor([0, -1, 2 ** 31 - 1], dtype=torch.int32)           # 0, 0xffffffff (wraps), 0x7fffffff
    return seeds, seeded, counters


def test_seeded_uniform_kernel_matches_host_form():
    rng = np.random.default_rng(5)
    for S, B, n in ((16, 12, 9), (257, 256, 256), (300, 200, 1), (8, 8, 0)):
        seeds, seeded, counters = _seed_tables(S, rng)
        slot_idx = torch.from_numpy(rng.permutation(S)[:B].astype(np.int32))
        rows = torch.from_numpy(rng.permutation(B)[:n].astype(np.int32))
        u = torch.from_numpy(rng.random(n).astype(np.float32))
        h = [t.clone() for t in (seeds, seeded, counters, u)]
        d = [t.cuda() for t in (seeds, seeded, counters, u)]
        for _ in range(3):                                                          # the counters advance from launch to launch
            ops.seeded_uniform(rows, slot_idx, h[0], h[1], h[2], h[3])
            ops.seeded_uniform(rows.cuda(), slot_idx.cuda(), d[0], d[1], d[2], d[3])
            torch.cuda.synchronize()
            assert np.array_equal(d[3].cpu().numpy().view(np.uint32), h[3].numpy().view(np.uint32)), (S, B, n)
            assert torch.equal(d[2].cpu(), h[2]), (S, B, n)
        sl = slot_idx[rows.long()].long() if n else torch.zeros(0, dtype=torch.long)
        unseeded = seeded[sl] == 0
        assert torch.equal(d[3].cpu()[unseeded], u[unseeded])                     # untouched
        moved = torch.zeros(S, dtype=torch.bool)
        moved[sl[~unseeded]] = True
        assert torch.equal(d[2].cpu()[~moved], counters[~moved])
        assert torch.equal(d[2].cpu()[moved].long() & 0xFFFFFFFF, (counters[moved].long() + 3) & 0xFFFFFFFF)


def _bias_case(n, V, cap, rng):
    S = n + 3
    lg = (rng.standard_normal((n, V)) * 4).astype(np.float16)
    lg[:, 0], lg[:, 1], lg[:, 2], lg[:, 3] = 65504, -65504, -np.inf, 65440
    counts = rng.integers(0, cap + 1, S).astype(np.int32)
    counts[:3] = [cap, 0, 1]
    ids = np.zeros((S, cap), np.int32)
    vals = rng.uniform(-100, 100, (S, cap)).astype(np.float32)
    vals[:, :4] = [100, -100, 100, 100]
    others = np.concatenate([np.arange(-20, 0), np.arange(4, V + 20)])           # some < 0 and some >= V: skipped
    for s in range(S):
        ids[s] = np.concatenate([[0, 1, 2, 3], rng.choice(others, cap - 4, replace=False)])
    slot_idx = rng.permutation(S)[:n].astype(np.int32)
    slot_idx[:min(n, 3)] = [0, 1, 2][:min(n, 3)]
    return [torch.from_numpy(x) for x in (lg, slot_idx, counts, ids, vals)]


@pytest.mark.parametrize("V,cap", [(65536, 1024), (320, 64), (50304, 7), (65536, 3000)])
def test_apply_logit_bias_kernel_matches_host_form(V, cap):
    rng = np.random.default_rng(V + cap)
    for n in (200, 3, 0):
        lg, slot_idx, counts, ids, vals = _bias_case(n, V, cap, rng)
        h = lg.clone()
        ops.apply_logit_bias(h, slot_idx, counts, ids, vals)
        d = lg.cuda()
        ops.apply_logit_bias(d, slot_idx.cuda(), counts.cuda(), ids.cuda(), vals.cuda())
        torch.cuda.synchronize()
        got = d.cpu()
        assert np.array_equal(got.numpy().view(np.uint16), h.numpy().view(np.uint16)), (V, cap, n)
        if n:
            assert got[0, 0].item() == 65504 and got[0, 1].item() == -65504 and got[0, 2].item() == float("-inf")
            assert torch.equal(got[1], lg[1])                                        # an empty list: the row is untouched
            assert bool(torch.isfinite(got[lg.isfinite()]).all())
        if n:                                                                       # without slot_idx: row i uses slot i
            d2, h2 = lg.cuda(), lg.clone()
            ops.apply_logit_bias(d2, None, counts.cuda(), ids.cuda(), vals.cuda())
            ops.apply_logit_bias(h2, None, counts, ids, vals)
            assert np.array_equal(d2.cpu().numpy().view(np.uint16), h2.numpy().view(np.uint16))


# ------------------------------------------------------------------------------------------------------------ the worker
def _run(m, V, specs, run_ahead, use_graph, batch_size=5, admit_all=False, torch_seed=77):
    """specs: (prompt, Task kwargs).  Returns per request (ids, raw logits per step, logprob entries)."""
    from chirrup_amd.core_structure import ModelLoadConfig, Task
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=batch_size, model=m, tokenizer=_Tok(), run_ahead=run_ahead)
    w._init_worker()
    assert w.use_graph
    w.use_graph = use_graph
    if admit_all:
        w.max_prefill_count = batch_size
    tasks = [Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(p), state=None,
                  stop_tokens=[], return_logits=True, **kw) for p, kw in specs]
    torch.manual_seed(torch_seed)
    for t in tasks:
        tq.put(t)
    for it in range(4000):
        if not w.step():
            break
    out = []
    for t in tasks:
        items = [p for k, p in t.output_queue.items if k == "token_generated"]
        assert t.output_queue.items[-1][0] == "task_completed" and len(items) == t.max_tokens
        out.append(([p[0] for p in items], [p[2].numpy() for p in items], [p[3] if len(p) > 3 else None for p in items]))
    return out


def _biased(lg, bias):
    lg = lg.copy()
    V = len(lg)
    for t, b in bias.items():
        if 0 <= t < V and np.isfinite(np.float32(lg[t])):
            lg[t] = np.float16(np.clip(np.float32(lg[t]) + np.float32(b), -65504, 65504))
    return lg


def replay_seeded(raw_logits, emitted, kw):
    """Host replay of a seeded sampled request: raw -> forbidden (-inf) -> bias -> penalties -> kept set -> inverse-CDF draw in
    float64 with the request's Philox uniform.  Returns per step (host id, doubtful): doubtful when the kept set is ambiguous
    (kept_sets) or u * total lies within 1e-5 (relative) of an edge of the drawn token's interval."""
    f16, f32 = np.float16, np.float32
    V = len(raw_logits[0])
    occ, alpha = np.zeros(V, f32), np.zeros(V, f32)
    T = float(f16(kw.get("temperature")))
    forbidden = sorted(set(kw.get("forbidden_tokens", ())))
    out = []
    for k, (raw, tok) in enumerate(zip(raw_logits, emitted)):
        lg = np.array(raw, dtype=f16).reshape(V)
        if forbidden:
            with np.errstate(over="ignore"):
                lg[forbidden] = (lg[forbidden].astype(f32) - f32(1e10)).astype(f16)
        lg = _biased(lg, kw.get("logit_bias", {}))
        lg, occ = M.apply_penalties(lg, occ, alpha, f16(kw["penalty_decay"]), f16(kw["frequency_penalty"]))
        sets = kept_sets(torch.softmax(torch.from_numpy(lg.astype(f32)), -1), kw["top_p"], kw.get("top_k", 0))
        x = lg.astype(np.float64)
        p = np.exp(x - x.max())
        p /= p.sum()
        u = float(ops.philox_uniform(kw["seed"], k))
        picks, doubtful = [], False
        for keep in sets:
            wgt = np.where(keep.numpy(), p ** (1.0 / T), 0.0)
            cum = np.cumsum(wgt)
            want = u * cum[-1]
            i = int(np.searchsorted(cum, want, side="right"))
            i = i if i < V else int(np.nonzero(wgt > 0)[0][-1])
            lo = cum[i - 1] if i > 0 else 0.0
            doubtful |= min(abs(want - lo), abs(cum[i] - want)) <= 1e-5 * cum[-1]
            picks.append(i)
        out.append((picks[0], doubtful or len(set(picks)) > 1))
        tok = int(tok)
        occ[tok] += f32(0.0 if tok in {10, 33, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58} else 1.0)
        alpha[tok] = f32(kw["presence_penalty"])
    return out


def _specs(V, rng):
    """Seeded sampled rows with penalties, forbidden tokens and biases, an unseeded neighbour, a biased greedy row, a reused slot.
    The 0.1B synthetic model's logits have a standard deviation of about 1 over 65 536 ids: at T >= 0.5 the kept weights are
    nearly uniform, every token's interval is ~1.5e-5 of the total, and the 1e-5 edge tolerance would cover most draws.  Its
    seeded rows therefore run at T 0.2-0.3 or top_k 20, where the replay decides almost every step."""
    P = lambda n: rng.integers(1, V, n).tolist()
    z = dict(frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0)
    T = (lambda small, big: big) if V <= 1024 else (lambda small, big: small)
    return [
        (P(5), dict(temperature=T(0.2, 1.0), top_p=1.0, top_k=0, seed=1, max_tokens=40, **z)),
        (P(3), dict(temperature=T(0.25, 0.7), top_p=0.9, top_k=0, seed=-2, max_tokens=36, frequency_penalty=0.5, presence_penalty=0.5,
                    penalty_decay=0.996)),
        (P(12), dict(temperature=1.5, top_p=1.0, top_k=20, seed=(1 << 64) - 3, max_tokens=44, frequency_penalty=0.3,
                     presence_penalty=0.2, penalty_decay=0.95, forbidden_tokens=[0, 5], logit_bias={7: 3.0, 8: -2.0, 9: 4.0})),
        (P(7), dict(temperature=1.0, top_p=0.3, top_k=0, max_tokens=30, **z)),                       # unseeded neighbour
        (P(2), dict(temperature=0.0, top_p=0.0, top_k=0, max_tokens=32, logit_bias={11: 2.0}, **z)),  # greedy, biased
        (P(9), dict(temperature=T(0.2, 1.2), top_p=0.95, top_k=0, seed=12345, max_tokens=40, logit_bias={int(t): float(b) for t, b in
                    zip(rng.permutation(V)[:64], rng.uniform(-5, 5, 64))}, **z)),
        (P(4), dict(temperature=T(0.3, 0.9), top_p=1.0, top_k=0, seed=1, max_tokens=38, frequency_penalty=1.0, presence_penalty=0.0,
                    penalty_decay=0.9)),                                                                 # a reused slot
    ]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
@pytest.mark.parametrize("model", MODELS)
def test_seeded_sampled_ids_equal_the_host_replay(model, run_ahead, use_graph):
    V = VOCAB[model]
    m = _model(model)
    specs = _specs(V, np.random.default_rng(V))
    runs = _run(m, V, specs, run_ahead, use_graph)
    steps = doubtful = differ = 0
    for i, ((_, kw), (ids, raw, _)) in enumerate(zip(specs, runs)):
        if kw["temperature"] == 0:                  # greedy + bias: the replay of the decode-step rule on the biased logits
            want, _ = replay_decode([_biased(np.array(r, np.float16), kw["logit_bias"]) for r in raw], ids, 0.0, 0.0, 1.0)
            assert ids == want, i
            continue
        if kw.get("seed") is None:
            continue
        for k, ((host, doubt), tok) in enumerate(zip(replay_seeded(raw, ids, kw), ids)):
            steps += 1
            doubtful += doubt
            differ += tok != host
            assert tok == host or doubt, (i, k, tok, host)
            assert tok not in kw.get("forbidden_tokens", ()), (i, k)
    print(f"{model}: {steps} seeded steps, {doubtful} doubtful, {differ} differ from the replay")
    assert steps >= 150 and doubtful <= steps // 10, (steps, doubtful, differ)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("model", MODELS)
def test_seeded_request_is_identical_at_another_slot_beside_other_requests(model, use_graph):
    """The same width at every step (equal prompt lengths and max_tokens, all admitted at once), a different slot, different
    neighbours: identical raw logits and ids.  Another seed gives another sequence."""
    V = VOCAB[model]
    m = _model(model)
    rng = np.random.default_rng(3)
    P = lambda: rng.integers(1, V, 6).tolist()
    z = dict(frequency_penalty=0.2, presence_penalty=0.1, penalty_decay=0.99, max_tokens=32)
    R = (P(), dict(temperature=1.0, top_p=0.95, top_k=0, seed=-777, logit_bias={3: 1.5}, **z))
    a = _run(m, V, [R, (P(), dict(temperature=0.8, top_p=0.5, top_k=0, **z)), (P(), dict(temperature=0.0, top_p=0.0, top_k=0, **z))],
             True, use_graph, admit_all=True)
    b = _run(m, V, [(P(), dict(temperature=1.3, top_p=1.0, top_k=5, seed=9, **z)), (P(), dict(temperature=0.0, top_p=0.0, top_k=0, **z)), R],
             True, use_graph, admit_all=True, torch_seed=5)
    assert a[0][0] == b[2][0]
    assert all(np.array_equal(x.view(np.uint16), y.view(np.uint16)) for x, y in zip(a[0][1], b[2][1]))
    other = _run(m, V, [(R[0], dict(R[1], seed=-776))], True, use_graph)
    assert other[0][0] != a[0][0]


@pytest.mark.parametrize("model", MODELS)
def test_bias_on_greedy_rows_and_logprobs_of_the_raw_output(model):
    V = VOCAB[model]
    m = _model(model)
    rng = np.random.default_rng(11)
    prompt = rng.integers(1, V, 5).tolist()
    g = dict(temperature=0.0, top_p=0.0, top_k=0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, max_tokens=24,
             logprobs=True, top_logprobs=5)
    alone = _run(m, V, [(prompt, g)], True, True)[0]
    first = alone[0][0]
    target = next(t for t in (17, 18, 19) if t not in alone[0])
    rest = [(prompt, dict(g, logit_bias={target: 100.0})), (prompt, dict(g, logit_bias={first: -100.0}))]
    plain, up, down = _run(m, V, [(prompt, g)] + rest, True, True)
    never = next(i for e in plain[2] for i, _ in e["top_logprobs"] if i not in plain[0])   # a runner-up never emitted
    side = _run(m, V, [(prompt, dict(g, logit_bias={never: -100.0}))] + rest, True, True)[0]   # the same width and neighbours
    assert up[0] == [target] * 24
    assert first not in down[0]
    assert side[0] == plain[0] and side[2] == plain[2]                     # a bias that changes no id changes no logprob
    for raw, tok, e in zip(up[1], up[0], up[2]):                            # the +100 row: logprobs of the raw output
        lp, ids = ops.token_logprobs(torch.from_numpy(raw).view(1, -1).cuda(), 5,
                                     targets=torch.tensor([tok], dtype=torch.int32, device="cuda"))
        assert e["logprob"] == lp[0, 0].item() < -1e-3
        assert e["top_logprobs"] == list(zip(ids[0].tolist(), lp[0, 1:].tolist()))


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("model", MODELS)
def test_slot_reuse_after_a_biased_and_a_seeded_request(model, use_graph):
    """One decode slot: a biased greedy request, then an unbiased one (matches an unbiased replay); a seeded request, then the
    same again (its counter restarted: the same ids)."""
    V = VOCAB[model]
    m = _model(model)
    rng = np.random.default_rng(21)
    p = rng.integers(1, V, 4).tolist()
    g = dict(temperature=0.0, top_p=0.0, top_k=0, frequency_penalty=0.4, presence_penalty=0.3, penalty_decay=0.98, max_tokens=20)
    s = dict(temperature=1.0, top_p=1.0, top_k=0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, max_tokens=20, seed=4)
    for run_ahead in (True, False):
        out = _run(m, V, [(p, dict(g, logit_bias={13: 100.0, 14: -5.0})), (p, g), (p, s), (p, s)], run_ahead, use_graph, batch_size=2)
        assert out[0][0] == [13] * 20
        want, _ = replay_decode(out[1][1], out[1][0], g["frequency_penalty"], g["presence_penalty"], g["penalty_decay"])
        assert out[1][0] == want
        assert out[2][0] == out[3][0]
