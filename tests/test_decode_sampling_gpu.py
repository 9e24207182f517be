"""GPU: the worker's penalised and sampled decode end to end against a host replay of the reference's decode-step rule
(util.replay_decode), and the edges of sample_topp's inverse-CDF draw.

The kernels of the decode step are pinned one by one elsewhere (test_worker_gpu.py); here they run together inside the real
Worker over many steps, with the state they keep on the device between steps: the occurrence / presence tables, the per-slot
id lists of ops.PenaltyLists and their dense fall-back, run-ahead steps in flight while a slot is handed to a new request."""
import os
import queue
import types

import numpy as np
import pytest
import torch

from util import check_sampled_step, replay_decode

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _Tok:
    def decode(self, ids, utf8_errors="strict"):
        return "".join(chr(65 + i % 26) for i in ids)


class _Sink:
    def __init__(self):
        self.items = []

    def put_nowait(self, x):
        self.items.append(x)


_MODELS = {}


def _model(name):
    """L2/C128: the golden tiny model (V = 320: holds the no-penalty ids); 0.1B: the synthetic 12 x 768 stack at V = 65 536."""
    if name not in _MODELS:
        from chirrup_amd.rwkv7 import RWKV_x070, model_args
        from chirrup_amd.synth import CONFIGS, make_state_dict

        if name == "L2C128":
            d = np.load(os.path.join(G, "model_L2_C128.npz"))
            zd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")}
            _MODELS[name] = RWKV_x070(types.SimpleNamespace(vocab_size=320, head_size=64, MODEL_NAME="unused"), state_dict=zd,
                                      device="cuda:0")
        else:
            L, C = CONFIGS["0.1B"]
            dev = torch.device("cuda", 0)
            _MODELS[name] = RWKV_x070(model_args("synthetic"), state_dict=make_state_dict(L, C, 65536, seed=3, device=dev), device=dev)
    return _MODELS[name]


def _free_run(m, prompt, n, state=None):
    """Greedy ids of `prompt` decoded alone without penalties (the streams the penalties must move away from)."""
    st = [t.clone() for t in state] if state is not None else m.generate_zero_state(1)
    lg = m.forward_seq_batch_seperate([list(prompt)], st)
    out = []
    for _ in range(n):
        out.append(int(lg[0].float().argmax()))
        lg = m.forward_seq_batch_seperate([[out[-1]]], st)
    return out


def _requests(m, V):
    """(prompt, Task kwargs, prefix state or None) of a mixed load: greedy rows with assorted penalties (decay < 1, presence
    alone), greedy rows with forbidden tokens (id 0 and the row's free-running arg-maxes), an unpenalised twin of two of them,
    sampled rows at T 0.7 / 1.0 / 1.5, top_p 0.3 / 0.9 / 1.0, top_k 0 / 20 with and without penalties, and a row that starts
    from a prefix state."""
    rng = np.random.default_rng(V)
    P = lambda n: rng.integers(1, V, n).tolist()
    g = dict(temperature=0.0, top_p=0.0, top_k=0)
    reqs = []
    p_a, p_b, p_c = P(5), P(17), P(3)
    # a negative presence penalty pulls the emitted ids back (the stream must leave its unpenalised twin's) and the choice among
    # them turns on the frequency term: small differences in decay / occurrence flip ids
    reqs.append((p_a, dict(g, frequency_penalty=1.0, presence_penalty=-8.0, penalty_decay=0.7, max_tokens=56), None))
    reqs.append((p_b, dict(g, frequency_penalty=1.0, presence_penalty=0.0, penalty_decay=0.9, max_tokens=48), None))
    reqs.append((p_a, dict(g, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, max_tokens=56), None))     # twin of 0
    reqs.append((P(1), dict(g, frequency_penalty=0.0, presence_penalty=0.8, penalty_decay=1.0, max_tokens=44), None))
    free = _free_run(m, p_c, 3)
    reqs.append((p_c, dict(g, frequency_penalty=0.3, presence_penalty=0.3, penalty_decay=0.98, max_tokens=60,
                           forbidden_tokens=[0] + free), None))
    reqs.append((p_b, dict(g, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, max_tokens=48), None))     # twin of 1
    reqs.append((P(9), dict(temperature=0.7, top_p=0.3, top_k=0, frequency_penalty=0.5, presence_penalty=0.5, penalty_decay=0.996,
                            max_tokens=52), None))
    reqs.append((P(2), dict(temperature=1.0, top_p=0.9, top_k=20, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0,
                            max_tokens=40), None))
    p_f = P(12)
    reqs.append((p_f, dict(temperature=1.5, top_p=1.0, top_k=0, frequency_penalty=0.4, presence_penalty=0.2, penalty_decay=0.95,
                           max_tokens=48, forbidden_tokens=[0] + _free_run(m, p_f, 2)), None))
    reqs.append((P(4), dict(temperature=1.0, top_p=1.0, top_k=20, frequency_penalty=0.0, presence_penalty=1.0, penalty_decay=1.0,
                            max_tokens=44), None))
    prefix, rest = P(24), P(6)
    st = m.generate_zero_state(1)
    m.forward_seq_batch_seperate([prefix], st)
    reqs.append((rest, dict(g, frequency_penalty=0.6, presence_penalty=0.4, penalty_decay=0.97, max_tokens=64), st))
    reqs.append((P(30), dict(temperature=0.7, top_p=0.9, top_k=0, frequency_penalty=0.8, presence_penalty=0.0, penalty_decay=0.99,
                             max_tokens=50, forbidden_tokens=[0, 1, 2]), None))
    reqs.append((P(7), dict(g, frequency_penalty=0.5, presence_penalty=0.5, penalty_decay=0.996, max_tokens=48), None))
    reqs.append((P(11), dict(g, frequency_penalty=2.0, presence_penalty=-4.0, penalty_decay=0.5, max_tokens=60), None))   # a reused slot
    return reqs


def _run(m, V, reqs, mode, run_ahead, use_graph, return_logits=True, seed=1234):
    """All requests through one fresh Worker (4 decode slots, staggered arrivals); the penalty tables in `mode`: "lists" (the
    default PenaltyLists, cap 4096), "cap8" (PenaltyLists of cap 8: rows cross into the dense pass mid-stream), "dense" (no
    lists).  Returns per request the emitted ids and, with return_logits, the raw logits of every step."""
    from chirrup_amd import ops
    from chirrup_amd.core_structure import ModelLoadConfig, Task
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V, head_size=64)
    tq, mq = queue.Queue(), queue.Queue()
    w = Worker("w0", [0], cfg, tq, mq, None, batch_size=5, model=m, tokenizer=_Tok(), run_ahead=run_ahead)
    w._init_worker()
    assert w.use_graph, "the HIP path (graph capable) is expected"
    w.use_graph = use_graph
    assert w._pen_lists is not None and w._pen_lists.cap == 4096
    if mode == "cap8":
        w._pen_lists = ops.PenaltyLists(w.real_state_size, V, w.device, cap=8)
    elif mode == "dense":
        w._pen_lists = None
    tasks = [Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(p), state=st,
                  stop_tokens=[], return_logits=return_logits, **kw) for p, kw, st in reqs]
    last_in_slot = {}
    install = w._install

    def _install(task, slot):                            # which request each slot served last
        last_in_slot[slot] = task
        install(task, slot)

    w._install = _install
    torch.manual_seed(seed)
    pending = list(tasks)
    for _ in range(3):
        tq.put(pending.pop(0))
    it = 0
    while True:
        if pending and it % 6 == 5:                      # one arrival every 6 iterations: slots are handed over mid-stream
            tq.put(pending.pop(0))
        busy = w.step()
        it += 1
        if not busy and not pending:
            break
        assert it < 4000
    out = []
    for t in tasks:
        items = [p for k, p in t.output_queue.items if k == "token_generated"]
        assert t.output_queue.items[-1][0] == "task_completed" and len(items) == t.max_tokens
        out.append(([p[0] for p in items], [p[2].numpy() for p in items] if return_logits else None))
    if mode != "dense":
        # the id lists left behind by each slot's last request hold exactly the ids it committed: the ids it emitted and, one
        # step ahead, the id its last speculative row sampled (last_ids); the bitmap marks the same ids.  A reset that missed
        # the count or the bitmap leaves the previous request's ids here.
        lists, last = w._pen_lists, w.last_ids.cpu().tolist()
        count, listed, bitmap = lists.count.cpu().tolist(), lists.ids.cpu().numpy(), lists.bits.cpu().numpy().view(np.uint32)
        for slot, t in last_in_slot.items():
            emitted = set(t.generated_tokens)
            extra = {last[slot]} if run_ahead else set()
            bits = {i for i in range(V) if (int(bitmap[slot, i >> 5]) >> (i & 31)) & 1}
            assert emitted <= bits <= emitted | extra, (slot, mode)
            if len(bits) > lists.cap:
                assert count[slot] == -1, (slot, mode)
            else:
                assert count[slot] == len(bits) and set(listed[slot, :count[slot]].tolist()) == bits, (slot, mode)
        if mode == "cap8":                               # the small cap really was exceeded (dense fall-back) by some slot
            assert -1 in count
    return out


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
@pytest.mark.parametrize("model", ["L2C128", "0.1B"])
def test_worker_penalised_and_sampled_decode_matches_host_replay(model, run_ahead, use_graph):
    """Every greedy id equals the host replay's (forbidden -> -inf, occurrence decay, penalty subtraction, arg-max, commit) at
    every step, exactly: the replay starts from the very logits the kernel saw.  Every sampled id is inside the kept set of
    the host-penalised logits and never forbidden.  The three penalty-table modes emit identical ids for every request (the
    same torch.rand calls), and a request's ids do not change when it stops asking for return_logits (the serving path)."""
    m = _model(model)
    V = 320 if model == "L2C128" else 65536
    reqs = _requests(m, V)
    runs = {mode: _run(m, V, reqs, mode, run_ahead, use_graph) for mode in ("lists", "cap8", "dense")}
    for i, ((_, kw, _), (ids, raw)) in enumerate(zip(reqs, runs["lists"])):
        greedy = kw["temperature"] == 0
        forbidden = kw.get("forbidden_tokens", ())
        for mode in ("cap8", "dense"):
            assert runs[mode][i][0] == ids, (i, mode)
        for mode in ("lists", "cap8", "dense"):         # the same ids from the same model: the same raw logits, replayed per mode
            want, pen = replay_decode(runs[mode][i][1], ids, kw["frequency_penalty"], kw["presence_penalty"], kw["penalty_decay"],
                                      forbidden, greedy=greedy)
            if greedy:
                k = next((k for k in range(len(ids)) if ids[k] != want[k]), None)
                assert k is None, (i, mode, k, ids[k], want[k])
            elif mode == "lists":
                for k, tok in enumerate(ids):
                    err = check_sampled_step(pen[k], tok, kw["top_p"], kw["top_k"], forbidden)
                    assert err is None, (i, k, err)
        assert not set(ids) & set(forbidden), i
    # the penalties changed the greedy streams: penalised requests differ from their unpenalised twins
    assert runs["lists"][0][0] != runs["lists"][2][0]
    if V == 320:
        assert runs["lists"][1][0] != runs["lists"][5][0]
    plain = _run(m, V, reqs, "lists", run_ahead, use_graph, return_logits=False)
    assert [p[0] for p in plain] == [r[0] for r in runs["lists"]]


# ---------------------------------------------------------------------------------------------------------------------------
# sample_topp: kept tokens of weight 0 are never drawn

def _draw(row, us, T, top_p, top_k=0, batch=2000):
    """sample_topp over one logits row once per uniform in `us`: one launch row per draw (ids are written per row), launched in
    batches of `batch` rows."""
    from chirrup_amd import ops

    V = row.numel()
    dev_row = row.to(torch.float16).cuda()
    out = []
    for s in range(0, len(us), batch):
        u = torch.tensor(np.asarray(us[s:s + batch], np.float32), device="cuda")
        n = u.numel()
        lg = dev_row.expand(n, V).contiguous()
        ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ops.sample_topp(lg, torch.arange(n, dtype=torch.int32, device="cuda"), torch.full((n,), T, dtype=torch.float16, device="cuda"),
                        torch.full((n,), top_p, dtype=torch.float16, device="cuda"), torch.full((n,), top_k, dtype=torch.int32, device="cuda"),
                        u, ids)
        out.append(ids.cpu().numpy())
        del lg
    return np.concatenate(out)


def _zero_weight_row(V, kind, seed):
    """One row whose kept set holds tokens of weight 0 beside tokens of clearly positive weight, at the ends of the kernel's
    per-lane chunks (ceil(V / 1024) tokens each), at id 0 and at id V - 1.
      "forbidden": T = 1, positive logits in [-2, 0], the rest -inf (forbidden tokens: weight exactly 0; kept with top_p = 1
                   when the kernel's mass sums round that way);
      "underflow": T = 0.1, positive logits in {0, -1/8, -1/4, -3/8}; -6 at the chunk ends, id 0 and id V - 1 (kept for certain
                   with top_p = 1: they hold ~1e-3 of the mass; p^(1/T) underflows to 0 in binary32), the rest -inf.
    Returns (logits fp16 [V], T, relative weight p^(1/T) / sum in float64)."""
    rng = np.random.default_rng(seed)
    per = -(-V // 1024)
    lg = np.full(V, -np.inf, np.float32)
    for c0 in range(0, V, per):
        c1 = min(c0 + per, V)
        cand = np.arange(max(c0, 1), c1 - 1)
        if len(cand) == 0:
            continue
        pos = rng.choice(cand, size=min(3, len(cand)), replace=False)
        if kind == "forbidden":
            lg[pos] = rng.uniform(-2.0, 0.0, len(pos))
        else:
            lg[pos] = -0.125 * rng.integers(0, 4, len(pos))
            lg[c1 - 1] = -6.0
    T = 1.0 if kind == "forbidden" else 0.1
    if kind == "underflow":
        lg[0] = lg[V - 1] = -6.0
    lg = lg.astype(np.float16)
    f = lg.astype(np.float64)
    Tq = float(np.float16(T))
    w = np.exp((f - f.max()) / Tq)
    if kind == "underflow":                               # binary32 p^(1/T) = exp((v - max - ln Z) / T) of the -6 tokens is 0
        z = np.exp(f - f.max()).sum()
        w[(f > -np.inf) & (((f - f.max() - np.log(z)) / Tq) < -110.0)] = 0.0
    w /= w.sum()
    assert np.all((w == 0) | (w >= 1e-6)), "every weight is clearly positive or exactly 0"
    return lg, T, w


@pytest.mark.parametrize("V", [8192, 50304, 65536])
@pytest.mark.parametrize("kind", ["forbidden", "underflow"])
def test_sample_topp_never_draws_a_zero_weight_token(kind, V):
    """Kept tokens of weight 0 (forbidden -inf logits with top_p = 1; p^(1/T) underflowing at T = 0.1) at the last position of
    the lanes' chunks, at id 0 and at id V - 1.  The uniform sweeps a few dozen binary32 neighbours of every chunk boundary's
    cumulative fraction (where the walk inside a lane, or the fall-back when no lane claims the draw, meets rounding),
    1 - 2^-24 and a grid in between: every draw has a positive weight and a finite logit."""
    lg, T, w = _zero_weight_row(V, kind, seed=V + len(kind))
    per = -(-V // 1024)
    cum = np.cumsum(w)
    ends = [min(c0 + per, V) - 1 for c0 in range(0, V, per)]
    bounds = np.unique(np.clip(cum[ends], 0.0, 1.0)).astype(np.float32)
    us = [bounds]
    x_up, x_dn = bounds.copy(), bounds.copy()
    for _ in range(32):
        x_up, x_dn = np.nextafter(x_up, np.float32(2)), np.nextafter(x_dn, np.float32(-1))
        us += [x_up, x_dn]
    us.append(np.linspace(0.0, 1.0, 4097, dtype=np.float32)[:-1])
    us.append(np.array([1.0 - 2.0 ** -24, 0.0], np.float32))
    us = np.concatenate(us)
    us = us[(us >= 0) & (us < 1)]
    ids = _draw(torch.from_numpy(lg), us, T, top_p=1.0)
    assert ids.min() >= 0 and ids.max() < V
    bad = (w[ids] == 0) | ~np.isfinite(lg[ids].astype(np.float32))
    assert not bad.any(), (int(bad.sum()), len(ids), sorted(set(ids[bad].tolist()))[:8], us[bad][:8].tolist())
