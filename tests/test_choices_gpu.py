"""GPU: parallel choices (n).  rwkv7_fork_states bit for bit against torch copies (NaN payloads, infinities, -0; one group with 1 and
15 destinations, several groups in one launch; every other slot unchanged) on the L2/C128 geometry and on the 7.2B geometry at 201
slots; rwkv7_seeded_uniform with choice streams against its host form; then the real Worker on the L2/C128 golden model and the 0.1B
synthetic model, graph and eager, run-ahead and in-step: the siblings' states right after the fork equal the parent's, greedy choices
agree with each other and with n = 1 requests run at the same width, seeded choices follow the host replay of their own stream."""
import queue

import numpy as np
import pytest
import torch

from chirrup_amd import ops
from oracle import rwkv7_np as M
from test_decode_sampling_gpu import _model, _Sink, _Tok
from util import kept_sets

pytestmark = pytest.mark.gpu
MODELS = ["L2C128", "0.1B"]
VOCAB = {"L2C128": 320, "0.1B": 65536}
SPECIAL = [0x7E01, 0xFE7F, 0x7C00, 0xFC00, 0x8000, 0x0000, 0xFFFF, 0x7C01, 0x0001]     # NaN payloads, +-inf, -0, 0, a subnormal


# ------------------------------------------------------------------------------------------------------------ the kernels
def _tables(L, C, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shift = torch.randint(-32768, 32768, (L, 2, S, C), dtype=torch.int32, device="cuda", generator=g).to(torch.int16)
    wkv = torch.randint(-32768, 32768, (L, S, C // 64, 64, 64), dtype=torch.int32, device="cuda", generator=g).to(torch.int16)
    sp = torch.tensor(SPECIAL, dtype=torch.int32).to(torch.int16).cuda()
    for t in (shift, wkv):
        flat = t.view(-1)
        flat[:len(SPECIAL)] = sp
        flat[-len(SPECIAL):] = sp
    shift[:, :, :, :len(SPECIAL)] = sp                     # in every slot and layer
    wkv[:, :, 0, 0, :len(SPECIAL)] = sp
    elapsed = torch.randint(-(1 << 31), (1 << 31) - 1, (S,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    return shift, wkv, elapsed


def _torch_fork(shift, wkv, elapsed, groups):
    for src, dsts in groups:
        d = torch.tensor(dsts, dtype=torch.long, device="cuda")
        s = torch.full_like(d, src)
        for t, dim in ((shift, 2), (wkv, 1), (elapsed, 0)):
            t.index_copy_(dim, d, t.index_select(dim, s))


GEOMS = {"L2C128": (2, 128, 17), "7.2B": (32, 4096, 201)}


def _cases(S):
    return [[(3, [S - 1])],
            [(0, list(range(1, 16)))],
            [(2, [7, 8]), (9, [1, S - 1]), (4, [3, 0, 11, 12]), (S - 2, [5, 6, 10, 13, 14])]]


@pytest.mark.parametrize("geom", list(GEOMS))
def test_fork_states_kernel_matches_the_torch_copy(geom):
    L, C, S = GEOMS[geom]
    shift, wkv, elapsed = _tables(L, C, S, seed=C + S)
    for case in _cases(S):
        got = [t.clone() for t in (shift, wkv, elapsed)]
        ops.fork_states([got[0].view(torch.float16), got[1].view(torch.float16), got[2]], case)
        want = [t.clone() for t in (shift, wkv, elapsed)]
        _torch_fork(*want, case)
        torch.cuda.synchronize()
        for name, a, b in zip(("shift", "wkv", "elapsed"), got, want):
            assert torch.equal(a, b), (geom, case, name)
        dsts = sorted(d for _, ds in case for d in ds)
        keep = torch.tensor([s for s in range(S) if s not in dsts], dtype=torch.long, device="cuda")
        assert torch.equal(got[0].index_select(2, keep), shift.index_select(2, keep))          # every other slot bit-unchanged
        assert torch.equal(got[1].index_select(1, keep), wkv.index_select(1, keep))
        assert torch.equal(got[2][keep], elapsed[keep])
        for src, ds in case:                                                                 # the specials survived the copy
            for d in ds:
                assert torch.equal(got[0][:, :, d, :len(SPECIAL)], shift[:, :, src, :len(SPECIAL)])
        del got, want
    torch.cuda.empty_cache()


def test_seeded_uniform_kernel_with_choice_streams():
    rng = np.random.default_rng(16)
    S, B = 40, 33
    seeds = torch.from_numpy(rng.integers(-(1 << 63), (1 << 63) - 1, S, dtype=np.int64))
    seeded = torch.from_numpy(rng.integers(0, 17, S).astype(np.int32))                      # 0: unseeded, 1 + j: choice j <= 15
    seeded[:4] = torch.tensor([1, 16, 2, 0], dtype=torch.int32)
    counters = torch.from_numpy(rng.integers(-(1 << 31), (1 << 31) - 1, S, dtype=np.int64).astype(np.int32))
    slot_idx = torch.from_numpy(rng.permutation(S)[:B].astype(np.int32))
    rows = torch.from_numpy(rng.permutation(B)[:30].astype(np.int32))
    u = torch.from_numpy(rng.random(30).astype(np.float32))
    h = [t.clone() for t in (seeds, seeded, counters, u)]
    d = [t.cuda() for t in (seeds, seeded, counters, u)]
    for _ in range(3):
        ops.seeded_uniform(rows, slot_idx, *h)
        ops.seeded_uniform(rows.cuda(), slot_idx.cuda(), *d)
        torch.cuda.synchronize()
        assert np.array_equal(d[3].cpu().numpy().view(np.uint32), h[3].numpy().view(np.uint32))
        assert torch.equal(d[2].cpu(), h[2])
    s0 = slot_idx[rows.long()].long()
    for i in range(30):                                                                      # each row drew from its own stream
        s = int(s0[i])
        if int(seeded[s]):
            c = (int(counters[s]) + 2) & 0xFFFFFFFF
            assert h[3][i].item() == float(ops.philox_uniform(int(seeds[s]), c, int(seeded[s]) - 1))


# ------------------------------------------------------------------------------------------------------------ the worker
def _worker(m, V, run_ahead, use_graph, batch_size=9):
    from chirrup_amd.core_structure import ModelLoadConfig
    from chirrup_amd.worker import Worker

    cfg = ModelLoadConfig(model_path="unused", vocab_path="unused", vocab_size=V, head_size=64)
    tq = queue.Queue()
    w = Worker("w0", [0], cfg, tq, queue.Queue(), None, batch_size=batch_size, model=m, tokenizer=_Tok(), run_ahead=run_ahead)
    w._init_worker()
    assert w.use_graph
    w.use_graph = use_graph
    w.max_prefill_count = batch_size
    return w, tq


def _task(prompt, state=None, **kw):
    from chirrup_amd.core_structure import Task

    return Task(output_queue=_Sink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(prompt), state=state,
                stop_tokens=[], return_logits=True, **kw)


def _group(prompt, n, state=None, **kw):
    others = [_task(prompt, choice_index=j, **kw) for j in range(1, n)]
    return [_task(prompt, state=state, siblings=others, **kw)] + others


def _drain(w, tasks):
    for _ in range(4000):
        if not w.step():
            break
    out = []
    for t in tasks:
        items = [p for k, p in t.output_queue.items if k == "token_generated"]
        assert t.output_queue.items[-1][0] == "task_completed" and len(items) == t.max_tokens
        out.append(([p[0] for p in items], [p[2].numpy() for p in items]))
    return out


def replay_seeded(raw_logits, emitted, kw, stream):
    """Host replay of a seeded sampled choice (test_seed_bias_gpu.replay_seeded with the uniforms of Philox stream `stream`): raw ->
    penalties -> kept set -> inverse-CDF draw in float64.  Returns per step (host id, doubtful): doubtful when the kept set is
    ambiguous or u * total lies within 1e-5 (relative) of an edge of the drawn token's interval."""
    f16, f32 = np.float16, np.float32
    V = len(raw_logits[0])
    occ, alpha = np.zeros(V, f32), np.zeros(V, f32)
    T = float(f16(kw["temperature"]))
    out = []
    for k, (raw, tok) in enumerate(zip(raw_logits, emitted)):
        lg, occ = M.apply_penalties(np.array(raw, dtype=f16).reshape(V), occ, alpha, f16(kw["penalty_decay"]), f16(kw["frequency_penalty"]))
        sets = kept_sets(torch.softmax(torch.from_numpy(lg.astype(f32)), -1), kw["top_p"], kw.get("top_k", 0))
        x = lg.astype(np.float64)
        p = np.exp(x - x.max())
        p /= p.sum()
        u = float(ops.philox_uniform(kw["seed"], k, stream))
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


def _seeded_kw(V):
    """Seeded sampled rows; the 0.1B synthetic model's nearly flat logits need a low temperature for the replay to decide most draws
    (test_seed_bias_gpu._specs)."""
    return dict(temperature=1.0 if V <= 1024 else 0.25, top_p=0.95, top_k=0, seed=-31337, frequency_penalty=0.2, presence_penalty=0.1,
                penalty_decay=0.99)


GREEDY = dict(temperature=0.0, top_p=0.0, top_k=0, frequency_penalty=0.3, presence_penalty=0.2, penalty_decay=0.98)


def _check_seeded(runs, kw, tag):
    steps = doubtful = 0
    for j, (ids, raw) in enumerate(runs):
        for k, ((host, doubt), tok) in enumerate(zip(replay_seeded(raw, ids, kw, j), ids)):
            steps += 1
            doubtful += doubt
            assert tok == host or doubt, (tag, j, k, tok, host)
    assert doubtful <= steps // 8, (tag, steps, doubtful)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
@pytest.mark.parametrize("model", MODELS)
def test_fork_after_a_prefill(model, run_ahead, use_graph, monkeypatch):
    """A 23-token prompt (chunked and single-token prefill) with n = 4: right after the fork every sibling's shift rows, WKV rows and
    step counter equal the parent's bit for bit (elapsed = P - 1); the greedy choices decode identical raw logits and ids; seeded
    choices follow their own streams' host replay."""
    V = VOCAB[model]
    m = _model(model)
    checked = []
    real = ops.fork_states

    def spy(pool, groups):
        real(pool, groups)
        torch.cuda.synchronize()
        for src, dsts in groups:
            for d in dsts:
                for t, dim in ((pool[0], 2), (pool[1], 1), (pool[2], 0)):
                    a, b = t.select(dim, d), t.select(dim, src)
                    assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a,
                                       b.view(torch.int16) if b.dtype == torch.float16 else b), (src, d)
            checked.append((src, list(dsts), int(pool[2][src])))

    monkeypatch.setattr(ops, "fork_states", spy)
    prompt = np.random.default_rng(V).integers(1, V, 23).tolist()
    w, tq = _worker(m, V, run_ahead, use_graph)
    g = _group(prompt, 4, max_tokens=24, **GREEDY)
    s = _group(prompt, 4, max_tokens=32, **_seeded_kw(V))
    for t in (g[0], s[0]):
        tq.put(t)
    greedy, seeded = _drain(w, g), _drain(w, s)
    assert sorted(len(d) for _, d, _ in checked) == [3, 3]                      # two groups, admitted together
    assert all(e == len(prompt) - 1 for _, _, e in checked)
    ids0, raw0 = greedy[0]
    for ids, raw in greedy[1:]:
        assert ids == ids0 and all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(raw, raw0))
    _check_seeded(seeded, _seeded_kw(V), (model, run_ahead, use_graph))


def _prefix_state(m, prompt):
    st = m.generate_zero_state(1)
    m.forward_seq_batch_seperate([list(prompt)], st)
    torch.cuda.synchronize()
    return [st[0][:, :, [0]].clone(), st[1][:, [0]].clone(), st[2][[0]].clone()]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("run_ahead", [True, False], ids=["run_ahead", "in_step"])
@pytest.mark.parametrize("model", MODELS)
def test_choices_equal_single_requests_at_the_same_width(model, run_ahead, use_graph):
    """The forward is not batch-invariant across row counts, so n = 4 is compared with four n = 1 requests side by side, both from
    the same prefix state (a cache hit) with one prompt token left: every step then runs at width 4 in both runs.  Greedy: eight
    identical streams.  Seeded: choice 0 equals the n = 1 requests with the same seed; choice j follows the replay of stream j."""
    V = VOCAB[model]
    m = _model(model)
    prompt = np.random.default_rng(V + 1).integers(1, V, 17).tolist()
    state = _prefix_state(m, prompt[:-1])
    fresh = lambda: [t.clone() for t in state]
    for kw, n_new in ((GREEDY, 24), (_seeded_kw(V), 32)):
        w, tq = _worker(m, V, run_ahead, use_graph)
        g = _group(prompt[-1:], 4, state=fresh(), max_tokens=n_new, **kw)
        tq.put(g[0])
        group = _drain(w, g)
        w, tq = _worker(m, V, run_ahead, use_graph)
        singles = [_task(prompt[-1:], state=fresh(), max_tokens=n_new, **kw) for _ in range(4)]
        for t in singles:
            tq.put(t)
        single = _drain(w, singles)
        ref_ids, ref_raw = single[0]
        for ids, raw in single[1:] + (group if kw is GREEDY else group[:1]):
            assert ids == ref_ids, (model, kw is GREEDY)
            assert all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(raw, ref_raw))
        if kw is not GREEDY:
            _check_seeded(group, kw, (model, run_ahead, use_graph))
            assert len({tuple(ids) for ids, _ in group}) == 4
