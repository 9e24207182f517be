"""GPU: sample_topp_kernel (csrc/sampler.hip) against the binary64 admissible-set reference of its own operation
(tests/sampler_ref.py; its bounds are derived there and checked on the CPU by test_sampler_ref_cpu.py).

Per vocabulary size and settings case, for every T of the reference's list: about 2000 random uniforms, and every binary32
uniform within 16 ulps of every lane boundary's point of the CDF (where two lanes' partial sums, reached through different trees
of binary32 additions, meet).  One launch row per draw.  Every returned id must be admissible; ids of rows that are not listed keep
their -1; a second launch returns the same bits; the logits lie between NaN canaries that stay NaN."""
import numpy as np
import pytest
import torch

import sampler_ref as R

pytestmark = pytest.mark.gpu
GAP = 64                                       # canary halves on either side of the logits (a multiple of 8: 16-byte alignment)


def _launch(x16, variants, us, vi, rng):
    """ids [n] of one launch with a row per draw: draw i uses variants[vi[i]] through its slot.  The rows are listed in a
    permuted order, their slots are a permutation of a larger table, and two more rows are not listed at all."""
    from chirrup_amd import ops

    V, n = x16.size, len(us)
    B, S = n + 2, n + 5
    buf = torch.full((B * V + 2 * GAP,), float("nan"), dtype=torch.float16, device="cuda")
    logits = buf[GAP:GAP + B * V].view(B, V)
    logits.copy_(torch.from_numpy(x16).cuda().expand(B, V))
    order = rng.permutation(B)[:n]                                     # launch index i -> logits row
    slot_of_row = rng.permutation(S)[:B]
    t, tp, tk = np.ones(S, np.float16), np.zeros(S, np.float16), np.zeros(S, np.int32)
    for i in range(n):
        T, P, K = variants[vi[i]]
        s = slot_of_row[order[i]]
        t[s], tp[s], tk[s] = T, P, K
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rows, slot_idx, u = dev(order.astype(np.int32)), dev(slot_of_row.astype(np.int32)), dev(us.astype(np.float32))
    t, tp, tk = dev(t), dev(tp), dev(tk)
    out = []
    for _ in range(2):
        ids = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        ops.sample_topp(logits, rows, t, tp, tk, u, ids, slot_idx=slot_idx)
        out.append(ids.cpu().numpy())
    assert np.array_equal(out[0], out[1]), "two launches differ"
    listed = np.zeros(B, bool)
    listed[order] = True
    assert (out[0][~listed] == -1).all(), "a row that is not listed was written"
    assert bool(torch.isnan(buf[:GAP]).all()) and bool(torch.isnan(buf[GAP + B * V:]).all())
    assert np.array_equal(logits[0].cpu().numpy().view(np.uint16), x16.view(np.uint16))
    return out[0][order]


@pytest.mark.parametrize("setting", R.SETTINGS)
@pytest.mark.parametrize("V", R.VS)
def test_every_draw_is_admissible(V, setting):
    big = V > 8200                                  # 100-128 KiB rows: batches of 1000 rows, ONE for the boundary sweep
    rng = np.random.default_rng(V)
    failures = []
    for T in R.TS:
        case = R.make_case(V, setting, T)
        for kind in ("random", "boundary"):
            us, vi = R.uniforms(case, kind, max_rows=1000 if big else None)
            nb = 1000 if big else 4000
            ids = np.concatenate([_launch(case["x"], case["variants"], us[s:s + nb], vi[s:s + nb], rng) for s in range(0, len(us), nb)])
            assert ids.min() >= 0 and ids.max() < V
            ok, single = np.zeros(len(us), bool), 0
            for v, prep in enumerate(case["preps"]):
                sel = vi == v
                ok[sel] = prep.accepts(us[sel], ids[sel])
                single += int((prep.sets(us[sel]) == 1).sum())
            print(f"{case['name']} {kind}: {len(us)} draws, {single / len(us):.4f} single-id, {int((~ok).sum())} outside")
            if not ok.all():
                bad = np.nonzero(~ok)[0]
                failures.append((case["name"], kind, len(bad), len(us), [(float(us[i]).hex(), int(ids[i])) for i in bad[:4]]))
    assert not failures, failures
