"""Shared by tests/test_state_codec_cpu.py and tests/test_state_codec_gpu.py: the MXINT8 state codec written down a second time,
straight from its definition (binary64 comparisons against the exact thresholds 127 * 2^(e-6), numpy's ties-to-even rint), and
the inputs both files use.  Nothing here imports chirrup_amd.quant: the host codec is held to this, the kernels to the host codec."""
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_MIN, E_MAX = -18, 15
HEAD_BYTES = 4224
THRESHOLDS = np.array([127.0 * 2.0 ** (e - 6) for e in range(E_MIN, E_MAX + 1)])      # exact in binary64, and in binary16
FIXTURE_STATES = (("model_small_state.npz", "c128:s1_out"), ("model_small_state.npz", "c768:s1_out"),
                  ("model_L3_C768.npz", "b2t5:s1_out"), ("model_L3_C768.npz", "greedy:s1_final"),
                  ("model_L2_C128.npz", "b3t5:s1_out"), ("model_L2_C128.npz", "greedy:s1_final"))


def exponent_by_definition(amax64: np.ndarray) -> np.ndarray:
    """The smallest integer e in [-18, 15] with amax <= 127 * 2^(e-6) (15 when there is none; an all-zero block gives -18)."""
    return np.minimum(np.searchsorted(THRESHOLDS, amax64, side="left"), E_MAX - E_MIN) + E_MIN


def pack_by_definition(x16: np.ndarray) -> np.ndarray:
    """binary16 [..., 64, 64] -> uint8 [..., 4224]."""
    lead = x16.shape[:-2]
    x = x16.astype(np.float64).reshape(lead + (128, 32))
    bad = ~np.isfinite(x).all(-1)
    amax = np.where(bad, 0.0, np.abs(np.where(np.isfinite(x), x, 0.0)).max(-1))
    e = exponent_by_definition(amax)
    c = np.clip(np.rint(x * 2.0 ** (6 - e)[..., None]), -127, 127)
    c = np.where(bad[..., None], 0.0, np.nan_to_num(c)).astype(np.int8)
    s = np.where(bad, 0xFF, e + 127).astype(np.uint8)
    return np.concatenate([c.view(np.uint8).reshape(lead + (4096,)), s], -1)


def unpack_by_definition(p: np.ndarray) -> np.ndarray:
    """uint8 [..., 4224] -> binary16 [..., 64, 64]; asserts that no value is rounded."""
    lead = p.shape[:-1]
    c = np.ascontiguousarray(p[..., :4096]).view(np.int8).astype(np.float64).reshape(lead + (128, 32))
    s = p[..., 4096:].astype(np.int64)
    v = c * 2.0 ** (s - 133)[..., None]
    v16 = v.astype(np.float16)
    ok = s != 0xFF
    assert np.array_equal(v16.astype(np.float64)[ok], v[ok])
    v16[~ok] = np.array(0x7E00, np.uint16).view(np.float16)
    return v16.reshape(lead + (64, 64))


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint16)


def boundary_values() -> np.ndarray:
    """Every 127 * 2^(e-6), e = -18..15, and the binary16 neighbours one ulp below and above (102 values, all finite)."""
    t = THRESHOLDS.astype(np.float16)
    assert np.array_equal(t.astype(np.float64), THRESHOLDS)
    return np.concatenate([np.nextafter(t, np.float16(0)), t, np.nextafter(t, np.float16(np.inf))])


def all_finite_patterns_heads(seed: int = 0) -> np.ndarray:
    """binary16 [n, 64, 64] holding every finite bit pattern (63488 of them, both signs, both zeros, every subnormal) at least
    once: each block gets 8 of them at random positions among 24 random partners of random magnitude 2^-20 .. 2^13."""
    rng = np.random.default_rng(seed)
    pat = np.arange(1 << 16, dtype=np.uint32)
    pat = pat[(pat & 0x7C00) != 0x7C00].astype(np.uint16)
    rng.shuffle(pat)
    n_blocks = len(pat) // 8
    n_heads = -(-n_blocks // 128)
    blocks = (rng.standard_normal((n_heads * 128, 32)) * 2.0 ** rng.integers(-20, 14, (n_heads * 128, 1))).astype(np.float16)
    for b in range(n_blocks):
        blocks[b, rng.choice(32, 8, replace=False)] = pat[8 * b: 8 * b + 8].view(np.float16)
    return blocks.reshape(n_heads, 64, 64)


def special_heads(seed: int = 1) -> np.ndarray:
    """binary16 [4, 64, 64]: the scale rule's boundary values as the amax of a block with random smaller partners (and alone),
    zero blocks (+0, -0, mixed), subnormal-only blocks, 2^-24 alone, 65504 and -65504 blocks, ties (k + 0.5 at e = 6), and blocks
    with one NaN, one +inf, one -inf among ordinary values."""
    rng = np.random.default_rng(seed)
    blocks = np.zeros((4 * 128, 32), np.float16)
    k = 0
    for v in boundary_values():
        blocks[k] = (rng.uniform(-1, 1, 32) * float(v)).astype(np.float16)
        blocks[k, rng.integers(32)] = v if k % 2 else -v
        blocks[k + 1, rng.integers(32)] = v
        k += 2
    blocks[k + 1] = np.float16(-0.0)
    blocks[k + 2, ::2] = np.float16(-0.0)
    k += 3                                                                  # three zero blocks
    blocks[k] = (rng.integers(-1023, 1024, 32).astype(np.int64).astype(np.float64) * 2.0 ** -24).astype(np.float16)
    blocks[k + 1, 7] = np.float16(2.0 ** -24)
    blocks[k + 2, 31] = np.float16(-2.0 ** -24)
    k += 3
    blocks[k] = (rng.uniform(-1, 1, 32) * 65504).astype(np.float16)
    blocks[k, 0], blocks[k, 31] = np.float16(65504), np.float16(-65504)
    blocks[k + 1, 5] = np.float16(65504)
    blocks[k + 2] = np.float16(65504)
    k += 3
    blocks[k] = np.concatenate([np.arange(-16, 16) + 0.5]).astype(np.float16)         # e = 6 needs amax in (63.5, 127]
    blocks[k, 0] = np.float16(100.0)
    blocks[k + 1] = -blocks[k]
    k += 2
    for bad in (np.nan, np.inf, -np.inf):
        blocks[k] = rng.standard_normal(32).astype(np.float16)
        blocks[k, rng.integers(32)] = np.float16(bad)
        k += 1
    blocks[k] = np.array(0xFE01, np.uint16).view(np.float16)                         # NaNs with a payload and a sign, all of them
    k += 1
    assert k <= len(blocks)
    rest = blocks[k:]
    rest[:] = (rng.standard_normal(rest.shape) * 2.0 ** rng.integers(-20, 14, (len(rest), 1))).astype(np.float16)
    return blocks.reshape(4, 64, 64)


def fixture_states():
    """[(name, binary16 [n, 64, 64])] of the six committed state arrays."""
    out = []
    for f, key in FIXTURE_STATES:
        out.append((f"{f}:{key}", np.load(os.path.join(G, f))[key].reshape(-1, 64, 64)))
    return out


def all_inputs() -> np.ndarray:
    """Every head of the three families above, binary16 [n, 64, 64]."""
    return np.concatenate([all_finite_patterns_heads(), special_heads()] + [a for _, a in fixture_states()], 0)
