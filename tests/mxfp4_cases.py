"""The exact GEMM cases of the MXFP4 kernels (csrc/mxfp4.hip), built like gemm_ref.f16_case.  TEST INFRASTRUCTURE ONLY, CPU only.

Every dequantised weight is E2M1(code) 2^e, a dyadic number, so the product with x on the grid i 2^-3 is the binary16 GEMM of
tests/gemm_ref.py fed the dequantised matrix: with e in -12..-6 the weights are wi 2^-13, wi = 2 E2M1(code) 2^(e + 12) an integer of
at most 768, and G.prove_exact / G.expected / G.expected_planes / G.assert_bits apply as they stand (the exact-sum lemma: every
binary32 sum is exact in any order, one admissible binary16 pattern per output).  tests/test_mxfp4_cpu.py proves the lemma's
condition for every case here; tests/test_mxfp4_gpu.py runs them."""
import numpy as np

import gemm_ref as G

F64 = np.float64
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
SEED = 7
E_LO, E_HI = -12, -6

# id -> (M, N, K, split counts whose planes are formed).  M: 1 row, 17 / 33 / 113 (a partial last 16-row tile; 2, 3, 8 tiles), 127 /
# 128 / 129 (8 full tiles and one row either side), 200 (13 tiles), 256 (16 tiles: the whole 64 KiB of LDS); N: 1, 2, 3 tile columns;
# K: one K-block, three (a split of 2 is cut back), six, 16 and 64 (the library's own split).
CASES = {
    "M1-N128-K64": (1, 128, 64, (1,)),
    "M17-N128-K192": (17, 128, 192, (1,)),
    "M33-N256-K1024": (33, 256, 1024, (1, 2, 4)),
    "M113-N384-K1024": (113, 384, 1024, (1, 2, 4, 16)),
    "M200-N256-K4096": (200, 256, 4096, (1, 2, 4, 16)),
    "M256-N128-K4096": (256, 128, 4096, (1,)),
    "M127-N128-K192": (127, 128, 192, (1, 3)),
    "M128-N128-K192": (128, 128, 192, (1, 3)),
    "M129-N256-K384": (129, 256, 384, (1, 2, 3, 6)),
}


def signed(codes):
    """E2M1 values of 4-bit codes (bit 3 = sign), binary64; code 8 is -0."""
    v = E2M1[codes & 7]
    return np.where(codes & 8, -v, v)


def mx_case(M, N, K, seed=SEED):
    """x [M,K] = xi 2^-3 (|xi| <= 31), codes [N,K] uniform in 0..15, block exponents eblk [N, K/32] uniform in -12..-6 drawn per
    32-block (the two halves of a K-block differ), and the same weights as the integers wi = 2 E2M1 2^(e + 12) with ew = -13."""
    rng = np.random.default_rng(seed)
    xi = G._grid(rng, (M, K), 8.0, 31)
    codes = rng.integers(0, 16, (N, K)).astype(np.uint8)
    eblk = rng.integers(E_LO, E_HI + 1, (N, K // 32))
    wi = 2.0 * signed(codes) * 2.0 ** (np.repeat(eblk, 32, axis=1) + 12) + 0.0
    return dict(xi=xi, wi=wi, bi=None, ex=-3, ew=-13, eb=-6, codes=codes, eblk=eblk)


_CASES = {}


def named(name):
    if name not in _CASES:
        M, N, K, _ = CASES[name]
        _CASES[name] = mx_case(M, N, K)
    return _CASES[name]


def scaled(case, sx, sw=0):
    """x times 2^sx, every block exponent plus sw (the lemma is scale-free)."""
    c = G.scaled(case, sx, sw)
    c["eblk"] = case["eblk"] + sw
    return c


# scaled cases: (base, sx, sw).  subnormal: x = xi 2^-21 (subnormal halves), every output a binary16 subnormal; overflow: x = xi 2^9,
# block exponents -8..-2, sums of ~2^15 with a good share past 65504
SCALED = {"subnormal": ("M33-N256-K1024", -18, 0), "overflow": ("M33-N256-K1024", 12, 4)}


def scaled_named(name):
    base, sx, sw = SCALED[name]
    return scaled(named(base), sx, sw), CASES[base][3]


def extreme_case(M=33, N=256, K=1024, seed=SEED):
    """Block exponents at the two ends of the accepted range.  An output row of W whose blocks mixed 2^-13 and 2^13 would spread its
    terms over 26 binades -- no binary32 sum of them is exact -- so every row n holds ONE of the two exponents (drawn per row: both
    occur inside every 16-row MFMA tile) and the case is the union of two exact sub-cases over the same x = xi 2^-10: rows at 2^13
    (wi = 2 E2M1, ew = 12; outputs of a few thousand) and rows at 2^-13 (ew = -14; outputs around the subnormal boundary 2^-14).
    Returns (case with codes / eblk for the kernel, {exponent: (column index, sub-case)})."""
    rng = np.random.default_rng(seed + 1)
    xi = G._grid(rng, (M, K), 8.0, 31)
    codes = rng.integers(0, 16, (N, K)).astype(np.uint8)
    erow = rng.choice([-13, 13], N)
    assert all((erow[i:i + 16] == -13).any() and (erow[i:i + 16] == 13).any() for i in range(0, N, 16))
    eblk = np.repeat(erow[:, None], K // 32, axis=1)
    subs = {}
    for e in (-13, 13):
        cols = np.nonzero(erow == e)[0]
        subs[e] = (cols, dict(xi=xi, wi=2.0 * signed(codes[cols]) + 0.0, bi=None, ex=-10, ew=e - 1, eb=-6))
    return dict(xi=xi, ex=-10, codes=codes, eblk=eblk), subs


def x_half(case):
    x = case["xi"] * 2.0 ** case["ex"]
    x16 = G.h(x)
    assert np.array_equal(x16.astype(F64), x)
    return x16


def packed(case):
    """(codes uint8 [N, K/2] with the low nibble = even k, scale bytes uint8 [N, K/32]) of a case."""
    c = case["codes"]
    scales = case["eblk"] + 127
    assert scales.min() >= 114 and scales.max() <= 140
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8), scales.astype(np.uint8)


def dequantised(case):
    """The weights as binary64, from codes and block exponents."""
    return signed(case["codes"]) * 2.0 ** np.repeat(case["eblk"], 32, axis=1)
