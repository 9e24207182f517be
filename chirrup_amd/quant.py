"""Quantisation, host side: the weight formats mm8 (w8a16, below) and MXFP4 (w4a16, second part of the file), and the MXINT8 codec of
the prefix-state arena's head states (last part).

Restates the reference's quantize_weight (scripts/test_mm8/benchmark.py:54-85, the rwkv pip package's
scheme): for w [N_in, M_out] subtract column minima mx and row minima my (order depends on the
shape), divide by column maxima rx and row maxima ry, store floor(w*256) clipped to uint8 and the
four vectors as fp16 (rx, ry pre-divided by 16).  Dequantisation: (q + 0.5) * ry * rx + my + mx.
"""
from typing import NamedTuple

import torch


class Mm8Weight(NamedTuple):
    qT: torch.Tensor   # uint8 [M_out, N_in]  (K-contiguous layout of the MFMA kernel; q = qT.t())
    mx: torch.Tensor   # fp16 [M_out]
    rx: torch.Tensor   # fp16 [M_out]
    my: torch.Tensor   # fp16 [N_in]
    ry: torch.Tensor   # fp16 [N_in]


def quantize_weight(w16: torch.Tensor):
    """w16 [N_in, M_out] -> (q uint8 [N,M], mx [M], rx [M], my [N,1], ry [N,1]) like the reference."""
    w = w16.float()
    if w.shape[0] > w.shape[1]:
        my = torch.amin(w, dim=1, keepdim=True); w = w - my
        mx = torch.amin(w, dim=0); w = w - mx
        rx = torch.amax(w, dim=0); w = w / rx
        ry = torch.amax(w, dim=1, keepdim=True); w = w / ry
    else:
        mx = torch.amin(w, dim=0); w = w - mx
        my = torch.amin(w, dim=1, keepdim=True); w = w - my
        rx = torch.amax(w, dim=0); w = w / rx
        ry = torch.amax(w, dim=1, keepdim=True); w = w / ry
    q = torch.clip(torch.floor(w * 256), min=0, max=255).to(torch.uint8)
    h = torch.float16
    return q, mx.to(h).contiguous(), (rx / 16).to(h).contiguous(), my.to(h).contiguous(), (ry / 16).to(h).contiguous()


def quantize_linear(weight_out_in: torch.Tensor) -> Mm8Weight:
    """A torch Linear weight [M_out, N_in] (y = x @ W.T) -> packed mm8 form.  The reference quantises
    the matrix in the orientation it multiplies with, w = W.T [N_in, M_out]."""
    q, mx, rx, my, ry = quantize_weight(weight_out_in.t())
    return Mm8Weight(q.t().contiguous(), mx, rx, my.reshape(-1).contiguous(), ry.reshape(-1).contiguous())


def untile_u8(flat: torch.Tensor, m_out: int, n_in: int) -> torch.Tensor:
    """Inverse of ops.tile_weight_u8 (inspection / tests): flat tile images -> uint8 [m_out, n_in] row-major.
    Tile (g, b) = 512 chunks of 16 B; row nr = c >> 2 at chunk position c & 3 holds logical chunk (c & 3) ^ ((nr >> 2) & 3)."""
    img = flat.view(m_out // 128, n_in // 64, 128, 4, 16)
    nr = torch.arange(128, device=flat.device)
    pos = torch.arange(4, device=flat.device).view(1, 4) ^ ((nr >> 2) & 3).view(128, 1)     # position of logical chunk lc in row nr
    rows = torch.gather(img, 3, pos.view(1, 1, 128, 4, 1).expand(m_out // 128, n_in // 64, 128, 4, 16))
    return rows.permute(0, 2, 1, 3, 4).reshape(m_out, n_in).contiguous()



# ---------------------------------------------------------------------------------------------------------------------
# MXFP4 (w4a16): OCP Microscaling FP4, blocks of 32 along K (include/chirrup_amd.h: mxfp4_*)

MXFP4_BLOCK = 32
MXFP4_E_MIN, MXFP4_E_MAX = -13, 13               # 0.5 * 2^e is a normal binary16 number and 6 * 2^e is finite
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MXFP4_TILE_BYTES = 128 * 32 + 128 * 2            # one (128 rows x 64 k) tile image: codes, then scales


class Mxfp4Weight(NamedTuple):
    codes: torch.Tensor    # uint8 [M_out, N_in / 2]: byte j of a row holds k = 2 j (low nibble) and 2 j + 1 (high nibble); bit 3 = sign
    scales: torch.Tensor   # uint8 [M_out, N_in / 32]: E8M0, the block's weights are E2M1(code) * 2^(scale - 127)


def check_mxfp4(w: Mxfp4Weight) -> None:
    """Refuse what the kernels do not define: mismatched shapes, scale bytes outside 2^-13 .. 2^13 (0xFF, the format's NaN, too)."""
    c, s = w.codes, w.scales
    if c.dtype != torch.uint8 or s.dtype != torch.uint8 or c.dim() != 2 or s.dim() != 2:
        raise ValueError("Mxfp4Weight: codes and scales must be uint8 matrices")
    if c.shape[0] != s.shape[0] or c.shape[1] * 2 != s.shape[1] * MXFP4_BLOCK or c.shape[1] == 0:
        raise ValueError(f"Mxfp4Weight: codes {tuple(c.shape)} and scales {tuple(s.shape)} do not describe one [M_out, N_in] matrix")
    if s.numel():
        lo, hi = int(s.min()), int(s.max())
        if lo < 127 + MXFP4_E_MIN or hi > 127 + MXFP4_E_MAX:
            raise ValueError(f"Mxfp4Weight: scale bytes {lo}..{hi} outside {127 + MXFP4_E_MIN}..{127 + MXFP4_E_MAX} "
                             f"(block exponents {MXFP4_E_MIN}..{MXFP4_E_MAX})")


def quantize_linear_mxfp4(weight: torch.Tensor) -> Mxfp4Weight:
    """A Linear weight [M_out, N_in] (y = x @ W.T) -> MXFP4: per 32-block along N_in the exponent e = clamp(ceil(log2(amax / 6)),
    -13, 13), i.e. the SMALLEST scale at which the block's largest element does not saturate (6 * 2^(e-1) < amax <= 6 * 2^e; the OCP
    specification's rule is floor(log2(amax)) - 2, which lets elements above 6 * 2^e clamp -- here |w - w~| <= 2^e for every element
    of an unclamped block); an all-zero block takes e = -13.  Elements: nearest value of the E2M1 grid, ties to the even code,
    clamped to +-6 (which only a block clamped at e = 13 can need).  Deterministic: no random rounding, exact comparisons in binary64."""
    if weight.dim() != 2 or weight.shape[1] % MXFP4_BLOCK or weight.shape[1] == 0 or weight.shape[0] == 0 or not weight.dtype.is_floating_point:
        raise ValueError(f"quantize_linear_mxfp4: expected a floating-point [M_out, N_in] matrix with N_in % {MXFP4_BLOCK} == 0, "
                         f"got {tuple(weight.shape)} {weight.dtype}")
    M, N = weight.shape
    w = weight.detach().to(torch.float64).reshape(M, N // MXFP4_BLOCK, MXFP4_BLOCK)
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_linear_mxfp4: the weight holds NaN or inf")
    amax = w.abs().amax(-1)
    _, ex = torch.frexp(amax / 6.0)                                  # amax / 6 = m 2^ex, m in [0.5, 1): ceil(log2) is ex or ex - 1
    e = ex.to(torch.int64)
    e = torch.where(torch.ldexp(torch.full_like(amax, 6.0), e - 1) >= amax, e - 1, e)      # exact: amax <= 6 * 2^(e-1)
    e = torch.where(torch.ldexp(torch.full_like(amax, 6.0), e) < amax, e + 1, e)
    e = torch.where(amax == 0, torch.full_like(e, MXFP4_E_MIN), e).clamp(MXFP4_E_MIN, MXFP4_E_MAX)
    y = torch.ldexp(w.abs(), (-e).unsqueeze(-1).expand_as(w)).clamp(max=6.0)                # exact scaling by a power of two
    # grid midpoints; a tie goes to the even code: 0.25 -> 0, 0.75 -> 2, 1.25 -> 2, 1.75 -> 4, 2.5 -> 4, 3.5 -> 6, 5 -> 6
    code = ((y > 0.25).to(torch.uint8) + (y >= 0.75).to(torch.uint8) + (y > 1.25).to(torch.uint8) + (y >= 1.75).to(torch.uint8)
            + (y > 2.5).to(torch.uint8) + (y >= 3.5).to(torch.uint8) + (y > 5.0).to(torch.uint8))
    code = code | (((w < 0) & (code > 0)).to(torch.uint8) << 3)      # (no negative zeros)
    code = code.reshape(M, N // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).contiguous()
    return Mxfp4Weight(codes, (e + 127).to(torch.uint8).contiguous())


def dequantize_mxfp4(w: Mxfp4Weight) -> torch.Tensor:
    """w~ as binary16 [M_out, N_in], exact: E2M1(code) * 2^(scale - 127)."""
    check_mxfp4(w)
    c = w.codes
    M, N = c.shape[0], c.shape[1] * 2
    nib = torch.stack([c & 15, c >> 4], -1).reshape(M, N).long()
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=c.device)
    e = (w.scales.to(torch.int32) - 127).repeat_interleave(MXFP4_BLOCK, dim=1)
    v = torch.ldexp(table[nib], e)
    out = v.to(torch.float16)
    assert bool((out.float() == v).all())
    return out


def mxfp4_tiled_bytes(m_out: int, n_in: int) -> int:
    return (m_out // 128) * (n_in // 64) * MXFP4_TILE_BYTES


def untile_mxfp4(flat: torch.Tensor, m_out: int, n_in: int) -> Mxfp4Weight:
    """Inverse of ops.tile_weight_mxfp4 (inspection / tests): flat tile images -> the row-major Mxfp4Weight.  Tile (g, b) is 4352 bytes:
    128 rows x 32 code bytes, position 8 q + 4 s + j of a row holding logical byte 16 s + 4 q + j of the K-block (k = 32 s + 8 q + 2 j, + 1),
    then 128 rows x 2 scale bytes."""
    G, B = m_out // 128, n_in // 64
    img = flat.view(G, B, MXFP4_TILE_BYTES)
    codes = img[..., :4096].reshape(G, B, 128, 4, 2, 4).permute(0, 2, 1, 4, 3, 5).reshape(m_out, n_in // 2)     # [g, r, b, s, q, j]
    scales = img[..., 4096:].reshape(G, B, 128, 2).permute(0, 2, 1, 3).reshape(m_out, n_in // 32)
    return Mxfp4Weight(codes.contiguous(), scales.contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# MXINT8 head states of the prefix-state arena (include/chirrup_amd.h: rwkv7_state_pack; DESIGN.md "MXINT8 prefix-state arena")

MXINT8_BLOCK = 32
MXINT8_E_MIN, MXINT8_E_MAX = -18, 15             # 2^(e-6) times a code of -127..127 is +-0 or a binary16 number
MXINT8_HEAD_ELEMS = 64 * 64
MXINT8_HEAD_BYTES = MXINT8_HEAD_ELEMS + MXINT8_HEAD_ELEMS // MXINT8_BLOCK     # 4096 codes, then 128 scale bytes
MXINT8_NAN_SCALE = 0xFF


def mxint8_block_exponent(amax16: torch.Tensor) -> torch.Tensor:
    """Block exponents (int32) of non-negative finite binary16 block maxima: the smallest e with amax <= 127 * 2^(e-6), held to
    [-18, 15].  From the bits alone: binary32 holds every binary16 value exactly and normalised, amax = f * 2^p with 1 <= f < 2, and
    f <= 127/64 is a comparison of the 23 fraction bits with 63/64.  An all-zero block takes -18."""
    b = amax16.to(torch.float16).to(torch.float32).view(torch.int32)
    e = (b >> 23) - 127 + ((b & 0x7FFFFF) > 0x7E0000).to(torch.int32)
    return torch.where(b == 0, torch.full_like(e, MXINT8_E_MIN), e).clamp(MXINT8_E_MIN, MXINT8_E_MAX)


def pack_state_mxint8(wkv: torch.Tensor) -> torch.Tensor:
    """Head states binary16 [..., 64, 64] -> uint8 [..., 4224]: per head 4096 int8 codes in element order, then 128 E8M0 scale bytes,
    one per block of 32 consecutive elements.  scale byte = e + 127 (mxint8_block_exponent); code = clamp(RNE(x * 2^(6-e)), -127,
    127) in two's complement (-128 is never written, -0 gives 0).  A block with a NaN or an infinity: scale byte 0xFF, codes 0.
    Deterministic and exact (the scaling is by a power of two, the rounding torch.round's ties-to-even); on the tensor's device."""
    if wkv.dtype != torch.float16 or wkv.dim() < 2 or tuple(wkv.shape[-2:]) != (64, 64):
        raise ValueError(f"pack_state_mxint8: expected binary16 [..., 64, 64], got {wkv.dtype} {tuple(wkv.shape)}")
    lead = tuple(wkv.shape[:-2])
    x = wkv.contiguous().reshape(lead + (MXINT8_HEAD_ELEMS // MXINT8_BLOCK, MXINT8_BLOCK))
    mag = (x.view(torch.int16).to(torch.int32) & 0x7FFF).amax(-1)                  # binary16 magnitudes order like their bits
    bad = mag >= 0x7C00
    e = mxint8_block_exponent(torch.where(bad, torch.zeros_like(mag), mag).to(torch.int16).view(torch.float16))
    y = torch.ldexp(x.to(torch.float32), (6 - e).unsqueeze(-1).expand(x.shape))   # exact
    codes = torch.round(y).clamp(-127, 127).to(torch.int8)
    codes = torch.where(bad.unsqueeze(-1), torch.zeros_like(codes), codes).view(torch.uint8)
    scales = torch.where(bad, torch.full_like(e, MXINT8_NAN_SCALE), e + 127).to(torch.uint8)
    return torch.cat([codes.reshape(lead + (MXINT8_HEAD_ELEMS,)), scales], -1).contiguous()


def unpack_state_mxint8(packed: torch.Tensor) -> torch.Tensor:
    """uint8 [..., 4224] -> binary16 [..., 64, 64]: code * 2^(scale - 133), which is +-0 or a binary16 number for every code and every
    scale byte 109..142 -- nothing is rounded.  Scale byte 0xFF gives 32 quiet NaNs (0x7E00); other bytes are held to 109..142."""
    if packed.dtype != torch.uint8 or packed.dim() < 1 or packed.shape[-1] != MXINT8_HEAD_BYTES:
        raise ValueError(f"unpack_state_mxint8: expected uint8 [..., {MXINT8_HEAD_BYTES}], got {packed.dtype} {tuple(packed.shape)}")
    lead = tuple(packed.shape[:-1])
    nb = MXINT8_HEAD_ELEMS // MXINT8_BLOCK
    codes = packed[..., :MXINT8_HEAD_ELEMS].contiguous().view(torch.int8).reshape(lead + (nb, MXINT8_BLOCK)).to(torch.float32)
    sb = packed[..., MXINT8_HEAD_ELEMS:].to(torch.int32)
    e = sb.clamp(127 + MXINT8_E_MIN, 127 + MXINT8_E_MAX) - 127
    v = torch.ldexp(codes, (e - 6).unsqueeze(-1).expand(codes.shape))
    out = v.to(torch.float16)
    nan = torch.full((), 0x7E00, dtype=torch.int16, device=packed.device).view(torch.float16)
    out = torch.where((sb == MXINT8_NAN_SCALE).unsqueeze(-1), nan, out)
    return out.reshape(lead + (64, 64))


def roundtrip_state_mxint8(wkv: torch.Tensor) -> torch.Tensor:
    """S~ = unpack(pack(S)): what a packed arena hands back for the head states S."""
    return unpack_state_mxint8(pack_state_mxint8(wkv))
