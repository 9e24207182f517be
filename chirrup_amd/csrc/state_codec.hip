// MXINT8 codec of the cached head states (include/chirrup_amd.h: rwkv7_state_pack / rwkv7_state_unpack; DESIGN.md "MXINT8
// prefix-state arena").  A head [64][64] binary16 becomes 4224 bytes: 4096 int8 codes in element order, then 128 E8M0 scale bytes,
// one per block of 32 consecutive elements.  scale byte = e + 127, e the smallest integer in [-18, 15] with amax <= 127 * 2^(e-6);
// code = clamp(RNE(x * 2^(6-e)), -127, 127); value = code * 2^(e-6), always +-0 or a binary16 number.  A block holding a NaN or an
// infinity takes scale byte 0xFF and codes 0 and unpacks to 32 quiet NaNs (0x7E00).
//
// Both kernels are streams: grid (H, L), one workgroup of 256 lanes per head, a lane owns 16 consecutive elements (two 16-byte
// vectors of binary16, one 16-byte vector of codes), so a block is a pair of neighbouring lanes and its amax one cross-lane
// exchange.  No LDS, no scratch.  The exponent comes from the bits of the block's amax, never from a logarithm; every product with
// a power of two is exact in binary32.  Bytes per head: 8192 + 4224.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/chirrup_amd.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;                      // 256 lanes x 16 elements = one head
constexpr int kHeadElems = 64 * 64;
constexpr int kHeadBytes = CHIRRUP_MXINT8_HEAD_BYTES;
constexpr int kEMin = -18, kEMax = 15;

inline bool mis16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

__device__ __forceinline__ float f16_bits(const uint32_t h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)h); }
__device__ __forceinline__ uint32_t bits_f16(const float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }

// the 16 magnitudes (bits 0..14) of a lane's two vectors -> their maximum as an integer: binary16 magnitudes order like their bits,
// and a NaN or an infinity is any value >= 0x7C00
__device__ __forceinline__ uint32_t max_mag(const u32x4 a, const u32x4 b) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        m = max(m, max(a[j] & 0x7FFFu, (a[j] >> 16) & 0x7FFFu));
        m = max(m, max(b[j] & 0x7FFFu, (b[j] >> 16) & 0x7FFFu));
    }
    return m;
}

// amax = f * 2^p with 1 <= f < 2 (binary32 normalises binary16 subnormals, exactly): e = p when f <= 127/64, else p + 1
__device__ __forceinline__ int block_exponent(const uint32_t mag) {
    if (mag == 0) return kEMin;
    const uint32_t b = __float_as_uint(f16_bits(mag));
    const int e = (int)(b >> 23) - 127 + ((b & 0x7FFFFFu) > 0x7E0000u ? 1 : 0);
    return min(max(e, kEMin), kEMax);
}

__device__ __forceinline__ uint32_t code_of(const uint32_t h16, const float up) {
    const float y = rintf(f16_bits(h16) * up);          // exact product, ties to even
    return (uint32_t)(int)fminf(fmaxf(y, -127.0f), 127.0f) & 0xFFu;
}

__device__ __forceinline__ uint32_t codes_of(const uint32_t w0, const uint32_t w1, const float up) {
    return code_of(w0 & 0xFFFFu, up) | (code_of(w0 >> 16, up) << 8) | (code_of(w1 & 0xFFFFu, up) << 16) | (code_of(w1 >> 16, up) << 24);
}

__global__ __launch_bounds__(kThreads) void state_pack_kernel(const int S, const int slot, const u32x4 *__restrict__ wkv,
                                                              uint8_t *__restrict__ packed) {
    const int h = blockIdx.x, l = blockIdx.y, H = gridDim.x, t = threadIdx.x;
    const u32x4 *src = wkv + (((int64_t)l * S + slot) * H + h) * (kHeadElems / 8) + 2 * t;
    uint8_t *dst = packed + ((int64_t)l * H + h) * kHeadBytes;
    const u32x4 a = src[0], b = src[1];
    uint32_t mag = max_mag(a, b);
    mag = max(mag, (uint32_t)__shfl_xor((int)mag, 1));                     // the other half of the block
    const bool bad = mag >= 0x7C00u;
    const int e = block_exponent(mag);
    const float up = __uint_as_float((uint32_t)(133 - e) << 23);           // 2^(6-e)
    u32x4 c;
    c[0] = codes_of(a[0], a[1], up), c[1] = codes_of(a[2], a[3], up), c[2] = codes_of(b[0], b[1], up), c[3] = codes_of(b[2], b[3], up);
    if (bad) c = u32x4{0u, 0u, 0u, 0u};
    reinterpret_cast<u32x4 *>(dst)[t] = c;
    // the scale bytes of a wave's 32 blocks, gathered into two 16-byte stores (lanes 0 and 32)
    uint32_t w = bad ? 0xFFu : (uint32_t)(e + 127);
    w |= (uint32_t)__shfl_down((int)w, 2) << 8;
    w |= (uint32_t)__shfl_down((int)w, 4) << 16;
    u32x4 s;
    s[0] = w, s[1] = (uint32_t)__shfl_down((int)w, 8), s[2] = (uint32_t)__shfl_down((int)w, 16), s[3] = (uint32_t)__shfl_down((int)w, 24);
    if ((t & 31) == 0) reinterpret_cast<u32x4 *>(dst + kHeadElems)[t >> 5] = s;
}

// two codes (bytes lo, lo + 1 of w) -> two binary16 values in one word; the conversion rounds nothing
__device__ __forceinline__ uint32_t pair_of(const uint32_t w, const int lo, const float down) {
    const float x0 = (float)(int)(int8_t)(w >> (8 * lo)) * down, x1 = (float)(int)(int8_t)(w >> (8 * lo + 8)) * down;
    return bits_f16(x0) | (bits_f16(x1) << 16);
}

__global__ __launch_bounds__(kThreads) void state_unpack_kernel(const int S, const int slot, const uint8_t *__restrict__ packed,
                                                                u32x4 *__restrict__ wkv) {
    const int h = blockIdx.x, l = blockIdx.y, H = gridDim.x, t = threadIdx.x;
    const uint8_t *src = packed + ((int64_t)l * H + h) * kHeadBytes;
    u32x4 *dst = wkv + (((int64_t)l * S + slot) * H + h) * (kHeadElems / 8) + 2 * t;
    const u32x4 c = reinterpret_cast<const u32x4 *>(src)[t];
    const uint32_t sb = src[kHeadElems + (t >> 1)];
    u32x4 a, b;
    if (sb == 0xFFu) {
        a = b = u32x4{0x7E007E00u, 0x7E007E00u, 0x7E007E00u, 0x7E007E00u};
    } else {
        const float down = __uint_as_float((min(max(sb, 109u), 142u) - 6u) << 23);      // 2^(e-6), e held to [-18, 15]
        a[0] = pair_of(c[0], 0, down), a[1] = pair_of(c[0], 2, down), a[2] = pair_of(c[1], 0, down), a[3] = pair_of(c[1], 2, down);
        b[0] = pair_of(c[2], 0, down), b[1] = pair_of(c[2], 2, down), b[2] = pair_of(c[3], 0, down), b[3] = pair_of(c[3], 2, down);
    }
    dst[0] = a, dst[1] = b;
}

int check(int L, int S, int H, int slot, const void *wkv, const void *packed) {
    if (L <= 0 || L > 65535 || S <= 0 || H <= 0 || H > (1 << 14) || slot < 0 || slot >= S) return CHIRRUP_E_SHAPE;
    if (!wkv || !packed) return CHIRRUP_E_NULL;
    if (mis16(wkv) || mis16(packed)) return CHIRRUP_E_ALIGN;
    return 0;
}

}  // namespace

extern "C" int rwkv7_state_pack(int L, int S, int H, int slot, const void *wkv, void *packed, void *stream) {
    if (const int rc = check(L, S, H, slot, wkv, packed)) return rc;
    hipLaunchKernelGGL(state_pack_kernel, dim3((unsigned)H, (unsigned)L), dim3(kThreads), 0, static_cast<hipStream_t>(stream), S, slot,
                       static_cast<const u32x4 *>(wkv), static_cast<uint8_t *>(packed));
    return (int)hipGetLastError();
}

extern "C" int rwkv7_state_unpack(int L, int S, int H, int slot, const void *packed, void *wkv, void *stream) {
    if (const int rc = check(L, S, H, slot, wkv, packed)) return rc;
    hipLaunchKernelGGL(state_unpack_kernel, dim3((unsigned)H, (unsigned)L), dim3(kThreads), 0, static_cast<hipStream_t>(stream), S, slot,
                       static_cast<const uint8_t *>(packed), static_cast<u32x4 *>(wkv));
    return (int)hipGetLastError();
}
