// MXFP4 (w4a16) weights: OCP Microscaling FP4 -- 32 E2M1 codes along K share one E8M0 power-of-two scale, 4.25 bits per weight.
//
//   w~[n][k] = E2M1(code[n][k]) * 2^(scale[n][k / 32] - 127),   E2M1: bit 3 sign, codes 0..7 -> 0, .5, 1, 1.5, 2, 3, 4, 6
//
// The host only hands over scale bytes 114..140 (exponents -13..13): every w~ is then +-0 or a NORMAL binary16 number, the
// conversion v_cvt_scalef32_pk_f16_fp4 (one byte -> two scaled halves) is exact, and the product is DEFINED as the binary16 GEMM
// of the dequantised matrix: exact products, binary32 accumulation, one rounding to binary16 after the optional relu^2.
//
// Tile image (mxfp4_tile_weight): tile (g = n / 128, b = k / 64) is 4352 consecutive bytes at ((g * K / 64) + b) * 4352:
//   [0, 4096)     codes: row r (n = 128 g + r) has 32 bytes at 32 r; byte position 8 q + 4 s + j (q 0..3, s 0..1, j 0..3) holds
//                 k = 64 b + 32 s + 8 q + 2 j (low nibble) and + 1 (high nibble).  Lane (c, q) of v_mfma_f32_16x16x32_f16 supplies
//                 A[n = c][k = 8 q .. 8 q + 7] of k-step s: its codes for BOTH k-steps of a K-block are the 8 bytes at 32 r + 8 q, and
//                 the 64 lanes of a wave read 512 consecutive bytes per 16-row tile.
//   [4096, 4352)  scales: byte 2 r + s is the E8M0 scale of row r, k-step s.
//
// mxfp4_gemm_kernel (1..256 rows of x): one workgroup of 4 waves per 128-row tile column and K-slice; a wave owns 32 rows of W as
// two 16-row tiles.  W goes global -> registers (8 + 2 bytes per lane, tile and K-block; streamed once, non-temporal), one
// K-block ahead, and is dequantised in registers between that read and the MFMA (4 conversions per fragment, no binary32
// multiply per weight); x goes through a double-buffered LDS image, XOR-swizzled like the ring GEMM's (conflict-free
// ds_read_b128).  A = W tile (16 n x 32 k), B = x^T (32 k x 16 m): lane (c, q) receives D[n = 4 q + i][m = c].
// Split-K over blockIdx.y: binary32 planes, summed in plane order by mxfp4_reduce_kernel or by the consumer (rwkv7_add_ln_mix,
// delta_partials).  Measured together and not adopted (profiles/r09_mxfp4.txt, section C): W four K-blocks ahead in a register
// ring plus two workgroups per tile from 128 rows on, one per half of the rows -- slower at every row count.
// The existing kernels are untouched: this is a translation unit of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/chirrup_amd.h"

namespace {

typedef _Float16 f16;
typedef f16 f16x2 __attribute__((ext_vector_type(2)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kKB = 64;            // K-block
constexpr int kTileRows = 128;     // rows of one tile image
constexpr int kCodeBytes = kTileRows * kKB / 2;
constexpr int kTileBytes = kCodeBytes + kTileRows * 2;      // 4352
constexpr int kMaxSplits = 64;

// E8M0 byte -> 2^(e - 127) (a normal binary32 number for every byte the host lets through)
__device__ __forceinline__ float scale_of(const uint32_t e8) { return __builtin_bit_cast(float, e8 << 23); }

// four bytes = eight codes in k order (low nibble first) -> eight binary16 values code * scale
__device__ __forceinline__ f16x8 dequant8(const uint32_t codes, const float scale) {
    const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(codes, scale, 0);
    const f16x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(codes, scale, 1);
    const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(codes, scale, 2);
    const f16x2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(codes, scale, 3);
    return (f16x8){a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

__device__ __forceinline__ float relu_sq(float v) {
    v = (float)(f16)v;                                 // relu(fp16(y))**2, as skinny_gemm.hip's apply_act
    return v <= 0.f ? 0.f : v * v;                     // (a NaN stays a NaN, as torch.relu keeps it)
}

// row-major codes [M_out][N_in / 2] (low nibble = even k) and scales [M_out][N_in / 32] -> tile images; one workgroup per tile
__global__ __launch_bounds__(256) void mxfp4_tile_kernel(const int K, const uint8_t *__restrict__ codes, const int64_t ldc,
                                                         const uint8_t *__restrict__ scales, const int64_t lds, uint8_t *__restrict__ out) {
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    uint8_t *dst = out + ((int64_t)g * (K / kKB) + b) * kTileBytes;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int d = i * 256 + tid;                   // dword of the code image: row r, position (q, s)
        const int r = d >> 3, q = (d >> 1) & 3, s = d & 1;
        const uint8_t *src = codes + (int64_t)(g * kTileRows + r) * ldc + b * 32 + 16 * s + 4 * q;
        *reinterpret_cast<uint32_t *>(dst + d * 4) = *reinterpret_cast<const uint32_t *>(src);
    }
    dst[kCodeBytes + tid] = scales[(int64_t)(g * kTileRows + (tid >> 1)) * lds + b * 2 + (tid & 1)];
}

// tile images -> binary16 [M_out][N_in] (row stride ldo); one workgroup per tile, a thread per (row, k-step): 32 values, 64 bytes
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(const int K, const uint8_t *__restrict__ wt, f16 *__restrict__ out, const int64_t ldo) {
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int r = tid >> 1, s = tid & 1;
    const uint8_t *tile = wt + ((int64_t)g * (K / kKB) + b) * kTileBytes;
    const float scale = scale_of(tile[kCodeBytes + tid]);
    f16 *dst = out + (int64_t)(g * kTileRows + r) * ldo + b * kKB + 32 * s;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t c = *reinterpret_cast<const uint32_t *>(tile + r * 32 + q * 8 + s * 4);
        *reinterpret_cast<f16x8 *>(dst + 8 * q) = dequant8(c, scale);
    }
}

template <int MT>
__global__ __launch_bounds__(256) void mxfp4_gemm_kernel(const int M, const int N, const int K, const int kb_per_slice,
                                                         const f16 *__restrict__ X, const int ldx, const uint8_t *__restrict__ Wt,
                                                         f16 *__restrict__ Y, const int ldy, float *__restrict__ part, const int act) {
    constexpr int kXBytes = MT * 16 * 128;             // one K-block of x: MT * 16 rows x 128 B
    constexpr int kXRounds = (MT * 128 + 255) / 256;   // 16-byte chunks per thread
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kXBytes];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int ng = blockIdx.x, kslice = blockIdx.y;
    const int kb0 = kslice * kb_per_slice, nkb = kb_per_slice;
    // this lane's bytes of the first tile image: codes of rows wave * 32 + 16 nt + c at 8 q, their two scales
    const uint8_t *wlane = Wt + ((int64_t)ng * (K / kKB) + kb0) * kTileBytes;
    const int code_off = (wave * 32 + c) * 32 + q * 8, scale_off = kCodeBytes + (wave * 32 + c) * 2;

    u32x4 xr[kXRounds];
    auto load_x = [&](const int kb) {
#pragma unroll
        for (int i = 0; i < kXRounds; i++) {
            const int e = i * 256 + tid, row = e >> 3, ch = e & 7;
            xr[i] = (u32x4){0u, 0u, 0u, 0u};
            if (row < M) xr[i] = *reinterpret_cast<const u32x4 *>(X + (int64_t)row * ldx + kb * kKB + ch * 8);
        }
    };
    auto store_x = [&](unsigned char *buf) {
#pragma unroll
        for (int i = 0; i < kXRounds; i++) {
            const int e = i * 256 + tid, row = e >> 3, ch = e & 7;
            if (e < MT * 128) *reinterpret_cast<u32x4 *>(buf + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)) = xr[i];
        }
    };
    u32x2 wc[2];
    uint32_t wsc[2];
    auto load_w = [&](const int i) {                   // K-block i of this slice
        const uint8_t *t = wlane + (int64_t)i * kTileBytes;
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            wc[nt] = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(t + code_off + nt * 512));
            wsc[nt] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(t + scale_off + nt * 32));
        }
    };

    f32x4 acc[2][MT];
#pragma unroll
    for (int nt = 0; nt < 2; nt++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    load_x(kb0);
    load_w(0);
    store_x(smem);
    __syncthreads();
    for (int i = 0; i < nkb; i++) {
        const unsigned char *xt = smem + (i & 1) * kXBytes;
        f16x8 wf[2][2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++) wf[nt][ks] = dequant8(wc[nt][ks], scale_of((wsc[nt] >> (8 * ks)) & 0xffu));
        const bool more = i + 1 < nkb;
        if (more) {
            load_x(kb0 + i + 1);
            load_w(i + 1);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int m = mt * 16 + c;
                const f16x8 xf = *reinterpret_cast<const f16x8 *>(xt + m * 128 + (((4 * ks + q) ^ ((m >> 1) & 7)) << 4));
#pragma unroll
                for (int nt = 0; nt < 2; nt++) acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt][ks], xf, acc[nt][mt], 0, 0, 0);
            }
        }
        if (more) store_x(smem + ((i + 1) & 1) * kXBytes);
        __syncthreads();
    }

    // lane (c, q): D[n = 4 q + e][m = c] -> four consecutive columns of output row m
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const int m = mt * 16 + c;
        if (m >= M) continue;
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            const int n = ng * kTileRows + wave * 32 + nt * 16 + 4 * q;
            const f32x4 v = acc[nt][mt];
            if (part) {
                *reinterpret_cast<f32x4 *>(part + ((int64_t)kslice * M + m) * N + n) = v;
            } else {
                f16x4 o;
#pragma unroll
                for (int e = 0; e < 4; e++) o[e] = (f16)(act == 1 ? relu_sq(v[e]) : v[e]);
                *reinterpret_cast<f16x4 *>(Y + (int64_t)m * ldy + n) = o;
            }
        }
    }
}

// Y = act(sum of the planes, in plane order), four columns per thread
__global__ __launch_bounds__(256) void mxfp4_reduce_kernel(const int M, const int N, const int splits, const float *__restrict__ part,
                                                           f16 *__restrict__ Y, const int ldy, const int act) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (int64_t)M * N / 4) return;
    const int m = (int)(gi / (N / 4)), n = (int)(gi % (N / 4)) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < splits; i++) s += __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(part + ((int64_t)i * M + m) * N + n));
    f16x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = (f16)(act == 1 ? relu_sq(s[e]) : s[e]);
    *reinterpret_cast<f16x4 *>(Y + (int64_t)m * ldy + n) = o;
}

inline bool mis(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// K-slices of a launch: as asked for, cut back to a divisor of the K-block count; 0 = enough workgroups to fill the chip
// (two per CU at few rows, one per CU above 64 rows, where the planes' bytes would pass the weights'), at least 4 K-blocks each
int pick_splits(int M, int N, int K, int splits) {
    const int nkb = K / kKB, tiles = N / kTileRows;
    if (splits > 0) {
        int s = splits < nkb ? splits : nkb;
        if (s > kMaxSplits) s = kMaxSplits;
        while (nkb % s) s--;
        return s;
    }
    int cus = chirrup_device_cu_count();
    if (cus <= 0) cus = 256;
    const int target = M > 64 ? cus : 2 * cus;
    int s = 1;
    while (2 * s <= 16 && tiles * 2 * s <= target && nkb % (2 * s) == 0 && nkb / (2 * s) >= 4) s *= 2;
    return s;
}

template <int MT>
void launch_mt(dim3 grid, hipStream_t st, int M, int N, int K, int kbs, const f16 *X, int ldx, const uint8_t *Wt, f16 *Y, int ldy,
               float *part, int act) {
    hipLaunchKernelGGL(mxfp4_gemm_kernel<MT>, grid, dim3(256), 0, st, M, N, K, kbs, X, ldx, Wt, Y, ldy, part, act);
}

int launch_gemm(int s, hipStream_t st, int M, int N, int K, const f16 *X, int ldx, const uint8_t *Wt, f16 *Y, int ldy, float *part, int act) {
    const dim3 grid(N / kTileRows, s);
    const int kbs = K / kKB / s;
#define MXFP4_CASE(MT) \
    case MT: launch_mt<MT>(grid, st, M, N, K, kbs, X, ldx, Wt, Y, ldy, part, act); break;
    switch ((M + 15) / 16) {
        MXFP4_CASE(1) MXFP4_CASE(2) MXFP4_CASE(3) MXFP4_CASE(4) MXFP4_CASE(5) MXFP4_CASE(6) MXFP4_CASE(7) MXFP4_CASE(8)
        MXFP4_CASE(9) MXFP4_CASE(10) MXFP4_CASE(11) MXFP4_CASE(12) MXFP4_CASE(13) MXFP4_CASE(14) MXFP4_CASE(15) MXFP4_CASE(16)
        default: return CHIRRUP_E_SHAPE;
    }
#undef MXFP4_CASE
    return (int)hipGetLastError();
}

inline int check_gemm(int M, int N, int K, const void *X, int ldx, const void *Wt) {
    if (M <= 0 || M > 256 || N <= 0 || K <= 0 || (N % kTileRows) || (K % kKB) || ldx < K || (ldx & 7) || N / kTileRows > 65535) return CHIRRUP_E_SHAPE;
    if (!X || !Wt) return CHIRRUP_E_NULL;
    if (mis(X, 16) || mis(Wt, 16)) return CHIRRUP_E_ALIGN;
    return 0;
}

}  // namespace

extern "C" int64_t mxfp4_tiled_bytes(int M_out, int N_in) {
    if (M_out <= 0 || N_in <= 0 || (M_out % kTileRows) || (N_in % kKB)) return 0;
    return (int64_t)(M_out / kTileRows) * (N_in / kKB) * kTileBytes;
}

extern "C" int mxfp4_tile_weight(int M_out, int N_in, const void *codes, int64_t ld_codes, const void *scales, int64_t ld_scales,
                                 void *Wt, void *stream) {
    if (M_out <= 0 || N_in <= 0 || (M_out % kTileRows) || (N_in % kKB) || ld_codes < N_in / 2 || (ld_codes & 3) || ld_scales < N_in / 32 ||
        N_in / kKB > 65535)
        return CHIRRUP_E_SHAPE;
    if (!codes || !scales || !Wt) return CHIRRUP_E_NULL;
    if (mis(codes, 4) || mis(Wt, 16)) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(mxfp4_tile_kernel, dim3(M_out / kTileRows, N_in / kKB), dim3(256), 0, static_cast<hipStream_t>(stream), N_in,
                       static_cast<const uint8_t *>(codes), ld_codes, static_cast<const uint8_t *>(scales), ld_scales, static_cast<uint8_t *>(Wt));
    return (int)hipGetLastError();
}

extern "C" int mxfp4_dequant_f16(int M_out, int N_in, const void *Wt, void *out, int64_t ld_out, void *stream) {
    if (M_out <= 0 || N_in <= 0 || (M_out % kTileRows) || (N_in % kKB) || ld_out < N_in || (ld_out & 7) || N_in / kKB > 65535) return CHIRRUP_E_SHAPE;
    if (!Wt || !out) return CHIRRUP_E_NULL;
    if (mis(Wt, 16) || mis(out, 16)) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(mxfp4_dequant_kernel, dim3(M_out / kTileRows, N_in / kKB), dim3(256), 0, static_cast<hipStream_t>(stream), N_in,
                       static_cast<const uint8_t *>(Wt), static_cast<f16 *>(out), ld_out);
    return (int)hipGetLastError();
}

extern "C" int mxfp4_gemm_splits(int M, int N, int K, int splits) {
    if (M <= 0 || M > 256 || N <= 0 || K <= 0 || (N % kTileRows) || (K % kKB) || splits < 0) return 0;
    return pick_splits(M, N, K, splits);
}

extern "C" int64_t mxfp4_gemm_workspace_bytes(int M, int N, int K, int splits) {
    const int s = mxfp4_gemm_splits(M, N, K, splits);
    return s > 1 ? (int64_t)s * M * N * (int64_t)sizeof(float) : 0;
}

extern "C" int mxfp4_gemm(int M, int N, int K, const void *X, int ldx, const void *Wt, void *Y, int ldy, int act, int splits,
                          void *workspace, void *stream) {
    const int bad = check_gemm(M, N, K, X, ldx, Wt);
    if (bad) return bad;
    if (ldy < N || (ldy & 3) || splits < 0) return CHIRRUP_E_SHAPE;
    if (act < 0 || act > 1) return CHIRRUP_E_UNSUPPORTED;
    if (!Y) return CHIRRUP_E_NULL;
    if (mis(Y, 8)) return CHIRRUP_E_ALIGN;
    const int s = pick_splits(M, N, K, splits);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s == 1)
        return launch_gemm(1, st, M, N, K, static_cast<const f16 *>(X), ldx, static_cast<const uint8_t *>(Wt), static_cast<f16 *>(Y), ldy, nullptr, act);
    if (!workspace) return CHIRRUP_E_NULL;
    if (mis(workspace, 16)) return CHIRRUP_E_ALIGN;
    float *part = static_cast<float *>(workspace);
    const int rc = launch_gemm(s, st, M, N, K, static_cast<const f16 *>(X), ldx, static_cast<const uint8_t *>(Wt), nullptr, 0, part, 0);
    if (rc) return rc;
    const int64_t total = (int64_t)M * N / 4;
    hipLaunchKernelGGL(mxfp4_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, M, N, s, part, static_cast<f16 *>(Y), ldy, act);
    return (int)hipGetLastError();
}

extern "C" int mxfp4_gemm_partial(int M, int N, int K, const void *X, int ldx, const void *Wt, int splits, float *partials, void *stream) {
    const int bad = check_gemm(M, N, K, X, ldx, Wt);
    if (bad) return -1000 - bad;
    if (splits < 0) return -1000 - CHIRRUP_E_SHAPE;
    if (!partials) return -1000 - CHIRRUP_E_NULL;
    if (mis(partials, 16)) return -1000 - CHIRRUP_E_ALIGN;
    const int s = pick_splits(M, N, K, splits);
    const int rc = launch_gemm(s, static_cast<hipStream_t>(stream), M, N, K, static_cast<const f16 *>(X), ldx, static_cast<const uint8_t *>(Wt),
                               nullptr, 0, partials, 0);
    return rc ? -1000 - rc : s;
}
