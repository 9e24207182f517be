// Beam search: device-side selection of the next beams and the state copies it asks for (include/chirrup_amd.h: rwkv7_beam_*;
// DESIGN.md "Beam search").
//
//   select : one wave per beam group.  The W x K candidates (cum = score[b] + lp, one binary32 addition) are ranked by counting, for
//            each candidate, the candidates that beat it under the strict total order (cum descending, b ascending, k ascending): the
//            ranks are a permutation of 0..N-1 whatever the lanes' schedule -- no atomics, no sort network.  Lane 0 then walks the
//            ranked list (at most 160 entries, normally W + a few) and places the next beams.  Everything that is indexed at run time
//            lives in LDS, so the kernel has no scratch.
//   copy   : grid (pieces of a layer, L, beam positions) like fork_states_kernel, but the source slot of a position is read from the
//            table the select kernel wrote: the host learns the parents one step late.  -1 (or anything out of range) returns at once.
// Neither is in the captured decode graphs; a step without a beam row launches nothing here.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/chirrup_amd.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxW = CHIRRUP_BEAM_MAX_W;               // 8
constexpr int kMaxK = 20;                               // W + S <= 20 (the top-K of rwkv7_token_logprobs)
constexpr int kMaxCand = kMaxW * kMaxK;                 // 160
constexpr int kMaxStops = 18;
constexpr int kDesc = CHIRRUP_BEAM_DESC_WORDS, kOut = CHIRRUP_BEAM_OUT_WORDS;
// words of a group's descriptor and of its output record
constexpr int kDescLpRow = 2, kDescOutRow = 10, kDescSlot = 18, kDescStop = 26;
constexpr int kOutParent = 0, kOutRank = 8, kOutCopy = 16, kOutId = 24, kOutScore = 32, kOutNFin = 40, kOutFinParent = 41,
              kOutFinId = 49, kOutFinCum = 57;
constexpr int kSelectThreads = 64;

__device__ __forceinline__ float neg_inf() { return __uint_as_float(0xFF800000u); }

// a beats b: cum descending, then the flat index b * K + k ascending (b ascending, then k ascending)
__device__ __forceinline__ bool beats(const float ca, const int ia, const float cb, const int ib) {
    return ca > cb || (ca == cb && ia < ib);
}

__global__ __launch_bounds__(kSelectThreads) void beam_select_kernel(const int n_lp_rows, const int k_cols, const float *__restrict__ lp,
                                                                    const int64_t lp_stride, const int32_t *__restrict__ cand_ids,
                                                                    const int64_t ids_stride, const int32_t *__restrict__ desc,
                                                                    float *__restrict__ scores, const int n_slots,
                                                                    int32_t *__restrict__ ids_out, const int n_ids,
                                                                    int32_t *__restrict__ out) {
    __shared__ float s_cum[kMaxCand];
    __shared__ int32_t s_id[kMaxCand];
    __shared__ int32_t s_stop[kMaxCand];                // 1: the candidate's id is a stop token of the group
    __shared__ int32_t s_order[kMaxCand];               // s_order[rank] = flat candidate index
    __shared__ int32_t s_desc[kDesc];
    __shared__ int32_t s_par[kMaxW], s_place[kMaxW], s_has[kMaxW], s_taken[kMaxW], s_cid[kMaxW];
    __shared__ float s_ccum[kMaxW], s_new[kMaxW];
    __shared__ int32_t s_newid[kMaxW], s_live[kMaxW];   // the id of a position's next beam; whether it has one
    __shared__ int32_t s_ok;

    const int g = blockIdx.x, lane = threadIdx.x;
    if (lane < kDesc) s_desc[lane] = desc[(int64_t)g * kDesc + lane];
    __syncthreads();
    const int W = s_desc[0], S = s_desc[1], K = W + S;
    if (lane == 0) {
        bool ok = W >= 2 && W <= kMaxW && S >= 1 && S <= kMaxStops && K <= kMaxK && K <= k_cols;
        for (int p = 0; ok && p < W; ++p) {
            const int r = s_desc[kDescLpRow + p], o = s_desc[kDescOutRow + p], s = s_desc[kDescSlot + p];
            ok = r >= 0 && r < n_lp_rows && o >= 0 && o < n_ids && s >= 0 && s < n_slots;
        }
        s_ok = ok;
    }
    __syncthreads();
    if (!s_ok) return;                                  // a malformed group writes nothing
    const int N = W * K;

    // candidates: the old scores are read here, by every lane that needs one, before anything is written
    for (int c = lane; c < N; c += kSelectThreads) {
        const int b = c / K, k = c - b * K;
        const int64_t row = s_desc[kDescLpRow + b];
        float cum = scores[s_desc[kDescSlot + b]] + lp[row * lp_stride + k];
        if (cum != cum) cum = neg_inf();                // a NaN orders as -inf: it becomes -inf
        const int id = cand_ids[row * ids_stride + k];
        int stop = 0;
        for (int j = 0; j < S; ++j) stop |= (s_desc[kDescStop + j] == id);
        s_cum[c] = cum;
        s_id[c] = id;
        s_stop[c] = stop;
    }
    __syncthreads();
    for (int c = lane; c < N; c += kSelectThreads) {
        const float cc = s_cum[c];
        int rank = 0;
        for (int o = 0; o < N; ++o) rank += beats(s_cum[o], o, cc, c) ? 1 : 0;
        s_order[rank] = c;
    }
    __syncthreads();
    if (lane != 0) return;

    int32_t *rec = out + (int64_t)g * kOut;
    int n_next = 0, n_fin = 0;
    for (int pos = 0; pos < N && n_next < W; ++pos) {   // the walk
        const int c = s_order[pos];
        const float cum = s_cum[c];
        if (s_stop[c]) {
            if (pos < W && cum - cum == 0.0f) {         // finite
                rec[kOutFinParent + n_fin] = c / K;
                rec[kOutFinId + n_fin] = s_id[c];
                rec[kOutFinCum + n_fin] = (int32_t)__float_as_uint(cum);
                ++n_fin;
            }
            continue;
        }
        s_par[n_next] = c / K;
        s_cid[n_next] = s_id[c];
        s_ccum[n_next] = cum;
        ++n_next;
    }
    rec[kOutNFin] = n_fin;
    for (int j = n_fin; j < kMaxW; ++j) {
        rec[kOutFinParent + j] = -1;
        rec[kOutFinId + j] = -1;
        rec[kOutFinCum + j] = 0;
    }
    // placement: the first chosen child of a parent stays in the parent's position; the others take the lowest positions whose old
    // beam has no chosen child
    for (int p = 0; p < W; ++p) s_has[p] = s_taken[p] = 0;
    for (int r = 0; r < n_next; ++r) {
        const int b = s_par[r];
        s_place[r] = s_has[b] ? -1 : b;
        s_has[b] = 1;
    }
    for (int p = 0; p < kMaxW; ++p) {
        rec[kOutParent + p] = -1;
        rec[kOutRank + p] = -1;
        rec[kOutCopy + p] = -1;
        rec[kOutId + p] = -1;
        rec[kOutScore + p] = (int32_t)0xFF800000u;
        s_new[p] = neg_inf();
        s_newid[p] = -1;
        s_live[p] = 0;
    }
    for (int r = 0; r < n_next; ++r) {
        int q = s_place[r], copy = -1;
        if (q < 0) {
            for (q = 0; q < W && (s_has[q] || s_taken[q]); ++q) {}
            if (q >= W) continue;                       // cannot happen: n_next <= W children over W positions
            s_taken[q] = 1;
            copy = s_desc[kDescSlot + s_par[r]];
        }
        rec[kOutParent + q] = s_par[r];
        rec[kOutRank + q] = r;
        rec[kOutCopy + q] = copy;
        rec[kOutId + q] = s_cid[r];
        rec[kOutScore + q] = (int32_t)__float_as_uint(s_ccum[r]);
        s_new[q] = s_ccum[r];
        s_newid[q] = s_cid[r];
        s_live[q] = 1;
    }
    // the sampler's ids and the score table: a position without a next beam (fewer than W candidates were left; the walk's proof
    // excludes it for K = W + S) gets a score of -inf and keeps its id
    for (int p = 0; p < W; ++p) {
        if (s_live[p]) ids_out[s_desc[kDescOutRow + p]] = s_newid[p];
        scores[s_desc[kDescSlot + p]] = s_new[p];
    }
}

constexpr int kCopyThreads = 256, kCopyVec = 4;

// the 16-byte vector u of slot `slot` in layer l: the WKV rows first, then the two shift rows (as fork_states_kernel lays a layer out)
__device__ __forceinline__ u32x4 *state_vec(u32x4 *shift, u32x4 *wkv, const int l, const int S, const int C, const int slot, const int u) {
    const int Wv = C * 8;                               // H x 64 x 64 x 2 B / 16 B
    if (u < Wv) return wkv + ((int64_t)l * S + slot) * Wv + u;
    const int R = C >> 3, v = u - Wv, r = v >= R;
    return shift + (((int64_t)l * 2 + r) * S + slot) * R + (v - r * R);
}

__global__ __launch_bounds__(kCopyThreads) void beam_copy_states_kernel(const int S, const int C, const int32_t *__restrict__ copy_src,
                                                                        const int64_t group_stride, const int32_t *__restrict__ dst,
                                                                        u32x4 *__restrict__ shift, u32x4 *__restrict__ wkv,
                                                                        int32_t *__restrict__ elapsed) {
    const int z = blockIdx.z, l = blockIdx.y;
    const int s = copy_src[(int64_t)(z / kMaxW) * group_stride + (z % kMaxW)], d = dst[z];
    if (s < 0 || s >= S || d < 0 || d >= S || s == d) return;
    if (blockIdx.x == 0 && l == 0 && threadIdx.x == 0) elapsed[d] = elapsed[s];
    const int total = C * 8 + (C >> 2);
    const int base = blockIdx.x * (kCopyThreads * kCopyVec) + threadIdx.x;
    u32x4 v[kCopyVec];
#pragma unroll
    for (int k = 0; k < kCopyVec; k++) {
        const int u = base + k * kCopyThreads;
        if (u < total) v[k] = *state_vec(shift, wkv, l, S, C, s, u);
    }
#pragma unroll
    for (int k = 0; k < kCopyVec; k++) {
        const int u = base + k * kCopyThreads;
        if (u < total) *state_vec(shift, wkv, l, S, C, d, u) = v[k];
    }
}

}  // namespace

extern "C" int rwkv7_beam_select(int n_groups, int n_lp_rows, int k_cols, const float *lp, int64_t lp_stride, const int32_t *cand_ids,
                                 int64_t ids_stride, const int32_t *desc, float *scores, int n_slots, int32_t *ids_out, int n_ids,
                                 int32_t *out, void *stream) {
    if (n_groups < 0) return CHIRRUP_E_SHAPE;
    if (n_groups == 0) return 0;
    if (n_groups > 65535 || n_lp_rows <= 0 || k_cols < 3 || k_cols > kMaxK || lp_stride < k_cols || ids_stride < k_cols || n_slots <= 0 ||
        n_ids <= 0)
        return CHIRRUP_E_SHAPE;
    if (!lp || !cand_ids || !desc || !scores || !ids_out || !out) return CHIRRUP_E_NULL;
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)n_groups), dim3(kSelectThreads), 0, static_cast<hipStream_t>(stream), n_lp_rows,
                       k_cols, lp, lp_stride, cand_ids, ids_stride, desc, scores, n_slots, ids_out, n_ids, out);
    return (int)hipGetLastError();
}

extern "C" int rwkv7_beam_copy_states(int n_groups, int L, int S, int C, int H, const int32_t *copy_src, int64_t group_stride,
                                      const int32_t *dst, void *shift, void *wkv, int32_t *elapsed, void *stream) {
    if (n_groups < 0) return CHIRRUP_E_SHAPE;
    if (n_groups == 0) return 0;
    if (n_groups > 65535 / kMaxW || L <= 0 || L > 65535 || S <= 0 || H <= 0 || C != H * 64 || C > (1 << 20) || group_stride < kMaxW)
        return CHIRRUP_E_SHAPE;
    if (!copy_src || !dst || !shift || !wkv || !elapsed) return CHIRRUP_E_NULL;
    if ((reinterpret_cast<uintptr_t>(shift) & 15) || (reinterpret_cast<uintptr_t>(wkv) & 15) || (reinterpret_cast<uintptr_t>(elapsed) & 3))
        return CHIRRUP_E_ALIGN;
    const int per_wg = kCopyThreads * kCopyVec;
    const unsigned pieces = (unsigned)((C * 8 + (C >> 2) + per_wg - 1) / per_wg);
    hipLaunchKernelGGL(beam_copy_states_kernel, dim3(pieces, (unsigned)L, (unsigned)(n_groups * kMaxW)), dim3(kCopyThreads), 0,
                       static_cast<hipStream_t>(stream), S, C, copy_src, group_stride, dst, static_cast<u32x4 *>(shift),
                       static_cast<u32x4 *>(wkv), elapsed);
    return (int)hipGetLastError();
}
