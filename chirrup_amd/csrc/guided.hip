// Guided decoding: per-slot finite automata over the vocabulary's bytes (include/chirrup_amd.h: rwkv7_guide_*).
//
// All guides of a worker live in one pool of global state rows: guide_next [P][256] int32 (absolute pool rows, -1 dead) and
// guide_allow [P][V/32] uint32 (bit t of a row: token t keeps a completion possible).  A slot's constraint is guide_state[slot]:
// an absolute row, or -1 for an unconstrained slot.
//   build   : fills the bitmap rows of one new guide -- one lane per (state, token) walks the token's bytes; the 64 decisions
//             of a wave leave through a ballot and one 8-byte vector store
//   apply   : logits of the listed rows -> -inf where the slot's state forbids the token (before the penalty / arg-max kernel)
//   advance : the sampled id's bytes move the slot's state (behind commit_sampled, no host round trip)
// None of this is in the sampler's kernels: a step without a guided row launches nothing here.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/chirrup_amd.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBuildThreads = 256;
constexpr int kApplyThreads = 256;
constexpr int kAdvanceThreads = 64;
constexpr uint32_t kNegInfPair = 0xFC00FC00u;      // two binary16 -inf

// The row after walking bytes [b0, b1) from `st`, or -1 once the walk has died (a row outside the pool counts as dead).
__device__ __forceinline__ int walk_bytes(int st, const int b0, const int b1, const uint8_t *__restrict__ tok_bytes,
                                          const int32_t *__restrict__ guide_next, const int P) {
    for (int i = b0; i < b1; ++i) {
        st = guide_next[(int64_t)st * 256 + tok_bytes[i]];
        if (st < 0 || st >= P) return -1;
    }
    return st;
}

// grid (ceil(V / 256), S): wave w of a workgroup decides tokens [base, base + 64) of state blockIdx.y; V % 64 == 0, so a wave is
// either wholly inside the vocabulary or wholly outside it.
__global__ __launch_bounds__(kBuildThreads) void guide_build_kernel(const int row0, const int P, const int V,
                                                                    const int32_t *__restrict__ guide_next,
                                                                    const int32_t *__restrict__ tok_off,
                                                                    const uint8_t *__restrict__ tok_bytes, const int n_special,
                                                                    const int32_t *__restrict__ special,
                                                                    const uint8_t *__restrict__ accept,
                                                                    uint32_t *__restrict__ guide_allow) {
    const int t = blockIdx.x * kBuildThreads + threadIdx.x;
    if (t >= V) return;                                         // (whole waves: V % 64 == 0)
    const int s = blockIdx.y;
    const int b0 = tok_off[t], b1 = tok_off[t + 1];
    bool ok = b1 > b0 && walk_bytes(row0 + s, b0, b1, tok_bytes, guide_next, P) >= 0;     // ids without an entry: never
    for (int k = 0; k < n_special; ++k)
        if (special[k] == t) ok = accept[s] != 0;               // a stop id ends the text: only where the text may end
    const uint64_t word = __ballot(ok);
    if ((threadIdx.x & 63) == 0)
        *reinterpret_cast<uint64_t *>(guide_allow + (int64_t)(row0 + s) * (V >> 5) + (t >> 5)) = word;
}

// One workgroup per listed row; a lane takes 8 logits (16 bytes) and the byte of the bitmap that covers them.
__global__ __launch_bounds__(kApplyThreads) void guide_apply_kernel(const int n_logit_rows, const int V, const int P,
                                                                    uint32_t *__restrict__ logits, const int32_t *__restrict__ rows,
                                                                    const int32_t *__restrict__ slot_idx, const int n_slots,
                                                                    const int32_t *__restrict__ guide_state,
                                                                    const uint32_t *__restrict__ guide_allow) {
    const int r = rows[blockIdx.x];
    if (r < 0 || r >= n_logit_rows) return;
    const int slot = slot_idx ? slot_idx[r] : r;
    if (slot < 0 || slot >= n_slots) return;
    const int st = guide_state[slot];
    if (st < 0 || st >= P) return;                              // an unconstrained slot
    const uint32_t *allow = guide_allow + (int64_t)st * (V >> 5);
    u32x4 *lg = reinterpret_cast<u32x4 *>(logits + (int64_t)r * (V >> 1));
    const u32x4 all_masked = {kNegInfPair, kNegInfPair, kNegInfPair, kNegInfPair};
    for (int g = threadIdx.x; g < (V >> 3); g += kApplyThreads) {
        const uint32_t bits = (allow[g >> 2] >> ((g & 3) * 8)) & 0xFFu;
        if (bits == 0xFFu) continue;                            // all eight allowed: not even read
        if (bits == 0u) {                                       // none allowed: nothing of the old values survives
            lg[g] = all_masked;
            continue;
        }
        const u32x4 old = lg[g];
        u32x4 v = old;
        for (int k = 0; k < 4; ++k) {
            uint32_t w = v[k];
            if (!((bits >> (2 * k)) & 1u)) w = (w & 0xFFFF0000u) | 0x0000FC00u;
            if (!((bits >> (2 * k + 1)) & 1u)) w = (w & 0x0000FFFFu) | 0xFC000000u;
            v[k] = w;
        }
        if (v[0] != old[0] || v[1] != old[1] || v[2] != old[2] || v[3] != old[3]) lg[g] = v;
    }
}

// One lane per listed row.
__global__ __launch_bounds__(kAdvanceThreads) void guide_advance_kernel(const int n_rows, const int n_ids, const int V, const int P,
                                                                        const int32_t *__restrict__ rows,
                                                                        const int32_t *__restrict__ slot_idx, const int n_slots,
                                                                        const int32_t *__restrict__ ids,
                                                                        const int32_t *__restrict__ tok_off,
                                                                        const uint8_t *__restrict__ tok_bytes,
                                                                        const int32_t *__restrict__ guide_next,
                                                                        int32_t *__restrict__ guide_state) {
    const int i = blockIdx.x * kAdvanceThreads + threadIdx.x;
    if (i >= n_rows) return;
    const int r = rows[i];
    if (r < 0 || r >= n_ids) return;
    const int slot = slot_idx ? slot_idx[r] : r;
    if (slot < 0 || slot >= n_slots) return;
    const int st = guide_state[slot];
    if (st < 0 || st >= P) return;
    const int id = ids[r];
    if (id < 0 || id >= V) return;
    const int b0 = tok_off[id], b1 = tok_off[id + 1];
    if (b1 <= b0) return;                                       // an id the vocabulary does not define
    const int nxt = walk_bytes(st, b0, b1, tok_bytes, guide_next, P);
    if (nxt >= 0) guide_state[slot] = nxt;                      // a dead walk (a stop id, a dropped run-ahead row) leaves the state
}

}  // namespace

extern "C" int rwkv7_guide_build(int S, int row0, int P, int V, const int32_t *guide_next, const int32_t *tok_off,
                                 const uint8_t *tok_bytes, int n_special, const int32_t *special, const uint8_t *accept,
                                 uint32_t *guide_allow, void *stream) {
    if (S < 0 || row0 < 0 || P <= 0 || (int64_t)row0 + S > P || V <= 0 || V % 64 != 0 || n_special < 0 || S > 65535)
        return CHIRRUP_E_SHAPE;
    if (S == 0) return 0;
    if (!guide_next || !tok_off || !tok_bytes || !accept || !guide_allow || (n_special > 0 && !special)) return CHIRRUP_E_NULL;
    if (reinterpret_cast<uintptr_t>(guide_allow) & 7) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(guide_build_kernel, dim3((unsigned)((V + kBuildThreads - 1) / kBuildThreads), (unsigned)S), dim3(kBuildThreads),
                       0, static_cast<hipStream_t>(stream), row0, P, V, guide_next, tok_off, tok_bytes, n_special, special, accept,
                       guide_allow);
    return (int)hipGetLastError();
}

extern "C" int rwkv7_guide_apply(int n_rows, int n_logit_rows, int V, int P, void *logits, const int32_t *rows,
                                 const int32_t *slot_idx, int n_slots, const int32_t *guide_state, const uint32_t *guide_allow,
                                 void *stream) {
    if (n_rows < 0 || n_logit_rows < 0 || V <= 0 || V % 32 != 0 || P <= 0 || n_slots <= 0) return CHIRRUP_E_SHAPE;
    if (n_rows == 0) return 0;
    if (!logits || !rows || !guide_state || !guide_allow) return CHIRRUP_E_NULL;
    if (reinterpret_cast<uintptr_t>(logits) & 15) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(guide_apply_kernel, dim3((unsigned)n_rows), dim3(kApplyThreads), 0, static_cast<hipStream_t>(stream),
                       n_logit_rows, V, P, static_cast<uint32_t *>(logits), rows, slot_idx, n_slots, guide_state, guide_allow);
    return (int)hipGetLastError();
}

extern "C" int rwkv7_guide_advance(int n_rows, int n_ids, int V, int P, const int32_t *rows, const int32_t *slot_idx, int n_slots,
                                   const int32_t *ids, const int32_t *tok_off, const uint8_t *tok_bytes, const int32_t *guide_next,
                                   int32_t *guide_state, void *stream) {
    if (n_rows < 0 || n_ids < 0 || V <= 0 || P <= 0 || n_slots <= 0) return CHIRRUP_E_SHAPE;
    if (n_rows == 0) return 0;
    if (!rows || !ids || !tok_off || !tok_bytes || !guide_next || !guide_state) return CHIRRUP_E_NULL;
    hipLaunchKernelGGL(guide_advance_kernel, dim3((unsigned)((n_rows + kAdvanceThreads - 1) / kAdvanceThreads)), dim3(kAdvanceThreads),
                       0, static_cast<hipStream_t>(stream), n_rows, n_ids, V, P, rows, slot_idx, n_slots, ids, tok_off, tok_bytes,
                       guide_next, guide_state);
    return (int)hipGetLastError();
}
