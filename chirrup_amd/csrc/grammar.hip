// Grammar-guided decoding: per-slot call/return automata over the vocabulary's bytes, with the call stack on the device
// (include/chirrup_amd.h: rwkv7_grammar_*; DESIGN.md "Grammar-guided decoding").
//
// The grammar guides of a worker live in a pool of their own: gr_next [P][256] int32 (>= 0 plain edge to an absolute row, -1 no
// move, -(c + 1) call site c), gr_meta [P][8] int32 (a row's own flags / need / guide base / depth bound in words 0..3, and in
// words 4..6 the call-site entry that row carries for its guide: start, after, need; word 7: the guide's stop ids), and the two
// bitmaps gr_allow / gr_maybe [P][V/32].  A slot's constraint is gr_state[slot] (a row, -1 unconstrained) and gr_stack[slot][4]:
// 32 call-site bytes, the top in the low byte of word 0, zero above the bottom.  In the kernels the stack is four 64-bit
// registers shifted as one 256-bit register: no indexed local array, no scratch.
//   build   : one lane per (state, token); a wave's 64 decisions leave through two ballots and two 8-byte stores
//   apply   : one workgroup per listed row; a token is allowed by its allow bit, or by its maybe bit and a full walk
//   advance : one lane per listed row; the sampled id's bytes move state and stack, a dying walk leaves both
//   reset   : start row (or -1) and the empty stack for a list of slots
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/chirrup_amd.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBuildThreads = 256;
constexpr int kApplyThreads = 256;
constexpr int kLaneThreads = 64;
constexpr uint32_t kNegInfPair = 0xFC00FC00u;      // two binary16 -inf
constexpr int kDepthMax = CHIRRUP_GRAMMAR_STACK_DEPTH;
constexpr int kMovesPerByte = 2 * kDepthMax + 2;   // returns, then calls, then the plain edge

enum { M_FLAGS = 0, M_NEED = 1, M_BASE = 2, M_DEPTH = 3, M_SITE_START = 4, M_SITE_AFTER = 5, M_SITE_NEED = 6, M_STOP = 7 };
constexpr int kFinal = 1, kCalled = 2;

struct Stack {
    uint64_t w0, w1, w2, w3;
};

__device__ __forceinline__ void push(Stack &s, const uint32_t c) {
    s.w3 = (s.w3 << 8) | (s.w2 >> 56);
    s.w2 = (s.w2 << 8) | (s.w1 >> 56);
    s.w1 = (s.w1 << 8) | (s.w0 >> 56);
    s.w0 = (s.w0 << 8) | c;
}

__device__ __forceinline__ uint32_t pop(Stack &s) {
    const uint32_t c = (uint32_t)(s.w0 & 0xFFu);
    s.w0 = (s.w0 >> 8) | (s.w1 << 56);
    s.w1 = (s.w1 >> 8) | (s.w2 << 56);
    s.w2 = (s.w2 >> 8) | (s.w3 << 56);
    s.w3 >>= 8;
    return c;
}

__device__ __forceinline__ int bytes_used(const uint64_t w) { return w ? 8 - (__clzll((long long)w) >> 3) : 0; }

__device__ __forceinline__ int depth_of(const Stack &s) {
    return s.w3 ? 24 + bytes_used(s.w3) : s.w2 ? 16 + bytes_used(s.w2) : s.w1 ? 8 + bytes_used(s.w1) : bytes_used(s.w0);
}

// What a guide's rows share, read from the row a walk starts in.
struct Guide {
    int base, depth, P;
    const int32_t *__restrict__ next;
    const int32_t *__restrict__ meta;
};

__device__ __forceinline__ int meta_of(const Guide &g, const int row, const int word) { return g.meta[(int64_t)row * 8 + word]; }

// The row of call site c's entry, or -1 when c is no site of a guide inside the pool.
__device__ __forceinline__ int site_row(const Guide &g, const uint32_t c) {
    const int64_t r = (int64_t)g.base + c;
    return (c >= 1 && c <= CHIRRUP_GRAMMAR_CALL_SITES && r >= 0 && r < g.P) ? (int)r : -1;
}

// Bytes [b0, b1) from (st, sk, d): the row reached, with sk and d moved, or -1 once the walk has died.  Per byte: a plain edge
// consumes it; a call pushes and goes on with the same byte at the called rule's start; a final state of a called rule that has no
// move for the byte returns.  A move that would leave less room under the depth bound than the target needs is refused.
__device__ __forceinline__ int walk_stack(int st, Stack &sk, int &d, const int b0, const int b1, const uint8_t *__restrict__ tok_bytes,
                                          const Guide &g) {
    for (int i = b0; i < b1; ++i) {
        const int byte = tok_bytes[i];
        int moves = 0;
        for (;;) {
            if (++moves > kMovesPerByte) return -1;
            const int v = g.next[(int64_t)st * 256 + byte];
            if (v >= 0) {
                if (v >= g.P || d + meta_of(g, v, M_NEED) > g.depth) return -1;
                st = v;
                break;
            }
            if (v < -1) {
                const uint32_t c = (uint32_t)(-v - 1);
                const int sr = site_row(g, c);
                if (sr < 0 || d >= kDepthMax || d + meta_of(g, sr, M_SITE_NEED) > g.depth) return -1;
                st = meta_of(g, sr, M_SITE_START);
                if (st < 0 || st >= g.P) return -1;
                push(sk, c);
                ++d;
                continue;
            }
            if (d == 0 || (meta_of(g, st, M_FLAGS) & (kFinal | kCalled)) != (kFinal | kCalled)) return -1;
            const int sr = site_row(g, pop(sk));
            --d;
            if (sr < 0) return -1;
            st = meta_of(g, sr, M_SITE_AFTER);
            if (st < 0 || st >= g.P) return -1;
        }
    }
    return st;
}

// Whether the text may end at (st, sk, d): the returns at its end reach a final state with an empty stack.
__device__ __forceinline__ bool ends_here(int st, Stack sk, int d, const Guide &g) {
    while (d > 0 && (meta_of(g, st, M_FLAGS) & (kFinal | kCalled)) == (kFinal | kCalled)) {
        const int sr = site_row(g, pop(sk));
        --d;
        if (sr < 0) return false;
        st = meta_of(g, sr, M_SITE_AFTER);
        if (st < 0 || st >= g.P) return false;
    }
    return d == 0 && (meta_of(g, st, M_FLAGS) & kFinal);
}

__device__ __forceinline__ Guide guide_of(const int st, const int P, const int32_t *__restrict__ gr_next, const int32_t *__restrict__ gr_meta) {
    Guide g;
    g.P = P;
    g.next = gr_next;
    g.meta = gr_meta;
    g.base = gr_meta[(int64_t)st * 8 + M_BASE];
    g.depth = min(gr_meta[(int64_t)st * 8 + M_DEPTH], kDepthMax);
    if (g.base < 0 || g.base >= P) g.depth = -1;        // a row of no guide: every move is refused
    return g;
}

// grid (ceil(V / 256), S): wave w of a workgroup decides tokens [base, base + 64) of state blockIdx.y; V % 64 == 0.
__global__ __launch_bounds__(kBuildThreads) void grammar_build_kernel(const int row0, const int P, const int V,
                                                                      const int32_t *__restrict__ gr_next,
                                                                      const int32_t *__restrict__ gr_meta,
                                                                      const int32_t *__restrict__ tok_off,
                                                                      const uint8_t *__restrict__ tok_bytes, const int n_special,
                                                                      const int32_t *__restrict__ special,
                                                                      uint32_t *__restrict__ gr_allow, uint32_t *__restrict__ gr_maybe) {
    const int t = blockIdx.x * kBuildThreads + threadIdx.x;
    if (t >= V) return;                                         // (whole waves: V % 64 == 0)
    const int s = blockIdx.y;
    const int b0 = tok_off[t], b1 = tok_off[t + 1];
    bool allow = false, maybe = false;
    int st = row0 + s;
    if (b1 > b0) {
        int i = b0;
        for (; i < b1; ++i) {
            const int v = gr_next[(int64_t)st * 256 + tok_bytes[i]];
            if (v >= 0) {
                if (v >= P) break;
                if (gr_meta[(int64_t)v * 8 + M_NEED] != 0) {    // whether the stack has the room decides
                    maybe = true;
                    break;
                }
                st = v;
                continue;
            }
            // a call, or a return from a final state of a called rule: the stack decides
            maybe = v < -1 || (gr_meta[(int64_t)st * 8 + M_FLAGS] & (kFinal | kCalled)) == (kFinal | kCalled);
            break;
        }
        allow = i == b1;
    }
    const int flags = gr_meta[(int64_t)(row0 + s) * 8 + M_FLAGS];
    for (int k = 0; k < n_special; ++k)
        if (special[k] == t) {                                  // a stop id ends the text: only where the text may end
            allow = (flags & (kFinal | kCalled)) == kFinal;
            maybe = (flags & (kFinal | kCalled)) == (kFinal | kCalled);
        }
    const uint64_t wa = __ballot(allow), wm = __ballot(maybe);
    if ((threadIdx.x & 63) == 0) {
        const int64_t at = (int64_t)(row0 + s) * (V >> 5) + (t >> 5);
        *reinterpret_cast<uint64_t *>(gr_allow + at) = wa;
        *reinterpret_cast<uint64_t *>(gr_maybe + at) = wm;
    }
}

// One workgroup per listed row; a lane takes 8 logits (16 bytes) and the byte of each bitmap that covers them.
__global__ __launch_bounds__(kApplyThreads) void grammar_apply_kernel(const int n_logit_rows, const int V, const int P,
                                                                      uint32_t *__restrict__ logits, const int32_t *__restrict__ rows,
                                                                      const int32_t *__restrict__ slot_idx, const int n_slots,
                                                                      const int32_t *__restrict__ gr_state,
                                                                      const uint64_t *__restrict__ gr_stack,
                                                                      const int32_t *__restrict__ gr_next,
                                                                      const int32_t *__restrict__ gr_meta,
                                                                      const uint32_t *__restrict__ gr_allow,
                                                                      const uint32_t *__restrict__ gr_maybe,
                                                                      const int32_t *__restrict__ tok_off,
                                                                      const uint8_t *__restrict__ tok_bytes) {
    const int r = rows[blockIdx.x];
    if (r < 0 || r >= n_logit_rows) return;
    const int slot = slot_idx ? slot_idx[r] : r;
    if (slot < 0 || slot >= n_slots) return;
    const int st = gr_state[slot];
    if (st < 0 || st >= P) return;                              // an unconstrained slot
    const Stack sk0 = {gr_stack[(int64_t)slot * 4], gr_stack[(int64_t)slot * 4 + 1], gr_stack[(int64_t)slot * 4 + 2],
                       gr_stack[(int64_t)slot * 4 + 3]};
    const int d0 = depth_of(sk0);
    const Guide g = guide_of(st, P, gr_next, gr_meta);
    const int n_stop = g.depth >= 0 ? min(max(meta_of(g, g.base, M_STOP), 0), P - 1 - g.base) : 0;
    const uint32_t *allow = gr_allow + (int64_t)st * (V >> 5);
    const uint32_t *maybe = gr_maybe + (int64_t)st * (V >> 5);
    u32x4 *lg = reinterpret_cast<u32x4 *>(logits + (int64_t)r * (V >> 1));
    const u32x4 all_masked = {kNegInfPair, kNegInfPair, kNegInfPair, kNegInfPair};
    for (int gq = threadIdx.x; gq < (V >> 3); gq += kApplyThreads) {
        uint32_t bits = (allow[gq >> 2] >> ((gq & 3) * 8)) & 0xFFu;
        uint32_t open = (maybe[gq >> 2] >> ((gq & 3) * 8)) & 0xFFu & ~bits;
        while (open) {                                          // the tokens whose outcome depends on this slot's stack
            const int k = __ffs(open) - 1;
            open &= open - 1;
            const int t = gq * 8 + k;
            bool stop = false;
            for (int j = 0; j < n_stop; ++j) stop |= meta_of(g, g.base + 1 + j, M_STOP) == t;
            bool ok;
            if (stop) {
                ok = ends_here(st, sk0, d0, g);
            } else {
                Stack sk = sk0;
                int d = d0;
                const int b0 = tok_off[t], b1 = tok_off[t + 1];
                ok = b1 > b0 && walk_stack(st, sk, d, b0, b1, tok_bytes, g) >= 0;
            }
            bits |= (uint32_t)ok << k;
        }
        if (bits == 0xFFu) continue;                            // all eight allowed: not even read
        if (bits == 0u) {                                       // none allowed: nothing of the old values survives
            lg[gq] = all_masked;
            continue;
        }
        const u32x4 old = lg[gq];
        u32x4 v = old;
        for (int k = 0; k < 4; ++k) {
            uint32_t w = v[k];
            if (!((bits >> (2 * k)) & 1u)) w = (w & 0xFFFF0000u) | 0x0000FC00u;
            if (!((bits >> (2 * k + 1)) & 1u)) w = (w & 0x0000FFFFu) | 0xFC000000u;
            v[k] = w;
        }
        if (v[0] != old[0] || v[1] != old[1] || v[2] != old[2] || v[3] != old[3]) lg[gq] = v;
    }
}

// One lane per listed row.
__global__ __launch_bounds__(kLaneThreads) void grammar_advance_kernel(const int n_rows, const int n_ids, const int V, const int P,
                                                                       const int32_t *__restrict__ rows,
                                                                       const int32_t *__restrict__ slot_idx, const int n_slots,
                                                                       const int32_t *__restrict__ ids,
                                                                       const int32_t *__restrict__ tok_off,
                                                                       const uint8_t *__restrict__ tok_bytes,
                                                                       const int32_t *__restrict__ gr_next,
                                                                       const int32_t *__restrict__ gr_meta,
                                                                       int32_t *__restrict__ gr_state, uint64_t *__restrict__ gr_stack) {
    const int i = blockIdx.x * kLaneThreads + threadIdx.x;
    if (i >= n_rows) return;
    const int r = rows[i];
    if (r < 0 || r >= n_ids) return;
    const int slot = slot_idx ? slot_idx[r] : r;
    if (slot < 0 || slot >= n_slots) return;
    const int st = gr_state[slot];
    if (st < 0 || st >= P) return;
    const int id = ids[r];
    if (id < 0 || id >= V) return;
    const int b0 = tok_off[id], b1 = tok_off[id + 1];
    if (b1 <= b0) return;                                       // an id the vocabulary does not define
    uint64_t *mine = gr_stack + (int64_t)slot * 4;
    Stack sk = {mine[0], mine[1], mine[2], mine[3]};
    int d = depth_of(sk);
    const Guide g = guide_of(st, P, gr_next, gr_meta);
    const int nxt = walk_stack(st, sk, d, b0, b1, tok_bytes, g);
    if (nxt < 0) return;                                        // a dead walk (a stop id, a dropped run-ahead row) leaves both
    gr_state[slot] = nxt;
    mine[0] = sk.w0;
    mine[1] = sk.w1;
    mine[2] = sk.w2;
    mine[3] = sk.w3;
}

__global__ __launch_bounds__(kLaneThreads) void grammar_reset_kernel(const int n, const int n_slots, const int32_t *__restrict__ slots,
                                                                     const int32_t *__restrict__ start,
                                                                     int32_t *__restrict__ gr_state, uint64_t *__restrict__ gr_stack) {
    const int i = blockIdx.x * kLaneThreads + threadIdx.x;
    if (i >= n) return;
    const int slot = slots[i];
    if (slot < 0 || slot >= n_slots) return;
    gr_state[slot] = start[i];
    for (int k = 0; k < 4; ++k) gr_stack[(int64_t)slot * 4 + k] = 0;
}

}  // namespace

extern "C" int rwkv7_grammar_build(int S, int row0, int P, int V, const int32_t *gr_next, const int32_t *gr_meta,
                                   const int32_t *tok_off, const uint8_t *tok_bytes, int n_special, const int32_t *special,
                                   uint32_t *gr_allow, uint32_t *gr_maybe, void *stream) {
    if (S < 0 || row0 < 0 || P <= 0 || (int64_t)row0 + S > P || V <= 0 || V % 64 != 0 || n_special < 0 || S > 65535)
        return CHIRRUP_E_SHAPE;
    if (S == 0) return 0;
    if (!gr_next || !gr_meta || !tok_off || !tok_bytes || !gr_allow || !gr_maybe || (n_special > 0 && !special)) return CHIRRUP_E_NULL;
    if ((reinterpret_cast<uintptr_t>(gr_allow) | reinterpret_cast<uintptr_t>(gr_maybe)) & 7) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(grammar_build_kernel, dim3((unsigned)((V + kBuildThreads - 1) / kBuildThreads), (unsigned)S), dim3(kBuildThreads),
                       0, static_cast<hipStream_t>(stream), row0, P, V, gr_next, gr_meta, tok_off, tok_bytes, n_special, special,
                       gr_allow, gr_maybe);
    return (int)hipGetLastError();
}

extern "C" int rwkv7_grammar_apply(int n_rows, int n_logit_rows, int V, int P, void *logits, const int32_t *rows,
                                   const int32_t *slot_idx, int n_slots, const int32_t *gr_state, const uint64_t *gr_stack,
                                   const int32_t *gr_next, const int32_t *gr_meta, const uint32_t *gr_allow, const uint32_t *gr_maybe,
                                   const int32_t *tok_off, const uint8_t *tok_bytes, void *stream) {
    if (n_rows < 0 || n_logit_rows < 0 || V <= 0 || V % 32 != 0 || P <= 0 || n_slots <= 0) return CHIRRUP_E_SHAPE;
    if (n_rows == 0) return 0;
    if (!logits || !rows || !gr_state || !gr_stack || !gr_next || !gr_meta || !gr_allow || !gr_maybe || !tok_off || !tok_bytes)
        return CHIRRUP_E_NULL;
    if ((reinterpret_cast<uintptr_t>(logits) & 15) || (reinterpret_cast<uintptr_t>(gr_stack) & 7)) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(grammar_apply_kernel, dim3((unsigned)n_rows), dim3(kApplyThreads), 0, static_cast<hipStream_t>(stream),
                       n_logit_rows, V, P, static_cast<uint32_t *>(logits), rows, slot_idx, n_slots, gr_state, gr_stack, gr_next, gr_meta,
                       gr_allow, gr_maybe, tok_off, tok_bytes);
    return (int)hipGetLastError();
}

extern "C" int rwkv7_grammar_advance(int n_rows, int n_ids, int V, int P, const int32_t *rows, const int32_t *slot_idx, int n_slots,
                                     const int32_t *ids, const int32_t *tok_off, const uint8_t *tok_bytes, const int32_t *gr_next,
                                     const int32_t *gr_meta, int32_t *gr_state, uint64_t *gr_stack, void *stream) {
    if (n_rows < 0 || n_ids < 0 || V <= 0 || P <= 0 || n_slots <= 0) return CHIRRUP_E_SHAPE;
    if (n_rows == 0) return 0;
    if (!rows || !ids || !tok_off || !tok_bytes || !gr_next || !gr_meta || !gr_state || !gr_stack) return CHIRRUP_E_NULL;
    if (reinterpret_cast<uintptr_t>(gr_stack) & 7) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(grammar_advance_kernel, dim3((unsigned)((n_rows + kLaneThreads - 1) / kLaneThreads)), dim3(kLaneThreads), 0,
                       static_cast<hipStream_t>(stream), n_rows, n_ids, V, P, rows, slot_idx, n_slots, ids, tok_off, tok_bytes, gr_next,
                       gr_meta, gr_state, gr_stack);
    return (int)hipGetLastError();
}

extern "C" int rwkv7_grammar_reset(int n, int n_slots, const int32_t *slots, const int32_t *start, int32_t *gr_state,
                                   uint64_t *gr_stack, void *stream) {
    if (n < 0 || n_slots <= 0) return CHIRRUP_E_SHAPE;
    if (n == 0) return 0;
    if (!slots || !start || !gr_state || !gr_stack) return CHIRRUP_E_NULL;
    if (reinterpret_cast<uintptr_t>(gr_stack) & 7) return CHIRRUP_E_ALIGN;
    hipLaunchKernelGGL(grammar_reset_kernel, dim3((unsigned)((n + kLaneThreads - 1) / kLaneThreads)), dim3(kLaneThreads), 0,
                       static_cast<hipStream_t>(stream), n, n_slots, slots, start, gr_state, gr_stack);
    return (int)hipGetLastError();
}
