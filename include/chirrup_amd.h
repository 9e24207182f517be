/*
 * chirrup_amd.h -- C ABI of libchirrup_amd.so, the MI355X (gfx950) RWKV-7 decode kernels.
 *
 * This is the drop-in boundary B2 of SURVEY.md section 8(b): the entry points are what the
 * reference's torch binding for this path calls (file:line given per function, relative to
 * the leonsama/chirrup tree), with three additions every function shares:
 *   - an explicit `void *stream` (a hipStream_t; NULL = the null stream),
 *   - an `int` return: 0 on success, CHIRRUP_E_* (< 0) for arguments the kernel would
 *     mis-handle (the reference only has `assert(H*_N_==C)`), or a positive hipError_t,
 *   - where it shards a state pool: an optional `slot_idx` indirection.
 * Plain pointers and sizes only; no torch types.  All pointers are DEVICE pointers.
 * All kernels are stateless and re-entrant; they may be called concurrently from several host
 * threads / processes, each on its own device and stream, and may be captured in a hipGraph.
 */
#ifndef CHIRRUP_AMD_H
#define CHIRRUP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHIRRUP_OK 0
#define CHIRRUP_E_SHAPE (-1)     /* C != H*64, non-positive sizes, size limits */
#define CHIRRUP_E_NULL (-2)      /* a required pointer is NULL */
#define CHIRRUP_E_ALIGN (-3)     /* pointer / stride not aligned as documented */
#define CHIRRUP_E_UNSUPPORTED (-4)

/* Library / ABI version and the gfx target the kernels were built for ("gfx950").
 * CHIRRUP_ABI_VERSION changes whenever an exported prototype changes incompatibly; a caller compares it with
 * chirrup_abi_version() of the library it loaded before making any other call (chirrup_amd/lib.py does).
 *   1  round 1
 *   2  round 2: skinny_gemm_f16 / _f16_group / _f16_partial gained row_halves (and tile_counters) ahead of `stream`,
 *      skinny_gemm_f16_grouped gained w_tiled, skinny_gemm_group_workspace_bytes gained K, skinny_gemm_select removed
 *   3  round 3: chirrup_mm8_fuse gained out_planes (the struct grew); new entry points only otherwise (rwkv7_tmix_gemms,
 *      rwkv7_tmix_gemms_mm8, rwkv7_tmix_wkv7_fused_mm8, skinny_untile_weight, the clock probes)
 *   4  round 4: rwkv7_tmix_gemms / _mm8 gained `status` (a sticky status word of the caller's) ahead of spin_limit and the status
 *      word moved to the END of the sync words; rwkv7_commit_sampled gained status_src / status_dst ahead of `stream`;
 *      new: mm8t_seq_exact, mm8t_exact_workspace_bytes, mm8_dequant_f16, chirrup_device_cu_count, rwkv7_penalize_argmax_listed,
 *      rwkv7_commit_sampled_listed */
#define CHIRRUP_ABI_VERSION 4
int chirrup_abi_version(void);
const char *chirrup_target_arch(void);

/*
 * WKV7 recurrent state update over T timesteps (decode: T = 1).
 * Replaces: cuda_forward_seq  Albatross/cuda/rwkv7_state_fwd_fp16.cpp:6 (launcher
 *           Albatross/cuda/rwkv7_state_fwd_fp16.cu:313-316, kernel :26-97), reached from
 *           torch.ops.rwkv7_state_fwd_fp16.forward_seq (Albatross/rwkv7.py:151).
 * state     binary16 [n_slots][H][64][64], updated in place. Batch row b uses slot
 *           slot_idx[b] when slot_idx != NULL, else slot b. Slots are slot_stride ELEMENTS
 *           apart (0 = dense, H*64*64). 16-byte aligned; slot_stride % 8 == 0.
 *           Two batch rows must not name the same slot.
 * r,w,k,v,a,b  binary16 [B][T][C] contiguous.   y  binary16 [B][T][C] out.
 * elapsed_t int32 [B] (tokens already consumed by each row; feeds the decay dither).
 * Arithmetic: exactly spec A1 of SURVEY.md section 8 -- binary16 storage AND binary16
 * accumulate in the reference's two-lane order, one rounding per operation, no FMA.
 */
int wkv7_fwd_seq(int B, int T, int C, int H, void *state, const void *r, const void *w,
                 const void *k, const void *v, const void *a, const void *b, void *y,
                 const int32_t *elapsed_t, const int32_t *slot_idx, int64_t slot_stride,
                 void *stream);

/* Single-timestep form.  Replaces: cuda_forward_one  Albatross/cuda/rwkv7_state_fwd_fp16.cpp:7
 * (launcher .cu:318-322, kernel .cu:99-167; torch.ops.rwkv7_state_fwd_fp16.forward_one,
 * Albatross/rwkv7.py:96,132).  r..b, y are [B][C]. Same arithmetic as wkv7_fwd_seq with T=1. */
int wkv7_fwd_one(int B, int C, int H, void *state, const void *r, const void *w, const void *k,
                 const void *v, const void *a, const void *b, void *y, const int32_t *elapsed_t,
                 const int32_t *slot_idx, int64_t slot_stride, void *stream);
/* The state-independent part of the update taken out of the sequential loop, for chunks of many tokens: wkv7_decay computes
 * w~ = exp(-e^-0.5 * sigmoid(w)) - 1 + dither(elapsed_t[b] + t) for every row at once (cu:23, :59; w, w_out binary16
 * [B][T][C]); wkv7_fwd_seq_decayed is wkv7_fwd_seq given w~ instead of w.  Together bit-identical to wkv7_fwd_seq. */
int wkv7_decay(int B, int T, int C, const void *w, const int32_t *elapsed_t, void *w_out, void *stream);
int wkv7_fwd_seq_decayed(int B, int T, int C, int H, void *state, const void *r, const void *w_decayed, const void *k,
                         const void *v, const void *a, const void *b, void *y, const int32_t *elapsed_t,
                         const int32_t *slot_idx, int64_t slot_stride, void *stream);

/*
 * Sparse binary16 vector x matrix: out[c] += sum_{d : vec[d] != 0} vec[d] * mat[d][c].
 * Replaces: cuda_spmv_forward  Albatross/cuda/rwkv7_state_fwd_fp16.cpp:8 (launcher .cu:324-330,
 *           kernel .cu:222-310) and the ROCm path rwkv_mm_sparsity,
 *           Albatross/rwkv_mm_op_triton.py:6-61 (bsz = 1 channel-mix, Albatross/rwkv7.py:659).
 * vec [D], mat [D][C] row-major, out [C]; binary16. As in the reference `out` is ACCUMULATED
 * into, so the caller zeroes it (Albatross/rwkv7.py:65). Requires C % 8 == 0.
 * Accumulation is binary32 in row order (the Triton path's arithmetic) and deterministic.
 * workspace: device scratch of spmv_fp16_workspace_bytes(D, C) bytes (may be NULL if 0).
 */
int64_t spmv_fp16_workspace_bytes(int D, int C);
int spmv_fp16(int D, int C, const void *vec, const void *mat, void *out, void *workspace,
              void *stream);

/*
 * mm8 (w8a16): y[i][k] = sum_j x[i][j] * ((w[j][k] + 0.5) * rx[k] * ry[j] + mx[k] + my[j]).
 * Replaces: rwkv_pip::mm8_seq and rwkv_pip::mm8_seq_opt  scripts/test_mm8/rwkv_pip_wrapper.cpp:51-84, :206-211
 *           (kernels scripts/test_mm8/rwkv_pip_operators.cu:59-97 and the _opt / wmma forms :205-558).
 * x [B][N] binary16 (row stride x_stride elements), w [N][M] uint8 (row stride w_stride),
 * mx,rx [M], my,ry [N] binary16, y [B][M] binary16 (row stride y_stride).
 * Runs on the matrix cores: w is re-laid into K-contiguous tile images in the workspace (mm8_pack) and multiplied by
 * mm8t_seq, i.e. binary32 accumulate in the algebraically split form of scripts/test_mm8/benchmark.py:167-179
 * (xs = fp16(x*ry) through MFMA, rank-1 corrections after) -- the reference's own tolerance between its split and
 * direct forms is rtol 1e-3 (benchmark_pure_pytorch.py:92).  Needs N % 64 == 0, M % 128 == 0, 16-byte aligned x / w and
 * w_stride % 16 == 0; any other shape runs mm8_seq_direct.  Static weights: pack once with mm8_pack and call
 * mm8t_seq(w_tiled = 1) directly (what chirrup_amd.ops.mm8_seq does behind a per-tensor cache).
 * workspace: mm8_seq_workspace_bytes(B, N, M) bytes of device scratch (0 for the direct fallback).
 */
int64_t mm8_seq_workspace_bytes(int B, int N, int M);
int mm8_seq(int B, int N, int M, const void *x, int x_stride, const void *w, int w_stride,
            const void *mx, const void *rx, const void *my, const void *ry, void *y,
            int y_stride, void *workspace, void *stream);
int mm8_seq_opt(int B, int N, int M, const void *x, int x_stride, const void *w, int w_stride,
                const void *mx, const void *rx, const void *my, const void *ry, void *y,
                int y_stride, void *workspace, void *stream);
/* The as-coded kernel (rwkv_pip_operators.cu:59-83): binary32 accumulate over j in order, one rounding per operation;
 * bit-identical to oracle_mm8_seq.  Any shape; FP32 VALU, not MFMA -- parity and ragged shapes only. */
int mm8_seq_direct(int B, int N, int M, const void *x, int x_stride, const void *w, int w_stride,
                   const void *mx, const void *rx, const void *my, const void *ry, void *y,
                   int y_stride, void *stream);
/* w [N][M] uint8 (row stride w_stride, % 16 == 0; N % 64 == 0, M % 128 == 0) -> mm8_packed_bytes(N, M) = N*M bytes in the
 * layout mm8t_seq(w_tiled = 1) reads: the transposed matrix wT [M][N] cut into 8-KiB (128 x 64) tile images. */
int64_t mm8_packed_bytes(int N, int M);
int mm8_pack(int N, int M, const void *w, int w_stride, void *packed, void *stream);

/* GEMV form, binary32 output that the caller zeroes (the reference accumulates with
 * atomicAdd).  Replaces: rwkv_pip::mm8_one  scripts/test_mm8/rwkv_pip_wrapper.cpp:86-119
 * (kernel scripts/test_mm8/rwkv_pip_operators.cu:150-189). x [N], y [M] float. */
int mm8_one(int N, int M, const void *x, const void *w, int w_stride, const void *mx,
            const void *rx, const void *my, const void *ry, float *y, void *stream);

/*
 * Fused element-wise chains between the GEMMs of one layer.  They replace runs of separate torch
 * ops in Albatross/rwkv7.py (lines given); every op of a chain still rounds to binary16 once, as
 * in the reference's eager execution, reductions accumulate in binary32.  All tensors binary16,
 * rows of C channels, C % 64 == 0, 16-byte aligned.
 *
 * rwkv7_add_ln_mix: x_new = x (+ delta, may be NULL) -> x_out (may be NULL; may alias x when T == 1 -- with T > 1, a
 *   delta and n_mix > 0 it must be a different buffer: row t re-reads x[t-1] + delta[t-1] for the token shift);
 *   cur = LayerNorm(x_new; ln_w, ln_b, eps); with n_mix in {1, 6}: token shift against the previous
 *   row (t > 0) or prev_in[b] (t == 0), out[m] = cur + (prev - cur) * mix[m], prev_out[b] = cur of
 *   the last row; with n_mix == 0: out = cur.   x,delta,x_out,out[m]: [B][T][C]; prev_*: [B][C];
 *   mix: [n_mix][C]; out planes are out_stride elements apart.  T > 1 needs prev_out != prev_in.
 *   slot_idx (may be NULL): batch row b carries its token-shift state in row slot_idx[b] of prev_*.
 *   delta_partials (may be NULL; then delta must be NULL): float [delta_splits][B][T][C] split-K partial sums of
 *   the GEMM that produced delta (skinny_gemm_f16_partial); delta = binary16(sum over splits) is formed in this
 *   kernel's prologue, saving the GEMM's separate reduce launch.
 *   Replaces rwkv7.py:523 + :621-623 (n_mix 6), :531-533 + :675-677 (n_mix 1), :548-550 (n_mix 0).
 */
int rwkv7_add_ln_mix(int B, int T, int C, int n_mix, const void *x, const void *delta, void *x_out,
                     const void *ln_w, const void *ln_b, float eps, const void *prev_in, void *prev_out,
                     const void *mix, void *out, int64_t out_stride, const int32_t *slot_idx,
                     const float *delta_partials, int delta_splits, void *stream);
/* The same kernel next to mm8 (w8a16) GEMMs, whose split form (scripts/test_mm8/benchmark.py:167-179) has an activation
 * prologue (xs = fp16(x*ry), S = {sum xs, sum x*my, sum x} per row) and rank-1 corrections after the matrix product:
 *   in_*  : delta_partials hold the CORE sums of an mm8 product (mm8t_gemm_partial) with output scales in_rx, in_mx [C] and
 *           the row sums in_S [B*T][3] of ITS prologue: delta = fp16(rx*(sum - 1023.5*S0) + S1 + mx*S2) is formed here (the
 *           u8 kernels multiply by 1024 + q, so the core sums carry 1024*S0, removed with the +0.5*S0 term) -- the
 *           product's reduce launch folded into this kernel (as delta_partials does for the binary16 GEMMs);
 *   out_* : (n_mix == 1 only) besides out, write the prologue of the mm8 product that consumes out: out_xs [B][T][C] and
 *           out_S [B*T][3] for input scales out_ry, out_my [C] -- that product's prologue launch folded in.
 * Either half may be all-NULL; fuse == NULL is rwkv7_add_ln_mix. */
typedef struct {
    const void *in_rx, *in_mx;   /* binary16 [C] */
    const float *in_S;           /* [B*T][in_S_parts][3]: the row sums as in_S_parts partial sums each (added up here) */
    const void *out_ry, *out_my; /* binary16 [C] */
    void *out_xs;                /* binary16 [B][T][C] */
    float *out_S;                /* [B*T][3] */
    int in_S_parts;              /* 0 or 1: one sum per row; mm8_reduce_rows writes mm8_row_parts(C) of them, mm8t_gemm_fused mm8_tile_parts(C) */
    int out_planes;              /* 0 or 1: the prologue of mix plane 0 (n_mix = 1, or 6); 2..3 (n_mix = 6): of planes 0..out_planes-1
                                    (r, k, v) -- out_ry / out_my then [out_planes][C], out_xs [out_planes][B*T][C] (plane stride =
                                    out_stride), out_S [out_planes][B*T][3] */
} chirrup_mm8_fuse;
int rwkv7_add_ln_mix_mm8(int B, int T, int C, int n_mix, const void *x, const void *delta, void *x_out,
                         const void *ln_w, const void *ln_b, float eps, const void *prev_in, void *prev_out,
                         const void *mix, void *out, int64_t out_stride, const int32_t *slot_idx,
                         const float *delta_partials, int delta_splits, const chirrup_mm8_fuse *fuse, void *stream);

/* rwkv7.py:629-637: a = sigmoid(a_pre); kk = normalize(k*k_k) per 64-channel head;
 * k <- k*(1+(a-1)*k_a) in place; neg_kk = -kk; kka = kk*a; and, when v_first != NULL (layer > 0),
 * v <- v + (v_first - v)*sigmoid(vg_pre) in place.  rows = B*T. */
int rwkv7_tmix_mid(int64_t rows, int C, void *k, void *v, const void *a_pre, const void *vg_pre,
                   const void *v_first, const void *k_k, const void *k_a, void *neg_kk, void *kka,
                   void *stream);

/* rwkv7.py:647-649 up to the output projection: out = (group_norm_H(y; lnx_w, lnx_b, eps) +
 * (sum_head r*k*r_k) * v) * g. */
int rwkv7_tmix_post(int64_t rows, int C, const void *y, const void *r, const void *k, const void *v,
                    const void *g, const void *r_k, const void *lnx_w, const void *lnx_b, float eps,
                    void *out, void *stream);

/* LoRA hidden activations in place on `nplanes` consecutive planes of plane_elems binary16 values,
 * plane ids first_plane.. in the order [v, w, a, g]: w -> tanh (rwkv7.py:626), g -> sigmoid (:630),
 * a and v unchanged (:629, :637). */
int rwkv7_lora_act(int nplanes, int first_plane, int64_t plane_elems, void *hbuf, void *stream);

/*
 * Fused time-mix core (one launch per layer): the gating chain of rwkv7.py:629-637 (as rwkv7_tmix_mid),
 * the WKV7 update of wkv7_fwd_seq with a = -kk, b = kk*a, and the output chain of :647-649 (as
 * rwkv7_tmix_post), all inside the WKV7 kernel -- lane j of a head's wavefront holds channel j, the
 * head reductions (L2 norm, group-norm moments, bonus sum) are wavefront shuffles, and k', v', -kk,
 * kk*a, y never exist in HBM.  r, w, k, v are the RAW projections ([B][T][C]); out [B][T][C].
 * vg_pre / v_first both NULL for layer 0.  Same arithmetic (one rounding per torch op) as the three
 * separate kernels; only the order of the binary32 head reductions differs.
 */
int rwkv7_tmix_wkv7_fused(int B, int T, int C, int H, void *state, const void *r, const void *w, const void *k,
                          const void *v, const void *a_pre, const void *vg_pre, const void *v_first, const void *g,
                          const void *k_k, const void *k_a, const void *r_k, const void *lnx_w, const void *lnx_b,
                          float eps, void *out, const int32_t *elapsed_t, const int32_t *slot_idx,
                          int64_t slot_stride, void *stream);
/* ... with the mm8 (w8a16) activation prologue of the GEMM that consumes `out` (att.output as uint8 weights, scripts/test_mm8/
 * benchmark.py:167-173, :447-452): out receives xs = binary16(o * ry) instead of o, and S [B*T][H][3] (float) each head's share of
 * the row sums {sum xs, sum o*my, sum o} (the consumer adds the H parts in head order: rwkv7_add_ln_mix_mm8 with in_S_parts = H).
 * ry = NULL: identical to rwkv7_tmix_wkv7_fused. */
int rwkv7_tmix_wkv7_fused_mm8(int B, int T, int C, int H, void *state, const void *r, const void *w, const void *k, const void *v,
                              const void *a_pre, const void *vg_pre, const void *v_first, const void *g, const void *k_k,
                              const void *k_a, const void *r_k, const void *lnx_w, const void *lnx_b, float eps, void *out,
                              const int32_t *elapsed_t, const int32_t *slot_idx, int64_t slot_stride, const void *ry,
                              const void *my, float *S, void *stream);

/* rwkv7.py:678: x <- relu(x)**2 in place over n elements (n % 8 == 0). */
int rwkv7_relu_sq(int64_t n, void *x, void *stream);

/*
 * Skinny-M MFMA GEMM for the decode step: Y[M][N] = act(X[M][K] . W[N][K]^T + bias), M <= 256,
 * binary16 in / binary32 accumulate / binary16 out.  Plays the role of the reference's
 * F.linear / torch.matmul calls on the projection weights (Albatross/rwkv7.py:625-630, :649, :678-679,
 * :551) for batch sizes where the library GEMM is operand-ingest bound.
 * W row-major [N][K] (the layout the reference keeps its `*.weight` tensors in), row stride ldw
 * elements; K % 64 == 0, N % 4 == 0, ldx % 8 == 0, ldw % 8 == 0.  act: 0 none, 1 relu(.)^2 (rwkv7.py:678).
 * splits: K-split factor (0 = the library's choice: enough workgroups for the 256 CUs at the kernel's tile width);
 * needs skinny_gemm_workspace_bytes(M,N,K,splits) bytes of device scratch when that is > 0.
 * skinny_gemm_splits: the factor a call with these sizes uses (Z = problems of a batched launch, 1 otherwise).
 */
int64_t skinny_gemm_workspace_bytes(int M, int N, int K, int splits);
int skinny_gemm_splits(int N, int K, int Z, int splits);
/* As skinny_gemm_f16 without bias/activation, but leaves the `splits` binary32 partial results
 * [splits][M][N] in `partials` for the consumer to sum (see rwkv7_add_ln_mix). Returns the split count used
 * (> 0) or a negative CHIRRUP_E_* / positive hipError_t is NOT distinguishable here, so errors are < 0 only. */
int skinny_gemm_f16_partial(int M, int N, int K, const void *X, int ldx, const void *W, int64_t ldw, int w_tiled, int splits,
                            int row_halves, float *partials, void *stream);
/* Z independent skinny GEMMs in ONE launch (RWKV-7's receptance/key/value projections, Albatross/rwkv7.py:603-605,
 * and its four LoRA pairs, :626-637): Y[z] = act(X[z] . W[z]^T + bias[z]).  Problem z's operands start z * (their
 * batch stride, in elements) after problem 0's; bias may be NULL.  act: 0 none, 1 relu(.)^2, 4 + p: LoRA hidden
 * planes (v, w, a, g) with problem 0 = plane p: tanh on w, sigmoid on g.  K must be a multiple of 64, M <= 256.
 * Needs skinny_gemm_batched_workspace_bytes(...) bytes of scratch when splits != 1 or act != 0. */
int64_t skinny_gemm_batched_workspace_bytes(int Z, int M, int N, int K, int splits);
int skinny_gemm_f16_batched(int Z, int M, int N, int K, const void *X, int ldx, int64_t x_bs, const void *W, int64_t ldw,
                            int64_t w_bs, const void *bias, int64_t bias_bs, void *Y, int ldy, int64_t y_bs, int act,
                            int splits, void *workspace, void *stream);
/* The same with a reduction length per problem: problem z uses only the first k_of[z] columns of X[z] and W[z]
 * (k_of[z] <= K, multiple of 64; NULL = K for all).  Operands zero-padded to a common K (the LoRA ranks 96/128/128/480
 * packed as 512) are then not streamed beyond their real rank.  Z <= 8; splits must be 1 when k_of is given.
 * w_tiled: every W[z] is the tile image (skinny_tile_weight) of its [N][K] matrix, N % 128 == 0.
 * row_halves: as below, honoured for splits == 1 and act == 0 (the LoRA up-projections: 4 x 32 tiles of 2..8 K-blocks get
 * twice the workgroups and, with half the x image per stage, a deeper operand ring). */
int skinny_gemm_f16_grouped(int Z, int M, int N, int K, const int *k_of, const void *X, int ldx, int64_t x_bs, const void *W,
                            int64_t ldw, int64_t w_bs, int w_tiled, const void *bias, int64_t bias_bs, void *Y, int ldy,
                            int64_t y_bs, int act, int splits, int row_halves, void *workspace, void *stream);
/* Up to 8 GEMMs that share M, K, the row strides of x and W (ldx, ldw) and the split count, in ONE launch plus one
 * reduce launch: y_i = act_i(x_i . w_i^T + bias_i), w_i binary16 [n_i][K].  This is one RWKV-7 layer's receptance /
 * key / value projections together with its four LoRA down-projections and their activations (Albatross/rwkv7.py:
 * 625-637): seven independent GEMMs over the same token rows that the reference issues one by one.
 * act: 0 none, 1 relu(.)^2, 2 tanh, 3 sigmoid (applied to the binary16-rounded sum, like a separate torch op).
 * splits = 0: the library's choice.  Unsplit launches apply bias / activation in the GEMM epilogue; split ones go through
 * binary32 partials and one reduce launch: workspace = skinny_gemm_group_workspace_bytes(...) bytes, 256-byte aligned.
 *
 * row_halves = 1 (here, in skinny_gemm_f16, skinny_gemm_f16_partial and skinny_gemm_f16_grouped; honoured for M > 32 with
 * the 128-column kernel): every tile and K-slice is worked on by TWO workgroups, one per half of the rows -- twice the
 * workgroups without more partial planes (an unsplit launch then fills the chip with no partials and no reduce launch);
 * both stream the W tile, side by side on one XCD so that HBM sees it once.  splits = 0 then chooses for twice the tiles;
 * skinny_gemm_splits / *_workspace_bytes stay upper bounds.  Results are bit-identical to row_halves = 0 at the same
 * split count (a row's sums never depend on other rows). */
typedef struct {
    const void *x;     /* [M][ldx] binary16 */
    const void *w;     /* [n][ldw] binary16 */
    void *y;           /* [M][ldy] binary16 */
    const void *bias;  /* [n] binary16 or NULL */
    int n, ldy, act;
    int w_tiled;       /* w is in the tile-image layout (skinny_tile_weight); needs n % 128 == 0 */
} chirrup_gemm_problem;
int64_t skinny_gemm_group_workspace_bytes(int count, const chirrup_gemm_problem *problems, int M, int K, int splits);
/* tile_counters (skinny_gemm_f16_group, skinny_gemm_f16; may be NULL): skinny_gemm_pair_counters() ints, ZERO before their first
 * use and used by no other launch that may run concurrently (one set per stream).  With them a launch of at most 32 rows whose
 * split count is 2..4 (at most 48 KB of partials per tile) needs no reduce launch: every K-slice of a
 * tile writes its binary32 partial, the last to finish adds the partials in slice order (its own from on-chip sums) and applies
 * bias / activation itself; it leaves the counter at zero.  Bit-identical to the reduce-launch path.
 * The hand-off between the workgroups uses write-through stores, one agent-scope atomic per workgroup and L1-bypassing loads, no
 * fences -- a form measured on gfx950 for ONE workgroup per CU and memory from hipMalloc (MI355X_MICROARCH.md, inter-workgroup
 * visibility): `workspace` and `tile_counters` must be hipMalloc'ed device memory (not host-mapped, not managed), and the library
 * only takes this path for launches whose workgroups need more than half of a CU's LDS (so that two can never share a CU).
 * A launch that does not complete (device fault, process killed) may leave counters non-zero: zero them again before reuse --
 * chirrup_amd does so at the head of every captured decode graph and after any failed call. */
int skinny_gemm_pair_counters(void);
/* Diagnostic for bench.py / tools (process-wide, not thread-safe): while buf != NULL every 128-column GEMM launch of at most
 * `pairs` workgroups writes, per workgroup, the duration of its main loop as {shader-clock ticks (s_memtime), ticks of the
 * constant 100-MHz counter (s_memrealtime)} into buf (uint64 [2 * pairs]); ticks / (100-MHz ticks) * 100 = the clock in MHz the
 * CU ran the loop at.  When pairs >= 3 x the launch's workgroups, 4 absolute 100-MHz stamps per workgroup follow the pairs
 * (buf[2 * workgroups + 4 * wg + {0..3}]: kernel entry, main loop start, main loop end, epilogue stores done): the launch's
 * timeline (tools/gemm_timeline.py).  buf = NULL switches it off again. */
int skinny_gemm_clock_probe(void *buf, int pairs);
/* Experiment (tools/exp_warm.py): while stages > 0 every 128-column launch is preceded by a launch of the
 * same grid that touches the first `stages % 100` K-blocks of each workgroup's W tile (stages / 100: 1 = the next tile's bytes,
 * 3 = a tile half the matrix away, 2 = no loads but `stages % 100` x ~4 us of idling); sink: 4 writable bytes.  Process-wide. */
int skinny_gemm_warm_probe(int stages, void *sink);
/* The chip's clock without load: one wavefront spins `iters` dependent VALU operations; out (uint64 [2]) receives {shader-clock
 * ticks, 100-MHz ticks}. */
int chirrup_clock_probe(int iters, void *out, void *stream);
/* Diagnostic (tools/ln_timeline.py): while buf is set every rwkv7_add_ln_mix* launch writes 8 100-MHz stamps per workgroup
 * (entry, row data arrived, mean, variance, normalised, stores issued, stores acknowledged, unused); NULL switches it off. */
int rwkv7_ln_probe(void *buf);
/* Launch-cost probe (tools/launch_cost.py): `grid` workgroups of `block` lanes that hold lds_bytes of LDS, idle for sleep x ~4 us
 * and do nothing else. */
int chirrup_noop_launch(int grid, int block, int lds_bytes, int sleep, void *sink, void *stream);
int skinny_gemm_f16_group(int count, const chirrup_gemm_problem *problems, int M, int K, int ldx, int64_t ldw, int splits,
                          int row_halves, void *workspace, void *tile_counters, void *stream);
int skinny_gemm_f16(int M, int N, int K, const void *X, int ldx, const void *W, int64_t ldw, int w_tiled, const void *bias,
                    void *Y, int ldy, int act, int splits, int row_halves, void *workspace, void *tile_counters, void *stream);
/*
 * R/K/V and the WHOLE LoRA chain of one RWKV-7 layer (Albatross/rwkv7.py:625-630, :637: four down-projections, tanh / sigmoid,
 * four up-projections + bias) in ONE launch: the chain runs on the CUs the R/K/V tiles leave idle, beside them, instead of as
 * a second launch behind them (round 2: 12 us per layer at 7.2B / bsz 200).
 *   main[i]  (n_main <= 4):  y = x . w^T                                        (as chirrup_gemm_problem; act as there)
 *   lora[p]  (n_lora <= 4):  hid = act(x . w^T)  [M][n of ld_hid], then  y = hid[:, :k_up] . w_up^T + bias  [M][up_n of up_ldy]
 * 1 <= M <= 256 rows (row_halves = 1 and M > 32: two workgroups per tile over the two halves of the rows, as elsewhere; whole-row
 * tiles otherwise, M <= 128 -- at <= 32 rows the main tiles are then split 2..4 ways over K and reduced inside the launch like
 * skinny_gemm_f16's), shared K (% 64), ldx; w of lora[p] row-major [n][K] (row stride ldw, n % 64 == 0); w_up a tile image
 * (skinny_tile_weight) of [up_n][up_kimg] whose first k_up columns are multiplied (k_up <= n, % 64); act: 0 none, 2 tanh,
 * 3 sigmoid.  workspace: rwkv7_tmix_gemms_workspace_bytes bytes; sync: rwkv7_tmix_sync_words() ints -- both hipMalloc'ed, sync
 * ZERO before the first launch (every completed launch leaves it zero; the workgroups hand tiles to each other through it with
 * write-through stores, one agent-scope atomic per workgroup and ONE agent-scope acquire per consumer: cdna_hip_programming.md
 * Guideline 16).  Every wait is bounded (spin_limit polls of ~0.25 us, 0 = default ~0.1 s): if one gives up -- another tenant
 * held most of the chip that long -- the STATUS word is OR-ed non-zero and this launch's LoRA outputs are undefined.  status: an
 * int32 of the caller's (one per device is enough: launches only ever OR into it, nobody but its owner clears it), or NULL =
 * sync[rwkv7_tmix_status_word()], the LAST sync word; words [0, rwkv7_tmix_status_word()) may be zeroed between launches at
 * any time (a captured decode graph zeroes them at the head of every replay) -- the status word must not be, or a step that
 * gave up is erased by the next one (ABI 4; rwkv7_commit_sampled hands the word to the host behind every step's sampled ids).
 * One launch at a time per (workspace, sync).  All chain workgroups must be resident at once (they wait for each other):
 * CHIRRUP_E_UNSUPPORTED on a device with fewer compute units than the chain has workgroups (chirrup_device_cu_count()).
 */
typedef struct {
    const void *x;      /* [M][ldx] binary16 */
    const void *w;      /* down-projection [n][K] binary16, row stride ldw */
    void *hid;          /* [M][ld_hid] binary16: columns [0, n) are written */
    const void *w_up;   /* tile image of the up-projection [up_n][up_kimg] */
    const void *bias;   /* [up_n] binary16 or NULL */
    void *y;            /* [M][up_ldy] binary16 */
    int n, k_up, act;
} chirrup_lora_problem;
/* A uint8 (mm8, w8a16) main problem of rwkv7_tmix_gemms_mm8: y = mm8(x, w) in the split form of scripts/test_mm8/benchmark.py:
 * 167-179 -- xs [M][ldx] = binary16(x * ry) and S [M][3] = {sum xs, sum x*my, sum x} are the product's activation prologue
 * (rwkv7_add_ln_mix_mm8 writes them for r, k, v with out_planes = 3), w the K-contiguous uint8 weights [n][K] (tile images of
 * skinny_tile_weight_u8 when w_tiled), rx / mx [n] the column scales.  n % 8 == 0, ldy % 8 == 0, 16-byte aligned y / rx / mx. */
typedef struct {
    const void *xs;
    const void *w;
    void *y;
    const void *rx, *mx;
    const float *S;
    int n, ldy, w_tiled;
} chirrup_mm8_problem;
int rwkv7_tmix_sync_words(void);
int rwkv7_tmix_status_word(void);
int64_t rwkv7_tmix_gemms_workspace_bytes(int M, int K, int n_main, const chirrup_gemm_problem *main_problems, int n_lora,
                                         const chirrup_lora_problem *lora, int row_halves);
int rwkv7_tmix_gemms(int M, int K, int ldx, int64_t ldw, int n_main, const chirrup_gemm_problem *main_problems, int n_lora,
                     const chirrup_lora_problem *lora, int ld_hid, int up_n, int up_kimg, int up_ldy, int row_halves, void *workspace,
                     void *sync, void *status, int spin_limit, void *stream);
/* Compute units of the current device (what the time-mix launch sizes its chain by). */
int chirrup_device_cu_count(void);
/* ... with uint8 main problems (R/K/V as mm8 weights; the rank-1 corrections run in each tile's epilogue); the LoRA problems,
 * workspace (size it with the binary16 call's function, passing n and w_tiled of the uint8 problems) and sync as above. */
int rwkv7_tmix_gemms_mm8(int M, int K, int ldx, int64_t ldw, int n_main, const chirrup_mm8_problem *main_problems, int n_lora,
                         const chirrup_lora_problem *lora, int ld_hid, int up_n, int up_kimg, int up_ldy, int row_halves,
                         void *workspace, void *sync, void *status, int spin_limit, void *stream);
/* Weights in the ring kernel's tile-image layout (w_tiled = 1 above and in chirrup_gemm_problem): W [N][K] binary16,
 * N % 128 == 0, K % 64 == 0, re-laid so that each (128 rows x 64 k) tile is 16 KiB of consecutive bytes in the order the
 * kernel keeps it in LDS.  A 1-KiB LDS-DMA wave-instruction then reads 1 KiB of consecutive memory instead of eight
 * 128-B pieces of eight rows K*2 bytes apart.  Wt: N*K elements, must not overlap W.  The row-major matrix is still
 * what every other consumer (library GEMMs of the prefill path) needs. */
int skinny_tile_weight(int N, int K, const void *W, int64_t ldw, void *Wt, void *stream);
/* ... and back: the row-major matrix (row stride ldw) of a tile image, for callers that keep only the images and need a
 * row-major operand now and then (library GEMMs of prefill chunks above 256 rows). */
int skinny_untile_weight(int N, int K, const void *Wt, void *W, int64_t ldw, void *stream);
/* The same for mm8t_seq's uint8 weights wT [M_out][N_in] (N = M_out, K = N_in): 8-KiB tile images, w_tiled = 1 there. */
int skinny_tile_weight_u8(int N, int K, const void *W, int64_t ldw, void *Wt, void *stream);

/*
 * mm8 (w8a16) on the matrix cores: same quantisation and result as mm8_seq, but the uint8 weights
 * are given K-CONTIGUOUS, wT[M_out][N_in] (the transpose of the reference's w[N_in][M_out]; weights
 * are static, the transpose is done once at load).  Evaluated in the reference's algebraically split
 * form (scripts/test_mm8/benchmark.py:167-179): xs = fp16(x*ry) through MFMA against the exact
 * uint8->binary16 weights, then y = rx*(acc + 0.5*sum xs) + sum x*my + mx*sum x.  act as above.
 * Replaces the tiled / WMMA variants scripts/test_mm8/rwkv_pip_operators.cu:205-558.  Any B: more than 256
 * rows (chunked prefill) are processed 256 at a time, each block re-streaming the weights.
 */
int64_t mm8t_workspace_bytes(int B, int N_in, int M_out, int splits);
int mm8t_seq(int B, int N_in, int M_out, const void *x, int x_stride, const void *wT, int64_t w_stride, int w_tiled,
             const void *mx, const void *rx, const void *my, const void *ry, void *y, int y_stride, int act,
             int splits, void *workspace, void *stream);
/* mm8t_seq with the arithmetic of the reference's mm8_seq -- kernel_mm_seq_fp16i8, scripts/test_mm8/rwkv_pip_operators.cu:59-83:
 * every product and every sum in binary32 -- at matrix-core speed: x*ry (two binary16 numbers: <= 22 significant bits, exact in
 * binary32) is split EXACTLY into hi + lo binary16 operands, multiplied in two passes with binary32 accumulation and reduced
 * with the rank-1 corrections.  Differs from the as-coded kernel only by the order of the binary32 sums (~1e-5 of the row
 * scale; mm8t_seq, which rounds xs to binary16 like the reference's mm8_seq_opt, rwkv_pip_wrapper.cpp:148-191: 2e-3).  Same
 * arguments as mm8t_seq; workspace: mm8t_exact_workspace_bytes. */
/* The dequantised matrix of mm8t_seq's weights as binary16 [M_out][N_in] row-major: out[m][k] = fp16(((q + 0.5) * rx[m]) * ry[k] +
 * mx[m] + my[k]) (the as-coded dequantisation, rwkv_pip_operators.cu:76-79, rounded once).  For products of more than 256 rows
 * (chunked prefill), which are MFMA-bound: one pass into a reused scratch, then a binary16 GEMM (the reference's own mm8_seq_opt
 * casts the uint8 matrix to binary16 in front of cuBLAS the same way, rwkv_pip_wrapper.cpp:163-176).  wT as in mm8t_seq. */
int mm8_dequant_f16(int M_out, int N_in, const void *wT, int64_t w_stride, int w_tiled, const void *rx, const void *mx, const void *ry,
                    const void *my, void *out, void *stream);
int64_t mm8t_exact_workspace_bytes(int B, int N_in, int M_out, int splits);
int mm8t_seq_exact(int B, int N_in, int M_out, const void *x, int x_stride, const void *wT, int64_t w_stride, int w_tiled,
                   const void *mx, const void *rx, const void *my, const void *ry, void *y, int y_stride, int act,
                   int splits, void *workspace, void *stream);

/*
 * Penalties + greedy token selection in one pass (rows decoded with temperature 0).
 * Replaces chirrup/worker.py:724-740 for those rows: occurrence *= decay; logits -= alpha_presence +
 * occurrence * frequency_penalty (binary32, rounded back into the binary16 logits in place);
 * ids[row] = argmax (chirrup/utils/samplers.py:195-221 with temperature 0; ties -> lowest id).
 * logits [B][V] binary16; occurrence, alpha_presence float [n_slots][V]; penalty_decay,
 * frequency_penalty binary16 [n_slots]; row b uses slot slot_idx[b] (or b).  occurrence == NULL:
 * arg-max only.  V % 8 == 0.
 */
int rwkv7_penalize_argmax(int B, int V, void *logits, float *occurrence, const float *alpha_presence,
                          const void *penalty_decay, const void *frequency_penalty, const int32_t *slot_idx,
                          int32_t *ids, void *stream);
/* The device-side consequences of sampling ids[row] for slot slot_idx[row] (row when slot_idx is NULL), row < n
 * (reference: chirrup/worker.py:527-535): last_ids[slot] = id; occurrence[slot][id] += penalty_weight[id];
 * alpha_presence[slot][id] = presence[slot * presence_stride].  occurrence / alpha_presence fp32 [n_slots][V],
 * penalty_weight fp32 [V], last_ids int32 [n_slots].  An id outside [0, V) only updates last_ids.
 * status_dst (may be NULL): *status_dst = status_src ? *status_src : 0 -- the sticky launch-status word of the time-mix launches
 * (rwkv7_tmix_gemms) placed behind the ids (status_dst = ids + n of a buffer of n + 1), so that the ONE device-to-host copy of a
 * step's ids also tells the host whether that step's launches gave up a bounded wait. */
int rwkv7_commit_sampled(int n, int V, const int32_t *ids, const int32_t *slot_idx, int32_t *last_ids, float *occurrence,
                         const float *penalty_weight, float *alpha_presence, const float *presence, int64_t presence_stride,
                         const int32_t *status_src, int32_t *status_dst, void *stream);
/* The penalty step without the dense pass over the tables (round 4).  A slot's occurrence / alpha_presence rows are zero except at
 * the ids it has sampled, so beside the (unchanged, dense, exact) tables every slot keeps the list of those ids: pen_list int32
 * [n_slots][cap], pen_count int32 [n_slots] (entries used; -1 = more than cap distinct ids: the slot takes the dense pass until it
 * is reset), pen_bits uint32 [n_slots][V / 32] (an id is listed once).  rwkv7_commit_sampled_listed = rwkv7_commit_sampled + the
 * list update; rwkv7_penalize_argmax_listed = rwkv7_penalize_argmax touching only the listed entries -- per element the same
 * arithmetic, which is the identity on entries that are zero: logits, occurrence and ids are bit-identical to the dense entry
 * points'.  Resetting a slot: zero its two table rows (or their listed entries), its pen_bits row and pen_count[slot].  The rows
 * of ONE commit launch must address distinct slots.  V % 32 == 0. */
int rwkv7_penalize_argmax_listed(int B, int V, void *logits, float *occurrence, const float *alpha_presence, const void *penalty_decay,
                                 const void *frequency_penalty, const int32_t *slot_idx, int32_t *ids, const int32_t *pen_list,
                                 const int32_t *pen_count, int cap, void *stream);
int rwkv7_commit_sampled_listed(int n, int V, const int32_t *ids, const int32_t *slot_idx, int32_t *last_ids, float *occurrence,
                                const float *penalty_weight, float *alpha_presence, const float *presence, int64_t presence_stride,
                                const int32_t *status_src, int32_t *status_dst, int32_t *pen_list, int32_t *pen_count,
                                uint32_t *pen_bits, int cap, void *stream);

/* The two ends of a decode step around the layers (Albatross/rwkv7.py:503-517 `_pre`: the embedding gather; :561-563 `_post`:
 * state[2] += T), each one launch.  rwkv7_embed_rows: x[b][t] = emb[token], token = tokens[b*T + t], or -- when that is negative and
 * `feedback` is given -- feedback[slot_idx[b]] (feedback[b] without slot_idx): the id the sampler left for that slot one step ago
 * (chirrup/worker.py:527: the reference round-trips it through the host).  emb binary16 [V][C], C % 8 == 0, x binary16 [B*T][C]; a
 * token outside [0, V) gives a zero row.  zero_words / n_zero: int32 words zeroed by the same launch (the caller's launch-sync words:
 * tile counters and time-mix hand-off words of the stream), or NULL / 0.  elapsed_rows (or NULL): elapsed_rows[b] = elapsed_pool[slot
 * of row b] -- the slot table's step counters in batch-row order, as the WKV7 entries take them.
 * rwkv7_advance_elapsed: elapsed[slot_idx[b]] += T for b < B (elapsed[b] without slot_idx; slots distinct). */
int rwkv7_embed_rows(int B, int T, int C, int V, const void *emb, const int64_t *tokens, const int32_t *slot_idx,
                     const int32_t *feedback, void *x, int32_t *zero_words, int n_zero, const int32_t *elapsed_pool,
                     int32_t *elapsed_rows, void *stream);
int rwkv7_advance_elapsed(int B, int T, const int32_t *slot_idx, int32_t *elapsed, void *stream);
/* dst[slot_idx[b]][0..C) = src[slot_idx[b]][0..C) for b < B: binary16 tables [n_slots][C] (C % 8 == 0, slots distinct) -- the commit of
 * a chunk's token-shift carry into the slot table (the T > 1 form of rwkv7_add_ln_mix writes the carry to a side table). */
int rwkv7_copy_slot_rows(int B, int C, const int32_t *slot_idx, const void *src, void *dst, void *stream);
/* Parallel choices of one prompt: group g < n_groups copies slot src[g] of the worker's state tables to every slot
 * dst[dst_offs[g] .. dst_offs[g + 1]), bit for bit -- shift binary16 [L][2][S][C], wkv binary16 [L][S][H][64][64] and elapsed int32
 * [S].  ONE launch for all groups; a workgroup reads its piece of a source layer once and writes it to each destination of its group
 * (16 B per lane, integer vectors: NaN payloads and -0 survive).  Destinations must be distinct, in [0, S) and no group's source
 * (the caller checks; slots outside [0, S) are skipped).  C == H * 64; shift and wkv 16-byte aligned.  n_groups == 0 launches
 * nothing.  Bytes per group: one slot's state read once, written once per destination. */
int rwkv7_fork_states(int n_groups, int L, int S, int C, int H, const int32_t *src, const int32_t *dst_offs, const int32_t *dst,
                      void *shift, void *wkv, int32_t *elapsed, void *stream);
/* Text embeddings: pools the ln_out rows of a prefill chunk per sequence.  xo binary16 [B][T][C] (the rows the head would multiply);
 * for i < n_seq with b = seq[i], s = slot[i], a = t0[i] in [0, T] (clamped to it):
 *   acc_sum[s][c]  continues its running binary32 sum over t = a..T-1 STRICTLY in token order, one channel at a time:
 *                  sum = sum + (float)xo[b][t][c], no contraction -- so a sum depends on the rows and their order only, not on how a
 *                  prompt was cut into chunks (the same rows pooled in one launch or in several give the same bits);
 *   acc_last[s]    = xo[b][T-1], copied as bits, when a < T;
 *   acc_count[s]  += T - a.
 * acc_sum float [n_slots][C], acc_last binary16 [n_slots][C], acc_count int32 [n_slots]; rows of the three tables that are not listed
 * (and those of a sequence with a == T) are not written.  Slots must be distinct; a b outside [0, B) or an s outside [0, n_slots) is
 * skipped.  ONE launch: parallel over channels and sequences only, no floating-point atomics, no split over t (loads are issued
 * ahead, the additions stay in order).  n_seq == 0 launches nothing.  C % 8 == 0; xo, acc_sum and acc_last 16-byte aligned.
 * Bytes: each pooled row read once (B*T*C*2 at most) + 6*C bytes of accumulators read and written per listed sequence. */
int rwkv7_pool_rows(int n_seq, int B, int T, int C, const void *xo, const int32_t *seq, const int32_t *t0, const int32_t *slot, int n_slots,
                    float *acc_sum, void *acc_last, int32_t *acc_count, void *stream);

/*
 * Sort-free top-p / top-k / temperature sampling of n_rows rows of `logits` (binary16 [B][V], V <= 65536,
 * V % 8 == 0), row list `rows` (indices into logits / ids).  Semantics of
 * sample_logits_rwkv_pip_compatible (chirrup/utils/samplers.py:171-255): softmax, drop everything below
 * the probability at which the descending cumulative sum reaches top_p, optional top-k, probs**(1/T), one
 * draw.  temperature / top_p binary16 and top_k int32 are per-slot tables addressed through slot_idx[row]
 * (or row); uniform[i] in [0,1) is the random number for rows[i]; ids[rows[i]] receives the token.
 * Ties at the top-k boundary are all kept; the draw is an inverse-CDF walk in token order.
 */
int rwkv7_sample_topp(int n_rows, int V, const void *logits, const int32_t *rows, const void *temperature,
                      const void *top_p, const int32_t *top_k, const int32_t *slot_idx, const float *uniform,
                      int32_t *ids, void *stream);

/*
 * Log-probabilities of n_rows rows of binary16 logits (V <= 65536, V % 8 == 0): launch row i reads logits row rows[i] (or i).
 * m = max l, Z = sum exp(l - m) in binary32 in a fixed order, lp(j) = (l_j - m) - log Z.  out_lp binary32 [n_rows][K + 1]:
 * out_lp[i][0] = lp of the target id target_ids[target_rows[i]] (target_ids[i] without target_rows; NaN when the id is outside
 * [0, V) or target_ids is NULL), out_lp[i][1 + k] = lp of out_ids[i][k] (int32 [n_rows][K]): the K (0..20, K <= V) ids of largest
 * logit, by logit descending then id ascending.  A row's outputs are bit-identical in every launch, whatever rows share it and
 * whatever K (a smaller K gives a prefix of the entries).  The target ids are read on the device: the sampler's ids buffer of the
 * same stream, with no host round trip.
 */
int rwkv7_token_logprobs(int n_rows, int V, int K, const void *logits, const int32_t *rows, const int32_t *target_ids,
                         const int32_t *target_rows, float *out_lp, int32_t *out_ids, void *stream);

/*
 * Per-request seeded uniforms for the sampler (Philox4x32-10, M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9,
 * W1 = 0xBB67AE85).  For each i < n_rows: r = rows[i], s = slot_idx[r].  When seeded[s] != 0:
 * uniform[i] = (x0 >> 8) * 2^-24 with x0 the first word of Philox(counter = (counters[s], seeded[s] - 1, 0, 0),
 * key = (lo32(seeds[s]), hi32(seeds[s]))), then counters[s] += 1.  Rows whose slot is not seeded keep uniform[i].
 * seeded[s] is 0 (unseeded) or 1 + j for choice j of a request with parallel choices (j = 0 for a single choice): counter word 1
 * is the choice's stream.  A slot appears at most once among the rows.  n_rows == 0 launches nothing; seeds must be 8-byte aligned.
 */
int rwkv7_seeded_uniform(int n_rows, const int32_t *rows, const int32_t *slot_idx, const uint64_t *seeds,
                         const int32_t *seeded, uint32_t *counters, float *uniform, void *stream);

/*
 * Logit bias of n_rows rows of binary16 logits [n_rows][V], in place.  Row i uses the list of slot s = slot_idx[i] (or i):
 * counts[s] entries (at most cap) of ids int32 [.][cap] and values binary32 [.][cap].  For each entry with 0 <= id < V and a
 * finite logit l: logits[i][id] = fp16(clamp(float(l) + value, -65504, 65504)), one rounding; other entries are skipped and
 * non-finite logits stay as they are.  The ids of one list must be distinct.  n_rows == 0 launches nothing.
 */
int rwkv7_apply_logit_bias(int n_rows, int V, int cap, void *logits, const int32_t *slot_idx, const int32_t *counts,
                           const int32_t *ids, const float *values, void *stream);

/*
 * Guided decoding (chirrup_amd/guided.py, DESIGN.md "Guided decoding").  All guides of a worker share one pool of state rows:
 * guide_next int32 [P][256] (entries are absolute pool rows, -1 = dead) and guide_allow uint32 [P][V/32] (bit t of a row: token t
 * is allowed in that state).  A slot's constraint is guide_state[slot]: a pool row, or -1 for an unconstrained slot.  The token
 * byte table is tok_off int32 [V + 1] (ascending offsets into tok_bytes; an id without a vocabulary entry has an empty range).
 * A row index outside [0, P) met anywhere counts as dead / unconstrained.
 *
 * rwkv7_guide_build fills guide_allow rows [row0, row0 + S) (row0 + S <= P, S <= 65535, V % 64 == 0, guide_allow 8-byte aligned):
 * bit (s, t) is set iff token t has bytes and walking them from row row0 + s through guide_next never meets a dead entry; for the
 * n_special ids in `special` (the request's stop tokens) the bit is accept[s] != 0 instead (accept uint8 [S]) -- their bytes are
 * not walked.  guide_next rows [row0, row0 + S) must already hold the guide (stream order).
 *
 * rwkv7_guide_apply: for i < n_rows, r = rows[i] (a row of binary16 logits [n_logit_rows][V], V % 32 == 0, 16-byte aligned),
 * s = slot_idx[r] (or r), st = guide_state[s] (n_slots entries): when st >= 0, logits[r][t] = -inf for every t whose bit in
 * guide_allow[st] is clear (NaN included); allowed entries and rows of unconstrained slots are not written.
 *
 * rwkv7_guide_advance: for i < n_rows, r = rows[i], s = slot_idx[r] (or r): when guide_state[s] >= 0 and ids[r] (n_ids entries)
 * has bytes, guide_state[s] = the row after walking them; the state is left as it is when the walk dies (a stop id, a row that
 * will be dropped) or the id is outside [0, V) or has no bytes.  A slot appears at most once among the rows.
 *
 * n_rows == 0 (S == 0) launches nothing.
 */
int rwkv7_guide_build(int S, int row0, int P, int V, const int32_t *guide_next, const int32_t *tok_off, const uint8_t *tok_bytes,
                      int n_special, const int32_t *special, const uint8_t *accept, uint32_t *guide_allow, void *stream);
int rwkv7_guide_apply(int n_rows, int n_logit_rows, int V, int P, void *logits, const int32_t *rows, const int32_t *slot_idx,
                      int n_slots, const int32_t *guide_state, const uint32_t *guide_allow, void *stream);
int rwkv7_guide_advance(int n_rows, int n_ids, int V, int P, const int32_t *rows, const int32_t *slot_idx, int n_slots,
                        const int32_t *ids, const int32_t *tok_off, const uint8_t *tok_bytes, const int32_t *guide_next,
                        int32_t *guide_state, void *stream);

/*
 * Grammar-guided decoding (chirrup_amd/guided.py: compile_grammar / StackDFA, DESIGN.md "Grammar-guided decoding"): a guide is a
 * deterministic call/return automaton over bytes, a slot's constraint a state row and a stack of call sites.  The grammar guides
 * of a worker share a pool of P rows of their own; a guide with S states, n call sites and k stop ids occupies
 * R = max(S, n + 1, k + 1) consecutive rows from its base row0, its states first:
 *
 *   gr_next  int32  [P][256]  row of a state: >= 0 a plain edge to an absolute pool row (the only move that consumes the byte),
 *                             -1 no move of the state's own, -(c + 1) for 1 <= c <= n: call site c (push c, go on with the same
 *                             byte at the site's start row)
 *   gr_meta  int32  [P][8]    words 0..3 describe the row as a state: flags (bit 0 final state of its rule, bit 1 its rule is
 *                             called, so a final state returns: pop c, go on with the same byte at site c's after row), need (the
 *                             least further stack depth a completion requires), row0 of its guide, the guide's depth bound
 *                             (1..CHIRRUP_GRAMMAR_STACK_DEPTH).  Words 4..6 of row row0 + c are call site c of the guide: start
 *                             row, after row (absolute), need = max(1 + need[start], need[after]).  Word 7 of row row0 is k, of
 *                             row row0 + 1 + j the j-th stop id.
 *   gr_allow, gr_maybe uint32 [P][V/32]  bit t of a state's row: token t is allowed under every stack / under some stacks only
 *   gr_state int32  [n_slots]      a slot's current row, -1 for a slot without a grammar
 *   gr_stack uint64 [n_slots][4]   32 call-site bytes, the top in the low byte of word 0, zero above the bottom (the depth is the
 *                                  number of non-zero bytes)
 *
 * A walk of bytes from (row, stack, depth d) takes, per byte: the plain edge to row v when d + need[v] <= bound; else the call
 * site c when d + need[c] <= bound and d < CHIRRUP_GRAMMAR_STACK_DEPTH; else, from a final state of a called rule with d > 0, the
 * return; else it dies.  The text may end where the returns reach a final state with d == 0.  A row or site outside the pool met
 * anywhere counts as dead.  The token byte table (tok_off, tok_bytes) is that of rwkv7_guide_build.
 *
 * rwkv7_grammar_build fills gr_allow / gr_maybe rows [row0, row0 + S) (V % 64 == 0, both 8-byte aligned; gr_next / gr_meta rows
 * of the guide already written, stream order): the allow bit of (s, t) is set iff t has bytes and all of them take plain edges
 * into rows with need == 0; the maybe bit iff allow is clear and the first byte that does not is a plain edge into a row with
 * need > 0, a call, or has no move in a final state of a called rule.  For the n_special stop ids the bits are instead
 * allow = final && !called, maybe = final && called of row row0 + s.
 *
 * rwkv7_grammar_apply: as rwkv7_guide_apply, with token t allowed iff its allow bit is set, or its maybe bit is set and its walk
 * from the slot's (row, stack) survives -- for a stop id of the guide, iff the text may end there.
 *
 * rwkv7_grammar_advance: as rwkv7_guide_advance; the walk of ids[r]'s bytes moves gr_state[s] and gr_stack[s], or leaves both
 * when it dies.  rwkv7_grammar_reset: for i < n, gr_state[slots[i]] = start[i] (a guide's row0, or -1) and the stack is emptied;
 * slots outside [0, n_slots) are skipped.
 */
#define CHIRRUP_GRAMMAR_STACK_DEPTH 32
#define CHIRRUP_GRAMMAR_CALL_SITES 255
int rwkv7_grammar_build(int S, int row0, int P, int V, const int32_t *gr_next, const int32_t *gr_meta, const int32_t *tok_off,
                        const uint8_t *tok_bytes, int n_special, const int32_t *special, uint32_t *gr_allow, uint32_t *gr_maybe,
                        void *stream);
int rwkv7_grammar_apply(int n_rows, int n_logit_rows, int V, int P, void *logits, const int32_t *rows, const int32_t *slot_idx,
                        int n_slots, const int32_t *gr_state, const uint64_t *gr_stack, const int32_t *gr_next, const int32_t *gr_meta,
                        const uint32_t *gr_allow, const uint32_t *gr_maybe, const int32_t *tok_off, const uint8_t *tok_bytes,
                        void *stream);
int rwkv7_grammar_advance(int n_rows, int n_ids, int V, int P, const int32_t *rows, const int32_t *slot_idx, int n_slots,
                          const int32_t *ids, const int32_t *tok_off, const uint8_t *tok_bytes, const int32_t *gr_next,
                          const int32_t *gr_meta, int32_t *gr_state, uint64_t *gr_stack, void *stream);
int rwkv7_grammar_reset(int n, int n_slots, const int32_t *slots, const int32_t *start, int32_t *gr_state, uint64_t *gr_stack,
                        void *stream);

/*
 * Beam search (DESIGN.md "Beam search").  A beam group of width W (2..CHIRRUP_BEAM_MAX_W) with S stop ids (S >= 1, W + S <= 20) holds
 * W slots of the worker's state tables, one per position.  Every step, rwkv7_token_logprobs gives each position's K = W + S most likely
 * ids; rwkv7_beam_select picks the next beams of every group of the step on the device and rwkv7_beam_copy_states moves the states
 * the selection asks for -- the host learns both one step late.
 *
 * rwkv7_beam_select: one launch, one wave per group g < n_groups.  desc int32 [n_groups][CHIRRUP_BEAM_DESC_WORDS] describes a group:
 *   desc[0] = W, desc[1] = S, desc[2 + p] = the row of position p in lp / cand_ids, desc[10 + p] = its element of ids_out (its row of
 *   the sampler's ids buffer), desc[18 + p] = its slot, desc[26 + j] = stop id j.
 * lp binary32 and cand_ids int32 hold k_cols >= K columns per row (row strides lp_stride / ids_stride in elements, n_lp_rows rows):
 * entry k of a row is the k-th candidate (logit descending, then id ascending) and its log-probability.  scores binary32 [n_slots].
 *   Candidate (b, k): cum = scores[slot b] + lp[row b][k], one binary32 addition; a NaN cum becomes -inf.
 *   Order: cum descending, then b ascending, then k ascending -- computed by counting, per candidate, the candidates that beat it:
 *   independent of lane scheduling, no floating-point atomics.
 *   Walk in that order with pos = candidates seen so far: a candidate whose id is a stop id is recorded as finished (parent b, id,
 *   cum) iff pos < W and cum is finite, and never becomes a beam; any other candidate is the next beam of rank 0, 1, ...; the walk
 *   ends with W next beams.
 *   Placement in rank order: the first chosen child of parent b stays in position b; every further child takes the lowest position
 *   whose old beam has no chosen child and gets copy_src = the slot of b.  No copy destination is a copy source.
 * Outputs: ids_out[desc[10 + p]] = the id of position p (n_ids elements); scores[slot p] = its cum; and out int32
 * [n_groups][CHIRRUP_BEAM_OUT_WORDS]: out[0 + p] = parent (old position), out[8 + p] = rank, out[16 + p] = copy_src (a slot, or -1),
 * out[24 + p] = id, out[32 + p] = the bits of its score, out[40] = finished records n, out[41 + j] / out[49 + j] / out[57 + j] = parent,
 * id and cum bits of record j < n.  Unused entries (p >= W, j >= n) are -1 (-inf bits for scores, 0 for cum).
 * A group whose descriptor is out of range (W, S, K > k_cols, a row, element or slot outside its table) writes nothing; elements of
 * groups that are not listed are untouched.  The slots of one launch must be distinct.  n_groups == 0 launches nothing.
 * CHIRRUP_E_SHAPE: n_groups < 0 or > 65535, k_cols outside 3..20, a stride below k_cols, a non-positive table size.
 *
 * rwkv7_beam_copy_states: grid (pieces of a layer, L, n_groups * CHIRRUP_BEAM_MAX_W) like rwkv7_fork_states.  Position z = g * 8 + p reads
 * s = copy_src[g * group_stride + p] (e.g. out + 16 of rwkv7_beam_select with group_stride CHIRRUP_BEAM_OUT_WORDS) and d = dst[z] FROM
 * DEVICE MEMORY; when both are in [0, S) and differ, slot s of shift binary16 [L][2][S][C], wkv binary16 [L][S][H][64][64] and elapsed
 * int32 [S] is copied to slot d, bit for bit (16 B per lane, integer vectors: NaN payloads and -0 survive); otherwise the workgroup
 * returns at once.  Destinations must be distinct and no position's source (the placement rule guarantees it).  C == H * 64; shift
 * and wkv 16-byte aligned; n_groups <= 8191; group_stride >= 8.  n_groups == 0 launches nothing.
 */
#define CHIRRUP_BEAM_MAX_W 8
#define CHIRRUP_BEAM_DESC_WORDS 44
#define CHIRRUP_BEAM_OUT_WORDS 65
int rwkv7_beam_select(int n_groups, int n_lp_rows, int k_cols, const float *lp, int64_t lp_stride, const int32_t *cand_ids,
                      int64_t ids_stride, const int32_t *desc, float *scores, int n_slots, int32_t *ids_out, int n_ids, int32_t *out,
                      void *stream);
int rwkv7_beam_copy_states(int n_groups, int L, int S, int C, int H, const int32_t *copy_src, int64_t group_stride, const int32_t *dst,
                           void *shift, void *wkv, int32_t *elapsed, void *stream);

/*
 * The pieces of mm8t_seq for a decode step that folds the mm8 prologue / reduce launches into the neighbouring kernels
 * (chirrup_amd/rwkv7.py, ffn_dtype = int8): LN kernel (prologue of ffn.key, rwkv7_add_ln_mix_mm8) -> mm8t_gemm_partial ->
 * mm8_reduce_rows (corrections + relu^2 of ffn.key AND the prologue of ffn.value) -> mm8t_gemm_partial -> next LN kernel
 * (corrections of ffn.value).  Same arithmetic and rounding points as mm8t_seq.
 * mm8t_gemm_partial: core sums of xs [B][N_in] (B <= 256) against wT into partials [splits][B][M_out]; returns the split
 *   count used (> 0) or a negative error.
 * mm8_reduce_rows: y = act(rx*(sum partials - 1023.5*S[.][0]) + S[.][1] + mx*S[.][2]) (y may be NULL), and when xs2 != NULL the
 *   prologue of the next product: xs2 = fp16(y*ry2), S2 = {sum xs2, sum y*my2, sum y} per row.  Row sums travel as partial
 *   sums: S is [B][S_parts][3], S2 is written as [B][mm8_row_parts(M_out)][3] (one part per 1024 columns), to be added in
 *   part order by the consumer (rwkv7_add_ln_mix_mm8: in_S_parts; this function: S_parts).
 */
int mm8_row_parts(int M_out);
int mm8t_gemm_partial(int B, int N_in, int M_out, const void *xs, int xs_stride, const void *wT, int64_t w_stride,
                      int w_tiled, int splits, int row_halves, float *partials, void *stream);
int mm8_reduce_rows(int B, int M_out, int splits, const float *partials, const void *rx, const void *mx, const float *S,
                    int S_parts, int act, void *y, int y_stride, const void *ry2, const void *my2, void *xs2, float *S2,
                    void *stream);
/* mm8t_gemm_partial + mm8_reduce_rows in ONE launch (unsplit; for products with enough 128-column tiles to fill the chip,
 * e.g. ffn.key with row_halves): corrections, relu^2 (act = 1), y (may be NULL) and the next product's prologue (xs2 and S2
 * [B][mm8_tile_parts(M_out)][3]; may be NULL) come out of the GEMM's own epilogue.  S: [B][S_parts][3].  B <= 256,
 * M_out < 32768, M_out % 8 == 0, 16-byte aligned vectors.  Same element arithmetic as mm8_reduce_rows; the row sums S2 are split per 128-column tile. */
int mm8_tile_parts(int M_out);
int mm8t_gemm_fused(int B, int N_in, int M_out, const void *xs, int xs_stride, const void *wT, int64_t w_stride, int w_tiled,
                    const void *rx, const void *mx, const float *S, int S_parts, int act, void *y, int y_stride,
                    const void *ry2, const void *my2, void *xs2, float *S2, int row_halves, void *stream);
/* mm8t_gemm_fused for few rows: the product is split `splits` ways over K (2..4; 0 = the library's choice) and the last of a tile's
 * workgroups to finish adds the other slices' sums to its own, in slice order, and runs the same epilogue -- no partials for a
 * consumer and no mm8_reduce_rows launch.  partials: room for splits x B x M_out binary32 values (hand-off slabs); tile_counters: as
 * skinny_gemm_f16.  B <= 64 and (splits - 1) * B <= 96, else CHIRRUP_E_UNSUPPORTED (use mm8t_gemm_partial + mm8_reduce_rows).
 * Same sums as mm8_reduce_rows over mm8t_gemm_partial at the same split count, bit for bit; S2 has mm8_tile_parts(M_out) parts per row
 * (as mm8t_gemm_fused), not mm8_row_parts. */
int mm8t_gemm_fused_split(int B, int N_in, int M_out, const void *xs, int xs_stride, const void *wT, int64_t w_stride, int w_tiled,
                          const void *rx, const void *mx, const float *S, int S_parts, int act, void *y, int y_stride,
                          const void *ry2, const void *my2, void *xs2, float *S2, int splits, float *partials,
                          void *tile_counters, void *stream);

/*
 * MXFP4 (w4a16) weights, csrc/mxfp4.hip: OCP Microscaling FP4.  A block of 32 E2M1 codes along K (the reduction dimension, N_in of
 * the Linear) shares one E8M0 scale byte s:  w~[n][k] = E2M1(code[n][k]) * 2^(s[n][k / 32] - 127);  code bit 3 is the sign, codes
 * 0..7 are 0, .5, 1, 1.5, 2, 3, 4, 6.  The caller passes only scale bytes 114..140 (2^-13 .. 2^13: every w~ is then +-0 or a normal
 * binary16 number); the kernels do not define anything else (chirrup_amd.quant refuses it on the host).
 *
 * mxfp4_tile_weight: codes [M_out][N_in / 2] uint8 row-major (row stride ld_codes bytes, a multiple of 4; low nibble = even k) and
 *   scales [M_out][N_in / 32] uint8 (row stride ld_scales) -> Wt, mxfp4_tiled_bytes(M_out, N_in) bytes (0: shape refused) of tile
 *   images: tile (n / 128, k / 64) is 4352 consecutive bytes, 128 rows x 32 code bytes then 128 rows x 2 scale bytes; code byte
 *   position 8 q + 4 s + j of a row holds k = 32 s + 8 q + 2 j, + 1 of the K-block.  M_out % 128 == 0, N_in % 64 == 0.
 * mxfp4_dequant_f16: Wt -> w~ as binary16 [M_out][N_in], row stride ld_out elements (a multiple of 8), exact.  What a forward of
 *   more than 256 rows multiplies through the library GEMM, like mm8_dequant_f16.
 * mxfp4_gemm: Y [M][N] = act(X [M][K] . w~ [N][K]^T), M = 1..256 rows, N % 128 == 0, K % 64 == 0: exact products, binary32
 *   accumulation, ONE rounding to binary16 after act (0 none, 1 relu(fp16(.))^2).  splits: K-slices (0 = the library's choice; cut
 *   back to a divisor of K / 64: mxfp4_gemm_splits tells); workspace: mxfp4_gemm_workspace_bytes, 16-byte aligned, needed above one
 *   slice.  X 16-byte aligned, ldx % 8 == 0; Y 8-byte aligned, ldy % 4 == 0.
 * mxfp4_gemm_partial: the K-slices' binary32 sums as planes partials [splits_used][M][N] (16-byte aligned) for a consumer that
 *   adds them (rwkv7_add_ln_mix: delta_partials).  Returns splits_used, or -1000 - error.
 */
int64_t mxfp4_tiled_bytes(int M_out, int N_in);
int mxfp4_tile_weight(int M_out, int N_in, const void *codes, int64_t ld_codes, const void *scales, int64_t ld_scales, void *Wt,
                      void *stream);
int mxfp4_dequant_f16(int M_out, int N_in, const void *Wt, void *out, int64_t ld_out, void *stream);
int mxfp4_gemm_splits(int M, int N, int K, int splits);
int64_t mxfp4_gemm_workspace_bytes(int M, int N, int K, int splits);
int mxfp4_gemm(int M, int N, int K, const void *X, int ldx, const void *Wt, void *Y, int ldy, int act, int splits, void *workspace,
               void *stream);
int mxfp4_gemm_partial(int M, int N, int K, const void *X, int ldx, const void *Wt, int splits, float *partials, void *stream);

/*
 * MXINT8 prefix-state arena, csrc/state_codec.hip: the head states of ONE slot of the worker's table wkv binary16 [L][S][H][64][64]
 * <-> a packed arena row uint8 [L][H][CHIRRUP_MXINT8_HEAD_BYTES].  A head is 4096 int8 codes in element order, then 128 E8M0 scale
 * bytes, one per block of 32 consecutive elements (a 64-element row is two blocks).  scale byte = e + 127, e the smallest integer
 * with amax <= 127 * 2^(e-6), held to [-18, 15] (an all-zero block: -18), from the bits of amax: with amax = f * 2^p, 1 <= f < 2,
 * e = p when f <= 127/64, else p + 1.  code = clamp(RNE(x * 2^(6-e)), -127, 127), two's complement, never -128; -0 gives code 0.
 * value = code * 2^(e-6): +-0 or a binary16 number for every code and exponent, so unpacking rounds nothing.  For a block not held
 * at e = 15, |x - value| <= 2^(e-7) < amax / 127; |x| > 65024 saturates to +-65024.  A block holding a NaN or an infinity takes
 * scale byte 0xFF and codes 0; scale byte 0xFF unpacks to 32 quiet NaNs (0x7E00).  Other scale bytes outside 109..142 unpack as
 * the nearest of the two.
 * Grid (H, L), 16-byte loads and stores, no LDS; 8192 + 4224 bytes per head.  0 <= slot < S; wkv and packed 16-byte aligned.  Only
 * slot `slot` is read (pack) or written (unpack); the packed row is written (pack) or read (unpack) in full.
 */
#define CHIRRUP_MXINT8_HEAD_BYTES 4224
int rwkv7_state_pack(int L, int S, int H, int slot, const void *wkv, void *packed, void *stream);
int rwkv7_state_unpack(int L, int S, int H, int slot, const void *packed, void *wkv, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CHIRRUP_AMD_H */
