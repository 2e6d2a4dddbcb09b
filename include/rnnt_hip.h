/*
 * rnnt_hip.h — C ABI of librnnt_hip.so: the MI355X (gfx950) native RNN-Transducer training hot path.
 *
 * The reference (YooSungHyun/RNNTransducer) has NO native code and therefore no FFI of its own
 * (SURVEY.md §0, §2b): every kernel it runs comes from a dependency.  This header declares the entry
 * points a maintainer would bind in place of those dependency calls; each one cites the reference call
 * site it replaces (paths relative to the reference repo).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions:
 *   - plain `extern "C"`, raw device pointers + explicit dims, `void* stream` is a hipStream_t;
 *   - return 0 on success, <0 on error; rnnt_hip_last_error() gives a thread-local message;
 *   - the CALLER owns all memory incl. workspaces (sizes from *_workspace_bytes); the library never
 *     allocates or frees device memory, never synchronises the device (the two *_check / *_debug_read
 *     diagnostics aside) and keeps no global mutable state other than the opt-in profiler and launch record below
 *     (off by default: event lists / a text record, each behind a mutex) and the thread-local error string;
 *   - all float tensors are fp32, all lengths/labels int32, token ids int64 (dataloader.py:21-24,28-36);
 *   - "time-major" = (T,B,F) contiguous; "batch-major" = (B,T,F) contiguous.
 */
#ifndef RNNT_HIP_H_
#define RNNT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNNT_HIP_ABI_VERSION 4

#define RNNT_OK 0
#define RNNT_ERR_INVALID (-1)   /* bad argument (dims, alignment, null pointer)            */
#define RNNT_ERR_LAUNCH (-2)    /* hip launch / runtime error                              */
#define RNNT_ERR_UNSUPPORTED (-3) /* configuration outside what the kernels handle         */
#define RNNT_ERR_TIMEOUT (-4)   /* a persistent kernel gave up on an inter-CU wait         */

int rnnt_hip_version(void);
const char* rnnt_hip_last_error(void);
/* number of compute units the persistent LSTM kernels size their grid against (0 = no device) */
int rnnt_hip_device_cus(void);

/* ------------------------------------------------------------------------------------------------
 * Opt-in live profiler (used by bench.py only).  While enabled, every kernel launch below is bracketed by two
 * HIP events recorded on the launch stream; collect() synchronises on them, sums elapsed ms / algorithmic work /
 * launch counts per kernel kind, and resets.  Off by default.
 * `work` unit: FLOPs for RNNT_K_GEMM and RNNT_K_GEMM_HP, algorithmic bytes for all other kinds.
 * ---------------------------------------------------------------------------------------------- */
enum {
  RNNT_K_GEMM = 0,       /* gemm_f32_kernel                                   */
  RNNT_K_LSTM_FWD = 1,   /* lstm_fwd_kernel (persistent recurrence)           */
  RNNT_K_LSTM_BWD = 2,   /* lstm_bwd_kernel                                   */
  RNNT_K_LSE = 3,        /* lse_sep_kernel / lse_dense_kernel                 */
  RNNT_K_ALPHABETA = 4,  /* alphabeta_kernel                                  */
  RNNT_K_LATGRAD = 5,    /* grad_sep_kernel / grad_dense_kernel + reduce_dc   */
  RNNT_K_MISC = 6,       /* permutes, column sums, embedding, logits          */
  RNNT_K_GEMM_HP = 7,    /* gemm_hp_kernel (half-pair operands, f16 MFMA)     */
  RNNT_K_HP_SPLIT = 8,   /* fp32 -> half-pair operand conversion passes       */
  RNNT_K_COUNT = 9
};
int rnnt_hip_prof_enable(int on);
int rnnt_hip_prof_collect(double* ms, double* work, int64_t* count, int nkinds);

/* Opt-in record of the persistent recurrence kernels launched (used by the tests that pin which kernel instance a shape runs).
 * enable(1) clears the record and starts it, enable(0) stops it and keeps what it holds.  While on, every launch of a recurrence
 * kernel (rnnt_hip_lstm_fwd / _bwd and their _ex forms) appends one line: the kernel's device symbol, whose template arguments
 * name the instance.  launch_log() copies the record (NUL-terminated, truncated to n - 1 bytes) and returns its full length.
 * Off by default; when off a launch pays one branch. */
int rnnt_hip_lstm_launch_log_enable(int on);
int64_t rnnt_hip_lstm_launch_log(char* buf, size_t n);

/* ------------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on f32-input MFMA (v_mfma_f32_32x32x2_f32):  C = op(A) . op(B) (+ bias)
 * Replaces the BLAS calls behind nn.Linear / the hoisted LSTM input projection:
 *   networks/encoder.py:76,103 (out_proj), networks/decoder.py:80,124 (out_proj),
 *   networks/transducer.py:39,69 (fc), and the W_ih.x_t half of nn.LSTM (encoder.py:67-75,99).
 *
 *   A(m,k) = A[rowoff_a(m) + k*a_sk]            if a_mc == 0   (k-contiguous rows, a_sk must be 1)
 *   A(m,k) = A[k*a_sk + m]                      if a_mc == 1   (m-contiguous, "transposed" operand)
 *     rowoff_a(m) = a_rowidx ? a_rowidx[m]*a_si : (m / a_div)*a_so + (m % a_div)*a_si
 *   B(k,n) = B[n*b_sn + k*b_sk]                 exactly one of b_sn, b_sk is 1
 *   C(m,n) = C[(m / c_div)*c_so + (m % c_div)*c_si + n]
 * flags: see RNNT_GEMM_*.
 *
 * Arithmetic: inputs, outputs and accumulators are fp32 in every mode.  Default (RNNT_GEMM_MODE unset or "bf16x6"):
 * each fp32 operand is split EXACTLY into three bf16 pieces and the six piece products of fp32 weight run on
 * v_mfma_f32_32x32x16_bf16 (error per product <= ~3 * 2^-24, the order of fp32 rounding itself).  "f32": the
 * f32-input MFMA (exact fp32 fma chain).  "bf16x3": first-order pieces only (~2^-16 per product), opt-in.
 * ---------------------------------------------------------------------------------------------- */
#define RNNT_GEMM_GELU_A 1u      /* apply gelu_tanh to A elements on load  (transducer.py:38,68)   */
#define RNNT_GEMM_GELU_B 2u      /* apply gelu_tanh to B elements on load                          */
#define RNNT_GEMM_ACCUM 4u       /* C += result                                                    */
#define RNNT_GEMM_MUL_DGELU 8u   /* C = result * gelu_tanh'(aux(m,n)), aux laid out like C          */
#define RNNT_GEMM_EXACT_F32 16u  /* multiply on v_mfma_f32_32x32x2_f32 (bit-exact fp32 fma chains) even when the
                                  * library default is the split-bf16 form (see below)                      */
#define RNNT_GEMM_HP_F16 32u     /* rnnt_hip_gemm_hp / rnnt_hp_problem only: ONE product hi.hi per fp32 product (the lo
                                  * halves of both operands are not read) — f16 operand rounding, fp32 accumulation; see
                                  * RNNT_PRECISION_F16. */

typedef struct rnnt_gemm_desc {
  int64_t M, N, K;
  const float* A;
  int64_t a_div, a_so, a_si, a_sk;
  int32_t a_mc;
  const int64_t* a_rowidx;
  const float* B;
  int64_t b_sn, b_sk;
  float* C;
  int64_t c_div, c_so, c_si;
  const float* bias; /* (N) or NULL */
  const float* aux;  /* for RNNT_GEMM_MUL_DGELU */
  uint32_t flags;
  void* workspace;   /* optional: enables deterministic split-K (slabs + fixed-order reduce) for GEMMs whose   */
  size_t workspace_bytes; /* output has too few tiles to fill the chip; see rnnt_hip_gemm_workspace_bytes     */
} rnnt_gemm_desc;

size_t rnnt_hip_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int rnnt_hip_gemm_f32(const rnnt_gemm_desc* d, void* stream);

/* What rnnt_hip_gemm_f32 would launch for this descriptor (read-only: no launch, no device access; the operand pointers are looked
 * at for their alignment only).  Both entries take their decisions from the same function, and the descriptor is validated as the
 * launch validates it.  An empty output (M or N zero) gives tiles = 0 and tile_m = tile_n = 0: nothing is launched.
 *   mode: 6 split-bf16 with six products (default), 3 first-order split-bf16, 0 f32-input MFMA (RNNT_GEMM_EXACT_F32 / RNNT_GEMM_MODE).
 *   tile_m x tile_n: 128x128 or 128x256 (256 threads), 256x256 (512 threads, mode 6 only).
 *   a_kc / b_kc: the operand's rows are k-contiguous (a_mc == 0 / b_sk == 1).  vec: 16-byte operand loads, else scalar ones.
 *   splits > 1: split-K into `splits` slabs of `kchunk` k each in the workspace, summed in fixed order by a second kernel that also
 *   applies bias, the C row map, MUL_DGELU and ACCUM.  tiles: workgroups per slab.
 * Used by the tests that pin which kernel instance a shape runs. */
typedef struct rnnt_gemm_plan {
  int32_t mode;
  int32_t tile_m, tile_n;
  int32_t a_kc, b_kc;
  int32_t vec;
  int32_t tiles;
  int32_t splits, kchunk;
} rnnt_gemm_plan;
int rnnt_hip_gemm_plan(const rnnt_gemm_desc* d, rnnt_gemm_plan* out);

/* ------------------------------------------------------------------------------------------------
 * fp32 GEMM on the f16 matrix cores through "half-pair" (hp) operands — the form the BIG products of the hot path use
 * inside rnnt_hip_lstm_fwd / _bwd (hoisted input projection of nn.LSTM, networks/encoder.py:67-75,99, and its backward
 * products dX, dW_ih, dW_hh): 3 instead of 6 MFMA products per fp32 product, operands streamed to LDS by LDS-DMA.
 *
 * hp planes of an fp32 matrix x (rows x K), scaled per row: amax[r] = max_k |x[r][k]| (fp32 bit patterns, `rows` device words
 *   next to the planes), v = x * 2^(14 - floor(log2 amax[r])), hi = fp16_rn(v), lo = fp16_rn(v - hi)
 *   (v = hi + lo to 2^-23 |v|, with a floor of 2^-40 amax[r]); layout: row-major, K padded to 32, one 128-byte line per
 *   (row, 32-k block): 32 hi | 32 lo.  rnnt_hip_hp_bytes(rows, K).
 * rnnt_hip_hp_split: transpose == 0: x is (rows x K), row stride ld; amax[rows] is written (amax_given must be 0).
 *   transpose == 1: x is (src_rows x >= rows), row stride ld; plane row r, index k holds x[k + shift][r] (0 outside
 *   [0, src_rows)) — the transposed operands of the weight-gradient products, time-shifted for dW_hh; amax[r] = maximum of source
 *   column r, computed here unless amax_given.
 * rnnt_hip_gemm_hp: C (M x N, row stride ldc) [+]= A (M x K) . B (N x K)^T + bias, both operands hp planes (NT form), fp32 out.
 *   flags: RNNT_GEMM_ACCUM, RNNT_GEMM_HP_F16 (one product hi.hi: the planes are the same, only their hi halves are multiplied —
 *   each operand element is rounded to 11 significant bits of its row-scaled value, products accumulate in fp32).
 *   workspace (optional, rnnt_hip_gemm_hp_workspace_bytes): deterministic split-K slabs.
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_hp_bytes(int64_t rows, int64_t K);
int rnnt_hip_hp_split(const float* x, int64_t rows, int64_t K, int64_t ld, int32_t transpose, int64_t src_rows, int64_t shift,
                      void* planes, uint32_t* amax, int32_t amax_given, void* stream);
/* both orientations of x (M x C, row stride ld) in one pass: planes_rm = what transpose == 0 writes given the row maxima rowmax[M],
 * planes_t = what transpose == 1 (shift 0, contraction length M) writes given the column maxima colmax[C]; both tables are inputs
 * (rnnt_hip_lstm_bwd's recurrence leaves them for dG).  Bitwise the same planes as two rnnt_hip_hp_split calls. */
int rnnt_hip_hp_split_both(const float* x, int64_t M, int64_t C, int64_t ld, const uint32_t* rowmax, const uint32_t* colmax,
                           void* planes_rm, void* planes_t, void* stream);
size_t rnnt_hip_gemm_hp_workspace_bytes(int64_t M, int64_t N, int64_t K);
int rnnt_hip_gemm_hp(const void* A, const uint32_t* a_amax, const void* B, const uint32_t* b_amax, int64_t M, int64_t N, int64_t K,
                     float* C, int64_t ldc, const float* bias, uint32_t flags, void* workspace, size_t workspace_bytes,
                     void* stream);

/* The arguments the ragged (variable-length) batches of rnnt_hip_lstm_fwd / _bwd run these kernels with, exposed for tests; the
 * entries above are these with no index table and the plain C map.  Every index table is a DEVICE array of int32 whose values the
 * caller guarantees to lie inside the tensors they address (they are not read on the host).
 * rnnt_hip_hp_split_ex: idx (or NULL).  transpose == 0: `rows` listed source rows, each converted IN PLACE (source row idx[i] ->
 *   plane row idx[i] and amax[idx[i]]; other plane rows and amax words are not touched).  transpose == 1: K listed source rows,
 *   packed along the contraction: plane row r, index k holds x[idx[k] + shift][r] (0 where idx[k] + shift is outside [0, src_rows)).
 *   Without amax_given the column maxima are still taken over all src_rows.
 * rnnt_hip_hp_split_both_ex: rowidx (or NULL), M = its length: source row rowidx[i] -> row-major plane row rowidx[i] (in place, scale
 *   from rowmax[rowidx[i]]) and index i of the transposed planes (packed, contraction length M).
 * rnnt_hip_hp_colmax: amax[c] = max_r |x[r * ld + c]| over a (rows x C) view, as fp32 bit patterns (0 for an empty view).
 * rnnt_hip_gemm_hp_ex: C(m, n) [+]= sum_k A(a_rowidx ? a_rowidx[m] : m, k) B(n, k) + bias[n], written to
 *   C[(mo / c_div) * c_so + (mo % c_div) * c_si + n] with mo = c_rowidx ? c_rowidx[m] : m  (rnnt_hip_gemm_hp: c_div = 1, c_so = ldc,
 *   c_si = 0).  a_rowidx gathers plane rows AND amax words of A, whose planes hold a_plane_rows >= M rows (0 without a_rowidx).
 * rnnt_hip_gemm_hp_plan: what rnnt_hip_gemm_hp / _ex launch for (M, N, K) and a workspace of workspace_bytes (0: none) — no launch,
 *   no device access; the launch and rnnt_hip_gemm_hp_workspace_bytes take their decisions from the same function.  tiles_m x tiles_n
 *   tiles of 256 x 256, walked in bands of group_m tile rows; splits > 1: split-K over `splits` slabs of kt_per_split K-tiles (32 k
 *   each; the last slab takes what is left), summed in fixed order; workspace_bytes_wanted = rnnt_hip_gemm_hp_workspace_bytes. */
int rnnt_hip_hp_split_ex(const float* x, int64_t rows, int64_t K, int64_t ld, int32_t transpose, int64_t src_rows, int64_t shift,
                         void* planes, uint32_t* amax, int32_t amax_given, const int32_t* idx, void* stream);
int rnnt_hip_hp_split_both_ex(const float* x, int64_t M, int64_t C, int64_t ld, const uint32_t* rowmax, const uint32_t* colmax,
                              void* planes_rm, void* planes_t, const int32_t* rowidx, void* stream);
int rnnt_hip_hp_colmax(const float* x, int64_t rows, int64_t C, int64_t ld, uint32_t* amax, void* stream);
typedef struct rnnt_hp_gemm_desc {
  const void* A; const uint32_t* a_amax;   /* planes of a_plane_rows (a_rowidx) or M rows x K + their row maxima */
  const void* B; const uint32_t* b_amax;   /* (N x K) */
  int64_t M, N, K;
  float* C;
  int64_t c_div, c_so, c_si;
  const float* bias;                       /* (N) or NULL */
  uint32_t flags;                          /* RNNT_GEMM_ACCUM, RNNT_GEMM_HP_F16 */
  void* workspace; size_t workspace_bytes; /* optional split-K slabs */
  const int32_t* a_rowidx; int64_t a_plane_rows;
  const int32_t* c_rowidx;
} rnnt_hp_gemm_desc;
int rnnt_hip_gemm_hp_ex(const rnnt_hp_gemm_desc* d, void* stream);
typedef struct rnnt_hp_gemm_plan {
  int32_t tiles_m, tiles_n, group_m;
  int32_t splits, kt_per_split;
  size_t workspace_bytes_wanted;
} rnnt_hp_gemm_plan;
int rnnt_hip_gemm_hp_plan(int64_t M, int64_t N, int64_t K, size_t workspace_bytes, rnnt_hp_gemm_plan* out);

/* Up to 4 such products in ONE queue-driven launch: 256 resident workgroups draw (problem, tile, K-split) units until none is left
 * (one launch tail instead of one per product).  xcd_skip: bit x set = workgroups that find themselves on XCD x leave at once, the
 * other XCDs do all the work — for products that run on a second stream beside a persistent recurrence (rnnt_lstm_bwd_desc.phase).
 * workspace: rnnt_hip_gemm_hp_grouped_workspace_bytes(...) bytes, 256-byte aligned (queue counters + deterministic split-K slabs).
 * Self-check: a kernel behind the launch compares the units completed with the units queued; if they differ (xcd_skip named XCDs the
 * device does not expose, so every workgroup left) it sets word 9 of `workspace` to 1 — callers of this entry that pass a non-zero
 * xcd_skip read it back; rnnt_hip_lstm_bwd raises its sticky status word instead (and only passes a mask on a 256-CU device).
 * Used internally by rnnt_hip_lstm_bwd for dW_ih / dW_hh; exposed for tests. */
typedef struct rnnt_hp_problem {
  const void* A; const uint32_t* a_amax;   /* (M x K) planes + row maxima */
  const void* B; const uint32_t* b_amax;   /* (N x K) */
  int64_t M, N, K;
  float* C; int64_t ldc;
  uint32_t flags;                          /* RNNT_GEMM_ACCUM, RNNT_GEMM_HP_F16 (the same for every problem of one launch) */
} rnnt_hp_problem;
size_t rnnt_hip_gemm_hp_grouped_workspace_bytes(const rnnt_hp_problem* problems, int32_t n);
int rnnt_hip_gemm_hp_grouped(const rnnt_hp_problem* problems, int32_t n, uint32_t xcd_skip, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * LSTM layer (both directions in one launch), packed-sequence semantics.
 * Replaces torch.nn.LSTM over a PackedSequence + sort/pack/unpack/unsort:
 *   networks/encoder.py:67-75 (ctor), :93-102 (forward);  networks/decoder.py:71-79, :105-120.
 *
 * Layouts: x (T,B,I) time-major [or any (x_st, x_sb) element strides], y (T,B,D*H) time-major.
 *   Frames t >= lens[b] produce y == 0 and contribute no gradient (pad_packed_sequence semantics,
 *   encoder.py:101); the reverse direction starts at each sequence's own last valid frame.
 *   Weights in torch layout: w_ih[d] (G*H,I), w_hh[d] (G*H,H), b_ih[d], b_hh[d] (G*H); G = 4 (LSTM: i,f,g,o),
 *   3 (GRU: r,z,n), 1 (Elman RNN).  The gate buffer always has 4 slots per hidden unit.
 *   Requirements: H % 4 == 0, D in {1,2}, B <= 64 per call, T >= 1.
 *
 * Stash written by fwd and consumed by bwd (caller-owned, sizes below):
 *   gates: D*T*B*4H floats ... activated gates, overwritten with dG by bwd
 *   cst  : D*T*B*H  floats ... cell states
 * ---------------------------------------------------------------------------------------------- */
#define RNNT_CELL_LSTM 0      /* gates i,f,g,o   weights (4H, .)                                        */
#define RNNT_CELL_GRU 1       /* gates r,z,n     weights (3H, .)  (torch.nn.GRU layout and equations)    */
#define RNNT_CELL_RNN_TANH 2  /* Elman           weights (H, .)                                          */
#define RNNT_CELL_RNN_RELU 3

typedef struct rnnt_lstm_desc {
  int32_t T, B, I, H, D;
  int32_t cell;        /* RNNT_CELL_*: the reference's supported_rnns = lstm | gru | rnn (encoder.py:48-52) */
  const int32_t* lens; /* (B) device */
  const float* x;
  int64_t x_st, x_sb; /* element strides of x over t and b (feature stride 1) */
  const float* w_ih[2];
  const float* w_hh[2];
  const float* b_ih[2];
  const float* b_hh[2];
  float* y;       /* (T,B,D*H) */
  float* y_drop;  /* (T,B,D*H) y with inter-layer dropout applied, or NULL when dropout_p == 0 */
  float dropout_p;
  uint64_t dropout_seed;
  float* gates;   /* (T,B,D*4H) permuted gate layout, see DESIGN.md */
  float* cst;     /* (D,T,H/4,B,4)  LSTM only (may be NULL for the other cells) */
  float* aux;     /* GRU backward only: (T,B,D*4H) scratch for the hidden-side gate gradients; else NULL */
  void* workspace;
  size_t workspace_bytes;
  uint32_t* status; /* optional: caller-owned STICKY device status word (4 bytes, zeroed once by the caller).  A persistent
                     * kernel that abandons an inter-workgroup wait (4 s bound; e.g. its workgroups lost co-residency to a
                     * concurrent kernel) stores 1 here; the library never clears it, every later launch handed the same
                     * word bails out at its first wait, and rnnt_hip_adamw_step_ex(guard = this word) skips the update.
                     * Read it back with an asynchronous 4-byte copy whenever convenient (rnntransducer_amd does so once per
                     * optimizer step, no extra synchronisation).  NULL: word 0 of the workspace, reset per launch, read by
                     * rnnt_hip_lstm_check(). */
  float x_abs_bound; /* optional (backward): > 0 = the caller guarantees |x| <= x_abs_bound everywhere (x is the dropped output of
                     * a bounded cell below: 1 / (1 - p)).  The half-pair planes of x^T then take this as their scale instead of
                     * a pass over x for its column maxima (absolute error of an element <= 2^-39 x_abs_bound either way).  0: measure. */
  const int32_t* row_idx; /* optional, ragged batches (what pack_padded_sequence buys the reference, encoder.py:93-96,99-101, without a packed
                     * copy): device table of the n_rows VALID time-major rows t*B + b (those with t < lens[b]), ascending.  The big products
                     * (input projection, dX, dW_ih, dW_hh) then run over n_rows instead of T*B rows — operand tiles are gathered / results
                     * scattered through this table — and every sync group of the recurrence runs max(lens of its rows) steps instead of T
                     * (reverse direction: from that frame down).  Rows that are not listed are then NOT written in gates / cst / y_drop,
                     * and y keeps what the caller put there: hand in y zero-filled (frames t >= lens[b] must read 0).  dx of such rows is
                     * written as 0 by the backward call, as without the table.  Results on valid frames do not depend on it.  Honoured by the default kernels (v5 recurrences + half-pair products); other shapes
                     * ignore it and compute all T*B rows.  NULL: all rows.  Same table for the forward and the backward call. */
  int32_t n_rows;   /* entries of row_idx (= sum of lens); ignored when row_idx is NULL */
} rnnt_lstm_desc;

size_t rnnt_hip_lstm_workspace_bytes(int32_t T, int32_t B, int32_t I, int32_t H, int32_t D);
/* largest B one call accepts for (H, D, cell); 0 = shape unsupported.  Bigger batches: split along B (rows are independent). */
int32_t rnnt_hip_lstm_max_batch(int32_t H, int32_t D, int32_t cell);
/* XCDs (of 8) a recurrence of this shape leaves without a workgroup (0 when its groups fill the chip or are not placed per XCD):
 * what a caller looks at before it puts phase 2 of one layer beside phase 1 of the next (rnnt_lstm_bwd_desc.phase). */
int32_t rnnt_hip_lstm_free_xcds(int32_t T, int32_t B, int32_t H, int32_t D, int32_t cell);
/* 1 if a layer of this shape honours rnnt_lstm_desc.row_idx (v5 recurrences + half-pair products: every consumer of the stash gathers
 * the valid rows), 0 if it ignores the table and computes all T*B rows. */
int32_t rnnt_hip_lstm_takes_row_idx(int32_t T, int32_t B, int32_t I, int32_t H, int32_t D, int32_t cell);
int rnnt_hip_lstm_fwd(const rnnt_lstm_desc* d, void* stream);

/* Compute precision of a layer (opt-in; rnnt_hip_lstm_fwd / _bwd are RNNT_PRECISION_FP32).  The reference trains with
 * `--precision 16` (model.py:28-31 hands it to Lightning's AMP), under which nn.LSTM (networks/encoder.py:67-75,99) multiplies f16
 * operands with fp32 accumulation.  RNNT_PRECISION_F16 is that trade on this library's forms: the recurrences (h . W_hh^T, dG . W_hh)
 * and the big products each call issues inside itself (input projection; dX, dW_ih, dW_hh, also as the grouped phase-2 launch) run
 * ONE product hi.hi of the half-pair operands instead of three (RNNT_GEMM_HP_F16).  Every row keeps its own power-of-two scale, so
 * nothing overflows and no loss scaling is needed; an operand element carries about 2^-11 relative error.  Cell math, gate
 * pre-activations, the stash, parameters and gradients stay fp32.
 *   precision: RNNT_PRECISION_FP32 = bitwise rnnt_hip_lstm_fwd / _bwd;  RNNT_PRECISION_F16 = the one-product forms where the layer
 *   has them (rnnt_hip_lstm_takes_f16), bitwise fp32 elsewhere.  Any other value: RNNT_ERR_INVALID.
 *   The forward and the backward call of one layer must pass the same precision (the backward is the derivative of the
 *   arithmetic its forward ran; the library does not check it). */
#define RNNT_PRECISION_FP32 0
#define RNNT_PRECISION_F16 1
int rnnt_hip_lstm_fwd_ex(const rnnt_lstm_desc* d, uint32_t precision, void* stream);
/* 1 if a layer of this shape really runs the one-product forms under RNNT_PRECISION_F16 (v5 recurrences in both directions of time
 * and the half-pair products), 0 if it computes in fp32 whatever it is asked (lstm.hip's v3 / v4 forms: H > 640 unless opted in,
 * RNNT_LSTM_NO_V5, the ReLU cell; products below the half-pair limits).  Products that stay on
 * rnnt_hip_gemm_f32 inside an f16 layer (an input narrower than 32 / 128 features) are fp32 either way. */
int32_t rnnt_hip_lstm_takes_f16(int32_t T, int32_t B, int32_t I, int32_t H, int32_t D, int32_t cell);

typedef struct rnnt_lstm_bwd_desc {
  rnnt_lstm_desc f;   /* same description as the forward call (x, weights, y, stash, workspace) */
  const float* dy;    /* (T,B,D*H) gradient w.r.t. y (w.r.t. y_drop when dropout_p > 0) */
  float* dx;          /* (T,B,I) time-major, or NULL (first layer: dataloader.py gives no grad to mel) */
  float* dw_ih[2];    /* (4H,I)  written (not accumulated) */
  float* dw_hh[2];    /* (4H,H) */
  float* db[2];       /* (G*H)  gradient of b_ih (== gradient of b_hh for LSTM / RNN) */
  float* db_hh[2];    /* (G*H)  GRU: gradient of b_hh (differs from b_ih in the n gate), required.  LSTM / RNN: optional second
                       * destination that receives the same values as db (grad b_hh == grad b_ih), or NULL */
  int32_t accumulate; /* 0: dw_ih / dw_hh / db / db_hh are written; 1: added to (the outputs are views of a flat gradient
                       * buffer that autograd would otherwise `+=` into with one extra kernel per parameter) */
  int32_t phase;      /* RNNT_LSTM_BWD_ALL (0): everything on `stream`.  The two halves can also be issued separately so that a
                       * caller overlaps the weight gradients of layer l with the recurrence of layer l-1 (autograd needs only dx
                       * to go on): RNNT_LSTM_BWD_RECUR (1) = reverse-time recurrence (gates -> dG in place) + dx;
                       * RNNT_LSTM_BWD_WEIGHTS (2) = dw_ih / dw_hh / db / db_hh from the dG that phase 1 left in `gates`, on any
                       * stream ordered after phase 1, with the SAME descriptor and workspace (which phase 1 of another layer must
                       * not reuse before phase 2 is done: alternate two workspaces). */
  int32_t beside_recurrence; /* phase 2 only, a hint: 1 = a recurrence of the same (B,H,D) runs concurrently on another stream; the
                       * big products then leave the XCDs that recurrence occupies alone (its workgroups exchange through their
                       * XCD's L2) and run as one queue-driven launch on the others.  Results do not depend on it (honoured only on a
                       * device that exposes all 8 XCDs; a launch that left work undone raises `f.status`). */
} rnnt_lstm_bwd_desc;
#define RNNT_LSTM_BWD_ALL 0
#define RNNT_LSTM_BWD_RECUR 1
#define RNNT_LSTM_BWD_WEIGHTS 2

int rnnt_hip_lstm_bwd(const rnnt_lstm_bwd_desc* d, void* stream);
/* rnnt_hip_lstm_bwd with a compute precision: the one of the layer's forward call (see rnnt_hip_lstm_fwd_ex) */
int rnnt_hip_lstm_bwd_ex(const rnnt_lstm_bwd_desc* d, uint32_t precision, void* stream);
/* reads back the persistent kernels' status word from a workspace (synchronises `stream`);
 * 0 = ok, RNNT_ERR_TIMEOUT if an inter-CU wait gave up.  For tests and the bench, not for hot loops. */
int rnnt_hip_lstm_check(const void* workspace, void* stream);
/* Diagnostics (a library built with -DRNNT_LSTM_DBG_STAMPS=1 only: the stamps are compiled out of the default build, where this
 * entry returns zeros): with RNNT_LSTM_DBG set in the environment the recurrences accumulate shader-clock cycles per step
 * phase (0 prefetch issue, 1 flag wait, 2 gather+MFMA, 3 reduce+cell math, 4 drain+barrier+flag, 5 stash stores) for
 * lane 0 of every workgroup; this copies the last launch's table (nwg x 8 u64) to host memory (synchronises). */
int rnnt_hip_lstm_debug_read(const void* workspace, int32_t T, int32_t B, int32_t I, int32_t H, int32_t D,
                             uint64_t* out, int32_t nwg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused joint + log-softmax + RNN-T lattice (never materialises (B,T,U+1,V) nor (B,T,U+1,2*O)).
 * Replaces JointNet.joint (networks/transducer.py:54-69) followed by RNNTLoss (model.py:39,57):
 *   z[b,t,u,:] = fc(gelu_tanh(cat(enc[b,t], dec[b,u]))) = A[b,t,:] + C[b,u,:] + bias     
 * Inputs here are the two small pre-GEMM results A = gelu(enc).W_e^T, C = gelu(dec).W_d^T (computed with
 * rnnt_hip_gemm_f32 + RNNT_GEMM_GELU_A) and fc.bias (V).  A(b,t,v) = A[b*a_sb + t*a_st + v],
 * C(b,u,v) = C[b*c_sb + u*c_su + v]  (so batch-major and time-major buffers both work, no copy).
 * Outputs: nll (B) = -log P(y|x) per utterance; dA, dC (same strides as A, C) = d(sum_b gscale*nll_b)/dA,dC.
 *   labels (B,U) int32 (U = U1-1), t_lens (B) int32 in [1,T], u_lens (B) int32 in [0,U].  U1 <= 512 for every V, forward and
 *   backward alike.  Lengths are not checked on the device.  One exception to t_lens >= 1 is defined: t_lens[b] = 0 (an utterance
 *   without frames has no alignment) gives nll[b] = +inf and exact zeros in row b of dA and dC, and leaves every other row bitwise
 *   as a batch without row b computes it.
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_joint_loss_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V);
int rnnt_hip_joint_loss_fwd_bwd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                const float* bias, const int32_t* labels, const int32_t* t_lens,
                                const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                float gscale, float* nll, float* dA, float* dC, void* workspace,
                                size_t workspace_bytes, void* stream);

/* The same in two calls, for autograd: the forward is rnnt_hip_joint_loss_fwd_bwd with dA = dC = NULL (it leaves
 * log-softmax terms, alpha, beta and log Z in `workspace`); this runs the gradient kernels from that workspace on the SAME
 * A / C / bias / labels / lengths, with the upstream gradient per utterance: d(sum_b gscale * gvec[b * gvec_stride] * nll_b)/dA,dC
 * (gvec device, gvec_stride 1 = one value per utterance, 0 = ONE scalar for all; NULL = ones).  reduction="mean" of model.py:39
 * arrives here as gscale = 1/B with gvec = the 0-d gradient of the mean (stride 0). */
int rnnt_hip_joint_loss_bwd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                            const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                            int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale, const float* gvec,
                            int32_t gvec_stride, float* dA, float* dC, void* workspace, size_t workspace_bytes, void* stream);
/* out[0] = scale * sum_i x[i] in a fixed order (reduction="mean" / "sum" of the per-utterance losses, model.py:39). */
int rnnt_hip_scaled_sum_f32(const float* x, int32_t n, float scale, float* out, void* stream);

/* Materialising joint for RNNTransducer.forward() (model.py:47-50): logits (B,T,U1,V) = A + C + bias. */
int rnnt_hip_joint_logits_fwd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                              const float* bias, int32_t B, int32_t T, int32_t U1, int32_t V, float* logits,
                              void* stream);

/* warp-transducer-shaped entry (model.py:39,57): loss + gradient from dense logits (B,T,U1,V).
 * grad may be NULL (forward only).  grad = d(sum_b gscale*nll_b)/d logits. */
int rnnt_hip_loss_from_logits_fwd_bwd(const float* logits, const int32_t* labels, const int32_t* t_lens,
                                      const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V,
                                      int32_t blank, float gscale, float* nll, float* grad, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* Embedding forward (networks/decoder.py:69,102): out[m,:] = W[idx[m],:]  (row padding_idx of W is zero by
 * construction, nn.Embedding(padding_idx=blank)).  Ids outside [0, V) give zero rows.  M == 0 does nothing (idx and out may be NULL). */
int rnnt_hip_embedding_fwd(const float* W, const int64_t* idx, int64_t M, int32_t H, int32_t V, float* out, void* stream);

/* Same, for logits/grad stored as fp16 or bf16 (torchaudio's RNNTLoss takes half logits: model.py:28-31); the
 * log-softmax, alpha/beta and gradient arithmetic stay fp32/fp64, only loads/stores convert. */
#define RNNT_DTYPE_F32 0
#define RNNT_DTYPE_F16 1
#define RNNT_DTYPE_BF16 2
int rnnt_hip_loss_from_logits_fwd_bwd_ex(const void* logits, int32_t dtype, const int32_t* labels, const int32_t* t_lens,
                                         const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                         float gscale, float* nll, void* grad, void* workspace, size_t workspace_bytes,
                                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * FastEmit regularisation (Yu et al., ICASSP 2021) of the three gradient entry points above: the same arguments plus
 * `fastemit_lambda` after `gscale`.  Per lattice cell (t,u) with occupancy w = cb + ce, blank-transition posterior cb and
 * label-transition posterior ce (0 at u = u_lens[b]), the gradient with respect to the LABEL log-probability is scaled by
 * (1 + lambda), the blank's is left alone, and the result goes through the log-softmax exactly:
 *   dz[t,u,v] = softmax_v (w + lambda ce) - [v = blank] cb - [v = y_u] (1 + lambda) ce
 * i.e. the exact gradient of  nll_b + lambda * sum_{t,u} stopgrad(ce[t,u]) * (-emit(t,u)).  sum_v dz = 0 in every cell, as for the
 * plain loss.  (Forms that scale only the label entry of the logit gradient lose that; this library does not reproduce them.)
 *   - ONLY THE GRADIENT CHANGES: nll is the unregularised -log P(y|x), bit for bit what lambda = 0 returns, so loss curves stay
 *     comparable across lambda.  The forward call (dA = dC = NULL / grad = NULL) ignores lambda apart from validating it.
 *   - lambda multiplies nothing else: gscale, gvec, strides, the t_lens[b] = 0 rule and the workspace (size and layout) are as
 *     above.  A row with u_lens[b] = 0 has no label transition: its gradient is bitwise that of lambda = 0.
 *   - lambda = 0 runs the same kernels as the entries above (which forward here with 0): bitwise the same results.
 *   - lambda < 0, NaN or infinite: RNNT_ERR_INVALID, before any device work.
 * ---------------------------------------------------------------------------------------------- */
int rnnt_hip_joint_loss_fwd_bwd_fastemit(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                         const float* bias, const int32_t* labels, const int32_t* t_lens,
                                         const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                         float gscale, float fastemit_lambda, float* nll, float* dA, float* dC, void* workspace,
                                         size_t workspace_bytes, void* stream);
int rnnt_hip_joint_loss_bwd_fastemit(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                     const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                     int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale,
                                     float fastemit_lambda, const float* gvec, int32_t gvec_stride, float* dA, float* dC,
                                     void* workspace, size_t workspace_bytes, void* stream);
int rnnt_hip_loss_from_logits_fwd_bwd_fastemit(const void* logits, int32_t dtype, const int32_t* labels, const int32_t* t_lens,
                                               const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                               float gscale, float fastemit_lambda, float* nll, void* grad, void* workspace,
                                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Alignment-restricted loss (Ar-RNN-T, Mahadeokar et al. 2021): per-label emission windows.  The _fastemit entries above plus two
 * device tables `emit_lo`, `emit_hi` of B rows of U = U1 - 1 int32 entries, row stride `win_stride` elements (positive, >= U: a
 * (B,U) view of a wider table passes).  Label u of row b (u < u_lens[b]) may be emitted at frame t only if
 *   max(emit_lo[b][u], 0) <= t <= min(emit_hi[b][u], t_lens[b] - 1);
 * entries at u >= u_lens[b] are never read; blank transitions are unrestricted.  The lattice is the usual one with emit(t,u) = -inf
 * outside the window: nll is -log of the sum over the paths that emit every label inside its window, the gradient is that value's
 * gradient (the same per-cell formula; a cell no allowed path visits contributes exactly 0).  Windows need not be monotone.
 *   - Work: with L[u] = max(0, lo[0..u-1]) and R[u] = min(hi[u..Ub-1], Tb-1), only cells with L[u] <= t <= R[u] can lie on an allowed
 *     path.  The V-wide terms of every other cell are not computed (log-sum-exp and gradient kernels); the sweep is unchanged.
 *   - An infeasible row (an empty window, windows that leave no monotone path, t_lens[b] = 0) returns nll = +inf and exact-zero
 *     dA / dC (grad) rows, without NaN: CTCLoss's convention for a transcript that does not fit its frames.
 *   - Full windows (lo <= 0, hi >= t_lens[b] - 1 for every label) give nll, dA, dC bit for bit those of the _fastemit entries
 *     with the same lambda; a row gives the same bits alone as in a batch; fastemit_lambda acts on the live cells as above.
 *   - Workspace: rnnt_hip_joint_loss_window_workspace_bytes (the plain layout followed by the band tables).  The backward-only entry
 *     takes the workspace of a forward call of rnnt_hip_joint_loss_fwd_bwd_window (dA = dC = NULL) on the same operands and windows.
 *   - Null window tables or a bad stride: RNNT_ERR_INVALID, before any device work.  The entries without windows are untouched.
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_joint_loss_window_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V);
int rnnt_hip_joint_loss_fwd_bwd_window(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                       const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                       int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale,
                                       float fastemit_lambda, const int32_t* emit_lo, const int32_t* emit_hi, int64_t win_stride,
                                       float* nll, float* dA, float* dC, void* workspace, size_t workspace_bytes, void* stream);
int rnnt_hip_joint_loss_bwd_window(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                   const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                   int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale, float fastemit_lambda,
                                   const float* gvec, int32_t gvec_stride, float* dA, float* dC, void* workspace,
                                   size_t workspace_bytes, void* stream);
int rnnt_hip_loss_from_logits_fwd_bwd_window(const void* logits, int32_t dtype, const int32_t* labels, const int32_t* t_lens,
                                             const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                             float gscale, float fastemit_lambda, const int32_t* emit_lo, const int32_t* emit_hi,
                                             int64_t win_stride, float* nll, void* grad, void* workspace, size_t workspace_bytes,
                                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lattice knowledge distillation (Panchapagesan et al., ICASSP 2021, "Efficient knowledge distillation for RNN-Transducer models"):
 * a teacher's per-cell distributions pull a student's, with three floats per lattice cell from each side and no (B,T,U+1,V) tensor.
 * Per cell (t,u) both softmaxes are collapsed to three classes -- blank, the cell's label y_u (only where u < u_lens[b]), everything
 * else -- and
 *   kd[b] = sum_{t < t_lens[b], u <= u_lens[b]} sum_k P_T(k) (log P_T(k) - log P_S(k))        (>= 0; 0 iff the collapsed cells agree)
 * The planes: blk, emit, rest (B,U1,T) fp32, plane(b,u,t) = plane[(b*U1 + u)*T + t]: log p(blank), log p(y_u) (0 at u = U1-1, the
 * padded label's log-probability at u_lens[b] <= u < U1-1: not read by the term) and rest = log sum_{v not in {blank, y_u}} p(v), over
 * every non-blank entry where u >= u_lens[b].  rest is a log-sum-exp over the entries themselves, exact to fp32 rounding down to
 * -80 and FLOORED there: finite whatever the logits are (an entry more than ~87 below the cell's largest logit underflows in fp32).
 *
 * rnnt_hip_joint_cell_logprobs (the teacher's side): the three planes of the operands of rnnt_hip_joint_loss_fwd_bwd into the
 * caller's buffers: one launch, no sweep, no workspace.  t_lens is not read (every frame of A is computed), u_lens ends the label
 * class.  blk and emit are the bits the loss computes on the same operands.
 *
 * rnnt_hip_joint_loss_fwd_bwd_kd / _bwd_kd: the _fastemit entries plus the teacher's planes t_blk / t_emit / t_rest (from the call
 * above on the teacher's operands with the SAME labels and lengths; entries outside a row's lattice are not used), the upstream
 * gradient of the KD term (kd_gscale, and in the backward-only entry kd_gvec / kd_gvec_stride, read as gscale / gvec / gvec_stride
 * are for the NLL) and the output kd (B).  Gradients: dA, dC = d(sum_b gscale gvec_b nll_b + kd_gscale kd_gvec_b kd_b)/dA,dC, the
 * teacher's planes being constants.  Either upstream may be 0: gscale = 0 (or gvec_b = 0) is pure distillation.
 *   - nll, and blk / emit / alpha / beta in the workspace, are bit for bit those of the _fastemit entries on the same operands.
 *   - kd: fp32 class terms, fp64 sums in a fixed order, no atomics: a row gives the same bits alone as in any batch.  A class with
 *     P_T(k) = 0 (a plane entry of -inf) contributes exactly 0; a row with t_lens[b] = 0 gives kd = 0 (and nll = +inf, zero gradients).
 *   - The gradient of the term per cell is p[v] (1 - rho) - [v = blank] (a - rho p_b) - [v = y_u] (c - rho p_y) with (a, c, r) the
 *     teacher's and (p_b, p_y, p_r) the student's collapsed probabilities and rho = r / p_r: the lattice gradient kernels' arithmetic
 *     on changed per-cell scalars, so it costs no further pass over V.  fastemit_lambda acts on the transducer term as above.
 *   - Workspace: rnnt_hip_joint_loss_kd_workspace_bytes (the plain layout followed by the student's rest plane).  The backward-only
 *     entry takes the workspace of a forward call of rnnt_hip_joint_loss_fwd_bwd_kd (dA = dC = NULL) on the same operands and planes.
 *   - RNNT_ERR_INVALID before any device work: null teacher planes, a null kd (forward), V < 3 (the third class would be empty), a
 *     kd_gvec_stride other than 0 / 1, a kd_gscale that is not finite.  There is no windowed and no dense-logits form.
 *   - Labels are non-blank by the loss's contract; a blank label is not detected.  The entries without KD are untouched.
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_joint_loss_kd_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V);
int rnnt_hip_joint_cell_logprobs(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                 const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens, int32_t B,
                                 int32_t T, int32_t U1, int32_t V, int32_t blank, float* blk, float* emit, float* rest, void* stream);
int rnnt_hip_joint_loss_fwd_bwd_kd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                   const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens, int32_t B,
                                   int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale, float fastemit_lambda,
                                   const float* t_blk, const float* t_emit, const float* t_rest, float kd_gscale, float* nll,
                                   float* kd, float* dA, float* dC, void* workspace, size_t workspace_bytes, void* stream);
int rnnt_hip_joint_loss_bwd_kd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                               const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens, int32_t B,
                               int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale, float fastemit_lambda, const float* gvec,
                               int32_t gvec_stride, const float* t_blk, const float* t_emit, const float* t_rest, float kd_gscale,
                               const float* kd_gvec, int32_t kd_gvec_stride, float* dA, float* dC, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Forced alignment: the best (Viterbi) RNN-T path of a KNOWN transcript, per utterance, on the device.  No (B,T,U+1,V) tensor:
 * the same two numbers per lattice cell as the loss, blk(t,u) = log p(blank | t,u) and emit(t,u) = log p(y_u | t,u), then the
 * lattice sweep of the loss in the (max, +) semiring:
 *   v(t,u) = max( v(t-1,u) + blk(t-1,u), v(t,u-1) + emit(t,u-1) ),  v(0,0) = 0,
 *   score  = v(Tb-1,Ub) + blk(Tb-1,Ub)            (Tb = t_lens[b], Ub = u_lens[b]),
 * accumulated in fp64 from the fp32 cell terms (an exact sum: no transcendental after the log-softmax).
 * Tie rule: on exactly equal candidates the blank predecessor (t-1,u) wins; the label predecessor (t,u-1) is taken only when it
 * is strictly greater.  The path is therefore a pure function of blk / emit.
 * Outputs: frames (B,U) int32 (U = U1-1): frames[b][u] = the frame at which label u is emitted on the best path, for u < u_lens[b]
 *   (non-decreasing in u, in [0, t_lens[b])); -1 for u >= u_lens[b].  score (B) fp64 = log-probability of the best path
 *   (<= -nll of the loss, which sums over all paths).
 * Limits and edge cases are the loss's: U1 <= 512, any V; t_lens[b] in [1,T]; t_lens[b] = 0 gives score[b] = -inf and frames -1
 *   in row b and leaves every other row as it is without row b; u_lens[b] = 0 is the all-blank path (finite score, no frame);
 *   T = 1 puts every label on frame 0.  Row b gives the same bits alone as inside any batch.  frames may be NULL when U1 = 1.
 * The fused form takes the operands and strides of rnnt_hip_joint_loss_fwd_bwd (and picks its log-softmax kernel by the same
 * vocabulary rule); the dense form takes logits (B,T,U1,V) stored as RNNT_DTYPE_F32 / _F16 / _BF16, as
 * rnnt_hip_loss_from_logits_fwd_bwd_ex does.  Both use a workspace of rnnt_hip_joint_align_workspace_bytes (0 for invalid
 * dims): 8 bytes + 1 bit per lattice cell.  Arguments are validated before any device work; nothing synchronises.
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_joint_align_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V);
int rnnt_hip_joint_align(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                         const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                         int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, int32_t* frames, double* score,
                         void* workspace, size_t workspace_bytes, void* stream);
int rnnt_hip_align_from_logits_ex(const void* logits, int32_t dtype, const int32_t* labels, const int32_t* t_lens,
                                  const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                  int32_t* frames, double* score, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTC loss on per-frame logits (the auxiliary loss on the encoder's output) and the greedy CTC decode.  csrc/ctc.hip, DESIGN.md §16.
 * logits(b,t,v) = logits[b*z_sb + t*z_st + v], finite fp32 (batch-major and time-major buffers both work, the inner stride is 1;
 * z_st >= V).  labels (B,U) int32, t_lens (B) int32 in [1,T], u_lens (B) int32 in [0,U]; U <= 511, any V, U = 0 allowed (labels may
 * then be NULL).  The blank is an ordinary vocabulary entry, blank in [0,V); a blank inside labels[b,:u_lens[b]] is not checked.
 * Logits of frames t >= t_lens[b] and labels at k >= u_lens[b] are never read.
 *   extended sequence l' of 2 u_lens[b] + 1 states (blank, y_0, blank, y_1, ..., blank), lp = log-softmax of a frame,
 *   alpha_t(s) = lp[t,l'_s] + logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), [l'_s != blank and l'_s != l'_{s-2}] alpha_{t-1}(s-2)),
 *   nll[b] = -logaddexp(alpha_{T_b-1}(S-1), alpha_{T_b-1}(S-2)); fp32 per-frame terms, fp64 lattice sums, fixed summation order.
 * A row with no path (t_lens[b] < u_lens[b] + number of k with y_k = y_{k+1}; also t_lens[b] = 0) gives nll[b] = +inf and an exactly
 * zero row of dlogits; every other row is bitwise what it is alone.
 * rnnt_hip_ctc_loss_fwd leaves the per-frame terms, alpha, beta and log Z in `workspace` (rnnt_hip_ctc_loss_workspace_bytes; 0 for
 * B, T or V < 1 or U < 0); rnnt_hip_ctc_loss_bwd, on the SAME operands and that workspace, writes
 *   dlogits(b,t,v) = gscale * gvec[b*gvec_stride] * (softmax(logits[b,t,:])[v] - sum_{s: l'_s = v} occ_t(s))   for t < t_lens[b],
 * exact zeros for t_lens[b] <= t < T, with the logits' strides (gvec device, gvec_stride 1 = one value per utterance, 0 = ONE scalar
 * for all, as in rnnt_hip_joint_loss_bwd; NULL = ones).  Repeated labels are summed in label order: no float atomics, the same bits
 * on every call.  Arguments are validated before any device work; nothing allocates or synchronises.
 * rnnt_hip_ctc_greedy: per frame the argmax over v (ties go to the LOWEST index); frame t's token is kept when it is not the blank
 * and differs from frame t-1's argmax.  tokens (B,T) int32: the first counts[b] entries of row b are the kept tokens (the rest of the
 * row is not written); counts (B) int32; frames (B,T) int32 or NULL: the first frame of each kept token's run.  One launch.
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_ctc_loss_workspace_bytes(int32_t B, int32_t T, int32_t U, int32_t V);
int rnnt_hip_ctc_loss_fwd(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* labels, const int32_t* t_lens,
                          const int32_t* u_lens, int32_t B, int32_t T, int32_t U, int32_t V, int32_t blank, float* nll,
                          void* workspace, size_t workspace_bytes, void* stream);
int rnnt_hip_ctc_loss_bwd(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* labels, const int32_t* t_lens,
                          const int32_t* u_lens, int32_t B, int32_t T, int32_t U, int32_t V, int32_t blank, float gscale,
                          const float* gvec, int32_t gvec_stride, float* dlogits, void* workspace, size_t workspace_bytes,
                          void* stream);
int rnnt_hip_ctc_greedy(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T, int32_t V,
                        int32_t blank, int32_t* tokens, int32_t* counts, int32_t* frames, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTC forced alignment: the best (Viterbi) CTC path of a KNOWN transcript, per utterance, on the device.  csrc/ctc.hip, DESIGN.md §28.
 * Operands and limits are those of rnnt_hip_ctc_loss_fwd: strides z_sb, z_st >= V (batch- and time-major buffers both work),
 * U <= 511, any V, U = 0 allowed (labels, first, last and token_logp may then be NULL); frames t >= t_lens[b] and labels past
 * u_lens[b] are never read; t_lens / u_lens are clamped to [0,T] / [0,U].
 *   lp[t,v] is the fp32 log-softmax the CTC loss computes (the same emission rows em[b][r][t] of the same kernel: the all-path loss
 *   and the best path are functions of the same fp32 numbers).  The (max, +) form of the alpha recurrence above, over l' of
 *   S = 2 U_b + 1 states:
 *     v_0(0) = lp[0,blank], v_0(1) = lp[0,y_0], everything else -inf
 *     v_t(s) = lp[t,l'_s] + max( v_{t-1}(s), v_{t-1}(s-1), [l'_s != blank and l'_s != l'_{s-2}] v_{t-1}(s-2) )
 *     score  = max( v_{T_b-1}(S-1), v_{T_b-1}(S-2) )
 *   accumulated in fp64 from the fp32 terms: no transcendental after the log-softmax, as in rnnt_hip_joint_align.
 * Tie rule: candidates are taken in the order written: stay, s-1, s-2.  A later candidate wins only when strictly greater.  At the
 *   end the last label state S-2 wins only when strictly greater than the trailing blank S-1.  The path is then a pure function of lp.
 * Outputs: first, last (B,U) int32: the first and last frame the best path spends in label u's state;
 *     first[u] <= last[u] < first[u+1], all inside [0, t_lens[b]); -1 for u >= u_lens[b].
 *   path (B,T) int32 or NULL: the token of the path's state at frame t (the blank id in blank states), -1 for t >= t_lens[b].
 *   token_logp (B,U) fp64 or NULL: sum_{t=first..last} lp[t,y_u], summed in ascending t; 0 for u >= u_lens[b].
 *   score (B) fp64 (<= -nll of rnnt_hip_ctc_loss_fwd, which sums over all paths).
 * Edge rows: a row with no path (t_lens[b] < u_lens[b] + number of k with y_k = y_{k+1}; also t_lens[b] = 0) gives score = -inf,
 *   first = last = -1, path = -1, token_logp = 0, and every other row is untouched by it.  u_lens[b] = 0 is the all-blank path:
 *   finite score, no frames.  Row b gives the same bits alone as in any batch; two calls give the same bits.
 * Workspace, rnnt_hip_ctc_align_workspace_bytes(B, T, U, V) bytes (0 for B, T or V < 1 or U < 0), with r(x) = x rounded up to 256:
 *     r(4 B (U+1) T)  emission rows em[b][r][t] (r = 0: blank, r = k+1: y_k), at offset 0
 *   + r(4 B T)        the frames' log-sum-exp
 *   + r(4 B (U+1))    the terms kernel's label chains (not used by the alignment)
 *   + r(12 B (U+1) ceil(T/32))   back-pointers: three bits per (frame, label position), in three planes of 32-frame words
 *   + r(4 B)          the end state of each row.
 * Three launches (terms, sweep, back-trace); arguments are validated before any device work; nothing allocates or synchronises.
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t U, int32_t V);
int rnnt_hip_ctc_align(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* labels, const int32_t* t_lens,
                       const int32_t* u_lens, int32_t B, int32_t T, int32_t U, int32_t V, int32_t blank, int32_t* first,
                       int32_t* last, int32_t* path, double* token_logp, double* score, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTC prefix beam search on per-frame logits (the encoder's CTC head), optionally with token fusion.  csrc/ctc_beam.hip, DESIGN.md §19.
 * Logits, strides and t_lens as for the CTC entries above (t_lens[b] is clamped to [0,T]; frames t >= t_lens[b] are never read).
 * Per utterance, lp[t,v] is the fp32 log-softmax of the logits row, as the CTC loss computes it.  A hypothesis is a prefix l (a token
 * list without blanks; equal adjacent tokens are legal) with two fp64 log-probabilities: pb, the mass of its paths ending in blank,
 * and pnb, the mass of its paths ending in l[-1]; p(l) = logaddexp(pb, pnb).  With fusion it also carries an automaton state and an
 * fp64 total = the sum of arc[s, k] over its tokens in append order from state 0 (it depends on the prefix only).
 *   start     the beam is [()] with pb = 0, pnb = -inf, state 0, total 0
 *   frame t   the beam holds at most W prefixes in rank order r = 0..; candidate tokens C_t = {k != blank : lp[t,k] >= token_min_logp}
 *             (token_min_logp = -inf: every non-blank token).  For the prefix l at rank r with last token e (none for ()):
 *               survivor l, id r (V+1):            pb' = p(l) + lp[t,blank]; stay term pnb(l) + lp[t,e] (-inf for ()), whether or not
 *                                                  e is in C_t
 *               extension l + k, k in C_t, id r (V+1) + 1 + k:   extension term pb(l) + lp[t,k] if k == e, else p(l) + lp[t,k]
 *             An extension l + k that equals a prefix l2 of the current beam is the same candidate as l2's survivor and takes the
 *             survivor's id; pnb' = logaddexp(stay term, extension term), a missing term being -inf (logaddexp(x, -inf) = x exactly).
 *             A prefix that was pruned earlier and is reached again is a new candidate with only its extension term.
 *             Candidate score = logaddexp(pb', pnb'); rank key = score + total', descending, then id ascending; candidates with
 *             score -inf are dropped; the first W form the next beam.
 *   output    up to W hypotheses per utterance, best first by score (with fusion: by score + total + final[state]), ties in the last
 *             frame's order; t_lens[b] = 0 gives [()] with score 0.  No length normalisation.
 * Outputs: counts (B) int32 = hypotheses of utterance b; for o < counts[b]: lens[b,o], tokens[b,o,:lens[b,o]] (tokens is (B, W, T)
 * int32; a prefix has at most t_lens[b] tokens), scores[b,o] (fp64: the CTC log-probability mass the search kept for that labelling),
 * with fusion fusion->fused_scores[b,o] = score + total + final[state] ((B, W) fp64; must not be NULL then), and frames (B, W, T)
 * int32 or NULL: per token the frame whose extension step first created its prefix-tree node (a prefix keeps ONE node however often
 * it is pruned and reached again; frames increase along a hypothesis).  Nothing is written for o >= counts[b] or past lens[b,o].
 * fusion: NULL, or the tables of rnnt_beam_fusion above over the SAME V (next values outside [0,S) are clamped); the unfused
 * instance of the kernel does not touch them, and an all-zero automaton gives the unfused lists and score bits.
 * Limits, checked on the host before any launch (RNNT_ERR_INVALID): 1 <= W <= 128, V >= 2, 0 <= blank < V, W (V+1) <= 2^24,
 * token_min_logp neither NaN nor +inf, n_states >= 1 and n_states * V <= 2^27, non-NULL pointers, workspace (8-byte aligned) of
 * rnnt_hip_ctc_beam_workspace_bytes(B, T, V, W) bytes (0 for sizes outside the limits): the candidate keys, the prefix tree of at
 * most 1 + W T nodes per utterance and the frames' log-sum-exps.  One launch, one workgroup per utterance, every sum in one fixed
 * order: the same bits on every call, and a row alone gives the bits it gives in any batch.
 * ---------------------------------------------------------------------------------------------- */
struct rnnt_beam_fusion;
size_t rnnt_hip_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t W);
int rnnt_hip_ctc_beam_search(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T, int32_t V,
                             int32_t blank, int32_t W, float token_min_logp, const struct rnnt_beam_fusion* fusion, int32_t* tokens,
                             int32_t* lens, double* scores, int32_t* frames, int32_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream);

/* One fused AdamW step over FLAT fp32 buffers (all parameters / gradients / moments of the module laid out back to back):
 * replaces torch.optim.AdamW's multi-tensor kernels at model.py:111-115.  Same update as torch (decoupled weight decay,
 * bias corrections from `step` >= 1). */
int rnnt_hip_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, void* stream);
/* Same with g scaled by `grad_scale` on load (1/world of the data-parallel average: train.py:45 DDP semantics, folded into
 * the update instead of a separate pass over the gradients) and an optional device guard word: when *guard != 0 (the sticky
 * LSTM status word, see rnnt_lstm_desc.status) the kernel leaves p, m, v untouched. */
int rnnt_hip_adamw_step_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int64_t step, float grad_scale, const uint32_t* guard, void* stream);

/* column sums: out[n] = sum_m X[m*ld + n]  (bias gradients: fc.bias, out_proj.bias, LSTM biases).
 * Two-stage fixed-order reduction; workspace = rnnt_hip_colsum_workspace_bytes(M, N) bytes.  M == 0 gives zeros (X may be NULL). */
size_t rnnt_hip_colsum_workspace_bytes(int64_t M, int64_t N);
int rnnt_hip_colsum_f32(const float* X, int64_t M, int64_t N, int64_t ld, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);
/* out[n] += column sum (flat-gradient accumulation) */
int rnnt_hip_colsum_f32_acc(const float* X, int64_t M, int64_t N, int64_t ld, float* out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Embedding backward (networks/decoder.py:69,102): dW[idx[m]] += dE[m] for idx[m] != padding_idx. dW (V,H)
 * must be zeroed by the caller.  Ids outside [0, V) are ignored; the hits of a row are added in token order (a fixed-order fp32
 * sum).  M == 0: dE and idx may be NULL. */
int rnnt_hip_embedding_bwd(const float* dE, const int64_t* idx, int64_t M, int32_t H, int32_t V, int64_t padding_idx,
                           float* dW, void* stream);
/* dW[v] += sum (row padding_idx untouched): accumulation into an existing gradient */
int rnnt_hip_embedding_bwd_acc(const float* dE, const int64_t* idx, int64_t M, int32_t H, int32_t V, int64_t padding_idx,
                               float* dW, void* stream);

/* Greedy decoding on device (replaces JointNet.recognize_greedy, networks/transducer.py:95-145, including its
 * single-step prediction-net call networks/decoder.py:121-123 and the 1-D joint networks/transducer.py:64-69).
 * One workgroup per utterance.  A = gelu(encoder_outputs) . fc.weight[:, :O_enc]^T + fc.bias for every frame
 * (time-major (T,B,V); computed by the caller with rnnt_hip_gemm_f32(RNNT_GEMM_GELU_A)).  Utterance b visits frames
 * t in [0, t_lens[b]) — the reference decodes one utterance per call, so its loop bound encoder_outputs.size(1) is that
 * utterance's own length; t_lens == NULL visits all T padded frames (what a batched reference call does).  Per frame: up to max_iters symbols; a symbol equal to the
 * last appended one still advances the prediction net but is not appended (transducer.py:132-137).
 * tokens (B,max_out) int64 (entries past ntok[b] are left untouched), ntok (B) int32; max_out >= T*max_iters never
 * truncates. */
#define RNNT_DECODE_MAX_LAYERS 8
typedef struct rnnt_decode_desc {
  int32_t T, B, V;       /* frames, utterances, vocabulary */
  int32_t Hp, O, L;      /* prediction-net hidden size (= embedding width), joint input width per side, layers */
  int32_t cell;          /* RNNT_CELL_* */
  int32_t blank, max_iters, max_out;
  const float* A;        /* (T,B,V) */
  const int32_t* t_lens; /* (B) device, or NULL */
  const float* emb;      /* (V,Hp)  decoder.embedding.weight */
  const float* w_ih[RNNT_DECODE_MAX_LAYERS]; /* (G*Hp,Hp) decoder.rnn.weight_ih_l{k} */
  const float* w_hh[RNNT_DECODE_MAX_LAYERS];
  const float* b_ih[RNNT_DECODE_MAX_LAYERS];
  const float* b_hh[RNNT_DECODE_MAX_LAYERS];
  const float* w_o;      /* (O,Hp)  decoder.out_proj.weight */
  const float* b_o;      /* (O) */
  const float* w_d;      /* fc.weight[:, O_enc:]  (V,O), row stride ld_d floats */
  int64_t ld_d;
  int64_t* tokens;
  int32_t* ntok;
} rnnt_decode_desc;
int rnnt_hip_greedy_decode(const rnnt_decode_desc* d, void* stream);

/* One prediction-net step for a batch with carried state (networks/decoder.py:121-123: `self.rnn(embedded,
 * prev_hidden_state)` on a (B,1) token column, as the reference's search loops call it).  h_in / c_in (L,B,Hp) may be NULL
 * (= zeros: prev_hidden_state None); h_out / c_out (L,B,Hp); the layer output is h_out[L-1].  c_* only for LSTM. */
typedef struct rnnt_prednet_step_desc {
  int32_t B, Hp, L, cell;
  const int64_t* tokens; /* (B) */
  const float* emb;      /* (V,Hp) */
  const float* w_ih[RNNT_DECODE_MAX_LAYERS];
  const float* w_hh[RNNT_DECODE_MAX_LAYERS];
  const float* b_ih[RNNT_DECODE_MAX_LAYERS];
  const float* b_hh[RNNT_DECODE_MAX_LAYERS];
  const float* h_in;
  const float* c_in;
  float* h_out;
  float* c_out;
} rnnt_prednet_step_desc;
int rnnt_hip_prednet_step(const rnnt_prednet_step_desc* d, void* stream);

/* On-device beam search (networks/transducer.py:215-361 with lm=None, hotwords=None: compare_key = asr_score, so the
 * _get_lm_beams bookkeeping (:147-213) never affects the result).  One workgroup per utterance walks all its frames
 * t < t_lens[b] (t_lens NULL: all T).  Per frame A = B_prev, B = []; while A is non-empty: the improved early-out
 * (:298-302, b_best = -9999.0 while B is empty), pop the max-asr_score hypothesis (first in insertion order on ties,
 * Python's max: :288,304), one prediction-net step on y_star[-1] from its state (:307-312), logp = log_softmax of the 1-D
 * joint (:313-315), best_prob = max(logp[1:]) (:317, index 0 skipped even when blank != 0), children k = 0..V-1 with fp64
 * scores (:319-350: blank -> B with the OLD state; others -> A with the new state, k appended to y_star unless it equals
 * y_star[-1]; improved prunes logp[k] < best_prob - expand_beam in fp32), then the stop check len(B) >= beam and
 * max B > max A (:355-358).  Divergence: where the reference's max(A) raises ValueError on an empty A (improved mode only)
 * the frame ends.  Result (:360-361): the last frame's B stable-sorted by asr_score / len(y_star) descending, first `beam`,
 * y_star with the leading blank.
 * A prediction-net step is a pure function of (state, token), so each pop's (h', C) is kept with its blank child and
 * reused when that child is popped in a later frame (memo).  y_star is a prefix tree of (parent, token) nodes.
 * Every structure is bounded by a cap; on overflow status[b] = RNNT_BEAM_ST_* and the utterance returns nothing. */
#define RNNT_BEAM_ST_OK 0
#define RNNT_BEAM_ST_CANDIDATES 1 /* A entries in one frame > max_candidates  */
#define RNNT_BEAM_ST_POPS 2       /* pops in one frame > max_pops             */
#define RNNT_BEAM_ST_STATES 3     /* live prediction-net states > max_states  */
#define RNNT_BEAM_ST_NODES 4      /* prefix-tree nodes > max_nodes            */
#define RNNT_BEAM_ST_LEN 5        /* a returned y_star longer than max_len    */
#define RNNT_BEAM_NSTATS 6        /* per utterance: pops, steps run, max pops/frame, max A entries/frame, max live states, nodes */
typedef struct rnnt_beam_desc {
  int32_t T, B, V;       /* frames, utterances, vocabulary (V >= 2) */
  int32_t Hp, O, L;      /* as rnnt_decode_desc */
  int32_t cell, blank;
  int32_t beam, improved; /* beam_widths, improved (0/1) */
  double state_beam, expand_beam;
  int32_t max_candidates, max_pops, max_states, max_nodes, max_len;  /* caps (see RNNT_BEAM_ST_*) */
  const float* A;        /* (T,B,V) gelu(enc) W_e^T + bias */
  const int32_t* t_lens; /* (B) device, or NULL */
  const float* emb;
  const float* w_ih[RNNT_DECODE_MAX_LAYERS];
  const float* w_hh[RNNT_DECODE_MAX_LAYERS];
  const float* b_ih[RNNT_DECODE_MAX_LAYERS];
  const float* b_hh[RNNT_DECODE_MAX_LAYERS];
  const float* w_o;
  const float* b_o;
  const float* w_d;      /* fc.weight[:, O_enc:], row stride ld_d floats */
  int64_t ld_d;
  void* workspace;       /* rnnt_hip_beam_workspace_bytes(d) bytes, 256-byte aligned */
  size_t workspace_bytes;
  int32_t* tokens;       /* (B, beam, max_len) y_star of rank r, leading blank included */
  int32_t* lens;         /* (B, beam) y_star lengths, 0 past count[b] */
  double* scores;        /* (B, beam) asr_score */
  int32_t* count;        /* (B) hypotheses returned: min(beam, len(B)) */
  int32_t* status;       /* (B) RNNT_BEAM_ST_* */
  int32_t* stats;        /* (B, RNNT_BEAM_NSTATS) or NULL */
} rnnt_beam_desc;
size_t rnnt_hip_beam_workspace_bytes(const rnnt_beam_desc* d);  /* 0 if the descriptor's sizes are invalid */
int rnnt_hip_beam_search(const rnnt_beam_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming greedy recognition (model.py:12-18: the model "continuously processes input samples and streams output
 * symbols"; unidirectional encoder, networks/encoder.py:62; single-step prediction net with carried state,
 * networks/decoder.py:121-123; the greedy loop of networks/transducer.py:95-145).  Features arrive in chunks of T frames per
 * batch of B independent streams; the per-stream state is carried in caller-owned device buffers.  Every per-element
 * product is computed in an order that depends neither on T, on B nor on the chunk boundaries, so any chunking of an
 * utterance gives the same bits (csrc/stream.hip).  fp32 throughout.
 *
 * rnnt_hip_stream_rnn_chunk: the encoder over one chunk (networks/encoder.py:93-103 with hidden state carried in and out).
 *   Stream b runs frames t < lens[b] (0..T); its state is left bitwise as it is past them.  h (L,B,H) (and c for LSTM) hold
 *   the state before the chunk on entry and after it on return.  out[t,b,:] = out_proj(h_top) at b*out_sb + t*out_st
 *   floats, zeros for t >= lens[b].  If A is not NULL it also writes the encoder half of the joint
 *   (networks/transducer.py:64-69), A (T,B,V) time-major = gelu(out) fc_w[:, :O]^T + fc_b, fc_w rows ld_fc floats apart.
 *   T + L + 1 (+1 with A) kernel launches, none of which waits on another workgroup.
 * ---------------------------------------------------------------------------------------------- */
#define RNNT_STREAM_MAX_LAYERS 8
typedef struct rnnt_stream_rnn_desc {
  int32_t T, B, F, H, L, cell; /* chunk frames, streams, input width, hidden, layers (1..8), RNNT_CELL_* */
  int32_t O, V;          /* out_proj width; vocabulary (only with A) */
  const float* x;        /* frame t of stream b at x + b*x_sb + t*x_st, F floats */
  int64_t x_sb, x_st;
  const int32_t* lens;   /* (B) device, in [0, T] */
  const float* w_ih[RNNT_STREAM_MAX_LAYERS]; /* encoder.rnn.weight_ih_l{k} (G*H, F or H) */
  const float* w_hh[RNNT_STREAM_MAX_LAYERS];
  const float* b_ih[RNNT_STREAM_MAX_LAYERS];
  const float* b_hh[RNNT_STREAM_MAX_LAYERS];
  float* h;              /* (L,B,H) in/out */
  float* c;              /* (L,B,H) in/out, LSTM only */
  const float* w_o;      /* encoder.out_proj.weight (O,H) */
  const float* b_o;      /* (O) */
  float* out;
  int64_t out_sb, out_st;
  const float* fc_w;     /* fc.weight, or NULL */
  int64_t ld_fc;
  const float* fc_b;
  float* A;              /* (T,B,V) or NULL */
  void* workspace;       /* rnnt_hip_stream_rnn_workspace_bytes(d) bytes, 256-byte aligned */
  size_t workspace_bytes;
} rnnt_stream_rnn_desc;
size_t rnnt_hip_stream_rnn_workspace_bytes(const rnnt_stream_rnn_desc* d);
int rnnt_hip_stream_rnn_chunk(const rnnt_stream_rnn_desc* d, void* stream);

/* rnnt_hip_stream_greedy: the greedy loop of networks/transducer.py:120-141 continued from carried state.  Per stream b (one
 *   workgroup each), for t < lens[b]: up to max_iters times { tok = argmax_v (A[t,b,v] + C[b,v]); blank ends the frame; tok
 *   is appended to tokens[b] unless it equals last[b]; the prediction net advances with tok from (h, c) and C becomes
 *   gelu(out_proj(h_top)) fc_w[:, O_enc:]^T }.  h / c / C / last are read on entry and written back; a stream with no frames
 *   is not touched.  ntok[b] = tokens appended in this call (at most max_out are stored).
 * rnnt_hip_stream_greedy_reset: rows[0..n_rows) start a new utterance as transducer.py:116-119 does: zero state, one
 *   prediction-net step on blank, last = blank.  Other rows are not touched.  A, lens, tokens, ntok unused. */
typedef struct rnnt_stream_greedy_desc {
  int32_t T, B, V, Hp, O, L, cell; /* as rnnt_decode_desc; T = chunk frames */
  int32_t blank, max_iters, max_out;
  const float* A;        /* (T,B,V) from rnnt_hip_stream_rnn_chunk */
  const int32_t* lens;   /* (B) device */
  const float* emb;
  const float* w_ih[RNNT_DECODE_MAX_LAYERS];
  const float* w_hh[RNNT_DECODE_MAX_LAYERS];
  const float* b_ih[RNNT_DECODE_MAX_LAYERS];
  const float* b_hh[RNNT_DECODE_MAX_LAYERS];
  const float* w_o;
  const float* b_o;
  const float* w_d;      /* fc.weight[:, O_enc:], row stride ld_d floats */
  int64_t ld_d;
  float* h;              /* (L,B,Hp) in/out */
  float* c;              /* (L,B,Hp) in/out, LSTM only */
  float* C;              /* (B,V) in/out: the prediction-net half of the joint for the current state */
  int64_t* last;         /* (B) in/out: last appended token */
  int64_t* tokens;       /* (B,max_out) */
  int32_t* ntok;         /* (B) */
} rnnt_stream_greedy_desc;
int rnnt_hip_stream_greedy(const rnnt_stream_greedy_desc* d, void* stream);
int rnnt_hip_stream_greedy_reset(const rnnt_stream_greedy_desc* d, const int32_t* rows, int32_t n_rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming beam search: the search of rnnt_hip_beam_search (networks/transducer.py:215-361 with lm=None, hotwords=None; the
 * call the reference's inference.py:56-64 makes) fed in chunks.  After any sequence of chunks that together fed frames
 * 0..n-1 of stream b, its n-best is what the offline search gives for an utterance of exactly those n frames, whatever the
 * chunking: the frame loop is the same kernel code (csrc/beam_shared.hpp) and the reference sets A = B at every frame with
 * nothing dropped (:287-288), so the whole last-frame B set is carried, with the state slots and prefix nodes it references.
 *
 * The workspace IS the carried state.  It starts with the layer-0 input table (V, G*Hp) (built by the reset entry when
 * build_table != 0: the weights must not change while a state is open), followed per stream by a 256-byte header of int32
 * { len(B), state slots in use, prefix nodes in use, committed length, RNNT_BEAM_ST_* status, frames consumed }, the A and B entries, the state
 * slots, the slot remap table, the prefix nodes and a node remap table.
 *
 * Chunk call, one workgroup per stream, one launch: load the header; run frames t < lens[b] of A (from
 * rnnt_hip_stream_rnn_chunk); collect the prefix tree (below); write the n-best; store the header.  lens[b] == 0: the
 * stream's workspace is not touched, count[b] = -1 ("the previous list again") and status[b] = 0.
 * Collection: every later hypothesis extends the y_star of a carried B entry, so the lowest common ancestor of their prefix
 * nodes is final.  The tokens on the chain below the old root down to that ancestor go to commit[b] (ncommit[b] of them), the
 * ancestor becomes the root, nodes on no path from it to a B entry are dropped and the rest compacted.  max_nodes therefore
 * bounds the live tree.  Node lengths stay absolute (the final sort divides by len(y_star)).
 * Results: tokens / out_lens hold only the tail of each y_star below the root (after this chunk's collection); the full y_star
 * is every token committed since the stream's reset, leading blank first, followed by the tail.  max_len caps that tail.
 * A cap overflow sets status[b] and the header's status; that stream is refused (same status again) until it is reset.  Other
 * streams are not affected.
 * Reset entry: rows[0..n_rows) (device int32) start a new utterance: B = { y_star [blank], score 0, state None }, committed
 * length 1 (the blank).  Other rows are not touched.  A, lens and the outputs are unused there.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rnnt_beam_stream_desc {
  int32_t T, B, V;       /* chunk frames (0 allowed for the size query and the reset), streams, vocabulary (V >= 2) */
  int32_t Hp, O, L;      /* as rnnt_decode_desc */
  int32_t cell, blank;
  int32_t beam, improved;
  double state_beam, expand_beam;
  int32_t max_candidates, max_pops, max_states, max_nodes, max_len;  /* caps (RNNT_BEAM_ST_*); max_len: uncommitted tail */
  const float* A;        /* (T,B,V) from rnnt_hip_stream_rnn_chunk */
  const int32_t* lens;   /* (B) device, frames of this chunk per stream, in [0, T] */
  const float* emb;
  const float* w_ih[RNNT_DECODE_MAX_LAYERS];
  const float* w_hh[RNNT_DECODE_MAX_LAYERS];
  const float* b_ih[RNNT_DECODE_MAX_LAYERS];
  const float* b_hh[RNNT_DECODE_MAX_LAYERS];
  const float* w_o;
  const float* b_o;
  const float* w_d;      /* fc.weight[:, O_enc:], row stride ld_d floats */
  int64_t ld_d;
  void* workspace;       /* rnnt_hip_beam_stream_workspace_bytes(d) bytes, 256-byte aligned: the carried state */
  size_t workspace_bytes;
  int32_t* tokens;       /* (B, beam, max_len) tail of y_star of rank r */
  int32_t* out_lens;     /* (B, beam) tail lengths, 0 past count[b] */
  double* scores;        /* (B, beam) asr_score */
  int32_t* count;        /* (B) hypotheses returned, -1 for a stream without frames in this chunk */
  int32_t* status;       /* (B) RNNT_BEAM_ST_* */
  int32_t* commit;       /* (B, max_nodes) tokens committed by this chunk */
  int32_t* ncommit;      /* (B) */
  int32_t* stats;        /* (B, RNNT_BEAM_NSTATS) of this chunk (nodes: live after collection), or NULL */
} rnnt_beam_stream_desc;
size_t rnnt_hip_beam_stream_workspace_bytes(const rnnt_beam_stream_desc* d);  /* 0 if the descriptor's sizes are invalid */
int rnnt_hip_beam_stream_reset(const rnnt_beam_stream_desc* d, const int32_t* rows, int32_t n_rows, int32_t build_table,
                               void* stream);
int rnnt_hip_beam_stream_chunk(const rnnt_beam_stream_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Token timestamps and confidences: what the four searches know at the moment they emit.  Each *_timed entry takes the
 * descriptor of its untimed entry (unchanged layout) plus a small struct of extra outputs, runs the SAME kernel (the extra
 * pointers are null in the untimed launch and are the only switch) and returns, besides, bitwise what the untimed entry
 * returns.  A null struct or a null output pointer is RNNT_ERR_INVALID.
 *
 * Greedy (rnnt_hip_greedy_decode_timed, rnnt_hip_stream_greedy_timed): for every token that is APPENDED (entry i of tokens[b])
 *   frames[b,i] = the encoder frame t at which it was chosen;
 *   logp[b,i]   = the log-softmax of the joint at that evaluation, at the chosen token: z[tok] - lse_v(z), z[v] = A[t,b,v] + C[v].
 * A symbol equal to the last appended one advances the prediction net without being appended and gets no entry.  Entries
 * past max_out are dropped exactly as tokens are.  The reduction behind lse is fp32 in an order fixed by (thread, lane, wave)
 * alone (a strided pass per thread, a wave butterfly, the waves in order): it depends neither on B, T nor on chunk
 * boundaries, and it runs only when a token is appended, never per blank evaluation.  Streaming: frames are absolute,
 * frame_base[b] + t with frame_base (B) int64 on the device = the frames stream b consumed since its last reset BEFORE this
 * chunk (NULL: 0); the offline entry ignores frame_base.  Frames are int32 (the low 32 bits of frame_base[b] + t): a stream
 * must be reset before it has consumed 2^31 frames.
 *
 * Beam (rnnt_hip_beam_search_timed, rnnt_hip_beam_stream_chunk_timed): every prefix-tree node carries the frame at which it
 * was created (the pop that materialises its token; -1 for the leading blank), so frames (B, beam, max_len) is aligned with
 * tokens: the frame at which each token of that y_star was appended.  Streaming: node frames are absolute (the stream's
 * consumed-frame count is one more int32 of the workspace header, zeroed by the reset entry and advanced by every chunk,
 * timed or not); frames holds the tail's frames beside the tail's tokens and commit_frames (B, max_nodes) the committed
 * tokens' frames beside commit.  Collection and compaction move the frame with its node.  No per-token confidence here: a
 * hypothesis has its score.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rnnt_greedy_timing {
  int32_t* frames;           /* (B,max_out) */
  float* logp;               /* (B,max_out) */
  const int64_t* frame_base; /* (B) device or NULL; streaming only */
} rnnt_greedy_timing;
int rnnt_hip_greedy_decode_timed(const rnnt_decode_desc* d, const rnnt_greedy_timing* timing, void* stream);
int rnnt_hip_stream_greedy_timed(const rnnt_stream_greedy_desc* d, const rnnt_greedy_timing* timing, void* stream);

typedef struct rnnt_beam_timing {
  int32_t* frames;        /* (B, beam, max_len) beside tokens */
  int32_t* commit_frames; /* (B, max_nodes) beside commit; streaming only */
} rnnt_beam_timing;
int rnnt_hip_beam_search_timed(const rnnt_beam_desc* d, const rnnt_beam_timing* timing, void* stream);
int rnnt_hip_beam_stream_chunk_timed(const rnnt_beam_stream_desc* d, const rnnt_beam_timing* timing, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Beam search with token-level fusion: hotword boosting and token / grapheme LM tables.  The reference's lm= / hotwords= branch
 * (networks/transducer.py:147-213, 253-264, 352-361; inference.py:56-64) ranks hypotheses by "lm_score" = asr_score plus a
 * score that depends on the decoded y_star alone; it computes that score with pyctcdecode and KenLM over text.  Here the score
 * is that of a weighted DETERMINISTIC AUTOMATON over token ids, held as dense tables on the device:
 *   next  (S, V) int32    next[s*V + k]: the state after appending token k in state s, in [0, S) (values outside are clamped)
 *   arc   (S, V) float32  the score added by that append
 *   final (S)    float32  added once, only when a hypothesis is ranked for output
 * State 0 is the start state: it belongs to y_star = [blank].  total(y) = sum_i arc[s_{i-1}, y_i] over the tokens after the
 * leading blank, accumulated in fp64 in append order.  The automaton advances only when a token is APPENDED: a blank child and
 * a child whose token equals y_star[-1] (the dedupe rule, :337, :345) keep state and total.
 * Every comparison the reference makes on compare_key uses key = asr_score + total: the pop argmax over A (:285-288), the best
 * of B (:293), the improved early-out (:295), the stop test (:355-358); the result is the last frame's B stable-sorted by
 * (asr_score + total + final[state]) / len(y_star) (:360).  The prune test stays on the fp32 ASR log-probabilities (:336).
 * `final` is never stored back, so the streaming search keeps "after every chunk the n-best is the offline result for the
 * frames so far".  scores still returns asr_score; fused_scores returns asr_score + total + final[state].
 * With positive arcs a frame's pop loop need not end (a hypothesis that keeps earning more than its log-probability falls; the
 * reference has the same hazard with hotwords): max_pops bounds it, status RNNT_BEAM_ST_POPS.
 *
 * The fused entries take the descriptor of their unfused entry (unchanged layout), the fusion struct, and a timing struct that
 * may be NULL (no frames).  They run the FUSED instance of the one kernel template (csrc/beam_shared.hpp); the unfused entries
 * are untouched.  The workspace is the unfused one followed, per utterance, by the total (fp64) and state (int32) of every A
 * and B entry: 12 * (max_candidates + max_pops) bytes rounded up to 256 twice; query it with the *_fused_workspace_bytes
 * entries.  A stream's automaton is fixed by rnnt_hip_beam_stream_reset_fused (which also seeds state 0, total 0): pass the
 * same tables to every chunk.  All argument checks (a NULL table, n_states < 1, n_states * V > 2^27, a misaligned or short
 * workspace) happen on the host before any device work.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rnnt_beam_fusion {
  const int32_t* next;   /* (S, V) device */
  const float* arc;      /* (S, V) device */
  const float* final;    /* (S) device */
  int32_t n_states;      /* S >= 1, S * V <= 2^27 */
  double* fused_scores;  /* (B, beam) device, beside scores: asr_score + total + final[state] */
} rnnt_beam_fusion;
size_t rnnt_hip_beam_fused_workspace_bytes(const rnnt_beam_desc* d);  /* 0 if the descriptor's sizes are invalid */
int rnnt_hip_beam_search_fused(const rnnt_beam_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_timing* timing, void* stream);
size_t rnnt_hip_beam_stream_fused_workspace_bytes(const rnnt_beam_stream_desc* d);
int rnnt_hip_beam_stream_reset_fused(const rnnt_beam_stream_desc* d, const rnnt_beam_fusion* fusion, const int32_t* rows,
                                     int32_t n_rows, int32_t build_table, void* stream);
int rnnt_hip_beam_stream_chunk_fused(const rnnt_beam_stream_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_timing* timing,
                                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frame-synchronous transducer beam search with batched hypothesis steps.  csrc/beam_sync.hip, DESIGN.md §20.
 * The search every other transducer toolkit decodes with (time-synchronous / "modified" beam search): every frame expands the
 * whole beam at once, emits at most max_symbols tokens, merges hypotheses with the same token sequence by logaddexp (a score is
 * probability mass, not one path), and advances the prediction net once for all new hypotheses together.  Its cost per frame is
 * bounded by W, V and S alone, with or without fusion.  rnnt_hip_beam_search stays the reference-faithful best-first search.
 *
 * Inputs: A (time-major: frame t of utterance b at A + t*a_st + b*a_sb, V floats) = gelu(enc_t) W_e^T + bias as for
 * rnnt_hip_beam_search; the prediction net and its half of the joint; blank; W = beam in [1,64]; S = max_symbols in [1,4];
 * token_min_logp (-inf: no pruning; neither NaN nor +inf); optionally the automaton of rnnt_beam_fusion over the same V.
 * Hypothesis: a prefix-tree node (its token sequence y; the root is [blank]; ONE node per prefix), an fp64 score, a
 * prediction-net state with its joint half Cv, and with fusion an automaton state and an fp64 total.
 * lp_h[v] = the fp32 log-softmax over v of A_t[v] + Cv_h[v].
 *   start    one hypothesis: the root, score 0; its state is one step on blank from the zero state
 *   frame    for each t < t_lens[b] (clamped to [0,T]; NULL: T), with C = the beam A and D = empty, rounds r = 0..S-1; an empty C
 *            stops the rounds:
 *     1. candidates of the member h at rank i of C: blank with value score_h + lp_h[blank], and every v != blank with
 *        lp_h[v] >= token_min_logp with value score_h + lp_h[v]; candidate id i V + v.  With fusion the rank key is
 *        value + total', total' = total_h for blank and total_h + arc[s_h, v] otherwise; the pruning test stays on lp.
 *        (Internal-LM subtraction, rnnt_hip_beam_sync_search_ilm below: total' = (total_h + arc[s_h, v]) - mu * ilm_h[v].)
 *     2. the min(W, #candidates) best by (key descending, id ascending) are selected; a value or key of -inf is dropped.
 *     3. in rank order: a selected blank closes h: it is added to D under h's node, and if that node is in D already the scores
 *        merge, score = logaddexp(old, new) (state and total are the same by construction).  A selected token v makes the
 *        child: its node is found among the parent node's children or created; it carries the new score, the automaton advanced
 *        (next values outside [0,S) are clamped) and the prediction-net state one step further.  If r < S-1 the child joins the
 *        next round's C in rank order; if r = S-1 it is added to D like a closed one: the frame advances without a blank, as
 *        greedy search does after max_iters tokens.
 *     4. the next A = the min(W, |D|) best of D by (score [+ total] descending, order of first insertion into D ascending).
 *   output   A after the last valid frame, best first by score (fused: score + total + final[state]), ties in A's order, no length
 *            normalisation; t_lens[b] = 0 gives [[blank]] with score 0.
 * Outputs: count (B) = hypotheses of utterance b; for o < count[b]: lens[b,o], tokens[b,o,:lens] (tokens is (B, W, 1 + S T) int32;
 * y with the leading blank, as rnnt_hip_beam_search returns y_star), scores[b,o] fp64, with fusion fusion->fused_scores[b,o], and
 * with timing timing->frames (B, W, 1 + S T): per token the frame at which its prefix's node was created (-1 for the leading
 * blank).  Nothing is written for o >= count[b] or past lens[b,o].
 * Bounds: at most W new nodes per round, 1 + W S T nodes per utterance, |D| <= (S+1) W, len(y) <= 1 + S T: everything is bounded in
 * advance, the search has no cap that can overflow and no error path at run time; the workspace query sizes all of it (the layer-0
 * input table, the candidate keys, the prefix tree and (S+2) W state slots per utterance).
 * step_group: 0, or a smaller number of hypotheses per step group than the LDS budget allows (rnnt_hip_beam_sync_step_group tells
 * the number in use, at most 8); a hypothesis's state is the same bits in any group, so results do not depend on it.
 * Every limit is checked on the host before any launch (RNNT_ERR_INVALID): W, S, V >= 2, blank, W V <= 2^24, 1 + W S T < 2^31 / 5,
 * the threshold, pointers, strides, the fusion tables (n_states >= 1, n_states * V <= 2^27, non-NULL tables and fused_scores), the
 * workspace (256-byte aligned, rnnt_hip_beam_sync_workspace_bytes(d) bytes; 0 for sizes outside the limits).
 * One table launch and one search launch, a workgroup per utterance, every sum in one fixed order: the same bits on every call,
 * and a row alone gives the bits it gives in any batch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rnnt_beam_sync_desc {
  int32_t T, B, V;       /* frames, utterances, vocabulary (V >= 2) */
  int32_t Hp, O, L;      /* as rnnt_decode_desc */
  int32_t cell, blank;
  int32_t beam, max_symbols; /* W in [1,64], S in [1,4] */
  int32_t step_group;    /* 0, or hypotheses per step group (smaller than the LDS would hold) */
  float token_min_logp;
  const float* A;        /* gelu(enc) W_e^T + bias, time-major */
  int64_t a_st, a_sb;    /* strides of A in floats: frame, utterance ((T,B,V) contiguous: B*V, V) */
  const int32_t* t_lens; /* (B) device, or NULL */
  const float* emb;
  const float* w_ih[RNNT_DECODE_MAX_LAYERS];
  const float* w_hh[RNNT_DECODE_MAX_LAYERS];
  const float* b_ih[RNNT_DECODE_MAX_LAYERS];
  const float* b_hh[RNNT_DECODE_MAX_LAYERS];
  const float* w_o;
  const float* b_o;
  const float* w_d;      /* fc.weight[:, O_enc:], row stride ld_d floats */
  int64_t ld_d;
  void* workspace;       /* rnnt_hip_beam_sync_workspace_bytes(d) bytes, 256-byte aligned */
  size_t workspace_bytes;
  int32_t* tokens;       /* (B, beam, 1 + max_symbols*T) */
  int32_t* lens;         /* (B, beam) */
  double* scores;        /* (B, beam) */
  int32_t* count;        /* (B) */
} rnnt_beam_sync_desc;
size_t rnnt_hip_beam_sync_workspace_bytes(const rnnt_beam_sync_desc* d);  /* 0 if the descriptor's sizes are invalid */
int rnnt_hip_beam_sync_step_group(const rnnt_beam_sync_desc* d);          /* hypotheses per step group; 0 if invalid */
int rnnt_hip_beam_sync_search(const rnnt_beam_sync_desc* d, const rnnt_beam_fusion* fusion /* or NULL */,
                              const rnnt_beam_timing* timing /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming frame-synchronous beam search: the search of rnnt_hip_beam_sync_search fed in chunks, the hypotheses carried on the
 * device.  csrc/beam_sync_stream.hip, DESIGN.md §21.  The kernel is the STREAM instance of the offline entry's template
 * (csrc/beam_sync_shared.hpp): the same frame loop, so the definition above holds word for word.
 *
 * After any sequence of chunks that together fed frames 0..n-1 of stream b since its last reset, its n-best is exactly what
 * rnnt_hip_beam_sync_search returns for an utterance of those n frames: the same token lists, the same fp64 score bits (and
 * fused_scores bits), the same per-token frames, whatever the chunking, 1-frame chunks and chunks in which the stream has no
 * frames included.  The cost per frame is the offline one, fixed by W, V and S; there is no pop loop and nothing a score can
 * overflow.  The only run-time error paths are the two caps max_nodes and max_len below.
 *
 * The workspace IS the carried state.  It starts with the layer-0 input table (V, G*Hp) (built by the reset entry when
 * build_table != 0: the weights must not change while a state is open), followed per stream by
 *   a 256-byte header of int32 { nA = members of the beam, prefix nodes in use, tokens committed since the reset (the leading
 *     blank counts), frames consumed since the reset, RNNT_BEAM_ST_* status, collections run, of those the ones run at a
 *     frame's start, largest node count seen };
 *   the beam A in rank order, W entries each of: fp64 score[W], fp64 fusion total[W], int32 node[W], automaton state[W], state
 *     slot[W], pending token[W].  pending token >= 0: a child of the last frame's last round whose prediction-net step has not
 *     run; its slot is its PARENT's (-1: the zero state) and the step runs at the next frame's first round, exactly as offline.
 *     Nothing steps after the last fed frame;
 *   (S+2) W prediction-net state slots (h | c | Cv);
 *   W V candidate keys (scratch of a round, not carried);
 *   the prefix tree, 5 int32 per node (parent, token, frame, first child, next sibling), max_nodes nodes;
 *   2 int32 per node of scratch for the collection.
 * Reset entry: rows[0..n_rows) (device int32) start a new utterance: the beam is the offline seed (the root, score 0, automaton
 * state 0, total 0, a pending step on blank from the zero state), the tree is the root, one token (the blank) is committed, no
 * frames are consumed.  Other rows are not touched.  A, lens and the outputs are unused there.
 * Chunk call, one launch, one workgroup per stream: load the beam; run frames t < lens[b] (clamped to [0,T]) of A; collect the
 * prefix tree; write the n-best; store the beam and the header.  lens[b] == 0: the stream's workspace is not touched,
 * count[b] = -1 ("the previous list again"), ncommit[b] = 0 and status[b] = the header's status.
 * Frames are absolute: a node created at frame t of this chunk is stamped (frames consumed before the chunk) + t.  Nodes always
 * carry their frame; timing only selects whether frames are written out.
 * Collection.  Every later hypothesis extends a member of the carried beam, so R = the lowest common ancestor of the members'
 * nodes is final.  The tokens (and frames) on the chain from below the old root down to R, R included, are appended to
 * commit[b] (commit_frames[b]); ncommit[b] counts them for the chunk.  R becomes node 0.  Kept are exactly: the nodes on a path
 * from R to a member, and every descendant of a member's node: those are the only nodes a later frame can look up again, and
 * keeping them keeps the offline rule "one node per prefix, stamped at its first creation" (keeping only the paths to the
 * members would re-create a prefix that is pruned and reached again, with a later frame).  Everything else is dropped; the
 * compaction preserves index order.  Node numbers and sibling order enter no decision of the search.
 * The kernel collects at the chunk's end and at the start of any frame that finds fewer than W S node slots free.  The
 * collected tree is a function of the frames fed alone.
 * Caps.  max_nodes (>= 1 + 4 W S) bounds the tree at any moment: if fewer than W S slots are free at a frame's start even
 * after collecting, status RNNT_BEAM_ST_NODES; the stream stops before that frame, and which frame that is depends only on the
 * frames fed, not on the chunking.  max_len (>= 1) bounds the tail of a RETURNED token sequence, the tokens below the root
 * after the chunk's last collection: a longer tail gives RNNT_BEAM_ST_LEN where it would be returned, at a chunk's end.
 * Either status is stored in the header (with the frames consumed until then): the stream's beam is no longer valid, count[b]
 * = 0, and every later chunk returns count[b] = -1 with that status until the stream is reset.  Other streams are unaffected.
 * Results: count / out_lens / tokens / scores (and fused_scores, frames) as rnnt_hip_beam_sync_search writes them, with rows of
 * max_len entries that hold the TAIL of each y below the root; the full y is every token committed since the reset, leading
 * blank first, followed by the tail.  Nothing is written for o >= count[b] or past out_lens[b,o].
 * fusion (or NULL): the automaton must be the same for every chunk of a stream; its state and total are carried with every
 * member, `final` is applied only where the n-best is ranked.  timing (or NULL): frames (B, beam, max_len) beside tokens and
 * commit_frames (B, max_nodes + S T) beside commit; both or neither.
 * Every check happens on the host before any launch (RNNT_ERR_INVALID): those of rnnt_hip_beam_sync_search, the two caps, the
 * workspace (256-byte aligned, rnnt_hip_beam_sync_stream_workspace_bytes(d) bytes; 0 for sizes outside the limits), T >= 1, the
 * pointers and strides of the chunk call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rnnt_beam_sync_stream_desc {
  int32_t T, B, V;       /* chunk frames (0 allowed for the size query and the reset), streams, vocabulary (V >= 2) */
  int32_t Hp, O, L;      /* as rnnt_decode_desc */
  int32_t cell, blank;
  int32_t beam, max_symbols; /* W in [1,64], S in [1,4] */
  int32_t step_group;    /* as rnnt_beam_sync_desc */
  float token_min_logp;
  int32_t max_nodes, max_len; /* caps: live prefix nodes (>= 1 + 4 W S), tokens of a returned tail (>= 1) */
  const float* A;        /* gelu(enc) W_e^T + bias of the chunk, time-major (rnnt_hip_stream_rnn_chunk) */
  int64_t a_st, a_sb;    /* strides of A in floats: frame, stream ((T,B,V) contiguous: B*V, V) */
  const int32_t* lens;   /* (B) device, frames of this chunk per stream, in [0, T] */
  const float* emb;
  const float* w_ih[RNNT_DECODE_MAX_LAYERS];
  const float* w_hh[RNNT_DECODE_MAX_LAYERS];
  const float* b_ih[RNNT_DECODE_MAX_LAYERS];
  const float* b_hh[RNNT_DECODE_MAX_LAYERS];
  const float* w_o;
  const float* b_o;
  const float* w_d;      /* fc.weight[:, O_enc:], row stride ld_d floats */
  int64_t ld_d;
  void* workspace;       /* rnnt_hip_beam_sync_stream_workspace_bytes(d) bytes, 256-byte aligned: the carried state */
  size_t workspace_bytes;
  int32_t* tokens;       /* (B, beam, max_len) tail of y of rank o */
  int32_t* out_lens;     /* (B, beam) tail lengths */
  double* scores;        /* (B, beam) */
  int32_t* count;        /* (B) hypotheses returned; -1 for a stream without frames in this chunk or failed earlier */
  int32_t* status;       /* (B) RNNT_BEAM_ST_OK, RNNT_BEAM_ST_NODES or RNNT_BEAM_ST_LEN */
  int32_t* commit;       /* (B, max_nodes + max_symbols*T) tokens committed by this chunk, oldest first */
  int32_t* ncommit;      /* (B) */
} rnnt_beam_sync_stream_desc;
size_t rnnt_hip_beam_sync_stream_workspace_bytes(const rnnt_beam_sync_stream_desc* d);  /* 0 if the descriptor's sizes are invalid */
int rnnt_hip_beam_sync_stream_reset(const rnnt_beam_sync_stream_desc* d, const int32_t* rows, int32_t n_rows, int32_t build_table,
                                    void* stream);
int rnnt_hip_beam_sync_stream_chunk(const rnnt_beam_sync_stream_desc* d, const rnnt_beam_fusion* fusion /* or NULL */,
                                    const rnnt_beam_timing* timing /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backoff n-gram fusion for the searches whose cost per frame is bounded: the frame-synchronous transducer search, its
 * streaming form and the CTC prefix beam search.  csrc/search_shared.hpp (ngram_lookup), DESIGN.md §23.
 * The automaton of rnnt_beam_fusion in sparse (CSR) form: one state per context of a backoff n-gram model, whose row lists only
 * the tokens the model lists after that context; every other token backs off.  Device tables:
 *   row_ptr (S+1) int32    arcs of state s are [row_ptr[s], row_ptr[s+1])
 *   tok     (E)   int32    token ids, strictly ascending inside a state
 *   arc     (E)   float32  the score of that append (weight * ln p)
 *   next    (E)   int32    state after the append
 *   bow     (S)   float32  the score of backing off from s (weight * ln backoff)
 *   backoff (S)   int32    where s backs off to; the root backs off to itself
 *   final   (S)   float32  added once, only when a hypothesis is ranked for output
 * State 0 is the start state.  The root's row lists every token 0..V-1 (so n_arcs >= V), which ends every lookup.
 * Lookup of token k in state s:
 *     acc = 0.0 (fp64); h = s
 *     repeat at most `order` times:
 *         if k is listed in h at e:  return arc' = (float)(acc + (double)arc[e]),  next[e]
 *         if h == root: break
 *         acc += (double)bow[h];  h = backoff[h]
 *     return (float)acc, root            (unreachable with tables as described)
 * arc' enters the search exactly where the dense arc[s*V + k] does, as (double)arc' added to the fp64 total in append order, and
 * next where the dense next does: a dense rnnt_beam_fusion filled with arc' and next for every (s, k) gives the same bits.
 * On the device every index read from a table is clamped into its range and the walk is bounded by order <= 8: tables that
 * break the description cost a wrong score, never an out-of-range read or an unbounded loop.
 * The *_ngram entries take the descriptor, the workspace and every other argument of the entry they extend, unchanged; they run
 * the backoff instance of the same kernel template.  Checked on the host before any launch (RNNT_ERR_INVALID), beside the
 * extended entry's own checks: a NULL struct or table, n_states >= 1, 0 <= root < n_states, 1 <= order <= 8, n_arcs >= V, a
 * non-NULL fused_scores.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rnnt_beam_ngram {
  const int32_t* row_ptr; /* (S+1) device */
  const int32_t* tok;     /* (E) device */
  const float* arc;       /* (E) device */
  const int32_t* next;    /* (E) device */
  const float* bow;       /* (S) device */
  const int32_t* backoff; /* (S) device */
  const float* final;     /* (S) device */
  int32_t root, order;    /* the empty context's state; the longest walk, in [1,8] */
  int32_t n_states, n_arcs; /* S >= 1, E >= V */
  double* fused_scores;   /* (B, beam) device, beside scores: score + total + final[state] */
} rnnt_beam_ngram;
int rnnt_hip_beam_sync_search_ngram(const rnnt_beam_sync_desc* d, const rnnt_beam_ngram* lm, const rnnt_beam_timing* timing /* or NULL */,
                                    void* stream);
int rnnt_hip_beam_sync_stream_chunk_ngram(const rnnt_beam_sync_stream_desc* d, const rnnt_beam_ngram* lm,
                                          const rnnt_beam_timing* timing /* or NULL */, void* stream);
int rnnt_hip_ctc_beam_search_ngram(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T,
                                   int32_t V, int32_t blank, int32_t W, float token_min_logp, const rnnt_beam_ngram* lm,
                                   int32_t* tokens, int32_t* lens, double* scores, int32_t* frames, int32_t* counts, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Internal-LM subtraction (ILME; Meng et al. 2021, "Internal Language Model Estimation for Domain-Adaptive End-to-End Speech
 * Recognition") for the frame-synchronous search and its streaming form.  csrc/beam_sync_shared.hpp, DESIGN.md §25.
 * A transducer's prediction net is a language model of the training transcripts; shallow fusion with an external LM counts a
 * language prior twice.  The internal LM is the joint with the encoder's contribution zeroed: the joint is
 * fc(gelu(cat(enc, dec))) and gelu(0) = 0, so the internal-LM logits of hypothesis h are exactly Cv_h[v] + bias[v], with Cv_h the
 * joint half the search already keeps per prediction-net state and bias = fc.bias.
 * Definition.  For v != blank:
 *     ilm_h[v] = ((Cv_h[v] + bias[v]) - m_h) - lse_h                                   (fp32)
 * the log-softmax over the NON-BLANK vocabulary: m_h = max over v != blank of Cv_h[v] + bias[v], lse_h = log of the sum over
 * v != blank of exp((Cv_h[v] + bias[v]) - m_h).  The blank is excluded from the maximum and from the sum.
 * With weight mu > 0, step 1 of rnnt_hip_beam_sync_search's definition changes in one place: for a candidate v != blank
 *     total' = (total_h + (double)arc[s_h, v]) - (double)mu * (double)ilm_h[v]         (fp64, no fused multiply-add)
 * This one expression is evaluated where the candidate keys are filled and again where the selected candidates are built: the
 * same bits at both.  The blank is unchanged (total' = total_h).  Everything else reads as before: ranking by score + total,
 * the top-W of D, the output order by score + total + final[state], fused_scores, frames; the pruning test stays on lp, the ASR
 * log-probability.  fused_scores = score + total + final with total = the automaton's arcs along y minus mu times the sum of
 * ilm over y's tokens.
 * ilm_h is a function of y alone, because the prediction-net state is; so are the automaton's state and total.  The merge
 * rule's "state and total are the same by construction" therefore still holds with the term in the total.
 * -mu * ilm_h[v] is a per-token bonus >= 0.  The search is bounded by W, V, S and T in advance and has no pop loop: no bonus,
 * however large, can make a cap overflow (rnnt_hip_beam_search's best-first search has no such bound and takes no ilm).
 * V = 2 has one non-blank token: m = the logit, exp(0) = 1, log 1 = 0, ilm = 0 and total' = (total + arc) - 0: the *_ilm entry
 * returns the bits of the entry it extends.
 * (m_h, lse_h) is computed once per prediction-net step (a wavefront per new state, lanes along v, in an order that depends on
 * neither the step group nor the hypothesis's place in it) and kept per state slot: 2 floats per slot behind the other
 * workspace parts ((B, NS, 2) offline; one more carried part per stream, which chunk boundaries and collections leave alone:
 * a collection moves prefix nodes, never state slots).  So the *_ilm entries have their own workspace queries, and a stream
 * opened for them its own reset.  The descriptor and every other argument are those of the entry they extend.
 * Entries: exactly one of fusion / lm is given (ILM subtraction alone: a one-state all-zero rnnt_beam_fusion); ilm is required.
 * Checked on the host before any launch (RNNT_ERR_INVALID), beside the extended entry's own checks: ilm NULL, bias NULL, weight
 * not finite or <= 0, both or neither of fusion / lm, the workspace smaller than the *_ilm query's size or misaligned.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rnnt_beam_ilm {
  const float* bias;      /* (V) fc.bias, device */
  float weight;           /* mu: finite, > 0 */
} rnnt_beam_ilm;
size_t rnnt_hip_beam_sync_ilm_workspace_bytes(const rnnt_beam_sync_desc* d);  /* 0 if the descriptor's sizes are invalid */
int rnnt_hip_beam_sync_search_ilm(const rnnt_beam_sync_desc* d, const rnnt_beam_fusion* fusion /* or NULL */,
                                  const rnnt_beam_ngram* lm /* or NULL */, const rnnt_beam_ilm* ilm,
                                  const rnnt_beam_timing* timing /* or NULL */, void* stream);
size_t rnnt_hip_beam_sync_stream_ilm_workspace_bytes(const rnnt_beam_sync_stream_desc* d);  /* 0 if the sizes are invalid */
int rnnt_hip_beam_sync_stream_reset_ilm(const rnnt_beam_sync_stream_desc* d, const int32_t* rows, int32_t n_rows, int32_t build_table,
                                        void* stream);
int rnnt_hip_beam_sync_stream_chunk_ilm(const rnnt_beam_sync_stream_desc* d, const rnnt_beam_fusion* fusion /* or NULL */,
                                        const rnnt_beam_ngram* lm /* or NULL */, const rnnt_beam_ilm* ilm,
                                        const rnnt_beam_timing* timing /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Internal-LM training (ILMT; Meng et al. 2021, "Internal Language Model Training for Domain-Adaptive End-to-End Speech
 * Recognition"; the same term on text alone: Meng et al. 2021, "Internal Language Model Adaptation with Text-Only Data for End-to-End
 * Speech Recognition").  csrc/ilm_loss.hip, DESIGN.md §26.
 * The cross-entropy of the internal LM of the ILME section above on the transcripts, as a training term.  C is the decoder half of
 * the joint, the (U1, B, V) operand of the fused loss: C(u,b,v) = C[b*c_sb + u*c_su + v] (batch-major and time-major buffers both
 * work, the inner stride is 1; c_su >= V), bias = fc.bias (V).  labels (B,U) int32 (U = U1-1), u_lens (B) int32 in [0,U] (clamped to
 * that range on the device), blank in [0,V).  For v != blank:
 *     z(u,b,v)   = C(u,b,v) + bias[v]
 *     lse(u,b)   = m + log sum_{v != blank} exp(z(u,b,v) - m),   m = max_{v != blank} z(u,b,v)
 *     ilm_nll[b] = sum_{u < u_lens[b]} (lse(u,b) - z(u,b,labels[b,u]))         evaluated as (m - z(u,b,y)) + log sum exp(z - m)
 *     dC(u,b,v)  = gscale * gvec[b*gvec_stride] * (exp(z(u,b,v) - lse(u,b)) - [v == labels[b,u]])     u < u_lens[b], v != blank
 *                = 0                                                 elsewhere (the blank column, u >= u_lens[b], row U1-1)
 * ilm_nll[b] is minus JointNet.ilm_score of row b: a per-utterance sum over tokens, not length-normalised.  Per-token terms are fp32
 * with the row maximum subtracted; the per-utterance sum is fp64 in a fixed order that depends on u_lens[b] alone, rounded once to
 * fp32.  No float atomics: the same bits on every call, and a row gives the same bits alone as in any batch.
 * V = 2 leaves one non-blank token: ilm_nll is exactly 0 and the gradient exactly zero.
 * A counted label that is the blank or lies outside [0,V) is not checked on the host (that would cost a synchronisation): the row
 * gets ilm_nll[b] = +inf and an exactly zero row of dC, every other row is bitwise what it is alone, and nothing is read out of
 * bounds.  Labels at u >= u_lens[b] and rows u >= u_lens[b] of C are never read.
 * rnnt_hip_ilm_loss_fwd: one launch.  lse, if given, receives lse(u,b) at lse[u*B + b] for u < u_lens[b] (other entries are not
 *   written) for the backward.
 * rnnt_hip_ilm_loss_bwd: one launch, on the SAME operands; lse = that buffer, or NULL: the rows' lse is recomputed (the same bits).
 *   dC has C's strides.  accumulate = 0 writes the whole dC (V entries of every row; cells that are not counted become exact zeros);
 *   accumulate != 0 adds into a dC that holds values already (the lattice gradient of rnnt_hip_joint_loss_bwd) as one rounded product
 *   and one addition per cell, and leaves uncounted rows and the blank column untouched.  gscale, gvec, gvec_stride as in
 *   rnnt_hip_joint_loss_bwd (gvec NULL = ones).
 * Arguments are validated before any device work (RNNT_ERR_INVALID): a null pointer (lse and gvec may be NULL), B < 1, U1 < 1,
 * V < 2, blank outside [0,V), c_su < V.  Nothing allocates or synchronises.
 * ---------------------------------------------------------------------------------------------- */
int rnnt_hip_ilm_loss_fwd(const float* C, int64_t c_sb, int64_t c_su, const float* bias, const int32_t* labels,
                          const int32_t* u_lens, int32_t B, int32_t U1, int32_t V, int32_t blank,
                          float* ilm_nll, float* lse /* (U1*B) or NULL */, void* stream);
int rnnt_hip_ilm_loss_bwd(const float* C, int64_t c_sb, int64_t c_su, const float* bias, const int32_t* labels,
                          const int32_t* u_lens, const float* lse /* or NULL: recompute */, int32_t B, int32_t U1,
                          int32_t V, int32_t blank, float gscale, const float* gvec, int32_t gvec_stride,
                          int32_t accumulate, float* dC, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Input side on device (datamodule.py:48-90, done offline on the host by the reference).
 * rnnt_hip_frontend_norm_pad: per utterance b (row b of wav, lens[b] samples): optional mean / population-variance
 *   normalisation (datamodule.py:87-90), reflect padding by `pad` samples at the utterance's own ends (torch.stft
 *   center=True), zeros up to Lp.  out (B, Lp).  lens[b] is clamped to [0, ld]; a row of length 0 is all zeros.  A
 *   length 0 < lens[b] <= pad is outside the contract (one reflection does not land inside the utterance; torch.stft
 *   raises there): the positions it cannot reach are written as 0.
 * The windowed DFT is then ONE rnnt_hip_gemm_f32 over the frames in place: M = B*F rows with a_div = F, a_so = Lp,
 *   a_si = hop, K = n_fft, B = hann * [cos | -sin] basis (2*n_bins, n_fft).
 * rnnt_hip_power_mel_log1p: spec (M, 2*n_bins) = [re | im] -> out (M, n_mels) = log1p(fb^T |X|^2), rows whose frame index
 *   (m % frames_per_utt) is >= nframes[m / frames_per_utt] are written as 0 (the collate's pad value, dataloader.py:40).
 * ---------------------------------------------------------------------------------------------- */
int rnnt_hip_frontend_norm_pad(const float* wav, int64_t ld, const int32_t* lens, int32_t B, int32_t pad, int64_t Lp,
                               int32_t normalize, float* out, void* stream);
int rnnt_hip_power_mel_log1p(const float* spec, int64_t M, int32_t n_bins, const float* fb, int32_t n_mels,
                             const int32_t* nframes, int32_t frames_per_utt, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MWER (minimum word error rate) training: the pieces between rnnt_hip_beam_sync_search and the fused loss (csrc/mwer.hip).
 * Errors are counted on token ids.
 * rnnt_hip_edit_distance: dist[p] = Levenshtein distance (substitution, insertion, deletion cost 1 each) between the first
 *   hyp_lens[p] tokens of row p of hyp (row stride hyp_ld) and the first ref_lens[p / ref_div] tokens of row p / ref_div of ref
 *   (row stride ref_ld): ref_div hypotheses share one reference without a copy.  Integer arithmetic, exact.  Either length may
 *   be 0; a length is clamped to [0, ld], and both ld must lie in [0, 511] (the loss's U + 1 <= 512) — longer rows are refused.
 *   One wavefront per pair.
 * rnnt_hip_nbest_pack: the search's outputs tokens (B, N, max_len) (leading blank included), counts (B), lens (B, N) -> the
 *   loss's inputs for rows r = b*N + n:  texts (B*N, Umax+1) int64 = blank, the hypothesis, blank padding;  labels (B*N, Umax)
 *   = the hypothesis, blank padding;  u_lens (B*N);  t_lens (B*N) = frame_lens[b], or 0 for an invalid row (the loss then gives
 *   +inf and exact-zero gradients for it);  valid (B*N) 0 / 1.  Row (b, n) is valid when n < counts[b] and its lens - 1 tokens
 *   are at most max_hyp_len and at most Umax; an invalid row is packed as the empty hypothesis.  lens of a rank >= counts[b]
 *   is not read.  N <= 64, Umax and max_hyp_len in [1, 511].
 * rnnt_hip_mwer_risk: per utterance b over its valid rows i (valid[b*N + i] != 0 and nll not NaN), in fp64:
 *     P^_i = softmax_i(-nll_i) (the minimum nll subtracted first),  Wbar = mean_i dist_i,
 *     risk[b] = sum_i P^_i (dist_i - Wbar),   weights[b*N + j] = gscale * d risk[b] / d nll_j = -gscale P^_j (dist_j - sum_i P^_i dist_i)
 *   both stored as fp32.  An invalid row has weight exactly 0 and its nll (+inf) never enters the arithmetic; fewer than two
 *   valid rows (or no valid row with a finite nll) give risk 0 and weights 0.  Sums run in index order, one wavefront per
 *   utterance: a row's result does not depend on the batch around it.  N <= 64.
 * All three check their arguments on the host before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
int rnnt_hip_edit_distance(const int32_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, const int32_t* ref, int64_t ref_ld,
                           const int32_t* ref_lens, int32_t ref_div, int32_t P, int32_t* dist, void* stream);
int rnnt_hip_nbest_pack(const int32_t* tokens, int64_t max_len, const int32_t* counts, const int32_t* lens, const int32_t* frame_lens,
                        int32_t B, int32_t N, int32_t Umax, int32_t max_hyp_len, int32_t blank, int64_t* texts, int32_t* labels,
                        int32_t* u_lens, int32_t* t_lens, int32_t* valid, void* stream);
int rnnt_hip_mwer_risk(const float* nll, const int32_t* dist, const int32_t* valid, int32_t B, int32_t N, double gscale, float* risk,
                       float* weights, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CTC-guided blank-frame skipping in front of the transducer searches.  csrc/ctc_skip.hip, DESIGN.md §29.
 * logits(b,t,v) = logits[b*z_sb + t*z_st + v] are the CTC head's fp32 logits (any layout through the strides, z_st >= V);
 * enc(b,t,o) = enc[b*e_sb + t*e_st + o] and enc_out(b,j,o) = enc_out[b*o_sb + j*o_st + o] are rows of O fp32 values
 * (e_st, o_st >= O).  Per utterance b, with T_b = t_lens[b] clamped to [0,T]:
 *   lp[t] = z[t,blank] - logsumexp_v z[t,:]   for t < T_b, in fp32 with the row maximum subtracted (the arithmetic, and the bits,
 *           of the CTC loss's per-frame terms);
 *   frame t is SKIPPED exactly when lp[t] > log_threshold (log_threshold = log p of a blank posterior p; 0 skips nothing, and a
 *           row whose lp is NaN is kept);
 *   the kept frames k_0 < k_1 < ... : enc_out(b,j,:) = enc(b,k_j,:) as a bitwise copy, frame_map[b*T + j] = k_j, for
 *           j < new_lens[b] = their number;  frame_map[b*T + j] = -1 for new_lens[b] <= j < T;  rows j >= new_lens[b] of enc_out
 *           are not written.
 *   blank_logp (B,T) fp32 or NULL: lp[t] for t < T_b (entries t >= T_b are not written).
 * Frames t >= T_b of logits and enc are never read (padding may hold anything).  enc_out must not overlap enc.  Two launches, no
 * atomics, no host sync, nothing allocated; row b gives the same bits alone as in any batch, and two calls give the same bits.
 * 16-byte copies when O % 4 == 0 and both buffers' addresses and strides are multiples of 16 bytes, 4-byte copies otherwise.
 * Checked on the host before any launch (RNNT_ERR_INVALID): B in [1,65535], T, O >= 1, V >= 2, 0 <= blank < V, log_threshold <= 0
 * and not NaN, the strides above, non-NULL pointers, no overlap, and a workspace (4-byte aligned) of
 * rnnt_hip_ctc_frame_skip_workspace_bytes(B, T) bytes (0 for B or T < 1): one 32-frame keep word per (utterance, tile).
 * ---------------------------------------------------------------------------------------------- */
size_t rnnt_hip_ctc_frame_skip_workspace_bytes(int32_t B, int32_t T);
int rnnt_hip_ctc_frame_skip(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T, int32_t V,
                            int32_t blank, float log_threshold, const float* enc, int64_t e_sb, int64_t e_st, int32_t O,
                            float* enc_out, int64_t o_sb, int64_t o_st, int32_t* new_lens, int32_t* frame_map, float* blank_logp,
                            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RNNT_HIP_H_ */
