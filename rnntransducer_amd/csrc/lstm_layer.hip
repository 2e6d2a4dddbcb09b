// One recurrent layer call (LSTM / GRU / Elman cells) on the host side: what runs for a shape (LayerPlan, resolved once per call by
// resolve_plan), the workspace (LstmWs / carve_lstm), the forward and the backward sequence of passes, and the shape queries of the
// C ABI, which are one-liners over the plan.  The recurrence kernels sit behind their launch functions in lstm.hip (v1 - v4) and
// lstm5.hip (v5) (lstm_shared.hpp), the products in gemm.hip / gemm_hp.hip; here are only the small layout kernels the layer launches.
#include "lstm_shared.hpp"

#include <string.h>

namespace rnnt {
namespace {

// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------
// db[d][g*H + j] = sum over the direction's (group, row) table of part[(d*rows_per_dir + r)*4H + 4j+g], fixed order
__global__ void db_reduce_kernel(const float* __restrict__ part, int rows_per_dir, int H, int ngate, float* __restrict__ o0,
                                 float* __restrict__ o1, int accumulate, float* __restrict__ p0 = nullptr,
                                 float* __restrict__ p1 = nullptr) {
  const int c = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  if (c >= 4 * H || (c & 3) >= ngate) return;
  const float* src = part + (long)d * rows_per_dir * 4 * H + c;
  float s = 0.f;
  for (int r = 0; r < rows_per_dir; ++r) s += src[(long)r * 4 * H];
  float* o = (d ? o1 : o0) + (c & 3) * H + (c >> 2);
  *o = accumulate ? *o + s : s;
  float* q = d ? p1 : p0;  // optional second destination (LSTM / Elman: grad b_hh == grad b_ih)
  if (q) {
    q += (c & 3) * H + (c >> 2);
    *q = accumulate ? *q + s : s;
  }
}
// out[(d*4H + 4j+g)*I + k] = g < ngate ? w[d][(g*H + j)*I + k] : 0      (4 slots per unit whatever the cell type)
__global__ void permute_w_kernel(const float* __restrict__ w0, const float* __restrict__ w1, int H, int I, int ngate,
                                 float* __restrict__ out) {
  const long per = (long)4 * H * I;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int d = blockIdx.y;
  if (idx >= per) return;
  const int k = (int)(idx % I), r = (int)(idx / I);
  const float* w = d ? w1 : w0;
  out[d * per + idx] = (r & 3) < ngate ? w[(long)((r & 3) * H + (r >> 2)) * I + k] : 0.f;
}
// dX rows of padded frames (t >= lens[b]) under a ragged plan (rnnt_lstm_desc.row_idx): the products skip them (row-gathered dX) or
// read dG rows the recurrence never wrote (dense dX), so they are set to exact zeros here, what the unplanned call leaves there.
// One wavefront per time-major row, grid-stride; rows of valid frames are not touched.
__global__ void __launch_bounds__(256) zero_padded_rows_kernel(float* __restrict__ x, const int* __restrict__ lens, int T, int B, int I) {
  const int lane = threadIdx.x & 63;
  const long nrow = (long)T * B;
  const long nw = ((long)gridDim.x * blockDim.x) >> 6;
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < nrow; r += nw) {
    if ((int)(r / B) < lens[r % B]) continue;
    float* row = x + r * I;
    for (int i = lane; i < I; i += 64) row[i] = 0.f;
  }
}
// inverse for gradients: dw[d][(g*H + j)*I + k] = in[(d*4H + 4j+g)*I + k]
__global__ void unpermute_w_kernel(const float* __restrict__ in, int H, int I, long in_dir_stride, int ngate,
                                   float* __restrict__ o0, float* __restrict__ o1, int accumulate, float* __restrict__ p0 = nullptr,
                                   float* __restrict__ p1 = nullptr) {
  const long per = (long)4 * H * I;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int d = blockIdx.y;
  if (idx >= per) return;
  const int k = (int)(idx % I), r = (int)(idx / I);
  float* o = d ? o1 : o0;
  if ((r & 3) < ngate) {
    const long off = (long)((r & 3) * H + (r >> 2)) * I + k;
    const float v = in[d * in_dir_stride + idx];
    o[off] = accumulate ? o[off] + v : v;
    float* q = d ? p1 : p0;
    if (q) q[off] = accumulate ? q[off] + v : v;
  }
}
// bias folded into the hoisted input projection: b_ih + b_hh per slot; GRU keeps b_hn out (it sits inside r * (.))
__global__ void permute_bias_kernel(const float* __restrict__ bi0, const float* __restrict__ bh0,
                                    const float* __restrict__ bi1, const float* __restrict__ bh1, int H, int ngate,
                                    int gru, float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int d = blockIdx.y;
  if (idx >= 4 * H) return;
  const int g = idx & 3, src = g * H + (idx >> 2);
  float v = 0.f;
  if (g < ngate) {
    const float bi = d ? bi1[src] : bi0[src], bh = d ? bh1[src] : bh0[src];
    v = (gru && g == 2) ? bi : bi + bh;
  }
  out[d * 4 * H + idx] = v;
}

// ------------------------------------------------------------------------------------------------
// the plan of a layer call: everything that is decided from the shape (and the env switches), decided once
// ------------------------------------------------------------------------------------------------
// the hp path pays for the big products only (the operand conversion passes are fixed costs)
inline bool use_hp(int T, int B, int I, int H, int D) {
  if (getenv("RNNT_GEMM_NO_HP")) return false;
  const long M = (long)T * B, N4 = (long)D * 4 * H;
  // gemm_hp.hip addresses an operand's planes with 32-bit buffer offsets: a shape with a plane of 4 GB or more (e.g. bi-H = 1024,
  // B = 64, T = 2048) stays on gemm.hip.  The bound is evaluated with the widest input a layer of this stack can see (I or D*H),
  // so the sizing query (rnnt_hip_lstm_workspace_bytes) and every layer's launch take the same decision.
  const long Iw = I > D * H ? I : (long)D * H;
  const size_t lim = (size_t)1 << 32;
  if (hp_plane_bytes(M, Iw) >= lim || hp_plane_bytes(Iw, M) >= lim || hp_plane_bytes(M, N4) >= lim || hp_plane_bytes(N4, M) >= lim ||
      hp_plane_bytes(H, M) >= lim)
    return false;
  return M >= 1024 && N4 >= 512 && H >= 128 && (getenv("RNNT_GEMM_FORCE_HP") || (M * N4 >= (1l << 22)));
}

enum class Form { NONE, V1, V2, V34, V5 };   // the recurrence kernels of a call, in rising order of preference

struct LayerPlan {
  bool accepted;      // v1 has a decomposition for (B, H, D): the acceptance test of every call, whatever form runs
  Form form;          // NONE: GRU / Elman cells without a grouped plan
  Plan v1;            // valid when accepted (it also sizes the v1 exchange buffers)
  Plan2 p2;           // form V2 (make_plan2) / V34, V5 (make_plan3): forward and backward run on the same one
  bool hp;            // the big products go to gemm_hp.hip
  // rnnt_lstm_desc.row_idx is honoured where EVERY consumer of the stash gathers the valid rows: v5 recurrences (group step bounds)
  // with the half-pair products (row gather in the operand fetch / k-gather in the transposed splits)
  bool takes_row_idx;
  // RNNT_PRECISION_F16 is honoured where the WHOLE layer runs the forms that have a one-product variant: v5 recurrences in both
  // directions of time and the half-pair products.  Everywhere else the layer computes in fp32, bitwise what RNNT_PRECISION_FP32 computes.
  bool takes_f16;
  int recurrence_xcds;   // XCDs the recurrence sits on: the placement rule shared by the backward (which XCDs its grouped products
                         // avoid) and the caller's decision to overlap at all
  int cus;
  size_t nflags, hx_bytes;   // step flags / exchange buffers: the maxima over every form the shape could run
};

// sizing and shape queries work without a device: assume the MI355X
inline int cus_or_mi355x() {
  const int cus = device_cus();
  return cus > 0 ? cus : 256;
}

// Order of preference V5 > V3/V4 > V2 > V1.  The environment is read on every call.
LayerPlan resolve_plan(int T, int B, int I, int H, int D, int cell, int cus) {
  LayerPlan lp = {};
  lp.form = Form::NONE;
  lp.recurrence_xcds = 8;
  lp.cus = cus;
  if (T < 1 || B < 1 || I < 1 || H < 4 || D < 1 || D > 2) return lp;
  lp.accepted = make_plan(B, H, D, cus, &lp.v1);
  Plan2 v2, v34;
  const bool has2 = make_plan2(B, H, D, cus, &v2), has34 = make_plan3(B, H, D, cus, &v34);
  if (has34) {
    lp.p2 = v34;
    lp.form = lstm5_supported(T, B, H, D, cell) ? Form::V5 : Form::V34;
  } else if (has2) {
    lp.p2 = v2;
    lp.form = Form::V2;
  } else if (lp.accepted && cell == RNNT_CELL_LSTM) {
    lp.form = Form::V1;
  }
  lp.hp = use_hp(T, B, I, H, D);
  lp.takes_f16 = lp.hp && lp.form == Form::V5;
  lp.takes_row_idx = lp.takes_f16 && I >= 32 && T > 1;
  if (lp.form == Form::V5) {
    const int NG = D * lp.p2.G;
    lp.recurrence_xcds = (NG <= 4 && lp.p2.NC <= 32 && !getenv("RNNT_LSTM_NO_XCD_STRIDE")) ? NG : 8;   // launch_persistent2: stride 8, group g on XCD g
  }
  // one workspace serves every form of the shape (the env switches move a call between them)
  auto widen = [&](size_t nflags, size_t hx_bytes) {
    if (nflags > lp.nflags) lp.nflags = nflags;
    if (hx_bytes > lp.hx_bytes) lp.hx_bytes = hx_bytes;
  };
  if (lp.accepted) widen((size_t)D * lp.v1.NC, (size_t)2 * D * H * lp.v1.Bp * 4 * 4);  // v1, sized for the backward exchange (B x 4H), fwd uses a quarter
  if (has2) widen((size_t)D * v2.G * v2.NC, (size_t)2 * D * v2.G * 4 * v2.BQ * 4 * v2.Kp * 4);
  if (has34) {
    widen((size_t)D * v34.G * v34.NC, (size_t)2 * D * v34.G * 4 * v34.BQ * v34.Kp * 6);           // v3: three bf16 planes of h
    widen((size_t)D * v34.G * v34.NC, (size_t)2 * D * v34.G * v34.NC * 4 * v34.BQ * v34.Kp * 4);  // v4: per-producer partial dh, fp32
  }
  return lp;
}

struct LstmWs {
  unsigned* flags;  // [16 words: status at word 0] [D*NC step flags], zeroed per launch
  size_t sync_bytes, nflags;
  float* hx;
  size_t hx_bytes;
  float* wp;   // (D*4H, I) permuted input weights; reused as dW_ih' in backward
  float* bp;   // (D*4H)
  float* dwhh; // (D*4H, H) scratch for dW_hh'
  unsigned long long* dbg;  // 256 workgroups x 8 phase counters (diagnostics)
  float* dbp;   // v4 backward: per-(group, row) time sums of dG (input side | hidden side), (2, D*G*NBR, 4H)
  size_t dbp_half;  // floats per side
  void* scratch;  // split-K slabs of the weight-gradient GEMMs / column-sum partials
  size_t scratch_bytes;
  // half-pair operand planes of the big products (gemm_hp.hip); null when the shape stays on gemm.hip
  bool hp;
  char* hp_x;    // fwd: x (T*B, I)            bwd: x^T (I, T*B)
  char* hp_w;    // fwd: W_ih' (D*4H, I)       bwd: W_ih'^T (I, D*4H)
  char* hp_dg;   // bwd: dG (T*B, D*4H)
  char* hp_dgt;  // bwd: dG^T (D*4H, T*B)
  char* hp_yt;   // bwd: time-shifted h^T per direction (D, H, T*B)
  // per-row maxima of those operands (the scales of their planes), one table each, neighbours in this order (M = T*B, N4 = D*4H words):
  uint32_t* amax_x;         // [M]   fwd: rows of x
  uint32_t* amax_w;         // [N4]  fwd: rows of W_ih'
  uint32_t* amax_dg_rows;   // [M]   bwd: rows of dG
  uint32_t* amax_dg_cols;   // [N4]  bwd: columns of dG (= rows of dG^T)
  uint32_t* amax_wt;        // [I]   bwd: rows of W_ih'^T
  uint32_t* amax_xt;        // [I]   bwd: rows of x^T
  uint32_t* amax_yt;        // [D*H] bwd: rows of h^T
  uint32_t* amax_dgh_cols;  // [N4]  bwd: columns of the hidden-side dG (GRU), left by the v5 recurrence
  size_t total;
};

LstmWs carve_lstm(void* ws, int T, int B, int I, int H, int D, const LayerPlan& lp) {
  LstmWs w;
  char* p = reinterpret_cast<char*>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += align_up(bytes, 256); return q; };
  w.nflags = lp.nflags;
  w.sync_bytes = align_up((2 * w.nflags + 16) * 4, 16);  // status block | step flags | XCC table
  w.flags = reinterpret_cast<unsigned*>(take(w.sync_bytes));
  w.hx_bytes = lp.hx_bytes;
  w.hx = reinterpret_cast<float*>(take(w.hx_bytes));
  w.wp = reinterpret_cast<float*>(take((size_t)D * 4 * H * I * 4));
  w.bp = reinterpret_cast<float*>(take((size_t)D * 4 * H * 4));
  w.dwhh = reinterpret_cast<float*>(take((size_t)D * 4 * H * H * 4));
  w.dbg = reinterpret_cast<unsigned long long*>(take(512 * 8 * 8));
  w.dbp_half = (size_t)D * (B + 64) * 4 * H;  // D*G*NBR <= D*(B + 4*G) rows of 4H
  w.dbp = reinterpret_cast<float*>(take(2 * w.dbp_half * 4));
  const int64_t M = (int64_t)T * B, N4 = (int64_t)D * 4 * H;
  size_t sc = rnnt_hip_gemm_workspace_bytes(N4, I, M);
  const size_t s2 = rnnt_hip_gemm_workspace_bytes(4 * H, H, M > B ? M - B : 1);
  const size_t s3 = rnnt_hip_colsum_workspace_bytes(M, N4);
  if (s2 > sc) sc = s2;
  if (s3 > sc) sc = s3;
  w.hp = lp.hp;
  if (w.hp) {
    const size_t h1 = hp_gemm_workspace_bytes(N4, I, M), h2 = hp_gemm_workspace_bytes(4 * H, H, M);
    if (h1 > sc) sc = h1;
    if (h2 > sc) sc = h2;
    const int64_t mn[3] = {N4 * I, (int64_t)4 * H * H, (int64_t)4 * H * H};   // the grouped launch keeps all slabs at once
    const size_t h3 = HPQ_HEADER_BYTES + hp_gemm_grouped_workspace_bytes(mn, 1 + D);   // queue counters in front of the slabs
    if (h3 > sc) sc = h3;
  }
  w.scratch_bytes = sc;
  w.scratch = take(sc);
  w.hp_x = w.hp_w = w.hp_dg = w.hp_dgt = w.hp_yt = nullptr;
  w.amax_x = w.amax_w = w.amax_dg_rows = w.amax_dg_cols = w.amax_wt = w.amax_xt = w.amax_yt = w.amax_dgh_cols = nullptr;
  if (w.hp) {
    uint32_t* hp_amax = reinterpret_cast<uint32_t*>(take((size_t)(2 * M + 3 * N4 + 2 * I + (int64_t)D * H) * 4));
    if (hp_amax) {   // (the backward's one fill relies on this order: see lstm_bwd_impl)
      w.amax_x = hp_amax;
      w.amax_w = hp_amax + M;
      w.amax_dg_rows = hp_amax + M + N4;
      w.amax_dg_cols = hp_amax + 2 * M + N4;
      w.amax_wt = hp_amax + 2 * M + 2 * N4;
      w.amax_xt = hp_amax + 2 * M + 2 * N4 + I;
      w.amax_yt = hp_amax + 2 * M + 2 * N4 + 2 * I;
      w.amax_dgh_cols = hp_amax + 2 * M + 2 * N4 + 2 * I + (int64_t)D * H;
    }
    w.hp_x = take(hp_plane_bytes(M, I) > hp_plane_bytes(I, M) ? hp_plane_bytes(M, I) : hp_plane_bytes(I, M));
    w.hp_w = take(hp_plane_bytes(N4, I) > hp_plane_bytes(I, N4) ? hp_plane_bytes(N4, I) : hp_plane_bytes(I, N4));
    w.hp_dg = take(hp_plane_bytes(M, N4));
    w.hp_dgt = take(hp_plane_bytes(N4, M));
    w.hp_yt = take((size_t)D * hp_plane_bytes(H, M));
  }
  w.total = off;
  return w;
}

// validates the descriptor and hands back the plan of the call with the workspace carved for it
int check_desc(const rnnt_lstm_desc* d, LayerPlan* lp, LstmWs* w) {
  RNNT_CHECK_ARG(d != nullptr, "lstm: null descriptor");
  RNNT_CHECK_ARG(d->T >= 1 && d->I >= 1, "lstm: T and I must be positive (T=%d I=%d)", d->T, d->I);
  const int cus = device_cus();
  RNNT_CHECK_ARG(cus > 0, "lstm: no HIP device");
  *lp = resolve_plan(d->T, d->B, d->I, d->H, d->D, d->cell, cus);
  if (!lp->accepted) {
    set_error("lstm: unsupported configuration B=%d H=%d D=%d (need H%%4==0, 1<=B<=64, D in {1,2}, slice must fit %d CUs)",
              d->B, d->H, d->D, cus);
    return RNNT_ERR_UNSUPPORTED;
  }
  RNNT_CHECK_ARG(d->cell >= RNNT_CELL_LSTM && d->cell <= RNNT_CELL_RNN_RELU, "lstm: unknown cell type %d", d->cell);
  RNNT_CHECK_ARG(d->lens && d->x && d->y && d->gates && (d->cst || d->cell != RNNT_CELL_LSTM), "lstm: null tensor");
  for (int k = 0; k < d->D; ++k)
    RNNT_CHECK_ARG(d->w_ih[k] && d->w_hh[k] && d->b_ih[k] && d->b_hh[k], "lstm: null weight (direction %d)", k);
  RNNT_CHECK_ARG(d->dropout_p >= 0.f && d->dropout_p < 1.f, "lstm: dropout_p must be in [0,1)");
  RNNT_CHECK_ARG(d->dropout_p == 0.f || d->y_drop, "lstm: dropout_p > 0 needs y_drop");
  RNNT_CHECK_ARG(d->x_abs_bound >= 0.f && d->x_abs_bound < 1e30f, "lstm: x_abs_bound must be 0 (measure) or a finite positive bound");
  RNNT_CHECK_ARG(!d->row_idx || (d->n_rows >= 1 && d->n_rows <= (int64_t)d->T * d->B), "lstm: row_idx needs 1 <= n_rows <= T*B (got %d)", d->n_rows);
  *w = carve_lstm(d->workspace, d->T, d->B, d->I, d->H, d->D, *lp);
  RNNT_CHECK_ARG(d->workspace && d->workspace_bytes >= w->total, "lstm: workspace too small (%zu < %zu)",
                 d->workspace_bytes, w->total);
  RNNT_CHECK_ARG((reinterpret_cast<uintptr_t>(d->gates) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->y) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(d->cst) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->aux) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(d->workspace) & 255) == 0,
                 "lstm: gates/y/cst must be 16-byte aligned, workspace 256-byte aligned");
  return RNNT_OK;
}

// the second direction's entry of a per-direction pair, the first one's again in a unidirectional layer (the kernels take both)
template <class P>
P second(P const (&x)[2], int D) { return D > 1 ? x[1] : x[0]; }

inline int gate_count(int cell) { return cell == RNNT_CELL_LSTM ? 4 : (cell == RNNT_CELL_GRU ? 3 : 1); }

inline bool x_is_plain(const rnnt_lstm_desc* d) { return d->x_sb == d->I && d->x_st == (int64_t)d->B * d->I; }

// valid frames only (rnnt_lstm_desc.row_idx): the same answer in the forward and the backward call of a layer
inline bool ragged_call(const rnnt_lstm_desc* d, const LayerPlan& lp) {
  return d->row_idx && d->n_rows > 0 && d->n_rows < (int64_t)d->T * d->B && x_is_plain(d) && lp.takes_row_idx;
}

void fill_kernel_args(const rnnt_lstm_desc* d, const LayerPlan& lp, const LstmWs& w, LstmK* k) {
  k->T = d->T; k->B = d->B; k->H = d->H; k->D = d->D;
  k->Bp = lp.v1.Bp; k->LDW = lp.v1.LDW;
  if (lp.form == Form::V2 || lp.form == Form::V34 || lp.form == Form::V5) {
    k->NC = lp.p2.NC; k->Hs = lp.p2.HS; k->G = lp.p2.G; k->Bg = lp.p2.Bg; k->Kp = lp.p2.Kp;
  } else {
    k->NC = lp.v1.NC; k->Hs = lp.v1.Hs; k->G = 1; k->Bg = d->B; k->Kp = d->H;
  }
  k->lens = d->lens; k->gates = d->gates; k->cst = d->cst; k->y = d->y;
  k->ydrop = d->dropout_p > 0.f ? d->y_drop : nullptr;
  k->keep_scale = d->dropout_p > 0.f ? 1.f / (1.f - d->dropout_p) : 1.f;
  k->drop_thresh = (unsigned)((double)d->dropout_p * 4294967296.0);
  k->seed = d->dropout_seed;
  k->w_hh[0] = d->w_hh[0]; k->w_hh[1] = second(d->w_hh, d->D);
  // status word: the caller's sticky device word when given (never reset by the library: a raised status makes every later
  // launch bail out at its first wait and stays visible until the caller reads it), else word 0 of the workspace (reset per launch)
  k->hx = w.hx; k->status = d->status ? d->status : w.flags; k->flags = w.flags + 16;
  k->dy = nullptr;
  k->cell = d->cell;
  k->b_hh[0] = d->b_hh[0]; k->b_hh[1] = second(d->b_hh, d->D);
  k->aux = d->aux;
  k->NGL = d->D;
  k->dbp = w.dbp; k->dbhp = w.dbp + w.dbp_half;
  k->dbg = getenv("RNNT_LSTM_DBG") ? w.dbg : nullptr;
  k->xcc = w.flags + 16 + w.nflags;
  k->allow_local = getenv("RNNT_LSTM_NO_XCD_LOCAL") ? 0 : 1;
  k->hw_math = getenv("RNNT_LSTM_EXACT_MATH") ? 0 : 1;
  k->pause = 0;
  k->gbound = 0;
  k->colmax = k->colmax_h = nullptr;
  k->rowmax = nullptr;
}

// the one place a recurrence is launched: k carries the plan's decomposition (fill_kernel_args)
int launch_recurrence(const LayerPlan& lp, const LstmK& k, bool backward, bool f16, hipStream_t s) {
  switch (lp.form) {
    case Form::V5:  // tagged-payload exchange, f16 matrix cores (lstm5.hip)
      return backward ? lstm5_bwd_launch(k, lp.p2, k.cell, s, f16) : lstm5_fwd_launch(k, lp.p2, k.cell, s, f16);
    case Form::V34:
      return backward ? lstm4_bwd_launch(k, lp.p2, k.cell, s) : lstm3_fwd_launch(k, lp.p2, k.cell, s);
    case Form::V2:
      return backward ? lstm2_bwd_launch(k, lp.p2, k.cell, s) : lstm2_fwd_launch(k, lp.p2, k.cell, s);
    case Form::V1:
      return backward ? lstm1_bwd_launch(k, lp.v1, s) : lstm1_fwd_launch(k, lp.v1, s);
    case Form::NONE:
      break;
  }
  if (backward) set_error("rnn: GRU / Elman cells need the grouped decomposition; B=%d H=%d does not fit", k.B, k.H);
  else set_error("rnn: GRU / Elman cells need the grouped decomposition (B/G <= 16 rows per group); B=%d H=%d does not fit", k.B, k.H);
  return RNNT_ERR_UNSUPPORTED;
}

// sync block and exchange buffers are neighbours in the workspace (carve_lstm): one fill
int reset_exchange(const LstmWs& w, hipStream_t s) {
  RNNT_CHECK_HIP(hipMemsetAsync(w.flags, 0, (size_t)(reinterpret_cast<char*>(w.hx) - reinterpret_cast<char*>(w.flags)) + w.hx_bytes, s));
  return RNNT_OK;
}

// gate-adjacent copy of W_ih (both directions stacked) in w.wp
int permute_w_ih(const rnnt_lstm_desc* d, const LstmWs& w, hipStream_t s) {
  const long per = (long)4 * d->H * d->I;
  hipLaunchKernelGGL(permute_w_kernel, dim3((unsigned)ceil_div(per, 256), d->D), dim3(256), 0, s, d->w_ih[0], second(d->w_ih, d->D),
                     d->H, d->I, gate_count(d->cell), w.wp);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// gate-adjacent (D*4H, I) gradient -> the torch layout of each direction's tensor (and of its optional twin)
int unpermute(const float* in, int H, int I, int D, int ngate, float* const (&out)[2], int acc, hipStream_t s, float* twin0 = nullptr,
              float* twin1 = nullptr) {
  const long per = (long)4 * H * I;
  hipLaunchKernelGGL(unpermute_w_kernel, dim3((unsigned)ceil_div(per, 256), D), dim3(256), 0, s, in, H, I, per, ngate, out[0],
                     second(out, D), acc, twin0, twin1);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

// The shape queries: sizing-style calls that work without a device (256 CUs assumed).

extern "C" int32_t rnnt_hip_lstm_max_batch(int32_t H, int32_t D, int32_t cell) {
  // largest per-call batch the persistent kernels take for this shape (callers split bigger batches along B:
  // sequences are independent, weight gradients add)
  const int cus = cus_or_mi355x();
  for (int B = 64; B >= 1; --B)
    if (resolve_plan(1, B, 1, H, D, cell, cus).form != Form::NONE) return B;
  return 0;
}

extern "C" int32_t rnnt_hip_lstm_takes_row_idx(int32_t T, int32_t B, int32_t I, int32_t H, int32_t D, int32_t cell) {
  return resolve_plan(T, B, I, H, D, cell, cus_or_mi355x()).takes_row_idx ? 1 : 0;
}

extern "C" int32_t rnnt_hip_lstm_takes_f16(int32_t T, int32_t B, int32_t I, int32_t H, int32_t D, int32_t cell) {
  return resolve_plan(T, B, I, H, D, cell, cus_or_mi355x()).takes_f16 ? 1 : 0;
}

extern "C" int32_t rnnt_hip_lstm_free_xcds(int32_t T, int32_t B, int32_t H, int32_t D, int32_t cell) {
  return 8 - resolve_plan(T, B, 1, H, D, cell, cus_or_mi355x()).recurrence_xcds;
}

extern "C" size_t rnnt_hip_lstm_workspace_bytes(int32_t T, int32_t B, int32_t I, int32_t H, int32_t D) {
  const LayerPlan lp = resolve_plan(T, B, I, H, D, RNNT_CELL_LSTM, cus_or_mi355x());   // (the sizes do not depend on the cell)
  return lp.accepted ? carve_lstm(nullptr, T, B, I, H, D, lp).total : 0;
}

static int lstm_fwd_impl(const rnnt_lstm_desc* d, uint32_t precision, void* stream) {
  LayerPlan lp;
  LstmWs w;
  if (int rc = check_desc(d, &lp, &w)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int H = d->H, D = d->D, I = d->I;
  const int64_t M = (int64_t)d->T * d->B, N4 = (int64_t)D * 4 * H;
  // one-product forms (RNNT_PRECISION_F16) where the whole layer has them, fp32 otherwise
  const bool f16 = precision == RNNT_PRECISION_F16 && lp.takes_f16;
  const unsigned hpf = f16 ? RNNT_GEMM_HP_F16 : 0u;
  const bool ragged = ragged_call(d, lp);
  const bool hp_proj = w.hp && x_is_plain(d) && I >= 32;   // the input projection on the f16 matrix cores (half-pair operands, gemm_hp.hip)

  // 1. gate-adjacent copy of W_ih (both directions stacked) and of b_ih + b_hh
  if (int rc = permute_w_ih(d, w, s)) return rc;
  hipLaunchKernelGGL(permute_bias_kernel, dim3((unsigned)ceil_div(4 * H, 256), D), dim3(256), 0, s, d->b_ih[0], d->b_hh[0],
                     second(d->b_ih, D), second(d->b_hh, D), H, gate_count(d->cell), d->cell == RNNT_CELL_GRU ? 1 : 0, w.bp);
  RNNT_CHECK_LAUNCH();
  // 2. hoisted input projection for all timesteps: gates[(t,b)][d*4H + 4j+g] = x(t,b,:) . W_ih'[.] + bias'
  if (hp_proj) {
    const int64_t Mv = ragged ? d->n_rows : M;             // rows the product runs over
    const int* ridx = ragged ? d->row_idx : nullptr;
    if (int rc = hp_split(d->x, Mv, I, I, w.amax_x, w.hp_x, s, ridx)) return rc;   // planes / maxima of the valid rows, in place
    if (int rc = hp_split(w.wp, N4, I, I, w.amax_w, w.hp_w, s)) return rc;
    if (int rc = hp_gemm(w.hp_x, w.amax_x, w.hp_w, w.amax_w, Mv, N4, I, d->gates, 1, N4, 0, w.bp, hpf, nullptr, 0, s, ridx, M, ridx)) return rc;
  } else {
    rnnt_gemm_desc g = {};
    g.M = M; g.N = N4; g.K = I;
    g.A = d->x; g.a_div = d->B; g.a_so = d->x_st; g.a_si = d->x_sb; g.a_sk = 1; g.a_mc = 0;
    g.B = w.wp; g.b_sn = I; g.b_sk = 1;
    g.C = d->gates; g.c_div = 1; g.c_so = g.N; g.c_si = 0;
    g.bias = w.bp;
    if (int rc = rnnt_hip_gemm_f32(&g, s)) return rc;
  }
  // 3. the recurrence
  if (int rc = reset_exchange(w, s)) return rc;
  LstmK k;
  fill_kernel_args(d, lp, w, &k);
  k.gbound = ragged ? 1 : 0;
  return launch_recurrence(lp, k, false, f16, s);
}

extern "C" int rnnt_hip_lstm_fwd(const rnnt_lstm_desc* d, void* stream) { return lstm_fwd_impl(d, RNNT_PRECISION_FP32, stream); }

extern "C" int rnnt_hip_lstm_fwd_ex(const rnnt_lstm_desc* d, uint32_t precision, void* stream) {
  RNNT_CHECK_ARG(precision == RNNT_PRECISION_FP32 || precision == RNNT_PRECISION_F16, "lstm_fwd_ex: precision must be 0 (fp32) or 1 (f16), got %u",
                 precision);
  return lstm_fwd_impl(d, precision, stream);
}

static int lstm_bwd_impl(const rnnt_lstm_bwd_desc* bd, uint32_t precision, void* stream) {
  RNNT_CHECK_ARG(bd != nullptr, "lstm_bwd: null descriptor");
  const rnnt_lstm_desc* d = &bd->f;
  LayerPlan lp;
  LstmWs w;
  if (int rc = check_desc(d, &lp, &w)) return rc;
  RNNT_CHECK_ARG(bd->dy, "lstm_bwd: null dy");
  const int T = d->T, B = d->B, H = d->H, D = d->D, I = d->I;
  const bool gru = d->cell == RNNT_CELL_GRU;
  const int ngate = gate_count(d->cell);
  RNNT_CHECK_ARG(!gru || d->aux, "lstm_bwd: GRU needs the aux buffer (T,B,D*4H)");
  for (int k = 0; k < D; ++k) RNNT_CHECK_ARG(!gru || bd->db_hh[k], "lstm_bwd: GRU needs db_hh");
  const int acc = bd->accumulate ? 1 : 0;       // += into dw_ih / dw_hh / db / db_hh (flat-gradient views) instead of =
  // LSTM / Elman: grad b_hh == grad b_ih; when the caller also hands db_hh it receives the same values (second destination)
  float* twin0 = gru ? nullptr : bd->db_hh[0];
  float* twin1 = gru ? nullptr : second(bd->db_hh, D);
  if (twin0 == bd->db[0]) twin0 = nullptr;
  if (twin1 == second(bd->db, D)) twin1 = nullptr;
  const float* ghid = gru ? d->aux : d->gates;  // hidden-side gate gradients (== input side except for GRU's n gate)
  RNNT_CHECK_ARG(x_is_plain(d), "lstm_bwd: x must be time-major contiguous (T,B,I)");
  for (int k = 0; k < D; ++k) RNNT_CHECK_ARG(bd->dw_ih[k] && bd->dw_hh[k] && bd->db[k], "lstm_bwd: null gradient output");
  hipStream_t s = (hipStream_t)stream;
  RNNT_CHECK_ARG(bd->phase >= RNNT_LSTM_BWD_ALL && bd->phase <= RNNT_LSTM_BWD_WEIGHTS, "lstm_bwd: phase must be 0, 1 or 2");
  // phase 1 = steps 1-2 (the chain autograd waits for), phase 2 = steps 3-5 (weight / bias gradients: any stream ordered after phase 1)
  const bool do_recur = bd->phase != RNNT_LSTM_BWD_WEIGHTS, do_weights = bd->phase != RNNT_LSTM_BWD_RECUR;

  // What this call runs, from the plan and the descriptor (the same in both phases of a two-phase backward, and — f16, ragged — the
  // same decision as the forward call of the layer)
  const bool f16 = precision == RNNT_PRECISION_F16 && lp.takes_f16;
  const unsigned hpf = f16 ? RNNT_GEMM_HP_F16 : 0u;
  const bool ragged = ragged_call(d, lp);
  const int* ridx = ragged ? d->row_idx : nullptr;
  const int64_t M = (int64_t)T * B, N4 = (int64_t)D * 4 * H;
  const int64_t Mv = ragged ? d->n_rows : M;   // rows (row-major operands: gathered by the GEMM) / contraction length (transposed planes: packed)
  const bool hp_in = w.hp && I >= 128;   // products with I as an output / contraction width on the f16 matrix cores
  // (a narrow input — the 80 mel bins of layer 0 — still goes to the half-pair kernel for dW_ih: one 256-wide tile column, split over K)
  const bool hp_dwih = hp_in || (w.hp && I >= 32 && !getenv("RNNT_GEMM_HP_NO_NARROW"));
  // the v3 / v4 / v5 backward recurrences sum their own cells of dG over time: db is reduced from db_rows partial rows per direction
  const bool fused_db = lp.form == Form::V34 || lp.form == Form::V5;
  const int db_rows = lp.p2.G * 4 * lp.p2.BQ;
  // v5 with the half-pair products: the recurrence also leaves the column maxima of dG (the scales of the half-pair dG^T planes): no
  // extra pass.  LSTM / Elman layers that hand on dx: it also leaves the row maxima, and ONE pass over dG then writes both
  // orientations of its planes (hp_split_both) instead of a row-major pass that measures each row first plus a transposed pass
  const bool v5_maxima = lp.form == Form::V5 && w.hp;
  const bool both = v5_maxima && !gru && hp_in && bd->dx && !getenv("RNNT_GEMM_HP_NO_FUSED_SPLIT");
  // the weight-gradient products of THIS layer may run beside the recurrence of the next one (same shape): that one sits on
  // XCDs 0 .. D*G-1 (launch_persistent2's stride-8 placement), the products keep to the others
  // (only on a device that exposes all 8 XCDs — the 256-CU SPX mode the placement rule was measured on; a partitioned device
  //  runs the products on every XCD it has, and gemm_hp.hip's check kernel raises the status word if a launch left units undone)
  const unsigned xcd_skip =
      (lp.form == Form::V5 && bd->beside_recurrence && lp.recurrence_xcds <= 4 && lp.cus == 256) ? (1u << lp.recurrence_xcds) - 1u : 0u;
  // All three weight-gradient products on the half-pair path (LSTM / Elman) beside a recurrence: their operand planes first, then
  // ONE queue-driven launch (gemm_hp.hip) that stays off the recurrence's XCDs.
  // (alone on the device three launches are faster: 1.13 vs 1.29 ms for a c2 layer, tools/gemm_hpq_bench.py — the queue form is for
  // the overlapped case, where it keeps off the recurrence's XCDs)
  const bool grouped = hp_in && T > 1 && !gru && (xcd_skip != 0u || getenv("RNNT_GEMM_HP_GROUP")) && !getenv("RNNT_GEMM_HP_NO_GROUP");
  int rc = RNNT_OK;

  // 1. reverse-time recurrence: gates (activated) -> dG in place
  if (do_recur)
    if ((rc = reset_exchange(w, s))) return rc;
  LstmK k;
  fill_kernel_args(d, lp, w, &k);
  k.dy = bd->dy;
  k.gbound = ragged ? 1 : 0;
  if (v5_maxima) {
    k.colmax = w.amax_dg_cols;
    k.colmax_h = w.amax_dgh_cols;
    if (both) k.rowmax = w.amax_dg_rows;
    // one fill from the first table the recurrence accumulates into to the end of the last.  The neighbours it covers, in carve_lstm's
    // order: [dG rows |] dG columns | W_ih'^T rows | x^T rows | h^T rows | hidden-side dG columns (those in between are written later)
    unsigned* first = both ? k.rowmax : k.colmax;
    if (do_recur) RNNT_CHECK_HIP(hipMemsetAsync(first, 0, (size_t)(w.amax_dgh_cols + N4 - first) * 4, s));
  }
  if (do_recur || lp.form == Form::NONE)   // (a cell without a plan fails in either phase)
    if ((rc = launch_recurrence(lp, k, true, f16, s))) return rc;

  if (w.hp) {  // half-pair planes of dG in both orientations (gemm_hp.hip is NT-only: transposed operands are materialised)
    if (do_recur && hp_in && bd->dx) {
      if (both) rc = hp_split_both(d->gates, Mv, N4, N4, w.amax_dg_rows, w.amax_dg_cols, w.hp_dg, w.hp_dgt, s, ridx);
      else rc = hp_split(d->gates, Mv, N4, N4, w.amax_dg_rows, w.hp_dg, s, ridx);
      if (rc) return rc;
    }
    if (do_weights && !v5_maxima)
      if ((rc = hp_colmax(d->gates, M, N4, N4, w.amax_dg_cols, s))) return rc;
    if (do_weights && !both)
      if ((rc = hp_split_t(d->gates, N4, Mv, N4, M, 0, w.amax_dg_cols, w.hp_dgt, s, ridx))) return rc;
  }
  // 2. dX = dG . W_ih'   (needs the permuted weights: rebuild them, the forward copy may have been overwritten)
  if (do_recur && bd->dx) {
    if ((rc = permute_w_ih(d, w, s))) return rc;
    if (hp_in) {
      if ((rc = hp_colmax(w.wp, N4, I, I, w.amax_wt, s))) return rc;
      if ((rc = hp_split_t(w.wp, I, N4, I, N4, 0, w.amax_wt, w.hp_w, s))) return rc;   // W_ih'^T: (I, contraction N4)
      if ((rc = hp_gemm(w.hp_dg, w.amax_dg_rows, w.hp_w, w.amax_wt, Mv, I, N4, bd->dx, 1, I, 0, nullptr, hpf, nullptr, 0, s, ridx, M, ridx))) return rc;
    } else {
      rnnt_gemm_desc g = {};
      g.M = M; g.N = I; g.K = N4;
      g.A = d->gates; g.a_div = 1; g.a_so = N4; g.a_si = 0; g.a_sk = 1; g.a_mc = 0;
      g.B = w.wp; g.b_sn = 1; g.b_sk = I;
      g.C = bd->dx; g.c_div = 1; g.c_so = I; g.c_si = 0;
      if ((rc = rnnt_hip_gemm_f32(&g, s))) return rc;
    }
    if (ragged) {
      hipLaunchKernelGGL(zero_padded_rows_kernel, dim3((unsigned)(ceil_div(M, 4) < 2048 ? ceil_div(M, 4) : 2048)), dim3(256), 0, s, bd->dx, d->lens, T, B, I);
      RNNT_CHECK_LAUNCH();
    }
  }
  if (!do_weights) return RNNT_OK;
  // 3. dW_ih' = dG^T . X  (both directions at once), un-permute rows into torch layout
  if (hp_dwih) {
    if (d->x_abs_bound > 0.f) {   // bounded input (the dropped output of the layer below): its bound is the scale, no pass over x
      uint32_t bits;
      memcpy(&bits, &d->x_abs_bound, 4);
      RNNT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)w.amax_xt, (int)bits, (size_t)I, s));
    } else if ((rc = hp_colmax(d->x, M, I, I, w.amax_xt, s))) return rc;
    if ((rc = hp_split_t(d->x, I, Mv, I, M, 0, w.amax_xt, w.hp_x, s, ridx))) return rc;     // X^T: (I, contraction over the (valid) frames)
    if (!grouped)
      if ((rc = hp_gemm(w.hp_dgt, w.amax_dg_cols, w.hp_x, w.amax_xt, N4, I, Mv, w.wp, 1, I, 0, nullptr, hpf, w.scratch, w.scratch_bytes, s))) return rc;
  } else {
    rnnt_gemm_desc g = {};
    g.M = N4; g.N = I; g.K = M;
    g.A = d->gates; g.a_mc = 1; g.a_sk = N4; g.a_div = 1;
    g.B = d->x; g.b_sn = 1; g.b_sk = I;
    g.C = w.wp; g.c_div = 1; g.c_so = I; g.c_si = 0;
    g.workspace = w.scratch; g.workspace_bytes = w.scratch_bytes;
    if ((rc = rnnt_hip_gemm_f32(&g, s))) return rc;
  }
  if (!grouped)   // (the grouped launch of step 4 computes dW_ih' too)
    if ((rc = unpermute(w.wp, H, I, D, ngate, bd->dw_ih, acc, s))) return rc;
  // 4. dW_hh'[d] = sum_t dG[t]^T . h_prev(t): time-shifted views of dG and y (padded frames are zero in both)
  if (w.hp && T > 1) {
    if (d->cell != RNNT_CELL_RNN_RELU) {   // |h| < 1 for LSTM / GRU / tanh cells: the planes of h^T take 1.0 as their scale
      RNNT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)w.amax_yt, 0x3f800000, (size_t)D * H, s));
    } else if ((rc = hp_colmax(d->y, M, (int64_t)D * H, (int64_t)D * H, w.amax_yt, s))) return rc;
    uint32_t* a_dgh = w.amax_dg_cols;   // column maxima of the gate gradients the hidden-side products read
    if (gru) {  // hidden-side gate gradients differ from the input-side ones in the n gate: their own transposed planes
      if (v5_maxima) a_dgh = w.amax_dgh_cols;   // left there by the v5 recurrence
      else if ((rc = hp_colmax(ghid, M, N4, N4, a_dgh, s))) return rc;
      if ((rc = hp_split_t(ghid, N4, Mv, N4, M, 0, a_dgh, w.hp_dgt, s, ridx))) return rc;
    }
    HpProblem pr[HP_GROUP_MAX];
    int npr = 0;
    if (grouped) pr[npr++] = HpProblem{w.hp_dgt, w.amax_dg_cols, w.hp_x, w.amax_xt, N4, I, Mv, w.wp, I, hpf};
    for (int dir = 0; dir < D; ++dir) {
      // h_prev of frame t is y[t-1] (forward direction) / y[t+1] (reverse): plane row j, index k = y[k -/+ B][dir*H + j], zero outside
      char* yt = w.hp_yt + (size_t)dir * hp_plane_bytes(H, M);
      uint32_t* a_y = w.amax_yt + (int64_t)dir * H;
      float* dwhh = w.dwhh + (int64_t)dir * 4 * H * H;
      // (ragged batches: frame (t, b) of the packed contraction takes y of padded row (t -/+ 1, b), which is a valid frame or holds 0)
      if ((rc = hp_split_t(d->y + (int64_t)dir * H, H, Mv, (int64_t)D * H, M, dir == 0 ? -B : B, a_y, yt, s, ridx))) return rc;
      const char* ag = w.hp_dgt + (size_t)dir * 4 * H * (size_t)ceil_div(Mv, 32) * 128;
      if (grouped) {
        pr[npr++] = HpProblem{ag, a_dgh + (int64_t)dir * 4 * H, yt, a_y, 4 * H, H, Mv, dwhh, H, hpf};
        continue;
      }
      if ((rc = hp_gemm(ag, a_dgh + (int64_t)dir * 4 * H, yt, a_y, 4 * H, H, Mv, dwhh, 1, H, 0, nullptr, hpf, w.scratch, w.scratch_bytes, s)))
        return rc;
    }
    if (grouped) {
      if ((rc = hp_gemm_grouped(pr, npr, xcd_skip, reinterpret_cast<unsigned*>(w.scratch), (char*)w.scratch + HPQ_HEADER_BYTES,
                                w.scratch_bytes - HPQ_HEADER_BYTES, s, k.status)))
        return rc;
      if ((rc = unpermute(w.wp, H, I, D, ngate, bd->dw_ih, acc, s))) return rc;
    }
  } else
  for (int dir = 0; dir < D; ++dir) {
    rnnt_gemm_desc g = {};
    g.M = 4 * H; g.N = H; g.K = (int64_t)(T - 1) * B;
    const int64_t shift_g = dir == 0 ? (int64_t)B * N4 : 0;           // dG rows t = 1..T-1 | 0..T-2
    const int64_t shift_y = dir == 0 ? 0 : (int64_t)B * D * H;        // y  rows t = 0..T-2 | 1..T-1
    g.A = ghid + shift_g + (int64_t)dir * 4 * H; g.a_mc = 1; g.a_sk = N4; g.a_div = 1;
    g.B = d->y + shift_y + (int64_t)dir * H; g.b_sn = 1; g.b_sk = (int64_t)D * H;
    g.C = w.dwhh + (int64_t)dir * 4 * H * H; g.c_div = 1; g.c_so = H; g.c_si = 0;
    g.workspace = w.scratch; g.workspace_bytes = w.scratch_bytes;
    if (g.K > 0) {
      if ((rc = rnnt_hip_gemm_f32(&g, s))) return rc;
    } else {
      RNNT_CHECK_HIP(hipMemsetAsync(g.C, 0, (size_t)4 * H * H * 4, s));
    }
  }
  if ((rc = unpermute(w.dwhh, H, H, D, ngate, bd->dw_hh, acc, s))) return rc;
  // 5. bias gradient = column sums of dG, un-permuted (the v4 / v5 recurrences already summed their own cells over time)
  if (fused_db) {
    hipLaunchKernelGGL(db_reduce_kernel, dim3((unsigned)ceil_div(4 * H, 256), D), dim3(256), 0, s, k.dbp, db_rows, H, ngate, bd->db[0],
                       second(bd->db, D), acc, twin0, twin1);
    RNNT_CHECK_LAUNCH();
    if (gru) {
      hipLaunchKernelGGL(db_reduce_kernel, dim3((unsigned)ceil_div(4 * H, 256), D), dim3(256), 0, s, k.dbhp, db_rows, H, ngate, bd->db_hh[0],
                         second(bd->db_hh, D), acc);
      RNNT_CHECK_LAUNCH();
    }
  } else {
    if ((rc = launch_colsum(d->gates, (long)M, (long)N4, (long)N4, w.bp, w.scratch, w.scratch_bytes, s))) return rc;
    if ((rc = unpermute(w.bp, H, 1, D, ngate, bd->db, acc, s, twin0, twin1))) return rc;
    if (gru) {  // b_hh sees the hidden-side gradients (n gate scaled by r)
      if ((rc = launch_colsum(ghid, (long)M, (long)N4, (long)N4, w.bp, w.scratch, w.scratch_bytes, s))) return rc;
      if ((rc = unpermute(w.bp, H, 1, D, ngate, bd->db_hh, acc, s))) return rc;
    }
  }
  return RNNT_OK;
}

extern "C" int rnnt_hip_lstm_bwd(const rnnt_lstm_bwd_desc* bd, void* stream) { return lstm_bwd_impl(bd, RNNT_PRECISION_FP32, stream); }

extern "C" int rnnt_hip_lstm_bwd_ex(const rnnt_lstm_bwd_desc* bd, uint32_t precision, void* stream) {
  RNNT_CHECK_ARG(precision == RNNT_PRECISION_FP32 || precision == RNNT_PRECISION_F16, "lstm_bwd_ex: precision must be 0 (fp32) or 1 (f16), got %u",
                 precision);
  return lstm_bwd_impl(bd, precision, stream);
}

extern "C" int rnnt_hip_lstm_check(const void* workspace, void* stream) {
  // word 0 of the workspace is the persistent kernels' status word (0 = ok, 1 = an inter-CU wait gave up)
  RNNT_CHECK_ARG(workspace != nullptr, "lstm_check: null workspace");
  unsigned st = 0;
  RNNT_CHECK_HIP(hipMemcpyAsync(&st, workspace, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream));
  RNNT_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  if (st != 0) {
    set_error("persistent LSTM kernel abandoned an inter-workgroup wait (status %u)", st);
    return RNNT_ERR_TIMEOUT;
  }
  return RNNT_OK;
}

extern "C" int rnnt_hip_lstm_debug_read(const void* workspace, int32_t T, int32_t B, int32_t I, int32_t H, int32_t D,
                                        uint64_t* out, int32_t nwg, void* stream) {
  RNNT_CHECK_ARG(workspace && out && nwg >= 1 && nwg <= 512, "lstm_debug_read: bad arguments");
  const LayerPlan lp = resolve_plan(T, B, I, H, D, RNNT_CELL_LSTM, device_cus());
  RNNT_CHECK_ARG(lp.accepted, "lstm_debug_read: unsupported shape");
  const LstmWs w = carve_lstm(const_cast<void*>(workspace), T, B, I, H, D, lp);
  RNNT_CHECK_HIP(hipMemcpyAsync(out, w.dbg, (size_t)nwg * 8 * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
  RNNT_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  return RNNT_OK;
}
