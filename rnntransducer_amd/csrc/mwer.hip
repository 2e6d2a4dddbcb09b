// MWER (minimum word error rate) training, the pieces between the frame-synchronous search and the fused loss (DESIGN.md §22,
// include/rnnt_hip.h):
//   rnnt_hip_edit_distance  Levenshtein distances of P (hypothesis, reference) pairs, one wavefront per pair
//   rnnt_hip_nbest_pack     the search's device outputs (tokens, counts | lens) -> the loss's inputs for rows r = b*N + n
//   rnnt_hip_mwer_risk      the expected-risk combination of N hypotheses per utterance and its gradient weights, in fp64
// Three small kernels: no inter-workgroup communication, nothing persistent, every sum in a fixed order.
#include "common.hpp"

namespace rnnt {
namespace {

constexpr int ED_MAX_LEN = 511;          // the loss's U + 1 <= 512
constexpr int ED_COLS = 8;               // DP columns per lane: 64 lanes x 8 = the 512 columns j = 0..511 of a row
constexpr int ED_BIG = 1 << 20;          // "no value": above every distance (<= 511), far from int overflow
constexpr int MWER_MAX_N = 64;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// One wavefront per pair p: the DP row D[i][0..R] over the reference, lane l owning columns 8l..8l+7.  Per hypothesis token h:
//   tmp[j] = min(prev[j] + 1, prev[j-1] + (h != r_j))           (deletion / substitution: from the previous row only)
//   cur[j] = min(tmp[j], cur[j-1] + 1) = j + min_{k<=j}(tmp[k] - k)   (insertions: a prefix minimum over the row)
// with tmp[0] = i.  The prefix minimum runs serially inside the lane, then as a scan over the lanes' totals.  Columns above R hold
// values nobody reads: a column only depends on lower ones.
__global__ void __launch_bounds__(64) edit_distance_kernel(const int* __restrict__ hyp, long hyp_ld, const int* __restrict__ hyp_lens,
                                                           const int* __restrict__ ref, long ref_ld, const int* __restrict__ ref_lens,
                                                           int ref_div, int* __restrict__ dist) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int q = p / ref_div;
  const int H = clampi(hyp_lens[p], 0, (int)hyp_ld), R = clampi(ref_lens[q], 0, (int)ref_ld);
  const int* hrow = hyp + (long)p * hyp_ld;
  const int* rrow = ref + (long)q * ref_ld;
  const int j0 = lane * ED_COLS;
  int rtok[ED_COLS], prev[ED_COLS];
#pragma unroll
  for (int c = 0; c < ED_COLS; ++c) {
    const int j = j0 + c;                                  // column j compares with reference token j - 1
    rtok[c] = (j >= 1 && j <= R) ? rrow[j - 1] : INT_MIN;  // INT_MIN: a column outside the reference never matches
    prev[c] = j;                                           // row 0: j insertions
  }
  for (int i = 1; i <= H; ++i) {
    const int h = hrow[i - 1];
    int left = __shfl_up(prev[ED_COLS - 1], 1);            // prev[j0 - 1]
    if (lane == 0) left = ED_BIG;
    int run = ED_BIG;                                      // min_{k in this lane, k <= j} (tmp[k] - k)
    int v[ED_COLS];
#pragma unroll
    for (int c = 0; c < ED_COLS; ++c) {
      const int j = j0 + c;
      int t = min(prev[c] + 1, left + (h != rtok[c] ? 1 : 0));
      if (j == 0) t = i;
      left = prev[c];
      run = min(run, t - j);
      v[c] = run;
    }
    int inc = run;                                         // inclusive scan-min of the lanes' totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int other = __shfl_up(inc, o);
      if (lane >= o) inc = min(inc, other);
    }
    int exc = __shfl_up(inc, 1);                           // the lanes below
    if (lane == 0) exc = ED_BIG;
#pragma unroll
    for (int c = 0; c < ED_COLS; ++c) prev[c] = min(min(v[c], exc) + j0 + c, ED_BIG);
  }
  int out = 0;
#pragma unroll
  for (int c = 0; c < ED_COLS; ++c) out = (R % ED_COLS == c) ? prev[c] : out;
  if (lane == R / ED_COLS) dist[p] = out;
}

// One thread per row r = b*N + n.  A row is valid when n < counts[b] and its hypothesis (lens - 1 tokens behind the leading blank)
// is no longer than max_hyp_len; lens of a rank >= counts[b] is not read (the search leaves it unwritten).
__global__ void __launch_bounds__(64) nbest_pack_kernel(const int* __restrict__ tokens, long max_len, const int* __restrict__ counts,
                                                        const int* __restrict__ lens, const int* __restrict__ frame_lens, int rows,
                                                        int N, int Umax, int max_hyp_len, int blank, long long* __restrict__ texts,
                                                        int* __restrict__ labels, int* __restrict__ u_lens, int* __restrict__ t_lens,
                                                        int* __restrict__ valid) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  const int b = r / N, n = r % N;
  int u = 0, ok = 0;
  if (n < counts[b]) {
    u = lens[r] - 1;
    ok = u >= 0 && u <= max_hyp_len && u <= Umax && (long)u + 1 <= max_len;
  }
  if (!ok) u = 0;
  const int* y = tokens + (long)r * max_len + 1;
  long long* tx = texts + (long)r * (Umax + 1);
  int* lb = labels + (long)r * Umax;
  tx[0] = blank;
  for (int k = 0; k < Umax; ++k) {
    const int tok = k < u ? y[k] : blank;
    tx[k + 1] = tok;
    lb[k] = tok;
  }
  u_lens[r] = u;
  t_lens[r] = ok ? frame_lens[b] : 0;   // 0 frames: the loss gives +inf and exact-zero gradients for the row
  valid[r] = ok;
}

// One wavefront per utterance, lane n = hypothesis n.  Every lane walks the N values in LDS in index order, so all sums have one
// fixed order and a row's result does not depend on the batch around it.
__global__ void __launch_bounds__(64) mwer_risk_kernel(const float* __restrict__ nll, const int* __restrict__ dist,
                                                       const int* __restrict__ valid, int N, double gscale, float* __restrict__ risk,
                                                       float* __restrict__ weights) {
  __shared__ double s_nll[MWER_MAX_N], s_w[MWER_MAX_N];
  __shared__ int s_ok[MWER_MAX_N];
  const int b = blockIdx.x, n = threadIdx.x;
  if (n < N) {
    const long r = (long)b * N + n;
    const double x = (double)nll[r];
    const int ok = valid[r] != 0 && x == x;   // a NaN row counts as invalid
    s_ok[n] = ok;
    s_nll[n] = ok ? x : 0.0;                  // an invalid row's +inf never enters the arithmetic
    s_w[n] = ok ? (double)dist[r] : 0.0;
  }
  __syncthreads();
  int cnt = 0;
  double mn = INFINITY, wsum = 0.0;
  for (int i = 0; i < N; ++i) {
    if (!s_ok[i]) continue;
    ++cnt;
    mn = fmin(mn, s_nll[i]);
    wsum += s_w[i];
  }
  double r_out = 0.0, w_out = 0.0;
  if (cnt >= 2 && mn < INFINITY) {            // mn = +inf: every valid row is impossible, there is no distribution to weigh
    double z = 0.0;
    for (int i = 0; i < N; ++i)
      if (s_ok[i]) z += exp(-(s_nll[i] - mn));
    const double wbar = wsum / (double)cnt;
    const double wn = n < N ? s_w[n] : 0.0;
    double dev = 0.0;                         // W_n - sum_i P^_i W_i as sum_i P^_i (W_n - W_i): the differences are exact integers,
    for (int i = 0; i < N; ++i)               // so equal W give exactly 0 and a dominant hypothesis loses nothing to cancellation
      if (s_ok[i]) {
        const double p = exp(-(s_nll[i] - mn)) / z;
        r_out += p * (s_w[i] - wbar);
        dev += p * (wn - s_w[i]);
      }
    if (n < N && s_ok[n]) w_out = gscale * (-(exp(-(s_nll[n] - mn)) / z) * dev);
  }
  if (n < N) weights[(long)b * N + n] = (float)w_out;
  if (n == 0) risk[b] = (float)r_out;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" int rnnt_hip_edit_distance(const int32_t* hyp, int64_t hyp_ld, const int32_t* hyp_lens, const int32_t* ref, int64_t ref_ld,
                                      const int32_t* ref_lens, int32_t ref_div, int32_t P, int32_t* dist, void* stream) {
  RNNT_CHECK_ARG(hyp && hyp_lens && ref && ref_lens && dist, "edit_distance: null pointer");
  RNNT_CHECK_ARG(P >= 1, "edit_distance: P = %d pairs, must be positive", P);
  RNNT_CHECK_ARG(ref_div >= 1, "edit_distance: ref_div = %d, must be positive", ref_div);
  RNNT_CHECK_ARG(hyp_ld >= 0 && hyp_ld <= ED_MAX_LEN && ref_ld >= 0 && ref_ld <= ED_MAX_LEN,
                 "edit_distance: sequences of up to %d tokens (hyp_ld = %lld, ref_ld = %lld)", ED_MAX_LEN, (long long)hyp_ld,
                 (long long)ref_ld);
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)P * (double)(hyp_ld + ref_ld + 3), (hipStream_t)stream);
  hipLaunchKernelGGL(edit_distance_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, hyp, (long)hyp_ld, hyp_lens, ref, (long)ref_ld,
                     ref_lens, ref_div, dist);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_nbest_pack(const int32_t* tokens, int64_t max_len, const int32_t* counts, const int32_t* lens,
                                   const int32_t* frame_lens, int32_t B, int32_t N, int32_t Umax, int32_t max_hyp_len, int32_t blank,
                                   int64_t* texts, int32_t* labels, int32_t* u_lens, int32_t* t_lens, int32_t* valid, void* stream) {
  RNNT_CHECK_ARG(tokens && counts && lens && frame_lens && texts && labels && u_lens && t_lens && valid, "nbest_pack: null pointer");
  RNNT_CHECK_ARG(B >= 1 && N >= 1 && N <= MWER_MAX_N, "nbest_pack: B = %d must be positive and N = %d in [1, %d]", B, N, MWER_MAX_N);
  RNNT_CHECK_ARG((int64_t)B * N < (1ll << 31), "nbest_pack: B * N = %lld rows", (long long)B * N);
  RNNT_CHECK_ARG(max_len >= 1, "nbest_pack: max_len = %lld, must be positive", (long long)max_len);
  RNNT_CHECK_ARG(Umax >= 1 && Umax <= ED_MAX_LEN && max_hyp_len >= 1 && max_hyp_len <= ED_MAX_LEN,
                 "nbest_pack: Umax = %d and max_hyp_len = %d must lie in [1, %d]", Umax, max_hyp_len, ED_MAX_LEN);
  RNNT_CHECK_ARG(blank >= 0, "nbest_pack: blank = %d", blank);
  const int rows = B * N;
  ProfScope prof(RNNT_K_MISC, (double)rows * (16.0 * Umax + 24.0), (hipStream_t)stream);
  hipLaunchKernelGGL(nbest_pack_kernel, dim3((unsigned)ceil_div(rows, 64)), dim3(64), 0, (hipStream_t)stream, tokens, (long)max_len,
                     counts, lens, frame_lens, rows, N, Umax, max_hyp_len, blank, reinterpret_cast<long long*>(texts), labels, u_lens,
                     t_lens, valid);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_mwer_risk(const float* nll, const int32_t* dist, const int32_t* valid, int32_t B, int32_t N, double gscale,
                                  float* risk, float* weights, void* stream) {
  RNNT_CHECK_ARG(nll && dist && valid && risk && weights, "mwer_risk: null pointer");
  RNNT_CHECK_ARG(B >= 1 && N >= 1 && N <= MWER_MAX_N, "mwer_risk: B = %d must be positive and N = %d in [1, %d]", B, N, MWER_MAX_N);
  RNNT_CHECK_ARG(gscale == gscale && gscale - gscale == 0.0, "mwer_risk: gscale must be finite");
  ProfScope prof(RNNT_K_MISC, 20.0 * (double)B * N, (hipStream_t)stream);
  hipLaunchKernelGGL(mwer_risk_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, nll, dist, valid, N, gscale, risk, weights);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}
