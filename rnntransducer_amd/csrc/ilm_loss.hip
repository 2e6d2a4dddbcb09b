// Internal-LM training (ILMT): the cross-entropy of the internal LM on the transcripts, and its gradient, for gfx950.
// DESIGN.md §26, include/rnnt_hip.h.
//
// The internal LM is the joint with the encoder half zeroed (§25): its logits at label position u of utterance b are
// z(u,b,v) = C(u,b,v) + bias[v], C = gelu(dec) W_d^T the (U1, B, V) tensor the fused loss already holds.  Over v != blank:
//   lse(u,b)   = m + log sum_v exp(z - m),  m = max_v z                              (fp32, lanes along v, butterfly reductions)
//   ilm_nll[b] = sum_{u < U_b} ((m - z(u,b,y_u)) + log sum_v exp(z - m))             (fp32 terms, fp64 sum in a fixed order)
//   dC(u,b,v)  = g_b (exp(z(u,b,v) - lse(u,b)) - [v == y_u])                         u < U_b, v != blank
// A counted label that is the blank or outside [0, V) makes its utterance infeasible: ilm_nll[b] = +inf, row b of dC exactly zero.
//
// Kernels (no inter-workgroup communication, no atomics; a value depends on its own utterance only):
//   ilm_fwd_kernel : a workgroup of 16 waves per utterance; wave w takes rows u = w, w + 16, ... and keeps an fp64 partial sum in
//                    that order, thread 0 adds the 16 partials in wave order.  The order depends on U_b alone, not on B or U1.
//   ilm_bwd_kernel : a wavefront per (u, b) row of dC; the row's lse is read, or recomputed by the forward's own row routine
//                    (the same bits).  Every wave first scans its utterance's counted labels for an invalid one (a ballot).
// Rows are read twice (maximum, then sum) from memory: a row is at most a few KB and stays in the cache between the passes, so
// there is no per-lane register budget and no second code path for a long row.
#include "common.hpp"
#include "lattice_shared.hpp"

namespace rnnt {
namespace {

constexpr int ILM_FWD_WAVES = 16;
constexpr int ILM_BWD_WAVES = 4;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }
__device__ __forceinline__ bool bad_label(int y, int V, int blank) { return y < 0 || y >= V || y == blank; }

// (m, log sum exp(z - m)) of one row over v != blank; every lane of the wave returns the same bits.  V >= 2: at least one entry.
__device__ __forceinline__ void ilm_row_stats(const float* __restrict__ c, const float* __restrict__ bias, int V, int blank, int lane,
                                              float& m, float& logs) {
  float mx = -__builtin_huge_valf();
  for (int v = lane; v < V; v += 64)
    if (v != blank) mx = fmaxf(mx, c[v] + bias[v]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int v = lane; v < V; v += 64)
    if (v != blank) s += expf((c[v] + bias[v]) - mx);
  s = wave_sum(s);
  m = mx;
  logs = logf(s);
}

__global__ void __launch_bounds__(ILM_FWD_WAVES * 64) ilm_fwd_kernel(const float* __restrict__ C, long c_sb, long c_su,
                                                                     const float* __restrict__ bias, const int* __restrict__ labels,
                                                                     const int* __restrict__ u_lens, int B, int U1, int V, int blank,
                                                                     float* __restrict__ ilm_nll, float* __restrict__ lse) {
  __shared__ double part[ILM_FWD_WAVES];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, U = U1 - 1;
  const int Ub = clampi(u_lens[b], 0, U);
  double acc = 0.0;
  for (int u = wave; u < Ub; u += ILM_FWD_WAVES) {
    const float* c = C + (long)b * c_sb + (long)u * c_su;
    float m, logs;
    ilm_row_stats(c, bias, V, blank, lane, m, logs);
    const int y = labels[(long)b * U + u];
    float term = __builtin_huge_valf();               // an invalid label: the utterance is infeasible (its logit is never read)
    if (!bad_label(y, V, blank)) term = (m - (c[y] + bias[y])) + logs;
    acc += (double)term;
    if (lse != nullptr && lane == 0) lse[(long)u * B + b] = m + logs;
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < ILM_FWD_WAVES; ++w) tot += part[w];
    ilm_nll[b] = (float)tot;
  }
}

__global__ void __launch_bounds__(ILM_BWD_WAVES * 64) ilm_bwd_kernel(const float* __restrict__ C, long c_sb, long c_su,
                                                                     const float* __restrict__ bias, const int* __restrict__ labels,
                                                                     const int* __restrict__ u_lens, const float* __restrict__ lse,
                                                                     int B, int U1, int V, int blank, float gscale,
                                                                     const float* __restrict__ gvec, int gvec_stride, int accumulate,
                                                                     float* __restrict__ dC) {
  const int lane = threadIdx.x & 63, U = U1 - 1;
  const long row = (long)blockIdx.x * ILM_BWD_WAVES + (threadIdx.x >> 6);
  if (row >= (long)U1 * B) return;                    // (uniform per wave; no barrier below)
  const int u = (int)(row / B), b = (int)(row % B);
  const int Ub = clampi(u_lens[b], 0, U);
  const int* yb = labels + (long)b * U;
  bool counted = u < Ub;
  if (counted) {                                      // an invalid label anywhere among the counted ones zeroes the whole utterance
    bool bad = false;
    for (int k = lane; k < Ub; k += 64) bad |= bad_label(yb[k], V, blank);
    counted = __ballot(bad) == 0ull;
  }
  const long off = (long)b * c_sb + (long)u * c_su;
  float* d = dC + off;
  if (!counted) {
    if (!accumulate)
      for (int v = lane; v < V; v += 64) d[v] = 0.f;
    return;
  }
  const float* c = C + off;
  float l;
  if (lse != nullptr) {
    l = lse[(long)u * B + b];
  } else {
    float m, logs;
    ilm_row_stats(c, bias, V, blank, lane, m, logs);
    l = m + logs;
  }
  const int y = yb[u];
  const float g = __fmul_rn(gscale, gvec != nullptr ? gvec[(long)b * gvec_stride] : 1.f);
  for (int v = lane; v < V; v += 64) {
    if (v == blank) {
      if (!accumulate) d[v] = 0.f;
      continue;
    }
    const float p = expf((c[v] + bias[v]) - l);
    // rounded product, then a separate addition: accumulate = 1 is bitwise prefill + the accumulate = 0 value (no fused multiply-add)
    const float val = __fmul_rn(g, p - (v == y ? 1.f : 0.f));
    d[v] = accumulate ? __fadd_rn(d[v], val) : val;
  }
}

int check_ilm_args(const char* what, const void* C, const void* bias, const void* labels, const void* u_lens, const void* out,
                   int64_t c_su, int32_t B, int32_t U1, int32_t V, int32_t blank) {
  RNNT_CHECK_ARG(C && bias && labels && u_lens && out, "%s: null pointer", what);
  RNNT_CHECK_ARG(B >= 1 && U1 >= 1, "%s: B = %d and U1 = %d must be positive", what, B, U1);
  RNNT_CHECK_ARG(V >= 2, "%s: V = %d: the internal LM needs a non-blank token (V >= 2)", what, V);
  RNNT_CHECK_ARG(blank >= 0 && blank < V, "%s: blank %d outside [0,%d)", what, blank, V);
  RNNT_CHECK_ARG(c_su >= V, "%s: c_su = %lld is below V = %d", what, (long long)c_su, V);
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" int rnnt_hip_ilm_loss_fwd(const float* C, int64_t c_sb, int64_t c_su, const float* bias, const int32_t* labels,
                                     const int32_t* u_lens, int32_t B, int32_t U1, int32_t V, int32_t blank, float* ilm_nll,
                                     float* lse, void* stream) {
  if (int rc = check_ilm_args("ilm_loss_fwd", C, bias, labels, u_lens, ilm_nll, c_su, B, U1, V, blank)) return rc;
  ProfScope prof(RNNT_K_MISC, 2.0 * 4.0 * (double)B * U1 * V, (hipStream_t)stream);
  hipLaunchKernelGGL(ilm_fwd_kernel, dim3(B), dim3(ILM_FWD_WAVES * 64), 0, (hipStream_t)stream, C, (long)c_sb, (long)c_su, bias,
                     labels, u_lens, B, U1, V, blank, ilm_nll, lse);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_ilm_loss_bwd(const float* C, int64_t c_sb, int64_t c_su, const float* bias, const int32_t* labels,
                                     const int32_t* u_lens, const float* lse, int32_t B, int32_t U1, int32_t V, int32_t blank,
                                     float gscale, const float* gvec, int32_t gvec_stride, int32_t accumulate, float* dC,
                                     void* stream) {
  if (int rc = check_ilm_args("ilm_loss_bwd", C, bias, labels, u_lens, dC, c_su, B, U1, V, blank)) return rc;
  RNNT_CHECK_ARG(gvec_stride >= 0, "ilm_loss_bwd: gvec_stride = %d is negative", gvec_stride);
  const int64_t rows = (int64_t)U1 * B;
  RNNT_CHECK_ARG(ceil_div(rows, ILM_BWD_WAVES) < (1ll << 31), "ilm_loss_bwd: U1 * B = %lld rows", (long long)rows);
  ProfScope prof(RNNT_K_MISC, 3.0 * 4.0 * (double)rows * V, (hipStream_t)stream);
  hipLaunchKernelGGL(ilm_bwd_kernel, dim3((unsigned)ceil_div(rows, ILM_BWD_WAVES)), dim3(ILM_BWD_WAVES * 64), 0, (hipStream_t)stream,
                     C, (long)c_sb, (long)c_su, bias, labels, u_lens, lse, B, U1, V, blank, gscale, gvec, gvec_stride,
                     accumulate != 0 ? 1 : 0, dC);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}
