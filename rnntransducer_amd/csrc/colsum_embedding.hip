// Kernels that serve the layers around the recurrences and have C entries of their own: deterministic column sums (bias gradients) and
// the embedding forward / backward of the prediction network.
#include "common.hpp"

namespace rnnt {
namespace {

// two-stage deterministic column sum.  stage 1: grid (ceil(N/64), RC): block (64 columns x 4 row lanes) sums its
// row chunk into part[rc][n]; stage 2: out[n] = sum_rc part[rc][n] in fixed order.
constexpr int COLSUM_RC_MAX = 128;
inline int colsum_chunks(long M, long N) {
  long want = ceil_div(2048, ceil_div(N, 64));  // ~2048 blocks in flight
  const long by_m = ceil_div(M, 64);
  if (want > by_m) want = by_m;
  if (want > COLSUM_RC_MAX) want = COLSUM_RC_MAX;
  return (int)(want < 1 ? 1 : want);
}
__global__ void __launch_bounds__(256) colsum_stage1_kernel(const float* __restrict__ X, long M, long N, long ld,
                                                            long rows_per_chunk, float* __restrict__ part) {
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
  const long n = (long)blockIdx.x * 64 + c;
  const long m0 = (long)blockIdx.y * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
  float s = 0.f;
  if (n < N)
    for (long m = m0 + r; m < m1; m += 4) s += X[m * ld + n];
  red[r][c] = s;
  __syncthreads();
  if (r == 0 && n < N) part[(long)blockIdx.y * N + n] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}
__global__ void __launch_bounds__(256) colsum_stage2_kernel(const float* __restrict__ part, long N, int rc,
                                                            float* __restrict__ out, int accumulate) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int k = 0; k < rc; ++k) s += part[(long)k * N + n];
  out[n] = accumulate ? out[n] + s : s;
}
}  // namespace

int launch_colsum(const float* X, long M, long N, long ld, float* out, void* ws, size_t ws_bytes, hipStream_t s,
                  int accumulate) {
  const int rc = colsum_chunks(M, N);
  RNNT_CHECK_ARG(ws && ws_bytes >= (size_t)rc * N * 4, "colsum: workspace too small (%zu < %zu)", ws_bytes, (size_t)rc * N * 4);
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)M * (double)N, s);
  const long rows = ceil_div(M, rc);
  hipLaunchKernelGGL(colsum_stage1_kernel, dim3((unsigned)ceil_div(N, 64), rc), dim3(256), 0, s, X, M, N, ld, rows, (float*)ws);
  RNNT_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_stage2_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, (const float*)ws, N, rc, out, accumulate);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

namespace {

__global__ void embedding_fwd_kernel(const float* __restrict__ W, const long* __restrict__ idx, long M, int H, int V,
                                     float* __restrict__ out) {
  const long total = M * H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / H;
    const int h = (int)(i % H);
    const long v = idx[m];
    out[i] = (v >= 0 && v < V) ? W[v * H + h] : 0.f;
  }
}

__global__ void __launch_bounds__(256) embedding_bwd_kernel(const float* __restrict__ dE, const long* __restrict__ idx, long M, int H, int V,
                                                            long pad, float* __restrict__ dW, int accumulate) {
  // one workgroup per vocabulary row: the tokens that hit it are compacted IN ORDER (ballot prefix) into LDS, then summed in that
  // fixed order (deterministic, no atomics) — the scan over all M tokens is done once per row, not once per feature
  constexpr int CAP = 2048;
  __shared__ int list[CAP];
  __shared__ int wcnt[4], nlist;
  const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (v == pad) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};   // features tid, tid + 256, ... (H <= 1024 keeps everything in registers; more: extra passes)
  for (int h0 = 0; h0 < H; h0 += 1024) {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = 0.f;
    for (long mb = 0; mb < M; mb += CAP) {   // batches of CAP tokens
      if (tid == 0) nlist = 0;
      __syncthreads();
      const long mend = min(M, mb + CAP);
      for (long m0 = mb; m0 < mend; m0 += 256) {
        const long m = m0 + tid;
        const bool hit = m < mend && idx[m] == v;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int base = nlist;
        for (int w = 0; w < wave; ++w) base += wcnt[w];
        if (hit) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int)(m - mb);
        __syncthreads();
        if (tid == 0) nlist += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
      }
      const int n = nlist;
      for (int i = 0; i < n; ++i) {
        const float* row = dE + (mb + list[i]) * H + h0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (h0 + tid + 256 * q < H) acc[q] += row[tid + 256 * q];
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int h = h0 + tid + 256 * q;
      if (h < H) dW[(long)v * H + h] = accumulate ? dW[(long)v * H + h] + acc[q] : acc[q];
    }
  }
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" size_t rnnt_hip_colsum_workspace_bytes(int64_t M, int64_t N) {
  if (M < 0 || N < 1) return 0;
  return (size_t)colsum_chunks((long)M, (long)N) * (size_t)N * 4;
}

extern "C" int rnnt_hip_colsum_f32(const float* X, int64_t M, int64_t N, int64_t ld, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  RNNT_CHECK_ARG((X || M == 0) && out && M >= 0 && N >= 1 && ld >= N, "colsum: bad arguments");
  return launch_colsum(X, (long)M, (long)N, (long)ld, out, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int rnnt_hip_colsum_f32_acc(const float* X, int64_t M, int64_t N, int64_t ld, float* out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  RNNT_CHECK_ARG((X || M == 0) && out && M >= 0 && N >= 1 && ld >= N, "colsum: bad arguments");
  return launch_colsum(X, (long)M, (long)N, (long)ld, out, workspace, workspace_bytes, (hipStream_t)stream, 1);
}

extern "C" int rnnt_hip_embedding_fwd(const float* W, const int64_t* idx, int64_t M, int32_t H, int32_t V, float* out,
                                      void* stream) {
  RNNT_CHECK_ARG(M >= 0 && W && ((idx && out) || M == 0) && H >= 1 && V >= 1, "embedding_fwd: bad arguments");
  if (M == 0) return RNNT_OK;
  const long blocks = ceil_div(M * H, 256);
  hipLaunchKernelGGL(embedding_fwd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, W,
                     (const long*)idx, (long)M, H, V, out);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

static int embedding_bwd_impl(const float* dE, const int64_t* idx, int64_t M, int32_t H, int32_t V, int64_t padding_idx,
                              float* dW, int accumulate, void* stream) {
  RNNT_CHECK_ARG(M >= 0 && ((dE && idx) || M == 0) && dW && H >= 1 && V >= 1, "embedding_bwd: bad arguments");
  hipLaunchKernelGGL(embedding_bwd_kernel, dim3(V), dim3(256), 0, (hipStream_t)stream, dE, (const long*)idx, (long)M, H, V,
                     (long)padding_idx, dW, accumulate);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}
extern "C" int rnnt_hip_embedding_bwd(const float* dE, const int64_t* idx, int64_t M, int32_t H, int32_t V,
                                      int64_t padding_idx, float* dW, void* stream) {
  return embedding_bwd_impl(dE, idx, M, H, V, padding_idx, dW, 0, stream);
}
extern "C" int rnnt_hip_embedding_bwd_acc(const float* dE, const int64_t* idx, int64_t M, int32_t H, int32_t V,
                                          int64_t padding_idx, float* dW, void* stream) {
  return embedding_bwd_impl(dE, idx, M, H, V, padding_idx, dW, 1, stream);
}
