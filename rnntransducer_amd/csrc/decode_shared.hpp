// Prediction-net step pieces shared by the search kernels (decode.hip: greedy search and the batched step; beam.hip: beam
// search).  One workgroup of DEC_THREADS threads owns one utterance; state vectors live in LDS, weights are streamed.
#pragma once
#include "common.hpp"

namespace rnnt {

constexpr int DEC_THREADS = 1024;
constexpr int DEC_MAX_LAYERS = RNNT_DECODE_MAX_LAYERS;

// y[r] = dot(W[r, :cols], x) (+ bias[r]) for r in [0, rows): one wave per group of RU rows (lanes along the contiguous k),
// 16 waves per pass.  All RU rows' loads are issued before any is consumed: a single row per wave keeps only 2 KB in
// flight per wave and the step becomes latency-bound (measured 308 us per prediction-net step at H=512).
constexpr int RU = 8;
__device__ __forceinline__ void matvec(const float* __restrict__ W, long ld, int rows, int cols, const float* __restrict__ x,
                                       float* __restrict__ y, const float* __restrict__ bias) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = DEC_THREADS / 64;
  for (int r0 = wave * RU; r0 < rows; r0 += nw * RU) {
    float s[RU];
#pragma unroll
    for (int i = 0; i < RU; ++i) s[i] = 0.f;
    for (int k = 4 * lane; k < cols; k += 256) {
      f32x4 w[RU];
#pragma unroll
      for (int i = 0; i < RU; ++i) {
        const int r = r0 + i < rows ? r0 + i : rows - 1;  // clamp: tail rows re-read the last row, result discarded
        w[i] = *reinterpret_cast<const f32x4*>(W + (long)r * ld + k);
      }
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + k);
#pragma unroll
      for (int i = 0; i < RU; ++i) s[i] += w[i][0] * xv[0] + w[i][1] * xv[1] + w[i][2] * xv[2] + w[i][3] * xv[3];
    }
#pragma unroll
    for (int i = 0; i < RU; ++i) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
    }
    if (lane < RU && r0 + lane < rows) {
      float v = s[0];
#pragma unroll
      for (int i = 1; i < RU; ++i) v = lane == i ? s[i] : v;
      y[r0 + lane] = v + (bias ? bias[r0 + lane] : 0.f);
    }
  }
}

__device__ __forceinline__ int cell_gates(int cell) { return cell == RNNT_CELL_LSTM ? 4 : (cell == RNNT_CELL_GRU ? 3 : 1); }

// The L stacked cells of one step (torch.nn.LSTM / GRU / RNN equations), in place on LDS state h[L][Hp], c[L][Hp].  On entry
// x[0:Hp] holds the layer-0 input (the token's embedding row); gi / gh are 4*Hp scratch each.  gi0, if not null, is the
// precomputed layer-0 input projection W_ih0 x + b_ih0 of this token (same matvec, so the same bits): x is then not read.
// P provides Hp, L, cell, w_ih[], w_hh[], b_ih[], b_hh[].  Ends with a barrier; the last layer's output is h[(L-1)*Hp:].
template <class P>
__device__ __forceinline__ void prednet_cells(const P& p, float* h, float* c, float* gi, float* gh, float* x, const float* gi0) {
  const int Hp = p.Hp, tid = threadIdx.x, NG = cell_gates(p.cell);
  for (int l = 0; l < p.L; ++l) {
    if (l == 0 && gi0) {
      for (int i = tid; i < NG * Hp; i += DEC_THREADS) gi[i] = gi0[i];
    } else {
      matvec(p.w_ih[l], Hp, NG * Hp, Hp, x, gi, p.b_ih[l]);
    }
    matvec(p.w_hh[l], Hp, NG * Hp, Hp, h + l * Hp, gh, p.b_hh[l]);
    __syncthreads();
    for (int j = tid; j < Hp; j += DEC_THREADS) {
      float hv;
      if (p.cell == RNNT_CELL_LSTM) {
        const float ig = sigmoidf_(gi[j] + gh[j]), fg = sigmoidf_(gi[Hp + j] + gh[Hp + j]);
        const float gg = tanhf(gi[2 * Hp + j] + gh[2 * Hp + j]), og = sigmoidf_(gi[3 * Hp + j] + gh[3 * Hp + j]);
        const float cv = fg * c[l * Hp + j] + ig * gg;
        c[l * Hp + j] = cv;
        hv = og * tanhf(cv);
      } else if (p.cell == RNNT_CELL_GRU) {
        const float rg = sigmoidf_(gi[j] + gh[j]), zg = sigmoidf_(gi[Hp + j] + gh[Hp + j]);
        const float ng = tanhf(gi[2 * Hp + j] + rg * gh[2 * Hp + j]);
        hv = (1.f - zg) * ng + zg * h[l * Hp + j];
      } else {
        const float pre = gi[j] + gh[j];
        hv = p.cell == RNNT_CELL_RNN_RELU ? fmaxf(pre, 0.f) : tanhf(pre);
      }
      h[l * Hp + j] = hv;
      x[j] = hv;  // input of the next layer (no dropout at inference)
    }
    __syncthreads();
  }
}

// C = gelu(out_proj(h_last)) . W_d^T (the prediction-net half of the joint, networks/transducer.py:64-69).  P provides O, V,
// Hp, w_o, b_o, w_d, ld_d.  dec is O floats of LDS scratch.  Ends with a barrier.
template <class P>
__device__ __forceinline__ void prednet_joint_half(const P& p, const float* h_last, float* dec, float* Cv) {
  matvec(p.w_o, p.Hp, p.O, p.Hp, h_last, dec, p.b_o);
  __syncthreads();
  for (int i = threadIdx.x; i < p.O; i += DEC_THREADS) dec[i] = gelu_tanh(dec[i]);
  __syncthreads();
  matvec(p.w_d, p.ld_d, p.V, p.O, dec, Cv, nullptr);
  __syncthreads();
}

// log-softmax of one joint evaluation at the token the argmax chose: z[tok] - lse_v(z) with z[v] = a[v] + Cv[v], fp32.  tok is
// the argmax, so z[tok] is the maximum and lse = z[tok] + log(sum_v exp(z[v] - z[tok])): one V-wide reduction.  Its order is
// fixed by (tid, lane, wave) alone: a strided pass per thread, the wave butterfly (a + b == b + a: every lane holds the same
// sum), then the waves in order; nothing depends on B, T or a chunk boundary.  All threads call it; red is DEC_THREADS / 64
// floats of LDS nobody reads at the call; every thread returns the value.  Ends with a barrier.
__device__ __forceinline__ float token_logp(const float* __restrict__ a, const float* __restrict__ Cv, int V, int tok, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float zt = a[tok] + Cv[tok];
  float s = 0.f;
  for (int v = tid; v < V; v += DEC_THREADS) s += expf((a[v] + Cv[v]) - zt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < DEC_THREADS / 64; ++w) r += red[w];
  __syncthreads();
  return -logf(r);
}

}  // namespace rnnt
