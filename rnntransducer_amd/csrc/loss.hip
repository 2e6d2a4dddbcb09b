// Fused joint + log-softmax + RNN-T lattice for gfx950.
//
// Replaces JointNet.joint (networks/transducer.py:54-69: repeat/cat/GELU/Linear materialising
// (B,T,U+1,2*O) three times and (B,T,U+1,V) once) followed by RNNTLoss(blank, reduction="mean")
// (model.py:39,57; arithmetic in third-party warp-transducer / torchaudio).  Uses the separable form
// z[b,t,u,:] = A[b,t,:] + C[b,u,:] + bias so only two floats per lattice cell are ever
// written: log p(blank) and log p(y_u).
//
// Kernels (all HBM/latency-bound integer+transcendental work; no MFMA here by design):
//   band_kernel                       : emission windows -> the band tables L, R and the feasibility flag of every row
//   lse_sep_kernel / lse_dense_kernel : per-cell log-sum-exp -> blk[b][u][t], emit[b][u][t] (u-major)
//   lse_sepv_kernel                   : lse_sep_kernel for V >= 256, a lane per vocabulary entry
//   alphabeta_kernel<K, MAX>          : one wavefront per (utterance, alpha|beta); lane l owns label
//                                       positions [l*K, l*K+K) and sweeps t with a one-lane skew, so each
//                                       step advances one anti-diagonal; neighbour hand-off by lane shuffle;
//                                       accumulators in fp64 with an fp32 log1p(exp(.)) correction term.
//                                       MAX = true: the same alpha sweep in the (max, +) semiring, for forced
//                                       alignment -- one back-pointer bit per cell instead of the cell store
//   grad_sep_kernel                   : dA[b,t,:] = sum_u dz, partial dC slabs per 32-frame tile (LDS adds)
//   reduce_dc_kernel                  : fixed-order sum of the slabs (bitwise reproducible, no float atomics)
//   grad_sepv_kernel                  : grad_sep_kernel with the vocabulary a grid dimension (V >= 256, or a table past LDS)
//   grad_dense_kernel                 : warp-transducer-shaped d/d logits for rnnt_hip_loss_from_logits_*
//   backtrace_kernel                  : forced alignment -- the best path, walked back through the MAX sweep's back-pointer bits
//   kd_value_kernel                   : lattice distillation -- the collapsed KL per utterance, fp64 sums in a fixed order
// The W / FE / KD template flags select the emission-window / FastEmit / distillation instances; all false: the kernels without them.
// The host half (from struct LossWs on): one LossCall per call, one check, four stages, three drivers behind the exported entries.
#include "common.hpp"
#include "lattice_shared.hpp"

#include <stdlib.h>

#include <type_traits>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

namespace rnnt {
namespace {

constexpr int TT = 32;  // frames per workgroup tile

// dense-logits entry points accept fp32, fp16 or bf16 storage (torchaudio's RNNTLoss takes half logits, model.py:28-31);
// all arithmetic stays fp32 / fp64
__device__ __forceinline__ float ldf(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float ldf(const __half* p, long i) { return __half2float(p[i]); }
__device__ __forceinline__ float ldf(const __hip_bfloat16* p, long i) { return __bfloat162float(p[i]); }
__device__ __forceinline__ void stf(float* p, long i, float v) { p[i] = v; }
__device__ __forceinline__ void stf(__half* p, long i, float v) { p[i] = __float2half(v); }
__device__ __forceinline__ void stf(__hip_bfloat16* p, long i, float v) { p[i] = __float2bfloat16(v); }
// ------------------------------------------------------------------------------------------------
// Emission windows (alignment-restricted loss; include/rnnt_hip.h).  Label u of row b may be emitted at frame t only
// if lo[b][u] <= t <= hi[b][u]: emit(t,u) = -inf elsewhere, everything else is the usual lattice.  The BAND is a work-skipping
// device on top of that: with L[u] = max(0, lo[0..u-1]) and R[u] = min(hi[u..Ub-1], Tb-1), a cell can lie on an allowed path only
// if L[u] <= t <= R[u]; both tables are non-decreasing in u, so the live cells of a frame (and of a 32-frame tile) are one interval
// of u.  Cells outside the band get blk = emit = -inf without their V-wide terms being computed (no allowed path passes through
// them, so the sums over allowed paths do not change) and the gradient kernels leave them out.  Every kernel below has a template
// flag W: the W = false instance is the code without this feature (the tables are never read).
// band_kernel: one workgroup per row.  An infeasible row (an empty window, windows that force labels out of order, no frame) gets
// an EMPTY band (L > R everywhere) and feas = 0: nothing of it is computed, its NLL is +inf and its gradient rows are exact zeros.
// Rows of the tables beyond u_len are empty too.  Entries lo / hi at u >= u_len are never read.
// ------------------------------------------------------------------------------------------------
constexpr int BAND_NONE_L = 0x3fffffff, BAND_NONE_R = -1;

struct Win {   // what the lse kernels read
  const int *L, *R;      // [B][U1] band
  const int *lo, *hi;    // the caller's windows, row stride `stride`
  const int* u_lens;
  long stride;
};

struct Band {   // what the gradient kernels read
  const int *L, *R;
};
// A kernel with the flag W takes its tables as a trailing parameter PACK: empty for W = false, so that instance has the parameter
// list (and the kernel-argument block) of the kernel without this feature; one Win / Band for W = true.  The flag KD (lattice
// distillation, below) adds its one struct to the same pack.  pick_tables<T> (lattice_shared.hpp): the pack's member of type T, or
// an empty T.

// ------------------------------------------------------------------------------------------------
// Lattice knowledge distillation (Panchapagesan et al. 2021; include/rnnt_hip.h).  Per lattice cell the teacher's and
// the student's distributions are collapsed to three classes -- blank, the cell's label y_u (u < U_b only), everything else -- and
// the term is the sum over the cells of KL(teacher || student).  The third class needs a third per-cell plane next to blk / emit:
//   rest[b][u][t] = log sum_{v not in {blank, y_u}} softmax(z)[v]        (u >= u_lens[b]: every non-blank entry)
// a log-sum-exp over the entries themselves (1 - p_blank - p_label would lose everything once the blank dominates), which the KD
// instances of the lse kernels take from the exponentials of the full sum: the same running maximum, a second accumulator that skips
// the two entries.  blk / emit of a KD instance are the bits of the plain one (the full sum is accumulated in the same order).
// FLOOR: an entry more than ~87 below the cell's largest logit underflows in fp32 (2^-126) and adds nothing; the plane is floored at
// KD_REST_FLOOR = -80, above that gap, so rest is finite whatever the logits are (V >= 3: the class is never empty) and is the true
// value to fp32 rounding wherever the true value is >= -80.  A student floored there has the class's gradient capped, not NaN.
// ------------------------------------------------------------------------------------------------
constexpr float KD_REST_FLOOR = -80.f;

struct KdLse {   // what the KD instances of the lse kernels take: where rest goes, and the label counts that end the label class
  float* rest;
  const int* u_lens;
};

struct KdGrad {   // what the KD instances of the gradient kernels take
  const float *t_blk, *t_emit, *t_rest;   // the teacher's planes, laid out as blk / emit
  const float* rest;                      // the student's third plane (workspace)
  float kscale;                           // upstream gradient of the KD term: kscale * kvec[b * kstride] (kvec null: kscale)
  const float* kvec;
  int kstride;
};

__global__ void __launch_bounds__(256) band_kernel(const int* __restrict__ lo, const int* __restrict__ hi, long stride,
                                                   const int* __restrict__ t_lens, const int* __restrict__ u_lens, int T, int U1,
                                                   int* __restrict__ L, int* __restrict__ R, int* __restrict__ feas) {
  __shared__ int sl[512], sr[512];   // U+1 <= 512
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = min(t_lens[b], T), Ub = max(min(u_lens[b], U1 - 1), 0);
  const int* lob = lo + (long)b * stride;
  const int* hib = hi + (long)b * stride;
  bool ok = Tb >= 1;
  for (int u = tid; u < Ub; u += 256) {
    const int l = max(lob[u], 0), h = min(hib[u], Tb - 1);
    sl[u] = l;
    sr[u] = h;
    ok = ok && l <= h;
  }
  __syncthreads();
  if (tid == 0) {         // L[u] = max(0, lo[0 .. u-1]): running maximum, in place (sl[u] <- L[u+1])
    int m = 0;
    for (int u = 0; u < Ub; ++u) { m = max(m, sl[u]); sl[u] = m; }
  } else if (tid == 64) {   // R[u] = min(hi[u .. Ub-1], Tb-1): running minimum from the end, in place
    int m = Tb - 1;
    for (int u = Ub - 1; u >= 0; --u) { m = min(m, sr[u]); sr[u] = m; }
  }
  __syncthreads();
  for (int u = tid; u <= Ub; u += 256) {
    const int l = u == 0 ? 0 : sl[u - 1], r = u == Ub ? Tb - 1 : sr[u];
    ok = ok && l <= r;
  }
  const int feasible = __syncthreads_and(ok);
  for (int u = tid; u < U1; u += 256) {
    const bool in = feasible && u <= Ub;
    L[(long)b * U1 + u] = in ? (u == 0 ? 0 : sl[u - 1]) : BAND_NONE_L;
    R[(long)b * U1 + u] = in ? (u == Ub ? Tb - 1 : sr[u]) : BAND_NONE_R;
  }
  if (tid == 0) feas[b] = feasible;
}

// ------------------------------------------------------------------------------------------------
// per-cell log-sum-exp, separable logits.  grid (ceil(T/32), ceil(U1/8), B), 256 threads = 32 t x 8 u
// W: a tile without a live cell only writes its -inf entries; in a live tile the threads of dead cells stage but do not sum
// ------------------------------------------------------------------------------------------------
constexpr int LSE_UT = 8, LSE_VC = 128;

template <bool W, bool KD, typename... WT>
__global__ void __launch_bounds__(256) lse_sep_kernel(const float* __restrict__ A, const float* __restrict__ C,
                                                      const float* __restrict__ bias, const int* __restrict__ labels,
                                                      int T, int U1, int V, int blank, long a_sb, long a_st,
                                                      long c_sb, long c_su, float* __restrict__ blk,
                                                      float* __restrict__ emit, WT... wt) {
  static_assert(sizeof...(WT) == (W ? 1 : 0) + (KD ? 1 : 0) && !(W && KD), "W = true takes one Win, KD = true one KdLse");
  const Win win = pick_tables<Win>(wt...);
  const KdLse kd = pick_tables<KdLse>(wt...);
  __shared__ float As[TT][LSE_VC + 1];
  __shared__ float Cs[LSE_UT][LSE_VC + 1];
  const int b = blockIdx.z, t0 = blockIdx.x * TT, u0 = blockIdx.y * LSE_UT;
  const int tid = threadIdx.x, tl = tid & 31, ul = tid >> 5;
  const int t = t0 + tl, u = u0 + ul;
  const float* Ab = A + (long)b * a_sb;
  const float* Cb = C + (long)b * c_sb;
  // KD: the cell's label entry (-1 where the row has no label: u >= u_lens[b]) and the second sum, without the blank and that entry
  int ykd = -1;
  float rs = 0.f;
  if (KD && u < U1 - 1 && u < kd.u_lens[b]) ykd = labels[(long)b * (U1 - 1) + u];
  bool live = true;
  if (W) {
    live = t < T && u < U1;
    if (live) live = t >= win.L[(long)b * U1 + u] && t <= win.R[(long)b * U1 + u];
    if (!__syncthreads_or(live)) {   // (uniform) no live cell in this tile
      if (t < T && u < U1) {
        const long o = ((long)b * U1 + u) * T + t;
        blk[o] = -__builtin_huge_valf();
        emit[o] = -__builtin_huge_valf();
      }
      return;
    }
  }

  float m = -__builtin_huge_valf(), s = 0.f;
  for (int v0 = 0; v0 < V; v0 += LSE_VC) {
    const int vc = min(LSE_VC, V - v0);
    __syncthreads();
    for (int i = tid; i < TT * LSE_VC; i += 256) {
      const int r = i / LSE_VC, c = i % LSE_VC;
      As[r][c] = (t0 + r < T && c < vc) ? Ab[(long)(t0 + r) * a_st + v0 + c] : 0.f;
    }
    for (int i = tid; i < LSE_UT * LSE_VC; i += 256) {
      const int r = i / LSE_VC, c = i % LSE_VC;
      Cs[r][c] = (u0 + r < U1 && c < vc) ? Cb[(long)(u0 + r) * c_su + v0 + c] + bias[v0 + c] : 0.f;
    }
    __syncthreads();
    if (W && !live) continue;   // (no barrier is skipped: both are above)
    float cm = -__builtin_huge_valf();
    for (int c = 0; c < vc; ++c) cm = fmaxf(cm, As[tl][c] + Cs[ul][c]);
    const float nm = fmaxf(m, cm);
    float cs = 0.f;
    if (KD) {   // the full sum as below (same order, same bits); the exponentials of the other entries go to the second sum too
      const int cb = blank - v0, cy = ykd - v0;
      float crs = 0.f;
      for (int c = 0; c < vc; ++c) {
        const float e = expf(As[tl][c] + Cs[ul][c] - nm);
        cs += e;
        crs += (c == cb || c == cy) ? 0.f : e;
      }
      rs = rs * expf(m - nm) + crs;
    } else {
      for (int c = 0; c < vc; ++c) cs += expf(As[tl][c] + Cs[ul][c] - nm);
    }
    s = s * expf(m - nm) + cs;
    m = nm;
  }
  if (t < T && u < U1) {
    const long o = ((long)b * U1 + u) * T + t;
    if (W && !live) {
      blk[o] = -__builtin_huge_valf();
      emit[o] = -__builtin_huge_valf();
      return;
    }
    const float lse = m + logf(s);
    const float zb = Ab[(long)t * a_st + blank] + Cb[(long)u * c_su + blank] + bias[blank];
    if (KD) kd.rest[o] = fmaxf(logf(rs) - logf(s), KD_REST_FLOOR);   // both sums are relative to the same maximum
    blk[o] = zb - lse;
    float e = 0.f;
    if (u < U1 - 1) {
      const int y = labels[(long)b * (U1 - 1) + u];
      e = Ab[(long)t * a_st + y] + Cb[(long)u * c_su + y] + bias[y] - lse;
    }
    if (W && u < U1 - 1 && u < win.u_lens[b] && (t < win.lo[(long)b * win.stride + u] || t > win.hi[(long)b * win.stride + u]))
      e = -__builtin_huge_valf();   // outside label u's window
    emit[o] = e;
  }
}


// ------------------------------------------------------------------------------------------------
// per-cell log-sum-exp for LARGE vocabularies (V >= 256: BASELINE configs[4], V = 2048).  Same outputs as lse_sep_kernel.
// lse_sep_kernel spends its time in ocml expf (~20 VALU instructions per element) and in two LDS reads per element; here a thread
// owns 4 label positions of one frame (every A value read from LDS feeds 4 cells), the chunk is staged pre-multiplied by log2(e) and
// the sum runs on v_exp_f32 (2^x): per element one add for the chunk maximum, then add + sub + v_exp_f32 + add.
// grid (ceil(T/32), ceil(U1/32), B), 256 threads = 32 t x 8 groups of 4 u.
// ------------------------------------------------------------------------------------------------
constexpr int LSV_UR = 4, LSV_UT = 8 * LSV_UR, LSV_VC = 128;
constexpr float LOG2E_F = 1.4426950408889634f, LN2_F = 0.6931471805599453f;

template <bool W, bool KD, typename... WT>
__global__ void __launch_bounds__(256) lse_sepv_kernel(const float* __restrict__ A, const float* __restrict__ C,
                                                       const float* __restrict__ bias, const int* __restrict__ labels,
                                                       int T, int U1, int V, int blank, long a_sb, long a_st,
                                                       long c_sb, long c_su, float* __restrict__ blk,
                                                       float* __restrict__ emit, WT... wt) {
  static_assert(sizeof...(WT) == (W ? 1 : 0) + (KD ? 1 : 0) && !(W && KD), "W = true takes one Win, KD = true one KdLse");
  const Win win = pick_tables<Win>(wt...);
  const KdLse kd = pick_tables<KdLse>(wt...);
  __shared__ float As[TT][LSV_VC + 1];
  __shared__ float Cs[LSV_UT][LSV_VC + 1];
  const int b = blockIdx.z, t0 = blockIdx.x * TT, u0 = blockIdx.y * LSV_UT;
  const int tid = threadIdx.x, tl = tid & 31, ug = tid >> 5;
  const int t = t0 + tl;
  const float* Ab = A + (long)b * a_sb;
  const float* Cb = C + (long)b * c_sb;
  bool live[LSV_UR], any = true;   // W: a thread sums when one of its four cells is live; a tile without a live cell only writes -inf
  if (W) {
    any = false;
#pragma unroll
    for (int r = 0; r < LSV_UR; ++r) {
      const int u = u0 + ug * LSV_UR + r;
      live[r] = t < T && u < U1;
      if (live[r]) live[r] = t >= win.L[(long)b * U1 + u] && t <= win.R[(long)b * U1 + u];
      any = any || live[r];
    }
    if (!__syncthreads_or(any)) {   // (uniform)
#pragma unroll
      for (int r = 0; r < LSV_UR; ++r) {
        const int u = u0 + ug * LSV_UR + r;
        if (t < T && u < U1) {
          const long o = ((long)b * U1 + u) * T + t;
          blk[o] = -__builtin_huge_valf();
          emit[o] = -__builtin_huge_valf();
        }
      }
      return;
    }
  }

  float m[LSV_UR], s[LSV_UR];   // running maximum (log2 domain) and sum of 2^(x - m)
#pragma unroll
  for (int r = 0; r < LSV_UR; ++r) { m[r] = -__builtin_huge_valf(); s[r] = 0.f; }
  int ykd[LSV_UR];   // KD: the cells' label entries (-1 where the row has no label) and the sums without the blank and that entry
  float rs[LSV_UR];
  if (KD) {
    const int Ub = kd.u_lens[b];
#pragma unroll
    for (int r = 0; r < LSV_UR; ++r) {
      const int u = u0 + ug * LSV_UR + r;
      ykd[r] = (u < U1 - 1 && u < Ub) ? labels[(long)b * (U1 - 1) + u] : -1;
      rs[r] = 0.f;
    }
  }
  for (int v0 = 0; v0 < V; v0 += LSV_VC) {
    const int vc = min(LSV_VC, V - v0);
    __syncthreads();
    for (int i = tid; i < TT * LSV_VC; i += 256) {
      const int r = i / LSV_VC, c = i % LSV_VC;
      As[r][c] = (t0 + r < T && c < vc) ? Ab[(long)(t0 + r) * a_st + v0 + c] * LOG2E_F : 0.f;
    }
    for (int i = tid; i < LSV_UT * LSV_VC; i += 256) {
      const int r = i / LSV_VC, c = i % LSV_VC;
      Cs[r][c] = (u0 + r < U1 && c < vc) ? (Cb[(long)(u0 + r) * c_su + v0 + c] + bias[v0 + c]) * LOG2E_F : 0.f;
    }
    __syncthreads();
    if (W && !any) continue;   // (no barrier is skipped: both are above)
    float cm[LSV_UR];
#pragma unroll
    for (int r = 0; r < LSV_UR; ++r) cm[r] = -__builtin_huge_valf();
    for (int c = 0; c < vc; ++c) {
      const float a = As[tl][c];
#pragma unroll
      for (int r = 0; r < LSV_UR; ++r) cm[r] = fmaxf(cm[r], a + Cs[ug * LSV_UR + r][c]);
    }
    float nm[LSV_UR], cs[LSV_UR];
#pragma unroll
    for (int r = 0; r < LSV_UR; ++r) { nm[r] = fmaxf(m[r], cm[r]); cs[r] = 0.f; }
    if (KD) {   // the full sums as below (same order, same bits); the exponentials of the other entries go to the second sums too
      const int cb = blank - v0;
      float crs[LSV_UR];
      int cy[LSV_UR];
#pragma unroll
      for (int r = 0; r < LSV_UR; ++r) { crs[r] = 0.f; cy[r] = ykd[r] - v0; }
      for (int c = 0; c < vc; ++c) {
        const float a = As[tl][c];
#pragma unroll
        for (int r = 0; r < LSV_UR; ++r) {
          const float e = __builtin_amdgcn_exp2f(a + Cs[ug * LSV_UR + r][c] - nm[r]);
          cs[r] += e;
          crs[r] += (c == cb || c == cy[r]) ? 0.f : e;
        }
      }
#pragma unroll
      for (int r = 0; r < LSV_UR; ++r) rs[r] = rs[r] * __builtin_amdgcn_exp2f(m[r] - nm[r]) + crs[r];
    } else {
      for (int c = 0; c < vc; ++c) {
        const float a = As[tl][c];
#pragma unroll
        for (int r = 0; r < LSV_UR; ++r) cs[r] += __builtin_amdgcn_exp2f(a + Cs[ug * LSV_UR + r][c] - nm[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < LSV_UR; ++r) {
      s[r] = s[r] * __builtin_amdgcn_exp2f(m[r] - nm[r]) + cs[r];   // (first chunk: s = 0, 2^-inf = 0)
      m[r] = nm[r];
    }
  }
#pragma unroll
  for (int r = 0; r < LSV_UR; ++r) {
    const int u = u0 + ug * LSV_UR + r;
    if (t < T && u < U1) {
      const long o = ((long)b * U1 + u) * T + t;
      if (W && !live[r]) {
        blk[o] = -__builtin_huge_valf();
        emit[o] = -__builtin_huge_valf();
        continue;
      }
      const float lse = (m[r] + __builtin_amdgcn_logf(s[r])) * LN2_F;   // v_log_f32 = log2
      const float zb = Ab[(long)t * a_st + blank] + Cb[(long)u * c_su + blank] + bias[blank];
      if (KD) kd.rest[o] = fmaxf((__builtin_amdgcn_logf(rs[r]) - __builtin_amdgcn_logf(s[r])) * LN2_F, KD_REST_FLOOR);
      blk[o] = zb - lse;
      float e = 0.f;
      if (u < U1 - 1) {
        const int y = labels[(long)b * (U1 - 1) + u];
        e = Ab[(long)t * a_st + y] + Cb[(long)u * c_su + y] + bias[y] - lse;
      }
      if (W && u < U1 - 1 && u < win.u_lens[b] && (t < win.lo[(long)b * win.stride + u] || t > win.hi[(long)b * win.stride + u]))
        e = -__builtin_huge_valf();   // outside label u's window
      emit[o] = e;
    }
  }
}

// dense logits (B,T,U1,V): one wavefront per cell, lanes along v, grid-stride over cells
template <typename TZ, bool W, typename... WT>
__global__ void __launch_bounds__(256) lse_dense_kernel(const TZ* __restrict__ Z, const int* __restrict__ labels,
                                                        int B, int T, int U1, int V, int blank,
                                                        float* __restrict__ blk, float* __restrict__ emit, WT... wt) {
  static_assert(sizeof...(WT) == (W ? 1 : 0), "W = true takes one Win");
  const Win win = pick_tables<Win>(wt...);
  const int lane = threadIdx.x & 63;
  const long ncell = (long)B * T * U1;
  const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((long)gridDim.x * blockDim.x) >> 6;
  for (long cell = wave0; cell < ncell; cell += nw) {
    if (W) {   // a cell outside the band: -inf entries, its logits are not read
      const int u = (int)(cell % U1);
      const long bt = cell / U1;
      const int t = (int)(bt % T), b = (int)(bt / T);
      if (t < win.L[(long)b * U1 + u] || t > win.R[(long)b * U1 + u]) {
        if (lane == 0) {
          const long o = ((long)b * U1 + u) * T + t;
          blk[o] = -__builtin_huge_valf();
          emit[o] = -__builtin_huge_valf();
        }
        continue;
      }
    }
    const TZ* z = Z + cell * V;
    float m = -__builtin_huge_valf();
    for (int v = lane; v < V; v += 64) m = fmaxf(m, ldf(z, v));
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(ldf(z, v) - m);
    s = wave_sum(s);
    if (lane == 0) {
      const int u = (int)(cell % U1);
      const long bt = cell / U1;
      const int t = (int)(bt % T), b = (int)(bt / T);
      const float lse = m + logf(s);
      const long o = ((long)b * U1 + u) * T + t;
      blk[o] = ldf(z, blank) - lse;
      float e = (u < U1 - 1) ? ldf(z, labels[(long)b * (U1 - 1) + u]) - lse : 0.f;
      if (W && u < U1 - 1 && u < win.u_lens[b] && (t < win.lo[(long)b * win.stride + u] || t > win.hi[(long)b * win.stride + u]))
        e = -__builtin_huge_valf();   // outside label u's window
      emit[o] = e;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// alpha / beta: one wavefront per (b, which).  fp64 accumulation, fp32 correction term.
// (logaddexp_d, the DPP hand-off shfl_up1 / shfl_down1, PF and AB_RSRC / AB_OOB are in lattice_shared.hpp, shared with ctc.hip)
// ------------------------------------------------------------------------------------------------
// The sweep is a chain of ~T + U dependent steps (one anti-diagonal each).  Every memory operation of the loop goes through a buffer
// resource with an out-of-range offset for lanes / steps that have no cell (loads return 0, stores are dropped): the loop body has NO
// branch around a memory operation, so hipcc counts how many younger operations may stay in flight when it waits for a ring slot
// (`s_waitcnt vmcnt(n)`, n > 0).  With the loads and stores inside `if (cell exists)` branches — the round-1 form — it could not, fell
// back to vmcnt(0) after every step and each step waited out the loads it had just issued for 8 steps later: 950 cycles per step at
// config 2 (0.41 ms per training step for a 1 040-step chain) against the ~300 the arithmetic takes.
//
// The semiring is the template flag MAX.  MAX = false, the loss: the (logaddexp, +) sums above, both directions picked by blockIdx.y,
// every cell stored in fp64, logZ of each direction to ll; the lengths are taken as they come (the loss's check is the caller's).
// MAX = true, forced alignment: the alpha direction alone (grid (B, 1); the beta branch is not compiled) in the (max, +) semiring,
//   v(t,u) = max( v(t-1,u) + blk(t-1,u), v(t,u-1) + emit(t,u-1) ),  v(0,0) = 0,  score = v(Tb-1,Ub) + blk(Tb-1,Ub)  -> ll[b]
// fp64 sums of the fp32 cell terms, no transcendental: the score is exact (-inf when the utterance has no frame).  TIE RULE: on
// exactly equal candidates the blank predecessor (t-1,u) wins (the label predecessor is taken only when it is strictly greater), so
// the path is a pure function of blk / emit.  Back-pointers in place of the cell store: ONE BIT per cell (1 = came from (t,u-1),
// i.e. label u-1 is emitted at frame t), 32 consecutive frames of one label row per word: bp[b][u][t >> 5] bit (t & 31).  A lane
// collects the bits of its K rows in registers and stores a word when its row reaches the end of a 32-frame block or the
// utterance's last frame; like every memory operation of the loop the store goes through the buffer resource with an out-of-range
// offset when there is nothing to store.  The lengths are the caller's: CLAMPED into the lattice (as backtrace_kernel clamps them),
// so a wrong length can neither reach another label row through u * T + t nor leave the score unwritten.
// The MAX instance has no alpha / beta to write, so the two kernel arguments before ll are its table instead: the words per label
// row and bp[B][U1][NW].  (Left unused beside a table of their own they cost the K = 2 instance 0.8 % of its time at config-5
// size: same loop, other registers.  As below each mode compiles to the instructions it had as a kernel of its own:
// profiles/lattice_sweeps_resource_usage.txt.)
template <bool MAX> using SweepOut0 = std::conditional_t<MAX, int, double* __restrict__>;                        // alpha | NW
template <bool MAX> using SweepOut1 = std::conditional_t<MAX, unsigned* __restrict__, double* __restrict__>;   // beta  | bp

template <int K, bool MAX = false>
__global__ void __launch_bounds__(64) alphabeta_kernel(const float* __restrict__ blk, const float* __restrict__ emit,
                                                       const int* __restrict__ t_lens, const int* __restrict__ u_lens,
                                                       int T, int U1, SweepOut0<MAX> alpha, SweepOut1<MAX> beta,
                                                       double* __restrict__ ll) {
  const int b = blockIdx.x, which = MAX ? 0 : blockIdx.y, lane = threadIdx.x;
  // valid cells: t < Tb, u <= Ub
  const int Tb = MAX ? min(t_lens[b], T) : t_lens[b], Ub = MAX ? max(min(u_lens[b], U1 - 1), 0) : u_lens[b];
  const long rowbase = (long)b * U1 * T;
  const int ulo = lane * K;
  const int lastlane = Ub / K;
  const int nsteps = Tb + lastlane;
  const int cells = U1 * T;
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(blk + rowbase), 0, cells * 4, AB_RSRC);
  const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(emit + rowbase), 0, cells * 4, AB_RSRC);
  // what the sweep writes: the cells of alpha | beta, or (MAX) the utterance's back-pointer words
  [[maybe_unused]] int NW = 0;
  __amdgpu_buffer_rsrc_t ro;
  if constexpr (MAX) {
    NW = alpha;
    ro = __builtin_amdgcn_make_buffer_rsrc(beta + (long)b * U1 * NW, 0, U1 * NW * 4, AB_RSRC);
  } else {
    ro = __builtin_amdgcn_make_buffer_rsrc((which == 0 ? alpha : beta) + rowbase, 0, cells * 8, AB_RSRC);
  }
  auto cell = [&](int u, int t) -> int { return (t >= 0 && t < Tb && u <= Ub) ? u * T + t : -1; };
  auto ld = [&](const __amdgpu_buffer_rsrc_t& r, int c) -> float {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, c >= 0 ? c * 4 : AB_OOB, 0, 0));
  };
  auto st = [&](double v, int c) {
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(i32x2, v), ro, c >= 0 ? c * 8 : AB_OOB, 0, 0);
  };
  auto stw = [&](unsigned v, int w) { __builtin_amdgcn_raw_buffer_store_b32((int)v, ro, w >= 0 ? w * 4 : AB_OOB, 0, 0); };
  const int nrounds = (nsteps + PF - 1) / PF;   // steps beyond nsteps touch no cell (every lane is past its last row)
  double llv = NEG_INF;

  if (which == 0) {
    double down[K];  // alpha[t-1][u] + blk[t-1][u]
    [[maybe_unused]] unsigned bits[K];  // MAX: back-pointer bits of the current 32-frame block of row ulo + k
#pragma unroll
    for (int k = 0; k < K; ++k) { down[k] = NEG_INF; bits[k] = 0u; }
    double eout = NEG_INF;  // alpha[t][uhi] + emit[t][uhi] of this lane's last cell at its current row
    // a row's blk/emit values are fetched PF steps ahead into a register ring
    float pb[PF][K], pe[PF][K];
#pragma unroll
    for (int j = 0; j < PF; ++j)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int c = cell(ulo + k, j - lane);
        pb[j][k] = ld(rb, c);
        pe[j][k] = ld(re, c);
      }
    for (int r = 0; r < nrounds; ++r) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const int t = r * PF + j - lane;
        const double carry = shfl_up1(eout, lane);
        float cb[K], ce[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { cb[k] = pb[j][k]; ce[k] = pe[j][k]; }
        // refill this ring slot with the row of step n + PF
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int c = cell(ulo + k, t + PF);
          pb[j][k] = ld(rb, c);
          pe[j][k] = ld(re, c);
        }
        const bool row = t >= 0 && t < Tb;
        const int sh = t & 31;
        const bool flush = sh == 31 || t == Tb - 1;
        double left = carry;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int u = ulo + k;
          const bool ok = row && u <= Ub;
          double a;
          if constexpr (MAX) {
            const bool from_label = left > down[k];   // strict: a tie keeps the blank predecessor; (0,0) and u = 0 see left = -inf
            a = (t == 0 && u == 0) ? 0.0 : (from_label ? left : down[k]);
            const unsigned nb = (sh == 0 ? 0u : bits[k]) | ((unsigned)from_label << sh);
            bits[k] = ok ? nb : bits[k];
            stw(nb, (ok && flush) ? u * NW + (t >> 5) : -1);
          } else {
            a = (t == 0 && u == 0) ? 0.0 : logaddexp_d(down[k], left);
            st(a, ok ? u * T + t : -1);
          }
          const double nd = a + (double)cb[k];
          down[k] = ok ? nd : down[k];
          left = ok ? ((u < Ub) ? a + (double)ce[k] : NEG_INF) : left;
          llv = (ok && t == Tb - 1 && u == Ub) ? nd : llv;
        }
        eout = row ? left : eout;
      }
    }
    if (lane == lastlane) ll[b] = llv;   // the lane that owns cell (Tb - 1, Ub): logZ, or (MAX) the best path's score
  } else if constexpr (!MAX) {
    double down[K];  // beta[t+1][u]
#pragma unroll
    for (int k = 0; k < K; ++k) down[k] = NEG_INF;
    double bout = NEG_INF;  // beta[t][ulo] of this lane's first cell at its current row
    // lane l at step n handles t = Tb-1 - (n - (lastlane - l)); lanes > lastlane own no valid cell
    float pb[PF][K], pe[PF][K];
#pragma unroll
    for (int j = 0; j < PF; ++j)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int c = cell(ulo + k, Tb - 1 - (j - (lastlane - lane)));
        pb[j][k] = ld(rb, c);
        pe[j][k] = ld(re, c);
      }
    for (int r = 0; r < nrounds; ++r) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const int t = Tb - 1 - (r * PF + j - (lastlane - lane));
        const double carry = shfl_down1(bout, lane);  // beta[t][(lane+1)*K]
        float cb[K], ce[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { cb[k] = pb[j][k]; ce[k] = pe[j][k]; }
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int c = cell(ulo + k, t - PF);
          pb[j][k] = ld(rb, c);
          pe[j][k] = ld(re, c);
        }
        const bool row = t >= 0 && t < Tb && lane <= lastlane;
        double right = carry;  // beta[t][u+1]
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {
          const int u = ulo + k;
          const bool ok = row && u <= Ub;
          const double ne = down[k] == NEG_INF ? NEG_INF : down[k] + (double)cb[k];
          const double em = (u < Ub && right != NEG_INF) ? right + (double)ce[k] : NEG_INF;
          const double v = (t == Tb - 1 && u == Ub) ? (double)cb[k] : logaddexp_d(ne, em);
          st(v, ok ? u * T + t : -1);
          down[k] = ok ? v : down[k];
          right = ok ? v : right;
          llv = (ok && t == 0 && u == 0) ? v : llv;
        }
        bout = row ? right : bout;
      }
    }
    if (lane == 0) ll[gridDim.x + b] = llv;   // the lane that owns cell (0, 0)
  }
}

// Back-trace from (Tb-1, Ub) to label row 0: one workgroup per utterance.  A zero word (below the current frame) is 32 blank steps
// at once, a set bit is found by a leading-zero count: about U + T/32 dependent loads instead of T + U.  The utterance's part of the
// table is first copied to LDS (coalesced) when the whole table of the call fits there; otherwise the walk reads the workspace.
// frames[b][u] = frame at which label u is emitted (u < Ub), -1 beyond (and everywhere when the utterance has no frame).
__global__ void __launch_bounds__(256) backtrace_kernel(const unsigned* __restrict__ bp, const int* __restrict__ t_lens,
                                                        const int* __restrict__ u_lens, int T, int U1, int NW, int in_lds,
                                                        int* __restrict__ frames) {
  extern __shared__ unsigned bt_tab[];
  const int b = blockIdx.x, tid = threadIdx.x, U = U1 - 1;
  const int Tb = min(t_lens[b], T), Ub = max(min(u_lens[b], U), 0);   // (lengths are the caller's: clamped so no access leaves the row)
  int* fr = frames + (long)b * U;
  const int nlab = Tb >= 1 ? Ub : 0;   // labels that receive a frame
  for (int i = nlab + tid; i < U; i += 256) fr[i] = -1;
  if (nlab == 0) return;   // (uniform)
  const unsigned* tp = bp + (long)b * U1 * NW;
  int stride = NW;
  if (in_lds) {
    const int nwb = ((Tb - 1) >> 5) + 1;   // words per row this utterance wrote
    for (int i = tid; i < (Ub + 1) * nwb; i += 256) bt_tab[i] = tp[(i / nwb) * NW + i % nwb];
    __syncthreads();
    tp = bt_tab;
    stride = nwb;
  }
  if (tid != 0) return;
  int t = Tb - 1, u = Ub;
  while (u > 0 && t >= 0) {
    const unsigned w = tp[u * stride + (t >> 5)] & (0xffffffffu >> (31 - (t & 31)));   // frames <= t of the block
    if (w == 0u) {
      t = (t & ~31) - 1;
    } else {
      t = (t & ~31) + 31 - __clz(w);
      fr[--u] = t;
    }
  }
  while (u > 0) fr[--u] = -1;   // (only with -inf cell terms: no finite path)
}

// ------------------------------------------------------------------------------------------------
// per-cell scalars for the gradient: occupancy w, row lse, blank- and label-transition posteriors
// ------------------------------------------------------------------------------------------------
struct CellS {
  float w, lse, cb, ce;
};

__device__ __forceinline__ CellS cell_scalars(const float* __restrict__ blk, const float* __restrict__ emit,
                                              const double* __restrict__ alpha, const double* __restrict__ beta,
                                              long rowbase, int T, int t, int u, int Tb, int Ub, double logZ,
                                              float zblank) {
  // (t, u) must be a cell of the lattice (t < Tb, u <= Ub).  All six loads are unconditional — the neighbours' indices are clamped
  // to the cell itself where the lattice ends and the value is dropped by a select — so a caller that builds several cells per thread
  // gets its loads issued back to back instead of one dependent round trip per `if`.
  CellS c;
  const long o = rowbase + (long)u * T + t;
  const bool last_t = t == Tb - 1, has_label = u < Ub;
  const double a = alpha[o], bt = beta[o];
  const double b_next_t = beta[last_t ? o : o + 1], b_next_u = beta[has_label ? o + T : o];
  const float lb = blk[o], le = emit[o];
  c.w = expf((float)(a + bt - logZ));
  c.lse = zblank - lb;
  const double tb = last_t ? ((u == Ub) ? a + (double)lb - logZ : NEG_INF) : a + (double)lb + b_next_t - logZ;
  c.cb = expf((float)tb);
  c.ce = has_label ? expf((float)(a + (double)le + b_next_u - logZ)) : 0.f;
  return c;
}

// FastEmit (include/rnnt_hip.h): the gradient with respect to the LABEL log-probability of every cell is scaled by
// (1 + lambda), the blank's is left alone, and the result goes through the log-softmax exactly:
//   dz[v] = softmax_v (w + lambda ce) - [v = blank] cb - [v = y_u] (1 + lambda) ce          (sum over v: still 0)
// i.e. the plain kernels' arithmetic on two changed per-cell scalars.  Every gradient kernel has a template flag FE: the FE = false
// instance is the code without this feature (lambda is never read), FE = true applies fastemit_cell where the scalars are made.
// A cell without a label transition (ce = 0: u = U_b) keeps its scalars bit for bit.
__device__ __forceinline__ void fastemit_cell(CellS& c, float lambda) {
  c.w = c.w + lambda * c.ce;
  c.ce = (1.f + lambda) * c.ce;
}

// Lattice distillation in the gradient kernels (KD = true).  With p the student's softmax of a cell, (a, c, r) the
// teacher's collapsed probabilities (blank, label, rest), (p_b, p_y, p_r) the student's and rho = r / p_r = exp(rest_T - rest_S),
//   d KL / dz[v] = p[v] (1 - rho) - [v = blank] (a - rho p_b) - [v = y_u] (c - rho p_y)
// which is again the plain kernels' arithmetic on changed per-cell scalars.  The two upstream gradients of a row (gn for the NLL,
// gk for the KD term; either may be 0) enter the scalars here and the kernels' final scale is 1.  In fp32 the three-scalar form
// cancels on the blank and label entries once rho is large (a peaked student: p[v] (1 - rho) + rho p_b against the p_b - a it should
// leave), so the KD instances split the work: the inner loops see those two entries of a cell with a logit that sends the
// exponential to 0 (kd_mask: they add exact zeros), and the cell's cb / ce slots carry the two entries COMPLETE,
//   cb <- gn (cb - w p_b) + gk (a - p_b)            ce <- gn (ce - w p_y) + gk (c - p_y)   (0 without a label: u = U_b)
// while every other entry is one product with w <- gn w + gk (1 - rho), of size at most gn + gk (p[v] rho <= r <= 1).
// rest_S >= KD_REST_FLOOR and the exponent is capped, so rho (and w) stay finite; a teacher class of probability 0 (-inf) is fine.
__device__ __forceinline__ void kd_cell(CellS& c, const KdGrad& kd, long o, float lb, float le, bool has_label, float gn, float gk) {
  const float pb = expf(lb), py = has_label ? expf(le) : 0.f;
  const float a = expf(kd.t_blk[o]), cl = has_label ? expf(kd.t_emit[o]) : 0.f;
  const float rho = expf(fminf(kd.t_rest[o] - kd.rest[o], 85.f));
  c.cb = gn * (c.cb - c.w * pb) + gk * (a - pb);
  c.ce = has_label ? gn * (c.ce - c.w * py) + gk * (cl - py) : 0.f;
  c.w = gn * c.w + gk * (1.f - rho);
}
constexpr float KD_MASKED = -1e30f;   // the logit of an entry the inner loop must not see: exp(x - lse) = 0

// Emission windows in the gradient kernels (W = true): [ua, ub] = the label positions u <= Ub whose band [L[u], R[u]] meets the
// frames [t0, t0 + TT) of this tile.  L and R are non-decreasing in u, so these positions are one interval; empty: ua > ub.
// Called by every thread of the workgroup (two barriers).
__device__ __forceinline__ void tile_band(const int* __restrict__ wL, const int* __restrict__ wR, int t0, int Ub, int tid,
                                          int nthreads, int* band, int& ua, int& ub) {
  if (tid == 0) { band[0] = BAND_NONE_L; band[1] = -1; }
  __syncthreads();
  for (int u = tid; u <= Ub; u += nthreads)
    if (wL[u] <= t0 + TT - 1 && wR[u] >= t0) {
      atomicMin(&band[0], u);
      atomicMax(&band[1], u);
    }
  __syncthreads();
  ua = band[0];
  ub = band[1];
}
constexpr float DEAD_LSE = 1e30f;   // the lse of a cell outside the band: exp(x - lse) = 0

// grid (ceil(T/32), B), 256 threads; wave w owns frames w, w+4, ... of the tile; lanes run along v.
// dynamic LDS: cells[TT][U1] (CellS) | Cs[U1][64] | dCs[U1][64] | ys[U1]
// W: the u loop runs over the chunks of 8 (aligned as without windows, so that full windows keep every sum's order) that meet the
// tile's interval; a dead cell inside them adds exact zeros, with no branch in the inner loop (a per-cell skip measured 1.9x slower
// with full windows: it serialises the table reads)
// KD: kd_cell where the scalars are made, kd_mask on the staged C values of a cell's blank and label entries, no final scale
template <bool FE, bool W, bool KD, typename... WT>
__global__ void __launch_bounds__(256) grad_sep_kernel(const float* __restrict__ A, const float* __restrict__ C,
                                                       const float* __restrict__ bias, const int* __restrict__ labels,
                                                       const int* __restrict__ t_lens, const int* __restrict__ u_lens,
                                                       const float* __restrict__ blk, const float* __restrict__ emit,
                                                       const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const double* __restrict__ ll, int T, int U1, int V, int blank,
                                                       long a_sb, long a_st, long c_sb, long c_su, float gscale_in,
                                                       const float* __restrict__ gvec, int gvec_stride,
                                                       float* __restrict__ dA, float* __restrict__ dCp, float fe_lambda,
                                                       WT... wt) {
  static_assert(sizeof...(WT) == (W ? 1 : 0) + (KD ? 1 : 0) && !(W && KD), "W = true takes one Band, KD = true one KdGrad");
  const Band bt = pick_tables<Band>(wt...);
  const KdGrad kd = pick_tables<KdGrad>(wt...);
  const int *wL = bt.L, *wR = bt.R;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  CellS* cells = reinterpret_cast<CellS*>(smem);
  float* Cs = reinterpret_cast<float*>(cells + TT * U1);
  float* dCs = Cs + U1 * 64;
  int* ys = reinterpret_cast<int*>(dCs + U1 * 64);

  const int b = blockIdx.y, tile = blockIdx.x, t0 = tile * TT, ntiles = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = t_lens[b], Ub = u_lens[b];
  const long rowbase = (long)b * U1 * T;
  const double logZ = ll[b];
  const float gscale = gvec ? gscale_in * gvec[(long)b * gvec_stride] : gscale_in;  // upstream gradient per utterance (stride 0: one scalar)
  const float* Ab = A + (long)b * a_sb;
  const float* Cb = C + (long)b * c_sb;
  float* dCtile = dCp + ((long)b * ntiles + tile) * U1 * V;

  int ua = 0, ub = Ub;
  if (W) {
    __shared__ int band[2];
    wL += (long)b * U1;
    wR += (long)b * U1;
    tile_band(wL, wR, t0, Ub, tid, 256, band, ua, ub);
  }

  // (KD: a position without a label transition, u >= Ub, has no label entry: -1, so kd_mask leaves that entry to the inner loop)
  for (int i = tid; i < U1; i += 256) ys[i] = (i < U1 - 1 && (!KD || i < Ub)) ? labels[(long)b * (U1 - 1) + i] : -1;
  const float gk = KD ? (kd.kvec ? kd.kscale * kd.kvec[(long)b * kd.kstride] : kd.kscale) : 0.f;
  for (int i = tid; i < TT * U1; i += 256) {
    const int u = i / TT, tl = i % TT, t = t0 + tl;   // consecutive threads -> consecutive frames: alpha / beta / blk / emit rows are read coalesced
    CellS c = {0.f, W ? DEAD_LSE : 0.f, 0.f, 0.f};
    if (t < Tb && u <= Ub && (!W || (t >= wL[u] && t <= wR[u]))) {
      const float zb = Ab[(long)t * a_st + blank] + Cb[(long)u * c_su + blank] + bias[blank];
      c = cell_scalars(blk, emit, alpha, beta, rowbase, T, t, u, Tb, Ub, logZ, zb);
      if (FE) fastemit_cell(c, fe_lambda);
      if (KD) {
        const long o = rowbase + (long)u * T + t;
        kd_cell(c, kd, o, blk[o], emit[o], u < Ub, gscale, gk);
      }
    }
    cells[tl * U1 + u] = c;
  }

  for (int v0 = 0; v0 < V; v0 += 64) {
    const int v = v0 + lane;
    const bool vok = v < V;
    __syncthreads();  // cells/ys ready (first pass); previous chunk's dCs flushed (later passes)
    for (int i = tid; i < U1 * 64; i += 256) {
      const int u = i >> 6, c = i & 63;
      Cs[i] = (v0 + c < V) ? Cb[(long)u * c_su + v0 + c] + bias[v0 + c] : 0.f;
      dCs[i] = 0.f;
    }
    __syncthreads();
    // A wave owns the frames tl = wave + 4*i (i < TT/4) of the tile and walks u in chunks of UC: dA of a frame (sum over
    // u) and dC of a label position (sum over the wave's frames) both accumulate in REGISTERS; the LDS adds that merge the
    // four waves' dC happen once per (u, wave) instead of once per (u, frame) -- 8x fewer, and they were the kernel's
    // bottleneck at large V (c5: V = 2048) -- and in a fixed order.
    constexpr int NF = TT / 4, UC = 8;
    float a[NF], accA[NF];
    bool fok[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int t = t0 + wave + 4 * i;
      fok[i] = t < Tb && vok;
      a[i] = fok[i] ? Ab[(long)t * a_st + v] : 0.f;
      accA[i] = 0.f;
    }
    for (int u0 = W ? (ua & ~(UC - 1)) : 0; u0 <= (W ? ub : Ub); u0 += UC) {
      float accC[UC], cs[UC];
      int yv[UC];
#pragma unroll
      for (int j = 0; j < UC; ++j) {
        const int u = min(u0 + j, U1 - 1);
        accC[j] = 0.f;
        cs[j] = Cs[u * 64 + lane];
        yv[j] = ys[u];
        if (KD && (v == blank || v == yv[j])) cs[j] = KD_MASKED;
      }
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        if (!fok[i]) continue;
        const CellS* crow = cells + (wave + 4 * i) * U1;
#pragma unroll
        for (int j = 0; j < UC; ++j) {
          const int u = u0 + j;
          if (u > Ub) break;
          const CellS c = crow[u];   // (W: a dead cell has w = cb = ce = 0 and an lse that sends the exponential to 0: g = 0 exactly)
          // v_exp_f32 form: |rel err| <~ 3e-7 on a value in [0, 1] (the softmax probability times a path weight <= 1), i.e. an
          // absolute gradient error ~1e-7 against the 2e-5 the tests allow; ocml expf was 2/3 of this loop's instructions
          float g = c.w * __expf(a[i] + cs[j] - c.lse);
          if (v == blank) g -= c.cb;
          if (v == yv[j]) g -= c.ce;
          accA[i] += g;
          accC[j] += g;
        }
      }
      // merge the four waves' sums in wave order: fixed order -> the step is bitwise reproducible (LDS float atomics were not);
      // u0 / Ub are uniform over the workgroup, so every wave meets every barrier
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (wave == w && vok) {
#pragma unroll
          for (int j = 0; j < UC; ++j)
            if (u0 + j <= Ub) dCs[(u0 + j) * 64 + lane] += accC[j];
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int t = t0 + wave + 4 * i;
      if (t < T && vok) dA[(long)b * a_sb + (long)t * a_st + v] = KD ? accA[i] : accA[i] * gscale;
    }
    __syncthreads();
    for (int i = tid; i < U1 * 64; i += 256) {
      const int u = i >> 6, c = i & 63;
      if (v0 + c < V) dCtile[(long)u * V + v0 + c] = dCs[i];
    }
  }
}


// ------------------------------------------------------------------------------------------------
// lattice gradient for LARGE vocabularies (V >= 256).  Same outputs as grad_sep_kernel (dA, per-tile dC slabs for reduce_dc_kernel).
// grad_sep_kernel keeps the whole vocabulary loop inside one workgroup per (utterance, 32-frame tile): 82 KB of LDS (one workgroup of
// 4 waves per CU), four barriers and an LDS merge of the waves' dC sums per 8 label positions and 64-entry vocabulary chunk — at
// V = 2048 it ran 5.6 ms for 4 G elements (profiles/r02_final_bench_c5.log), 7x off the v_exp_f32 rate.  Here the vocabulary is a
// GRID dimension and a LANE owns one vocabulary entry v for the whole tile: dA[t][v] (sum over u) and dC[u][v] (sum over the tile's
// frames) are both plain register sums of that lane — no cross-lane or cross-wave merge, no barrier after the cell table is built,
// LDS holds the per-cell scalars only (read as broadcasts).  The blank / label corrections leave the inner loop: the one wave whose
// 64 entries contain the blank (a label) subtracts them in a second, exp-free pass.  Arithmetic per element: two adds, v_exp_f32
// (2^x on operands pre-multiplied by log2 e), one multiply, two accumulations.
// grid (ceil(T/32), ceil(V / (64 NW)), B), 64 NW threads; dynamic LDS: cells[TT][UL] (CellS, lse in the log2 domain) | ys[U1]
// CHUNKED = false: UL = U1, the whole table at once (every U+1 whose table fits in LDS: 516 (U+1) bytes <= 160 KiB, U+1 <= 317).
// CHUNKED = true : the table holds UL (a multiple of UC) label positions at a time and is rebuilt per chunk; accA keeps accumulating
// in registers across the chunks and the dC rows are written per 8-row block as before, so the arithmetic (and its order) is the
// unchunked kernel's.  Every wave stays to the end (the chunks' barriers), the ones beyond the vocabulary only help build the table.
// W (emission windows): cells outside the band enter the table as cells outside the lattice do (exact zeros), and an 8-row block
// that does not meet the tile's interval [ua, ub] skips its 32 x 8 x 64 exponentials and stores its zero dC rows.
// KD (lattice distillation): kd_cell where the scalars are made, the masked logit in cs2 for a cell's blank and label entries (set
// per 8-row block, outside the inner loop), whose complete values the correction pass then subtracts as it subtracts cb / ce; no final scale.
// ------------------------------------------------------------------------------------------------
template <int NW, bool CHUNKED, bool FE, bool W, bool KD, typename... WT>
__global__ void __launch_bounds__(64 * NW, 3) grad_sepv_kernel(const float* __restrict__ A, const float* __restrict__ C,
                                                            const float* __restrict__ bias, const int* __restrict__ labels,
                                                            const int* __restrict__ t_lens, const int* __restrict__ u_lens,
                                                            const float* __restrict__ blk, const float* __restrict__ emit,
                                                            const double* __restrict__ alpha, const double* __restrict__ beta,
                                                            const double* __restrict__ ll, int T, int U1, int V, int blank,
                                                            long a_sb, long a_st, long c_sb, long c_su, float gscale_in,
                                                            const float* __restrict__ gvec, int gvec_stride,
                                                            float* __restrict__ dA, float* __restrict__ dCp, int ul,
                                                            float fe_lambda, WT... wt) {
  static_assert(sizeof...(WT) == (W ? 1 : 0) + (KD ? 1 : 0) && !(W && KD), "W = true takes one Band, KD = true one KdGrad");
  const Band bt = pick_tables<Band>(wt...);
  const KdGrad kd = pick_tables<KdGrad>(wt...);
  const int *wL = bt.L, *wR = bt.R;
  const int UL = CHUNKED ? ul : U1;                      // label positions per table
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* wl = reinterpret_cast<float2*>(smem);          // [TT][UL] {occupancy w, row lse * log2 e}: what the inner loop reads (8-byte broadcasts)
  float2* cbe = wl + TT * UL;                            // [TT][UL] {P(blank transition), P(label transition)}: the correction pass
  int* ys = reinterpret_cast<int*>(cbe + TT * UL);       // [U1]

  const int b = blockIdx.z, tile = blockIdx.x, t0 = tile * TT, ntiles = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int vw0 = (blockIdx.y * NW + wave) * 64;     // first vocabulary entry of this wave
  const int v = vw0 + lane;
  const bool vok = v < V;
  const int Tb = t_lens[b], Ub = u_lens[b];
  const int Tbc = max(Tb, 1);                         // t_lens[b] = 0 (no cell): the table's clamped loads stay at frame 0 of the row
  const long rowbase = (long)b * U1 * T;
  const double logZ = ll[b];
  const float gscale = gvec ? gscale_in * gvec[(long)b * gvec_stride] : gscale_in;
  const float* Ab = A + (long)b * a_sb;
  const float* Cb = C + (long)b * c_sb;
  float* dCtile = dCp + ((long)b * ntiles + tile) * U1 * V;
  const int nf = max(0, min(TT, Tb - t0));            // valid frames of this tile (uniform)
  int ua = 0, ub = Ub;
  if (W) {
    __shared__ int band[2];
    wL += (long)b * U1;
    wR += (long)b * U1;
    tile_band(wL, wR, t0, Ub, tid, 64 * NW, band, ua, ub);
  }

  // (KD: a position without a label transition, u >= Ub, has no label entry: -1)
  for (int i = tid; i < U1; i += 64 * NW) ys[i] = (i < U1 - 1 && (!KD || i < Ub)) ? labels[(long)b * (U1 - 1) + i] : -1;
  const float gk = KD ? (kd.kvec ? kd.kscale * kd.kvec[(long)b * kd.kstride] : kd.kscale) : 0.f;
  const float bias_blank = bias[blank];
  float a2[TT], accA[TT];
  const bool has_blank = blank >= vw0 && blank < vw0 + 64;   // uniform over the wave
  constexpr int UC = 8;
  for (int uc0 = 0; uc0 < U1; uc0 += UL) {
    const int nrow = min(UL, U1 - uc0);                  // label positions uc0 .. uc0 + nrow - 1 in this table
    if (uc0 > 0) __syncthreads();                        // every wave is done with the previous chunk's table
    // the cell table: four cells per thread and round, every load unconditional (indices clamped into the lattice, results dropped by
    // selects) so that the 4 x 8 loads of a round are in flight together; consecutive threads -> consecutive frames (coalesced rows)
    for (int i0 = tid; i0 < TT * nrow; i0 += 64 * NW * 4) {
      CellS c[4];
      bool in[4];
      int dst[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * 64 * NW;
        const int u = min(uc0 + i / TT, U1 - 1), tl = i % TT, t = t0 + tl;
        in[q] = i < TT * nrow && t < Tb && u <= Ub;
        if (W) in[q] = in[q] && t >= wL[u] && t <= wR[u];   // (u <= U1 - 1: inside the tables)
        dst[q] = i < TT * nrow ? tl * UL + (u - uc0) : -1;
        const int tc = min(t, Tbc - 1), uc = max(min(u, Ub), 0);   // a cell of the lattice whatever (t, u) is (frame 0 of an empty row)
        const float zb = Ab[(long)tc * a_st + blank] + Cb[(long)uc * c_su + blank] + bias_blank;
        c[q] = cell_scalars(blk, emit, alpha, beta, rowbase, T, tc, uc, Tbc, Ub, logZ, zb);
        if (FE) fastemit_cell(c[q], fe_lambda);   // both tables carry the FastEmit values: wl its w, cbe its ce
        if (KD) {   // (the clamped cell: inside the planes whatever (t, u) is)
          const long o = rowbase + (long)uc * T + tc;
          kd_cell(c[q], kd, o, blk[o], emit[o], uc < Ub, gscale, gk);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (dst[q] >= 0) {
          // cells outside the utterance's lattice: w = 0 and an lse that sends 2^(x - lse) to 0, so the inner loop needs no per-cell test
          wl[dst[q]] = in[q] ? make_float2(c[q].w, c[q].lse * LOG2E_F) : make_float2(0.f, 1e30f);
          cbe[dst[q]] = in[q] ? make_float2(c[q].cb, c[q].ce) : make_float2(0.f, 0.f);
        }
      }
    }
    __syncthreads();
    if (vw0 >= V) {   // (whole wave beyond the vocabulary: nothing to do; unchunked no barrier follows, chunked it builds the next table)
      if (CHUNKED) continue;
      return;
    }

    if (uc0 == 0) {
#pragma unroll
      for (int tl = 0; tl < TT; ++tl) {
        a2[tl] = (tl < nf && vok) ? Ab[(long)(t0 + tl) * a_st + v] * LOG2E_F : 0.f;
        accA[tl] = 0.f;
      }
    }
    const float bias_v = vok ? bias[v] : 0.f;
    for (int u0 = uc0; u0 < uc0 + nrow; u0 += UC) {
      float accC[UC], cs2[UC];
#pragma unroll
      for (int j = 0; j < UC; ++j) {
        const int u = min(u0 + j, U1 - 1);
        accC[j] = 0.f;
        cs2[j] = vok ? (Cb[(long)u * c_su + v] + bias_v) * LOG2E_F : 0.f;
        if (KD) cs2[j] = (v == blank || v == ys[u]) ? KD_MASKED : cs2[j];
      }
      if (W ? (u0 <= ub && u0 + UC > ua) : (u0 <= Ub)) {
        // branch-free over the whole 32 x 8 block (cells outside the lattice contribute exact zeros; label positions beyond U1 - 1
        // re-read the last row's table entries, whose sums are not stored): the 256 table reads and v_exp_f32 pipeline freely
#pragma unroll
        for (int tl = 0; tl < TT; ++tl) {
#pragma unroll
          for (int j = 0; j < UC; ++j) {
            const float2 c = wl[tl * UL + (min(u0 + j, U1 - 1) - uc0)];
            // the softmax probability (<= 1: the exponent is z - lse <= 0) times the cell's occupancy
            const float g = c.x * __builtin_amdgcn_exp2f(a2[tl] + cs2[j] - c.y);
            accA[tl] += (u0 + j < U1) ? g : 0.f;   // (a -1e30 entry in cs2 instead of this select: hipcc then spilled — 3.3 instead of 2.1 ms)
            accC[j] += g;
          }
          // two frames (16 table reads) per scheduling region: without the fence hipcc hoists all 256 reads of the block to its top
          // (288 registers: one wave per SIMD; with a register cap: spills), with it 131 registers and three waves per SIMD cover the reads
          if (tl & 1) __builtin_amdgcn_sched_barrier(0);
        }
        // corrections: - P(blank transition) on the blank entry, - P(label transition) on the label's entry
#pragma unroll
        for (int j = 0; j < UC; ++j) {
          const int u = u0 + j;
          if (u <= Ub) {
            const int y = ys[u];
            const bool mine = y >= vw0 && y < vw0 + 64;   // uniform
            if (mine || has_blank) {
#pragma unroll
              for (int tl = 0; tl < TT; ++tl) {
                if (tl < nf) {
                  const float2 c = cbe[tl * UL + (u - uc0)];
                  const float corr = (v == blank ? c.x : 0.f) + (v == y ? c.y : 0.f);
                  accA[tl] -= corr;
                  accC[j] -= corr;
                }
              }
            }
          }
        }
      }
      if (vok) {
#pragma unroll
        for (int j = 0; j < UC; ++j)
          if (u0 + j < U1) dCtile[(long)(u0 + j) * V + v] = accC[j];   // rows beyond Ub: zeros (reduce_dc_kernel sums every row)
      }
    }
  }
  if (vw0 >= V) return;
  if (vok) {
#pragma unroll
    for (int tl = 0; tl < TT; ++tl)
      if (t0 + tl < T) dA[(long)b * a_sb + (long)(t0 + tl) * a_st + v] = KD ? accA[tl] : accA[tl] * gscale;
  }
}

__global__ void __launch_bounds__(256) reduce_dc_kernel(const float* __restrict__ dCp, int ntiles, long per_b, int V,
                                                        long c_sb, long c_su, float gscale_in, const float* __restrict__ gvec,
                                                        int gvec_stride, float* __restrict__ dC) {
  const int b = blockIdx.y;
  const float gscale = gvec ? gscale_in * gvec[(long)b * gvec_stride] : gscale_in;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_b) return;
  const float* src = dCp + (long)b * ntiles * per_b + i;
  float s = 0.f;
  for (int k = 0; k < ntiles; ++k) s += src[(long)k * per_b];
  dC[(long)b * c_sb + (i / V) * c_su + (i % V)] = s * gscale;
}

// dense d/d logits: one wavefront per cell
template <typename TZ, bool FE, bool W, typename... WT>
__global__ void __launch_bounds__(256) grad_dense_kernel(const TZ* __restrict__ Z, const int* __restrict__ labels,
                                                         const int* __restrict__ t_lens, const int* __restrict__ u_lens,
                                                         const float* __restrict__ blk, const float* __restrict__ emit,
                                                         const double* __restrict__ alpha, const double* __restrict__ beta,
                                                         const double* __restrict__ ll, int B, int T, int U1, int V,
                                                         int blank, float gscale, TZ* __restrict__ G, float fe_lambda, WT... wt) {
  static_assert(sizeof...(WT) == (W ? 1 : 0), "W = true takes one Band");
  const Band bt = pick_tables<Band>(wt...);
  const int *wL = bt.L, *wR = bt.R;
  const int lane = threadIdx.x & 63;
  const long ncell = (long)B * T * U1;
  const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((long)gridDim.x * blockDim.x) >> 6;
  for (long cell = wave0; cell < ncell; cell += nw) {
    const int u = (int)(cell % U1);
    const long bt = cell / U1;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const int Tb = t_lens[b], Ub = u_lens[b];
    const TZ* z = Z + cell * V;
    TZ* g = G + cell * V;
    bool dead = t >= Tb || u > Ub;
    if (W) dead = dead || t < wL[(long)b * U1 + u] || t > wR[(long)b * U1 + u];   // outside the band: a zero gradient
    if (dead) {
      for (int v = lane; v < V; v += 64) stf(g, v, 0.f);
      continue;
    }
    CellS c = cell_scalars(blk, emit, alpha, beta, (long)b * U1 * T, T, t, u, Tb, Ub, ll[b], ldf(z, blank));
    if (FE) fastemit_cell(c, fe_lambda);
    const int y = (u < U1 - 1) ? labels[(long)b * (U1 - 1) + u] : -1;
    for (int v = lane; v < V; v += 64) {
      float x = c.w * expf(ldf(z, v) - c.lse);
      if (v == blank) x -= c.cb;
      if (v == y && u < Ub) x -= c.ce;
      stf(g, v, x * gscale);
    }
  }
}

__global__ void __launch_bounds__(256) joint_logits_kernel(const float* __restrict__ A, const float* __restrict__ C,
                                                           const float* __restrict__ bias, int T, int U1, int V,
                                                           long a_sb, long a_st, long c_sb, long c_su, long total,
                                                           float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int v = (int)(i % V);
    long r = i / V;
    const int u = (int)(r % U1);
    r /= U1;  // r = b*T + t
    const long b = r / T, t = r % T;
    out[i] = A[b * a_sb + t * a_st + v] + C[b * c_sb + u * c_su + v] + bias[v];
  }
}

__global__ void nll_kernel(const double* __restrict__ ll, int B, float* __restrict__ nll) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) nll[b] = (float)(-ll[b]);
}

// emission windows: an infeasible row's NLL is +inf by its flag (its sweeps ran on an all -inf lattice: ll = -inf as well)
__global__ void nll_window_kernel(const double* __restrict__ ll, const int* __restrict__ feas, int B, float* __restrict__ nll) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) nll[b] = feas[b] ? (float)(-ll[b]) : __builtin_huge_valf();
}

// lattice distillation, the value: kd[b] = sum over the cells (t < Tb, u <= Ub) and the classes k (blank, label -- u < Ub only --, rest) of
// P_T(k) (log P_T(k) - log P_S(k)).  One workgroup per utterance.  The class terms are fp32, a class the teacher gives probability 0
// adds exactly 0; thread i sums the cells i, i + 256, ... in fp64, then a tree over LDS: a fixed order that depends on the row's own
// lengths alone, so a row gives the same bits alone as in any batch.  A row without cells gives 0.
__global__ void __launch_bounds__(256) kd_value_kernel(const float* __restrict__ blk, const float* __restrict__ emit,
                                                       const float* __restrict__ rest, const float* __restrict__ t_blk,
                                                       const float* __restrict__ t_emit, const float* __restrict__ t_rest,
                                                       const int* __restrict__ t_lens, const int* __restrict__ u_lens, int T,
                                                       int U1, float* __restrict__ kd) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = max(min(t_lens[b], T), 0), Ub = max(min(u_lens[b], U1 - 1), 0);
  const long rowbase = (long)b * U1 * T;
  const int ncell = Tb * (Ub + 1);
  auto term = [](float lt, float ls) -> float {
    const float p = expf(lt);
    return p > 0.f ? p * (lt - ls) : 0.f;
  };
  double s = 0.0;
  for (int i = tid; i < ncell; i += 256) {
    const int u = i / Tb, t = i - u * Tb;
    const long o = rowbase + (long)u * T + t;
    s += (double)term(t_blk[o], blk[o]);
    if (u < Ub) s += (double)term(t_emit[o], emit[o]);
    s += (double)term(t_rest[o], rest[o]);
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) kd[b] = (float)red[0];
}

// out[0] = scale * sum_i x[i]: one wavefront, fixed order (lane partial sums over i = lane, lane + 64, ... then a butterfly)
__global__ void __launch_bounds__(64) scaled_sum_kernel(const float* __restrict__ x, int n, float scale, float* __restrict__ out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += x[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[0] = s * scale;
}

struct LossWs {
  float *blk, *emit;
  double *alpha, *beta, *ll;
  float* dCp;
  float* rest;         // lattice distillation: the student's third plane, laid out as blk / emit; null without KD
  int *L, *R, *feas;   // the band tables ([B][U1] int32) and feasibility flags ([B]) of the windowed loss: null without windows
  unsigned* bp;        // forced alignment: the back-pointer table bp[B][U1][nw = ceil(T/32)], one bit per cell
  int nw;
  size_t total;
};

// ------------------------------------------------------------------------------------------------
// Host half.  Every exported loss / alignment entry fills ONE description of its call, a LossCall, and hands it to a driver:
// run_loss (forward, and the backward when gradients are asked for), run_loss_bwd (the backward alone, on the workspace a forward
// left) or run_align.  A driver checks the whole call before any device work (check_call, which also carves the workspace) and
// then composes the stages: lse -> sweep (+ nll) [-> kd] -> grad, lse -> viterbi, or lse alone into the caller's planes.  A further
// variant of the loss is a field here.
// ------------------------------------------------------------------------------------------------
struct LossCall {
  const char* who = "";   // the entry's name, for messages
  // operands: separable (z = A + C + bias, element strides), or dense logits (B,T,U1,V) in `dtype` storage
  bool dense = false;
  const float *A = nullptr, *C = nullptr, *bias = nullptr;
  int64_t a_sb = 0, a_st = 0, c_sb = 0, c_su = 0;
  const void* logits = nullptr;
  int dtype = RNNT_DTYPE_F32;
  const int32_t *labels = nullptr, *t_lens = nullptr, *u_lens = nullptr;
  int B = 0, T = 0, U1 = 0, V = 0, blank = 0;
  // the gradient: upstream scale, FastEmit's weight, per-utterance upstream gradients (backward-only calls)
  float gscale = 1.f, fastemit_lambda = 0.f;
  const float* gvec = nullptr;
  int gvec_stride = 0;
  // emission windows.  windowed: the call works on the band tables of the workspace -- a forward builds them from emit_lo /
  // emit_hi (rows win_stride apart), a backward-only call finds them there
  bool windowed = false;
  const int32_t *emit_lo = nullptr, *emit_hi = nullptr;
  int64_t win_stride = 0;
  // lattice distillation (KD): the teacher's three planes (B,U1,T), the upstream gradient of the KD term (as gscale / gvec are the
  // NLL's) and where the per-utterance value goes (forward calls).  Separable operands only, no windows.
  bool kd = false;
  const float *t_blk = nullptr, *t_emit = nullptr, *t_rest = nullptr;
  float kd_gscale = 1.f;
  const float* kd_gvec = nullptr;
  int kd_gvec_stride = 0;
  float* kd_out = nullptr;
  // the teacher's side: the three planes of the operands themselves, into the caller's buffers (Drive::Planes)
  float *p_blk = nullptr, *p_emit = nullptr, *p_rest = nullptr;
  // outputs: the loss (dA / dC separable, grad dense; null: no backward) or the alignment
  float *nll = nullptr, *dA = nullptr, *dC = nullptr;
  void* grad = nullptr;
  int32_t* frames = nullptr;
  double* score = nullptr;
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  hipStream_t stream = nullptr;
};

// the loss: alpha | beta | logZ | blk | emit | the dC slabs, then (windowed) the band tables L, R and the feasibility flags, or (KD)
// the student's rest plane
LossWs carve(void* ws, int B, int T, int U1, int V, bool windowed, bool kd = false) {
  LossWs w{};
  Carver c{reinterpret_cast<char*>(ws)};
  const size_t cells = (size_t)B * T * U1, ntiles = ceil_div(T, TT);
  w.alpha = c.take<double>(cells * 8);
  w.beta = c.take<double>(cells * 8);
  w.ll = c.take<double>((size_t)B * 2 * 8);
  w.blk = c.take<float>(cells * 4);
  w.emit = c.take<float>(cells * 4);
  w.dCp = c.take<float>((size_t)B * ntiles * U1 * V * 4);
  if (windowed) {
    w.L = c.take<int>((size_t)B * U1 * 4);
    w.R = c.take<int>((size_t)B * U1 * 4);
    w.feas = c.take<int>((size_t)B * 4);
  }
  if (kd) w.rest = c.take<float>(cells * 4);
  w.total = c.off;
  return w;
}

// forced alignment: blk / emit as the loss lays them out, then the back-pointer table
LossWs carve_align(void* ws, int B, int T, int U1) {
  LossWs w{};
  Carver c{reinterpret_cast<char*>(ws)};
  const size_t cells = (size_t)B * T * U1;
  w.blk = c.take<float>(cells * 4);
  w.emit = c.take<float>(cells * 4);
  w.nw = (int)ceil_div(T, 32);
  w.bp = c.take<unsigned>((size_t)B * U1 * w.nw * 4);
  w.total = c.off;
  return w;
}

// ---- dispatch helpers: a run-time choice handed to a generic lambda as a type (BoolT / IntT / TypeT, and dispatch_k for the K of
// the sweep kernel, are in lattice_shared.hpp) ----
// the storage type of dense logits: f(TypeT<float | __half | __hip_bfloat16>)
template <typename F>
int dispatch_dtype(int dtype, const char* who, F&& f) {
  switch (dtype) {
    case RNNT_DTYPE_F32: return f(TypeT<float>{});
    case RNNT_DTYPE_F16: return f(TypeT<__half>{});
    case RNNT_DTYPE_BF16: return f(TypeT<__hip_bfloat16>{});
    default: set_error("%s: unknown dtype code %d", who, dtype); return RNNT_ERR_INVALID;
  }
}

// The kernel instance of a call.  W: f(BoolT<W>, tables...) -- the W = true instance and its one table struct with emission
// windows, the W = false instance (the kernel without that feature) and no table without.
template <typename Tab, typename F>
int pick_w(bool windowed, const Tab& tab, F&& f) {
  return windowed ? f(BoolT<true>{}, tab) : f(BoolT<false>{});
}
// <FE, W> of the gradient kernels: f(BoolT<FE>, BoolT<W>, lambda, tables...).  lambda = 0 launches the FE = false instances (the
// kernels as they are without FastEmit), lambda > 0 the FE = true ones.
template <typename F>
int pick_fe_w(const LossCall& c, const LossWs& w, F&& f) {
  return pick_w(w.L != nullptr, Band{w.L, w.R}, [&](auto win, auto... wt) {
    return c.fastemit_lambda != 0.f ? f(BoolT<true>{}, win, c.fastemit_lambda, wt...) : f(BoolT<false>{}, win, 0.f, wt...);
  });
}

// <FE, W, KD> of the separable gradient kernels: f(BoolT<FE>, BoolT<W>, BoolT<KD>, lambda, tables...).  A KD call has no windows: its
// pack is the one KdGrad; every other call takes the <FE, W> instances above with KD = false (the kernels without distillation).
template <typename F>
int pick_fe_w_kd(const LossCall& c, const LossWs& w, F&& f) {
  if (c.kd) {
    const KdGrad k = {c.t_blk, c.t_emit, c.t_rest, w.rest, c.kd_gscale, c.kd_gvec, c.kd_gvec_stride};
    return c.fastemit_lambda != 0.f ? f(BoolT<true>{}, BoolT<false>{}, BoolT<true>{}, c.fastemit_lambda, k)
                                    : f(BoolT<false>{}, BoolT<false>{}, BoolT<true>{}, 0.f, k);
  }
  return pick_fe_w(c, w, [&](auto fe, auto win, float lam, auto... wt) { return f(fe, win, BoolT<false>{}, lam, wt...); });
}

// vocabularies from 256 entries take the lane-per-entry kernels (lse_sepv_kernel, grad_sepv_kernel); RNNT_LOSS_SMALLV_KERNELS=1 keeps
// the round-1 kernels everywhere, RNNT_LOSS_LARGEV_KERNELS=1 takes the new ones for every V (A/B and tests)
bool large_vocab(int V) {
  if (getenv("RNNT_LOSS_SMALLV_KERNELS")) return false;
  return V >= 256 || getenv("RNNT_LOSS_LARGEV_KERNELS") != nullptr;
}

unsigned dense_grid(long ncell) { return (unsigned)(ceil_div(ncell, 4) < 16384 ? ceil_div(ncell, 4) : 16384); }

enum class Drive { Forward, Backward, Align, Planes };

// Every argument check of every entry, before any device work; then the workspace, carved, and its size.
int check_call(const LossCall& c, Drive drive, LossWs* w) {
  const char* who = c.who;
  RNNT_CHECK_ARG(c.B >= 1 && c.T >= 1 && c.U1 >= 1 && c.V >= 1, "%s: dims must be positive (B=%d T=%d U1=%d V=%d)", who, c.B, c.T, c.U1, c.V);
  RNNT_CHECK_ARG(c.blank >= 0 && c.blank < c.V, "%s: blank %d outside [0,%d)", who, c.blank, c.V);
  RNNT_CHECK_ARG(c.U1 <= 64 * 8, "%s: U+1 = %d exceeds the 512 label positions one wavefront sweeps", who, c.U1);
  RNNT_CHECK_ARG((int64_t)c.U1 * c.T * 8 < (1ll << 31), "%s: one utterance's lattice (T = %d x U+1 = %d, fp64) exceeds the 2 GB a buffer resource addresses", who, c.T, c.U1);
  RNNT_CHECK_ARG(c.t_lens && c.u_lens, "%s: null lengths", who);
  RNNT_CHECK_ARG(c.U1 == 1 || c.labels, "%s: null labels", who);
  if (c.dense) {
    if (int rc = dispatch_dtype(c.dtype, who, [](auto) { return RNNT_OK; })) return rc;
    RNNT_CHECK_ARG(c.logits, "%s: null logits", who);
  } else {
    RNNT_CHECK_ARG(c.A && c.C && c.bias, "%s: null A/C/bias", who);
  }
  // FastEmit's lambda is read by the backward only, but checked in every call that carries one: finite and >= 0
  if (drive != Drive::Align && drive != Drive::Planes)
    RNNT_CHECK_ARG(c.fastemit_lambda >= 0.f && c.fastemit_lambda <= 3.4028234664e38f, "%s: fastemit_lambda must be finite and >= 0 (got %g)", who, (double)c.fastemit_lambda);
  if (c.kd || drive == Drive::Planes) {   // lattice distillation: three classes per cell, separable operands, no windows
    RNNT_CHECK_ARG(!c.dense, "%s: distillation takes the separable operands, not dense logits", who);
    RNNT_CHECK_ARG(!c.windowed, "%s: distillation does not combine with emission windows", who);
    RNNT_CHECK_ARG(c.V >= 3, "%s: distillation needs V >= 3 (blank, label, rest), got %d", who, c.V);
  }
  if (c.kd) {
    RNNT_CHECK_ARG(c.t_blk && c.t_emit && c.t_rest, "%s: null teacher planes", who);
    RNNT_CHECK_ARG(c.kd_gscale >= -3.4028234664e38f && c.kd_gscale <= 3.4028234664e38f, "%s: kd_gscale must be finite (got %g)", who, (double)c.kd_gscale);
  }
  switch (drive) {
    case Drive::Planes:
      RNNT_CHECK_ARG(c.p_blk && c.p_emit && c.p_rest, "%s: null output planes", who);
      *w = LossWs{};
      w->blk = c.p_blk, w->emit = c.p_emit, w->rest = c.p_rest;
      return RNNT_OK;
    case Drive::Forward:
      RNNT_CHECK_ARG(c.nll, "%s: null nll", who);
      RNNT_CHECK_ARG(!c.kd || c.kd_out, "%s: null kd", who);
      RNNT_CHECK_ARG((c.dA == nullptr) == (c.dC == nullptr), "%s: dA and dC must both be given or both be NULL", who);
      if (c.windowed) {
        RNNT_CHECK_ARG(c.emit_lo && c.emit_hi, "%s: null emit_lo / emit_hi", who);
        RNNT_CHECK_ARG(c.win_stride >= 1 && c.win_stride >= c.U1 - 1, "%s: the window tables' row stride %lld must be positive and at least U = %d",
                       who, (long long)c.win_stride, c.U1 - 1);
      }
      break;
    case Drive::Backward:
      // historical: the backward-only entries have always refused V = 1 and null labels (at U = 0 too), which the forward accepts
      RNNT_CHECK_ARG(c.V >= 2 && c.labels, "%s: V must be at least 2 and labels given", who);
      RNNT_CHECK_ARG(c.dA && c.dC, "%s: null dA/dC", who);
      RNNT_CHECK_ARG(c.gvec_stride == 0 || c.gvec_stride == 1, "%s: gvec_stride must be 0 (one scalar) or 1 (per utterance)", who);
      RNNT_CHECK_ARG(!c.kd || c.kd_gvec_stride == 0 || c.kd_gvec_stride == 1, "%s: kd_gvec_stride must be 0 (one scalar) or 1 (per utterance)", who);
      break;
    case Drive::Align:
      RNNT_CHECK_ARG(c.score, "%s: null score", who);
      RNNT_CHECK_ARG(c.U1 == 1 || c.frames, "%s: null frames", who);
      break;
  }
  *w = drive == Drive::Align ? carve_align(c.workspace, c.B, c.T, c.U1) : carve(c.workspace, c.B, c.T, c.U1, c.V, c.windowed, c.kd);
  RNNT_CHECK_ARG(c.workspace && c.workspace_bytes >= w->total, "%s: workspace too small (%zu < %zu)", who, c.workspace_bytes, w->total);
  return RNNT_OK;
}

// stage 1: blk / emit of every lattice cell, from the separable operands or from dense logits (the loss and the alignment share
// it); with emission windows the band tables first, then the W = true instances; with a rest plane to fill (KD) the KD instances
int stage_lse(const LossCall& c, const LossWs& w) {
  hipStream_t s = c.stream;
  const bool windowed = w.L != nullptr;
  if (windowed) {
    hipLaunchKernelGGL(band_kernel, dim3(c.B), dim3(256), 0, s, c.emit_lo, c.emit_hi, (long)c.win_stride, c.t_lens, c.u_lens, c.T, c.U1,
                       w.L, w.R, w.feas);
    RNNT_CHECK_LAUNCH();
  }
  const Win win = {w.L, w.R, c.emit_lo, c.emit_hi, c.u_lens, (long)c.win_stride};
  if (c.dense) {
    const long ncell = (long)c.B * c.T * c.U1;
    dispatch_dtype(c.dtype, c.who, [&](auto tz) {
      using TZ = typename decltype(tz)::type;
      ProfScope prof(RNNT_K_LSE, (double)sizeof(TZ) * (double)ncell * c.V + 8.0 * (double)ncell, s);
      return pick_w(windowed, win, [&](auto W, auto... wt) {
        hipLaunchKernelGGL((lse_dense_kernel<TZ, decltype(W)::value, decltype(wt)...>), dim3(dense_grid(ncell)), dim3(256), 0, s,
                           (const TZ*)c.logits, c.labels, c.B, c.T, c.U1, c.V, c.blank, w.blk, w.emit, wt...);
        return RNNT_OK;
      });
    });
  } else {
    const int ntiles = (int)ceil_div(c.T, TT);
    const double cells = (double)c.B * c.T * c.U1;
    ProfScope prof(RNNT_K_LSE, 4.0 * ((double)c.B * c.T * c.V + (double)c.B * c.U1 * c.V) + 8.0 * cells, s);
    auto launch = [&](auto W, auto KD, auto... wt) {
      constexpr bool Wv = decltype(W)::value, KDv = decltype(KD)::value;
      if (large_vocab(c.V))
        hipLaunchKernelGGL((lse_sepv_kernel<Wv, KDv, decltype(wt)...>), dim3(ntiles, (unsigned)ceil_div(c.U1, LSV_UT), c.B), dim3(256), 0, s,
                           c.A, c.C, c.bias, c.labels, c.T, c.U1, c.V, c.blank, (long)c.a_sb, (long)c.a_st, (long)c.c_sb, (long)c.c_su,
                           w.blk, w.emit, wt...);
      else
        hipLaunchKernelGGL((lse_sep_kernel<Wv, KDv, decltype(wt)...>), dim3(ntiles, (unsigned)ceil_div(c.U1, LSE_UT), c.B), dim3(256), 0, s,
                           c.A, c.C, c.bias, c.labels, c.T, c.U1, c.V, c.blank, (long)c.a_sb, (long)c.a_st, (long)c.c_sb, (long)c.c_su,
                           w.blk, w.emit, wt...);
      return RNNT_OK;
    };
    if (w.rest)
      launch(BoolT<false>{}, BoolT<true>{}, KdLse{w.rest, c.u_lens});
    else
      pick_w(windowed, win, [&](auto W, auto... wt) { return launch(W, BoolT<false>{}, wt...); });
  }
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// stage 2 of the loss: the alpha | beta sweep (it reads the masked tables of a windowed call as they are), then the NLL per row
int stage_sweep(const LossCall& c, const LossWs& w) {
  hipStream_t s = c.stream;
  {
    ProfScope prof(RNNT_K_ALPHABETA, 2.0 * (8.0 + 8.0) * (double)c.B * c.T * c.U1, s);  // read blk+emit, write alpha|beta (fp64)
    dispatch_k(c.U1, [&](auto k) {
      hipLaunchKernelGGL((alphabeta_kernel<decltype(k)::value>), dim3(c.B, 2), dim3(64), 0, s, w.blk, w.emit, c.t_lens, c.u_lens, c.T, c.U1,
                         w.alpha, w.beta, w.ll);
    });
    RNNT_CHECK_LAUNCH();
  }
  const dim3 grid((unsigned)ceil_div(c.B, 64));
  if (w.feas)
    hipLaunchKernelGGL(nll_window_kernel, grid, dim3(64), 0, s, w.ll, w.feas, c.B, c.nll);
  else
    hipLaunchKernelGGL(nll_kernel, grid, dim3(64), 0, s, w.ll, c.B, c.nll);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// the stage of a KD forward call: the distillation term's value per utterance, from the student's and the teacher's planes
int stage_kd(const LossCall& c, const LossWs& w) {
  ProfScope prof(RNNT_K_MISC, 24.0 * (double)c.B * c.T * c.U1, c.stream);
  hipLaunchKernelGGL(kd_value_kernel, dim3(c.B), dim3(256), 0, c.stream, w.blk, w.emit, w.rest, c.t_blk, c.t_emit, c.t_rest, c.t_lens, c.u_lens,
                     c.T, c.U1, c.kd_out);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// stage 3 of the loss, separable: dA and the per-tile dC slabs, then their fixed-order sum.  (KD: both upstream gradients are in the
// cell scalars already, so the kernels and the slab sum scale by 1)
int stage_grad_sep(const LossCall& c, const LossWs& w) {
  return pick_fe_w_kd(c, w, [&](auto fe_t, auto w_t, auto kd_t, float fe, auto... wt) -> int {
    constexpr bool FE = decltype(fe_t)::value, W = decltype(w_t)::value, KD = decltype(kd_t)::value;
    hipStream_t s = c.stream;
    const int T = c.T, U1 = c.U1, V = c.V, ntiles = (int)ceil_div(T, TT);
    const double cells = (double)c.B * T * U1;
    ProfScope prof(RNNT_K_LATGRAD, 4.0 * 2.0 * ((double)c.B * T * V + (double)c.B * U1 * V) + 24.0 * cells, s);
    constexpr size_t LDS_MAX = 160 * 1024;
    const size_t lds_sep = (size_t)TT * U1 * sizeof(CellS) + (size_t)U1 * 64 * 4 * 2 + (size_t)U1 * 4;   // 1028 (U+1): U+1 <= 159
    // what every gradient kernel takes between its grid and the slab pitch
#define GRAD_SEP_ARGS                                                                                                           \
    c.A, c.C, c.bias, c.labels, c.t_lens, c.u_lens, w.blk, w.emit, w.alpha, w.beta, w.ll, T, U1, V, c.blank, (long)c.a_sb, (long)c.a_st, \
        (long)c.c_sb, (long)c.c_su, c.gscale, c.gvec, c.gvec_stride, c.dA, w.dCp
    // a lane per vocabulary entry, the vocabulary a grid dimension (grad_sepv_kernel): V >= 256, and every U+1 whose grad_sep_kernel
    // table does not fit in LDS (any V)
    if (large_vocab(V) || lds_sep > LDS_MAX) {
      constexpr int NW = 4;   // 256 vocabulary entries per workgroup (8 waves per workgroup measured slower: 5.2 vs 4.6 ms at config 5)
      const dim3 grid(ntiles, (unsigned)ceil_div(V, 64 * NW), c.B), block(64 * NW);
      const size_t per_row = (size_t)TT * sizeof(CellS);
      const size_t lds = (size_t)U1 * per_row + (size_t)U1 * 4;   // 516 (U+1): the whole table up to U+1 = 317
      if (lds <= LDS_MAX) {
        if (lds > 64 * 1024)
          RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)grad_sepv_kernel<NW, false, FE, W, KD, decltype(wt)...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((grad_sepv_kernel<NW, false, FE, W, KD, decltype(wt)...>), grid, block, lds, s, GRAD_SEP_ARGS, U1, fe, wt...);
      } else {   // the table in chunks of label positions: as few chunks as fit, of equal size rounded up to the 8-row block
        const int ul_max = (int)((LDS_MAX - (size_t)U1 * 4) / per_row) & ~7;
        const int nchunks = (int)ceil_div(U1, ul_max);
        const int ul = (int)ceil_div(ceil_div(U1, nchunks), 8) * 8;
        const size_t lds_c = (size_t)ul * per_row + (size_t)U1 * 4;
        RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)grad_sepv_kernel<NW, true, FE, W, KD, decltype(wt)...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c));
        hipLaunchKernelGGL((grad_sepv_kernel<NW, true, FE, W, KD, decltype(wt)...>), grid, block, lds_c, s, GRAD_SEP_ARGS, ul, fe, wt...);
      }
    } else {
      if (lds_sep > 64 * 1024)
        RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)grad_sep_kernel<FE, W, KD, decltype(wt)...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sep));
      hipLaunchKernelGGL((grad_sep_kernel<FE, W, KD, decltype(wt)...>), dim3(ntiles, c.B), dim3(256), lds_sep, s, GRAD_SEP_ARGS, fe, wt...);
    }
#undef GRAD_SEP_ARGS
    RNNT_CHECK_LAUNCH();
    const long per_b = (long)U1 * V;
    hipLaunchKernelGGL(reduce_dc_kernel, dim3((unsigned)ceil_div(per_b, 256), c.B), dim3(256), 0, s, w.dCp, ntiles, per_b, V, (long)c.c_sb,
                       (long)c.c_su, KD ? 1.f : c.gscale, KD ? nullptr : c.gvec, c.gvec_stride, c.dC);
    RNNT_CHECK_LAUNCH();
    return RNNT_OK;
  });
}

// stage 3 of the loss: the lattice gradient under the call's <FE, W> instance -- the separable dA / dC above, or dense d/d logits
int stage_grad(const LossCall& c, const LossWs& w) {
  if (!c.dense) return stage_grad_sep(c, w);
  return dispatch_dtype(c.dtype, c.who, [&](auto tz) -> int {
    using TZ = typename decltype(tz)::type;
    hipStream_t s = c.stream;
    const long ncell = (long)c.B * c.T * c.U1;
    ProfScope prof(RNNT_K_LATGRAD, 2.0 * sizeof(TZ) * (double)ncell * c.V + 24.0 * (double)ncell, s);
    pick_fe_w(c, w, [&](auto fe, auto win, float lam, auto... wt) {
      hipLaunchKernelGGL((grad_dense_kernel<TZ, decltype(fe)::value, decltype(win)::value, decltype(wt)...>), dim3(dense_grid(ncell)), dim3(256),
                         0, s, (const TZ*)c.logits, c.labels, c.t_lens, c.u_lens, w.blk, w.emit, w.alpha, w.beta, w.ll, c.B, c.T, c.U1, c.V,
                         c.blank, c.gscale, (TZ*)c.grad, lam, wt...);
      return RNNT_OK;
    });
    RNNT_CHECK_LAUNCH();
    return RNNT_OK;
  });
}

// stage 2 of the alignment: the max-plus sweep (one back-pointer bit per cell), then the back-trace
int stage_viterbi(const LossCall& c, const LossWs& w) {
  hipStream_t s = c.stream;
  // one scope over BOTH launches (sweep: read blk + emit, write one bit per cell; back-trace: read the bits back), booked under the
  // lattice-sweep kind of the loss: the profiler's kinds are part of the ABI (rnnt_hip_prof_collect), which this feature leaves as it
  // is, so a process that trains and aligns sees both sweeps summed in that slot
  ProfScope prof(RNNT_K_ALPHABETA, (8.0 + 0.25) * (double)c.B * c.T * c.U1, s);
  dispatch_k(c.U1, [&](auto k) {
    hipLaunchKernelGGL((alphabeta_kernel<decltype(k)::value, true>), dim3(c.B, 1), dim3(64), 0, s, w.blk, w.emit, c.t_lens, c.u_lens, c.T, c.U1,
                       w.nw, w.bp, c.score);
  });
  RNNT_CHECK_LAUNCH();
  constexpr size_t LDS_MAX = 160 * 1024;
  const size_t lds = (size_t)c.U1 * w.nw * 4;   // U+1 = 512 label rows by T = 2560 frames fit
  const int in_lds = lds <= LDS_MAX;
  if (in_lds && lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)backtrace_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(backtrace_kernel, dim3(c.B), dim3(256), in_lds ? lds : 0, s, w.bp, c.t_lens, c.u_lens, c.T, c.U1, w.nw, in_lds, c.frames);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// ---- the drivers ----
int run_loss(const LossCall& c) {   // forward; the backward too when the call has somewhere to put it
  LossWs w;
  if (int rc = check_call(c, Drive::Forward, &w)) return rc;
  if (int rc = stage_lse(c, w)) return rc;
  if (int rc = stage_sweep(c, w)) return rc;
  if (c.kd)
    if (int rc = stage_kd(c, w)) return rc;
  return (c.dense ? c.grad != nullptr : c.dA != nullptr) ? stage_grad(c, w) : RNNT_OK;
}

// the second half of a forward call made without gradients: the workspace still holds blk / emit / alpha / beta / logZ (and the band
// tables of a windowed call) of that call on the SAME operands, labels, lengths and windows
int run_loss_bwd(const LossCall& c) {
  LossWs w;
  if (int rc = check_call(c, Drive::Backward, &w)) return rc;
  return stage_grad(c, w);
}

// the teacher's side of the distillation: blk / emit / rest of the operands into the caller's planes -- no sweep, no workspace
int run_planes(const LossCall& c) {
  LossWs w;
  if (int rc = check_call(c, Drive::Planes, &w)) return rc;
  return stage_lse(c, w);
}

int run_align(const LossCall& c) {
  LossWs w;
  if (int rc = check_call(c, Drive::Align, &w)) return rc;
  if (int rc = stage_lse(c, w)) return rc;
  return stage_viterbi(c, w);
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

// ---- the exported entries: each fills a LossCall from its positional arguments (the names below are the parameters') ----
#define FILL_COMMON(c, WHO)                                                                                                  \
  LossCall c;                                                                                                                \
  c.who = WHO, c.labels = labels, c.t_lens = t_lens, c.u_lens = u_lens, c.B = B, c.T = T, c.U1 = U1, c.V = V, c.blank = blank; \
  c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = (hipStream_t)stream
#define FILL_SEP(c, WHO) \
  FILL_COMMON(c, WHO);   \
  c.A = A, c.a_sb = a_sb, c.a_st = a_st, c.C = C, c.c_sb = c_sb, c.c_su = c_su, c.bias = bias
#define FILL_DENSE(c, WHO) \
  FILL_COMMON(c, WHO);     \
  c.dense = true, c.logits = logits, c.dtype = dtype
#define FILL_WINDOWS(c) c.windowed = true, c.emit_lo = emit_lo, c.emit_hi = emit_hi, c.win_stride = win_stride

extern "C" size_t rnnt_hip_joint_loss_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V) {
  if (B < 1 || T < 1 || U1 < 1 || V < 1) return 0;
  return carve(nullptr, B, T, U1, V, false).total;
}

extern "C" int rnnt_hip_joint_loss_fwd_bwd_fastemit(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb,
                                                    int64_t c_su, const float* bias, const int32_t* labels,
                                                    const int32_t* t_lens, const int32_t* u_lens, int32_t B, int32_t T,
                                                    int32_t U1, int32_t V, int32_t blank, float gscale, float fastemit_lambda,
                                                    float* nll, float* dA, float* dC, void* workspace, size_t workspace_bytes,
                                                    void* stream) {
  FILL_SEP(c, "joint_loss");
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.nll = nll, c.dA = dA, c.dC = dC;
  return run_loss(c);
}

extern "C" int rnnt_hip_joint_loss_fwd_bwd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb,
                                           int64_t c_su, const float* bias, const int32_t* labels,
                                           const int32_t* t_lens, const int32_t* u_lens, int32_t B, int32_t T,
                                           int32_t U1, int32_t V, int32_t blank, float gscale, float* nll, float* dA,
                                           float* dC, void* workspace, size_t workspace_bytes, void* stream) {
  return rnnt_hip_joint_loss_fwd_bwd_fastemit(A, a_sb, a_st, C, c_sb, c_su, bias, labels, t_lens, u_lens, B, T, U1, V, blank, gscale, 0.f,
                                              nll, dA, dC, workspace, workspace_bytes, stream);
}

extern "C" int rnnt_hip_joint_loss_bwd_fastemit(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                                const float* bias, const int32_t* labels, const int32_t* t_lens,
                                                const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                                float gscale, float fastemit_lambda, const float* gvec, int32_t gvec_stride,
                                                float* dA, float* dC, void* workspace, size_t workspace_bytes, void* stream) {
  FILL_SEP(c, "joint_loss_bwd");
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.gvec = gvec, c.gvec_stride = gvec_stride, c.dA = dA, c.dC = dC;
  return run_loss_bwd(c);
}

extern "C" int rnnt_hip_joint_loss_bwd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                       const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                       int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale,
                                       const float* gvec, int32_t gvec_stride, float* dA, float* dC, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return rnnt_hip_joint_loss_bwd_fastemit(A, a_sb, a_st, C, c_sb, c_su, bias, labels, t_lens, u_lens, B, T, U1, V, blank, gscale, 0.f,
                                          gvec, gvec_stride, dA, dC, workspace, workspace_bytes, stream);
}

/* ---- emission windows (include/rnnt_hip.h): the entries above with the band tables and the W = true kernel instances ---- */
extern "C" size_t rnnt_hip_joint_loss_window_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V) {
  if (B < 1 || T < 1 || U1 < 1 || V < 1) return 0;
  return carve(nullptr, B, T, U1, V, true).total;
}

extern "C" int rnnt_hip_joint_loss_fwd_bwd_window(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb,
                                                  int64_t c_su, const float* bias, const int32_t* labels, const int32_t* t_lens,
                                                  const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                                  float gscale, float fastemit_lambda, const int32_t* emit_lo,
                                                  const int32_t* emit_hi, int64_t win_stride, float* nll, float* dA, float* dC,
                                                  void* workspace, size_t workspace_bytes, void* stream) {
  FILL_SEP(c, "joint_loss_window");
  FILL_WINDOWS(c);
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.nll = nll, c.dA = dA, c.dC = dC;
  return run_loss(c);
}

extern "C" int rnnt_hip_joint_loss_bwd_window(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                              const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                              int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale,
                                              float fastemit_lambda, const float* gvec, int32_t gvec_stride, float* dA, float* dC,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  FILL_SEP(c, "joint_loss_bwd_window");
  c.windowed = true;
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.gvec = gvec, c.gvec_stride = gvec_stride, c.dA = dA, c.dC = dC;
  return run_loss_bwd(c);
}

/* ---- lattice knowledge distillation (include/rnnt_hip.h): the _fastemit entries with the teacher's planes and the KD instances ---- */
#define FILL_KD(c) c.kd = true, c.t_blk = t_blk, c.t_emit = t_emit, c.t_rest = t_rest, c.kd_gscale = kd_gscale
extern "C" size_t rnnt_hip_joint_loss_kd_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V) {
  if (B < 1 || T < 1 || U1 < 1 || V < 1) return 0;
  return carve(nullptr, B, T, U1, V, false, true).total;
}

extern "C" int rnnt_hip_joint_cell_logprobs(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                            const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                            int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float* blk, float* emit,
                                            float* rest, void* stream) {
  void* workspace = nullptr;
  const size_t workspace_bytes = 0;
  FILL_SEP(c, "joint_cell_logprobs");
  c.p_blk = blk, c.p_emit = emit, c.p_rest = rest;
  return run_planes(c);
}

extern "C" int rnnt_hip_joint_loss_fwd_bwd_kd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                              const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                              int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale,
                                              float fastemit_lambda, const float* t_blk, const float* t_emit, const float* t_rest,
                                              float kd_gscale, float* nll, float* kd, float* dA, float* dC, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  FILL_SEP(c, "joint_loss_kd");
  FILL_KD(c);
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.nll = nll, c.kd_out = kd, c.dA = dA, c.dC = dC;
  return run_loss(c);
}

extern "C" int rnnt_hip_joint_loss_bwd_kd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                          const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                          int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, float gscale,
                                          float fastemit_lambda, const float* gvec, int32_t gvec_stride, const float* t_blk,
                                          const float* t_emit, const float* t_rest, float kd_gscale, const float* kd_gvec,
                                          int32_t kd_gvec_stride, float* dA, float* dC, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  FILL_SEP(c, "joint_loss_bwd_kd");
  FILL_KD(c);
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.gvec = gvec, c.gvec_stride = gvec_stride;
  c.kd_gvec = kd_gvec, c.kd_gvec_stride = kd_gvec_stride, c.dA = dA, c.dC = dC;
  return run_loss_bwd(c);
}

extern "C" int rnnt_hip_scaled_sum_f32(const float* x, int32_t n, float scale, float* out, void* stream) {
  RNNT_CHECK_ARG(x && out && n >= 0, "scaled_sum: bad arguments");
  hipLaunchKernelGGL(scaled_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, x, n, scale, out);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_joint_logits_fwd(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb,
                                         int64_t c_su, const float* bias, int32_t B, int32_t T, int32_t U1, int32_t V,
                                         float* logits, void* stream) {
  RNNT_CHECK_ARG(A && C && bias && logits, "joint_logits: null pointer");
  RNNT_CHECK_ARG(B >= 1 && T >= 1 && U1 >= 1 && V >= 1, "joint_logits: dims must be positive");
  const long total = (long)B * T * U1 * V;
  const unsigned grid = (unsigned)(ceil_div(total, 256) < 65536 ? ceil_div(total, 256) : 65536);
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)total, (hipStream_t)stream);
  hipLaunchKernelGGL(joint_logits_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, A, C, bias, T, U1, V, (long)a_sb, (long)a_st, (long)c_sb, (long)c_su, total, logits);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

/* ---- the loss on dense logits in fp32 / f16 / bf16 storage ---- */
extern "C" int rnnt_hip_loss_from_logits_fwd_bwd_fastemit(const void* logits, int32_t dtype, const int32_t* labels,
                                                          const int32_t* t_lens, const int32_t* u_lens, int32_t B, int32_t T,
                                                          int32_t U1, int32_t V, int32_t blank, float gscale, float fastemit_lambda,
                                                          float* nll, void* grad, void* workspace, size_t workspace_bytes,
                                                          void* stream) {
  FILL_DENSE(c, "loss_from_logits");
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.nll = nll, c.grad = grad;
  return run_loss(c);
}

extern "C" int rnnt_hip_loss_from_logits_fwd_bwd_window(const void* logits, int32_t dtype, const int32_t* labels,
                                                        const int32_t* t_lens, const int32_t* u_lens, int32_t B, int32_t T,
                                                        int32_t U1, int32_t V, int32_t blank, float gscale, float fastemit_lambda,
                                                        const int32_t* emit_lo, const int32_t* emit_hi, int64_t win_stride,
                                                        float* nll, void* grad, void* workspace, size_t workspace_bytes,
                                                        void* stream) {
  FILL_DENSE(c, "loss_from_logits_window");
  FILL_WINDOWS(c);
  c.gscale = gscale, c.fastemit_lambda = fastemit_lambda, c.nll = nll, c.grad = grad;
  return run_loss(c);
}

extern "C" int rnnt_hip_loss_from_logits_fwd_bwd_ex(const void* logits, int32_t dtype, const int32_t* labels,
                                                    const int32_t* t_lens, const int32_t* u_lens, int32_t B, int32_t T,
                                                    int32_t U1, int32_t V, int32_t blank, float gscale, float* nll, void* grad,
                                                    void* workspace, size_t workspace_bytes, void* stream) {
  return rnnt_hip_loss_from_logits_fwd_bwd_fastemit(logits, dtype, labels, t_lens, u_lens, B, T, U1, V, blank, gscale, 0.f, nll, grad,
                                                    workspace, workspace_bytes, stream);
}

extern "C" int rnnt_hip_loss_from_logits_fwd_bwd(const float* logits, const int32_t* labels, const int32_t* t_lens,
                                                 const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V,
                                                 int32_t blank, float gscale, float* nll, float* grad, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
  return rnnt_hip_loss_from_logits_fwd_bwd_ex(logits, RNNT_DTYPE_F32, labels, t_lens, u_lens, B, T, U1, V, blank, gscale, nll, grad,
                                              workspace, workspace_bytes, stream);
}

/* ---- forced alignment (include/rnnt_hip.h): lse kernels of the loss, max-plus sweep, back-trace ---- */
extern "C" size_t rnnt_hip_joint_align_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V) {
  if (B < 1 || T < 1 || U1 < 1 || V < 1) return 0;
  return carve_align(nullptr, B, T, U1).total;
}

extern "C" int rnnt_hip_joint_align(const float* A, int64_t a_sb, int64_t a_st, const float* C, int64_t c_sb, int64_t c_su,
                                    const float* bias, const int32_t* labels, const int32_t* t_lens, const int32_t* u_lens,
                                    int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank, int32_t* frames, double* score,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  FILL_SEP(c, "joint_align");
  c.frames = frames, c.score = score;
  return run_align(c);
}

extern "C" int rnnt_hip_align_from_logits_ex(const void* logits, int32_t dtype, const int32_t* labels, const int32_t* t_lens,
                                             const int32_t* u_lens, int32_t B, int32_t T, int32_t U1, int32_t V, int32_t blank,
                                             int32_t* frames, double* score, void* workspace, size_t workspace_bytes, void* stream) {
  FILL_DENSE(c, "align_from_logits");
  c.frames = frames, c.score = score;
  return run_align(c);
}

