// Shared by the two lattice files (loss.hip: RNN-T, ctc.hip: CTC).  Device: wavefront reductions, the log-space sum with fp64
// accumulators, the one-lane neighbour hand-off, the buffer-resource constants of the sweeps and the optional-table pack.  Host: the
// workspace carver and the type-valued dispatch of their host halves.
#pragma once
#include "common.hpp"

#include <type_traits>

namespace rnnt {

constexpr double NEG_INF = -__builtin_huge_val();

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

__device__ __forceinline__ double logaddexp_d(double a, double b) {
  const double m = fmax(a, b);
  if (m == NEG_INF) return NEG_INF;
  const float d = (float)(fmin(a, b) - m);  // <= 0, -inf allowed
  // fp32 correction term in [0, ln 2]: hardware exp/log (abs err ~1e-7) -- the fp64 running sums keep the lattice exact
  return m + (double)__logf(1.0f + __expf(d));
}
// neighbour hand-off across the whole wavefront by DPP (wave_shr:1 / wave_shl:1): two moves per fp64, no LDS permute
__device__ __forceinline__ double shfl_up1(double x, int lane) {
  const long long b = __builtin_bit_cast(long long, x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x138, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x138, 0xf, 0xf, false);
  const double y = __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
  return lane == 0 ? NEG_INF : y;
}
__device__ __forceinline__ double shfl_down1(double x, int lane) {
  const long long b = __builtin_bit_cast(long long, x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x130, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x130, 0xf, 0xf, false);
  const double y = __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
  return lane == 63 ? NEG_INF : y;
}

constexpr int PF = 8;  // per-row values in flight per lane (register ring)
constexpr int AB_RSRC = 0x00027000, AB_OOB = 0x7ffffff0;

// A kernel takes the tables of an optional feature as a trailing parameter PACK: pick_tables<T> is the pack's member of type T, or
// an empty T (the instance without the feature, whose parameter list stays that of the kernel without it).
template <typename T>
__device__ __forceinline__ T pick_tables() { return T{}; }
template <typename T, typename H, typename... R>
__device__ __forceinline__ T pick_tables(H h, R... r) {
  if constexpr (std::is_same<T, H>::value) return h;
  else return pick_tables<T>(r...);
}

// ---- host helpers of the two files ----
struct Carver {   // consecutive 256-byte aligned pieces of a workspace (a null base: sizes only)
  char* p;
  size_t off = 0;
  template <typename T>
  T* take(size_t bytes) {
    char* q = p ? p + off : nullptr;
    off += align_up(bytes, 256);
    return reinterpret_cast<T*>(q);
  }
};

// a run-time choice handed to a generic lambda as a type
template <bool X> struct BoolT { static constexpr bool value = X; };
template <int X> struct IntT { static constexpr int value = X; };
template <typename T> struct TypeT { using type = T; };

// K label positions per lane of the sweep kernels (alphabeta_kernel, ctc_sweep_kernel): f(IntT<K>), K in {1, 2, 3, 4, 8}
template <typename F>
void dispatch_k(int U1, F&& f) {
  switch ((int)ceil_div(U1, 64)) {
    case 1: f(IntT<1>{}); break;
    case 2: f(IntT<2>{}); break;
    case 3: f(IntT<3>{}); break;
    case 4: f(IntT<4>{}); break;
    default: f(IntT<8>{}); break;
  }
}

}  // namespace rnnt
