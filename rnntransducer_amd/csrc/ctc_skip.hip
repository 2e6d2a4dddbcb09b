// CTC-guided blank-frame skipping in front of the transducer searches, for gfx950.  DESIGN.md §29.
//
// Per utterance b and frame t < T_b: lp[t] = z[t,blank] - logsumexp_v z[t,:], in fp32 with the row maximum subtracted, the arithmetic
// of ctc_terms_kernel (ctc.hip).  The frame is SKIPPED exactly when lp[t] > log_threshold (a NaN row is therefore kept).  The kept
// frames' rows of `enc` are copied, in order and bit for bit, to rows 0 .. new_lens[b]-1 of `enc_out`; frame_map[b][j] is the
// original frame of kept frame j, -1 for j >= new_lens[b].
//
// Kernels, both on a (ceil(T/32), B) grid of 256 threads, no atomics, nothing that depends on the batch around a row:
//   skip_mark_kernel   : a wavefront per frame, lanes along v (wave w takes frames w, w+4, ... of the 32-frame tile); the tile's keep
//                        bits leave as ONE word words[b][tile]; lp goes to blank_logp on request.  Tiles past T_b return at once and
//                        write nothing: the gather reads only the ceil(T_b/32) words of a row.
//   skip_gather_kernel : wave 0 sums the popcounts of the row's words (those below its own tile: the tile's base offset; all: new_lens),
//                        striding over them, so any T works; the r-th set bit of the tile's word is row base + r.  Wave w copies kept
//                        rows w, w+4, ... with 16-byte accesses when O % 4 == 0 and every address and stride allows (VEC), 4-byte
//                        ones otherwise.  Threads 0..31 write the tile's frame_map entries and the -1 of entries t0 .. t0+31 that
//                        lie at or behind new_lens[b]; tile 0 writes new_lens[b].
// Frames t >= T_b of logits and enc are never read.
#include "common.hpp"
#include "lattice_shared.hpp"

namespace rnnt {
namespace {

constexpr int TT = 32;   // frames per workgroup tile = bits per keep word

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

__global__ void __launch_bounds__(256) skip_mark_kernel(const float* __restrict__ Z, long z_sb, long z_st,
                                                        const int* __restrict__ t_lens, int T, int V, int blank, float log_thr,
                                                        unsigned* __restrict__ words, int nt, float* __restrict__ blank_logp) {
  __shared__ int keep_s[TT];
  const int b = blockIdx.y, tile = blockIdx.x, t0 = tile * TT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = clampi(t_lens[b], 0, T);
  if (t0 >= Tb) return;   // (uniform)
  if (tid < TT) keep_s[tid] = 0;
  __syncthreads();
  const float* Zb = Z + (long)b * z_sb;
  for (int tl = wave; tl < TT && t0 + tl < Tb; tl += 4) {
    const float* z = Zb + (long)(t0 + tl) * z_st;
    float m = -__builtin_huge_valf();
    for (int v = lane; v < V; v += 64) m = fmaxf(m, z[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(z[v] - m);
    s = wave_sum(s);
    if (lane == 0) {
      const float lse = m + logf(s);
      const float lp = z[blank] - lse;
      keep_s[tl] = !(lp > log_thr);
      if (blank_logp) blank_logp[(long)b * T + t0 + tl] = lp;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const unsigned long long bits = __ballot(lane < TT && keep_s[lane & (TT - 1)] != 0);
    if (lane == 0) words[(long)b * nt + tile] = (unsigned)bits;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) skip_gather_kernel(const unsigned* __restrict__ words, int nt, const int* __restrict__ t_lens,
                                                          int T, const unsigned* __restrict__ enc, long e_sb, long e_st, int O,
                                                          unsigned* __restrict__ out, long o_sb, long o_st,
                                                          int* __restrict__ new_lens, int* __restrict__ frame_map) {
  __shared__ int src_s[TT];   // tile-local frame of the r-th kept frame
  __shared__ int sum_s[2];    // kept frames below this tile | of the whole row
  const int b = blockIdx.y, tile = blockIdx.x, t0 = tile * TT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = clampi(t_lens[b], 0, T);
  const int ntb = (Tb + TT - 1) / TT;   // the words the mark kernel wrote for this row
  const unsigned* wb = words + (long)b * nt;
  if (wave == 0) {
    int below = 0, all = 0;
    for (int i = lane; i < ntb; i += 64) {
      const int c = __popc(wb[i]);
      all += c;
      below += i < tile ? c : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      below += __shfl_xor(below, o);
      all += __shfl_xor(all, o);
    }
    if (lane == 0) sum_s[0] = below, sum_s[1] = all;
  }
  const unsigned w = tile < ntb ? wb[tile] : 0u;   // (uniform)
  if (tid < TT && ((w >> tid) & 1u)) src_s[__popc(w & ((1u << tid) - 1u))] = tid;
  __syncthreads();
  const int base = sum_s[0], total = sum_s[1], n = __popc(w);   // base + n <= total <= Tb <= T
  if (tile == 0 && tid == 0) new_lens[b] = total;
  if (tid < TT) {
    int* fm = frame_map + (long)b * T;
    if (tid < n) fm[base + tid] = t0 + src_s[tid];
    const int j = t0 + tid;
    if (j >= total && j < T) fm[j] = -1;
  }
  const unsigned* eb = enc + (long)b * e_sb;
  unsigned* ob = out + (long)b * o_sb;
  for (int r = wave; r < n; r += 4) {
    const unsigned* src = eb + (long)(t0 + src_s[r]) * e_st;
    unsigned* dst = ob + (long)(base + r) * o_st;
    if constexpr (VEC) {
      const u32x4* s4 = reinterpret_cast<const u32x4*>(src);
      u32x4* d4 = reinterpret_cast<u32x4*>(dst);
#pragma unroll 4
      for (int c = lane; c < (O >> 2); c += 64) d4[c] = s4[c];
    } else {
#pragma unroll 4
      for (int c = lane; c < O; c += 64) dst[c] = src[c];
    }
  }
}

bool aligned16(const void* p, int64_t a, int64_t b) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && a % 4 == 0 && b % 4 == 0; }

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" size_t rnnt_hip_ctc_frame_skip_workspace_bytes(int32_t B, int32_t T) {
  if (B < 1 || T < 1) return 0;
  return align_up((size_t)B * (size_t)ceil_div(T, TT) * 4, 256);
}

extern "C" int rnnt_hip_ctc_frame_skip(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T,
                                       int32_t V, int32_t blank, float log_threshold, const float* enc, int64_t e_sb, int64_t e_st,
                                       int32_t O, float* enc_out, int64_t o_sb, int64_t o_st, int32_t* new_lens, int32_t* frame_map,
                                       float* blank_logp, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "ctc_frame_skip";
  RNNT_CHECK_ARG(B >= 1 && T >= 1 && O >= 1, "%s: B, T, O must be positive (B=%d T=%d O=%d)", what, B, T, O);
  RNNT_CHECK_ARG(B <= 65535, "%s: B = %d exceeds the 65535 rows of one launch", what, B);
  RNNT_CHECK_ARG(V >= 2, "%s: V = %d < 2 (a blank and at least one token)", what, V);
  RNNT_CHECK_ARG(blank >= 0 && blank < V, "%s: blank %d outside [0,%d)", what, blank, V);
  RNNT_CHECK_ARG(log_threshold <= 0.f, "%s: log_threshold %g must be a log-probability, <= 0 and not NaN", what, (double)log_threshold);
  RNNT_CHECK_ARG(logits && t_lens && enc && enc_out && new_lens && frame_map, "%s: null logits/lengths/enc/enc_out/new_lens/frame_map", what);
  RNNT_CHECK_ARG(z_sb >= 1 && z_st >= V, "%s: logits strides (z_sb = %lld, z_st = %lld) must be positive, z_st >= V", what, (long long)z_sb, (long long)z_st);
  RNNT_CHECK_ARG(e_sb >= 1 && e_st >= O && o_sb >= 1 && o_st >= O, "%s: row strides (e_sb = %lld, e_st = %lld, o_sb = %lld, o_st = %lld) must be positive, e_st and o_st >= O",
                 what, (long long)e_sb, (long long)e_st, (long long)o_sb, (long long)o_st);
  {   // enc_out must not alias enc: the gather reads rows other workgroups may already have overwritten
    const float *e0 = enc, *e1 = enc + (B - 1) * e_sb + (T - 1) * e_st + O;
    const float *o0 = enc_out, *o1 = enc_out + (B - 1) * o_sb + (T - 1) * o_st + O;
    RNNT_CHECK_ARG(o1 <= e0 || e1 <= o0, "%s: enc_out overlaps enc", what);
  }
  const size_t need = rnnt_hip_ctc_frame_skip_workspace_bytes(B, T);
  RNNT_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, need);
  RNNT_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "%s: workspace must be 4-byte aligned", what);
  hipStream_t s = (hipStream_t)stream;
  const int nt = (int)ceil_div(T, TT);
  const dim3 grid((unsigned)nt, (unsigned)B);
  unsigned* words = reinterpret_cast<unsigned*>(workspace);
  {
    ProfScope prof(RNNT_K_MISC, 4.0 * (double)B * T * V, s);
    hipLaunchKernelGGL(skip_mark_kernel, grid, dim3(256), 0, s, logits, (long)z_sb, (long)z_st, t_lens, T, V, blank, log_threshold, words, nt,
                       blank_logp);
  }
  RNNT_CHECK_LAUNCH();
  const bool vec = O % 4 == 0 && aligned16(enc, e_sb, e_st) && aligned16(enc_out, o_sb, o_st);
  ProfScope prof(RNNT_K_MISC, 8.0 * (double)B * T * O + 4.0 * (double)B * T, s);
  const unsigned* src = reinterpret_cast<const unsigned*>(enc);
  unsigned* dst = reinterpret_cast<unsigned*>(enc_out);
  if (vec)
    hipLaunchKernelGGL(skip_gather_kernel<true>, grid, dim3(256), 0, s, words, nt, t_lens, T, src, (long)e_sb, (long)e_st, O, dst, (long)o_sb,
                       (long)o_st, new_lens, frame_map);
  else
    hipLaunchKernelGGL(skip_gather_kernel<false>, grid, dim3(256), 0, s, words, nt, t_lens, T, src, (long)e_sb, (long)e_st, O, dst, (long)o_sb,
                       (long)o_st, new_lens, frame_map);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}
