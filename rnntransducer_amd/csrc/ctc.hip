// CTC loss on the encoder's logits, the greedy (best-path) CTC decode, and the forced alignment of a known transcript, for gfx950.
// DESIGN.md §16, §28.
//
// Per utterance b: frames t < T_b, labels y_0..y_{U_b-1}, extended sequence l' of S = 2 U_b + 1 states (l'_{2k} = blank,
// l'_{2k+1} = y_k), lp[t,v] = z[t,v] - logsumexp_v z[t,:].
//   alpha_0(0) = lp[0,blank], alpha_0(1) = lp[0,y_0], every other alpha_0(s) = -inf
//   alpha_t(s) = lp[t,l'_s] + logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), [l'_s != blank and l'_s != l'_{s-2}] alpha_{t-1}(s-2))
//   logZ = logaddexp(alpha_{T_b-1}(S-1), alpha_{T_b-1}(S-2)),  NLL_b = -logZ;  beta is the mirror image
//   dz[b,t,v] = g_b (softmax(z[b,t,:])[v] - sum_{s: l'_s = v} occ_t(s)),  occ_t(s) = exp(alpha_t(s) + beta_t(s) - lp[t,l'_s] - logZ)
// Arithmetic as in loss.hip: fp32 per-frame terms, fp64 lattice sums with the fp32 log1p(exp(.)) correction of logaddexp_d, the
// 3-term sum as two nested 2-term sums in the order written above.  A row without any path (T_b < U_b + repeats) has logZ = -inf:
// NLL = +inf and an exactly zero gradient row.
//
// Kernels:
//   ctc_terms_kernel     : row log-sum-exp of every valid frame (a wavefront per frame, lanes along v) and the U_b + 1 emission rows the
//                          sweep reads, label-major over t: em[b][0][t] = lp[t,blank], em[b][k+1][t] = lp[t,y_k]; the tile-0
//                          workgroup of an utterance also links equal labels into chains (for the gradient's fixed-order sums)
//   ctc_sweep_kernel<K, MAX> : one wavefront per (utterance, alpha|beta); lane l owns label positions [l*K, l*K+K), each a blank state
//                          and the label state behind it (position U_b: the trailing blank only); every state steps at every t, the
//                          neighbour lane's boundary states arrive by DPP; memory operations unconditional through buffer
//                          resources, per-row values prefetched PF steps ahead (loss.hip explains why).  MAX = true: forced
//                          alignment, the same alpha sweep in the (max, +) semiring, one wavefront per utterance, three
//                          back-pointer bits per (frame, position) packed into 32-frame words instead of the cell stores
//   ctc_grad_kernel      : grid (32-frame tile, utterance); occupancies of the tile in LDS, then softmax - sum occ per frame; equal
//                          labels are summed along their chain by the lane of the first occurrence: fixed order, no float atomics
//   ctc_greedy_kernel    : a workgroup per utterance: argmax per frame (ties to the lowest index), collapse, ballot compaction
//   ctc_backtrace_kernel : a workgroup per utterance: the best path walked backwards a word at a time, then first / last / path /
//                          token_logp
// The host half (from struct CtcCall on): one CtcCall per call, one check, four stages behind the exported entries.
#include "common.hpp"
#include "lattice_shared.hpp"

namespace rnnt {
namespace {

constexpr int TT = 32;           // frames per workgroup tile
constexpr int CH_NONE = 0x3ff;   // chain code: no later position carries the same label (positions are < 512)
constexpr int CH_FIRST = 1 << 30;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

// ------------------------------------------------------------------------------------------------
// per-frame terms.  grid (ceil(T/32), B), 256 threads: wave w takes frames w, w+4, ... of the tile, lanes run along v.
// Frames t >= T_b and label positions k >= U_b are never read (padded logits and labels may hold anything).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ctc_terms_kernel(const float* __restrict__ Z, long z_sb, long z_st,
                                                        const int* __restrict__ labels, const int* __restrict__ t_lens,
                                                        const int* __restrict__ u_lens, int T, int U, int V, int blank,
                                                        float* __restrict__ em, float* __restrict__ lse_out,
                                                        int* __restrict__ chain) {
  __shared__ float lse_s[TT];
  __shared__ int ys[512];
  const int b = blockIdx.y, t0 = blockIdx.x * TT, U1 = U + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = clampi(t_lens[b], 0, T), Ub = clampi(u_lens[b], 0, U);
  if (t0 >= Tb) return;   // (uniform)
  const float* Zb = Z + (long)b * z_sb;
  for (int i = tid; i < Ub; i += 256) ys[i] = labels[(long)b * U + i];
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
      lse_s[tl] = lse;
      lse_out[(long)b * T + t0 + tl] = lse;
    }
  }
  __syncthreads();
  // consecutive threads -> consecutive frames: the emission rows are written coalesced
  for (int i = tid; i < TT * (Ub + 1); i += 256) {
    const int r = i / TT, tl = i % TT, t = t0 + tl;
    if (t < Tb) {
      const int v = r == 0 ? blank : ys[r - 1];
      // (a label outside the vocabulary is the caller's error, as in the RNN-T loss; it is not dereferenced)
      em[((long)b * U1 + r) * T + t] = (v >= 0 && v < V) ? Zb[(long)t * z_st + v] - lse_s[tl] : 0.f;
    }
  }
  if (blockIdx.x == 0) {
    // chain[u] = the next position with the same label (CH_NONE: none) | CH_FIRST when no earlier position carries it
    for (int u = tid; u < Ub; u += 256) {
      const int y = ys[u];
      int nxt = CH_NONE, first = CH_FIRST;
      for (int k = u + 1; k < Ub; ++k)
        if (ys[k] == y) { nxt = k; break; }
      for (int k = u - 1; k >= 0; --k)
        if (ys[k] == y) { first = 0; break; }
      chain[(long)b * U1 + u] = nxt | first;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// alpha / beta: one wavefront per (b, which).  Position u of a lane = blank state 2u and label state 2u+1.
// sB / sL hold alpha_{t-1} (beta_{t+1}) of the lane's states when step t starts; a lane walks its positions against the direction of
// the dependence, so the neighbour's value it reads is still the previous step's.
//
// The semiring is the template flag MAX.  MAX = false, the loss: the sums of the file's header, both directions picked by
// blockIdx.y, both states of every position stored in fp64, logZ and the NLL at the end of the alpha direction.
// MAX = true, forced alignment: the alpha direction alone (grid (B, 1); the beta branch is not compiled) in the
// (max, +) semiring on the same emission rows, same lane ownership:
//   v_t(s) = lp[t,l'_s] + max( v_{t-1}(s), v_{t-1}(s-1), [l'_s != blank and l'_s != l'_{s-2}] v_{t-1}(s-2) )
// fp64 sums of the fp32 emission rows, no transcendental.  TIE RULE: the candidates are taken in the order written (stay, s-1, s-2)
// and a later one wins only when strictly greater, so a -inf candidate never beats a -inf incumbent and the path is a pure function
// of lp.  Back-pointers in place of the cell stores: three bits per (frame, position) in three planes of 32-frame words,
// bp[b][plane][u][t >> 5] bit (t & 31):
//   plane 0: the blank state of position u was entered from the label state of position u-1
//   plane 1: the label state of position u was entered from its own blank state (s-1)
//   plane 2: the label state of position u was entered from the label state of position u-1 (s-2)
// (no bit: the state stayed; frame 0 has no predecessor and never a bit).  A lane collects the bits of its K positions in registers
// and stores the words when the step ends a 32-frame block or the utterance; like every memory operation of the loop the stores go
// through a buffer resource, with an out-of-range offset when there is nothing to store.  At the end score = max(v(S-1), v(S-2))
// goes to ll[b] (-inf for a row without any path) and fin[b] says which of the two it was (the label state wins only when strictly
// greater).  The MAX instance takes its tables as a trailing CtcBackPtr (the pack is empty for the loss, whose instances keep their
// kernel-argument block); aB / aL / bB / bL / nll are not read then.
// ------------------------------------------------------------------------------------------------
struct CtcBackPtr {
  unsigned* bp;   // bp[B][3][U + 1][nw]
  int nw;         // words per position: ceil(T / 32)
  int* fin;       // [B]: 1 when the best path ends in the last label state, 0 in the trailing blank
};

template <int K, bool MAX = false, typename... BT>
__global__ void __launch_bounds__(64) ctc_sweep_kernel(const float* __restrict__ em, const int* __restrict__ labels,
                                                       const int* __restrict__ t_lens, const int* __restrict__ u_lens, int T,
                                                       int U, double* __restrict__ aB, double* __restrict__ aL,
                                                       double* __restrict__ bB, double* __restrict__ bL,
                                                       double* __restrict__ ll, float* __restrict__ nll, BT... bt) {
  const int b = blockIdx.x, which = MAX ? 0 : blockIdx.y, lane = threadIdx.x, U1 = U + 1;
  const CtcBackPtr bk = pick_tables<CtcBackPtr>(bt...);
  const int Tb = clampi(t_lens[b], 0, T), Ub = clampi(u_lens[b], 0, U);
  const long rowbase = (long)b * U1 * T;
  const int cells = U1 * T, NW = bk.nw, pwords = U1 * NW;
  const int ulo = lane * K;
  const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(em + rowbase), 0, cells * 4, AB_RSRC);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((which == 0 ? aB : bB) + rowbase, 0, cells * 8, AB_RSRC);
  const __amdgpu_buffer_rsrc_t rL = __builtin_amdgcn_make_buffer_rsrc((which == 0 ? aL : bL) + rowbase, 0, cells * 8, AB_RSRC);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(bk.bp + (long)b * 3 * pwords, 0, 3 * pwords * 4, AB_RSRC);   // MAX
  auto ld = [&](int c) -> float {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(re, c >= 0 ? c * 4 : AB_OOB, 0, 0));
  };
  auto st = [&](const __amdgpu_buffer_rsrc_t& r, double v, int c) {
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(i32x2, v), r, c >= 0 ? c * 8 : AB_OOB, 0, 0);
  };
  auto stw = [&](unsigned v, int w) { __builtin_amdgcn_raw_buffer_store_b32((int)v, rw, w >= 0 ? w * 4 : AB_OOB, 0, 0); };
  // emission rows: row 0 = blank (the same value for every lane), row u + 1 = label u
  auto cellB = [&](int t) -> int { return (t >= 0 && t < Tb) ? t : -1; };
  auto cellL = [&](int u, int t) -> int { return (t >= 0 && t < Tb && u < Ub) ? (u + 1) * T + t : -1; };
  const int* yb = labels + (long)b * U;
  // skip[k]: the label state of position u may be entered from (alpha) / may leave to (beta) the neighbouring LABEL state
  bool skip[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = ulo + k;
    const int lo = which == 0 ? u - 1 : u;
    skip[k] = (lo >= 0 && lo + 1 < Ub) ? (yb[lo] != yb[lo + 1]) : false;
  }
  const int nrounds = (Tb + PF - 1) / PF;   // steps beyond Tb touch nothing
  double sB[K], sL[K];
  [[maybe_unused]] unsigned w0[K], w1[K], w2[K];   // MAX: back-pointer bits of the current 32-frame block, one word per plane
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sB[k] = sL[k] = NEG_INF;
    w0[k] = w1[k] = w2[k] = 0u;
  }
  float pb[PF], pl[PF][K];

  if (which == 0) {
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      pb[j] = ld(cellB(j));
#pragma unroll
      for (int k = 0; k < K; ++k) pl[j][k] = ld(cellL(ulo + k, j));
    }
    for (int r = 0; r < nrounds; ++r) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const int t = r * PF + j;
        const double carry = shfl_up1(sL[K - 1], lane);   // alpha_{t-1} of the label state before this lane's first blank
        const float cb = pb[j];
        float cl[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cl[k] = pl[j][k];
        pb[j] = ld(cellB(t + PF));
#pragma unroll
        for (int k = 0; k < K; ++k) pl[j][k] = ld(cellL(ulo + k, t + PF));
        const bool row = t < Tb;
        const int sh = t & 31, wi = t >> 5;
        const bool flush = row && (sh == 31 || t == Tb - 1);   // (uniform)
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {
          const int u = ulo + k;
          const double prevL = k > 0 ? sL[k - 1] : carry;
          const bool okB = row && u <= Ub, okL = row && u < Ub;
          double nB, nL;
          bool c0 = false, c1 = false, c2 = false;   // MAX: the back-pointer bits of this step
          if (t == 0) {   // (uniform)
            nB = u == 0 ? (double)cb : NEG_INF;
            nL = u == 0 ? (double)cl[k] : NEG_INF;
          } else if constexpr (MAX) {
            c0 = prevL > sB[k];
            nB = (double)cb + (c0 ? prevL : sB[k]);
            c1 = sB[k] > sL[k];
            double m = c1 ? sB[k] : sL[k];
            c2 = skip[k] && prevL > m;
            m = c2 ? prevL : m;
            c1 = c1 && !c2;
            nL = (double)cl[k] + m;
          } else {
            nB = (double)cb + logaddexp_d(sB[k], prevL);
            double x = logaddexp_d(sL[k], sB[k]);
            x = skip[k] ? logaddexp_d(x, prevL) : x;
            nL = (double)cl[k] + x;
          }
          if constexpr (MAX) {
            const unsigned n0 = (sh == 0 ? 0u : w0[k]) | ((unsigned)c0 << sh);
            const unsigned n1 = (sh == 0 ? 0u : w1[k]) | ((unsigned)c1 << sh);
            const unsigned n2 = (sh == 0 ? 0u : w2[k]) | ((unsigned)c2 << sh);
            w0[k] = n0;
            w1[k] = n1;
            w2[k] = n2;
            stw(n0, (okB && flush) ? u * NW + wi : -1);
            stw(n1, (okL && flush) ? pwords + u * NW + wi : -1);
            stw(n2, (okL && flush) ? 2 * pwords + u * NW + wi : -1);
          } else {
            st(rB, nB, okB ? u * T + t : -1);
            st(rL, nL, okL ? u * T + t : -1);
          }
          sB[k] = okB ? nB : sB[k];
          sL[k] = okL ? nL : sL[k];
        }
      }
    }
    // logZ = logaddexp(alpha(S-1), alpha(S-2)): the trailing blank of position Ub and the label state before it
    // (MAX: score = max of the two, the label state only when strictly greater)
    const double prevL = shfl_up1(sL[K - 1], lane);
    double vB = NEG_INF, vL = NEG_INF;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (ulo + k == Ub) {
        vB = sB[k];
        vL = k > 0 ? sL[k - 1] : prevL;
      }
    }
    if (lane == Ub / K) {
      if constexpr (MAX) {
        const bool lab = vL > vB;
        ll[b] = lab ? vL : vB;
        bk.fin[b] = lab ? 1 : 0;
      } else {
        const double z = logaddexp_d(vB, vL);
        ll[b] = z;
        nll[b] = (float)(-z);
      }
    }
  } else if constexpr (!MAX) {
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      pb[j] = ld(cellB(Tb - 1 - j));
#pragma unroll
      for (int k = 0; k < K; ++k) pl[j][k] = ld(cellL(ulo + k, Tb - 1 - j));
    }
    for (int r = 0; r < nrounds; ++r) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        const int t = Tb - 1 - (r * PF + j);
        const double carryB = shfl_down1(sB[0], lane);   // beta_{t+1} of the next lane's first blank and first label state
        const double carryL = shfl_down1(sL[0], lane);
        const float cb = pb[j];
        float cl[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cl[k] = pl[j][k];
        pb[j] = ld(cellB(t - PF));
#pragma unroll
        for (int k = 0; k < K; ++k) pl[j][k] = ld(cellL(ulo + k, t - PF));
        const bool row = t >= 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int u = ulo + k;
          const double nextB = k < K - 1 ? sB[k + 1] : carryB;
          const double nextL = k < K - 1 ? sL[k + 1] : carryL;
          const bool okB = row && u <= Ub, okL = row && u < Ub;
          double nB, nL;
          if (t == Tb - 1) {   // (uniform)
            nB = u == Ub ? (double)cb : NEG_INF;
            nL = u == Ub - 1 ? (double)cl[k] : NEG_INF;
          } else {
            nB = (double)cb + logaddexp_d(sB[k], sL[k]);
            double x = logaddexp_d(sL[k], nextB);
            x = skip[k] ? logaddexp_d(x, nextL) : x;
            nL = (double)cl[k] + x;
          }
          st(rB, nB, okB ? u * T + t : -1);
          st(rL, nL, okL ? u * T + t : -1);
          sB[k] = okB ? nB : sB[k];
          sL[k] = okL ? nL : sL[k];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// gradient with respect to the raw logits.  grid (ceil(T/32), B), 256 threads.
// dynamic LDS: occ[TT][U1] (label-state occupancies) | bpart[8][TT] | bsum[TT] | lse_s[TT] | ys[U1] | ch[U1] | islab[ceil(V/32)]
// Who writes dz[t][v]: the blank entry and every entry that is no label of the utterance come from the pass along v; the entry of a
// label value comes from the lane of that value's FIRST position, which adds the occupancies of the value's positions in position
// order (chain built by ctc_terms_kernel).  Every entry has one writer and every sum one order.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ctc_grad_kernel(const float* __restrict__ Z, long z_sb, long z_st,
                                                       const int* __restrict__ labels, const int* __restrict__ t_lens,
                                                       const int* __restrict__ u_lens, const float* __restrict__ em,
                                                       const float* __restrict__ lse, const int* __restrict__ chain,
                                                       const double* __restrict__ aB, const double* __restrict__ aL,
                                                       const double* __restrict__ bB, const double* __restrict__ bL,
                                                       const double* __restrict__ ll, int T, int U, int V, int blank,
                                                       float gscale_in, const float* __restrict__ gvec, int gvec_stride,
                                                       float* __restrict__ dZ) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int U1 = U + 1;
  float* occ = reinterpret_cast<float*>(smem);
  float* bpart = occ + TT * U1;
  float* bsum = bpart + 8 * TT;
  float* lse_s = bsum + TT;
  int* ys = reinterpret_cast<int*>(lse_s + TT);
  int* ch = ys + U1;
  unsigned* islab = reinterpret_cast<unsigned*>(ch + U1);

  const int b = blockIdx.y, t0 = blockIdx.x * TT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = clampi(t_lens[b], 0, T), Ub = clampi(u_lens[b], 0, U);
  const double logZ = ll[b];
  const float g = gvec ? gscale_in * gvec[(long)b * gvec_stride] : gscale_in;  // upstream gradient per utterance (stride 0: one scalar)
  const float* Zb = Z + (long)b * z_sb;
  float* dZb = dZ + (long)b * z_sb;
  const int tend = min(t0 + TT, T);

  if (t0 >= Tb || logZ == NEG_INF) {   // (uniform) padded frames; a row without any path: exact zeros
    for (int t = t0 + wave; t < tend; t += 4)
      for (int v = lane; v < V; v += 64) dZb[(long)t * z_st + v] = 0.f;
    return;
  }
  const int nvw = (V + 31) / 32;
  for (int i = tid; i < nvw; i += 256) islab[i] = 0u;
  for (int i = tid; i < Ub; i += 256) {
    ys[i] = labels[(long)b * U + i];
    ch[i] = chain[(long)b * U1 + i];
  }
  if (tid < TT) lse_s[tid] = (t0 + tid < Tb) ? lse[(long)b * T + t0 + tid] : 0.f;
  __syncthreads();
  for (int i = tid; i < Ub; i += 256) {
    const int y = ys[i];
    if (y >= 0 && y < V) atomicOr(&islab[y >> 5], 1u << (y & 31));   // (an integer OR: the result does not depend on the order)
  }
  // occupancies of the tile: thread -> (position u = i / 32, frame i % 32), so alpha / beta / em rows are read coalesced and a thread
  // stays on one frame; its blank-state occupancies add up in position order, then the 8 partial sums per frame in a fixed order
  const long rowbase = (long)b * U1 * T;
  const int tl_own = tid & (TT - 1);
  float bacc = 0.f;
  for (int i = tid; i < TT * (Ub + 1); i += 256) {
    const int u = i / TT, t = t0 + tl_own;
    float ol = 0.f;
    if (t < Tb) {
      const long o = rowbase + (long)u * T + t;
      const float eb = em[rowbase + t];
      bacc += expf((float)(aB[o] + bB[o] - (double)eb - logZ));
      if (u < Ub) ol = expf((float)(aL[o] + bL[o] - (double)em[o + T] - logZ));
    }
    occ[tl_own * U1 + u] = ol;
  }
  bpart[(tid >> 5) * TT + tl_own] = bacc;
  __syncthreads();
  if (tid < TT) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) s += bpart[w * TT + tid];
    bsum[tid] = s;
  }
  __syncthreads();

  for (int tl = wave; t0 + tl < tend; tl += 4) {
    const int t = t0 + tl;
    const float* z = Zb + (long)t * z_st;
    float* dz = dZb + (long)t * z_st;
    if (t >= Tb) {
      for (int v = lane; v < V; v += 64) dz[v] = 0.f;
      continue;
    }
    const float l = lse_s[tl];
    for (int v = lane; v < V; v += 64) {
      const float p = expf(z[v] - l);
      if (v == blank) dz[v] = g * (p - bsum[tl]);
      else if (!((islab[v >> 5] >> (v & 31)) & 1u)) dz[v] = g * p;
    }
    const float* orow = occ + tl * U1;
    for (int u0 = 0; u0 < Ub; u0 += 64) {
      const int u = u0 + lane;
      if (u < Ub && (ch[u] & CH_FIRST)) {
        const int y = ys[u];
        if (y >= 0 && y < V && y != blank) {
          float s = orow[u];
          for (int n = ch[u] & CH_NONE; n < Ub; n = ch[n] & CH_NONE) s += orow[n];   // (positions increase along a chain: at most Ub steps)
          dz[y] = g * (expf(z[y] - l) - s);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// greedy decode.  grid (B), 1024 threads; frames in chunks of 1024: argmax per frame (a wavefront per frame, ties to the lowest
// index), then a thread per frame: keep a token that is not blank and differs from the previous frame's argmax; positions by ballot.
// ------------------------------------------------------------------------------------------------
constexpr int GR_T = 1024;

__global__ void __launch_bounds__(GR_T) ctc_greedy_kernel(const float* __restrict__ Z, long z_sb, long z_st,
                                                          const int* __restrict__ t_lens, int T, int V, int blank,
                                                          int* __restrict__ tokens, int* __restrict__ counts,
                                                          int* __restrict__ frames) {
  __shared__ int am[GR_T];
  __shared__ int wcnt[GR_T / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = clampi(t_lens[b], 0, T);
  const float* Zb = Z + (long)b * z_sb;
  int base = 0, prev = blank;   // (no frame before the first: nothing to differ from)
  for (int c0 = 0; c0 < Tb; c0 += GR_T) {
    const int n = min(GR_T, Tb - c0);
    for (int tl = wave; tl < n; tl += GR_T / 64) {
      const float* z = Zb + (long)(c0 + tl) * z_st;
      float best = -__builtin_huge_valf();
      int bi = 0x7fffffff;
      for (int v = lane; v < V; v += 64) {
        const float x = z[v];
        if (x > best) { best = x; bi = v; }   // ascending v: the first of equal values stays
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (lane == 0) am[tl] = bi;
    }
    __syncthreads();
    const int mine = tid < n ? am[tid] : blank;
    const int before = tid == 0 ? prev : am[tid - 1];
    const bool keep = tid < n && mine != blank && mine != before;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    const int last = am[n - 1];
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int w = 0; w < GR_T / 64; ++w) {
      off += w < wave ? wcnt[w] : 0;
      total += wcnt[w];
    }
    if (keep) {
      const long o = (long)b * T + off + __popcll(bal & ((1ull << lane) - 1ull));
      tokens[o] = mine;
      if (frames) frames[o] = c0 + tid;
    }
    base += total;
    prev = last;
    __syncthreads();   // am / wcnt are rewritten by the next chunk
  }
  if (tid == 0) counts[b] = base;
}

// Back-trace and outputs of the alignment: one workgroup per utterance.  Thread 0 walks the path backwards a WORD at a time: inside a
// state the next event is the highest set bit at or below the current frame (a zero word is up to 32 stay steps at once, a set bit is
// found by a leading-zero count): about 2 U_b + T_b / 32 dependent loads instead of T_b.  The utterance's part of the three planes is
// first copied to LDS (coalesced) when the host found room for it; otherwise the walk reads the workspace.  Then every thread writes
// outputs: first / last from the walk, path by a binary search of the frame among the spans, token_logp as the ascending fp64 sum of
// the label's emission row over its span.  dynamic LDS: first[U1] | last[U1] | ys[U1] | table (in_lds)
__global__ void __launch_bounds__(256) ctc_backtrace_kernel(const unsigned* __restrict__ bp, const float* __restrict__ em,
                                                            const int* __restrict__ labels, const int* __restrict__ t_lens,
                                                            const int* __restrict__ u_lens, const double* __restrict__ score,
                                                            const int* __restrict__ fin, int T, int U, int NW, int in_lds,
                                                            int blank, int* __restrict__ first, int* __restrict__ last,
                                                            int* __restrict__ path, double* __restrict__ token_logp) {
  extern __shared__ int bt_s[];
  const int b = blockIdx.x, tid = threadIdx.x, U1 = U + 1;
  const int Tb = clampi(t_lens[b], 0, T), Ub = clampi(u_lens[b], 0, U);
  int* first_s = bt_s;
  int* last_s = first_s + U1;
  int* ys = last_s + U1;
  unsigned* tab = reinterpret_cast<unsigned*>(ys + U1);
  if (score[b] == NEG_INF) {   // (uniform) no path: also Tb = 0
    for (int u = tid; u < U; u += 256) {
      first[(long)b * U + u] = -1;
      last[(long)b * U + u] = -1;
      if (token_logp) token_logp[(long)b * U + u] = 0.0;
    }
    if (path)
      for (int t = tid; t < T; t += 256) path[(long)b * T + t] = -1;
    return;
  }
  for (int u = tid; u < Ub; u += 256) ys[u] = labels[(long)b * U + u];
  const unsigned* tp = bp + (long)b * 3 * U1 * NW;
  int stride = NW, pstride = U1 * NW;
  if (in_lds) {
    const int nwb = ((Tb - 1) >> 5) + 1, per = (Ub + 1) * nwb;   // words per row, per plane, this utterance wrote or may read
    for (int i = tid; i < 3 * per; i += 256) {
      const int p = i / per, rem = i % per;
      tab[i] = tp[(long)p * U1 * NW + (rem / nwb) * NW + rem % nwb];
    }
    tp = tab;
    stride = nwb;
    pstride = per;
  }
  __syncthreads();
  if (tid == 0) {
    int t = Tb - 1, inlab = fin[b] != 0 && Ub > 0, u = inlab ? Ub - 1 : Ub;
    if (inlab) last_s[u] = t;
    while (t >= 0) {
      const int wi = t >> 5;
      const unsigned mask = 0xffffffffu >> (31 - (t & 31));   // frames <= t of the block
      if (inlab) {
        const unsigned b1 = tp[pstride + u * stride + wi] & mask, b2 = tp[2 * pstride + u * stride + wi] & mask;
        const unsigned w = b1 | b2;
        if (w == 0u) {
          t = (t & ~31) - 1;
          if (t < 0) first_s[u] = 0;   // the path starts in this label state (u = 0)
          continue;
        }
        const int bit = 31 - __clz(w);
        const int te = (t & ~31) + bit;   // the frame at which the path entered the state: >= 1, frame 0 never carries a bit
        first_s[u] = te;
        t = te - 1;
        if ((b2 >> bit) & 1u) {
          if (u == 0) break;   // (never on bits this call wrote)
          last_s[--u] = t;
        } else {
          inlab = 0;
        }
      } else {
        const unsigned w = tp[u * stride + wi] & mask;
        if (w == 0u) {
          t = (t & ~31) - 1;
          continue;
        }
        if (u == 0) break;   // (never on bits this call wrote)
        t = (t & ~31) + 31 - __clz(w) - 1;
        inlab = 1;
        last_s[--u] = t;
      }
    }
  }
  __syncthreads();
  for (int u = tid; u < U; u += 256) {
    const bool ok = u < Ub;
    const int f = ok ? clampi(first_s[u], 0, Tb - 1) : -1, l = ok ? clampi(last_s[u], 0, Tb - 1) : -1;
    first[(long)b * U + u] = f;
    last[(long)b * U + u] = l;
    if (token_logp) {
      double s = 0.0;
      if (ok) {
        const float* row = em + ((long)b * U1 + u + 1) * T;
        for (int t = f; t <= l; ++t) s += (double)row[t];
      }
      token_logp[(long)b * U + u] = s;
    }
  }
  if (path) {
    for (int t = tid; t < T; t += 256) {
      int tok = -1;
      if (t < Tb) {
        int lo = 0, hi = Ub;   // the number of labels whose span starts at or before t
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (first_s[mid] <= t) lo = mid + 1;
          else hi = mid;
        }
        tok = (lo > 0 && t <= last_s[lo - 1]) ? ys[lo - 1] : blank;
      }
      path[(long)b * T + t] = tok;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Host half, after the pattern of loss.hip.  Every exported loss / alignment entry fills ONE description of its call, a CtcCall,
// checks the whole call before any device work (check_ctc, which also carves the workspace) and then composes the stages:
// terms -> sweep (forward), grad (backward, on the workspace the forward left), terms -> viterbi + back-trace (alignment).
// ------------------------------------------------------------------------------------------------
struct CtcCall {
  const char* who = "";   // the entry's name, for messages
  const float* logits = nullptr;
  int64_t z_sb = 0, z_st = 0;
  const int32_t *labels = nullptr, *t_lens = nullptr, *u_lens = nullptr;
  int B = 0, T = 0, U = 0, V = 0, blank = 0;
  float* nll = nullptr;   // forward
  // backward: upstream scale, per-utterance upstream gradients, the gradient
  float gscale = 1.f;
  const float* gvec = nullptr;
  int gvec_stride = 0;
  float* dlogits = nullptr;
  // alignment
  int32_t *first = nullptr, *last = nullptr, *path = nullptr;
  double *token_logp = nullptr, *score = nullptr;
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  hipStream_t stream = nullptr;
};

struct CtcWs {
  float *em, *lse;
  int* chain;
  double *aB, *aL, *bB, *bL, *ll;   // the loss
  unsigned* bp;                     // the alignment: back-pointer planes bp[B][3][U + 1][nw = ceil(T/32)] and the final states
  int* fin;
  int nw;
  size_t total;
};

enum class CtcDrive { Forward, Backward, Align };

// the loss: alpha (blank, label states) | beta (the same) | logZ | em | lse | chain;  the alignment: em | lse | chain | bp | fin
CtcWs carve_ctc(void* ws, int B, int T, int U, bool align) {
  CtcWs w{};
  Carver c{reinterpret_cast<char*>(ws)};
  const size_t U1 = (size_t)U + 1, cells = (size_t)B * T * U1;
  if (!align) {
    w.aB = c.take<double>(cells * 8);
    w.aL = c.take<double>(cells * 8);
    w.bB = c.take<double>(cells * 8);
    w.bL = c.take<double>(cells * 8);
    w.ll = c.take<double>((size_t)B * 8);
  }
  w.em = c.take<float>(cells * 4);
  w.lse = c.take<float>((size_t)B * T * 4);
  w.chain = c.take<int>((size_t)B * U1 * 4);
  if (align) {
    w.nw = (int)ceil_div(T, 32);
    w.bp = c.take<unsigned>((size_t)B * 3 * U1 * w.nw * 4);
    w.fin = c.take<int>((size_t)B * 4);
  }
  w.total = c.off;
  return w;
}

constexpr size_t LDS_MAX = 160 * 1024;
size_t grad_lds_bytes(int U, int V) {
  return (size_t)TT * (U + 1) * 4 + (8 * TT + 2 * TT) * 4 + (size_t)(U + 1) * 8 + (size_t)ceil_div(V, 32) * 4;
}

// Every argument check of every entry, before any device work; then the workspace, carved, and its size.
int check_ctc(const CtcCall& c, CtcDrive drive, CtcWs* w) {
  const char* what = c.who;
  const int B = c.B, T = c.T, U = c.U, V = c.V;
  RNNT_CHECK_ARG(B >= 1 && T >= 1 && U >= 0 && V >= 1, "%s: B, T, V must be positive and U >= 0 (B=%d T=%d U=%d V=%d)", what, B, T, U, V);
  RNNT_CHECK_ARG(c.blank >= 0 && c.blank < V, "%s: blank %d outside [0,%d)", what, c.blank, V);
  RNNT_CHECK_ARG(U <= 511, "%s: U = %d exceeds the 511 labels one wavefront sweeps", what, U);
  RNNT_CHECK_ARG((int64_t)(U + 1) * T * 8 < (1ll << 31), "%s: one utterance's lattice (T = %d x U+1 = %d, fp64) exceeds the 2 GB a buffer resource addresses", what, T, U + 1);
  RNNT_CHECK_ARG(grad_lds_bytes(U, V) <= LDS_MAX, "%s: V = %d with U = %d does not fit the gradient kernel's LDS tables", what, V, U);
  RNNT_CHECK_ARG(c.logits && c.t_lens && c.u_lens, "%s: null logits/lengths", what);
  RNNT_CHECK_ARG(U == 0 || c.labels, "%s: null labels", what);
  RNNT_CHECK_ARG(c.z_sb >= 1 && c.z_st >= V, "%s: logits strides (z_sb = %lld, z_st = %lld) must be positive, z_st >= V", what, (long long)c.z_sb, (long long)c.z_st);
  switch (drive) {
    case CtcDrive::Forward:
      RNNT_CHECK_ARG(c.nll, "%s: null nll", what);
      break;
    case CtcDrive::Backward:
      RNNT_CHECK_ARG(c.dlogits, "%s: null dlogits", what);
      RNNT_CHECK_ARG(c.gvec_stride == 0 || c.gvec_stride == 1, "%s: gvec_stride must be 0 (one scalar) or 1 (per utterance)", what);
      break;
    case CtcDrive::Align:
      RNNT_CHECK_ARG(c.score, "%s: null score", what);
      RNNT_CHECK_ARG(U == 0 || (c.first && c.last), "%s: null first/last", what);
      break;
  }
  *w = carve_ctc(c.workspace, B, T, U, drive == CtcDrive::Align);
  RNNT_CHECK_ARG(c.workspace && c.workspace_bytes >= w->total, "%s: workspace too small (%zu < %zu)", what, c.workspace_bytes, w->total);
  return RNNT_OK;
}

// stage 1 of the loss and of the alignment: the row log-sum-exp, the emission rows and the label chains
int stage_terms(const CtcCall& c, const CtcWs& w) {
  {
    ProfScope prof(RNNT_K_LSE, 4.0 * (double)c.B * c.T * c.V + 4.0 * (double)c.B * c.T * (c.U + 1), c.stream);
    hipLaunchKernelGGL(ctc_terms_kernel, dim3((unsigned)ceil_div(c.T, TT), c.B), dim3(256), 0, c.stream, c.logits, (long)c.z_sb, (long)c.z_st,
                       c.labels, c.t_lens, c.u_lens, c.T, c.U, c.V, c.blank, w.em, w.lse, w.chain);
  }
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// stage 2 of the loss: the alpha | beta sweep, logZ and the NLL.  Booked under the lattice-sweep kind of the RNN-T loss: the
// profiler's kinds are part of the ABI, which CTC leaves as it is
int stage_sweep(const CtcCall& c, const CtcWs& w) {
  // read the emission rows, write both states of a position (fp64)
  ProfScope prof(RNNT_K_ALPHABETA, 2.0 * (4.0 + 16.0) * (double)c.B * c.T * (c.U + 1), c.stream);
  dispatch_k(c.U + 1, [&](auto k) {
    hipLaunchKernelGGL((ctc_sweep_kernel<decltype(k)::value>), dim3(c.B, 2), dim3(64), 0, c.stream, w.em, c.labels, c.t_lens, c.u_lens, c.T,
                       c.U, w.aB, w.aL, w.bB, w.bL, w.ll, c.nll);
  });
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// the backward: the workspace still holds the emission rows, alpha, beta and logZ of rnnt_hip_ctc_loss_fwd on the SAME operands
int stage_grad(const CtcCall& c, const CtcWs& w) {
  const size_t lds = grad_lds_bytes(c.U, c.V);
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)ctc_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_LATGRAD, 2.0 * 4.0 * (double)c.B * c.T * c.V + 36.0 * (double)c.B * c.T * (c.U + 1), c.stream);
  hipLaunchKernelGGL(ctc_grad_kernel, dim3((unsigned)ceil_div(c.T, TT), c.B), dim3(256), lds, c.stream, c.logits, (long)c.z_sb, (long)c.z_st,
                     c.labels, c.t_lens, c.u_lens, w.em, w.lse, w.chain, w.aB, w.aL, w.bB, w.bL, w.ll, c.T, c.U, c.V, c.blank, c.gscale, c.gvec,
                     c.gvec_stride, c.dlogits);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// stage 2 of the alignment: the max-plus sweep (read the emission rows, write three bits per position), booked under the
// lattice-sweep kind like the sweeps of the loss, then the back-trace under the kind of the small kernels, so that a profile shows
// its share: the kinds are part of the ABI
int stage_viterbi(const CtcCall& c, const CtcWs& w) {
  hipStream_t s = c.stream;
  const double cells = (double)c.B * c.T * (c.U + 1);
  {
    ProfScope prof(RNNT_K_ALPHABETA, (4.0 + 3.0 / 8.0) * cells, s);
    dispatch_k(c.U + 1, [&](auto k) {
      hipLaunchKernelGGL((ctc_sweep_kernel<decltype(k)::value, true, CtcBackPtr>), dim3(c.B, 1), dim3(64), 0, s, w.em, c.labels, c.t_lens,
                         c.u_lens, c.T, c.U, (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, c.score,
                         (float*)nullptr, CtcBackPtr{w.bp, w.nw, w.fin});
    });
  }
  RNNT_CHECK_LAUNCH();
  ProfScope prof(RNNT_K_MISC, 3.0 / 8.0 * cells + 4.0 * (double)c.B * (c.T + 2 * c.U), s);
  const size_t small = (size_t)3 * (c.U + 1) * 4, table = (size_t)3 * (c.U + 1) * w.nw * 4;
  const int in_lds = small + table <= 64 * 1024;
  hipLaunchKernelGGL(ctc_backtrace_kernel, dim3(c.B), dim3(256), in_lds ? small + table : small, s, w.bp, w.em, c.labels, c.t_lens, c.u_lens,
                     c.score, w.fin, c.T, c.U, w.nw, in_lds, c.blank, c.first, c.last, c.path, c.token_logp);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

// ---- the exported entries: each fills a CtcCall from its positional arguments (the names below are the parameters') ----
#define FILL_CTC(c, WHO)                                                                                                          \
  CtcCall c;                                                                                                                      \
  c.who = WHO, c.logits = logits, c.z_sb = z_sb, c.z_st = z_st, c.labels = labels, c.t_lens = t_lens, c.u_lens = u_lens, c.B = B, \
  c.T = T, c.U = U, c.V = V, c.blank = blank, c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = (hipStream_t)stream

extern "C" size_t rnnt_hip_ctc_loss_workspace_bytes(int32_t B, int32_t T, int32_t U, int32_t V) {
  if (B < 1 || T < 1 || U < 0 || V < 1) return 0;
  return carve_ctc(nullptr, B, T, U, false).total;
}

extern "C" int rnnt_hip_ctc_loss_fwd(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* labels, const int32_t* t_lens,
                                     const int32_t* u_lens, int32_t B, int32_t T, int32_t U, int32_t V, int32_t blank, float* nll,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  FILL_CTC(c, "ctc_loss_fwd");
  c.nll = nll;
  CtcWs w;
  if (int rc = check_ctc(c, CtcDrive::Forward, &w)) return rc;
  if (int rc = stage_terms(c, w)) return rc;
  return stage_sweep(c, w);
}

extern "C" int rnnt_hip_ctc_loss_bwd(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* labels, const int32_t* t_lens,
                                     const int32_t* u_lens, int32_t B, int32_t T, int32_t U, int32_t V, int32_t blank, float gscale,
                                     const float* gvec, int32_t gvec_stride, float* dlogits, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  FILL_CTC(c, "ctc_loss_bwd");
  c.gscale = gscale, c.gvec = gvec, c.gvec_stride = gvec_stride, c.dlogits = dlogits;
  CtcWs w;
  if (int rc = check_ctc(c, CtcDrive::Backward, &w)) return rc;
  return stage_grad(c, w);
}

extern "C" int rnnt_hip_ctc_greedy(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T,
                                   int32_t V, int32_t blank, int32_t* tokens, int32_t* counts, int32_t* frames, void* stream) {
  RNNT_CHECK_ARG(B >= 1 && T >= 1 && V >= 1, "ctc_greedy: dims must be positive (B=%d T=%d V=%d)", B, T, V);
  RNNT_CHECK_ARG(blank >= 0 && blank < V, "ctc_greedy: blank %d outside [0,%d)", blank, V);
  RNNT_CHECK_ARG(logits && t_lens && tokens && counts, "ctc_greedy: null logits/lengths/tokens/counts");
  RNNT_CHECK_ARG(z_sb >= 1 && z_st >= V, "ctc_greedy: logits strides (z_sb = %lld, z_st = %lld) must be positive, z_st >= V", (long long)z_sb, (long long)z_st);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)B * T * V, s);
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(GR_T), 0, s, logits, (long)z_sb, (long)z_st, t_lens, T, V, blank, tokens, counts,
                     frames);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

/* ---- forced alignment under CTC (include/rnnt_hip.h): the terms kernel of the loss, max-plus sweep, back-trace ---- */
extern "C" size_t rnnt_hip_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t U, int32_t V) {
  if (B < 1 || T < 1 || U < 0 || V < 1) return 0;
  return carve_ctc(nullptr, B, T, U, true).total;
}

extern "C" int rnnt_hip_ctc_align(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* labels, const int32_t* t_lens,
                                  const int32_t* u_lens, int32_t B, int32_t T, int32_t U, int32_t V, int32_t blank, int32_t* first,
                                  int32_t* last, int32_t* path, double* token_logp, double* score, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  FILL_CTC(c, "ctc_align");
  c.first = first, c.last = last, c.path = path, c.token_logp = token_logp, c.score = score;
  CtcWs w;
  if (int rc = check_ctc(c, CtcDrive::Align, &w)) return rc;
  if (int rc = stage_terms(c, w)) return rc;
  return stage_viterbi(c, w);
}
