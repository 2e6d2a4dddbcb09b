// CTC prefix beam search on per-frame logits (the encoder's CTC head), with token fusion, for gfx950.  DESIGN.md §19.
//
// Definition (include/rnnt_hip.h states it in full).  lp[t,v] = z[t,v] - logsumexp_v z[t,:] in fp32, as ctc_terms_kernel (ctc.hip).
// A hypothesis is a prefix l (tokens without blanks) with pb / pnb, the fp64 log-mass of its paths ending in blank / in l[-1];
// p = logaddexp(pb, pnb).  Frame t, member at rank r with last token e, candidate tokens C_t = {k != blank: lp[t,k] >= min_logp}:
//   survivor   id r(V+1)      : pb' = p + lp[t,blank];  pnb' = logaddexp(pnb + lp[t,e], extension term of its parent, if the parent
//                               is in the beam and l[-1] is in C_t)
//   extension  id r(V+1)+1+k  : pnb' = (k == e ? pb : p) + lp[t,k], unless l + k is a member of the beam: then it is that
//                               member's survivor
//   key = logaddexp(pb', pnb') + total'; the first W by (key descending, id ascending) are the next beam.
//
// Prefix tree: nodes (parent, token, frame, first_child, next_sibling), append-only, node 0 = the empty prefix.  A node is looked up
// among its parent's children before it is created, so a prefix has ONE node however often it is pruned and reached again, and
// "l + k is a member" is the comparison (parent node, token) against the at most W members.
//
// One workgroup of 1024 threads per utterance, no communication between workgroups.  Per frame:
//   fill     every candidate's key as an order-preserving 64-bit integer into the utterance's scratch (0 = no candidate); lanes along
//            the flat candidate index, so along v within a member's row
//   select   the W best by (key descending, lowest id), gathered into LDS and ranked there: select_top, select_rank
//            (search_shared.hpp)
//   build    the next beam in rank order: survivors copy, extensions find or create their node (the prefix tree of
//            search_shared.hpp)
// Every sum has one fixed order (logaddexp_d is symmetric in its arguments) and every output one writer: bitwise reproducible, and
// a row's result does not depend on the batch around it.  Loops are bounded by T, W, V or the 11 digits of the select.
#include "search_shared.hpp"

namespace rnnt {
namespace {

constexpr int CB_THREADS = 1024;
constexpr int CB_WMAX = 128;
constexpr int CB_IDBITS = 24;   // candidate ids r (V+1) + j fit 24 bits: three 8-bit digits break exact ties

struct CbBeam {
  double pb[CB_WMAX], pnb[CB_WMAX], tot[CB_WMAX];
  int node[CB_WMAX], st[CB_WMAX], tok[CB_WMAX], par[CB_WMAX];   // tok / par: the node's token and parent (-1 for the empty prefix)
};

struct CbShared {
  CbBeam beam[2];
  double p[CB_WMAX], cpb[CB_WMAX], cpnb[CB_WMAX];   // p of the members; pb' / pnb' of their survivors
  int src[CB_WMAX];                                 // rank of the member whose extension by tok[r] is member r (-1: none)
  SelectState<CB_WMAX> sel;
  int pending[CB_WMAX];                             // by rank: its node is still to be created
  int nnodes;
};

// FUSE: the fusion policy (search_shared.hpp).  FUSE_DENSE reads farc / fnext at (state, token); FUSE_NGRAM asks ngram_lookup (ng)
// for the same two values at the same two places, the candidate-key fill and the build of the selected extensions.
template <int FUSE>
__global__ void __launch_bounds__(CB_THREADS) ctc_beam_kernel(const float* __restrict__ Z, long z_sb, long z_st,
                                                              const int* __restrict__ t_lens, int T, int V, int blank, int W,
                                                              float min_logp, const int* __restrict__ fnext,
                                                              const float* __restrict__ farc, const float* __restrict__ ffinal,
                                                              int n_states, float* __restrict__ lse_ws, u64* __restrict__ key_ws,
                                                              int* __restrict__ node_ws, int* __restrict__ tokens,
                                                              int* __restrict__ lens, double* __restrict__ scores,
                                                              double* __restrict__ fused, int* __restrict__ frames,
                                                              int* __restrict__ counts, const NgramLm ng) {
  constexpr bool FUSED = FUSE != FUSE_NONE;
  __shared__ CbShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = clampi(t_lens[b], 0, T);
  const int V1 = V + 1;
  const long maxn = 1 + (long)W * T;
  const float* Zb = Z + (long)b * z_sb;
  float* lse = lse_ws + (long)b * T;
  u64* ck = key_ws + (long)b * W * V1;
  const PrefixTree nd = tree_view(node_ws + (long)b * 5 * maxn, maxn);

  // row log-sum-exp of every valid frame, the arithmetic of ctc_terms_kernel: a wavefront per frame, lanes along v
  for (int t = wave; t < Tb; t += CB_THREADS / 64) {
    const float* z = Zb + (long)t * z_st;
    float m = -__builtin_huge_valf();
    for (int v = lane; v < V; v += 64) m = fmaxf(m, z[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(z[v] - m);
    s = wave_sum(s);
    if (lane == 0) lse[t] = m + logf(s);
  }
  if (tid < 2 * CB_WMAX) {   // every slot of both beams holds a valid (dead) member from the start
    CbBeam& c = sh.beam[tid / CB_WMAX];
    const int r = tid % CB_WMAX;
    c.pb[r] = NEG_INF; c.pnb[r] = NEG_INF; c.tot[r] = 0.0;
    c.node[r] = 0; c.st[r] = 0; c.tok[r] = -1; c.par[r] = -1;
  }
  __syncthreads();
  if (tid == 0) {
    CbBeam& c = sh.beam[0];
    c.pb[0] = 0.0; c.pnb[0] = NEG_INF; c.tot[0] = 0.0;
    c.node[0] = 0; c.st[0] = 0; c.tok[0] = -1; c.par[0] = -1;
    tree_root(nd, -1);   // the empty prefix
    sh.nnodes = 1;
  }
  __threadfence_block();
  __syncthreads();

  int n = 1, cur = 0;
  for (int t = 0; t < Tb; ++t) {
    CbBeam& c = sh.beam[cur];
    CbBeam& nw = sh.beam[cur ^ 1];
    const float* z = Zb + (long)t * z_st;
    const float l = lse[t];
    // ---- members: p, and the member (if any) whose extension by tok[r] is member r
    if (tid < n) {
      sh.p[tid] = logaddexp_d(c.pb[tid], c.pnb[tid]);
      int s = -1;
      const int par = c.par[tid];
      if (par >= 0)
        for (int r = 0; r < n; ++r)
          if (c.node[r] == par) s = r;   // (nodes of members are distinct: at most one hit)
      sh.src[tid] = s;
    }
    if (tid == 0) select_reset(sh.sel);
    __syncthreads();
    // ---- fill: keys of all n (V+1) candidates
    const int N = n * V1;
    for (int idx = tid; idx < N; idx += CB_THREADS) {
      const int r = idx / V1, j = idx - r * V1;
      u64 key = 0ull;
      if (j == 0) {
        const int e = c.tok[r], s = sh.src[r];
        const double pbn = sh.p[r] + (double)(z[blank] - l);
        double pnbn = NEG_INF;
        if (e >= 0) {
          const float le = z[e] - l;
          pnbn = c.pnb[r] + (double)le;                      // the stay term: whether or not e is a candidate token
          if (s >= 0 && le >= min_logp) {                    // its parent's extension by e, when e is one
            const double ext = (c.tok[s] == e ? c.pb[s] : sh.p[s]) + (double)le;
            pnbn = logaddexp_d(pnbn, ext);
          }
        }
        sh.cpb[r] = pbn;
        sh.cpnb[r] = pnbn;
        const double k = logaddexp_d(pbn, pnbn) + (FUSED ? c.tot[r] : 0.0);
        if (k > NEG_INF) key = sortable_key(k);
      } else {
        const int k = j - 1;
        const float lk = z[k] - l;
        if (k != blank && lk >= min_logp) {
          double x = (k == c.tok[r] ? c.pb[r] : sh.p[r]) + (double)lk;
          if constexpr (FUSE == FUSE_NGRAM) {   // only a candidate that passed the prune walks the tables
            int unused;
            x += c.tot[r] + (double)ngram_lookup(ng, c.st[r], k, unused);
          } else if (FUSED) x += c.tot[r] + (double)farc[(long)c.st[r] * V + k];
          if (x > NEG_INF) key = sortable_key(x);
        }
      }
      ck[idx] = key;
    }
    __threadfence_block();
    __syncthreads();
    // an extension that is a member of the beam is that member's survivor: its own slot is no candidate (one writer: member r)
    if (tid < n && sh.src[tid] >= 0) ck[sh.src[tid] * V1 + 1 + c.tok[tid]] = 0ull;
    __threadfence_block();
    __syncthreads();

    // ---- select the min(W, candidates) best in the order (key descending, id ascending)
    const int m = select_top<CB_WMAX, CB_IDBITS, CB_THREADS>(sh.sel, ck, N, W);
    // ---- build the next beam in rank order
    int rank = -1, kk = -1;
    if (tid < m) {
      const int id = sh.sel.sel_id[tid];
      rank = select_rank(sh.sel, tid, m);
      const int r = id / V1, j = id - r * V1;
      int pend = 0;
      if (j == 0) {
        nw.pb[rank] = sh.cpb[r]; nw.pnb[rank] = sh.cpnb[r]; nw.tot[rank] = c.tot[r];
        nw.node[rank] = c.node[r]; nw.st[rank] = c.st[r]; nw.tok[rank] = c.tok[r]; nw.par[rank] = c.par[r];
      } else {
        kk = j - 1;
        const float lk = z[kk] - l;
        nw.pb[rank] = NEG_INF;
        nw.pnb[rank] = (kk == c.tok[r] ? c.pb[r] : sh.p[r]) + (double)lk;
        if constexpr (FUSE == FUSE_NGRAM) {
          int ns;
          const float arc = ngram_lookup(ng, c.st[r], kk, ns);   // the fill's value: the same walk, the same bits
          nw.tot[rank] = c.tot[r] + (double)arc;
          nw.st[rank] = ns;
        } else if (FUSED) {
          const long o = (long)c.st[r] * V + kk;
          nw.tot[rank] = c.tot[r] + (double)farc[o];
          nw.st[rank] = clampi(fnext[o], 0, n_states - 1);
        } else {
          nw.tot[rank] = 0.0;
          nw.st[rank] = 0;
        }
        const int par = c.node[r];
        nw.tok[rank] = kk;
        nw.par[rank] = par;
        const int ch = tree_find_child(nd, par, kk, V);   // the prefix's node, if it was created before
        nw.node[rank] = ch;
        pend = ch < 0 ? 1 : 0;
      }
      sh.pending[rank] = pend;
    }
    __syncthreads();
    if (tid == 0) tree_number(sh.pending, nw.node, m, sh.nnodes);
    __syncthreads();
    if (rank >= 0 && sh.pending[rank]) tree_link(nd, maxn, sh.pending, nw.par, nw.node, rank, m, kk, t);
    __threadfence_block();
    __syncthreads();
    n = m;
    cur ^= 1;
  }

  // ---- output: stable order by score (FUSED: score + total + final[state]), then the back-trace of every hypothesis
  CbBeam& c = sh.beam[cur];
  if (tid < n) {
    const double sc = logaddexp_d(c.pb[tid], c.pnb[tid]);
    sh.p[tid] = sc;
    sh.cpb[tid] = FUSED ? (sc + c.tot[tid]) + (double)ffinal[FUSE == FUSE_NGRAM ? clampi(c.st[tid], 0, n_states - 1) : c.st[tid]] : sc;
  }
  __syncthreads();
  if (tid < n) {
    const double key = sh.cpb[tid];
    const long base = (long)b * W + output_slot(sh.cpb, tid, n, W);
    lens[base] = tree_backtrace(nd, c.node[tid], false, T, tokens + base * T, frames ? frames + base * T : nullptr);
    scores[base] = sh.p[tid];
    if (FUSED) fused[base] = key;
  }
  if (tid == 0) counts[b] = n;
}

struct CbWs {
  float* lse;
  u64* keys;
  int* nodes;
  size_t total;
};

CbWs carve_cb(void* ws, int64_t B, int64_t T, int64_t V, int64_t W) {
  CbWs w;
  char* p = reinterpret_cast<char*>(ws);
  size_t off = 0;
  w.keys = reinterpret_cast<u64*>(ws_take(p, off, (size_t)B * W * (V + 1) * 8));
  w.nodes = reinterpret_cast<int*>(ws_take(p, off, (size_t)B * 5 * (1 + W * T) * 4));
  w.lse = reinterpret_cast<float*>(ws_take(p, off, (size_t)B * T * 4));
  w.total = off;
  return w;
}

bool cb_dims_ok(int64_t B, int64_t T, int64_t V, int64_t W) {
  return B >= 1 && T >= 1 && V >= 2 && W >= 1 && W <= CB_WMAX && W * (V + 1) <= (1ll << CB_IDBITS) && 1 + W * T < (1ll << 31) / 5;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" size_t rnnt_hip_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t W) {
  if (!cb_dims_ok(B, T, V, W)) return 0;
  return carve_cb(nullptr, B, T, V, W).total;
}

// the search behind both entries: fusion (dense tables), lm (backoff tables), or neither
static int cb_search(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T, int32_t V,
                     int32_t blank, int32_t W, float token_min_logp, const rnnt_beam_fusion* fusion, const rnnt_beam_ngram* lm,
                     bool ngram, int32_t* tokens, int32_t* lens, double* scores, int32_t* frames, int32_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream) {
  RNNT_CHECK_ARG(B >= 1 && T >= 1, "ctc_beam_search: B and T must be positive (B=%d T=%d)", B, T);
  RNNT_CHECK_ARG(W >= 1 && W <= CB_WMAX, "ctc_beam_search: beam width W = %d outside [1,%d]", W, CB_WMAX);
  RNNT_CHECK_ARG(V >= 2, "ctc_beam_search: V = %d < 2 (a blank and at least one token)", V);
  RNNT_CHECK_ARG(blank >= 0 && blank < V, "ctc_beam_search: blank %d outside [0,%d)", blank, V);
  int rc = check_token_min_logp(token_min_logp, "ctc_beam_search");
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(cb_dims_ok(B, T, V, W), "ctc_beam_search: W (V+1) = %lld exceeds 2^%d candidates per frame, or W T = %lld the node index",
                 (long long)W * (V + 1), CB_IDBITS, (long long)W * T);
  RNNT_CHECK_ARG(logits && t_lens && tokens && lens && scores && counts, "ctc_beam_search: null logits/lengths/tokens/lens/scores/counts");
  RNNT_CHECK_ARG(z_sb >= 1 && z_st >= V, "ctc_beam_search: logits strides (z_sb = %lld, z_st = %lld) must be positive, z_st >= V",
                 (long long)z_sb, (long long)z_st);
  if (fusion && (rc = check_fusion_struct(fusion, V, "ctc_beam_search")) != RNNT_OK) return rc;
  NgramLm ng{};
  if (ngram && (rc = check_ngram_struct(lm, V, ng, "ctc_beam_search_ngram")) != RNNT_OK) return rc;
  const CbWs w = carve_cb(workspace, B, T, V, W);
  RNNT_CHECK_ARG(workspace && workspace_bytes >= w.total, "ctc_beam_search: workspace too small (%zu < %zu)", workspace_bytes, w.total);
  RNNT_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "ctc_beam_search: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)B * T * V * (1.0 + W), s);
  if (ngram)
    hipLaunchKernelGGL((ctc_beam_kernel<FUSE_NGRAM>), dim3(B), dim3(CB_THREADS), 0, s, logits, (long)z_sb, (long)z_st, t_lens, T, V, blank,
                       W, token_min_logp, (const int*)nullptr, (const float*)nullptr, lm->final, lm->n_states, w.lse, w.keys, w.nodes,
                       tokens, lens, scores, lm->fused_scores, frames, counts, ng);
  else if (fusion)
    hipLaunchKernelGGL((ctc_beam_kernel<FUSE_DENSE>), dim3(B), dim3(CB_THREADS), 0, s, logits, (long)z_sb, (long)z_st, t_lens, T, V, blank, W,
                       token_min_logp, fusion->next, fusion->arc, fusion->final, fusion->n_states, w.lse, w.keys, w.nodes, tokens,
                       lens, scores, fusion->fused_scores, frames, counts, ng);
  else
    hipLaunchKernelGGL((ctc_beam_kernel<FUSE_NONE>), dim3(B), dim3(CB_THREADS), 0, s, logits, (long)z_sb, (long)z_st, t_lens, T, V, blank, W,
                       token_min_logp, (const int*)nullptr, (const float*)nullptr, (const float*)nullptr, 1, w.lse, w.keys, w.nodes,
                       tokens, lens, scores, (double*)nullptr, frames, counts, ng);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_ctc_beam_search(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T,
                                        int32_t V, int32_t blank, int32_t W, float token_min_logp, const rnnt_beam_fusion* fusion,
                                        int32_t* tokens, int32_t* lens, double* scores, int32_t* frames, int32_t* counts,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  return cb_search(logits, z_sb, z_st, t_lens, B, T, V, blank, W, token_min_logp, fusion, nullptr, false, tokens, lens, scores, frames,
                   counts, workspace, workspace_bytes, stream);
}

extern "C" int rnnt_hip_ctc_beam_search_ngram(const float* logits, int64_t z_sb, int64_t z_st, const int32_t* t_lens, int32_t B, int32_t T,
                                              int32_t V, int32_t blank, int32_t W, float token_min_logp, const rnnt_beam_ngram* lm,
                                              int32_t* tokens, int32_t* lens, double* scores, int32_t* frames, int32_t* counts,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  return cb_search(logits, z_sb, z_st, t_lens, B, T, V, blank, W, token_min_logp, nullptr, lm, true, tokens, lens, scores, frames, counts,
                   workspace, workspace_bytes, stream);
}
