// What the frame-synchronous searches share (ctc_beam.hip: CTC prefix beam search; beam_sync.hip: transducer beam search with
// batched steps): the top-W select over a frame's candidate keys, the prefix tree, the stable output order,
// and the host-side checks of the fusion struct and of token_min_logp (those also serve beam_shared.hpp's fused entries).
// One workgroup of THREADS threads owns one utterance; every function here is called by all of its threads unless it says
// otherwise.
#pragma once
#include "common.hpp"
#include "lattice_shared.hpp"

namespace rnnt {

typedef unsigned long long u64;

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

// order-preserving map of a double that is > -inf and not NaN onto [2^52, 2^64): 0 stays free for "no candidate"
__device__ __forceinline__ u64 sortable_key(double x) {
  const u64 u = __builtin_bit_cast(u64, x + 0.0);   // (-0.0 + 0.0 = +0.0: one pattern per value)
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// ---- fusion policies ----------------------------------------------------------------------------------------------------
// How a search kernel reads its automaton: not at all, the dense (S, V) tables of rnnt_beam_fusion, or the backoff n-gram
// tables of rnnt_beam_ngram through ngram_lookup.
enum { FUSE_NONE = 0, FUSE_DENSE = 1, FUSE_NGRAM = 2 };
constexpr int NGRAM_MAX_ORDER = 8;

struct NgramLm {   // rnnt_beam_ngram's tables (include/rnnt_hip.h), checked by check_ngram_struct
  const int *row_ptr, *tok, *next, *backoff;
  const float *arc, *bow;
  int root, order, n_states, n_arcs;
};

// The lookup of include/rnnt_hip.h (rnnt_beam_ngram): the float32 the append of token k in state s adds, and the state after
// it.  Per level a binary search of the state's row (the root lists every token, so entry k of its row is tried first).  Every
// index read from a table is clamped into the table it indexes, the search of a row is bounded by 32 halvings and the walk by
// order <= NGRAM_MAX_ORDER levels: tables that break the contract give a wrong score, nothing else.  k in [0, V), V <= n_arcs.
__device__ __forceinline__ float ngram_lookup(const NgramLm& g, int s, int k, int& nxt) {
  double acc = 0.0;
  int h = clampi(s, 0, g.n_states - 1);
  for (int lvl = 0; lvl < NGRAM_MAX_ORDER && lvl < g.order; ++lvl) {
    const int lo = clampi(g.row_ptr[h], 0, g.n_arcs), hi = clampi(g.row_ptr[h + 1], lo, g.n_arcs);
    int e = -1;
    if (h == g.root && k < hi - lo && g.tok[lo + k] == k) e = lo + k;
    if (e < 0) {
      int a = lo, b = hi;
      for (int it = 0; it < 32 && a < b; ++it) {
        const int m = a + ((b - a) >> 1);
        if (g.tok[m] < k) a = m + 1;
        else b = m;
      }
      if (a < hi && g.tok[a] == k) e = a;
    }
    if (e >= 0) {
      nxt = clampi(g.next[e], 0, g.n_states - 1);
      return (float)(acc + (double)g.arc[e]);
    }
    if (h == g.root) break;
    acc += (double)g.bow[h];
    h = clampi(g.backoff[h], 0, g.n_states - 1);
  }
  nxt = g.root;
  return (float)acc;
}

// ---- select -----------------------------------------------------------------------------------------------------------
// The W best of N candidates in the order (key descending, id ascending); the id of a candidate is its index in the key
// array, a key of 0 is no candidate.  Radix select of the W-th best over 8-bit digits: integer LDS histograms (the counts do
// not depend on the order of the atomic adds), at most 8 passes over the key and IDBITS / 8 over the complemented id, and it
// stops at the first pass whose bin holds exactly what is still missing.  Then the selected candidates are gathered into LDS
// (in no particular order) and ranked there by counting: the total order is strict, so ranks are a permutation.

// LDS state of the select; a member of each kernel's __shared__ struct.  WMAX: the widest beam.
template <int WMAX>
struct SelectState {
  u64 sel_key[WMAX];   // the selected candidates, in the order the gather's atomics gave them
  u64 kprefix;         // the digits of the threshold key chosen so far (all 64 bits after pass 7)
  int sel_id[WMAX];
  int hist[256];
  int nvalid, nsel, need, bin, cnt;
  unsigned iprefix;    // then the digits of the threshold's complemented id
};

// by ONE thread, a barrier before select_top: the caller's fill lies in between
template <int WMAX>
__device__ __forceinline__ void select_reset(SelectState<WMAX>& s) {
  s.nvalid = 0; s.nsel = 0; s.kprefix = 0ull; s.iprefix = 0u;
}

// the bin d with sum_{d' > d} hist[d'] < need <= sum_{d' >= d} hist[d'] (wave 0; lane l owns bins 255-4l .. 252-4l)
template <int WMAX>
__device__ __forceinline__ void select_pick_bin(SelectState<WMAX>& sh, int lane) {
  int h[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { h[i] = sh.hist[255 - 4 * lane - i]; s += h[i]; }
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  const int need = sh.need;
  const unsigned long long hit = __ballot(inc >= need);
  if (hit == 0ull) {   // (fewer matches than needed: cannot happen while need <= the number of candidates; keep the state sane)
    if (lane == 0) { sh.bin = 0; sh.cnt = need; }
    return;
  }
  const int first = __ffsll((long long)hit) - 1;
  if (lane == first) {
    int above = inc - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (above + h[i] >= need) {
        sh.bin = 255 - 4 * lane - i;
        sh.cnt = h[i];
        sh.need = need - above;
        break;
      }
      above += h[i];
    }
  }
}

// Selects among ck[0, N) and gathers into sh.sel_key / sel_id; returns how many: min(W, candidates).  After select_reset and
// a barrier that also orders the writes of ck; ends with a barrier.  N <= 2^IDBITS.
template <int WMAX, int IDBITS, int THREADS>
__device__ __forceinline__ int select_top(SelectState<WMAX>& sh, const u64* ck, int N, int W) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int passes = 0;
  for (int pass = 0; pass < 8 + IDBITS / 8; ++pass) {   // (uniform)
    if (tid < 256) sh.hist[tid] = 0;
    __syncthreads();
    const u64 kprefix = sh.kprefix;
    const unsigned iprefix = sh.iprefix;
    int mine = 0;
    for (int idx = tid; idx < N; idx += THREADS) {
      const u64 key = ck[idx];
      if (key == 0ull) continue;
      ++mine;
      int digit;
      if (pass < 8) {
        if (pass > 0 && (key >> (64 - 8 * pass)) != kprefix) continue;
        digit = (int)((key >> (56 - 8 * pass)) & 255ull);
      } else {   // exact ties of the key: the LOWEST id first, so the digits of the complemented id
        const int q = pass - 8;
        const unsigned nid = ~(unsigned)idx & ((1u << IDBITS) - 1u);
        if (key != kprefix) continue;
        if (q > 0 && (nid >> (IDBITS - 8 * q)) != iprefix) continue;
        digit = (int)((nid >> (IDBITS - 8 - 8 * q)) & 255u);
      }
      atomicAdd(&sh.hist[digit], 1);
    }
    if (pass == 0) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
      if (lane == 0 && mine) atomicAdd(&sh.nvalid, mine);
    }
    __syncthreads();
    if (pass == 0 && tid == 0) sh.need = min(W, sh.nvalid);
    __syncthreads();
    if (sh.need == 0) break;   // (uniform) no candidate at all: nothing is selected
    if (wave == 0) select_pick_bin(sh, lane);
    __syncthreads();
    const bool done = sh.cnt == sh.need;   // the whole bin is taken
    passes = pass + 1;
    __syncthreads();
    if (tid == 0) {
      if (pass < 8) sh.kprefix = (kprefix << 8) | (u64)sh.bin;
      else sh.iprefix = (iprefix << 8) | (unsigned)sh.bin;
    }
    if (done) break;   // (uniform)
  }
  __syncthreads();
  // ---- gather the selected candidates
  if (min(W, sh.nvalid) > 0) {
    const u64 kprefix = sh.kprefix;
    const unsigned iprefix = sh.iprefix;
    for (int idx = tid; idx < N; idx += THREADS) {
      const u64 key = ck[idx];
      if (key == 0ull) continue;
      bool take;
      if (passes <= 8) {
        take = (key >> (64 - 8 * passes)) >= kprefix;
      } else {
        const unsigned nid = ~(unsigned)idx & ((1u << IDBITS) - 1u);
        take = key > kprefix || (key == kprefix && (nid >> (IDBITS - 8 * (passes - 8))) >= iprefix);
      }
      if (take) {
        const int slot = atomicAdd(&sh.nsel, 1);
        if (slot < WMAX) { sh.sel_key[slot] = key; sh.sel_id[slot] = idx; }
      }
    }
  }
  __syncthreads();
  return min(min(W, sh.nvalid), sh.nsel);   // (the select takes exactly min(W, candidates))
}

// rank of gathered entry i among the m gathered: how many come before it
template <int WMAX>
__device__ __forceinline__ int select_rank(const SelectState<WMAX>& sh, int i, int m) {
  const u64 key = sh.sel_key[i];
  const int id = sh.sel_id[i];
  int rank = 0;
  for (int j = 0; j < m; ++j) {
    const u64 ok = sh.sel_key[j];
    rank += (ok > key || (ok == key && sh.sel_id[j] < id)) ? 1 : 0;
  }
  return rank;
}

// position of entry i of key[0, n) in the stable order by key descending, kept below W: where a kernel writes its output
__device__ __forceinline__ int output_slot(const double* key, int i, int n, int W) {
  const double k = key[i];
  int o = 0;
  for (int j = 0; j < n; ++j) o += (key[j] > k || (key[j] == k && j < i)) ? 1 : 0;
  return min(o, W - 1);
}

// ---- prefix tree ------------------------------------------------------------------------------------------------------
// Nodes (parent, token, frame, first_child, next_sibling) in the utterance's 5 * maxn ints of global memory, append-only,
// node 0 = the root.  A node is looked up among its parent's children before it is created, so a prefix has ONE node however
// often it is pruned and reached again.
struct PrefixTree {
  int *parent, *token, *frame, *child, *sib;
};

__device__ __forceinline__ PrefixTree tree_view(int* ws, long maxn) {
  PrefixTree nd;
  nd.parent = ws;
  nd.token = nd.parent + maxn;
  nd.frame = nd.token + maxn;
  nd.child = nd.frame + maxn;
  nd.sib = nd.child + maxn;
  return nd;
}

// by ONE thread.  token: what the root stands for (CTC: -1, the empty prefix; transducer: the leading blank)
__device__ __forceinline__ void tree_root(const PrefixTree& nd, int token) {
  nd.parent[0] = -1; nd.token[0] = token; nd.frame[0] = -1; nd.child[0] = -1; nd.sib[0] = -1;
}

// the child of par with token v, or -1 (a node has fewer than V children)
__device__ __forceinline__ int tree_find_child(const PrefixTree& nd, int par, int v, int V) {
  int ch = nd.child[par];
  for (int i = 0; i < V && ch >= 0; ++i) {
    if (nd.token[ch] == v) break;
    ch = nd.sib[ch];
  }
  return ch;
}

// Creation of a frame's (round's) new nodes, two steps with a barrier between them.  Per rank r < m, in LDS: pending[r] = its
// node is to be created, par[r] = that node's parent, node[r] = its number.
// 1. by ONE thread: the new nodes are numbered in rank order
__device__ __forceinline__ void tree_number(const int* pending, int* node, int m, int& nnodes) {
  int nn = nnodes;
  for (int i = 0; i < m; ++i)
    if (pending[i]) node[i] = nn++;
  nnodes = nn;
}
// 2. by the thread of every pending rank: writes its node (token tok, frame t); the first new child of a parent links all of
//    that parent's new children, in rank order, in front of the child list
__device__ __forceinline__ void tree_link(const PrefixTree& nd, long maxn, const int* pending, const int* par_of, const int* node,
                                          int rank, int m, int tok, int t) {
  const int me = node[rank], par = par_of[rank];
  if (me >= maxn) return;   // (at most W new nodes per frame or round: never)
  nd.parent[me] = par; nd.token[me] = tok; nd.frame[me] = t; nd.child[me] = -1;
  bool leader = true;
  for (int i = 0; i < rank; ++i) leader = leader && !(pending[i] && par_of[i] == par);
  if (leader) {
    int head = nd.child[par];
    for (int i = rank; i < m; ++i) {
      if (pending[i] && par_of[i] == par) {
        nd.sib[node[i]] = head;
        head = node[i];
      }
    }
    nd.child[par] = head;
  }
}

// Writes the tokens (and frames, if not null) on the path to node x, oldest first, and returns how many.  with_root: the root
// is written too and counts (transducer: the leading blank, frame -1); otherwise the path ends below it (CTC).  cap: the row
// length, which no path exceeds.
__device__ __forceinline__ int tree_backtrace(const PrefixTree& nd, int x, bool with_root, int cap, int* tokens, int* frames) {
  int len = with_root ? 1 : 0;
  for (int y = x; y > 0 && len < cap; y = nd.parent[y]) ++len;
  for (int i = len - 1; i >= 0; --i) {
    tokens[i] = nd.token[x];
    if (frames) frames[i] = nd.frame[x];
    x = i > 0 ? nd.parent[x] : x;
  }
  return len;
}

// ---- host -------------------------------------------------------------------------------------------------------------
// the next `bytes` of a workspace carved in 256-byte steps (p null: sizes only)
inline char* ws_take(char* p, size_t& off, size_t bytes) {
  char* q = p ? p + off : nullptr;
  off += align_up(bytes, 256);
  return q;
}

// a fused entry's rnnt_beam_fusion (not null), before any device work: tables (n_states, V) over the search's V
inline int check_fusion_struct(const rnnt_beam_fusion* f, int V, const char* who) {
  RNNT_CHECK_ARG(f->n_states >= 1, "%s: fusion needs n_states >= 1, got %d", who, f->n_states);
  RNNT_CHECK_ARG((int64_t)f->n_states * V <= ((int64_t)1 << 27),
                 "%s: fusion n_states = %d with V = %d: the tables are (n_states, V) and hold at most 2^27 entries", who, f->n_states, V);
  RNNT_CHECK_ARG(f->next && f->arc && f->final, "%s: null fusion table (next, arc, final) with n_states %d", who, f->n_states);
  RNNT_CHECK_ARG(f->fused_scores, "%s: null fused_scores output with a fusion automaton", who);
  return RNNT_OK;
}

// an *_ngram entry's rnnt_beam_ngram, before any device work; fills the kernel's view of it
inline int check_ngram_struct(const rnnt_beam_ngram* g, int V, NgramLm& lm, const char* who) {
  RNNT_CHECK_ARG(g != nullptr, "%s: null ngram struct", who);
  RNNT_CHECK_ARG(g->row_ptr && g->tok && g->arc && g->next && g->bow && g->backoff && g->final,
                 "%s: null ngram table (row_ptr, tok, arc, next, bow, backoff, final)", who);
  RNNT_CHECK_ARG(g->n_states >= 1, "%s: ngram needs n_states >= 1, got %d", who, g->n_states);
  RNNT_CHECK_ARG(g->root >= 0 && g->root < g->n_states, "%s: ngram root %d outside [0, n_states = %d)", who, g->root, g->n_states);
  RNNT_CHECK_ARG(g->order >= 1 && g->order <= NGRAM_MAX_ORDER, "%s: ngram order %d outside [1,%d]", who, g->order, NGRAM_MAX_ORDER);
  RNNT_CHECK_ARG(g->n_arcs >= V, "%s: ngram n_arcs = %d < V = %d (the root lists every token)", who, g->n_arcs, V);
  RNNT_CHECK_ARG(g->fused_scores, "%s: null fused_scores output with an ngram automaton", who);
  lm.row_ptr = g->row_ptr; lm.tok = g->tok; lm.next = g->next; lm.backoff = g->backoff; lm.arc = g->arc; lm.bow = g->bow;
  lm.root = g->root; lm.order = g->order; lm.n_states = g->n_states; lm.n_arcs = g->n_arcs;
  return RNNT_OK;
}

inline int check_token_min_logp(float x, const char* who) {
  RNNT_CHECK_ARG(!(x != x) && x < __builtin_huge_valf(), "%s: token_min_logp must be a number below +inf (-inf: no pruning)", who);
  return RNNT_OK;
}

}  // namespace rnnt
