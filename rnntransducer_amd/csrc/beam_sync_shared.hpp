// The kernel of the frame-synchronous transducer beam search, beam_sync_kernel<FUSE, STREAM, ILM>, and what its two launchers share:
// beam_sync.hip (the offline entry, STREAM = false; the definition and the kernel's plan stand at its top) and
// beam_sync_stream.hip (the search fed in chunks, STREAM = true).  STREAM adds only what lies around the frame
// loop: the load of the carried beam in place of the seed, the prefix-tree collection (bs_collect, at the chunk's end and at the
// start of a frame that finds fewer than W S node slots free), the store, and the `commit` output.  ILM (only with a fusion
// policy) subtracts the internal language model: a (max, lse) pair per state slot, written by the step that fills
// the slot, and one more term where the fusion arc is added.  Nothing of it lives in BsShared: the other instances keep their LDS.
#pragma once
#include "beam_shared.hpp"
#include "search_shared.hpp"

namespace rnnt {
namespace {

constexpr int BS_WMAX = 64;
constexpr int BS_SMAX = 4;
constexpr int BS_DMAX = (BS_SMAX + 1) * BS_WMAX;
constexpr int BS_SLOTMAX = (BS_SMAX + 2) * BS_WMAX;
constexpr int BS_IDBITS = 24;   // candidate ids i V + v fit 24 bits: three 8-bit digits break exact ties
constexpr int BS_GT = 8;        // hypotheses per step group at most: 8 RU x 8 accumulators per lane
constexpr int BS_NW = DEC_THREADS / 64;

struct BsList {   // C of one round, in rank order
  double score[BS_WMAX], tot[BS_WMAX];
  int node[BS_WMAX], st[BS_WMAX];
  int slot[BS_WMAX];    // the state's slot; while tok >= 0: the PARENT's slot (-1: the zero state), the step is still to run
  int tok[BS_WMAX];     // the token of the pending step, or -1
  float mx[BS_WMAX], ls[BS_WMAX];   // of the member's joint row: lp[v] = ((A[v] + Cv[v]) - mx) - ls
};

struct BsShared {
  BsList c[2];
  // D, in order of first insertion
  double dscore[BS_DMAX], dtot[BS_DMAX];
  int dnode[BS_DMAX], dst[BS_DMAX], dslot[BS_DMAX], dtok[BS_DMAX];
  SelectState<BS_WMAX> sel;
  // the selected candidates by rank
  double rval[BS_WMAX], rtot[BS_WMAX];
  int rnode[BS_WMAX], rpar[BS_WMAX], rst[BS_WMAX], rslot[BS_WMAX], rtok[BS_WMAX];
  int pending[BS_WMAX];   // its node is still to be created
  int tod[BS_WMAX];       // goes to D this round
  int dpos[BS_WMAX];      // index in D (before this round) of its node, or -1
  int dup[BS_WMAX];       // lowest rank of an earlier entry of this round that goes to D under the same node, or -1
  int target[BS_WMAX];    // its index in D / in the next C
  int freelist[BS_SLOTMAX], used[BS_SLOTMAX];
  int gidx[BS_WMAX];      // step: the members that advance, in member order
  int gnew[BS_WMAX];      //       and the slots they get
  int wcount[BS_NW];
  int nnodes, nD, nnext, npend, fpos;
  // STREAM only: the collection's root, lowest member node and new node count; the chunk's tokens committed so far; the
  // stream's counters (header words BSS_*); the status that ends the chunk for this stream
  int cR, cmin, cnew, ncommit, ncollect, ncollect_in, peak, fail;
};

struct BsK : PredNet {
  int T, B, W, S, G;
  float min_logp;
  const float* A;
  long a_st, a_sb;
  const int* t_lens;
  const float* table;   // (V, NG*Hp) layer-0 input projection
  float* slots;         // (B, NS, SF)
  int SF, NS;
  u64* keys;            // (B, W*V)
  int* nodes;           // (B, 5, maxn)
  long maxn;
  int max_len;
  int* tokens;
  int* lens;
  double* scores;
  int* counts;
  int* frames;
  const int* fnext;
  const float* farc;
  const float* ffinal;
  int n_states;
  NgramLm ng;           // FUSE_NGRAM: the backoff tables in place of fnext / farc (ffinal, n_states and fused serve both)
  double* fused;
  // STREAM (beam_sync_stream.hip): stream b's carried state is the workspace part at ws + b * ws_stride, laid out by the off_*
  char* ws;
  size_t ws_stride, off_beam, off_slots, off_keys, off_nodes, off_mark, off_remap;
  int* status;          // (B)
  int* commit;          // (B, commit_ld) the tokens this chunk's collections committed, oldest first
  int* commit_frames;   // beside commit, or null
  int* ncommit;         // (B)
  long commit_ld;
  const int* rows;      // the reset kernel's row list
  // ILM: fc.bias (V), the weight mu, and the (NS, 2) float pairs (m, lse) per state slot: offline at ilm + b NS 2, STREAM in
  // stream b's workspace part at off_ilm
  const float* ilm_bias;
  float ilm_w;
  float* ilm;
  size_t off_ilm;
};

// Internal-LM subtraction (include/rnnt_hip.h).  The log-probability of token v != blank under the pair (m, lse) of a slot:
__device__ __forceinline__ float ilm_logp(const float* Cv, const float* bias, float m, float lse, int v) {
  return ((Cv[v] + bias[v]) - m) - lse;
}
// total' of a non-blank candidate: the header's ONE fp64 expression, called where the keys are filled and where the selected
// candidates are built.  Contraction is off: a fused multiply-add at one of the two places and not at the other would break
// "the same bits".  ilm == 0 (V = 2) gives (tot + arc) - 0: the fused instance's bits.
template <bool ILM>
__device__ __forceinline__ double fused_total(double tot, float arc, float mu, float ilm) {
#pragma clang fp contract(off)
  if constexpr (ILM) return (tot + (double)arc) - (double)mu * (double)ilm;
  else return tot + (double)arc;
}

// int32 words of a stream's 256-byte workspace header (include/rnnt_hip.h: rnnt_beam_sync_stream_desc)
enum { BSS_NA = 0, BSS_NNODES, BSS_COMMITTED, BSS_FRAMES, BSS_STATUS, BSS_NCOLLECT, BSS_NCOLLECT_IN, BSS_PEAK, BSS_WORDS };
constexpr size_t BSS_HEADER_BYTES = 256;
constexpr int BSS_MEMBER = 2;   // bs_collect's mark: 1 = on a path from R to a member, | BSS_MEMBER = a member's own node

// y_j[r] = dot(W[r, :cols], x_j) (+ bias[r]) for r in [0, rows) and the g <= BS_GT hypotheses j of a group: matvec
// (decode_shared.hpp) with the RU weight rows of a wave loaded once and used for every j.  x_j = x + j * xs (LDS, 16-byte
// aligned); y_j = yof(j).  Per j the sums are matvec's, term for term and in its order.  The four-term sum of a k chunk is
// written as one product and three fused multiply-adds, with contraction off around it: left to the compiler, the unrolled
// copies for different j were contracted differently (which product of a*b + c*d is rounded is its choice), and a
// hypothesis's bits depended on its position in the group (measured: 1e-6 in the scores between groups of 8 and of 3).
template <class YOF>
__device__ __forceinline__ void matvec_group(const float* __restrict__ Wm, long ld, int rows, int cols, const float* x, int xs,
                                             int g, YOF yof, const float* __restrict__ bias) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: the row addresses stay scalar
  for (int r0 = wave * RU; r0 < rows; r0 += BS_NW * RU) {
    float s[BS_GT][RU];
#pragma unroll
    for (int j = 0; j < BS_GT; ++j)
#pragma unroll
      for (int i = 0; i < RU; ++i) s[j][i] = 0.f;
    for (int k = 4 * lane; k < cols; k += 256) {
      f32x4 w[RU];
#pragma unroll
      for (int i = 0; i < RU; ++i) {
        const int r = r0 + i < rows ? r0 + i : rows - 1;   // clamp: tail rows re-read the last row, result discarded
        w[i] = *reinterpret_cast<const f32x4*>(Wm + (long)r * ld + k);
      }
#pragma unroll
      for (int j = 0; j < BS_GT; ++j) {
        if (j < g) {   // (uniform)
          const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (long)j * xs + k);
#pragma unroll
          for (int i = 0; i < RU; ++i) {   // matvec's four-term sum, its contraction spelled out (see above)
            float t = w[i][0] * xv[0];
            t = __builtin_fmaf(w[i][1], xv[1], t);
            t = __builtin_fmaf(w[i][2], xv[2], t);
            t = __builtin_fmaf(w[i][3], xv[3], t);
            s[j][i] += t;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < BS_GT; ++j) {
      if (j < g) {   // (uniform)
#pragma unroll
        for (int i = 0; i < RU; ++i) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) s[j][i] += __shfl_xor(s[j][i], o);
        }
        if (lane < RU && r0 + lane < rows) {
          float v = s[j][0];
#pragma unroll
          for (int i = 1; i < RU; ++i) v = lane == i ? s[j][i] : v;
          yof(j)[r0 + lane] = v + (bias ? bias[r0 + lane] : 0.f);
        }
      }
    }
  }
}

// dynamic LDS of the step: per hypothesis of a group h[L Hp] | c[L Hp] (LSTM) | gh[NG Hp] | gi[NG Hp] (L > 1) | dec[O]
struct BsStepLds {
  float *h, *c, *gh, *gi, *dec;
  int LH, NG;
};
inline size_t bs_step_floats(int L, int Hp, int O, int cell) {
  return (size_t)L * Hp * (cell == RNNT_CELL_LSTM ? 2 : 1) + (size_t)cell_gates(cell) * Hp * (L > 1 ? 2 : 1) + O;
}

// The members of `ls` (n of them) whose step is pending advance together: each gets a free slot, reads its parent's state and
// writes (h', c', Cv') there.  Ends with a barrier.  ILM: then a wavefront per new slot reduces Cv + bias over v != blank to the
// slot's pair (m, lse) in ilmp: lanes along v, wave_max / wave_sum as the row log-softmax below, so the order of the sums
// depends neither on the group size nor on the hypothesis's place in a group.
template <bool ILM>
__device__ __forceinline__ void bs_step_pending(const BsK& p, BsShared& sh, BsList& ls, int n, float* slots, const BsStepLds& sl,
                                                float* ilmp) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Hp = p.Hp, L = p.L, LH = sl.LH, NG = sl.NG, SF = p.SF, V = p.V;
  const bool lstm = p.cell == RNNT_CELL_LSTM;
  if (wave == 0) {   // W <= 64: one wavefront sees every member
    const bool pend = lane < n && ls.tok[lane] >= 0;
    const unsigned long long bal = __ballot(pend);
    const int pos = __popcll(bal & ((1ull << lane) - 1ull));
    if (pend) {
      sh.gidx[pos] = lane;
      sh.gnew[pos] = sh.freelist[min(sh.fpos + pos, p.NS - 1)];   // (the free list never runs out: (S+2) W slots)
    }
    if (lane == 0) sh.npend = __popcll(bal);
  }
  __syncthreads();
  const int np = sh.npend;
  if (np == 0) return;   // (uniform)
  for (int g0 = 0; g0 < np; g0 += p.G) {
    const int g = min(p.G, np - g0);
    for (int e = tid; e < g * LH; e += DEC_THREADS) {
      const int j = e / LH, i = e - j * LH;
      const int ps = min(ls.slot[sh.gidx[g0 + j]], p.NS - 1);
      const float* st = ps >= 0 ? slots + (long)ps * SF : nullptr;
      sl.h[e] = st ? st[i] : 0.f;
      if (lstm) sl.c[e] = st ? st[LH + i] : 0.f;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      if (l > 0)
        matvec_group(p.w_ih[l], Hp, NG * Hp, Hp, sl.h + (l - 1) * Hp, LH, g, [&](int j) { return sl.gi + (long)j * NG * Hp; },
                     p.b_ih[l]);
      matvec_group(p.w_hh[l], Hp, NG * Hp, Hp, sl.h + l * Hp, LH, g, [&](int j) { return sl.gh + (long)j * NG * Hp; }, p.b_hh[l]);
      __syncthreads();
      for (int e = tid; e < g * Hp; e += DEC_THREADS) {
        const int j = e / Hp, i = e - j * Hp;
        // layer 0: the table row of the token (W_ih0 emb[tok] + b_ih0, matvec's bits); deeper: this group's gi
        const float* gi = l == 0 ? p.table + (long)ls.tok[sh.gidx[g0 + j]] * NG * Hp : sl.gi + (long)j * NG * Hp;
        const float* gh = sl.gh + (long)j * NG * Hp;
        float* h = sl.h + (long)j * LH + l * Hp;
        float hv;
        if (lstm) {
          float* c = sl.c + (long)j * LH + l * Hp;
          const float ig = sigmoidf_(gi[i] + gh[i]), fg = sigmoidf_(gi[Hp + i] + gh[Hp + i]);
          const float gg = tanhf(gi[2 * Hp + i] + gh[2 * Hp + i]), og = sigmoidf_(gi[3 * Hp + i] + gh[3 * Hp + i]);
          const float cv = fg * c[i] + ig * gg;
          c[i] = cv;
          hv = og * tanhf(cv);
        } else if (p.cell == RNNT_CELL_GRU) {
          const float rg = sigmoidf_(gi[i] + gh[i]), zg = sigmoidf_(gi[Hp + i] + gh[Hp + i]);
          const float ng = tanhf(gi[2 * Hp + i] + rg * gh[2 * Hp + i]);
          hv = (1.f - zg) * ng + zg * h[i];
        } else {
          const float pre = gi[i] + gh[i];
          hv = p.cell == RNNT_CELL_RNN_RELU ? fmaxf(pre, 0.f) : tanhf(pre);
        }
        h[i] = hv;   // also the next layer's input
      }
      __syncthreads();
    }
    // Cv = gelu(out_proj(h_last)) . W_d^T, straight into the new slot
    matvec_group(p.w_o, Hp, p.O, Hp, sl.h + (L - 1) * Hp, LH, g, [&](int j) { return sl.dec + (long)j * p.O; }, p.b_o);
    __syncthreads();
    for (int e = tid; e < g * p.O; e += DEC_THREADS) sl.dec[e] = gelu_tanh(sl.dec[e]);
    __syncthreads();
    matvec_group(p.w_d, p.ld_d, V, p.O, sl.dec, p.O, g, [&](int j) { return slots + (long)sh.gnew[g0 + j] * SF + (SF - V); },
                 nullptr);
    for (int e = tid; e < g * LH; e += DEC_THREADS) {
      const int j = e / LH, i = e - j * LH;
      float* dst = slots + (long)sh.gnew[g0 + j] * SF;
      dst[i] = sl.h[e];
      if (lstm) dst[LH + i] = sl.c[e];
    }
    __syncthreads();
  }
  if (tid < np) {
    const int mi = sh.gidx[tid];
    ls.slot[mi] = sh.gnew[tid];
    ls.tok[mi] = -1;
  }
  if (tid == 0) sh.fpos += np;
  __threadfence_block();   // the slots are read through global memory by this workgroup's other waves
  __syncthreads();
  if constexpr (ILM) {   // behind the fence: every Cv of this call is visible; gnew is not rewritten before the next call
    for (int j = wave; j < np; j += BS_NW) {
      const int s = clampi(sh.gnew[j], 0, p.NS - 1);   // (clamp: always in range)
      const float* Cv = slots + (long)s * SF + (SF - V);
      float m = -__builtin_huge_valf();
      for (int v = lane; v < V; v += 64)
        if (v != p.blank) m = fmaxf(m, Cv[v] + p.ilm_bias[v]);
      m = wave_max(m);
      float sum = 0.f;
      for (int v = lane; v < V; v += 64)
        if (v != p.blank) sum += expf((Cv[v] + p.ilm_bias[v]) - m);
      sum = wave_sum(sum);
      if (lane == 0) { ilmp[2 * s] = m; ilmp[2 * s + 1] = logf(sum); }
    }
    __threadfence_block();
    __syncthreads();
  }
}

// The free list: every slot the n members of c do not hold, in slot order; sh.fpos = 0.  Ends with a barrier.
__device__ __forceinline__ void bs_free_list(BsShared& sh, const BsList& c, int n, int NS) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < NS; i += DEC_THREADS) sh.used[i] = 0;
  __syncthreads();
  if (tid < n) sh.used[clampi(c.slot[tid], 0, NS - 1)] = 1;   // (slots of members are distinct)
  __syncthreads();
  const bool fr = tid < NS && !sh.used[tid < NS ? tid : 0];
  const unsigned long long bal = __ballot(fr);
  if (lane == 0) sh.wcount[wave] = __popcll(bal);
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += sh.wcount[w];
  if (fr) sh.freelist[before + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
  if (tid == 0) sh.fpos = 0;
  __syncthreads();
}

// Collection of a stream's prefix tree (STREAM only).  The beam `a` (nA members, their nodes distinct) is all
// that refers to the tree: called between frames.  R = the lowest common ancestor of the members' nodes.  Kept, exactly: R, the
// nodes on a path from R to a member, and every descendant of a member's node (what a later frame can find again: a hypothesis
// extends a member, and tree_find_child looks below its node).  The chain from below the old root down to R goes to commit
// (sh.ncommit counts it), R becomes node 0, the kept nodes are compacted IN INDEX ORDER (a parent's index is below its
// children's, before and after), and a child list keeps its order: descending index, as tree_link builds it.  mark and remap:
// maxn ints each of the stream's workspace.  Ends with a barrier; sh.nnodes is the new count.
__device__ __forceinline__ void bs_collect(BsShared& sh, const PrefixTree& nd, int* mark, int* remap, BsList& a, int nA, int* commit,
                                           int* commit_frames, long commit_cap) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = sh.nnodes;
  for (int x = tid; x < n; x += DEC_THREADS) mark[x] = 0;
  if (tid == 0) { sh.cmin = n; sh.peak = max(sh.peak, n); }
  if (tid < BS_WMAX) sh.target[tid] = tid < nA ? clampi(a.node[tid], 0, n - 1) : -1;   // (target: free between frames)
  __threadfence_block();
  __syncthreads();
  if (tid < nA) atomicMin(&sh.cmin, sh.target[tid]);
  // R by pairwise reduction; of two nodes the one with the larger index is no ancestor of the other, so it steps up
  for (int o = BS_WMAX / 2; o > 0; o >>= 1) {
    if (tid < o) {
      int x = sh.target[tid], y = sh.target[tid + o];
      if (x < 0) x = y;
      else if (y >= 0)
        for (int i = 0; i < 2 * n && x != y; ++i) {
          if (x > y) x = max(nd.parent[x], 0);
          else y = max(nd.parent[y], 0);
        }
      sh.target[tid] = x;
    }
    __syncthreads();
  }
  if (tid == 0) sh.cR = max(sh.target[0], 0);
  __syncthreads();
  // mark: 1 on the paths from R to the members (plain stores of one value), then BSS_MEMBER on the members' own nodes
  if (tid < nA)
    for (int y = clampi(a.node[tid], 0, n - 1); y >= sh.cR; y = nd.parent[y]) mark[y] = 1;
  __threadfence_block();
  __syncthreads();
  if (tid < nA) mark[clampi(a.node[tid], 0, n - 1)] = BSS_MEMBER | 1;
  __threadfence_block();
  __syncthreads();
  const int R = sh.cR, mn = sh.cmin;
  for (int x = tid; x < n; x += DEC_THREADS) {
    int keep = mark[x] != 0 ? 1 : 0;   // R, or on a path from R to a member
    if (!keep && x > mn)   // below a member's node?  (ancestors have lower indices: the walk ends below the lowest member)
      for (int y = nd.parent[x]; y >= mn; y = nd.parent[y])
        if (mark[y] & BSS_MEMBER) { keep = 1; break; }
    remap[x] = keep;
  }
  __threadfence_block();
  __syncthreads();
  // new indices: an exclusive scan of keep in index order; thread tid owns the nodes [tid seg, (tid + 1) seg)
  {
    const int seg = (n + DEC_THREADS - 1) / DEC_THREADS;
    const int lo = min(tid * seg, n), hi = min(lo + seg, n);
    int cnt = 0;
    for (int x = lo; x < hi; ++x) cnt += remap[x];
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    if (lane == 63) sh.wcount[wave] = inc;
    __syncthreads();
    int base = inc - cnt;
    for (int w = 0; w < wave; ++w) base += sh.wcount[w];
    if (tid == DEC_THREADS - 1) sh.cnew = base + cnt;
    for (int x = lo; x < hi; ++x) remap[x] = remap[x] ? base++ : -1;
  }
  __threadfence_block();
  __syncthreads();
  // mark[y] = the first kept node of the sibling chain that starts at y (y itself if kept), as a new index, or -1
  for (int y = tid; y < n; y += DEC_THREADS) {
    int z = y;
    for (int i = 0; i < n && z >= 0 && remap[z] < 0; ++i) z = nd.sib[z];
    mark[y] = z >= 0 ? remap[z] : -1;
  }
  if (tid == 0) {   // the committed chain, oldest first: from below the old root down to R
    int k = 0;
    for (int y = R; y > 0; y = nd.parent[y]) ++k;
    const int nc = sh.ncommit;
    int y = R;
    for (int i = k - 1; i >= 0; --i) {
      if (nc + i < commit_cap) {   // (the entry sizes commit for every token a chunk can commit: always)
        commit[nc + i] = nd.token[y];
        if (commit_frames) commit_frames[nc + i] = nd.frame[y];
      }
      y = nd.parent[y];
    }
    sh.ncommit = nc + k;
  }
  __threadfence_block();
  __syncthreads();
  // the move, DEC_THREADS nodes a round in index order: a new index is at most the old one, so a round overwrites only nodes
  // that this round or an earlier one has read
  for (int x0 = 0; x0 < n; x0 += DEC_THREADS) {
    const int x = x0 + tid;
    int j = -1, pa = -1, tk = 0, fr = 0, ch = -1, sb = -1;
    if (x < n && (j = remap[x]) >= 0) {
      pa = nd.parent[x]; tk = nd.token[x]; fr = nd.frame[x]; ch = nd.child[x]; sb = nd.sib[x];
      pa = (x == R || pa < 0) ? -1 : remap[pa];
      ch = ch >= 0 ? mark[ch] : -1;
      sb = sb >= 0 ? mark[sb] : -1;
    }
    __syncthreads();
    if (j >= 0) { nd.parent[j] = pa; nd.token[j] = tk; nd.frame[j] = fr; nd.child[j] = ch; nd.sib[j] = sb; }
    __threadfence_block();
    __syncthreads();
  }
  if (tid < nA) a.node[tid] = max(remap[clampi(a.node[tid], 0, n - 1)], 0);   // (a member's node is kept: never -1)
  if (tid == 0) { sh.nnodes = sh.cnew; sh.ncollect += 1; }
  __syncthreads();
}

// FUSE: the fusion policy (search_shared.hpp).  FUSE_DENSE reads farc / fnext at (state, token); FUSE_NGRAM asks ngram_lookup
// for the same two values at the same two places, the candidate-key fill and the build of the selected children.
// ILM: internal-LM subtraction on top of a fusion policy (the term of fused_total at the same two places).
template <int FUSE, bool STREAM, bool ILM = false>
__global__ void __launch_bounds__(DEC_THREADS) beam_sync_kernel(const BsK p) {
  constexpr bool FUSED = FUSE != FUSE_NONE;
  static_assert(!ILM || FUSED, "internal-LM subtraction rides on a fusion policy");
  __shared__ BsShared sh;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = p.V, W = p.W, S = p.S, SF = p.SF, NS = p.NS, blank = p.blank;
  const int Tb = p.t_lens ? clampi(p.t_lens[b], 0, p.T) : p.T;
  const long maxn = p.maxn;
  char* wsb = STREAM ? p.ws + (size_t)b * p.ws_stride : nullptr;   // STREAM: everything of stream b lies in its workspace part
  int* hdr = reinterpret_cast<int*>(wsb);
  int fbase = 0;   // STREAM: the frames consumed before this chunk; a node's frame is absolute
  if constexpr (STREAM) {
    const int st = hdr[BSS_STATUS];
    if (Tb == 0 || st != RNNT_BEAM_ST_OK) {   // (uniform) no frames, or failed earlier: the workspace is not touched
      if (tid == 0) { p.counts[b] = -1; p.status[b] = st; p.ncommit[b] = 0; }
      return;
    }
    fbase = hdr[BSS_FRAMES];
  }
  u64* ck = STREAM ? reinterpret_cast<u64*>(wsb + p.off_keys) : p.keys + (long)b * W * V;
  float* slots = STREAM ? reinterpret_cast<float*>(wsb + p.off_slots) : p.slots + (long)b * NS * SF;
  const PrefixTree nd = tree_view(STREAM ? reinterpret_cast<int*>(wsb + p.off_nodes) : p.nodes + (long)b * 5 * maxn, maxn);
  float* ilmp = !ILM ? nullptr : STREAM ? reinterpret_cast<float*>(wsb + p.off_ilm) : p.ilm + (long)b * NS * 2;
  BsStepLds sl;
  sl.NG = cell_gates(p.cell);
  sl.LH = p.L * p.Hp;
  {
    float* f = reinterpret_cast<float*>(smem);
    sl.h = f; f += (long)p.G * sl.LH;
    sl.c = f; if (p.cell == RNNT_CELL_LSTM) f += (long)p.G * sl.LH;
    sl.gh = f; f += (long)p.G * sl.NG * p.Hp;
    sl.gi = f; if (p.L > 1) f += (long)p.G * sl.NG * p.Hp;
    sl.dec = f;
  }

  if (tid < 2 * BS_WMAX) {   // every slot of both lists holds a valid (dead) member from the start
    BsList& c = sh.c[tid / BS_WMAX];
    const int r = tid % BS_WMAX;
    c.score[r] = NEG_INF; c.tot[r] = 0.0; c.node[r] = 0; c.st[r] = 0; c.slot[r] = -1; c.tok[r] = -1; c.mx[r] = 0.f; c.ls[r] = 0.f;
  }
  for (int i = tid; i < BS_SLOTMAX; i += DEC_THREADS) sh.freelist[i] = min(i, NS - 1);   // (every entry names a slot, always)
  __syncthreads();
  int nA = 1, cur = 0;
  if constexpr (STREAM) {   // the carried beam in place of the seed (the reset kernel stored the seed in the same form)
    nA = clampi(hdr[BSS_NA], 0, W);
    if (tid < nA) {
      BsList& c = sh.c[0];
      const double* bd = reinterpret_cast<const double*>(wsb + p.off_beam);
      const int* bi = reinterpret_cast<const int*>(bd + 2 * W);
      c.score[tid] = bd[tid]; c.tot[tid] = bd[W + tid];
      c.node[tid] = bi[tid]; c.st[tid] = bi[W + tid]; c.slot[tid] = bi[2 * W + tid]; c.tok[tid] = bi[3 * W + tid];
    }
    if (tid == 0) {
      sh.nnodes = hdr[BSS_NNODES]; sh.nD = 0; sh.nnext = 0;
      sh.ncommit = 0; sh.ncollect = hdr[BSS_NCOLLECT]; sh.ncollect_in = hdr[BSS_NCOLLECT_IN]; sh.peak = hdr[BSS_PEAK]; sh.fail = 0;
    }
    __syncthreads();
    // the pending steps of the first frame take slots that no member refers to, as its state or as its parent's
    bs_free_list(sh, sh.c[0], nA, NS);
  } else {
    if (tid == 0) {
      BsList& c = sh.c[0];
      c.score[0] = 0.0; c.tot[0] = 0.0; c.node[0] = 0; c.st[0] = 0;
      c.slot[0] = -1; c.tok[0] = blank;   // one step on blank from the zero state, as every search here primes an utterance
      tree_root(nd, blank);   // the leading blank
      sh.nnodes = 1; sh.fpos = 0; sh.nD = 0; sh.nnext = 0;
    }
    __threadfence_block();
    __syncthreads();
  }

  int tdone = 0;   // STREAM: the frames this chunk consumed
  for (int t = 0; t < Tb; ++t) {
    if constexpr (STREAM) {
      // a frame makes at most W S nodes.  Fewer slots free: collect; still fewer: max_nodes cannot hold the live tree.  The
      // collected tree is a function of the frames fed alone, so this end does not depend on the chunking.
      if (sh.nnodes + W * S > maxn) {   // (uniform)
        bs_collect(sh, nd, reinterpret_cast<int*>(wsb + p.off_mark), reinterpret_cast<int*>(wsb + p.off_remap), sh.c[cur], nA,
                   p.commit + (long)b * p.commit_ld, p.commit_frames ? p.commit_frames + (long)b * p.commit_ld : nullptr, p.commit_ld);
        if (tid == 0) {
          sh.ncollect_in += 1;
          if (sh.nnodes + W * S > maxn) sh.fail = RNNT_BEAM_ST_NODES;
        }
        __syncthreads();
        if (sh.fail) break;   // (uniform)
      }
    }
    const float* At = p.A + (long)t * p.a_st + (long)b * p.a_sb;
    int n = nA;
    if (tid == 0) sh.nD = 0;
    __syncthreads();
    for (int r = 0; r < S && n > 0; ++r) {   // (n is uniform)
      BsList& c = sh.c[cur];
      BsList& nx = sh.c[cur ^ 1];
      const bool last_round = r == S - 1;
      // round 0: the survivors among the last frame's last-round children (frame 0: the root); later: this frame's children
      bs_step_pending<ILM>(p, sh, c, n, slots, sl, ilmp);
      if (r == 0) bs_free_list(sh, c, n, NS);   // the free list of this frame: every slot the beam does not hold
      if (tid == 0) { select_reset(sh.sel); sh.nnext = 0; }
      // ---- log-softmax of every member row and its candidate keys: a wavefront per row, lanes along v
      for (int i = wave; i < n; i += BS_NW) {
        const float* Cv = slots + (long)clampi(c.slot[i], 0, NS - 1) * SF + (SF - V);   // (clamp: always in range)
        float m = -__builtin_huge_valf();
        for (int v = lane; v < V; v += 64) m = fmaxf(m, At[v] + Cv[v]);
        m = wave_max(m);
        float s = 0.f;
        for (int v = lane; v < V; v += 64) s += expf((At[v] + Cv[v]) - m);
        s = wave_sum(s);
        const float lse = logf(s);
        if (lane == 0) { c.mx[i] = m; c.ls[i] = lse; }
        const double sc = c.score[i], tt = FUSED ? c.tot[i] : 0.0;
        const int st = FUSED ? c.st[i] : 0;
        float im = 0.f, il = 0.f;   // ILM: the pair of the member's slot
        if constexpr (ILM) { im = ilmp[2 * clampi(c.slot[i], 0, NS - 1)]; il = ilmp[2 * clampi(c.slot[i], 0, NS - 1) + 1]; }
        for (int v = lane; v < V; v += 64) {
          const float lp = ((At[v] + Cv[v]) - m) - lse;
          u64 key = 0ull;
          if (v == blank || lp >= p.min_logp) {
            const double val = sc + (double)lp;
            double k = val;
            if constexpr (FUSE == FUSE_NGRAM) {   // only a candidate that passed the prune walks the tables
              int unused;
              k = val + (v == blank ? tt : fused_total<ILM>(tt, ngram_lookup(p.ng, st, v, unused), p.ilm_w,
                                                            ILM ? ilm_logp(Cv, p.ilm_bias, im, il, v) : 0.f));
            } else if (FUSED)
              k = val + (v == blank ? tt : fused_total<ILM>(tt, p.farc[(long)st * V + v], p.ilm_w,
                                                            ILM ? ilm_logp(Cv, p.ilm_bias, im, il, v) : 0.f));
            if (val > NEG_INF && k > NEG_INF) key = sortable_key(k);   // (NaN compares false: dropped)
          }
          ck[(long)i * V + v] = key;
        }
      }
      __threadfence_block();
      __syncthreads();

      // ---- select the min(W, candidates) best in the order (key descending, id ascending)
      const int m = select_top<BS_WMAX, BS_IDBITS, DEC_THREADS>(sh.sel, ck, n * V, W);
      const int nD0 = sh.nD;

      // ---- build, by rank: the closed hypothesis or the child, its node, and where it goes
      int rank = -1;
      if (tid < m) {
        const int id = sh.sel.sel_id[tid];
        rank = select_rank(sh.sel, tid, m);
        const int i = id / V, v = id - i * V;
        const float* Cv = slots + (long)clampi(c.slot[i], 0, NS - 1) * SF + (SF - V);   // (clamp: always in range)
        const float lp = ((At[v] + Cv[v]) - c.mx[i]) - c.ls[i];   // the fill's expression: the same bits
        sh.rval[rank] = c.score[i] + (double)lp;
        int node, pend = 0;
        if (v == blank) {
          node = c.node[i];
          sh.rtot[rank] = FUSED ? c.tot[i] : 0.0;
          sh.rst[rank] = FUSED ? c.st[i] : 0;
          sh.rtok[rank] = -1;
          sh.rpar[rank] = -1;
          sh.tod[rank] = 1;
        } else {
          float ilm = 0.f;   // ILM: the fill's value, from the same pair: the same bits
          if constexpr (ILM) {
            const float* ip = ilmp + 2 * clampi(c.slot[i], 0, NS - 1);
            ilm = ilm_logp(Cv, p.ilm_bias, ip[0], ip[1], v);
          }
          if constexpr (FUSE == FUSE_NGRAM) {
            int ns;
            const float arc = ngram_lookup(p.ng, c.st[i], v, ns);   // the fill's value: the same walk, the same bits
            sh.rtot[rank] = fused_total<ILM>(c.tot[i], arc, p.ilm_w, ilm);
            sh.rst[rank] = ns;
          } else if (FUSED) {
            const long o = (long)c.st[i] * V + v;
            sh.rtot[rank] = fused_total<ILM>(c.tot[i], p.farc[o], p.ilm_w, ilm);
            sh.rst[rank] = clampi(p.fnext[o], 0, p.n_states - 1);
          } else {
            sh.rtot[rank] = 0.0;
            sh.rst[rank] = 0;
          }
          const int par = c.node[i];
          sh.rtok[rank] = v;
          sh.rpar[rank] = par;
          node = tree_find_child(nd, par, v, V);   // the prefix's node, if it was created before
          pend = node < 0 ? 1 : 0;
          sh.tod[rank] = last_round ? 1 : 0;
        }
        sh.rslot[rank] = c.slot[i];   // a closed hypothesis keeps its state; a child's step starts from its parent's
        sh.rnode[rank] = node;
        sh.pending[rank] = pend;
        int dp = -1;
        if (sh.tod[rank] && !pend)
          for (int q = 0; q < nD0; ++q)
            if (sh.dnode[q] == node) dp = q;   // (nodes of D are distinct: at most one hit)
        sh.dpos[rank] = dp;
      }
      __syncthreads();
      if (rank >= 0) {   // an earlier entry of this round under the same node (a new node has none)
        int du = -1;
        if (sh.tod[rank] && !sh.pending[rank])
          for (int q = rank - 1; q >= 0; --q)
            if (sh.tod[q] && !sh.pending[q] && sh.rnode[q] == sh.rnode[rank]) du = q;
        sh.dup[rank] = du;
      }
      __syncthreads();
      if (tid == 0) {   // in rank order: new nodes are numbered, D grows, the next C fills
        tree_number(sh.pending, sh.rnode, m, sh.nnodes);
        int nDn = nD0, nxt = 0;
        for (int i = 0; i < m; ++i) {
          if (sh.tod[i]) sh.target[i] = sh.dpos[i] >= 0 ? sh.dpos[i] : (sh.dup[i] >= 0 ? sh.target[sh.dup[i]] : nDn++);
          else sh.target[i] = nxt++;
        }
        sh.nD = nDn; sh.nnext = nxt;
      }
      __syncthreads();
      if (rank >= 0) {
        const int me = sh.rnode[rank], tg = sh.target[rank];
        if (sh.pending[rank]) tree_link(nd, maxn, sh.pending, sh.rpar, sh.rnode, rank, m, sh.rtok[rank], fbase + t);
        if (!sh.tod[rank]) {   // the child joins the next round's C; its step runs at that round's start
          nx.score[tg] = sh.rval[rank]; nx.tot[tg] = sh.rtot[rank]; nx.node[tg] = me; nx.st[tg] = sh.rst[rank];
          nx.slot[tg] = sh.rslot[rank]; nx.tok[tg] = sh.rtok[rank];
        } else if (sh.dup[rank] < 0 && tg < BS_DMAX) {   // one writer per entry of D: the first of this round under its node
          double s = sh.dpos[rank] >= 0 ? logaddexp_d(sh.dscore[tg], sh.rval[rank]) : sh.rval[rank];
          for (int i = rank + 1; i < m; ++i)
            if (sh.tod[i] && sh.dup[i] == rank) s = logaddexp_d(s, sh.rval[i]);
          sh.dscore[tg] = s;
          if (sh.dpos[rank] < 0) {   // state, total and automaton state are the same by construction: the first stays
            sh.dtot[tg] = sh.rtot[rank]; sh.dnode[tg] = me; sh.dst[tg] = sh.rst[rank];
            sh.dslot[tg] = sh.rslot[rank]; sh.dtok[tg] = sh.rtok[rank];
          }
        }
      }
      __threadfence_block();
      __syncthreads();
      n = sh.nnext;
      cur ^= 1;
    }

    // ---- the next beam: the min(W, |D|) best of D by (score [+ total] descending, insertion order ascending)
    const int nD = sh.nD;
    BsList& a = sh.c[cur];
    if (tid < nD) {
      const double key = FUSED ? sh.dscore[tid] + sh.dtot[tid] : sh.dscore[tid];
      int o = 0;
      for (int i = 0; i < nD; ++i) {
        const double k = FUSED ? sh.dscore[i] + sh.dtot[i] : sh.dscore[i];
        o += (k > key || (k == key && i < tid)) ? 1 : 0;
      }
      if (o < W) {
        a.score[o] = sh.dscore[tid]; a.tot[o] = sh.dtot[tid]; a.node[o] = sh.dnode[tid]; a.st[o] = sh.dst[tid];
        a.slot[o] = sh.dslot[tid]; a.tok[o] = sh.dtok[tid];
      }
    }
    __syncthreads();
    nA = min(W, nD);
    tdone = t + 1;
  }

  BsList& a = sh.c[cur];
  if constexpr (STREAM) {
    // ---- the chunk's end: collect, so that the tails below are as short as they can be and the carried tree as small
    if (!sh.fail)
      bs_collect(sh, nd, reinterpret_cast<int*>(wsb + p.off_mark), reinterpret_cast<int*>(wsb + p.off_remap), a, nA,
                 p.commit + (long)b * p.commit_ld, p.commit_frames ? p.commit_frames + (long)b * p.commit_ld : nullptr, p.commit_ld);
    if (!sh.fail && tid < nA) {   // max_len: the tail of a returned sequence, the tokens below the root
      int len = 0;
      for (int y = a.node[tid]; y > 0 && len <= p.max_len; y = nd.parent[y]) ++len;
      if (len > p.max_len) sh.fail = RNNT_BEAM_ST_LEN;   // (one value, whoever writes it)
    }
    __syncthreads();
    if (sh.fail) {   // (uniform) the stream stops here: its status word refuses every later chunk until it is reset
      if (tid == 0) {
        hdr[BSS_STATUS] = sh.fail; hdr[BSS_FRAMES] = fbase + tdone;
        hdr[BSS_NCOLLECT] = sh.ncollect; hdr[BSS_NCOLLECT_IN] = sh.ncollect_in; hdr[BSS_PEAK] = sh.peak;
        p.counts[b] = 0; p.status[b] = sh.fail; p.ncommit[b] = 0;
      }
      return;
    }
  }

  // ---- output: stable order by score (FUSED: score + total + final[state]), then the back-trace of every hypothesis
  if (tid < nA) sh.rval[tid] = FUSED ? (a.score[tid] + a.tot[tid]) + (double)p.ffinal[FUSE == FUSE_NGRAM ? clampi(a.st[tid], 0, p.n_states - 1) : a.st[tid]] : a.score[tid];
  __syncthreads();
  if (tid < nA) {
    const double key = sh.rval[tid];
    const long base = (long)b * W + output_slot(sh.rval, tid, nA, W);
    const int ML = p.max_len;   // the root carries the leading blank and frame -1; STREAM: the tail below the root
    p.lens[base] = tree_backtrace(nd, a.node[tid], !STREAM, ML, p.tokens + base * ML, p.frames ? p.frames + base * ML : nullptr);
    p.scores[base] = a.score[tid];
    if (FUSED) p.fused[base] = key;
  }
  if (tid == 0) p.counts[b] = nA;
  if constexpr (STREAM) {   // ---- the store: the beam in rank order, then the header
    if (tid < nA) {
      double* bd = reinterpret_cast<double*>(wsb + p.off_beam);
      int* bi = reinterpret_cast<int*>(bd + 2 * W);
      bd[tid] = a.score[tid]; bd[W + tid] = a.tot[tid];
      bi[tid] = a.node[tid]; bi[W + tid] = a.st[tid]; bi[2 * W + tid] = a.slot[tid]; bi[3 * W + tid] = a.tok[tid];
    }
    if (tid == 0) {
      hdr[BSS_NA] = nA; hdr[BSS_NNODES] = sh.nnodes; hdr[BSS_COMMITTED] += sh.ncommit; hdr[BSS_FRAMES] = fbase + tdone;
      hdr[BSS_NCOLLECT] = sh.ncollect; hdr[BSS_NCOLLECT_IN] = sh.ncollect_in; hdr[BSS_PEAK] = sh.peak;
      p.status[b] = RNNT_BEAM_ST_OK; p.ncommit[b] = sh.ncommit;
    }
  }
}

// ---- host: what the two launchers share --------------------------------------------------------------------------------
// the step group: as many hypotheses as the LDS budget holds beside the kernel's static LDS, at most BS_GT; 0: not even one
template <class D>
int bs_group(const D* d) {
  const size_t per = bs_step_floats(d->L, d->Hp, d->O, d->cell) * sizeof(float);
  const size_t room = DEC_MAX_LDS - align_up(sizeof(BsShared), 256);
  size_t g = room / per;
  if (g > (size_t)BS_GT) g = BS_GT;
  if (d->step_group > 0 && (size_t)d->step_group < g) g = d->step_group;
  return (int)g;
}

// V, W, S, blank and the candidate ids of a descriptor (D: rnnt_beam_sync_desc or rnnt_beam_sync_stream_desc)
template <class D>
int bs_check_search_dims(const D* d, const char* who) {
  RNNT_CHECK_ARG(d->V >= 2, "%s: V = %d < 2 (a blank and at least one token)", who, d->V);
  RNNT_CHECK_ARG(d->beam >= 1 && d->beam <= BS_WMAX, "%s: beam width W = %d outside [1,%d]", who, d->beam, BS_WMAX);
  RNNT_CHECK_ARG(d->max_symbols >= 1 && d->max_symbols <= BS_SMAX, "%s: max_symbols S = %d outside [1,%d]", who, d->max_symbols,
                 BS_SMAX);
  RNNT_CHECK_ARG(d->blank >= 0 && d->blank < d->V, "%s: blank %d outside [0,%d)", who, d->blank, d->V);
  RNNT_CHECK_ARG((int64_t)d->beam * d->V <= (1ll << BS_IDBITS), "%s: W V = %lld exceeds 2^%d candidates per round", who,
                 (long long)d->beam * d->V, BS_IDBITS);
  return RNNT_OK;
}

// the threshold, the step group, the prediction net's sizes and the step's LDS
template <class D>
int bs_check_step(const D* d, const char* who) {
  int rc = check_token_min_logp(d->token_min_logp, who);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->step_group >= 0, "%s: step_group %d < 0 (0: as many as the LDS holds)", who, d->step_group);
  if ((rc = prednet_check_dims<true>(d, who, RNNT_ERR_INVALID)) != RNNT_OK) return rc;
  RNNT_CHECK_ARG(bs_group(d) >= 1, "%s: one hypothesis's step needs %zu B of LDS beside %zu B of search state (> 160 KiB)", who,
                 bs_step_floats(d->L, d->Hp, d->O, d->cell) * sizeof(float), sizeof(BsShared));
  return RNNT_OK;
}

// an *_ilm entry's arguments, before any device work: the struct, and exactly one of the two automaton forms
inline int bs_check_ilm(const rnnt_beam_ilm* ilm, const rnnt_beam_fusion* fusion, const rnnt_beam_ngram* lm, const char* who) {
  RNNT_CHECK_ARG(ilm != nullptr, "%s: null ilm struct", who);
  RNNT_CHECK_ARG(ilm->bias != nullptr, "%s: null ilm bias (fc.bias, V floats on the device)", who);
  RNNT_CHECK_ARG(ilm->weight > 0.f && ilm->weight < __builtin_huge_valf(), "%s: ilm weight must be finite and > 0, got %g", who,
                 (double)ilm->weight);
  RNNT_CHECK_ARG((fusion != nullptr) != (lm != nullptr), "%s: takes exactly one of fusion and lm, got %s", who,
                 fusion ? "both" : "neither");
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

