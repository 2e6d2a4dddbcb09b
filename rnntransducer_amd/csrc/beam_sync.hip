// Frame-synchronous transducer beam search with batched hypothesis steps, for gfx950.  DESIGN.md §20.
//
// Definition (include/rnnt_hip.h states it in full).  A_t = gelu(enc_t) W_e^T + bias (time-major, the caller's), the prediction
// net and its half of the joint (PredNet), blank, W = beam width in [1,64], S = max_symbols in [1,4], token_min_logp.
// A hypothesis is a prefix-tree node (its token sequence y; root = [blank]; ONE node per prefix), an fp64 score, a
// prediction-net state with its joint half Cv, and with fusion an automaton state and an fp64 total.
// lp_h[v] = fp32 log-softmax over v of A_t[v] + Cv_h[v].
//   start   one hypothesis: the root, score 0, state = one step on blank from the zero state
//   frame t < T_b: C = the beam A, D = empty; rounds r = 0..S-1, stopping when C is empty:
//     1. candidates of member h at rank i of C: blank with value score_h + lp_h[blank]; every v != blank with
//        lp_h[v] >= token_min_logp with value score_h + lp_h[v]; id = i V + v.  Fused: key = value + total', total' = total_h
//        for blank, total_h + arc[s_h, v] otherwise; the pruning test stays on lp.
//     2. the min(W, #candidates) best by (key descending, id ascending) are selected; a value (or key) of -inf is dropped.
//     3. in rank order: a selected blank closes h: it goes to D under h's node, merged by score = logaddexp(old, new) if that
//        node is in D already.  A selected token v makes the child: its node is found among the parent node's children or
//        created; it carries the new score, the automaton advanced and the prediction-net state one step further.  r < S-1:
//        the child joins the next round's C in rank order.  r = S-1: the child goes to D like a closed one.
//     4. the next A = the min(W, |D|) best of D by (score [+ total] descending, order of first insertion ascending).
//   output  A after the last valid frame, best first by score (fused: score + total + final[state]), ties in A's order, no
//           length normalisation; T_b = 0 gives [[blank]] with score 0.
// Bounds: at most W new nodes per round, 1 + W S T nodes per utterance, |D| <= (S+1) W, len(y) <= 1 + S T.  Nothing can
// overflow at run time: the workspace query sizes all of it.
//
// One workgroup of 1024 threads per utterance, one launch per batch, no traffic between workgroups.  The beam, C and D live in
// LDS.  Per round:
//   step     the members of C that have no state yet (the last round's children; at a frame's end the new A's) advance TOGETHER
//            (batched step, below)
//   softmax  a wavefront per member row, lanes along v; the same wavefront then fills the row's candidate keys as
//            order-preserving 64-bit integers (0 = no candidate)
//   select   the W best by (key descending, lowest id): select_top of search_shared.hpp, the function ctc_beam.hip calls
//   build    ranked by counting, one writer per element; nodes are found or created in the prefix tree of search_shared.hpp
// A child's step is deferred to the round that reads its state: the children of a frame's last round get theirs at the next
// frame's start, so only if they survive the frame's top-W of D, and nothing steps after the last frame.
//
// Batched step.  The hypotheses to advance are staged in LDS in groups of G (the host computes G from the LDS budget, at most
// BS_GT = 8).  Each wave loads its RU weight rows ONCE per group and forms the dot product with every hypothesis of the group:
// W_hh, the deeper layers' W_ih, w_o and w_d are streamed once per group, not once per hypothesis.  Per hypothesis the
// arithmetic is matvec's (decode_shared.hpp), expression for expression: the same four-term sum per k chunk, the same
// butterfly, the same bias add; the cells and the joint half are those of prednet_cells / prednet_joint_half; layer 0 reads the
// (V, G Hp) input table beam_table_kernel builds.  No sum depends on the group: a hypothesis's h, c and Cv are the same bits
// whatever the group it sits in, and a row alone gives the bits it gives in any batch.
// State slots (h | c | Cv) live in the caller's workspace, (S+2) W per utterance: W for the beam, (S-1) W for the rounds'
// children, W for the next beam's pending steps; the free list is rebuilt at every frame's start from the slots the beam holds.
// All score sums are fp64 with logaddexp_d in the fixed order above: bitwise reproducible.
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
  double* fused;
};

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
// writes (h', c', Cv') there.  Ends with a barrier.
__device__ __forceinline__ void bs_step_pending(const BsK& p, BsShared& sh, BsList& ls, int n, float* slots, const BsStepLds& sl) {
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
}

template <bool FUSED>
__global__ void __launch_bounds__(DEC_THREADS) beam_sync_kernel(const BsK p) {
  __shared__ BsShared sh;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = p.V, W = p.W, S = p.S, SF = p.SF, NS = p.NS, blank = p.blank;
  const int Tb = p.t_lens ? clampi(p.t_lens[b], 0, p.T) : p.T;
  const long maxn = p.maxn;
  u64* ck = p.keys + (long)b * W * V;
  float* slots = p.slots + (long)b * NS * SF;
  const PrefixTree nd = tree_view(p.nodes + (long)b * 5 * maxn, maxn);
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
  if (tid == 0) {
    BsList& c = sh.c[0];
    c.score[0] = 0.0; c.tot[0] = 0.0; c.node[0] = 0; c.st[0] = 0;
    c.slot[0] = -1; c.tok[0] = blank;   // one step on blank from the zero state, as every search here primes an utterance
    tree_root(nd, blank);   // the leading blank
    sh.nnodes = 1; sh.fpos = 0; sh.nD = 0; sh.nnext = 0;
  }
  __threadfence_block();
  __syncthreads();

  int nA = 1, cur = 0;
  for (int t = 0; t < Tb; ++t) {
    const float* At = p.A + (long)t * p.a_st + (long)b * p.a_sb;
    int n = nA;
    if (tid == 0) sh.nD = 0;
    __syncthreads();
    for (int r = 0; r < S && n > 0; ++r) {   // (n is uniform)
      BsList& c = sh.c[cur];
      BsList& nx = sh.c[cur ^ 1];
      const bool last_round = r == S - 1;
      // round 0: the survivors among the last frame's last-round children (frame 0: the root); later: this frame's children
      bs_step_pending(p, sh, c, n, slots, sl);
      if (r == 0) {   // the free list of this frame: every slot the beam does not hold, in slot order
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
        for (int v = lane; v < V; v += 64) {
          const float lp = ((At[v] + Cv[v]) - m) - lse;
          u64 key = 0ull;
          if (v == blank || lp >= p.min_logp) {
            const double val = sc + (double)lp;
            double k = val;
            if (FUSED) k = val + (v == blank ? tt : tt + (double)p.farc[(long)st * V + v]);
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
          if (FUSED) {
            const long o = (long)c.st[i] * V + v;
            sh.rtot[rank] = c.tot[i] + (double)p.farc[o];
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
        if (sh.pending[rank]) tree_link(nd, maxn, sh.pending, sh.rpar, sh.rnode, rank, m, sh.rtok[rank], t);
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
  }

  // ---- output: stable order by score (FUSED: score + total + final[state]), then the back-trace of every hypothesis
  BsList& a = sh.c[cur];
  if (tid < nA) sh.rval[tid] = FUSED ? (a.score[tid] + a.tot[tid]) + (double)p.ffinal[a.st[tid]] : a.score[tid];
  __syncthreads();
  if (tid < nA) {
    const double key = sh.rval[tid];
    const long base = (long)b * W + output_slot(sh.rval, tid, nA, W);
    const int ML = p.max_len;   // the root carries the leading blank and frame -1
    p.lens[base] = tree_backtrace(nd, a.node[tid], true, ML, p.tokens + base * ML, p.frames ? p.frames + base * ML : nullptr);
    p.scores[base] = a.score[tid];
    if (FUSED) p.fused[base] = key;
  }
  if (tid == 0) p.counts[b] = nA;
}

struct BsWs {
  float* table;
  u64* keys;
  int* nodes;
  float* slots;
  size_t total;
  int SF, NS;
  long maxn;
};

BsWs carve_bs(void* ws, const rnnt_beam_sync_desc* d) {
  BsWs w;
  char* p = reinterpret_cast<char*>(ws);
  size_t off = 0;
  const int64_t B = d->B, W = d->beam, S = d->max_symbols, V = d->V, T = d->T;
  w.SF = slot_floats(d->L, d->Hp, d->cell, d->V);
  w.NS = (int)((S + 2) * W);
  w.maxn = 1 + W * S * T;
  w.table = reinterpret_cast<float*>(ws_take(p, off, (size_t)V * cell_gates(d->cell) * d->Hp * 4));
  w.keys = reinterpret_cast<u64*>(ws_take(p, off, (size_t)B * W * V * 8));
  w.nodes = reinterpret_cast<int*>(ws_take(p, off, (size_t)B * 5 * w.maxn * 4));
  w.slots = reinterpret_cast<float*>(ws_take(p, off, (size_t)B * w.NS * w.SF * 4));
  w.total = off;
  return w;
}

// the step group: as many hypotheses as the LDS budget holds beside the kernel's static LDS, at most BS_GT; 0: not even one
int bs_group(const rnnt_beam_sync_desc* d) {
  const size_t per = bs_step_floats(d->L, d->Hp, d->O, d->cell) * sizeof(float);
  const size_t room = DEC_MAX_LDS - align_up(sizeof(BsShared), 256);
  size_t g = room / per;
  if (g > (size_t)BS_GT) g = BS_GT;
  if (d->step_group > 0 && (size_t)d->step_group < g) g = d->step_group;
  return (int)g;
}

int bs_check_dims(const rnnt_beam_sync_desc* d, const char* who) {
  RNNT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  RNNT_CHECK_ARG(d->T >= 1 && d->B >= 1, "%s: T and B must be positive (T=%d B=%d)", who, d->T, d->B);
  RNNT_CHECK_ARG(d->V >= 2, "%s: V = %d < 2 (a blank and at least one token)", who, d->V);
  RNNT_CHECK_ARG(d->beam >= 1 && d->beam <= BS_WMAX, "%s: beam width W = %d outside [1,%d]", who, d->beam, BS_WMAX);
  RNNT_CHECK_ARG(d->max_symbols >= 1 && d->max_symbols <= BS_SMAX, "%s: max_symbols S = %d outside [1,%d]", who, d->max_symbols,
                 BS_SMAX);
  RNNT_CHECK_ARG(d->blank >= 0 && d->blank < d->V, "%s: blank %d outside [0,%d)", who, d->blank, d->V);
  RNNT_CHECK_ARG((int64_t)d->beam * d->V <= (1ll << BS_IDBITS), "%s: W V = %lld exceeds 2^%d candidates per round", who,
                 (long long)d->beam * d->V, BS_IDBITS);
  RNNT_CHECK_ARG(1 + (int64_t)d->beam * d->max_symbols * d->T < (1ll << 31) / 5, "%s: 1 + W S T = %lld nodes exceed the node index",
                 who, 1 + (long long)d->beam * d->max_symbols * d->T);
  int rc = check_token_min_logp(d->token_min_logp, who);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->step_group >= 0, "%s: step_group %d < 0 (0: as many as the LDS holds)", who, d->step_group);
  if ((rc = prednet_check_dims<true>(d, who, RNNT_ERR_INVALID)) != RNNT_OK) return rc;
  RNNT_CHECK_ARG(bs_group(d) >= 1, "%s: one hypothesis's step needs %zu B of LDS beside %zu B of search state (> 160 KiB)", who,
                 bs_step_floats(d->L, d->Hp, d->O, d->cell) * sizeof(float), sizeof(BsShared));
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" size_t rnnt_hip_beam_sync_workspace_bytes(const rnnt_beam_sync_desc* d) {
  if (bs_check_dims(d, "beam_sync_search") != RNNT_OK) return 0;
  return carve_bs(nullptr, d).total;
}

extern "C" int rnnt_hip_beam_sync_step_group(const rnnt_beam_sync_desc* d) {
  if (bs_check_dims(d, "beam_sync_search") != RNNT_OK) return 0;
  return bs_group(d);
}

extern "C" int rnnt_hip_beam_sync_search(const rnnt_beam_sync_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_timing* timing,
                                         void* stream) {
  const char* who = "beam_sync_search";
  int rc = bs_check_dims(d, who);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->A && d->tokens && d->lens && d->scores && d->count, "%s: null A/tokens/lens/scores/count", who);
  RNNT_CHECK_ARG(d->a_st >= 1 && d->a_sb >= 1, "%s: A strides (a_st = %lld, a_sb = %lld) must be positive", who, (long long)d->a_st,
                 (long long)d->a_sb);
  RNNT_CHECK_ARG(timing == nullptr || timing->frames, "%s: timing given without its output (frames)", who);
  BsK k;
  if ((rc = fill_prednet<true>(d, k, who)) != RNNT_OK) return rc;
  if (fusion && (rc = check_fusion_struct(fusion, d->V, who)) != RNNT_OK) return rc;
  const BsWs w = carve_bs(d->workspace, d);
  RNNT_CHECK_ARG(d->workspace && d->workspace_bytes >= w.total, "%s: workspace too small (%zu < %zu)", who, d->workspace_bytes, w.total);
  RNNT_CHECK_ARG((reinterpret_cast<uintptr_t>(d->workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  k.T = d->T; k.B = d->B; k.W = d->beam; k.S = d->max_symbols; k.G = bs_group(d);
  k.min_logp = d->token_min_logp;
  k.A = d->A; k.a_st = (long)d->a_st; k.a_sb = (long)d->a_sb; k.t_lens = d->t_lens;
  k.table = w.table; k.slots = w.slots; k.SF = w.SF; k.NS = w.NS; k.keys = w.keys; k.nodes = w.nodes; k.maxn = w.maxn;
  k.max_len = 1 + d->max_symbols * d->T;
  k.tokens = d->tokens; k.lens = d->lens; k.scores = d->scores; k.counts = d->count;
  k.frames = timing ? timing->frames : nullptr;
  k.fnext = fusion ? fusion->next : nullptr; k.farc = fusion ? fusion->arc : nullptr; k.ffinal = fusion ? fusion->final : nullptr;
  k.n_states = fusion ? fusion->n_states : 1; k.fused = fusion ? fusion->fused_scores : nullptr;
  const size_t lds = (size_t)k.G * bs_step_floats(d->L, d->Hp, d->O, d->cell) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  const void* fn = fusion ? (const void*)beam_sync_kernel<true> : (const void*)beam_sync_kernel<false>;
  if (lds + sizeof(BsShared) > 64 * 1024) RNNT_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V * d->beam, s);
  BeamK tk{};   // the layer-0 input table: the beam search's kernel, the same matvec and so the same bits
  static_cast<PredNet&>(tk) = static_cast<const PredNet&>(k);
  tk.table = w.table;
  hipLaunchKernelGGL(beam_table_kernel, dim3(d->V), dim3(DEC_THREADS), (size_t)d->Hp * sizeof(float), s, tk);
  RNNT_CHECK_LAUNCH();
  if (fusion) hipLaunchKernelGGL((beam_sync_kernel<true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else hipLaunchKernelGGL((beam_sync_kernel<false>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}
