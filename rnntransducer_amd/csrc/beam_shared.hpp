// The beam-search kernel shared by the offline search (beam.hip: one launch walks an utterance from [blank] to its last
// frame) and the streaming search (beam_stream.hip: one launch per chunk starts from the carried hypothesis set and leaves
// that set behind).  ONE kernel template: the frame loop (pop / step / log-softmax / children, memo, slot compaction) and the
// n-best selection are the same statements for both, so the two searches cannot drift apart.  STREAM only adds what lies
// around them: load the per-stream header instead of seeding [blank], collect the prefix tree after the last frame of the
// chunk, write y_star tails relative to the committed root, store the header.
//
// FUSED (the rnnt_hip_beam_*_fused entries; token-level fusion, include/rnnt_hip.h): every hypothesis also carries the state of
// a dense deterministic automaton over token ids and the fp64 total of the arc scores its y_star collected, and every place
// the reference switches compare_key to "lm_score" (networks/transducer.py:253-256, 285-295, 355-360) ranks by asr_score +
// total.  The two fields live in side arrays beside A and B, so Hyp stays 32 bytes and the unfused layout does not move; with
// FUSED = false every fused statement is compiled out and the kernel is statement for statement the unfused one.
#pragma once
#include "decode_shared.hpp"
#include "search_shared.hpp"   // check_fusion_struct: one check of the fusion struct for every fused search

namespace rnnt {
namespace {

struct Hyp {       // an A or B entry (32 bytes)
  double score;    // asr_score (fp64: Python floats, transducer.py:322)
  int node;        // prefix-tree node of y_star (without `tok`)
  int tok;         // token appended to node's y_star, or -1
  int state;       // slot of hidden_state, -1 = None (zeros)
  int memo;        // slot holding step(state, last token) = (h', C), or -1
  int live;        // still in A
  int pad;
};

// per-stream header of the streaming workspace (ints at the start of a stream's workspace; STREAM only)
enum { BS_NB = 0, BS_NSLOTS = 1, BS_NNODES = 2, BS_ROOT_LEN = 3, BS_STATUS = 4, BS_FRAMES = 5, BS_HEADER_BYTES = 256 };

struct BeamK : PredNet {
  int T, B, beam, improved;
  int max_cands, max_pops, max_states, max_nodes, max_len;
  double state_beam, expand_beam;
  const float* A;
  const int* t_lens;
  const float* table;  // (V, G*Hp) layer-0 input projection
  char* ws;            // per-utterance workspaces, `ws_stride` bytes each
  size_t ws_stride, off_a, off_b, off_slots, off_remap, off_nodes, off_nmap;
  int slot_floats;     // h[L*Hp] | c[L*Hp] (LSTM) | C[V], padded to 4
  int* tokens;
  int* lens;
  double* scores;
  int* count;
  int* status;
  int* stats;
  int* commit;         // STREAM: (B, max_nodes) tokens committed by this chunk's collection
  int* ncommit;        // STREAM: (B)
  const int* rows;     // stream reset: the rows to seed
  int* frames;         // timed entries: (B, beam, max_len) frame at which each y_star token was appended (-1: the leading
                       // blank), beside `tokens`; null otherwise
  int* commit_frames;  // STREAM, timed entry: (B, max_nodes) beside `commit`; null otherwise
  // FUSED only (null / 0 otherwise)
  const int* fnext;      // (S, V) state after appending token k in state s
  const float* farc;     // (S, V) score of that append
  const float* ffinal;   // (S) added once, inside the n-best selection only
  int n_states;          // S
  double* fused_scores;  // (B, beam) asr_score + total + final, beside `scores`
  size_t off_fa, off_fb; // side arrays of A and B: total[n] (double) | fstate[n] (int)
};

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Per-utterance workspace: [header (stream only)] | A entries | B entries | state slots | slot remap | prefix nodes
// | [node remap (stream only)] | [fusion side arrays of A, of B (fused only): total (double) per entry, then fstate (int)]
struct BeamLayout {
  size_t table_bytes, off_a, off_b, off_slots, off_remap, off_nodes, off_nmap, off_fa, off_fb, stride;
  int slot_floats;
};

static BeamLayout beam_layout(int V, int Hp, int L, int cell, int max_candidates, int max_pops, int max_states, int max_nodes,
                              bool stream, bool fused = false) {
  BeamLayout l;
  l.table_bytes = align256((size_t)V * cell_gates(cell) * Hp * sizeof(float));
  l.slot_floats = slot_floats(L, Hp, cell, V);
  l.off_a = stream ? (size_t)BS_HEADER_BYTES : 0;
  l.off_b = l.off_a + align256((size_t)max_candidates * sizeof(Hyp));
  l.off_slots = l.off_b + align256((size_t)max_pops * sizeof(Hyp));
  l.off_remap = l.off_slots + align256((size_t)max_states * l.slot_floats * sizeof(float));
  l.off_nodes = l.off_remap + align256((size_t)max_states * sizeof(int));
  l.off_nmap = l.off_nodes + align256((size_t)max_nodes * sizeof(int4));
  l.stride = l.off_nmap + (stream ? align256((size_t)max_nodes * sizeof(int)) : 0);
  l.off_fa = l.off_fb = 0;
  if (fused) {   // after everything else: the offsets above are the unfused ones
    l.off_fa = l.stride;
    l.off_fb = l.off_fa + align256((size_t)max_candidates * (sizeof(double) + sizeof(int)));
    l.stride = l.off_fb + align256((size_t)max_pops * (sizeof(double) + sizeof(int)));
  }
  return l;
}

static inline size_t beam_lds_bytes(int L, int Hp, int O, int V) {
  return 20 * sizeof(double) + 32 * sizeof(int) + 16 * sizeof(float) +
         ((size_t)2 * L * Hp + 9 * (size_t)Hp + O + 2 * (size_t)V) * sizeof(float);
}

// table[k] = W_ih0 emb[k] + b_ih0, one workgroup per token
__global__ void __launch_bounds__(DEC_THREADS) beam_table_kernel(const BeamK p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* x = reinterpret_cast<float*>(smem);
  const int k = blockIdx.x, NG = cell_gates(p.cell);
  for (int i = threadIdx.x; i < p.Hp; i += DEC_THREADS) x[i] = p.emb[(long)k * p.Hp + i];
  __syncthreads();
  matvec(p.w_ih[0], p.Hp, NG * p.Hp, p.Hp, x, const_cast<float*>(p.table) + (long)k * NG * p.Hp, p.b_ih[0]);
}

// (key desc, index asc) merge: Python's max / stable sort keep the first of equal keys
__device__ __forceinline__ bool better(double s, int i, double bs, int bi) { return s > bs || (s == bs && i < bi); }

// dynamic LDS: redd[16] ctld[4] (double) | redi[16] ctl[16] (int) | redf[16] | h[L*Hp] | c[L*Hp] | gi[4Hp] | gh[4Hp] | x[Hp]
//              | dec[O] | Cv[V] | logp[V]
template <bool STREAM, bool FUSED>
__global__ void __launch_bounds__(DEC_THREADS) beam_search_kernel(const BeamK p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* redd = reinterpret_cast<double*>(smem);
  double* ctld = redd + 16;
  int* redi = reinterpret_cast<int*>(ctld + 4);
  int* ctl = redi + 16;
  float* redf = reinterpret_cast<float*>(ctl + 16);
  const int Hp = p.Hp, V = p.V, L = p.L;
  float* h = redf + 16;
  float* c = h + L * Hp;
  float* gi = c + L * Hp;
  float* gh = gi + 4 * Hp;
  float* x = gh + 4 * Hp;
  float* dec = x + Hp;
  float* Cv = dec + p.O;
  float* logp = Cv + V;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = DEC_THREADS / 64;
  const int b = blockIdx.x;
  const bool lstm = p.cell == RNNT_CELL_LSTM;
  const int NG = cell_gates(p.cell);
  char* ws = p.ws + (size_t)b * p.ws_stride;
  Hyp* cands = reinterpret_cast<Hyp*>(ws + p.off_a);
  Hyp* bents = reinterpret_cast<Hyp*>(ws + p.off_b);
  float* slots = reinterpret_cast<float*>(ws + p.off_slots);
  int* remap = reinterpret_cast<int*>(ws + p.off_remap);
  int4* nodes = reinterpret_cast<int4*>(ws + p.off_nodes);  // (parent, token, len, frame of creation: -1 for [blank])
  int* hdr = reinterpret_cast<int*>(ws);                    // STREAM only
  const int SF = p.slot_floats;
  // FUSED: fusion total and automaton state of A entry i (ftA, fsA) and of B entry i (ftB, fsB); they describe the entry's
  // full y_star, pending `tok` included
  double* ftA = nullptr; int* fsA = nullptr; double* ftB = nullptr; int* fsB = nullptr;
  if constexpr (FUSED) {
    ftA = reinterpret_cast<double*>(ws + p.off_fa); fsA = reinterpret_cast<int*>(ftA + p.max_cands);
    ftB = reinterpret_cast<double*>(ws + p.off_fb); fsB = reinterpret_cast<int*>(ftB + p.max_pops);
  }

  // block-wide argmax of (key desc, index asc); every thread returns the winner (index -1: no candidate)
  auto block_argmax = [&](double key, int idx, double& best) -> int {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ok = __shfl_xor(key, o);
      const int oi = __shfl_xor(idx, o);
      if (better(ok, oi, key, idx)) { key = ok; idx = oi; }
    }
    if (lane == 0) { redd[wave] = key; redi[wave] = idx; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NW; ++w)
        if (better(redd[w], redi[w], key, idx)) { key = redd[w]; idx = redi[w]; }
      ctld[0] = key;
      ctl[0] = idx;
    }
    __syncthreads();
    best = ctld[0];
    const int r = ctl[0];
    __syncthreads();
    return r == 0x7fffffff ? -1 : r;
  };
  // block-wide float reduction in a fixed order (deterministic); max or sum
  auto block_reduce = [&](float v, bool is_max) -> float {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o);
      v = is_max ? fmaxf(v, ov) : v + ov;
    }
    if (lane == 0) redf[wave] = v;
    __syncthreads();
    float r = redf[0];
    for (int w = 1; w < NW; ++w) r = is_max ? fmaxf(r, redf[w]) : r + redf[w];
    __syncthreads();
    return r;
  };
  // exclusive position of this thread's `keep` among the workgroup's, in thread order; `total` = how many keep
  auto block_rank = [&](bool keep, int& total) -> int {
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) redi[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < NW; ++w) {
      before += w < wave ? redi[w] : 0;
      total += redi[w];
    }
    return before + __popcll(bal & ((1ull << lane) - 1ull));
  };
  auto fail = [&](int code) {
    if (tid == 0) {
      p.status[b] = code;
      p.count[b] = 0;
      if constexpr (STREAM) hdr[BS_STATUS] = code;   // the stream stays refused until it is reset
    }
    for (int r = tid; r < p.beam; r += DEC_THREADS) p.lens[(long)b * p.beam + r] = 0;
  };

  int nB, nslots, nnodes;
  int root_len = 0;   // STREAM: tokens committed so far = length of the root's y_star; offline the root is written out too
  int t_base = 0;     // STREAM: frames the stream consumed before this chunk (node frames are absolute)
  int Tb = p.t_lens ? p.t_lens[b] : p.T;
  Tb = Tb < 0 ? 0 : (Tb > p.T ? p.T : Tb);
  if constexpr (STREAM) {
    if (tid == 0) p.ncommit[b] = 0;
    if (Tb == 0) {   // no frames: the stream's workspace stays bitwise as it is; count -1 = "the previous list again"
      if (tid == 0) { p.count[b] = -1; p.status[b] = RNNT_BEAM_ST_OK; }
      return;
    }
    const int st = hdr[BS_STATUS];
    __syncthreads();
    if (st != RNNT_BEAM_ST_OK) { fail(st); return; }
    nB = hdr[BS_NB]; nslots = hdr[BS_NSLOTS]; nnodes = hdr[BS_NNODES]; root_len = hdr[BS_ROOT_LEN];
    t_base = hdr[BS_FRAMES];
  } else {
    // y_star = [blank], state None (transducer.py:276-284)
    if (tid == 0) {
      nodes[0] = make_int4(-1, p.blank, 1, -1);
      Hyp r0;
      r0.score = 0.0; r0.node = 0; r0.tok = -1; r0.state = -1; r0.memo = -1; r0.live = 1; r0.pad = 0;
      bents[0] = r0;
      if constexpr (FUSED) { ftB[0] = 0.0; fsB[0] = 0; }   // state 0 belongs to y_star = [blank]
    }
    __syncthreads();
    nB = 1; nslots = 0; nnodes = 1;
  }
  long long pops_total = 0, steps_total = 0;
  int max_pops_seen = 0, max_cands_seen = 0, max_slots_seen = 0;

  for (int t = 0; t < Tb; ++t) {
    // ---- A = B_prev (transducer.py:287-288); keep only the state slots it references, compacted in slot order ----
    if (nB > p.max_cands) { fail(RNNT_BEAM_ST_CANDIDATES); return; }
    for (int s = tid; s < nslots; s += DEC_THREADS) remap[s] = -1;
    __syncthreads();
    for (int i = tid; i < nB; i += DEC_THREADS) {
      Hyp e = bents[i];
      e.tok = -1;
      e.live = 1;
      cands[i] = e;
      if constexpr (FUSED) { ftA[i] = ftB[i]; fsA[i] = fsB[i]; }
      if (e.state >= 0) remap[e.state] = 1;
      if (e.memo >= 0) remap[e.memo] = 1;
    }
    __syncthreads();
    if (tid == 0) {
      int n = 0;
      for (int s = 0; s < nslots; ++s)
        if (remap[s] >= 0) remap[s] = n++;
      ctl[1] = n;
    }
    __syncthreads();
    const int nlive = ctl[1];
    for (int s = 0; s < nslots; ++s) {  // increasing s, destination r <= s: never overwrites a slot still to be moved
      const int r = remap[s];
      if (r >= 0 && r != s) {
        for (int i = tid; i < SF; i += DEC_THREADS) slots[(long)r * SF + i] = slots[(long)s * SF + i];
        __syncthreads();
      }
    }
    for (int i = tid; i < nB; i += DEC_THREADS) {
      if (cands[i].state >= 0) cands[i].state = remap[cands[i].state];
      if (cands[i].memo >= 0) cands[i].memo = remap[cands[i].memo];
    }
    __syncthreads();
    nslots = nlive;
    int nA = nB;
    nB = 0;
    double bestB = 0.0;
    int npops = 0;
    const float* At = p.A + ((long)t * p.B + b) * V;

    for (;;) {  // at most max_pops + 1 passes
      double abest;
      double key = -__builtin_huge_val();
      int idx = 0x7fffffff;
      if constexpr (FUSED) {   // compare_key = "lm_score" (:285-288): asr_score + fusion total
        for (int i = tid; i < nA; i += DEC_THREADS)
          if (cands[i].live) {
            const double k = cands[i].score + ftA[i];
            if (better(k, i, key, idx)) { key = k; idx = i; }
          }
      } else {
        for (int i = tid; i < nA; i += DEC_THREADS)
          if (cands[i].live && better(cands[i].score, i, key, idx)) { key = cands[i].score; idx = i; }
      }
      const int ia = block_argmax(key, idx, abest);
      if (ia < 0) break;  // A empty (transducer.py:286; after a pop the reference's max(A) would raise here instead)
      if (npops > 0 && nB >= p.beam && bestB > abest) break;  // :355-358
      if (p.improved && (nB == 0 ? -9999.0 : bestB) >= p.state_beam + abest) break;  // :291-302
      if (npops >= p.max_pops) { fail(RNNT_BEAM_ST_POPS); return; }

      // ---- pop (transducer.py:304) ----
      const Hyp a = cands[ia];
      double a_ft = 0.0;   // FUSED: the popped entry's total and state, uniform across the workgroup
      int a_fs = 0;
      if constexpr (FUSED) { a_ft = ftA[ia]; a_fs = fsA[ia]; }
      __syncthreads();
      if (tid == 0) cands[ia].live = 0;
      int node = a.node, last;
      if (a.tok >= 0) {
        if (nnodes >= p.max_nodes) { fail(RNNT_BEAM_ST_NODES); return; }
        const int len = nodes[a.node].z + 1;
        if (tid == 0) nodes[nnodes] = make_int4(a.node, a.tok, len, t_base + t);
        node = nnodes++;
        last = a.tok;
      } else {
        last = nodes[a.node].y;
      }
      int S = a.memo;
      if (S < 0) {  // one prediction-net step on y_star[-1] from the popped state (:307-312)
        if (nslots >= p.max_states) { fail(RNNT_BEAM_ST_STATES); return; }
        S = nslots++;
        const float* st = a.state >= 0 ? slots + (long)a.state * SF : nullptr;
        for (int i = tid; i < L * Hp; i += DEC_THREADS) {
          h[i] = st ? st[i] : 0.f;
          c[i] = (st && lstm) ? st[L * Hp + i] : 0.f;
        }
        for (int i = tid; i < Hp; i += DEC_THREADS) x[i] = p.emb[(long)last * Hp + i];
        __syncthreads();
        prednet_cells(p, h, c, gi, gh, x, p.table + (long)last * NG * Hp);
        prednet_joint_half(p, h + (L - 1) * Hp, dec, Cv);
        float* sl = slots + (long)S * SF;
        for (int i = tid; i < L * Hp; i += DEC_THREADS) {
          sl[i] = h[i];
          if (lstm) sl[L * Hp + i] = c[i];
        }
        for (int v = tid; v < V; v += DEC_THREADS) sl[SF - V + v] = Cv[v];  // C sits at the end of the slot
        ++steps_total;
      }
      const float* Cs = slots + (long)S * SF + (SF - V);
      __syncthreads();

      // ---- logp = log_softmax(joint) in fp32 (:313-315) ----
      float m = -__builtin_huge_valf();
      for (int v = tid; v < V; v += DEC_THREADS) {
        const float z = At[v] + Cs[v];
        logp[v] = z;
        m = fmaxf(m, z);
      }
      m = block_reduce(m, true);
      float s = 0.f;
      for (int v = tid; v < V; v += DEC_THREADS) s += expf(logp[v] - m);
      const float ls = logf(block_reduce(s, false));
      float bp = -__builtin_huge_valf();
      for (int v = tid; v < V; v += DEC_THREADS) {
        const float l = (logp[v] - m) - ls;
        logp[v] = l;
        if (v >= 1) bp = fmaxf(bp, l);
      }
      const float thr = block_reduce(bp, true) - (float)p.expand_beam;  // best_prob = max(logp[1:]) (:317), fp32 tensor math

      // ---- children (:319-350): blank -> B (old state, memo = this step), the rest -> A in k order ----
      const double sb = a.score + (double)logp[p.blank];
      if (tid == 0) {
        Hyp e;
        e.score = sb; e.node = node; e.tok = -1; e.state = a.state; e.memo = S; e.live = 0; e.pad = 0;
        bents[nB] = e;  // nB == npops < max_pops
        if constexpr (FUSED) { ftB[nB] = a_ft; fsB[nB] = a_fs; }   // a blank appends nothing: state and total as popped
      }
      const double sbk = FUSED ? sb + a_ft : sb;   // a_ft is 0.0 and unused without fusion: sbk is sb itself
      bestB = (nB == 0 || sbk > bestB) ? sbk : bestB;
      ++nB;
      int base = nA;
      for (int k0 = 0; k0 < V; k0 += DEC_THREADS) {
        const int k = k0 + tid;
        const bool keep = k < V && k != p.blank && (!p.improved || logp[k] >= thr);
        int total;
        const int pos = base + block_rank(keep, total);
        if (keep && pos < p.max_cands) {
          Hyp e;
          e.score = a.score + (double)logp[k];
          e.node = node; e.tok = k == last ? -1 : k; e.state = S; e.memo = -1; e.live = 1; e.pad = 0;
          cands[pos] = e;
          if constexpr (FUSED) {   // threads run along k: both loads are coalesced; no barrier inside this divergent region
            double ft = a_ft;
            int fs = a_fs;
            if (k != last) {       // the dedupe child appends nothing (:337, :345)
              const long at = (long)a_fs * V + k;
              const int ns = p.fnext[at];
              fs = ns < 0 ? 0 : (ns >= p.n_states ? p.n_states - 1 : ns);   // a table out of range cannot index out of bounds
              ft = a_ft + (double)p.farc[at];
            }
            ftA[pos] = ft; fsA[pos] = fs;
          }
        }
        base += total;
        __syncthreads();
      }
      if (base > p.max_cands) { fail(RNNT_BEAM_ST_CANDIDATES); return; }
      nA = base;
      ++npops;
      __syncthreads();
    }
    pops_total += npops;
    max_pops_seen = npops > max_pops_seen ? npops : max_pops_seen;
    max_cands_seen = nA > max_cands_seen ? nA : max_cands_seen;
    max_slots_seen = nslots > max_slots_seen ? nslots : max_slots_seen;
  }

  if constexpr (STREAM) {
    // ---- prefix-node collection.  Every later hypothesis extends the y_star of a carried B entry, so the lowest common
    // ancestor R of their nodes is final: the chain root..R is committed, R becomes the root, and only the nodes on a path
    // from R to a B entry stay (compacted in index order: a parent keeps a lower index than its children, R gets 0).
    // Node lengths stay absolute.  Node numbers never enter a decision, so no result changes.  Loops <= nnodes passes. ----
    if (nB > 0) {
      int* nmap = reinterpret_cast<int*>(ws + p.off_nmap);
      for (int n = tid; n < nnodes; n += DEC_THREADS) nmap[n] = 0;
      __syncthreads();
      for (int i = tid; i < nB; i += DEC_THREADS) {   // mark every path from a B entry up to the root
        int n = bents[i].node;
        for (int s = 0; s < nnodes && n >= 0; ++s) { nmap[n] = 1; n = nodes[n].x; }
      }
      __syncthreads();
      if (tid == 0) {   // the path of entry 0 holds R
        int n = bents[0].node;
        for (int s = 0; s < nnodes && n >= 0; ++s) { nmap[n] = 2; n = nodes[n].x; }
      }
      __syncthreads();
      double key = -__builtin_huge_val();
      int idx = 0x7fffffff;
      for (int i = tid; i < nB; i += DEC_THREADS) {   // where entry i's path joins entry 0's; R is the shallowest of these
        int n = bents[i].node;
        for (int s = 0; s < nnodes && nmap[n] != 2; ++s) n = nodes[n].x;
        const double k = -(double)nodes[n].z;
        if (better(k, n, key, idx)) { key = k; idx = n; }
      }
      double kbest;
      const int R = block_argmax(key, idx, kbest);
      const int lenR = nodes[R].z, nnew = lenR - root_len;
      if (tid == 0) {
        int* out = p.commit + (long)b * p.max_nodes;   // nnew < nnodes <= max_nodes
        int* outf = p.commit_frames ? p.commit_frames + (long)b * p.max_nodes : nullptr;
        int n = R;
        for (int j = nnew - 1; j >= 0; --j) {
          const int4 nd = nodes[n];
          out[j] = nd.y;
          if (outf) outf[j] = nd.w;
          n = nd.x;
        }
        p.ncommit[b] = nnew;
      }
      int base = 0;
      for (int k0 = 0; k0 < nnodes; k0 += DEC_THREADS) {   // new index = rank among the kept nodes
        const int n = k0 + tid;
        const bool keep = n < nnodes && nmap[n] != 0 && nodes[n].z >= lenR;
        int total;
        const int pos = base + block_rank(keep, total);
        if (n < nnodes) nmap[n] = keep ? pos : -1;
        base += total;
        __syncthreads();
      }
      for (int k0 = 0; k0 < nnodes; k0 += DEC_THREADS) {   // destination <= source, sources of this pass read before any write
        const int n = k0 + tid;
        const int dst = n < nnodes ? nmap[n] : -1;
        int4 nd = make_int4(0, 0, 0, 0);
        if (dst >= 0) nd = nodes[n];
        __syncthreads();
        if (dst >= 0) {
          nd.x = n == R ? -1 : nmap[nd.x];
          nodes[dst] = nd;
        }
        __syncthreads();
      }
      for (int i = tid; i < nB; i += DEC_THREADS) bents[i].node = nmap[bents[i].node];
      __syncthreads();
      nnodes = base;
      root_len = lenR;
    }
  }

  // ---- n-best (:360-361): stable sort by asr_score / len(y_star) descending, first `beam` ----
  const int nout = nB < p.beam ? nB : p.beam;
  for (int i = tid; i < nB; i += DEC_THREADS) bents[i].live = 1;
  __syncthreads();
  for (int r = 0; r < nout; ++r) {
    double key = -__builtin_huge_val();
    int idx = 0x7fffffff;
    for (int i = tid; i < nB; i += DEC_THREADS)
      if (bents[i].live) {
        double k;
        if constexpr (FUSED) k = (bents[i].score + ftB[i] + (double)p.ffinal[fsB[i]]) / (double)nodes[bents[i].node].z;
        else k = bents[i].score / (double)nodes[bents[i].node].z;
        if (better(k, i, key, idx)) { key = k; idx = i; }
      }
    double kbest;
    const int ib = block_argmax(key, idx, kbest);
    const Hyp e = bents[ib];
    const int len = nodes[e.node].z;
    if (len - root_len > p.max_len) { fail(RNNT_BEAM_ST_LEN); return; }
    if (tid == 0) {
      bents[ib].live = 0;
      int* out = p.tokens + ((long)b * p.beam + r) * p.max_len;
      int* outf = p.frames ? p.frames + ((long)b * p.beam + r) * p.max_len : nullptr;
      int n = e.node;
      for (int j = len - 1; j >= root_len; --j) {  // offline: len steps, the root has length 1; STREAM: the tail below the root
        const int4 nd = nodes[n];
        out[j - root_len] = nd.y;
        if (outf) outf[j - root_len] = nd.w;
        n = nd.x;
      }
      p.lens[(long)b * p.beam + r] = len - root_len;
      p.scores[(long)b * p.beam + r] = e.score;
      if constexpr (FUSED)   // `final` is applied here only and never stored back: the carried B set stays chunk-invariant
        p.fused_scores[(long)b * p.beam + r] = e.score + ftB[ib] + (double)p.ffinal[fsB[ib]];
    }
    __syncthreads();
  }
  for (int r = nout + tid; r < p.beam; r += DEC_THREADS) p.lens[(long)b * p.beam + r] = 0;
  if (tid == 0) {
    p.count[b] = nout;
    p.status[b] = RNNT_BEAM_ST_OK;
    if (p.stats) {
      int* st = p.stats + (long)b * RNNT_BEAM_NSTATS;
      st[0] = (int)pops_total; st[1] = (int)steps_total; st[2] = max_pops_seen; st[3] = max_cands_seen;
      st[4] = max_slots_seen; st[5] = nnodes;
    }
    if constexpr (STREAM) {
      hdr[BS_NB] = nB; hdr[BS_NSLOTS] = nslots; hdr[BS_NNODES] = nnodes; hdr[BS_ROOT_LEN] = root_len;
      hdr[BS_FRAMES] = t_base + Tb;
    }
  }
}

// checks and copies the descriptor fields both searches share (D: rnnt_beam_desc or rnnt_beam_stream_desc); t_lens, lens and
// the workspace layout are the caller's
template <class D>
static int beam_fill_common(const D* d, BeamK& k, const char* who) {
  RNNT_CHECK_ARG(d->tokens && d->scores && d->count && d->status, "%s: null pointer", who);
  const int rc = fill_prednet<true>(d, k, who);
  if (rc != RNNT_OK) return rc;
  k.T = d->T; k.B = d->B;
  k.beam = d->beam; k.improved = d->improved ? 1 : 0; k.state_beam = d->state_beam; k.expand_beam = d->expand_beam;
  k.max_cands = d->max_candidates; k.max_pops = d->max_pops; k.max_states = d->max_states; k.max_nodes = d->max_nodes;
  k.max_len = d->max_len;
  k.A = d->A;
  k.tokens = d->tokens; k.scores = d->scores; k.count = d->count; k.status = d->status; k.stats = d->stats;
  k.commit = nullptr; k.ncommit = nullptr; k.rows = nullptr; k.frames = nullptr; k.commit_frames = nullptr;
  k.fnext = nullptr; k.farc = nullptr; k.ffinal = nullptr; k.n_states = 0; k.fused_scores = nullptr; k.off_fa = k.off_fb = 0;
  return RNNT_OK;
}

static inline void beam_set_layout(BeamK& k, void* workspace, const BeamLayout& l) {
  k.table = reinterpret_cast<const float*>(workspace);
  k.ws = reinterpret_cast<char*>(workspace) + l.table_bytes;
  k.ws_stride = l.stride; k.off_a = l.off_a; k.off_b = l.off_b; k.off_slots = l.off_slots; k.off_remap = l.off_remap;
  k.off_nodes = l.off_nodes; k.off_nmap = l.off_nmap; k.off_fa = l.off_fa; k.off_fb = l.off_fb;
  k.slot_floats = l.slot_floats;
}

// the fused entries' extra struct, checked on the host before any device work; copies it into the kernel's descriptor
static int beam_fill_fusion(const rnnt_beam_fusion* f, int V, BeamK& k, const char* who) {
  RNNT_CHECK_ARG(f != nullptr, "%s: null fusion struct", who);
  const int rc = check_fusion_struct(f, V, who);
  if (rc != RNNT_OK) return rc;
  k.fnext = f->next; k.farc = f->arc; k.ffinal = f->final; k.n_states = f->n_states; k.fused_scores = f->fused_scores;
  return RNNT_OK;
}

template <class D>
static int beam_check_dims(const D* d, const char* who, int min_T) {
  RNNT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  RNNT_CHECK_ARG(d->T >= min_T && d->B >= 1 && d->V >= 2, "%s: bad dims (V >= 2)", who);
  const int rc = prednet_check_dims<true>(d, who, RNNT_ERR_INVALID);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->blank >= 0 && d->blank < d->V && d->beam >= 1, "%s: bad blank / beam width", who);
  RNNT_CHECK_ARG(d->max_candidates >= 1 && d->max_pops >= 1 && d->max_states >= 1 && d->max_nodes >= 1 && d->max_len >= 1,
                 "%s: caps must be >= 1", who);
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt
