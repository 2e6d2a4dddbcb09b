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
// The kernel (beam_sync_kernel<FUSE, STREAM, ILM>) lives in beam_sync_shared.hpp: this file launches its STREAM = false
// instances, beam_sync_stream.hip the streaming ones.  ILM (the *_ilm entries): internal-LM subtraction, for a
// non-blank candidate total' = (total_h + arc[s_h, v]) - mu * ilm_h[v] with ilm_h the log-softmax over v != blank of Cv_h + fc.bias.
#include "beam_sync_shared.hpp"

namespace rnnt {
namespace {

struct BsWs {
  float* table;
  u64* keys;
  int* nodes;
  float* slots;
  float* ilm;   // the *_ilm entries only: (B, NS, 2) pairs, behind every other part
  size_t total;
  int SF, NS;
  long maxn;
};

BsWs carve_bs(void* ws, const rnnt_beam_sync_desc* d, bool ilm = false) {
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
  w.ilm = ilm ? reinterpret_cast<float*>(ws_take(p, off, (size_t)B * w.NS * 2 * 4)) : nullptr;
  w.total = off;
  return w;
}

int bs_check_dims(const rnnt_beam_sync_desc* d, const char* who) {
  RNNT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  RNNT_CHECK_ARG(d->T >= 1 && d->B >= 1, "%s: T and B must be positive (T=%d B=%d)", who, d->T, d->B);
  int rc = bs_check_search_dims(d, who);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(1 + (int64_t)d->beam * d->max_symbols * d->T < (1ll << 31) / 5, "%s: 1 + W S T = %lld nodes exceed the node index",
                 who, 1 + (long long)d->beam * d->max_symbols * d->T);
  return bs_check_step(d, who);
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

// the search behind every entry: fusion (dense tables), lm (backoff tables), or neither; ilm on top of either of the two
static int bs_search(const rnnt_beam_sync_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_ngram* lm, bool ngram,
                     const rnnt_beam_ilm* ilm, const rnnt_beam_timing* timing, void* stream, const char* who) {
  int rc = bs_check_dims(d, who);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->A && d->tokens && d->lens && d->scores && d->count, "%s: null A/tokens/lens/scores/count", who);
  RNNT_CHECK_ARG(d->a_st >= 1 && d->a_sb >= 1, "%s: A strides (a_st = %lld, a_sb = %lld) must be positive", who, (long long)d->a_st,
                 (long long)d->a_sb);
  RNNT_CHECK_ARG(timing == nullptr || timing->frames, "%s: timing given without its output (frames)", who);
  BsK k;
  if ((rc = fill_prednet<true>(d, k, who)) != RNNT_OK) return rc;
  if (fusion && (rc = check_fusion_struct(fusion, d->V, who)) != RNNT_OK) return rc;
  k.ng = NgramLm{};
  if (ngram && (rc = check_ngram_struct(lm, d->V, k.ng, who)) != RNNT_OK) return rc;
  const BsWs w = carve_bs(d->workspace, d, ilm != nullptr);
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
  if (ngram) { k.ffinal = lm->final; k.n_states = lm->n_states; k.fused = lm->fused_scores; }
  k.ilm_bias = ilm ? ilm->bias : nullptr; k.ilm_w = ilm ? ilm->weight : 0.f; k.ilm = w.ilm; k.off_ilm = 0;
  const size_t lds = (size_t)k.G * bs_step_floats(d->L, d->Hp, d->O, d->cell) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  const void* fn = ilm      ? (ngram ? (const void*)beam_sync_kernel<FUSE_NGRAM, false, true>
                                     : (const void*)beam_sync_kernel<FUSE_DENSE, false, true>)
                   : ngram  ? (const void*)beam_sync_kernel<FUSE_NGRAM, false>
                   : fusion ? (const void*)beam_sync_kernel<FUSE_DENSE, false>
                            : (const void*)beam_sync_kernel<FUSE_NONE, false>;
  if (lds + sizeof(BsShared) > 64 * 1024) RNNT_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V * d->beam, s);
  BeamK tk{};   // the layer-0 input table: the beam search's kernel, the same matvec and so the same bits
  static_cast<PredNet&>(tk) = static_cast<const PredNet&>(k);
  tk.table = w.table;
  hipLaunchKernelGGL(beam_table_kernel, dim3(d->V), dim3(DEC_THREADS), (size_t)d->Hp * sizeof(float), s, tk);
  RNNT_CHECK_LAUNCH();
  if (ilm && ngram) hipLaunchKernelGGL((beam_sync_kernel<FUSE_NGRAM, false, true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else if (ilm) hipLaunchKernelGGL((beam_sync_kernel<FUSE_DENSE, false, true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else if (ngram) hipLaunchKernelGGL((beam_sync_kernel<FUSE_NGRAM, false>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else if (fusion) hipLaunchKernelGGL((beam_sync_kernel<FUSE_DENSE, false>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else hipLaunchKernelGGL((beam_sync_kernel<FUSE_NONE, false>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_beam_sync_search(const rnnt_beam_sync_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_timing* timing,
                                         void* stream) {
  return bs_search(d, fusion, nullptr, false, nullptr, timing, stream, "beam_sync_search");
}

extern "C" int rnnt_hip_beam_sync_search_ngram(const rnnt_beam_sync_desc* d, const rnnt_beam_ngram* lm, const rnnt_beam_timing* timing,
                                               void* stream) {
  return bs_search(d, nullptr, lm, true, nullptr, timing, stream, "beam_sync_search_ngram");
}

// internal-LM subtraction: the workspace of the entry it extends plus the (B, NS, 2) pairs
extern "C" size_t rnnt_hip_beam_sync_ilm_workspace_bytes(const rnnt_beam_sync_desc* d) {
  if (bs_check_dims(d, "beam_sync_search_ilm") != RNNT_OK) return 0;
  return carve_bs(nullptr, d, true).total;
}

extern "C" int rnnt_hip_beam_sync_search_ilm(const rnnt_beam_sync_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_ngram* lm,
                                             const rnnt_beam_ilm* ilm, const rnnt_beam_timing* timing, void* stream) {
  const char* who = "beam_sync_search_ilm";
  const int rc = bs_check_ilm(ilm, fusion, lm, who);
  if (rc != RNNT_OK) return rc;
  return bs_search(d, fusion, lm, lm != nullptr, ilm, timing, stream, who);
}
