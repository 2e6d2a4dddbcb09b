// Streaming frame-synchronous beam search: rnnt_hip_beam_sync_search's search fed in chunks (semantics in include/rnnt_hip.h,
// DESIGN.md §21).  The kernel is beam_sync_kernel<FUSE, true> of beam_sync_shared.hpp: the offline frame loop, started from the
// carried beam of the stream's workspace instead of the seed, with the prefix-tree collection (bs_collect) at the chunk's end
// and wherever a frame would not find W S free node slots.  One launch per chunk, one workgroup per stream; a stream's part of
// the workspace is touched only by its workgroup, so a stream's result cannot depend on the others.  Chunk invariance: A is
// chunk-invariant (stream.hip); the frame loop reads scores, tokens and ranks, never slot or node numbers; a collected tree
// holds every node a later frame can find again, so a prefix keeps its ONE node and that node's frame.
#include "beam_sync_shared.hpp"

namespace rnnt {
namespace {

// rows[blockIdx.x] of a streaming workspace start a new utterance: the offline search's seed as a carried beam (the root, score
// 0, a pending step on blank from the zero state), the root node, no frames consumed
__global__ void __launch_bounds__(64) beam_sync_stream_reset_kernel(const BsK p) {
  const int b = p.rows[blockIdx.x];
  if (b < 0 || b >= p.B) return;
  char* wsb = p.ws + (size_t)b * p.ws_stride;
  int* hdr = reinterpret_cast<int*>(wsb);
  const int i = threadIdx.x, W = p.W;
  if (i < (int)(BSS_HEADER_BYTES / 4)) hdr[i] = i == BSS_NA || i == BSS_NNODES || i == BSS_COMMITTED || i == BSS_PEAK ? 1 : 0;
  if (i == 0) {
    double* bd = reinterpret_cast<double*>(wsb + p.off_beam);
    int* bi = reinterpret_cast<int*>(bd + 2 * W);
    bd[0] = 0.0; bd[W] = 0.0;
    bi[0] = 0; bi[W] = 0; bi[2 * W] = -1; bi[3 * W] = p.blank;
    tree_root(tree_view(reinterpret_cast<int*>(wsb + p.off_nodes), p.maxn), p.blank);
  }
}

struct BssLayout {
  size_t table_bytes, stride, off_beam, off_slots, off_keys, off_nodes, off_mark, off_remap, off_ilm;
  int SF, NS;
};

// ilm: the layout of the *_ilm entries, one more carried part per stream behind the others: the (NS, 2) pairs of the state slots
BssLayout bss_layout(const rnnt_beam_sync_stream_desc* d, bool ilm = false) {
  BssLayout l;
  const size_t W = d->beam, S = d->max_symbols, V = d->V, N = d->max_nodes;
  l.SF = slot_floats(d->L, d->Hp, d->cell, d->V);
  l.NS = (int)((S + 2) * W);
  l.table_bytes = align_up(V * cell_gates(d->cell) * d->Hp * sizeof(float), 256);
  size_t off = BSS_HEADER_BYTES;
  l.off_beam = off;  off += align_up(W * 32, 256);                       // score, total (fp64); node, state, slot, token (int32)
  l.off_slots = off; off += align_up((size_t)l.NS * l.SF * sizeof(float), 256);
  l.off_keys = off;  off += align_up(W * V * sizeof(u64), 256);          // a round's candidate keys: scratch, not carried
  l.off_nodes = off; off += align_up(5 * N * sizeof(int), 256);
  l.off_mark = off;  off += align_up(N * sizeof(int), 256);              // the collection's two scratch arrays
  l.off_remap = off; off += align_up(N * sizeof(int), 256);
  l.off_ilm = off;   if (ilm) off += align_up((size_t)l.NS * 2 * sizeof(float), 256);
  l.stride = off;
  return l;
}

int bss_check_dims(const rnnt_beam_sync_stream_desc* d, const char* who) {
  RNNT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  RNNT_CHECK_ARG(d->T >= 0 && d->B >= 1, "%s: T must not be negative and B positive (T=%d B=%d)", who, d->T, d->B);
  int rc = bs_check_search_dims(d, who);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->max_nodes >= 1 + 4 * d->beam * d->max_symbols && (int64_t)d->max_nodes < (1ll << 31) / 5,
                 "%s: max_nodes = %d outside [1 + 4 W S = %d, 2^31 / 5): a frame makes up to W S nodes", who, d->max_nodes,
                 1 + 4 * d->beam * d->max_symbols);
  RNNT_CHECK_ARG(d->max_len >= 1, "%s: max_len = %d < 1", who, d->max_len);
  return bs_check_step(d, who);
}

// everything but A, lens and the outputs: the reset entry needs no more
int bss_fill(const rnnt_beam_sync_stream_desc* d, BsK& k, const char* who, bool ilm = false) {
  int rc = bss_check_dims(d, who);
  if (rc != RNNT_OK) return rc;
  if ((rc = fill_prednet<true>(d, k, who)) != RNNT_OK) return rc;
  const BssLayout l = bss_layout(d, ilm);
  RNNT_CHECK_ARG(d->workspace && (reinterpret_cast<uintptr_t>(d->workspace) & 255) == 0 &&
                 d->workspace_bytes >= l.table_bytes + l.stride * (size_t)d->B,
                 "%s: workspace must be 256-byte aligned and hold rnnt_hip_beam_sync_stream%s_workspace_bytes() = %zu bytes", who,
                 ilm ? "_ilm" : "", l.table_bytes + l.stride * (size_t)d->B);
  k.T = d->T; k.B = d->B; k.W = d->beam; k.S = d->max_symbols; k.G = bs_group(d);
  k.min_logp = d->token_min_logp;
  k.A = nullptr; k.a_st = 0; k.a_sb = 0; k.t_lens = nullptr;
  k.table = reinterpret_cast<const float*>(d->workspace);
  k.slots = nullptr; k.keys = nullptr; k.nodes = nullptr;
  k.SF = l.SF; k.NS = l.NS; k.maxn = d->max_nodes; k.max_len = d->max_len;
  k.tokens = nullptr; k.lens = nullptr; k.scores = nullptr; k.counts = nullptr; k.frames = nullptr;
  k.fnext = nullptr; k.farc = nullptr; k.ffinal = nullptr; k.n_states = 1; k.fused = nullptr; k.ng = NgramLm{};
  k.ws = reinterpret_cast<char*>(d->workspace) + l.table_bytes;
  k.ws_stride = l.stride;
  k.off_beam = l.off_beam; k.off_slots = l.off_slots; k.off_keys = l.off_keys; k.off_nodes = l.off_nodes;
  k.off_mark = l.off_mark; k.off_remap = l.off_remap;
  k.off_ilm = l.off_ilm; k.ilm = nullptr; k.ilm_bias = nullptr; k.ilm_w = 0.f;
  k.status = nullptr; k.commit = nullptr; k.commit_frames = nullptr; k.ncommit = nullptr; k.commit_ld = 0; k.rows = nullptr;
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" size_t rnnt_hip_beam_sync_stream_workspace_bytes(const rnnt_beam_sync_stream_desc* d) {
  if (bss_check_dims(d, "beam_sync_stream") != RNNT_OK) return 0;
  const BssLayout l = bss_layout(d);
  return l.table_bytes + l.stride * (size_t)d->B;
}

// the reset behind both entries: the two differ in the workspace's layout alone (the pairs need no seed: a slot's pair is
// written by the step that fills the slot, before anything reads it)
static int bss_reset(const rnnt_beam_sync_stream_desc* d, const int32_t* rows, int32_t n_rows, int32_t build_table, bool ilm,
                     void* stream, const char* who) {
  BsK k;
  const int rc = bss_fill(d, k, who, ilm);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(n_rows >= 0 && (rows || n_rows == 0), "%s: bad row list", who);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->V * d->Hp, s);
  if (build_table) {   // the layer-0 input table: the beam search's kernel, the same matvec and so the same bits
    BeamK tk{};
    static_cast<PredNet&>(tk) = static_cast<const PredNet&>(k);
    tk.table = reinterpret_cast<float*>(d->workspace);
    hipLaunchKernelGGL(beam_table_kernel, dim3(d->V), dim3(DEC_THREADS), (size_t)d->Hp * sizeof(float), s, tk);
    RNNT_CHECK_LAUNCH();
  }
  if (n_rows > 0) {
    k.rows = rows;
    hipLaunchKernelGGL(beam_sync_stream_reset_kernel, dim3(n_rows), dim3(64), 0, s, k);
    RNNT_CHECK_LAUNCH();
  }
  return RNNT_OK;
}

extern "C" int rnnt_hip_beam_sync_stream_reset(const rnnt_beam_sync_stream_desc* d, const int32_t* rows, int32_t n_rows,
                                               int32_t build_table, void* stream) {
  return bss_reset(d, rows, n_rows, build_table, false, stream, "beam_sync_stream_reset");
}

// the chunk call behind every entry: fusion (dense tables), lm (backoff tables), or neither; ilm on top of either of the two
static int bss_chunk(const rnnt_beam_sync_stream_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_ngram* lm, bool ngram,
                     const rnnt_beam_ilm* ilm, const rnnt_beam_timing* timing, void* stream, const char* who) {
  BsK k;
  int rc = bss_fill(d, k, who, ilm != nullptr);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->T >= 1 && d->A && d->lens, "%s: needs T >= 1 frames, A and lens", who);
  RNNT_CHECK_ARG(d->a_st >= 1 && d->a_sb >= 1, "%s: A strides (a_st = %lld, a_sb = %lld) must be positive", who, (long long)d->a_st,
                 (long long)d->a_sb);
  RNNT_CHECK_ARG(d->tokens && d->out_lens && d->scores && d->count && d->status && d->commit && d->ncommit,
                 "%s: null tokens/out_lens/scores/count/status/commit/ncommit", who);
  RNNT_CHECK_ARG(timing == nullptr || (timing->frames && timing->commit_frames),
                 "%s: timing given without its outputs (frames, commit_frames)", who);
  if (fusion && (rc = check_fusion_struct(fusion, d->V, who)) != RNNT_OK) return rc;
  if (ngram && (rc = check_ngram_struct(lm, d->V, k.ng, who)) != RNNT_OK) return rc;
  k.A = d->A; k.a_st = (long)d->a_st; k.a_sb = (long)d->a_sb; k.t_lens = d->lens;
  k.tokens = d->tokens; k.lens = d->out_lens; k.scores = d->scores; k.counts = d->count;
  k.status = d->status; k.commit = d->commit; k.ncommit = d->ncommit;
  k.commit_ld = (long)d->max_nodes + (long)d->max_symbols * d->T;
  k.frames = timing ? timing->frames : nullptr; k.commit_frames = timing ? timing->commit_frames : nullptr;
  k.fnext = fusion ? fusion->next : nullptr; k.farc = fusion ? fusion->arc : nullptr; k.ffinal = fusion ? fusion->final : nullptr;
  k.n_states = fusion ? fusion->n_states : 1; k.fused = fusion ? fusion->fused_scores : nullptr;
  if (ngram) { k.ffinal = lm->final; k.n_states = lm->n_states; k.fused = lm->fused_scores; }
  if (ilm) { k.ilm_bias = ilm->bias; k.ilm_w = ilm->weight; }
  const size_t lds = (size_t)k.G * bs_step_floats(d->L, d->Hp, d->O, d->cell) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  const void* fn = ilm      ? (ngram ? (const void*)beam_sync_kernel<FUSE_NGRAM, true, true>
                                     : (const void*)beam_sync_kernel<FUSE_DENSE, true, true>)
                   : ngram  ? (const void*)beam_sync_kernel<FUSE_NGRAM, true>
                   : fusion ? (const void*)beam_sync_kernel<FUSE_DENSE, true>
                            : (const void*)beam_sync_kernel<FUSE_NONE, true>;
  if (lds + sizeof(BsShared) > 64 * 1024) RNNT_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V * d->beam, s);
  if (ilm && ngram) hipLaunchKernelGGL((beam_sync_kernel<FUSE_NGRAM, true, true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else if (ilm) hipLaunchKernelGGL((beam_sync_kernel<FUSE_DENSE, true, true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else if (ngram) hipLaunchKernelGGL((beam_sync_kernel<FUSE_NGRAM, true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else if (fusion) hipLaunchKernelGGL((beam_sync_kernel<FUSE_DENSE, true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  else hipLaunchKernelGGL((beam_sync_kernel<FUSE_NONE, true>), dim3(d->B), dim3(DEC_THREADS), lds, s, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_beam_sync_stream_chunk(const rnnt_beam_sync_stream_desc* d, const rnnt_beam_fusion* fusion,
                                               const rnnt_beam_timing* timing, void* stream) {
  return bss_chunk(d, fusion, nullptr, false, nullptr, timing, stream, "beam_sync_stream_chunk");
}

extern "C" int rnnt_hip_beam_sync_stream_chunk_ngram(const rnnt_beam_sync_stream_desc* d, const rnnt_beam_ngram* lm,
                                                     const rnnt_beam_timing* timing, void* stream) {
  return bss_chunk(d, nullptr, lm, true, nullptr, timing, stream, "beam_sync_stream_chunk_ngram");
}

// internal-LM subtraction: a stream opened for it carries the pairs of its state slots, so its workspace has
// its own size and the reset that knows that layout
extern "C" size_t rnnt_hip_beam_sync_stream_ilm_workspace_bytes(const rnnt_beam_sync_stream_desc* d) {
  if (bss_check_dims(d, "beam_sync_stream_ilm") != RNNT_OK) return 0;
  const BssLayout l = bss_layout(d, true);
  return l.table_bytes + l.stride * (size_t)d->B;
}

extern "C" int rnnt_hip_beam_sync_stream_reset_ilm(const rnnt_beam_sync_stream_desc* d, const int32_t* rows, int32_t n_rows,
                                                   int32_t build_table, void* stream) {
  return bss_reset(d, rows, n_rows, build_table, true, stream, "beam_sync_stream_reset_ilm");
}

extern "C" int rnnt_hip_beam_sync_stream_chunk_ilm(const rnnt_beam_sync_stream_desc* d, const rnnt_beam_fusion* fusion,
                                                   const rnnt_beam_ngram* lm, const rnnt_beam_ilm* ilm, const rnnt_beam_timing* timing,
                                                   void* stream) {
  const char* who = "beam_sync_stream_chunk_ilm";
  const int rc = bs_check_ilm(ilm, fusion, lm, who);
  if (rc != RNNT_OK) return rc;
  return bss_chunk(d, fusion, lm, lm != nullptr, ilm, timing, stream, who);
}
