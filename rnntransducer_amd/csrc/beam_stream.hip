// Streaming beam search: rnnt_hip_beam_search's search fed in chunks (semantics in include/rnnt_hip.h).  The kernel is
// beam_search_kernel<true> of beam_shared.hpp: the offline frame loop and n-best selection, started from the carried B set of
// the stream's workspace instead of [blank], followed by the prefix-node collection.  One persistent launch per chunk, one
// workgroup per stream; a stream's workspace is touched only by its workgroup, so a stream's result cannot depend on the
// others.  Chunk invariance: A is chunk-invariant (stream.hip), the search is sequential per-stream code whose decisions
// read scores, tokens and insertion indices in A, never slot or node numbers.
#include "beam_shared.hpp"

namespace rnnt {
namespace {

// rows[blockIdx.x] starts a new utterance: y_star = [blank], state None (transducer.py:276-284), committed = [blank], no
// frames consumed (header word BS_FRAMES = 0)
__global__ void __launch_bounds__(64) beam_stream_reset_kernel(const BeamK p) {
  const int b = p.rows[blockIdx.x];
  if (b < 0 || b >= p.B) return;
  char* ws = p.ws + (size_t)b * p.ws_stride;
  int* hdr = reinterpret_cast<int*>(ws);
  const int i = threadIdx.x;
  if (i < BS_HEADER_BYTES / 4) hdr[i] = i == BS_NB || i == BS_NNODES || i == BS_ROOT_LEN ? 1 : 0;
  if (i == 0) {
    reinterpret_cast<int4*>(ws + p.off_nodes)[0] = make_int4(-1, p.blank, 1, -1);
    Hyp r0;
    r0.score = 0.0; r0.node = 0; r0.tok = -1; r0.state = -1; r0.memo = -1; r0.live = 1; r0.pad = 0;
    reinterpret_cast<Hyp*>(ws + p.off_b)[0] = r0;
    if (p.off_fb) {   // fused layout: B entry 0 starts in automaton state 0 with total 0
      double* ftB = reinterpret_cast<double*>(ws + p.off_fb);
      ftB[0] = 0.0;
      reinterpret_cast<int*>(ftB + p.max_pops)[0] = 0;
    }
  }
}

BeamLayout stream_layout(const rnnt_beam_stream_desc* d, bool fused = false) {
  return beam_layout(d->V, d->Hp, d->L, d->cell, d->max_candidates, d->max_pops, d->max_states, d->max_nodes, true, fused);
}

// `fusion` null = the unfused workspace layout; a stream keeps the layout (and the automaton) it was reset with
int stream_fill(const rnnt_beam_stream_desc* d, BeamK& k, const char* who, const rnnt_beam_fusion* fusion = nullptr) {
  int rc = beam_check_dims(d, who, 0);
  if (rc != RNNT_OK) return rc;
  if ((rc = beam_fill_common(d, k, who)) != RNNT_OK) return rc;
  if (fusion && (rc = beam_fill_fusion(fusion, d->V, k, who)) != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->out_lens && d->commit && d->ncommit, "%s: null pointer", who);
  k.t_lens = d->lens; k.lens = d->out_lens; k.commit = d->commit; k.ncommit = d->ncommit;
  const BeamLayout l = stream_layout(d, fusion != nullptr);
  RNNT_CHECK_ARG(d->workspace && (reinterpret_cast<uintptr_t>(d->workspace) & 255) == 0 &&
                 d->workspace_bytes >= l.table_bytes + l.stride * (size_t)d->B,
                 "%s: workspace must be 256-byte aligned and hold rnnt_hip_beam_stream%s_workspace_bytes() bytes", who,
                 fusion ? "_fused" : "");
  beam_set_layout(k, d->workspace, l);
  const size_t lds = beam_lds_bytes(d->L, d->Hp, d->O, d->V);
  RNNT_CHECK_ARG(lds <= DEC_MAX_LDS, "%s: state needs %zu B of LDS (> 160 KiB)", who, lds);
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" size_t rnnt_hip_beam_stream_workspace_bytes(const rnnt_beam_stream_desc* d) {
  if (beam_check_dims(d, "beam_stream", 0) != RNNT_OK) return 0;
  const BeamLayout l = stream_layout(d);
  return l.table_bytes + l.stride * (size_t)d->B;
}

extern "C" size_t rnnt_hip_beam_stream_fused_workspace_bytes(const rnnt_beam_stream_desc* d) {
  if (beam_check_dims(d, "beam_stream_fused", 0) != RNNT_OK) return 0;
  const BeamLayout l = stream_layout(d, true);
  return l.table_bytes + l.stride * (size_t)d->B;
}

static int beam_stream_reset_launch(const rnnt_beam_stream_desc* d, const rnnt_beam_fusion* fusion, const char* who,
                                    const int32_t* rows, int32_t n_rows, int32_t build_table, void* stream) {
  BeamK k;
  const int rc = stream_fill(d, k, who, fusion);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(n_rows >= 0 && (rows || n_rows == 0), "%s: bad row list", who);
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->V * d->Hp, (hipStream_t)stream);
  if (build_table) {
    hipLaunchKernelGGL(beam_table_kernel, dim3(d->V), dim3(DEC_THREADS), (size_t)d->Hp * sizeof(float), (hipStream_t)stream, k);
    RNNT_CHECK_LAUNCH();
  }
  if (n_rows > 0) {
    k.rows = rows;
    hipLaunchKernelGGL(beam_stream_reset_kernel, dim3(n_rows), dim3(64), 0, (hipStream_t)stream, k);
    RNNT_CHECK_LAUNCH();
  }
  return RNNT_OK;
}

extern "C" int rnnt_hip_beam_stream_reset(const rnnt_beam_stream_desc* d, const int32_t* rows, int32_t n_rows, int32_t build_table,
                                          void* stream) {
  return beam_stream_reset_launch(d, nullptr, "beam_stream_reset", rows, n_rows, build_table, stream);
}

extern "C" int rnnt_hip_beam_stream_reset_fused(const rnnt_beam_stream_desc* d, const rnnt_beam_fusion* fusion, const int32_t* rows,
                                                int32_t n_rows, int32_t build_table, void* stream) {
  RNNT_CHECK_ARG(fusion != nullptr, "beam_stream_reset_fused: null fusion struct");
  return beam_stream_reset_launch(d, fusion, "beam_stream_reset_fused", rows, n_rows, build_table, stream);
}

// all entries: `timing` null = the untimed search (the kernel's two frame pointers are null, nothing else differs); `fusion`
// null = the unfused kernel instance and layout
static int beam_stream_chunk_launch(const rnnt_beam_stream_desc* d, const rnnt_beam_timing* timing, const rnnt_beam_fusion* fusion,
                                    const char* who, void* stream) {
  BeamK k;
  const int rc = stream_fill(d, k, who, fusion);
  if (rc != RNNT_OK) return rc;
  if (timing) { k.frames = timing->frames; k.commit_frames = timing->commit_frames; }
  RNNT_CHECK_ARG(d->T >= 1 && d->A && d->lens, "%s: needs T >= 1 frames, A and lens", who);
  const size_t lds = beam_lds_bytes(d->L, d->Hp, d->O, d->V);
  const void* fn = fusion ? (const void*)beam_search_kernel<true, true> : (const void*)beam_search_kernel<true, false>;
  if (lds > 64 * 1024) RNNT_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V, (hipStream_t)stream);
  if (fusion)
    hipLaunchKernelGGL((beam_search_kernel<true, true>), dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL((beam_search_kernel<true, false>), dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_beam_stream_chunk(const rnnt_beam_stream_desc* d, void* stream) {
  return beam_stream_chunk_launch(d, nullptr, nullptr, "beam_stream_chunk", stream);
}

extern "C" int rnnt_hip_beam_stream_chunk_timed(const rnnt_beam_stream_desc* d, const rnnt_beam_timing* timing, void* stream) {
  RNNT_CHECK_ARG(timing != nullptr && timing->frames && timing->commit_frames,
                 "beam_stream_chunk_timed: null timing outputs (frames, commit_frames)");
  return beam_stream_chunk_launch(d, timing, nullptr, "beam_stream_chunk", stream);
}

// token-level fusion: the stream's automaton is the one its state was reset with; `timing` may be null (no frames)
extern "C" int rnnt_hip_beam_stream_chunk_fused(const rnnt_beam_stream_desc* d, const rnnt_beam_fusion* fusion,
                                                const rnnt_beam_timing* timing, void* stream) {
  RNNT_CHECK_ARG(fusion != nullptr, "beam_stream_chunk_fused: null fusion struct");
  RNNT_CHECK_ARG(timing == nullptr || (timing->frames && timing->commit_frames),
                 "beam_stream_chunk_fused: timing given without its outputs (frames, commit_frames)");
  return beam_stream_chunk_launch(d, timing, fusion, "beam_stream_chunk_fused", stream);
}
