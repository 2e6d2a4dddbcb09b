// On-device RNN-T beam search (networks/transducer.py:215-361 with lm=None, hotwords=None; semantics in include/rnnt_hip.h).
//
// ONE persistent launch per batch: one workgroup (DEC_THREADS threads) per utterance walks all its frames.  As in greedy
// search (decode.hip), logits = A[t] + C with A = gelu(enc) W_e^T + bias precomputed for all frames by the caller and
// C = gelu(dec) W_d^T; the prediction-net step and C use the same code (decode_shared.hpp).  Per pop the remaining work
// is: a block-wide argmax over the live A entries, one step (or none: memo), a V-wide log-softmax, and child generation.
//
// Exact shortcuts:
//   * memo: a step is a pure function of (state, token).  A blank child keeps its parent's state and y_star, so popping it
//     in a later frame repeats the parent's step; each pop's result slot (h', C) is stored with its blank child and reused.
//   * layer 0's input projection W_ih0 emb[k] + b_ih0 is a (V, G*Hp) table built once per call (beam_table_kernel, same
//     matvec, same bits), so only W_hh0 h and the deeper layers are streamed per step.
//   * y_star is a prefix tree of (parent, token, length) nodes.  An A entry is (node, appended token or -1): its node is only
//     made when it is popped, so nodes <= pops.  The dedupe rule (transducer.py:333,343) reads the last token only.
// Token-level fusion (rnnt_hip_beam_search_fused: hotword boosting, token LM tables) is the FUSED instance of the same kernel.
// The kernel itself lives in beam_shared.hpp, shared with the streaming search (beam_stream.hip).
// Per-utterance workspace (global memory, touched only by its workgroup): A entries of the current frame, B entries, state
// slots (h, c, C), a slot remap table and the prefix nodes.  State slots are compacted at every frame start (only the
// slots the carried B entries reference stay), so they scale with pops per frame.  Every loop is bounded by a cap; on
// overflow the utterance writes its status and exits (all threads together: every branch below is workgroup-uniform).
#include "beam_shared.hpp"

using namespace rnnt;

static BeamLayout beam_layout(const rnnt_beam_desc* d, bool fused = false) {
  return beam_layout(d->V, d->Hp, d->L, d->cell, d->max_candidates, d->max_pops, d->max_states, d->max_nodes, false, fused);
}

extern "C" size_t rnnt_hip_beam_workspace_bytes(const rnnt_beam_desc* d) {
  if (beam_check_dims(d, "beam_search", 1) != RNNT_OK) return 0;
  const BeamLayout l = beam_layout(d);
  return l.table_bytes + l.stride * (size_t)d->B;
}

extern "C" size_t rnnt_hip_beam_fused_workspace_bytes(const rnnt_beam_desc* d) {
  if (beam_check_dims(d, "beam_search_fused", 1) != RNNT_OK) return 0;
  const BeamLayout l = beam_layout(d, true);
  return l.table_bytes + l.stride * (size_t)d->B;
}

// all entries: `timing` null = the untimed search (the kernel's frames pointer is null, nothing else differs); `fusion` null =
// the unfused kernel instance and the unfused workspace layout
static int beam_search_launch(const rnnt_beam_desc* d, const rnnt_beam_timing* timing, const rnnt_beam_fusion* fusion,
                              const char* who, void* stream) {
  int rc = beam_check_dims(d, who, 1);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->A && d->lens, "%s: null pointer", who);
  BeamK k;
  if ((rc = beam_fill_common(d, k, who)) != RNNT_OK) return rc;
  if (fusion && (rc = beam_fill_fusion(fusion, d->V, k, who)) != RNNT_OK) return rc;
  k.t_lens = d->t_lens;
  k.lens = d->lens;
  k.frames = timing ? timing->frames : nullptr;
  const BeamLayout l = beam_layout(d, fusion != nullptr);
  RNNT_CHECK_ARG(d->workspace && (reinterpret_cast<uintptr_t>(d->workspace) & 255) == 0 &&
                 d->workspace_bytes >= l.table_bytes + l.stride * (size_t)d->B,
                 "%s: workspace must be 256-byte aligned and hold rnnt_hip_beam%s_workspace_bytes() bytes", who,
                 fusion ? "_fused" : "");
  beam_set_layout(k, d->workspace, l);
  const size_t lds = beam_lds_bytes(d->L, d->Hp, d->O, d->V);
  RNNT_CHECK_ARG(lds <= DEC_MAX_LDS, "%s: state needs %zu B of LDS (> 160 KiB)", who, lds);
  const void* fn = fusion ? (const void*)beam_search_kernel<false, true> : (const void*)beam_search_kernel<false, false>;
  if (lds > 64 * 1024) RNNT_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V, (hipStream_t)stream);
  hipLaunchKernelGGL(beam_table_kernel, dim3(d->V), dim3(DEC_THREADS), (size_t)d->Hp * sizeof(float), (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  if (fusion)
    hipLaunchKernelGGL((beam_search_kernel<false, true>), dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  else
    hipLaunchKernelGGL((beam_search_kernel<false, false>), dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_beam_search(const rnnt_beam_desc* d, void* stream) {
  return beam_search_launch(d, nullptr, nullptr, "beam_search", stream);
}

extern "C" int rnnt_hip_beam_search_timed(const rnnt_beam_desc* d, const rnnt_beam_timing* timing, void* stream) {
  RNNT_CHECK_ARG(timing != nullptr && timing->frames, "beam_search_timed: null timing output (frames)");
  return beam_search_launch(d, timing, nullptr, "beam_search", stream);
}

// token-level fusion (include/rnnt_hip.h): `timing` may be null (no frames)
extern "C" int rnnt_hip_beam_search_fused(const rnnt_beam_desc* d, const rnnt_beam_fusion* fusion, const rnnt_beam_timing* timing,
                                          void* stream) {
  RNNT_CHECK_ARG(fusion != nullptr, "beam_search_fused: null fusion struct");
  RNNT_CHECK_ARG(timing == nullptr || timing->frames, "beam_search_fused: timing given without its output (frames)");
  return beam_search_launch(d, timing, fusion, "beam_search_fused", stream);
}
