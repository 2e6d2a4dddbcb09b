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
// The kernel itself lives in beam_shared.hpp, shared with the streaming search (beam_stream.hip).
// Per-utterance workspace (global memory, touched only by its workgroup): A entries of the current frame, B entries, state
// slots (h, c, C), a slot remap table and the prefix nodes.  State slots are compacted at every frame start (only the
// slots the carried B entries reference stay), so they scale with pops per frame.  Every loop is bounded by a cap; on
// overflow the utterance writes its status and exits (all threads together: every branch below is workgroup-uniform).
#include "beam_shared.hpp"

using namespace rnnt;

static BeamLayout beam_layout(const rnnt_beam_desc* d) {
  return beam_layout(d->V, d->Hp, d->L, d->cell, d->max_candidates, d->max_pops, d->max_states, d->max_nodes, false);
}

extern "C" size_t rnnt_hip_beam_workspace_bytes(const rnnt_beam_desc* d) {
  if (beam_check_dims(d, "beam_search", 1) != RNNT_OK) return 0;
  const BeamLayout l = beam_layout(d);
  return l.table_bytes + l.stride * (size_t)d->B;
}

// both entries: `timing` null = the untimed search (the kernel's frames pointer is null, nothing else differs)
static int beam_search_launch(const rnnt_beam_desc* d, const rnnt_beam_timing* timing, void* stream) {
  int rc = beam_check_dims(d, "beam_search", 1);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->A && d->lens, "beam_search: null pointer");
  BeamK k;
  if ((rc = beam_fill_common(d, k, "beam_search")) != RNNT_OK) return rc;
  k.t_lens = d->t_lens;
  k.lens = d->lens;
  k.frames = timing ? timing->frames : nullptr;
  const BeamLayout l = beam_layout(d);
  RNNT_CHECK_ARG(d->workspace && (reinterpret_cast<uintptr_t>(d->workspace) & 255) == 0 &&
                 d->workspace_bytes >= l.table_bytes + l.stride * (size_t)d->B,
                 "beam_search: workspace must be 256-byte aligned and hold rnnt_hip_beam_workspace_bytes() bytes");
  beam_set_layout(k, d->workspace, l);
  const size_t lds = beam_lds_bytes(d->L, d->Hp, d->O, d->V);
  RNNT_CHECK_ARG(lds <= DEC_MAX_LDS, "beam_search: state needs %zu B of LDS (> 160 KiB)", lds);
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)beam_search_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V, (hipStream_t)stream);
  hipLaunchKernelGGL(beam_table_kernel, dim3(d->V), dim3(DEC_THREADS), (size_t)d->Hp * sizeof(float), (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_search_kernel<false>, dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_beam_search(const rnnt_beam_desc* d, void* stream) { return beam_search_launch(d, nullptr, stream); }

extern "C" int rnnt_hip_beam_search_timed(const rnnt_beam_desc* d, const rnnt_beam_timing* timing, void* stream) {
  RNNT_CHECK_ARG(timing != nullptr && timing->frames, "beam_search_timed: null timing output (frames)");
  return beam_search_launch(d, timing, stream);
}
