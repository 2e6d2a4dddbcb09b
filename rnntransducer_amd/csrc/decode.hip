// On-device greedy RNN-T decoding.
//
// Replaces JointNet.recognize_greedy (networks/transducer.py:95-145): a host loop over frames with one `.item()` device
// sync per emitted symbol, a single-step prediction-net call (networks/decoder.py:121-123) and the 1-D joint
// (networks/transducer.py:64-69) per symbol.
//
// Semantics kept exactly: per utterance, for t in 0..t_lens[b]-1 (the reference decodes one utterance per call, so its
// encoder_outputs.size(1) IS that utterance's length; t_lens = null visits all T padded frames, which is what a batched
// reference call would do): up to `max_iters` times { tok = argmax_v joint(enc_t, dec); if tok == blank: stop this
// frame; append tok unless it equals the last appended token; advance the prediction net with tok }.
//
// Mapping: logits = A[t] + C with A = gelu(enc) W_e^T + bias for all frames (one hot-path GEMM, computed by the
// caller) and C = gelu(dec) W_d^T, which only changes when a symbol is emitted.  ONE workgroup (1024 threads) per
// utterance keeps the prediction-net state in LDS and streams the weights (L2 / Infinity-Cache resident, shared by
// all utterances) for each emitted symbol; the per-frame work is a V-wide argmax.  No inter-workgroup communication.
//
// The search loop itself (greedy_frames), its parameter struct and its LDS carve-up live in decode_shared.hpp: the streaming
// search (stream.hip) runs the same loop from carried state.  This file has the kernel that primes and runs it from frame
// 0, the batched single step, and their entries.
#include "decode_shared.hpp"

namespace rnnt {
namespace {

// zero state, one step on blank (decoder_input = [[blank]], pred_tokens = [blank]: transducer.py:118-119), then the frame loop
// of decode_shared.hpp from frame 0
__global__ void __launch_bounds__(DEC_THREADS) greedy_decode_kernel(const GreedyK p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GreedyLds s(smem, p.L, p.Hp, p.O, p.V);
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < 2 * p.L * p.Hp; i += DEC_THREADS) s.h[i] = 0.f;  // h and c (hidden_state = None -> zeros)
  __syncthreads();
  prednet_step_lds(p, s, p.blank);
  int n = 0;
  long long last = p.blank;
  int Tb = p.lens ? p.lens[b] : p.T;
  Tb = Tb < 0 ? 0 : (Tb > p.T ? p.T : Tb);
  greedy_frames(p, s, b, Tb, greedy_frame_base(p, b), last, n);   // frame_base is null here: base 0
  if (threadIdx.x == 0) p.ntok[b] = n < p.max_out ? n : p.max_out;
}

// One prediction-net step for a batch (networks/decoder.py:121-123: `self.rnn(embedded, prev_hidden_state)` on a (B,1) token
// column): one workgroup per batch row, state through LDS, same matvec / cell code as the search kernel.
struct StepK : PredNet {   // no joint half: V = O = 0, w_o / b_o / w_d null
  int B;
  const long long* tokens;  // (B)
  const float* h_in;  // (L,B,Hp) or null (zeros)
  const float* c_in;  // LSTM only; or null
  float* h_out;       // (L,B,Hp)
  float* c_out;       // LSTM only
};

__global__ void __launch_bounds__(DEC_THREADS) prednet_step_kernel(const StepK p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Hp = p.Hp, L = p.L;
  float* h = reinterpret_cast<float*>(smem);
  float* c = h + L * Hp;
  float* gi = c + L * Hp;
  float* gh = gi + 4 * Hp;
  float* x = gh + 4 * Hp;
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int i = tid; i < L * Hp; i += DEC_THREADS) {
    const int l = i / Hp, j = i % Hp;
    h[i] = p.h_in ? p.h_in[((long)l * p.B + b) * Hp + j] : 0.f;
    c[i] = (p.c_in && p.cell == RNNT_CELL_LSTM) ? p.c_in[((long)l * p.B + b) * Hp + j] : 0.f;
  }
  const long long tok = p.tokens[b];
  for (int i = tid; i < Hp; i += DEC_THREADS) x[i] = p.emb[tok * Hp + i];
  __syncthreads();
  prednet_cells(p, h, c, gi, gh, x, nullptr);
  for (int i = tid; i < L * Hp; i += DEC_THREADS) {
    const int l = i / Hp, j = i % Hp;
    p.h_out[((long)l * p.B + b) * Hp + j] = h[i];
    if (p.c_out && p.cell == RNNT_CELL_LSTM) p.c_out[((long)l * p.B + b) * Hp + j] = c[i];
  }
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

// both entries: `timing` null = the untimed search (the kernel's frames pointer is null, nothing else differs)
static int greedy_decode_launch(const rnnt_decode_desc* d, const rnnt_greedy_timing* timing, void* stream) {
  RNNT_CHECK_ARG(d != nullptr, "greedy_decode: null descriptor");
  RNNT_CHECK_ARG(d->T >= 1 && d->B >= 1 && d->V >= 1, "greedy_decode: bad dims");
  int rc = prednet_check_dims<true>(d, "greedy_decode", RNNT_ERR_INVALID);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->blank >= 0 && d->blank < d->V && d->max_iters >= 1 && d->max_out >= 1, "greedy_decode: bad blank/max_iters/max_out");
  RNNT_CHECK_ARG(d->A && d->tokens && d->ntok, "greedy_decode: null pointer");
  GreedyK k{};   // no carried state: rows, h, c, Cs, last, frame_base stay null
  if ((rc = fill_prednet<true>(d, k, "greedy_decode")) != RNNT_OK) return rc;
  k.T = d->T; k.B = d->B; k.max_iters = d->max_iters; k.max_out = d->max_out;
  k.A = d->A; k.lens = d->t_lens;
  k.tokens = (long long*)d->tokens; k.ntok = d->ntok;
  k.frames = timing ? timing->frames : nullptr;
  k.logp = timing ? timing->logp : nullptr;
  const size_t lds = greedy_lds_bytes(d->L, d->Hp, d->O, d->V);
  RNNT_CHECK_ARG(lds <= DEC_MAX_LDS, "greedy_decode: state needs %zu B of LDS (> 160 KiB)", lds);
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)greedy_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V, (hipStream_t)stream);
  hipLaunchKernelGGL(greedy_decode_kernel, dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_greedy_decode(const rnnt_decode_desc* d, void* stream) { return greedy_decode_launch(d, nullptr, stream); }

extern "C" int rnnt_hip_greedy_decode_timed(const rnnt_decode_desc* d, const rnnt_greedy_timing* timing, void* stream) {
  RNNT_CHECK_ARG(timing != nullptr && timing->frames && timing->logp, "greedy_decode_timed: null timing outputs (frames, logp)");
  return greedy_decode_launch(d, timing, stream);
}

extern "C" int rnnt_hip_prednet_step(const rnnt_prednet_step_desc* d, void* stream) {
  RNNT_CHECK_ARG(d != nullptr, "prednet_step: null descriptor");
  RNNT_CHECK_ARG(d->B >= 1, "prednet_step: bad dims");
  int rc = prednet_check_dims<false>(d, "prednet_step", RNNT_ERR_INVALID);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->tokens && d->h_out && (d->c_out || d->cell != RNNT_CELL_LSTM), "prednet_step: null pointer");
  StepK k;
  if ((rc = fill_prednet<false>(d, k, "prednet_step")) != RNNT_OK) return rc;
  k.B = d->B; k.tokens = (const long long*)d->tokens;
  k.h_in = d->h_in; k.c_in = d->c_in; k.h_out = d->h_out; k.c_out = d->c_out;
  const size_t lds = ((size_t)2 * d->L * d->Hp + 9 * d->Hp) * 4;
  RNNT_CHECK_ARG(lds <= DEC_MAX_LDS, "prednet_step: state needs %zu B of LDS (> 160 KiB)", lds);
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)prednet_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 8.0 * (double)d->L * d->B * d->Hp, (hipStream_t)stream);
  hipLaunchKernelGGL(prednet_step_kernel, dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}
