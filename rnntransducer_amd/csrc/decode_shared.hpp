// What the search kernels share (decode.hip: offline greedy search and the batched step; stream.hip: streaming greedy search;
// beam_shared.hpp: both beam searches).  One workgroup of DEC_THREADS threads owns one utterance; state vectors live in LDS,
// weights are streamed.  Here: the prediction-net block of every kernel-parameter struct (PredNet) with its one host-side
// check and fill, the prediction-net step pieces, and THE greedy search: its parameter struct (GreedyK), its LDS carve-up and
// size (GreedyLds, greedy_lds_bytes) and its frame loop (greedy_frames), which the offline and the streaming kernel both run.
#pragma once
#include "common.hpp"

namespace rnnt {

constexpr int DEC_THREADS = 1024;
constexpr int DEC_MAX_LAYERS = RNNT_DECODE_MAX_LAYERS;
constexpr size_t DEC_MAX_LDS = 160 * 1024;

// The prediction net and its half of the joint as the kernels read them; every search's parameter struct derives from it.
// `blank` belongs to the block (every search but the batched step reads it), and it makes the ints six: 24 bytes, so `emb`
// follows them at an 8-byte boundary and the struct has no hole.  A derived struct's own members start after `ld_d`, at the
// end of this block.  (With five ints, and the 4-byte hole before `emb`, this toolchain's resource report showed the two
// greedy kernels with 12-16 more bytes of scratch per lane; nothing relies on that.)
struct PredNet {
  int V, Hp, O, L, cell, blank;
  const float* emb;  // (V, Hp)
  const float* w_ih[DEC_MAX_LAYERS];
  const float* w_hh[DEC_MAX_LAYERS];
  const float* b_ih[DEC_MAX_LAYERS];
  const float* b_hh[DEC_MAX_LAYERS];
  const float* w_o;  // (O, Hp)
  const float* b_o;  // (O)
  const float* w_d;  // fc.weight[:, O_enc:] : (V, O) with row stride ld_d
  long ld_d;
};

// Sizes of a descriptor's prediction net (D: any rnnt_*_desc that carries one).  JOINT = false: the batched step, whose
// descriptor has no out_proj / fc half.  A layer count outside the limit returns `layers_rc`: the entries differ in it.
template <bool JOINT, class D>
int prednet_check_dims(const D* d, const char* who, int layers_rc) {
  bool ok = d->Hp >= 4 && d->Hp % 4 == 0;
  if constexpr (JOINT) ok = ok && d->O >= 4 && d->O % 4 == 0;
  RNNT_CHECK_ARG(ok, "%s: bad dims (hidden and output sizes must be multiples of 4)", who);
  if (d->L < 1 || d->L > DEC_MAX_LAYERS) {
    set_error("%s: %d prediction-net layers (RNNT_DECODE_MAX_LAYERS = %d)", who, d->L, DEC_MAX_LAYERS);
    return layers_rc;
  }
  RNNT_CHECK_ARG(d->cell >= RNNT_CELL_LSTM && d->cell <= RNNT_CELL_RNN_RELU, "%s: unknown cell type", who);
  return RNNT_OK;
}

// Null, alignment and per-layer weight checks of a descriptor's prediction net, and its copy into k.  After
// prednet_check_dims (d->L indexes the weight arrays).
template <bool JOINT, class D>
int fill_prednet(const D* d, PredNet& k, const char* who) {
  RNNT_CHECK_ARG(d->emb, "%s: null pointer", who);
  k.Hp = d->Hp; k.L = d->L; k.cell = d->cell; k.emb = d->emb;
  if constexpr (JOINT) {
    RNNT_CHECK_ARG(d->w_o && d->b_o && d->w_d, "%s: null pointer", who);
    RNNT_CHECK_ARG(d->ld_d % 4 == 0 && (reinterpret_cast<uintptr_t>(d->w_d) & 15) == 0, "%s: fc slice must be 16-byte aligned", who);
    k.V = d->V; k.O = d->O; k.blank = d->blank; k.w_o = d->w_o; k.b_o = d->b_o; k.w_d = d->w_d; k.ld_d = d->ld_d;
  } else {
    k.V = 0; k.O = 0; k.blank = 0; k.w_o = k.b_o = k.w_d = nullptr; k.ld_d = 0;
  }
  for (int l = 0; l < d->L; ++l) {   // last, as every entry always had it: after the other pointers and the alignment
    RNNT_CHECK_ARG(d->w_ih[l] && d->w_hh[l] && d->b_ih[l] && d->b_hh[l], "%s: null weight (layer %d)", who, l);
    k.w_ih[l] = d->w_ih[l]; k.w_hh[l] = d->w_hh[l]; k.b_ih[l] = d->b_ih[l]; k.b_hh[l] = d->b_hh[l];
  }
  return RNNT_OK;
}

// y[r] = dot(W[r, :cols], x) (+ bias[r]) for r in [0, rows): one wave per group of RU rows (lanes along the contiguous k),
// 16 waves per pass.  All RU rows' loads are issued before any is consumed: a single row per wave keeps only 2 KB in
// flight per wave and the step becomes latency-bound (measured 308 us per prediction-net step at H=512).
constexpr int RU = 8;
__device__ __forceinline__ void matvec(const float* __restrict__ W, long ld, int rows, int cols, const float* __restrict__ x,
                                       float* __restrict__ y, const float* __restrict__ bias) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = DEC_THREADS / 64;
  for (int r0 = wave * RU; r0 < rows; r0 += nw * RU) {
    float s[RU];
#pragma unroll
    for (int i = 0; i < RU; ++i) s[i] = 0.f;
    for (int k = 4 * lane; k < cols; k += 256) {
      f32x4 w[RU];
#pragma unroll
      for (int i = 0; i < RU; ++i) {
        const int r = r0 + i < rows ? r0 + i : rows - 1;  // clamp: tail rows re-read the last row, result discarded
        w[i] = *reinterpret_cast<const f32x4*>(W + (long)r * ld + k);
      }
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + k);
      // One explicit fma chain per row: the rounding of a row's sum must not depend on which of the RU slots the row sits in.
      // Written as `s += w0 x0 + w1 x1 + w2 x2 + w3 x3` the compiler contracts some slots into fma chains and packs the products
      // of others in pairs (two rounded multiplies), so two rows with equal weights could differ in the last bit and a tie of
      // the frame argmax went to the higher index (tests/test_gpu_search_shapes.py, the tie cases).
#pragma unroll
      for (int i = 0; i < RU; ++i) {
        float a = s[i];
        a = __builtin_fmaf(w[i][0], xv[0], a);
        a = __builtin_fmaf(w[i][1], xv[1], a);
        a = __builtin_fmaf(w[i][2], xv[2], a);
        a = __builtin_fmaf(w[i][3], xv[3], a);
        s[i] = a;
      }
    }
#pragma unroll
    for (int i = 0; i < RU; ++i) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
    }
    if (lane < RU && r0 + lane < rows) {
      float v = s[0];
#pragma unroll
      for (int i = 1; i < RU; ++i) v = lane == i ? s[i] : v;
      y[r0 + lane] = v + (bias ? bias[r0 + lane] : 0.f);
    }
  }
}

__host__ __device__ __forceinline__ int cell_gates(int cell) { return cell == RNNT_CELL_LSTM ? 4 : (cell == RNNT_CELL_GRU ? 3 : 1); }

// floats of a stored prediction-net state: h[L*Hp] | c[L*Hp] (LSTM) | C[V], padded to 4
inline int slot_floats(int L, int Hp, int cell, int V) { return (L * Hp * (cell == RNNT_CELL_LSTM ? 2 : 1) + V + 3) & ~3; }

// The L stacked cells of one step (torch.nn.LSTM / GRU / RNN equations), in place on LDS state h[L][Hp], c[L][Hp].  On entry
// x[0:Hp] holds the layer-0 input (the token's embedding row); gi / gh are 4*Hp scratch each.  gi0, if not null, is the
// precomputed layer-0 input projection W_ih0 x + b_ih0 of this token (same matvec, so the same bits): x is then not read.
// P provides Hp, L, cell, w_ih[], w_hh[], b_ih[], b_hh[].  Ends with a barrier; the last layer's output is h[(L-1)*Hp:].
template <class P>
__device__ __forceinline__ void prednet_cells(const P& p, float* h, float* c, float* gi, float* gh, float* x, const float* gi0) {
  const int Hp = p.Hp, tid = threadIdx.x, NG = cell_gates(p.cell);
  for (int l = 0; l < p.L; ++l) {
    if (l == 0 && gi0) {
      for (int i = tid; i < NG * Hp; i += DEC_THREADS) gi[i] = gi0[i];
    } else {
      matvec(p.w_ih[l], Hp, NG * Hp, Hp, x, gi, p.b_ih[l]);
    }
    matvec(p.w_hh[l], Hp, NG * Hp, Hp, h + l * Hp, gh, p.b_hh[l]);
    __syncthreads();
    for (int j = tid; j < Hp; j += DEC_THREADS) {
      float hv;
      if (p.cell == RNNT_CELL_LSTM) {
        const float ig = sigmoidf_(gi[j] + gh[j]), fg = sigmoidf_(gi[Hp + j] + gh[Hp + j]);
        const float gg = tanhf(gi[2 * Hp + j] + gh[2 * Hp + j]), og = sigmoidf_(gi[3 * Hp + j] + gh[3 * Hp + j]);
        const float cv = fg * c[l * Hp + j] + ig * gg;
        c[l * Hp + j] = cv;
        hv = og * tanhf(cv);
      } else if (p.cell == RNNT_CELL_GRU) {
        const float rg = sigmoidf_(gi[j] + gh[j]), zg = sigmoidf_(gi[Hp + j] + gh[Hp + j]);
        const float ng = tanhf(gi[2 * Hp + j] + rg * gh[2 * Hp + j]);
        hv = (1.f - zg) * ng + zg * h[l * Hp + j];
      } else {
        const float pre = gi[j] + gh[j];
        hv = p.cell == RNNT_CELL_RNN_RELU ? fmaxf(pre, 0.f) : tanhf(pre);
      }
      h[l * Hp + j] = hv;
      x[j] = hv;  // input of the next layer (no dropout at inference)
    }
    __syncthreads();
  }
}

// C = gelu(out_proj(h_last)) . W_d^T (the prediction-net half of the joint, networks/transducer.py:64-69).  P provides O, V,
// Hp, w_o, b_o, w_d, ld_d.  dec is O floats of LDS scratch.  Ends with a barrier.
template <class P>
__device__ __forceinline__ void prednet_joint_half(const P& p, const float* h_last, float* dec, float* Cv) {
  matvec(p.w_o, p.Hp, p.O, p.Hp, h_last, dec, p.b_o);
  __syncthreads();
  for (int i = threadIdx.x; i < p.O; i += DEC_THREADS) dec[i] = gelu_tanh(dec[i]);
  __syncthreads();
  matvec(p.w_d, p.ld_d, p.V, p.O, dec, Cv, nullptr);
  __syncthreads();
}

// log-softmax of one joint evaluation at the token the argmax chose: z[tok] - lse_v(z) with z[v] = a[v] + Cv[v], fp32.  tok is
// the argmax, so z[tok] is the maximum and lse = z[tok] + log(sum_v exp(z[v] - z[tok])): one V-wide reduction.  Its order is
// fixed by (tid, lane, wave) alone: a strided pass per thread, the wave butterfly (a + b == b + a: every lane holds the same
// sum), then the waves in order; nothing depends on B, T or a chunk boundary.  All threads call it; red is DEC_THREADS / 64
// floats of LDS nobody reads at the call; every thread returns the value.  Ends with a barrier.
__device__ __forceinline__ float token_logp(const float* __restrict__ a, const float* __restrict__ Cv, int V, int tok, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float zt = a[tok] + Cv[tok];
  float s = 0.f;
  for (int v = tid; v < V; v += DEC_THREADS) s += expf((a[v] + Cv[v]) - zt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < DEC_THREADS / 64; ++w) r += red[w];
  __syncthreads();
  return -logf(r);
}

// ---- greedy search ----------------------------------------------------------------------------------------------------
// Per utterance, for t in 0..Tb-1: up to `max_iters` times { tok = argmax_v (A[t] + C); if tok == blank: stop this frame;
// append tok unless it equals the last appended token; advance the prediction net with tok }.  The offline search
// (decode.hip) starts from the primed state; the streaming search (stream.hip) from the state the last chunk left.
struct GreedyK : PredNet {
  int T, B, max_iters, max_out;
  const float* A;      // (T,B,V) time-major, bias included
  const int* lens;     // (B) frames to visit per utterance; offline: or null (= T)
  const int* rows;     // prime: the rows to (re)initialise
  float* h;            // carried state, null offline: (L,B,Hp)
  float* c;            //   (L,B,Hp) LSTM only
  float* Cs;           //   (B,V) joint half of the current state
  long long* last;     //   (B) last appended token
  long long* tokens;   // (B,max_out)
  int* ntok;           // (B)
  int* frames;         // (B,max_out) frame of each appended token, or null (the untimed entries)
  float* logp;         // (B,max_out) log-softmax of the joint at the appended token; with frames
  const long long* frame_base;  // streaming: (B) frames the stream consumed before this chunk, or null (0)
};

// dynamic LDS of the greedy kernels: h[L][Hp] | c[L][Hp] | gi[4Hp] | gh[4Hp] | x[Hp] | dec[O] | Cv[V] | redv[16] redi[16] | ctl[8]
struct GreedyLds {
  float *h, *c, *gi, *gh, *x, *dec, *Cv, *redv;
  int *redi, *ctl;  // ctl[0] = token chosen this evaluation
  __device__ GreedyLds(char* smem, int L, int Hp, int O, int V) {
    h = reinterpret_cast<float*>(smem);
    c = h + L * Hp;
    gi = c + L * Hp;
    gh = gi + 4 * Hp;
    x = gh + 4 * Hp;
    dec = x + Hp;
    Cv = dec + O;
    redv = Cv + V;
    redi = reinterpret_cast<int*>(redv + 16);
    ctl = redi + 16;
  }
};
inline size_t greedy_lds_bytes(int L, int Hp, int O, int V) {
  return ((size_t)2 * L * Hp + 8 * Hp + Hp + O + V + 32 + 8) * 4;
}

// frame number reported for a chunk's frame 0: what the stream consumed before (timed streaming entry), else 0
__device__ __forceinline__ int greedy_frame_base(const GreedyK& p, int b) {
  return p.frames && p.frame_base ? (int)p.frame_base[b] : 0;   // frames are int32: reset before 2^31 frames
}

// one prediction-net step with input token `tok`, then C = gelu(out_proj(h_last)) . W_d^T
__device__ __forceinline__ void prednet_step_lds(const GreedyK& p, GreedyLds& s, int tok) {
  for (int i = threadIdx.x; i < p.Hp; i += DEC_THREADS) s.x[i] = p.emb[(long)tok * p.Hp + i];
  __syncthreads();
  prednet_cells(p, s.h, s.c, s.gi, s.gh, s.x, nullptr);
  prednet_joint_half(p, s.h + (p.L - 1) * p.Hp, s.dec, s.Cv);
}

// tok = argmax_v (a[v] + Cv[v]); lowest index among equal maxima (torch.argmax on a 1-D tensor).  Every thread returns it.
__device__ __forceinline__ int frame_argmax(const float* a, const float* Cv, int V, GreedyLds& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float best = -__builtin_huge_valf();
  int bi = 0x7fffffff;
  for (int v = tid; v < V; v += DEC_THREADS) {
    const float z = a[v] + Cv[v];
    if (z > best || (z == best && v < bi)) { best = z; bi = v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) { s.redv[wave] = best; s.redi[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < DEC_THREADS / 64; ++w)
      if (s.redv[w] > best || (s.redv[w] == best && s.redi[w] < bi)) { best = s.redv[w]; bi = s.redi[w]; }
    s.ctl[0] = bi;
  }
  __syncthreads();
  const int tok = s.ctl[0];
  __syncthreads();
  return tok;
}

// The frame loop of utterance b over frames [0, Tb) of p.A, from the state in `s` (h, c, Cv), the last appended token `last`
// and n tokens appended so far; frame t is reported as t_base + t.  Leaves the state after the last step in `s`.
__device__ __forceinline__ void greedy_frames(const GreedyK& p, GreedyLds& s, int b, int Tb, int t_base, long long& last, int& n) {
  const int tid = threadIdx.x, V = p.V;
  for (int t = 0; t < Tb; ++t) {
    for (int u = 0; u < p.max_iters; ++u) {
      const float* a = p.A + ((long)t * p.B + b) * V;
      const int tok = frame_argmax(a, s.Cv, V, s);
      if (tok == p.blank) break;
      if (last != tok) {
        if (p.frames && n < p.max_out) {  // timed entries: one more V-wide reduction per appended token
          const float lp = token_logp(a, s.Cv, V, tok, s.redv);
          if (tid == 0) {
            p.frames[(long)b * p.max_out + n] = t_base + t;
            p.logp[(long)b * p.max_out + n] = lp;
          }
        }
        if (n < p.max_out && tid == 0) p.tokens[(long)b * p.max_out + n] = tok;
        ++n;
        last = tok;
      }
      prednet_step_lds(p, s, tok);
    }
  }
}

}  // namespace rnnt
