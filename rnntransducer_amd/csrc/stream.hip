// Streaming greedy recognition: features arrive in chunks, per-stream encoder / prediction-net / greedy state carries from
// one chunk to the next (model.py:12-18 of the reference: "continuously processes input samples and streams output symbols";
// a unidirectional encoder, networks/encoder.py:62, and the single-step prediction-net branch, networks/decoder.py:121-123).
//
// Three pieces, every one of them with a per-element arithmetic that depends neither on the chunk length T nor on where the
// chunk boundaries fall nor on the number of streams B, so that any chunking of an utterance gives the same bits:
//
//  1. stream_rnn_step_kernel: one wavefront step of the stacked recurrence.  Launch k runs layer l at frame k - l for every
//     l (T + L - 1 launches per chunk); a workgroup owns SR_UNITS hidden units (all gates of them) of one layer for all B
//     streams, stages only its rows of W_ih / W_hh in LDS and writes its units of h_t into a two-slot ring (slot t & 1), so
//     no workgroup ever waits on another inside a launch.  A gate pre-activation is a dot product in a fixed order: lane i
//     of a wave accumulates k = i, i + 64, ... with fmaf, then a fixed butterfly adds the 64 lane partials.
//  2. stream_gemm_kernel: out_proj of the top layer and the encoder half of the joint, A = gelu(enc) W_e^T + bias.  Every
//     output element is one k-ordered fmaf chain from k = 0 (the tiling only decides which thread runs it), bias added last.
//  3. stream_greedy_kernel: the greedy search continued from carried state (prediction-net h / c, the joint half C of that
//     state, the last appended token) instead of priming; stream_prime_kernel primes listed rows as transducer.py:116-119
//     does (zero state, one blank step).  The search loop is greedy_frames of decode_shared.hpp, the one the offline
//     kernel (decode.hip) runs, on the same parameter struct and LDS carve-up: this file only loads and stores the state
//     around it.
#include "decode_shared.hpp"

namespace rnnt {
namespace {

constexpr int SR_THREADS = 256;   // 4 waves
constexpr int SR_WAVES = SR_THREADS / 64;
constexpr int SR_UNITS = 4;       // hidden units per workgroup
constexpr int SR_SLOTS = 64;      // accumulators per lane in one pass: (stream, gate row) pairs, one per lane after the butterfly
constexpr size_t SR_MAX_LDS = 160 * 1024;

struct StreamRnnK {
  int T, B, F, H, L, cell, k, l_lo;
  const float* x;
  long long x_sb, x_st;
  const int* lens;
  const float* w_ih[RNNT_STREAM_MAX_LAYERS];
  const float* w_hh[RNNT_STREAM_MAX_LAYERS];
  const float* b_ih[RNNT_STREAM_MAX_LAYERS];
  const float* b_hh[RNNT_STREAM_MAX_LAYERS];
  float* ring;       // (L,2,B,H): slot t & 1 holds layer l's h after frame t
  const float* h0;   // (L,B,H) state before the chunk
  float* c;          // (L,B,H) LSTM cell state, updated in place (each unit has one owner); null otherwise
  float* y;          // (T,B,H) top layer's h per frame
};

// v[0..63] per lane -> lane i holds slot i summed over the 64 lanes.  The same tree for every slot: at offset o the lanes
// differing in bit o add their partials (a + b == b + a in IEEE arithmetic, so the result does not depend on which lane adds).
// Compile-time offsets so that v stays in registers.
template <int O>
__device__ __forceinline__ void reduce_scatter_step(float (&v)[SR_SLOTS], int lane) {
  const bool hi = (lane & O) != 0;
#pragma unroll
  for (int i = 0; i < O; ++i) {
    const float send = hi ? v[i] : v[i + O];
    const float keep = hi ? v[i + O] : v[i];
    v[i] = keep + __shfl_xor(send, O);
  }
  if constexpr (O > 1) reduce_scatter_step<O / 2>(v, lane);
}

__device__ __forceinline__ float reduce_scatter64(float (&v)[SR_SLOTS]) {
  reduce_scatter_step<SR_SLOTS / 2>(v, threadIdx.x & 63);
  return v[0];
}

// acc[s * R + r] = sum_k Ws[r * K + k] * X(b0 + s)[k]; returns this lane's slot after the butterfly.  Streams past B re-read
// stream B - 1 (their slots are discarded).
template <int R, int NB>
__device__ __forceinline__ float gate_dots(const float* Ws, int K, const float* base, long long sb, int b0, int B) {
  const int lane = threadIdx.x & 63;
  float acc[SR_SLOTS];
#pragma unroll
  for (int i = 0; i < SR_SLOTS; ++i) acc[i] = 0.f;
  const float* xs[NB];
#pragma unroll
  for (int s = 0; s < NB; ++s) xs[s] = base + (long long)(b0 + s < B ? b0 + s : B - 1) * sb;
  for (int kk = lane; kk < K; kk += 64) {
    float xv[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) xv[s] = xs[s][kk];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float w = Ws[r * K + kk];
#pragma unroll
      for (int s = 0; s < NB; ++s) acc[s * R + r] = __builtin_fmaf(w, xv[s], acc[s * R + r]);
    }
  }
  return reduce_scatter64(acc);
}

// rows r = g * SR_UNITS + j of a workgroup's slice <-> global gate row g * H + u0 + j (torch's gate-major layout)
__device__ __forceinline__ void stage_rows(float* dst, const float* W, int R, int K, int H, int u0) {
  if ((K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
    const int K4 = K >> 2;
    for (int i = threadIdx.x; i < R * K4; i += SR_THREADS) {
      const int r = i / K4, q = i - r * K4;
      const long grow = (long)(r / SR_UNITS) * H + u0 + r % SR_UNITS;
      reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(W + grow * K)[q];
    }
  } else {
    for (int i = threadIdx.x; i < R * K; i += SR_THREADS) {
      const int r = i / K, q = i - r * K;
      dst[i] = W[((long)(r / SR_UNITS) * H + u0 + r % SR_UNITS) * K + q];
    }
  }
}

template <int G>
__global__ void __launch_bounds__(SR_THREADS) stream_rnn_step_kernel(const StreamRnnK p) {
  constexpr int R = G * SR_UNITS;
  constexpr int NB = SR_SLOTS / R;   // streams per pass: 4 (LSTM), 5 (GRU), 16 (RNN)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int l = p.l_lo + blockIdx.y, t = p.k - l, u0 = blockIdx.x * SR_UNITS;
  const int H = p.H, B = p.B, K_in = l == 0 ? p.F : H;
  float* Wi = reinterpret_cast<float*>(smem);
  float* Wh = Wi + R * K_in;
  stage_rows(Wi, p.w_ih[l], R, K_in, H, u0);
  stage_rows(Wh, p.w_hh[l], R, H, H, u0);
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long BH = (long long)B * H;
  float* out_slot = p.ring + (2 * l + (t & 1)) * BH;
  const float* hprev = t == 0 ? p.h0 + l * BH : p.ring + (2 * l + ((t - 1) & 1)) * BH;
  const float* xin;
  long long xsb;
  if (l == 0) { xin = p.x + (long long)t * p.x_st; xsb = p.x_sb; }
  else { xin = p.ring + (2 * (l - 1) + (t & 1)) * BH; xsb = H; }
  // bias of this lane's slot (slot = s * R + r)
  const int rr = lane % R;
  const int grow = (rr / SR_UNITS) * H + u0 + rr % SR_UNITS;
  const float bi = lane < NB * R ? p.b_ih[l][grow] : 0.f, bh = lane < NB * R ? p.b_hh[l][grow] : 0.f;

  const int ngroups = (B + NB - 1) / NB;
  for (int gidx = wave; gidx < ngroups; gidx += SR_WAVES) {
    const int b0 = gidx * NB;
    const float vi = gate_dots<R, NB>(Wi, K_in, xin, xsb, b0, B) + bi;
    const float vh = gate_dots<R, NB>(Wh, H, hprev, H, b0, B) + bh;
    // lane q < NB * SR_UNITS finishes unit j = q % SR_UNITS of stream b0 + q / SR_UNITS; gather its gates (all lanes shuffle)
    const int s = lane / SR_UNITS, j = lane % SR_UNITS;
    float gi[G], gh[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int src = (s * R + g * SR_UNITS + j) & 63;
      gi[g] = __shfl(vi, src);
      gh[g] = __shfl(vh, src);
    }
    const int b = b0 + s;
    if (lane < NB * SR_UNITS && b < B) {
      const long long e = (long long)b * H + u0 + j;
      const float hp = hprev[e];
      float hv;
      if (t >= p.lens[b]) {
        hv = hp;   // past this stream's frames: carry the state unchanged
      } else if constexpr (G == 4) {   // torch.nn.LSTM: i, f, g, o
        const float ig = sigmoidf_(gi[0] + gh[0]), fg = sigmoidf_(gi[1] + gh[1]);
        const float gg = tanhf(gi[2] + gh[2]), og = sigmoidf_(gi[3] + gh[3]);
        float* cp = p.c + l * BH + e;
        const float cv = fg * *cp + ig * gg;
        *cp = cv;
        hv = og * tanhf(cv);
      } else if constexpr (G == 3) {   // torch.nn.GRU: r, z, n
        const float rg = sigmoidf_(gi[0] + gh[0]), zg = sigmoidf_(gi[1] + gh[1]);
        const float ng = tanhf(gi[2] + rg * gh[2]);
        hv = (1.f - zg) * ng + zg * hp;
      } else {
        const float pre = gi[0] + gh[0];
        hv = p.cell == RNNT_CELL_RNN_RELU ? fmaxf(pre, 0.f) : tanhf(pre);
      }
      out_slot[e] = hv;
      if (l == p.L - 1) p.y[(long long)t * BH + e] = hv;
    }
  }
}

// h_state[l] = ring[l][(T - 1) & 1] (the carried rows hold their old state there)
__global__ void __launch_bounds__(SR_THREADS) stream_state_out_kernel(const float* ring, float* h, int L, long long BH, int T) {
  const long long n = (long long)L * BH;
  for (long long i = (long long)blockIdx.x * SR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SR_THREADS) {
    const long long l = i / BH, e = i - l * BH;
    h[i] = ring[(2 * l + ((T - 1) & 1)) * BH + e];
  }
}

// C[m, n] = sum_k act(A[m, k]) W[n, k] + bias[n] for row m = t * Bdiv + b, zero where t >= lens[b].  64 x 64 tile per
// workgroup, 4 x 4 elements per thread, each one k-ordered fmaf chain.
constexpr int SG_TILE = 64, SG_KT = 16;
struct StreamGemmK {
  int M, N, K, Bdiv, gelu_a;
  const float* A;
  long long a_sb, a_st;
  const float* W;
  long long ldw;
  const float* bias;
  const int* lens;
  float* C;
  long long c_sb, c_st;
};

__global__ void __launch_bounds__(SR_THREADS) stream_gemm_kernel(const StreamGemmK p) {
  __shared__ float As[SG_KT][SG_TILE + 1];
  __shared__ float Ws[SG_KT][SG_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.x * SG_TILE, n0 = blockIdx.y * SG_TILE;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < p.K; k0 += SG_KT) {
#pragma unroll
    for (int q = 0; q < SG_TILE * SG_KT / SR_THREADS; ++q) {
      const int e = tid + q * SR_THREADS, r = e / SG_KT, kk = e % SG_KT, k = k0 + kk;
      const int m = m0 + r, n = n0 + r;
      float a = 0.f, w = 0.f;
      if (m < p.M && k < p.K) {
        const int t = m / p.Bdiv, b = m - t * p.Bdiv;
        a = p.A[b * p.a_sb + t * p.a_st + k];
        if (p.gelu_a) a = gelu_tanh(a);
      }
      if (n < p.N && k < p.K) w = p.W[n * p.ldw + k];
      As[kk][r] = a;
      Ws[kk][r] = w;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SG_KT; ++kk) {
      float a[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = As[kk][ty + 16 * i]; w[i] = Ws[kk][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(a[i], w[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 16 * i;
    if (m >= p.M) continue;
    const int t = m / p.Bdiv, b = m - t * p.Bdiv;
    const bool valid = !p.lens || t < p.lens[b];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx + 16 * j;
      if (n < p.N) p.C[b * p.c_sb + t * p.c_st + n] = valid ? acc[i][j] + (p.bias ? p.bias[n] : 0.f) : 0.f;
    }
  }
}

__device__ __forceinline__ void state_out(const GreedyK& p, const GreedyLds& s, int b) {
  const int Hp = p.Hp;
  for (int i = threadIdx.x; i < p.L * Hp; i += DEC_THREADS) {
    const int l = i / Hp, j = i - l * Hp;
    p.h[((long)l * p.B + b) * Hp + j] = s.h[i];
    if (p.cell == RNNT_CELL_LSTM) p.c[((long)l * p.B + b) * Hp + j] = s.c[i];
  }
  for (int v = threadIdx.x; v < p.V; v += DEC_THREADS) p.Cs[(long)b * p.V + v] = s.Cv[v];
}

// rows[blockIdx.x]: zero state, one prediction-net step on blank (transducer.py:116-119), last token = blank
__global__ void __launch_bounds__(DEC_THREADS) stream_prime_kernel(const GreedyK p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GreedyLds s(smem, p.L, p.Hp, p.O, p.V);
  const int b = p.rows[blockIdx.x];
  for (int i = threadIdx.x; i < 2 * p.L * p.Hp; i += DEC_THREADS) s.h[i] = 0.f;
  __syncthreads();
  prednet_step_lds(p, s, p.blank);
  state_out(p, s, b);
  if (threadIdx.x == 0) p.last[b] = p.blank;
}

// continues the search of decode_shared.hpp from the carried state over this chunk's frames
__global__ void __launch_bounds__(DEC_THREADS) stream_greedy_kernel(const GreedyK p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GreedyLds s(smem, p.L, p.Hp, p.O, p.V);
  const int tid = threadIdx.x, b = blockIdx.x, Hp = p.Hp, V = p.V;
  int Tb = p.lens[b];
  Tb = Tb < 0 ? 0 : (Tb > p.T ? p.T : Tb);
  if (Tb == 0) {   // no frames: the state stays bitwise as it is
    if (tid == 0) p.ntok[b] = 0;
    return;
  }
  for (int i = tid; i < p.L * Hp; i += DEC_THREADS) {
    const int l = i / Hp, j = i - l * Hp;
    s.h[i] = p.h[((long)l * p.B + b) * Hp + j];
    s.c[i] = p.cell == RNNT_CELL_LSTM ? p.c[((long)l * p.B + b) * Hp + j] : 0.f;
  }
  for (int v = tid; v < V; v += DEC_THREADS) s.Cv[v] = p.Cs[(long)b * V + v];
  __syncthreads();
  int n = 0;
  long long last = p.last[b];
  greedy_frames(p, s, b, Tb, greedy_frame_base(p, b), last, n);
  state_out(p, s, b);
  if (tid == 0) {
    p.last[b] = last;
    p.ntok[b] = n < p.max_out ? n : p.max_out;
  }
}

size_t rnn_lds_bytes(int G, int F, int H) { return (size_t)G * SR_UNITS * ((F > H ? F : H) + H) * sizeof(float); }

template <int G>
int launch_rnn_steps(const StreamRnnK& base, size_t lds, hipStream_t s) {
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)stream_rnn_step_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int k = 0; k < base.T + base.L - 1; ++k) {
    StreamRnnK p = base;
    p.k = k;
    p.l_lo = k - base.T + 1 > 0 ? k - base.T + 1 : 0;
    const int l_hi = k < base.L - 1 ? k : base.L - 1;
    hipLaunchKernelGGL(stream_rnn_step_kernel<G>, dim3(base.H / SR_UNITS, l_hi - p.l_lo + 1), dim3(SR_THREADS), lds, s, p);
    RNNT_CHECK_LAUNCH();
  }
  return RNNT_OK;
}

int launch_gemm(const StreamGemmK& p, hipStream_t s) {
  hipLaunchKernelGGL(stream_gemm_kernel, dim3((unsigned)ceil_div(p.M, SG_TILE), (unsigned)ceil_div(p.N, SG_TILE)), dim3(SR_THREADS), 0,
                     s, p);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// checks and copies what the reset and the chunk entries share; A, lens, the outputs and max_iters / max_out are the chunk's
int fill_greedy(const rnnt_stream_greedy_desc* d, GreedyK& k, const char* who) {
  RNNT_CHECK_ARG(d->B >= 1 && d->V >= 1, "%s: bad dims", who);
  int rc = prednet_check_dims<true>(d, who, RNNT_ERR_UNSUPPORTED);
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(d->blank >= 0 && d->blank < d->V, "%s: blank outside [0, V)", who);
  RNNT_CHECK_ARG(d->h && d->C && d->last && (d->c || d->cell != RNNT_CELL_LSTM), "%s: null pointer", who);
  if ((rc = fill_prednet<true>(d, k, who)) != RNNT_OK) return rc;
  const size_t lds = greedy_lds_bytes(d->L, d->Hp, d->O, d->V);
  if (lds > DEC_MAX_LDS) {
    set_error("%s: prediction-net state and joint row need %zu B of LDS (limit 160 KiB)", who, lds);
    return RNNT_ERR_UNSUPPORTED;
  }
  k.T = d->T; k.B = d->B; k.max_iters = d->max_iters; k.max_out = d->max_out;
  k.A = d->A; k.lens = d->lens; k.rows = nullptr;
  k.h = d->h; k.c = d->c; k.Cs = d->C; k.last = (long long*)d->last;
  k.tokens = (long long*)d->tokens; k.ntok = d->ntok;
  k.frames = nullptr; k.logp = nullptr; k.frame_base = nullptr;
  return RNNT_OK;
}

}  // namespace
}  // namespace rnnt

using namespace rnnt;

extern "C" size_t rnnt_hip_stream_rnn_workspace_bytes(const rnnt_stream_rnn_desc* d) {
  if (!d || d->T < 1 || d->B < 1 || d->H < 1 || d->L < 1) return 0;
  const size_t ring = (size_t)d->L * 2 * d->B * d->H, y = (size_t)d->T * d->B * d->H;
  return align_up(ring * 4, 256) + align_up(y * 4, 256);
}

extern "C" int rnnt_hip_stream_rnn_chunk(const rnnt_stream_rnn_desc* d, void* stream) {
  RNNT_CHECK_ARG(d != nullptr, "stream_rnn_chunk: null descriptor");
  RNNT_CHECK_ARG(d->T >= 1 && d->B >= 1 && d->F >= 1 && d->H >= 4 && d->O >= 1, "stream_rnn_chunk: bad dims");
  RNNT_CHECK_ARG(d->cell >= RNNT_CELL_LSTM && d->cell <= RNNT_CELL_RNN_RELU, "stream_rnn_chunk: unknown cell type");
  if (d->H % SR_UNITS != 0) {
    set_error("stream_rnn_chunk: hidden size %d is not a multiple of %d (units per workgroup)", d->H, SR_UNITS);
    return RNNT_ERR_UNSUPPORTED;
  }
  if (d->L < 1 || d->L > RNNT_STREAM_MAX_LAYERS) {
    set_error("stream_rnn_chunk: %d layers (RNNT_STREAM_MAX_LAYERS = %d)", d->L, RNNT_STREAM_MAX_LAYERS);
    return RNNT_ERR_UNSUPPORTED;
  }
  const int G = d->cell == RNNT_CELL_LSTM ? 4 : (d->cell == RNNT_CELL_GRU ? 3 : 1);
  const size_t lds = rnn_lds_bytes(G, d->F, d->H);
  if (lds > SR_MAX_LDS) {
    set_error("stream_rnn_chunk: a workgroup's weight rows need %zu B of LDS (limit 160 KiB: %d gates x %d units x (max(F, H) + H) floats)",
              lds, G, SR_UNITS);
    return RNNT_ERR_UNSUPPORTED;
  }
  RNNT_CHECK_ARG(d->x && d->lens && d->h && d->w_o && d->out && (d->c || d->cell != RNNT_CELL_LSTM), "stream_rnn_chunk: null pointer");
  RNNT_CHECK_ARG(d->workspace && d->workspace_bytes >= rnnt_hip_stream_rnn_workspace_bytes(d) &&
                     (reinterpret_cast<uintptr_t>(d->workspace) & 255) == 0,
                 "stream_rnn_chunk: workspace needs %zu bytes, 256-byte aligned", rnnt_hip_stream_rnn_workspace_bytes(d));
  RNNT_CHECK_ARG(!d->A || (d->fc_w && d->fc_b && d->V >= 1 && d->ld_fc >= d->O), "stream_rnn_chunk: joint half needs fc_w, fc_b, V");
  StreamRnnK k;
  k.T = d->T; k.B = d->B; k.F = d->F; k.H = d->H; k.L = d->L; k.cell = d->cell; k.k = 0; k.l_lo = 0;
  k.x = d->x; k.x_sb = d->x_sb; k.x_st = d->x_st; k.lens = d->lens;
  for (int l = 0; l < d->L; ++l) {
    RNNT_CHECK_ARG(d->w_ih[l] && d->w_hh[l] && d->b_ih[l] && d->b_hh[l], "stream_rnn_chunk: null weight (layer %d)", l);
    k.w_ih[l] = d->w_ih[l]; k.w_hh[l] = d->w_hh[l]; k.b_ih[l] = d->b_ih[l]; k.b_hh[l] = d->b_hh[l];
  }
  char* ws = static_cast<char*>(d->workspace);
  const size_t BH = (size_t)d->B * d->H;
  k.ring = reinterpret_cast<float*>(ws);
  k.y = reinterpret_cast<float*>(ws + align_up((size_t)d->L * 2 * BH * 4, 256));
  k.h0 = d->h; k.c = d->c;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)G * d->H * (d->F + (2.0 * d->L - 1) * d->H) * d->T * d->B, s);
  int rc = G == 4 ? launch_rnn_steps<4>(k, lds, s) : (G == 3 ? launch_rnn_steps<3>(k, lds, s) : launch_rnn_steps<1>(k, lds, s));
  if (rc != RNNT_OK) return rc;
  const long long n = (long long)d->L * BH;
  hipLaunchKernelGGL(stream_state_out_kernel, dim3((unsigned)(ceil_div(n, SR_THREADS) < 2048 ? ceil_div(n, SR_THREADS) : 2048)),
                     dim3(SR_THREADS), 0, s, (const float*)k.ring, d->h, d->L, (long long)BH, d->T);
  RNNT_CHECK_LAUNCH();
  // out_proj of the top layer: to the caller's layout, and to a time-major copy for the joint half
  StreamGemmK g;
  g.M = d->T * d->B; g.N = d->O; g.K = d->H; g.Bdiv = d->B; g.gelu_a = 0;
  g.A = k.y; g.a_sb = d->H; g.a_st = (long long)BH; g.W = d->w_o; g.ldw = d->H; g.bias = d->b_o; g.lens = d->lens;
  g.C = d->out; g.c_sb = d->out_sb; g.c_st = d->out_st;
  if ((rc = launch_gemm(g, s)) != RNNT_OK) return rc;
  if (d->A) {
    StreamGemmK a;
    a.M = d->T * d->B; a.N = d->V; a.K = d->O; a.Bdiv = d->B; a.gelu_a = 1;
    a.A = d->out; a.a_sb = d->out_sb; a.a_st = d->out_st; a.W = d->fc_w; a.ldw = d->ld_fc; a.bias = d->fc_b; a.lens = nullptr;
    a.C = d->A; a.c_sb = d->V; a.c_st = (long long)d->B * d->V;
    if ((rc = launch_gemm(a, s)) != RNNT_OK) return rc;
  }
  return RNNT_OK;
}

extern "C" int rnnt_hip_stream_greedy_reset(const rnnt_stream_greedy_desc* d, const int32_t* rows, int32_t n_rows, void* stream) {
  RNNT_CHECK_ARG(d != nullptr, "stream_greedy_reset: null descriptor");
  GreedyK k;
  const int rc = fill_greedy(d, k, "stream_greedy_reset");
  if (rc != RNNT_OK) return rc;
  RNNT_CHECK_ARG(n_rows >= 0 && (rows || n_rows == 0), "stream_greedy_reset: bad row list");
  if (n_rows == 0) return RNNT_OK;
  k.rows = rows;
  const size_t lds = greedy_lds_bytes(d->L, d->Hp, d->O, d->V);
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)stream_prime_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)n_rows * d->V, (hipStream_t)stream);
  hipLaunchKernelGGL(stream_prime_kernel, dim3(n_rows), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

// both entries: `timing` null = the untimed search (the kernel's frames pointer is null, nothing else differs)
static int stream_greedy_launch(const rnnt_stream_greedy_desc* d, const rnnt_greedy_timing* timing, void* stream) {
  RNNT_CHECK_ARG(d != nullptr, "stream_greedy: null descriptor");
  GreedyK k;
  const int rc = fill_greedy(d, k, "stream_greedy");
  if (rc != RNNT_OK) return rc;
  if (timing) { k.frames = timing->frames; k.logp = timing->logp; k.frame_base = (const long long*)timing->frame_base; }
  RNNT_CHECK_ARG(d->T >= 1 && d->max_iters >= 1 && d->max_out >= 1, "stream_greedy: bad T / max_iters / max_out");
  RNNT_CHECK_ARG(d->A && d->lens && d->tokens && d->ntok, "stream_greedy: null pointer");
  const size_t lds = greedy_lds_bytes(d->L, d->Hp, d->O, d->V);
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)stream_greedy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope prof(RNNT_K_MISC, 4.0 * (double)d->T * d->B * d->V, (hipStream_t)stream);
  hipLaunchKernelGGL(stream_greedy_kernel, dim3(d->B), dim3(DEC_THREADS), lds, (hipStream_t)stream, k);
  RNNT_CHECK_LAUNCH();
  return RNNT_OK;
}

extern "C" int rnnt_hip_stream_greedy(const rnnt_stream_greedy_desc* d, void* stream) { return stream_greedy_launch(d, nullptr, stream); }

extern "C" int rnnt_hip_stream_greedy_timed(const rnnt_stream_greedy_desc* d, const rnnt_greedy_timing* timing, void* stream) {
  RNNT_CHECK_ARG(timing != nullptr && timing->frames && timing->logp, "stream_greedy_timed: null timing outputs (frames, logp)");
  return stream_greedy_launch(d, timing, stream);
}
