// Persistent, length-aware LSTM layer for gfx950: both directions of one layer in ONE launch.
//
// Replaces torch.nn.LSTM over a PackedSequence plus the sort/pack/unpack/unsort around it
// (networks/encoder.py:67-75,93-102; networks/decoder.py:71-79,105-120).
//
// Decomposition:
//   * the input projection X.W_ih^T + b_ih + b_hh for ALL timesteps is hoisted into one MFMA GEMM
//     (gemm.hip) that writes gate pre-activations time-major with the 4 gates of a hidden unit adjacent:
//     gates[t][b][d][4*j + g];
//   * the recurrence runs in one persistent kernel: direction d, hidden slice [j0, j0+Hs) per workgroup
//     (Hs = 4/8/16 units -> D*H/Hs workgroups, one per CU).  The workgroup keeps its 4*Hs rows of W_hh
//     in LDS for the whole sequence, its cell state in registers, and at every step
//       1. waits for the per-workgroup step flags of its direction (sc1 polls, bounded spin),
//       2. gathers h_{t-1} (B x H, write-through exchange buffer, sc1 16-B loads), split-K over the 4 waves,
//          v_mfma_f32_16x16x4_f32 (rows = gate rows, cols = batch),
//       3. reduces the 4 partial tiles through LDS, applies the gate non-linearities, masks t >= len[b],
//       4. writes activated gates (in place of the pre-activations), c_t, y_t and its slice of h_t
//          (sc1 16-B stores), drains, and publishes flag = step+1.
//   * backward mirrors it with dG (B x 4H) as the exchanged vector and v_mfma_f32_4x4x1_16B_f32
//     (16 k-blocks per instruction, so the 4-unit slice wastes no matrix lanes).
//   Packed-sequence semantics need no sort: a row is simply masked while t >= len[b]; its state stays 0,
//   so the reverse direction starts from zero at each sequence's own last frame and padded outputs are 0.
//
// Inter-workgroup protocol: MI355X_MICROARCH "Valid forms" row 1 — every exchanged byte is stored sc1 by
// its owner, every storing wave drains vmcnt(0), workgroup barrier, ONE lane publishes an sc1 flag; the
// consumer polls with sc1 loads from one wave, joins a workgroup barrier, then every wave reads the bytes
// with sc1 loads.  No dispatch-order or XCD-placement assumption; all spins are bounded (status word).
#include "lstm_shared.hpp"

#include <string.h>

namespace rnnt {
namespace {

// ------------------------------------------------------------------------------------------------
// forward recurrence
// dynamic LDS: Wl[4*Hs][LDW] | part[4][MT][NT][64] f32x4 | abort flag
// ------------------------------------------------------------------------------------------------
template <int MT, int NT>
__global__ void __launch_bounds__(256) lstm_fwd_kernel(const LstmK p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Wl = reinterpret_cast<float*>(smem);
  f32x4* part = reinterpret_cast<f32x4*>(Wl + 4 * p.Hs * p.LDW);
  int* abort_lds = reinterpret_cast<int*>(part + 4 * MT * NT * 64);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int d = blockIdx.x / p.NC, wg = blockIdx.x % p.NC;
  const int H = p.H, B = p.B, D = p.D, T = p.T, Bp = p.Bp, LDW = p.LDW;
  const int j0 = wg * p.Hs;
  const int R = 4 * p.Hs;

  // stage this workgroup's rows of W_hh: LDS row r = 4*ul + g  <->  torch row g*H + j0 + ul
  {
    const float* W = p.w_hh[d];
    for (int idx = tid; idx < R * LDW; idx += 256) {
      const int r = idx / LDW, k = idx % LDW;
      Wl[idx] = (k < H) ? W[(long)((r & 3) * H + j0 + (r >> 2)) * H + k] : 0.f;
    }
    if (tid == 0) *abort_lds = 0;
  }

  const long hx_floats = (long)(H / 4) * Bp * 4;
  __amdgpu_buffer_rsrc_t hx_rsrc[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    hx_rsrc[par] = __builtin_amdgcn_make_buffer_rsrc(p.hx + ((long)par * D + d) * hx_floats, 0, (int)(hx_floats * 4),
                                                     RSRC_FLAGS);
  unsigned* flags = p.flags + d * p.NC;

  // cell ownership: threads [0, MT*NT*64): tile (mt, nt), lane (n, q) -> unit 4*mt+q, batch 16*nt+n
  const bool owner = tid < MT * NT * 64;
  const int omt = owner ? (tid >> 6) / NT : 0, ont = owner ? (tid >> 6) % NT : 0;
  const int ob = 16 * ont + n, oj = j0 + 4 * omt + q;
  const int olen = (owner && ob < B) ? p.lens[ob] : 0;
  float c_state = 0.f;

  const int KG = (H + 15) / 16, KGW = (KG + 3) / 4;
  const int kg_begin = wave * KGW, kg_end = min(KG, kg_begin + KGW);
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    const int t = (d == 0) ? s : T - 1 - s;
    // (1) this cell's gate pre-activations (independent of the recurrence: issue first)
    f32x4 xp = {0.f, 0.f, 0.f, 0.f};
    const long grow = ((long)t * B + ob) * D + d;
    if (owner && ob < B) xp = *reinterpret_cast<const f32x4*>(p.gates + grow * 4 * H + 4 * oj);

    // (2) h_{t-1} . W_hh^T for this slice, split-K over the four waves
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      if (!wait_flags(flags, p.NC, (unsigned)s, p.status, abort_lds)) return;
      const __amdgpu_buffer_rsrc_t hr = hx_rsrc[(s - 1) & 1];
      for (int kg0 = kg_begin; kg0 < kg_end; kg0 += 8) {
        i32x4 hf[8][NT];
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          if (kg0 + g < kg_end) {
#pragma unroll
            for (int j = 0; j < NT; ++j)
              hf[g][j] = __builtin_amdgcn_raw_buffer_load_b128(hr, ((4 * (kg0 + g) + q) * Bp + 16 * j + n) * 16, 0, AUX_SC1);
          }
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          if (kg0 + g < kg_end) {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
              const f32x4 a = *reinterpret_cast<const f32x4*>(&Wl[(16 * i + n) * LDW + 16 * (kg0 + g) + 4 * q]);
#pragma unroll
              for (int j = 0; j < NT; ++j) {
                const f32x4 h = __builtin_bit_cast(f32x4, hf[g][j]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], h[e], acc[i][j], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    // (3) partial tiles -> LDS, reduce, gate math
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) part[((wave * MT + i) * NT + j) * 64 + lane] = acc[i][j];
    __syncthreads();
    if (owner) {
      f32x4 g4 = xp;
#pragma unroll
      for (int w = 0; w < 4; ++w) g4 += part[((w * MT + omt) * NT + ont) * 64 + lane];
      const bool active = t < olen;
      float hval = 0.f;
      f32x4 gact = {0.f, 0.f, 0.f, 0.f};
      if (active) {
        const float ig = sigmoidf_(g4[0]), fg = sigmoidf_(g4[1]), gg = tanhf(g4[2]), og = sigmoidf_(g4[3]);
        c_state = fg * c_state + ig * gg;
        hval = og * tanhf(c_state);
        gact = (f32x4){ig, fg, gg, og};
      } else {
        c_state = 0.f;
      }
      // gather the 4 units of this tile row-group into lanes q == 0 (same wave: lanes n, n+16, n+32, n+48)
      f32x4 h4, c4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h4[e] = __shfl(hval, n + 16 * e);
        c4[e] = __shfl(c_state, n + 16 * e);
      }
      if (q == 0) {  // exchange slice first: it is what the other workgroups wait for
        const int chunk = (j0 >> 2) + omt;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, h4), hx_rsrc[s & 1], (chunk * Bp + ob) * 16, 0, AUX_SC1);
      }
      if (ob < B) {
        *reinterpret_cast<f32x4*>(p.gates + grow * 4 * H + 4 * oj) = gact;
        if (q == 0) {
          const int chunk = (j0 >> 2) + omt;
          *reinterpret_cast<f32x4*>(p.cst + ((((long)d * T + t) * (H / 4) + chunk) * B + ob) * 4) = c4;
          const long yo = grow * H + j0 + 4 * omt;
          *reinterpret_cast<f32x4*>(p.y + yo) = h4;
          if (p.ydrop) {
            f32x4 hd;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              hd[e] = (hash_u32(p.seed, (unsigned long long)(yo + e)) >= p.drop_thresh) ? h4[e] * p.keep_scale : 0.f;
            *reinterpret_cast<f32x4*>(p.ydrop + yo) = hd;
          }
        }
      }
    }
    // (4) publish step s
    publish_flag(flags + wg, (unsigned)(s + 1));
  }
}


// ------------------------------------------------------------------------------------------------
// backward recurrence
//   dh_t = dy_t + dG_{t'} . W_hh   (t' = the step processed just before), contraction over all 4H gate rows
//   v_mfma_f32_4x4x1_16B_f32: block = one hidden unit j' of a 16-unit group, A rows = this slice's 4 units,
//   B cols = 4 batch rows, 4 instructions (one per gate) per (16-unit group, batch quad).
// dynamic LDS: WT[UG][MT][64] f32x4 | part[16][MT*BG*16] floats | abort flag
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dpp_ror_add(float x) {
  // sum over the 4 lanes of each 16-lane row that share lane%4 (row_ror:4, row_ror:8)
  int xi = __builtin_bit_cast(int, x);
  float y = x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(xi, xi, 0x124, 0xf, 0xf, false));
  int yi = __builtin_bit_cast(int, y);
  return y + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(yi, yi, 0x128, 0xf, 0xf, false));
}

template <int MT, int NT>
__global__ void __launch_bounds__(256) lstm_bwd_kernel(const LstmK p) {
  constexpr int BG = 4 * NT;  // batch quads
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, B = p.B, D = p.D, T = p.T, Bp = p.Bp;
  const int UG = (H + 15) / 16, UGW = (UG + 3) / 4;
  f32x4* WT = reinterpret_cast<f32x4*>(smem);
  float* part = reinterpret_cast<float*>(WT + UG * MT * 64);
  int* abort_lds = reinterpret_cast<int*>(part + 16 * MT * BG * 16);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = lane >> 2, l4 = lane & 3, row = lane >> 4;
  const int d = blockIdx.x / p.NC, wg = blockIdx.x % p.NC;
  const int j0 = wg * p.Hs;

  // stage W_hh columns of this slice: WT[ug][m][lane = 4*blk + i][e] = W_hh[e*H + 16*ug + blk][j0 + 4*m + i]
  {
    const float* W = p.w_hh[d];
    for (int idx = tid; idx < UG * MT * 64; idx += 256) {
      const int ln = idx & 63, m = (idx >> 6) % MT, ug = (idx >> 6) / MT;
      const int jp = 16 * ug + (ln >> 2), jj = j0 + 4 * m + (ln & 3);
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      if (jp < H) {
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = W[(long)(e * H + jp) * H + jj];
      }
      WT[idx] = w;
    }
    if (tid == 0) *abort_lds = 0;
  }

  const long gx_floats = (long)H * Bp * 4;
  __amdgpu_buffer_rsrc_t gx_rsrc[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    gx_rsrc[par] = __builtin_amdgcn_make_buffer_rsrc(p.hx + ((long)par * D + d) * gx_floats, 0, (int)(gx_floats * 4),
                                                     RSRC_FLAGS);
  unsigned* flags = p.flags + d * p.NC;

  // cell ownership: tid = ((m*BG + bg)*4 + i)*4 + jb  -> unit j0 + 4m + i, batch 4*bg + jb
  const bool owner = tid < MT * BG * 16;
  const int ojb = tid & 3, oi = (tid >> 2) & 3, obg = (tid >> 4) % BG, om = (tid >> 4) / BG;
  const int ob = 4 * obg + ojb, oj = j0 + 4 * om + oi;
  const int olen = (owner && ob < B) ? p.lens[ob] : 0;
  const int ochunk = oj >> 2;
  float dc_carry = 0.f;

  const int ug_begin = wave * UGW, ug_end = min(UG, ug_begin + UGW);
  __syncthreads();

  for (int s = 0; s < T; ++s) {
    const int t = (d == 0) ? T - 1 - s : s;
    const int tprev = (d == 0) ? t - 1 : t + 1;  // where c_{prev} of the forward recurrence lives
    // (1) prefetch this cell's stash (independent of the recurrence)
    f32x4 gt = {0.f, 0.f, 0.f, 0.f};
    float c_t = 0.f, c_p = 0.f, dyv = 0.f;
    const long grow = ((long)t * B + ob) * D + d;
    const bool active = owner && ob < B && t < olen;
    if (active) {
      gt = *reinterpret_cast<const f32x4*>(p.gates + grow * 4 * H + 4 * oj);
      c_t = p.cst[((((long)d * T + t) * (H / 4) + ochunk) * B + ob) * 4 + (oj & 3)];
      if (tprev >= 0 && tprev < T) c_p = p.cst[((((long)d * T + tprev) * (H / 4) + ochunk) * B + ob) * 4 + (oj & 3)];
      const long yo = grow * H + oj;
      dyv = p.dy[yo];
      if (p.ydrop) dyv = (hash_u32(p.seed, (unsigned long long)yo) >= p.drop_thresh) ? dyv * p.keep_scale : 0.f;
    }

    // (2) dG_{prev step} . W_hh[:, slice], split over unit groups (K) across the four waves
    f32x4 acc[MT][BG];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int g = 0; g < BG; ++g) acc[m][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      if (!wait_flags(flags, p.NC, (unsigned)s, p.status, abort_lds)) return;
      const __amdgpu_buffer_rsrc_t gr = gx_rsrc[(s - 1) & 1];
      for (int ug = ug_begin; ug < ug_end; ++ug) {
        i32x4 gf[BG];
#pragma unroll
        for (int g = 0; g < BG; ++g)
          gf[g] = __builtin_amdgcn_raw_buffer_load_b128(gr, ((16 * ug + blk) * Bp + 4 * g + l4) * 16, 0, AUX_SC1);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const f32x4 w = WT[(ug * MT + m) * 64 + lane];
#pragma unroll
          for (int g = 0; g < BG; ++g) {
            const f32x4 x = __builtin_bit_cast(f32x4, gf[g]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[m][g] = __builtin_amdgcn_mfma_f32_4x4x1f32(w[e], x[e], acc[m][g], 0, 0, 0);
          }
        }
      }
    }
    // (3) sum the 16 k-blocks: 4 lanes per row by DPP, then 4 rows x 4 waves through LDS
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int g = 0; g < BG; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = dpp_ror_add(acc[m][g][i]);
          if ((lane & 15) < 4) part[(wave * 4 + row) * (MT * BG * 16) + ((m * BG + g) * 4 + i) * 4 + l4] = v;
        }
    __syncthreads();
    if (owner) {
      float dh = dyv;
#pragma unroll
      for (int k = 0; k < 16; ++k) dh += part[k * (MT * BG * 16) + tid];
      f32x4 dg4 = {0.f, 0.f, 0.f, 0.f};
      if (active) {
        const float ig = gt[0], fg = gt[1], gg = gt[2], og = gt[3];
        const float tc = tanhf(c_t);
        const float dc = dh * og * (1.f - tc * tc) + dc_carry;
        dg4[0] = dc * gg * ig * (1.f - ig);
        dg4[1] = dc * c_p * fg * (1.f - fg);
        dg4[2] = dc * ig * (1.f - gg * gg);
        dg4[3] = dh * tc * og * (1.f - og);
        dc_carry = dc * fg;
      } else {
        dc_carry = 0.f;
      }
      // exchange first (what the other workgroups wait for), then the stash for the weight-gradient GEMMs
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, dg4), gx_rsrc[s & 1], (oj * Bp + ob) * 16, 0, AUX_SC1);
      if (ob < B) *reinterpret_cast<f32x4*>(p.gates + grow * 4 * H + 4 * oj) = dg4;
    }
    // (4) publish step s
    publish_flag(flags + wg, (unsigned)(s + 1));
  }
}


// ================================================================================================
// v2 recurrence: D*G sync groups (direction x batch slice) of NC workgroups; a workgroup owns HS hidden units.
// Measured (tools/sync_probe.hip, profiles/r01_sync_probe.txt): one flag+gather round costs 1.8-2.7 us in a
// 32-member group with a 16 KB payload vs 6.5-9.4 us in a 128..256-member group with 64 KB -- the cost scales with
// members and bytes, not with XCD placement.  So the batch is cut into G slices of Bg <= 16 rows; each group's
// exchange vector is Bg x H (fwd) / Bg x 4H (bwd) and only NC = H/HS workgroups wait on each other.
// Matrix cores: v_mfma_f32_4x4x1_16B_f32 -- 16 independent 4x4 outer products per instruction.  Blocks are
// (k-slice, row-quad): fwd rows = the 4 gates of one unit, bwd rows = 4 units; columns = 4 batch rows.  No lane is
// wasted on an 8-row batch slice, and a lane ends up holding exactly the values one cell update needs.
// ================================================================================================

// acc[bq] += sum_{s < Ls} A(ks, s) (x) B(row, ks, s) over this wave's K range.  A comes from LDS (WA_w[s/4][lane] f32x4),
// B is gathered from the group's exchange rows (global, sc1) in 4 KB blocks through a wave-private LDS stage so that
// one 16-B ds_read broadcasts a batch row's values to the 16 lanes that need them.
template <int KS, int BQ>
__device__ __forceinline__ void gather_mma(__amdgpu_buffer_rsrc_t src, int row_stride_f, int kbase, int Ls,
                                           const f32x4* __restrict__ WA_w, float* __restrict__ hs, int lane, int myks,
                                           f32x4 (&acc)[BQ]) {
  constexpr int NB = 4 * BQ;             // batch rows of the group (padded)
  constexpr int SB = 256 / (NB * KS);    // 4-step columns per staged block (256 float4 = 4 KB)
  constexpr int LDB = 4 * SB + (SB > 1 ? 4 : 0);
  const int ns4 = Ls >> 2;
  const int nblk = (ns4 + SB - 1) / SB;
  f32x4 acc2[2][BQ];
#pragma unroll
  for (int bq = 0; bq < BQ; ++bq) acc2[0][bq] = acc2[1][bq] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int blk0 = 0; blk0 < nblk; blk0 += 4) {
    i32x4 r[4][4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = lane + 64 * q;
        const int s4l = f % SB, ks = (f / SB) % KS, row = f / (SB * KS);
        const int s4 = (blk0 + bb) * SB + s4l;
        const bool ok = (blk0 + bb) < nblk && s4 < ns4;
        const int off = ok ? (row * row_stride_f + kbase + ks * Ls + 4 * s4) * 4 : 0x7ffffff0;  // out of range reads 0
        r[bb][q] = __builtin_amdgcn_raw_buffer_load_b128(src, off, 0, AUX_SC1);
      }
    }
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const int blk = blk0 + bb;
      if (blk < nblk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = lane + 64 * q;
          const int s4l = f % SB, ks = (f / SB) % KS, row = f / (SB * KS);
          *reinterpret_cast<i32x4*>(&hs[(row * KS + ks) * LDB + 4 * s4l]) = r[bb][q];
        }
        const int nsl = min(SB, ns4 - blk * SB);
        // software pipeline: chunks of U steps, register ping-pong, so the next chunk's LDS reads are in flight
        // under this chunk's MFMAs; two accumulator sets (even/odd step) keep dependent MFMAs 2*BQ apart
        constexpr int U = 4;
        const f32x4* wa = WA_w + (long)blk * SB * 64 + lane;
        const float* hb = hs + ((lane & 3) * KS + myks) * LDB;
        auto lds_load = [&](int s0, f32x4(&av)[U], f32x4(&bv)[U][BQ]) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            av[u] = wa[(s0 + u) * 64];
#pragma unroll
            for (int bq = 0; bq < BQ; ++bq) bv[u][bq] = *reinterpret_cast<const f32x4*>(&hb[4 * bq * KS * LDB + 4 * (s0 + u)]);
          }
        };
        auto mma = [&](const f32x4(&av)[U], const f32x4(&bv)[U][BQ]) {
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int bq = 0; bq < BQ; ++bq)
                acc2[u & 1][bq] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[u][e], bv[u][bq][e], acc2[u & 1][bq], 0, 0, 0);
        };
        const int nfull = nsl / U;
        if (nfull > 0) {
          f32x4 a0[U], b0[U][BQ], a1[U], b1[U][BQ];
          lds_load(0, a0, b0);
          int c = 0;
          for (; c + 2 <= nfull; c += 2) {
            lds_load((c + 1) * U, a1, b1);
            mma(a0, b0);
            if (c + 2 < nfull) lds_load((c + 2) * U, a0, b0);
            mma(a1, b1);
          }
          if (c < nfull) mma(a0, b0);
        }
        for (int s4l = nfull * U; s4l < nsl; ++s4l) {
          const f32x4 av = wa[s4l * 64];
#pragma unroll
          for (int bq = 0; bq < BQ; ++bq) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&hb[4 * bq * KS * LDB + 4 * s4l]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc2[0][bq] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[e], bv[e], acc2[0][bq], 0, 0, 0);
          }
        }
      }
    }
  }
#pragma unroll
  for (int bq = 0; bq < BQ; ++bq) acc[bq] += acc2[0][bq] + acc2[1][bq];
}

template <int KS, int BQ>
__host__ __device__ constexpr int stage_floats() {
  return 1024 + 4 * BQ * KS * 4;  // 4 KB block + per-(row, slice) padding
}

// dynamic LDS: WA[4][Ls/4][64] f32x4 | hs[4][stage_floats] | part[4][BQ][64] f32x4 | abort
// CELL: 0 LSTM (slots i,f,g,o), 1 GRU (slots r,z,n,-), 2 Elman RNN (slot 0; tanh or relu by p.cell).  Every cell type keeps
// the 4-slots-per-unit layout of the gate buffer and of the MFMA row-quads; unused slots carry zero weights.
template <int HS, int BQ, int CELL>
__global__ void __launch_bounds__(256) lstm_fwd2_kernel(const LstmK p) {
  constexpr int NGATE = CELL == 0 ? 4 : (CELL == 1 ? 3 : 1);
  constexpr int KS = 16 / HS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, B = p.B, D = p.D, T = p.T, Kp = p.Kp;
  const int Kw = Kp / 4, Ls = Kw / KS, ns4 = Ls / 4;
  f32x4* WA = reinterpret_cast<f32x4*>(smem);
  float* hs_all = reinterpret_cast<float*>(WA + 4 * ns4 * 64);
  f32x4* part = reinterpret_cast<f32x4*>(hs_all + 4 * stage_floats<KS, BQ>());
  int* abort_lds = reinterpret_cast<int*>(part + 4 * BQ * 64);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NG = D * p.G;
  // consecutive ids -> different groups; with a launch stride of 8 the XCD round-robin keeps every group on one XCD (speed only)
  const int gid = blockIdx.x % p.NGL, wg = blockIdx.x / p.NGL;
  if (gid >= NG) return;
  const int d = gid / p.G, g = gid % p.G;
  const int b0 = g * p.Bg, j0 = wg * HS;

  {  // weights: lane = 4*blk + i, blk = ks*HS + rq  <->  W_hh[(gate i)*H + j0 + rq][k], k = w*Kw + ks*Ls + 4*s4 + e
    const float* W = p.w_hh[d];
    for (int idx = tid; idx < 4 * ns4 * 64; idx += 256) {
      const int ln = idx & 63, s4 = (idx >> 6) % ns4, w = (idx >> 6) / ns4;
      const int i = ln & 3, blk = ln >> 2, rq = blk % HS, ks = blk / HS;
      const int k = w * Kw + ks * Ls + 4 * s4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < NGATE) {
        const float* row = W + (long)(i * H + j0 + rq) * H;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < H) v[e] = row[k + e];
      }
      WA[idx] = v;
    }
    if (tid == 0) *abort_lds = 0;
  }
  constexpr int NBR = 4 * BQ;
  const long hx_floats = (long)NBR * Kp;
  __amdgpu_buffer_rsrc_t hx_rsrc[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    hx_rsrc[par] = __builtin_amdgcn_make_buffer_rsrc(p.hx + ((long)par * NG + gid) * hx_floats, 0, (int)(hx_floats * 4), RSRC_FLAGS);
  unsigned* flags = p.flags + gid * p.NC;

  // cell owners: tid = obq*(4*HS) + 4*unit + j : the lane that ends up with the 4 gate sums of (unit, batch row 4*obq+j)
  const bool owner = tid < BQ * 4 * HS;
  const int ol = tid % (4 * HS), obq = tid / (4 * HS);
  const int ounit = ol >> 2, brow = 4 * obq + (ol & 3);
  const int ob = b0 + brow, oj = j0 + ounit;
  const bool valid = owner && brow < p.Bg && ob < B;
  const int olen = valid ? p.lens[ob] : 0;
  float c_state = 0.f;  // LSTM: cell state; GRU / RNN: previous hidden state of this cell
  const float bhn = (CELL == 1 && owner) ? p.b_hh[d][2 * H + oj] : 0.f;
  const int myks = (lane >> 2) / HS;
  // per-step addresses advance by constant strides: keep running offsets instead of 64-bit multiplies in the loop
  const int t_first = (d == 0) ? 0 : T - 1;
  const long tdir = (d == 0) ? 1 : -1;
  long g_off = (((long)t_first * B + ob) * D + d) * 4 * H + 4 * oj;                   // gates
  long c_off = ((((long)d * T + t_first) * (H / 4) + (oj >> 2)) * B + ob) * 4;        // cst
  long y_off = (((long)t_first * B + ob) * D + d) * H + oj;                           // y / y_drop
  const long g_step = tdir * (long)B * D * 4 * H, c_step = tdir * (long)H * B, y_step = tdir * (long)B * D * H;
  const int hx_off = (brow * Kp + oj) * 4;
  __syncthreads();
  unsigned long long dsum[6] = {0, 0, 0, 0, 0, 0}, dlast = clock64();
  const bool local = p.allow_local && group_is_xcd_local(p.xcc + gid * p.NC, p.NC, wg, p.status, abort_lds);

  auto run = [&](auto local_tag) -> bool {
  constexpr bool LOCAL = decltype(local_tag)::value;
  for (int s = 0; s < T; ++s) {
    const int t = (d == 0) ? s : T - 1 - s;
    f32x4 xp = {0.f, 0.f, 0.f, 0.f};
    if (valid) xp = *reinterpret_cast<const f32x4*>(p.gates + g_off);

    f32x4 acc[BQ];
#pragma unroll
    for (int bq = 0; bq < BQ; ++bq) acc[bq] = (f32x4){0.f, 0.f, 0.f, 0.f};
    DBG_STAMP(0);  // prefetch issue
    if (s > 0) {
      if (!wait_flags(flags, p.NC, (unsigned)s, p.status, abort_lds)) return false;
      DBG_STAMP(1);  // flag wait
      gather_mma<KS, BQ>(hx_rsrc[(s - 1) & 1], Kp, wave * Kw, Ls, WA + wave * ns4 * 64,
                         hs_all + wave * stage_floats<KS, BQ>(), lane, myks, acc);
      DBG_STAMP(2);  // gather + MFMA
    }
#pragma unroll
    for (int bq = 0; bq < BQ; ++bq) part[(wave * BQ + bq) * 64 + lane] = acc[bq];
    __syncthreads();
    f32x4 gact = {0.f, 0.f, 0.f, 0.f}, h4 = {0.f, 0.f, 0.f, 0.f}, c4 = {0.f, 0.f, 0.f, 0.f};
    bool quad_lead = false;
    if (owner) {
      f32x4 rec = {0.f, 0.f, 0.f, 0.f};  // h_{t-1} . W_hh^T for this cell's slots
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) rec += part[(w * BQ + obq) * 64 + ks * 4 * HS + ol];
      const bool active = valid && t < olen;
      float hval = 0.f;
      if (active) {
        if constexpr (CELL == 0) {
          const f32x4 g4 = xp + rec;
          const float ig = sig_sel(g4[0], p.hw_math), fg = sig_sel(g4[1], p.hw_math), gg = tanh_sel(g4[2], p.hw_math), og = sig_sel(g4[3], p.hw_math);
          c_state = fg * c_state + ig * gg;
          hval = og * tanh_sel(c_state, p.hw_math);
          gact = (f32x4){ig, fg, gg, og};
        } else if constexpr (CELL == 1) {
          const float rg = sig_sel(xp[0] + rec[0], p.hw_math), zg = sig_sel(xp[1] + rec[1], p.hw_math);
          const float hn = rec[2] + bhn;
          const float ng = tanh_sel(xp[2] + rg * hn, p.hw_math);
          hval = (1.f - zg) * ng + zg * c_state;
          c_state = hval;
          gact = (f32x4){rg, zg, ng, hn};
        } else {
          const float pre = xp[0] + rec[0];
          hval = (p.cell == RNNT_CELL_RNN_RELU) ? fmaxf(pre, 0.f) : tanh_sel(pre, p.hw_math);
          c_state = hval;
          gact = (f32x4){hval, 0.f, 0.f, 0.f};
        }
      } else {
        c_state = 0.f;
      }
      // 4 consecutive units of one batch row sit in lanes l, l+4, l+8, l+12: collect them in the first
      h4 = (f32x4){hval, row_shl<0x104>(hval), row_shl<0x108>(hval), row_shl<0x10C>(hval)};
      c4 = (f32x4){c_state, row_shl<0x104>(c_state), row_shl<0x108>(c_state), row_shl<0x10C>(c_state)};
      quad_lead = (ounit & 3) == 0;
      if (quad_lead)  // ONLY the exchange slice is stored before the flag: it is what the group waits for
        exchange_store<LOCAL>(__builtin_bit_cast(i32x4, h4), hx_rsrc[s & 1], hx_off);
    }
    DBG_STAMP(3);  // LDS reduce + cell math + exchange store issue
    publish_flag2<LOCAL>(flags + wg, (unsigned)(s + 1));
    DBG_STAMP(4);  // drain + barrier + flag
    // stash / layer-output stores AFTER the flag: they overlap the group's next exchange instead of delaying it
    if (valid) {
      *reinterpret_cast<f32x4*>(p.gates + g_off) = gact;
      if (quad_lead) {
        if constexpr (CELL == 0) *reinterpret_cast<f32x4*>(p.cst + c_off) = c4;
        const long yo = y_off;
        *reinterpret_cast<f32x4*>(p.y + yo) = h4;
        if (p.ydrop) {
          f32x4 hd;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            hd[e] = (hash_u32(p.seed, (unsigned long long)(yo + e)) >= p.drop_thresh) ? h4[e] * p.keep_scale : 0.f;
          *reinterpret_cast<f32x4*>(p.ydrop + yo) = hd;
        }
      }
    }
    g_off += g_step;
    c_off += c_step;
    y_off += y_step;
    DBG_STAMP(5);  // stash stores issue
  }
  return true;
  };
  const bool ok = local ? run(std::true_type{}) : run(std::false_type{});
  if (!ok) return;
  if (p.dbg && tid == 0) {
    for (int i = 0; i < 6; ++i) p.dbg[blockIdx.x * 8 + i] = dsum[i];
    unsigned xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    p.dbg[blockIdx.x * 8 + 6] = local ? 1 : 0;
    p.dbg[blockIdx.x * 8 + 7] = xcc_id & 0xf;
  }
}

// ================================================================================================
// v3 forward: the recurrent product on the bf16 matrix cores, W_hh stationary in REGISTERS.
//
// Same decomposition as v2 (sync groups = direction x batch slice, a workgroup owns HS = 16 hidden units, split-K over the
// 4 waves), but h_{t-1} . W_hh^T runs as v_mfma_f32_16x16x32_bf16 on exact bf16 pieces (common.hpp: 6 piece products =
// fp32 accuracy) instead of v_mfma_f32_4x4x1_16B_f32: 96 MFMAs x 16 cycles per wave and step instead of 256 x 12.2.
//   M = the workgroup's 64 gate columns (4 blocks of 16 = 4 units x 4 gate slots), N = the group's batch rows (<= 16),
//   K = this wave's quarter of the hidden vector (NKS steps of 32).
//   A (stationary): lane -> gate column 16*mb + (lane&15), k = 32*ks + 8*(lane>>4) + e: the wave's W_hh slice as
//     3 bf16 pieces = 4*NKS*12 VGPRs, split once at kernel start: no LDS copy of the weights, no per-step weight reads.
//   B (per step): lane -> batch row (lane&15), the same 8 consecutive k.  The PRODUCER of a hidden value splits it (one cell
//     per lane: 4 VALU) and publishes three bf16 planes [row][Kp]; a consumer's operand piece is then 16 contiguous bytes:
//     three 16-B sc1 loads per k-step straight into MFMA operand registers, no LDS stage and no split on the critical path
//     (splitting at the consumers cost 176 VALU per lane and step in every one of the group's 32 workgroups).
//   D: lane -> (unit 4*mb + (lane>>4), row lane&15), its 4 registers = the 4 gate slots of that cell.
// Cross-wave reduction through LDS; wave w then owns units 4w..4w+3: one cell per lane, no DPP gymnastics.
// Stash layouts (gates, cst, y) are those of v2, so lstm_bwd2_kernel consumes them unchanged.
// dynamic LDS: part[4 waves][4 mb][64] f32x4 | abort
// ================================================================================================
// MB: 16-gate-column blocks per workgroup (the workgroup owns 4*MB hidden units); MB = 5 with 8 waves and K padded to 768 is
// the H = 640 form: 32 workgroups per sync group, which fit one XCD (40 would not)
// NLB: the last NLB of the MB gate-column blocks keep their W_hh pieces in LDS instead of registers (8-wave forms: two waves
// per SIMD share a 256-register cap)
template <int NKS, int CELL, int NWV = 4, int MB = 4, int NLB = 0>
__global__ void __launch_bounds__(64 * NWV) lstm_fwd3_kernel(const LstmK p) {
  constexpr int NGATE = CELL == 0 ? 4 : (CELL == 1 ? 3 : 1);
  constexpr int HS = 4 * MB;
  static_assert(MB <= NWV, "one owner wave per gate-column block");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, B = p.B, D = p.D, T = p.T, Kp = p.Kp;
  constexpr int Kw = 32 * NKS;
  f32x4* part = reinterpret_cast<f32x4*>(smem);
  int* abort_lds = reinterpret_cast<int*>(part + NWV * MB * 64);
  constexpr int NRB = MB - NLB;
  u32x4* wl = reinterpret_cast<u32x4*>(reinterpret_cast<char*>(abort_lds) + 16) + (long)(threadIdx.x >> 6) * NLB * NKS * 3 * 64;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NG = D * p.G;
  const int gid = blockIdx.x % p.NGL, wg = blockIdx.x / p.NGL;
  if (gid >= NG) return;
  const int d = gid / p.G, g = gid % p.G;
  const int b0 = g * p.Bg, j0 = wg * HS;
  const int lrow = lane & 15, lq = lane >> 4;

  bf16x8 wp[NRB][NKS][3];
  {
    const float* W = p.w_hh[d];
    const int gate = lrow & 3;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const float* row = W + (long)(gate * H + j0 + 4 * mb + (lrow >> 2)) * H;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const int k = wave * Kw + 32 * ks + 8 * lq;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (gate < NGATE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (k + e < H) lo[e] = row[k + e];
            if (k + 4 + e < H) hi[e] = row[k + 4 + e];
          }
        }
        if (mb < NRB) {
          split8(lo, hi, wp[mb < NRB ? mb : 0][ks]);
        } else {
          bf16x8 tmp[3];
          split8(lo, hi, tmp);
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) wl[(((mb - NRB) * NKS + ks) * 3 + pl) * 64 + lane] = __builtin_bit_cast(u32x4, tmp[pl]);
        }
      }
    }
    if (tid == 0) *abort_lds = 0;
  }
  const int NBR = 4 * ((p.Bg + 3) / 4);  // exchange rows of the group (as allocated by the host: 4*BQ)
  // the exchange carries h already split by its producer: three bf16 planes [row][Kp] per (parity, group), 6 bytes per value
  const int plane_b = NBR * Kp * 2;
  const long hx_bytes = 3l * plane_b;
  __amdgpu_buffer_rsrc_t hx_rsrc[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    hx_rsrc[par] = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(p.hx) + ((long)par * NG + gid) * hx_bytes, 0,
                                                     (int)hx_bytes, RSRC_FLAGS);
  unsigned* flags = p.flags + gid * p.NC;

  // one cell per lane of waves 0..3: unit 4*wave + lq of this workgroup, batch row lrow of this group (with NWV = 8 the
  // upper four waves only contribute their K-slice of the product)
  const bool ownw = wave < MB;
  const int ownb = ownw ? wave : 0;
  const int brow = lrow;
  const int ob = b0 + brow, oj = j0 + 4 * ownb + lq;
  const bool inrow = ownw && brow < NBR;
  const bool valid = ownw && brow < p.Bg && ob < B;
  const int olen = valid ? p.lens[ob] : 0;
  float c_state = 0.f;
  const float bhn = (CELL == 1 && ownw) ? p.b_hh[d][2 * H + oj] : 0.f;
  const int t_first = (d == 0) ? 0 : T - 1;
  const long tdir = (d == 0) ? 1 : -1;
  long g_off = (((long)t_first * B + ob) * D + d) * 4 * H + 4 * oj;
  long c_off = ((((long)d * T + t_first) * (H / 4) + (oj >> 2)) * B + ob) * 4 + (oj & 3);
  long y_off = (((long)t_first * B + ob) * D + d) * H + oj;
  const long g_step = tdir * (long)B * D * 4 * H, c_step = tdir * (long)H * B, y_step = tdir * (long)B * D * H;
  const int hx_off = (brow * Kp + oj) * 2;
  const int gat_off = brow < NBR ? (brow * Kp + wave * Kw + 8 * lq) * 2 : 0x7ffffff0;  // rows beyond the group read 0
  __syncthreads();
  unsigned long long dsum[6] = {0, 0, 0, 0, 0, 0}, dlast = clock64();
  const bool local = p.allow_local && group_is_xcd_local(p.xcc + gid * p.NC, p.NC, wg, p.status, abort_lds);

  auto run = [&](auto local_tag) -> bool {
  constexpr bool LOCAL = decltype(local_tag)::value;
  for (int s = 0; s < T; ++s) {
    const int t = (d == 0) ? s : T - 1 - s;
    f32x4 xp = {0.f, 0.f, 0.f, 0.f};
    if (valid) xp = *reinterpret_cast<const f32x4*>(p.gates + g_off);

    f32x4 acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    DBG_STAMP(0);
    if (s > 0) {
      if (!wait_flags(flags, p.NC, (unsigned)s, p.status, abort_lds)) return false;
      DBG_STAMP(1);
      i32x4 raw[NKS][3];
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          raw[ks][pl] = __builtin_amdgcn_raw_buffer_load_b128(hx_rsrc[(s - 1) & 1], gat_off + 64 * ks + pl * plane_b, 0, AUX_SC1);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        bf16x8 hp[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) hp[pl] = __builtin_bit_cast(bf16x8, raw[ks][pl]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          bf16x8 w0, w1, w2;
          if (mb < NRB) {
            w0 = wp[mb < NRB ? mb : 0][ks][0]; w1 = wp[mb < NRB ? mb : 0][ks][1]; w2 = wp[mb < NRB ? mb : 0][ks][2];
          } else {
            const u32x4* f = wl + ((mb - NRB) * NKS + ks) * 3 * 64 + lane;
            w0 = __builtin_bit_cast(bf16x8, f[0]); w1 = __builtin_bit_cast(bf16x8, f[64]); w2 = __builtin_bit_cast(bf16x8, f[128]);
          }
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, hp[0], acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, hp[1], acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, hp[2], acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, hp[0], acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, hp[1], acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, hp[0], acc[mb], 0, 0, 0);
        }
      }
      DBG_STAMP(2);
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) part[(wave * MB + mb) * 64 + lane] = acc[mb];
    __syncthreads();
    f32x4 rec = part[ownb * 64 + lane];
#pragma unroll
    for (int w = 1; w < NWV; ++w) rec += part[(w * MB + ownb) * 64 + lane];
    const bool active = valid && t < olen;
    float hval = 0.f;
    f32x4 gact = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      if constexpr (CELL == 0) {
        const f32x4 g4 = xp + rec;
        const float ig = sig_sel(g4[0], p.hw_math), fg = sig_sel(g4[1], p.hw_math), gg = tanh_sel(g4[2], p.hw_math), og = sig_sel(g4[3], p.hw_math);
        c_state = fg * c_state + ig * gg;
        hval = og * tanh_sel(c_state, p.hw_math);
        gact = (f32x4){ig, fg, gg, og};
      } else if constexpr (CELL == 1) {
        const float rg = sig_sel(xp[0] + rec[0], p.hw_math), zg = sig_sel(xp[1] + rec[1], p.hw_math);
        const float hn = rec[2] + bhn;
        const float ng = tanh_sel(xp[2] + rg * hn, p.hw_math);
        hval = (1.f - zg) * ng + zg * c_state;
        c_state = hval;
        gact = (f32x4){rg, zg, ng, hn};
      } else {
        const float pre = xp[0] + rec[0];
        hval = (p.cell == RNNT_CELL_RNN_RELU) ? fmaxf(pre, 0.f) : tanh_sel(pre, p.hw_math);
        c_state = hval;
        gact = (f32x4){hval, 0.f, 0.f, 0.f};
      }
    } else {
      c_state = 0.f;
    }
    if (inrow) {  // ONLY the exchange slice is stored before the flag: h = h0 + h1 + h2 exactly, one bf16 per plane
      const unsigned u0 = __float_as_uint(hval);
      const float r1 = hval - __uint_as_float(u0 & 0xffff0000u);
      const unsigned u1 = __float_as_uint(r1);
      const unsigned u2 = __float_as_uint(r1 - __uint_as_float(u1 & 0xffff0000u));
      constexpr int AUX = LOCAL ? 0 : AUX_SC1;
      __builtin_amdgcn_raw_buffer_store_b16((short)(u0 >> 16), hx_rsrc[s & 1], hx_off, 0, AUX);
      __builtin_amdgcn_raw_buffer_store_b16((short)(u1 >> 16), hx_rsrc[s & 1], hx_off + plane_b, 0, AUX);
      __builtin_amdgcn_raw_buffer_store_b16((short)(u2 >> 16), hx_rsrc[s & 1], hx_off + 2 * plane_b, 0, AUX);
    }
    DBG_STAMP(3);
    publish_flag2<LOCAL>(flags + wg, (unsigned)(s + 1));
    DBG_STAMP(4);
    if (valid) {
      *reinterpret_cast<f32x4*>(p.gates + g_off) = gact;
      if constexpr (CELL == 0) p.cst[c_off] = c_state;
      p.y[y_off] = hval;
      if (p.ydrop)
        p.ydrop[y_off] = (hash_u32(p.seed, (unsigned long long)y_off) >= p.drop_thresh) ? hval * p.keep_scale : 0.f;
    }
    g_off += g_step;
    c_off += c_step;
    y_off += y_step;
    DBG_STAMP(5);
  }
  return true;
  };
  const bool ok = local ? run(std::true_type{}) : run(std::false_type{});
  if (!ok) return;
  if (p.dbg && tid == 0) {
    for (int i = 0; i < 6; ++i) p.dbg[blockIdx.x * 8 + i] = dsum[i];
    unsigned xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    p.dbg[blockIdx.x * 8 + 6] = local ? 1 : 0;
    p.dbg[blockIdx.x * 8 + 7] = xcc_id & 0xf;
  }
}

// dynamic LDS: WA[4][Ls/4][64] f32x4 | hs[4][stage_floats] | part[4][BQ][64] f32x4 | abort
template <int HS, int BQ, int CELL>
__global__ void __launch_bounds__(256) lstm_bwd2_kernel(const LstmK p) {
  constexpr int NGATE = CELL == 0 ? 4 : (CELL == 1 ? 3 : 1);
  constexpr int UQ = HS / 4, KS = 16 / UQ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, B = p.B, D = p.D, T = p.T, Kp = p.Kp;
  const int Kw = Kp, Ls = Kw / KS, ns4 = Ls / 4;  // contraction index k = 4*j' + gate over 4*Kp, a quarter per wave
  f32x4* WA = reinterpret_cast<f32x4*>(smem);
  float* hs_all = reinterpret_cast<float*>(WA + 4 * ns4 * 64);
  float* part = hs_all + 4 * stage_floats<KS, BQ>();
  int* abort_lds = reinterpret_cast<int*>(part + 4 * BQ * 64 * 4);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NG = D * p.G;
  const int gid = blockIdx.x % p.NGL, wg = blockIdx.x / p.NGL;
  if (gid >= NG) return;
  const int d = gid / p.G, g = gid % p.G;
  const int b0 = g * p.Bg, j0 = wg * HS;

  {  // weights: lane = 4*blk + i, blk = ks*UQ + uq  <->  W_hh[(gate k&3)*H + (k>>2)][j0 + 4*uq + i]
    const float* W = p.w_hh[d];
    for (int idx = tid; idx < 4 * ns4 * 64; idx += 256) {
      const int ln = idx & 63, s4 = (idx >> 6) % ns4, w = (idx >> 6) / ns4;
      const int i = ln & 3, blk = ln >> 2, uq = blk % UQ, ks = blk / UQ;
      const int k = w * Kw + ks * Ls + 4 * s4;  // multiple of 4: e is the gate, k>>2 the unit j'
      const int jp = k >> 2, col = j0 + 4 * uq + i;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (jp < H) {
#pragma unroll
        for (int e = 0; e < NGATE; ++e) v[e] = W[(long)(e * H + jp) * H + col];
      }
      WA[idx] = v;
    }
    if (tid == 0) *abort_lds = 0;
  }
  constexpr int NBR = 4 * BQ;
  const long gx_floats = (long)NBR * 4 * Kp;
  __amdgpu_buffer_rsrc_t gx_rsrc[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    gx_rsrc[par] = __builtin_amdgcn_make_buffer_rsrc(p.hx + ((long)par * NG + gid) * gx_floats, 0, (int)(gx_floats * 4), RSRC_FLAGS);
  unsigned* flags = p.flags + gid * p.NC;

  // cell owners: tid = ((obq*UQ + uq)*4 + i)*4 + j -> unit j0 + 4*uq + i, batch row 4*obq + j
  const bool owner = tid < BQ * HS * 4;
  const int ojb = tid & 3, oi = (tid >> 2) & 3, ouq = (tid >> 4) % UQ, obq = (tid >> 4) / UQ;
  const int brow = 4 * obq + ojb, ob = b0 + brow, oj = j0 + 4 * ouq + oi;
  const bool valid = owner && brow < p.Bg && ob < B;
  const int olen = valid ? p.lens[ob] : 0;
  float dc_carry = 0.f;
  const int myks = (lane >> 2) / UQ;
  const int t_first = (d == 0) ? T - 1 : 0;
  const long tdir = (d == 0) ? -1 : 1;
  long g_off = (((long)t_first * B + ob) * D + d) * 4 * H + 4 * oj;
  long c_off = ((((long)d * T + t_first) * (H / 4) + (oj >> 2)) * B + ob) * 4 + (oj & 3);
  long y_off = (((long)t_first * B + ob) * D + d) * H + oj;
  const long g_step = tdir * (long)B * D * 4 * H, c_step = tdir * (long)H * B, y_step = tdir * (long)B * D * H;
  const int gx_off = (brow * 4 * Kp + 4 * oj) * 4;
  __syncthreads();
  unsigned long long dsum[6] = {0, 0, 0, 0, 0, 0}, dlast = clock64();
  const bool local = p.allow_local && group_is_xcd_local(p.xcc + gid * p.NC, p.NC, wg, p.status, abort_lds);

  auto run = [&](auto local_tag) -> bool {
  constexpr bool LOCAL = decltype(local_tag)::value;
  for (int s = 0; s < T; ++s) {
    const int t = (d == 0) ? T - 1 - s : s;
    const int tprev = (d == 0) ? t - 1 : t + 1;
    f32x4 gt = {0.f, 0.f, 0.f, 0.f};
    float c_t = 0.f, c_p = 0.f, dyv = 0.f;
    const bool active = valid && t < olen;
    if (active) {
      gt = *reinterpret_cast<const f32x4*>(p.gates + g_off);
      if constexpr (CELL == 0) {
        c_t = p.cst[c_off];
        if (tprev >= 0 && tprev < T) c_p = p.cst[c_off + c_step];  // the backward walks towards the forward's t_prev
      } else if constexpr (CELL == 1) {
        if (tprev >= 0 && tprev < T) c_p = p.y[y_off + y_step];    // GRU: h_{t_prev} of this cell (0 at the sequence start)
      }
      const long yo = y_off;
      dyv = p.dy[yo];
      if (p.ydrop) dyv = (hash_u32(p.seed, (unsigned long long)yo) >= p.drop_thresh) ? dyv * p.keep_scale : 0.f;
    }

    f32x4 acc[BQ];
#pragma unroll
    for (int bq = 0; bq < BQ; ++bq) acc[bq] = (f32x4){0.f, 0.f, 0.f, 0.f};
    DBG_STAMP(0);  // prefetch issue
    if (s > 0) {
      if (!wait_flags(flags, p.NC, (unsigned)s, p.status, abort_lds)) return false;
      DBG_STAMP(1);  // flag wait
      gather_mma<KS, BQ>(gx_rsrc[(s - 1) & 1], 4 * Kp, wave * Kw, Ls, WA + wave * ns4 * 64,
                         hs_all + wave * stage_floats<KS, BQ>(), lane, myks, acc);
      DBG_STAMP(2);  // gather + MFMA
    }
#pragma unroll
    for (int bq = 0; bq < BQ; ++bq) *reinterpret_cast<f32x4*>(&part[((wave * BQ + bq) * 64 + lane) * 4]) = acc[bq];
    __syncthreads();
    f32x4 dg4 = {0.f, 0.f, 0.f, 0.f}, dgh4 = {0.f, 0.f, 0.f, 0.f};
    if (owner) {
      float dh = dyv;
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) dh += part[((w * BQ + obq) * 64 + 4 * (ks * UQ + ouq) + ojb) * 4 + oi];
      if (active) {
        if constexpr (CELL == 0) {
          const float ig = gt[0], fg = gt[1], gg = gt[2], og = gt[3];
          const float tc = tanh_sel(c_t, p.hw_math);
          const float dc = dh * og * (1.f - tc * tc) + dc_carry;
          dg4[0] = dc * gg * ig * (1.f - ig);
          dg4[1] = dc * c_p * fg * (1.f - fg);
          dg4[2] = dc * ig * (1.f - gg * gg);
          dg4[3] = dh * tc * og * (1.f - og);
          dc_carry = dc * fg;
          dgh4 = dg4;
        } else if constexpr (CELL == 1) {
          const float rg = gt[0], zg = gt[1], ng = gt[2], hn = gt[3];
          dh += dc_carry;                       // direct path dh_t -> dh_{t_prev} through z
          const float dn_pre = dh * (1.f - zg) * (1.f - ng * ng);
          const float dz_pre = dh * (c_p - ng) * zg * (1.f - zg);
          const float dr_pre = dn_pre * hn * rg * (1.f - rg);
          dg4 = (f32x4){dr_pre, dz_pre, dn_pre, 0.f};        // input side: dX, dW_ih, db_ih
          dgh4 = (f32x4){dr_pre, dz_pre, dn_pre * rg, 0.f};  // hidden side: W_hh^T product, dW_hh, db_hh
          dc_carry = dh * zg;
        } else {
          const float hv = gt[0];
          const float dpre = (p.cell == RNNT_CELL_RNN_RELU) ? (hv > 0.f ? dh : 0.f) : dh * (1.f - hv * hv);
          dg4 = (f32x4){dpre, 0.f, 0.f, 0.f};
          dgh4 = dg4;
        }
      } else {
        dc_carry = 0.f;
      }
      exchange_store<LOCAL>(__builtin_bit_cast(i32x4, dgh4), gx_rsrc[s & 1], gx_off);
    }
    DBG_STAMP(3);  // LDS reduce + cell math + exchange store issue
    publish_flag2<LOCAL>(flags + wg, (unsigned)(s + 1));
    DBG_STAMP(4);  // drain + barrier + flag
    if (valid) {  // stash after the flag (off the critical path)
      *reinterpret_cast<f32x4*>(p.gates + g_off) = dg4;
      if constexpr (CELL == 1) *reinterpret_cast<f32x4*>(p.aux + g_off) = dgh4;
    }
    g_off += g_step;
    c_off += c_step;
    y_off += y_step;
    DBG_STAMP(5);  // stash stores issue
  }
  return true;
  };
  const bool ok = local ? run(std::true_type{}) : run(std::false_type{});
  if (!ok) return;
  if (p.dbg && tid == 0) {
    for (int i = 0; i < 6; ++i) p.dbg[blockIdx.x * 8 + i] = dsum[i];
    unsigned xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    p.dbg[blockIdx.x * 8 + 6] = local ? 1 : 0;
    p.dbg[blockIdx.x * 8 + 7] = xcc_id & 0xf;
  }
}

// ================================================================================================
// v4 backward ("scatter form"): the recurrent product dh_{t-1} = dG_t . W_hh with the roles of the exchange swapped.
//
// v2 gathers ALL of dG_t (rows x 4H: 64 KB per workgroup and step at H = 512) and multiplies by its 16 columns of W_hh.
// Here a workgroup multiplies ITS OWN 64 gate columns of dG_t (rows x 64, local, produced by its own cell math) by its 64
// ROWS of W_hh and publishes the partial dh_{t-1} for ALL hidden units (rows x H); a consumer then sums, for its 16 units,
// the NC partial slices (NC x rows x 16 floats = 16 KB at H = 512: the forward's exchange volume, a quarter of v2's).
// The product runs on the bf16 matrix cores on exact bf16 pieces (common.hpp), W_hh stationary in registers:
//   M = output units (this wave's Kp/64 blocks of 16), N = the group's batch rows (<= 16), K = the 64 own gate columns
//   (2 steps of 32);  A: lane -> output unit 16*mb + (lane&15), k = 32*ks + 8*(lane>>4) + e = 4*(own unit) + gate;
//   B: lane -> row (lane&15), the same 8 gate columns, read from a 4 KB LDS image of the cell math's dG and split;
//   D: lane -> (units 16*mb + 4*(lane>>4) .. +3, row lane&15): one 16-byte store straight into the exchange buffer.
// Exchange buffer: partial[parity][group][producer][row][Kp] fp32.  Protocol, owners, cell math and stash as in v2.
// dynamic LDS: red[256] f32x4 | dgs[16][DGS_LD] float | abort
// ================================================================================================
// NOB: 16-unit output blocks per wave (Kp / 16 / NWV); MB: the workgroup owns 4*MB units = 16*MB gate columns
// NLB: of a wave's NOB output blocks, the last NLB keep their W_hh pieces in LDS (MFMA-operand order, one 16-byte fragment
// per lane) instead of registers: the 8-wave forms run two waves per SIMD under a 256-register cap
template <int NOB, int BQ, int CELL, int NWV = 4, int MB = 4, int NLB = 0>
__global__ void __launch_bounds__(64 * NWV) lstm_bwd4_kernel(const LstmK p) {
  constexpr int NGATE = CELL == 0 ? 4 : (CELL == 1 ? 3 : 1);
  constexpr int HS = 4 * MB, UQ = MB;
  constexpr int NT = 64 * NWV;
  constexpr int NMB = NOB;
  constexpr int NRB = NOB - NLB;          // output blocks whose W pieces stay in registers
  constexpr int KSB = (16 * MB + 31) / 32;   // 32-deep k-steps over the own gate columns (zero padded)
  constexpr int NBR = 4 * BQ;           // exchange rows of the group
  constexpr int DGS_LD = 32 * KSB + 4;   // floats per row of the dG image (+ pad)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, B = p.B, D = p.D, T = p.T, Kp = p.Kp;
  f32x4* red = reinterpret_cast<f32x4*>(smem);
  float* dgs = reinterpret_cast<float*>(red + NT);
  int* abort_lds = reinterpret_cast<int*>(dgs + 16 * DGS_LD);
  // [wave][NLB][KSB][3][64] 16-byte fragments, after a 16-byte aligned gap
  u32x4* wl = reinterpret_cast<u32x4*>(reinterpret_cast<char*>(abort_lds) + 16) + (long)(threadIdx.x >> 6) * NLB * KSB * 3 * 64;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NG = D * p.G;
  const int gid = blockIdx.x % p.NGL, wg = blockIdx.x / p.NGL;
  if (gid >= NG) return;
  const int d = gid / p.G, g = gid % p.G;
  const int b0 = g * p.Bg, j0 = wg * HS;
  const int lrow = lane & 15, lq = lane >> 4;

  bf16x8 wp[NRB > 0 ? NRB : 1][KSB][3];
  {
    const float* W = p.w_hh[d];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb) {
      const int u = 16 * (wave * NMB + mb) + lrow;  // output unit = column of W_hh
#pragma unroll
      for (int ks = 0; ks < KSB; ++ks) {
        const int c = 32 * ks + 8 * lq;             // own gate column 4*unit + gate; c is a multiple of 8
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (u < H) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (e < NGATE) {
              if ((c >> 2) < HS) lo[e] = W[(long)(e * H + j0 + (c >> 2)) * H + u];
              if ((c >> 2) + 1 < HS) hi[e] = W[(long)(e * H + j0 + (c >> 2) + 1) * H + u];
            }
          }
        }
        if (mb < NRB) {
          split8(lo, hi, wp[mb < NRB ? mb : 0][ks]);
        } else {
          bf16x8 tmp[3];
          split8(lo, hi, tmp);
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) wl[(((mb - NRB) * KSB + ks) * 3 + pl) * 64 + lane] = __builtin_bit_cast(u32x4, tmp[pl]);
        }
      }
    }
    for (int i = tid; i < 16 * DGS_LD; i += NT) dgs[i] = 0.f;
    if (tid == 0) *abort_lds = 0;
  }
  const long px_floats = (long)p.NC * NBR * Kp;  // one group's partials of one parity
  __amdgpu_buffer_rsrc_t px_rsrc[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    px_rsrc[par] = __builtin_amdgcn_make_buffer_rsrc(p.hx + ((long)par * NG + gid) * px_floats, 0, (int)(px_floats * 4), RSRC_FLAGS);
  unsigned* flags = p.flags + gid * p.NC;

  // cell owners (as v2): tid = ((obq*UQ + uq)*4 + i)*4 + j -> unit j0 + 4*uq + i, batch row 4*obq + j
  const bool owner = tid < BQ * HS * 4;
  const int ojb = tid & 3, oi = (tid >> 2) & 3, ouq = (tid >> 4) % UQ, obq = (tid >> 4) / UQ;  // valid for tid < BQ*HS*4
  const int brow = 4 * obq + ojb, ob = b0 + brow, oj = j0 + 4 * ouq + oi;
  const bool valid = owner && brow < p.Bg && ob < B;
  const int olen = valid ? p.lens[ob] : 0;
  float dc_carry = 0.f;
  f32x4 db_acc = {0.f, 0.f, 0.f, 0.f}, dbh_acc = {0.f, 0.f, 0.f, 0.f};  // bias gradients: time sums of this cell's dG
  const int t_first = (d == 0) ? T - 1 : 0;
  const long tdir = (d == 0) ? -1 : 1;
  long g_off = (((long)t_first * B + ob) * D + d) * 4 * H + 4 * oj;
  long c_off = ((((long)d * T + t_first) * (H / 4) + (oj >> 2)) * B + ob) * 4 + (oj & 3);
  long y_off = (((long)t_first * B + ob) * D + d) * H + oj;
  const long g_step = tdir * (long)B * D * 4 * H, c_step = tdir * (long)H * B, y_step = tdir * (long)B * D * H;
  // gather: thread -> (row, unit quad) pair pr = tid % (NBR*UQ) and producer class q = tid / (NBR*UQ); it sums the partial
  // slices of producers q, q + NQ, ... for that pair; owners then add the NQ class sums
  constexpr int NPAIR = NBR * UQ, NQ = NT / NPAIR;
  const int gq = tid / NPAIR, gpr = tid % NPAIR;
  const int grow = gpr / UQ, guq = gpr % UQ;
  const bool gact = gq < NQ;
  const int gat_base = (gq * NBR + grow) * Kp + j0 + 4 * guq;  // floats; + NQ producers per visit
  const int gat_step = NQ * NBR * Kp;
  // publish: lane -> row lrow, units 16*mbg + 4*lq .. +3
  const int pub_base = lrow < NBR ? ((wg * NBR + lrow) * Kp + 16 * wave * NMB + 4 * lq) * 4 : 0x7ffffff0;
  __syncthreads();
  unsigned long long dsum[6] = {0, 0, 0, 0, 0, 0}, dlast = clock64();
  const bool local = p.allow_local && group_is_xcd_local(p.xcc + gid * p.NC, p.NC, wg, p.status, abort_lds);

  auto run = [&](auto local_tag) -> bool {
  constexpr bool LOCAL = decltype(local_tag)::value;
  for (int s = 0; s < T; ++s) {
    const int t = (d == 0) ? T - 1 - s : s;
    const int tprev = (d == 0) ? t - 1 : t + 1;
    f32x4 gt = {0.f, 0.f, 0.f, 0.f};
    float c_t = 0.f, c_p = 0.f, dyv = 0.f;
    const bool active = valid && t < olen;
    if (active) {
      gt = *reinterpret_cast<const f32x4*>(p.gates + g_off);
      if constexpr (CELL == 0) {
        c_t = p.cst[c_off];
        if (tprev >= 0 && tprev < T) c_p = p.cst[c_off + c_step];
      } else if constexpr (CELL == 1) {
        if (tprev >= 0 && tprev < T) c_p = p.y[y_off + y_step];
      }
      const long yo = y_off;
      dyv = p.dy[yo];
      if (p.ydrop) dyv = (hash_u32(p.seed, (unsigned long long)yo) >= p.drop_thresh) ? dyv * p.keep_scale : 0.f;
    }
    DBG_STAMP(0);  // prefetch issue
    f32x4 gsum = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      if (!wait_flags(flags, p.NC, (unsigned)s, p.status, abort_lds)) return false;
      DBG_STAMP(1);  // flag wait
      const __amdgpu_buffer_rsrc_t src = px_rsrc[(s - 1) & 1];
      constexpr int NI = 4;
      for (int w0 = 0; w0 < p.NC; w0 += NQ * NI) {
        i32x4 r[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const bool ok = gact && w0 + gq + NQ * i < p.NC;
          r[i] = __builtin_amdgcn_raw_buffer_load_b128(src, ok ? (gat_base + (w0 / NQ + i) * gat_step) * 4 : 0x7ffffff0, 0, AUX_SC1);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) gsum += __builtin_bit_cast(f32x4, r[i]);
      }
    }
    red[tid] = gsum;
    __syncthreads();
    DBG_STAMP(2);  // gather + partial sums
    f32x4 dg4 = {0.f, 0.f, 0.f, 0.f}, dgh4 = {0.f, 0.f, 0.f, 0.f};
    if (owner) {
      float dh = dyv;
#pragma unroll
      for (int q = 0; q < NQ; ++q) dh += red[q * NPAIR + brow * UQ + ouq][oi];
      if (active) {
        if constexpr (CELL == 0) {
          const float ig = gt[0], fg = gt[1], gg = gt[2], og = gt[3];
          const float tc = tanh_sel(c_t, p.hw_math);
          const float dc = dh * og * (1.f - tc * tc) + dc_carry;
          dg4[0] = dc * gg * ig * (1.f - ig);
          dg4[1] = dc * c_p * fg * (1.f - fg);
          dg4[2] = dc * ig * (1.f - gg * gg);
          dg4[3] = dh * tc * og * (1.f - og);
          dc_carry = dc * fg;
          dgh4 = dg4;
        } else if constexpr (CELL == 1) {
          const float rg = gt[0], zg = gt[1], ng = gt[2], hn = gt[3];
          dh += dc_carry;
          const float dn_pre = dh * (1.f - zg) * (1.f - ng * ng);
          const float dz_pre = dh * (c_p - ng) * zg * (1.f - zg);
          const float dr_pre = dn_pre * hn * rg * (1.f - rg);
          dg4 = (f32x4){dr_pre, dz_pre, dn_pre, 0.f};
          dgh4 = (f32x4){dr_pre, dz_pre, dn_pre * rg, 0.f};
          dc_carry = dh * zg;
        } else {
          const float hv = gt[0];
          const float dpre = (p.cell == RNNT_CELL_RNN_RELU) ? (hv > 0.f ? dh : 0.f) : dh * (1.f - hv * hv);
          dg4 = (f32x4){dpre, 0.f, 0.f, 0.f};
          dgh4 = dg4;
        }
      } else {
        dc_carry = 0.f;
      }
      db_acc += dg4;
      if constexpr (CELL == 1) dbh_acc += dgh4;
      *reinterpret_cast<f32x4*>(&dgs[brow * DGS_LD + 4 * (4 * ouq + oi)]) = dgh4;  // own gate column 4*unit + gate
    }
    __syncthreads();
    DBG_STAMP(3);  // LDS reduce + cell math
    {
      bf16x8 gp[KSB][3];
#pragma unroll
      for (int ks = 0; ks < KSB; ++ks) {
        const float* src = dgs + lrow * DGS_LD + 32 * ks + 8 * lq;
        split8(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), gp[ks]);
      }
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSB; ++ks) {
          bf16x8 w0, w1, w2;
          if (mb < NRB) {
            w0 = wp[mb < NRB ? mb : 0][ks][0]; w1 = wp[mb < NRB ? mb : 0][ks][1]; w2 = wp[mb < NRB ? mb : 0][ks][2];
          } else {
            const u32x4* f = wl + ((mb - NRB) * KSB + ks) * 3 * 64 + lane;
            w0 = __builtin_bit_cast(bf16x8, f[0]); w1 = __builtin_bit_cast(bf16x8, f[64]); w2 = __builtin_bit_cast(bf16x8, f[128]);
          }
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, gp[ks][0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, gp[ks][1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, gp[ks][2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, gp[ks][0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, gp[ks][1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, gp[ks][0], acc, 0, 0, 0);
        }
        exchange_store<LOCAL>(__builtin_bit_cast(i32x4, acc), px_rsrc[s & 1], pub_base + 64 * mb);
      }
    }
    publish_flag2<LOCAL>(flags + wg, (unsigned)(s + 1));
    DBG_STAMP(4);  // MFMA + partial stores + drain + barrier + flag
    if (valid) {
      *reinterpret_cast<f32x4*>(p.gates + g_off) = dg4;
      if constexpr (CELL == 1) *reinterpret_cast<f32x4*>(p.aux + g_off) = dgh4;
    }
    g_off += g_step;
    c_off += c_step;
    y_off += y_step;
    DBG_STAMP(5);  // stash stores issue
  }
  return true;
  };
  const bool ok = local ? run(std::true_type{}) : run(std::false_type{});
  if (!ok) return;
  if (owner) {  // one row of the (group, exchange row) table per cell row; summed over rows and groups by db_reduce_kernel
    const long row = (long)gid * NBR + brow;
    *reinterpret_cast<f32x4*>(p.dbp + row * 4 * H + 4 * oj) = db_acc;
    if constexpr (CELL == 1) *reinterpret_cast<f32x4*>(p.dbhp + row * 4 * H + 4 * oj) = dbh_acc;
  }
  if (p.dbg && tid == 0) {
    for (int i = 0; i < 6; ++i) p.dbg[blockIdx.x * 8 + i] = dsum[i];
    unsigned xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    p.dbg[blockIdx.x * 8 + 6] = local ? 1 : 0;
    p.dbg[blockIdx.x * 8 + 7] = xcc_id & 0xf;
  }
}

}  // namespace

// host side ----------------------------------------------------------------------------------------------------
// What each kernel generation of this file takes (make_plan*) and one pair of launch functions per generation (as lstm5.hip): the
// layer code (lstm_layer.hip) resolves the plans once per call and names no kernel.

// v1: one 4- / 8- / 16-unit slice of all (padded) rows per workgroup.  Every layer call needs this plan to exist (the acceptance test).
bool make_plan(int B, int H, int D, int cus, Plan* pl) {
  if (H < 4 || H % 4 != 0 || B < 1 || B > 64 || D < 1 || D > 2) return false;
  const int NT = B <= 16 ? 1 : (B <= 32 ? 2 : 4);
  pl->NT = NT;
  pl->Bp = 16 * NT;
  const int KG = (H + 15) / 16;
  pl->LDW = 16 * KG + 4;
  for (int per_cu = 1; per_cu <= 2; ++per_cu) {
    for (int Hs = 4; Hs <= 16; Hs *= 2) {
      if (H % Hs != 0) continue;
      const int MT = Hs / 4, NC = H / Hs;
      // each of the 256 threads owns one cell of one 4-unit x 16-row tile: at most 4 tiles (an 8-unit slice of 64 rows left half
      // its units uncomputed)
      if (MT * NT > 4) continue;
      const size_t lds_fwd = (size_t)4 * Hs * pl->LDW * 4 + (size_t)4 * MT * NT * 64 * 16 + 16;
      const size_t lds_bwd = (size_t)KG * MT * 64 * 16 + (size_t)16 * MT * 4 * NT * 16 * 4 + 16;
      const size_t lds = lds_fwd > lds_bwd ? lds_fwd : lds_bwd;
      if (lds * per_cu > 160 * 1024) continue;
      if ((long)D * NC > (long)cus * per_cu) continue;
      pl->Hs = Hs; pl->NC = NC; pl->MT = MT; pl->wgs_per_cu = per_cu;
      pl->lds_fwd = lds_fwd; pl->lds_bwd = lds_bwd;
      return true;
    }
  }
  return false;
}

// v2 decomposition: largest hidden slice whose W_hh rows fit LDS (fewest workgroups per sync group), then as many
// batch slices as the CUs allow.  Returns false when the shape does not fit (caller falls back to v1).
bool make_plan2(int B, int H, int D, int cus, Plan2* pl) {
  if (H < 4 || H % 4 != 0 || B < 1 || D < 1 || D > 2) return false;
  if (getenv("RNNT_LSTM_V1")) return false;
  const int Kp = (int)align_up((size_t)H, 64);
  for (int HS = 16; HS >= 4; HS /= 2) {
    if (H % HS != 0) continue;
    const int NC = H / HS;
    const int Gmax = cus / (D * NC);
    if (Gmax < 1) continue;
    int G = (int)ceil_div(B, 4);
    if (G > Gmax) G = Gmax;
    const int Bg = (int)ceil_div(B, G);
    if (Bg > 16) continue;
    G = (int)ceil_div(B, Bg);
    const int BQ = Bg <= 4 ? 1 : (Bg <= 8 ? 2 : 4);
    const int KSf = 16 / HS, KSb = 64 / HS;
    const size_t wa = (size_t)16 * Kp * HS;
    const size_t part = (size_t)4 * BQ * 64 * 16;
    const size_t lds_f = wa + (size_t)4 * (1024 + 4 * BQ * KSf * 4) * 4 + part + 16;
    const size_t lds_b = wa + (size_t)4 * (1024 + 4 * BQ * KSb * 4) * 4 + part + 16;
    if (lds_f > 160 * 1024 || lds_b > 160 * 1024) continue;
    pl->HS = HS; pl->NC = NC; pl->G = G; pl->Bg = Bg; pl->BQ = BQ; pl->Kp = Kp;
    pl->lds_fwd = lds_f; pl->lds_bwd = lds_b;
    return true;
  }
  return false;
}

// v3 / v4 (W_hh in registers, bf16 pieces): 16 units per workgroup, H a multiple of 128 with H/128 among the instantiated
// k-step counts (H <= 640), no LDS constraint.  The forward (v3) and the backward (v4) take the same plan; v5 (lstm5.hip) too.
bool make_plan3(int B, int H, int D, int cus, Plan2* pl) {
  if (getenv("RNNT_LSTM_V1") || getenv("RNNT_LSTM_V2")) return false;
  if (H % 128 != 0 || B < 1 || D < 1 || D > 2) return false;
  const int nks = H / 128;
  // H = 768 / 1024: 8 waves x 3 / 4 k-steps (4 waves would need 288 / 384 operand registers per lane).
  // H = 640: 20 units per workgroup (5 blocks), 8 waves, K padded to 768 -> 32 workgroups per sync group, which fit one XCD
  //          (the 16-unit form has 40 and runs the write-through exchange: measured 4.9 / 7.1 us per step vs 3.2 / 2.9)
  if (!(nks >= 1 && nks <= 6) && nks != 8) return false;
  // (its backward keeps one of the six output blocks' W_hh pieces in LDS: with all 216 operand registers per lane it spilled 66-80
  //  and lost to the 16-unit / 4-wave form, 66.0 vs 63.8 ms per c5 step; with 180 it takes 45.5)
  const bool h640 = nks == 5;
  const int MB = h640 ? 5 : 4, HS = 4 * MB;
  const int NC = H / HS;
  const int Gmax = cus / (D * NC);
  if (Gmax < 1) return false;
  int G = (int)ceil_div(B, 4);
  // (as many groups as the chip takes: a step's cost grows with the rows a group exchanges — 16-row instead of 8-row groups at c2:
  //  39.8 vs 32.0 ms per step)
  if (G > Gmax) G = Gmax;
  const int Bg = (int)ceil_div(B, G);
  if (Bg > 16) return false;
  G = (int)ceil_div(B, Bg);
  pl->HS = HS; pl->NC = NC; pl->G = G; pl->Bg = Bg; pl->BQ = Bg <= 4 ? 1 : (Bg <= 8 ? 2 : 4);
  pl->Kp = h640 ? 768 : H;
  pl->MB = MB;
  const int nwv = (nks >= 6 || h640) ? 8 : 4;
  const int ksb = (16 * MB + 31) / 32;
  pl->lds_fwd = (size_t)nwv * MB * 64 * 16 + 16;
  pl->lds_bwd = (size_t)nwv * 64 * 16 + 16 * (32 * ksb + 4) * 4 + 16;
  return true;
}

namespace {

template <typename K>
int launch_persistent(K kernel, const LstmK& k, const Plan& pl, size_t lds, hipStream_t s, const char* what) {
  if (lds > 64 * 1024)
    RNNT_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int per_cu = 0;
  RNNT_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds));
  const int cus = device_cus();
  if (per_cu < 1 || (long)k.D * k.NC > (long)cus * (per_cu < pl.wgs_per_cu ? per_cu : pl.wgs_per_cu)) {
    set_error("%s: %d workgroups cannot be co-resident (%d CUs x %d per CU)", what, k.D * k.NC, cus, per_cu);
    return RNNT_ERR_UNSUPPORTED;
  }
  {
    // algorithmic bytes of the recurrence: gates read+write (4H), c (H), y or dy (H) per (t,b,d) [+ weights once]
    const double per_tb = (k.dy ? (8.0 + 2.0 + 1.0) : (8.0 + 1.0 + 1.0)) * k.H * 4.0;
    ProfScope prof(k.dy ? RNNT_K_LSTM_BWD : RNNT_K_LSTM_FWD,
                   per_tb * k.T * k.B * k.D + 4.0 * 4.0 * k.H * k.H * k.D, s);
    hipLaunchKernelGGL(kernel, dim3(k.D * k.NC), dim3(256), lds, s, k);
  }
  RNNT_CHECK_LAUNCH();
  if (g_launch_log_on.load(std::memory_order_relaxed)) launch_log_note((const void*)kernel, s);
  return RNNT_OK;
}

}  // namespace

int lstm1_fwd_launch(const LstmK& k, const Plan& pl, hipStream_t s) {
  return dispatch<1, 2, 4>(pl.MT, "lstm_fwd MT", [&](auto MT) {
    return dispatch<1, 2, 4>(pl.NT, "lstm_fwd NT", [&](auto NT) {
      return launch_persistent(lstm_fwd_kernel<MT, NT>, k, pl, pl.lds_fwd, s, "lstm_fwd");
    });
  });
}

int lstm1_bwd_launch(const LstmK& k, const Plan& pl, hipStream_t s) {
  return dispatch<1, 2, 4>(pl.MT, "lstm_bwd MT", [&](auto MT) {
    return dispatch<1, 2, 4>(pl.NT, "lstm_bwd NT", [&](auto NT) {
      return launch_persistent(lstm_bwd_kernel<MT, NT>, k, pl, pl.lds_bwd, s, "lstm_bwd");
    });
  });
}

int lstm2_fwd_launch(const LstmK& k, const Plan2& p2, int cell, hipStream_t s) {
  return dispatch<4, 8, 16>(p2.HS, "lstm_fwd2 HS", [&](auto HS) {
    return dispatch<1, 2, 4>(p2.BQ, "lstm_fwd2 BQ", [&](auto BQ) {
      return dispatch<0, 1, 2>(cell_form(cell), "lstm_fwd2 cell", [&](auto C) {
        return launch_persistent2(lstm_fwd2_kernel<HS, BQ, C>, k, p2, p2.lds_fwd, s, "lstm_fwd2");
      });
    });
  });
}

int lstm2_bwd_launch(const LstmK& k, const Plan2& p2, int cell, hipStream_t s) {
  return dispatch<4, 8, 16>(p2.HS, "lstm_bwd2 HS", [&](auto HS) {
    return dispatch<1, 2, 4>(p2.BQ, "lstm_bwd2 BQ", [&](auto BQ) {
      return dispatch<0, 1, 2>(cell_form(cell), "lstm_bwd2 cell", [&](auto C) {
        return launch_persistent2(lstm_bwd2_kernel<HS, BQ, C>, k, p2, p2.lds_bwd, s, "lstm_bwd2");
      });
    });
  });
}

int lstm3_fwd_launch(const LstmK& k, const Plan2& p2, int cell, hipStream_t s) {
  const int nks = p2.Kp / 128, c = cell_form(cell);
  if (p2.MB == 5) {  // H = 640: 5 blocks, 8 waves x 3 k-steps over K padded to 768
    const size_t lds5 = p2.lds_fwd + 8 * 1 * 3 * 3 * 1024;  // one of the five blocks' pieces in LDS
    return dispatch<0, 1, 2>(c, "lstm_fwd3 cell", [&](auto C) {
      return launch_persistent2(lstm_fwd3_kernel<3, C, 8, 5, 1>, k, p2, lds5, s, "lstm_fwd3", 512);
    });
  }
  if (nks == 4) {  // H = 512 forward: 8 waves x 2 k-steps (12.5 vs 13.1 ms per c2 step)
    const size_t lds = (size_t)8 * 4 * 64 * 16 + 16;
    return dispatch<0, 1, 2>(c, "lstm_fwd3 cell", [&](auto C) {
      return launch_persistent2(lstm_fwd3_kernel<2, C, 8>, k, p2, lds, s, "lstm_fwd3", 512);
    });
  }
  if (nks <= 3)
    return dispatch<1, 2, 3>(nks, "lstm_fwd3 k-steps", [&](auto N) {
      return dispatch<0, 1, 2>(c, "lstm_fwd3 cell", [&](auto C) {
        return launch_persistent2(lstm_fwd3_kernel<N, C>, k, p2, p2.lds_fwd, s, "lstm_fwd3");
      });
    });
  // H = 768 / 1024: 8 waves x 3 / 4 k-steps
  return dispatch<3, 4>(p2.Kp / (32 * 8), "lstm_fwd3 k-steps", [&](auto N) {
    const size_t lds8 = p2.lds_fwd + 8 * 1 * N * 3 * 1024;  // one of the four blocks' pieces in LDS
    return dispatch<0, 1, 2>(c, "lstm_fwd3 cell", [&](auto C) {
      return launch_persistent2(lstm_fwd3_kernel<N, C, 8, 4, 1>, k, p2, lds8, s, "lstm_fwd3", 512);
    });
  });
}

int lstm4_bwd_launch(const LstmK& k, const Plan2& p2, int cell, hipStream_t s) {
  const int c = cell_form(cell);
  if (p2.MB == 5)  // H = 640: own 80 gate columns (3 k-steps), 48 output blocks over 8 waves
    return dispatch<1, 2, 4>(p2.BQ, "lstm_bwd4 BQ", [&](auto BQ) {
      return dispatch<0, 1, 2>(c, "lstm_bwd4 cell", [&](auto C) {
        return launch_persistent2(lstm_bwd4_kernel<6, BQ, C, 8, 5, 1>, k, p2, p2.lds_bwd + 8 * 1 * 3 * 3 * 1024, s, "lstm_bwd4", 512);
      });
    });
  if (p2.Kp <= 512)  // (H = 512 backward with 8 waves: 12.9 vs 11.9 ms per c2 step -> stays at 4)
    return dispatch<2, 4, 6, 8>(p2.Kp / (16 * 4), "lstm_bwd4 output blocks", [&](auto NOB) {
      return dispatch<1, 2, 4>(p2.BQ, "lstm_bwd4 BQ", [&](auto BQ) {
        return dispatch<0, 1, 2>(c, "lstm_bwd4 cell", [&](auto C) {
          return launch_persistent2(lstm_bwd4_kernel<NOB, BQ, C>, k, p2, p2.lds_bwd, s, "lstm_bwd4");
        });
      });
    });
  // H = 768 / 1024: 8 waves, 6 / 8 output blocks each
  return dispatch<6, 8>(p2.Kp / (16 * 8), "lstm_bwd4 output blocks", [&](auto NOB) {
    return dispatch<1, 2, 4>(p2.BQ, "lstm_bwd4 BQ", [&](auto BQ) {
      return dispatch<0, 1, 2>(c, "lstm_bwd4 cell", [&](auto C) {
        return launch_persistent2(lstm_bwd4_kernel<NOB, BQ, C, 8, 4, 2>, k, p2, p2.lds_bwd + 8 * 2 * 2 * 3 * 1024, s, "lstm_bwd4", 512);
      });
    });
  });
}

}  // namespace rnnt
