// Attention backward of NlosPoseSformer with the patch queries on the 16-bit matrix cores (hp_sformer_attention_backward_p,
// HP_PRECISION_BF16 / HP_PRECISION_FP16, dim_head 32 and 64).  Two passes, each of which recomputes
// P = exp2(s' - lse') from the forward's saved log-sum-exp (s' = (q log2 e) . k, lse' = lse log2 e): no running maximum, no
// rescale, one v_exp_f32 per score and pass.  Every sum has one owner and a fixed order; there is no float atomic.
//
//   delta      delta = rowsum(dO o O): one wave per token row of the merged (B, Ntok, heads dh) layout, 16-byte loads,
//              the dh / 4 lanes of a head reduced by xor shuffles.
//   key pass   k_attn16_bwd_dkv: a workgroup owns 128 keys (32 per wave, the key on the MFMA lane) of one (b, head, frame)'s key
//              set [nj joint keys | the frame's n patches] and sweeps the frame's patch queries in 32-row tiles.  S = Q K^T and
//              dP = dO V^T (-lse' and -delta are their initial accumulators) come out with the query index in the registers: P
//              and dS = P o (dP - delta) are, converted in place, the B operands of dV^T += dO^T P and dK^T += Q^T dS.  Q and
//              dO tiles go through LDS twice over: by rows ([query][d]) for S and dP, transposed ([d][query slot], as the
//              forward stages V^T) for the two updates.  The MFMA k-slot order of the second pair is the accumulator's row
//              order (slot (half, j) of step t <-> register 8t + j <-> row (j&3) + 8(2t + (j>>2)) + 4 half), as in
//              k_attention_patch_h16.  dK^T / dV^T stay in accumulators over the whole sweep.  Joint keys: one partial per
//              frame, summed in frame order by the fp32 path's kernel.
//   query pass k_attn16_bwd_dq: the forward's dataflow (the query on the lane): S^T = K Q^T, dP^T = V dO^T,
//              dQ^T += K^T dS^T.  dQ has one owner; the price is seven products instead of five.
//   joint      the nj joint queries stay exact fp32: dQ through the fp32 path's split / merge kernels; dK0 and their share
//              of dV in k_attn16_bwd_joint_kv (a key per thread or lane pair, fmaf chains), which runs after the key pass and
//              ADDS into dV.
#include <algorithm>
#include <cfloat>
#include <type_traits>

#include "hp_internal.h"

namespace hp {

using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int BT = 256;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float MASKED = -1.0e30f;   // initial accumulator of a masked score: exp2 of it is 0

template <typename H>
__device__ __forceinline__ f32x16 mfma16(const __attribute__((ext_vector_type(8))) H a, const __attribute__((ext_vector_type(8))) H b,
                                         f32x16 c) {
  if constexpr (std::is_same<H, _Float16>::value) return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// row r of a 32-row tile -> its place in the k order of the second MFMA pair (see the header)
__device__ __forceinline__ int slot_of(int r) { return (r >> 4) * 16 + ((r >> 2) & 1) * 8 + (r & 3) + 4 * ((r >> 3) & 1); }

// 8 consecutive floats (16-byte aligned) -> one 16-bit MFMA fragment, scaled
template <typename H>
__device__ __forceinline__ __attribute__((ext_vector_type(8))) H load_frag(const float* p, float scale) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  __attribute__((ext_vector_type(8))) H f;
  f[0] = (H)(a.x * scale);
  f[1] = (H)(a.y * scale);
  f[2] = (H)(a.z * scale);
  f[3] = (H)(a.w * scale);
  f[4] = (H)(b.x * scale);
  f[5] = (H)(b.y * scale);
  f[6] = (H)(b.z * scale);
  f[7] = (H)(b.w * scale);
  return f;
}

// grid ceil(B Ntok / 4): wave = one token row; delta[(b heads + head) Ntok + tok]
__global__ __launch_bounds__(BT) void k_attn16_bwd_delta(const float* __restrict__ out, const float* __restrict__ dout,
                                                         float* __restrict__ delta, long rows, int heads, int dh, int Ntok) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;   // (whole waves leave: the shuffles below stay inside full waves)
  const int inner4 = heads * dh / 4, g = dh / 4;   // float4 per row, lanes per head: 8 or 16
  const float4* o = (const float4*)(out + row * heads * dh);
  const float4* d = (const float4*)(dout + row * heads * dh);
  const long b = row / Ntok;
  const int tok = (int)(row - b * Ntok);
  for (int i0 = 0; i0 < inner4; i0 += 64) {
    const int i = i0 + lane;
    float s = 0.f;
    if (i < inner4) {
      const float4 a = o[i], c = d[i];
      s = fmaf(a.w, c.w, fmaf(a.z, c.z, fmaf(a.y, c.y, a.x * c.x)));
    }
    for (int x = 1; x < g; x <<= 1) s += __shfl_xor(s, x);
    if (i < inner4 && (lane & (g - 1)) == 0) delta[(b * heads + i / g) * Ntok + tok] = s;
  }
}

// Transposed store of one accumulator block (32 rows of d in the registers, the lane's key / query in the column) as 128-byte
// row pieces: dst_row(c) is the destination row of column c of this wave's tile (nullptr: not stored), d0 the first d.
template <typename F>
__device__ __forceinline__ void store_block(float* os, const f32x16& acc, int lane, int d0, F dst_row) {
  const int col = lane & 31, half = lane >> 5;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) os[col * 33 + (r & 3) + 8 * (r >> 2) + 4 * half] = acc[r];
  __syncthreads();
  for (int i = lane; i < 32 * 32; i += 64) {
    const int c = i >> 5, d = i & 31;
    float* dst = dst_row(c);
    if (dst) dst[d0 + d] = os[c * 33 + d];
  }
}

// grid (ceil((nj + n) / 128), B heads frames)
template <typename H, int DH>
__global__ __launch_bounds__(BT) void k_attn16_bwd_dkv(const float* __restrict__ Q, const float* __restrict__ K,
                                                       const float* __restrict__ V, const float* __restrict__ dout,
                                                       const float* __restrict__ lse, const float* __restrict__ delta,
                                                       float* __restrict__ dK, float* __restrict__ dV, float* __restrict__ ws_dk,
                                                       float* __restrict__ ws_dv, int heads, int Ntok, int nj, int n, int frames) {
  constexpr int ND = DH / 32, KS = DH / 16, LDB = DH + 8, LDT = 32 + 8;
  constexpr int QPR = DH / 4, RPP = BT / QPR, NP = 32 / RPP;   // float4 per row, rows per staging pass, passes
  using h8 = __attribute__((ext_vector_type(8))) H;
  using h4 = __attribute__((ext_vector_type(4))) H;
  __shared__ __attribute__((aligned(16))) H Qh[32 * LDB];   // [query][d], carrying log2 e
  __shared__ __attribute__((aligned(16))) H Gh[32 * LDB];   // dO [query][d]
  __shared__ __attribute__((aligned(16))) H Qt[DH * LDT];   // [d][query slot]
  __shared__ __attribute__((aligned(16))) H Gt[DH * LDT];
  __shared__ __attribute__((aligned(16))) float Ls[32];     // -lse log2 e of the tile's queries (MASKED past n)
  __shared__ __attribute__((aligned(16))) float Ds[32];     // -delta
  __shared__ float os[4][32 * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int bh = blockIdx.y / frames, f = blockIdx.y % frames;
  const int b = bh / heads, head = bh % heads, inner = heads * DH;
  const long bhN = (long)bh * Ntok;
  const int nkeys = nj + n;
  const int key0 = blockIdx.x * 128 + wave * 32;
  const bool active = key0 < nkeys;   // wave-uniform: a wave without keys only helps staging
  const float* Qb = Q + bhN * DH;
  const float* Gb = dout + (long)b * Ntok * inner + head * DH;
  const float* lse_b = lse + bhN;
  const float* delta_b = delta + bhN;
  // B operands of S and dP: this lane's key, d = 16 s + 8 half .. + 7 (a key past the last one re-reads the last: not stored)
  h8 kf[KS], vf[KS];
  {
    const int kj = min(key0 + col, nkeys - 1);
    const long tok = bhN + (kj < nj ? kj : nj + f * n + (kj - nj));
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      kf[s] = load_frag<H>(K + tok * DH + 16 * s + 8 * half, 1.0f);
      vf[s] = load_frag<H>(V + tok * DH + 16 * s + 8 * half, 1.0f);
    }
  }
  f32x16 dk[ND], dv[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk[a][r] = 0.f;
      dv[a][r] = 0.f;
    }
  const int sr = tid / QPR, dq = (tid % QPR) * 4;   // staging: rows sr + RPP u, channels dq .. dq + 3
  float4 qv[NP], gv[NP];
  float lv = 0.f, dl = 0.f;
  auto request = [&](int qt) {
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int tok = nj + f * n + min(qt * 32 + sr + RPP * u, n - 1);   // rows past n: any finite row (masked through Ls)
      qv[u] = *(const float4*)(Qb + (long)tok * DH + dq);
      gv[u] = *(const float4*)(Gb + (long)tok * inner + dq);
    }
    if (tid < 32) {
      const int qi = qt * 32 + tid;
      const int tok = nj + f * n + min(qi, n - 1);
      lv = qi < n ? -lse_b[tok] * LOG2E : MASKED;
      dl = qi < n ? -delta_b[tok] : 0.f;
    }
  };
  const int nqt = (n + 31) / 32;
  request(0);
  for (int qt = 0; qt < nqt; ++qt) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int r = sr + RPP * u, sl = slot_of(r);
      *(h4*)(Qh + r * LDB + dq) = (h4){(H)(qv[u].x * LOG2E), (H)(qv[u].y * LOG2E), (H)(qv[u].z * LOG2E), (H)(qv[u].w * LOG2E)};
      *(h4*)(Gh + r * LDB + dq) = (h4){(H)gv[u].x, (H)gv[u].y, (H)gv[u].z, (H)gv[u].w};
      Qt[(dq + 0) * LDT + sl] = (H)qv[u].x;
      Qt[(dq + 1) * LDT + sl] = (H)qv[u].y;
      Qt[(dq + 2) * LDT + sl] = (H)qv[u].z;
      Qt[(dq + 3) * LDT + sl] = (H)qv[u].w;
      Gt[(dq + 0) * LDT + sl] = (H)gv[u].x;
      Gt[(dq + 1) * LDT + sl] = (H)gv[u].y;
      Gt[(dq + 2) * LDT + sl] = (H)gv[u].z;
      Gt[(dq + 3) * LDT + sl] = (H)gv[u].w;
    }
    if (tid < 32) {
      Ls[tid] = lv;
      Ds[tid] = dl;
    }
    if (qt + 1 < nqt) request(qt + 1);
    __syncthreads();
    if (!active) continue;   // (wave-uniform; the barriers above stay uniform)
    // S'[query][key] - lse' and dP[query][key] - delta: register 4 g + i is query row 8 g + 4 half + i
    f32x16 sacc, pacc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 l4 = *(const float4*)(Ls + 8 * g + 4 * half), d4 = *(const float4*)(Ds + 8 * g + 4 * half);
      sacc[4 * g + 0] = l4.x;
      sacc[4 * g + 1] = l4.y;
      sacc[4 * g + 2] = l4.z;
      sacc[4 * g + 3] = l4.w;
      pacc[4 * g + 0] = d4.x;
      pacc[4 * g + 1] = d4.y;
      pacc[4 * g + 2] = d4.z;
      pacc[4 * g + 3] = d4.w;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      sacc = mfma16<H>(*(const h8*)(Qh + col * LDB + 16 * s + 8 * half), kf[s], sacc);
      pacc = mfma16<H>(*(const h8*)(Gh + col * LDB + 16 * s + 8 * half), vf[s], pacc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sacc[r] = __builtin_amdgcn_exp2f(sacc[r]);   // P (0 for the rows past n)
      pacc[r] *= sacc[r];                          // dS
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      h8 pf, sf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pf[j] = (H)sacc[8 * t + j];
        sf[j] = (H)pacc[8 * t + j];
      }
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        dv[a] = mfma16<H>(*(const h8*)(Gt + (32 * a + col) * LDT + 16 * t + 8 * half), pf, dv[a]);
        dk[a] = mfma16<H>(*(const h8*)(Qt + (32 * a + col) * LDT + 16 * t + 8 * half), sf, dk[a]);
      }
    }
  }
  // a patch key's own rows of dK / dV, or this frame's partial of a joint key
  auto row_of = [&](float* grad, float* ws, int c) -> float* {
    const int kj = key0 + c;
    if (kj >= nkeys) return nullptr;
    return kj >= nj ? grad + (bhN + nj + f * n + (kj - nj)) * DH : ws + (((long)bh * frames + f) * nj + kj) * DH;
  };
#pragma unroll
  for (int a = 0; a < ND; ++a) {
    store_block(os[wave], dk[a], lane, 32 * a, [&](int c) { return row_of(dK, ws_dk, c); });
    store_block(os[wave], dv[a], lane, 32 * a, [&](int c) { return row_of(dV, ws_dv, c); });
  }
}

// grid (ceil(n / 128), B heads frames): dQ of the frame's patch queries
template <typename H, int DH>
__global__ __launch_bounds__(BT) void k_attn16_bwd_dq(const float* __restrict__ Q, const float* __restrict__ K,
                                                      const float* __restrict__ V, const float* __restrict__ dout,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      float* __restrict__ dQ, int heads, int Ntok, int nj, int n, int frames) {
  constexpr int ND = DH / 32, KS = DH / 16, LDB = DH + 8, LDT = 32 + 8;
  constexpr int QPR = DH / 4, RPP = BT / QPR, NP = 32 / RPP;
  using h8 = __attribute__((ext_vector_type(8))) H;
  using h4 = __attribute__((ext_vector_type(4))) H;
  __shared__ __attribute__((aligned(16))) H Kh[32 * LDB];   // [key][d]
  __shared__ __attribute__((aligned(16))) H Vh[32 * LDB];   // [key][d]
  __shared__ __attribute__((aligned(16))) H Kt[DH * LDT];   // [d][key slot]
  __shared__ float os[4][32 * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int bh = blockIdx.y / frames, f = blockIdx.y % frames;
  const int b = bh / heads, head = bh % heads, inner = heads * DH;
  const long bhN = (long)bh * Ntok;
  const int nkeys = nj + n;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const float* Kb = K + bhN * DH;
  const float* Vb = V + bhN * DH;
  // B operands: this lane's query (carrying log2 e) and its dO row; -lse' and -delta are the initial accumulators
  h8 qf[KS], gf[KS];
  float nl, nd;
  {
    const long tok = nj + f * n + min(q0 + col, n - 1);   // a query past n re-reads the last one: not stored
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[s] = load_frag<H>(Q + (bhN + tok) * DH + 16 * s + 8 * half, LOG2E);
      gf[s] = load_frag<H>(dout + ((long)b * Ntok + tok) * inner + head * DH + 16 * s + 8 * half, 1.0f);
    }
    nl = -lse[bhN + tok] * LOG2E;
    nd = -delta[bhN + tok];
  }
  f32x16 dq[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[a][r] = 0.f;
  const int sr = tid / QPR, dc = (tid % QPR) * 4;
  float4 kv[NP], vv[NP];
  auto request = [&](int tile) {
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int kj = min(tile * 32 + sr + RPP * u, nkeys - 1);   // rows past the last key: any finite row (masked below)
      const int tok = kj < nj ? kj : nj + f * n + (kj - nj);
      kv[u] = *(const float4*)(Kb + (long)tok * DH + dc);
      vv[u] = *(const float4*)(Vb + (long)tok * DH + dc);
    }
  };
  const int ntiles = (nkeys + 31) / 32;
  request(0);
  for (int tile = 0; tile < ntiles; ++tile) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int r = sr + RPP * u, sl = slot_of(r);
      *(h4*)(Kh + r * LDB + dc) = (h4){(H)kv[u].x, (H)kv[u].y, (H)kv[u].z, (H)kv[u].w};
      *(h4*)(Vh + r * LDB + dc) = (h4){(H)vv[u].x, (H)vv[u].y, (H)vv[u].z, (H)vv[u].w};
      Kt[(dc + 0) * LDT + sl] = (H)kv[u].x;
      Kt[(dc + 1) * LDT + sl] = (H)kv[u].y;
      Kt[(dc + 2) * LDT + sl] = (H)kv[u].z;
      Kt[(dc + 3) * LDT + sl] = (H)kv[u].w;
    }
    if (tile + 1 < ntiles) request(tile + 1);
    __syncthreads();
    // S'^T[key][query] - lse' and dP^T[key][query] - delta
    f32x16 sacc, pacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sacc[r] = nl;
      pacc[r] = nd;
    }
    if (tile == ntiles - 1 && (nkeys & 31) != 0) {   // ragged last tile (workgroup-uniform): mask the keys past the end
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * half >= nkeys) sacc[r] = MASKED;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      sacc = mfma16<H>(*(const h8*)(Kh + col * LDB + 16 * s + 8 * half), qf[s], sacc);
      pacc = mfma16<H>(*(const h8*)(Vh + col * LDB + 16 * s + 8 * half), gf[s], pacc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) pacc[r] *= __builtin_amdgcn_exp2f(sacc[r]);   // dS^T
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      h8 sf;
#pragma unroll
      for (int j = 0; j < 8; ++j) sf[j] = (H)pacc[8 * t + j];
#pragma unroll
      for (int a = 0; a < ND; ++a) dq[a] = mfma16<H>(*(const h8*)(Kt + (32 * a + col) * LDT + 16 * t + 8 * half), sf, dq[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < ND; ++a)
    store_block(os[wave], dq[a], lane, 32 * a, [&](int c) -> float* {
      const int qi = q0 + c;
      return qi < n ? dQ + (bhN + nj + f * n + qi) * DH : nullptr;
    });
}

// x + (x of the other lane of the pair); quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float pair_sum16(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
}

// The nj joint queries against every key, exact fp32: dK0 (written) and their share of dV (ADDED: runs after the key pass and
// the joint-key sum on the same stream).  A key belongs to one thread (dh 32) or to a lane pair with 32 values of d on each
// lane (dh 64), as in the fp32 path's dkv kernels.  grid (ceil(Ntok / (256 / PAIR)), B heads)
template <int DH>
__global__ __launch_bounds__(BT) void k_attn16_bwd_joint_kv(const float* __restrict__ Q, const float* __restrict__ K0,
                                                            const float* __restrict__ V, const float* __restrict__ dout,
                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                            float* __restrict__ dK0, float* __restrict__ dV, int heads, int Ntok,
                                                            int nj) {
  constexpr int PAIR = DH / 32, HD = 32;
  __shared__ __attribute__((aligned(16))) float Qs[32 * DH];
  __shared__ __attribute__((aligned(16))) float Gs[32 * DH];
  __shared__ float Ls[32], Ds[32];
  const int bh = blockIdx.y, b = bh / heads, head = bh % heads, inner = heads * DH;
  const long bhN = (long)bh * Ntok;
  for (int i = threadIdx.x; i < nj * DH; i += BT) {
    const int r = i / DH, d = i - r * DH;
    Qs[i] = Q[(bhN + r) * DH + d];
    Gs[i] = dout[((long)b * Ntok + r) * inner + head * DH + d];
  }
  if (threadIdx.x < nj) {
    Ls[threadIdx.x] = lse[bhN + threadIdx.x];
    Ds[threadIdx.x] = delta[bhN + threadIdx.x];
  }
  __syncthreads();
  const int d0 = (threadIdx.x % PAIR) * HD;
  const int kj = blockIdx.x * (BT / PAIR) + threadIdx.x / PAIR;
  const bool valid = kj < Ntok;
  const long row = (bhN + min(kj, Ntok - 1)) * DH + d0;   // (a key past the end re-reads the last one: not stored)
  float k[HD], v[HD], dk[HD], dv[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    k[d] = K0[row + d];
    v[d] = V[row + d];
    dk[d] = 0.f;
    dv[d] = 0.f;
  }
  for (int r = 0; r < nj; ++r) {
    const float* q = Qs + r * DH + d0;
    const float* g = Gs + r * DH + d0;
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      s = fmaf(k[d], q[d], s);
      dp = fmaf(v[d], g[d], dp);
    }
    if (PAIR == 2) {
      s = pair_sum16(s);
      dp = pair_sum16(dp);
    }
    const float p = __expf(s - Ls[r]);
    const float ds = p * (dp - Ds[r]);
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      dv[d] = fmaf(p, g[d], dv[d]);
      dk[d] = fmaf(ds, q[d], dk[d]);
    }
  }
  if (valid) {
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      dK0[row + d] = dk[d];
      dV[row + d] += dv[d];
    }
  }
}

// k_attn16_bwd_joint_kv with a key mask (hp_sformer_attention_backward_masked_p), statement for statement: key_mask (B, Ntok),
// one byte per token, nonzero = attendable.  A patch key (index >= nj) whose byte is 0 has P = 0 for every joint query: it is
// left out of the sweep, its dK0 row is written as zeros and nothing is added to its dV row.  The joint tokens' bytes are never
// read.  The same thread / lane pair owns a key and the fmaf chains of an attendable key are the unmasked ones: with an
// all-nonzero mask the bits are k_attn16_bwd_joint_kv's.  Same grid.
template <int DH>
__global__ __launch_bounds__(BT) void k_attn16_bwd_joint_kv_masked(const float* __restrict__ Q, const float* __restrict__ K0,
                                                                   const float* __restrict__ V, const float* __restrict__ dout,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   float* __restrict__ dK0, float* __restrict__ dV, int heads,
                                                                   int Ntok, int nj, const unsigned char* __restrict__ key_mask) {
  constexpr int PAIR = DH / 32, HD = 32;
  __shared__ __attribute__((aligned(16))) float Qs[32 * DH];
  __shared__ __attribute__((aligned(16))) float Gs[32 * DH];
  __shared__ float Ls[32], Ds[32];
  const int bh = blockIdx.y, b = bh / heads, head = bh % heads, inner = heads * DH;
  const long bhN = (long)bh * Ntok;
  for (int i = threadIdx.x; i < nj * DH; i += BT) {
    const int r = i / DH, d = i - r * DH;
    Qs[i] = Q[(bhN + r) * DH + d];
    Gs[i] = dout[((long)b * Ntok + r) * inner + head * DH + d];
  }
  if (threadIdx.x < nj) {
    Ls[threadIdx.x] = lse[bhN + threadIdx.x];
    Ds[threadIdx.x] = delta[bhN + threadIdx.x];
  }
  __syncthreads();
  const int d0 = (threadIdx.x % PAIR) * HD;
  const int kj = blockIdx.x * (BT / PAIR) + threadIdx.x / PAIR;
  const bool valid = kj < Ntok;
  const long row = (bhN + min(kj, Ntok - 1)) * DH + d0;   // (a key past the end re-reads the last one: not stored)
  // does this key take part in the joint queries' soft-max (both lanes of a dh-64 pair share kj)
  const bool att = kj < nj || key_mask[(long)b * Ntok + min(kj, Ntok - 1)] != 0;
  float k[HD], v[HD], dk[HD], dv[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    k[d] = K0[row + d];
    v[d] = V[row + d];
    dk[d] = 0.f;
    dv[d] = 0.f;
  }
  for (int r = 0; att && r < nj; ++r) {   // (the pair exchange inside never crosses this condition)
    const float* q = Qs + r * DH + d0;
    const float* g = Gs + r * DH + d0;
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      s = fmaf(k[d], q[d], s);
      dp = fmaf(v[d], g[d], dp);
    }
    if (PAIR == 2) {
      s = pair_sum16(s);
      dp = pair_sum16(dp);
    }
    const float p = __expf(s - Ls[r]);
    const float ds = p * (dp - Ds[r]);
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      dv[d] = fmaf(p, g[d], dv[d]);
      dk[d] = fmaf(ds, q[d], dk[d]);
    }
  }
  if (valid) {
#pragma unroll
    for (int d = 0; d < HD; ++d) dK0[row + d] = dk[d];
    if (att) {
#pragma unroll
      for (int d = 0; d < HD; ++d) dV[row + d] += dv[d];
    }
  }
}

}  // namespace hp

using namespace hp;

// the same three regions at every precision: delta, the joint keys' per-frame partials, the joint queries' split partials
extern "C" size_t hp_sformer_attention_backward_p_workspace_bytes(int B, int heads, int dh, int Ntok, int num_joints, int frames,
                                                                  int precision) {
  (void)precision;
  return hp_sformer_attention_backward_workspace_bytes(B, heads, dh, Ntok, num_joints, frames);
}

// The 16-bit backward's launches, shared by hp_sformer_attention_backward_p (key_mask null) and
// hp_sformer_attention_backward_masked_p (key_mask set: only the joint queries apply it, so the patch queries' three launches and
// the joint keys' sum are the unmasked ones; the joint queries take k_attn16_bwd_joint_kv_masked and the fp32 path's masked dQ).
// Every argument check comes before the first device call.
static int attn_bwd16(const char* who, const float* Q, const float* K, const float* K0, const float* V, const float* out,
                      const float* dout, const float* lse, float* dQ, float* dK, float* dK0, float* dV, int B, int heads, int dh, int Ntok,
                      int num_joints, int patches_per_frame, int frames, int precision, const unsigned char* key_mask, void* workspace,
                      size_t workspace_bytes, void* stream) {
  HP_REQUIRE(precision == HP_PRECISION_BF16 || precision == HP_PRECISION_FP16, "%s: precision %d not built", who, precision);
  HP_REQUIRE(Q && K && K0 && V && out && dout && lse && dQ && dK && dK0 && dV && workspace, "%s: null argument", who);
  HP_REQUIRE(B > 0 && heads > 0 && frames > 0 && patches_per_frame > 0 && num_joints >= 0 && num_joints <= 32 &&
                 Ntok == num_joints + frames * patches_per_frame,
             "%s: bad token layout", who);
  if (dh != 32 && dh != 64) {
    set_error("%s: dim_head %d not built for the 16-bit backward (32, 64)", who, dh);
    return HP_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < hp_sformer_attention_backward_p_workspace_bytes(B, heads, dh, Ntok, num_joints, frames, precision)) {
    set_error("%s: workspace too small", who);
    return HP_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int BH = B * heads, nj = num_joints, n = patches_per_frame;
  HP_REQUIRE((long)BH * frames < 65536, "%s: B * heads * frames must stay below 65536", who);
  float* delta = (float*)workspace;
  float* ws_dk = delta + (size_t)BH * Ntok;
  float* ws_dv = ws_dk + (size_t)BH * frames * nj * dh;
  float* part = ws_dv + (size_t)BH * frames * nj * dh;
  const long rows = (long)B * Ntok;
  {
    HP_PROF("sformer_attn_bwd16_delta", st);
    hipLaunchKernelGGL(k_attn16_bwd_delta, dim3((unsigned)((rows + 3) / 4)), dim3(BT), 0, st, out, dout, delta, rows, heads, dh, Ntok);
  }
  const dim3 gkv((nj + n + 127) / 128, BH * frames), gq((n + 127) / 128, BH * frames);
  const bool bf = precision == HP_PRECISION_BF16;
  {
    HP_PROF("sformer_attn_bwd16_dkv", st);
#define HP_DKV16(T, D) hipLaunchKernelGGL((k_attn16_bwd_dkv<T, D>), gkv, dim3(BT), 0, st, Q, K, V, dout, lse, delta, dK, dV, ws_dk, ws_dv, heads, Ntok, nj, n, frames)
    if (dh == 64 && bf) HP_DKV16(__bf16, 64);
    else if (dh == 64) HP_DKV16(_Float16, 64);
    else if (bf) HP_DKV16(__bf16, 32);
    else HP_DKV16(_Float16, 32);
#undef HP_DKV16
  }
  {
    HP_PROF("sformer_attn_bwd16_dq", st);
#define HP_DQ16(T, D) hipLaunchKernelGGL((k_attn16_bwd_dq<T, D>), gq, dim3(BT), 0, st, Q, K, V, dout, lse, delta, dQ, heads, Ntok, nj, n, frames)
    if (dh == 64 && bf) HP_DQ16(__bf16, 64);
    else if (dh == 64) HP_DQ16(_Float16, 64);
    else if (bf) HP_DQ16(__bf16, 32);
    else HP_DQ16(_Float16, 32);
#undef HP_DQ16
  }
  if (nj > 0) {
    {
      HP_PROF("sformer_attn_bwd_joint_keys", st);
      launch_attn_bwd_joint_keys(ws_dk, ws_dv, dK, dV, BH, Ntok, dh, nj, frames, st);
    }
    {
      HP_PROF("sformer_attn_bwd16_joint_kv", st);
      const dim3 gj64((Ntok + 127) / 128, BH), gj32((Ntok + 255) / 256, BH);
      if (key_mask && dh == 64) hipLaunchKernelGGL((k_attn16_bwd_joint_kv_masked<64>), gj64, dim3(BT), 0, st, Q, K0, V, dout, lse, delta, dK0, dV, heads, Ntok, nj, key_mask);
      else if (key_mask) hipLaunchKernelGGL((k_attn16_bwd_joint_kv_masked<32>), gj32, dim3(BT), 0, st, Q, K0, V, dout, lse, delta, dK0, dV, heads, Ntok, nj, key_mask);
      else if (dh == 64) hipLaunchKernelGGL((k_attn16_bwd_joint_kv<64>), gj64, dim3(BT), 0, st, Q, K0, V, dout, lse, delta, dK0, dV, heads, Ntok, nj);
      else hipLaunchKernelGGL((k_attn16_bwd_joint_kv<32>), gj32, dim3(BT), 0, st, Q, K0, V, dout, lse, delta, dK0, dV, heads, Ntok, nj);
    }
    {
      HP_PROF("sformer_attn_bwd_dq_joint", st);
      if (key_mask) launch_attn_bwd_dq_joint_masked(Q, K0, V, dout, lse, delta, part, dQ, BH, heads, dh, Ntok, nj, key_mask, st);
      else launch_attn_bwd_dq_joint(Q, K0, V, dout, lse, delta, part, dQ, BH, heads, dh, Ntok, nj, st);
    }
  } else {
    HP_CHECK_HIP(hipMemsetAsync(dK0, 0, sizeof(float) * (size_t)BH * Ntok * dh, st));   // no joint queries: dK0 is exactly zero
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_sformer_attention_backward_p(const float* Q, const float* K, const float* K0, const float* V, const float* out,
                                               const float* dout, const float* lse, float* dQ, float* dK, float* dK0, float* dV, int B,
                                               int heads, int dh, int Ntok, int num_joints, int patches_per_frame, int frames,
                                               int precision, void* workspace, size_t workspace_bytes, void* stream) {
  if (precision == HP_PRECISION_FP32)
    return hp_sformer_attention_backward(Q, K, K0, V, out, dout, lse, dQ, dK, dK0, dV, B, heads, dh, Ntok, num_joints, patches_per_frame,
                                         frames, workspace, workspace_bytes, stream);
  return attn_bwd16("hp_sformer_attention_backward_p", Q, K, K0, V, out, dout, lse, dQ, dK, dK0, dV, B, heads, dh, Ntok, num_joints,
                    patches_per_frame, frames, precision, nullptr, workspace, workspace_bytes, stream);
}

extern "C" size_t hp_sformer_attention_backward_masked_p_workspace_bytes(int B, int heads, int dh, int Ntok, int num_joints, int frames,
                                                                         int precision) {
  return hp_sformer_attention_backward_p_workspace_bytes(B, heads, dh, Ntok, num_joints, frames, precision);
}

// hp_sformer_attention_backward_masked with a precision: FP32 forwards to it; BF16 / FP16 are hp_sformer_attention_backward_p's
// launches with the joint queries' two kernels exchanged for their masked siblings (mask_patch_queries must be 0).
extern "C" int hp_sformer_attention_backward_masked_p(const float* Q, const float* K, const float* K0, const float* V, const float* out,
                                                      const float* dout, const float* lse, float* dQ, float* dK, float* dK0, float* dV,
                                                      int B, int heads, int dh, int Ntok, int num_joints, int patches_per_frame,
                                                      int frames, const unsigned char* key_mask, int mask_patch_queries, int precision,
                                                      void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "hp_sformer_attention_backward_masked_p";
  HP_REQUIRE(key_mask, "%s: null key_mask", who);
  if (precision == HP_PRECISION_FP32)
    return hp_sformer_attention_backward_masked(Q, K, K0, V, out, dout, lse, dQ, dK, dK0, dV, B, heads, dh, Ntok, num_joints,
                                                patches_per_frame, frames, key_mask, mask_patch_queries, workspace, workspace_bytes, stream);
  HP_REQUIRE(precision == HP_PRECISION_BF16 || precision == HP_PRECISION_FP16, "%s: precision %d not built", who, precision);
  if (int rc = attn_masked16_check(who, num_joints, mask_patch_queries)) return rc;
  return attn_bwd16(who, Q, K, K0, V, out, dout, lse, dQ, dK, dK0, dV, B, heads, dh, Ntok, num_joints, patches_per_frame, frames, precision,
                    key_mask, workspace, workspace_bytes, stream);
}
