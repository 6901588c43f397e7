// Attention with a key mask (frame masks of TimeSformer): hp_sformer_attention_masked, hp_sformer_attention_lse_masked,
// hp_sformer_attention_backward_masked and hp_sformer_attention_backward_grouped_masked.
//
// The kernels are the exact-fp32 kernels of sformer_kernels.hip (k_attention, k_attention64) and sformer_backward.hip
// (k_attn_bwd_*), statement for statement, plus key_mask (B, Ntok): one byte per token in the call's token order, nonzero =
// attendable; the joint tokens' bytes are never read (a joint / class key is always attendable, so no key set is empty).
// They are siblings in a file of their own, not a template flag on the originals, so that the unmasked kernels keep their
// code and registers.  Same grids, tiling, key splits and order of accumulation: with an all-true mask every output has the
// unmasked entry's bits.
//   forward   a masked key's score is replaced by -FLT_MAX (a select), which the soft-max already treats as "no key" (the
//             tile tails): it is left out of the maximum, the sum, lse and P V.  The tile's 32 mask bytes are staged next to
//             the K / V tile; a lane takes the bytes of its 16 keys as four 4-byte LDS reads.
//   backward  P = 0 for a masked key: the key's row is left out of the sweep it would have taken part in, so the fmaf chains
//             over the remaining keys / queries are the unmasked ones.  delta, the joint keys' ordered sum and the joint
//             queries' ordered merge are the unmasked launches.
// mask_patch_queries == 0 (TimeSformer's spatial attention): only the joint queries apply the mask; the patch queries'
// forward and dQ launches are then the unmasked kernels themselves.  No float atomics, no scratch, fixed summation order.
#include <algorithm>
#include <cfloat>

#include "hp_internal.h"

namespace hp {

using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int ST = 256;   // threads per block, forward
constexpr int SB = 256;   // threads per block, backward
constexpr int QT = 64;    // query rows per LDS tile of the dkv sweep
constexpr int KT = 64;    // key rows per LDS tile of the dq sweep
constexpr int HD = 32;    // dh 64: d per lane of a pair
constexpr int PB = SB / 2;   // dh 64: keys / queries per workgroup

// the mask bytes of the lane's 16 keys: register r = 4 j + i <-> key i + 8 j + 4 half of the tile <-> byte i of word 2 j + half
__device__ __forceinline__ void attn_mask_words(unsigned (&mw)[4], const unsigned char* ms, int half) {
#pragma unroll
  for (int j = 0; j < 4; ++j) mw[j] = ((const unsigned*)ms)[2 * j + half];
}
__device__ __forceinline__ bool attn_key_masked(const unsigned (&mw)[4], int r) { return ((mw[r >> 2] >> (8 * (r & 3))) & 0xffu) == 0u; }

// ---- forward ------------------------------------------------------------------------------------------------------------
// k_attention (mode 0: patch queries, mode 1: joint queries over key splits) with the key mask
template <int DH, bool LSE>
__global__ __launch_bounds__(ST) void k_attention_masked(const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ V, float* __restrict__ out, int heads, int Ntok, int nj, int n, int frames, int mode,
    float* __restrict__ part, float* __restrict__ lse, const unsigned char* __restrict__ key_mask) {
  constexpr int LD = DH + 1;
  __shared__ float Ks[4][32 * LD];
  __shared__ float Vs[4][32 * LD];
  __shared__ float mrg_m[4][32], mrg_l[4][32];
  __shared__ __attribute__((aligned(16))) unsigned char Ms[4 * 32];   // the staged tiles' mask bytes: region 0, or one region per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  int bh, f = 0;
  if (mode == 0) {
    bh = blockIdx.y / frames;
    f = blockIdx.y % frames;
  } else {
    bh = blockIdx.y;
  }
  const int b = bh / heads, head = bh % heads;
  const float* Qb = Q + (long)bh * Ntok * DH;
  const float* Kb = K + (long)bh * Ntok * DH;
  const float* Vb = V + (long)bh * Ntok * DH;
  const int nkeys = mode == 0 ? nj + n : Ntok;
  const int nq = mode == 0 ? n : nj;
  // this lane's query
  const int qi = mode == 0 ? blockIdx.x * 128 + wave * 32 + col : col;
  const bool qvalid = qi < nq;
  const int qtok = mode == 0 ? nj + f * n + qi : qi;
  float qreg[DH / 2];
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) qreg[s] = qvalid ? Qb[(long)qtok * DH + 2 * s + half] : 0.f;

  f32x16 oacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
  float m = -FLT_MAX, l = 0.f;

  const int ntiles = (nkeys + 31) / 32;
  // joint mode: blockIdx.x is a key split; inside the split the tiles are dealt to the 4 waves
  const int nsplit = mode == 0 ? 1 : (int)gridDim.x;
  const int tiles_per_split = (ntiles + nsplit - 1) / nsplit;
  const int tile0 = mode == 0 ? 0 : (int)blockIdx.x * tiles_per_split;
  const int tile_end = mode == 0 ? ntiles : min(ntiles, tile0 + tiles_per_split);
  const int steps = mode == 0 ? ntiles : (tiles_per_split + 3) / 4;
  for (int it = 0; it < steps; ++it) {
    const int tile = mode == 0 ? it : tile0 + it * 4 + wave;
    __syncthreads();
    if (mode == 0) {  // one tile for the whole block, staged by all 256 threads into region 0
      for (int i = tid; i < 32 * DH; i += ST) {
        const int kr = i / DH, d = i - kr * DH;
        const int kj = tile * 32 + kr;
        float kv = 0.f, vv = 0.f;
        if (kj < nkeys) {
          const int tok = kj < nj ? kj : nj + f * n + (kj - nj);
          kv = Kb[(long)tok * DH + d];
          vv = Vb[(long)tok * DH + d];
        }
        Ks[0][kr * LD + d] = kv;
        Vs[0][kr * LD + d] = vv;
      }
      if (tid < 32) {
        const int kj = tile * 32 + tid;
        Ms[tid] = kj < nj ? 1 : kj < nkeys ? key_mask[(long)b * Ntok + nj + f * n + (kj - nj)] : 0;
      }
    } else {  // every wave stages its own tile
      for (int i = lane; i < 32 * DH; i += 64) {
        const int kr = i / DH, d = i - kr * DH;
        const int kj = tile * 32 + kr;
        float kv = 0.f, vv = 0.f;
        if (kj < nkeys && tile < tile_end) {
          kv = Kb[(long)kj * DH + d];
          vv = Vb[(long)kj * DH + d];
        }
        Ks[wave][kr * LD + d] = kv;
        Vs[wave][kr * LD + d] = vv;
      }
      if (lane < 32) {
        const int kj = tile * 32 + lane;
        Ms[wave * 32 + lane] = kj < nj ? 1 : (kj < nkeys && tile < tile_end) ? key_mask[(long)b * Ntok + kj] : 0;
      }
    }
    __syncthreads();
    const float* ks = mode == 0 ? Ks[0] : Ks[wave];
    const float* vs = mode == 0 ? Vs[0] : Vs[wave];
    if (tile >= tile_end) continue;  // (joint mode tail; barriers above stay uniform)
    // S^T[key][query]
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[col * LD + 2 * s + half], qreg[s], sacc, 0, 0, 0);
    float tm = -FLT_MAX;
    unsigned mw[4];
    attn_mask_words(mw, Ms + (mode == 0 ? 0 : wave * 32), half);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (key >= nkeys) sacc[r] = -FLT_MAX;
      if (attn_key_masked(mw, r)) sacc[r] = -FLT_MAX;
      tm = fmaxf(tm, sacc[r]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    const float mn = fmaxf(m, tm);
    const float alpha = __expf(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pr = sacc[r] > -FLT_MAX ? __expf(sacc[r] - mn) : 0.f;
      sacc[r] = pr;
      ps += pr;
    }
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[r] *= alpha;
    // O^T[d][query] += V^T[d][key] P[key][query], k order = accumulator row order of P
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int key = (s & 3) + 8 * (s >> 2) + 4 * half;
      const float a = col < DH ? vs[key * LD + col] : 0.f;
      oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sacc[s], oacc, 0, 0, 0);
    }
  }

  const int inner = heads * DH;
  if (mode == 0) {
    // normalise, transpose through LDS (region `wave` of Ks is free now) and store 128-byte rows
    __syncthreads();
    float* os = Ks[wave];  // [32 queries][LD]
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = (r & 3) + 8 * (r >> 2) + 4 * half;
      if (d < DH) os[col * LD + d] = oacc[r] * inv;
    }
    if (LSE && qvalid && half == 0) lse[(long)bh * Ntok + qtok] = m + logf(l);
    __syncthreads();
    for (int i = lane; i < 32 * DH; i += 64) {
      const int qr = i / DH, d = i - qr * DH;
      const int q2 = blockIdx.x * 128 + wave * 32 + qr;
      if (q2 < nq) out[((long)b * Ntok + nj + f * n + q2) * inner + head * DH + d] = os[qr * LD + d];
    }
  } else {
    // merge the 4 waves' partial results for the same 32 queries
    __syncthreads();
    float* os = Ks[wave];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = (r & 3) + 8 * (r >> 2) + 4 * half;
      if (d < DH) os[col * LD + d] = oacc[r];
    }
    if (half == 0) {
      mrg_m[wave][col] = m;
      mrg_l[wave][col] = l;
    }
    __syncthreads();
    // partial record of this split for every (query, d): unnormalised O, plus (max, sum) per query
    float* rec = part + ((long)blockIdx.y * nsplit + blockIdx.x) * (32 * (DH + 2));
    for (int i = tid; i < 32 * DH; i += ST) {
      const int qr = i / DH, d = i - qr * DH;
      float M = -FLT_MAX;
      for (int w = 0; w < 4; ++w) M = fmaxf(M, mrg_m[w][qr]);
      float Lsum = 0.f, o = 0.f;
      for (int w = 0; w < 4; ++w) {
        const float sc = mrg_l[w][qr] > 0.f ? __expf(mrg_m[w][qr] - M) : 0.f;
        Lsum += mrg_l[w][qr] * sc;
        o += Ks[w][qr * LD + d] * sc;
      }
      rec[qr * (DH + 2) + d] = o;
      if (d == 0) {
        rec[qr * (DH + 2) + DH] = M;
        rec[qr * (DH + 2) + DH + 1] = Lsum;
      }
    }
  }
}

template <bool LSE>
__global__ __launch_bounds__(ST) void k_attention64_masked(const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ V, float* __restrict__ out, int heads, int Ntok, int nj, int n, int frames, int mode,
    float* __restrict__ part, float* __restrict__ lse, const unsigned char* __restrict__ key_mask) {
  constexpr int DH = 64, LD = DH + 1;
  __shared__ float Ks[4][32 * LD];
  __shared__ __attribute__((aligned(16))) float Vs[32 * DH];   // patch mode: the workgroup's V tile
  __shared__ float mrg_m[4][32], mrg_l[4][32];
  __shared__ __attribute__((aligned(16))) unsigned char Ms[4 * 32];   // the staged tiles' mask bytes: region 0, or one region per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  int bh, f = 0;
  if (mode == 0) {
    bh = blockIdx.y / frames;
    f = blockIdx.y % frames;
  } else {
    bh = blockIdx.y;
  }
  const int b = bh / heads, head = bh % heads;
  const float* Qb = Q + (long)bh * Ntok * DH;
  const float* Kb = K + (long)bh * Ntok * DH;
  const float* Vb = V + (long)bh * Ntok * DH;
  const int nkeys = mode == 0 ? nj + n : Ntok;
  const int nq = mode == 0 ? n : nj;
  const int qi = mode == 0 ? blockIdx.x * 128 + wave * 32 + col : col;
  const bool qvalid = qi < nq;
  const int qtok = mode == 0 ? nj + f * n + qi : qi;
  float qreg[DH / 2];
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) qreg[s] = qvalid ? Qb[(long)qtok * DH + 2 * s + half] : 0.f;

  f32x16 oacc0, oacc1;   // O^T rows d = 0..31 and 32..63
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    oacc0[r] = 0.f;
    oacc1[r] = 0.f;
  }
  float m = -FLT_MAX, l = 0.f;

  const int ntiles = (nkeys + 31) / 32;
  const int nsplit = mode == 0 ? 1 : (int)gridDim.x;
  const int tiles_per_split = (ntiles + nsplit - 1) / nsplit;
  const int tile0 = mode == 0 ? 0 : (int)blockIdx.x * tiles_per_split;
  const int tile_end = mode == 0 ? ntiles : min(ntiles, tile0 + tiles_per_split);
  const int steps = mode == 0 ? ntiles : (tiles_per_split + 3) / 4;
  for (int it = 0; it < steps; ++it) {
    const int tile = mode == 0 ? it : tile0 + it * 4 + wave;
    __syncthreads();
    if (mode == 0) {  // one tile for the whole block: 32 keys x 16 float4 of K and of V, two of each per thread
      for (int i = tid; i < 32 * (DH / 4); i += ST) {
        const int kr = i / (DH / 4), d = (i - kr * (DH / 4)) * 4;
        const int kj = tile * 32 + kr;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (kj < nkeys) {
          const int tok = kj < nj ? kj : nj + f * n + (kj - nj);
          kv = *(const float4*)(Kb + (long)tok * DH + d);
          vv = *(const float4*)(Vb + (long)tok * DH + d);
        }
        float* kd = Ks[0] + kr * LD + d;
        kd[0] = kv.x;
        kd[1] = kv.y;
        kd[2] = kv.z;
        kd[3] = kv.w;
        *(float4*)(Vs + kr * DH + d) = vv;
      }
      if (tid < 32) {
        const int kj = tile * 32 + tid;
        Ms[tid] = kj < nj ? 1 : kj < nkeys ? key_mask[(long)b * Ntok + nj + f * n + (kj - nj)] : 0;
      }
    } else {  // every wave stages the K rows of its own tile
      for (int i = lane; i < 32 * (DH / 4); i += 64) {
        const int kr = i / (DH / 4), d = (i - kr * (DH / 4)) * 4;
        const int kj = tile * 32 + kr;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kj < nkeys && tile < tile_end) kv = *(const float4*)(Kb + (long)kj * DH + d);
        float* kd = Ks[wave] + kr * LD + d;
        kd[0] = kv.x;
        kd[1] = kv.y;
        kd[2] = kv.z;
        kd[3] = kv.w;
      }
      if (lane < 32) {
        const int kj = tile * 32 + lane;
        Ms[wave * 32 + lane] = kj < nj ? 1 : (kj < nkeys && tile < tile_end) ? key_mask[(long)b * Ntok + kj] : 0;
      }
    }
    __syncthreads();
    const float* ks = mode == 0 ? Ks[0] : Ks[wave];
    if (tile >= tile_end) continue;  // (joint mode tail; barriers above stay uniform)
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[col * LD + 2 * s + half], qreg[s], sacc, 0, 0, 0);
    float tm = -FLT_MAX;
    unsigned mw[4];
    attn_mask_words(mw, Ms + (mode == 0 ? 0 : wave * 32), half);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (key >= nkeys) sacc[r] = -FLT_MAX;
      if (attn_key_masked(mw, r)) sacc[r] = -FLT_MAX;
      tm = fmaxf(tm, sacc[r]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    const float mn = fmaxf(m, tm);
    const float alpha = __expf(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pr = sacc[r] > -FLT_MAX ? __expf(sacc[r] - mn) : 0.f;
      sacc[r] = pr;
      ps += pr;
    }
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      oacc0[r] *= alpha;
      oacc1[r] *= alpha;
    }
    // O^T[d][query] += V^T[d][key] P[key][query], k order = accumulator row order of P; d = col and 32 + col
    if (mode == 0) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int key = (s & 3) + 8 * (s >> 2) + 4 * half;
        oacc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * DH + col], sacc[s], oacc0, 0, 0, 0);
        oacc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * DH + 32 + col], sacc[s], oacc1, 0, 0, 0);
      }
    } else {
      float va[16], vb[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int kj = tile * 32 + (s & 3) + 8 * (s >> 2) + 4 * half;
        va[s] = kj < nkeys ? Vb[(long)kj * DH + col] : 0.f;
        vb[s] = kj < nkeys ? Vb[(long)kj * DH + 32 + col] : 0.f;
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        oacc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[s], sacc[s], oacc0, 0, 0, 0);
        oacc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb[s], sacc[s], oacc1, 0, 0, 0);
      }
    }
  }

  const int inner = heads * DH;
  __syncthreads();
  float* os = Ks[wave];  // [32 queries][LD]; every K region is free now
  if (mode == 0) {
    // normalise, transpose through LDS and store 256-byte rows
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = (r & 3) + 8 * (r >> 2) + 4 * half;
      os[col * LD + d] = oacc0[r] * inv;
      os[col * LD + 32 + d] = oacc1[r] * inv;
    }
    if (LSE && qvalid && half == 0) lse[(long)bh * Ntok + qtok] = m + logf(l);
    __syncthreads();
    for (int i = lane; i < 32 * DH; i += 64) {
      const int qr = i / DH, d = i - qr * DH;
      const int q2 = blockIdx.x * 128 + wave * 32 + qr;
      if (q2 < nq) out[((long)b * Ntok + nj + f * n + q2) * inner + head * DH + d] = os[qr * LD + d];
    }
  } else {
    // merge the 4 waves' partial results for the same 32 queries
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = (r & 3) + 8 * (r >> 2) + 4 * half;
      os[col * LD + d] = oacc0[r];
      os[col * LD + 32 + d] = oacc1[r];
    }
    if (half == 0) {
      mrg_m[wave][col] = m;
      mrg_l[wave][col] = l;
    }
    __syncthreads();
    float* rec = part + ((long)blockIdx.y * nsplit + blockIdx.x) * (32 * (DH + 2));
    for (int i = tid; i < 32 * DH; i += ST) {
      const int qr = i / DH, d = i - qr * DH;
      float M = -FLT_MAX;
      for (int w = 0; w < 4; ++w) M = fmaxf(M, mrg_m[w][qr]);
      float Lsum = 0.f, o = 0.f;
      for (int w = 0; w < 4; ++w) {
        const float sc = mrg_l[w][qr] > 0.f ? __expf(mrg_m[w][qr] - M) : 0.f;
        Lsum += mrg_l[w][qr] * sc;
        o += Ks[w][qr * LD + d] * sc;
      }
      rec[qr * (DH + 2) + d] = o;
      if (d == 0) {
        rec[qr * (DH + 2) + DH] = M;
        rec[qr * (DH + 2) + DH + 1] = Lsum;
      }
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// Stage `rows` query rows (token index tok0 + r) of one (b, head) into LDS: Q (bh-major), dO (merged heads), lse, delta.
template <int DH>
__device__ __forceinline__ void stage_queries(float* Qs, float* Gs, float* Ls, float* Ds, const float* Qb, const float* dout_b,
                                              const float* lse_b, const float* delta_b, int inner, int head, int tok0, int rows) {
  for (int i = threadIdx.x; i < QT * DH; i += SB) {
    const int r = i / DH, d = i - r * DH;
    float q = 0.f, g = 0.f;
    if (r < rows) {
      q = Qb[(long)(tok0 + r) * DH + d];
      g = dout_b[(long)(tok0 + r) * inner + head * DH + d];
    }
    Qs[i] = q;
    Gs[i] = g;
  }
  if (threadIdx.x < QT) {
    const int r = threadIdx.x;
    Ls[r] = r < rows ? lse_b[tok0 + r] : 0.f;
    Ds[r] = r < rows ? delta_b[tok0 + r] : 0.f;
  }
}

// One query row against this thread's key: p = exp(s - lse), dp = dO . v, ds = p (dp - delta); dv += p dO, dk += ds q.
template <int DH>
__device__ __forceinline__ void dkv_row(const float* q, const float* g, float lse, float delta, const float (&k)[DH],
                                        const float (&v)[DH], float (&dk)[DH], float (&dv)[DH]) {
  float s = 0.f, dp = 0.f;
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    s = fmaf(k[d], q[d], s);
    dp = fmaf(v[d], g[d], dp);
  }
  const float p = __expf(s - lse);
  const float ds = p * (dp - delta);
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    dv[d] = fmaf(p, g[d], dv[d]);
    dk[d] = fmaf(ds, q[d], dk[d]);
  }
}

template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_dkv_masked(const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ K0, const float* __restrict__ V, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dK, float* __restrict__ dK0, float* __restrict__ dV,
    float* __restrict__ ws_dk, float* __restrict__ ws_dv, int heads, int Ntok, int nj, int n, int frames,
    const unsigned char* __restrict__ key_mask, int mask_patch_queries) {
  __shared__ __attribute__((aligned(16))) float Qs[QT * DH];
  __shared__ __attribute__((aligned(16))) float Gs[QT * DH];
  __shared__ float Ls[QT], Ds[QT];
  const int bh = blockIdx.y / frames, f = blockIdx.y % frames;
  const int b = bh / heads, head = bh % heads, inner = heads * DH;
  const int kj = blockIdx.x * SB + threadIdx.x;
  const bool valid = kj < nj + n;
  const int tok = kj < nj ? kj : nj + f * n + (kj - nj);
  const long bhN = (long)bh * Ntok;
  const float* Qb = Q + bhN * DH;
  const float* dout_b = dout + (long)b * Ntok * inner;
  const float* lse_b = lse + bhN;
  const float* delta_b = delta + bhN;
  // does this key take part in the joint queries' / the patch queries' soft-max (both lanes of a dh-64 pair share kj)
  const bool jatt = kj < nj || (valid && key_mask[(long)b * Ntok + tok] != 0);
  const bool patt = jatt || !mask_patch_queries;
  float k[DH], v[DH], dk[DH], dv[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    k[d] = valid ? K[(bhN + tok) * DH + d] : 0.f;
    v[d] = valid ? V[(bhN + tok) * DH + d] : 0.f;
    dk[d] = 0.f;
    dv[d] = 0.f;
  }
  // the frame's n patch queries
  for (int q0 = 0; q0 < n; q0 += QT) {
    const int rows = min(QT, n - q0);
    __syncthreads();
    stage_queries<DH>(Qs, Gs, Ls, Ds, Qb, dout_b, lse_b, delta_b, inner, head, nj + f * n + q0, rows);
    __syncthreads();
    if (patt)
      for (int r = 0; r < rows; ++r) dkv_row<DH>(Qs + r * DH, Gs + r * DH, Ls[r], Ds[r], k, v, dk, dv);
  }
  // patch-query part of dK: a patch key's own row, or this frame's partial of a joint key
  if (valid) {
    float* dst = kj >= nj ? dK + (bhN + tok) * DH : ws_dk + (((long)bh * frames + f) * nj + kj) * DH;
#pragma unroll
    for (int d = 0; d < DH; ++d) dst[d] = dk[d];
  }
  // the nj joint queries attend to the keys BEFORE the rotary embedding (K0); a joint key takes them once (frame 0)
  const bool joint = valid && (kj >= nj || f == 0);
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    k[d] = joint ? K0[(bhN + tok) * DH + d] : 0.f;
    dk[d] = 0.f;
  }
  if (nj > 0) {
    __syncthreads();
    stage_queries<DH>(Qs, Gs, Ls, Ds, Qb, dout_b, lse_b, delta_b, inner, head, 0, nj);
    __syncthreads();
    if (joint && jatt)
      for (int r = 0; r < nj; ++r) dkv_row<DH>(Qs + r * DH, Gs + r * DH, Ls[r], Ds[r], k, v, dk, dv);
  }
  if (joint) {
#pragma unroll
    for (int d = 0; d < DH; ++d) dK0[(bhN + tok) * DH + d] = dk[d];
  }
  if (valid) {
    float* dst = kj >= nj ? dV + (bhN + tok) * DH : ws_dv + (((long)bh * frames + f) * nj + kj) * DH;
#pragma unroll
    for (int d = 0; d < DH; ++d) dst[d] = dv[d];
  }
}

template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_dq_patch_masked(const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ V, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dQ, int heads, int Ntok, int nj, int n, int frames,
    const unsigned char* __restrict__ key_mask) {
  __shared__ __attribute__((aligned(16))) float Ks[KT * DH];
  __shared__ __attribute__((aligned(16))) float Vs[KT * DH];
  __shared__ __attribute__((aligned(16))) unsigned char Ms[KT];   // the tile's mask bytes
  const int bh = blockIdx.y / frames, f = blockIdx.y % frames;
  const int b = bh / heads, head = bh % heads, inner = heads * DH;
  const int qi = blockIdx.x * SB + threadIdx.x;
  const bool valid = qi < n;
  const int tok = nj + f * n + min(qi, n - 1);
  const long bhN = (long)bh * Ntok;
  float q[DH], g[DH], dq[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    q[d] = Q[(bhN + tok) * DH + d];
    g[d] = dout[((long)b * Ntok + tok) * inner + head * DH + d];
    dq[d] = 0.f;
  }
  const float L = lse[bhN + tok], Dl = delta[bhN + tok];
  const int nkeys = nj + n;
  for (int k0 = 0; k0 < nkeys; k0 += KT) {
    const int rows = min(KT, nkeys - k0);
    __syncthreads();
    for (int i = threadIdx.x; i < KT * DH; i += SB) {
      const int r = i / DH, d = i - r * DH;
      const int kj = k0 + r;
      float kv = 0.f, vv = 0.f;
      if (r < rows) {
        const int kt = kj < nj ? kj : nj + f * n + (kj - nj);
        kv = K[(bhN + kt) * DH + d];
        vv = V[(bhN + kt) * DH + d];
      }
      Ks[i] = kv;
      Vs[i] = vv;
    }
    if (threadIdx.x < KT) {
      const int r = threadIdx.x, kj = k0 + r;
      Ms[r] = kj < nj ? 1 : r < rows ? key_mask[(long)b * Ntok + nj + f * n + (kj - nj)] : 0;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      if (Ms[r] == 0) continue;
      const float* kr = Ks + r * DH;
      const float* vr = Vs + r * DH;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        s = fmaf(q[d], kr[d], s);
        dp = fmaf(g[d], vr[d], dp);
      }
      const float ds = __expf(s - L) * (dp - Dl);
#pragma unroll
      for (int d = 0; d < DH; ++d) dq[d] = fmaf(ds, kr[d], dq[d]);
    }
  }
  if (valid) {
#pragma unroll
    for (int d = 0; d < DH; ++d) dQ[(bhN + tok) * DH + d] = dq[d];
  }
}

template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_dq_joint_masked(const float* __restrict__ Q, const float* __restrict__ K0,
    const float* __restrict__ V, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ part, int heads, int Ntok, int nj, const unsigned char* __restrict__ key_mask) {
  __shared__ float red[8][32][DH + 1];
  const int bh = blockIdx.y, b = bh / heads, head = bh % heads, inner = heads * DH;
  const int qr = threadIdx.x & 31, sub = threadIdx.x >> 5;
  const int nsplit = gridDim.x, per = (Ntok + nsplit - 1) / nsplit;
  const int kbeg = blockIdx.x * per, kend = min(Ntok, kbeg + per);
  const long bhN = (long)bh * Ntok;
  float dq[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) dq[d] = 0.f;
  if (qr < nj) {
    float q[DH], g[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      q[d] = Q[(bhN + qr) * DH + d];
      g[d] = dout[((long)b * Ntok + qr) * inner + head * DH + d];
    }
    const float L = lse[bhN + qr], Dl = delta[bhN + qr];
    for (int kj = kbeg + sub; kj < kend; kj += 8) {
      if (kj >= nj && key_mask[(long)b * Ntok + kj] == 0) continue;
      const float* kr = K0 + (bhN + kj) * DH;
      const float* vr = V + (bhN + kj) * DH;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        s = fmaf(q[d], kr[d], s);
        dp = fmaf(g[d], vr[d], dp);
      }
      const float ds = __expf(s - L) * (dp - Dl);
#pragma unroll
      for (int d = 0; d < DH; ++d) dq[d] = fmaf(ds, kr[d], dq[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < DH; ++d) red[sub][qr][d] = dq[d];
  __syncthreads();
  float* rec = part + ((long)bh * nsplit + blockIdx.x) * 32 * DH;
  for (int i = threadIdx.x; i < 32 * DH; i += SB) {
    const int r = i / DH, d = i - r * DH;
    float s = 0.f;
    for (int u = 0; u < 8; ++u) s += red[u][r][d];
    rec[i] = s;
  }
}

// x + (x of the other lane of the pair); quad_perm [1, 0, 3, 2].  Both lanes of a pair are always active together.
__device__ __forceinline__ float pair_sum(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
}

__device__ __forceinline__ void dkv_row_pair(const float* q, const float* g, float lse, float delta, const float (&k)[HD],
                                             const float (&v)[HD], float (&dk)[HD], float (&dv)[HD]) {
  float s = 0.f, dp = 0.f;
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    s = fmaf(k[d], q[d], s);
    dp = fmaf(v[d], g[d], dp);
  }
  s = pair_sum(s);
  dp = pair_sum(dp);
  const float p = __expf(s - lse);
  const float ds = p * (dp - delta);
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    dv[d] = fmaf(p, g[d], dv[d]);
    dk[d] = fmaf(ds, q[d], dk[d]);
  }
}

__global__ __launch_bounds__(SB) void k_attn_bwd_dkv64_masked(const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ K0, const float* __restrict__ V, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dK, float* __restrict__ dK0, float* __restrict__ dV,
    float* __restrict__ ws_dk, float* __restrict__ ws_dv, int heads, int Ntok, int nj, int n, int frames,
    const unsigned char* __restrict__ key_mask, int mask_patch_queries) {
  constexpr int DH = 64;
  __shared__ __attribute__((aligned(16))) float Qs[QT * DH];
  __shared__ __attribute__((aligned(16))) float Gs[QT * DH];
  __shared__ float Ls[QT], Ds[QT];
  const int bh = blockIdx.y / frames, f = blockIdx.y % frames;
  const int b = bh / heads, head = bh % heads, inner = heads * DH;
  const int hf = threadIdx.x & 1, d0 = hf * HD;
  const int kj = blockIdx.x * PB + (threadIdx.x >> 1);
  const bool valid = kj < nj + n;
  const int tok = kj < nj ? kj : nj + f * n + (kj - nj);
  const long bhN = (long)bh * Ntok;
  const float* Qb = Q + bhN * DH;
  const float* dout_b = dout + (long)b * Ntok * inner;
  const float* lse_b = lse + bhN;
  const float* delta_b = delta + bhN;
  // does this key take part in the joint queries' / the patch queries' soft-max (both lanes of a dh-64 pair share kj)
  const bool jatt = kj < nj || (valid && key_mask[(long)b * Ntok + tok] != 0);
  const bool patt = jatt || !mask_patch_queries;
  float k[HD], v[HD], dk[HD], dv[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    k[d] = valid ? K[(bhN + tok) * DH + d0 + d] : 0.f;
    v[d] = valid ? V[(bhN + tok) * DH + d0 + d] : 0.f;
    dk[d] = 0.f;
    dv[d] = 0.f;
  }
  // the frame's n patch queries
  for (int q0 = 0; q0 < n; q0 += QT) {
    const int rows = min(QT, n - q0);
    __syncthreads();
    stage_queries<DH>(Qs, Gs, Ls, Ds, Qb, dout_b, lse_b, delta_b, inner, head, nj + f * n + q0, rows);
    __syncthreads();
    if (patt)
      for (int r = 0; r < rows; ++r) dkv_row_pair(Qs + r * DH + d0, Gs + r * DH + d0, Ls[r], Ds[r], k, v, dk, dv);
  }
  // patch-query part of dK: a patch key's own row, or this frame's partial of a joint key
  if (valid) {
    float* dst = (kj >= nj ? dK + (bhN + tok) * DH : ws_dk + (((long)bh * frames + f) * nj + kj) * DH) + d0;
#pragma unroll
    for (int d = 0; d < HD; ++d) dst[d] = dk[d];
  }
  // the nj joint queries attend to the keys BEFORE the rotary embedding (K0); a joint key takes them once (frame 0)
  const bool joint = valid && (kj >= nj || f == 0);
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    k[d] = joint ? K0[(bhN + tok) * DH + d0 + d] : 0.f;
    dk[d] = 0.f;
  }
  if (nj > 0) {
    __syncthreads();
    stage_queries<DH>(Qs, Gs, Ls, Ds, Qb, dout_b, lse_b, delta_b, inner, head, 0, nj);
    __syncthreads();
    if (joint && jatt)   // (both lanes of a pair share kj: the exchange inside never crosses this branch)
      for (int r = 0; r < nj; ++r) dkv_row_pair(Qs + r * DH + d0, Gs + r * DH + d0, Ls[r], Ds[r], k, v, dk, dv);
  }
  if (joint) {
#pragma unroll
    for (int d = 0; d < HD; ++d) dK0[(bhN + tok) * DH + d0 + d] = dk[d];
  }
  if (valid) {
    float* dst = (kj >= nj ? dV + (bhN + tok) * DH : ws_dv + (((long)bh * frames + f) * nj + kj) * DH) + d0;
#pragma unroll
    for (int d = 0; d < HD; ++d) dst[d] = dv[d];
  }
}

__global__ __launch_bounds__(SB) void k_attn_bwd_dq_patch64_masked(const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ V, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dQ, int heads, int Ntok, int nj, int n, int frames,
    const unsigned char* __restrict__ key_mask) {
  constexpr int DH = 64;
  __shared__ __attribute__((aligned(16))) float Ks[KT * DH];
  __shared__ __attribute__((aligned(16))) float Vs[KT * DH];
  __shared__ __attribute__((aligned(16))) unsigned char Ms[KT];   // the tile's mask bytes
  const int bh = blockIdx.y / frames, f = blockIdx.y % frames;
  const int b = bh / heads, head = bh % heads, inner = heads * DH;
  const int hf = threadIdx.x & 1, d0 = hf * HD;
  const int qi = blockIdx.x * PB + (threadIdx.x >> 1);
  const bool valid = qi < n;
  const int tok = nj + f * n + min(qi, n - 1);
  const long bhN = (long)bh * Ntok;
  float q[HD], g[HD], dq[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    q[d] = Q[(bhN + tok) * DH + d0 + d];
    g[d] = dout[((long)b * Ntok + tok) * inner + head * DH + d0 + d];
    dq[d] = 0.f;
  }
  const float L = lse[bhN + tok], Dl = delta[bhN + tok];
  const int nkeys = nj + n;
  for (int k0 = 0; k0 < nkeys; k0 += KT) {
    const int rows = min(KT, nkeys - k0);
    __syncthreads();
    // 64 rows x 16 float4 of K and of V: four of each per thread, all eight loads in flight before the first LDS store (a tile
    // is twice the bytes of the dh-32 kernel's for half the queries)
    float4 kq[4], vq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = threadIdx.x + u * SB, r = i / (DH / 4), d = (i - r * (DH / 4)) * 4;
      const int kj = k0 + r;
      kq[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      vq[u] = kq[u];
      if (r < rows) {
        const int kt = kj < nj ? kj : nj + f * n + (kj - nj);
        kq[u] = *(const float4*)(K + (bhN + kt) * DH + d);
        vq[u] = *(const float4*)(V + (bhN + kt) * DH + d);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = threadIdx.x + u * SB;
      *(float4*)(Ks + 4 * i) = kq[u];
      *(float4*)(Vs + 4 * i) = vq[u];
    }
    if (threadIdx.x < KT) {
      const int r = threadIdx.x, kj = k0 + r;
      Ms[r] = kj < nj ? 1 : r < rows ? key_mask[(long)b * Ntok + nj + f * n + (kj - nj)] : 0;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      if (Ms[r] == 0) continue;
      // The K half-row is read ONCE, as eight 16-byte reads, and kept for the dQ update.  The two lanes of a pair read rows
      // 128 bytes apart: the same bank under the 32-bank rule of the 4- and 8-byte LDS reads (a 2-way conflict the dh-32
      // kernel, whose wave reads one address, never has), distinct banks under the 64-bank rule of ds_read_b128.
      const float4* kr = (const float4*)(Ks + r * DH + d0);
      const float4* vr = (const float4*)(Vs + r * DH + d0);
      float4 kk[HD / 4];
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int u = 0; u < HD / 4; ++u) {
        kk[u] = kr[u];
        const float4 vv = vr[u];
        s = fmaf(q[4 * u + 0], kk[u].x, s);
        s = fmaf(q[4 * u + 1], kk[u].y, s);
        s = fmaf(q[4 * u + 2], kk[u].z, s);
        s = fmaf(q[4 * u + 3], kk[u].w, s);
        dp = fmaf(g[4 * u + 0], vv.x, dp);
        dp = fmaf(g[4 * u + 1], vv.y, dp);
        dp = fmaf(g[4 * u + 2], vv.z, dp);
        dp = fmaf(g[4 * u + 3], vv.w, dp);
      }
      s = pair_sum(s);
      dp = pair_sum(dp);
      const float ds = __expf(s - L) * (dp - Dl);
#pragma unroll
      for (int u = 0; u < HD / 4; ++u) {
        dq[4 * u + 0] = fmaf(ds, kk[u].x, dq[4 * u + 0]);
        dq[4 * u + 1] = fmaf(ds, kk[u].y, dq[4 * u + 1]);
        dq[4 * u + 2] = fmaf(ds, kk[u].z, dq[4 * u + 2]);
        dq[4 * u + 3] = fmaf(ds, kk[u].w, dq[4 * u + 3]);
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int d = 0; d < HD; ++d) dQ[(bhN + tok) * DH + d0 + d] = dq[d];
  }
}

__global__ __launch_bounds__(SB) void k_attn_bwd_dq_joint64_masked(const float* __restrict__ Q, const float* __restrict__ K0,
    const float* __restrict__ V, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ part, int heads, int Ntok, int nj, const unsigned char* __restrict__ key_mask) {
  constexpr int DH = 64;
  __shared__ float red[4][32][DH + 1];
  const int bh = blockIdx.y, b = bh / heads, head = bh % heads, inner = heads * DH;
  const int hf = threadIdx.x & 1, d0 = hf * HD, qr = (threadIdx.x >> 1) & 31, sub = threadIdx.x >> 6;
  const int nsplit = gridDim.x, per = (Ntok + nsplit - 1) / nsplit;
  const int kbeg = blockIdx.x * per, kend = min(Ntok, kbeg + per);
  const long bhN = (long)bh * Ntok;
  float dq[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) dq[d] = 0.f;
  if (qr < nj) {
    float q[HD], g[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      q[d] = Q[(bhN + qr) * DH + d0 + d];
      g[d] = dout[((long)b * Ntok + qr) * inner + head * DH + d0 + d];
    }
    const float L = lse[bhN + qr], Dl = delta[bhN + qr];
    for (int kj = kbeg + sub; kj < kend; kj += 4) {
      // (both lanes of a pair share kj: the exchange below never crosses this branch)
      if (kj >= nj && key_mask[(long)b * Ntok + kj] == 0) continue;
      const float* kr = K0 + (bhN + kj) * DH + d0;
      const float* vr = V + (bhN + kj) * DH + d0;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) {
        s = fmaf(q[d], kr[d], s);
        dp = fmaf(g[d], vr[d], dp);
      }
      s = pair_sum(s);
      dp = pair_sum(dp);
      const float ds = __expf(s - L) * (dp - Dl);
#pragma unroll
      for (int d = 0; d < HD; ++d) dq[d] = fmaf(ds, kr[d], dq[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < HD; ++d) red[sub][qr][d0 + d] = dq[d];
  __syncthreads();
  float* rec = part + ((long)bh * nsplit + blockIdx.x) * 32 * DH;
  for (int i = threadIdx.x; i < 32 * DH; i += SB) {
    const int r = i / DH, d = i - r * DH;
    float s = 0.f;
    for (int u = 0; u < 4; ++u) s += red[u][r][d];
    rec[i] = s;
  }
}

template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_grouped_masked(const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ K0, const float* __restrict__ V, const float* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, float* __restrict__ dQ, float* __restrict__ dK, float* __restrict__ dK0,
    float* __restrict__ dV, float* __restrict__ ws_dk, float* __restrict__ ws_dv, int heads, int Ntok, int nj, int n,
    int groups, int G, int wg_per_bh, const unsigned char* __restrict__ key_mask, int mask_patch_queries) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int rmax = G * n;
  float* A = lds;                 // phase 1: Q rows of the patch queries;  phase 2: K rows of the patch keys
  float* Bm = A + rmax * DH;      // phase 1: dO rows;                      phase 2: V rows
  float* Ls = Bm + rmax * DH;
  float* Ds = Ls + rmax;
  float* Aj = Ds + rmax;          // phase 1: Q of the joint queries;       phase 2: K of the joint keys
  float* Bj = Aj + nj * DH;       // phase 1: dO of the joint queries;      phase 2: V of the joint keys
  float* Lj = Bj + nj * DH;
  float* Dj = Lj + nj;
  unsigned char* Mk = (unsigned char*)(Dj + nj);   // the patch rows' mask bytes
  const int bh = blockIdx.x / wg_per_bh, g0 = (blockIdx.x % wg_per_bh) * G;
  const int Gw = min(G, groups - g0), rows = Gw * n, per = nj + n;
  const int b = bh / heads, head = bh % heads, inner = heads * DH;
  const long bhN = (long)bh * Ntok;
  const int tok0 = nj + g0 * n;
  const float* Qb = Q + bhN * DH;
  const float* dout_b = dout + (long)b * Ntok * inner;
  for (int i = threadIdx.x; i < rows * DH; i += SB) {
    const int r = i / DH, d = i - r * DH;
    A[i] = Qb[(long)(tok0 + r) * DH + d];
    Bm[i] = dout_b[(long)(tok0 + r) * inner + head * DH + d];
  }
  for (int i = threadIdx.x; i < nj * DH; i += SB) {
    const int r = i / DH, d = i - r * DH;
    Aj[i] = Qb[(long)r * DH + d];
    Bj[i] = dout_b[(long)r * inner + head * DH + d];
  }
  for (int r = threadIdx.x; r < rows; r += SB) {
    Ls[r] = lse[bhN + tok0 + r];
    Ds[r] = delta[bhN + tok0 + r];
  }
  for (int r = threadIdx.x; r < nj; r += SB) {
    Lj[r] = lse[bhN + r];
    Dj[r] = delta[bhN + r];
  }
  for (int r = threadIdx.x; r < rows; r += SB) Mk[r] = key_mask[(long)b * Ntok + tok0 + r];
  __syncthreads();
  // ---- phase 1: dK, dK0, dV
  {
    const int t = threadIdx.x;
    const bool valid = t < Gw * per;
    const int gl = valid ? t / per : 0, kj = valid ? t - gl * per : 0, g = g0 + gl;
    const int tok = kj < nj ? kj : nj + g * n + (kj - nj);
    // does this key take part in the joint queries' / the patch queries' soft-max (both lanes of a dh-64 pair share kj)
    const bool jatt = kj < nj || (valid && Mk[gl * n + (kj - nj)] != 0);
    const bool patt = jatt || !mask_patch_queries;
    float k[DH], v[DH], dk[DH], dv[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      k[d] = valid ? K[(bhN + tok) * DH + d] : 0.f;
      v[d] = valid ? V[(bhN + tok) * DH + d] : 0.f;
      dk[d] = 0.f;
      dv[d] = 0.f;
    }
    if (valid && patt)
      for (int r = 0; r < n; ++r) {
        const int row = gl * n + r;
        dkv_row<DH>(A + row * DH, Bm + row * DH, Ls[row], Ds[row], k, v, dk, dv);
      }
    if (valid) {
      float* dst = kj >= nj ? dK + (bhN + tok) * DH : ws_dk + (((long)bh * groups + g) * nj + kj) * DH;
#pragma unroll
      for (int d = 0; d < DH; ++d) dst[d] = dk[d];
    }
    // a joint key takes the joint queries once (group 0); with nj = 0 every dK0 row is written as zero
    const bool joint = valid && (kj >= nj || g == 0);
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      k[d] = joint ? K0[(bhN + tok) * DH + d] : 0.f;
      dk[d] = 0.f;
    }
    if (joint) {
      if (jatt)
        for (int r = 0; r < nj; ++r) dkv_row<DH>(Aj + r * DH, Bj + r * DH, Lj[r], Dj[r], k, v, dk, dv);
#pragma unroll
      for (int d = 0; d < DH; ++d) dK0[(bhN + tok) * DH + d] = dk[d];
    }
    if (valid) {
      float* dst = kj >= nj ? dV + (bhN + tok) * DH : ws_dv + (((long)bh * groups + g) * nj + kj) * DH;
#pragma unroll
      for (int d = 0; d < DH; ++d) dst[d] = dv[d];
    }
  }
  // ---- phase 2: dQ of the patch queries
  const int t = threadIdx.x;
  const bool qvalid = t < rows;
  const int qrow = qvalid ? t : 0;
  float q[DH], gq[DH], dq[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    q[d] = A[qrow * DH + d];
    gq[d] = Bm[qrow * DH + d];
    dq[d] = 0.f;
  }
  const float Lq = Ls[qrow], Dq = Ds[qrow];
  __syncthreads();
  const float* Kb = K + bhN * DH;
  const float* Vb = V + bhN * DH;
  for (int i = threadIdx.x; i < rows * DH; i += SB) {
    A[i] = Kb[(long)tok0 * DH + i];
    Bm[i] = Vb[(long)tok0 * DH + i];
  }
  for (int i = threadIdx.x; i < nj * DH; i += SB) {
    Aj[i] = Kb[i];
    Bj[i] = Vb[i];
  }
  __syncthreads();
  if (qvalid) {
    const int gl = t / n;
    for (int kj = 0; kj < per; ++kj) {
      if (kj >= nj && mask_patch_queries && Mk[gl * n + kj - nj] == 0) continue;
      const float* kr = kj < nj ? Aj + kj * DH : A + (gl * n + kj - nj) * DH;
      const float* vr = kj < nj ? Bj + kj * DH : Bm + (gl * n + kj - nj) * DH;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        s = fmaf(q[d], kr[d], s);
        dp = fmaf(gq[d], vr[d], dp);
      }
      const float ds = __expf(s - Lq) * (dp - Dq);
#pragma unroll
      for (int d = 0; d < DH; ++d) dq[d] = fmaf(ds, kr[d], dq[d]);
    }
#pragma unroll
    for (int d = 0; d < DH; ++d) dQ[(bhN + tok0 + t) * DH + d] = dq[d];
  }
}

}  // namespace hp

using namespace hp;

// hp_sformer_attention (fp32) and hp_sformer_attention_lse with the key mask: their launches, grids, key splits and merge.  With
// mask_patch_queries == 0 the patch queries are not masked at all: their launch IS the unmasked kernel.  want_lse false: the
// inference form.  precision HP_PRECISION_BF16 / _FP16 (the _p entries; mask_patch_queries 0, dh 32 / 64): the patch queries'
// launch is the unmasked 16-bit patch kernel, the joint queries keep the masked exact-fp32 path.  Every argument check comes
// before the first device call.
static int attention_masked(const char* who, const float* Q, const float* K, const float* K0, const float* V, float* out, float* lse,
                            int B, int heads, int dh, int Ntok, int num_joints, int patches_per_frame, int frames,
                            const unsigned char* key_mask, int mask_patch_queries, void* workspace, void* stream, bool want_lse,
                            int precision = HP_PRECISION_FP32) {
  HP_REQUIRE(key_mask, "%s: null key_mask", who);
  HP_REQUIRE(Q && K && K0 && V && out && workspace && (lse || !want_lse), "%s: null argument", who);
  HP_REQUIRE(B > 0 && heads > 0 && frames > 0 && patches_per_frame > 0 && num_joints >= 0 && num_joints <= 32 &&
                 Ntok == num_joints + frames * patches_per_frame,
             "%s: bad token layout", who);
  HP_REQUIRE(mask_patch_queries == 0 || mask_patch_queries == 1, "%s: mask_patch_queries must be 0 or 1", who);
  if (num_joints == 0) {
    set_error("%s: num_joints 0 not built (with no joint / class key an all-masked group would have an empty key set)", who);
    return HP_ERR_UNSUPPORTED;
  }
  const bool p16 = precision != HP_PRECISION_FP32;
  if (p16) {
    if (int rc = attn_masked16_check(who, num_joints, mask_patch_queries)) return rc;
    if (dh != 32 && dh != 64) {
      set_error("%s: dim_head %d not built for the 16-bit patch attention (32, 64)", who, dh);
      return HP_ERR_UNSUPPORTED;
    }
  }
  if (dh != 16 && dh != 24 && dh != 32 && dh != 64) {
    set_error("%s: dim_head %d not built (16, 24, 32, 64)", who, dh);
    return HP_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const int ntiles = (Ntok + 31) / 32;
  const int nsplit = std::max(1, std::min(ATTN_JOINT_SPLITS, ntiles / 4));
  float* part = (float*)workspace;
  float* const lse_out = want_lse ? lse : nullptr;
  const dim3 gp((patches_per_frame + 127) / 128, B * heads * frames), gj(nsplit, B * heads);
#define HP_ATTM(KERN, GRID, KK, MODE, LSEP) \
  hipLaunchKernelGGL(KERN, GRID, dim3(ST), 0, st, Q, KK, V, out, heads, Ntok, num_joints, patches_per_frame, frames, MODE, part, LSEP, key_mask)
  {
    HP_PROF("sformer_attention_patch", st);
    if (p16) {
      launch_attention_patch16(Q, K, V, out, lse_out, B, heads, dh, Ntok, num_joints, patches_per_frame, frames, precision, st);
    } else if (!mask_patch_queries) {
      launch_attention_patch(Q, K, V, out, lse_out, B, heads, dh, Ntok, num_joints, patches_per_frame, frames, st);
    } else if (want_lse) {
      if (dh == 64) HP_ATTM((k_attention64_masked<true>), gp, K, 0, lse);
      else if (dh == 32) HP_ATTM((k_attention_masked<32, true>), gp, K, 0, lse);
      else if (dh == 24) HP_ATTM((k_attention_masked<24, true>), gp, K, 0, lse);
      else HP_ATTM((k_attention_masked<16, true>), gp, K, 0, lse);
    } else {
      if (dh == 64) HP_ATTM((k_attention64_masked<false>), gp, K, 0, lse_out);
      else if (dh == 32) HP_ATTM((k_attention_masked<32, false>), gp, K, 0, lse_out);
      else if (dh == 24) HP_ATTM((k_attention_masked<24, false>), gp, K, 0, lse_out);
      else HP_ATTM((k_attention_masked<16, false>), gp, K, 0, lse_out);
    }
  }
  {
    HP_PROF("sformer_attention_joint", st);
    float* const nol = nullptr;   // (the joint queries' lse is the merge's)
    if (dh == 64) HP_ATTM((k_attention64_masked<false>), gj, K0, 1, nol);
    else if (dh == 32) HP_ATTM((k_attention_masked<32, false>), gj, K0, 1, nol);
    else if (dh == 24) HP_ATTM((k_attention_masked<24, false>), gj, K0, 1, nol);
    else HP_ATTM((k_attention_masked<16, false>), gj, K0, 1, nol);
    launch_attention_joint_merge(part, out, lse_out, B * heads, heads, dh, Ntok, num_joints, nsplit, st);
  }
#undef HP_ATTM
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_sformer_attention_masked(const float* Q, const float* K, const float* K0, const float* V, float* out, int B, int heads,
                                           int dh, int Ntok, int num_joints, int patches_per_frame, int frames,
                                           const unsigned char* key_mask, int mask_patch_queries, void* workspace, void* stream) {
  return attention_masked("hp_sformer_attention_masked", Q, K, K0, V, out, nullptr, B, heads, dh, Ntok, num_joints, patches_per_frame,
                          frames, key_mask, mask_patch_queries, workspace, stream, false);
}

extern "C" int hp_sformer_attention_lse_masked(const float* Q, const float* K, const float* K0, const float* V, float* out, float* lse,
                                               int B, int heads, int dh, int Ntok, int num_joints, int patches_per_frame, int frames,
                                               const unsigned char* key_mask, int mask_patch_queries, void* workspace, void* stream) {
  return attention_masked("hp_sformer_attention_lse_masked", Q, K, K0, V, out, lse, B, heads, dh, Ntok, num_joints, patches_per_frame,
                          frames, key_mask, mask_patch_queries, workspace, stream, true);
}

// The two forward entries with a precision: FP32 forwards to them; BF16 / FP16 exchange the patch queries' launch only.
#define HP_MASKED_P_HEAD(WHO)                                                                                       \
  HP_REQUIRE(key_mask, "%s: null key_mask", WHO);                                                                   \
  HP_REQUIRE(precision == HP_PRECISION_FP32 || precision == HP_PRECISION_BF16 || precision == HP_PRECISION_FP16,    \
             "%s: precision %d not built", WHO, precision)
extern "C" int hp_sformer_attention_masked_p(const float* Q, const float* K, const float* K0, const float* V, float* out, int B, int heads,
                                             int dh, int Ntok, int num_joints, int patches_per_frame, int frames,
                                             const unsigned char* key_mask, int mask_patch_queries, int precision, void* workspace,
                                             void* stream) {
  HP_MASKED_P_HEAD("hp_sformer_attention_masked_p");
  if (precision == HP_PRECISION_FP32)
    return hp_sformer_attention_masked(Q, K, K0, V, out, B, heads, dh, Ntok, num_joints, patches_per_frame, frames, key_mask,
                                       mask_patch_queries, workspace, stream);
  return attention_masked("hp_sformer_attention_masked_p", Q, K, K0, V, out, nullptr, B, heads, dh, Ntok, num_joints, patches_per_frame,
                          frames, key_mask, mask_patch_queries, workspace, stream, false, precision);
}

extern "C" int hp_sformer_attention_lse_masked_p(const float* Q, const float* K, const float* K0, const float* V, float* out, float* lse,
                                                 int B, int heads, int dh, int Ntok, int num_joints, int patches_per_frame, int frames,
                                                 const unsigned char* key_mask, int mask_patch_queries, int precision, void* workspace,
                                                 void* stream) {
  HP_MASKED_P_HEAD("hp_sformer_attention_lse_masked_p");
  if (precision == HP_PRECISION_FP32)
    return hp_sformer_attention_lse_masked(Q, K, K0, V, out, lse, B, heads, dh, Ntok, num_joints, patches_per_frame, frames, key_mask,
                                           mask_patch_queries, workspace, stream);
  return attention_masked("hp_sformer_attention_lse_masked_p", Q, K, K0, V, out, lse, B, heads, dh, Ntok, num_joints, patches_per_frame,
                          frames, key_mask, mask_patch_queries, workspace, stream, true, precision);
}
#undef HP_MASKED_P_HEAD

// launch_attn_bwd_dq_joint with the key mask (dh 16 / 24 / 32 / 64): the same splits, sub-ranges and ordered merge (shared with the
// 16-bit masked backward of sformer_backward16.hip)
void hp::launch_attn_bwd_dq_joint_masked(const float* Q, const float* K0, const float* V, const float* dout, const float* lse,
                                         const float* delta, float* part, float* dQ, int BH, int heads, int dh, int Ntok, int nj,
                                         const unsigned char* key_mask, hipStream_t st) {
  const int nsplit = std::max(1, std::min(ATTN_BWD_DQ_SPLITS, (Ntok + 255) / 256));
  const dim3 gj(nsplit, BH);
#define HP_DQJ(D) hipLaunchKernelGGL((k_attn_bwd_dq_joint_masked<D>), gj, dim3(SB), 0, st, Q, K0, V, dout, lse, delta, part, heads, Ntok, nj, key_mask)
  if (dh == 64) hipLaunchKernelGGL(k_attn_bwd_dq_joint64_masked, gj, dim3(SB), 0, st, Q, K0, V, dout, lse, delta, part, heads, Ntok, nj, key_mask);
  else if (dh == 32) HP_DQJ(32);
  else if (dh == 24) HP_DQJ(24);
  else HP_DQJ(16);
#undef HP_DQJ
  launch_attn_bwd_dq_joint_merge(part, dQ, BH, Ntok, dh, nj, nsplit, st);
}

// LDS of k_attn_bwd_grouped_masked: k_attn_bwd_grouped's images (two (G n) x dh + lse, delta of the patch rows; the same for the
// nj joint rows) and the mask bytes of the G n patch rows, rounded up to whole floats
static size_t grouped_masked_lds_bytes(int dh, int nj, int n, int G) {
  return sizeof(float) * ((size_t)G * n * (2 * dh + 2) + (size_t)nj * (2 * dh + 2)) + (((size_t)G * n + 3) & ~(size_t)3);
}

// Arguments of the masked backward entries, checked before any device call.
static int attn_bwd_masked_check(const char* who, const void* key_mask, int num_joints, int mask_patch_queries) {
  HP_REQUIRE(key_mask, "%s: null key_mask", who);
  HP_REQUIRE(mask_patch_queries == 0 || mask_patch_queries == 1, "%s: mask_patch_queries must be 0 or 1", who);
  if (num_joints == 0) {
    set_error("%s: num_joints 0 not built (with no joint / class key an all-masked group would have an empty key set)", who);
    return HP_ERR_UNSUPPORTED;
  }
  return HP_OK;
}

extern "C" size_t hp_sformer_attention_backward_masked_workspace_bytes(int B, int heads, int dh, int Ntok, int num_joints, int frames) {
  return hp_sformer_attention_backward_workspace_bytes(B, heads, dh, Ntok, num_joints, frames);
}

// hp_sformer_attention_backward's launches with the masked instantiations (the patch queries' dQ keeps the unmasked kernel when
// they do not apply the mask).  delta, the joint keys' frame-ordered sum and the joint queries' merge are shared.
extern "C" int hp_sformer_attention_backward_masked(const float* Q, const float* K, const float* K0, const float* V, const float* out,
                                                    const float* dout, const float* lse, float* dQ, float* dK, float* dK0, float* dV,
                                                    int B, int heads, int dh, int Ntok, int num_joints, int patches_per_frame,
                                                    int frames, const unsigned char* key_mask, int mask_patch_queries, void* workspace,
                                                    size_t workspace_bytes, void* stream) {
  if (int rc = attn_bwd_masked_check("hp_sformer_attention_backward_masked", key_mask, num_joints, mask_patch_queries)) return rc;
  HP_REQUIRE(Q && K && K0 && V && out && dout && lse && dQ && dK && dK0 && dV && workspace,
             "hp_sformer_attention_backward_masked: null argument");
  HP_REQUIRE(B > 0 && heads > 0 && frames > 0 && patches_per_frame > 0 && num_joints <= 32 &&
                 Ntok == num_joints + frames * patches_per_frame,
             "hp_sformer_attention_backward_masked: bad token layout");
  if (dh != 16 && dh != 24 && dh != 32 && dh != 64) {
    set_error("hp_sformer_attention_backward_masked: dim_head %d not built (16, 24, 32, 64)", dh);
    return HP_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < hp_sformer_attention_backward_masked_workspace_bytes(B, heads, dh, Ntok, num_joints, frames)) {
    set_error("hp_sformer_attention_backward_masked: workspace too small");
    return HP_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int BH = B * heads, nj = num_joints, n = patches_per_frame, mpq = mask_patch_queries;
  float* delta = (float*)workspace;
  float* ws_dk = delta + (size_t)BH * Ntok;
  float* ws_dv = ws_dk + (size_t)BH * frames * nj * dh;
  float* part = ws_dv + (size_t)BH * frames * nj * dh;
  {
    HP_PROF("sformer_attn_bwd_delta", st);
    launch_attn_bwd_delta(out, dout, delta, B, heads, dh, Ntok, st);
  }
  const dim3 gkv((nj + n + SB - 1) / SB, BH * frames), gq((n + SB - 1) / SB, BH * frames);
  const dim3 gkv64((nj + n + PB - 1) / PB, BH * frames), gq64((n + PB - 1) / PB, BH * frames);
  {
    HP_PROF("sformer_attn_bwd_dkv", st);
#define HP_DKV(D) hipLaunchKernelGGL((k_attn_bwd_dkv_masked<D>), gkv, dim3(SB), 0, st, Q, K, K0, V, dout, lse, delta, dK, dK0, dV, ws_dk, ws_dv, heads, Ntok, nj, n, frames, key_mask, mpq)
    if (dh == 64)
      hipLaunchKernelGGL(k_attn_bwd_dkv64_masked, gkv64, dim3(SB), 0, st, Q, K, K0, V, dout, lse, delta, dK, dK0, dV, ws_dk, ws_dv, heads, Ntok,
                         nj, n, frames, key_mask, mpq);
    else if (dh == 32) HP_DKV(32);
    else if (dh == 24) HP_DKV(24);
    else HP_DKV(16);
#undef HP_DKV
  }
  {
    HP_PROF("sformer_attn_bwd_joint_keys", st);
    launch_attn_bwd_joint_keys(ws_dk, ws_dv, dK, dV, BH, Ntok, dh, nj, frames, st);
  }
  {
    HP_PROF("sformer_attn_bwd_dq", st);
#define HP_DQM(D) hipLaunchKernelGGL((k_attn_bwd_dq_patch_masked<D>), gq, dim3(SB), 0, st, Q, K, V, dout, lse, delta, dQ, heads, Ntok, nj, n, frames, key_mask)
    if (!mpq) launch_attn_bwd_dq_patch(Q, K, V, dout, lse, delta, dQ, BH, heads, dh, Ntok, nj, n, frames, st);
    else if (dh == 64)
      hipLaunchKernelGGL(k_attn_bwd_dq_patch64_masked, gq64, dim3(SB), 0, st, Q, K, V, dout, lse, delta, dQ, heads, Ntok, nj, n, frames, key_mask);
    else if (dh == 32) HP_DQM(32);
    else if (dh == 24) HP_DQM(24);
    else HP_DQM(16);
#undef HP_DQM
  }
  {
    HP_PROF("sformer_attn_bwd_dq_joint", st);
    launch_attn_bwd_dq_joint_masked(Q, K0, V, dout, lse, delta, part, dQ, BH, heads, dh, Ntok, nj, key_mask, st);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" size_t hp_sformer_attention_backward_grouped_masked_workspace_bytes(int B, int heads, int dh, int Ntok, int num_joints,
                                                                               int groups) {
  return hp_sformer_attention_backward_workspace_bytes(B, heads, dh, Ntok, num_joints, groups);
}

// hp_sformer_attention_backward_grouped with the key mask: bit-equal to hp_sformer_attention_backward_masked.
extern "C" int hp_sformer_attention_backward_grouped_masked(const float* Q, const float* K, const float* K0, const float* V,
                                                            const float* out, const float* dout, const float* lse, float* dQ,
                                                            float* dK, float* dK0, float* dV, int B, int heads, int dh, int Ntok,
                                                            int num_joints, int patches_per_group, int groups,
                                                            const unsigned char* key_mask, int mask_patch_queries, void* workspace,
                                                            size_t workspace_bytes, void* stream) {
  if (int rc = attn_bwd_masked_check("hp_sformer_attention_backward_grouped_masked", key_mask, num_joints, mask_patch_queries)) return rc;
  HP_REQUIRE(Q && K && K0 && V && out && dout && lse && dQ && dK && dK0 && dV && workspace,
             "hp_sformer_attention_backward_grouped_masked: null argument");
  HP_REQUIRE(B > 0 && heads > 0 && groups > 0 && patches_per_group > 0 && num_joints <= 32 &&
                 Ntok == num_joints + groups * patches_per_group,
             "hp_sformer_attention_backward_grouped_masked: bad token layout");
  if (dh != 16 && dh != 24 && dh != 32) {
    set_error("hp_sformer_attention_backward_grouped_masked: dim_head %d not built (16, 24, 32)", dh);
    return HP_ERR_UNSUPPORTED;
  }
  if (patches_per_group > ATTN_GROUPED_MAX_N) {
    set_error("hp_sformer_attention_backward_grouped_masked: %d tokens per group not built (at most %d; use "
              "hp_sformer_attention_backward_masked)",
              patches_per_group, ATTN_GROUPED_MAX_N);
    return HP_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < hp_sformer_attention_backward_grouped_masked_workspace_bytes(B, heads, dh, Ntok, num_joints, groups)) {
    set_error("hp_sformer_attention_backward_grouped_masked: workspace too small");
    return HP_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int BH = B * heads, nj = num_joints, n = patches_per_group;
  float* delta = (float*)workspace;
  float* ws_dk = delta + (size_t)BH * Ntok;
  float* ws_dv = ws_dk + (size_t)BH * groups * nj * dh;
  float* part = ws_dv + (size_t)BH * groups * nj * dh;
  int G = std::max(1, std::min(SB / (nj + n), groups));
  while (G > 1 && grouped_masked_lds_bytes(dh, nj, n, G) > 65536) --G;
  const int wg_per_bh = (groups + G - 1) / G;
  const long nwg = (long)BH * wg_per_bh;
  HP_REQUIRE(nwg < (1l << 31), "hp_sformer_attention_backward_grouped_masked: grid too large");
  const size_t lds = grouped_masked_lds_bytes(dh, nj, n, G);
  {
    HP_PROF("sformer_attn_bwd_delta", st);
    launch_attn_bwd_delta(out, dout, delta, B, heads, dh, Ntok, st);
  }
  {
    HP_PROF("sformer_attn_bwd_grouped", st);
#define HP_GRP(D) hipLaunchKernelGGL((k_attn_bwd_grouped_masked<D>), dim3((unsigned)nwg), dim3(SB), lds, st, Q, K, K0, V, dout, lse, delta, dQ, dK, dK0, dV, ws_dk, ws_dv, heads, Ntok, nj, n, groups, G, wg_per_bh, key_mask, mask_patch_queries)
    if (dh == 32) HP_GRP(32);
    else if (dh == 24) HP_GRP(24);
    else HP_GRP(16);
#undef HP_GRP
  }
  {
    HP_PROF("sformer_attn_bwd_joint_keys", st);
    launch_attn_bwd_joint_keys(ws_dk, ws_dv, dK, dV, BH, Ntok, dh, nj, groups, st);
  }
  {
    HP_PROF("sformer_attn_bwd_dq_joint", st);
    launch_attn_bwd_dq_joint_masked(Q, K0, V, dout, lse, delta, part, dQ, BH, heads, dh, Ntok, nj, key_mask, st);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
