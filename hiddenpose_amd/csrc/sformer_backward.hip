// NlosPoseSformer backward (models/NlosPoseSformer.py:95-151 under autograd): attention with joint tokens, the qkv split
// with axial RoPE, LayerNorm, GEGLU, Linear (on the 1x1x1 implicit-GEMM convolution gradients), patchify and the
// joint-token batch sum.  Every reduction runs in a fixed order: two calls on the same inputs give identical outputs
// (no float atomics anywhere in this file).
//
// Attention backward (exact fp32, VALU fmaf chains; P recomputed from Q, K and the forward's lse):
//   delta     delta = rowsum(dO o O), one thread per (b, head, token)
//   dkv       one workgroup per 256-key block of one (b, head, frame); the key is the thread: k, v, dk, dv live in its
//             registers while the workgroup sweeps the frame's n patch queries (64-row tiles of Q, dO, lse, delta in LDS),
//             then the nj joint queries with the key's K0 row (dK0; dV keeps accumulating).  The nj joint keys are shared by
//             every frame: their per-frame partials go to a workspace and are summed over the frames in frame order.
//   dq_patch  one thread per patch query, 64-key tiles of K and V in LDS, keys [nj joint rows of K | the frame's patches]
//   dq_joint  the nj joint queries against all Ntok rows of K0: key splits x 8 sub-ranges per workgroup, the 8 sub-ranges
//             summed through LDS, the splits by a merge kernel, both in index order.
//   grouped   short groups (n <= 64, TimeSformer's time attention): dkv and dq_patch of several whole groups in one
//             workgroup, same arithmetic and order (hp_sformer_attention_backward_grouped).
//   dh 64     dkv, dq_patch and dq_joint with the key / query on a lane PAIR, 32 values of d per lane (k_attn_bwd_*64 below).
#include <algorithm>
#include <cfloat>

#include "hp_internal.h"
#include "hp_philox.h"

namespace hp {

constexpr int SB = 256;   // threads per block
constexpr int QT = 64;    // query rows per LDS tile of the dkv sweep
constexpr int KT = 64;    // key rows per LDS tile of the dq sweep
constexpr int DQ_SPLITS = ATTN_BWD_DQ_SPLITS;

static unsigned bgrid(long n) { return (unsigned)std::max<long>(1, std::min<long>((n + SB - 1) / SB, 256 * 8)); }

// delta[bh][tok] = sum_d dout[b][tok][head*dh + d] * out[b][tok][head*dh + d]
__global__ __launch_bounds__(SB) void k_attn_bwd_delta(const float* __restrict__ out, const float* __restrict__ dout,
                                                       float* __restrict__ delta, int B, int heads, int dh, int Ntok) {
  const long total = (long)B * heads * Ntok;
  const int inner = heads * dh;
  for (long i = (long)blockIdx.x * SB + threadIdx.x; i < total; i += (long)gridDim.x * SB) {
    const int tok = (int)(i % Ntok);
    const long bh = i / Ntok;
    const int head = (int)(bh % heads);
    const long b = bh / heads;
    const float* o = out + (b * Ntok + tok) * inner + head * dh;
    const float* g = dout + (b * Ntok + tok) * inner + head * dh;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s = fmaf(o[d], g[d], s);
    delta[i] = s;
  }
}

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

// grid (ceil((nj + n) / SB), B * heads * frames); key kj of frame f's key set [nj joint tokens | frame f's patches]
template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_dkv(const float* __restrict__ Q, const float* __restrict__ K,
                                                     const float* __restrict__ K0, const float* __restrict__ V,
                                                     const float* __restrict__ dout, const float* __restrict__ lse,
                                                     const float* __restrict__ delta, float* __restrict__ dK,
                                                     float* __restrict__ dK0, float* __restrict__ dV,
                                                     float* __restrict__ ws_dk, float* __restrict__ ws_dv, int heads, int Ntok,
                                                     int nj, int n, int frames) {
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
    if (joint)
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

// dK and dV of the joint keys: the per-frame partials summed in frame order.  One thread per (bh, joint key, d).
__global__ __launch_bounds__(SB) void k_attn_bwd_joint_keys(const float* __restrict__ ws_dk, const float* __restrict__ ws_dv,
                                                            float* __restrict__ dK, float* __restrict__ dV, int BH, int Ntok, int dh,
                                                            int nj, int frames) {
  const long i = (long)blockIdx.x * SB + threadIdx.x;
  if (i >= (long)BH * nj * dh) return;
  const int d = (int)(i % dh), j = (int)((i / dh) % nj);
  const long bh = i / ((long)dh * nj);
  float sk = 0.f, sv = 0.f;
  for (int f = 0; f < frames; ++f) {
    const long o = ((bh * frames + f) * nj + j) * dh + d;
    sk += ws_dk[o];
    sv += ws_dv[o];
  }
  dK[(bh * Ntok + j) * dh + d] = sk;
  dV[(bh * Ntok + j) * dh + d] = sv;
}

// grid (ceil(n / SB), B * heads * frames): dQ of frame f's patch queries; keys [nj joint rows of K | the frame's patches]
template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_dq_patch(const float* __restrict__ Q, const float* __restrict__ K,
                                                          const float* __restrict__ V, const float* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          float* __restrict__ dQ, int heads, int Ntok, int nj, int n, int frames) {
  __shared__ __attribute__((aligned(16))) float Ks[KT * DH];
  __shared__ __attribute__((aligned(16))) float Vs[KT * DH];
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
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
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

// grid (nsplit, B * heads): partial dQ of the nj joint queries over key split blockIdx.x of all Ntok rows of K0.
// Thread = (query tid & 31, sub-range tid >> 5); sub-range s takes the split's keys s, s + 8, s + 16, ...
template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_dq_joint(const float* __restrict__ Q, const float* __restrict__ K0,
                                                          const float* __restrict__ V, const float* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          float* __restrict__ part, int heads, int Ntok, int nj) {
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

__global__ __launch_bounds__(SB) void k_attn_bwd_dq_joint_merge(const float* __restrict__ part, float* __restrict__ dQ, int BH, int Ntok,
                                                                int dh, int nj, int nsplit) {
  const long i = (long)blockIdx.x * SB + threadIdx.x;
  if (i >= (long)BH * nj * dh) return;
  const int d = (int)(i % dh), j = (int)((i / dh) % nj);
  const long bh = i / ((long)dh * nj);
  float s = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) s += part[((bh * nsplit + sp) * 32 + j) * dh + d];
  dQ[(bh * Ntok + j) * dh + d] = s;
}

// ---- dim_head 64: d split over a lane pair ---------------------------------------------------------------------------------
// The key-per-thread form would hold k, v, dk, dv = 4 x 64 floats per thread at this width and spill.  Here a key (dkv) or a
// query (dq) belongs to the lane PAIR (2i, 2i + 1): lane hf of the pair holds d = 32 hf .. 32 hf + 31 of every row it keeps, so
// the register set is the one of the dh-32 kernels.  The two 32-term halves of a dot product meet in one xor-1 exchange (a DPP
// quad permute: VALU, no trip through the LDS crossbar as ds_bpermute would take in the middle of a dependent chain); a + b and
// b + a are the same float, so both lanes go on with identical s, dp, p and ds.  A workgroup takes 128 keys or queries; the LDS
// tiles, the sweep order, the joint-key partials and the joint-query splits are unchanged.
constexpr int HD = 32;       // d per lane
constexpr int PB = SB / 2;   // keys / queries per workgroup

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

// grid (ceil((nj + n) / PB), B * heads * frames); k_attn_bwd_dkv with the key on a lane pair
__global__ __launch_bounds__(SB) void k_attn_bwd_dkv64(const float* __restrict__ Q, const float* __restrict__ K,
                                                       const float* __restrict__ K0, const float* __restrict__ V,
                                                       const float* __restrict__ dout, const float* __restrict__ lse,
                                                       const float* __restrict__ delta, float* __restrict__ dK,
                                                       float* __restrict__ dK0, float* __restrict__ dV,
                                                       float* __restrict__ ws_dk, float* __restrict__ ws_dv, int heads, int Ntok,
                                                       int nj, int n, int frames) {
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
    if (joint)   // (both lanes of a pair share kj: the exchange inside never crosses this branch)
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

// grid (ceil(n / PB), B * heads * frames): k_attn_bwd_dq_patch with the query on a lane pair
__global__ __launch_bounds__(SB) void k_attn_bwd_dq_patch64(const float* __restrict__ Q, const float* __restrict__ K,
                                                            const float* __restrict__ V, const float* __restrict__ dout,
                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                            float* __restrict__ dQ, int heads, int Ntok, int nj, int n, int frames) {
  constexpr int DH = 64;
  __shared__ __attribute__((aligned(16))) float Ks[KT * DH];
  __shared__ __attribute__((aligned(16))) float Vs[KT * DH];
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
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
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

// grid (nsplit, B * heads): k_attn_bwd_dq_joint with the query on a lane pair.  Thread = (d half tid & 1, query (tid >> 1) & 31,
// sub-range tid >> 6); sub-range s takes the split's keys s, s + 4, s + 8, ...; the 4 sub-ranges are summed through LDS in order.
__global__ __launch_bounds__(SB) void k_attn_bwd_dq_joint64(const float* __restrict__ Q, const float* __restrict__ K0,
                                                            const float* __restrict__ V, const float* __restrict__ dout,
                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                            float* __restrict__ part, int heads, int Ntok, int nj) {
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

// Transpose of k_qkv_prepare: dQ, dK, dK0, dV (B, heads, Ntok, dh) -> dqkv (B, Ntok, 3 inner).
// q' = R(scale q): dq = scale R^T(dQ); k' = R(k) on patch tokens, k0 = k: dk = R^T(dK) + dK0; dv = dV.
// R on pair (d, d^1): t'[d] = t[d] cos[d] + sgn(d) t[d^1] sin[d], sgn(d) = +1 for odd d, -1 for even d, so
// R^T(g)[d] = g[d] cos[d] - sgn(d) g[d^1] sin[d^1].
__global__ __launch_bounds__(SB) void k_qkv_prepare_bwd(const float* __restrict__ dQ, const float* __restrict__ dK,
                                                        const float* __restrict__ dK0, const float* __restrict__ dV,
                                                        float* __restrict__ dqkv, int B, int Ntok, int heads, int dh, int nj,
                                                        int n, float scale, const float* __restrict__ sin_t,
                                                        const float* __restrict__ cos_t, int rot_dim) {
  const int inner = heads * dh;
  const long total = (long)B * Ntok * inner;
  for (long i = (long)blockIdx.x * SB + threadIdx.x; i < total; i += (long)gridDim.x * SB) {
    const int d = (int)(i % dh);
    long t = i / dh;
    const int h = (int)(t % heads);
    t /= heads;
    const int tok = (int)(t % Ntok);
    const int b = (int)(t / Ntok);
    const long o = (((long)b * heads + h) * Ntok + tok) * dh + d;
    float gq = dQ[o], gk = dK[o];
    if (tok >= nj && d < rot_dim) {
      const int pos = (tok - nj) % n;
      const int dp = d ^ 1;
      const long op = o - d + dp;
      const float cs = cos_t[pos * rot_dim + d], snp = sin_t[pos * rot_dim + dp];
      const float sgn = (d & 1) ? 1.f : -1.f;
      gq = gq * cs - sgn * dQ[op] * snp;
      gk = gk * cs - sgn * dK[op] * snp;
    }
    float* dst = dqkv + ((long)b * Ntok + tok) * 3 * inner + h * dh + d;
    dst[0] = gq * scale;
    dst[inner] = gk + dK0[o];
    dst[2 * inner] = dV[o];
  }
}

// LayerNorm backward, one wave per row (rows dealt round-robin over the grid's waves, a fixed assignment for a given rows):
// dx[src] += rstd (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat)); per-workgroup column partials of dy xhat and dy
// in LDS (a lane owns its columns inside its wave's image), written as part[blockIdx.x][2 dim].
__global__ __launch_bounds__(SB) void k_layernorm_bwd(const float* __restrict__ x, const float* __restrict__ dy,
                                                      float* __restrict__ dx, long rows, int dim, const float* __restrict__ gamma,
                                                      float eps, int rpb, long batch_stride_rows, float* __restrict__ part) {
  extern __shared__ float lds[];   // [4 waves][2 dim]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* acc = lds + wave * 2 * dim;
  for (int i = lane; i < 2 * dim; i += 64) acc[i] = 0.f;
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const long src = rpb > 0 ? (row / rpb) * batch_stride_rows + (row % rpb) : row;
    const float* p = x + src * dim;
    const float* g = dy + row * dim;
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) s += p[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)dim;
    float q = 0.f;
    for (int i = lane; i < dim; i += 64) {
      const float d = p[i] - mean;
      q += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)dim + eps);
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane; i < dim; i += 64) {
      const float xh = (p[i] - mean) * rstd, gg = g[i] * gamma[i];
      s1 += gg;
      s2 += gg * xh;
      acc[i] += g[i] * xh;
      acc[dim + i] += g[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    const float m1 = s1 / (float)dim, m2 = s2 / (float)dim;
    float* o = dx + src * dim;
    for (int i = lane; i < dim; i += 64) {
      const float xh = (p[i] - mean) * rstd;
      o[i] += rstd * (g[i] * gamma[i] - m1 - xh * m2);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * dim; i += SB)
    part[(long)blockIdx.x * 2 * dim + i] = ((lds[i] + lds[2 * dim + i]) + lds[4 * dim + i]) + lds[6 * dim + i];
}

// column sums of a [nblk][cols] partial matrix, in block order
__global__ __launch_bounds__(SB) void k_sum_partials(const float* __restrict__ part, float* __restrict__ out0,
                                                     float* __restrict__ out1, int nblk, int cols, int split) {
  const int c = blockIdx.x * SB + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
  for (int k = 0; k < nblk; ++k) s += part[(long)k * cols + c];
  if (c < split) out0[c] = s;
  else out1[c - split] = s;
}

// column partial sums over row chunks: part[chunk][c] = sum over rows [chunk * per, ...) of x[r * ld + c]
__global__ __launch_bounds__(SB) void k_colsum_partial(const float* __restrict__ x, float* __restrict__ part, long rows, int cols,
                                                       long ld, long per) {
  const int c = blockIdx.x * SB + threadIdx.x;
  if (c >= cols) return;
  const long r0 = (long)blockIdx.y * per, r1 = std::min(rows, r0 + per);
  float s = 0.f;
  for (long r = r0; r < r1; ++r) s += x[r * ld + c];
  part[(long)blockIdx.y * cols + c] = s;
}

// Short groups (TimeSformer's time attention: n = frames of one patch position, hp*wp groups per (b, head)).  One
// workgroup takes G whole consecutive groups of one (b, head); its patch rows are the contiguous token range
// [nj + g0 n, nj + (g0 + G) n).  Phase 1 (thread = key, G (nj + n) threads): Q, dO, lse, delta of the G groups' patch
// queries and of the nj joint queries staged once; a key sweeps its group's n queries (and, for a patch key or a joint key
// of group 0, the joint queries with its K0 row), exactly as k_attn_bwd_dkv does.  Phase 2 (thread = patch query, G n
// threads): the query keeps its q, dO, lse, delta in registers, K and V of the G groups and of the joint rows replace the
// phase-1 images, and the query sweeps [joint keys | its group's keys] as k_attn_bwd_dq_patch does.  Joint-key partials
// go to the per-group workspace (summed in group order by k_attn_bwd_joint_keys).  grid x = B * heads * ceil(groups / G).
template <int DH>
__global__ __launch_bounds__(SB) void k_attn_bwd_grouped(const float* __restrict__ Q, const float* __restrict__ K,
                                                         const float* __restrict__ K0, const float* __restrict__ V,
                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, float* __restrict__ dQ,
                                                         float* __restrict__ dK, float* __restrict__ dK0, float* __restrict__ dV,
                                                         float* __restrict__ ws_dk, float* __restrict__ ws_dv, int heads, int Ntok,
                                                         int nj, int n, int groups, int G, int wg_per_bh) {
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
  __syncthreads();
  // ---- phase 1: dK, dK0, dV
  {
    const int t = threadIdx.x;
    const bool valid = t < Gw * per;
    const int gl = valid ? t / per : 0, kj = valid ? t - gl * per : 0, g = g0 + gl;
    const int tok = kj < nj ? kj : nj + g * n + (kj - nj);
    float k[DH], v[DH], dk[DH], dv[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      k[d] = valid ? K[(bhN + tok) * DH + d] : 0.f;
      v[d] = valid ? V[(bhN + tok) * DH + d] : 0.f;
      dk[d] = 0.f;
      dv[d] = 0.f;
    }
    if (valid)
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

// Phi(t) and phi(t) of the exact erf GELU: what every activation backward below derives from.
__device__ __forceinline__ void gelu_cdf_pdf(float t, float& cdf, float& pdf) {
  cdf = 0.5f * (1.0f + erff(t * 0.70710678118654752f));
  pdf = 0.39894228040143268f * __expf(-0.5f * t * t);
}

// du = dy * gelu'(u), gelu(u) = u Phi(u): gelu'(u) = Phi(u) + u phi(u) (exact erf form); du may alias dy
__global__ __launch_bounds__(SB) void k_gelu_bwd(const float* __restrict__ u, const float* dy, float* du, long n) {
  for (long i = (long)blockIdx.x * SB + threadIdx.x; i < n; i += (long)gridDim.x * SB) {
    const float t = u[i];
    float cdf, pdf;
    gelu_cdf_pdf(t, cdf, pdf);
    du[i] = dy[i] * (cdf + t * pdf);
  }
}

// k_gelu_bwd on the dropped gradient: dy first goes through the dropout site's mask (element i of the site's tensor is
// element i here), g = kept ? dy * scale : 0 rounded once, exactly hp_dropout_forward's value; then the line above.  A thread
// owns the Philox block's four elements; du may alias dy.
__global__ __launch_bounds__(SB) void k_gelu_bwd_dropout(const float* __restrict__ u, const float* dy, float* du, long n,
                                                         const DropoutParams d) {
  const long ngroups = (n + 3) >> 2;
  for (long gi = (long)blockIdx.x * SB + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * SB) {
    const uint4 w4 = philox4x32_10((unsigned long long)gi, d);
    const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
    float g[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) g[c] = 4 * gi + c < n ? dropout_apply(dy[4 * gi + c], w[c], d) : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long i = 4 * gi + c;
      if (i < n) {
        const float t = u[i];
        float cdf, pdf;
        gelu_cdf_pdf(t, cdf, pdf);
        du[i] = g[c] * (cdf + t * pdf);
      }
    }
  }
}

// du (rows, 2H) from dg (rows, H) and u: g = a gelu(t), gelu(t) = t Phi(t): da = dg gelu(t), dt = dg a (Phi(t) + t phi(t))
__global__ __launch_bounds__(SB) void k_geglu_bwd(const float* __restrict__ u, const float* __restrict__ dg, float* __restrict__ du,
                                                  long rows, int Hd) {
  const long total = rows * Hd;
  for (long i = (long)blockIdx.x * SB + threadIdx.x; i < total; i += (long)gridDim.x * SB) {
    const long r = i / Hd;
    const int c = (int)(i - r * Hd);
    const float a = u[r * 2 * Hd + c], t = u[r * 2 * Hd + Hd + c], g = dg[i];
    float cdf, pdf;
    gelu_cdf_pdf(t, cdf, pdf);
    du[r * 2 * Hd + c] = g * t * cdf;
    du[r * 2 * Hd + Hd + c] = g * a * (cdf + t * pdf);
  }
}

// k_geglu_bwd on the dropped gradient (see k_gelu_bwd_dropout): the site's tensor is dg, (rows, Hd) row-major.  `vec` (the
// host's finding, uniform): Hd is a multiple of 4 and the three arrays are 16-byte aligned, so a group lies in one row and
// moves as float4; the arithmetic per element is the same either way.
__device__ __forceinline__ void geglu_bwd_elem(float a, float t, float g, float& da, float& dt) {
  float cdf, pdf;
  gelu_cdf_pdf(t, cdf, pdf);
  da = g * t * cdf;
  dt = g * a * (cdf + t * pdf);
}
__global__ __launch_bounds__(SB) void k_geglu_bwd_dropout(const float* __restrict__ u, const float* __restrict__ dg,
                                                          float* __restrict__ du, long rows, int Hd, int vec, const DropoutParams d) {
  const long total = rows * Hd, ngroups = (total + 3) >> 2;
  for (long gi = (long)blockIdx.x * SB + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * SB) {
    const uint4 w4 = philox4x32_10((unsigned long long)gi, d);
    if (vec) {
      const long r = (4 * gi) / Hd;
      const int c = (int)(4 * gi - r * Hd);
      const float4 g4 = *reinterpret_cast<const float4*>(dg + 4 * gi);
      const float4 a4 = *reinterpret_cast<const float4*>(u + r * 2 * Hd + c);
      const float4 t4 = *reinterpret_cast<const float4*>(u + r * 2 * Hd + Hd + c);
      float4 da, dt;
      geglu_bwd_elem(a4.x, t4.x, dropout_apply(g4.x, w4.x, d), da.x, dt.x);
      geglu_bwd_elem(a4.y, t4.y, dropout_apply(g4.y, w4.y, d), da.y, dt.y);
      geglu_bwd_elem(a4.z, t4.z, dropout_apply(g4.z, w4.z, d), da.z, dt.z);
      geglu_bwd_elem(a4.w, t4.w, dropout_apply(g4.w, w4.w, d), da.w, dt.w);
      *reinterpret_cast<float4*>(du + r * 2 * Hd + c) = da;
      *reinterpret_cast<float4*>(du + r * 2 * Hd + Hd + c) = dt;
      continue;
    }
    const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long i = 4 * gi + k;
      if (i < total) {
        const long r = i / Hd;
        const int c = (int)(i - r * Hd);
        geglu_bwd_elem(u[r * 2 * Hd + c], u[r * 2 * Hd + Hd + c], dropout_apply(dg[i], w[k], d), du[r * 2 * Hd + c],
                       du[r * 2 * Hd + Hd + c]);
      }
    }
  }
}

// gradient of patchify: video[b f c (h p1) (w p2)] <- tokens[(b f h w) (p1 p2 c)]; one thread per video element
__global__ __launch_bounds__(SB) void k_unpatchify(const float* __restrict__ tok, float* __restrict__ v, int B, int Fr, int C, int H,
                                                   int W, int ps) {
  const int hp = H / ps, wp = W / ps, pd = ps * ps * C;
  const long total = (long)B * Fr * C * H * W;
  for (long i = (long)blockIdx.x * SB + threadIdx.x; i < total; i += (long)gridDim.x * SB) {
    const int x = (int)(i % W);
    long t = i / W;
    const int y = (int)(t % H);
    t /= H;
    const int c = (int)(t % C);
    t /= C;  // t = b * Fr + f
    v[i] = tok[((t * hp + y / ps) * wp + x / ps) * pd + ((y % ps) * ps + x % ps) * C + c];
  }
}

// djt[j][d] = sum over b (in order) of dx[b][j][d]
__global__ __launch_bounds__(SB) void k_joint_token_bwd(const float* __restrict__ dx, float* __restrict__ djt, int B, int nj,
                                                        long Ntok, int dim) {
  const int i = blockIdx.x * SB + threadIdx.x;
  if (i >= nj * dim) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += dx[(long)b * Ntok * dim + i];
  djt[i] = s;
}

static int ln_blocks(long rows) { return (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 1024)); }
static int colsum_chunks(long rows) { return (int)std::max<long>(1, std::min<long>((rows + 255) / 256, 256)); }

constexpr int GROUPED_MAX_N = ATTN_GROUPED_MAX_N;   // tokens per group of k_attn_bwd_grouped
// LDS of k_attn_bwd_grouped: two (G n) x dh images + lse, delta of the patch rows; the same for the nj joint rows
static size_t grouped_lds_bytes(int dh, int nj, int n, int G) {
  return sizeof(float) * ((size_t)G * n * (2 * dh + 2) + (size_t)nj * (2 * dh + 2));
}

}  // namespace hp

using namespace hp;

extern "C" size_t hp_sformer_attention_backward_workspace_bytes(int B, int heads, int dh, int Ntok, int num_joints, int frames) {
  const size_t bh = (size_t)B * heads;
  return sizeof(float) * (bh * Ntok                                     // delta
                          + 2 * bh * frames * num_joints * dh           // joint-key partials of dK, dV
                          + bh * DQ_SPLITS * 32 * dh);                  // joint-query dQ partials
}

extern "C" int hp_sformer_attention_backward(const float* Q, const float* K, const float* K0, const float* V, const float* out,
                                             const float* dout, const float* lse, float* dQ, float* dK, float* dK0, float* dV, int B,
                                             int heads, int dh, int Ntok, int num_joints, int patches_per_frame, int frames,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  HP_REQUIRE(Q && K && K0 && V && out && dout && lse && dQ && dK && dK0 && dV && workspace,
             "hp_sformer_attention_backward: null argument");
  HP_REQUIRE(B > 0 && heads > 0 && frames > 0 && patches_per_frame > 0 && num_joints >= 0 && num_joints <= 32 &&
                 Ntok == num_joints + frames * patches_per_frame,
             "hp_sformer_attention_backward: bad token layout");
  if (dh != 16 && dh != 24 && dh != 32 && dh != 64) {
    set_error("hp_sformer_attention_backward: dim_head %d not built (16, 24, 32, 64)", dh);
    return HP_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < hp_sformer_attention_backward_workspace_bytes(B, heads, dh, Ntok, num_joints, frames)) {
    set_error("hp_sformer_attention_backward: workspace too small");
    return HP_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int BH = B * heads, nj = num_joints, n = patches_per_frame;
  float* delta = (float*)workspace;
  float* ws_dk = delta + (size_t)BH * Ntok;
  float* ws_dv = ws_dk + (size_t)BH * frames * nj * dh;
  float* part = ws_dv + (size_t)BH * frames * nj * dh;
  {
    HP_PROF("sformer_attn_bwd_delta", st);
    hipLaunchKernelGGL(k_attn_bwd_delta, dim3(bgrid((long)BH * Ntok)), dim3(SB), 0, st, out, dout, delta, B, heads, dh, Ntok);
  }
  const dim3 gkv((nj + n + SB - 1) / SB, BH * frames), gq((n + SB - 1) / SB, BH * frames);
  const dim3 gkv64((nj + n + PB - 1) / PB, BH * frames), gq64((n + PB - 1) / PB, BH * frames);   // dh 64: a lane pair per key / query
  {
    HP_PROF("sformer_attn_bwd_dkv", st);
#define HP_DKV(D) hipLaunchKernelGGL((k_attn_bwd_dkv<D>), gkv, dim3(SB), 0, st, Q, K, K0, V, dout, lse, delta, dK, dK0, dV, ws_dk, ws_dv, heads, Ntok, nj, n, frames)
    if (dh == 64)
      hipLaunchKernelGGL(k_attn_bwd_dkv64, gkv64, dim3(SB), 0, st, Q, K, K0, V, dout, lse, delta, dK, dK0, dV, ws_dk, ws_dv, heads, Ntok, nj, n,
                         frames);
    else if (dh == 32) HP_DKV(32);
    else if (dh == 24) HP_DKV(24);
    else HP_DKV(16);
#undef HP_DKV
  }
  if (nj > 0) {
    HP_PROF("sformer_attn_bwd_joint_keys", st);
    const long total = (long)BH * nj * dh;
    hipLaunchKernelGGL(k_attn_bwd_joint_keys, dim3((unsigned)((total + SB - 1) / SB)), dim3(SB), 0, st, ws_dk, ws_dv, dK, dV, BH, Ntok, dh,
                       nj, frames);
  }
  {
    HP_PROF("sformer_attn_bwd_dq", st);
#define HP_DQ(D) hipLaunchKernelGGL((k_attn_bwd_dq_patch<D>), gq, dim3(SB), 0, st, Q, K, V, dout, lse, delta, dQ, heads, Ntok, nj, n, frames)
    if (dh == 64) hipLaunchKernelGGL(k_attn_bwd_dq_patch64, gq64, dim3(SB), 0, st, Q, K, V, dout, lse, delta, dQ, heads, Ntok, nj, n, frames);
    else if (dh == 32) HP_DQ(32);
    else if (dh == 24) HP_DQ(24);
    else HP_DQ(16);
#undef HP_DQ
  }
  if (nj > 0) {
    HP_PROF("sformer_attn_bwd_dq_joint", st);
    const int nsplit = std::max(1, std::min(DQ_SPLITS, (Ntok + 255) / 256));
    const dim3 gj(nsplit, BH);
#define HP_DQJ(D) hipLaunchKernelGGL((k_attn_bwd_dq_joint<D>), gj, dim3(SB), 0, st, Q, K0, V, dout, lse, delta, part, heads, Ntok, nj)
    if (dh == 64) hipLaunchKernelGGL(k_attn_bwd_dq_joint64, gj, dim3(SB), 0, st, Q, K0, V, dout, lse, delta, part, heads, Ntok, nj);
    else if (dh == 32) HP_DQJ(32);
    else if (dh == 24) HP_DQJ(24);
    else HP_DQJ(16);
#undef HP_DQJ
    const long total = (long)BH * nj * dh;
    hipLaunchKernelGGL(k_attn_bwd_dq_joint_merge, dim3((unsigned)((total + SB - 1) / SB)), dim3(SB), 0, st, part, dQ, BH, Ntok, dh, nj,
                       nsplit);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

// The exact-fp32 pieces the 16-bit backward (sformer_backward16.hip) shares with this file, launched on `st`:
// the joint keys' per-frame dK / dV partials summed in frame order, and dQ of the joint queries (splits + ordered merge).
namespace hp {
void launch_attn_bwd_joint_keys(const float* ws_dk, const float* ws_dv, float* dK, float* dV, int BH, int Ntok, int dh, int nj, int frames,
                                hipStream_t st) {
  const long total = (long)BH * nj * dh;
  hipLaunchKernelGGL(k_attn_bwd_joint_keys, dim3((unsigned)((total + SB - 1) / SB)), dim3(SB), 0, st, ws_dk, ws_dv, dK, dV, BH, Ntok, dh, nj,
                     frames);
}
void launch_attn_bwd_dq_joint(const float* Q, const float* K0, const float* V, const float* dout, const float* lse, const float* delta,
                              float* part, float* dQ, int BH, int heads, int dh, int Ntok, int nj, hipStream_t st) {
  const int nsplit = std::max(1, std::min(DQ_SPLITS, (Ntok + 255) / 256));
  const dim3 gj(nsplit, BH);
  if (dh == 64) hipLaunchKernelGGL(k_attn_bwd_dq_joint64, gj, dim3(SB), 0, st, Q, K0, V, dout, lse, delta, part, heads, Ntok, nj);
  else hipLaunchKernelGGL((k_attn_bwd_dq_joint<32>), gj, dim3(SB), 0, st, Q, K0, V, dout, lse, delta, part, heads, Ntok, nj);
  const long total = (long)BH * nj * dh;
  hipLaunchKernelGGL(k_attn_bwd_dq_joint_merge, dim3((unsigned)((total + SB - 1) / SB)), dim3(SB), 0, st, part, dQ, BH, Ntok, dh, nj, nsplit);
}
// ... and the ones the masked entries (sformer_masked.hip) share with the entries of this file
void launch_attn_bwd_delta(const float* out, const float* dout, float* delta, int B, int heads, int dh, int Ntok, hipStream_t st) {
  hipLaunchKernelGGL(k_attn_bwd_delta, dim3(bgrid((long)B * heads * Ntok)), dim3(SB), 0, st, out, dout, delta, B, heads, dh, Ntok);
}
void launch_attn_bwd_dq_patch(const float* Q, const float* K, const float* V, const float* dout, const float* lse, const float* delta,
                              float* dQ, int BH, int heads, int dh, int Ntok, int nj, int n, int frames, hipStream_t st) {
  const dim3 gq((n + SB - 1) / SB, BH * frames), gq64((n + PB - 1) / PB, BH * frames);
#define HP_DQ(D) hipLaunchKernelGGL((k_attn_bwd_dq_patch<D>), gq, dim3(SB), 0, st, Q, K, V, dout, lse, delta, dQ, heads, Ntok, nj, n, frames)
  if (dh == 64) hipLaunchKernelGGL(k_attn_bwd_dq_patch64, gq64, dim3(SB), 0, st, Q, K, V, dout, lse, delta, dQ, heads, Ntok, nj, n, frames);
  else if (dh == 32) HP_DQ(32);
  else if (dh == 24) HP_DQ(24);
  else HP_DQ(16);
#undef HP_DQ
}
void launch_attn_bwd_dq_joint_merge(const float* part, float* dQ, int BH, int Ntok, int dh, int nj, int nsplit, hipStream_t st) {
  const long total = (long)BH * nj * dh;
  hipLaunchKernelGGL(k_attn_bwd_dq_joint_merge, dim3((unsigned)((total + SB - 1) / SB)), dim3(SB), 0, st, part, dQ, BH, Ntok, dh, nj, nsplit);
}
}  // namespace hp

// groups per workgroup of k_attn_bwd_grouped: as many whole groups as G (nj + n) <= SB threads allow, while the LDS images
// stay within 64 KiB
static int grouped_groups_per_wg(int dh, int nj, int n, int groups) {
  int G = std::max(1, std::min(SB / (nj + n), groups));
  while (G > 1 && grouped_lds_bytes(dh, nj, n, G) > 65536) --G;
  return G;
}

extern "C" size_t hp_sformer_attention_backward_grouped_workspace_bytes(int B, int heads, int dh, int Ntok, int num_joints,
                                                                        int groups) {
  return hp_sformer_attention_backward_workspace_bytes(B, heads, dh, Ntok, num_joints, groups);
}

extern "C" int hp_sformer_attention_backward_grouped(const float* Q, const float* K, const float* K0, const float* V,
                                                     const float* out, const float* dout, const float* lse, float* dQ, float* dK,
                                                     float* dK0, float* dV, int B, int heads, int dh, int Ntok, int num_joints,
                                                     int patches_per_group, int groups, void* workspace, size_t workspace_bytes,
                                                     void* stream) {
  HP_REQUIRE(Q && K && K0 && V && out && dout && lse && dQ && dK && dK0 && dV && workspace,
             "hp_sformer_attention_backward_grouped: null argument");
  HP_REQUIRE(B > 0 && heads > 0 && groups > 0 && patches_per_group > 0 && num_joints >= 0 && num_joints <= 32 &&
                 Ntok == num_joints + groups * patches_per_group,
             "hp_sformer_attention_backward_grouped: bad token layout");
  if (dh != 16 && dh != 24 && dh != 32) {
    set_error("hp_sformer_attention_backward_grouped: dim_head %d not built (16, 24, 32)", dh);
    return HP_ERR_UNSUPPORTED;
  }
  if (patches_per_group > GROUPED_MAX_N) {
    set_error("hp_sformer_attention_backward_grouped: %d tokens per group not built (at most %d; use hp_sformer_attention_backward)",
              patches_per_group, GROUPED_MAX_N);
    return HP_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < hp_sformer_attention_backward_grouped_workspace_bytes(B, heads, dh, Ntok, num_joints, groups)) {
    set_error("hp_sformer_attention_backward_grouped: workspace too small");
    return HP_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int BH = B * heads, nj = num_joints, n = patches_per_group;
  float* delta = (float*)workspace;
  float* ws_dk = delta + (size_t)BH * Ntok;
  float* ws_dv = ws_dk + (size_t)BH * groups * nj * dh;
  float* part = ws_dv + (size_t)BH * groups * nj * dh;
  const int G = grouped_groups_per_wg(dh, nj, n, groups);
  const int wg_per_bh = (groups + G - 1) / G;
  const long nwg = (long)BH * wg_per_bh;
  HP_REQUIRE(nwg < (1l << 31), "hp_sformer_attention_backward_grouped: grid too large");
  const size_t lds = grouped_lds_bytes(dh, nj, n, G);
  {
    HP_PROF("sformer_attn_bwd_delta", st);
    hipLaunchKernelGGL(k_attn_bwd_delta, dim3(bgrid((long)BH * Ntok)), dim3(SB), 0, st, out, dout, delta, B, heads, dh, Ntok);
  }
  {
    HP_PROF("sformer_attn_bwd_grouped", st);
#define HP_GRP(D) hipLaunchKernelGGL((k_attn_bwd_grouped<D>), dim3((unsigned)nwg), dim3(SB), lds, st, Q, K, K0, V, dout, lse, delta, dQ, dK, dK0, dV, ws_dk, ws_dv, heads, Ntok, nj, n, groups, G, wg_per_bh)
    if (dh == 32) HP_GRP(32);
    else if (dh == 24) HP_GRP(24);
    else HP_GRP(16);
#undef HP_GRP
  }
  if (nj > 0) {
    HP_PROF("sformer_attn_bwd_joint_keys", st);
    const long total = (long)BH * nj * dh;
    hipLaunchKernelGGL(k_attn_bwd_joint_keys, dim3((unsigned)((total + SB - 1) / SB)), dim3(SB), 0, st, ws_dk, ws_dv, dK, dV, BH, Ntok, dh,
                       nj, groups);
  }
  if (nj > 0) {
    HP_PROF("sformer_attn_bwd_dq_joint", st);
    const int nsplit = std::max(1, std::min(DQ_SPLITS, (Ntok + 255) / 256));
    const dim3 gj(nsplit, BH);
#define HP_DQJ(D) hipLaunchKernelGGL((k_attn_bwd_dq_joint<D>), gj, dim3(SB), 0, st, Q, K0, V, dout, lse, delta, part, heads, Ntok, nj)
    if (dh == 32) HP_DQJ(32);
    else if (dh == 24) HP_DQJ(24);
    else HP_DQJ(16);
#undef HP_DQJ
    const long total = (long)BH * nj * dh;
    hipLaunchKernelGGL(k_attn_bwd_dq_joint_merge, dim3((unsigned)((total + SB - 1) / SB)), dim3(SB), 0, st, part, dQ, BH, Ntok, dh, nj,
                       nsplit);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_gelu_backward(const float* u, const float* dy, float* du, long n, void* stream) {
  HP_REQUIRE(u && dy && du && n > 0, "hp_gelu_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("gelu_bwd", st);
  hipLaunchKernelGGL(k_gelu_bwd, dim3(bgrid(n)), dim3(SB), 0, st, u, dy, du, n);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_sformer_qkv_prepare_backward(const float* dQ, const float* dK, const float* dK0, const float* dV, float* dqkv, int B,
                                               int Ntok, int heads, int dh, int num_joints, int patches_per_frame, float scale,
                                               const float* sin_t, const float* cos_t, int rot_dim, void* stream) {
  HP_REQUIRE(dQ && dK && dK0 && dV && dqkv && (rot_dim == 0 || (sin_t && cos_t)) && rot_dim <= dh && rot_dim % 2 == 0 &&
                 patches_per_frame > 0,
             "hp_sformer_qkv_prepare_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("sformer_qkv_prepare_bwd", st);
  hipLaunchKernelGGL(k_qkv_prepare_bwd, dim3(bgrid((long)B * Ntok * heads * dh)), dim3(SB), 0, st, dQ, dK, dK0, dV, dqkv, B, Ntok, heads,
                     dh, num_joints, patches_per_frame, scale, sin_t, cos_t, rot_dim);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" size_t hp_layernorm_backward_workspace_bytes(long rows, int dim) {
  return sizeof(float) * (size_t)ln_blocks(rows) * 2 * dim;
}

extern "C" int hp_layernorm_backward(const float* x, const float* dy, float* dx, float* dgamma, float* dbeta, long rows, int dim,
                                     const float* gamma, float eps, int rows_per_batch, long batch_stride_rows, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  HP_REQUIRE(x && dy && dx && dgamma && dbeta && gamma && workspace && rows > 0 && dim > 0 && dim <= 1024,
             "hp_layernorm_backward: bad argument (dim <= 1024)");
  if (workspace_bytes < hp_layernorm_backward_workspace_bytes(rows, dim)) {
    set_error("hp_layernorm_backward: workspace too small");
    return HP_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ln_blocks(rows);
  float* part = (float*)workspace;
  HP_PROF("layernorm_bwd", st);
  hipLaunchKernelGGL(k_layernorm_bwd, dim3(nblk), dim3(SB), sizeof(float) * 8 * dim, st, x, dy, dx, rows, dim, gamma, eps, rows_per_batch,
                     batch_stride_rows, part);
  hipLaunchKernelGGL(k_sum_partials, dim3((2 * dim + SB - 1) / SB), dim3(SB), 0, st, part, dgamma, dbeta, nblk, 2 * dim, dim);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_geglu_backward(const float* u, const float* dg, float* du, long rows, int hidden, void* stream) {
  HP_REQUIRE(u && dg && du && rows > 0 && hidden > 0, "hp_geglu_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("geglu_bwd", st);
  hipLaunchKernelGGL(k_geglu_bwd, dim3(bgrid(rows * hidden)), dim3(SB), 0, st, u, dg, du, rows, hidden);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_geglu_backward_dropout(const float* u, const float* dg, float* du, long rows, int hidden, double p,
                                         unsigned long long seed, unsigned long long stream, void* stream_handle) {
  const char* who = "hp_geglu_backward_dropout";
  HP_REQUIRE(u && dg && du && rows > 0 && hidden > 0, "%s: bad argument (null pointer, rows or hidden <= 0)", who);
  DropoutParams d;
  const int rc = dropout_params(who, rows * hidden, 0, p, seed, stream, &d);
  if (rc != HP_OK) return rc;
  hipStream_t st = (hipStream_t)stream_handle;
  HP_PROF("geglu_bwd_dropout", st);
  const int vec = hidden % 4 == 0 && ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(dg) | reinterpret_cast<uintptr_t>(du)) & 15u) == 0;
  hipLaunchKernelGGL(k_geglu_bwd_dropout, dim3(bgrid((rows * hidden + 3) / 4)), dim3(SB), 0, st, u, dg, du, rows, hidden, vec, d);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_gelu_backward_dropout(const float* u, const float* dy, float* du, long n, double p, unsigned long long seed,
                                        unsigned long long stream, void* stream_handle) {
  const char* who = "hp_gelu_backward_dropout";
  HP_REQUIRE(u && dy && du && n > 0, "%s: bad argument (null pointer or n <= 0)", who);
  DropoutParams d;
  const int rc = dropout_params(who, n, 0, p, seed, stream, &d);
  if (rc != HP_OK) return rc;
  hipStream_t st = (hipStream_t)stream_handle;
  HP_PROF("gelu_bwd_dropout", st);
  hipLaunchKernelGGL(k_gelu_bwd_dropout, dim3(bgrid((n + 3) / 4)), dim3(SB), 0, st, u, dy, du, n, d);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" size_t hp_linear_backward_data_workspace_bytes(int K, int N) { return sizeof(float) * (size_t)K * N; }

extern "C" int hp_linear_backward_data(const float* dy, const float* w, const float* addend, float* dx, long M, int K, int N,
                                       int precision, void* workspace, size_t workspace_bytes, void* stream) {
  HP_REQUIRE(dy && w && dx && workspace && M >= 1 && M < (1l << 31) && K >= 4 && N >= 1 && addend != dx,
             "hp_linear_backward_data: bad argument");
  if (workspace_bytes < hp_linear_backward_data_workspace_bytes(K, N)) {
    set_error("hp_linear_backward_data: workspace too small");
    return HP_ERR_WORKSPACE;
  }
  hp_conv_desc d{1, 1, 1, (int)M, K, N, 1, 1, 0, 0, precision, 0};
  int rc = hp_conv3d_pack_weight(&d, w, nullptr, workspace, stream);
  if (rc) return rc;
  return hp_conv3d_backward_data(&d, dy, (const float*)workspace, dx, addend, stream);
}

extern "C" size_t hp_linear_backward_weight_workspace_bytes(long M, int K, int N) {
  return sizeof(float) * ((size_t)K * N + (size_t)colsum_chunks(M) * N);
}

extern "C" int hp_linear_backward_weight(const float* x, const float* dy, float* dw, float* db, long M, int K, int N, int precision,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  HP_REQUIRE(x && dy && dw && workspace && M >= 1 && M < (1l << 31) && K >= 4 && N >= 1, "hp_linear_backward_weight: bad argument");
  if (workspace_bytes < hp_linear_backward_weight_workspace_bytes(M, K, N)) {
    set_error("hp_linear_backward_weight: workspace too small");
    return HP_ERR_WORKSPACE;
  }
  hp_conv_desc d{1, 1, 1, (int)M, K, N, 1, 1, 0, 0, precision, 0};
  float* dw_packed = (float*)workspace;
  int rc = hp_conv3d_backward_weight(&d, x, dy, dw_packed, stream);
  if (rc) return rc;
  rc = hp_conv3d_unpack_wgrad(&d, dw_packed, dw, stream);
  if (rc) return rc;
  if (db) {
    hipStream_t st = (hipStream_t)stream;
    const int chunks = colsum_chunks(M);
    const long per = (M + chunks - 1) / chunks;
    float* part = dw_packed + (size_t)K * N;
    HP_PROF("linear_bias_bwd", st);
    hipLaunchKernelGGL(k_colsum_partial, dim3((N + SB - 1) / SB, chunks), dim3(SB), 0, st, dy, part, M, N, (long)N, per);
    hipLaunchKernelGGL(k_sum_partials, dim3((N + SB - 1) / SB), dim3(SB), 0, st, part, db, db, chunks, N, N);
    HP_CHECK_HIP(hipGetLastError());
  }
  return HP_OK;
}

extern "C" int hp_sformer_unpatchify(const float* tokens, float* video, int B, int frames, int C, int H, int W, int patch, void* stream) {
  HP_REQUIRE(tokens && video && patch > 0 && H % patch == 0 && W % patch == 0, "hp_sformer_unpatchify: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("sformer_unpatchify", st);
  hipLaunchKernelGGL(k_unpatchify, dim3(bgrid((long)B * frames * C * H * W)), dim3(SB), 0, st, tokens, video, B, frames, C, H, W, patch);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_sformer_joint_token_backward(const float* dx, float* djt, int B, int num_joints, long Ntok, int dim, void* stream) {
  HP_REQUIRE(dx && djt && B > 0 && num_joints > 0 && dim > 0 && Ntok >= num_joints, "hp_sformer_joint_token_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("sformer_joint_token_bwd", st);
  hipLaunchKernelGGL(k_joint_token_bwd, dim3((num_joints * dim + SB - 1) / SB), dim3(SB), 0, st, dx, djt, B, num_joints, Ntok, dim);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
