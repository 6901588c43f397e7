// Entry of FeatureExtraction at stride 1 or 2 and any channel count (models/feature_extraction.py:122-171):
//
//   a   = Conv3d(1, C, 3, stride s, bias)(ReplicationPad3d(1)(x))     learned branch, (B,C,Do,Ho,Wo)
//   box = conv3d(x, weights(1,1,3,3,3), stride s, padding 1)          zero-padded box filter, (B,1,Do,Ho,Wo)
//   y   = ResConv(ResConv(a)) + box                                   box broadcast over the C channels
//
// x (B,1,D,H,W) is the large tensor (the outputs are 1/s^3 of its volume each), so ONE kernel reads it once and writes both
// branches.  The kernels are memory-bound stencils in the mould of k_stencil_c1 (dconv_kernels.hip): a thread owns NX
// consecutive output x of one output row (4 at stride 1, 2 at stride 2: in both cases the input columns 4t-1 .. 4t+3(+1), i.e.
// one aligned 16-byte load plus one or two border words) and slides along z with its 3 planes x 3 rows x NC columns in
// registers.  Both branches read the SAME clamped window: the learned branch uses it as it is (replicate padding = clamped
// read position), the box branch zeroes the taps whose position lay outside (row / column masks fixed per thread, plane mask
// per step).  Weights are wave-uniform: broadcast LDS reads in the forward, register sums in the backward.  Channels are
// taken in groups of CG (1, 2 or 4) accumulator sets per output; a wider layer walks its z range once per group (the slab
// of one workgroup is re-read from cache, not from HBM).
// Exact fp32 whatever the thin-channel precision switch says: cin == 1.
//
// Backward: weight / bias gradients are per-workgroup partial sums added in a fixed order by a second kernel (no float
// atomics: two runs are bit-identical); the input gradient is a gather over the output-sized gradients, see k_fe_entry_dgrad.
#include <algorithm>
#include <cstdint>

#include "hp_internal.h"

namespace hp {

template <int S>
struct FeTile {
  static constexpr int NX = S == 1 ? 4 : 2;   // outputs per thread along x
  static constexpr int NC = S == 1 ? 6 : 5;   // window columns: input x 4t-1 .. 4t+NC-2
  static constexpr int TX = 64 * NX;          // outputs per workgroup along x
  static constexpr int TY = 4;                // output rows per workgroup (one per wave)
};

// The window walk shared by the forward and the weight-gradient kernel: clamped addressing of the 3 x NC window of one
// thread, fixed for the whole z walk, and the masks of the zero-padded branch.  Loads are raw buffer loads on a descriptor
// of the sample's true extent: a per-lane column offset (VGPR) plus a plane + row offset that is the same for the whole
// wave (a wave is one output row; SGPR), so a window element costs no 64-bit address arithmetic and no address registers.
// Every offset is clamped into the volume; the descriptor's range check is a second line of defence only.
template <int S>
struct FeWindow {
  static constexpr int NC = FeTile<S>::NC;
  unsigned rbyte[3], cbyte[NC], qbyte, plane_bytes;
  bool rok[3], cok[NC];
  bool vec;
  __amdgpu_buffer_rsrc_t rs;
  // oy must be wave-uniform
  __device__ __forceinline__ void init(const float* xb, int ox0, int oy, int D, int H, int W, bool vec_) {
    const int ix0 = ox0 * S;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int yy = oy * S - 1 + r;
      rok[r] = (unsigned)yy < (unsigned)H;
      rbyte[r] = (unsigned)(min(max(yy, 0), H - 1) * W) * 4u;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int xx = ix0 - 1 + c;
      cok[c] = (unsigned)xx < (unsigned)W;
      cbyte[c] = (unsigned)min(max(xx, 0), W - 1) * 4u;
    }
    vec = vec_;   // rows of whole quads at a 16-byte aligned base: columns ix0 .. ix0+3 (< W for every live lane) in one load
    qbyte = (unsigned)min(ix0, max(W - 4, 0)) * 4u;
    plane_bytes = (unsigned)(H * W) * 4u;
    rs = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, hp_extent((long)D * H * W, 0, 4), 0x00020000);
  }
  // plane zin (wave-uniform) of the sample, read clamped into the volume
  __device__ __forceinline__ void load(int zin, int D, float (&v)[3][NC]) const {
    const unsigned zo = (unsigned)min(max(zin, 0), D - 1) * plane_bytes;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const unsigned so = __builtin_amdgcn_readfirstlane(zo + rbyte[r]);   // uniform by construction; says so to the compiler
      if (vec) {
        const float4 q = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, qbyte, so, 0));
        v[r][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, cbyte[0], so, 0));
        v[r][1] = q.x; v[r][2] = q.y; v[r][3] = q.z; v[r][4] = q.w;
        if constexpr (NC == 6) v[r][5] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, cbyte[5], so, 0));
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[r][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, cbyte[c], so, 0));
      }
    }
  }
};

// grid: (B * zsplit, ceil(Ho / 4), ceil(Wo / TX)), 256 threads: wave = output row, lane = NX outputs.
// The (CG + 1) * 27 weights of a channel group live in LDS, one 4 * CG-byte record per tap (a broadcast read per tap and
// step): as scalars they are more than the SGPR file holds next to the window addressing, and hoisted into VGPRs they would
// halve the occupancy of a kernel whose only job is to keep loads in flight.  `lds0` is an opaque zero added to the LDS
// offsets inside the loop so that the reads stay there.
template <int S, int CG>
__global__ __launch_bounds__(256, 2) void k_fe_entry_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ wbox,
                                                         float* __restrict__ a, float* __restrict__ box, int C, int D, int H, int W,
                                                         int Do, int Ho, int Wo, int zsplit, int zchunk, int vec_in, int vec_out) {
  constexpr int NX = FeTile<S>::NX, NC = FeTile<S>::NC;
  __shared__ __attribute__((aligned(16))) float sw[27 * CG];
  __shared__ float swb[27], sbias[CG];
  const int tx = threadIdx.x & 63, ty = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ox0 = (blockIdx.z * 64 + tx) * NX, oy = blockIdx.y * FeTile<S>::TY + ty;
  const int b = blockIdx.x / zsplit, zb = (blockIdx.x % zsplit) * zchunk, ze = min(Do, zb + zchunk);
  const bool live = oy < Ho && ox0 < Wo;   // idle lanes and rows only help staging the weights
  FeWindow<S> win;
  const float* xb = x + (long)b * D * H * W;
  win.init(xb, live ? ox0 : 0, oy < Ho ? oy : 0, D, H, W, vec_in != 0);   // (the row stays wave-uniform)
  const long Vo = (long)Do * Ho * Wo;
  for (int c0 = 0; c0 < C; c0 += CG) {
    __syncthreads();   // the previous group's readers are done
    if (threadIdx.x < 27 * CG) {
      const int t = threadIdx.x / CG, k = threadIdx.x % CG;
      sw[threadIdx.x] = c0 + k < C ? w[(long)(c0 + k) * 27 + t] : 0.f;
    }
    if (threadIdx.x < 27) swb[threadIdx.x] = wbox[threadIdx.x];
    if (threadIdx.x < CG) sbias[threadIdx.x] = (bias && c0 + threadIdx.x < C) ? bias[c0 + threadIdx.x] : 0.f;
    __syncthreads();
    if (!live) continue;
    float bv[CG];
#pragma unroll
    for (int k = 0; k < CG; ++k) bv[k] = sbias[k];
    float p0[3][NC], p1[3][NC], p2[3][NC];
    // output plane z reads input planes S*z-1 .. S*z+1
    win.load(zb * S - 1, D, p0);
    win.load(zb * S, D, p1);
    win.load(zb * S + 1, D, p2);
    for (int z = zb; z < ze; ++z) {
      // request the planes of the next step before this step's arithmetic (the last step re-reads clamped planes)
      float n0[3][NC], n1[3][NC];
      if constexpr (S == 2) win.load(z * S + 2, D, n0);
      win.load(z * S + S + 1, D, n1);
      int lds0 = 0;
      asm volatile("" : "+v"(lds0));
      float acc[CG][NX], ab[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        ab[i] = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) acc[k][i] = bv[k];
      }
      auto plane = [&](const float (&pp)[3][NC], int dz) {
        const bool zok = (unsigned)(z * S - 1 + dz) < (unsigned)D;   // uniform
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          // zero-padded branch: plane and row masks go into the (uniform) weight, column masks into the window values
          const bool zrok = zok && win.rok[dy];
          float vm[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) vm[c] = win.cok[c] ? pp[dy][c] : 0.f;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int t = dz * 9 + dy * 3 + dx;
            float wk[CG];
            if constexpr (CG == 4) {
              const float4 q = *reinterpret_cast<const float4*>(&sw[t * 4 + lds0]);
              wk[0] = q.x; wk[1] = q.y; wk[2] = q.z; wk[3] = q.w;
            } else if constexpr (CG == 2) {
              const float2 q = *reinterpret_cast<const float2*>(&sw[t * 2 + lds0]);
              wk[0] = q.x; wk[1] = q.y;
            } else {
              wk[0] = sw[t + lds0];
            }
            const float wz = zrok ? swb[t + lds0] : 0.f;
#pragma unroll
            for (int i = 0; i < NX; ++i) {
#pragma unroll
              for (int k = 0; k < CG; ++k) acc[k][i] = fmaf(wk[k], pp[dy][i * S + dx], acc[k][i]);
              ab[i] = fmaf(wz, vm[i * S + dx], ab[i]);
            }
          }
        }
      };
      plane(p0, 0);
      plane(p1, 1);
      plane(p2, 2);
      const long ob = ((long)z * Ho + oy) * Wo + ox0;
#pragma unroll
      for (int k = 0; k < CG; ++k) {
        if (c0 + k >= C) continue;
        float* dst = a + ((long)b * C + c0 + k) * Vo + ob;
        if (vec_out) {   // Wo % NX == 0 and aligned bases: a lane's NX outputs are one aligned store
          if constexpr (NX == 4) *reinterpret_cast<float4*>(dst) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
          else *reinterpret_cast<float2*>(dst) = make_float2(acc[k][0], acc[k][1]);
        } else {
#pragma unroll
          for (int i = 0; i < NX; ++i)
            if (ox0 + i < Wo) dst[i] = acc[k][i];
        }
      }
      if (c0 == 0) {
        float* dst = box + (long)b * Vo + ob;
        if (vec_out) {
          if constexpr (NX == 4) *reinterpret_cast<float4*>(dst) = make_float4(ab[0], ab[1], ab[2], ab[3]);
          else *reinterpret_cast<float2*>(dst) = make_float2(ab[0], ab[1]);
        } else {
#pragma unroll
          for (int i = 0; i < NX; ++i)
            if (ox0 + i < Wo) dst[i] = ab[i];
        }
      }
      // slide: S new planes
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if constexpr (S == 1) {
            p0[r][c] = p1[r][c]; p1[r][c] = p2[r][c]; p2[r][c] = n1[r][c];
          } else {
            p0[r][c] = p2[r][c]; p1[r][c] = n0[r][c]; p2[r][c] = n1[r][c];
          }
        }
    }
  }
}

// Weight / bias gradients of both branches, same grid and walk as the forward.  Per workgroup and channel group the threads'
// register sums are added across the wave (xor shuffles), then across the four waves in a fixed order, and written as ONE
// partial record of P = 28 * C + 27 floats: channel c at [c * 28, c * 28 + 27) with its bias gradient at c * 28 + 27, the box
// filter at [28 * C, 28 * C + 27).  k_fe_entry_wreduce adds the records.
template <int S, int CG>
__global__ __launch_bounds__(256, 2) void k_fe_entry_wgrad(const float* __restrict__ x, const float* __restrict__ ga,
                                                        const float* __restrict__ gbox, float* __restrict__ partial, int C, int D,
                                                        int H, int W, int Do, int Ho, int Wo, int zsplit, int zchunk, int vec_in) {
  constexpr int NX = FeTile<S>::NX, NC = FeTile<S>::NC;
  __shared__ float sred[4][CG * 28 + 27];
  const int tx = threadIdx.x & 63, ty = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ox0 = (blockIdx.z * 64 + tx) * NX, oy = blockIdx.y * FeTile<S>::TY + ty;
  const int b = blockIdx.x / zsplit, zb = (blockIdx.x % zsplit) * zchunk, ze = min(Do, zb + zchunk);
  const bool live = oy < Ho && ox0 < Wo;   // idle lanes stay for the reductions and contribute zeros
  FeWindow<S> win;
  const float* xb = x + (long)b * D * H * W;
  win.init(xb, live ? ox0 : 0, oy < Ho ? oy : 0, D, H, W, vec_in != 0);   // (the row stays wave-uniform)
  const long Vo = (long)Do * Ho * Wo;
  const int P = 28 * C + 27;
  const long wg = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  float* rec = partial + wg * P;
  for (int c0 = 0; c0 < C; c0 += CG) {
    float dwa[CG][27], dba[CG], dwb[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      dwb[t] = 0.f;
#pragma unroll
      for (int k = 0; k < CG; ++k) dwa[k][t] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < CG; ++k) dba[k] = 0.f;
    if (live) {
      float p0[3][NC], p1[3][NC], p2[3][NC];
      win.load(zb * S - 1, D, p0);
      win.load(zb * S, D, p1);
      win.load(zb * S + 1, D, p2);
      for (int z = zb; z < ze; ++z) {
        float n0[3][NC], n1[3][NC];
        if constexpr (S == 2) win.load(z * S + 2, D, n0);
        win.load(z * S + S + 1, D, n1);
        const long ob = ((long)z * Ho + oy) * Wo + ox0;
        float g[CG][NX], gb[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          const bool in = ox0 + i < Wo;
          gb[i] = (in && c0 == 0) ? gbox[(long)b * Vo + ob + i] : 0.f;
#pragma unroll
          for (int k = 0; k < CG; ++k) {
            g[k][i] = (in && c0 + k < C) ? ga[((long)b * C + c0 + k) * Vo + ob + i] : 0.f;
            dba[k] += g[k][i];
          }
        }
        const bool zok[3] = {(unsigned)(z * S - 1) < (unsigned)D, true, (unsigned)(z * S + 1) < (unsigned)D};
        auto plane = [&](const float (&pp)[3][NC], int dz) {
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
              const int t = dz * 9 + dy * 3 + dx;
#pragma unroll
              for (int i = 0; i < NX; ++i) {
                const float v = pp[dy][i * S + dx];
#pragma unroll
                for (int k = 0; k < CG; ++k) dwa[k][t] = fmaf(g[k][i], v, dwa[k][t]);
                const bool ok = zok[dz] && win.rok[dy] && win.cok[i * S + dx];
                dwb[t] = fmaf(gb[i], ok ? v : 0.f, dwb[t]);
              }
            }
        };
        plane(p0, 0);
        plane(p1, 1);
        plane(p2, 2);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if constexpr (S == 1) {
              p0[r][c] = p1[r][c]; p1[r][c] = p2[r][c]; p2[r][c] = n1[r][c];
            } else {
              p0[r][c] = p2[r][c]; p1[r][c] = n0[r][c]; p2[r][c] = n1[r][c];
            }
          }
      }
    }
    // wave sums (all 64 lanes are here), then the four waves in a fixed order
    auto wsum = [&](float v) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      return v;
    };
#pragma unroll
    for (int k = 0; k < CG; ++k) {
#pragma unroll
      for (int t = 0; t < 27; ++t) {
        const float s = wsum(dwa[k][t]);
        if (tx == 0) sred[ty][k * 28 + t] = s;
      }
      const float s = wsum(dba[k]);
      if (tx == 0) sred[ty][k * 28 + 27] = s;
    }
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      const float s = wsum(dwb[t]);
      if (tx == 0) sred[ty][CG * 28 + t] = s;
    }
    __syncthreads();
    const int q = threadIdx.x;
    if (q < CG * 28 + 27) {
      const float s = (sred[0][q] + sred[1][q]) + (sred[2][q] + sred[3][q]);
      if (q < CG * 28) {
        if (c0 + q / 28 < C) rec[(c0 + q / 28) * 28 + q % 28] = s;
      } else if (c0 == 0) {
        rec[28 * C + (q - CG * 28)] = s;
      }
    }
    __syncthreads();
  }
}

// dw / dbias / dweights = sum of the nwg partial records, in a fixed order: 16 entries x 16 strided slices per workgroup,
// each slice added sequentially, the slices added in index order.
__global__ __launch_bounds__(256) void k_fe_entry_wreduce(const float* __restrict__ partial, long nwg, int C, float* __restrict__ dw,
                                                          float* __restrict__ dbias, float* __restrict__ dwbox) {
  __shared__ float s[16][17];
  const int P = 28 * C + 27;
  const int kl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int k = blockIdx.x * 16 + kl;
  float acc = 0.f;
  if (k < P)
    for (long i = sl; i < nwg; i += 16) acc += partial[i * P + k];
  s[sl][kl] = acc;
  __syncthreads();
  if (sl == 0 && k < P) {
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) v += s[j][kl];
    if (k < 28 * C) {
      const int c = k / 28, t = k % 28;
      if (t < 27) dw[c * 27 + t] = v;
      else if (dbias) dbias[c] = v;
    } else {
      dwbox[k - 28 * C] = v;
    }
  }
}

// Input gradient: the adjoint of both branches in one pass over the output-sized gradients, as a gather (each input voxel
// sums the (output, tap) pairs that read it: no atomics).  Per axis, input coordinate i of an extent n with no outputs is read
//   directly   by tap t of output o = (i + 1 - t) / s, where that division is exact and o < no        (slots 0 .. 2), and,
//   in the replicate-padded branch only, through the taps that pointed outside the volume and were clamped onto the border:
//   i == 0      by tap 0 of output 0 (position -1)                                                          (slot 3),
//   i == n - 1  by tap 2 of output no - 1 when s * (no - 1) + 1 == n (position n)                            (slot 4).
// At stride 2 the last condition is the parity of n: for even n the last window reads n-3 .. n-1 and never touches the right
// pad; for odd n it reads n-2 .. n and the tap at n folds onto n-1.  No window reaches further out than -1 or n.  The 3-D sum
// runs over the product of the three axes' slots; the zero-padded box branch takes part where all three are direct.
// grid: (B * D, ceil(H / 4), ceil(W / 64)): z and y slots are wave-uniform, x slots per lane.
struct FeSlots {
  int o[5];
  bool on[5];
};
template <int S>
__device__ __forceinline__ FeSlots fe_slots(int i, int n, int no) {
  FeSlots p;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int q = i + 1 - t;
    p.on[t] = q >= 0 && q % S == 0 && q / S < no;
    p.o[t] = p.on[t] ? q / S : 0;
  }
  p.on[3] = i == 0;
  p.o[3] = 0;
  p.on[4] = i == n - 1 && S * (no - 1) + 1 == n;
  p.o[4] = no - 1;
  return p;
}

template <int S>
__global__ __launch_bounds__(256) void k_fe_entry_dgrad(const float* __restrict__ ga, const float* __restrict__ gbox,
                                                        const float* __restrict__ w, const float* __restrict__ wbox,
                                                        float* __restrict__ gx, int C, int D, int H, int W, int Do, int Ho, int Wo) {
  constexpr int TAP[5] = {0, 1, 2, 0, 2};
  const int ix = blockIdx.z * 64 + (threadIdx.x & 63), iy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.x / D, iz = blockIdx.x % D;
  if (iy >= H || ix >= W) return;
  const FeSlots sz = fe_slots<S>(iz, D, Do), sy = fe_slots<S>(iy, H, Ho), sx = fe_slots<S>(ix, W, Wo);
  const long Vo = (long)Do * Ho * Wo;
  const float* gab = ga + (long)b * C * Vo;
  const float* gbb = gbox + (long)b * Vo;
  float acc = 0.f;
#pragma unroll
  for (int jz = 0; jz < 5; ++jz) {
    if (!sz.on[jz]) continue;
#pragma unroll
    for (int jy = 0; jy < 5; ++jy) {
      if (!sy.on[jy]) continue;
#pragma unroll
      for (int jx = 0; jx < 5; ++jx) {
        if (!sx.on[jx]) continue;
        const int tap = TAP[jz] * 9 + TAP[jy] * 3 + TAP[jx];
        const long off = ((long)sz.o[jz] * Ho + sy.o[jy]) * Wo + sx.o[jx];
        for (int c = 0; c < C; ++c) acc = fmaf(gab[c * Vo + off], w[c * 27 + tap], acc);
        if (jz < 3 && jy < 3 && jx < 3) acc = fmaf(gbb[off], wbox[tap], acc);
      }
    }
  }
  gx[(((long)b * D + iz) * H + iy) * W + ix] = acc;
}

// The join and its adjoint: y = t + box broadcast over the channels; gbox = sum_c gy (channels in index order), gt = gy.
// Output-sized tensors only (1/8 of the input volume at stride 2).  grid: (ceil(V / (256 * 4)), B * C) / (.., B).
__global__ __launch_bounds__(256) void k_bcast_add(const float* __restrict__ t, const float* __restrict__ box, float* __restrict__ y,
                                                   int C, long V, int vec) {
  const long v0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  const long bc = blockIdx.y, b = bc / C;
  if (v0 >= V) return;
  if (vec) {
    const float4 p = *reinterpret_cast<const float4*>(t + bc * V + v0), q = *reinterpret_cast<const float4*>(box + b * V + v0);
    *reinterpret_cast<float4*>(y + bc * V + v0) = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
  } else {
    for (long v = v0; v < min(V, v0 + 4); ++v) y[bc * V + v] = t[bc * V + v] + box[b * V + v];
  }
}

__global__ __launch_bounds__(256) void k_channel_sum(const float* __restrict__ gy, float* __restrict__ gbox, int C, long V, int vec) {
  const long v0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  const long b = blockIdx.y;
  if (v0 >= V) return;
  if (vec) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < C; ++c) {
      const float4 p = *reinterpret_cast<const float4*>(gy + (b * C + c) * V + v0);
      s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    *reinterpret_cast<float4*>(gbox + b * V + v0) = s;
  } else {
    for (long v = v0; v < min(V, v0 + 4); ++v) {
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += gy[(b * C + c) * V + v];
      gbox[b * V + v] = s;
    }
  }
}

namespace {
struct FeGeom {
  int Do, Ho, Wo, tiles_x, tiles_y, zsplit, zchunk;
  long nwg;
};
// The z range of a workgroup depends on the sample's extents only (not on B or C), so that the partial-record count, and with
// it the workspace, is linear in B: about 1024 workgroups per sample where the volume allows and at most ceil(Do / 8) chunks, i.e.
// about 8 output planes or more each (Do = 9 gives 5 + 4; a chunk re-reads one or two halo planes).
FeGeom fe_geom(int B, int D, int H, int W, int s) {
  FeGeom q;
  q.Do = (D - 1) / s + 1;
  q.Ho = (H - 1) / s + 1;
  q.Wo = (W - 1) / s + 1;
  const int tx = s == 1 ? FeTile<1>::TX : FeTile<2>::TX;
  q.tiles_x = (q.Wo + tx - 1) / tx;
  q.tiles_y = (q.Ho + 3) / 4;
  const long cols = (long)q.tiles_x * q.tiles_y;
  q.zsplit = (int)std::max<long>(1, std::min<long>((q.Do + 7) / 8, (1024 + cols - 1) / cols));
  q.zchunk = (q.Do + q.zsplit - 1) / q.zsplit;
  q.zsplit = (q.Do + q.zchunk - 1) / q.zchunk;
  q.nwg = cols * q.zsplit * B;
  return q;
}
bool fe_shape_ok(int B, int C, int D, int H, int W, int s) {
  return B >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && (s == 1 || s == 2) && (long)D * H * W < (1l << 29);
}
bool aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }
}  // namespace

}  // namespace hp

using namespace hp;

#define HP_FE_ARGS(who)                                                                                                     \
  HP_REQUIRE(stride == 1 || stride == 2, who ": stride must be 1 or 2 (got %d)", stride);                                   \
  HP_REQUIRE(C >= 1, who ": C must be at least 1 (got %d)", C);                                                             \
  HP_REQUIRE(B >= 1 && D >= 1 && H >= 1 && W >= 1, who ": extents must be positive (B %d, D %d, H %d, W %d)", B, D, H, W);  \
  HP_REQUIRE((long)D * H * W < (1l << 29), who ": a volume of 2^29 voxels or more per sample is not supported (%d x %d x %d)", D, H, W)

extern "C" int hp_fe_entry_forward(const float* x, const float* w, const float* bias, const float* box_w, float* a, float* box,
                                   int B, int C, int D, int H, int W, int stride, void* stream) {
  HP_FE_ARGS("hp_fe_entry_forward");
  HP_REQUIRE(x && w && box_w && a && box, "hp_fe_entry_forward: null pointer (x, w, box_w, a and box are required)");
  const FeGeom q = fe_geom(B, D, H, W, stride);
  HP_REQUIRE((long)B * q.zsplit < (1l << 31) && q.tiles_y < 65536 && q.tiles_x < 65536, "hp_fe_entry_forward: volume too large for the grid");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("fe_entry_fwd", st);
  const int nx = stride == 1 ? 4 : 2;
  const int vec_in = (W % 4 == 0 && aligned(x, 16)) ? 1 : 0;
  const int vec_out = (q.Wo % nx == 0 && aligned(a, 4 * nx) && aligned(box, 4 * nx)) ? 1 : 0;
  dim3 grid((unsigned)(B * q.zsplit), (unsigned)q.tiles_y, (unsigned)q.tiles_x);
#define HP_FE_FWD(S, CG)                                                                                                        \
  hipLaunchKernelGGL((k_fe_entry_fwd<S, CG>), grid, dim3(256), 0, st, x, w, bias, box_w, a, box, C, D, H, W, q.Do, q.Ho, q.Wo, \
                     q.zsplit, q.zchunk, vec_in, vec_out)
  // channel group per walk: 4 accumulator sets at stride 2; 2 at stride 1, whose wider window leaves no registers for more
  if (stride == 1) {
    if (C == 1) HP_FE_FWD(1, 1);
    else HP_FE_FWD(1, 2);
  } else {
    if (C == 1) HP_FE_FWD(2, 1);
    else if (C == 2) HP_FE_FWD(2, 2);
    else HP_FE_FWD(2, 4);
  }
#undef HP_FE_FWD
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" size_t hp_fe_entry_backward_workspace_bytes(int B, int C, int D, int H, int W, int stride) {
  if (!fe_shape_ok(B, C, D, H, W, stride)) return 0;
  const FeGeom q = fe_geom(B, D, H, W, stride);
  return sizeof(float) * (size_t)q.nwg * (size_t)(28 * C + 27);
}

extern "C" int hp_fe_entry_backward(const float* x, const float* ga, const float* gbox, const float* w, const float* box_w, float* dw,
                                    float* dbias, float* dbox_w, float* gx, int B, int C, int D, int H, int W, int stride,
                                    void* workspace, void* stream) {
  HP_FE_ARGS("hp_fe_entry_backward");
  HP_REQUIRE(x && ga && gbox && w && box_w && dw && dbox_w && workspace,
             "hp_fe_entry_backward: null pointer (only dbias and gx are optional)");
  const FeGeom q = fe_geom(B, D, H, W, stride);
  HP_REQUIRE((long)B * q.zsplit < (1l << 31) && (long)B * D < (1l << 31) && q.tiles_y < 65536 && q.tiles_x < 65536 && (H + 3) / 4 < 65536 &&
                 (W + 63) / 64 < 65536,
             "hp_fe_entry_backward: volume too large for the grid");
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)workspace;
  const int vec_in = (W % 4 == 0 && aligned(x, 16)) ? 1 : 0;
  {
    HP_PROF("fe_entry_wgrad", st);
    dim3 grid((unsigned)(B * q.zsplit), (unsigned)q.tiles_y, (unsigned)q.tiles_x);
#define HP_FE_WG(S, CG)                                                                                                          \
  hipLaunchKernelGGL((k_fe_entry_wgrad<S, CG>), grid, dim3(256), 0, st, x, ga, gbox, partial, C, D, H, W, q.Do, q.Ho, q.Wo, q.zsplit, \
                     q.zchunk, vec_in)
    // two channels per walk at most: 27 * (CG + 1) + CG running sums per thread next to the window
    if (stride == 1) {
      if (C == 1) HP_FE_WG(1, 1);
      else HP_FE_WG(1, 2);
    } else {
      if (C == 1) HP_FE_WG(2, 1);
      else HP_FE_WG(2, 2);
    }
#undef HP_FE_WG
    const int P = 28 * C + 27;
    hipLaunchKernelGGL(k_fe_entry_wreduce, dim3((unsigned)((P + 15) / 16)), dim3(256), 0, st, partial, q.nwg, C, dw, dbias, dbox_w);
    HP_CHECK_HIP(hipGetLastError());
  }
  if (gx) {
    HP_PROF("fe_entry_dgrad", st);
    dim3 grid((unsigned)(B * D), (unsigned)((H + 3) / 4), (unsigned)((W + 63) / 64));
    if (stride == 1)
      hipLaunchKernelGGL((k_fe_entry_dgrad<1>), grid, dim3(256), 0, st, ga, gbox, w, box_w, gx, C, D, H, W, q.Do, q.Ho, q.Wo);
    else
      hipLaunchKernelGGL((k_fe_entry_dgrad<2>), grid, dim3(256), 0, st, ga, gbox, w, box_w, gx, C, D, H, W, q.Do, q.Ho, q.Wo);
    HP_CHECK_HIP(hipGetLastError());
  }
  return HP_OK;
}

extern "C" int hp_bcast_add_forward(const float* t, const float* box, float* y, int B, int C, long V, void* stream) {
  HP_REQUIRE(t && box && y, "hp_bcast_add_forward: null pointer");
  HP_REQUIRE(B >= 1 && C >= 1 && V >= 1 && (long)B * C < 65536, "hp_bcast_add_forward: B, C, V must be positive and B * C below 65536");
  const long bx = (V + 1023) / 1024;
  HP_REQUIRE(bx < (1l << 31), "hp_bcast_add_forward: volume too large for the grid");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("bcast_add", st);
  const int vec = (V % 4 == 0 && aligned(t, 16) && aligned(box, 16) && aligned(y, 16)) ? 1 : 0;
  hipLaunchKernelGGL(k_bcast_add, dim3((unsigned)bx, (unsigned)(B * C)), dim3(256), 0, st, t, box, y, C, V, vec);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_channel_sum(const float* gy, float* gbox, int B, int C, long V, void* stream) {
  HP_REQUIRE(gy && gbox, "hp_channel_sum: null pointer");
  HP_REQUIRE(B >= 1 && C >= 1 && V >= 1 && B < 65536, "hp_channel_sum: B, C, V must be positive and B below 65536");
  const long bx = (V + 1023) / 1024;
  HP_REQUIRE(bx < (1l << 31), "hp_channel_sum: volume too large for the grid");
  hipStream_t st = (hipStream_t)stream;
  HP_PROF("channel_sum", st);
  const int vec = (V % 4 == 0 && aligned(gy, 16) && aligned(gbox, 16)) ? 1 : 0;
  hipLaunchKernelGGL(k_channel_sum, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, st, gy, gbox, C, V, vec);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
