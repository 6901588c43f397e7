// HP_BUILD: -ffp-contract=off
// Seeded dropout of the transformer heads' training paths (hp_dropout_forward, hp_dropout_mask).  DESIGN 4.4.7.
//
// The mask generator is hp_philox.h: one Philox4x32-10 block serves the four consecutive elements 4 blk .. 4 blk + 3 of the
// tensor's flat index space, so a thread owns whole blocks ("groups").  A call covers elements first .. first + n - 1 of the
// logical tensor; group gi of the call is block (first >> 2) + gi and starts (first & 3) elements before x[4 gi].  A group
// that lies wholly inside the call moves 16 bytes per array where that array's address allows it (the alignment is the same
// for every group of an array, so the branch is uniform) and four dwords where it does not; the at most two groups cut by
// the call's ends move their valid elements one by one.  Every element goes through the same __fmul_rn / __fadd_rn whichever
// width fetched it (contraction is off for the file as well).  64-bit element arithmetic, no LDS, no atomics, no scratch.
#include "hp_philox.h"

namespace hp {

constexpr int DR_BT = 256;                  // threads of a block
constexpr int DR_GPT = 4;                   // groups per thread
constexpr int DR_GPB = DR_BT * DR_GPT;      // groups per block (4096 elements)

typedef float dr_f4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 dr_ld4(const float* p, bool al) {
  if (al) {
    const dr_f4v t = *(const dr_f4v*)p;
    return make_float4(t.x, t.y, t.z, t.w);
  }
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void dr_st4(float* p, float4 v, bool al) {
  if (al) {
    const dr_f4v t = {v.x, v.y, v.z, v.w};
    *(dr_f4v*)p = t;
    return;
  }
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
// Is the address `lead` floats before p 16-byte aligned?  (The group grid of an array starts there.)
__device__ __forceinline__ bool dr_al16(const float* p, int lead) {
  return ((reinterpret_cast<uintptr_t>(p) - (uintptr_t)(4 * lead)) & 15u) == 0;
}

// Elements of group `i0 .. i0 + 3` that lie in [0, n), one by one.
__device__ __forceinline__ float4 dr_ld_part(const float* p, long i0, long n) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i0 >= 0 && i0 < n) v.x = p[i0];
  if (i0 + 1 >= 0 && i0 + 1 < n) v.y = p[i0 + 1];
  if (i0 + 2 >= 0 && i0 + 2 < n) v.z = p[i0 + 2];
  if (i0 + 3 >= 0 && i0 + 3 < n) v.w = p[i0 + 3];
  return v;
}
__device__ __forceinline__ void dr_st_part(float* p, long i0, long n, float4 v) {
  if (i0 >= 0 && i0 < n) p[i0] = v.x;
  if (i0 + 1 >= 0 && i0 + 1 < n) p[i0 + 1] = v.y;
  if (i0 + 2 >= 0 && i0 + 2 < n) p[i0 + 2] = v.z;
  if (i0 + 3 >= 0 && i0 + 3 < n) p[i0 + 3] = v.w;
}

// y may alias x or addend: a thread reads every element it owns before it writes one, and no two threads share an element.
template <bool ADD>
__global__ __launch_bounds__(DR_BT) void k_dropout_fwd(const float* x, const float* addend, float* y, long n, long first,
                                                       const DropoutParams d) {
  const int lead = (int)(first & 3);
  const long blk0 = first >> 2, ngroups = (lead + n + 3) >> 2;
  const bool ax = dr_al16(x, lead), ay = dr_al16(y, lead), aa = ADD && dr_al16(addend, lead);
  const long g0 = (long)blockIdx.x * DR_GPB + threadIdx.x;
  float4 X[DR_GPT], A[DR_GPT];
#pragma unroll
  for (int k = 0; k < DR_GPT; ++k) {
    const long gi = g0 + (long)k * DR_BT;
    if (gi < ngroups) {
      const long i0 = 4 * gi - lead;
      if (i0 >= 0 && i0 + 4 <= n) {
        X[k] = dr_ld4(x + i0, ax);
        if (ADD) A[k] = dr_ld4(addend + i0, aa);
      } else {
        X[k] = dr_ld_part(x, i0, n);
        if (ADD) A[k] = dr_ld_part(addend, i0, n);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DR_GPT; ++k) {
    const long gi = g0 + (long)k * DR_BT;
    if (gi < ngroups) {
      const long i0 = 4 * gi - lead;
      const uint4 w = philox4x32_10((unsigned long long)(blk0 + gi), d);
      float4 r = make_float4(dropout_apply(X[k].x, w.x, d), dropout_apply(X[k].y, w.y, d), dropout_apply(X[k].z, w.z, d),
                             dropout_apply(X[k].w, w.w, d));
      if (ADD) r = make_float4(__fadd_rn(r.x, A[k].x), __fadd_rn(r.y, A[k].y), __fadd_rn(r.z, A[k].z), __fadd_rn(r.w, A[k].w));
      if (i0 >= 0 && i0 + 4 <= n) dr_st4(y + i0, r, ay);
      else dr_st_part(y, i0, n, r);
    }
  }
}

__global__ __launch_bounds__(DR_BT) void k_dropout_mask(unsigned char* mask, long n, long first, const DropoutParams d) {
  const int lead = (int)(first & 3);
  const long blk0 = first >> 2, ngroups = (lead + n + 3) >> 2;
  const long gi = (long)blockIdx.x * DR_BT + threadIdx.x;
  if (gi >= ngroups) return;
  const long i0 = 4 * gi - lead;
  const uint4 w = philox4x32_10((unsigned long long)(blk0 + gi), d);
  if (i0 >= 0 && i0 < n) mask[i0] = dropout_kept(w.x, d) ? 1 : 0;
  if (i0 + 1 >= 0 && i0 + 1 < n) mask[i0 + 1] = dropout_kept(w.y, d) ? 1 : 0;
  if (i0 + 2 >= 0 && i0 + 2 < n) mask[i0 + 2] = dropout_kept(w.z, d) ? 1 : 0;
  if (i0 + 3 >= 0 && i0 + 3 < n) mask[i0 + 3] = dropout_kept(w.w, d) ? 1 : 0;
}

}  // namespace hp

using namespace hp;

extern "C" int hp_dropout_forward(const float* x, const float* addend, float* y, long n, long first, double p,
                                  unsigned long long seed, unsigned long long stream, void* stream_handle) {
  const char* who = "hp_dropout_forward";
  DropoutParams d;
  const int rc = dropout_params(who, n, first, p, seed, stream, &d);
  if (rc != HP_OK) return rc;
  if (n == 0) return HP_OK;
  HP_REQUIRE(x != nullptr, "%s: null x", who);
  HP_REQUIRE(y != nullptr, "%s: null y", who);
  const long nblocks = (((first & 3) + n + 3) / 4 + DR_GPB - 1) / DR_GPB;
  HP_REQUIRE(nblocks < 0x7fffffffl, "%s: n %ld exceeds one launch", who, n);
  hipStream_t st = (hipStream_t)stream_handle;
  HP_PROF("dropout_fwd", st);
  if (addend) hipLaunchKernelGGL(k_dropout_fwd<true>, dim3((unsigned)nblocks), dim3(DR_BT), 0, st, x, addend, y, n, first, d);
  else hipLaunchKernelGGL(k_dropout_fwd<false>, dim3((unsigned)nblocks), dim3(DR_BT), 0, st, x, addend, y, n, first, d);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_dropout_mask(unsigned char* mask, long n, long first, double p, unsigned long long seed,
                               unsigned long long stream, void* stream_handle) {
  const char* who = "hp_dropout_mask";
  DropoutParams d;
  const int rc = dropout_params(who, n, first, p, seed, stream, &d);
  if (rc != HP_OK) return rc;
  if (n == 0) return HP_OK;
  HP_REQUIRE(mask != nullptr, "%s: null mask", who);
  const long nblocks = (((first & 3) + n + 3) / 4 + DR_BT - 1) / DR_BT;
  HP_REQUIRE(nblocks < 0x7fffffffl, "%s: n %ld exceeds one launch", who, n);
  hipStream_t st = (hipStream_t)stream_handle;
  HP_PROF("dropout_mask", st);
  hipLaunchKernelGGL(k_dropout_mask, dim3((unsigned)nblocks), dim3(DR_BT), 0, st, mask, n, first, d);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
