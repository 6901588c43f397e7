// Internal helpers shared by the translation units of libhiddenpose_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include "hp_host.h"

namespace hp {

#define HP_CHECK_HIP(expr)                                                              \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      ::hp::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return HP_ERR_HIP;                                                                \
    }                                                                                   \
  } while (0)

// Optional per-kernel timing with HIP events on the launch stream (hp_profile_* in the C ABI).
// Disabled by default: one relaxed atomic load per launch.
struct ProfScope {
  ProfScope(const char* name, hipStream_t st);
  ~ProfScope();
  int slot = -1;
  hipStream_t st = nullptr;
  hipEvent_t stop = nullptr;
};
#define HP_PROF(name, stream) ::hp::ProfScope _hp_prof_scope(name, stream)

// Exact-fp32 launches of sformer_backward.hip that the 16-bit attention backward (sformer_backward16.hip) reuses (dh 32 / 64).
constexpr int ATTN_JOINT_SPLITS = 32;    // key splits of the joint queries' forward partial records (32 queries x (dh + 2) floats each)
constexpr int ATTN_GROUPED_MAX_N = 64;   // tokens per group of the grouped attention backward
constexpr int ATTN_BWD_DQ_SPLITS = 32;   // key splits of the joint queries' dQ partials (32 queries x dh floats each)
void launch_attn_bwd_joint_keys(const float* ws_dk, const float* ws_dv, float* dK, float* dV, int BH, int Ntok, int dh, int nj, int frames,
                                hipStream_t st);
void launch_attn_bwd_dq_joint(const float* Q, const float* K0, const float* V, const float* dout, const float* lse, const float* delta,
                              float* part, float* dQ, int BH, int heads, int dh, int Ntok, int nj, hipStream_t st);
// Unmasked exact-fp32 launches (dh 16 / 24 / 32 / 64) that the masked attention entries (sformer_masked.hip) share with
// hp_sformer_attention(_lse) and hp_sformer_attention_backward(_grouped): the patch queries' forward (lse may be null) and dQ
// when they do not apply the mask, the joint queries' split merges, delta.
void launch_attention_patch(const float* Q, const float* K, const float* V, float* out, float* lse, int B, int heads, int dh, int Ntok,
                            int nj, int n, int frames, hipStream_t st);
void launch_attention_joint_merge(const float* part, float* out, float* lse, int BH, int heads, int dh, int Ntok, int nj, int nsplit,
                                  hipStream_t st);
void launch_attn_bwd_delta(const float* out, const float* dout, float* delta, int B, int heads, int dh, int Ntok, hipStream_t st);
void launch_attn_bwd_dq_patch(const float* Q, const float* K, const float* V, const float* dout, const float* lse, const float* delta,
                              float* dQ, int BH, int heads, int dh, int Ntok, int nj, int n, int frames, hipStream_t st);
void launch_attn_bwd_dq_joint_merge(const float* part, float* dQ, int BH, int Ntok, int dh, int nj, int nsplit, hipStream_t st);
// What the masked entries at a 16-bit precision (hp_sformer_attention*_masked_p) take from the other two files: the 16-bit patch
// queries' forward of sformer_kernels.hip (dh 32 / 64, HP_PRECISION_BF16 / _FP16; lse may be null) and the masked joint queries'
// dQ of sformer_masked.hip.  Their shared argument rule: only the joint / class queries apply the mask.
void launch_attention_patch16(const float* Q, const float* K, const float* V, float* out, float* lse, int B, int heads, int dh, int Ntok,
                              int nj, int n, int frames, int precision, hipStream_t st);
void launch_attn_bwd_dq_joint_masked(const float* Q, const float* K0, const float* V, const float* dout, const float* lse,
                                     const float* delta, float* part, float* dQ, int BH, int heads, int dh, int Ntok, int nj,
                                     const unsigned char* key_mask, hipStream_t st);
inline int attn_masked16_check(const char* who, int num_joints, int mask_patch_queries) {
  HP_REQUIRE(mask_patch_queries == 0 || mask_patch_queries == 1, "%s: mask_patch_queries must be 0 or 1", who);
  if (mask_patch_queries) {
    set_error("%s: mask_patch_queries 1 not built at a 16-bit precision (only the joint / class queries apply the mask there)", who);
    return HP_ERR_UNSUPPORTED;
  }
  if (num_joints == 0) {
    set_error("%s: num_joints 0 not built (with no joint / class key an all-masked group would have an empty key set)", who);
    return HP_ERR_UNSUPPORTED;
  }
  return HP_OK;
}

// ---- activation tensors stored as fp32 or bf16 (BASELINE configs[2]: bf16 with fp32 accumulators / statistics).  The
// element type of a tensor is a RUNTIME flag of the call (`half` != 0: bf16), so one kernel serves both layouts: the
// branch is uniform over the launch and the conversion is a shift (load) or one v_cvt_pk_bf16_f32 per pair (store).
#ifdef __HIPCC__
__device__ __forceinline__ float4 hp_ld4(const void* p, long i, int half) {  // elements i .. i+3 (i % 4 == 0)
  if (half) {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(p) + i);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
  return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i);
}
__device__ __forceinline__ float hp_ld1(const void* p, long i, int half) {
  if (half) return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(p)[i] << 16);
  return reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ unsigned short hp_f2bf(float v) {  // round to nearest even, NaN stays NaN
  typedef __attribute__((ext_vector_type(2))) float hp_f32x2;
  typedef __attribute__((ext_vector_type(2))) __bf16 hp_bf16x2;
  const hp_bf16x2 h = __builtin_convertvector((hp_f32x2){v, 0.f}, hp_bf16x2);
  return __builtin_bit_cast(unsigned int, h) & 0xffffu;
}
__device__ __forceinline__ void hp_st4(void* p, long i, float4 v, int half) {
  if (half) {
    typedef __attribute__((ext_vector_type(2))) float hp_f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 hp_bf16x2;
    const hp_bf16x2 lo = __builtin_convertvector((hp_f32x2){v.x, v.y}, hp_bf16x2);
    const hp_bf16x2 hi = __builtin_convertvector((hp_f32x2){v.z, v.w}, hp_bf16x2);
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p) + i) =
        make_uint2(__builtin_bit_cast(unsigned int, lo), __builtin_bit_cast(unsigned int, hi));
    return;
  }
  *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + i) = v;
}
// num_records of a raw buffer descriptor whose base lies `base_off` elements into a tensor of `total` elements of `esz`
// bytes: the tensor's TRUE remaining extent, so that an addressing slip reads zeros / drops the store instead of touching
// whatever is allocated next to the tensor (round 3's descriptors all said 2^31: the range check was the sign bit only).
// Capped at 2^31: offsets with bit 31 set stay out of range (the "force this lane out of range" idiom of the tile loads),
// and tensors whose remainder genuinely exceeds 2 GiB (layer 1 and the stem at the headline shape) keep that cap.
// A base below the tensor (negative base_off: tiles whose first taps reach outside the volume, masked per lane) only
// lengthens the extent; the low end is guarded by those masks, not by the descriptor.
__device__ __forceinline__ unsigned hp_extent(long total, long base_off, int esz) {
  const long bytes = (total - base_off) * esz;
  return bytes >= 0x80000000l ? 0x80000000u : bytes > 0 ? (unsigned)bytes : 0u;
}
__device__ __forceinline__ void hp_st1(void* p, long i, float v, int half) {
  if (half) reinterpret_cast<unsigned short*>(p)[i] = hp_f2bf(v);
  else reinterpret_cast<float*>(p)[i] = v;
}
#endif

}  // namespace hp
