// The seeded dropout's mask generator, shared by dropout_kernels.hip and the activation backwards of
// sformer_backward.hip.  Philox4x32-10 over the flat row-major index space of a tensor: element e takes output word e & 3 of
// the block with counter (lo32(e >> 2), hi32(e >> 2), lo32(stream), hi32(stream)) and key (lo32(seed), hi32(seed)); it is
// kept iff word >= T, T = floor(p 2^32 + 0.5) in [0, 2^32].  A mask depends on (seed, stream, e, p) alone.
#pragma once
#include <cmath>

#include "hp_internal.h"

namespace hp {

struct DropoutParams {
  unsigned long long threshold;   // T
  float scale;                    // (float)(1 / (1 - p)), 0 for p = 1
  unsigned key0, key1, stream0, stream1;
};

// The argument checks every dropout entry shares (no device call behind them) and the host-side constants, in double.
inline int dropout_params(const char* who, long n, long first, double p, unsigned long long seed, unsigned long long stream,
                          DropoutParams* out) {
  HP_REQUIRE(n >= 0, "%s: n %ld < 0", who, n);
  HP_REQUIRE(first >= 0, "%s: first %ld < 0", who, first);
  HP_REQUIRE(p >= 0.0 && p <= 1.0, "%s: p %g outside [0, 1] (or not a number)", who, p);
  out->threshold = (unsigned long long)std::floor(p * 4294967296.0 + 0.5);
  out->scale = p >= 1.0 ? 0.f : (float)(1.0 / (1.0 - p));
  out->key0 = (unsigned)(seed & 0xffffffffull);
  out->key1 = (unsigned)(seed >> 32);
  out->stream0 = (unsigned)(stream & 0xffffffffull);
  out->stream1 = (unsigned)(stream >> 32);
  return HP_OK;
}

#ifdef __HIPCC__
// The four words of block `blk`.
__device__ __forceinline__ uint4 philox4x32_10(unsigned long long blk, const DropoutParams& d) {
  unsigned c0 = (unsigned)blk, c1 = (unsigned)(blk >> 32), c2 = d.stream0, c3 = d.stream1;
  unsigned k0 = d.key0, k1 = d.key1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}
__device__ __forceinline__ bool dropout_kept(unsigned word, const DropoutParams& d) { return (unsigned long long)word >= d.threshold; }
// kept ? v * scale : 0, the product rounded once
__device__ __forceinline__ float dropout_apply(float v, unsigned word, const DropoutParams& d) {
  return dropout_kept(word, d) ? __fmul_rn(v, d.scale) : 0.f;
}
// The word of one element (for paths that do not walk whole blocks).
__device__ __forceinline__ unsigned philox_word(long e, const DropoutParams& d) {
  const uint4 w = philox4x32_10((unsigned long long)e >> 2, d);
  const int l = (int)(e & 3);
  return l == 0 ? w.x : l == 1 ? w.y : l == 2 ? w.z : w.w;
}
#endif

}  // namespace hp
