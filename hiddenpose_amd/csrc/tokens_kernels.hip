// HP_BUILD: -ffp-contract=off
// Token assembly of the transformer heads' entry (hp_tokens_assemble_forward / _backward).  DESIGN 4.4.8.
//
//   forward    x[b, t, :] = (t < nl ? lead[t, :] : emb[b, t - nl, :]) (+ pos[t, :])
//   backward   dpos[t, :] = sum_b dx[b, t, :] (t < Ntok; 0 for Ntok <= t < pos_rows), dlead = its first nl rows,
//              demb[b, t - nl, :] = dx[b, t, :]
//
// Both are one pass over the token matrix and pure bandwidth: a work item is one float4 (dim % 4 == 0 and every base 16-byte
// aligned; the host picks the width, so the branch does not exist on the device) or one float, the grid is bounded and walks
// the items with a grid-stride loop, element indices are 64-bit.  The forward's item is one element of x; the backward's is
// one (t, column) of the table, whose thread walks the batch in ascending b: it reads every dx element once, copies it to
// demb and adds it to its running sum, so the sum's order is fixed, there is no atomic and two calls give the same bits.
// Plain vector stores, no LDS, no scratch.
#include "hp_internal.h"

namespace hp {

constexpr int TA_BT = 256;          // threads of a block
constexpr long TA_MAX_GRID = 2048;  // blocks: 256 CUs x 8; the grid-stride loop takes the rest

typedef float ta_f4v __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ T ta_zero();
template <>
__device__ __forceinline__ float ta_zero<float>() { return 0.f; }
template <>
__device__ __forceinline__ ta_f4v ta_zero<ta_f4v>() { return ta_f4v{0.f, 0.f, 0.f, 0.f}; }

// T = float: dimv = dim; T = ta_f4v: dimv = dim / 4.  ADD: pos is given.
template <typename T, bool ADD>
__global__ __launch_bounds__(TA_BT) void k_tokens_assemble_fwd(const T* __restrict__ lead, const T* __restrict__ emb,
                                                               const T* __restrict__ pos, T* __restrict__ x, long total, int nl,
                                                               long Ntok, int dimv) {
  const long per_b = Ntok * dimv, lead_items = (long)nl * dimv, emb_per_b = per_b - lead_items;
  const long step = (long)gridDim.x * TA_BT;
  for (long i = (long)blockIdx.x * TA_BT + threadIdx.x; i < total; i += step) {
    const long b = i / per_b, r = i - b * per_b;   // r = t * dimv + column: the offset into lead and pos as well
    T v = r < lead_items ? lead[r] : emb[b * emb_per_b + (r - lead_items)];
    if (ADD) v = v + pos[r];
    x[i] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(TA_BT) void k_tokens_assemble_bwd(const T* __restrict__ dx, T* __restrict__ dlead, T* __restrict__ dpos,
                                                               T* __restrict__ demb, int B, int nl, long Ntok, int dimv,
                                                               long items) {
  const long per_b = Ntok * dimv, lead_items = (long)nl * dimv, emb_per_b = per_b - lead_items;
  const long step = (long)gridDim.x * TA_BT;
  for (long r = (long)blockIdx.x * TA_BT + threadIdx.x; r < items; r += step) {
    if (r >= per_b) {   // table rows past the clip (items > per_b only with dpos)
      dpos[r] = ta_zero<T>();
      continue;
    }
    const bool patch = r >= lead_items;
    T acc = dx[r];
    if (patch && demb) demb[r - lead_items] = acc;
    for (int b = 1; b < B; ++b) {
      const T v = dx[(long)b * per_b + r];
      if (patch && demb) demb[(long)b * emb_per_b + (r - lead_items)] = v;
      acc = acc + v;
    }
    if (dpos) dpos[r] = acc;
    if (!patch && dlead) dlead[r] = acc;
  }
}

static inline bool ta_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline unsigned ta_grid(long items) {
  const long blocks = (items + TA_BT - 1) / TA_BT;
  return (unsigned)(blocks < TA_MAX_GRID ? blocks : TA_MAX_GRID);
}

}  // namespace hp

using namespace hp;

static int tokens_geometry(const char* who, int B, int nl, long Ntok, int dim) {
  HP_REQUIRE(B >= 1, "%s: B %d (must be >= 1)", who, B);
  HP_REQUIRE(dim >= 1, "%s: dim %d (must be >= 1)", who, dim);
  HP_REQUIRE(nl >= 0, "%s: nl %d (must be >= 0)", who, nl);
  HP_REQUIRE(Ntok > nl, "%s: Ntok %ld must exceed nl %d", who, Ntok, nl);
  HP_REQUIRE(Ntok <= 0x7fffffffffffffffl / dim / B, "%s: B %d x Ntok %ld x dim %d exceeds the index range", who, B, Ntok, dim);
  return HP_OK;
}

extern "C" int hp_tokens_assemble_forward(const float* lead, const float* emb, const float* pos, float* x, int B, int nl, long Ntok,
                                          int dim, long pos_rows, void* stream) {
  const char* who = "hp_tokens_assemble_forward";
  HP_REQUIRE(x != nullptr, "%s: null x", who);
  HP_REQUIRE(emb != nullptr, "%s: null emb", who);
  const int rc = tokens_geometry(who, B, nl, Ntok, dim);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(lead != nullptr || nl == 0, "%s: null lead with nl %d", who, nl);
  HP_REQUIRE(pos == nullptr || Ntok <= pos_rows, "%s: Ntok %ld exceeds pos_rows %ld", who, Ntok, pos_rows);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = dim % 4 == 0 && ta_al16(x) && ta_al16(emb) && ta_al16(lead) && ta_al16(pos);
  const int dimv = vec ? dim / 4 : dim;
  const long total = (long)B * Ntok * dimv;
  HP_PROF("tokens_assemble_fwd", st);
  const dim3 grid(ta_grid(total)), block(TA_BT);
  if (vec) {
    const ta_f4v *l4 = (const ta_f4v*)lead, *e4 = (const ta_f4v*)emb, *p4 = (const ta_f4v*)pos;
    if (pos) hipLaunchKernelGGL((k_tokens_assemble_fwd<ta_f4v, true>), grid, block, 0, st, l4, e4, p4, (ta_f4v*)x, total, nl, Ntok, dimv);
    else hipLaunchKernelGGL((k_tokens_assemble_fwd<ta_f4v, false>), grid, block, 0, st, l4, e4, p4, (ta_f4v*)x, total, nl, Ntok, dimv);
  } else {
    if (pos) hipLaunchKernelGGL((k_tokens_assemble_fwd<float, true>), grid, block, 0, st, lead, emb, pos, x, total, nl, Ntok, dimv);
    else hipLaunchKernelGGL((k_tokens_assemble_fwd<float, false>), grid, block, 0, st, lead, emb, pos, x, total, nl, Ntok, dimv);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_tokens_assemble_backward(const float* dx, float* dlead, float* dpos, float* demb, int B, int nl, long Ntok, int dim,
                                           long pos_rows, void* stream) {
  const char* who = "hp_tokens_assemble_backward";
  HP_REQUIRE(dx != nullptr, "%s: null dx", who);
  const int rc = tokens_geometry(who, B, nl, Ntok, dim);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(dpos == nullptr || Ntok <= pos_rows, "%s: Ntok %ld exceeds pos_rows %ld", who, Ntok, pos_rows);
  HP_REQUIRE(dpos == nullptr || pos_rows <= 0x7fffffffffffffffl / dim, "%s: pos_rows %ld x dim %d exceeds the index range", who,
             pos_rows, dim);
  if (!dlead && !dpos && !demb) return HP_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = dim % 4 == 0 && ta_al16(dx) && ta_al16(dlead) && ta_al16(dpos) && ta_al16(demb);
  const int dimv = vec ? dim / 4 : dim;
  // without demb and dpos only the lead rows have work; the table's rows past the clip exist only in dpos
  const long rows = dpos ? pos_rows : demb ? Ntok : (long)nl;
  if (rows == 0) return HP_OK;
  const long items = rows * dimv;
  HP_PROF("tokens_assemble_bwd", st);
  const dim3 grid(ta_grid(items)), block(TA_BT);
  if (vec)
    hipLaunchKernelGGL((k_tokens_assemble_bwd<ta_f4v>), grid, block, 0, st, (const ta_f4v*)dx, (ta_f4v*)dlead, (ta_f4v*)dpos,
                       (ta_f4v*)demb, B, nl, Ntok, dimv, items);
  else
    hipLaunchKernelGGL((k_tokens_assemble_bwd<float>), grid, block, 0, st, dx, dlead, dpos, demb, B, nl, Ntok, dimv, items);
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
