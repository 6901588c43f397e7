// HP_BUILD: -ffp-contract=off
// The optimizer stage: torch's Adam (L2 weight decay) and SGD (momentum, dampening, Nesterov, weight decay) over a whole
// parameter group in ONE launch (hp_optim_adam_multi, hp_optim_sgd_multi).  DESIGN 4.6.
//
// A block owns one OPT_CHUNK-element chunk of one tensor.  The host compacts the caller's records (tensors with n == 0
// leave), appends the prefix of their chunk counts and sends both to the caller's workspace with one asynchronous copy from
// a pinned staging ring; the block finds its tensor by a binary search of the prefix.  Every element goes through the same
// explicit fmaf / __fmul_rn / __fdiv_rn / __fsqrt_rn sequence whichever access width fetched it (contraction is off for the
// file as well), so its result bits depend on its values alone: not on alignment, chunk position or the launch geometry.
// No atomics, no LDS, no scratch.
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "hp_internal.h"

namespace hp {

constexpr int OPT_BT = 256;               // threads of a block
constexpr int OPT_VPT = 4;                // 16-byte groups per thread and array
constexpr int OPT_CHUNK = OPT_BT * OPT_VPT * 4;   // 4096 elements of one tensor per block

typedef float opt_f4v __attribute__((ext_vector_type(4)));

// The record's pointers are device (global) memory; loaded from a table they would be generic and cost flat accesses.
#define HP_OPT_GLOBAL __attribute__((address_space(1)))
// Four consecutive elements.  `al`: the address is 16-byte aligned (uniform over the chunk: chunks start at multiples of 4096
// elements and the peeled head is the same in every chunk of a tensor).  NT: the non-temporal hint of DESIGN 4.3 for
// arrays that are touched once per step.
template <bool NT>
__device__ __forceinline__ float4 opt_ld4(const float* p, bool al) {
  if (al) {
    const HP_OPT_GLOBAL opt_f4v* q = (const HP_OPT_GLOBAL opt_f4v*)p;
    const opt_f4v t = NT ? __builtin_nontemporal_load(q) : *q;
    return make_float4(t.x, t.y, t.z, t.w);
  }
  const HP_OPT_GLOBAL float* q = (const HP_OPT_GLOBAL float*)p;
  if (NT) return make_float4(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2),
                             __builtin_nontemporal_load(q + 3));
  return make_float4(q[0], q[1], q[2], q[3]);
}
template <bool NT>
__device__ __forceinline__ void opt_st4(float* p, float4 v, bool al) {
  if (al) {
    const opt_f4v t = {v.x, v.y, v.z, v.w};
    HP_OPT_GLOBAL opt_f4v* q = (HP_OPT_GLOBAL opt_f4v*)p;
    if (NT) __builtin_nontemporal_store(t, q);
    else *q = t;
    return;
  }
  HP_OPT_GLOBAL float* q = (HP_OPT_GLOBAL float*)p;
  if (NT) {
    __builtin_nontemporal_store(v.x, q);
    __builtin_nontemporal_store(v.y, q + 1);
    __builtin_nontemporal_store(v.z, q + 2);
    __builtin_nontemporal_store(v.w, q + 3);
  } else {
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
  }
}
template <bool NT>
__device__ __forceinline__ float opt_ld1(const float* p) {
  const HP_OPT_GLOBAL float* q = (const HP_OPT_GLOBAL float*)p;
  return NT ? __builtin_nontemporal_load(q) : *q;
}
template <bool NT>
__device__ __forceinline__ void opt_st1(float* p, float v) {
  HP_OPT_GLOBAL float* q = (HP_OPT_GLOBAL float*)p;
  if (NT) __builtin_nontemporal_store(v, q);
  else *q = v;
}

__device__ __forceinline__ bool opt_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Largest i with prefix[i] <= b (prefix[0] = 0 <= b < prefix[cnt] = the grid).
__device__ __forceinline__ int opt_find(const int* __restrict__ prefix, int cnt, int b) {
  int lo = 0, hi = cnt;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Elements peeled off the front of every chunk: when all arrays of a tensor are misaligned by the SAME number of elements
// the interior behind 4 - a scalar elements is 16-byte aligned in each of them.  Otherwise nothing is peeled and each array
// moves 16 bytes at a time if its own address allows it, as four dwords if not.
__device__ __forceinline__ int opt_head(const float* a, const float* b, const float* c, const float* d) {
  const unsigned ma = (unsigned)(reinterpret_cast<uintptr_t>(a) >> 2) & 3u, mb = (unsigned)(reinterpret_cast<uintptr_t>(b) >> 2) & 3u,
                 mc = (unsigned)(reinterpret_cast<uintptr_t>(c) >> 2) & 3u, md = (unsigned)(reinterpret_cast<uintptr_t>(d) >> 2) & 3u;
  return (ma == mb && ma == mc && ma == md) ? (int)((4u - ma) & 3u) : 0;
}

struct AdamHyper {
  float beta2, om_beta1, om_beta2, eps, wd;   // om_*: 1 - beta, rounded from double
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamHyper h, float step, float isb2) {
  if (h.wd != 0.f) g = fmaf(h.wd, p, g);
  m = fmaf(__fsub_rn(g, m), h.om_beta1, m);
  v = fmaf(__fmul_rn(h.om_beta2, g), g, __fmul_rn(h.beta2, v));
  const float denom = fmaf(__fsqrt_rn(v), isb2, h.eps);
  p = fmaf(-step, __fdiv_rn(m, denom), p);
}

template <bool NT>
__global__ __launch_bounds__(OPT_BT) void k_optim_adam_multi(const hp_optim_adam_rec* __restrict__ tab, const int* __restrict__ prefix,
                                                              int cnt, const AdamHyper h) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ti = opt_find(prefix, cnt, b);
  const hp_optim_adam_rec r = tab[ti];
  const long off = (long)(b - prefix[ti]) * OPT_CHUNK;
  const int len = (int)(r.n - off < OPT_CHUNK ? r.n - off : OPT_CHUNK);
  float* p = r.p + off;
  const float* g = r.g + off;
  float* m = r.m + off;
  float* v = r.v + off;
  int head = opt_head(p, g, m, v);
  if (head > len) head = len;
  const int nvec = (len - head) >> 2;
  const bool ap = opt_al16(p + head), ag = opt_al16(g + head), am = opt_al16(m + head), av = opt_al16(v + head);
  float4 P[OPT_VPT], G[OPT_VPT], M[OPT_VPT], V[OPT_VPT];
#pragma unroll
  for (int k = 0; k < OPT_VPT; ++k) {
    const int j = tid + k * OPT_BT;
    if (j < nvec) {
      const int e = head + 4 * j;
      P[k] = opt_ld4<false>(p + e, ap);
      G[k] = opt_ld4<NT>(g + e, ag);
      M[k] = opt_ld4<NT>(m + e, am);
      V[k] = opt_ld4<NT>(v + e, av);
    }
  }
#pragma unroll
  for (int k = 0; k < OPT_VPT; ++k) {
    const int j = tid + k * OPT_BT;
    if (j < nvec) {
      const int e = head + 4 * j;
      adam_elem(P[k].x, G[k].x, M[k].x, V[k].x, h, r.lr_over_bc1, r.inv_sqrt_bc2);
      adam_elem(P[k].y, G[k].y, M[k].y, V[k].y, h, r.lr_over_bc1, r.inv_sqrt_bc2);
      adam_elem(P[k].z, G[k].z, M[k].z, V[k].z, h, r.lr_over_bc1, r.inv_sqrt_bc2);
      adam_elem(P[k].w, G[k].w, M[k].w, V[k].w, h, r.lr_over_bc1, r.inv_sqrt_bc2);
      opt_st4<false>(p + e, P[k], ap);
      opt_st4<NT>(m + e, M[k], am);
      opt_st4<NT>(v + e, V[k], av);
    }
  }
  // the peeled head (elements 0 .. head-1) and the tail behind the last whole group: at most 3 + 3 scalar elements
  const int ntail = len - head - 4 * nvec;
  if (tid < head + ntail) {
    const int e = tid < head ? tid : head + 4 * nvec + (tid - head);
    float pe = opt_ld1<false>(p + e), me = opt_ld1<NT>(m + e), ve = opt_ld1<NT>(v + e);
    adam_elem(pe, opt_ld1<NT>(g + e), me, ve, h, r.lr_over_bc1, r.inv_sqrt_bc2);
    opt_st1<false>(p + e, pe);
    opt_st1<NT>(m + e, me);
    opt_st1<NT>(v + e, ve);
  }
}

struct SgdHyper {
  float lr, mu, om_damp, wd;   // om_damp: 1 - dampening, rounded from double
  int nesterov;
};

// HAS_BUF: momentum != 0.  `first`: the tensor's first step (buf is written, not read).
template <bool HAS_BUF>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, const SgdHyper h, bool first) {
  if (h.wd != 0.f) g = fmaf(h.wd, p, g);
  if (HAS_BUF) {
    buf = first ? g : fmaf(h.mu, buf, __fmul_rn(h.om_damp, g));
    g = h.nesterov ? fmaf(h.mu, buf, g) : buf;
  }
  p = fmaf(-h.lr, g, p);
}

template <bool NT, bool HAS_BUF>
__global__ __launch_bounds__(OPT_BT) void k_optim_sgd_multi(const hp_optim_sgd_rec* __restrict__ tab, const int* __restrict__ prefix,
                                                             int cnt, const SgdHyper h) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ti = opt_find(prefix, cnt, b);
  const hp_optim_sgd_rec r = tab[ti];
  const long off = (long)(b - prefix[ti]) * OPT_CHUNK;
  const int len = (int)(r.n - off < OPT_CHUNK ? r.n - off : OPT_CHUNK);
  float* p = r.p + off;
  const float* g = r.g + off;
  float* bf = HAS_BUF ? r.buf + off : p;
  const bool first = r.first_step != 0, rd = HAS_BUF && !first;
  int head = opt_head(p, g, bf, bf);
  if (head > len) head = len;
  const int nvec = (len - head) >> 2;
  const bool ap = opt_al16(p + head), ag = opt_al16(g + head), ab = opt_al16(bf + head);
  float4 P[OPT_VPT], G[OPT_VPT], B[OPT_VPT];
#pragma unroll
  for (int k = 0; k < OPT_VPT; ++k) {
    const int j = tid + k * OPT_BT;
    B[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < nvec) {
      const int e = head + 4 * j;
      P[k] = opt_ld4<false>(p + e, ap);
      G[k] = opt_ld4<NT>(g + e, ag);
      if (rd) B[k] = opt_ld4<NT>(bf + e, ab);
    }
  }
#pragma unroll
  for (int k = 0; k < OPT_VPT; ++k) {
    const int j = tid + k * OPT_BT;
    if (j < nvec) {
      const int e = head + 4 * j;
      sgd_elem<HAS_BUF>(P[k].x, G[k].x, B[k].x, h, first);
      sgd_elem<HAS_BUF>(P[k].y, G[k].y, B[k].y, h, first);
      sgd_elem<HAS_BUF>(P[k].z, G[k].z, B[k].z, h, first);
      sgd_elem<HAS_BUF>(P[k].w, G[k].w, B[k].w, h, first);
      opt_st4<false>(p + e, P[k], ap);
      if (HAS_BUF) opt_st4<NT>(bf + e, B[k], ab);
    }
  }
  const int ntail = len - head - 4 * nvec;
  if (tid < head + ntail) {
    const int e = tid < head ? tid : head + 4 * nvec + (tid - head);
    float pe = opt_ld1<false>(p + e), be = rd ? opt_ld1<NT>(bf + e) : 0.f;
    sgd_elem<HAS_BUF>(pe, opt_ld1<NT>(g + e), be, h, first);
    opt_st1<false>(p + e, pe);
    if (HAS_BUF) opt_st1<NT>(bf + e, be);
  }
}

// ---- the pinned staging ring: OPT_RING slots per device, each guarded by an event recorded behind its copy, so the host
// waits only when it is OPT_RING optimizer calls ahead of the device.  Slots are allocated on first use and grow by doubling;
// a steady training loop allocates nothing.
constexpr int OPT_RING = 8;
struct OptSlot {
  void* host = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
};
struct OptRing {
  OptSlot slot[OPT_RING];
  int next = 0;
};
static std::mutex g_opt_mu;
static std::map<int, OptRing> g_opt_ring;

// A slot of at least `bytes`, free for the host to write (its previous copy has left it).  Called with g_opt_mu held.
static int opt_slot_acquire(size_t bytes, OptSlot** out) {
  int dev = 0;
  HP_CHECK_HIP(hipGetDevice(&dev));
  OptRing& ring = g_opt_ring[dev];
  OptSlot& s = ring.slot[ring.next];
  ring.next = (ring.next + 1) % OPT_RING;
  if (!s.ev) HP_CHECK_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  if (s.used) HP_CHECK_HIP(hipEventSynchronize(s.ev));
  if (s.cap < bytes) {
    size_t cap = s.cap ? s.cap : (size_t)64 << 10;
    while (cap < bytes) cap *= 2;
    if (s.host) HP_CHECK_HIP(hipHostFree(s.host));
    s.host = nullptr;
    s.cap = 0;
    HP_CHECK_HIP(hipHostMalloc(&s.host, cap, hipHostMallocPortable));
    s.cap = cap;
  }
  *out = &s;
  return HP_OK;
}

static size_t opt_align16(size_t v) { return (v + 15) & ~(size_t)15; }
static size_t opt_workspace_bytes(int count, size_t rec) {
  if (count < 0) return 0;
  return opt_align16((size_t)count * rec) + opt_align16(((size_t)count + 1) * sizeof(int));
}

static bool opt_nt() {   // A/B switch of the non-temporal hint (HP_OPTIM_NT=0: plain accesses); read at every call
  const char* e = std::getenv("HP_OPTIM_NT");
  return !(e && std::strcmp(e, "0") == 0);
}

// Compacts the records with n > 0 into a staging slot, appends the chunk prefix, sends both to `workspace` and returns the
// device addresses and the grid.  REC has a member `long n`.
template <class REC>
static int opt_upload(const REC* recs, int count, int live, void* workspace, hipStream_t st, const REC** d_tab, const int** d_prefix,
                      int* grid) {
  const size_t tab_bytes = opt_align16((size_t)live * sizeof(REC)), bytes = tab_bytes + ((size_t)live + 1) * sizeof(int);
  std::lock_guard<std::mutex> lk(g_opt_mu);
  OptSlot* s = nullptr;
  const int rc = opt_slot_acquire(bytes, &s);
  if (rc != HP_OK) return rc;
  REC* h_tab = (REC*)s->host;
  int* h_prefix = (int*)((char*)s->host + tab_bytes);
  int k = 0, chunks = 0;
  for (int i = 0; i < count; ++i) {
    if (recs[i].n == 0) continue;
    h_tab[k] = recs[i];
    h_prefix[k++] = chunks;
    chunks += (int)((recs[i].n + OPT_CHUNK - 1) / OPT_CHUNK);
  }
  h_prefix[k] = chunks;
  HP_CHECK_HIP(hipMemcpyAsync(workspace, s->host, bytes, hipMemcpyHostToDevice, st));
  HP_CHECK_HIP(hipEventRecord(s->ev, st));
  s->used = true;
  *d_tab = (const REC*)workspace;
  *d_prefix = (const int*)((const char*)workspace + tab_bytes);
  *grid = chunks;
  return HP_OK;
}

// The checks every record shares; `live` = records with n > 0.  The grid (one block per chunk) must fit an int.
#define HP_OPT_CHECK_COMMON(who)                                                                                          \
  HP_REQUIRE(count >= 0, "%s: count %d < 0", who, count);                                                                 \
  if (count == 0) return HP_OK;                                                                                           \
  HP_REQUIRE(recs != nullptr, "%s: null record table", who);                                                              \
  int live = 0;                                                                                                           \
  long chunks = 0;                                                                                                        \
  for (int i = 0; i < count; ++i) {                                                                                       \
    HP_REQUIRE(recs[i].n >= 0, "%s: record %d: n %ld < 0", who, i, recs[i].n);                                            \
    if (recs[i].n > 0) {                                                                                                  \
      ++live;                                                                                                             \
      chunks += (recs[i].n + OPT_CHUNK - 1) / OPT_CHUNK;                                                                  \
    }                                                                                                                     \
  }                                                                                                                       \
  HP_REQUIRE(chunks < 0x7fffffffl, "%s: %ld chunks of %d elements exceed one launch", who, chunks, OPT_CHUNK)

}  // namespace hp

using namespace hp;

extern "C" size_t hp_optim_adam_multi_workspace_bytes(int count) { return opt_workspace_bytes(count, sizeof(hp_optim_adam_rec)); }
extern "C" size_t hp_optim_sgd_multi_workspace_bytes(int count) { return opt_workspace_bytes(count, sizeof(hp_optim_sgd_rec)); }

extern "C" int hp_optim_adam_multi(const hp_optim_adam_rec* recs, int count, double beta1, double beta2, double eps,
                                   double weight_decay, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "hp_optim_adam_multi";
  HP_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, "%s: beta1 %g outside [0, 1)", who, beta1);
  HP_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, "%s: beta2 %g outside [0, 1)", who, beta2);
  HP_REQUIRE(eps >= 0.0, "%s: eps %g < 0", who, eps);
  HP_REQUIRE(weight_decay >= 0.0, "%s: weight_decay %g < 0", who, weight_decay);
  HP_OPT_CHECK_COMMON(who);
  for (int i = 0; i < count; ++i) {
    const hp_optim_adam_rec& r = recs[i];
    HP_REQUIRE(r.lr_over_bc1 >= 0.f, "%s: record %d: lr_over_bc1 %g: lr < 0 (or not a number)", who, i, (double)r.lr_over_bc1);
    HP_REQUIRE(r.inv_sqrt_bc2 > 0.f, "%s: record %d: inv_sqrt_bc2 %g must be positive", who, i, (double)r.inv_sqrt_bc2);
    HP_REQUIRE(r.n == 0 || (r.p && r.g && r.m && r.v), "%s: record %d: null pointer", who, i);
  }
  if (live == 0) return HP_OK;
  HP_REQUIRE(workspace != nullptr, "%s: null workspace", who);
  HP_REQUIRE(workspace_bytes >= hp_optim_adam_multi_workspace_bytes(count), "%s: workspace too small (%zu < %zu bytes)", who,
             workspace_bytes, hp_optim_adam_multi_workspace_bytes(count));
  hipStream_t st = (hipStream_t)stream;
  const hp_optim_adam_rec* d_tab = nullptr;
  const int* d_prefix = nullptr;
  int grid = 0;
  const int rc = opt_upload(recs, count, live, workspace, st, &d_tab, &d_prefix, &grid);
  if (rc != HP_OK) return rc;
  const AdamHyper h = {(float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)weight_decay};
  {
    HP_PROF("k_optim_adam_multi", st);
    if (opt_nt()) hipLaunchKernelGGL(k_optim_adam_multi<true>, dim3((unsigned)grid), dim3(OPT_BT), 0, st, d_tab, d_prefix, live, h);
    else hipLaunchKernelGGL(k_optim_adam_multi<false>, dim3((unsigned)grid), dim3(OPT_BT), 0, st, d_tab, d_prefix, live, h);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_optim_sgd_multi(const hp_optim_sgd_rec* recs, int count, double lr, double momentum, double dampening,
                                  double weight_decay, int nesterov, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "hp_optim_sgd_multi";
  HP_REQUIRE(lr >= 0.0, "%s: lr %g < 0", who, lr);
  HP_REQUIRE(momentum >= 0.0, "%s: momentum %g < 0", who, momentum);
  HP_REQUIRE(weight_decay >= 0.0, "%s: weight_decay %g < 0", who, weight_decay);
  HP_REQUIRE(nesterov == 0 || nesterov == 1, "%s: nesterov must be 0 or 1", who);
  HP_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "%s: nesterov needs momentum > 0 and dampening 0", who);
  HP_REQUIRE(dampening == dampening, "%s: dampening is not a number", who);
  HP_OPT_CHECK_COMMON(who);
  const bool has_buf = momentum != 0.0;
  for (int i = 0; i < count; ++i) {
    const hp_optim_sgd_rec& r = recs[i];
    HP_REQUIRE(r.n == 0 || (r.p && r.g && (r.buf || !has_buf)), "%s: record %d: null pointer", who, i);
  }
  if (live == 0) return HP_OK;
  HP_REQUIRE(workspace != nullptr, "%s: null workspace", who);
  HP_REQUIRE(workspace_bytes >= hp_optim_sgd_multi_workspace_bytes(count), "%s: workspace too small (%zu < %zu bytes)", who,
             workspace_bytes, hp_optim_sgd_multi_workspace_bytes(count));
  hipStream_t st = (hipStream_t)stream;
  const hp_optim_sgd_rec* d_tab = nullptr;
  const int* d_prefix = nullptr;
  int grid = 0;
  const int rc = opt_upload(recs, count, live, workspace, st, &d_tab, &d_prefix, &grid);
  if (rc != HP_OK) return rc;
  const SgdHyper h = {(float)lr, (float)momentum, (float)(1.0 - dampening), (float)weight_decay, nesterov};
  {
    HP_PROF("k_optim_sgd_multi", st);
    const bool nt = opt_nt();
#define HP_SGD_LAUNCH(NT, HB) hipLaunchKernelGGL((k_optim_sgd_multi<NT, HB>), dim3((unsigned)grid), dim3(OPT_BT), 0, st, d_tab, d_prefix, live, h)
    if (nt && has_buf) HP_SGD_LAUNCH(true, true);
    else if (nt) HP_SGD_LAUNCH(true, false);
    else if (has_buf) HP_SGD_LAUNCH(false, true);
    else HP_SGD_LAUNCH(false, false);
#undef HP_SGD_LAUNCH
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
