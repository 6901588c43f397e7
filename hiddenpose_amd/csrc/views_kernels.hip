// HP_BUILD: -ffp-contract=off
// Three-view projections of a volume (utils/visualizer.py:33-57 volume_log, :155-185 threeviews_log).
//
// x: P contiguous fp32 planes (T, H, W).  One pass over x gives the three axis projections of every plane,
//   front (H, W) over t, top (T, W) over h, left (T, H) over w,
// as maxima of max(x, 0) (HP_VIEWS_MAX_CLAMPED) or as plain sums (HP_VIEWS_SUM), and the maximum of each finished view.
//
//   k_views_tile     one workgroup = one (16 frames, 16 rows, 64 columns) tile, 4 waves of 4 rows each, a lane per column.
//                    Every element is loaded once.  The tile's three partial projections go to slabs in the workspace:
//                    front[tc] (H, W) from registers, top[hc] (T, W) through LDS (the four waves' rows), left[wc] (T, H)
//                    from a butterfly across the wave's 64 columns.  A thread has the 16 loads of 4 frames in flight.
//   k_views_combine  a thread per pixel of a view adds / maximises its slabs in chunk order and writes the view; the
//                    workgroup's maximum goes to the workspace.
//   k_views_vmax     one workgroup per (plane, view) reduces those maxima.
// No atomics anywhere and a fixed order everywhere: two calls give equal bits in both modes.
//
// NaN follows NumPy (`v[v < 0] = 0; np.max`): a NaN is never below zero, stays, and wins every maximum.  In max mode
// values travel as the bit patterns of non-negative floats, where unsigned order is float order, with every NaN
// canonicalised to 0x7fc00000, which is above +inf.  -0.0 clamps to +0.0.
#include <cstdint>

#include "hp_internal.h"

namespace hp {

constexpr int VW_BT = 256;   // threads of every kernel here
constexpr int VW_TT = 16;    // frames of a tile
constexpr int VW_TH = 16;    // rows of a tile: 4 waves x 4 rows
constexpr int VW_TW = 64;    // columns of a tile: one per lane
constexpr int VW_ROWS = 4;   // rows per wave
constexpr int VW_TU = 4;     // frames in flight per thread (VW_TT is a multiple)
static_assert(VW_TU * VW_ROWS == 16 && VW_TT % VW_TU == 0, "wave_reduce_lines carries 16 lines");
constexpr int VW_PCHUNK = 32768;   // planes per launch (grid.y / grid.z)

template <int MODE>
struct ViewOp;
template <>
struct ViewOp<HP_VIEWS_MAX_CLAMPED> {
  static __device__ __forceinline__ float identity() { return 0.f; }
  static __device__ __forceinline__ float prep(float x) {
    const float c = x > 0.f ? x : 0.f;
    return x != x ? __uint_as_float(0x7fc00000u) : c;
  }
  static __device__ __forceinline__ float comb(float a, float b) {
    const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
    return __uint_as_float(ua > ub ? ua : ub);
  }
};
template <>
struct ViewOp<HP_VIEWS_SUM> {
  static __device__ __forceinline__ float identity() { return 0.f; }
  static __device__ __forceinline__ float prep(float x) { return x; }
  static __device__ __forceinline__ float comb(float a, float b) { return a + b; }
};

// NaN-propagating maximum of finished pixels (any sign): np.max.
__device__ __forceinline__ float vw_pmax(float a, float b) { return (a > b || a != a) ? a : b; }

struct ViewsGeom {
  int T, H, W;
  int nTc, nHc, nWc;      // tiles along t, h, w
  int nb;                 // combine workgroups per view: ceil(max pixels of a view / VW_BT)
  long V;                 // T * H * W
  long off_top, off_left, off_pmax, per_plane;   // float offsets inside a plane's workspace (front slabs at 0)
};

// The 16 reductions over the wave's 64 columns (VW_TU frames x VW_ROWS rows) in 17 cross-lane moves instead of 16 x 6: a
// butterfly that halves the number of lines a lane carries while the distance is 32, 16, 8, 4 (the lane keeps the lower
// half of its lines where the distance's bit of its index is clear, the upper half where it is set, and receives the
// partner's values of the same lines), then finishes the one line left over distances 2 and 1.  Line `held` of the caller
// ends up in every lane of its group of four.  The order of the additions is fixed by the lane index alone.
template <class Op>
__device__ __forceinline__ float wave_reduce_lines(float (&v)[16], int lane) {
#pragma unroll
  for (int n = 8, off = 32; n >= 1; n >>= 1, off >>= 1) {
    const bool upper = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const float keep = upper ? v[i + n] : v[i], send = upper ? v[i] : v[i + n];
      v[i] = Op::comb(keep, __shfl_xor(send, off, 64));
    }
  }
  float a = v[0];
  a = Op::comb(a, __shfl_xor(a, 2, 64));
  a = Op::comb(a, __shfl_xor(a, 1, 64));
  return a;
}

template <int MODE>
__global__ __launch_bounds__(VW_BT) void k_views_tile(const float* __restrict__ x, float* __restrict__ ws, const ViewsGeom g) {
  using Op = ViewOp<MODE>;
  __shared__ float s_top[VW_TT][VW_BT / 64][VW_TW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wc = blockIdx.x % g.nWc, hc = (blockIdx.x / g.nWc) % g.nHc, tc = blockIdx.x / (g.nWc * g.nHc);
  const long p = blockIdx.y;
  const float* __restrict__ xp = x + p * g.V;
  float* __restrict__ wp = ws + p * g.per_plane;
  const int w = wc * VW_TW + lane, h0 = hc * VW_TH + wave * VW_ROWS, t0 = tc * VW_TT;
  const int tn = min(VW_TT, g.T - t0);
  const bool wok = w < g.W;
  float accf[VW_ROWS];
#pragma unroll
  for (int r = 0; r < VW_ROWS; ++r) accf[r] = Op::identity();
  float* __restrict__ sl_left = wp + g.off_left + (long)wc * g.T * g.H;
  // lane -> which of the VW_TU * VW_ROWS line reductions it ends up holding (see wave_reduce_lines)
  const int held = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
  const int held_u = held / VW_ROWS, held_r = held % VW_ROWS;
  int rowoff[VW_ROWS];
  bool rok[VW_ROWS];
#pragma unroll
  for (int r = 0; r < VW_ROWS; ++r) {
    rowoff[r] = min(h0 + r, g.H - 1) * g.W + min(w, g.W - 1);
    rok[r] = wok && h0 + r < g.H;
  }
  for (int tt = 0; tt < tn; tt += VW_TU) {
    // Every load of VW_TU frames is issued before the first use.  The loads are unconditional, from addresses clamped into
    // the plane, and what lies outside the volume is replaced afterwards: a load under a condition would be waited for on
    // the spot, one at a time.
    float v[VW_TU * VW_ROWS];
#pragma unroll
    for (int u = 0; u < VW_TU; ++u) {
      const float* __restrict__ xt = xp + (long)min(t0 + tt + u, g.T - 1) * g.H * g.W;
#pragma unroll
      for (int r = 0; r < VW_ROWS; ++r) v[u * VW_ROWS + r] = xt[rowoff[r]];
    }
#pragma unroll
    for (int u = 0; u < VW_TU; ++u)
#pragma unroll
      for (int r = 0; r < VW_ROWS; ++r) {
        const float q = Op::prep(v[u * VW_ROWS + r]);
        v[u * VW_ROWS + r] = (rok[r] && tt + u < tn) ? q : Op::identity();
      }
#pragma unroll
    for (int u = 0; u < VW_TU; ++u) {
      float topacc = Op::identity();
#pragma unroll
      for (int r = 0; r < VW_ROWS; ++r) {
        accf[r] = Op::comb(accf[r], v[u * VW_ROWS + r]);
        topacc = Op::comb(topacc, v[u * VW_ROWS + r]);
      }
      if (tt + u < tn) s_top[tt + u][wave][lane] = topacc;
    }
    const float mine = wave_reduce_lines<Op>(v, lane);
    if ((lane & 3) == 0 && tt + held_u < tn && h0 + held_r < g.H) sl_left[(long)(t0 + tt + held_u) * g.H + h0 + held_r] = mine;
  }
  if (wok) {
    float* __restrict__ sl_front = wp + (long)tc * g.H * g.W;
#pragma unroll
    for (int r = 0; r < VW_ROWS; ++r)
      if (h0 + r < g.H) sl_front[(long)(h0 + r) * g.W + w] = accf[r];
  }
  __syncthreads();
  float* __restrict__ sl_top = wp + g.off_top + (long)hc * g.T * g.W;
  for (int i = threadIdx.x; i < tn * VW_TW; i += VW_BT) {
    const int tt = i >> 6, l = i & 63, col = wc * VW_TW + l;
    if (col >= g.W) continue;
    float a = s_top[tt][0][l];
#pragma unroll
    for (int k = 1; k < VW_BT / 64; ++k) a = Op::comb(a, s_top[tt][k][l]);
    sl_top[(long)(t0 + tt) * g.W + col] = a;
  }
}

template <int MODE>
__global__ __launch_bounds__(VW_BT) void k_views_combine(float* ws, float* __restrict__ front, float* __restrict__ top,
                                                         float* __restrict__ left, const ViewsGeom g) {
  using Op = ViewOp<MODE>;
  __shared__ float s[VW_BT];
  const int view = blockIdx.y;
  const long p = blockIdx.z;
  const long npix = view == 0 ? (long)g.H * g.W : view == 1 ? (long)g.T * g.W : (long)g.T * g.H;
  if ((long)blockIdx.x * VW_BT >= npix) return;     // uniform: this view has fewer workgroups than the largest one
  const int nchunk = view == 0 ? g.nTc : view == 1 ? g.nHc : g.nWc;
  const float* slab = ws + p * g.per_plane + (view == 0 ? 0 : view == 1 ? g.off_top : g.off_left);
  float* __restrict__ out = (view == 0 ? front : view == 1 ? top : left) + p * npix;
  const long pix = (long)blockIdx.x * VW_BT + threadIdx.x;
  float a = 0.f;
  if (pix < npix) {
    a = slab[pix];
    for (int c = 1; c < nchunk; ++c) a = Op::comb(a, slab[(long)c * npix + pix]);
    out[pix] = a;
  }
  s[threadIdx.x] = a;
  __syncthreads();
  if (pix >= npix) s[threadIdx.x] = s[0];           // a pixel of this workgroup stands in: thread 0 always holds one
  __syncthreads();
  for (int n = VW_BT / 2; n >= 1; n >>= 1) {
    if ((int)threadIdx.x < n) s[threadIdx.x] = vw_pmax(s[threadIdx.x], s[threadIdx.x + n]);
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[p * g.per_plane + g.off_pmax + (long)view * g.nb + blockIdx.x] = s[0];
}

__global__ __launch_bounds__(VW_BT) void k_views_vmax(const float* __restrict__ ws, float* __restrict__ vmax, const ViewsGeom g) {
  __shared__ float s[VW_BT];
  const int view = blockIdx.x;
  const long p = blockIdx.y;
  const long npix = view == 0 ? (long)g.H * g.W : view == 1 ? (long)g.T * g.W : (long)g.T * g.H;
  const int nb = (int)((npix + VW_BT - 1) / VW_BT);
  const float* __restrict__ pm = ws + p * g.per_plane + g.off_pmax + (long)view * g.nb;
  float a = pm[0];
  for (int i = threadIdx.x; i < nb; i += VW_BT) a = vw_pmax(a, pm[i]);
  s[threadIdx.x] = a;
  __syncthreads();
  for (int n = VW_BT / 2; n >= 1; n >>= 1) {
    if ((int)threadIdx.x < n) s[threadIdx.x] = vw_pmax(s[threadIdx.x], s[threadIdx.x + n]);
    __syncthreads();
  }
  if (threadIdx.x == 0) vmax[p * 3 + view] = s[0];
}

// out_front = front / vmax_front; out_top = rot90(top / vmax_top, 2); out_left = rot90(left / vmax_left, 3).
// A zero maximum gives a zero view; the division is IEEE (no fast-math in this file).
__global__ __launch_bounds__(VW_BT) void k_views_orient(const float* __restrict__ front, const float* __restrict__ top,
                                                        const float* __restrict__ left, const float* __restrict__ vmax,
                                                        float* __restrict__ out_front, float* __restrict__ out_top,
                                                        float* __restrict__ out_left, int T, int H, int W) {
  const int view = blockIdx.y;
  const long p = blockIdx.z;
  const long npix = view == 0 ? (long)H * W : view == 1 ? (long)T * W : (long)T * H;
  const long o = (long)blockIdx.x * VW_BT + threadIdx.x;
  if (o >= npix) return;
  const float m = vmax[p * 3 + view];
  float v;
  float* out;
  if (view == 0) {
    v = front[p * npix + o];
    out = out_front;
  } else if (view == 1) {          // out (T, W): out[i, j] = n[T-1-i, W-1-j], the flat index reversed
    v = top[p * npix + (npix - 1 - o)];
    out = out_top;
  } else {                         // out (H, T): out[i, j] = n[T-1-j, i] of n (T, H)
    const int i = (int)(o / T), j = (int)(o % T);
    v = left[p * npix + (long)(T - 1 - j) * H + i];
    out = out_left;
  }
  out[p * npix + o] = m == 0.f ? 0.f : v / m;
}

// ---------------------------------------------------------------- host side
static int views_check_shape(const char* who, int P, int T, int H, int W) {
  HP_REQUIRE(P >= 1 && T >= 1 && H >= 1 && W >= 1, "%s: P, T, H, W must be at least 1 (P %d, T %d, H %d, W %d)", who, P, T, H, W);
  HP_REQUIRE((long)T * H * W < 0x80000000l, "%s: a plane of %ld voxels reaches the 2^31 a plane is indexed with", who,
             (long)T * H * W);
  return HP_OK;
}

static ViewsGeom views_geom(int T, int H, int W) {
  ViewsGeom g;
  g.T = T;
  g.H = H;
  g.W = W;
  g.V = (long)T * H * W;
  g.nTc = (T + VW_TT - 1) / VW_TT;
  g.nHc = (H + VW_TH - 1) / VW_TH;
  g.nWc = (W + VW_TW - 1) / VW_TW;
  const long hw = (long)H * W, tw = (long)T * W, th = (long)T * H;
  const long mx = hw > tw ? (hw > th ? hw : th) : (tw > th ? tw : th);
  g.nb = (int)((mx + VW_BT - 1) / VW_BT);
  g.off_top = (long)g.nTc * hw;
  g.off_left = g.off_top + (long)g.nHc * tw;
  g.off_pmax = g.off_left + (long)g.nWc * th;
  g.per_plane = (g.off_pmax + 3l * g.nb + 3) & ~3l;
  return g;
}

}  // namespace hp

using namespace hp;

extern "C" size_t hp_volume_views_workspace_bytes(int P, int T, int H, int W, int mode) {
  if (P < 1 || T < 1 || H < 1 || W < 1 || (long)T * H * W >= 0x80000000l) return 0;
  if (mode != HP_VIEWS_MAX_CLAMPED && mode != HP_VIEWS_SUM) return 0;
  const ViewsGeom g = views_geom(T, H, W);
  size_t bytes;
  if (__builtin_mul_overflow((size_t)g.per_plane * sizeof(float), (size_t)P, &bytes)) return 0;
  return bytes;
}

extern "C" int hp_volume_views(const float* x, float* front, float* top, float* left, float* vmax, int P, int T, int H, int W,
                               int mode, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "hp_volume_views";
  HP_REQUIRE(x && front && top && left && vmax, "%s: null pointer", who);
  const int rc = views_check_shape(who, P, T, H, W);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(mode == HP_VIEWS_MAX_CLAMPED || mode == HP_VIEWS_SUM, "%s: mode %d is neither HP_VIEWS_MAX_CLAMPED nor HP_VIEWS_SUM",
             who, mode);
  const size_t need = hp_volume_views_workspace_bytes(P, T, H, W, mode);
  HP_REQUIRE(need != 0, "%s: P = %d planes of this size exceed the addressable workspace", who, P);
  HP_REQUIRE(workspace != nullptr, "%s: null workspace", who);
  if (workspace_bytes < need) {
    set_error("%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    return HP_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const ViewsGeom g = views_geom(T, H, W);
  const unsigned tiles = (unsigned)((long)g.nTc * g.nHc * g.nWc);
  for (int p0 = 0; p0 < P; p0 += VW_PCHUNK) {
    const unsigned np = (unsigned)(P - p0 < VW_PCHUNK ? P - p0 : VW_PCHUNK);
    const float* xc = x + (long)p0 * g.V;
    float* wsc = (float*)workspace + (long)p0 * g.per_plane;
    float* fc = front + (long)p0 * H * W;
    float* tc = top + (long)p0 * T * W;
    float* lc = left + (long)p0 * T * H;
    {
      HP_PROF("k_views_tile", st);
      if (mode == HP_VIEWS_SUM)
        hipLaunchKernelGGL(k_views_tile<HP_VIEWS_SUM>, dim3(tiles, np), dim3(VW_BT), 0, st, xc, wsc, g);
      else
        hipLaunchKernelGGL(k_views_tile<HP_VIEWS_MAX_CLAMPED>, dim3(tiles, np), dim3(VW_BT), 0, st, xc, wsc, g);
    }
    {
      HP_PROF("k_views_combine", st);
      if (mode == HP_VIEWS_SUM)
        hipLaunchKernelGGL(k_views_combine<HP_VIEWS_SUM>, dim3((unsigned)g.nb, 3, np), dim3(VW_BT), 0, st, wsc, fc, tc, lc, g);
      else
        hipLaunchKernelGGL(k_views_combine<HP_VIEWS_MAX_CLAMPED>, dim3((unsigned)g.nb, 3, np), dim3(VW_BT), 0, st, wsc, fc, tc, lc, g);
    }
    {
      HP_PROF("k_views_vmax", st);
      hipLaunchKernelGGL(k_views_vmax, dim3(3, np), dim3(VW_BT), 0, st, wsc, vmax + (long)p0 * 3, g);
    }
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_views_orient(const float* front, const float* top, const float* left, const float* vmax, float* out_front,
                               float* out_top, float* out_left, int P, int T, int H, int W, void* stream) {
  const char* who = "hp_views_orient";
  HP_REQUIRE(front && top && left && vmax && out_front && out_top && out_left, "%s: null pointer", who);
  const int rc = views_check_shape(who, P, T, H, W);
  if (rc != HP_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const ViewsGeom g = views_geom(T, H, W);
  for (int p0 = 0; p0 < P; p0 += VW_PCHUNK) {
    const unsigned np = (unsigned)(P - p0 < VW_PCHUNK ? P - p0 : VW_PCHUNK);
    const long hw = (long)p0 * H * W, tw = (long)p0 * T * W, th = (long)p0 * T * H;
    HP_PROF("k_views_orient", st);
    hipLaunchKernelGGL(k_views_orient, dim3((unsigned)g.nb, 3, np), dim3(VW_BT), 0, st, front + hw, top + tw, left + th,
                       vmax + (long)p0 * 3, out_front + hw, out_top + tw, out_left + th, T, H, W);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
