// HP_BUILD: -ffp-contract=off
// Losses of the transformer heads: the Gaussian heat-map MSE that TokenPose-L trains on (utils/criterion.py:166-270,
// JointsMSELoss / JointTarget) and the label-smoothed KL loss of the 1-D coordinate classifiers ("SimDR", :10-63,
// NMTNORMCritierion), forward and backward.
//
// Heat-map: one workgroup walks whole (b, j) maps.  A map of at least 1024 elements has the workgroup to itself; smaller maps
// are grouped 4 or 16 to a workgroup and each wave walks whole maps, so a workgroup keeps a few waves busy.  The Gaussian is
// separable: ex[W] and ey[H] are built once per map in LDS (W + H expf instead of W * H) and a target value is one product.
// The target map is never stored: the backward builds the two tables again.  An element's result bits depend on its values
// alone (the same expression whichever access width fetched it; contraction is off for the file), and the element -> thread
// assignment does not depend on any pointer's alignment, so the loss bits do not either.
// SimDR: one wave per (row, axis).  Rows of at most 512 bins live in registers; longer rows take one online max + sum pass.
// Both losses are summed without atomics: per-map / per-row partials in double go to the caller's workspace and a one-block
// kernel adds them in a fixed order, so the loss is bit-reproducible.
#include <cmath>

#include "hp_internal.h"

namespace hp {

constexpr int HL_BT = 256;            // threads of a workgroup
constexpr int HL_GMAX = 16;           // maps of one workgroup at most
constexpr int HL_TAB_MAX = 15360;     // floats of Gaussian tables in a workgroup's LDS (60 KB)
constexpr int HL_LDS_HEAD = 224;      // bytes in front of the tables: 4 doubles, 16 flags, 16 (mu_x, mu_y)
constexpr int SD_REG = 8;             // SimDR: row elements a lane keeps in registers (64 * 8 = 512 bins)

typedef float hl_f4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool hl_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
__device__ __forceinline__ float4 hl_ld4(const float* p, bool al) {
  if (al) {
    const hl_f4v t = *reinterpret_cast<const hl_f4v*>(p);
    return make_float4(t.x, t.y, t.z, t.w);
  }
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void hl_st4(float* p, float4 v, bool al) {
  if (al) {
    const hl_f4v t = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<hl_f4v*>(p) = t;
    return;
  }
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
__device__ __forceinline__ double hl_wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float hl_wsumf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float hl_wmaxf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// adjust_target_weight (utils/criterion.py:227-239): int() truncates toward zero, the arithmetic is float32.
__device__ __forceinline__ bool hl_in_range(float mx, float my, float t, int H, int W) {
  const double ulx = truncf(mx - t), uly = truncf(my - t);
  const double brx = truncf(mx + t + 1.0f), bry = truncf(my + t + 1.0f);
  return !(ulx >= (double)W || uly >= (double)H || brx < 0.0 || bry < 0.0);
}

enum { HEAT_RENDER = 0, HEAT_FWD = 1, HEAT_BWD = 2 };

// One element: g the target value, p the prediction.  RENDER stores g; BWD stores ((p - g) w^2 / N) gloss, the multiplication
// by gloss last (so a scaled loss scales the gradient by exactly one more rounding); FWD adds (w (p - g))^2 in double.
template <int MODE>
__device__ __forceinline__ float heat_elem(float p, float g, float w, float invN, float gl, double& acc) {
  if (MODE == HEAT_RENDER) return g;
  if (MODE == HEAT_FWD) {
    const double d = (double)(w * (p - g));
    acc += d * d;
    return 0.f;
  }
  return (((p - g) * (w * w)) * invN) * gl;
}

template <int MODE>
__global__ __launch_bounds__(HL_BT) void k_heat(const float* __restrict__ pred, const float* __restrict__ joints,
                                                const float* __restrict__ vis, const float* __restrict__ flags_in,
                                                const float* __restrict__ gloss, float* __restrict__ out,
                                                float* __restrict__ flags_out, double* __restrict__ partial, int R, int H, int W,
                                                int G, int team, float tmp, float two_s2, float invN, int use_tw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hl_smem[];
  double* red = reinterpret_cast<double*>(hl_smem);
  float* fl = reinterpret_cast<float*>(hl_smem + 32);
  float* mu = fl + HL_GMAX;
  float* tab = mu + 2 * HL_GMAX;
  const int tid = threadIdx.x, WH = W + H, HW = H * W;
  const long r0 = (long)blockIdx.x * G;

  if (tid < G && r0 + tid < R) {
    const long r = r0 + tid;
    const float mx = joints[2 * r], my = joints[2 * r + 1];
    float f;
    if (MODE == HEAT_BWD) {
      f = flags_in[r];
    } else {
      f = hl_in_range(mx, my, tmp, H, W) ? (MODE == HEAT_RENDER && vis ? vis[r] : 1.0f) : 0.0f;
      flags_out[r] = f;
    }
    fl[tid] = f;
    mu[2 * tid] = mx;
    mu[2 * tid + 1] = my;
  }
  __syncthreads();
  for (int i = tid; i < G * WH; i += HL_BT) {
    const int g = i / WH, k = i - g * WH;
    if (r0 + g < R) {
      const float d = k < W ? (float)k - mu[2 * g] : (float)(k - W) - mu[2 * g + 1];
      tab[i] = expf(-(d * d) / two_s2);
    }
  }
  __syncthreads();

  const int nteams = HL_BT / team, tm = tid / team, tl = tid - tm * team;
  const float gl = MODE == HEAT_BWD ? gloss[0] : 1.0f;
  for (int g = tm; g < G; g += nteams) {     // team == HL_BT only with G == 1: the barrier below is reached by every thread
    const long r = r0 + g;
    if (r >= R) break;
    const float f = fl[g];
    const bool draw = MODE == HEAT_RENDER ? f > 0.5f : f != 0.0f;
    const float w = (MODE == HEAT_RENDER || !use_tw) ? 1.0f : f;
    const float* ex = tab + g * WH;
    const float* ey = ex + W;
    const float* p = MODE == HEAT_RENDER ? nullptr : pred + r * HW;
    float* o = MODE == HEAT_FWD ? nullptr : out + r * HW;
    const bool ap = MODE != HEAT_RENDER && hl_al16(p), ao = MODE != HEAT_FWD && hl_al16(o);
    const int nvec = HW >> 2;
    double acc = 0.0;
    for (int v = tl; v < nvec; v += team) {
      const int e = 4 * v;
      int y = e / W, x = e - y * W;
      const float4 P = MODE == HEAT_RENDER ? make_float4(0.f, 0.f, 0.f, 0.f) : hl_ld4(p + e, ap);
      const float pin[4] = {P.x, P.y, P.z, P.w};
      float res[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gv = draw ? ex[x] * ey[y] : 0.0f;
        res[j] = heat_elem<MODE>(pin[j], gv, w, invN, gl, acc);
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
      if (MODE != HEAT_FWD) hl_st4(o + e, make_float4(res[0], res[1], res[2], res[3]), ao);
    }
    const int e = 4 * nvec + tl;     // the last HW % 4 elements
    if (tl < HW - 4 * nvec) {
      const int y = e / W, x = e - y * W;
      const float gv = draw ? ex[x] * ey[y] : 0.0f;
      const float res = heat_elem<MODE>(MODE == HEAT_RENDER ? 0.f : p[e], gv, w, invN, gl, acc);
      if (MODE != HEAT_FWD) o[e] = res;
    }
    if (MODE == HEAT_FWD) {
      acc = hl_wsum(acc);
      if (team == 64) {
        if (tl == 0) partial[r] = acc;
      } else {
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) partial[r] = ((red[0] + red[1]) + red[2]) + red[3];
      }
    }
  }
}

// loss = scale * sum of `count` partials, added in a fixed order in double.
__global__ __launch_bounds__(HL_BT) void k_sum_partials(const double* __restrict__ part, long count, double scale,
                                                        float* __restrict__ loss) {
  __shared__ double sh[HL_BT];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (long i = tid; i < count; i += HL_BT) a += part[i];
  sh[tid] = a;
  __syncthreads();
  for (int s = HL_BT / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(sh[0] * scale);
}

// ---------------------------------------------------------------- SimDR
struct SimdrAxis {
  const float* x;
  float* dx;
  long stride;      // elements between rows
  int n;            // bins
  float u_f, conf_f, t_out_f, inv_jbn;   // backward: ls / (n - 1), 1 - ls, sum of t when no bin holds the confidence, 1 / (J B n)
  double u, conf, ent_in, ent_out;       // forward: the same in double and sum t log t with / without the confidence bin
};
struct SimdrArgs {
  SimdrAxis ax[3];
};

__device__ __forceinline__ SimdrAxis sd_axis(const SimdrArgs& a, int i) { return i == 0 ? a.ax[0] : i == 1 ? a.ax[1] : a.ax[2]; }
// .long() of the target: truncation toward zero.  Anything that cannot be a bin (|t| >= 2^30, NaN) is -1: no bin matches.
__device__ __forceinline__ int sd_label(float t) { return fabsf(t) < 1073741824.0f ? (int)t : -1; }

__global__ __launch_bounds__(HL_BT) void k_simdr_fwd(const SimdrArgs args, const float* __restrict__ target,
                                                     const float* __restrict__ weight, int R, float* __restrict__ stat,
                                                     double* __restrict__ partial) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (HL_BT / 64) + (threadIdx.x >> 6)));
  const int lane = threadIdx.x & 63;
  if (wv >= R * 3) return;
  const int r = wv / 3, a = wv - 3 * r;
  const SimdrAxis A = sd_axis(args, a);
  const int n = A.n;
  const float* x = A.x + (long)r * A.stride;
  const int label = sd_label(target[3 * (long)r + a]);
  const bool in = label >= 0 && label < n;
  float M, sum, xl = 0.f;
  double sx = 0.0;
  if (n <= 64 * SD_REG) {
    float v[SD_REG];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < SD_REG; ++i) {
      const int k = lane + 64 * i;
      v[i] = k < n ? x[k] : -INFINITY;
      m = fmaxf(m, v[i]);
    }
    M = hl_wmaxf(m);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SD_REG; ++i) {
      const int k = lane + 64 * i;
      if (k < n) {
        s += expf(v[i] - M);
        sx += (double)v[i];
        if (k == label) xl = v[i];
      }
    }
    sum = hl_wsumf(s);
  } else {
    float m = -INFINITY, s = 0.f;
    for (int k = lane; k < n; k += 64) {     // n > 512: every lane has elements
      const float xv = x[k];
      if (xv > m) {
        s = s * expf(m - xv) + 1.0f;
        m = xv;
      } else {
        s += expf(xv - m);
      }
      sx += (double)xv;
      if (k == label) xl = xv;
    }
    M = hl_wmaxf(m);
    sum = hl_wsumf(s * expf(m - M));
  }
  sx = hl_wsum(sx);
  xl = hl_wsumf(xl);          // one lane holds it, the others add zeros
  if (lane == 0) {
    const float logsum = logf(sum);     // s_k = (x_k - M) - logsum
    const double s_all = sx - (double)n * (double)M - (double)n * (double)logsum;
    const double s_lab = ((double)xl - (double)M) - (double)logsum;
    const double dot = in ? A.u * (s_all - s_lab) + A.conf * s_lab : A.u * s_all;
    const double row = ((in ? A.ent_in : A.ent_out) - dot) / (double)n;
    partial[wv] = (weight ? (double)weight[r] : 1.0) * row;
    stat[2 * (long)wv] = M;
    stat[2 * (long)wv + 1] = logsum;
  }
}

__global__ __launch_bounds__(HL_BT) void k_simdr_bwd(const SimdrArgs args, const float* __restrict__ target,
                                                     const float* __restrict__ weight, const float* __restrict__ stat,
                                                     const float* __restrict__ gloss, int R) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (HL_BT / 64) + (threadIdx.x >> 6)));
  const int lane = threadIdx.x & 63;
  if (wv >= R * 3) return;
  const int r = wv / 3, a = wv - 3 * r;
  const SimdrAxis A = sd_axis(args, a);
  const int n = A.n;
  const float* x = A.x + (long)r * A.stride;
  float* dx = A.dx + (long)r * A.stride;
  const int label = sd_label(target[3 * (long)r + a]);
  const bool in = label >= 0 && label < n;
  const float M = stat[2 * (long)wv], logsum = stat[2 * (long)wv + 1];
  const float c = (weight ? weight[r] : 1.0f) * A.inv_jbn, gl = gloss[0];
  const float T = in ? 1.0f : A.t_out_f;
  for (int k = lane; k < n; k += 64) {
    const float p = expf((x[k] - M) - logsum);
    const float t = k == label ? A.conf_f : A.u_f;
    dx[k] = ((p * T - t) * c) * gl;
  }
}

// ---------------------------------------------------------------- host side
static size_t hl_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The checks every heat-map entry shares.  Maps are indexed with 32 bits inside a map and 64 bits across maps.
static int heat_check(const char* who, long R, int H, int W, double sigma) {
  HP_REQUIRE(R >= 1 && H >= 1 && W >= 1, "%s: B, J, H, W must be at least 1 (maps %ld, H %d, W %d)", who, R, H, W);
  HP_REQUIRE(std::isfinite(sigma) && sigma > 0.0, "%s: sigma %g must be positive and finite", who, sigma);
  HP_REQUIRE(R <= 0x7fffffffl, "%s: %ld maps exceed the 2^31 - 1 a launch indexes", who, R);
  HP_REQUIRE((long)H * W <= 0x7fffffffl - 8, "%s: H * W = %ld exceeds the 32-bit index of a map", who, (long)H * W);
  if ((long)H + W > HL_TAB_MAX) {
    set_error("%s: H + W = %ld not built (the Gaussian tables of a map take H + W <= %d floats of LDS)", who, (long)H + W, HL_TAB_MAX);
    return HP_ERR_UNSUPPORTED;
  }
  return HP_OK;
}

struct HeatLaunch {
  int G, team, grid;
  size_t lds;
};
static HeatLaunch heat_launch(long R, int H, int W) {
  const long HW = (long)H * W;
  HeatLaunch l;
  l.G = HW >= 1024 ? 1 : HW >= 256 ? 4 : HL_GMAX;
  if (l.G == HL_GMAX && (long)l.G * (H + W) > HL_TAB_MAX) l.G = 4;     // long thin maps
  l.team = l.G == 1 ? HL_BT : 64;
  l.grid = (int)((R + l.G - 1) / l.G);
  l.lds = HL_LDS_HEAD + (size_t)l.G * (H + W) * sizeof(float);
  return l;
}

template <int MODE>
static void heat_run(const float* pred, const float* joints, const float* vis, const float* flags_in, const float* gloss, float* out,
                     float* flags_out, double* partial, long R, int H, int W, double sigma, double tmp, int use_tw, hipStream_t st) {
  const HeatLaunch l = heat_launch(R, H, W);
  const float invN = (float)(1.0 / ((double)R * H * W));
  hipLaunchKernelGGL(k_heat<MODE>, dim3((unsigned)l.grid), dim3(HL_BT), l.lds, st, pred, joints, vis, flags_in, gloss, out, flags_out,
                     partial, (int)R, H, W, l.G, l.team, (float)tmp, (float)(2.0 * sigma * sigma), invN, use_tw);
}

static int simdr_check(const char* who, const void* px, int nx, long sx, const void* py, int ny, long sy, const void* pz, int nz, long sz,
                       const void* target, int B, int J, double ls) {
  HP_REQUIRE(px && py && pz && target, "%s: null pointer", who);
  HP_REQUIRE(B >= 1 && J >= 1, "%s: B, J must be at least 1 (B %d, J %d)", who, B, J);
  HP_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every axis needs at least 2 bins (%d, %d, %d)", who, nx, ny, nz);
  HP_REQUIRE(sx >= nx && sy >= ny && sz >= nz, "%s: a row stride is shorter than its row (%ld, %ld, %ld)", who, sx, sy, sz);
  HP_REQUIRE(std::isfinite(ls) && ls >= 0.0 && ls < 1.0, "%s: label_smoothing %g outside [0, 1)", who, ls);
  HP_REQUIRE((long)B * J <= 0x7fffffffl / 3, "%s: B * J = %ld rows exceed the (2^31 - 1) / 3 a launch indexes", who, (long)B * J);
  return HP_OK;
}

static double xlogx(double v) { return v > 0.0 ? v * std::log(v) : 0.0; }
static SimdrAxis simdr_axis(const float* x, float* dx, int n, long stride, double ls, long R) {
  SimdrAxis a;
  a.x = x;
  a.dx = dx;
  a.stride = stride;
  a.n = n;
  a.u = ls / (double)(n - 1);
  a.conf = 1.0 - ls;
  a.ent_in = (double)(n - 1) * xlogx(a.u) + xlogx(a.conf);
  a.ent_out = (double)n * xlogx(a.u);
  a.u_f = (float)a.u;
  a.conf_f = (float)a.conf;
  a.t_out_f = (float)((double)n * a.u);
  a.inv_jbn = (float)(1.0 / ((double)R * n));
  return a;
}

}  // namespace hp

using namespace hp;

extern "C" int hp_joint_heatmaps(const float* joints, const float* vis, int R, int H, int W, double sigma, double tmp_size,
                                 float* target, float* flags, void* stream) {
  const char* who = "hp_joint_heatmaps";
  HP_REQUIRE(joints && target && flags, "%s: null pointer", who);
  const int rc = heat_check(who, R, H, W, sigma);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(std::isfinite(tmp_size) && tmp_size >= 0.0, "%s: tmp_size %g must be finite and not negative", who, tmp_size);
  hipStream_t st = (hipStream_t)stream;
  {
    HP_PROF("k_heat_render", st);
    heat_run<HEAT_RENDER>(nullptr, joints, vis, nullptr, nullptr, target, flags, nullptr, R, H, W, sigma, tmp_size, 0, st);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" size_t hp_joints_mse_workspace_bytes(int B, int J) {
  if (B < 1 || J < 1) return 0;
  return hl_align16((size_t)B * (size_t)J * sizeof(double));
}

extern "C" int hp_joints_mse_forward(const float* pred, const float* joints, int B, int J, int H, int W, double sigma,
                                     int use_target_weight, float* flags, float* loss, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  const char* who = "hp_joints_mse_forward";
  HP_REQUIRE(pred && joints && flags && loss, "%s: null pointer", who);
  HP_REQUIRE(B >= 1 && J >= 1, "%s: B, J, H, W must be at least 1 (B %d, J %d)", who, B, J);
  const long R = (long)B * J;
  const int rc = heat_check(who, R, H, W, sigma);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(use_target_weight == 0 || use_target_weight == 1, "%s: use_target_weight must be 0 or 1", who);
  HP_REQUIRE(workspace != nullptr, "%s: null workspace", who);
  HP_REQUIRE(workspace_bytes >= hp_joints_mse_workspace_bytes(B, J), "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes,
             hp_joints_mse_workspace_bytes(B, J));
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  {
    HP_PROF("k_heat_mse_fwd", st);
    heat_run<HEAT_FWD>(pred, joints, nullptr, nullptr, nullptr, nullptr, flags, partial, R, H, W, sigma, sigma, use_target_weight, st);
  }
  {
    HP_PROF("k_sum_partials", st);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(HL_BT), 0, st, partial, R, 0.5 / ((double)R * H * W), loss);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_joints_mse_backward(const float* pred, const float* joints, const float* flags, const float* gloss, int B, int J,
                                      int H, int W, double sigma, int use_target_weight, float* dpred, void* stream) {
  const char* who = "hp_joints_mse_backward";
  HP_REQUIRE(pred && joints && flags && gloss && dpred, "%s: null pointer", who);
  HP_REQUIRE(B >= 1 && J >= 1, "%s: B, J, H, W must be at least 1 (B %d, J %d)", who, B, J);
  const long R = (long)B * J;
  const int rc = heat_check(who, R, H, W, sigma);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(use_target_weight == 0 || use_target_weight == 1, "%s: use_target_weight must be 0 or 1", who);
  hipStream_t st = (hipStream_t)stream;
  {
    HP_PROF("k_heat_mse_bwd", st);
    heat_run<HEAT_BWD>(pred, joints, nullptr, flags, gloss, dpred, nullptr, nullptr, R, H, W, sigma, sigma, use_target_weight, st);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" size_t hp_simdr_loss_workspace_bytes(int B, int J) {
  if (B < 1 || J < 1) return 0;
  return hl_align16((size_t)B * (size_t)J * 3 * sizeof(double));
}

extern "C" int hp_simdr_loss_forward(const float* pred_x, int nx, long stride_x, const float* pred_y, int ny, long stride_y,
                                     const float* pred_z, int nz, long stride_z, const float* target, const float* weight, int B, int J,
                                     double label_smoothing, float* stat, float* loss, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  const char* who = "hp_simdr_loss_forward";
  const int rc = simdr_check(who, pred_x, nx, stride_x, pred_y, ny, stride_y, pred_z, nz, stride_z, target, B, J, label_smoothing);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(stat && loss, "%s: null pointer", who);
  HP_REQUIRE(workspace != nullptr, "%s: null workspace", who);
  HP_REQUIRE(workspace_bytes >= hp_simdr_loss_workspace_bytes(B, J), "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes,
             hp_simdr_loss_workspace_bytes(B, J));
  const long R = (long)B * J;
  SimdrArgs args;
  args.ax[0] = simdr_axis(pred_x, nullptr, nx, stride_x, label_smoothing, R);
  args.ax[1] = simdr_axis(pred_y, nullptr, ny, stride_y, label_smoothing, R);
  args.ax[2] = simdr_axis(pred_z, nullptr, nz, stride_z, label_smoothing, R);
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const unsigned grid = (unsigned)((R * 3 + HL_BT / 64 - 1) / (HL_BT / 64));
  {
    HP_PROF("k_simdr_fwd", st);
    hipLaunchKernelGGL(k_simdr_fwd, dim3(grid), dim3(HL_BT), 0, st, args, target, weight, (int)R, stat, partial);
  }
  {
    HP_PROF("k_sum_partials", st);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(HL_BT), 0, st, partial, R * 3, 1.0 / (double)R, loss);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}

extern "C" int hp_simdr_loss_backward(const float* pred_x, int nx, long stride_x, const float* pred_y, int ny, long stride_y,
                                      const float* pred_z, int nz, long stride_z, const float* target, const float* weight, int B, int J,
                                      double label_smoothing, const float* stat, const float* gloss, float* dx, float* dy, float* dz,
                                      void* stream) {
  const char* who = "hp_simdr_loss_backward";
  const int rc = simdr_check(who, pred_x, nx, stride_x, pred_y, ny, stride_y, pred_z, nz, stride_z, target, B, J, label_smoothing);
  if (rc != HP_OK) return rc;
  HP_REQUIRE(stat && gloss && dx && dy && dz, "%s: null pointer", who);
  const long R = (long)B * J;
  SimdrArgs args;
  args.ax[0] = simdr_axis(pred_x, dx, nx, stride_x, label_smoothing, R);
  args.ax[1] = simdr_axis(pred_y, dy, ny, stride_y, label_smoothing, R);
  args.ax[2] = simdr_axis(pred_z, dz, nz, stride_z, label_smoothing, R);
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((R * 3 + HL_BT / 64 - 1) / (HL_BT / 64));
  {
    HP_PROF("k_simdr_bwd", st);
    hipLaunchKernelGGL(k_simdr_bwd, dim3(grid), dim3(HL_BT), 0, st, args, target, weight, stat, gloss, (int)R);
  }
  HP_CHECK_HIP(hipGetLastError());
  return HP_OK;
}
