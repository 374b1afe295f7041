// optim.hip -- the parameter update of DNNTraining.py's training step (DNNDefine.get_optimizer: tf.train.* of TF 1.x at
// their default hyper-parameters), for every tensor of a model in one launch.
//
// With g the gradient, p the parameter and r the tensor's rate, everything float32, every operation rounded on its own
// in the order written (no contraction: a fused a * b + c would be another rule, bit for bit):
//   sgd                                    p <- p - r g
//   momentum (mu)            a (0)         a <- a mu + g;                 p <- p - a r
//   adagrad                  a (0.1)       a <- a + g g;                  p <- p - (g r) / sqrt(a)
//   adadelta (rho, eps)      a (0), b (0)  a <- a rho + (g g) (1 - rho);  u = (sqrt(b + eps) / sqrt(a + eps)) g;
//                                          p <- p - u r;                  b <- b rho + (u u) (1 - rho)
//   adam (beta1, beta2, eps) m (0), v (0)  m <- m + (g - m) (1 - beta1);  v <- v + (g g - v) (1 - beta2);
//                                          p <- p - (m alpha) / (sqrt(v) + eps),
//                                          alpha = r sqrt(1 - beta2_power) / (1 - beta1_power) (float32, on the host)
//   rmsprop (rho, eps)       s (1)         s <- s + (g g - s) (1 - rho);  p <- p - (g r) / sqrt(s + eps)
// (the slots' initial values are the caller's).  1 - rho, 1 - beta are float32 differences formed on the host.  The
// division and the square root are the correctly rounded ones the build's flags give; subnormals are kept.
//
// optimizer_step_kernel: the table of the tensors travels in the kernel's arguments (nothing is copied to the device per
// call).  A block of 256 threads owns kOptBlock consecutive elements of one tensor, which it finds by a search over the
// tensors' first blocks -- the same for all its lanes, in scalar registers.  Where param, grad and the slots of a tensor
// are all 16-byte aligned the elements move as float4 (a tail shorter than 4 one by one), otherwise one by one.  A
// non-finite gradient element stores 1 into its tensor's status; the update is applied as written all the same.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "batch.hpp"
#include "common.hpp"

namespace wm {

constexpr int kOptMaxTensors = 64;
constexpr int kOptBlock = 4096;          // elements per block: 256 threads x 4 x float4

struct OptTable {
  float* param[kOptMaxTensors];
  const float* grad[kOptMaxTensors];
  float* slot0[kOptMaxTensors];
  float* slot1[kOptMaxTensors];
  int64_t count[kOptMaxTensors];
  float rate[kOptMaxTensors];            // adam: alpha
  int first[kOptMaxTensors];             // the tensor's first block
  int vec[kOptMaxTensors];               // its pointers are 16-byte aligned
  int n;
  float c0, c1, c2, c3, eps;             // momentum: mu; adadelta, rmsprop: rho, 1 - rho; adam: 1 - beta1, 1 - beta2
  int* status;
};

template <int RULE>
__device__ __forceinline__ void opt_update(float g, float& p, float& a, float& b, float r, const OptTable& t) {
#pragma clang fp contract(off)
  if (RULE == 0) {
    const float d = r * g;
    p = p - d;
  } else if (RULE == 1) {
    const float am = a * t.c0;
    a = am + g;
    const float d = a * r;
    p = p - d;
  } else if (RULE == 2) {
    const float gg = g * g;
    a = a + gg;
    const float gr = g * r;
    const float d = gr / sqrtf(a);
    p = p - d;
  } else if (RULE == 3) {
    const float gg = g * g;
    const float ar = a * t.c0;
    const float gs = gg * t.c1;
    a = ar + gs;
    const float nb = b + t.eps;
    const float na = a + t.eps;
    const float q = sqrtf(nb) / sqrtf(na);
    const float u = q * g;
    const float d = u * r;
    p = p - d;
    const float br = b * t.c0;
    const float uu = u * u;
    const float us = uu * t.c1;
    b = br + us;
  } else if (RULE == 4) {
    const float gm = g - a;
    const float dm = gm * t.c0;
    a = a + dm;
    const float gg = g * g;
    const float gv = gg - b;
    const float dv = gv * t.c1;
    b = b + dv;
    const float ma = a * r;
    const float den = sqrtf(b) + t.eps;
    const float d = ma / den;
    p = p - d;
  } else {
    const float gg = g * g;
    const float gs = gg - a;
    const float ds = gs * t.c1;
    a = a + ds;
    const float gr = g * r;
    const float se = a + t.eps;
    const float d = gr / sqrtf(se);
    p = p - d;
  }
}

__device__ __forceinline__ bool opt_finite(float g) { return fabsf(g) < __builtin_inff(); }

template <int RULE>
__global__ __launch_bounds__(256) void optimizer_step_kernel(const OptTable t) {
  constexpr bool S0 = RULE != 0, S1 = RULE == 3 || RULE == 4;
  // the last tensor whose first block is not beyond this block: t.first ascends, t.first[0] == 0
  const int blk = (int)blockIdx.x;
  int lo = 0, hi = t.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.first[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  const int k = lo;
  const int64_t n = t.count[k];
  const int64_t e0 = (int64_t)(blk - t.first[k]) * kOptBlock;
  float* __restrict__ P = t.param[k];
  const float* __restrict__ G = t.grad[k];
  float* __restrict__ A = S0 ? t.slot0[k] : nullptr;
  float* __restrict__ B = S1 ? t.slot1[k] : nullptr;
  const float r = t.rate[k];
  const int tid = (int)threadIdx.x;
  bool bad = false;
  if (t.vec[k]) {
    float4 g[4], p[4], a[4], b[4];
    bool on[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t e = e0 + (int64_t)(i * 256 + tid) * 4;
      on[i] = e + 3 < n;
      g[i] = p[i] = a[i] = b[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (on[i]) {
        g[i] = *reinterpret_cast<const float4*>(G + e);
        p[i] = *reinterpret_cast<const float4*>(P + e);
        if (S0) a[i] = *reinterpret_cast<const float4*>(A + e);
        if (S1) b[i] = *reinterpret_cast<const float4*>(B + e);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!on[i]) continue;
      const int64_t e = e0 + (int64_t)(i * 256 + tid) * 4;
      bad |= !(opt_finite(g[i].x) && opt_finite(g[i].y) && opt_finite(g[i].z) && opt_finite(g[i].w));
      opt_update<RULE>(g[i].x, p[i].x, a[i].x, b[i].x, r, t);
      opt_update<RULE>(g[i].y, p[i].y, a[i].y, b[i].y, r, t);
      opt_update<RULE>(g[i].z, p[i].z, a[i].z, b[i].z, r, t);
      opt_update<RULE>(g[i].w, p[i].w, a[i].w, b[i].w, r, t);
      *reinterpret_cast<float4*>(P + e) = p[i];
      if (S0) *reinterpret_cast<float4*>(A + e) = a[i];
      if (S1) *reinterpret_cast<float4*>(B + e) = b[i];
    }
    // the tensor's last n % 4 elements, in its last block
    const int64_t e = (n & ~(int64_t)3) + tid;
    if (tid < 3 && e < n && e >= e0 && e < e0 + kOptBlock) {
      const float g1 = G[e];
      float p1 = P[e], a1 = S0 ? A[e] : 0.0f, b1 = S1 ? B[e] : 0.0f;
      bad |= !opt_finite(g1);
      opt_update<RULE>(g1, p1, a1, b1, r, t);
      P[e] = p1;
      if (S0) A[e] = a1;
      if (S1) B[e] = b1;
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < kOptBlock / 256; ++i) {
      const int64_t e = e0 + i * 256 + tid;
      if (e >= n) break;
      const float g1 = G[e];
      float p1 = P[e], a1 = S0 ? A[e] : 0.0f, b1 = S1 ? B[e] : 0.0f;
      bad |= !opt_finite(g1);
      opt_update<RULE>(g1, p1, a1, b1, r, t);
      P[e] = p1;
      if (S0) A[e] = a1;
      if (S1) B[e] = b1;
    }
  }
  if (bad && t.status != nullptr) t.status[k] = 1;
}

// ---- host ----------------------------------------------------------------------------------------------------------
static bool opt_fin(float v) { return v - v == 0.0f; }

int check_optimizer_step(const WorldMi355OptimizerOption* o, int n_tensors, float* const* param, const float* const* grad,
                         float* const* slot0, float* const* slot1, const int64_t* count, const float* rate) {
  if (!o || !param || !grad || !count || !rate) return WM_ERR_BAD_ARG;
  if (n_tensors < 1 || n_tensors > kOptMaxTensors || o->rule < 0 || o->rule > 5) return WM_ERR_BAD_ARG;
  const bool s0 = o->rule != 0, s1 = o->rule == 3 || o->rule == 4;
  if ((s0 && !slot0) || (s1 && !slot1)) return WM_ERR_BAD_ARG;
  if (!opt_fin(o->momentum) || !opt_fin(o->rho) || !opt_fin(o->beta1) || !opt_fin(o->beta2) || !opt_fin(o->epsilon) ||
      !opt_fin(o->beta1_power) || !opt_fin(o->beta2_power))
    return WM_ERR_BAD_ARG;
  if (o->rule == 4 && !(o->beta1_power > 0.0f && o->beta1_power < 1.0f && o->beta2_power > 0.0f && o->beta2_power < 1.0f))
    return WM_ERR_BAD_ARG;
  int64_t blocks = 0;
  for (int k = 0; k < n_tensors; ++k) {
    if (!param[k] || !grad[k] || (s0 && !slot0[k]) || (s1 && !slot1[k])) return WM_ERR_BAD_ARG;
    if (count[k] < 1 || !(rate[k] >= 0.0f) || !opt_fin(rate[k])) return WM_ERR_BAD_ARG;
    blocks += (count[k] + kOptBlock - 1) / kOptBlock;
    if (blocks > (int64_t)0x7fffffff) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

int launch_optimizer_step(Context& c, hipStream_t st, const WorldMi355OptimizerOption& o, int n_tensors, float* const* param,
                          const float* const* grad, float* const* slot0, float* const* slot1, const int64_t* count,
                          const float* rate, int* d_status) {
  if (const int rc = check_optimizer_step(&o, n_tensors, param, grad, slot0, slot1, count, rate)) return rc;
  const bool s0 = o.rule != 0, s1 = o.rule == 3 || o.rule == 4;
  OptTable t;
  memset(&t, 0, sizeof(t));
  t.n = n_tensors;
  t.status = d_status;
  t.eps = o.epsilon;
  float scale = 1.0f, unbias = 1.0f;     // alpha = (r scale) / unbias
  switch (o.rule) {
    case 1: t.c0 = o.momentum; break;
    case 3:
    case 5: t.c0 = o.rho; t.c1 = 1.0f - o.rho; break;
    case 4:
      t.c0 = 1.0f - o.beta1;
      t.c1 = 1.0f - o.beta2;
      scale = sqrtf(1.0f - o.beta2_power);
      unbias = 1.0f - o.beta1_power;
      break;
    default: break;
  }
  int64_t blocks = 0;
  for (int k = 0; k < n_tensors; ++k) {
    t.param[k] = param[k];
    t.grad[k] = grad[k];
    t.slot0[k] = s0 ? slot0[k] : nullptr;
    t.slot1[k] = s1 ? slot1[k] : nullptr;
    t.count[k] = count[k];
    if (o.rule == 4) {
      const float rs = rate[k] * scale;
      t.rate[k] = rs / unbias;
    } else {
      t.rate[k] = rate[k];
    }
    t.first[k] = (int)blocks;
    t.vec[k] = (((uintptr_t)t.param[k] | (uintptr_t)t.grad[k] | (uintptr_t)t.slot0[k] | (uintptr_t)t.slot1[k]) % 16 == 0) ? 1 : 0;
    blocks += (count[k] + kOptBlock - 1) / kOptBlock;
  }
  if (d_status != nullptr)
    if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)n_tensors, st))) return rc;
  TimedScope ts_(&c, st, "optimizer_step_kernel");
  const dim3 g((unsigned)blocks), b(256);
  switch (o.rule) {
    case 0: hipLaunchKernelGGL((optimizer_step_kernel<0>), g, b, 0, st, t); break;
    case 1: hipLaunchKernelGGL((optimizer_step_kernel<1>), g, b, 0, st, t); break;
    case 2: hipLaunchKernelGGL((optimizer_step_kernel<2>), g, b, 0, st, t); break;
    case 3: hipLaunchKernelGGL((optimizer_step_kernel<3>), g, b, 0, st, t); break;
    case 4: hipLaunchKernelGGL((optimizer_step_kernel<4>), g, b, 0, st, t); break;
    default: hipLaunchKernelGGL((optimizer_step_kernel<5>), g, b, 0, st, t); break;
  }
  return wm_check(hipGetLastError());
}

}  // namespace wm
