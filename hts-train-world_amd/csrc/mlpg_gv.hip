// mlpg_gv.hip -- parameter generation considering global variance (what HMGenS does with USEHMMGV = 1 and OPTKIND = NEWTON,
// scripts/Training.pl:1892-1903): the stage that stands in mlpg's place when the trajectories are to keep an utterance's
// variance; include/world_mi355.h states the definition and tests/gv_reference.py states it in numpy.
//
// launch_mlpg_gv runs mlpg.hip's solve first (no voicing mask: the start c0 is the float32 trajectory before the
// overwrite; flagged columns are recorded one by one) and then mlpg_gv_kernel: one workgroup of 256 lanes per column
// (utterance, stream, dimension), frames across lanes (frame t belongs to lane t mod 256), every trial parallel over t.
//   set-up     row t of R = W' P W as its upper band R[t][t + j], j = 0 .. B = 2 max h_i, and r = W' P mu, from the stream's
//              taps in LDS and the float32 means and variances; to the batch's workspace, [column][j][t], so that a
//              lane's loads of one j are adjacent.  Rc is then a stencil of half-width B: the upper band of row t and, by
//              symmetry, entry j of rows t - j.
//   state      c, the candidate c' and the direction d: in LDS when T <= kGvLdsFrames (3 x 16 KB; with the membership
//              bytes and the taps 50.6 KB of the 64 KB a workgroup may declare, three workgroups per CU), else behind
//              the column's band in the workspace.  The code is one: the pointers are generic.
//   sums       sum c, then (sum e^2, c'Rc, c'r) together: a lane adds its own frames in order of t, the 64 lanes of a wave
//              by a butterfly, the 4 waves in a fixed order.  The order depends on T alone, every lane ends with the same
//              bits, and so the accept / reject branch is uniform in the workgroup.
// Workspace per frame and column: (B + 2) doubles, (B + 5) in a batch that holds an utterance above kGvLdsFrames.
#include <math.h>
#include <string.h>

#include "batch.hpp"
#include "common.hpp"
#include "streamwin.hpp"

namespace wm {

constexpr int kGvThreads = 256, kGvWaves = kGvThreads / 64;
constexpr int kGvLdsFrames = 2048;
constexpr int kGvRow = 16;                         // taps of a window in LDS

struct GvMeta {
  WinTable<kWinMaxTaps> win;
  int n_streams, edge, var_per_frame, input_type;
  int hmax[kWinMaxStreams], blk0[kWinMaxStreams], col0[kWinMaxStreams];
  int64_t ws_off[kWinMaxStreams];                  // in doubles
  int width, spill, max_iter, scale;
  float unvoiced;
  double epsilon, step_init, step_inc, step_dec, w_hmm, w_gv;
  const float* mean[kWinMaxStreams];
  const float* var[kWinMaxStreams];
  const float* msd[kWinMaxStreams];
  const float* gv_mean[kWinMaxStreams];
  const float* gv_var[kWinMaxStreams];
  float* out[kWinMaxStreams];
  int64_t ld_mean, ld_var;
};
static_assert(sizeof(GvMeta) <= 3072, "passed by value: well inside the 4 KB of kernel arguments");

// The coefficient of row (tau, i) of W at column tp in [0, T): window.pl's clamp lands the taps beyond an end on the
// end frame (edge 1), SPTK drops them (edge 0).  Any tau and tp: 0 where the row does not reach the column.
__device__ __forceinline__ double gv_coef(const double* w, int edge, int size, int tau, int tp, int T) {
  const int k = tp - tau + ((size - 1) >> 1);
  if (edge == 0 || (tp > 0 && tp < T - 1)) return k >= 0 && k < size ? w[k] : 0.0;
  int lo = tp == 0 ? 0 : k, hi = tp == T - 1 ? size - 1 : k;
  lo = lo < 0 ? 0 : lo;
  hi = hi > size - 1 ? size - 1 : hi;
  double a = 0.0;
  for (int kk = lo; kk <= hi; ++kk) a += w[kk];
  return a;
}

// x[k] summed over the workgroup, the same bits in every lane: butterfly in the wave, then the waves in order.  red is
// the kernel's one scratch for it, read as [4][K]: a round's first barrier keeps it from the readers of the round before.
template <int K>
__device__ __forceinline__ void gv_reduce(double (&x)[K], double (*red)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x[k] += __shfl_xor(x[k], off, 64);
  __syncthreads();                                                       // the last round's readers of red are through
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = x[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

__global__ __launch_bounds__(kGvThreads) void mlpg_gv_kernel(GvMeta m, const int64_t* __restrict__ f_off,
                                                             const unsigned char* __restrict__ gv_mask,
                                                             const int* __restrict__ colflag, double* __restrict__ ws,
                                                             double* __restrict__ info, int* __restrict__ status) {
  int s = 0;
#pragma unroll
  for (int q = 1; q < kWinMaxStreams; ++q)
    if (q < m.n_streams && (int)blockIdx.x >= m.blk0[q]) s = q;
  const int dim = m.win.dim[s];
  const int rel = (int)blockIdx.x - m.blk0[s];
  const int u = rel / dim, col = rel - u * dim;
  const int64_t fb = f_off[u];
  const int T = (int)(f_off[u + 1] - fb);
  const int tid = (int)threadIdx.x;
  __shared__ double wz[kWinMaxWin][kGvRow];
  __shared__ double lds[3][kGvLdsFrames];
  __shared__ double red[kGvWaves][3];
  __shared__ unsigned char gl[kGvLdsFrames];
  for (int e = tid; e < kWinMaxWin * kGvRow; e += kGvThreads) {
    const int i = e / kGvRow, k = e - i * kGvRow;
    wz[i][k] = i < m.win.nwin[s] && k < m.win.wsize[s][i] ? m.win.w[s][i][k < kWinMaxTaps ? k : 0] : 0.0;
  }
  if (T <= 0) return;
  const int64_t colid = (int64_t)u * m.width + m.col0[s] + col;
  double* __restrict__ inf_out = info != nullptr ? info + colid * 4 : nullptr;
  if (colflag[colid] != 0) {                       // ParameterGeneration's flagged column: zeros, whatever the voicing
    if (inf_out != nullptr && tid < 4) inf_out[tid] = 0.0;
    return;
  }
  const int nwin = m.win.nwin[s], B = 2 * m.hmax[s], edge = m.edge;
  const int64_t ldm = m.ld_mean, ldv = m.var_per_frame ? m.ld_var : 0, vb = m.var_per_frame ? fb : 0;
  const float* __restrict__ mean = m.mean[s] + col;
  const float* __restrict__ var = m.var[s] + col;
  const float* __restrict__ msd = m.msd[s];
  float* __restrict__ out = m.out[s] + (fb * dim + col);
  const bool fits = T <= kGvLdsFrames;
  const int P = B + 2 + (m.spill ? 3 : 0);
  double* band = ws + m.ws_off[s] + (fb * dim + (int64_t)col * T) * P;      // band[j * T + t] = R[t][t + j]
  double* rr = band + (int64_t)(B + 1) * T;
  double* c = fits ? lds[0] : rr + T;
  double* cn = fits ? lds[1] : rr + 2 * (int64_t)T;
  double* d = fits ? lds[2] : rr + 3 * (int64_t)T;

  auto voiced = [&](int t) -> bool { return msd == nullptr || msd[(fb + t) * ldm] >= 0.5f; };
  auto member = [&](int t) -> bool { return voiced(t) && (gv_mask == nullptr || gv_mask[fb + t] != 0); };
  auto in_g = [&](int t) -> bool { return fits ? gl[t] != 0 : member(t); };
  auto finish = [&](const double* x) {
    for (int t = tid; t < T; t += kGvThreads) out[(int64_t)t * dim] = voiced(t) ? (float)x[t] : m.unvoiced;
  };

  // the start, the GV set and its size
  double cnt[1] = {0.0};
  for (int t = tid; t < T; t += kGvThreads) {
    c[t] = (double)out[(int64_t)t * dim];
    const bool g = member(t);
    if (fits) gl[t] = g ? 1 : 0;
    cnt[0] += g ? 1.0 : 0.0;
  }
  gv_reduce<1>(cnt, reinterpret_cast<double(*)[1]>(&red[0][0]));
  const double N = cnt[0];

  // m and v of x over G, two passes; x is visible to the workgroup
  auto mean_of = [&](const double* x) -> double {
    double a[1] = {0.0};
    for (int t = tid; t < T; t += kGvThreads) a[0] += in_g(t) ? x[t] : 0.0;
    gv_reduce<1>(a, reinterpret_cast<double(*)[1]>(&red[0][0]));
    return a[0] / N;
  };
  const float gm = m.gv_mean[s][col], gvv = m.gv_var[s][col];
  const float finf = __builtin_inff();
  const bool bad_gv = !(gm > 0.0f && gm < finf && gvv > 0.0f && gvv < finf);
  const double mu_v = (double)gm, p_v = 1.0 / (double)gvv;
  double m0 = 0.0, v0 = 0.0;
  if (N >= 2.0) {
    m0 = mean_of(c);
    double a[1] = {0.0};
    for (int t = tid; t < T; t += kGvThreads) {
      const double e = in_g(t) ? c[t] - m0 : 0.0;
      a[0] = __builtin_fma(e, e, a[0]);
    }
    gv_reduce<1>(a, reinterpret_cast<double(*)[1]>(&red[0][0]));
    v0 = a[0] / N;
  }
  const bool degenerate = !(N >= 2.0 && v0 > 0.0 && v0 < (double)finf);
  if (bad_gv || degenerate) {                      // uniform: the column is ParameterGeneration's
    if (tid == 0 && status != nullptr) atomicOr(status + u, bad_gv ? 1 : 4);
    if (inf_out != nullptr && tid < 4) inf_out[tid] = 0.0;
    finish(c);
    return;
  }

  // R's upper band and r
  const bool is_prec = m.input_type != 0;
  auto precision = [&](int tau, int i) -> double {
    const double v = (double)var[(vb + tau) * ldv + i * dim];
    return is_prec ? v : 1.0 / v;
  };
  for (int t = tid; t < T; t += kGvThreads) {
    double z = 0.0;
    for (int i = 0; i < nwin; ++i) {
      const int size = m.win.wsize[s][i], h = (size - 1) >> 1;
      const int lo = t - h < 0 ? 0 : t - h, hi = t + h > T - 1 ? T - 1 : t + h;
      for (int tau = lo; tau <= hi; ++tau)
        z = __builtin_fma(precision(tau, i) * gv_coef(wz[i], edge, size, tau, t, T),
                          (double)mean[(fb + tau) * ldm + i * dim], z);
    }
    rr[t] = z;
    for (int j = 0; j <= B; ++j) {
      double a = 0.0;
      if (t + j < T)
        for (int i = 0; i < nwin; ++i) {
          const int size = m.win.wsize[s][i], h = (size - 1) >> 1;
          const int lo = t - h < 0 ? 0 : t - h, hi = t + h > T - 1 ? T - 1 : t + h;
          for (int tau = lo; tau <= hi; ++tau)
            a = __builtin_fma(precision(tau, i) * gv_coef(wz[i], edge, size, tau, t, T),
                              gv_coef(wz[i], edge, size, tau, t + j, T), a);
        }
      band[(int64_t)j * T + t] = a;
    }
  }
  __syncthreads();

  const double hw = m.w_hmm / ((double)nwin * (double)T), gw = m.w_gv * p_v;
  auto r_dot = [&](const double* x, int t) -> double {                    // (R x)_t
    double a = band[t] * x[t];
    for (int j = 1; j <= B; ++j) {
      if (t + j < T) a = __builtin_fma(band[(int64_t)j * T + t], x[t + j], a);
      if (t - j >= 0) a = __builtin_fma(band[(int64_t)j * T + t - j], x[t - j], a);
    }
    return a;
  };
  // f(x) with its m and v; x is made visible first
  auto objective = [&](const double* x, double& mx, double& vx) -> double {
    __syncthreads();
    mx = mean_of(x);
    double a[3] = {0.0, 0.0, 0.0};
    for (int t = tid; t < T; t += kGvThreads) {
      const double xt = x[t], e = in_g(t) ? xt - mx : 0.0;
      a[0] = __builtin_fma(e, e, a[0]);
      a[1] = __builtin_fma(xt, r_dot(x, t), a[1]);
      a[2] = __builtin_fma(xt, rr[t], a[2]);
    }
    gv_reduce<3>(a, red);
    vx = a[0] / N;
    const double dv = vx - mu_v;
    return hw * (-0.5 * a[1] + a[2]) - 0.5 * gw * dv * dv;
  };
  auto direction = [&](const double* x, double mx, double vx) {           // d at x, whose m and v are mx and vx
    const double dv = vx - mu_v;
    for (int t = tid; t < T; t += kGvThreads) {
      const bool g = in_g(t);
      const double e = g ? x[t] - mx : 0.0, rtt = band[t];
      const double grad = hw * (rr[t] - r_dot(x, t)) - gw * dv * (2.0 / N) * e;
      const double H = -hw * rtt - (g ? gw * (2.0 / (N * N)) * ((N - 1.0) * dv + 2.0 * e * e) : 0.0);
      const double floor_ = 1.0e-3 * hw * rtt;
      d[t] = grad / (-H > floor_ ? -H : floor_);
    }
  };

  if (m.scale != 0) {
    const double k = sqrt(mu_v / v0);
    for (int t = tid; t < T; t += kGvThreads)
      if (in_g(t)) c[t] = m0 + k * (c[t] - m0);
  }
  double mc, vc;
  double f = objective(c, mc, vc);
  const double f_start = f;
  double step = m.step_init;
  int trials = 0, accepts = 0;
  if (m.max_iter > 0) direction(c, mc, vc);
  for (int k = 0; k < m.max_iter; ++k) {
    for (int t = tid; t < T; t += kGvThreads) cn[t] = __builtin_fma(step, d[t], c[t]);
    double mn, vn;
    const double fn = objective(cn, mn, vn);
    ++trials;
    if (fn >= f) {                                 // the same bits in every lane: uniform
      double* sw = c;
      c = cn;
      cn = sw;
      const double gain = (fn - f) / fabs(fn);
      f = fn;
      mc = mn;
      vc = vn;
      ++accepts;
      step *= m.step_inc;
      if (m.epsilon > 0.0 && gain < m.epsilon) break;
      if (k + 1 < m.max_iter) direction(c, mc, vc);
    } else {
      step *= m.step_dec;
    }
  }
  if (inf_out != nullptr && tid == 0) {
    inf_out[0] = f_start;
    inf_out[1] = f;
    inf_out[2] = (double)trials;
    inf_out[3] = (double)accepts;
  }
  finish(c);
}

// What WorldMi355ParameterGenerationGv refuses beyond check_mlpg, on the host alone.
int check_mlpg_gv(int n_streams, const int* dims, const float* const* gv_mean, const float* const* gv_var,
                  const WorldMi355GvOption* gv) {
  if (!gv_mean || !gv_var || !gv) return WM_ERR_BAD_ARG;
  for (int s = 0; s < n_streams; ++s)
    if (!gv_mean[s] || !gv_var[s]) return WM_ERR_BAD_ARG;
  auto positive = [](double x) { return x > 0.0 && x < HUGE_VAL; };
  if (gv->max_iter < 0 || gv->max_iter > 100000 || gv->scale < 0 || gv->scale > 1) return WM_ERR_BAD_ARG;
  if (!(gv->epsilon >= 0.0 && gv->epsilon < HUGE_VAL) || !(gv->gv_weight >= 0.0 && gv->gv_weight < HUGE_VAL))
    return WM_ERR_BAD_ARG;
  if (!positive(gv->step_init) || !positive(gv->step_inc) || !positive(gv->step_dec) || !positive(gv->hmm_weight))
    return WM_ERR_BAD_ARG;
  return WM_OK;
}

struct GvWs : StageWs {
  double* d = nullptr;
  int* flag = nullptr;
  int64_t cap = 0, flag_cap = 0;                   // in doubles, in ints
};

int launch_mlpg_gv(Batch& b, hipStream_t st, int n_streams, const float* const* mean, int64_t ld_mean,
                   const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                   const double* const* const* windows, const int* const* window_sizes, const float* const* msd,
                   const WorldMi355MlpgOption& opt, const float* const* gv_mean, const float* const* gv_var,
                   const unsigned char* gv_mask, const WorldMi355GvOption& gv, float* const* out, double* info,
                   int* d_status) {
  if (const int rc = check_mlpg(n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes, &opt, out))
    return rc;
  if (const int rc = check_mlpg_gv(n_streams, dims, gv_mean, gv_var, &gv)) return rc;
  if (b.total_f <= 0 || b.n_utt <= 0) return WM_OK;
  GvMeta m;
  memset(&m, 0, sizeof(m));
  m.n_streams = n_streams;
  m.edge = opt.edge;
  m.var_per_frame = opt.var_per_frame != 0;
  m.input_type = opt.input_type;
  m.unvoiced = (float)opt.unvoiced_value;
  m.ld_mean = ld_mean;
  m.ld_var = ld_var;
  m.spill = b.max_f0_len > kGvLdsFrames;
  m.max_iter = gv.max_iter;
  m.scale = gv.scale;
  m.epsilon = gv.epsilon;
  m.step_init = gv.step_init;
  m.step_inc = gv.step_inc;
  m.step_dec = gv.step_dec;
  m.w_hmm = gv.hmm_weight;
  m.w_gv = gv.gv_weight;
  int64_t need = 0, blocks = 0;
  for (int s = 0; s < n_streams; ++s) {
    win_fill(m.win, s, s, dims, n_windows, windows, window_sizes);
    m.hmax[s] = win_hmax(n_windows[s], window_sizes[s]);
    m.blk0[s] = (int)blocks;
    m.col0[s] = m.width;
    m.ws_off[s] = need;
    m.mean[s] = mean[s];
    m.var[s] = var[s];
    m.msd[s] = msd != nullptr ? msd[s] : nullptr;
    m.gv_mean[s] = gv_mean[s];
    m.gv_var[s] = gv_var[s];
    m.out[s] = out[s];
    m.width += dims[s];
    blocks += (int64_t)dims[s] * b.n_utt;
    need += b.total_f * (int64_t)dims[s] * (2 * m.hmax[s] + 2 + (m.spill ? 3 : 0));
    if (blocks > (int64_t)1 << 28) return WM_ERR_BAD_ARG;
  }
  const int64_t n_flag = (int64_t)b.n_utt * m.width;
  GvWs* W = nullptr;
  if (const int rc = grow_ws(b.mlpg_gv, st, W, [&](const GvWs& w) { return w.cap >= need && w.flag_cap >= n_flag; },
                             [&](GvWs& n) {
                               n.cap = need;
                               n.flag_cap = n_flag;
                               if (const int rc = wm_check(n.alloc(&n.d, sizeof(double) * (size_t)need))) return rc;
                               return wm_check(n.alloc(&n.flag, sizeof(int) * (size_t)n_flag));
                             }))
    return rc;
  if (const int rc = wm_check(hipMemsetAsync(W->flag, 0, sizeof(int) * (size_t)n_flag, st))) return rc;
  // the start: the solve without the voicing overwrite, which mlpg_gv_kernel applies at its end
  if (const int rc = launch_mlpg_flags(b, st, n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes,
                                       nullptr, opt, out, d_status, W->flag))
    return rc;
  TimedScope ts_(b.ctx, st, "mlpg_gv_kernel");
  hipLaunchKernelGGL(mlpg_gv_kernel, dim3((unsigned)blocks), dim3(kGvThreads), 0, st, m, b.d_f_off, gv_mask, W->flag,
                     W->d, info, d_status);
  return wm_check(hipGetLastError());
}

}  // namespace wm
