// mlpg.hip -- smooth static trajectories from the means and variances of static and dynamic features (SPTK `mlpg`,
// scripts/Training.pl:2755-2810 gen_param): the inverse of cmp_compose_kernel (codec.hip), the stage between a model's
// `cmp`-layout rows and WorldMi355RecipeDecode / WorldMi355MelCepstrumToSpectrum.
//
// One column (utterance, stream, dimension) with T frames and the stream's windows w_0 .. w_{n-1} (centre tap h_i):
//   W   (n T) x T, row (tau, i) holds w_i[k] at column tau + k - h_i (edge 0: a column outside [0, T) is dropped, SPTK's
//       rule; edge 1: the column is clamped, window.pl's rule and cmp_compose_kernel's),
//   P   diag(1 / variance),    out = c with (W' P W) c = W' P mu.
// R = W' P W is symmetric, banded (half-bandwidth 2 max h_i) and positive definite with a static window.  The kernel
// is the banded LDL' of banded.hpp in double, right-looking, one column per lane and sequential in t:
//   forward   row t of R and of r = W' P mu is built from the taps that reach frame t (float32 loads, double sums) and
//             takes in the updates earlier pivots owe it (banded.hpp's register triangle).  z / d and the B multipliers
//             go to the batch's workspace, [frame][k][column].
//   backward  c[t] = z[t] / d[t] - sum_j l[t][j] c[t + j], float32 out, voicing mask.
// B is a template parameter (0, 2, 4, 14) and the launcher takes the smallest that holds a stream's band.
//
// Packing: one wave per (utterance, stream, 64 dimensions).  T, the windows and the edge cases are then the same in all
// 64 lanes: the block keeps its stream's taps in LDS and every branch on t is wave-uniform.  The price is idle
// lanes when a stream is narrow ("Parameter generation").
#include <math.h>
#include <string.h>

#include "banded.hpp"
#include "batch.hpp"
#include "common.hpp"

namespace wm {

struct MlpgMeta {
  BandTable<kWinMaxTaps> t;
  int edge, var_per_frame, input_type;
  float unvoiced;
  const float* mean[kWinMaxStreams];
  const float* var[kWinMaxStreams];
  const float* msd[kWinMaxStreams];
  float* out[kWinMaxStreams];
  int64_t ld_mean, ld_var;
};
static_assert(sizeof(MlpgMeta) == 2264, "the kernel's arguments are the size they were before the tables were shared");

// The row length of the taps in LDS (band_stage_taps): an index tp - tau + h_i with tau in [t - h_i, t + h_i] and tp in
// [t, t + B] lies in [0, 2 h_i + B] <= 28.
constexpr int kMlpgRow = 32;

// The coefficient of row (tau, i) of W at column tp < T, tau - h_i <= tp; with edge 0, tp <= tau + h_i + 14.
__device__ __forceinline__ double mlpg_coef(const double (*wz)[kMlpgRow], int edge, int i, int size, int tau, int tp,
                                            int T) {
  const int k = tp - tau + ((size - 1) >> 1);
  if (edge == 0 || (tp > 0 && tp < T - 1)) return wz[i][k];
  int lo = tp == 0 ? 0 : k, hi = tp == T - 1 ? size - 1 : k;          // the taps that the clamp lands on an end frame
  hi = hi > size - 1 ? size - 1 : hi;
  double a = 0.0;
  for (int kk = lo; kk <= hi; ++kk) a += wz[i][kk];
  return a;
}

// Where a flagged column is also recorded by itself (the status word is per utterance): p[u * width + col0[slot] + col],
// for the GV generation that follows the solve (mlpg_gv.hip).  p == nullptr: nothing is recorded.
struct MlpgColFlags {
  int* p;
  int width;
  int col0[kWinMaxStreams];
};

template <int B>
__global__ __launch_bounds__(64) void mlpg_kernel(MlpgMeta m, const int64_t* __restrict__ f_off,
                                                  double* __restrict__ ws, int* __restrict__ status, MlpgColFlags cf) {
  constexpr int BB = B > 0 ? B : 1;
  const BandBlock blk = band_decode(m.t);
  const int s = blk.s, u = blk.u, col = blk.col;
  const int64_t fb = f_off[u];
  const int T = (int)(f_off[u + 1] - fb);
  const int dim = m.t.win.dim[s];
  __shared__ double wz[kWinMaxWin][kMlpgRow];
  band_stage_taps(m.t, s, wz);
  __syncthreads();
  if (T <= 0 || col >= dim) return;
  const int nwin = m.t.win.nwin[s], hmax = m.t.hmax[s], edge = m.edge;
  const float* __restrict__ mean = m.mean[s] + col;
  const float* __restrict__ var = m.var[s] + col;
  const float* __restrict__ msd = m.msd[s];
  float* __restrict__ out = m.out[s] + col;
  const int64_t ldm = m.ld_mean, ldv = m.var_per_frame ? m.ld_var : 0;   // one variance row: every frame reads row 0
  const int64_t vb = m.var_per_frame ? fb : 0;
  double* __restrict__ wc = ws + m.t.ws_off[s] + col;
  const float inf = __builtin_inff();
  bool bad = false, sing = false;
  const bool is_prec = m.input_type != 0;
  auto precision = [&](float v) -> double {
    if (is_prec) {
      bad |= !(v >= 0.0f && v < inf);
      return (double)v;
    }
    bad |= !(v > 0.0f && v < inf);
    return 1.0 / (double)v;
  };
  auto store = [&](int t, double c) {
    const bool voiced = msd == nullptr || msd[(fb + t) * ldm] >= 0.5f;
    out[(fb + t) * (int64_t)dim] = voiced ? (float)c : m.unvoiced;
  };

  // with one variance row, the rows of R away from the ends are all the same: fi[j] = sum_i p_i sum_k w_i[k] w_i[k + j]
  double pw[kWinMaxWin], fi[B + 1];
#pragma unroll
  for (int j = 0; j <= B; ++j) fi[j] = 0.0;
#pragma unroll
  for (int i = 0; i < kWinMaxWin; ++i) {
    pw[i] = 0.0;
    if (!m.var_per_frame && i < nwin) {
      pw[i] = precision(var[i * dim]);
      band_fi_add<B>(pw[i], wz[i], m.t.win.wsize[s][i], fi);
    }
  }

  double D[BB][BB], q[BB];
#pragma unroll
  for (int a = 0; a < BB; ++a) {
    q[a] = 0.0;
#pragma unroll
    for (int j = 0; j < BB; ++j) D[a][j] = 0.0;
  }

  for (int t = 0; t < T; ++t) {
    double e[B + 1], z = 0.0;
    // every row that reaches t exists, and neither t nor a column those rows reach is an end frame
    const bool inner = !m.var_per_frame && t >= hmax && t >= edge && t + 2 * hmax + edge <= T - 1;
    if (inner) {
#pragma unroll
      for (int j = 0; j <= B; ++j) e[j] = fi[j];
#pragma unroll
      for (int i = 0; i < kWinMaxWin; ++i)
        if (i < nwin) {
          const int size = m.t.win.wsize[s][i], h = (size - 1) >> 1;
          const float* mp = mean + (fb + t - h) * ldm + i * dim;
          for (int k = size - 1; k >= 0; --k, mp += ldm) {                // row tau = t + h - k
            const float mu = *mp;
            bad |= !(fabsf(mu) < inf);
            z = __builtin_fma(pw[i] * wz[i][k], (double)mu, z);
          }
        }
    } else {
#pragma unroll
      for (int j = 0; j <= B; ++j) e[j] = 0.0;
#pragma unroll
      for (int i = 0; i < kWinMaxWin; ++i)
        if (i < nwin) {
          const int size = m.t.win.wsize[s][i], h = (size - 1) >> 1;
          const int lo = t - h < 0 ? 0 : t - h, hi = t + h > T - 1 ? T - 1 : t + h;
          for (int tau = lo; tau <= hi; ++tau) {
            const float mu = mean[(fb + tau) * ldm + i * dim];
            const float vv = var[(vb + tau) * ldv + i * dim];
            bad |= !(fabsf(mu) < inf);
            const double at = mlpg_coef(wz, edge, i, size, tau, t, T);
            const double pa = precision(vv) * at;
            z = __builtin_fma(pa, (double)mu, z);
            // the columns after t as if none of them were an end frame: put right below
            const double* wk = &wz[i][t - tau + h];
            e[0] = __builtin_fma(pa, at, e[0]);
#pragma unroll
            for (int j = 1; j <= B; ++j) e[j] = __builtin_fma(pa, wk[j], e[j]);
          }
        }
      const int j1 = T - 1 - t;                                           // the last frame's column
#pragma unroll
      for (int j = 1; j <= B; ++j) e[j] = j <= j1 ? e[j] : 0.0;
      if (B > 0 && edge != 0 && j1 >= 1 && j1 <= B) {                     // the clamp lands the rows' tails on it
        double ee = 0.0;
#pragma unroll
        for (int i = 0; i < kWinMaxWin; ++i)
          if (i < nwin) {
            const int size = m.t.win.wsize[s][i], h = (size - 1) >> 1;
            const int lo = t - h < 0 ? 0 : t - h, hi = t + h > T - 1 ? T - 1 : t + h;
            for (int tau = lo; tau <= hi; ++tau) {
              const double p = precision(var[(vb + tau) * ldv + i * dim]);
              ee = __builtin_fma(p * mlpg_coef(wz, edge, i, size, tau, t, T), mlpg_coef(wz, edge, i, size, tau, T - 1, T), ee);
            }
          }
#pragma unroll
        for (int j = 1; j <= B; ++j) e[j] = j == j1 ? ee : e[j];
      }
    }
    if (B > 0) {
#pragma unroll
      for (int j = 0; j < B; ++j) e[j] += D[0][j];
      z += q[0];
    }
    const double d = e[0];
    sing |= !(d > 0.0 && d < (double)inf);
    const double inv = 1.0 / d;
    const double zi = z * inv;
    if (B == 0) {
      store(t, zi);
    } else {
      double* wr = wc + (fb + t) * (int64_t)((B + 1) * dim);
      wr[0] = zi;
      band_pivot<B>(e, z, inv, D, q, wr, dim);
    }
  }

  // a flagged column is zeros, whatever the voicing
  const bool flagged = bad || sing;
  if (flagged) {
    if (status != nullptr) atomicOr(status + u, bad ? 1 : 2);
    if (cf.p != nullptr) cf.p[(int64_t)u * cf.width + cf.col0[s] + col] = 1;
    for (int t = 0; t < T; ++t) out[(fb + t) * (int64_t)dim] = 0.0f;
    return;
  }
  if (B > 0) {
    double c[BB];
#pragma unroll
    for (int j = 0; j < BB; ++j) c[j] = 0.0;                           // c[j] = c[t + 1 + j]
#pragma unroll 4
    for (int t = T - 1; t >= 0; --t) {
      const double* wr = wc + (fb + t) * (int64_t)((B + 1) * dim);
      double v = wr[0];
#pragma unroll
      for (int a = 1; a <= B; ++a) v = __builtin_fma(-wr[(int64_t)a * dim], c[a - 1], v);
#pragma unroll
      for (int j = BB - 1; j > 0; --j) c[j] = c[j - 1];
      c[0] = v;
      store(t, v);
    }
  }
}

// What WorldMi355ParameterGeneration refuses, on the host alone: no device call is made for a refused argument set.
int check_mlpg(int n_streams, const float* const* mean, int64_t ld_mean, const float* const* var, int64_t ld_var,
               const int* dims, const int* n_windows, const double* const* const* windows,
               const int* const* window_sizes, const WorldMi355MlpgOption* opt, float* const* out) {
  if (!mean || !var || !opt || !out) return WM_ERR_BAD_ARG;
  if (const int rc = check_windows(n_streams, dims, n_windows, windows, window_sizes, kWinMaxStreams, kWinMaxWin, kWinMaxTaps))
    return rc;
  if (opt->edge < 0 || opt->edge > 1 || opt->input_type < 0 || opt->input_type > 1) return WM_ERR_BAD_ARG;
  for (int s = 0; s < n_streams; ++s) {
    if (!mean[s] || !var[s] || !out[s]) return WM_ERR_BAD_ARG;
    const int64_t row = (int64_t)dims[s] * n_windows[s];
    if (ld_mean < row || (opt->var_per_frame && ld_var < row)) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

struct MlpgWs : StageWs {
  double* d = nullptr;
  int64_t cap = 0;           // in doubles
};

int launch_mlpg(Batch& b, hipStream_t st, int n_streams, const float* const* mean, int64_t ld_mean,
                const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                const double* const* const* windows, const int* const* window_sizes, const float* const* msd,
                const WorldMi355MlpgOption& opt, float* const* out, int* d_status) {
  return launch_mlpg_flags(b, st, n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes, msd, opt,
                           out, d_status, nullptr);
}

// launch_mlpg, which also sets d_colflag[u][column over the statics of all streams] of every flagged column (the caller
// zeroes it); nullptr: launch_mlpg itself.
int launch_mlpg_flags(Batch& b, hipStream_t st, int n_streams, const float* const* mean, int64_t ld_mean,
                      const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                      const double* const* const* windows, const int* const* window_sizes, const float* const* msd,
                      const WorldMi355MlpgOption& opt, float* const* out, int* d_status, int* d_colflag) {
  if (const int rc = check_mlpg(n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes, &opt, out))
    return rc;
  if (b.total_f <= 0 || b.n_utt <= 0) return WM_OK;
  // the factor: (B + 1) doubles per frame and column of the streams with a band
  BandPlan plan;
  if (const int rc = band_plan(plan, n_streams, dims, n_windows, window_sizes, b.total_f, b.n_utt,
                               [](int B) { return B > 0 ? B + 1 : 0; }))
    return rc;
  const int64_t need = plan.need;                        // 0: no stream has a band, the kernels take no workspace
  MlpgWs* W = static_cast<MlpgWs*>(b.mlpg.get());
  if (need > 0)
    if (const int rc = grow_ws(b.mlpg, st, W, [&](const MlpgWs& w) { return w.cap >= need; }, [&](MlpgWs& n) {
          n.cap = need;
          return wm_check(n.alloc(&n.d, sizeof(double) * (size_t)need));
        }))
      return rc;
  if (d_status != nullptr)
    if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st))) return rc;
  TimedScope ts_(b.ctx, st, "mlpg_kernel");
  for (int g = 0; g < 4; ++g) {
    MlpgMeta m;
    memset(&m, 0, sizeof(m));
    m.edge = opt.edge;
    m.var_per_frame = opt.var_per_frame != 0;
    m.input_type = opt.input_type;
    m.unvoiced = (float)opt.unvoiced_value;
    m.ld_mean = ld_mean;
    m.ld_var = ld_var;
    int src[kWinMaxStreams];
    const int blocks = band_group(m.t, src, plan, kBands[g], n_streams, dims, n_windows, windows, window_sizes, b.n_utt);
    if (m.t.n_streams == 0) continue;
    for (int k = 0; k < m.t.n_streams; ++k) {
      m.mean[k] = mean[src[k]];
      m.var[k] = var[src[k]];
      m.msd[k] = msd != nullptr ? msd[src[k]] : nullptr;
      m.out[k] = out[src[k]];
    }
    double* d_ws = W != nullptr ? W->d : nullptr;
    MlpgColFlags cf;
    memset(&cf, 0, sizeof(cf));
    cf.p = d_colflag;
    for (int q = 0; q < n_streams; ++q) cf.width += dims[q];
    for (int k = 0; k < m.t.n_streams; ++k)
      for (int q = 0; q < src[k]; ++q) cf.col0[k] += dims[q];
    switch (kBands[g]) {
      case 0: hipLaunchKernelGGL((mlpg_kernel<0>), dim3(blocks), dim3(64), 0, st, m, b.d_f_off, d_ws, d_status, cf); break;
      case 2: hipLaunchKernelGGL((mlpg_kernel<2>), dim3(blocks), dim3(64), 0, st, m, b.d_f_off, d_ws, d_status, cf); break;
      case 4: hipLaunchKernelGGL((mlpg_kernel<4>), dim3(blocks), dim3(64), 0, st, m, b.d_f_off, d_ws, d_status, cf); break;
      default: hipLaunchKernelGGL((mlpg_kernel<14>), dim3(blocks), dim3(64), 0, st, m, b.d_f_off, d_ws, d_status, cf); break;
    }
  }
  return wm_check(hipGetLastError());
}

}  // namespace wm
