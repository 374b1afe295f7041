// trj.hip -- the recipe's trajectory training criterion with its gradients (data/scripts/DNNDefine.py:240-399
// trajectory_cost, driven by DNNTraining.py -w win; scripts/Training.pl:930-940): the trajectory likelihood of the
// observed statics under the model's means and the trained variances, the voicing (MSD) term and the GV term.
//
// One column (utterance, stream, dimension) with T frames, windows w_0 .. w_{n-1} (centre tap h_i) and ONE variance row:
//   W_i  T x T, row tau holds w_i[h_i + j] at column tau + j (a column outside [0, T) is dropped: mlpg.hip's edge 0),
//   A = sum_i p_i W_i' W_i,  r = sum_i p_i W_i' mu_i,  c = A^-1 r,  e = o - c,
//   logdet = ln det A,  mahal = e' A e = sum_i p_i |W_i e|^2,  pv = mean_t (c_t - mean c)^2,  ov the same of o.
// The reference forms A^-1 densely (O(T^3) per column); A is banded with half-bandwidth B = 2 max h_i and the kernel
// keeps the banded LDL' of banded.hpp (mlpg_kernel's) in double, one column per lane, one wave per (utterance, stream, 64 dimensions):
//   sweep 1, forward   factor A, z = L^-1 (r - A o), sum ln d_t, the running mean and M2 of o (Welford), the input
//                      checks: the system is solved for x = c - o = -e (see there);
//   sweep 2, backward  x, c = o + x with its running mean and M2, and the band of A^-1 by the backward recurrence
//                      Z[t][t+k] = [k == 0] / d_t - sum_a l[t][a] Z[t+a][t+k]   (Takahashi),
//                      of which tr(A^-1 W_i' W_i) needs only the entries within the band;
//   sweep 3, forward   y = L^-1 g with g_t = (4 / T)(pv - ov)(c_t - mean c) / gv_var: it has to wait for mean c and pv;
//   sweep 4, backward  s = A^-1 g, and trailing it by h_i frames EVERY band multiply W_i x, W_i o, W_i s: the
//                      quadratic form, the gradients with respect to the means (-2 p_i W_i e and p_i W_i s) and the
//                      sums of the gradients with respect to the precisions.
// The workspace holds, per frame and column, [x (z / d before sweep 2) | l_1 .. l_B | 1 / d (y / d after sweep 3)],
// laid [frame][k][column].  Per-column terms go to a table [utterance][column][term]; trj_reduce_kernel sums them per
// utterance in column order, adds the voicing term and zeroes what a flagged utterance received.
#include <math.h>
#include <string.h>

#include "banded.hpp"
#include "batch.hpp"
#include "common.hpp"

namespace wm {

constexpr int kTrjRow = 16, kTrjTerms = 4;        // terms: ln det A, e' A e, (pv - ov)^2 / gv_var, ln gv_var
struct TrjMeta {
  BandTable<kTrjMaxTaps> t;
  int D;                                          // all columns of the call
  int width;                                      // of a row of grad_var
  double gv_weight;
  int col0[kWinMaxStreams];                      // the stream's first column among the D
  int var0[kWinMaxStreams];                      // the stream's window 0 in a row of grad_var
  const float* pred[kWinMaxStreams];
  const float* obs[kWinMaxStreams];
  const float* var[kWinMaxStreams];
  const float* gv_var[kWinMaxStreams];
  float* c[kWinMaxStreams];                      // or null
  float* grad[kWinMaxStreams];                   // or null
  int64_t ld, ld_grad;
};
static_assert(sizeof(TrjMeta) == 1080, "the kernel's arguments are the size they were before the tables were shared");

// A sum over the frames of an utterance whose terms share a sign (ln d_t, the trace, the quadratic form): the same
// value added T times rounds the same way T times, so the lost parts are kept and added at the end (Neumaier).
struct TrjSum {
  double s = 0.0, c = 0.0;
  __device__ __forceinline__ void add(double x) {
    const double t = s + x;
    c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
    s = t;
  }
  __device__ __forceinline__ double get() const { return s + c; }
};

template <int B>
__global__ __launch_bounds__(64) void trj_kernel(TrjMeta m, const int64_t* __restrict__ f_off, double* __restrict__ ws,
                                                 double* __restrict__ tab, double* __restrict__ grad_var,
                                                 int* __restrict__ status) {
  constexpr int BB = B > 0 ? B : 1;
  const BandBlock blk = band_decode(m.t);
  const int s = blk.s, u = blk.u, col = blk.col;
  const int64_t fb = f_off[u];
  const int T = (int)(f_off[u + 1] - fb);
  const int dim = m.t.win.dim[s];
  // the taps (an index up to 2 h + B <= 8 needs no range check: 4 x 16 entries, 64 lanes), and
  // gz[i][k] = sum_m w_i[m] w_i[m + k], row t of W_i' W_i at column t + k away from the ends
  __shared__ double wz[kWinMaxWin][kTrjRow];
  __shared__ double gz[kWinMaxWin][8];
  band_stage_taps(m.t, s, wz);
  __syncthreads();
  if (threadIdx.x < kWinMaxWin * 8) {
    const int i = (int)threadIdx.x >> 3, k = (int)threadIdx.x & 7;
    double a = 0.0;
    for (int mm = 0; mm + k < kTrjRow; ++mm) a = __builtin_fma(wz[i][mm], wz[i][mm + k], a);
    gz[i][k] = a;
  }
  __syncthreads();
  if (T <= 0 || col >= dim) return;
  const int nwin = m.t.win.nwin[s], hmax = m.t.hmax[s];
  const float* __restrict__ pred = m.pred[s] + col;
  const float* __restrict__ obs = m.obs[s] + col;
  float* __restrict__ cout = m.c[s] != nullptr ? m.c[s] + col : nullptr;
  float* __restrict__ grad = m.grad[s] != nullptr ? m.grad[s] + col : nullptr;
  const int64_t ld = m.ld, ldg = m.ld_grad;
  const int64_t row = (int64_t)(B + 2) * dim;                            // doubles per frame of this stream's workspace
  double* __restrict__ wc = ws + m.t.ws_off[s] + col;
  const float inf = __builtin_inff();
  bool bad = false, sing = false;

  // one variance row: the rows of A away from the ends are all fi[j] = sum_i p_i gz[i][j]
  double pw[kWinMaxWin], fi[B + 1];
#pragma unroll
  for (int j = 0; j <= B; ++j) fi[j] = 0.0;
#pragma unroll
  for (int i = 0; i < kWinMaxWin; ++i) {
    pw[i] = 0.0;
    if (i < nwin) {
      const float v = m.var[s][i * dim + col];
      bad |= !(v > 0.0f && v < inf);
      pw[i] = 1.0 / (double)v;
      band_fi_add<B>(pw[i], wz[i], m.t.win.wsize[s][i], fi);
    }
  }
  const float gvf = m.gv_var[s][col];
  bad |= !(gvf > 0.0f && gvf < inf);
  const double gvv = (double)gvf;

  // ---- sweep 1: the factor, z / d for the right-hand side r - A o, ln det A, the moments of o ----
  // The system is solved for x = c - o: its right-hand side sum_i p_i W_i' (mu_i - W_i o) is made of differences of
  // float32 values, which double forms (nearly) exactly, so e = -x carries the solve's error relative to |e| and not
  // the rounding of a c that may be a thousand times larger.  Row tau of every window enters once, when t = tau - h_i.
  TrjSum logdet;
  double mo = 0.0, m2o = 0.0;
  {
    double D[BB][BB], q[BB], ow[B + 1], dw[kWinMaxWin][B + 1];          // ow[j] = o[t + j]; dw[i][k] = (mu_i - W_i o)[t + h_i - k]
#pragma unroll
    for (int a = 0; a < BB; ++a) {
      q[a] = 0.0;
#pragma unroll
      for (int j = 0; j < BB; ++j) D[a][j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j <= B; ++j) {
      ow[j] = 0.0;
#pragma unroll
      for (int i = 0; i < kWinMaxWin; ++i) dw[i][j] = 0.0;
    }
    for (int t = -B; t < T; ++t) {
#pragma unroll
      for (int j = 0; j < B; ++j) ow[j] = ow[j + 1];
      {
        float of = 0.0f;
        if (t + B < T) {                                                 // t + B >= 0
          of = obs[(fb + t + B) * ld];
          bad |= !(fabsf(of) < inf);
        }
        ow[B] = (double)of;
      }
      if (t < -hmax) continue;
#pragma unroll
      for (int i = 0; i < kWinMaxWin; ++i)
        if (i < nwin) {
          const int tau = t + ((m.t.win.wsize[s][i] - 1) >> 1);
          double dn = 0.0;
          if (tau >= 0 && tau <= T - 1) {
            const float mu = pred[(fb + tau) * ld + i * dim];
            bad |= !(fabsf(mu) < inf);
            double yo = 0.0;
#pragma unroll
            for (int k = 0; k <= B; ++k) yo = __builtin_fma(wz[i][k], ow[k], yo);   // zeros beyond the window's taps
            dn = (double)mu - yo;
          }
#pragma unroll
          for (int k = B; k > 0; --k) dw[i][k] = dw[i][k - 1];
          dw[i][0] = dn;
        }
      if (t < 0) continue;
      double e[B + 1], z = 0.0;
      {
        const double o = ow[0], dl = o - mo;
        mo += dl / (double)(t + 1);
        m2o = __builtin_fma(dl, o - mo, m2o);
      }
#pragma unroll
      for (int i = 0; i < kWinMaxWin; ++i)
        if (i < nwin) {
          double zi = 0.0;
#pragma unroll
          for (int k = 0; k <= B; ++k) zi = __builtin_fma(wz[i][k], dw[i][k], zi);  // rows beyond the ends hold zeros
          z = __builtin_fma(pw[i], zi, z);
        }
      const bool inner = t >= hmax && t + 2 * hmax <= T - 1;             // every row that reaches t exists, whole
      if (inner) {
#pragma unroll
        for (int j = 0; j <= B; ++j) e[j] = fi[j];
      } else {
#pragma unroll
        for (int j = 0; j <= B; ++j) e[j] = 0.0;
#pragma unroll
        for (int i = 0; i < kWinMaxWin; ++i)
          if (i < nwin) {
            const int size = m.t.win.wsize[s][i], h = (size - 1) >> 1;
            const int lo = t - h < 0 ? 0 : t - h, hi = t + h > T - 1 ? T - 1 : t + h;
            for (int tau = lo; tau <= hi; ++tau) {
              const double* wk = &wz[i][t - tau + h];
              const double pa = pw[i] * wk[0];
#pragma unroll
              for (int j = 0; j <= B; ++j) e[j] = __builtin_fma(pa, wk[j], e[j]);
            }
          }
        const int j1 = T - 1 - t;                                         // the last frame's column
#pragma unroll
        for (int j = 1; j <= B; ++j) e[j] = j <= j1 ? e[j] : 0.0;
      }
      if (B > 0) {
#pragma unroll
        for (int j = 0; j < B; ++j) e[j] += D[0][j];
        z += q[0];
      }
      const double d = e[0];
      sing |= !(d > 0.0 && d < (double)inf);
      const double inv = 1.0 / d;
      logdet.add(log(d));
      double* wr = wc + (fb + t) * row;
      wr[0] = z * inv;
      wr[(int64_t)(B + 1) * dim] = inv;
      band_pivot<B>(e, z, inv, D, q, wr, dim);
    }
  }

  // a flagged column: zeros in c, its bit in the status; trj_reduce_kernel zeroes the utterance's costs and gradients
  if (bad || sing) {
    atomicOr(status + u, bad ? 1 : 2);
    if (cout != nullptr)
      for (int t = 0; t < T; ++t) cout[(fb + t) * (int64_t)dim] = 0.0f;
    return;
  }

  // ---- sweep 2: x = c - o, c and its moments, the band of A^-1 and the traces ----
  TrjSum tr[kWinMaxWin];
  double mc = 0.0, m2c = 0.0;
  {
    double cw[BB], Zw[BB][B + 1];                                       // x[t + 1 + j]; Zw[r][j] = Z[t + 1 + r][t + 1 + r + j]
#pragma unroll
    for (int a = 0; a < BB; ++a) {
      cw[a] = 0.0;
#pragma unroll
      for (int j = 0; j <= B; ++j) Zw[a][j] = 0.0;
    }
    for (int t = T - 1; t >= 0; --t) {
      double* wr = wc + (fb + t) * row;
      double l[BB], Zn[B + 1], v = wr[0];
#pragma unroll
      for (int a = 1; a <= B; ++a) {
        l[a - 1] = wr[(int64_t)a * dim];
        v = __builtin_fma(-l[a - 1], cw[a - 1], v);
      }
#pragma unroll
      for (int j = BB - 1; j > 0; --j) cw[j] = cw[j - 1];
      cw[0] = v;
      wr[0] = v;
      {
        const double c = (double)obs[(fb + t) * ld] + v, dl = c - mc;
        if (cout != nullptr) cout[(fb + t) * (int64_t)dim] = (float)c;
        mc += dl / (double)(T - t);
        m2c = __builtin_fma(dl, c - mc, m2c);
      }
      Zn[0] = wr[(int64_t)(B + 1) * dim];
#pragma unroll
      for (int k = 1; k <= B; ++k) {
        double zk = 0.0;
#pragma unroll
        for (int a = 1; a <= B; ++a)                                      // Z[t + a][t + k], by symmetry from the upper band
          zk = __builtin_fma(-l[a - 1], k >= a ? Zw[a - 1][k - a] : Zw[k - 1][a - k], zk);
        Zn[k] = zk;
      }
#pragma unroll
      for (int a = 1; a <= B; ++a) Zn[0] = __builtin_fma(-l[a - 1], Zn[a], Zn[0]);
#pragma unroll
      for (int i = 0; i < kWinMaxWin; ++i)
        if (i < nwin) {
          const int h = (m.t.win.wsize[s][i] - 1) >> 1;
          double acc = 0.0;
          if (t >= h && t + h <= T - 1) {
#pragma unroll
            for (int k = 1; k <= B; ++k) acc = __builtin_fma(Zn[k], gz[i][k], acc);
            acc = __builtin_fma(2.0, acc, Zn[0] * gz[i][0]);
          } else {                                                       // the rows of W_i that reach t, cut at the ends
            const int hi = t + h > T - 1 ? T - 1 : t + h;
#pragma unroll
            for (int k = 0; k <= B; ++k) {
              const int lo = t + k - h < 0 ? 0 : t + k - h;
              double g = 0.0;
              for (int tau = lo; tau <= hi; ++tau) g = __builtin_fma(wz[i][h + t - tau], wz[i][h + t + k - tau], g);
              acc = __builtin_fma(k == 0 ? 1.0 : 2.0, Zn[k] * g, acc);
            }
          }
          tr[i].add(acc);
        }
#pragma unroll
      for (int r = BB - 1; r > 0; --r)
#pragma unroll
        for (int j = 0; j <= B; ++j) Zw[r][j] = Zw[r - 1][j];
#pragma unroll
      for (int j = 0; j <= B; ++j) Zw[0][j] = Zn[j];
    }
  }
  const double pv = m2c / (double)T, ov = m2o / (double)T, diff = pv - ov;
  const double gs = 4.0 / (double)T * diff / gvv;

  // ---- sweep 3: y = L^-1 g, y / d over 1 / d ----
  {
    double q[BB];
#pragma unroll
    for (int a = 0; a < BB; ++a) q[a] = 0.0;
    for (int t = 0; t < T; ++t) {
      double* wr = wc + (fb + t) * row;
      double y = gs * (((double)obs[(fb + t) * ld] + wr[0]) - mc);
      if (B > 0) y += q[0];
#pragma unroll
      for (int a = 1; a <= B; ++a) q[a - 1] = __builtin_fma(-wr[(int64_t)a * dim], y, a < B ? q[a < B ? a : 0] : 0.0);
      wr[(int64_t)(B + 1) * dim] *= y;
    }
  }

  // ---- sweep 4: s = A^-1 g and, h_i frames behind it, row tau = t + h_i of every W_i on x, o and s ----
  // W_i e = -W_i x, and the residual mu_i - W_i c = (mu_i - W_i o) + W_i e, again by way of the exact difference.
  const double inv_dt = 1.0 / ((double)m.D * (double)T), gv_2d = m.gv_weight / (2.0 * (double)m.D);
  TrjSum mah, dpt[kWinMaxWin];
  double dpg[kWinMaxWin];
#pragma unroll
  for (int i = 0; i < kWinMaxWin; ++i) dpg[i] = 0.0;
  {
    double sw[B + 1], xw[B + 1], ow[B + 1];                              // s, x, o at t + j
#pragma unroll
    for (int j = 0; j <= B; ++j) sw[j] = xw[j] = ow[j] = 0.0;
    for (int t = T - 1; t >= -hmax; --t) {
      double sv = 0.0, xv = 0.0, ov_ = 0.0;
      if (t >= 0) {
        const double* wr = wc + (fb + t) * row;
        sv = wr[(int64_t)(B + 1) * dim];
#pragma unroll
        for (int a = 1; a <= B; ++a) sv = __builtin_fma(-wr[(int64_t)a * dim], sw[a - 1], sv);   // sw[a - 1] is still s[t + a]
        xv = wr[0];
        ov_ = (double)obs[(fb + t) * ld];
      }
#pragma unroll
      for (int j = B; j > 0; --j) {
        sw[j] = sw[j - 1];
        xw[j] = xw[j - 1];
        ow[j] = ow[j - 1];
      }
      sw[0] = sv;
      xw[0] = xv;
      ow[0] = ov_;
#pragma unroll
      for (int i = 0; i < kWinMaxWin; ++i)
        if (i < nwin) {
          const int tau = t + ((m.t.win.wsize[s][i] - 1) >> 1);
          if (tau >= 0 && tau <= T - 1) {
            double yx = 0.0, yo = 0.0, ys = 0.0;
#pragma unroll
            for (int k = 0; k <= B; ++k) {                               // zeros beyond the window's 2 h + 1 taps
              const double wk = wz[i][k];
              yx = __builtin_fma(wk, xw[k], yx);
              yo = __builtin_fma(wk, ow[k], yo);
              ys = __builtin_fma(wk, sw[k], ys);
            }
            const double ye = -yx, r = ((double)pred[(fb + tau) * ld + i * dim] - yo) + ye;
            mah.add(pw[i] * ye * ye);
            dpt[i].add(ye * (ye - 2.0 * r));
            dpg[i] = __builtin_fma(ys, r, dpg[i]);
            if (grad != nullptr) grad[(fb + tau) * ldg + i * dim] = (float)(pw[i] * (gv_2d * ys - inv_dt * ye));
          }
        }
    }
  }

  double* tp = tab + ((int64_t)u * m.D + m.col0[s] + col) * kTrjTerms;
  tp[0] = logdet.get();
  tp[1] = mah.get();
  tp[2] = diff * diff / gvv;
  tp[3] = log(gvv);
  if (grad_var != nullptr) {
    double* gp = grad_var + (int64_t)u * m.width + m.var0[s] + col;
#pragma unroll
    for (int i = 0; i < kWinMaxWin; ++i)
      if (i < nwin) gp[i * dim] = -pw[i] * pw[i] * (0.5 * inv_dt * (dpt[i].get() - tr[i].get()) + gv_2d * dpg[i]);
  }
}

// One block per utterance: the voicing term, the sums of the column table in column order, the three costs; a flagged
// utterance's costs and gradients become zeros.  Every sum is taken in an order that T and the streams alone decide.
struct TrjReduceMeta {
  int n_streams, D, M, width;
  double msd_weight;
  int dim[kWinMaxStreams], nwin[kWinMaxStreams], var0[kWinMaxStreams];
  const float* msd_pred[kWinMaxStreams];         // null: the stream has no voicing column
  const float* msd_obs[kWinMaxStreams];
  const float* msd_var[kWinMaxStreams];
  float* grad[kWinMaxStreams];                   // or null
  float* grad_msd[kWinMaxStreams];               // or null
  int64_t ld, ld_grad;
};

__global__ __launch_bounds__(64) void trj_reduce_kernel(TrjReduceMeta m, const int64_t* __restrict__ f_off,
                                                        const double* __restrict__ tab, int* __restrict__ status,
                                                        double* __restrict__ cost, double* __restrict__ grad_var) {
  const int u = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int64_t fb = f_off[u];
  const int T = (int)(f_off[u + 1] - fb);
  __shared__ double red[64];
  __shared__ double sq[kWinMaxStreams], sums[kTrjTerms];
  __shared__ int flag;
  const float inf = __builtin_inff();
  if (lane == 0) flag = T > 0 ? status[u] : 0;
  __syncthreads();
  bool bad = false;
  for (int s = 0; s < m.n_streams; ++s) {
    if (m.msd_pred[s] == nullptr) continue;                              // the same in every lane
    const float v = m.msd_var[s][0];
    bad |= T > 0 && !(v > 0.0f && v < inf);
    double a = 0.0;
    for (int t = lane; t < T; t += 64) {
      const float p = m.msd_pred[s][(fb + t) * m.ld], o = m.msd_obs[s][(fb + t) * m.ld];
      bad |= !(fabsf(p) < inf && fabsf(o) < inf);
      const double d = (double)p - (double)o;
      a = __builtin_fma(d, d, a);
    }
    red[lane] = a;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
      if (lane < w) red[lane] += red[lane + w];
      __syncthreads();
    }
    if (lane == 0) sq[s] = red[0];
    __syncthreads();
  }
  if (bad) atomicOr(&flag, 1);
  __syncthreads();
  const bool flagged = flag != 0;
  if (lane == 0 && T > 0) status[u] = flag;
  if (flagged || T <= 0) {
    if (lane < 3) cost[(int64_t)u * 3 + lane] = 0.0;
    if (grad_var != nullptr)
      for (int k = lane; k < m.width; k += 64) grad_var[(int64_t)u * m.width + k] = 0.0;
    for (int s = 0; s < m.n_streams; ++s) {
      const int cols = m.dim[s] * m.nwin[s];
      if (m.grad[s] != nullptr)
        for (int64_t e = lane; e < (int64_t)T * cols; e += 64) m.grad[s][(fb + e / cols) * m.ld_grad + e % cols] = 0.0f;
      if (m.grad_msd[s] != nullptr && m.msd_pred[s] != nullptr)
        for (int t = lane; t < T; t += 64) m.grad_msd[s][(fb + t) * m.ld_grad] = 0.0f;
    }
    return;
  }
  if (lane < kTrjTerms) {
    double a = 0.0;
    const double* tp = tab + (int64_t)u * m.D * kTrjTerms + lane;
    for (int d = 0; d < m.D; ++d) a += tp[(int64_t)d * kTrjTerms];
    sums[lane] = a;
  }
  __syncthreads();
  const double dT = (double)T, dD = (double)m.D, dM = (double)m.M;
  double lnvar = 0.0, mahal = 0.0;
  for (int s = 0; s < m.n_streams; ++s) {
    if (m.msd_pred[s] == nullptr) continue;
    const double v = (double)m.msd_var[s][0];
    lnvar += log(v);
    mahal += sq[s] / v;
    const double gp = m.msd_weight / (v * dM * dT);
    if (m.grad_msd[s] != nullptr)
      for (int t = lane; t < T; t += 64)
        m.grad_msd[s][(fb + t) * m.ld_grad] =
            (float)(gp * ((double)m.msd_pred[s][(fb + t) * m.ld] - (double)m.msd_obs[s][(fb + t) * m.ld]));
    if (grad_var != nullptr && lane == 0)
      grad_var[(int64_t)u * m.width + m.var0[s] - 1] = m.msd_weight * (dT / v - sq[s] / (v * v)) / (2.0 * dM * dT);
  }
  if (lane == 0) {
    cost[(int64_t)u * 3 + 0] = (dD * dT * kLn2Pi - sums[0] + sums[1]) / (2.0 * dD * dT);
    cost[(int64_t)u * 3 + 1] = m.M > 0 ? (dM * dT * kLn2Pi + dT * lnvar + mahal) / (2.0 * dM * dT) : 0.0;
    cost[(int64_t)u * 3 + 2] = (dD * kLn2Pi + sums[3] + sums[2]) / (2.0 * dD);
  }
}

// What WorldMi355TrajectoryCost refuses, on the host alone: no device call is made for a refused argument set.
int check_trj(int n_streams, const float* const* pred, const float* const* obs, int64_t ld, const float* const* var,
              const float* const* gv_var, const int* dims, const int* n_windows, const double* const* const* windows,
              const int* const* window_sizes, const float* const* msd_pred, const float* const* msd_obs,
              const float* const* msd_var, const WorldMi355TrajectoryOption* opt, const double* cost,
              float* const* grad_pred, float* const* grad_msd, int64_t ld_grad) {
  if (!pred || !obs || !var || !gv_var || !opt || !cost) return WM_ERR_BAD_ARG;
  if (const int rc = check_windows(n_streams, dims, n_windows, windows, window_sizes, kWinMaxStreams, kWinMaxWin, kTrjMaxTaps))
    return rc;
  if (opt->edge != 0 || !(opt->msd_weight == opt->msd_weight) || !(opt->gv_weight == opt->gv_weight)) return WM_ERR_BAD_ARG;
  if (msd_pred != nullptr && (!msd_obs || !msd_var)) return WM_ERR_BAD_ARG;
  for (int s = 0; s < n_streams; ++s) {
    if (!pred[s] || !obs[s] || !var[s] || !gv_var[s]) return WM_ERR_BAD_ARG;
    const int64_t row = (int64_t)dims[s] * n_windows[s];
    if (ld < row || (grad_pred != nullptr && !grad_pred[s])) return WM_ERR_BAD_ARG;
    if ((grad_pred != nullptr || grad_msd != nullptr) && ld_grad < row) return WM_ERR_BAD_ARG;
    if (msd_pred != nullptr && msd_pred[s] != nullptr && (!msd_obs[s] || !msd_var[s])) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

struct TrjWs : StageWs {
  double* d = nullptr;
  int* status = nullptr;
  int64_t cap = 0, cap_utt = 0;     // in doubles; in utterances
};

int launch_trj(Batch& b, hipStream_t st, int n_streams, const float* const* pred, const float* const* obs, int64_t ld,
               const float* const* var, const float* const* gv_var, const int* dims, const int* n_windows,
               const double* const* const* windows, const int* const* window_sizes, const float* const* msd_pred,
               const float* const* msd_obs, const float* const* msd_var, const WorldMi355TrajectoryOption& opt,
               double* cost, float* const* c, float* const* grad_pred, float* const* grad_msd, int64_t ld_grad,
               double* grad_var, int* d_status) {
  if (const int rc = check_trj(n_streams, pred, obs, ld, var, gv_var, dims, n_windows, windows, window_sizes, msd_pred,
                               msd_obs, msd_var, &opt, cost, grad_pred, grad_msd, ld_grad))
    return rc;
  if (b.total_f <= 0 || b.n_utt <= 0) return WM_OK;
  BandPlan plan;
  if (const int rc = band_plan(plan, n_streams, dims, n_windows, window_sizes, b.total_f, b.n_utt,
                               [](int B) { return B + 2; }))
    return rc;
  int col0[kWinMaxStreams], var0[kWinMaxStreams], D = 0, M = 0, width = 0;
  int64_t need = plan.need;
  for (int s = 0; s < n_streams; ++s) {
    const bool has_msd = msd_pred != nullptr && msd_pred[s] != nullptr;
    col0[s] = D;
    var0[s] = width + (has_msd ? 1 : 0);
    if ((int64_t)D + dims[s] > (int64_t)1 << 24) return WM_ERR_BAD_ARG;
    D += dims[s];
    M += has_msd ? 1 : 0;
    width = var0[s] + dims[s] * n_windows[s];
  }
  const int64_t tab_off = need;
  need += (int64_t)b.n_utt * D * kTrjTerms;
  TrjWs* W = nullptr;
  if (const int rc = grow_ws(b.trj, st, W, [&](const TrjWs& w) { return w.cap >= need && w.cap_utt >= b.n_utt; },
                             [&](TrjWs& n) {
                               n.cap = need;
                               n.cap_utt = b.n_utt;
                               if (const int rc = wm_check(n.alloc(&n.d, sizeof(double) * (size_t)need))) return rc;
                               return wm_check(n.alloc(&n.status, sizeof(int) * (size_t)b.n_utt));
                             }))
    return rc;
  if (d_status == nullptr) d_status = W->status;
  if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st))) return rc;
  TimedScope ts_(b.ctx, st, "trj_kernel");
  for (int g = 0; g < 3; ++g) {                          // five taps: no stream has the widest band
    TrjMeta m;
    memset(&m, 0, sizeof(m));
    m.D = D;
    m.width = width;
    m.gv_weight = opt.gv_weight;
    m.ld = ld;
    m.ld_grad = ld_grad;
    int src[kWinMaxStreams];
    const int blocks = band_group(m.t, src, plan, kBands[g], n_streams, dims, n_windows, windows, window_sizes, b.n_utt);
    if (m.t.n_streams == 0) continue;
    for (int k = 0; k < m.t.n_streams; ++k) {
      const int s = src[k];
      m.col0[k] = col0[s];
      m.var0[k] = var0[s];
      m.pred[k] = pred[s];
      m.obs[k] = obs[s];
      m.var[k] = var[s];
      m.gv_var[k] = gv_var[s];
      m.c[k] = c != nullptr ? c[s] : nullptr;
      m.grad[k] = grad_pred != nullptr ? grad_pred[s] : nullptr;
    }
    double* tab = W->d + tab_off;
    switch (kBands[g]) {
      case 0: hipLaunchKernelGGL((trj_kernel<0>), dim3(blocks), dim3(64), 0, st, m, b.d_f_off, W->d, tab, grad_var, d_status); break;
      case 2: hipLaunchKernelGGL((trj_kernel<2>), dim3(blocks), dim3(64), 0, st, m, b.d_f_off, W->d, tab, grad_var, d_status); break;
      default: hipLaunchKernelGGL((trj_kernel<4>), dim3(blocks), dim3(64), 0, st, m, b.d_f_off, W->d, tab, grad_var, d_status); break;
    }
  }
  TrjReduceMeta r;
  memset(&r, 0, sizeof(r));
  r.n_streams = n_streams;
  r.D = D;
  r.M = M;
  r.width = width;
  r.msd_weight = opt.msd_weight;
  r.ld = ld;
  r.ld_grad = ld_grad;
  for (int s = 0; s < n_streams; ++s) {
    r.dim[s] = dims[s];
    r.nwin[s] = n_windows[s];
    r.var0[s] = var0[s];
    const bool has_msd = msd_pred != nullptr && msd_pred[s] != nullptr;
    r.msd_pred[s] = has_msd ? msd_pred[s] : nullptr;
    r.msd_obs[s] = has_msd ? msd_obs[s] : nullptr;
    r.msd_var[s] = has_msd ? msd_var[s] : nullptr;
    r.grad[s] = grad_pred != nullptr ? grad_pred[s] : nullptr;
    r.grad_msd[s] = grad_msd != nullptr ? grad_msd[s] : nullptr;
  }
  hipLaunchKernelGGL(trj_reduce_kernel, dim3(b.n_utt), dim3(64), 0, st, r, b.d_f_off, W->d + tab_off, d_status, cost,
                     grad_var);
  return wm_check(hipGetLastError());
}

}  // namespace wm
