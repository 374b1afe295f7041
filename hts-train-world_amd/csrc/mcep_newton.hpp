// mcep_newton.hpp -- what SPTK's mcep (test/sptkfunctions.cpp:11-184) does once the periodogram stands (:119-177),
// and its solver theq (test/theq.cpp:286-357), on one wavefront: shared by mcep_kernel (mcep.hip: rows of spectra) and
// mgcep_kernel (mgcep.hip: windowed frames and waveforms), which differ only in how they fill the periodogram in LDS.
//
//   c = IFFT[log x] (:119-134): the sequence is real and even, so the inverse real transform takes it by pairs
//     (k, N - k) with zero imaginary parts and only c[0 .. F/2] is kept;
//   mc = freqt(c, F/2 -> m, a) (:136-138), lane per output coefficient (freqt.hpp);
//   up to itr2 Newton steps (:142-177): freqt(mc, m -> F/2, -a), lane per input coefficient; forward real transform,
//     x / exp(2 Re C) and the inverse transform in one pass over the pairs (rfft_filter_pairs: the spectrum never
//     leaves the registers); frqtr(F/2 -> 2 m, a), lane per output, two outputs per lane beyond 64; the stop test
//     exactly where the reference has it; theq over the lanes; mc += d.
//
// theq is a block-Levinson recursion with 2 x 2 pivots over n = m + 1 steps.  Lane j holds x[j], p[j] and the block
// r[j]; what step i needs at lane j from lane i - j are (a) r[i - j], which moves one lane per step (DPP shift, lane 0
// fed by v_readlane), (b) x[i - j] after the step's update, one ds_bpermute gather per step, which shifted by one lane is
// also the xx[i + 1 - j] of the next step.  The inner products ex, ep are masked wave sums (wave_sum4: a tree, not the
// reference's left-to-right order); every 2 x 2 product and inverse is the reference's expression, computed by all
// lanes from the broadcast sums, so the pivots -- and the decision to stop -- are wave-uniform.
#pragma once
#include <math.h>

#include "common.hpp"
#include "fastmath.hpp"
#include "fft.hpp"
#include "freqt.hpp"

namespace wm {

struct McepArgs {
  double alpha, dd, eps, f;
  int m, itr1, itr2, square;   // square: the rows are amplitudes (itype 3), else periodograms (itype 4)
};

// inverse() of theq.cpp:90-112; false where the reference returns -1
__device__ __forceinline__ bool theq_inverse(double y0, double y1, double y2, double y3, double eps, double& x0,
                                             double& x1, double& x2, double& x3) {
#pragma clang fp contract(off)
  const double det = y0 * y3 - y1 * y2;
  x0 = y3 / det;
  x1 = -y1 / det;
  x2 = -y2 / det;
  x3 = y0 / det;
  return !(fabs(det) < eps || det != det);
}

// theq(t, h, a, b, n, eps): lane j < n holds t[j], h1 = h[n - 1 + j], h2 = h[n - 1 - j] (the block r[j], :323-327) and
// b[j]; the solution a[j] comes back in lane j.  Returns false at a singular pivot (wave-uniform).
__device__ __forceinline__ bool theq_wave(double tj, double h1, double h2, double bj, int n, double eps, int lane,
                                          double& sol) {
#pragma clang fp contract(off)
  const double r00 = readlane_d(tj, 0), r01 = readlane_d(h1, 0), r02 = readlane_d(h2, 0);
  double vx0 = r00, vx1 = r01, vx2 = r02, vx3 = r00;                       // :334-337
  double P0 = 0.0, P1 = 0.0;
  {                                                                        // cal_p0 :142-154
    double i0, i1, i2, i3;
    if (!theq_inverse(r00, r01, r02, r00, eps, i0, i1, i2, i3)) return false;
    const double s0 = readlane_d(bj, 0), s1 = readlane_d(bj, n - 1);
    if (lane == 0) {
      P0 = i0 * s0 + i1 * s1;
      P1 = i2 * s0 + i3 * s1;
    }
  }
  double X0 = lane == 0 ? 1.0 : 0.0, X1 = 0.0, X2 = 0.0, X3 = X0;          // :330
  double Rt = lane == 0 ? tj : 0.0, Rh1 = lane == 0 ? h1 : 0.0, Rh2 = lane == 0 ? h2 : 0.0;   // r[i - j] at step i
  double Q0 = 0.0, Q1 = 0.0, Q2 = 0.0, Q3 = 0.0;                           // x[i - j] after step i
  for (int i = 1; i < n; ++i) {
    {
      const double ti = readlane_d(tj, i), h1i = readlane_d(h1, i), h2i = readlane_d(h2, i);
      Rt = dpp_get<0x138, 0xf, 0xf>(Rt);
      Rh1 = dpp_get<0x138, 0xf, 0xf>(Rh1);
      Rh2 = dpp_get<0x138, 0xf, 0xf>(Rh2);
      if (lane == 0) { Rt = ti; Rh1 = h1i; Rh2 = h2i; }
    }
    const bool act = lane < i;
    // cal_ex :156-177, cal_ep :179-195
    double e0 = act ? Rt * X0 + Rh1 * X2 : 0.0, e1 = act ? Rt * X1 + Rh1 * X3 : 0.0;
    double e2 = act ? Rh2 * X0 + Rt * X2 : 0.0, e3 = act ? Rh2 * X1 + Rt * X3 : 0.0;
    wave_sum4(e0, e1, e2, e3);
    double p0 = act ? Rt * P0 + Rh1 * P1 : 0.0, p1 = act ? Rh2 * P0 + Rt * P1 : 0.0, z0 = 0.0, z1 = 0.0;
    wave_sum4(p0, p1, z0, z1);
    // cal_bx :197-207
    double s0, s1, s2, s3;
    if (!theq_inverse(vx3, vx2, vx1, vx0, eps, s0, s1, s2, s3)) return false;
    const double bx0 = s0 * e0 + s1 * e2, bx1 = s0 * e1 + s1 * e3, bx2 = s2 * e0 + s3 * e2, bx3 = s2 * e1 + s3 * e3;
    // cal_x :209-236: x[j] -= crstrns(xx[i - j]) bx for 0 < j < i, x[i] = -bx
    Q0 = dpp_get<0x138, 0xf, 0xf>(Q0);
    Q1 = dpp_get<0x138, 0xf, 0xf>(Q1);
    Q2 = dpp_get<0x138, 0xf, 0xf>(Q2);
    Q3 = dpp_get<0x138, 0xf, 0xf>(Q3);
    {
      const double d0 = Q3 * bx0 + Q2 * bx2, d1 = Q3 * bx1 + Q2 * bx3, d2 = Q1 * bx0 + Q0 * bx2, d3 = Q1 * bx1 + Q0 * bx3;
      const bool upd = lane >= 1 && lane < i;
      X0 = lane == i ? -bx0 : (upd ? X0 - d0 : X0);
      X1 = lane == i ? -bx1 : (upd ? X1 - d1 : X1);
      X2 = lane == i ? -bx2 : (upd ? X2 - d2 : X2);
      X3 = lane == i ? -bx3 : (upd ? X3 - d3 : X3);
    }
    // cal_vx :238-250
    vx0 -= e3 * bx0 + e2 * bx2;
    vx1 -= e3 * bx1 + e2 * bx3;
    vx2 -= e1 * bx0 + e0 * bx2;
    vx3 -= e1 * bx1 + e0 * bx3;
    // cal_g :252-266
    const double t0 = readlane_d(bj, i) - p0, t1 = readlane_d(bj, n - 1 - i) - p1;
    double u0, u1, u2, u3;
    if (!theq_inverse(vx3, vx2, vx1, vx0, eps, u0, u1, u2, u3)) return false;
    const double g0 = u0 * t0 + u1 * t1, g1 = u2 * t0 + u3 * t1;
    // cal_p :268-284: p[j] += crstrns(x[i - j]) g for j < i, p[i] = g
    const int from = (i - lane) & 63;
    Q0 = __shfl(X0, from, 64);
    Q1 = __shfl(X1, from, 64);
    Q2 = __shfl(X2, from, 64);
    Q3 = __shfl(X3, from, 64);
    {
      const double a0 = Q3 * g0 + Q2 * g1, a1 = Q1 * g0 + Q0 * g1;
      P0 = lane == i ? g0 : (act ? P0 + a0 : P0);
      P1 = lane == i ? g1 : (act ? P1 + a1 : P1);
    }
  }
  sol = P0;                                                                // :353-354
  return true;
}

// The frame's analysis from its periodogram per[0 .. F/2] (LDS, every value positive and finite): mc[lane], lane <= m, in
// `mcv` (0 in the other lanes) and mcep's return in `st` (0 / -1; 1 where theq met a singular pivot, mcv then the last
// iterate).  img is the FFT image: the cepstra between the stages live in it, each consumed into registers before a
// transform writes it.  al = (-a)^lane, nb = freqt's b for -a.  The loop count is wave-uniform (one frame per wave).
template <int F>
__device__ __forceinline__ void mcep_newton(const double* per, cpx* img, const FftTw<F / 2>& tw, const McepArgs& o, double al,
                                            double nb, int lane, double& mcv, int& st) {
  constexpr int N = F / 2, M = N / 64;
  static_assert(2 * FftLds<N>::kElems >= N + 2 + 64, "a cepstrum and freqt's 64 dummy slots fit the image");
  double* cep = reinterpret_cast<double*>(img);
  const int m = o.m, n = m + 1;
  wave_sync();
  cpx v[M];
  // c = IFFT[log x] / F
  rfft_backward_pairs_f<N>([&](int q, cpx& a, cpx& b) {
    if (q < M / 2) {
      const int k = lane + 64 * q;
      a = make_double2(wm_log(per[k]) / F, 0.0);
      b = make_double2(wm_log(per[N - k]) / F, 0.0);
    } else {
      a = make_double2(wm_log(per[N / 2]) / F, 0.0);
      b = a;
    }
  }, v, img, tw, lane);
  wave_sync();
#pragma unroll
  for (int q = 0; q <= M / 2; ++q) {
    const int i0 = 2 * (lane + 64 * q);
    if (i0 <= N) cep[i0] = (i0 == 0 || i0 == N) ? v[q].x * 0.5 : v[q].x;      // :136-137
    if (i0 + 1 <= N) cep[i0 + 1] = v[q].y;
  }
  wave_sync();
  double s = uniform_d(cep[0]);
  {
    double unused;
    freqt_contract<0, false>(cep, N, m, o.alpha, lane, mcv, unused);         // :138
  }
  mcv = lane <= m ? mcv : 0.0;
  st = -1;
  for (int it = 1; it <= o.itr2; ++it) {
    wave_sync();
    double cin = __shfl(mcv, (m - lane) & 63, 64);
    cin = lane <= m ? cin : 0.0;
    freqt_expand<64>(cin, lane, m, N, -o.alpha, nb, lane == m, cep, cep + (N + 2) + lane);   // :144
    wave_sync();
#pragma unroll
    for (int q = 0; q < M; ++q) {
      const int i0 = 2 * (lane + 64 * q);
      v[q] = make_double2(i0 <= N ? cep[imin(i0, N)] : 0.0, i0 + 1 <= N ? cep[imin(i0 + 1, N)] : 0.0);
    }
    // c = IFFT[x / exp(2 Re FFT[c])] / F (:145-148)
    rfft_filter_pairs<N>(v, img, tw, lane, M / 2 + 1, [&](int q, cpx& xk, cpx& xr) {
      if (q < M / 2) {
        const int k = lane + 64 * q;
        xk = make_double2(per[k] / wm_exp(xk.x + xk.x) / F, 0.0);
        xr = make_double2(per[N - k] / wm_exp(xr.x + xr.x) / F, 0.0);
      } else {
        xk = make_double2(per[N / 2] / wm_exp(xk.x + xk.x) / F, 0.0);
        xr = xk;
      }
    });
    wave_sync();
#pragma unroll
    for (int q = 0; q <= M / 2; ++q) {
      const int i0 = 2 * (lane + 64 * q);
      if (i0 <= N) cep[i0] = v[q].x;
      if (i0 + 1 <= N) cep[i0 + 1] = v[q].y;
    }
    wave_sync();
    double r1, r2;                                                           // r(k), k = lane and 64 + lane (:149)
    if (2 * m + 1 > 64) freqt_contract<1, true>(cep, N, 2 * m, o.alpha, lane, r1, r2);
    else freqt_contract<1, false>(cep, N, 2 * m, o.alpha, lane, r1, r2);
    const double t = readlane_d(r1, 0);
    if (it >= o.itr1) {                                                      // :151-158
      if (__builtin_amdgcn_readfirstlane(fabs((t - s) / t) < o.dd ? 1 : 0)) {
        st = 0;
        break;
      }
      s = t;
    }
    // :160-168
    const bool even = (lane & 1) == 0;
    const double bj = r1 - al;
    const double y1 = even ? r1 - t : r1, y2 = even ? r2 - t : r2;
    double tj = (even && lane >= 2) ? r1 + t : r1;
    tj = lane == 0 ? t + t : tj;
    wave_sync();
    cep[lane] = y1;
    cep[64 + lane] = y2;
    wave_sync();
    const double h1 = cep[imin(n - 1 + lane, 127)], h2 = cep[imax(n - 1 - lane, 0)];
    double d;
    const bool ok = theq_wave(tj, h1, h2, bj, n, o.f, lane, d);              // :170
    if (!__builtin_amdgcn_readfirstlane(ok ? 1 : 0)) {
      st = 1;
      break;
    }
    mcv = lane <= m ? mcv + d : 0.0;                                         // :175-176
  }
}

}  // namespace wm
