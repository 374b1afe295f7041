// mgc2sp.hip -- spectra from mel-generalized cepstra on the device (the decoder half).
//
// Restates the CLIs' SPTK port: mgc2sp(mgc, m, a, g, x, y, flng = fft_size) (test/sptkfunctions.cpp:186-219), i.e.
// mgc2mgc(mgc, m, a, g, c, F/2, 0, 0) (:221-254) and c2sp (:256-274).  One 64-lane workgroup per frame, persistent over
// the batch's frames:
//
//   a != 0 (:245-250): freqt from m to F/2 coefficients with warp -a (freqt.hpp: the reference's expressions in its
//     order, lane per input coefficient), gnorm with g over all F/2 coefficients, gc2gc(c, F/2, g, c, F/2, 0), ignorm
//     with 0;
//   a == 0 (:240-244): the row itself, gnorm over m, gc2gc(ca, m, g, c, F/2, 0), ignorm;
//   g == 0 in either branch: gc2gc's sums are multiplied by 0 and the chain is c0 -> log(exp(c0)); it is skipped;
//   c2sp: zero-padded to F, one real forward transform, bins 0 .. F/2: x = Re (ln |H|), y = Im (fftr's sign is the
//     forward transform's, tests/golden/sptk_mgc2sp_full.npz: y_sign).
//
// gc2gc towards gamma 0 (:347-385, g2 = 0: ss2 is never needed) is the triangular recurrence
//   c2[i] = ca[i] - g / i * sum_{j = 1}^{i - 1} j c2[j] ca[i - j],     ca[k] = 0 beyond m1,
// F/2 sequential outputs whose sums grow to F/2 terms.  It runs right-looking, with no cross-lane reduction: with
// u[j] = j c2[j] the recurrence is u[i] = i ca[i] - g sum_j u[j] ca[i - j], free of the division.  Lane l owns the outputs
// i = 64 r + l + 1 and keeps their partial sums in registers; once u[j] is final it is broadcast (v_readlane) and every
// later output adds its u[j] ca[i - j] by one fused multiply-add, ca read from LDS at a distance that moves one element
// per step (64 zeros in front of ca[1] stand for i - j <= 0, so no lane is masked).  The sums of the block that is being
// finished are register 0; after its 64 steps the registers move down one.  c2[i] = u[i] / i is one division per output.
// The sums run in ascending j with fused products where the reference runs descending with three roundings per
// term: the results differ from the reference's by its own rounding error, which the fixture measures (sens, figure
// (b) of tools/gen_golden_mgc2sp.py).  With a == 0 only ca[1 .. m] is non-zero: two registers per step instead of up to
// F/128.
#include <math.h>

#include "batch.hpp"
#include "common.hpp"
#include "fft.hpp"
#include "freqt.hpp"

namespace wm {

struct Mgc2spArgs {
  double alpha, gamma;
  int m, fmt;                  // fmt: 0 ln |H|, 3 |H|, 4 |H|^2 (WorldMi355Mgc2spOption.out_format)
};

template <int F>
__global__ __launch_bounds__(64) void mgc2sp_kernel(const double* __restrict__ mc, Mgc2spArgs o, int64_t total_frames,
                                                    double* __restrict__ sp, double* __restrict__ ph,
                                                    int* __restrict__ status) {
  constexpr int N = F / 2, M = N / 64, BINS = N + 1;
  // the cepstrum lives in the FFT image until the transform's registers have taken it
  __shared__ __attribute__((aligned(16))) cpx img[FftLds<N>::kElems];
  __shared__ double caz[64 + N + 1];                   // 64 zeros and a zero for ca[0], then ca[1 .. F/2]
  static_assert(2 * FftLds<N>::kElems >= N + 2 + 64, "a cepstrum and freqt's 64 dummy slots fit the image");
  double* cep = reinterpret_cast<double*>(img);
  const int lane0 = threadIdx.x;
  FftTw<N> tw;
  tw.init(lane0);
  const int m = o.m;
  const double g = o.gamma;
  const double nb = 1 - (-o.alpha) * (-o.alpha);       // freqt's b for -a
  const int m1 = o.alpha == 0.0 ? m : N;               // gc2gc's input order (:243, :248)
  const int dlim = imin((m1 + 63) / 64 + 1, M);        // registers a step can reach: i - j <= m1
  for (int64_t frame = blockIdx.x; frame < total_frames; frame += gridDim.x) {
    const int lane = opaque_lane(lane0);
    wave_sync();
    // lane s feeds coefficient m - s (freqt walks c1[m] .. c1[0])
    const double cin = lane <= m ? mc[frame * (int64_t)(m + 1) + (m - lane)] : 0.0;
    bool ok = __ballot(!(fabs(cin) < __builtin_inf())) == 0ull;
    if (ok) {
      if (o.alpha != 0.0) {
        freqt_expand<64>(cin, lane, m, N, -o.alpha, nb, lane == m, cep, cep + (N + 2) + lane);   // :246
      } else {
#pragma unroll
        for (int q = 0; q <= M; ++q)
          if (lane + 64 * q <= N) cep[lane + 64 * q] = 0.0;
        wave_sync();
        if (lane <= m) cep[m - lane] = cin;                                                      // :241
      }
      wave_sync();
      const double c0 = uniform_d(cep[0]);
      if (g == 0.0) {
        if (lane == 0) cep[0] = log(exp(c0));                                                    // gnorm, ignorm at 0
      } else {
        double kk;
        {
#pragma clang fp contract(off)
          kk = 1.0 + g * c0;                                                                     // :318
        }
        ok = __builtin_amdgcn_readfirstlane(kk > 0.0 ? 1 : 0) != 0;                              // the reference's pow: NaN
        if (ok) {
          // gnorm (:319-321) into the zero-prefixed copy
          caz[lane] = 0.0;
          if (lane == 0) caz[64] = 0.0;
#pragma unroll
          for (int q = 0; q < M; ++q) {
            const int k = lane + 64 * q + 1;
            caz[64 + k] = k <= m1 ? cep[k] / kk : 0.0;
          }
          wave_sync();
          if (lane == 0) cep[0] = log(pow(kk, 1.0 / g));                                         // :321, :341
          double acc[M];
#pragma unroll
          for (int d = 0; d < M; ++d) acc[d] = 0.0;
          const double* zp = caz + 64 + lane;
          for (int rj = 0; rj < M; ++rj) {
            const int i_own = 64 * rj + lane + 1;
            const double ica = (double)i_own * caz[64 + i_own];
            const int lim = imin(M - rj, dlim);
            for (int l = 0; l < 64; ++l) {
              // u[j], j = 64 rj + l + 1, is final in lane l: every later output takes its term
              const double uj = readlane_d(__builtin_fma(-g, acc[0], ica), l);
#pragma unroll
              for (int d = 0; d < M; ++d)
                if (d < lim) acc[d] = __builtin_fma(uj, zp[64 * d - l], acc[d]);
            }
            cep[i_own] = __builtin_fma(-g, acc[0], ica) / (double)i_own;
#pragma unroll
            for (int d = 0; d + 1 < M; ++d) acc[d] = acc[d + 1];
            acc[M - 1] = 0.0;
          }
        }
      }
    }
    double* srow = sp + frame * (int64_t)BINS;
    double* prow = ph != nullptr ? ph + frame * (int64_t)BINS : nullptr;
    if (ok) {
      wave_sync();
      cpx v[M];
#pragma unroll
      for (int q = 0; q < M; ++q) {
        const int i0 = 2 * (lane + 64 * q);
        v[q] = make_double2(i0 <= N ? cep[imin(i0, N)] : 0.0, i0 + 1 <= N ? cep[imin(i0 + 1, N)] : 0.0);
      }
      auto put = [&](int k, cpx X) {
        double x = X.x;
        if (o.fmt == 3) x = exp(x);
        else if (o.fmt == 4) x = exp(x + x);
        srow[k] = x;
        if (prow != nullptr) prow[k] = X.y;
      };
      // c2sp (:256-274): c[0 .. F/2] zero-padded to F is M / 2 + 1 packed registers
      rfft_forward_pairs_f<N, M / 2 + 1>(v, img, tw, lane, [&](int q, cpx a, cpx b) {
        if (q < M / 2) {
          const int k = lane + 64 * q;
          put(k, a);
          put(N - k, b);
        } else if (lane == 0) {
          put(N / 2, a);
        }
      });
    } else {
      for (int k = lane; k < BINS; k += 64) {
        srow[k] = 0.0;
        if (prow != nullptr) prow[k] = 0.0;
      }
    }
    if (status != nullptr && lane == 0) status[frame] = ok ? 0 : 1;
  }
}

// What WorldMi355MelCepstrumToSpectrum refuses, on the host alone: no device call is made for a refused option set.
int check_mgc2sp(const Batch& b, const double* d_mc, const WorldMi355Mgc2spOption& opt, const double* d_sp) {
  const int F = b.p.fft_size;
  if (F != 512 && F != 1024 && F != 2048 && F != 4096) return WM_ERR_UNSUPPORTED_FFT;
  if (!d_mc || !d_sp) return WM_ERR_BAD_ARG;
  if (opt.order < 1 || opt.order > 63 || opt.order > F / 2) return WM_ERR_BAD_ARG;
  if (!(fabs(opt.alpha) < 1.0) || !(opt.gamma >= -1.0 && opt.gamma <= 0.0)) return WM_ERR_BAD_ARG;
  if (opt.out_format != 0 && opt.out_format != 3 && opt.out_format != 4) return WM_ERR_UNSUPPORTED;
  return WM_OK;
}

int launch_mgc2sp(Batch& b, hipStream_t st, const double* d_mc, const WorldMi355Mgc2spOption& opt, double* d_sp,
                  double* d_phase, int* d_status) {
  if (const int rc = check_mgc2sp(b, d_mc, opt, d_sp)) return rc;
  const int F = b.p.fft_size;
  const int64_t tf = b.total_f;
  if (tf <= 0) return WM_OK;
  Mgc2spArgs a;
  a.alpha = opt.alpha;
  a.gamma = opt.gamma;
  a.m = opt.order;
  a.fmt = opt.out_format;
  TimedScope ts_(b.ctx, st, "mgc2sp_kernel");
#define WM_MGC2SP_CASE(FF)                                                                               \
  case FF: {                                                                                             \
    const int per_ = persistent_grid(*b.ctx, mgc2sp_kernel<FF>, 64, (int64_t)1 << 40);                   \
    hipLaunchKernelGGL((mgc2sp_kernel<FF>), dim3((int)(tf < per_ ? tf : per_)), dim3(64), 0, st, d_mc, a, tf, d_sp, \
                       d_phase, d_status);                                                               \
  } break;
  switch (F) {
    WM_MGC2SP_CASE(512)
    WM_MGC2SP_CASE(1024)
    WM_MGC2SP_CASE(2048)
    WM_MGC2SP_CASE(4096)
  }
#undef WM_MGC2SP_CASE
  return wm_check(hipGetLastError());
}

}  // namespace wm
