// mcep.hip -- mel-cepstral analysis of spectra on the device (the encoder half).
//
// Restates the CLIs' SPTK port: mcep (test/sptkfunctions.cpp:11-184) with flng = fft_size and its Toeplitz-plus-Hankel
// solver theq (test/theq.cpp:286-357).  One 64-lane workgroup per frame, persistent over the batch's frames:
//
//   periodogram x[k] from the row (:85-94), kept in LDS: every Newton step reads it again;
//   everything from :119 on -- the initial estimate, the Newton steps and theq -- is mcep_newton (mcep_newton.hpp),
//     shared with the kernel that starts from windowed frames or waveforms (mgcep.hip).
#include <math.h>

#include "batch.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "fft.hpp"
#include "mcep_newton.hpp"

namespace wm {

template <int F>
__global__ __launch_bounds__(64) void mcep_kernel(const double* __restrict__ spec, McepArgs o, int64_t total_frames,
                                                  double* __restrict__ mc_out, int* __restrict__ status) {
  constexpr int N = F / 2, M = N / 64, BINS = N + 1;
  __shared__ __attribute__((aligned(16))) cpx img[FftLds<N>::kElems];
  __shared__ double per[BINS + 1];
  const int lane0 = threadIdx.x;
  FftTw<N> tw;
  tw.init(lane0);
  const int m = o.m, n = m + 1;
  double al = 1.0;                                     // 1, (-a), (-a)^2, ... by the reference's recurrence (:129-131)
  for (int i = 1; i < 64; ++i) {
    const double nx = -o.alpha * al;
    al = i <= lane0 ? nx : al;
  }
  const double nb = 1 - (-o.alpha) * (-o.alpha);       // freqt's b for -a
  for (int64_t frame = blockIdx.x; frame < total_frames; frame += gridDim.x) {
    const int lane = opaque_lane(lane0);
    const double* row = spec + frame * (int64_t)BINS;
    wave_sync();
    bool bad = false;
    {
      double rv[M + 1];
#pragma unroll
      for (int q = 0; q <= M; ++q) rv[q] = row[imin(lane + 64 * q, BINS - 1)];
#pragma unroll
      for (int q = 0; q <= M; ++q) {
        const double x = o.square ? rv[q] * rv[q] + o.eps : rv[q] + o.eps;       // :85-94
        bad = bad || !(x > 0.0 && x < __builtin_inf());
        if (q < M || lane == 0) per[lane + 64 * q] = x;
      }
    }
    double mcv = 0.0;
    int st = 2;                                        // a periodogram value <= 0 (:119-124) or not finite
    if (__ballot(bad) == 0ull) mcep_newton<F>(per, img, tw, o, al, nb, lane, mcv, st);
    if (lane <= m) mc_out[frame * (int64_t)n + lane] = mcv;
    if (status != nullptr && lane == 0) status[frame] = st;
  }
}

// What WorldMi355MelCepstrum refuses, on the host alone: no device call is made for a refused option set.
int check_mel_cepstrum(const Batch& b, const double* d_spec, const WorldMi355McepOption& opt, const double* d_mc) {
  const int F = b.p.fft_size;
  if (F != 512 && F != 1024 && F != 2048 && F != 4096) return WM_ERR_UNSUPPORTED_FFT;
  if (!d_spec || !d_mc) return WM_ERR_BAD_ARG;
  if (opt.order < 1 || opt.order > 63 || opt.itr1 < 0 || opt.itr2 < 0 || opt.itr2 > 1000) return WM_ERR_BAD_ARG;
  if (!(fabs(opt.alpha) < 1.0) || opt.dd != opt.dd || opt.f != opt.f) return WM_ERR_BAD_ARG;
  if (opt.etype != 0 && opt.etype != 1) return opt.etype == 2 ? WM_ERR_UNSUPPORTED : WM_ERR_BAD_ARG;
  if (opt.etype == 1 && !(opt.e >= 0.0)) return WM_ERR_BAD_ARG;                   // :21-24
  if (opt.itype != 3 && opt.itype != 4) return opt.itype >= 0 && opt.itype <= 2 ? WM_ERR_UNSUPPORTED : WM_ERR_BAD_ARG;
  return WM_OK;
}

int launch_mel_cepstrum(Batch& b, hipStream_t st, const double* d_spec, const WorldMi355McepOption& opt, double* d_mc,
                        int* d_status) {
  if (const int rc = check_mel_cepstrum(b, d_spec, opt, d_mc)) return rc;
  const int F = b.p.fft_size;
  const int64_t tf = b.total_f;
  if (tf <= 0) return WM_OK;
  McepArgs a;
  a.alpha = opt.alpha;
  a.dd = opt.dd;
  a.eps = opt.etype == 1 ? opt.e : 0.0;
  a.f = opt.f < 0.0 ? 1.0e-6 : opt.f;                                             // theq.cpp:319-320
  a.m = opt.order;
  a.itr1 = opt.itr1;
  a.itr2 = opt.itr2;
  a.square = opt.itype == 3 ? 1 : 0;
  TimedScope ts_(b.ctx, st, "mcep_kernel");
#define WM_MCEP_CASE(FF)                                                                                 \
  case FF: {                                                                                             \
    const int per_ = persistent_grid(*b.ctx, mcep_kernel<FF>, 64, (int64_t)1 << 40);                     \
    hipLaunchKernelGGL((mcep_kernel<FF>), dim3((int)(tf < per_ ? tf : per_)), dim3(64), 0, st, d_spec, a, tf, d_mc, \
                       d_status);                                                                        \
  } break;
  switch (F) {
    WM_MCEP_CASE(512)
    WM_MCEP_CASE(1024)
    WM_MCEP_CASE(2048)
    WM_MCEP_CASE(4096)
  }
#undef WM_MCEP_CASE
  return wm_check(hipGetLastError());
}

}  // namespace wm
