// mgcep.hip -- mel-cepstra from windowed frames and from waveforms: the recipe line that starts at a waveform
// (data/Makefile.in:134-137),
//
//   x2x +sf raw | frame -l L -p P | window -l L -L F -w type -n norm | mgcep -a alpha -m order -l F -e eps > mgc
//
// at gamma 0, where mgcep is the CLIs' SPTK port mcep (test/sptkfunctions.cpp:11-184) with itype 0, "windowed data
// sequence" (:66-72).  One 64-lane workgroup per frame, persistent over the batch's frames, as mcep_kernel (mcep.hip);
// only the way the periodogram in LDS is filled differs:
//
//   the frame, F real values as N = F / 2 packed complex ones in registers (lane l holds elements l + 64 m):
//     rows mode      a row of F doubles, one 16-byte load per element;
//     waveform mode  gathered from the batch's packed samples -- frame j of an utterance of T samples holds
//                    z[i] = x[j P - L / 2 + i], i < L, zero outside [0, T) -- times the window table (read from global
//                    memory: the same L doubles for every frame), rounded to float32 once where SPTK's pipe between
//                    `window` and `mgcep` is asked for, and F - L zeros.  Lanes read consecutive sample pairs;
//   one forward real transform of F points by the N-point pair machinery (fft.hpp: the spectrum never goes to LDS as
//     complex values), |X|^2 + eps for the bins 0 .. F / 2 into the periodogram the Newton loop reads (:68-71; the
//     reference keeps both halves, which differ by rounding at most);
//   etype 2: the floor max 10^(e / 10) by the reference's own expressions (:104-117), the maximum over the wave;
//   then mcep_newton (mcep_newton.hpp), shared with mcep_kernel.
//
// The periodogram never exists in HBM: a frame costs P new samples of traffic, where a stored periodogram would cost
// 8 (F / 2 + 1) bytes per frame written and read again.
#include <math.h>
#include <string.h>

#include <vector>

#include "batch.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "fft.hpp"
#include "mcep_newton.hpp"

namespace wm {

struct MgcepFront {
  const double* win;              // waveform mode: the window table [L]; rows mode: NULL
  const int64_t *x_off, *f_off;   // waveform mode: the batch's sample and frame offsets, its sample counts and the
  const int* x_len;               //   frame -> utterance map
  const int* frame_utt;
  int L, P, f32;                  // frame length and shift; f32: round the windowed sample to float32
  int floor;                      // etype 2: floor the periodogram at (sqrt(max) floor_amp)^2
  double floor_amp;               // 10^(e / 20)
};

// x[i] * x[i] + y[i] * y[i] + eps (:70), as the reference rounds it
__device__ __forceinline__ double mgcep_power(cpx a, double eps) {
#pragma clang fp contract(off)
  return a.x * a.x + a.y * a.y + eps;
}

template <int F>
__global__ __launch_bounds__(64) void mgcep_kernel(const double* __restrict__ in, MgcepFront fr, McepArgs o,
                                                   int64_t total_frames, double* __restrict__ mc_out,
                                                   int* __restrict__ status) {
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
    wave_sync();
    {
      cpx v[M];
      if (fr.win == nullptr) {
        const double2* row = reinterpret_cast<const double2*>(in + frame * (int64_t)F);
#pragma unroll
        for (int q = 0; q < M; ++q) v[q] = row[lane + 64 * q];
      } else {
        const int u = __builtin_amdgcn_readfirstlane(fr.frame_utt[frame]);
        const int64_t base = fr.x_off[u];
        const int64_t T = fr.x_len[u];
        const int64_t s0 = (frame - fr.f_off[u]) * (int64_t)fr.P - fr.L / 2;      // the sample under the frame's i = 0
#pragma unroll
        for (int q = 0; q < M; ++q) {
          double e[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int i = 2 * (lane + 64 * q) + h;
            const int64_t t = s0 + i;
            const bool live = i < fr.L, inside = live && t >= 0 && t < T;
            const double z = inside ? in[base + t] : 0.0;
            const double w = live ? fr.win[i] : 0.0;
            double p = w * z;
            if (fr.f32) p = (double)(float)p;
            e[h] = live ? p : 0.0;
          }
          v[q] = make_double2(e[0], e[1]);
        }
      }
      rfft_forward_pairs_f<N>(v, img, tw, lane, [&](int q, cpx a, cpx b) {
        if (q < M / 2) {
          const int k = lane + 64 * q;                 // lane 0, q = 0: the bins 0 and N
          per[k] = mgcep_power(a, o.eps);
          per[N - k] = mgcep_power(b, o.eps);
        } else if (lane == 0) {
          per[N / 2] = mgcep_power(a, o.eps);
        }
      });
    }
    wave_sync();
    bool bad = false;
    {
      double xv[M + 1];
#pragma unroll
      for (int q = 0; q <= M; ++q) xv[q] = per[imin(lane + 64 * q, BINS - 1)];
      if (fr.floor) {                                  // :104-117
        double mx = 0.0;
#pragma unroll
        for (int q = 0; q <= M; ++q) mx = fmax(mx, xv[q]);
        double mn = sqrt(wave_max(mx)) * fr.floor_amp;
        mn = mn * mn;
#pragma unroll
        for (int q = 0; q <= M; ++q) {
          if (xv[q] < mn) xv[q] = mn;
          if (q < M || lane == 0) per[lane + 64 * q] = xv[q];
        }
      }
#pragma unroll
      for (int q = 0; q <= M; ++q) bad = bad || !(xv[q] > 0.0 && xv[q] < __builtin_inf());
    }
    double mcv = 0.0;
    int st = 2;                                        // a periodogram value <= 0 (:119-124) or not finite
    if (__ballot(bad) == 0ull) mcep_newton<F>(per, img, tw, o, al, nb, lane, mcv, st);
    if (lane <= m) mc_out[frame * (int64_t)n + lane] = mcv;
    if (status != nullptr && lane == 0) status[frame] = st;
  }
}

// frame's count (the rule in include/world_mi355.h): ceil((T + L / 2) / P), nothing for an empty utterance
int sptk_frames(int64_t n_samples, int frame_length, int frame_shift, int64_t* n_frames) {
  if (!n_frames || n_samples < 0 || frame_shift < 1 || frame_shift > frame_length) return WM_ERR_BAD_ARG;
  *n_frames = n_samples == 0 ? 0 : (n_samples + frame_length / 2 + frame_shift - 1) / frame_shift;
  return WM_OK;
}

// window's table in double: Blackman, Hamming, Hanning, rectangular; as it is, or scaled to sum w^2 = 1 or sum w = 1
int sptk_window(int type, int normalize, int length, double* w) {
  if (type == 3 || type == 4) return WM_ERR_UNSUPPORTED;                          // Bartlett, trapezoid
  if (!w || type < 0 || type > 5 || normalize < 0 || normalize > 2 || length < 2) return WM_ERR_BAD_ARG;
  const double a = 2.0 * M_PI / (length - 1);
  for (int i = 0; i < length; ++i) {
    switch (type) {
      case 0: w[i] = 0.42 - 0.5 * cos(a * i) + 0.08 * cos(2.0 * a * i); break;
      case 1: w[i] = 0.54 - 0.46 * cos(a * i); break;
      case 2: w[i] = 0.5 - 0.5 * cos(a * i); break;
      default: w[i] = 1.0;
    }
  }
  if (normalize != 0) {
    double s = 0.0, lost = 0.0;                    // compensated: the sum is good to its last bit whatever the length
    for (int i = 0; i < length; ++i) {
      const double term = (normalize == 1 ? w[i] * w[i] : w[i]) - lost, next = s + term;
      lost = (next - s) - term;
      s = next;
    }
    if (!(s > 0.0)) return WM_ERR_BAD_ARG;         // Hanning of two points: nothing to scale
    const double g = normalize == 1 ? 1.0 / sqrt(s) : 1.0 / s;
    for (int i = 0; i < length; ++i) w[i] *= g;
  }
  return WM_OK;
}

// What both WorldMi355MelCepstrumOf... calls refuse, on the host alone: no device call is made for a refused set.
// window == NULL with frame_length == 0 checks the rows form.
int check_mgcep(const Batch& b, const double* d_in, bool waveform, const double* window, int frame_length,
                int frame_shift, const WorldMi355McepOption& opt, const double* d_mc) {
  const int F = b.p.fft_size;
  if (F != 512 && F != 1024 && F != 2048 && F != 4096) return WM_ERR_UNSUPPORTED_FFT;
  if (!d_in || !d_mc) return WM_ERR_BAD_ARG;
  if (opt.order < 1 || opt.order > 63 || opt.itr1 < 0 || opt.itr2 < 0 || opt.itr2 > 1000) return WM_ERR_BAD_ARG;
  if (!(fabs(opt.alpha) < 1.0) || opt.dd != opt.dd || opt.f != opt.f) return WM_ERR_BAD_ARG;
  if (opt.itype != 0) return WM_ERR_BAD_ARG;
  if (opt.etype < 0 || opt.etype > 2) return WM_ERR_BAD_ARG;
  if (opt.etype == 1 && !(opt.e >= 0.0)) return WM_ERR_BAD_ARG;                   // :21-24
  if (opt.etype == 2 && !(opt.e < 0.0)) return WM_ERR_BAD_ARG;                    // :26-29
  if (!waveform) return WM_OK;
  if (!window || frame_length > F || frame_shift < 1 || frame_shift > frame_length) return WM_ERR_BAD_ARG;
  if (b.total_x <= 0) return WM_ERR_BAD_ARG;                                      // a batch made without x_lengths
  for (int u = 0; u < b.n_utt; ++u) {
    int64_t J = 0;
    if (sptk_frames(b.x_len[u], frame_length, frame_shift, &J) || J != b.f0_len[u]) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

struct MgcepWs : StageWs {
  double* win = nullptr;
  int cap = 0;                                    // in doubles
  std::vector<double> h_win;                      // the table as uploaded: the copy's source lives as long as the batch
};

static int launch_mgcep(Batch& b, hipStream_t st, const double* d_in, const MgcepFront& front,
                        const WorldMi355McepOption& opt, double* d_mc, int* d_status) {
  const int F = b.p.fft_size;
  const int64_t tf = b.total_f;
  McepArgs a;
  a.alpha = opt.alpha;
  a.dd = opt.dd;
  a.eps = opt.etype == 1 ? opt.e : 0.0;
  a.f = opt.f < 0.0 ? 1.0e-6 : opt.f;                                             // theq.cpp:319-320
  a.m = opt.order;
  a.itr1 = opt.itr1;
  a.itr2 = opt.itr2;
  a.square = 0;
  MgcepFront fr = front;
  fr.floor = opt.etype == 2 ? 1 : 0;
  fr.floor_amp = opt.etype == 2 ? pow(10.0, opt.e / 20.0) : 0.0;                  // :111
  TimedScope ts_(b.ctx, st, "mgcep_kernel");
#define WM_MGCEP_CASE(FF)                                                                                \
  case FF: {                                                                                             \
    const int per_ = persistent_grid(*b.ctx, mgcep_kernel<FF>, 64, (int64_t)1 << 40);                    \
    hipLaunchKernelGGL((mgcep_kernel<FF>), dim3((int)(tf < per_ ? tf : per_)), dim3(64), 0, st, d_in, fr, a, tf, d_mc, \
                       d_status);                                                                        \
  } break;
  switch (F) {
    WM_MGCEP_CASE(512)
    WM_MGCEP_CASE(1024)
    WM_MGCEP_CASE(2048)
    WM_MGCEP_CASE(4096)
  }
#undef WM_MGCEP_CASE
  return wm_check(hipGetLastError());
}

int launch_mel_cepstrum_of_frames(Batch& b, hipStream_t st, const double* d_frames, const WorldMi355McepOption& opt,
                                  double* d_mc, int* d_status) {
  if (const int rc = check_mgcep(b, d_frames, false, nullptr, 0, 0, opt, d_mc)) return rc;
  if (b.total_f <= 0) return WM_OK;
  MgcepFront fr;
  memset(&fr, 0, sizeof(fr));
  return launch_mgcep(b, st, d_frames, fr, opt, d_mc, d_status);
}

int launch_mel_cepstrum_of_waveform(Batch& b, hipStream_t st, const double* d_x, const double* window, int frame_length,
                                    int frame_shift, int pipe_float32, const WorldMi355McepOption& opt, double* d_mc,
                                    int* d_status) {
  if (const int rc = check_mgcep(b, d_x, true, window, frame_length, frame_shift, opt, d_mc)) return rc;
  if (b.total_f <= 0) return WM_OK;
  MgcepWs* W = nullptr;
  const int rc = grow_ws(b.mgcep, st, W, [&](const MgcepWs& w) { return w.cap >= frame_length; }, [&](MgcepWs& n) {
    n.cap = frame_length;
    return wm_check(n.alloc(&n.win, sizeof(double) * (size_t)frame_length));
  });
  if (rc) return rc;
  W->h_win.assign(window, window + frame_length);
  if (const int rc2 = wm_check(hipMemcpyAsync(W->win, W->h_win.data(), sizeof(double) * (size_t)frame_length,
                                              hipMemcpyHostToDevice, st)))
    return rc2;
  MgcepFront fr;
  memset(&fr, 0, sizeof(fr));
  fr.win = W->win;
  fr.x_off = b.d_x_off;
  fr.f_off = b.d_f_off;
  fr.x_len = b.d_x_len;
  fr.frame_utt = b.d_frame_utt;
  fr.L = frame_length;
  fr.P = frame_shift;
  fr.f32 = pipe_float32 ? 1 : 0;
  return launch_mgcep(b, st, d_x, fr, opt, d_mc, d_status);
}

}  // namespace wm
