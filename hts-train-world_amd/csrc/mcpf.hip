// mcpf.hip -- the recipe's mel-cepstral postfilter (formant emphasis) on the device.
//
// Restates postfiltering_mcp (scripts/Training.pl:2642-2687), which gen_wave (:2813-2845) runs on every generated .mgc
// before mgc2sp: six SPTK tools per utterance.  For one frame c[0 .. m] at warp alpha and w = [1, 1, beta, ..., beta]:
//
//   r0 = E(c), p_r0 = E(w c), E(v) = c2acr -m co -M 0 -l L of freqt -m m -a alpha -M co -A 0 of v      (:2654-2662)
//        = (1 / L) sum_{k < L} exp(2 x_k), x_k the log amplitude at bin k of v taken to warp 0 and cut at order co;
//   delta = 1/2 ln(r0 / p_r0), added to coefficient 0 of mc2b(w c), then b2mc                          (:2664-2682)
//
// mc2b and b2mc are inverse to each other and b[0] enters v[0] alone, so the net effect is
//   out[0] = c[0] + delta,     out[k] = w[k] c[k]  (k >= 1).
//
// What is computed here is the co -> infinity limit of E at the script's own bins.  Neither freqt nor a transform is
// needed for it: x_k = sum_j v[j] cos(j W_k) at the warped frequency W_k of w_k = 2 pi k / L,
//   cos W_k = ((1 + a^2) cos w_k - 2 a) / (1 + a^2 - 2 a cos w_k),
// a Chebyshev series in that node.  c[0] and c[1] are common to both series: with A_k = c[1] cos W_k and
// B_k = sum_{j >= 2} c[j] cos(j W_k) the log spectra are c0 + A + B and c0 + A + beta B, c0 cancels in the ratio, and
//   delta = 1/2 ln( sum_k v_k e^{2 (A_k + B_k)} / sum_k v_k e^{2 (A_k + beta B_k)} ),  k = 0 .. L/2, v = 1, 2, ..., 2, 1:
// one Clenshaw recurrence and two exponentials per bin.  The limit differs from the script's value by at most twice
// the truncation tail sum_{n > co} |freqt(w c)[n]| -- 5e-431 at the recipe's setting (m 49, alpha 0.55, co 2047,
// L 4096; in double the series itself underflows there) -- while the script's own result carries the float32 rounding
// of its intermediate files, 1e-7
// (tests/golden/sptk_postfilter.npz: tail, recipe_f32_gap; tools/gen_golden_postfilter.py).
//
// mcpf_kernel<NQ>, L = 128 NQ (NQ = 1 also serves L = 64): one wave per frame, persistent over the batch's frames.
// Lane l owns the bins l + 64 q, q < NQ; twice their nodes are computed once per wave and stay in registers.  The
// frame's row is one coalesced load, lane j holding c[j]; the recurrence takes c[j] by v_readlane (wave-uniform) and
// runs eight bins per lane side by side.  The bin L/2 has the node -1: B = sum (-1)^j c[j], one wave sum.  The two
// sums are added per lane in ascending q and across the wave by the fixed DPP tree of wave_sum(), so a frame's
// result depends on nothing but its row.  No LDS.
#include <math.h>

#include "batch.hpp"
#include "common.hpp"
#include "fastmath.hpp"

namespace wm {

struct McpfArgs {
  double alpha, beta;
  int m, half;                 // half = length / 2: the bins are 0 .. half
};

// wm_exp_k (fastmath.hpp: its reduction, its polynomial, its coefficient pack) without the branch to the library
// function, so that a lane keeps several exponentials in flight: the argument is held to [-800, 800] by two selects (a
// NaN passes through) and ldexp carries the ends to 0 and to +infinity.
__device__ __forceinline__ double mcpf_exp(double x, const ExpK& k) {
  x = x < -800.0 ? -800.0 : (x > 800.0 ? 800.0 : x);
  const double kd = rint(x * k.l2e);
  double r = fma(-kd, k.ln2h, x);
  r = fma(-kd, k.ln2l, r);
  double p = k.c[0];
#pragma unroll
  for (int i = 1; i < 11; ++i) p = fma(p, r, k.c[i]);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return fm_ldexp(p, (int)kd);
}

template <int NQ>
__global__ __launch_bounds__(64) void mcpf_kernel(const double* mc, McpfArgs o, int64_t total_frames, double* out,
                                                  double* gain, int* status) {
  constexpr int G = NQ < 8 ? NQ : 8;                   // bins in flight per lane
  const int lane = threadIdx.x;
  const int m = o.m;
  double x2[NQ];                                       // 2 cos W_k of the lane's bins
  {
    SinCosPiK sk;
    sk.load();
    const double a2 = o.alpha + o.alpha, p = __builtin_fma(o.alpha, o.alpha, 1.0);
    const double inv_half = 1.0 / (double)o.half;      // a power of two: k / half is exact
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double sn, cs;
      wm_sincospi_k((double)(lane + 64 * q) * inv_half, sk, &sn, &cs);
      const double x = __builtin_fma(p, cs, -a2) / __builtin_fma(-a2, cs, p);
      x2[q] = x + x;
    }
  }
  ExpK ek;
  ek.load();
  const double beta = o.beta;
  for (int64_t frame = blockIdx.x; frame < total_frames; frame += gridDim.x) {
    const int64_t at = frame * (int64_t)(m + 1);
    const double cin = lane <= m ? mc[at + lane] : 0.0;
    int st = __ballot(!(fabs(cin) < __builtin_inf())) == 0ull ? 0 : 1;
    double delta = 0.0;
    if (st == 0) {
      const double c1 = readlane_d(cin, 1);
      // the bin L/2: node -1, A = -c1, B = sum_{j >= 2} (-1)^j c[j] (lanes beyond m hold 0)
      const double b_end = wave_sum(lane >= 2 ? ((lane & 1) ? -cin : cin) : 0.0);
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int q0 = 0; q0 < NQ; q0 += G) {
        // Clenshaw: b_j = c[j] + 2 x b_{j+1} - b_{j+2}, j = m .. 2, two steps per pass so that the two registers
        // trade places instead of being moved: b1 holds b_m at the start, the pairs leave the newer value in b1
        double b1[G], b2[G];
        int j = m - 1;
        {
          const double cm = readlane_d(cin, m);
#pragma unroll
          for (int g = 0; g < G; ++g) { b1[g] = cm; b2[g] = 0.0; }
        }
        if ((m & 1) != 0) {                            // an odd number of steps is left: one by itself
          const double cj = readlane_d(cin, j);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const double t = __builtin_fma(x2[q0 + g], b1[g], cj - b2[g]);
            b2[g] = b1[g];
            b1[g] = t;
          }
          --j;
        }
        for (; j >= 3; j -= 2) {
          const double ca = readlane_d(cin, j), cb = readlane_d(cin, j - 1);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            b2[g] = __builtin_fma(x2[q0 + g], b1[g], ca - b2[g]);
            b1[g] = __builtin_fma(x2[q0 + g], b2[g], cb - b1[g]);
          }
        }
        double u1[G], u2[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          // c[0] = c[1] = 0 in the series: b_1 = 2 x b_2 - b_3, B = x b_1 - b_2
          const double bb = __builtin_fma(x2[q0 + g], b1[g], -b2[g]);
          const double B2 = __builtin_fma(x2[q0 + g], bb, -(b1[g] + b1[g]));             // 2 B
          const double A2 = c1 * x2[q0 + g];                                              // 2 A
          u1[g] = A2 + B2;
          u2[g] = __builtin_fma(beta, B2, A2);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) u1[g] = mcpf_exp(u1[g], ek);
#pragma unroll
        for (int g = 0; g < G; ++g) u2[g] = mcpf_exp(u2[g], ek);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          double e1 = u1[g], e2 = u2[g];
          if (q0 + g == 0 && lane == 0) { e1 *= 0.5; e2 *= 0.5; }                        // v_0 = 1 beside v_k = 2
          if (NQ == 1 && lane >= o.half) { e1 = 0.0; e2 = 0.0; }                         // L = 64: 32 bins
          s1 += e1;
          s2 += e2;
        }
        // a group is finished before the next begins: left to itself the compiler runs every recurrence first and holds
        // all NQ arguments for one run of exponentials (214 registers at NQ = 32)
        s1 = opaque_d(s1);
        s2 = opaque_d(s2);
      }
      if (lane == 0) {
        const double B2 = b_end + b_end, A2 = -(c1 + c1);
        s1 += 0.5 * mcpf_exp(A2 + B2, ek);
        s2 += 0.5 * mcpf_exp(__builtin_fma(beta, B2, A2), ek);
      }
      const double S1 = wave_sum(s1), S2 = wave_sum(s2);
      if (S1 > 0.0 && S1 < __builtin_inf() && S2 > 0.0 && S2 < __builtin_inf()) {
        const double r = S1 / S2;
        // the quotient leaves the normal range only for sums hundreds of decades apart
        delta = r >= 2.2250738585072014e-308 && r < __builtin_inf() ? 0.5 * wm_log(r) : 0.5 * (log(S1) - log(S2));
      } else {
        st = 2;
      }
    }
    if (lane <= m) {
      double v = 0.0;
      if (st == 0) v = lane == 0 ? cin + delta : (lane == 1 ? cin : beta * cin);
      out[at + lane] = v;
    }
    if (lane == 0) {
      if (gain != nullptr) gain[frame] = delta;
      if (status != nullptr) status[frame] = st;
    }
  }
}

// beta == 1 or order == 1: the rows as they are, gain 0 (gen_wave skips the step at 1.0, :2838)
__global__ __launch_bounds__(256) void mcpf_identity_kernel(const double* mc, int64_t n, int64_t total_frames,
                                                            double* out, double* gain, int* status) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    if (out != mc) out[i] = mc[i];
    if (i < total_frames) {
      if (gain != nullptr) gain[i] = 0.0;
      if (status != nullptr) status[i] = 0;
    }
  }
}

// What WorldMi355MelCepstrumPostfilter refuses, on the host alone: no device call is made for a refused option set.
int check_mcpf(const double* d_mc, const WorldMi355McpfOption* opt, const double* d_out) {
  if (!d_mc || !opt || !d_out) return WM_ERR_BAD_ARG;
  if (opt->order < 1 || opt->order > 63) return WM_ERR_BAD_ARG;
  if (!(fabs(opt->alpha) < 1.0) || !(fabs(opt->beta) < __builtin_inf())) return WM_ERR_BAD_ARG;
  const int L = opt->length;
  if (L < 64 || L > 8192 || (L & (L - 1)) != 0) return WM_ERR_BAD_ARG;
  return WM_OK;
}

int launch_mcpf(Batch& b, hipStream_t st, const double* d_mc, const WorldMi355McpfOption& opt, double* d_out,
                double* d_gain, int* d_status) {
  if (const int rc = check_mcpf(d_mc, &opt, d_out)) return rc;
  const int64_t tf = b.total_f;
  if (tf <= 0) return WM_OK;
  TimedScope ts_(b.ctx, st, "mcpf_kernel");
  if (opt.beta == 1.0 || opt.order == 1) {
    const int64_t n = tf * (opt.order + 1);            // >= 2 tf: the frame index fits the same walk
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(mcpf_identity_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, d_mc, n, tf,
                       d_out, d_gain, d_status);
    return wm_check(hipGetLastError());
  }
  McpfArgs a;
  a.alpha = opt.alpha;
  a.beta = opt.beta;
  a.m = opt.order;
  a.half = opt.length / 2;
  // every frame costs the same: the grid is the waves that are resident at once, without persistent_grid's
  // oversubscription (which answers frames of uneven cost)
#define WM_MCPF_CASE(NQ)                                                                                       \
  case NQ: {                                                                                                   \
    const int64_t slots_ = persistent_grid(*b.ctx, mcpf_kernel<NQ>, 64, (int64_t)1 << 40);                     \
    const int64_t per_ = imax(1, (int)(slots_ / imax(1, b.ctx->oversub)));                                     \
    hipLaunchKernelGGL((mcpf_kernel<NQ>), dim3((int)(tf < per_ ? tf : per_)), dim3(64), 0, st, d_mc, a, tf, d_out, \
                       d_gain, d_status);                                                                      \
  } break;
  switch (imax(1, opt.length / 128)) {
    WM_MCPF_CASE(1)
    WM_MCPF_CASE(2)
    WM_MCPF_CASE(4)
    WM_MCPF_CASE(8)
    WM_MCPF_CASE(16)
    WM_MCPF_CASE(32)
    WM_MCPF_CASE(64)
  }
#undef WM_MCPF_CASE
  return wm_check(hipGetLastError());
}

}  // namespace wm
