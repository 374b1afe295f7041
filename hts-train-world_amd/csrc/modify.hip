// modify.hip -- WORLD's parameter modification on the device: F0 scaling and formant shift.
//
// Restates ParameterModification (externs/WORLD_v2/test/test.cpp:201-238), the step a caller places between analysis
// and synthesis.  Per utterance u, shift = f0_scale[u] and ratio = formant_ratio[u]:
//
//   f0_out[i] = f0[i] * shift                                                             (:204-207)
//   per frame, F = fft_size, n = F / 2 + 1, l[j] = log(sp[j]):                            (:211-227)
//     x1[j] = ratio * j / F * fs  (knots, evaluated left to right),  x2[i] = (double)i / F * fs  (queries)
//     out[i] = exp(interp1(x1, l, n, x2, n)[i])
//   if ratio < 1, c = int(F / 2.0 * ratio):  out[j] = out[c - 1], j = c .. F / 2          (:228-232)
//
// interp1 (src/matlabfunctions.cpp:157-182, with histc :136-155): k = clamp(#{j : x1[j] <= x2[i]}, 1, n - 1),
// s = (x2[i] - x1[k-1]) / (x1[k] - x1[k-1]), value l[k-1] + s (l[k] - l[k-1]).  Both axes are evaluated per bin with
// the reference's expressions in the reference's order, without contraction, so k and s are the reference's, ties
// (s == 0) included; a zero bin's -inf therefore meets the same products and makes NaN at the same bins.  Nothing is
// repaired.  The aperiodicity is not touched, as in the reference.
//
// modify_sp_kernel<F>: one wavefront per frame row, persistent over the batch's frames.  The row is read once, as
// F / 4 16-byte loads per wave and one 8-byte load (a row of F / 2 + 1 doubles starts on a 16-byte boundary every second
// frame: the single element is the last one there and the first one elsewhere), and l = wm_log(sp) is kept in LDS,
// (F / 2 + 1) doubles.  Lane t produces the bins t, t + 64, ...: the count starts from floor(i / ratio) + 1 and is
// confirmed by the two comparisons x1[c] <= x2[i] and x1[c-1] > x2[i]; two LDS reads, one wm_exp.  A bin of the fill
// region evaluates the query c - 1 instead of its own: the same expressions on the same operands, hence the bits of
// bin c - 1.  Nothing is stored before the whole row is in LDS, so sp_out == sp is safe.  The factors of an utterance
// come from a table in device memory, [2][n_utt], through the batch's frame -> utterance map; the table is filled from
// the caller's host arrays by kernel arguments (mlsa.hip's way: no host block outlives the call, nothing waits).
#include <math.h>
#include <string.h>

#include "batch.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "wavesync.hpp"

namespace wm {

namespace {

struct ModifyWs : StageWs {       // Batch::modify
  double* fac = nullptr;          // [2][n_utt]: shift, ratio
};

struct ModifyChunk {
  double v[128];
};
__global__ __launch_bounds__(128) void modify_put_kernel(const ModifyChunk c, int n, double* __restrict__ dst) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

typedef double double2_a16 __attribute__((ext_vector_type(2), aligned(16)));

template <int F>
__global__ __launch_bounds__(64) void modify_sp_kernel(const double* in, const double* __restrict__ ratio_of,
                                                       const int* __restrict__ frame_utt, int fs,
                                                       int64_t total_frames, double* out) {
#pragma clang fp contract(off)
  constexpr int BINS = F / 2 + 1, P = F / 256, M = F / 128;      // pairs per lane; bins per lane (lane 0: one more)
  __shared__ __attribute__((aligned(16))) double ls[BINS + 1];
  const int lane0 = threadIdx.x;
  ExpK ek;
  ek.load();
  const double dF = (double)F, dfs = (double)fs;
  for (int64_t frame = blockIdx.x; frame < total_frames; frame += gridDim.x) {
    const int lane = opaque_lane(lane0);
    const double* row = in + frame * (int64_t)BINS;
    const double ratio = uniform_d(ratio_of[frame_utt[frame]]);
    const int h = (int)(((uintptr_t)row >> 3) & 1u);             // 1: the row starts 8 bytes past a 16-byte boundary
    wave_sync();                                                 // the previous row's readers are done with ls
    {
      double2_a16 rv[P];
#pragma unroll
      for (int p = 0; p < P; ++p) rv[p] = *reinterpret_cast<const double2_a16*>(row + h + 2 * (lane + 64 * p));
      const double single = row[h ? 0 : F / 2];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int j = h + 2 * (lane + 64 * p);
        ls[j] = wm_log(rv[p].x);
        ls[j + 1] = wm_log(rv[p].y);
      }
      if (lane == 0) ls[h ? 0 : F / 2] = wm_log(single);
    }
    wave_sync();
    const int fill = ratio < 1.0 ? (int)(dF / 2.0 * ratio) : BINS;   // c of :229; >= 1 for every accepted ratio
    double* orow = out + frame * (int64_t)BINS;
#pragma unroll 4
    for (int m = 0; m <= M; ++m) {
      const int bin = lane + 64 * m;
      if (bin < BINS) {
        const int i = bin >= fill ? fill - 1 : bin;
        const double x2 = (double)i / dF * dfs;
        // the count #{j : x1[j] <= x2}: x1 is strictly increasing, so it is the c with x1[c-1] <= x2 < x1[c]
        int c = (int)fmin(floor((double)i / ratio) + 1.0, (double)BINS);
        while (c < BINS && ratio * (double)c / dF * dfs <= x2) ++c;
        while (c > 0 && ratio * (double)(c - 1) / dF * dfs > x2) --c;
        const int k = c < 1 ? 1 : (c > BINS - 1 ? BINS - 1 : c);
        const double xa = ratio * (double)(k - 1) / dF * dfs, xb = ratio * (double)k / dF * dfs;
        const double s = (x2 - xa) / (xb - xa);
        const double y0 = ls[k - 1], y1 = ls[k];
        orow[bin] = wm_exp_k(y0 + s * (y1 - y0), ek);
      }
    }
  }
}

__global__ __launch_bounds__(256) void modify_f0_kernel(const double* f0, const double* __restrict__ shift_of,
                                                        const int* __restrict__ frame_utt, int64_t n, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = f0[i] * shift_of[frame_utt[i]];
}

int upload_factors(hipStream_t st, const double* src, int n, double* dst) {
  for (int at = 0; at < n; at += 128) {
    ModifyChunk c;
    const int k = imin(128, n - at);
    memset(&c, 0, sizeof(c));
    memcpy(c.v, src + at, sizeof(double) * (size_t)k);
    hipLaunchKernelGGL(modify_put_kernel, dim3(1), dim3(128), 0, st, c, k, dst + at);
  }
  return wm_check(hipGetLastError());
}

// [a, a + n) and [b, b + n) share an element without being the same range
bool partial_overlap(const double* a, const double* b, int64_t n) {
  if (a == b || n <= 0) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(double);
  return pa < pb ? pb - pa < bytes : pa - pb < bytes;
}

}  // namespace

// What WorldMi355ModifyFeatures refuses, on the host alone: no device call is made for a refused argument set.
int check_modify(const Batch& b, const double* f0_scale, const double* formant_ratio, const double* d_f0,
                 const double* d_sp, const double* d_f0_out, const double* d_sp_out) {
  if (!f0_scale && !formant_ratio) return WM_ERR_BAD_ARG;
  const int F = b.p.fft_size;
  if (f0_scale) {
    if (!d_f0 || !d_f0_out) return WM_ERR_BAD_ARG;
    for (int u = 0; u < b.n_utt; ++u)
      if (!(f0_scale[u] > 0.0 && f0_scale[u] < HUGE_VAL)) return WM_ERR_BAD_ARG;
    if (partial_overlap(d_f0, d_f0_out, b.total_f)) return WM_ERR_BAD_ARG;
  }
  if (formant_ratio) {
    if (!d_sp || !d_sp_out) return WM_ERR_BAD_ARG;
    if (F != 512 && F != 1024 && F != 2048 && F != 4096) return WM_ERR_UNSUPPORTED_FFT;
    for (int u = 0; u < b.n_utt; ++u) {
      const double r = formant_ratio[u];
      // below 2 / F the fill would copy out[-1]; from F / 2 on every bin but 0 reads the first segment alone
      if (!(r > 0.0 && r < HUGE_VAL) || r < 2.0 / F || r > (double)F) return WM_ERR_BAD_ARG;
    }
    if (partial_overlap(d_sp, d_sp_out, b.total_f * (int64_t)(F / 2 + 1))) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

int launch_modify(Batch& b, hipStream_t st, const double* f0_scale, const double* formant_ratio, const double* d_f0,
                  const double* d_sp, double* d_f0_out, double* d_sp_out) {
  if (const int rc = check_modify(b, f0_scale, formant_ratio, d_f0, d_sp, d_f0_out, d_sp_out)) return rc;
  const int64_t tf = b.total_f;
  if (tf <= 0 || b.n_utt <= 0) return WM_OK;
  if (!b.modify) {
    std::unique_ptr<ModifyWs> W(new ModifyWs());
    if (const int rc = wm_check(W->alloc(&W->fac, sizeof(double) * 2 * (size_t)b.n_utt))) return rc;
    b.modify = std::move(W);
  }
  const ModifyWs& W = static_cast<const ModifyWs&>(*b.modify);
  double* d_shift = W.fac;
  double* d_ratio = W.fac + b.n_utt;
  if (f0_scale)
    if (const int rc = upload_factors(st, f0_scale, b.n_utt, d_shift)) return rc;
  if (formant_ratio)
    if (const int rc = upload_factors(st, formant_ratio, b.n_utt, d_ratio)) return rc;
  if (f0_scale) {
    const int64_t blocks = (tf + 255) / 256;
    hipLaunchKernelGGL(modify_f0_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, d_f0, d_shift,
                       b.d_frame_utt, tf, d_f0_out);
    if (const int rc = wm_check(hipGetLastError())) return rc;
  }
  if (!formant_ratio) return WM_OK;
  TimedScope ts_(b.ctx, st, "modify_kernel");
#define WM_MODIFY_CASE(FF)                                                                                   \
  case FF: {                                                                                                 \
    const int per_ = persistent_grid(*b.ctx, modify_sp_kernel<FF>, 64, (int64_t)1 << 40);                    \
    hipLaunchKernelGGL((modify_sp_kernel<FF>), dim3((int)(tf < per_ ? tf : per_)), dim3(64), 0, st, d_sp,    \
                       d_ratio, b.d_frame_utt, b.p.fs, tf, d_sp_out);                                        \
  } break;
  switch (b.p.fft_size) {
    WM_MODIFY_CASE(512)
    WM_MODIFY_CASE(1024)
    WM_MODIFY_CASE(2048)
    WM_MODIFY_CASE(4096)
  }
#undef WM_MODIFY_CASE
  return wm_check(hipGetLastError());
}

}  // namespace wm
