// ffo.hip -- what the recipe's `ffo` and `stats` targets (data/Makefile.in:325-459) and make_data_gv
// (scripts/Training.pl:1402-1491) need on the device: gap interpolation, `ffo` rows, per-utterance column moments.
//
// interpolate_gaps_kernel restates data/scripts/interpolate.pl:68-105.  A block is one utterance, a wave takes one
// column (waves beyond the first take the columns w, w + waves, ...) and walks it 64 frames at a time.  __ballot of
// "valid" is the chunk's mask; a lane's previous valid frame is the highest set bit below it (clz), its next the lowest
// above it (ctz).  Across chunks the previous valid frame is carried along; the next one is found by reading ahead to
// the first chunk with a set bit, and that answer is kept for as long as it lies beyond the chunk at hand, so a long
// gap is read ahead once.  a + step (t - lo) is evaluated in double with the product and the sum rounded separately, as
// Perl evaluates it: the float32 result has the script's bits.  A lane's result depends on its own column of its own
// utterance; there are no atomics (the status word is put together in LDS by the block's waves).
//
// ffo_compose_kernel is cmp_compose_kernel with a voicing column in front of the streams that have one: the values
// come from the same device function, cmp_window_value (streamwin.hpp).
//
// column_moments_kernel: block (utterance, 64 columns), four waves, a lane per column -- the arrangement and the
// summation order of mspf_mean_kernel (mspf.hip): wave q sums the 32-frame blocks q, q + 4, ... (each block in frame
// order, then added to the wave's sum), the four sums are added as (0 + 1) + (2 + 3).  Two passes in that order: the
// kept values and their count, then the squared deviations from the mean just computed.  The order depends on the
// utterance's length alone, so the bits do not depend on the batch around the utterance.
#include <math.h>
#include <string.h>

#include "batch.hpp"
#include "common.hpp"
#include "streamwin.hpp"

namespace wm {

constexpr int kGapMaxWaves = 4;                     // columns of an utterance taken side by side

__global__ __launch_bounds__(64 * kGapMaxWaves) void interpolate_gaps_kernel(
    const float* __restrict__ x, int dim, float ignore, const int64_t* __restrict__ f_off, float* __restrict__ out,
    float* __restrict__ voiced, int* __restrict__ status) {
#pragma clang fp contract(off)
  typedef unsigned long long u64;
  const int u = (int)blockIdx.x;
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
  const int64_t fb = f_off[u];
  const int64_t T = f_off[u + 1] - fb;
  __shared__ int empty[kGapMaxWaves];
  bool none = false;                                // a column of this wave's holds no valid value
  for (int col = w; col < dim; col += waves) {
    const float* __restrict__ xc = x + fb * dim + col;
    float* __restrict__ oc = out + fb * dim + col;
    int64_t lo_carry = -1;                          // the last valid frame in front of the chunk
    int64_t known_hi = -1;                          // the first valid frame behind some earlier chunk, T: there is none
    for (int64_t c0 = 0; c0 < T; c0 += 64) {
      const int64_t t = c0 + lane;
      const bool inb = t < T;
      const float v = inb ? xc[t * dim] : ignore;
      const bool valid = inb && !(v == ignore);     // NaN is a value, as in the script's ==
      const u64 mask = __ballot(valid);
      const u64 below = mask & (((u64)1 << lane) - 1);
      const u64 above = lane == 63 ? (u64)0 : mask & ~(((u64)2 << lane) - 1);
      const int64_t end = c0 + 64;
      const int last_in = (int)(T - c0 < 64 ? T - c0 : 64) - 1;
      const bool trailing = mask == 0 || 63 - __builtin_clzll(mask) < last_in;      // the same in every lane
      if (trailing && known_hi < end) {
        known_hi = T;
        for (int64_t c1 = end; c1 < T; c1 += 64) {
          const int64_t t1 = c1 + lane;
          const u64 m1 = __ballot(t1 < T && !(xc[t1 * dim] == ignore));
          if (m1 != 0) {
            known_hi = c1 + __builtin_ctzll(m1);
            break;
          }
        }
      }
      const int64_t lo = below != 0 ? c0 + 63 - __builtin_clzll(below) : lo_carry;
      const int64_t hi = above != 0 ? c0 + __builtin_ctzll(above) : (trailing ? known_hi : T);
      if (inb) {
        float r;
        if (valid) {
          r = v;
        } else if (lo < 0 && hi >= T) {
          r = 0.0f;                                 // the script dies here: status bit 1
        } else if (lo < 0) {
          r = xc[hi * dim];
        } else if (hi >= T) {
          r = xc[lo * dim];
        } else {
          const double a = (double)xc[lo * dim];
          const double step = ((double)xc[hi * dim] - a) / (double)(hi - lo);
          r = (float)(a + step * (double)(t - lo));
        }
        oc[t * dim] = r;
        if (col == 0 && voiced != nullptr) voiced[fb + t] = valid ? 1.0f : 0.0f;
      }
      if (mask != 0) lo_carry = c0 + 63 - __builtin_clzll(mask);
    }
    none |= T > 0 && lo_carry < 0;
  }
  if (status == nullptr) return;                    // the same in every thread
  if (lane == 0) empty[w] = none ? 1 : 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    int st = 0;
    for (int q = 0; q < waves; ++q) st |= empty[q];
    status[u] = st;
  }
}

struct FfoMeta {
  CmpMeta c;                                        // c.col0 and c.total_cols are the `cmp` row's and not used here
  int row0[kWinMaxStreams];                         // the stream's first column in the `ffo` row, its voicing column if any
  int width;
  const float* msd[kWinMaxStreams];
};

__global__ __launch_bounds__(256) void ffo_compose_kernel(FfoMeta m, const int* __restrict__ frame_utt,
                                                          const int64_t* __restrict__ f_off, int64_t total_frames,
                                                          float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total_frames * m.width) return;
  const int64_t frame = idx / m.width;
  const int col = (int)(idx - frame * m.width);
  int s = 0;
#pragma unroll
  for (int q = 1; q < kWinMaxStreams; ++q)
    if (q < m.c.n_streams && col >= m.row0[q]) s = q;
  int c = col - m.row0[s];
  if (m.msd[s] != nullptr) {
    if (c == 0) {
      out[idx] = m.msd[s][frame];
      return;
    }
    --c;
  }
  const int dim = m.c.win.dim[s];
  const int wi = c / dim, j = c - wi * dim;
  const int u = frame_utt[frame];
  out[idx] = cmp_window_value(m.c, s, wi, j, frame, f_off[u], f_off[u + 1] - 1);
}

__global__ __launch_bounds__(256) void column_moments_kernel(const float* __restrict__ x, int64_t ld, int width, int chunks,
                                                             int use_ignore, float ignore,
                                                             const int64_t* __restrict__ f_off,
                                                             int64_t* __restrict__ count, double* __restrict__ mean,
                                                             double* __restrict__ m2) {
#pragma clang fp contract(off)
  const int u = (int)(blockIdx.x / (unsigned)chunks);
  const int lane = (int)threadIdx.x & 63, q = (int)threadIdx.x >> 6;
  const int col = ((int)blockIdx.x - u * chunks) * 64 + lane;
  const int64_t fb = f_off[u];
  const int64_t T = f_off[u + 1] - fb;
  __shared__ double part[4][64];
  __shared__ int64_t kept[4][64];
  const float* __restrict__ xc = x + fb * ld + (col < width ? col : 0);
  const bool on = col < width;
  double s = 0.0;
  int64_t n = 0;
  if (on) {
    for (int64_t t0 = 32 * q; t0 < T; t0 += 128) {
      const int64_t t1 = t0 + 32 < T ? t0 + 32 : T;
      double p = 0.0;
      for (int64_t t = t0; t < t1; ++t) {
        const float v = xc[t * ld];
        if (use_ignore && v == ignore) continue;
        p += (double)v;
        ++n;
      }
      s += p;
    }
  }
  part[q][lane] = s;
  kept[q][lane] = n;
  __syncthreads();
  const int64_t n_all = (kept[0][lane] + kept[1][lane]) + (kept[2][lane] + kept[3][lane]);
  const double mu = n_all > 0 ? ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) / (double)n_all : 0.0;
  __syncthreads();
  s = 0.0;
  if (on) {
    for (int64_t t0 = 32 * q; t0 < T; t0 += 128) {
      const int64_t t1 = t0 + 32 < T ? t0 + 32 : T;
      double p = 0.0;
      for (int64_t t = t0; t < t1; ++t) {
        const float v = xc[t * ld];
        if (use_ignore && v == ignore) continue;
        const double d = (double)v - mu;
        p += d * d;
      }
      s += p;
    }
  }
  part[q][lane] = s;
  __syncthreads();
  if (q == 0 && on) {
    const int64_t at = (int64_t)u * width + col;
    count[at] = n_all;
    mean[at] = mu;
    m2[at] = n_all > 0 ? (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]) : 0.0;
  }
}

// What the three entry points refuse, on the host alone: no device call is made for a refused argument set.
int check_interpolate_gaps(const float* d_x, int dim, double ignore_value, const float* d_out) {
  if (!d_x || !d_out || dim < 1 || d_out == d_x) return WM_ERR_BAD_ARG;     // a lane reads frames other lanes write
  if (!(fabs(ignore_value) < __builtin_inf())) return WM_ERR_BAD_ARG;
  return WM_OK;
}
int check_compose_ffo(int n_streams, const float* const* d_data, const int* dims, const int* n_windows,
                      const double* const* const* windows, const int* const* window_sizes, const float* d_out) {
  return check_compose_cmp(n_streams, d_data, dims, n_windows, windows, window_sizes, d_out);   // msd may be null
}
int check_column_moments(const float* d_x, int64_t ld, int width, const double* ignore_value, const int64_t* d_count,
                         const double* d_mean, const double* d_m2) {
  if (!d_x || !d_count || !d_mean || !d_m2 || width < 1 || ld < width) return WM_ERR_BAD_ARG;
  if (ignore_value != nullptr && !(fabs(*ignore_value) < __builtin_inf())) return WM_ERR_BAD_ARG;
  return WM_OK;
}

int launch_interpolate_gaps(Batch& b, hipStream_t st, const float* d_x, int dim, double ignore_value, float* d_out,
                            float* d_voiced, int* d_status) {
  if (const int rc = check_interpolate_gaps(d_x, dim, ignore_value, d_out)) return rc;
  if (b.n_utt <= 0) return WM_OK;
  if (b.total_f <= 0) {
    if (d_status != nullptr) return wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st));
    return WM_OK;
  }
  const int waves = dim < kGapMaxWaves ? dim : kGapMaxWaves;
  TimedScope ts_(b.ctx, st, "interpolate_gaps_kernel");
  hipLaunchKernelGGL(interpolate_gaps_kernel, dim3((unsigned)b.n_utt), dim3(64 * waves), 0, st, d_x, dim,
                     (float)ignore_value, b.d_f_off, d_out, d_voiced, d_status);
  return wm_check(hipGetLastError());
}

int launch_compose_ffo(Batch& b, hipStream_t st, int n_streams, const float* const* d_data, const int* dims,
                       const int* n_windows, const double* const* const* windows, const int* const* window_sizes,
                       const float* const* d_msd, float* d_out) {
  if (const int rc = check_compose_ffo(n_streams, d_data, dims, n_windows, windows, window_sizes, d_out)) return rc;
  FfoMeta m;
  memset(&m, 0, sizeof(m));
  cmp_fill_meta(m.c, n_streams, d_data, dims, n_windows, windows, window_sizes);
  int col = 0;
  for (int s = 0; s < n_streams; ++s) {
    m.row0[s] = col;
    m.msd[s] = d_msd != nullptr ? d_msd[s] : nullptr;
    col += (m.msd[s] != nullptr ? 1 : 0) + dims[s] * n_windows[s];
  }
  m.width = col;
  const int64_t n = b.total_f * col;
  if (n <= 0) return WM_OK;
  TimedScope ts_(b.ctx, st, "ffo_compose_kernel");
  hipLaunchKernelGGL(ffo_compose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m, b.d_frame_utt, b.d_f_off,
                     b.total_f, d_out);
  return wm_check(hipGetLastError());
}

int launch_column_moments(Batch& b, hipStream_t st, const float* d_x, int64_t ld, int width, const double* ignore_value,
                          int64_t* d_count, double* d_mean, double* d_m2) {
  if (const int rc = check_column_moments(d_x, ld, width, ignore_value, d_count, d_mean, d_m2)) return rc;
  if (b.n_utt <= 0) return WM_OK;
  const int chunks = (width + 63) / 64;
  if ((int64_t)chunks * b.n_utt > (int64_t)1 << 30) return WM_ERR_BAD_ARG;
  TimedScope ts_(b.ctx, st, "column_moments_kernel");
  hipLaunchKernelGGL(column_moments_kernel, dim3((unsigned)(chunks * b.n_utt)), dim3(256), 0, st, d_x, ld, width, chunks,
                     ignore_value != nullptr ? 1 : 0, ignore_value != nullptr ? (float)*ignore_value : 0.0f, b.d_f_off,
                     d_count, d_mean, d_m2);
  return wm_check(hipGetLastError());
}

}  // namespace wm
