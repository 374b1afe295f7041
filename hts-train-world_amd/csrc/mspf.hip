// mspf.hip -- the recipe's modulation-spectrum postfilter and its statistics on the device.
//
// Restates postfiltering_mspf (scripts/Training.pl:2950-3000, msmp2seq :3003-3038), which gen_wave runs instead of
// postfiltering_mcp when USEMSPF is set, and the forward half that make_mspf (:3133-3221) runs over the training set.
// Settings: frame_length Lw (odd), fft_length N, emphasis e; S = (Lw - 1) / 2, K = N / 2 + 1.  One column x[0 .. T):
//   1  mu = mean(x), y = x - mu
//   2  J = ceil((T + S) / S) frames, z_j[i] = w[i] y[j S - S + i] (y = 0 outside [0, T)), zeros up to N
//   3  w: SPTK's Bartlett window, 2 i / (Lw - 1) for i < Lw / 2, else 2 - 2 i / (Lw - 1)
//   4  X_j = DFT_N(z_j), m_j[k] = 1/2 ln(|X_j[k]|^2 + 1e-30)
//   5  m' = m + e (((m - mean_gen[k]) / std_gen[k]) std_nat[k] + mean_nat[k] - m)
//   6  X'_j[k] = exp(m') X_j[k] / |X_j[k]| (exp(m') where |X_j[k]|^2 is 0), v_j the inverse real transform
//   7  seq[j S + n] += v_j[n] for all n < N, out[t] = seq[S + t] + mu
// The statistics are sum m and sum m^2 per column and bin over every frame, the all-zero trailing frames included.
//
// Mapping: one column per lane, as mlpg_kernel.  A wave takes 64 adjacent columns of one time segment (kMspfSegment
// frames) of one utterance; rows are read and written coalesced and the tables lie [k][column][4].  The N-point real
// transform is a complex transform of N / 2 points in the lane's registers (Dft<R> of fft.hpp up to 16, one more level
// for 32) and a split, all twiddles compile-time constants: no cross-lane exchange.  The spectrum is never an array:
// the bins are taken in pairs (k, N / 2 - k) out of the packed transform, converted and put back as the packed input
// of the inverse transform, in place (MspfBins).  std_nat / std_gen is formed once per bin on the host; the window is
// the definition's own expression, evaluated once per block into LDS.  The overlap-add accumulator is a
// ring of N samples per lane in LDS, [n][lane]: a lane touches its own column only, so there is no barrier.  After
// frame j the samples j S .. j S + S - 1 are complete, are written out and their slots cleared.  A segment starts at
// the first frame that reaches its first sample, with a cleared ring, so every sample is summed from zero in ascending
// frame order whichever segment owns it: the bits do not depend on the segmentation, nor on the batch around the
// utterance.  The means come from mspf_mean_kernel (blocks of 32 frames, four waves taking the blocks in turn, a
// fixed tree at the end); a column whose mean is not finite -- a non-finite input, or a sum that overflows -- is
// status bit 1 and zeros, in every segment alike.  A column with a result that is not finite (bit 2) is found by
// whichever segment meets it: the segment marks the column in a per-utterance flag word and mspf_zero_kernel clears
// the marked columns afterwards.
#include <math.h>
#include <string.h>

#include <vector>

#include "batch.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "fft.hpp"

namespace wm {

constexpr int kMspfSegment = 256;                   // output frames per wave

struct MspfArgs {
  int dim, Lw, S, chunks, max_segs;
  double emphasis;
};

// cos(2 pi k / 64), k = 0 .. 16; the sine is the same table read backwards
struct MspfTw {
  static constexpr double kC[17] = {1.0,
                                    0.99518472667219688624,
                                    0.98078528040323044913,
                                    0.95694033573220886494,
                                    0.92387953251128675613,
                                    0.88192126434835502971,
                                    0.83146961230254523708,
                                    0.77301045336273696081,
                                    0.70710678118654752440,
                                    0.63439328416364549822,
                                    0.55557023301960222474,
                                    0.47139673682599764856,
                                    0.38268343236508977173,
                                    0.29028467725446236764,
                                    0.19509032201612826785,
                                    0.09801714032956060199,
                                    0.0};
  // W_64^k = (cos, -sin)(2 pi k / 64) for any k
  static constexpr double re(int k) {
    const int q = (k & 63) >> 4, r = k & 15;
    return q == 0 ? kC[r] : q == 1 ? -kC[16 - r] : q == 2 ? -kC[r] : kC[16 - r];
  }
  static constexpr double im(int k) {
    const int q = (k & 63) >> 4, r = k & 15;
    return -(q == 0 ? kC[16 - r] : q == 1 ? kC[r] : q == 2 ? -kC[16 - r] : -kC[r]);
  }
};

// the complex transform of M = 8, 16 or 32 points in registers, natural order in and out
template <int M, int Q = 0> struct MspfLevel {
  __device__ static __forceinline__ void run(cpx (&e)[M / 2], cpx (&o)[M / 2]) {
    if constexpr (Q < M / 2) {
      bfly_tw(e[Q], o[Q], make_double2(MspfTw::re(Q * (64 / M)), MspfTw::im(Q * (64 / M))));
      MspfLevel<M, Q + 1>::run(e, o);
    }
  }
};
template <int M> __device__ __forceinline__ void mspf_cfft(cpx (&v)[M]) {
  if constexpr (M <= 16) {
    Dft<M>::run(v);
  } else {
    cpx e[M / 2], o[M / 2];
#pragma unroll
    for (int r = 0; r < M / 2; ++r) {
      e[r] = v[2 * r];
      o[r] = v[2 * r + 1];
    }
    Dft<M / 2>::run(e);
    __builtin_amdgcn_sched_barrier(0);
    Dft<M / 2>::run(o);
    __builtin_amdgcn_sched_barrier(0);
    MspfLevel<M>::run(e, o);
#pragma unroll
    for (int q = 0; q < M / 2; ++q) {
      v[q] = e[q];
      v[q + M / 2] = o[q];
    }
  }
}

// The spectrum of the N = 2 M real points, bin by bin, from Z = DFT_M of z[n] = x[2 n] + i x[2 n + 1], and back, in
// place.  With E = (Z[k] + conj Z[M - k]) / 2, O = -i (Z[k] - conj Z[M - k]) / 2 and P = W_N^k O:
//   X[k] = E + P,   X[M - k] = conj(E - P).
// f.at<bin>(X) returns the new value of the bin; the bins come in the order 0, M, 1, M - 1, 2, ...
// Back: E' = A + conj B, P' = A - conj B (A, B the new X[k], X[M - k]),
// O' = conj(W_N^k) P', Z'[k] = E' + i O', Z'[M - k] = conj E' + i conj O'; what is stored is conj Z', so that the
// inverse transform is the forward one, and the halves and its 1 / M are one factor 1 / N at the end.  With BACK false
// f is only called.  A pair is finished before the next begins (the scheduler would otherwise start every bin's table
// loads at once and hold their results).
template <int M, bool BACK, int Kk, class F> struct MspfBins {
  __device__ static __forceinline__ void run(cpx (&Z)[M], F& f) {
    if constexpr (Kk == 0) {
      cpx A = make_double2(Z[0].x + Z[0].y, 0.0), B = make_double2(Z[0].x - Z[0].y, 0.0);
      A = f.template at<0>(A);
      B = f.template at<M>(B);
      if constexpr (BACK) Z[0] = make_double2(A.x + B.x, -(A.x - B.x));
      __builtin_amdgcn_sched_barrier(0);
      MspfBins<M, BACK, 1, F>::run(Z, f);
    } else if constexpr (Kk <= M / 2) {
      constexpr double c = MspfTw::re(Kk * (32 / M)), s = MspfTw::im(Kk * (32 / M));
      const cpx a = Z[Kk], b = Z[M - Kk];
      const double ex = 0.5 * (a.x + b.x), ey = 0.5 * (a.y - b.y);
      const double ox = 0.5 * (a.y + b.y), oy = -0.5 * (a.x - b.x);
      const double px = __builtin_fma(c, ox, -(s * oy)), py = __builtin_fma(c, oy, s * ox);
      cpx A = make_double2(ex + px, ey + py), B = make_double2(ex - px, py - ey);
      A = f.template at<Kk>(A);
      if constexpr (Kk < M / 2) B = f.template at<M - Kk>(B);
      else B = A;                                                       // the bin N / 4 is its own partner
      if constexpr (BACK) {
        const double fx = A.x + B.x, fy = A.y - B.y;
        const double qx = A.x - B.x, qy = A.y + B.y;
        const double rx = __builtin_fma(c, qx, s * qy), ry = __builtin_fma(c, qy, -(s * qx));   // conj(W) P'
        Z[Kk] = make_double2(fx - ry, -(fy + rx));
        if constexpr (Kk < M / 2) Z[M - Kk] = make_double2(fx + ry, fy - rx);
      }
      __builtin_amdgcn_sched_barrier(0);
      MspfBins<M, BACK, Kk + 1, F>::run(Z, f);
    }
  }
};

// A value the compiler must take as new where this stands.  Inside the frame loop it keeps what is the same in every
// frame -- the window, the row offsets of the tables -- from being computed once in front of the loop and held in
// registers throughout: 64 window values alone are 128 registers.
template <class T> __device__ __forceinline__ T mspf_fresh(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the window in LDS, wz[0 .. 64): 2 i / (Lw - 1) for i < S, 2 - 2 i / (Lw - 1) up to Lw, zeros beyond
__device__ __forceinline__ void mspf_window(double* wz, int lane, const MspfArgs& a) {
  const double up = 2.0 * (double)lane / (double)(a.Lw - 1);
  wz[lane] = lane >= a.Lw ? 0.0 : (lane < a.S ? up : 2.0 - up);
}

// steps 2-4 of frame j for the lane's column, up to the packed transform Z of the windowed frame.  Eight rows are loaded
// at a time, at a row index clamped to the utterance (a select puts the zero), and groups beyond the window are skipped.
template <int N>
__device__ __forceinline__ void mspf_forward(const double* __restrict__ xc, int64_t ld, int T, int j, const MspfArgs& a,
                                             const double* wz, double mu, cpx (&z)[N / 2]) {
  const int base = j * a.S - a.S;
  const double* wl = mspf_fresh(wz);
#pragma unroll
  for (int g = 0; g < N; g += 8) {
    if (g < a.Lw) {
#pragma unroll
      for (int i = g; i < g + 8; ++i) {
        const int s = base + i;
        const int sc = s < 0 ? 0 : (s > T - 1 ? T - 1 : s);
        const double raw = xc[(int64_t)sc * ld];
        const double v = s == sc ? wl[i] * (raw - mu) : 0.0;
        if (i & 1) z[i >> 1].y = v;
        else z[i >> 1].x = v;
      }
    } else {
#pragma unroll
      for (int i = g; i < g + 8; i += 2) z[i >> 1] = make_double2(0.0, 0.0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  mspf_cfft<N / 2>(z);
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ double mspf_logamp(cpx X, double& r2) {
  r2 = __builtin_fma(X.x, X.x, X.y * X.y);
  return 0.5 * wm_log(r2 + 1e-30);
}

// steps 5 and 6 on one bin.  The tables lie [k][column][4]: mean_gen, std_nat / std_gen, mean_nat, 0.  Two pointers
// walk them from both ends in the order MspfBins takes the bins.
template <int N> struct MspfConvert {
  const double* lo;
  const double* hi;
  int64_t step;
  double emphasis;
  template <int Kb> __device__ __forceinline__ cpx at(cpx X) {
    const double* p;
    if constexpr (Kb <= N / 4) {
      p = lo;
      lo += step;
    } else {
      p = hi;
      hi -= step;
    }
    const double2 t01 = *reinterpret_cast<const double2*>(p);
    const double t2 = p[2];
    double r2;
    const double m = mspf_logamp(X, r2);
    const double tgt = __builtin_fma(m - t01.x, t01.y, t2);
    const double amp = wm_exp(__builtin_fma(emphasis, tgt - m, m));
    if (!(r2 > 0.0)) return make_double2(amp, 0.0);
    const double sc = amp / sqrt(r2);
    return make_double2(sc * X.x, sc * X.y);
  }
};
// the sums of the statistics, in LDS [2 K][lane]
template <int N> struct MspfAdd {
  double (*acc)[64];
  int lane;
  template <int Kb> __device__ __forceinline__ cpx at(cpx X) {
    double r2;
    const double m = mspf_logamp(X, r2);
    acc[Kb][lane] += m;
    acc[N / 2 + 1 + Kb][lane] = __builtin_fma(m, m, acc[N / 2 + 1 + Kb][lane]);
    return X;
  }
};

// Column means per utterance: block (utterance, 64 columns), four waves.  Wave q sums the 32-frame blocks q, q + 4, ...
// (each block in frame order, then added to the wave's sum), and the four sums are added as (0 + 1) + (2 + 3).  A
// column with a value that is not finite gets NaN.
__global__ __launch_bounds__(256) void mspf_mean_kernel(const double* __restrict__ x, const int64_t* __restrict__ f_off,
                                                        int dim, int chunks, double* __restrict__ mean) {
  const int u = (int)(blockIdx.x / (unsigned)chunks);
  const int lane = (int)threadIdx.x & 63, q = (int)threadIdx.x >> 6;
  const int col = ((int)blockIdx.x - u * chunks) * 64 + lane;
  const int64_t fb = f_off[u];
  const int T = (int)(f_off[u + 1] - fb);
  __shared__ double part[4][64];
  __shared__ int nonfinite[64];
  if (q == 0) nonfinite[lane] = 0;
  __syncthreads();
  double s = 0.0;
  bool bad = false;
  if (col < dim) {
    const double* __restrict__ xc = x + fb * dim + col;
    for (int t0 = 32 * q; t0 < T; t0 += 128) {
      const int t1 = t0 + 32 < T ? t0 + 32 : T;
      double p = 0.0;
      for (int t = t0; t < t1; ++t) {
        const double v = xc[(int64_t)t * dim];
        bad |= !(fabs(v) < __builtin_inf());
        p += v;
      }
      s += p;
    }
  }
  part[q][lane] = s;
  if (bad) atomicOr(&nonfinite[lane], 1);
  __syncthreads();
  if (q == 0 && col < dim && T > 0) {
    const double tot = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    mean[(int64_t)u * dim + col] = nonfinite[lane] ? __builtin_nan("") : tot / (double)T;
  }
}

template <int N>
__global__ __launch_bounds__(64) void mspf_kernel(const double* __restrict__ x, MspfArgs a,
                                                  const int64_t* __restrict__ f_off, const double* __restrict__ mean,
                                                  const double* __restrict__ tab, double* __restrict__ out,
                                                  int* __restrict__ colflag, int* __restrict__ status) {
  constexpr int M = N / 2, K = M + 1;
  __shared__ double ring[N][64];
  __shared__ double wz[64];
  const int lane = (int)threadIdx.x;
  mspf_window(wz, lane, a);
  __syncthreads();
  const int per_utt = a.chunks * a.max_segs;
  const int u = (int)(blockIdx.x / (unsigned)per_utt);
  const int rel = (int)blockIdx.x - u * per_utt;
  const int seg = rel / a.chunks;
  const int col = (rel - seg * a.chunks) * 64 + lane;
  const int64_t fb = f_off[u];
  const int T = (int)(f_off[u + 1] - fb);
  const int t_lo = seg * kMspfSegment;
  if (t_lo >= T || col >= a.dim) return;
  const int t_hi = t_lo + kMspfSegment < T ? t_lo + kMspfSegment : T;
  const int S = a.S, dim = a.dim;
  const int64_t ld = dim;
  const double* __restrict__ xc = x + fb * ld + col;
  double* __restrict__ oc = out + fb * ld + col;
  const double mu = mean[(int64_t)u * dim + col];
  const bool bad_in = !(fabs(mu) < __builtin_inf());
  const double* __restrict__ tc = tab + (int64_t)col * 4;
#pragma unroll
  for (int n = 0; n < N; ++n) ring[n][lane] = 0.0;
  MspfConvert<N> conv;
  conv.emphasis = a.emphasis;
  // the frames that reach the samples S + t_lo .. S + t_hi - 1 of seq: j S <= p < j S + N
  const int p_lo = S + t_lo;
  const int j_lo = p_lo < N ? 0 : (p_lo - N) / S + 1;
  const int j_hi = (S + t_hi - 1) / S;                                // < J = ceil((T + S) / S)
  bool bad_out = false;
  for (int j = j_lo; j <= j_hi; ++j) {
    cpx z[M];
    mspf_forward<N>(xc, ld, T, j, a, wz, mu, z);
    conv.step = mspf_fresh((int64_t)dim * 4);
    conv.lo = tc;
    conv.hi = tc + M * conv.step;
    MspfBins<M, true, 0, MspfConvert<N>>::run(z, conv);
    __builtin_amdgcn_sched_barrier(0);
    mspf_cfft<M>(z);
    const int p0 = j * S;
    constexpr double inv_n = 1.0 / (double)N;
#pragma unroll
    for (int n = 0; n < M; ++n) {
      ring[(p0 + 2 * n) & (N - 1)][lane] += inv_n * z[n].x;
      ring[(p0 + 2 * n + 1) & (N - 1)][lane] -= inv_n * z[n].y;
      if ((n & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    for (int q = 0; q < S; ++q) {
      const int p = p0 + q, t = p - S;
      if (t >= t_lo && t < t_hi) {
        const double v = ring[p & (N - 1)][lane] + mu;
        bad_out |= !(fabs(v) < __builtin_inf());
        oc[(int64_t)t * ld] = bad_in ? 0.0 : v;
      }
      ring[p & (N - 1)][lane] = 0.0;
    }
  }
  if (bad_in) {
    if (status != nullptr) atomicOr(status + u, 1);
  } else if (bad_out) {
    atomicOr(colflag + (int64_t)u * dim + col, 2);
    if (status != nullptr) atomicOr(status + u, 2);
  }
}

// a column that some segment marked is zeros in every frame of its utterance
__global__ __launch_bounds__(256) void mspf_zero_kernel(const int* __restrict__ colflag, const int* __restrict__ frame_utt,
                                                        int dim, int64_t n, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int64_t frame = idx / dim;
  const int col = (int)(idx - frame * dim);
  if (colflag[(int64_t)frame_utt[frame] * dim + col] != 0) out[idx] = 0.0;
}

// The forward half over a whole utterance: sum m and sum m^2 per bin of the lane's column, in frame order, to
// part[utterance][0 / 1][k][column]; the sums are kept in LDS, [2 K][lane], a lane touching its own column only.
template <int N>
__global__ __launch_bounds__(64) void mspf_stats_kernel(const double* __restrict__ x, MspfArgs a,
                                                        const int64_t* __restrict__ f_off,
                                                        const double* __restrict__ mean, double* __restrict__ part) {
  constexpr int M = N / 2, K = M + 1;
  __shared__ double acc[2 * K][64];
  __shared__ double wz[64];
  const int lane = (int)threadIdx.x;
  mspf_window(wz, lane, a);
  __syncthreads();
  const int u = (int)(blockIdx.x / (unsigned)a.chunks);
  const int col = ((int)blockIdx.x - u * a.chunks) * 64 + lane;
  const int64_t fb = f_off[u];
  const int T = (int)(f_off[u + 1] - fb);
  if (col >= a.dim) return;
  const int dim = a.dim;
#pragma unroll
  for (int k = 0; k < 2 * K; ++k) acc[k][lane] = 0.0;
  MspfAdd<N> add{acc, lane};
  if (T > 0) {
    const double* __restrict__ xc = x + fb * (int64_t)dim + col;
    const double mu = mean[(int64_t)u * dim + col];
    const int J = (T + a.S + a.S - 1) / a.S;
    for (int j = 0; j < J; ++j) {
      cpx z[M];
      mspf_forward<N>(xc, dim, T, j, a, wz, mu, z);
      MspfBins<M, false, 0, MspfAdd<N>>::run(z, add);
    }
  }
  double* __restrict__ pc = part + (int64_t)u * 2 * K * dim + col;
#pragma unroll
  for (int k = 0; k < 2 * K; ++k) pc[(int64_t)k * dim] = acc[k][lane];
}

// the utterances' sums added in index order: sum, sumsq [column][k]
__global__ __launch_bounds__(256) void mspf_stats_add_kernel(const double* __restrict__ part, int n_utt, int dim, int K,
                                                             double* __restrict__ sum, double* __restrict__ sumsq) {
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);             // k * dim + column
  if (idx >= K * dim) return;
  const int k = idx / dim, col = idx - k * dim;
  double s1 = 0.0, s2 = 0.0;
  for (int u = 0; u < n_utt; ++u) {
    const double* p = part + (int64_t)u * 2 * K * dim;
    s1 += p[idx];
    s2 += p[(int64_t)K * dim + idx];
  }
  sum[(int64_t)col * K + k] = s1;
  sumsq[(int64_t)col * K + k] = s2;
}

// What the three entry points refuse, on the host alone: no device call is made for a refused argument set.
static int check_mspf_option(const WorldMi355MspfOption* opt) {
  if (!opt) return WM_ERR_BAD_ARG;
  const int N = opt->fft_length, Lw = opt->frame_length;
  if (N != 16 && N != 32 && N != 64) return WM_ERR_BAD_ARG;
  if (Lw < 3 || Lw > N - 1 || Lw % 2 == 0) return WM_ERR_BAD_ARG;
  if (!(fabs(opt->emphasis) < __builtin_inf())) return WM_ERR_BAD_ARG;
  return WM_OK;
}
int check_column_means(const double* d_x, int dim, const double* d_mean) {
  if (!d_x || !d_mean || dim < 1) return WM_ERR_BAD_ARG;
  return WM_OK;
}
int check_mspf(const double* d_x, int dim, const WorldMi355MspfOption* opt, const double* mean_gen, const double* std_gen,
               const double* mean_nat, const double* std_nat, const double* d_out) {
  if (!d_x || !d_out || !mean_gen || !std_gen || !mean_nat || !std_nat || dim < 1) return WM_ERR_BAD_ARG;
  if (const int rc = check_mspf_option(opt)) return rc;
  if (d_out == d_x) return WM_ERR_BAD_ARG;                            // a segment reads its neighbours' input
  const int64_t n = (int64_t)dim * (opt->fft_length / 2 + 1);
  for (int64_t i = 0; i < n; ++i) {
    if (!(fabs(mean_gen[i]) < __builtin_inf()) || !(fabs(mean_nat[i]) < __builtin_inf())) return WM_ERR_BAD_ARG;
    if (!(fabs(std_nat[i]) < __builtin_inf()) || !(std_gen[i] > 0.0 && std_gen[i] < __builtin_inf())) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}
int check_mspf_stats(const double* d_x, int dim, const WorldMi355MspfOption* opt, const double* d_sum,
                     const double* d_sumsq, const int64_t* n_frames) {
  if (!d_x || !d_sum || !d_sumsq || !n_frames || dim < 1) return WM_ERR_BAD_ARG;
  return check_mspf_option(opt);
}

struct MspfWs : StageWs {
  double *mean = nullptr, *tab = nullptr, *part = nullptr;
  int* flag = nullptr;
  int64_t cap[4] = {0, 0, 0, 0};                  // mean, tab, part in doubles; flag in ints
  std::vector<double> h_tab;                      // the tables as uploaded: the copy's source lives as long as the batch
};

// the batch's workspace with room for `need` (mean, tab, part, flag): the postfilter and the statistics share it, so a
// replacement keeps what either had -- every block is max(old, need)
static int mspf_ws(Batch& b, hipStream_t st, const int64_t (&need)[4], MspfWs** out) {
  int64_t cap[4];
  const MspfWs* old = static_cast<const MspfWs*>(b.mspf.get());
  for (int i = 0; i < 4; ++i) cap[i] = old != nullptr && old->cap[i] > need[i] ? old->cap[i] : need[i];
  auto fits = [&](const MspfWs& w) { return w.cap[0] >= need[0] && w.cap[1] >= need[1] && w.cap[2] >= need[2] && w.cap[3] >= need[3]; };
  return grow_ws(b.mspf, st, *out, fits, [&](MspfWs& n) {
    for (int i = 0; i < 4; ++i) n.cap[i] = cap[i];
    if (cap[0] > 0)
      if (const int rc = wm_check(n.alloc(&n.mean, sizeof(double) * (size_t)cap[0]))) return rc;
    if (cap[1] > 0)
      if (const int rc = wm_check(n.alloc(&n.tab, sizeof(double) * (size_t)cap[1]))) return rc;
    if (cap[2] > 0)
      if (const int rc = wm_check(n.alloc(&n.part, sizeof(double) * (size_t)cap[2]))) return rc;
    return cap[3] > 0 ? wm_check(n.alloc(&n.flag, sizeof(int) * (size_t)cap[3])) : WM_OK;
  });
}

static void mspf_args(const WorldMi355MspfOption& opt, int dim, int max_len, MspfArgs* a) {
  memset(a, 0, sizeof(*a));
  a->dim = dim;
  a->Lw = opt.frame_length;
  a->S = (opt.frame_length - 1) / 2;
  a->chunks = (dim + 63) / 64;
  a->max_segs = (max_len + kMspfSegment - 1) / kMspfSegment;
  a->emphasis = opt.emphasis;
}

static int launch_means(Batch& b, hipStream_t st, const double* d_x, int dim, double* d_mean) {
  const int chunks = (dim + 63) / 64;
  if ((int64_t)chunks * b.n_utt > (int64_t)1 << 30) return WM_ERR_BAD_ARG;
  hipLaunchKernelGGL(mspf_mean_kernel, dim3((unsigned)(chunks * b.n_utt)), dim3(256), 0, st, d_x, b.d_f_off, dim, chunks,
                     d_mean);
  return wm_check(hipGetLastError());
}

int launch_column_means(Batch& b, hipStream_t st, const double* d_x, int dim, double* d_mean) {
  if (const int rc = check_column_means(d_x, dim, d_mean)) return rc;
  if (b.n_utt <= 0) return WM_OK;
  // an utterance without frames has no mean: its row is zeros
  if (const int rc = wm_check(hipMemsetAsync(d_mean, 0, sizeof(double) * (size_t)b.n_utt * dim, st))) return rc;
  if (b.total_f <= 0) return WM_OK;
  return launch_means(b, st, d_x, dim, d_mean);
}

int launch_mspf(Batch& b, hipStream_t st, const double* d_x, int dim, const WorldMi355MspfOption& opt,
                const double* mean_gen, const double* std_gen, const double* mean_nat, const double* std_nat,
                double* d_out, int* d_status) {
  if (const int rc = check_mspf(d_x, dim, &opt, mean_gen, std_gen, mean_nat, std_nat, d_out)) return rc;
  if (b.n_utt <= 0) return WM_OK;
  if (d_status != nullptr)
    if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st))) return rc;
  if (b.total_f <= 0) return WM_OK;
  const int K = opt.fft_length / 2 + 1;
  MspfArgs a;
  mspf_args(opt, dim, b.max_f0_len, &a);
  const int64_t blocks = (int64_t)b.n_utt * a.chunks * a.max_segs;
  if (blocks > (int64_t)1 << 30) return WM_ERR_BAD_ARG;
  const int64_t need[4] = {(int64_t)b.n_utt * dim, (int64_t)4 * K * dim, 0, (int64_t)b.n_utt * dim};
  MspfWs* W = nullptr;
  if (const int rc = mspf_ws(b, st, need, &W)) return rc;
  W->h_tab.assign((size_t)4 * K * dim, 0.0);                          // [k][column][4]
  for (int c = 0; c < dim; ++c)
    for (int k = 0; k < K; ++k) {
      const size_t at = ((size_t)k * dim + c) * 4, from = (size_t)c * K + k;
      W->h_tab[at] = mean_gen[from];
      W->h_tab[at + 1] = std_nat[from] / std_gen[from];
      W->h_tab[at + 2] = mean_nat[from];
    }
  if (const int rc = wm_check(hipMemcpyAsync(W->tab, W->h_tab.data(), sizeof(double) * W->h_tab.size(),
                                             hipMemcpyHostToDevice, st)))
    return rc;
  if (const int rc = wm_check(hipMemsetAsync(W->flag, 0, sizeof(int) * (size_t)b.n_utt * dim, st))) return rc;
  if (const int rc = launch_means(b, st, d_x, dim, W->mean)) return rc;
  TimedScope ts_(b.ctx, st, "mspf_kernel");
#define WM_MSPF_CASE(NN)                                                                                         \
  case NN:                                                                                                       \
    hipLaunchKernelGGL((mspf_kernel<NN>), dim3((unsigned)blocks), dim3(64), 0, st, d_x, a, b.d_f_off, W->mean, W->tab, \
                       d_out, W->flag, d_status);                                                                \
    break;
  switch (opt.fft_length) {
    WM_MSPF_CASE(16)
    WM_MSPF_CASE(32)
    WM_MSPF_CASE(64)
  }
#undef WM_MSPF_CASE
  const int64_t n = b.total_f * dim;
  hipLaunchKernelGGL(mspf_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W->flag, b.d_frame_utt, dim, n,
                     d_out);
  return wm_check(hipGetLastError());
}

int launch_mspf_stats(Batch& b, hipStream_t st, const double* d_x, int dim, const WorldMi355MspfOption& opt,
                      const double* d_mean, double* d_sum, double* d_sumsq, int64_t* n_frames) {
  if (const int rc = check_mspf_stats(d_x, dim, &opt, d_sum, d_sumsq, n_frames)) return rc;
  const int K = opt.fft_length / 2 + 1, S = (opt.frame_length - 1) / 2;
  int64_t frames = 0;
  for (int u = 0; u < b.n_utt; ++u)
    if (b.f0_len[u] > 0) frames += (b.f0_len[u] + S + S - 1) / S;
  *n_frames = frames;
  if (b.n_utt <= 0 || b.total_f <= 0) {                              // nothing to add: the sums are zeros
    if (const int rc = wm_check(hipMemsetAsync(d_sum, 0, sizeof(double) * (size_t)K * dim, st))) return rc;
    return wm_check(hipMemsetAsync(d_sumsq, 0, sizeof(double) * (size_t)K * dim, st));
  }
  MspfArgs a;
  mspf_args(opt, dim, b.max_f0_len, &a);
  const int64_t blocks = (int64_t)b.n_utt * a.chunks;
  if (blocks > (int64_t)1 << 30) return WM_ERR_BAD_ARG;
  const int64_t need[4] = {d_mean == nullptr ? (int64_t)b.n_utt * dim : 0, 0, (int64_t)b.n_utt * 2 * K * dim, 0};
  MspfWs* W = nullptr;
  if (const int rc = mspf_ws(b, st, need, &W)) return rc;
  if (d_mean == nullptr) {
    if (const int rc = launch_means(b, st, d_x, dim, W->mean)) return rc;
    d_mean = W->mean;
  }
  TimedScope ts_(b.ctx, st, "mspf_stats_kernel");
#define WM_MSPF_CASE(NN)                                                                                         \
  case NN:                                                                                                       \
    hipLaunchKernelGGL((mspf_stats_kernel<NN>), dim3((unsigned)blocks), dim3(64), 0, st, d_x, a, b.d_f_off, d_mean,  \
                       W->part);                                                                                 \
    break;
  switch (opt.fft_length) {
    WM_MSPF_CASE(16)
    WM_MSPF_CASE(32)
    WM_MSPF_CASE(64)
  }
#undef WM_MSPF_CASE
  hipLaunchKernelGGL(mspf_stats_add_kernel, dim3((unsigned)((K * dim + 255) / 256)), dim3(256), 0, st, W->part, b.n_utt, dim,
                     K, d_sum, d_sumsq);
  return wm_check(hipGetLastError());
}

int mspf_segment_frames() { return kMspfSegment; }

}  // namespace wm
