// mlsa.hip -- waveforms from mel-cepstra: SPTK's `excite | dfs | vopr -a | mglsadf` as gen_wave's first branch drives them
// (scripts/Training.pl:2873-2899), by the definition in include/world_mi355.h (SPTK is not in the reference tree; parity
// with it is unpinned, tests/mlsa_reference.py states the definition in float64).
//
//   mlsa_walk_kernel    one thread per utterance: excite's pulse walk, which is sequential per sample; writes excite's
//                       output x (pulses, zeros, and g in the unvoiced frames) and flags a bad pitch
//   mlsa_b_kernel       one thread per frame: b = mc2b(mc) in the definition's order and bits, flags a bad coefficient
//   mlsa_fir_kernel     WorldMi355MlsaExcitation's e = dfs(lowpass, x) + dfs(highpass, g), one thread per sample
//   mlsa_filter_kernel  one wavefront per utterance, longest utterance first.  The filter is strictly sequential in time;
//                       its parallelism is along the all-pass chain and across the Pade stages.  Lane k holds b[k], its
//                       increment and, per stage, the chain's state d[k] -- all in registers.  mlsafir's inner loop is
//                       the first-order recurrence d'[k] = u[k] - alpha d'[k-1] along k, u[1] = aa x + alpha d[1],
//                       u[k] = d[k] + alpha d[k+1]: a weighted inclusive scan over the wave, six DPP steps with the
//                       weights (-alpha)^distance.  The lanes keep d' unshifted (d[k] of the next sample is d'[k-1]), so
//                       the shift is the one wave_shr that builds u.  The pd stages of a sample read the previous
//                       sample's pt2, so their scans are independent and interleave; their dot products with b are taken
//                       four at a time (wave_sum4).  Samples are staged 64 at a time with lanes as samples (the FIRs of
//                       the fused form, the loads of the other), handed over by v_readlane and stored 64 at a time.
// No LDS, no atomics.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#include "batch.hpp"
#include "common.hpp"

namespace wm {

namespace {
constexpr int kMlsaMaxTaps = 256;
constexpr int kMlsaMaxOrder = 62;
constexpr int kMlsaMaxPade = 7;

// nrandom at seed 1: the first n values of g
void noise_fill(double* out, int64_t n) {
  uint32_t next = 1;
  auto rnd = [&next]() {
    next = next * 1103515245u + 12345u;
    return (double)((next / 65536u) % 32768u) / 32767.0;
  };
  for (int64_t i = 0; i < n; i += 2) {
    double r1, r2, s;
    do {
      r1 = 2.0 * rnd() - 1.0;
      r2 = 2.0 * rnd() - 1.0;
      s = r1 * r1 + r2 * r2;
    } while (s > 1.0 || s == 0.0);
    s = sqrt(-2.0 * log(s) / s);
    out[i] = r1 * s;
    if (i + 1 < n) out[i + 1] = r2 * s;
  }
}
}  // namespace

int mlsa_samples(int n_frames, int frame_shift, int* n_samples) {
  if (!n_samples || n_frames < 2 || frame_shift < 1) return WM_ERR_BAD_ARG;
  const int64_t n = (int64_t)(n_frames - 1) * frame_shift;
  if (n > (int64_t)INT32_MAX) return WM_ERR_BAD_ARG;
  *n_samples = (int)n;
  return WM_OK;
}

int mlsa_pade(int order, double* row) {
  if (!row || order < 1 || order > kMlsaMaxPade) return WM_ERR_BAD_ARG;
  static const double p4[5] = {1.0, 0.4999273, 0.1067005, 0.01170221, 0.0005656279};
  static const double p5[6] = {1.0, 0.4999391, 0.1107098, 0.01369984, 0.0009564853, 0.00003041721};
  if (order == 4 || order == 5) {
    for (int k = 0; k <= order; ++k) row[k] = order == 4 ? p4[k] : p5[k];
    return WM_OK;
  }
  // L! (2L-k)! / ((2L)! k! (L-k)!) = [L (L-1) .. (L-k+1)] / [k! 2L (2L-1) .. (2L-k+1)]: both integers below 2^53,
  // one division: the double nearest to the rational
  const int L = order;
  for (int k = 0; k <= L; ++k) {
    double num = 1.0, den = 1.0;
    for (int i = 0; i < k; ++i) {
      num *= (double)(L - i);
      den *= (double)(i + 1) * (double)(2 * L - i);
    }
    row[k] = num / den;
  }
  return WM_OK;
}

int mlsa_noise(int64_t n, double* out) {
  if (n < 0 || (!out && n > 0)) return WM_ERR_BAD_ARG;
  noise_fill(out, n);
  return WM_OK;
}

// What the three calls refuse, on the host alone.  mode: 1 excitation, 2 filter, 3 both (synthesis).
int check_mlsa(const Batch& b, int mode, const void* pitch, const void* mc, const double* lowpass, int n_low,
               const double* highpass, int n_high, const WorldMi355MlsaOption* opt, const void* e, const void* y) {
  if (!opt) return WM_ERR_BAD_ARG;
  if (opt->frame_shift < 1) return WM_ERR_BAD_ARG;
  if (mode & 1) {
    if (!pitch || !lowpass || !highpass) return WM_ERR_BAD_ARG;
    if (n_low < 1 || n_low > kMlsaMaxTaps || n_high < 1 || n_high > kMlsaMaxTaps) return WM_ERR_BAD_ARG;
    for (int k = 0; k < n_low; ++k)
      if (!(fabs(lowpass[k]) < HUGE_VAL)) return WM_ERR_BAD_ARG;
    for (int k = 0; k < n_high; ++k)
      if (!(fabs(highpass[k]) < HUGE_VAL)) return WM_ERR_BAD_ARG;
  }
  if (mode & 2) {
    if (!mc || !y) return WM_ERR_BAD_ARG;
    if (opt->order < 1 || opt->order > kMlsaMaxOrder || opt->pade_order < 1 || opt->pade_order > kMlsaMaxPade)
      return WM_ERR_BAD_ARG;
    if (!(fabs(opt->alpha) < 1.0)) return WM_ERR_BAD_ARG;
    if (opt->use_pade)
      for (int k = 0; k <= opt->pade_order; ++k)
        if (!(fabs(opt->pade[k]) < HUGE_VAL)) return WM_ERR_BAD_ARG;
  }
  if (mode != 3 && !e) return WM_ERR_BAD_ARG;
  for (int u = 0; u < b.n_utt; ++u) {
    int n = 0;
    if (mlsa_samples(b.f0_len[u], opt->frame_shift, &n) || n != b.y_len[u]) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

namespace {

// excite -n -p P at interpolation period 1, one thread per utterance
__global__ __launch_bounds__(64) void mlsa_walk_kernel(const float* __restrict__ pitch, const int64_t* __restrict__ f_off,
                                                       const int64_t* __restrict__ y_off, int n_utt, int P, int f32,
                                                       const double* __restrict__ g, double* __restrict__ x,
                                                       int* __restrict__ flag) {
#pragma clang fp contract(off)
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= n_utt) return;
  const float* pt = pitch + f_off[u];
  const int T = (int)(f_off[u + 1] - f_off[u]);
  double* xo = x + y_off[u];
  bool bad = false;
  for (int f = 0; f < T; ++f) {
    const float v = pt[f];
    if (!(v >= 0.0f) || v > 3.0e38f) bad = true;          // NaN, negative, +inf
  }
  if (bad) {
    flag[u] = 1;                                          // the sample kernels write the zeros
    return;
  }
  double p1 = (double)pt[0], cnt = p1;
  int64_t used = 0, n = 0;
  for (int f = 1; f < T; ++f) {
    const double p2 = (double)pt[f];
    double inc;
    if (p1 != 0.0 && p2 != 0.0) {
      inc = (p2 - p1) / (double)P;
    } else {
      inc = 0.0;
      cnt = p2;
      p1 = 0.0;
    }
    for (int i = 0; i < P; ++i) {
      double v;
      if (p1 == 0.0) {
        v = g[used++];
      } else {
        cnt += 1.0;
        if (cnt >= p1) {
          v = sqrt(p1);
          cnt -= p1;
        } else {
          v = 0.0;
        }
      }
      p1 += inc;
      xo[n++] = f32 ? (double)(float)v : v;
    }
    p1 = p2;
  }
}

// b = mc2b(mc), one thread per frame
__global__ __launch_bounds__(256) void mlsa_b_kernel(const float* __restrict__ mc, const int* __restrict__ frame_utt,
                                                     int64_t total_f, int m, double alpha, double* __restrict__ bco,
                                                     int* __restrict__ flag) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= total_f) return;
  const float* c = mc + f * (m + 1);
  double* bo = bco + f * (m + 1);
  double bn = (double)c[m];
  bool bad = !(fabs(bn) < HUGE_VAL);
  bo[m] = bn;
  for (int i = m - 1; i >= 0; --i) {
    const double v = (double)c[i];
    bad = bad || !(fabs(v) < HUGE_VAL);
    bn = v - alpha * bn;
    bo[i] = bn;
  }
  if (bad) flag[frame_utt[f]] = 1;
}

// e[n] of one utterance: x and g are the utterance's excite output and the noise, lp / hp the taps (wave-uniform loads)
__device__ __forceinline__ double mlsa_e_at(const double* __restrict__ x, const double* __restrict__ g,
                                            const double* __restrict__ lp, int nl, const double* __restrict__ hp, int nh,
                                            int n, int f32) {
  double lo = 0.0, hi = 0.0;
  const int kl = imin(nl - 1, n), kh = imin(nh - 1, n);
  for (int k = 0; k <= kl; ++k) lo = __builtin_fma(lp[k], x[n - k], lo);
  for (int k = 0; k <= kh; ++k) {
    const double gv = g[n - k];
    hi = __builtin_fma(hp[k], f32 ? (double)(float)gv : gv, hi);
  }
  if (f32) {
    lo = (double)(float)lo;
    hi = (double)(float)hi;
  }
  const double e = lo + hi;
  return f32 ? (double)(float)e : e;
}

__global__ __launch_bounds__(256) void mlsa_fir_kernel(const double* __restrict__ x, const double* __restrict__ g,
                                                       const double* __restrict__ taps, int nl, int nh,
                                                       const int64_t* __restrict__ y_off, const int* __restrict__ flag,
                                                       int f32, double* __restrict__ e) {
  const int u = blockIdx.x;
  const int64_t y0 = y_off[u];
  const int N = (int)(y_off[u + 1] - y0);
  const bool zero = flag[u] != 0;
  for (int n = blockIdx.y * 256 + threadIdx.x; n < N; n += 256 * gridDim.y)
    e[y0 + n] = zero ? 0.0 : mlsa_e_at(x + y0, g, taps, nl, taps + kMlsaMaxTaps, nh, n, f32);
}

struct MlsaArgs {
  const double* e;         // the excitation (the two-call form), or
  const double* x;         // excite's output with
  const double* g;
  const double* taps;      // [2][kMlsaMaxTaps]
  int nl, nh;
  const double* bco;       // [total_f][m + 1]
  const int64_t* f_off;
  const int64_t* y_off;
  const int* order;        // utterances, longest first
  const int* flag;
  double* y;
  int* status;
  int m, P, f32;
  double alpha;
  double pp[kMlsaMaxPade + 1];
};

// the weighted inclusive scan v[k] <- sum_{j <= k} w^(k - j) v[j] over the wave
__device__ __forceinline__ double mlsa_scan(double v, double w1, double w2, double w4, double w8, double w15, double w31) {
  v = __builtin_fma(w1, dpp_get<0x111, 0xf, 0xf>(v), v);      // row_shr:1
  v = __builtin_fma(w2, dpp_get<0x112, 0xf, 0xf>(v), v);      // row_shr:2
  v = __builtin_fma(w4, dpp_get<0x114, 0xf, 0xf>(v), v);      // row_shr:4
  v = __builtin_fma(w8, dpp_get<0x118, 0xf, 0xf>(v), v);      // row_shr:8
  v = __builtin_fma(w15, dpp_get<0x142, 0xa, 0xf>(v), v);     // row_bcast:15 -> rows 1, 3
  v = __builtin_fma(w31, dpp_get<0x143, 0xc, 0xf>(v), v);     // row_bcast:31 -> rows 2, 3
  return v;
}

template <int PD, bool FUSED>
__global__ __launch_bounds__(64) void mlsa_filter_kernel(const MlsaArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int u = a.order[blockIdx.x];
  const int64_t f0 = a.f_off[u], y0 = a.y_off[u];
  const int T = (int)(a.f_off[u + 1] - f0);
  const int N = (int)(a.y_off[u + 1] - y0);
  double* yo = a.y + y0;
  if (a.flag[u] != 0) {
    for (int n = lane; n < N; n += 64) yo[n] = 0.0;
    if (a.status != nullptr && lane == 0) a.status[u] = 1;
    return;
  }
  const int m = a.m, P = a.P, m1 = m + 1;
  const double alpha = a.alpha, aa = 1.0 - alpha * alpha;
  const double w1 = -alpha, w2 = w1 * w1, w4 = w2 * w2, w8 = w4 * w4;
  double w15 = 1.0, w31 = 1.0;                                // (-alpha)^(lane in row + 1), (-alpha)^(lane - 31)
  for (int i = 0; i < (lane & 15) + 1; ++i) w15 *= w1;
  for (int i = 0; i < lane - 31; ++i) w31 *= w1;
  const bool in_chain = lane >= 1 && lane <= m, in_sum = lane >= 2 && lane <= m;
  const double* bf = a.bco + f0 * m1;
  double b = lane <= m ? bf[lane] : 0.0;
  double b_next = lane <= m ? bf[m1 + lane] : 0.0;
  double inc = (b_next - b) / (double)P;
  double s[PD], d1[PD + 1], pt1[PD + 1], pt2[PD + 1];
#pragma unroll
  for (int i = 0; i < PD; ++i) s[i] = 0.0;
#pragma unroll
  for (int i = 0; i <= PD; ++i) d1[i] = pt1[i] = pt2[i] = 0.0;
  int frame = 0, in_frame = 0;
  bool bad_out = false;
  for (int n0 = 0; n0 < N; n0 += 64) {
    const int n = n0 + lane;
    double eb = 0.0;
    if (n < N) {
      if (FUSED)
        eb = mlsa_e_at(a.x + y0, a.g, a.taps, a.nl, a.taps + kMlsaMaxTaps, a.nh, n, a.f32);
      else
        eb = a.e[y0 + n];
    }
    double yb = 0.0;
    const int cnt = imin(64, N - n0);
    for (int j = 0; j < cnt; ++j) {
      double x = readlane_d(eb, j);
      const double b0 = readlane_d(b, 0), b1 = readlane_d(b, 1);
      x = x * exp(b0);
      double out = 0.0;
#pragma unroll
      for (int i = PD; i >= 1; --i) {                         // mlsadf1
        d1[i] = aa * pt1[i - 1] + alpha * d1[i];
        pt1[i] = d1[i] * b1;
        const double v = pt1[i] * a.pp[i];
        x += (i & 1) ? v : -v;
        out += v;
      }
      pt1[0] = x;
      out += x;
      x = out;
      double part[(PD + 3) / 4 * 4];
#pragma unroll
      for (int i = 0; i < (PD + 3) / 4 * 4; ++i) part[i] = 0.0;
#pragma unroll
      for (int i = 1; i <= PD; ++i) {                         // the PD all-pass chains, each fed by the previous sample's pt2
        const double below = dpp_get<0x138, 0xf, 0xf>(s[i - 1]);        // wave_shr:1
        double uu = (lane == 1 ? aa * pt2[i - 1] : below) + alpha * s[i - 1];
        uu = in_chain ? uu : 0.0;
        uu = mlsa_scan(uu, w1, w2, w4, w8, w15, w31);
        s[i - 1] = uu;
        part[i - 1] = in_sum ? uu * b : 0.0;
      }
#pragma unroll
      for (int q = 0; q < (PD + 3) / 4; ++q) wave_sum4(part[4 * q], part[4 * q + 1], part[4 * q + 2], part[4 * q + 3]);
      out = 0.0;
#pragma unroll
      for (int i = PD; i >= 1; --i) {                         // mlsadf2
        pt2[i] = part[i - 1];
        const double v = pt2[i] * a.pp[i];
        x += (i & 1) ? v : -v;
        out += v;
      }
      pt2[0] = x;
      out += x;
      if (a.f32) out = (double)(float)out;
      yb = lane == j ? out : yb;
      if (++in_frame == P) {                                  // b = b_next exactly, and the next frame's increments
        in_frame = 0;
        ++frame;
        b = b_next;
        if (frame + 1 < T) {
          b_next = lane <= m ? bf[(int64_t)(frame + 1) * m1 + lane] : 0.0;
          inc = (b_next - b) / (double)P;
        } else {
          inc = 0.0;
        }
      } else {
        b += inc;
      }
    }
    if (n < N) {
      yo[n] = yb;
      bad_out = bad_out || !(fabs(yb) < HUGE_VAL);
    }
  }
  const bool any = __ballot(bad_out) != 0;
  if (a.status != nullptr && lane == 0) a.status[u] = any ? 2 : 0;
}

struct MlsaNoiseWs : StageWs {
  double* g = nullptr;
  int64_t cap = 0;
  std::vector<double> h;                                      // the table as uploaded: the copy's source
};

struct MlsaWs : StageWs {
  double* bco = nullptr;                                      // b of every frame
  double* x = nullptr;                                        // excite's output
  double* taps = nullptr;                                     // [2][kMlsaMaxTaps]
  int* flag = nullptr;                                        // [n_utt]: a bad pitch or coefficient
  int* order = nullptr;                                       // [n_utt]: longest first
  int64_t bco_cap = 0, x_cap = 0;                             // in doubles
  std::vector<int> h_order;
};

// the first `count` values of g on the device: made once per context, grown on demand by grow_ws' rule
int ensure_noise(Context& c, hipStream_t st, int64_t count, const double*& g) {
  MlsaNoiseWs* W = nullptr;
  int64_t cap = count + count / 4 + 4096;
  if (c.mlsa_noise) cap = std::max(cap, 2 * static_cast<const MlsaNoiseWs&>(*c.mlsa_noise).cap);
  const int rc = grow_ws(c.mlsa_noise, st, W, [&](const MlsaNoiseWs& w) { return w.cap >= count; }, [&](MlsaNoiseWs& n) {
    n.h.resize((size_t)cap);
    noise_fill(n.h.data(), cap);
    if (const int rc2 = wm_check(n.alloc(&n.g, sizeof(double) * (size_t)cap))) return rc2;
    n.cap = cap;
    return wm_check(hipMemcpyAsync(n.g, n.h.data(), sizeof(double) * (size_t)cap, hipMemcpyHostToDevice, st));
  });
  if (rc) return rc;
  g = W->g;
  return WM_OK;
}

int ensure_ws(Batch& b, hipStream_t st, int64_t need_b, int64_t need_x, MlsaWs*& W) {
  if (b.mlsa) {                                               // a rebuilt workspace serves the earlier calls' sizes too
    const MlsaWs& old = static_cast<const MlsaWs&>(*b.mlsa);
    need_b = std::max(need_b, old.bco_cap);
    need_x = std::max(need_x, old.x_cap);
  }
  const int rc = grow_ws(b.mlsa, st, W, [&](const MlsaWs& w) { return w.bco_cap >= need_b && w.x_cap >= need_x; },
                         [&](MlsaWs& n) {
                           n.bco_cap = need_b;
                           n.x_cap = need_x;
                           if (const int r = wm_check(n.alloc(&n.bco, sizeof(double) * (size_t)(need_b ? need_b : 1)))) return r;
                           if (const int r = wm_check(n.alloc(&n.x, sizeof(double) * (size_t)(need_x ? need_x : 1)))) return r;
                           if (const int r = wm_check(n.alloc(&n.taps, sizeof(double) * 2 * kMlsaMaxTaps))) return r;
                           if (const int r = wm_check(n.alloc(&n.flag, sizeof(int) * (size_t)b.n_utt))) return r;
                           if (const int r = wm_check(n.alloc(&n.order, sizeof(int) * (size_t)b.n_utt))) return r;
                           n.h_order.resize((size_t)b.n_utt);
                           std::iota(n.h_order.begin(), n.h_order.end(), 0);
                           std::stable_sort(n.h_order.begin(), n.h_order.end(),
                                            [&](int p, int q) { return b.y_len[p] > b.y_len[q]; });
                           return wm_check(hipMemcpyAsync(n.order, n.h_order.data(), sizeof(int) * (size_t)b.n_utt,
                                                          hipMemcpyHostToDevice, st));
                         });
  if (rc) return rc;
  return wm_check(hipMemsetAsync(W->flag, 0, sizeof(int) * (size_t)b.n_utt, st));
}

// The taps travel as kernel arguments, 128 at a time: no host block has to outlive the call, and nothing waits for the
// stream (a copy from pageable memory would).
struct MlsaChunk {
  double v[128];
};
__global__ __launch_bounds__(128) void mlsa_put_kernel(const MlsaChunk c, int n, double* __restrict__ dst) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

int upload_taps(MlsaWs& W, hipStream_t st, const double* lowpass, int n_low, const double* highpass, int n_high) {
  for (int set = 0; set < 2; ++set) {
    const double* src = set ? highpass : lowpass;
    const int n = set ? n_high : n_low;
    for (int at = 0; at < n; at += 128) {
      MlsaChunk c;
      const int k = imin(128, n - at);
      memset(&c, 0, sizeof(c));
      memcpy(c.v, src + at, sizeof(double) * (size_t)k);
      hipLaunchKernelGGL(mlsa_put_kernel, dim3(1), dim3(128), 0, st, c, k, W.taps + set * kMlsaMaxTaps + at);
    }
  }
  return wm_check(hipGetLastError());
}

int queue_walk(Batch& b, hipStream_t st, const float* d_pitch, const WorldMi355MlsaOption& opt, const double* g, MlsaWs& W) {
  hipLaunchKernelGGL(mlsa_walk_kernel, dim3((unsigned)((b.n_utt + 63) / 64)), dim3(64), 0, st, d_pitch, b.d_f_off, b.d_y_off,
                     b.n_utt, opt.frame_shift, opt.pipe_float32 ? 1 : 0, g, W.x, W.flag);
  return wm_check(hipGetLastError());
}

int queue_filter(Batch& b, hipStream_t st, bool fused, const double* d_e, const double* g, int n_low, int n_high,
                 const float* d_mc, const WorldMi355MlsaOption& opt, MlsaWs& W, double* d_y, int* d_status) {
  const int m = opt.order;
  hipLaunchKernelGGL(mlsa_b_kernel, dim3((unsigned)((b.total_f + 255) / 256)), dim3(256), 0, st, d_mc, b.d_frame_utt,
                     b.total_f, m, opt.alpha, W.bco, W.flag);
  if (const int rc = wm_check(hipGetLastError())) return rc;
  MlsaArgs a;
  memset(&a, 0, sizeof(a));
  a.e = d_e;
  a.x = W.x;
  a.g = g;
  a.taps = W.taps;
  a.nl = n_low;
  a.nh = n_high;
  a.bco = W.bco;
  a.f_off = b.d_f_off;
  a.y_off = b.d_y_off;
  a.order = W.order;
  a.flag = W.flag;
  a.y = d_y;
  a.status = d_status;
  a.m = m;
  a.P = opt.frame_shift;
  a.f32 = opt.pipe_float32 ? 1 : 0;
  a.alpha = opt.alpha;
  if (opt.use_pade) {
    for (int k = 0; k <= opt.pade_order; ++k) a.pp[k] = opt.pade[k];
  } else if (const int rc = mlsa_pade(opt.pade_order, a.pp)) {
    return rc;
  }
  TimedScope ts_(b.ctx, st, "mlsa_kernel");
  const dim3 grid((unsigned)b.n_utt), block(64);
#define WM_MLSA_CASE(PD)                                                                   \
  case PD:                                                                                 \
    if (fused)                                                                             \
      hipLaunchKernelGGL((mlsa_filter_kernel<PD, true>), grid, block, 0, st, a);           \
    else                                                                                   \
      hipLaunchKernelGGL((mlsa_filter_kernel<PD, false>), grid, block, 0, st, a);          \
    break;
  switch (opt.pade_order) {
    WM_MLSA_CASE(1)
    WM_MLSA_CASE(2)
    WM_MLSA_CASE(3)
    WM_MLSA_CASE(4)
    WM_MLSA_CASE(5)
    WM_MLSA_CASE(6)
    WM_MLSA_CASE(7)
  }
#undef WM_MLSA_CASE
  return wm_check(hipGetLastError());
}

}  // namespace

int launch_mlsa_excitation(Batch& b, hipStream_t st, const float* d_pitch, const double* lowpass, int n_low,
                           const double* highpass, int n_high, const WorldMi355MlsaOption& opt, double* d_e) {
  if (const int rc = check_mlsa(b, 1, d_pitch, nullptr, lowpass, n_low, highpass, n_high, &opt, d_e, nullptr)) return rc;
  const double* g = nullptr;
  if (const int rc = ensure_noise(*b.ctx, st, b.max_y_len, g)) return rc;
  MlsaWs* W = nullptr;
  if (const int rc = ensure_ws(b, st, 0, b.total_y, W)) return rc;
  if (const int rc = upload_taps(*W, st, lowpass, n_low, highpass, n_high)) return rc;
  if (const int rc = queue_walk(b, st, d_pitch, opt, g, *W)) return rc;
  const int parts = imax(1, imin(64, (b.max_y_len + 4095) / 4096));
  hipLaunchKernelGGL(mlsa_fir_kernel, dim3((unsigned)b.n_utt, (unsigned)parts), dim3(256), 0, st, W->x, g, W->taps, n_low,
                     n_high, b.d_y_off, W->flag, opt.pipe_float32 ? 1 : 0, d_e);
  return wm_check(hipGetLastError());
}

int launch_mlsa_filter(Batch& b, hipStream_t st, const double* d_e, const float* d_mc, const WorldMi355MlsaOption& opt,
                       double* d_y, int* d_status) {
  if (const int rc = check_mlsa(b, 2, nullptr, d_mc, nullptr, 0, nullptr, 0, &opt, d_e, d_y)) return rc;
  MlsaWs* W = nullptr;
  if (const int rc = ensure_ws(b, st, b.total_f * (opt.order + 1), 0, W)) return rc;
  return queue_filter(b, st, false, d_e, nullptr, 0, 0, d_mc, opt, *W, d_y, d_status);
}

int launch_mlsa_synthesis(Batch& b, hipStream_t st, const float* d_pitch, const float* d_mc, const double* lowpass,
                          int n_low, const double* highpass, int n_high, const WorldMi355MlsaOption& opt, double* d_y,
                          int* d_status) {
  if (const int rc = check_mlsa(b, 3, d_pitch, d_mc, lowpass, n_low, highpass, n_high, &opt, nullptr, d_y)) return rc;
  const double* g = nullptr;
  if (const int rc = ensure_noise(*b.ctx, st, b.max_y_len, g)) return rc;
  MlsaWs* W = nullptr;
  if (const int rc = ensure_ws(b, st, b.total_f * (opt.order + 1), b.total_y, W)) return rc;
  if (const int rc = upload_taps(*W, st, lowpass, n_low, highpass, n_high)) return rc;
  if (const int rc = queue_walk(b, st, d_pitch, opt, g, *W)) return rc;
  return queue_filter(b, st, true, nullptr, g, n_low, n_high, d_mc, opt, *W, d_y, d_status);
}

}  // namespace wm
