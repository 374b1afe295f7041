// lsp.hip -- MGC-LSP rows to LPC and MGC rows, and the recipe's LSP postfilter, on the device.
//
// With GAMMA != 0 the recipe's `mgc` stream holds MGC-LSP rows [gain, lsp_1 .. lsp_m] (data/Makefile.in:138-146, 186-192).
// gen_wave and postfiltering_lsp (scripts/Training.pl:2690-2752, :2846-2868) take them back by
//   lspcheck -c -r 0.1 -g -G 1e-10 | lsp2lpc | mgc2mgc -n -u
// SPTK's lspcheck and lsp2lpc are not in the reference tree: PARITY WITH SPTK'S COMMANDS IS UNPINNED.  The yardstick is
// the definition in include/world_mi355.h, which tests/lsp_reference.py states in float64.  For one row x[0 .. m],
// w[i] = x[i], r = min_distance, G = min_gain, d = r pi / (m + 1) (rounded on the host in that expression):
//
//   check     range: w <- |w|, then w <- 2 pi - w where w > pi.  order: sorted ascending.  distance: ONE pass,
//             i = 1 .. m-1 ascending on the values the steps before left: t = w[i+1] - w[i]; t < d: s = 0.5 (d - t),
//             w[i] -= s, w[i+1] += s.  gain: K = exp(x[0]) under log_gain, else x[0]; K < G: K <- G and the checked row's
//             gain is log(G) (rounded on the host) or G; otherwise the gain keeps its bits.  Plain expressions, no
//             contraction: the checked LSPs are the restatement's bits.
//   status    1 a range, order or distance step changed a value, 2 the gain was raised, 4 a non-finite input value (zeros),
//             8 a non-finite result (zeros), 16 the checked LSPs are not strictly increasing inside (0, pi).
//   lsp2lpc   A = (P + Q) / 2, f_i(z) = 1 - 2 cos(w[i]) z^-1 + z^-2, P the f_i of odd i, Q of even i; even m: P (1 + z^-1),
//             Q (1 - z^-1); odd m: Q (1 - z^-2).  Row [K, a_1 .. a_m].  ORDER OF THE PRODUCTS: both start from 1; the
//             quadratic factors of P and of Q in turn, each polynomial's own in the bit-reversed order of their positions
//             (factor_order below), each c[k] <- (c[k] + p_i c[k-1]) + c[k-2] with p_i = -2 cos(w[i]) (the device
//             library's cos); then the further factor, c[k] +- c[k-1] or c[k] - c[k-2]; then 0.5 (P[k] + Q[k]).  In
//             ascending i the partial products -- roots on one arc of the circle -- grow to 1e4 at order 34 and 1e8 at
//             63, and P + Q, whose coefficients are of order 1, is then off by 5e-9 and 6e-2; in this order they stay
//             below 40 and the row is good to 2e-13 (tests/test_lsp_host.py measures both).
//   filter    postfiltering_lsp's :2709-2736 on the RAW row: i = 2 .. m-1, d1 = beta (w[i+1] - w[i]),
//             d2 = beta (w[i] - w[i-1]), p[i] = w[i-1] + d2 + (d2 d2 ((w[i+1] - w[i-1]) - (d1 + d2))) / ((d2 d2) + (d1 d1)),
//             p[i] = w[i] where d1 == 0 and d2 == 0, the ends as they are.  The script reads the values through
//             `x2x +fa`'s text; that rounding is not modelled.
//
// lsp_kernel: one 64-lane wave per row (m + 1 <= 64), persistent over the batch's rows; lane k holds x[k], later
// coefficient k of P and of Q.  The filter step and the range step are lane-parallel with the neighbours taken by
// ds_bpermute; the order step is a rank sort (m wave-uniform broadcasts, every lane counts the values before its own) and
// one 64-double LDS row to put each value at its rank; the distance pass is the one sequential chain, m - 1 steps on
// broadcast pairs; a quadratic factor is one step with two one-lane DPP shifts (wave_shr:1, lane 0 reads 0), m steps in
// all.  The alternative, a lane per row with the order as a template parameter, keeps x, P and Q of a row in one lane:
// 3 (m + 1) doubles, 210 registers at the recipe's order 34 (two waves per SIMD) and 384 at 63 (one), where this form
// takes 30 at eight waves per SIMD ("MGC-LSP rows to MGC and the LSP postfilter").
//
// The postfilter (launch_lsp_postfilter) needs the energy 1/2 ln sum_{k < L} c2[k]^2 of the checked raw row and of the
// checked [gain, p], c2 = mgc2mgc -n -u towards (L - 1, 0, 1): two lsp_kernel launches leave two LPC rows per frame in the
// stage's workspace, mgc2mgc_kernel's energy form (mgc2mgc.hip) turns each into one double, lsp_gain_kernel puts
// ene1 - ene2 into the gain.  No row of L coefficients exists anywhere.
#include <math.h>

#include "batch.hpp"
#include "common.hpp"

namespace wm {

struct LspArgs {
  double d;                    // the least distance, r pi / (m + 1)
  double min_gain, floor_gain; // G, and the checked row's gain where it is raised: log(G) under log_gain, else G
  double beta;
  int m, log_gain;
  int filter;                  // the filter step first: the rest works on [gain, p]
  int convert;                 // check and lsp2lpc
  int status_or;               // or the bits into status[] instead of writing them (the second launch of the postfilter)
  unsigned char order[64];     // the i of lsp2lpc's quadratic factors in the order they are taken (factor_order)
};

// filtered: the rows [gain, p] (with `filter`), may be lsp itself; lpc, checked: NULL or rows of their own
__global__ __launch_bounds__(64) void lsp_kernel(const double* lsp, LspArgs o, int64_t total_rows, double* filtered,
                                                 double* lpc, double* checked, int* status) {
  __shared__ double sorted[64];
  const int lane0 = threadIdx.x;
  const int m = o.m;
  for (int64_t row = blockIdx.x; row < total_rows; row += gridDim.x) {
    const int lane = opaque_lane(lane0);
    const int64_t at = row * (int64_t)(m + 1);
    const bool own = lane >= 1 && lane <= m;           // the lanes of w[1 .. m]
    const double x = lane <= m ? lsp[at + lane] : 0.0;
    int st = __ballot(!(fabs(x) < __builtin_inf())) == 0ull ? 0 : 4;
    const double gain = readlane_d(x, 0);
    double w = own ? x : 0.0;
    if (st == 0 && o.filter) {
#pragma clang fp contract(off)
      const double lo = __shfl(w, lane - 1), hi = __shfl(w, lane + 1);
      if (lane >= 2 && lane <= m - 1) {
        const double d1 = o.beta * (hi - w);
        const double d2 = o.beta * (w - lo);
        if (!(d1 == 0.0 && d2 == 0.0)) w = lo + d2 + (d2 * d2 * ((hi - lo) - (d1 + d2))) / ((d2 * d2) + (d1 * d1));
      }
      if (__ballot(!(fabs(w) < __builtin_inf())) != 0ull) st = 8;
    }
    if (filtered != nullptr && lane <= m) filtered[at + lane] = st != 0 ? 0.0 : (lane == 0 ? gain : w);
    double K = 0.0, cg = 0.0, a = 0.0;
    if (st == 0 && o.convert) {
      bool changed;
      {
#pragma clang fp contract(off)
        // ---- range
        const double w0 = w;
        w = fabs(w);
        if (w > kPi) w = 2.0 * kPi - w;
        changed = own && w != w0;
        // ---- order: the rank of a value is the number of values before it, equal ones in their given order
        int rank = 0;
        for (int j = 1; j <= m; ++j) {
          const double wj = readlane_d(w, j);
          rank += (wj < w || (wj == w && j < lane)) ? 1 : 0;
        }
        wave_sync();
        if (own) sorted[rank + 1] = w;
        wave_sync();
        const double ws = own ? sorted[lane] : 0.0;
        changed = changed || ws != w;
        w = ws;
        // ---- distance: one pass
        const double wd = w;
        for (int i = 1; i < m; ++i) {
          const double lo = readlane_d(w, i), hi = readlane_d(w, i + 1);
          const double t = hi - lo;
          if (t < o.d) {
            const double s = 0.5 * (o.d - t);
            if (lane == i) w = lo - s;
            if (lane == i + 1) w = hi + s;
          }
        }
        changed = changed || w != wd;
      }
      if (__ballot(changed) != 0ull) st |= 1;
      const double next = __shfl(w, lane + 1);
      if (__ballot(own && !(w > 0.0 && w < kPi && (lane == m || w < next))) != 0ull) st |= 16;
      // ---- gain
      K = o.log_gain ? uniform_d(exp(gain)) : gain;
      cg = gain;
      if (K < o.min_gain) {
        K = o.min_gain;
        cg = o.floor_gain;
        st |= 2;
      }
      // ---- lsp2lpc
      {
#pragma clang fp contract(off)
        const double pw = -2.0 * cos(w);
        double P = lane == 0 ? 1.0 : 0.0, Q = P;
        for (int t = 0; t < m; ++t) {
          const int i = o.order[t];
          const double pi = readlane_d(pw, i);
          if (i & 1) {
            const double s1 = dpp_get<0x138, 0xf, 0xf>(P);      // wave_shr:1 -- lane k reads lane k - 1, lane 0 reads 0
            const double s2 = dpp_get<0x138, 0xf, 0xf>(s1);
            P = (P + pi * s1) + s2;
          } else {
            const double s1 = dpp_get<0x138, 0xf, 0xf>(Q);
            const double s2 = dpp_get<0x138, 0xf, 0xf>(s1);
            Q = (Q + pi * s1) + s2;
          }
        }
        if (m & 1) {
          Q = Q - dpp_get<0x138, 0xf, 0xf>(dpp_get<0x138, 0xf, 0xf>(Q));
        } else {
          P = P + dpp_get<0x138, 0xf, 0xf>(P);
          Q = Q - dpp_get<0x138, 0xf, 0xf>(Q);
        }
        a = 0.5 * (P + Q);
      }
      const double v = lane == 0 ? K : (own ? a : 0.0);
      if (__ballot(!(fabs(v) < __builtin_inf())) != 0ull) st |= 8;
    }
    if (o.convert && lane <= m) {
      const bool zero = (st & 12) != 0;
      if (lpc != nullptr) lpc[at + lane] = zero ? 0.0 : (lane == 0 ? K : a);
      if (checked != nullptr) checked[at + lane] = zero ? 0.0 : (lane == 0 ? cg : w);
    }
    if (status != nullptr && lane == 0) status[row] = o.status_or ? (status[row] | st) : st;
  }
}

// beta == 1 or m <= 2: the rows as they are, status 0, energies (where asked for) 0
__global__ __launch_bounds__(256) void lsp_identity_kernel(const double* lsp, int64_t n, int64_t total_rows, double* out,
                                                           double* ene1, double* ene2, int* status) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    if (out != lsp) out[i] = lsp[i];
    if (i < total_rows) {
      if (ene1 != nullptr) ene1[i] = 0.0;
      if (ene2 != nullptr) ene2[i] = 0.0;
      status[i] = 0;
    }
  }
}

// WorldMi355LspToMelGeneralizedCepstrum: a row the conversion flags (its zeros are in place) is bit 8, unless the check
// had flagged it already
__global__ __launch_bounds__(256) void lsp_status_kernel(const int* converted, int64_t total_rows, int* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total_rows && converted[i] != 0 && (status[i] & 12) == 0) status[i] |= 8;
}

// The end of the postfilter, a lane per row: the two energies (NaN where the conversion flagged the row) into the
// caller's arrays and, with `compensation`, their difference into the gain
__global__ __launch_bounds__(256) void lsp_gain_kernel(const double* e1, const double* e2, int m, int log_gain,
                                                       int compensation, int64_t total_rows, double* out, double* ene1,
                                                       double* ene2, int* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total_rows) return;
  int st = status[i];
  double a = 0.0, b = 0.0;
  if ((st & 12) == 0) {
#pragma clang fp contract(off)
    a = e1[i];
    b = e2[i];
    double g = out[i * (int64_t)(m + 1)];
    if (compensation) g = log_gain ? g + (a - b) : g * exp(a - b);
    if (fabs(a) < __builtin_inf() && fabs(b) < __builtin_inf() && fabs(g) < __builtin_inf()) {
      if (compensation) out[i * (int64_t)(m + 1)] = g;
    } else {
      st |= 8;
    }
  }
  if ((st & 12) != 0) {
    a = b = 0.0;
    for (int k = 0; k <= m; ++k) out[i * (int64_t)(m + 1) + k] = 0.0;
    status[i] = st;
  }
  if (ene1 != nullptr) ene1[i] = a;
  if (ene2 != nullptr) ene2[i] = b;
}

namespace {

// [a, a + na) and [b, b + nb) share a byte
bool bytes_meet(const void* a, int64_t na, const void* b, int64_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

int check_lsp_option(int order, double alpha, double gamma, double r, double G) {
  if (order < 1 || order > 63) return WM_ERR_BAD_ARG;
  if (!(fabs(alpha) < 1.0) || !(gamma >= -1.0 && gamma < 0.0)) return WM_ERR_BAD_ARG;
  if (!(r >= 0.0 && r <= 1.0) || !(G > 0.0 && G < __builtin_inf())) return WM_ERR_BAD_ARG;
  return WM_OK;
}

// the stage's workspace: one block of doubles, grown by grow_ws' rule
struct LspWs : StageWs {
  double* d = nullptr;
  int64_t cap = 0;             // in doubles
};

int lsp_workspace(Batch& b, hipStream_t st, int64_t doubles, double** out) {
  LspWs* ws = nullptr;
  const int rc = grow_ws<LspWs>(
      b.lsp, st, ws, [&](const LspWs& w) { return w.cap >= doubles; },
      [&](LspWs& w) {
        if (const int e = wm_check(w.alloc(&w.d, sizeof(double) * (size_t)doubles))) return e;
        w.cap = doubles;
        return (int)WM_OK;
      });
  if (rc) return rc;
  *out = ws->d;
  return WM_OK;
}

// The order of lsp2lpc's quadratic factors: P's (odd i) and Q's (even i) in turn, each polynomial's own by the
// bit-reversed order of their positions (position j = 0, 1, ... among its factors in ascending i, sorted by the reversal
// of j's binary digits over ceil(log2 n) bits).
void factor_order(int m, unsigned char* out) {
  int seq[2][32], n[2] = {(m + 1) / 2, m / 2};
  for (int q = 0; q < 2; ++q) {
    int bits = 1, at = 0;
    while ((1 << bits) < n[q]) ++bits;
    for (int r = 0; r < (1 << bits); ++r) {            // ascending reversal = the positions in bit-reversed order
      int j = 0;
      for (int k = 0; k < bits; ++k) j |= ((r >> k) & 1) << (bits - 1 - k);
      if (j < n[q]) seq[q][at++] = 2 * j + 1 + q;
    }
  }
  int at = 0;
  for (int t = 0; t < n[0]; ++t) {
    out[at++] = (unsigned char)seq[0][t];
    if (t < n[1]) out[at++] = (unsigned char)seq[1][t];
  }
  for (; at < 64; ++at) out[at] = 0;
}

LspArgs lsp_args(int order, int log_gain, double r, double G) {
  LspArgs a;
  factor_order(order, a.order);
  {
#pragma clang fp contract(off)
    a.d = r * kPi / (order + 1);
  }
  a.min_gain = G;
  a.floor_gain = log_gain ? log(G) : G;
  a.beta = 1.0;
  a.m = order;
  a.log_gain = log_gain != 0;
  a.filter = 0;
  a.convert = 1;
  a.status_or = 0;
  return a;
}

void launch_rows(Batch& b, hipStream_t st, const double* d_lsp, const LspArgs& a, double* d_filtered, double* d_lpc,
                 double* d_checked, int* d_status) {
  const int64_t tf = b.total_f;
  // every row costs the same: the waves that are resident at once, as mcpf_kernel's launch
  const int64_t slots = persistent_grid(*b.ctx, lsp_kernel, 64, (int64_t)1 << 40);
  const int64_t per = imax(1, (int)(slots / imax(1, b.ctx->oversub)));
  hipLaunchKernelGGL(lsp_kernel, dim3((int)(tf < per ? tf : per)), dim3(64), 0, st, d_lsp, a, tf, d_filtered, d_lpc,
                     d_checked, d_status);
}

WorldMi355MgcConvertOption convert_option(int order, double alpha, double gamma, int out_order, double out_alpha,
                                          double out_gamma) {
  WorldMi355MgcConvertOption c;
  c.in_order = order;
  c.in_alpha = alpha;
  c.in_gamma = gamma;
  c.in_normalized = 1;
  c.in_multiplied = 1;
  c.out_order = out_order;
  c.out_alpha = out_alpha;
  c.out_gamma = out_gamma;
  c.out_normalized = 0;
  c.out_multiplied = 0;
  return c;
}

}  // namespace

// What WorldMi355LspToLpc refuses, on the host alone: no device call is made for a refused set.
int check_lsp(int64_t total_rows, const double* d_lsp, const WorldMi355LspOption* opt, const double* d_lpc,
              const double* d_checked) {
  if (!d_lsp || !opt || !d_lpc) return WM_ERR_BAD_ARG;
  if (const int rc = check_lsp_option(opt->order, opt->alpha, opt->gamma, opt->min_distance, opt->min_gain)) return rc;
  const int64_t n = total_rows > 0 ? total_rows * (opt->order + 1) * (int64_t)sizeof(double) : 0;
  if (bytes_meet(d_lsp, n, d_lpc, n) || bytes_meet(d_lsp, n, d_checked, n) || bytes_meet(d_lpc, n, d_checked, n))
    return WM_ERR_BAD_ARG;
  return WM_OK;
}

int launch_lsp_to_lpc(Batch& b, hipStream_t st, const double* d_lsp, const WorldMi355LspOption& opt, double* d_lpc,
                      double* d_checked, int* d_status) {
  if (const int rc = check_lsp(b.total_f, d_lsp, &opt, d_lpc, d_checked)) return rc;
  if (b.total_f <= 0) return WM_OK;
  TimedScope ts_(b.ctx, st, "lsp_kernel");
  launch_rows(b, st, d_lsp, lsp_args(opt.order, opt.log_gain, opt.min_distance, opt.min_gain), nullptr, d_lpc, d_checked,
              d_status);
  return wm_check(hipGetLastError());
}

int check_lsp_to_mgc(int64_t total_rows, const double* d_lsp, const WorldMi355LspOption* opt, int out_order,
                     double out_alpha, double out_gamma, const double* d_out, const int* d_status) {
  if (!d_lsp || !opt || !d_out || !d_status) return WM_ERR_BAD_ARG;
  if (const int rc = check_lsp_option(opt->order, opt->alpha, opt->gamma, opt->min_distance, opt->min_gain)) return rc;
  const WorldMi355MgcConvertOption c = convert_option(opt->order, opt->alpha, opt->gamma, out_order, out_alpha, out_gamma);
  if (const int rc = check_mgc2mgc(total_rows, d_lsp, &c, d_out)) return rc;
  const int64_t rows = total_rows > 0 ? total_rows : 0;
  const int64_t ns = rows * (int64_t)sizeof(int);
  if (bytes_meet(d_status, ns, d_lsp, rows * (opt->order + 1) * (int64_t)sizeof(double)) ||
      bytes_meet(d_status, ns, d_out, rows * (out_order + 1) * (int64_t)sizeof(double)))
    return WM_ERR_BAD_ARG;
  return WM_OK;
}

int launch_lsp_to_mgc(Batch& b, hipStream_t st, const double* d_lsp, const WorldMi355LspOption& opt, int out_order,
                      double out_alpha, double out_gamma, double* d_out, int* d_status) {
  const int64_t tf = b.total_f;
  if (const int rc = check_lsp_to_mgc(tf, d_lsp, &opt, out_order, out_alpha, out_gamma, d_out, d_status)) return rc;
  if (tf <= 0) return WM_OK;
  // the LPC rows, and the conversion's own status behind them
  double* d_lpc = nullptr;
  const int64_t row_doubles = tf * (opt.order + 1);
  if (const int rc = lsp_workspace(b, st, row_doubles + (tf + 1) / 2, &d_lpc)) return rc;
  int* d_converted = (int*)(d_lpc + row_doubles);
  {
    TimedScope ts_(b.ctx, st, "lsp_kernel");
    launch_rows(b, st, d_lsp, lsp_args(opt.order, opt.log_gain, opt.min_distance, opt.min_gain), nullptr, d_lpc, nullptr,
                d_status);
    if (const int rc = wm_check(hipGetLastError())) return rc;
  }
  const WorldMi355MgcConvertOption c = convert_option(opt.order, opt.alpha, opt.gamma, out_order, out_alpha, out_gamma);
  if (const int rc = launch_mgc2mgc(b, st, d_lpc, c, d_out, d_converted)) return rc;
  hipLaunchKernelGGL(lsp_status_kernel, dim3((unsigned)((tf + 255) / 256)), dim3(256), 0, st, d_converted, tf, d_status);
  return wm_check(hipGetLastError());
}

int check_lsp_postfilter(int64_t total_rows, const double* d_lsp, const WorldMi355LspPostfilterOption* opt,
                         const double* d_out, const double* d_ene1, const double* d_ene2, const int* d_status) {
  if (!d_lsp || !opt || !d_out || !d_status) return WM_ERR_BAD_ARG;
  if (const int rc = check_lsp_option(opt->order, opt->alpha, opt->gamma, opt->min_distance, opt->min_gain)) return rc;
  if (!(fabs(opt->beta) < __builtin_inf())) return WM_ERR_BAD_ARG;
  const int L = opt->length;
  if (L < 64 || L > 4096 || (L & (L - 1)) != 0) return WM_ERR_BAD_ARG;
  const int64_t rows = total_rows > 0 ? total_rows : 0;
  const int64_t n = rows * (opt->order + 1) * (int64_t)sizeof(double), ne = rows * (int64_t)sizeof(double);
  const int64_t ns = rows * (int64_t)sizeof(int);
  if (d_out != d_lsp && bytes_meet(d_lsp, n, d_out, n)) return WM_ERR_BAD_ARG;      // in place, or apart
  const void* p[5] = {d_lsp, d_out, d_ene1, d_ene2, d_status};
  const int64_t bytes[5] = {n, n, ne, ne, ns};
  for (int i = 0; i < 5; ++i)
    for (int j = i < 2 ? 2 : i + 1; j < 5; ++j)
      if (bytes_meet(p[i], bytes[i], p[j], bytes[j])) return WM_ERR_BAD_ARG;
  return WM_OK;
}

int launch_lsp_postfilter(Batch& b, hipStream_t st, const double* d_lsp, const WorldMi355LspPostfilterOption& opt,
                          double* d_out, double* d_ene1, double* d_ene2, int* d_status) {
  const int64_t tf = b.total_f;
  if (const int rc = check_lsp_postfilter(tf, d_lsp, &opt, d_out, d_ene1, d_ene2, d_status)) return rc;
  if (tf <= 0) return WM_OK;
  const int m = opt.order;
  const dim3 per_row((unsigned)((tf + 255) / 256));
  if (opt.beta == 1.0 || m <= 2) {
    TimedScope ts_(b.ctx, st, "lsp_kernel");
    const int64_t n = tf * (m + 1);                    // >= 2 tf: the row index fits the same walk
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(lsp_identity_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, d_lsp, n, tf,
                       d_out, d_ene1, d_ene2, d_status);
    return wm_check(hipGetLastError());
  }
  LspArgs a = lsp_args(m, opt.log_gain, opt.min_distance, opt.min_gain);
  a.beta = opt.beta;
  if (!opt.compensation && !d_ene1 && !d_ene2) {
    // the script as written: the filtered LSPs beside the gain as it is
    TimedScope ts_(b.ctx, st, "lsp_kernel");
    a.filter = 1;
    a.convert = 0;
    launch_rows(b, st, d_lsp, a, d_out, nullptr, nullptr, d_status);
    return wm_check(hipGetLastError());
  }
  // two LPC rows and two doubles per frame
  double* ws = nullptr;
  const int64_t row_doubles = tf * (m + 1);
  if (const int rc = lsp_workspace(b, st, 2 * row_doubles + 2 * tf, &ws)) return rc;
  double *lpc1 = ws, *lpc2 = ws + row_doubles, *e1 = ws + 2 * row_doubles, *e2 = e1 + tf;
  {
    TimedScope ts_(b.ctx, st, "lsp_kernel");
    launch_rows(b, st, d_lsp, a, nullptr, lpc1, nullptr, d_status);                 // the raw row, before `out` may replace it
    a.filter = 1;
    a.status_or = 1;
    launch_rows(b, st, d_lsp, a, d_out, lpc2, nullptr, d_status);
    if (const int rc = wm_check(hipGetLastError())) return rc;
  }
  const WorldMi355MgcConvertOption c = convert_option(m, opt.alpha, opt.gamma, opt.length - 1, 0.0, 1.0);
  if (const int rc = launch_mgc2mgc_energy(b, st, lpc1, c, e1)) return rc;
  if (const int rc = launch_mgc2mgc_energy(b, st, lpc2, c, e2)) return rc;
  hipLaunchKernelGGL(lsp_gain_kernel, per_row, dim3(256), 0, st, e1, e2, m, opt.log_gain != 0, opt.compensation != 0, tf,
                     d_out, d_ene1, d_ene2, d_status);
  return wm_check(hipGetLastError());
}

}  // namespace wm
