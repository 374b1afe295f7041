// mgc2mgc.hip -- conversion between mel-generalized cepstra on the device: SPTK's `mgc2mgc`.
//
// Restates the core of the CLIs' SPTK port, mgc2mgc(c1, m1, a1, g1, c2, m2, a2, g2) (test/sptkfunctions.cpp:221-254), in
// its own branches, a = (a2 - a1) / (1 - a1 a2) computed on the host in that expression (:238):
//
//   a == 0 (:240-244): gnorm over m1 with g1 (:313-328), gc2gc(m1, g1 -> m2, g2) (:347-385), ignorm with g2 (:330-345);
//   a != 0 (:245-250): freqt from m1 to m2 coefficients with warp a (:596-631; freqt.hpp: the reference's expressions in
//     its order, lane per input coefficient when m1 <= 63, lane per output otherwise), gnorm over M2 with g1,
//     gc2gc(m2, g1 -> m2, g2), ignorm with g2;
//   g1 == g2 == 0: gc2gc's sums are multiplied by 0; they are skipped, the chain is c0 -> log(exp(c0)).
//
// Around the core, the four flags of SPTK's command (include/world_mi355.h; FLAG SEMANTICS UNPINNED AGAINST SPTK'S
// COMMAND: the command is not in the reference tree): -n ignorm and -u the division by g1 before it, -N gnorm and -U the
// product with g2 after it.  The flag steps, gnorm's division and ignorm's product are the reference's expressions without
// contraction; pow, exp and log are the device library's.
//
// One 64-lane workgroup per row, persistent over the batch's rows.  Towards m2 <= 64 coefficients (the recipe's orders)
// gc2gc runs in the reference's own order, every product and addition with its rounding: the whole chain is then the
// reference's bits wherever the device library's pow / exp / log return libm's.  Beyond 64 outputs
// that order, sequential in both of its loops, is out of reach, and the general gc2gc (:368-382),
//   c2[i] = ca[i] + (g2 ss2 - g1 ss1) / i,  ss2 = sum_k k ca[k] c2[i-k],  ss1 = sum_k (i-k) ca[k] c2[i-k],  ca[k] = 0 beyond
//   its input order,
// runs right-looking as in mgc2sp_kernel, with no cross-lane reduction: with u[j] = j c2[j],
//   g2 ss2 - g1 ss1 = g2 i Sc - (g1 + g2) Su,   Sc = sum_j ca[i-j] c2[j],   Su = sum_j ca[i-j] u[j],
// so c2[i] = ca[i] + g2 Sc - (g1 + g2) Su / i.  Lane l owns the outputs i = 64 r + l + 1 and keeps Sc and Su of each in
// registers; once c2[j] is final in its lane it is broadcast (v_readlane), u[j] is its product with j, and every later
// output adds its two terms by one fused multiply-add each, ca read from LDS at a distance that moves one element per
// step (64 zeros in front of ca[1] stand for i - j <= 0, so no lane is masked).  The sums of the block that is being
// finished are register 0; after its 64 steps the registers move down one.  An output is written to global memory when it
// is final; nothing reads c2 back.  The sums run in ascending j with fused products where the reference runs in
// descending j with three roundings per term, and 1 / i is a rounded reciprocal: the results differ from the
// reference's by its own rounding error, which the fixture measures (sens of tools/gen_golden_mgc2mgc.py).
//
// Instantiated by size class of m2 (M blocks of 64 outputs), so the recipe's orders do not carry the registers and LDS
// of 4095: DESIGN.md, "Mel-generalized cepstrum conversion", says what each class uses.
#include <math.h>

#include "batch.hpp"
#include "common.hpp"
#include "freqt.hpp"

namespace wm {

struct Mgc2mgcArgs {
  double g1, g2;
  double a, b;                 // the warp (:238) and freqt's 1 - a a (:616), both rounded on the host
  int m1, m2;
  int in_norm, in_mul, out_norm, out_mul;
};

// The energy form's sum of squares, an unevaluated pair h + l per lane: a square enters exactly (the product and its
// rounding error by one fma each), the additions keep their rounding errors (two-sum), so the total is good to the last
// bit of a double and beyond.  It has to be: for a row whose gain is tiny the sum is 1 - 2 K and the energy, 1/2 ln of
// it, is -K -- what a sum rounded to 1e-16 would bury.
struct SquareSum {
  double h = 0.0, l = 0.0;
  __device__ __forceinline__ void add_square(double v) {
#pragma clang fp contract(off)
    const double p = v * v, pe = __builtin_fma(v, v, -p);
    const double t = h + p, b = t - h;
    l = l + (((h - (t - b)) + (p - b)) + pe);
    h = t;
  }
  template <int CTRL, int ROW_MASK> __device__ __forceinline__ void add_lanes() {
#pragma clang fp contract(off)
    const double oh = dpp_get<CTRL, ROW_MASK, 0xf>(h), ol = dpp_get<CTRL, ROW_MASK, 0xf>(l);   // 0 where there is no source
    const double t = h + oh, b = t - h;
    l = (l + ol) + ((h - (t - b)) + (oh - b));
    h = t;
  }
  // 1/2 ln of the wave's total, by wave_scan_incl()'s fixed tree: a row's bits depend on nothing but the row
  __device__ __forceinline__ double half_log_total() {
    add_lanes<0x111, 0xf>();
    add_lanes<0x112, 0xf>();
    add_lanes<0x114, 0xf>();
    add_lanes<0x118, 0xf>();
    add_lanes<0x142, 0xa>();
    add_lanes<0x143, 0xc>();
    const double th = lane63(h), tl = lane63(l);
    return 0.5 * (log(th) + tl / th);
  }
};

extern __shared__ double mgc2mgc_row[];   // the plain input row of the lane-per-output freqt (m1 > 63): m1 + 1 doubles

template <int M, bool ENERGY = false>
__global__ __launch_bounds__(64) void mgc2mgc_kernel(const double* __restrict__ in, Mgc2mgcArgs o, int64_t total_rows,
                                                     double* __restrict__ out, int* __restrict__ status) {
  constexpr int N = 64 * M;                            // the class holds outputs 1 .. N
  constexpr int G = M < 4 ? M : 4;                     // accumulator pairs per LDS read group of the recurrence
  __shared__ double caz[64 + N + 1];                   // 64 zeros and a zero for ca[0], then ca[1 .. N]
  const int lane0 = threadIdx.x;
  const int m1 = o.m1, m2 = o.m2;
  const double g1 = o.g1, g2 = o.g2;
  const bool warp = o.a != 0.0;
  const int mg = imin(warp ? m2 : m1, N);              // gc2gc's input order (:243, :248), as far as an output reads it
  const int nblk = (m2 + 63) / 64;
  const int dlim = imin((mg + 63) / 64 + 1, M);        // registers a step can reach: i - j <= mg
  for (int64_t row = blockIdx.x; row < total_rows; row += gridDim.x) {
    const int lane = opaque_lane(lane0);
    const double* src = in + row * (int64_t)(m1 + 1);
    double* dst = ENERGY ? out : out + row * (int64_t)(m2 + 1);   // the energy form stores no coefficient
    wave_sync();
    // ---- the row as given: every coefficient finite, c[0] to every lane
    bool bad = false;
    for (int k = lane; k <= m1; k += 64) bad = bad || !(fabs(src[k]) < __builtin_inf());
    bool ok = __ballot(bad) == 0ull;
    int code = 1;
    double c0 = 0.0, kin = 1.0;                        // the plain row's c[0]; ignorm's factor of -n
    if (ok) {
#pragma clang fp contract(off)
      const double c0raw = uniform_d(src[0]);
      if (o.in_norm) {                                 // -n: ignorm (:330-345); the gain is c[0] itself
        ok = c0raw > 0.0;
        if (g1 != 0.0) {
          kin = uniform_d(pow(c0raw, g1));
          c0 = (kin - 1.0) / g1;
        } else {
          c0 = uniform_d(log(c0raw));
        }
      } else if (o.in_mul) {                           // -u alone
        c0 = (c0raw - 1.0) / g1;
      } else {
        c0 = c0raw;
      }
      if (g1 != 0.0) ok = ok && 1.0 + g1 * c0 > 0.0;   // the gain of the plain row
      ok = __builtin_amdgcn_readfirstlane(ok ? 1 : 0) != 0;
    }
    // coefficient k >= 1 of the plain row
    auto plain = [&](double v) {
#pragma clang fp contract(off)
      if (o.in_norm && g1 != 0.0) v = kin * v;
      if (o.in_mul) v = v / g1;
      return v;
    };
    double K = 1.0;                                    // the normalized gain gnorm leaves in c[0] (:321, :324)
    if (ok) {
      // ---- the coefficients gnorm reads, into caz[64 + k]
      if (!warp) {
#pragma unroll
        for (int q = 0; q < M; ++q) {
          const int k = lane + 64 * q + 1;
          caz[64 + k] = k <= mg ? plain(src[k]) : 0.0;
        }
      } else if (m1 <= 63) {
        // lane s feeds coefficient m1 - s (freqt walks c1[m1] .. c1[0])
        const double cin = lane < m1 ? plain(src[m1 - lane]) : (lane == m1 ? c0 : 0.0);
        freqt_expand<64>(cin, lane, m1, m2, o.a, o.b, lane == m1, caz + 64, caz + lane);        // :246
        wave_sync();
        c0 = uniform_d(caz[64]);
#pragma unroll
        for (int q = 0; q < M; ++q) {
          const int k = lane + 64 * q + 1;
          if (k > m2) caz[64 + k] = 0.0;
        }
      } else {
        if constexpr (M == 1) {                        // m1 > 63 >= m2
          for (int k = lane; k <= m1; k += 64) mgc2mgc_row[k] = k == 0 ? c0 : plain(src[k]);
          wave_sync();
          double o1, o2;
          freqt_contract<0, false>(mgc2mgc_row, m1, m2, o.a, lane, o1, o2);                       // :246
          c0 = readlane_d(o1, 0);
          caz[64 + lane + 1] = 0.0;
          wave_sync();
          if (lane >= 1 && lane <= m2) caz[64 + lane] = o1;
        }
      }
      caz[lane] = 0.0;
      if (lane == 0) caz[64] = 0.0;
      wave_sync();
      // ---- gnorm with g1 (:313-328)
      if (g1 != 0.0) {
#pragma clang fp contract(off)
        const double kk = 1.0 + g1 * c0;                                                          // :318
        ok = __builtin_amdgcn_readfirstlane(kk > 0.0 ? 1 : 0) != 0;                               // the reference's pow: NaN
        if (ok) {
#pragma unroll
          for (int q = 0; q < M; ++q) {
            const int k = lane + 64 * q + 1;
            caz[64 + k] = caz[64 + k] / kk;                                                       // :320
          }
          K = uniform_d(pow(kk, 1.0 / g1));                                                       // :321
        }
        wave_sync();
      } else {
        K = uniform_d(exp(c0));                                                                   // :324
      }
    }
    if (ok) {
      // ---- ignorm with g2 (:330-345) and the output flags, per coefficient as it becomes final
      double k2 = 1.0, c20, kk2 = 1.0;
      {
#pragma clang fp contract(off)
        if (g2 != 0.0) {
          k2 = uniform_d(pow(K, g2));                                                             // :334
          c20 = (k2 - 1.0) / g2;                                                                  // :338
        } else {
          c20 = uniform_d(log(K));                                                                // :341
        }
        if (o.out_norm) {                              // -N: gnorm with g2
          if (g2 != 0.0) {
            kk2 = 1.0 + g2 * c20;
            c20 = uniform_d(pow(kk2, 1.0 / g2));
          } else {
            c20 = uniform_d(exp(c20));
          }
        } else if (o.out_mul) {                        // -U alone
          c20 = c20 * g2 + 1.0;
        }
      }
      auto finish = [&](double v) {
#pragma clang fp contract(off)
        if (g2 != 0.0) v = k2 * v;                                                                // :337
        if (o.out_norm && g2 != 0.0) v = v / kk2;
        if (o.out_mul) v = v * g2;
        return v;
      };
      bool nonfinite = !(fabs(c20) < __builtin_inf());
      SquareSum esum;                                  // the energy form: this lane's c2[k]^2, in ascending k
      if constexpr (ENERGY) {
        if (lane == 0) esum.add_square(c20);
      } else {
        if (lane == 0) dst[0] = c20;
      }
      if (g1 == 0.0 && g2 == 0.0) {
        // gc2gc between gamma 0 and gamma 0 leaves ca (:379, :381 with both factors 0)
#pragma unroll
        for (int q = 0; q < M; ++q) {
          const int i = lane + 64 * q + 1;
          if (i <= m2) {
            const double v = finish(caz[64 + i]);
            nonfinite = nonfinite || !(fabs(v) < __builtin_inf());
            if constexpr (ENERGY) esum.add_square(v);
            else dst[i] = v;
          }
        }
      } else if (M == 1) {
        // m2 <= 64: gc2gc in the reference's own order (:368-382), every product and every addition its rounding.
        // Lane k holds ca[k] and, for the output i in work, w = c2[i - k]: from one output to the next w moves up one
        // lane and lane 1 takes the new c2[i].  ss2 and ss1 are summed over k = 1 .. min in that order along the lanes,
        // one lane per step (lane k adds its term to what lane k - 1 held the step before; lane 0 holds the 0.0 they
        // start from), so an output costs min(order, i - 1) steps of two additions.
#pragma clang fp contract(off)
        const double cak = caz[64 + lane];                       // ca[0] is stored as 0: lane 0 adds nothing
        const double kd = (double)lane;
        double w = 0.0, vout = 0.0;
        for (int i = 1; i <= m2; ++i) {
          const double id = (double)i;
          const double cc = cak * w;                             // :373
          const double p2 = kd * cc, p1 = (id - kd) * cc;        // :374, :375
          const int steps = imin(mg, i - 1);                     // :370
          double a2 = 0.0, a1 = 0.0;
          for (int t = 0; t < steps; ++t) {
            a2 = dpp_get<0x138, 0xf, 0xf>(a2) + p2;              // wave_shr:1 -- lane k reads lane k - 1, lane 0 reads 0
            a1 = dpp_get<0x138, 0xf, 0xf>(a1) + p1;
          }
          const double ss2 = readlane_d(a2, steps), ss1 = readlane_d(a1, steps);
          const double s = (g2 * ss2 - g1 * ss1) / id;
          const double c2i = i <= mg ? caz[64 + i] + s : s;      // :378-381
          const double v = finish(c2i);
          if (lane == i - 1) vout = v;
          w = dpp_get<0x138, 0xf, 0xf>(w);
          if (lane == 1) w = c2i;
        }
        if (lane < m2) {
          nonfinite = nonfinite || !(fabs(vout) < __builtin_inf());
          if constexpr (ENERGY) esum.add_square(vout);
          else dst[lane + 1] = vout;
        }
      } else {
        const double gs = g1 + g2;
        double sc[M], su[M];
#pragma unroll
        for (int d = 0; d < M; ++d) sc[d] = su[d] = 0.0;
        const double* zp = caz + 64 + lane;
        for (int rj = 0; rj < nblk; ++rj) {
          const int i_own = 64 * rj + lane + 1;
          const double cai = caz[64 + i_own];
          const double w = -gs * (1.0 / (double)i_own);
          const int lim = imin(nblk - rj, dlim);
          double jd = (double)(64 * rj);
          // the last output, c2[m2], reads c2[j] up to j = m2 - 1: a continuation past m2 is neither computed nor able
          // to flag the row
          const int steps = imin(64, m2 - 64 * rj - 1);
          for (int l = 0; l < steps; ++l) {
            // c2[j], j = 64 rj + l + 1, is final in lane l: every later output takes its two terms
            jd += 1.0;
            const double cj = readlane_d(__builtin_fma(w, su[0], __builtin_fma(g2, sc[0], cai)), l);
            const double uj = cj * jd;
            // G registers per test of the wave-uniform bound: their LDS reads are issued together.  A register past
            // `lim` in its group reads zeros of the table, or belongs to an output past m2 that nobody finishes
#pragma unroll
            for (int d0 = 0; d0 < M; d0 += G)
              if (d0 < lim) {
                double z[G];
#pragma unroll
                for (int g = 0; g < G; ++g) z[g] = zp[64 * (d0 + g) - l];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                  sc[d0 + g] = __builtin_fma(cj, z[g], sc[d0 + g]);
                  su[d0 + g] = __builtin_fma(uj, z[g], su[d0 + g]);
                }
              }
          }
          if (i_own <= m2) {
            const double v = finish(__builtin_fma(w, su[0], __builtin_fma(g2, sc[0], cai)));
            nonfinite = nonfinite || !(fabs(v) < __builtin_inf());
            if constexpr (ENERGY) esum.add_square(v);
            else dst[i_own] = v;
          }
#pragma unroll
          for (int d = 0; d + 1 < M; ++d) {
            sc[d] = sc[d + 1];
            su[d] = su[d + 1];
          }
          sc[M - 1] = su[M - 1] = 0.0;
        }
      }
      if (__ballot(nonfinite) != 0ull) {
        ok = false;
        code = 2;
      }
      if constexpr (ENERGY) {
        const double ene = esum.half_log_total();
        ok = ok && fabs(ene) < __builtin_inf();
        if (ok && lane == 0) dst[row] = ene;
      }
    }
    if constexpr (ENERGY) {
      if (!ok && lane == 0) dst[row] = __builtin_nan("");   // what the storing form flags
    } else {
      if (!ok)
        for (int k = lane; k <= m2; k += 64) dst[k] = 0.0;
    }
    if (status != nullptr && lane == 0) status[row] = ok ? 0 : code;
  }
}

namespace {

// [a, a + na) and [b, b + nb) share an element
bool ranges_meet(const double* a, int64_t na, const double* b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb * sizeof(double) && pb < pa + (uintptr_t)na * sizeof(double);
}

int size_class(int m2) {
  int c = 1;
  while (64 * c < m2) c *= 2;
  return c;
}

}  // namespace

// What WorldMi355MelGeneralizedCepstrumConvert refuses, on the host alone: no device call is made for a refused set.
int check_mgc2mgc(int64_t total_rows, const double* d_in, const WorldMi355MgcConvertOption* opt, const double* d_out) {
  if (!d_in || !opt || !d_out) return WM_ERR_BAD_ARG;
  const int m1 = opt->in_order, m2 = opt->out_order;
  if (m1 < 1 || m1 > 4095 || m2 < 1 || m2 > 4095 || imin(m1, m2) > 63) return WM_ERR_BAD_ARG;
  if (!(fabs(opt->in_alpha) < 1.0) || !(fabs(opt->out_alpha) < 1.0)) return WM_ERR_BAD_ARG;
  if (!(opt->in_gamma >= -1.0 && opt->in_gamma <= 1.0) || !(opt->out_gamma >= -1.0 && opt->out_gamma <= 1.0))
    return WM_ERR_BAD_ARG;
  if (opt->in_multiplied && opt->in_gamma == 0.0) return WM_ERR_BAD_ARG;
  if (opt->out_multiplied && opt->out_gamma == 0.0) return WM_ERR_BAD_ARG;
  if (total_rows > 0 && ranges_meet(d_in, total_rows * (m1 + 1), d_out, total_rows * (m2 + 1))) return WM_ERR_BAD_ARG;
  return WM_OK;
}

namespace {

Mgc2mgcArgs mgc2mgc_args(const WorldMi355MgcConvertOption& opt) {
  Mgc2mgcArgs a;
  {
#pragma clang fp contract(off)
    a.a = (opt.out_alpha - opt.in_alpha) / (1 - opt.in_alpha * opt.out_alpha);                    // :238
    a.b = 1 - a.a * a.a;                                                                          // :616
  }
  a.g1 = opt.in_gamma;
  a.g2 = opt.out_gamma;
  a.m1 = opt.in_order;
  a.m2 = opt.out_order;
  a.in_norm = opt.in_normalized != 0;
  a.in_mul = opt.in_multiplied != 0;
  a.out_norm = opt.out_normalized != 0;
  a.out_mul = opt.out_multiplied != 0;
  return a;
}

}  // namespace

int launch_mgc2mgc(Batch& b, hipStream_t st, const double* d_in, const WorldMi355MgcConvertOption& opt, double* d_out,
                   int* d_status) {
  const int64_t tf = b.total_f;
  if (const int rc = check_mgc2mgc(tf, d_in, &opt, d_out)) return rc;
  if (tf <= 0) return WM_OK;
  const Mgc2mgcArgs a = mgc2mgc_args(opt);
  // the lane-per-output freqt reads its input row from LDS
  const int dyn = a.a != 0.0 && a.m1 > 63 ? (int)sizeof(double) * (a.m1 + 1) : 0;
  TimedScope ts_(b.ctx, st, "mgc2mgc_kernel");
#define WM_MGC2MGC_CASE(MM)                                                                                 \
  case MM: {                                                                                                \
    const int per_ = persistent_grid(*b.ctx, mgc2mgc_kernel<MM>, 64, (int64_t)1 << 40);                     \
    hipLaunchKernelGGL((mgc2mgc_kernel<MM>), dim3((int)(tf < per_ ? tf : per_)), dim3(64), dyn, st, d_in, a, tf, d_out, \
                       d_status);                                                                           \
  } break;
  switch (size_class(a.m2)) {
    WM_MGC2MGC_CASE(1)
    WM_MGC2MGC_CASE(2)
    WM_MGC2MGC_CASE(4)
    WM_MGC2MGC_CASE(8)
    WM_MGC2MGC_CASE(16)
    WM_MGC2MGC_CASE(32)
    WM_MGC2MGC_CASE(64)
  }
#undef WM_MGC2MGC_CASE
  return wm_check(hipGetLastError());
}

// The energy form (postfiltering_lsp's `mgc2mgc | vopr -m | vsum | sopr -LN -m 0.5`, scripts/Training.pl:2702-2705): the
// same rows through the same chain, each c2[k] squared into its lane's sum where the storing form writes it, one double per
// row out.  d_ene and d_in share no element: both are the caller's own workspace (lsp.hip).
int launch_mgc2mgc_energy(Batch& b, hipStream_t st, const double* d_in, const WorldMi355MgcConvertOption& opt,
                          double* d_ene) {
  const int64_t tf = b.total_f;
  if (!d_ene) return WM_ERR_BAD_ARG;
  if (const int rc = check_mgc2mgc(0, d_in, &opt, d_ene)) return rc;
  if (tf <= 0) return WM_OK;
  const Mgc2mgcArgs a = mgc2mgc_args(opt);
  const int dyn = a.a != 0.0 && a.m1 > 63 ? (int)sizeof(double) * (a.m1 + 1) : 0;
  TimedScope ts_(b.ctx, st, "mgc2mgc_kernel");
#define WM_MGC2MGC_CASE(MM)                                                                                 \
  case MM: {                                                                                                \
    const int per_ = persistent_grid(*b.ctx, mgc2mgc_kernel<MM, true>, 64, (int64_t)1 << 40);               \
    hipLaunchKernelGGL((mgc2mgc_kernel<MM, true>), dim3((int)(tf < per_ ? tf : per_)), dim3(64), dyn, st, d_in, a, tf, \
                       d_ene, (int*)nullptr);                                                               \
  } break;
  switch (size_class(a.m2)) {
    WM_MGC2MGC_CASE(1)
    WM_MGC2MGC_CASE(2)
    WM_MGC2MGC_CASE(4)
    WM_MGC2MGC_CASE(8)
    WM_MGC2MGC_CASE(16)
    WM_MGC2MGC_CASE(32)
    WM_MGC2MGC_CASE(64)
  }
#undef WM_MGC2MGC_CASE
  return wm_check(hipGetLastError());
}

}  // namespace wm
