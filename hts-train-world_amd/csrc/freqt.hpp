// freqt.hpp -- SPTK's frequency transformations (test/sptkfunctions.cpp: freqt :596-631, frqtr :651-684) on one
// wavefront, shared by the bap decoder (codec.hip) and the mel-cepstral analysis (mcep.hip).
//
// Both are the two-dimensional recurrence g_i[j] = g_{i-1}[j-1] + a (g_{i-1}[j] - g_i[j-1]) over the input step i and
// the output index j, sequential in both, with their own expressions at j = 0 (and j = 1 for freqt).  It runs as a
// systolic pipeline along whichever of the two is at most 64 (or 127) long: a lane owns one row (or column), computes
// one element per time step and reads what its left neighbour produced in the previous step by a one-lane DPP shift.
// Every element is the reference's expression in the reference's order (no FMA contraction).
#pragma once
#include "common.hpp"

namespace wm {

// freqt from order + 1 coefficients to h + 1, lane per INPUT step: lane s of a group of W lanes feeds coefficient
// order - s as `cin` (the reference walks c1[order] .. c1[0]; lanes beyond `order` feed 0 and compute values nobody
// reads).  The lane with store_lane set (s == order of a live frame) writes c[0 .. h]; every other lane writes its
// steady-phase values to `dummy`, a slot of its own, so the loop has no exec-mask branch.  b = 1 - a a.
// The loop is issue-bound, so it is split into the start-up steps, where some row is still at one of its two special
// first elements, and a steady phase of ten instructions per step without selects.
template <int W>
__device__ __forceinline__ void freqt_expand(double cin, int s, int order, int h, double a, double b, bool store_lane,
                                             double* c, double* dummy) {
#pragma clang fp contract(off)
  double last = 0.0, prev_up = 0.0, own_prev = 0.0;
  // start-up: until step order + 1 some row is still at its first (j = 0) or second (j = 1) element, which
  // have their own expressions (:620-623)
  for (int t = 0; t <= order + 1; ++t) {
    double up = dpp_get<0x138, 0xf, 0xf>(last);              // wave_shr:1 -- lane s reads lane s-1, lane 0 reads 0
    if (W < 64 && s == 0) up = 0.0;                          // g_{-1} = 0 between two packed frames too
    const int j = t - s;
    const double B = up - (j >= 2 ? own_prev : 0.0);
    const double A = j == 0 ? cin : prev_up * (j == 1 ? b : 1.0);
    const double val = A + a * B;
    // a row that has not started (j < 0) computes values nobody reads: its right neighbour is one step
    // behind it, and j = 0 takes nothing from the row's own state
    prev_up = up;
    own_prev = val;
    last = val;
    if (store_lane && j >= 0) c[j] = val;
  }
  // steady state: every row is at j >= 2, the general element g[j] = d[j-1] + a (d[j] - g[j-1]) (:624-625).
  // A row that is finished (j > h) again computes values nobody reads.  Every lane stores every step -- the
  // row that carries the result into the cepstrum, the others into a slot of their own -- so the loop has
  // no exec-mask branch.
  {
    double* dst = store_lane ? c + 2 : dummy;
    const int adv = store_lane ? 1 : 0;
    for (int t = order + 2; t <= h + order; ++t) {
      double up = dpp_get<0x138, 0xf, 0xf>(last);
      if (W < 64 && s == 0) up = 0.0;
      const double val = prev_up + a * (up - own_prev);
      prev_up = up;
      own_prev = val;
      last = val;
      *dst = val;
      dst += adv;
    }
  }
}

// The other way round, lane per OUTPUT index: from the n1 + 1 values src[0 .. n1] (LDS) to nout + 1 values, output j
// in lane j (o1) and, with TWO, output 64 + j in o2 (frqtr's 2 m + 1 autocorrelations can be 127).  Lane j works on
// input step t - j at time t; rows that have not started hold the zeros the reference's fillz() leaves, and zeros
// reproduce themselves, so nothing marks the start; a lane keeps the value of its last real step (t - j == n1).
// The inputs come 64 at a time in one LDS read; lane 0 takes its value of the step by v_readlane.
//   MODE 0, freqt :619-626:  g[0] = c + a d[0];  g[1] = b d[0] + a d[1];  g[j] = d[j-1] + a (d[j] - g[j-1])
//   MODE 1, frqtr :672-679:  g[0] = c;           g[j] = d[j-1] + a (d[j] - g[j-1]),  j >= 1
template <int MODE, bool TWO>
__device__ __forceinline__ void freqt_contract(const double* src, int n1, int nout, double a, int lane, double& o1,
                                               double& o2) {
#pragma clang fp contract(off)
  static_assert(MODE == 1 || !TWO, "freqt is used towards at most 64 coefficients");
  const double b = 1 - a * a;
  const double ka = (MODE == 0 && lane == 1) ? b : 1.0;
  const bool use_up = lane >= (MODE == 0 ? 2 : 1);
  double last1 = 0.0, pu1 = 0.0, last2 = 0.0, pu2 = 0.0;
  o1 = 0.0;
  o2 = 0.0;
  const int T = n1 + nout;                                   // the last time step
  for (int base = 0; base <= T; base += 64) {
    const int idx = n1 - (base + lane);
    const double chunk = src[idx > 0 ? idx : 0];
    const int qn = T + 1 - base < 64 ? T + 1 - base : 64;
    for (int q = 0; q < qn; ++q) {
      const int t = base + q;
      const double cin = readlane_d(chunk, q);
      const double up = dpp_get<0x138, 0xf, 0xf>(last1);     // wave_shr:1
      if (TWO) {
        const double carry = lane63(last1);                  // output 63 feeds output 64
        double up2 = dpp_get<0x138, 0xf, 0xf>(last2);
        up2 = lane == 0 ? carry : up2;
        const double val2 = pu2 + a * (last2 - up2);
        pu2 = up2;
        last2 = val2;
        if (t - 64 - lane == n1) o2 = val2;
      }
      double val = pu1 * ka + a * (last1 - (use_up ? up : 0.0));
      if (lane == 0) val = MODE == 0 ? cin + a * last1 : cin;
      pu1 = up;
      last1 = val;
      if (t - lane == n1) o1 = val;
    }
  }
}

}  // namespace wm
