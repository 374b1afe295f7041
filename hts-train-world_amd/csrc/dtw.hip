// dtw.hip -- objective evaluation: dynamic-time-warping alignment of two feature sequences per utterance and the
// distortion measures along a path (mel-cepstral distortion, lf0 error, V/UV error), by the definition in
// include/world_mi355.h.  The reference tree holds no evaluation code; tests/dtw_reference.py states the definition in numpy.
//
//   dtw_kernel         one wavefront per pair, longest pair (T_a T_b) first.  Rows of A go in strips of 64: lane l owns row
//                      64 strip + l and keeps its `count` columns in registers as doubles (templated over a padded count;
//                      the padding holds zeros on both sides and adds +0 to the sum).  Inside a strip the sweep is skewed:
//                      at step s lane l handles column j = s - l, so D(i-1, j) and D(i-1, j-1) are lane l - 1's values of
//                      the last two steps (one wave_shr:1 each) and D(i, j-1) is the lane's own.  Lane 0 takes the previous
//                      strip's last row from a T_b-long buffer, 64 columns per load with lanes as columns and one
//                      v_readlane per step; lane 63's values go back the same way, 64 per store.  Two such buffers
//                      alternate, so a strip never writes what it reads.  Rows of B are staged through LDS 64 at a time,
//                      transposed ([column][row mod 128], 129 floats per column), so each row is fetched once per strip and
//                      a step's reads of one column are 64 consecutive words.  One back-pointer byte per cell, four steps
//                      of a lane packed into a dword: [strip][step / 4][lane], 256 contiguous bytes per store.
//   dtw_path_kernel    one wavefront per pair: the backward walk.  Sixteen dword rows of back-pointers (64 steps of the
//                      strip) are staged in LDS per refill, every lane follows the same walk on broadcast reads and lane 0
//                      writes the pairs from the end of the utterance's capacity backwards; the wave then moves them to
//                      the front and writes (-1, -1) behind them.  Also path_len and status.
//   dtw_distortion_kernel  one wavefront per (utterance, group): lanes as pairs for the per-pair measure, then the sums in
//                      pair order by v_readlane, as the definition's sequential sum.
// No inline assembly, no atomics, no spin waits; the host waits only where grow_ws does.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#include "batch.hpp"
#include "common.hpp"

namespace wm {

namespace {
constexpr int kDtwMaxCount = 64;
constexpr int kDtwMaxLen = 32767;
constexpr int kDtwMaxGroups = 8;
constexpr int kDtwRing = 128;                   // B rows resident in LDS: two tiles of 64
constexpr int kDtwLdsRow = kDtwRing + 1;        // floats per column: the pad keeps the tile's stores off one bank
constexpr int kDtwWalkRows = 16;                // dword rows of back-pointers per LDS refill of the walk: 64 steps

// one pair's share of the workspace: back-pointer dwords and the doubles of the two row buffers
inline int64_t dtw_bp_dwords(int ta, int tb) {
  if (ta < 1 || tb < 1) return 0;
  const int64_t strips = (ta + 63) / 64, rows = ((int64_t)tb + 63 + 3) / 4;
  return strips * rows * 64;
}
inline int64_t dtw_row_doubles(int ta, int tb) { return ta > 64 && tb > 0 ? 2 * (int64_t)tb : 0; }

// the allocations of a workspace for these pairs, in the order ensure_ws makes them
struct DtwPlan {
  int64_t bp_dwords = 0, row_doubles = 0;
  size_t bytes[7];
  DtwPlan(int n_utt, const int* ta, const int64_t* b_off) {
    for (int u = 0; u < n_utt; ++u) {
      const int tb = (int)(b_off[u + 1] - b_off[u]);
      bp_dwords += dtw_bp_dwords(ta[u], tb);
      row_doubles += dtw_row_doubles(ta[u], tb);
    }
    const size_t n = (size_t)(n_utt > 0 ? n_utt : 1);
    bytes[0] = 4 * (size_t)(bp_dwords ? bp_dwords : 1);
    bytes[1] = 8 * (size_t)(row_doubles ? row_doubles : 1);
    bytes[2] = 8 * (n + 1);                     // b_off
    bytes[3] = 8 * (n + 1);                     // bp_off
    bytes[4] = 8 * (n + 1);                     // row_off
    bytes[5] = 4 * n;                           // order
    bytes[6] = 4 * n;                           // flag
  }
};

int check_b_off(int n_utt, const int64_t* b_off) {
  if (!b_off || b_off[0] != 0) return WM_ERR_BAD_ARG;
  for (int u = 0; u < n_utt; ++u) {
    if (b_off[u + 1] < b_off[u]) return WM_ERR_BAD_ARG;
    if (b_off[u + 1] - b_off[u] > kDtwMaxLen) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}
}  // namespace

int dtw_workspace_bytes(int n_utt, const int* a_lengths, const int* b_lengths, int64_t* bytes) {
  if (!bytes || n_utt < 0 || (n_utt > 0 && (!a_lengths || !b_lengths))) return WM_ERR_BAD_ARG;
  std::vector<int64_t> b_off((size_t)n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) {
    if (a_lengths[u] < 0 || a_lengths[u] > kDtwMaxLen || b_lengths[u] < 0 || b_lengths[u] > kDtwMaxLen) return WM_ERR_BAD_ARG;
    b_off[(size_t)u + 1] = b_off[(size_t)u] + b_lengths[u];
  }
  const DtwPlan plan(n_utt, a_lengths, b_off.data());
  int64_t total = 0;
  for (const size_t s : plan.bytes) total += (int64_t)dev_alloc_size(s);
  *bytes = total;
  return WM_OK;
}

int check_dtw(const Batch& b, const float* a, int64_t ld_a, const float* bs, int64_t ld_b, const int64_t* b_off, int first,
              int count, const int* path, const int* path_len, const double* cost) {
  if (!a || !bs || !path || !path_len || !cost) return WM_ERR_BAD_ARG;
  if (count < 1 || count > kDtwMaxCount || first < 0) return WM_ERR_BAD_ARG;
  if ((int64_t)first + count > ld_a || (int64_t)first + count > ld_b) return WM_ERR_BAD_ARG;
  if (const int rc = check_b_off(b.n_utt, b_off)) return rc;
  for (int u = 0; u < b.n_utt; ++u)
    if (b.f0_len[u] > kDtwMaxLen) return WM_ERR_BAD_ARG;
  return WM_OK;
}

int check_distortion(const Batch& b, const int* path, const int* path_len, const int64_t* b_off, int n_groups,
                     const WorldMi355DistortionGroup* groups, const WorldMi355DistortionOption* opt, const double* out) {
  if (!groups || !opt || !out || (path == nullptr) != (path_len == nullptr)) return WM_ERR_BAD_ARG;
  if (n_groups < 1 || n_groups > kDtwMaxGroups) return WM_ERR_BAD_ARG;
  if (!(fabs(opt->voiced_above) < HUGE_VAL)) return WM_ERR_BAD_ARG;
  if (const int rc = check_b_off(b.n_utt, b_off)) return rc;
  for (int g = 0; g < n_groups; ++g) {
    const WorldMi355DistortionGroup& q = groups[g];
    if (!q.a || !q.b || q.first < 0 || q.count < 1 || q.count > kDtwMaxCount) return WM_ERR_BAD_ARG;
    if ((int64_t)q.first + q.count > q.ld_a || (int64_t)q.first + q.count > q.ld_b) return WM_ERR_BAD_ARG;
    if (q.kind != 0 && q.kind != 1) return WM_ERR_BAD_ARG;
    if (q.kind == 1 && q.count != 1) return WM_ERR_BAD_ARG;
  }
  for (int u = 0; u < b.n_utt; ++u)
    if (b.f0_len[u] > kDtwMaxLen) return WM_ERR_BAD_ARG;
  return WM_OK;
}

namespace {

struct DtwArgs {
  const float* a;
  const float* b;
  int64_t ld_a, ld_b;
  const int64_t* f_off;
  const int64_t* b_off;
  const int64_t* bp_off;     // in dwords
  const int64_t* row_off;    // in doubles
  const int* order;          // pairs, longest first
  unsigned* bp;
  double* row;
  int* flag;                 // [n_utt]: the status bits
  double* cost;
  int first, count;
};

template <int CP>
__global__ __launch_bounds__(64) void dtw_kernel(const DtwArgs p) {
#pragma clang fp contract(off)
  __shared__ float tile[CP * kDtwLdsRow];
  const int lane = threadIdx.x;
  const int u = p.order[blockIdx.x];
  const int64_t a0 = p.f_off[u], b0 = p.b_off[u];
  const int Ta = (int)(p.f_off[u + 1] - a0), Tb = (int)(p.b_off[u + 1] - b0);
  const int count = p.count;
  if (Ta < 1 || Tb < 1) {
    if (lane == 0) {
      p.flag[u] = 2;
      p.cost[u] = 0.0;
    }
    return;
  }
  const float* A = p.a + a0 * p.ld_a + p.first;
  const float* B = p.b + b0 * p.ld_b + p.first;
  {                                                           // a non-finite value in the used columns of either side
    bool bad = false;
    for (int idx = lane; idx < Ta * count; idx += 64) {
      const int r = idx / count, k = idx - r * count;
      bad = bad || !(fabsf(A[(int64_t)r * p.ld_a + k]) <= 3.402823466e+38f);
    }
    for (int idx = lane; idx < Tb * count; idx += 64) {
      const int r = idx / count, k = idx - r * count;
      bad = bad || !(fabsf(B[(int64_t)r * p.ld_b + k]) <= 3.402823466e+38f);
    }
    if (__ballot(bad) != 0) {
      if (lane == 0) {
        p.flag[u] = 1;
        p.cost[u] = __builtin_nan("");
      }
      return;
    }
  }
  const double inf = __builtin_inf();
  const int n_strips = (Ta + 63) / 64;
  const int q_rows = (Tb + 63 + 3) / 4;                       // dword rows of back-pointers per strip
  unsigned* bpw = p.bp + p.bp_off[u];
  double* rowbuf = p.row + p.row_off[u];                      // [2][Tb], touched only when n_strips > 1
  double cost = 0.0;
  for (int strip = 0; strip < n_strips; ++strip) {
    const int rows = imin(64, Ta - 64 * strip);
    const int i = 64 * strip + lane;
    const bool hand_on = strip + 1 < n_strips;                // lane 63's row feeds the next strip
    const double* prow = rowbuf + (int64_t)((strip + 1) & 1) * Tb;
    double* orow = rowbuf + (int64_t)(strip & 1) * Tb;
    double av[CP];
    {                                                         // the strip's rows of A through the tile's LDS, [row][CP + 1]:
      __syncthreads();                                        // coalesced loads, zeros beyond `rows` and `count`
#pragma unroll 4
      for (int idx = lane; idx < 64 * CP; idx += 64) {
        const int r = idx / CP, k = idx - r * CP;
        float v = 0.0f;
        if (r < rows && k < count) v = A[(int64_t)(64 * strip + r) * p.ld_a + k];
        tile[r * (CP + 1) + k] = v;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < CP; ++k) av[k] = (double)tile[lane * (CP + 1) + k];
    }
    double cur = inf, prev = inf;                             // the lane's D of the last step and of the one before
    double rb = inf, wb = 0.0, up0_last = inf;
    unsigned acc = 0;
    const int n_steps = Tb + rows - 1;
    for (int s = 0; s < n_steps; ++s) {
      if ((s & 63) == 0) {                                    // rows s .. s + 63 of B, and of the previous strip's last row
        __syncthreads();
#pragma unroll 8
        for (int it = 0; it < CP; ++it) {
          const int idx = it * 64 + lane;
          const int r = idx / CP, k = idx - r * CP;
          const int j = s + r;
          const float v = B[(int64_t)imin(j, Tb - 1) * p.ld_b + imin(k, count - 1)];
          tile[k * kDtwLdsRow + (j & (kDtwRing - 1))] = (k < count && j < Tb) ? v : 0.0f;
        }
        if (strip > 0) rb = (s + lane < Tb) ? prow[s + lane] : inf;
        __syncthreads();
      }
      const int j = s - lane;
      const bool valid = j >= 0 && j < Tb && lane < rows;
      const int jj = j & (kDtwRing - 1);
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < CP; ++k) {
        const double df = av[k] - (double)tile[k * kDtwLdsRow + jj];
        sum = __builtin_fma(df, df, sum);
      }
      const double d = sqrt(sum);
      double up = dpp_get<0x138, 0xf, 0xf>(cur);              // wave_shr:1
      double dg = dpp_get<0x138, 0xf, 0xf>(prev);
      const double up0 = strip > 0 ? readlane_d(rb, s & 63) : inf;
      if (lane == 0) {
        up = up0;
        dg = up0_last;
      }
      up0_last = up0;
      const double left = cur;
      double best;
      unsigned bp;
      if (dg <= up && dg <= left) {
        best = dg;
        bp = 0;
      } else if (up <= left) {
        best = up;
        bp = 1;
      } else {
        best = left;
        bp = 2;
      }
      if (i == 0 && j == 0) best = 0.0;
      prev = cur;
      cur = valid ? d + best : inf;
      acc |= bp << (8 * (s & 3));
      if ((s & 3) == 3 || s == n_steps - 1) {
        bpw[((int64_t)strip * q_rows + (s >> 2)) * 64 + lane] = acc;
        acc = 0;
      }
      if (hand_on && s >= 63) {                               // D(64 strip + 63, s - 63), 64 columns per store
        const int jo = s - 63;
        const double last = readlane_d(cur, 63);
        if (lane == (jo & 63)) wb = last;
        if ((jo & 63) == 63 || jo == Tb - 1) {
          if (lane <= (jo & 63)) orow[(jo & ~63) + lane] = wb;
        }
      }
    }
    cost = readlane_d(cur, rows - 1);
  }
  if (lane == 0) {
    p.flag[u] = 0;
    p.cost[u] = cost;
  }
}

struct DtwPathArgs {
  const int64_t* f_off;
  const int64_t* b_off;
  const int64_t* bp_off;
  const int* order;
  const unsigned* bp;
  const int* flag;
  int* path;                 // [sum (Ta + Tb - 1)][2]
  int* path_len;
  int* status;
};

__global__ __launch_bounds__(64) void dtw_path_kernel(const DtwPathArgs p) {
  __shared__ unsigned tile[kDtwWalkRows * 64];
  const int lane = threadIdx.x;
  const int u = p.order[blockIdx.x];
  const int64_t a0 = p.f_off[u], b0 = p.b_off[u];
  const int Ta = (int)(p.f_off[u + 1] - a0), Tb = (int)(p.b_off[u + 1] - b0);
  const int cap = imax(0, Ta + Tb - 1);
  int2* out = reinterpret_cast<int2*>(p.path) + (a0 + b0 - u);
  const int flag = p.flag[u];
  if (p.status != nullptr && lane == 0) p.status[u] = flag;
  if (flag != 0) {
    for (int n = lane; n < cap; n += 64) out[n] = make_int2(-1, -1);
    if (lane == 0) p.path_len[u] = 0;
    return;
  }
  const int q_rows = (Tb + 63 + 3) / 4;
  const unsigned* bpw = p.bp + p.bp_off[u];
  int i = Ta - 1, j = Tb - 1, pos = cap - 1;                  // every lane follows the same walk
  int at_strip = -1, q_lo = 0, q_hi = -1;
  for (int n = 0; n < cap; ++n) {
    if (lane == 0) out[pos] = make_int2(i, j);
    if ((i == 0 && j == 0) || i < 0 || j < 0) break;
    const int strip = i >> 6, l = i & 63, s = j + l, q = s >> 2;
    if (strip != at_strip || q < q_lo || q > q_hi) {
      __syncthreads();
      q_hi = q;
      q_lo = imax(0, q - (kDtwWalkRows - 1));
      for (int r = 0; r <= q_hi - q_lo; ++r) tile[r * 64 + lane] = bpw[((int64_t)strip * q_rows + q_lo + r) * 64 + lane];
      at_strip = strip;
      __syncthreads();
    }
    const unsigned bp = (tile[(q - q_lo) * 64 + l] >> (8 * (s & 3))) & 3u;
    if (bp == 0) {
      --i;
      --j;
    } else if (bp == 1) {
      --i;
    } else {
      --j;
    }
    --pos;
  }
  pos = imax(pos, 0);
  const int len = cap - pos;                                  // the pairs lie in [pos, cap): to the front, in order
  __syncthreads();
  if (pos > 0) {
    for (int c = 0; c < len; c += 64) {
      const int n = c + lane;
      int2 v = make_int2(-1, -1);
      if (n < len) v = out[pos + n];
      __syncthreads();
      if (n < len) out[n] = v;
      __syncthreads();
    }
  }
  for (int n = len + lane; n < cap; n += 64) out[n] = make_int2(-1, -1);
  if (lane == 0) p.path_len[u] = len;
}

struct DtwDistArgs {
  WorldMi355DistortionGroup g[kDtwMaxGroups];
  const int64_t* f_off;
  const int64_t* b_off;
  const int* path;
  const int* path_len;
  const unsigned char* mask;
  double voiced_above;
  double scale;              // 10 / ln 10, the host's
  double* out;               // [n_utt][n_groups][4]
  int n_groups;
};

__global__ __launch_bounds__(64) void dtw_distortion_kernel(const DtwDistArgs p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int u = blockIdx.x, gi = blockIdx.y;
  const WorldMi355DistortionGroup g = p.g[gi];
  const int64_t a0 = p.f_off[u], b0 = p.b_off[u];
  const int Ta = (int)(p.f_off[u + 1] - a0), Tb = (int)(p.b_off[u + 1] - b0);
  const int n_pairs = p.path != nullptr ? imin(p.path_len[u], imax(0, Ta + Tb - 1)) : imin(Ta, Tb);
  const int2* pairs = p.path != nullptr ? reinterpret_cast<const int2*>(p.path) + (a0 + b0 - u) : nullptr;
  const float* A = g.a + a0 * g.ld_a + g.first;
  const float* B = g.b + b0 * g.ld_b + g.first;
  const double scale = p.scale;
  double s0 = 0.0, s1 = 0.0;
  long long n0 = 0, n1 = 0, n2 = 0;
  for (int c = 0; c < n_pairs; c += 64) {
    const int n = c + lane;
    int i = n, j = n;
    if (pairs != nullptr && n < n_pairs) {
      const int2 v = pairs[n];
      i = v.x;
      j = v.y;
    }
    bool counted = n < n_pairs && i >= 0 && i < Ta && j >= 0 && j < Tb;
    if (counted && p.mask != nullptr) counted = p.mask[b0 + j] != 0;
    double e = 0.0, e2 = 0.0;
    bool both = false, differ = false;
    if (counted) {
      const float* ar = A + (int64_t)i * g.ld_a;
      const float* br = B + (int64_t)j * g.ld_b;
      if (g.kind == 0) {
        double sum = 0.0;
        for (int k = 0; k < g.count; ++k) {
          const double df = (double)ar[k] - (double)br[k];
          sum += df * df;
        }
        e = scale * sqrt(2.0 * sum);
        e2 = e * e;
      } else {
        const double av = (double)ar[0], bv = (double)br[0];
        const bool va = av > p.voiced_above, vb = bv > p.voiced_above;
        both = va && vb;
        differ = va != vb;
        if (both) {
          const double df = av - bv;
          e = df * df;
        }
      }
    }
    const int m = imin(64, n_pairs - c);
    for (int q = 0; q < m; ++q) {                             // the sums in pair order
      s0 += readlane_d(e, q);
      s1 += readlane_d(e2, q);
    }
    n0 += __popcll(__ballot(counted));
    n1 += __popcll(__ballot(both));
    n2 += __popcll(__ballot(differ));
  }
  if (lane == 0) {
    double* o = p.out + ((int64_t)u * p.n_groups + gi) * 4;
    if (g.kind == 0) {
      o[0] = s0;
      o[1] = s1;
      o[2] = (double)n0;
      o[3] = 0.0;
    } else {
      o[0] = s0;
      o[1] = (double)n1;
      o[2] = (double)n2;
      o[3] = (double)n0;
    }
  }
}

struct DtwWs : StageWs {
  unsigned* bp = nullptr;
  double* row = nullptr;
  int64_t* b_off = nullptr;
  int64_t* bp_off = nullptr;
  int64_t* row_off = nullptr;
  int* order = nullptr;
  int* flag = nullptr;
  bool with_fill = false;                                     // bp and row hold what the pairs' alignment needs
  std::vector<int64_t> h_b_off, h_bp_off, h_row_off;          // as uploaded: the copies' sources
  std::vector<int> h_order;
};

// The descriptors of the pairs belong to (the batch, b_off); a call with another b_off rebuilds them by grow_ws' rule.
// want_fill: the back-pointer and row buffers too (DtwAlign); FeatureDistortion alone needs b_off on the device only.
int ensure_ws(Batch& b, hipStream_t st, const int64_t* b_off, bool want_fill, DtwWs*& W) {
  const size_t n = (size_t)b.n_utt;
  auto same = [&](const DtwWs& w) {
    return w.h_b_off.size() == n + 1 && memcmp(w.h_b_off.data(), b_off, 8 * (n + 1)) == 0;
  };
  if (b.dtw && same(static_cast<const DtwWs&>(*b.dtw)))       // a rebuilt workspace serves the earlier calls too
    want_fill = want_fill || static_cast<const DtwWs&>(*b.dtw).with_fill;
  return grow_ws(b.dtw, st, W, [&](const DtwWs& w) { return same(w) && (w.with_fill || !want_fill); }, [&](DtwWs& w) {
    const DtwPlan plan(b.n_utt, b.f0_len.data(), b_off);
    w.with_fill = want_fill;
    if (const int r = wm_check(w.alloc(&w.bp, want_fill ? plan.bytes[0] : 4))) return r;
    if (const int r = wm_check(w.alloc(&w.row, want_fill ? plan.bytes[1] : 8))) return r;
    if (const int r = wm_check(w.alloc(&w.b_off, plan.bytes[2]))) return r;
    if (const int r = wm_check(w.alloc(&w.bp_off, plan.bytes[3]))) return r;
    if (const int r = wm_check(w.alloc(&w.row_off, plan.bytes[4]))) return r;
    if (const int r = wm_check(w.alloc(&w.order, plan.bytes[5]))) return r;
    if (const int r = wm_check(w.alloc(&w.flag, plan.bytes[6]))) return r;
    w.h_b_off.assign(b_off, b_off + n + 1);
    w.h_bp_off.assign(n + 1, 0);
    w.h_row_off.assign(n + 1, 0);
    std::vector<int64_t> cells(n, 0);
    for (size_t u = 0; u < n; ++u) {
      const int tb = (int)(b_off[u + 1] - b_off[u]);
      w.h_bp_off[u + 1] = w.h_bp_off[u] + dtw_bp_dwords(b.f0_len[u], tb);
      w.h_row_off[u + 1] = w.h_row_off[u] + dtw_row_doubles(b.f0_len[u], tb);
      cells[u] = (int64_t)b.f0_len[u] * tb;
    }
    w.h_order.resize(n);
    std::iota(w.h_order.begin(), w.h_order.end(), 0);
    std::stable_sort(w.h_order.begin(), w.h_order.end(), [&](int x, int y) { return cells[(size_t)x] > cells[(size_t)y]; });
    if (const int r = wm_check(hipMemcpyAsync(w.b_off, w.h_b_off.data(), 8 * (n + 1), hipMemcpyHostToDevice, st))) return r;
    if (const int r = wm_check(hipMemcpyAsync(w.bp_off, w.h_bp_off.data(), 8 * (n + 1), hipMemcpyHostToDevice, st))) return r;
    if (const int r = wm_check(hipMemcpyAsync(w.row_off, w.h_row_off.data(), 8 * (n + 1), hipMemcpyHostToDevice, st))) return r;
    return wm_check(hipMemcpyAsync(w.order, w.h_order.data(), 4 * n, hipMemcpyHostToDevice, st));
  });
}

}  // namespace

int launch_dtw_align(Batch& b, hipStream_t st, const float* d_a, int64_t ld_a, const float* d_b, int64_t ld_b,
                     const int64_t* b_off, int first, int count, int* d_path, int* d_path_len, double* d_cost,
                     int* d_status) {
  if (const int rc = check_dtw(b, d_a, ld_a, d_b, ld_b, b_off, first, count, d_path, d_path_len, d_cost)) return rc;
  DtwWs* W = nullptr;
  if (const int rc = ensure_ws(b, st, b_off, true, W)) return rc;
  DtwArgs a;
  memset(&a, 0, sizeof(a));
  a.a = d_a;
  a.b = d_b;
  a.ld_a = ld_a;
  a.ld_b = ld_b;
  a.f_off = b.d_f_off;
  a.b_off = W->b_off;
  a.bp_off = W->bp_off;
  a.row_off = W->row_off;
  a.order = W->order;
  a.bp = W->bp;
  a.row = W->row;
  a.flag = W->flag;
  a.cost = d_cost;
  a.first = first;
  a.count = count;
  const dim3 grid((unsigned)b.n_utt), block(64);
  {
    TimedScope ts_(b.ctx, st, "dtw_kernel");
    if (count <= 8)
      hipLaunchKernelGGL(dtw_kernel<8>, grid, block, 0, st, a);
    else if (count <= 16)
      hipLaunchKernelGGL(dtw_kernel<16>, grid, block, 0, st, a);
    else if (count <= 32)
      hipLaunchKernelGGL(dtw_kernel<32>, grid, block, 0, st, a);
    else if (count <= 48)
      hipLaunchKernelGGL(dtw_kernel<48>, grid, block, 0, st, a);
    else if (count <= 56)
      hipLaunchKernelGGL(dtw_kernel<56>, grid, block, 0, st, a);
    else
      hipLaunchKernelGGL(dtw_kernel<64>, grid, block, 0, st, a);
  }
  if (const int rc = wm_check(hipGetLastError())) return rc;
  DtwPathArgs q;
  memset(&q, 0, sizeof(q));
  q.f_off = b.d_f_off;
  q.b_off = W->b_off;
  q.bp_off = W->bp_off;
  q.order = W->order;
  q.bp = W->bp;
  q.flag = W->flag;
  q.path = d_path;
  q.path_len = d_path_len;
  q.status = d_status;
  {
    TimedScope ts_(b.ctx, st, "dtw_path_kernel");
    hipLaunchKernelGGL(dtw_path_kernel, grid, block, 0, st, q);
  }
  return wm_check(hipGetLastError());
}

int launch_feature_distortion(Batch& b, hipStream_t st, const int* d_path, const int* d_path_len, const int64_t* b_off,
                              const unsigned char* d_b_mask, int n_groups, const WorldMi355DistortionGroup* groups,
                              const WorldMi355DistortionOption& opt, double* d_out) {
  if (const int rc = check_distortion(b, d_path, d_path_len, b_off, n_groups, groups, &opt, d_out)) return rc;
  DtwWs* W = nullptr;
  if (const int rc = ensure_ws(b, st, b_off, false, W)) return rc;
  DtwDistArgs a;
  memset(&a, 0, sizeof(a));
  for (int g = 0; g < n_groups; ++g) a.g[g] = groups[g];
  a.f_off = b.d_f_off;
  a.b_off = W->b_off;
  a.path = d_path;
  a.path_len = d_path_len;
  a.mask = d_b_mask;
  a.voiced_above = opt.voiced_above;
  a.scale = 10.0 / log(10.0);
  a.out = d_out;
  a.n_groups = n_groups;
  TimedScope ts_(b.ctx, st, "dtw_distortion_kernel");
  hipLaunchKernelGGL(dtw_distortion_kernel, dim3((unsigned)b.n_utt, (unsigned)n_groups), dim3(64), 0, st, a);
  return wm_check(hipGetLastError());
}

}  // namespace wm
