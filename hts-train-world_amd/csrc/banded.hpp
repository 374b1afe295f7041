// banded.hpp -- what mlpg_kernel<B> (mlpg.hip) and trj_kernel<B> (trj.hip) share: the banded LDL' of R = W' P W in
// double, right-looking, one column (utterance, stream, dimension) per lane and one wave per (utterance, stream, 64
// dimensions), B = 2 max h_i the half-bandwidth and a template parameter.
//   host    streams are grouped by B, one launch per group; band_plan lays the streams' workspaces out and checks the
//           grid, band_group fills a group's table;
//   device  the block -> (stream, utterance, column) decode, the stream's taps in LDS, the interior row fi of R, and
//           the pivot step: the updates earlier pivots owe a row wait in a register triangle D[a][j] (row t + a,
//           offset j), which every pivot shifts by one row IN the multiply-add that updates it, so the triangle is
//           indexed at compile time and never moves.
#pragma once
#include "streamwin.hpp"

namespace wm {

// The streams of one launch: a window table with what the decode and the factor need beside it.
template <int TAPS>
struct BandTable {
  int n_streams;                                  // of this launch: the streams that share one B
  int hmax[kWinMaxStreams];
  int chunks[kWinMaxStreams], blk0[kWinMaxStreams];            // 64-lane chunks per utterance; first block of the stream
  int64_t ws_off[kWinMaxStreams];                 // in doubles
  WinTable<TAPS> win;
};

// the instantiation that holds a stream's band (half-bandwidth 2 max h_i)
constexpr int kBands[4] = {0, 2, 4, 14};
inline int band_of(int hmax) { return hmax == 0 ? 0 : hmax == 1 ? 2 : hmax == 2 ? 4 : 14; }

struct BandPlan {
  int hmax[kWinMaxStreams], band[kWinMaxStreams];
  int64_t ws_off[kWinMaxStreams], need;           // in doubles
};

// Every stream's band and its place in the workspace, which holds ws_cols(B) doubles per frame and column of a stream.
template <class WsCols>
inline int band_plan(BandPlan& p, int n_streams, const int* dims, const int* n_windows, const int* const* window_sizes,
                     int64_t total_f, int n_utt, WsCols ws_cols) {
  p.need = 0;
  for (int s = 0; s < n_streams; ++s) {
    p.hmax[s] = win_hmax(n_windows[s], window_sizes[s]);
    p.band[s] = band_of(p.hmax[s]);
    p.ws_off[s] = p.need;
    p.need += total_f * (int64_t)ws_cols(p.band[s]) * dims[s];
    if (((int64_t)dims[s] + 63) / 64 * n_utt > (int64_t)1 << 28) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

// The streams of band B into the zeroed t, src[k] the stream in slot k; returns the launch's blocks.
template <int TAPS>
inline int band_group(BandTable<TAPS>& t, int (&src)[kWinMaxStreams], const BandPlan& p, int B, int n_streams,
                      const int* dims, const int* n_windows, const double* const* const* windows,
                      const int* const* window_sizes, int n_utt) {
  int blocks = 0;
  for (int s = 0; s < n_streams; ++s) {
    if (p.band[s] != B) continue;
    const int k = t.n_streams++;
    src[k] = s;
    win_fill(t.win, k, s, dims, n_windows, windows, window_sizes);
    t.hmax[k] = p.hmax[s];
    t.chunks[k] = (dims[s] + 63) / 64;
    t.blk0[k] = blocks;
    blocks += t.chunks[k] * n_utt;
    t.ws_off[k] = p.ws_off[s];
  }
  return blocks;
}

// block -> (stream slot, utterance, column); by value: through references the kernels took one scalar register more
struct BandBlock { int s, u, col; };
template <int TAPS>
__device__ __forceinline__ BandBlock band_decode(const BandTable<TAPS>& t) {
  int s = 0;
#pragma unroll
  for (int q = 1; q < kWinMaxStreams; ++q)
    if (q < t.n_streams && (int)blockIdx.x >= t.blk0[q]) s = q;
  const int rel = (int)blockIdx.x - t.blk0[s];
  const int u = rel / t.chunks[s];
  return {s, u, (rel - u * t.chunks[s]) * 64 + (int)threadIdx.x};
}

// Stream s' taps as the block keeps them in LDS: window i at wz[i][0 .. size), zeros up to ROW, so that an index up to
// 2 h_i + B needs no range check.  The caller's __syncthreads follows.
template <int ROW, int TAPS>
__device__ __forceinline__ void band_stage_taps(const BandTable<TAPS>& t, int s, double (*wz)[ROW]) {
  for (int e = (int)threadIdx.x; e < kWinMaxWin * ROW; e += 64) {
    const int i = e / ROW, k = e - i * ROW;
    wz[i][k] = i < t.win.nwin[s] && k < t.win.wsize[s][i] ? t.win.w[s][i][k < TAPS ? k : 0] : 0.0;
  }
}

// fi[j] += p sum_k w[k] w[k + j]: with one variance row, a window's share of every row of R away from the ends
template <int B>
__device__ __forceinline__ void band_fi_add(double p, const double* w, int size, double (&fi)[B + 1]) {
  for (int k = 0; k < size; ++k) {
    const double pk = p * w[k];
#pragma unroll
    for (int j = 0; j <= B; ++j) fi[j] = __builtin_fma(pk, w[k + j], fi[j]);
  }
}

// The pivot at row t, whose row e of R and right-hand side z have taken D[0] and q[0] in: the multipliers l_a = e[a] / d
// to wr[a * dim], and what rows t + 1 .. t + B owe to it into the triangle, which moves up one row.
template <int B, int BB>
__device__ __forceinline__ void band_pivot(const double (&e)[B + 1], double z, double inv, double (&D)[BB][BB],
                                           double (&q)[BB], double* wr, int64_t dim) {
#pragma unroll
  for (int a = 1; a <= B; ++a) {
    const double l = e[a] * inv;
    wr[(int64_t)a * dim] = l;
    // row t + a becomes row (t + 1) + (a - 1): the shift is the destination of the update
#pragma unroll
    for (int j = 0; j + a <= B; ++j)
      D[a - 1][j] = __builtin_fma(-l, e[a + j], (a < B && j + a < B) ? D[a < B ? a : 0][j] : 0.0);
    q[a - 1] = __builtin_fma(-l, z, a < B ? q[a < B ? a : 0] : 0.0);
  }
}
}  // namespace wm
