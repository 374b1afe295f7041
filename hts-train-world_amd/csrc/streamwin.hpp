// streamwin.hpp -- the stream/window argument bundle (n_streams, dims, n_windows, windows, window_sizes) that
// WorldMi355ComposeCmp, ComposeFfo, ParameterGeneration and TrajectoryCost take: its limits, its one host validator,
// the table the kernels' by-value metadata embeds with its one fill, and the `cmp` row's window sum, which
// cmp_compose_kernel (codec.hip) and ffo_compose_kernel (ffo.hip) both evaluate.
#pragma once
#include <string.h>

#include "batch.hpp"

namespace wm {

constexpr int kWinMaxStreams = 4, kWinMaxWin = 4, kWinMaxTaps = 15;
constexpr int kTrjMaxTaps = 5;                    // the trajectory criterion's windows: TrjMeta holds this many per window

// What every entry point refuses in the bundle, on the host alone.  A caller's own check keeps what is its own: data
// pointers, strides, options and outputs.
inline int check_windows(int n_streams, const int* dims, const int* n_windows, const double* const* const* windows,
                         const int* const* window_sizes, int max_streams, int max_win, int max_taps) {
  if (!dims || !n_windows || !windows || !window_sizes) return WM_ERR_BAD_ARG;
  if (n_streams < 1 || n_streams > max_streams) return WM_ERR_BAD_ARG;
  for (int s = 0; s < n_streams; ++s) {
    if (!windows[s] || !window_sizes[s]) return WM_ERR_BAD_ARG;
    if (dims[s] < 1 || n_windows[s] < 1 || n_windows[s] > max_win) return WM_ERR_BAD_ARG;
    for (int i = 0; i < n_windows[s]; ++i) {
      const int size = window_sizes[s][i];
      if (!windows[s][i] || size < 1 || size > max_taps || size % 2 != 1) return WM_ERR_BAD_ARG;   // window.pl:96-98
    }
  }
  return WM_OK;
}

// The windows of up to kWinMaxStreams streams as a kernel receives them, TAPS values per window.
template <int TAPS>
struct WinTable {
  int dim[kWinMaxStreams], nwin[kWinMaxStreams];
  int wsize[kWinMaxStreams][kWinMaxWin];
  double w[kWinMaxStreams][kWinMaxWin][TAPS];
};

// Stream s of a checked bundle into slot k of a zeroed table.
template <int TAPS>
inline void win_fill(WinTable<TAPS>& t, int k, int s, const int* dims, const int* n_windows,
                     const double* const* const* windows, const int* const* window_sizes) {
  t.dim[k] = dims[s];
  t.nwin[k] = n_windows[s];
  for (int i = 0; i < n_windows[s]; ++i) {
    const int size = window_sizes[s][i];
    t.wsize[k][i] = size;
    for (int j = 0; j < size; ++j) t.w[k][i][j] = windows[s][i][j];
  }
}

// a stream's largest centre tap, max h_i
inline int win_hmax(int n_windows, const int* window_sizes) {
  int hmax = 0;
  for (int i = 0; i < n_windows; ++i) hmax = hmax > (window_sizes[i] - 1) / 2 ? hmax : (window_sizes[i] - 1) / 2;
  return hmax;
}

// ---- the `cmp` row: out[frame] = [stream 0: win 1 | win 2 | ... ][stream 1: ...]... -------------------------------
struct CmpMeta {
  int n_streams, total_cols;
  WinTable<kWinMaxTaps> win;
  int col0[kWinMaxStreams];
  unsigned chk[kWinMaxStreams][kWinMaxWin];                 // bit k: tap k takes part in the boundary check
  const float* data[kWinMaxStreams];
};

// One value of the composed row: window wi of stream s at dim j of `frame`, whose utterance covers frames lo .. hi.
__device__ __forceinline__ float cmp_window_value(const CmpMeta& m, int s, int wi, int j, int64_t frame, int64_t lo,
                                                  int64_t hi) {
#pragma clang fp contract(off)
  const int dim = m.win.dim[s];
  const int size = m.win.wsize[s][wi], nlr = (size - 1) / 2;
  const float* src = m.data[s];
  bool boundary = false;
  double acc = 0.0;
  for (int k = 0; k < size; ++k) {
    int64_t l = frame + (k - nlr);
    l = l < lo ? lo : (l > hi ? hi : l);
    const double v = (double)src[l * dim + j];
    if (((m.chk[s][wi] >> k) & 1u) && v == -1.0e+10) boundary = true;
    acc += m.win.w[s][wi][k] * v;
  }
  return boundary ? -1.0e+10f : (float)acc;
}

// the streams of a checked bundle into m; col0 and total_cols are the `cmp` row's
inline void cmp_fill_meta(CmpMeta& m, int n_streams, const float* const* d_data, const int* dims, const int* n_windows,
                          const double* const* const* windows, const int* const* window_sizes) {
  memset(&m, 0, sizeof(m));
  m.n_streams = n_streams;
  int col = 0;
  for (int s = 0; s < n_streams; ++s) {
    win_fill(m.win, s, s, dims, n_windows, windows, window_sizes);
    m.col0[s] = col;
    m.data[s] = d_data[s];
    for (int i = 0; i < n_windows[s]; ++i) {
      const int size = window_sizes[s][i];
      unsigned chk = (1u << size) - 1u;                           // window.pl:83-94: leading / trailing zero taps
      for (int k = 0; k < size; ++k) { if (windows[s][i][k] != 0.0) break; chk &= ~(1u << k); }
      for (int k = size - 1; k >= 0; --k) { if (windows[s][i][k] != 0.0) break; chk &= ~(1u << k); }
      m.chk[s][i] = chk;
    }
    col += dims[s] * n_windows[s];
  }
  m.total_cols = col;
}

}  // namespace wm
