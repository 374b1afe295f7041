// dnn_train.hip -- the training pass of the recipe's acoustic model (data/scripts/DNNTraining.py with
// DNNDefine.inference at keep_prob < 1, DNNDefine.cost and their gradients), for a whole batch of utterances.  It shares
// dnn.hip's tile conventions, activation codes, input check and workspace through dnn.hpp.
//
// Forward with dropout (TF 1.x tf.nn.dropout, div(x, keep_prob) * mask), per frame t of utterance u with speaker s(u):
//   a_i = act_h((h_{i-1} W_i + b_i) + sd_i[s(u)]),   h_i = m ? fl(a_i / p) : 0,   out = act_o(h_{L-1} W_o + b_o),
// m the Philox4x32-10 mask of (seed, offset, layer i, batch row t, unit n): it does not depend on the chunk or the tile.
// Backward from G = dloss/dout:
//   dz_o = G act_o'(out),  dh_{i-1} = dz_i W_i',  da_i = m ? fl(dh_i / p) : 0,  dz_i = da_i act_h'(a_i),
//   dW_i = h_{i-1}' dz_i,  db_i = sum_t dz_i,  dsd_i[s] = sum over the rows of speaker s.
// The three matrix products run on one tile engine (dnn_gemm_tile: 128 x 128 x 32 tiles, 2 x 2 accumulators of 32 x 32 per
// wave on v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain); an operand is read either along its reduction index and
// transposed into LDS (TRANS) or along its output index and copied (direct):
//   dnn_train_layer_kernel   C = A W          A TRANS,  W direct     epilogue: bias, speaker row, activation, mask
//                            (a layer without a mask -- the output layer, every layer at keep_prob 1 -- is dnn_layer_kernel)
//   dnn_dgrad_kernel         dh = dz W'       dz TRANS, W TRANS      epilogue: mask / p, act'(a)
//   dnn_wgrad_kernel         dW = h' dz       h direct, dz direct    accumulators loaded from dW after the first chunk,
// so that dW is one chain over the batch's rows in order, whatever the chunking.  Everything beyond M / N / K is zero in
// LDS and is never read from memory.  A flagged utterance's rows of dz are zero and its rows of h (or x) read as zero in
// dnn_wgrad_kernel: it adds exact zeros to every gradient.
// db and dsd: dnn_colsum_kernel sums an utterance's rows in double in column_moments_kernel's order (groups of 32 frames
// dealt to four waves, a lane per column); an utterance cut by a chunk boundary carries its four wave sums and its open
// group's sum to the next chunk, so the order depends on the utterance's length alone.  dnn_fold_kernel adds the
// finished utterances in order into double accumulators and rounds once.  No atomics on any value.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "batch.hpp"
#include "common.hpp"
#include "dnn.hpp"

namespace wm {

struct DnnMask {
  float p;                 // keep_prob; 1: no dropout
  uint32_t k0, k1;         // seed & 0xffffffff, seed >> 32
  uint32_t offset;         // the caller's step counter
};

// Philox4x32-10 (Salmon et al., SC'11): word n & 3 of counter (t, n >> 2, layer, offset).
__device__ __forceinline__ uint32_t dnn_philox_word(uint32_t t, uint32_t n, uint32_t layer, const DnnMask& d) {
  uint32_t c0 = t, c1 = n >> 2, c2 = layer, c3 = d.offset, k0 = d.k0, k1 = d.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const uint32_t w = (n & 3u) == 0 ? c0 : (n & 3u) == 1 ? c1 : (n & 3u) == 2 ? c2 : c3;
  return w;
}
__device__ __forceinline__ bool dnn_keep(uint32_t t, uint32_t n, uint32_t layer, const DnnMask& d) {
  return (float)(dnn_philox_word(t, n, layer, d) >> 8) * 5.9604644775390625e-8f < d.p;     // exact: r < 2^24
}

// The masks of a lane's 64 accumulator elements (bit b * 32 + a * 16 + r: accumulator tile (a, b), register r), in a
// loop that stays rolled: sixty-four interleaved Philox chains would not fit the register file.
__device__ __forceinline__ uint64_t dnn_keep_bits(uint32_t row_base, uint32_t col_base, uint32_t layer, const DnnMask& d) {
  uint64_t bits = 0;
#pragma unroll 1
  for (int e = 0; e < 64; ++e) {
    const uint32_t r = (uint32_t)e & 15u;
    const uint32_t row = row_base + (((uint32_t)e >> 4) & 1u) * 32u + (r & 3u) + 8u * (r >> 2);
    if (dnn_keep(row, col_base + ((uint32_t)e >> 5) * 32u, layer, d)) bits |= (uint64_t)1 << e;
  }
  return bits;
}

// the derivative from the float32 activation value
template <int ACT> __device__ __forceinline__ float dnn_act_deriv(float a) {
  if (ACT == 1) return a * (1.0f - a);
  if (ACT == 2) return 1.0f - a * a;
  if (ACT == 3) return a > 0.0f ? 1.0f : 0.0f;
  return 1.0f;
}

// An operand of a tile product: element (outer o, reduction r) at p[o * ld + r] (TRANS) or p[r * ld + o] (direct).
struct DnnOperand {
  const float* p;
  int64_t ld;
  int vec;                 // 16-byte loads are possible
  const int* frame_utt;    // direct only, or null: a reduction row of a flagged utterance reads as zeros
  const int* status;
};

template <bool TRANS>
__device__ __forceinline__ void dnn_fetch(const DnnOperand& s, int outer0, int n_outer, int red0, int n_red, int tid,
                                          float4 (&reg)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // TRANS: outer tid >> 3 + 32 i, four reduction indices from (tid & 7) 4; direct: reduction tid >> 5 + 8 i, four outer
    const int o = TRANS ? outer0 + (tid >> 3) + 32 * i : outer0 + (tid & 31) * 4;
    const int r = TRANS ? red0 + (tid & 7) * 4 : red0 + (tid >> 5) + 8 * i;
    const int along = TRANS ? r : o, n_along = TRANS ? n_red : n_outer;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool live = o < n_outer && r < n_red;
    if (!TRANS && live && s.status != nullptr) live = s.status[s.frame_utt[r]] == 0;
    if (live) {
      const float* src = TRANS ? s.p + (int64_t)o * s.ld + r : s.p + (int64_t)r * s.ld + o;
      if (s.vec && along + 3 < n_along) {
        v = *reinterpret_cast<const float4*>(src);
      } else {
        v.x = src[0];
        if (along + 1 < n_along) v.y = src[1];
        if (along + 2 < n_along) v.z = src[2];
        if (along + 3 < n_along) v.w = src[3];
      }
    }
    reg[i] = v;
  }
}

template <bool TRANS> __device__ __forceinline__ void dnn_stash(float* lds, int tid, const float4 (&reg)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (TRANS) {
      float* dst = lds + (tid & 7) * 4 * kDnnLd + (tid >> 3) + 32 * i;
      dst[0] = reg[i].x;
      dst[kDnnLd] = reg[i].y;
      dst[2 * kDnnLd] = reg[i].z;
      dst[3 * kDnnLd] = reg[i].w;
    } else {
      *reinterpret_cast<float4*>(lds + ((tid >> 5) + 8 * i) * kDnnLd + (tid & 31) * 4) = reg[i];
    }
  }
}

// acc += A B over the reduction 0 .. K - 1 in order, for the 128 x 128 tile at (row0, col0) of an M x N product; the
// wave's accumulators as in dnn_layer_kernel.
template <bool TA, bool TB>
__device__ __forceinline__ void dnn_gemm_tile(const DnnOperand& A, const DnnOperand& B, int M, int N, int K, int row0,
                                              int col0, dnn_f32x16 (&acc)[2][2]) {
  __shared__ __attribute__((aligned(16))) float As[kDnnBK * kDnnLd];   // [k][row]
  __shared__ __attribute__((aligned(16))) float Bs[kDnnBK * kDnnLd];   // [k][column]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
  float4 ra[4], rb[4];
  dnn_fetch<TA>(A, row0, M, 0, K, tid, ra);
  dnn_fetch<TB>(B, col0, N, 0, K, tid, rb);
  for (int k0 = 0; k0 < K; k0 += kDnnBK) {
    dnn_stash<TA>(As, tid, ra);
    dnn_stash<TB>(Bs, tid, rb);
    __syncthreads();
    if (k0 + kDnnBK < K) {
      dnn_fetch<TA>(A, row0, M, k0 + kDnnBK, K, tid, ra);
      dnn_fetch<TB>(B, col0, N, k0 + kDnnBK, K, tid, rb);
    }
    const float* ap = As + half * kDnnLd + wm * 64 + l31;
    const float* bp = Bs + half * kDnnLd + wn * 64 + l31;
#pragma unroll
    for (int kk = 0; kk < kDnnBK; kk += 2) {
      const float a0 = ap[kk * kDnnLd], a1 = ap[kk * kDnnLd + 32];
      const float b0 = bp[kk * kDnnLd], b1 = bp[kk * kDnnLd + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void dnn_acc_zero(dnn_f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
}

struct DnnTrainLayer {
  DnnOperand A, W;         // A [M][K] TRANS, W [K][N] direct
  const float* bias;
  const float* sd;         // null, or [n_spkrs][N]
  const int* spk;
  const int* frame_utt;    // of row 0 of this chunk
  float* act;              // null, or a [M][N] contiguous (kept for the backward pass)
  float* C;                // h = m ? a / p : 0, [M][N] contiguous
  int64_t ldc;
  int M, N, K, tiles_n;
  uint32_t t0, layer;      // batch row of row 0; the layer of the mask
  DnnMask mask;
};

template <int ACT>
__global__ __launch_bounds__(256) void dnn_train_layer_kernel(DnnTrainLayer p) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int tile_m = (int)(blockIdx.x / (unsigned)p.tiles_n), tile_n = (int)blockIdx.x - tile_m * p.tiles_n;
  const int row0 = tile_m * kDnnBM, col0 = tile_n * kDnnBN;
  const int M = p.M, N = p.N;
  dnn_f32x16 acc[2][2];
  dnn_acc_zero(acc);
  dnn_gemm_tile<true, false>(p.A, p.W, M, N, p.K, row0, col0, acc);
  const uint64_t kept = dnn_keep_bits(p.t0 + (uint32_t)(row0 + wm * 64 + 4 * half), (uint32_t)(col0 + wn * 64 + l31), p.layer,
                                      p.mask);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int col = col0 + wn * 64 + b * 32 + l31;
    if (col >= N) continue;
    const float bias = p.bias[col];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row >= M) continue;
        float v = acc[a][b][r] + bias;
        if (p.sd != nullptr) v = v + p.sd[(int64_t)p.spk[p.frame_utt[row]] * N + col];
        v = dnn_act<ACT>(v);
        if (p.act != nullptr) p.act[(int64_t)row * N + col] = v;
        v = ((kept >> (b * 32 + a * 16 + r)) & 1) != 0 ? v / p.mask.p : 0.0f;
        p.C[(int64_t)row * p.ldc + col] = v;
      }
    }
  }
}

struct DnnDgrad {
  DnnOperand dz, W;        // dz [M][N] TRANS (reduction n), W [K][N] TRANS (outer k, reduction n)
  const float* act;        // a of the layer below, [M][K] contiguous
  const int* frame_utt;
  const int* status;
  float* out;              // dz of the layer below, [M][K] contiguous
  int M, N, K, tiles_n;    // tiles_n over K
  uint32_t t0, layer;      // the layer below: its mask
  DnnMask mask;
};

template <int ACT, bool DROP>
__global__ __launch_bounds__(256) void dnn_dgrad_kernel(DnnDgrad p) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int tile_m = (int)(blockIdx.x / (unsigned)p.tiles_n), tile_n = (int)blockIdx.x - tile_m * p.tiles_n;
  const int row0 = tile_m * kDnnBM, col0 = tile_n * kDnnBN;
  const int M = p.M, K = p.K;
  dnn_f32x16 acc[2][2];
  dnn_acc_zero(acc);
  dnn_gemm_tile<true, true>(p.dz, p.W, M, K, p.N, row0, col0, acc);
  const uint64_t kept = DROP ? dnn_keep_bits(p.t0 + (uint32_t)(row0 + wm * 64 + 4 * half), (uint32_t)(col0 + wn * 64 + l31),
                                             p.layer, p.mask) : 0;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int col = col0 + wn * 64 + b * 32 + l31;
    if (col >= K) continue;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row >= M) continue;
        float v = 0.0f;
        if (p.status[p.frame_utt[row]] == 0) {
          v = acc[a][b][r];
          if (DROP) v = ((kept >> (b * 32 + a * 16 + r)) & 1) != 0 ? v / p.mask.p : 0.0f;
          v = v * dnn_act_deriv<ACT>(p.act[(int64_t)row * K + col]);
        }
        p.out[(int64_t)row * K + col] = v;
      }
    }
  }
}

struct DnnWgrad {
  DnnOperand h, dz;        // h [rows][K] direct (outer k), dz [rows][N] direct (outer n); reduction: the rows
  float* dW;               // [K][N] contiguous
  int rows, N, K, tiles_n;
  int accumulate;          // a chunk after the first: the chain goes on from dW
};

__global__ __launch_bounds__(256) void dnn_wgrad_kernel(DnnWgrad p) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int tile_m = (int)(blockIdx.x / (unsigned)p.tiles_n), tile_n = (int)blockIdx.x - tile_m * p.tiles_n;
  const int row0 = tile_m * kDnnBM, col0 = tile_n * kDnnBN;
  const int K = p.K, N = p.N;
  dnn_f32x16 acc[2][2];
  dnn_acc_zero(acc);
  if (p.accumulate) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = col0 + wn * 64 + b * 32 + l31;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (row < K && col < N) acc[a][b][r] = p.dW[(int64_t)row * N + col];
        }
      }
    }
  }
  dnn_gemm_tile<false, false>(p.h, p.dz, K, N, p.rows, row0, col0, acc);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int col = col0 + wn * 64 + b * 32 + l31;
    if (col >= N) continue;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < K) p.dW[(int64_t)row * N + col] = acc[a][b][r];
      }
    }
  }
}

// dz_o = G act_o'(out), in place over `out` [rows][D] contiguous; zeros in the rows of a flagged utterance.
template <int ACT>
__global__ __launch_bounds__(256) void dnn_dzo_kernel(float* __restrict__ out, const float* __restrict__ G, int64_t ld_g, int D,
                                                      int64_t rows, const int* __restrict__ frame_utt,
                                                      const int* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= rows * D) return;
  const int64_t t = e / D;
  const int d = (int)(e - t * D);
  float v = 0.0f;
  if (status[frame_utt[t]] == 0) v = G[t * ld_g + d] * dnn_act_deriv<ACT>(out[e]);
  out[e] = v;
}

// Block (utterance u0 + blockIdx / colchunks, 64 columns): the rows of the utterance that lie in this chunk (batch rows
// r0 .. r0 + rows - 1; dz holds them from row 0), summed in column_moments_kernel's order.  state: [4 waves][s, open
// group][max_n]; read when the utterance began in an earlier chunk, written when it goes on in the next.
__global__ __launch_bounds__(256) void dnn_colsum_kernel(const float* __restrict__ dz, int64_t ld, int N, int colchunks, int u0,
                                                         int64_t r0, int64_t rows, const int64_t* __restrict__ f_off,
                                                         const double* __restrict__ st_in, double* __restrict__ st_out,
                                                         int max_n, double* __restrict__ U) {
#pragma clang fp contract(off)
  const int u = u0 + (int)(blockIdx.x / (unsigned)colchunks);
  const int lane = (int)threadIdx.x & 63, q = (int)threadIdx.x >> 6;
  const int col = ((int)blockIdx.x - (u - u0) * colchunks) * 64 + lane;
  const int64_t fb = f_off[u], T = f_off[u + 1] - fb;
  const int64_t lo = fb > r0 ? fb : r0, hi = fb + T < r0 + rows ? fb + T : r0 + rows;
  if (hi <= lo) return;
  const int64_t ta = lo - fb, tb = hi - fb;
  const bool on = col < N;
  __shared__ double part[4][64];
  double s = 0.0, open = 0.0, p_in = 0.0;
  if (on) {
    if (ta > 0) {
      s = st_in[(int64_t)(q * 2) * max_n + col];
      p_in = st_in[(int64_t)(q * 2 + 1) * max_n + col];
    }
    const int64_t g0 = ta / 32;
    for (int64_t g = g0 + ((q - (int)(g0 & 3)) & 3); 32 * g < tb; g += 4) {
      const int64_t t0 = 32 * g > ta ? 32 * g : ta;
      const int64_t t1 = 32 * g + 32 < tb ? 32 * g + 32 : tb;
      double p = 32 * g < ta ? p_in : 0.0;
      for (int64_t t = t0; t < t1; ++t) p += (double)dz[(fb + t - r0) * ld + col];
      if (t1 == 32 * g + 32 || t1 == T) s += p; else open = p;
    }
  }
  if (tb < T) {
    if (on) {
      st_out[(int64_t)(q * 2) * max_n + col] = s;
      st_out[(int64_t)(q * 2 + 1) * max_n + col] = open;
    }
    return;
  }
  part[q][lane] = s;
  __syncthreads();
  if (q == 0 && on) U[(int64_t)u * max_n + col] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// A thread per column: the utterances ua .. ub - 1 (those that end in this chunk) join the double accumulators in order
// (acc row 0: db; row 1 + s: dsd of speaker s), and the float32 gradients are rewritten from them.
__global__ __launch_bounds__(256) void dnn_fold_kernel(const double* __restrict__ U, int max_n, int N, int ua, int ub,
                                                       const int64_t* __restrict__ f_off, const int* __restrict__ spk,
                                                       double* __restrict__ acc, int n_spkrs, float* __restrict__ db,
                                                       float* __restrict__ dsd) {
#pragma clang fp contract(off)
  const int n = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (n >= N) return;
  for (int u = ua; u < ub; ++u) {
    if (f_off[u + 1] <= f_off[u]) continue;
    const double v = U[(int64_t)u * max_n + n];
    if (db != nullptr) acc[n] += v;
    if (dsd != nullptr) acc[(int64_t)(1 + spk[u]) * max_n + n] += v;
  }
  if (db != nullptr) db[n] = (float)acc[n];
  if (dsd != nullptr)
    for (int s = 0; s < n_spkrs; ++s) dsd[(int64_t)s * N + n] = (float)acc[(int64_t)(1 + s) * max_n + n];
}

// dnn_cost_kernel with the two gradients of the cost: one block per utterance, the same sums in the same order.
__global__ __launch_bounds__(256) void dnn_cost_grad_kernel(float* __restrict__ out, int64_t ld_out, const float* __restrict__ obs,
                                                            int64_t ld_obs, const float* __restrict__ variances,
                                                            const int* __restrict__ spk, int D,
                                                            const int64_t* __restrict__ f_off, int* __restrict__ status,
                                                            double* __restrict__ cost, float* __restrict__ grad_out,
                                                            int64_t ld_grad, double* __restrict__ grad_var, int want) {
#pragma clang fp contract(off)
  const int u = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t fb = f_off[u];
  const int64_t T = f_off[u + 1] - fb;
  __shared__ int flag;
  __shared__ double part[4][64], red[2][64];
  const float inf = __builtin_inff();
  if (tid == 0) flag = T > 0 ? status[u] : 0;
  __syncthreads();
  const float* __restrict__ var = want ? variances + (int64_t)spk[u] * D : nullptr;
  if (want && T > 0) {
    bool bad = false;
    for (int d = tid; d < D; d += 256) {
      const float v = var[d];
      bad |= !(v > 0.0f && v < inf);
    }
    if (bad) atomicOr(&flag, 2);
  }
  __syncthreads();
  const int fl = flag;
  if (tid == 0 && T > 0) status[u] = fl;
  if (fl != 0 || T <= 0) {
    if (fl != 0)
      for (int64_t e = tid; e < T * D; e += 256) {
        out[(fb + e / D) * ld_out + e % D] = 0.0f;
        if (grad_out != nullptr) grad_out[(fb + e / D) * ld_grad + e % D] = 0.0f;
      }
    if (grad_var != nullptr)
      for (int d = tid; d < D; d += 256) grad_var[(int64_t)u * D + d] = 0.0;
    if (cost != nullptr && tid == 0) cost[u] = 0.0;
    return;
  }
  if (!want) return;
  if (grad_out != nullptr) {
    const double td = (double)T * (double)D;
    for (int64_t e = tid; e < T * D; e += 256) {
      const int64_t t = fb + e / D;
      const int d = (int)(e % D);
      grad_out[t * ld_grad + d] = (float)(((double)out[t * ld_out + d] - (double)obs[t * ld_obs + d]) / ((double)var[d] * td));
    }
  }
  double lnsum = 0.0, msum = 0.0;                      // thread 0's
  for (int c0 = 0; c0 < D; c0 += 64) {
    const int col = c0 + lane;
    const bool on = col < D;
    double s = 0.0;
    if (on) {
      const float* __restrict__ oc = out + fb * ld_out + col;
      const float* __restrict__ bc = obs + fb * ld_obs + col;
      for (int64_t t0 = 32 * q; t0 < T; t0 += 128) {
        const int64_t t1 = t0 + 32 < T ? t0 + 32 : T;
        double g = 0.0;
        for (int64_t t = t0; t < t1; ++t) {
          const double d = (double)bc[t * ld_obs] - (double)oc[t * ld_out];
          g += d * d;
        }
        s += g;
      }
    }
    part[q][lane] = s;
    __syncthreads();
    if (q == 0) {
      const double v = on ? (double)var[col] : 1.0;
      const double S = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      red[0][lane] = on ? S / v : 0.0;
      red[1][lane] = on ? log(v) : 0.0;
      if (on && grad_var != nullptr) grad_var[(int64_t)u * D + col] = (1.0 / v - S / ((double)T * v * v)) / (2.0 * (double)D);
    }
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
      if (tid < w) {
        red[0][tid] += red[0][tid + w];
        red[1][tid] += red[1][tid + w];
      }
      __syncthreads();
    }
    if (tid == 0) {
      msum += red[0][0];
      lnsum += red[1][0];
    }
    __syncthreads();
  }
  if (cost != nullptr && tid == 0) cost[u] = 0.5 * (kLn2Pi + lnsum / (double)D + msum / ((double)T * (double)D));
}

// ---- host ----------------------------------------------------------------------------------------------------------
static bool dnn_drop_ok(const WorldMi355Dropout* d) { return d == nullptr || (d->keep_prob > 0.0f && d->keep_prob <= 1.0f); }

static DnnMask dnn_mask_of(const WorldMi355Dropout* d) {
  DnnMask k;
  k.p = d != nullptr ? d->keep_prob : 1.0f;
  k.k0 = d != nullptr ? (uint32_t)(d->seed & 0xffffffffu) : 0u;
  k.k1 = d != nullptr ? (uint32_t)(d->seed >> 32) : 0u;
  k.offset = d != nullptr ? d->offset : 0u;
  return k;
}

int check_dnn_train_forward(int n_utt, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop, const float* x,
                            int64_t ld_x, const int* spkr, const float* out, int64_t ld_out, const float* obs, int64_t ld_obs,
                            const double* cost, const float* grad_out, int64_t ld_grad, const double* grad_var) {
  if (const int rc = check_dnn(n_utt, m, x, ld_x, spkr, out, ld_out, nullptr, 0, nullptr)) return rc;
  if (cost != nullptr || grad_out != nullptr || grad_var != nullptr) {           // either gradient asks what a cost asks
    if (!obs || !m->variances || ld_obs < m->n_outputs) return WM_ERR_BAD_ARG;
  }
  if (!dnn_drop_ok(drop)) return WM_ERR_BAD_ARG;
  if (grad_out != nullptr && ld_grad < m->n_outputs) return WM_ERR_BAD_ARG;
  return WM_OK;
}

int check_dnn_backward(int n_utt, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop, const float* x,
                       int64_t ld_x, const int* spkr, const float* grad_out, int64_t ld_grad, float* const* grad_weights,
                       float* const* grad_biases, float* const* grad_spkr_weights) {
  if (!grad_out) return WM_ERR_BAD_ARG;
  if (const int rc = check_dnn(n_utt, m, x, ld_x, spkr, grad_out, ld_grad, nullptr, 0, nullptr)) return rc;
  if (!dnn_drop_ok(drop)) return WM_ERR_BAD_ARG;
  if (grad_spkr_weights != nullptr && m->spkr_weights == nullptr) return WM_ERR_BAD_ARG;
  for (int i = 0; i <= m->n_layers; ++i) {
    if (grad_weights != nullptr && !grad_weights[i]) return WM_ERR_BAD_ARG;
    if (grad_biases != nullptr && !grad_biases[i]) return WM_ERR_BAD_ARG;
    if (i < m->n_layers && grad_spkr_weights != nullptr && !grad_spkr_weights[i]) return WM_ERR_BAD_ARG;
  }
  return WM_OK;
}

// The training workspace is the forward pass's with more in it: launch_dnn finds its two ping-pong buffers (the dz
// buffers here), its speaker and status arrays in the base; kept, grown and released by the same rule.
struct DnnTrainWs : DnnWs {
  float* act[kDnnMaxLayers] = {};   // a_i, [rows][units[i]]
  float* hd[kDnnMaxLayers] = {};    // h_i when keep_prob < 1 (h_i = a_i otherwise)
  double* U = nullptr;              // [utterances][max_w]: an utterance's column sums
  double* state = nullptr;          // [layers + 1][2][4][2][max_w]: the utterance cut by a chunk boundary
  double* acc = nullptr;            // [layers + 1][1 + speakers][max_w]
  int64_t rows = 0;
  int max_w = 0, n_act = 0, n_hd = 0, n_spk = 0;
};

static int dnn_train_ws(Batch& b, hipStream_t st, int64_t rows, int max_w, int n_act, int n_hd, int n_spk, DnnTrainWs** out) {
  auto fits = [&](const DnnWs& held) {                   // a forward pass's plain DnnWs never does
    if (!held.train) return false;
    const DnnTrainWs& w = static_cast<const DnnTrainWs&>(held);
    return w.rows >= rows && w.max_w >= max_w && w.n_act >= n_act && w.n_hd >= n_hd && w.n_spk >= n_spk && w.cap_utt >= b.n_utt;
  };
  return grow_ws<DnnTrainWs, DnnWs>(b.dnn, st, *out, fits, [&](DnnTrainWs& n) {
    n.train = true;
    n.cap = rows * (int64_t)max_w;
    n.n_buf = 2;
    n.cap_utt = b.n_utt;
    n.rows = rows;
    n.max_w = max_w;
    n.n_act = n_act;
    n.n_hd = n_hd;
    n.n_spk = n_spk;
    const size_t buf = sizeof(float) * (size_t)rows * (size_t)max_w;
    for (int k = 0; k < 2; ++k)
      if (const int rc = wm_check(n.alloc(&n.h[k], buf))) return rc;
    for (int k = 0; k < n_act; ++k)
      if (const int rc = wm_check(n.alloc(&n.act[k], buf))) return rc;
    for (int k = 0; k < n_hd; ++k)
      if (const int rc = wm_check(n.alloc(&n.hd[k], buf))) return rc;
    if (const int rc = wm_check(n.alloc(&n.spk, sizeof(int) * (size_t)b.n_utt))) return rc;
    if (const int rc = wm_check(n.alloc(&n.status, sizeof(int) * (size_t)b.n_utt))) return rc;
    const size_t wd = sizeof(double) * (size_t)max_w;
    if (const int rc = wm_check(n.alloc(&n.U, wd * (size_t)b.n_utt))) return rc;
    if (const int rc = wm_check(n.alloc(&n.state, wd * 16 * (size_t)(kDnnMaxLayers + 1)))) return rc;
    return wm_check(n.alloc(&n.acc, wd * (size_t)(1 + n_spk) * (size_t)(kDnnMaxLayers + 1)));
  });
}

static DnnOperand dnn_operand(const float* p, int64_t ld) {
  DnnOperand o;
  o.p = p;
  o.ld = ld;
  o.vec = ((uintptr_t)p % 16 == 0 && ld % 4 == 0) ? 1 : 0;
  o.frame_utt = nullptr;
  o.status = nullptr;
  return o;
}

static void dnn_launch_train_layer(int act, const DnnTrainLayer& L, hipStream_t st) {
  const int64_t blocks = (int64_t)((L.M + kDnnBM - 1) / kDnnBM) * L.tiles_n;
  const dim3 g((unsigned)blocks), t(256);
  switch (act) {
    case 0: hipLaunchKernelGGL((dnn_train_layer_kernel<0>), g, t, 0, st, L); break;
    case 1: hipLaunchKernelGGL((dnn_train_layer_kernel<1>), g, t, 0, st, L); break;
    case 2: hipLaunchKernelGGL((dnn_train_layer_kernel<2>), g, t, 0, st, L); break;
    default: hipLaunchKernelGGL((dnn_train_layer_kernel<3>), g, t, 0, st, L); break;
  }
}

template <bool DROP> static void dnn_launch_dgrad(int act, const DnnDgrad& L, hipStream_t st) {
  const int64_t blocks = (int64_t)((L.M + kDnnBM - 1) / kDnnBM) * L.tiles_n;
  const dim3 g((unsigned)blocks), t(256);
  switch (act) {
    case 0: hipLaunchKernelGGL((dnn_dgrad_kernel<0, DROP>), g, t, 0, st, L); break;
    case 1: hipLaunchKernelGGL((dnn_dgrad_kernel<1, DROP>), g, t, 0, st, L); break;
    case 2: hipLaunchKernelGGL((dnn_dgrad_kernel<2, DROP>), g, t, 0, st, L); break;
    default: hipLaunchKernelGGL((dnn_dgrad_kernel<3, DROP>), g, t, 0, st, L); break;
  }
}

// The layers of one chunk (batch rows r0 .. r0 + rows - 1).  keep: the backward pass's call -- a_i goes to W->act[i], h_i
// to W->hd[i] (W->act[i] itself without dropout) and the outputs to `out`; otherwise h ping-pongs between W->h[0 / 1].
static void dnn_train_chunk(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const DnnMask& mask, DnnTrainWs* W,
                            bool keep, const float* x, int64_t ld_x, int64_t r0, int64_t rows, float* out, int64_t ld_out,
                            int* d_status) {
  const bool drop = mask.p < 1.0f;
  const float* A = x + r0 * ld_x;
  int64_t lda = ld_x;
  int K = m.n_inputs;
  for (int i = 0; i <= m.n_layers; ++i) {
    const bool last = i == m.n_layers;
    const int N = last ? m.n_outputs : m.units[i];
    float* C = last ? out : keep ? (drop ? W->hd[i] : W->act[i]) : W->h[i & 1];
    const int64_t ldc = last ? ld_out : (int64_t)N;
    const float* sd = !last && m.spkr_weights != nullptr ? m.spkr_weights[i] : nullptr;
    if (drop && !last) {
      DnnTrainLayer L;
      memset(&L, 0, sizeof(L));
      L.M = (int)rows;
      L.N = N;
      L.K = K;
      L.A = dnn_operand(A, lda);
      L.W = dnn_operand(m.weights[i], N);
      L.bias = m.biases[i];
      L.sd = sd;
      L.spk = W->spk;
      L.frame_utt = b.d_frame_utt + r0;
      L.act = keep ? W->act[i] : nullptr;
      L.C = C;
      L.ldc = ldc;
      L.tiles_n = (N + kDnnBN - 1) / kDnnBN;
      L.t0 = (uint32_t)r0;
      L.layer = (uint32_t)i;
      L.mask = mask;
      dnn_launch_train_layer(m.hidden_activation, L, st);
    } else {                                  // no mask on this layer: the forward call's own kernel
      DnnLayer L;
      memset(&L, 0, sizeof(L));
      L.A = A;
      L.lda = lda;
      L.K = K;
      L.M = (int)rows;
      L.N = N;
      L.W = m.weights[i];
      L.bias = m.biases[i];
      L.sd = sd;
      L.spk = W->spk;
      L.frame_utt = b.d_frame_utt + r0;
      L.C = C;
      L.ldc = ldc;
      L.status = last ? d_status : nullptr;
      L.tiles_n = (N + kDnnBN - 1) / kDnnBN;
      L.a_vec = ((uintptr_t)L.A % 16 == 0 && L.lda % 4 == 0) ? 1 : 0;
      L.w_vec = ((uintptr_t)L.W % 16 == 0 && L.N % 4 == 0) ? 1 : 0;
      dnn_launch_layer(last ? m.output_activation : m.hidden_activation, L, st);
    }
    A = C;
    lda = ldc;
    K = N;
  }
}

static int dnn_train_prepare(const Batch& b, const WorldMi355AcousticModel& m, int64_t* chunk_out, int* max_w_out) {
  int64_t chunk = m.max_chunk_frames > 0 ? m.max_chunk_frames : kDnnChunk;
  chunk = chunk < kDnnMaxChunk ? chunk : kDnnMaxChunk;
  chunk = chunk < b.total_f ? chunk : b.total_f;
  int max_w = m.n_outputs;
  for (int i = 0; i < m.n_layers; ++i) max_w = max_w > m.units[i] ? max_w : m.units[i];
  const int64_t wide = (std::max(max_w, m.n_inputs) + kDnnBN - 1) / kDnnBN;       // of any product's tile grid
  if ((chunk + kDnnBM - 1) / kDnnBM * wide > (int64_t)0x7fffffff || wide * wide > (int64_t)0x7fffffff) return WM_ERR_BAD_ARG;
  *chunk_out = chunk;
  *max_w_out = max_w;
  return WM_OK;
}

static int dnn_upload_spk(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const int* spkr, DnnTrainWs* W) {
  W->h_spk.resize((size_t)b.n_utt);
  for (int u = 0; u < b.n_utt; ++u) W->h_spk[(size_t)u] = spkr != nullptr ? spkr[u] : m.n_spkrs - 1;
  return wm_check(hipMemcpyAsync(W->spk, W->h_spk.data(), sizeof(int) * (size_t)b.n_utt, hipMemcpyHostToDevice, st));
}

int launch_dnn_train_forward(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const WorldMi355Dropout* drop,
                             const float* x, int64_t ld_x, const int* spkr, float* out, int64_t ld_out, const float* obs,
                             int64_t ld_obs, double* cost, float* grad_out, int64_t ld_grad, double* grad_var, int* d_status) {
  if (const int rc = check_dnn_train_forward(b.n_utt, &m, drop, x, ld_x, spkr, out, ld_out, obs, ld_obs, cost, grad_out, ld_grad,
                                             grad_var))
    return rc;
  if (b.total_f <= 0 || b.n_utt <= 0) return WM_OK;
  int64_t chunk = 0;
  int max_w = 0;
  if (const int rc = dnn_train_prepare(b, m, &chunk, &max_w)) return rc;
  DnnTrainWs* W = nullptr;
  if (const int rc = dnn_train_ws(b, st, chunk, max_w, 0, 0, m.n_spkrs, &W)) return rc;
  if (const int rc = dnn_upload_spk(b, st, m, spkr, W)) return rc;
  if (d_status == nullptr) d_status = W->status;
  if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st))) return rc;
  const int want = (cost != nullptr || grad_out != nullptr || grad_var != nullptr) ? 1 : 0;
  const DnnMask mask = dnn_mask_of(drop);
  {
    TimedScope ts_(b.ctx, st, "dnn_layer_kernel");
    dnn_launch_check(st, x, ld_x, m.n_inputs, b.total_f, b.d_frame_utt, d_status, 1);
    if (want) dnn_launch_check(st, obs, ld_obs, m.n_outputs, b.total_f, b.d_frame_utt, d_status, 1);
    for (int64_t r0 = 0; r0 < b.total_f; r0 += chunk) {
      const int64_t rows = b.total_f - r0 < chunk ? b.total_f - r0 : chunk;
      dnn_train_chunk(b, st, m, mask, W, false, x, ld_x, r0, rows, out + r0 * ld_out, ld_out, d_status);
    }
  }
  {
    TimedScope ts_(b.ctx, st, "dnn_cost_kernel");
    hipLaunchKernelGGL(dnn_cost_grad_kernel, dim3((unsigned)b.n_utt), dim3(256), 0, st, out, ld_out, obs, ld_obs, m.variances,
                       (const int*)W->spk, m.n_outputs, (const int64_t*)b.d_f_off, d_status, cost, grad_out, ld_grad, grad_var,
                       want);
  }
  return wm_check(hipGetLastError());
}

int launch_dnn_backward(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const WorldMi355Dropout* drop,
                        const float* x, int64_t ld_x, const int* spkr, const float* G, int64_t ld_g, float* const* gW,
                        float* const* gB, float* const* gS, int* d_status) {
  if (const int rc = check_dnn_backward(b.n_utt, &m, drop, x, ld_x, spkr, G, ld_g, gW, gB, gS)) return rc;
  const int L = m.n_layers;
  auto width = [&](int i) { return i == L ? m.n_outputs : m.units[i]; };
  auto fan_in = [&](int i) { return i == 0 ? m.n_inputs : m.units[i - 1]; };
  if (b.total_f <= 0 || b.n_utt <= 0) {                       // nothing to sum: the gradients are zeros
    for (int i = 0; i <= L; ++i) {
      if (gW != nullptr)
        if (const int rc = wm_check(hipMemsetAsync(gW[i], 0, sizeof(float) * (size_t)fan_in(i) * (size_t)width(i), st))) return rc;
      if (gB != nullptr)
        if (const int rc = wm_check(hipMemsetAsync(gB[i], 0, sizeof(float) * (size_t)width(i), st))) return rc;
      if (gS != nullptr && i < L)
        if (const int rc = wm_check(hipMemsetAsync(gS[i], 0, sizeof(float) * (size_t)m.n_spkrs * (size_t)width(i), st))) return rc;
    }
    return WM_OK;
  }
  int64_t chunk = 0;
  int max_w = 0;
  if (const int rc = dnn_train_prepare(b, m, &chunk, &max_w)) return rc;
  const DnnMask mask = dnn_mask_of(drop);
  const bool dropping = mask.p < 1.0f;
  DnnTrainWs* W = nullptr;
  if (const int rc = dnn_train_ws(b, st, chunk, max_w, L, dropping ? L : 0, m.n_spkrs, &W)) return rc;
  if (const int rc = dnn_upload_spk(b, st, m, spkr, W)) return rc;
  if (d_status == nullptr) d_status = W->status;
  if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st))) return rc;
  const size_t acc_layer = (size_t)(1 + W->n_spk) * (size_t)W->max_w;
  if (const int rc = wm_check(hipMemsetAsync(W->acc, 0, sizeof(double) * acc_layer * (size_t)(L + 1), st))) return rc;
  TimedScope ts_(b.ctx, st, "dnn_backward_kernel");
  dnn_launch_check(st, x, ld_x, m.n_inputs, b.total_f, b.d_frame_utt, d_status, 1);
  dnn_launch_check(st, G, ld_g, m.n_outputs, b.total_f, b.d_frame_utt, d_status, 1);
  // an utterance's status is settled before any of its rows reaches a gradient: with more than one chunk a forward pass
  // of every chunk comes first (a non-finite output in a later chunk flags rows of an earlier one)
  if (b.total_f > chunk)
    for (int64_t r0 = 0; r0 < b.total_f; r0 += chunk) {
      const int64_t rows = b.total_f - r0 < chunk ? b.total_f - r0 : chunk;
      dnn_train_chunk(b, st, m, mask, W, false, x, ld_x, r0, rows, W->h[L & 1], m.n_outputs, d_status);
    }
  int chunk_no = 0;
  for (int64_t r0 = 0; r0 < b.total_f; r0 += chunk, ++chunk_no) {
    const int64_t rows = b.total_f - r0 < chunk ? b.total_f - r0 : chunk;
    const int* fu = b.d_frame_utt + r0;
    // the utterances that end in this chunk, and those with rows in it
    const int ua = (int)(std::upper_bound(b.f_off.begin() + 1, b.f_off.end(), r0) - (b.f_off.begin() + 1));
    const int ub = (int)(std::upper_bound(b.f_off.begin() + 1, b.f_off.end(), r0 + rows) - (b.f_off.begin() + 1));
    const int ue = (int)(std::lower_bound(b.f_off.begin(), b.f_off.begin() + b.n_utt, r0 + rows) - b.f_off.begin());
    float* cur = W->h[0];
    float* nxt = W->h[1];
    dnn_train_chunk(b, st, m, mask, W, true, x, ld_x, r0, rows, cur, m.n_outputs, d_status);
    {
      const int64_t n = rows * (int64_t)m.n_outputs;
      const dim3 g((unsigned)((n + 255) / 256)), t(256);
      const float* Gc = G + r0 * ld_g;
      switch (m.output_activation) {
        case 0: hipLaunchKernelGGL((dnn_dzo_kernel<0>), g, t, 0, st, cur, Gc, ld_g, m.n_outputs, rows, fu, (const int*)d_status); break;
        case 1: hipLaunchKernelGGL((dnn_dzo_kernel<1>), g, t, 0, st, cur, Gc, ld_g, m.n_outputs, rows, fu, (const int*)d_status); break;
        case 2: hipLaunchKernelGGL((dnn_dzo_kernel<2>), g, t, 0, st, cur, Gc, ld_g, m.n_outputs, rows, fu, (const int*)d_status); break;
        default: hipLaunchKernelGGL((dnn_dzo_kernel<3>), g, t, 0, st, cur, Gc, ld_g, m.n_outputs, rows, fu, (const int*)d_status); break;
      }
    }
    for (int i = L; i >= 0; --i) {
      const int N = width(i), K = fan_in(i);
      // the input of layer i: x, or h_{i-1}
      const float* hin = i == 0 ? x + r0 * ld_x : (dropping ? W->hd[i - 1] : W->act[i - 1]);
      const int64_t ld_h = i == 0 ? ld_x : (int64_t)K;
      if (gW != nullptr) {
        DnnWgrad P;
        memset(&P, 0, sizeof(P));
        P.h = dnn_operand(hin, ld_h);
        P.h.frame_utt = fu;
        P.h.status = d_status;
        P.dz = dnn_operand(cur, N);
        P.dW = gW[i];
        P.rows = (int)rows;
        P.N = N;
        P.K = K;
        P.tiles_n = (N + kDnnBN - 1) / kDnnBN;
        P.accumulate = chunk_no > 0 ? 1 : 0;
        const int64_t blocks = (int64_t)((K + kDnnBM - 1) / kDnnBM) * P.tiles_n;
        hipLaunchKernelGGL(dnn_wgrad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, P);
      }
      float* db = gB != nullptr ? gB[i] : nullptr;
      float* dsd = gS != nullptr && i < L ? gS[i] : nullptr;
      if (db != nullptr || dsd != nullptr) {
        const int colchunks = (N + 63) / 64;
        double* state = W->state + (size_t)i * 16 * (size_t)W->max_w;
        const double* st_in = state + (size_t)((chunk_no + 1) & 1) * 8 * (size_t)W->max_w;
        double* st_out = state + (size_t)(chunk_no & 1) * 8 * (size_t)W->max_w;
        if (ue > ua)
          hipLaunchKernelGGL(dnn_colsum_kernel, dim3((unsigned)((int64_t)(ue - ua) * colchunks)), dim3(256), 0, st,
                             (const float*)cur, (int64_t)N, N, colchunks, ua, r0, rows, (const int64_t*)b.d_f_off, st_in,
                             st_out, W->max_w, W->U);
        hipLaunchKernelGGL(dnn_fold_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const double*)W->U, W->max_w,
                           N, ua, ub, (const int64_t*)b.d_f_off, (const int*)W->spk, W->acc + (size_t)i * acc_layer, m.n_spkrs,
                           db, dsd);
      }
      if (i == 0) break;
      DnnDgrad P;
      memset(&P, 0, sizeof(P));
      P.dz = dnn_operand(cur, N);
      P.W = dnn_operand(m.weights[i], N);
      P.act = W->act[i - 1];
      P.frame_utt = fu;
      P.status = d_status;
      P.out = nxt;
      P.M = (int)rows;
      P.N = N;
      P.K = K;
      P.tiles_n = (K + kDnnBN - 1) / kDnnBN;
      P.t0 = (uint32_t)r0;
      P.layer = (uint32_t)(i - 1);
      P.mask = mask;
      if (dropping) dnn_launch_dgrad<true>(m.hidden_activation, P, st);
      else dnn_launch_dgrad<false>(m.hidden_activation, P, st);
      std::swap(cur, nxt);
    }
  }
  return wm_check(hipGetLastError());
}

}  // namespace wm
