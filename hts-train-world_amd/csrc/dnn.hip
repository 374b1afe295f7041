// dnn.hip -- the forward pass of the recipe's acoustic model (data/scripts/DNNDefine.py:113-191 inference, as
// DNNSynthesis.py:129-229 runs it with keep_prob 1) and its frame-level cost (DNNDefine.py:231-237), for a whole batch
// of utterances: `.ffi` rows in, `ffo`-layout means out.
//
// Per frame of utterance u with speaker s(u):
//   h_{i+1} = act_h((h_i W_i + b_i) + sd_i[s(u)])     (the speaker row only in SAT mode),   out = act_o(h_L W_o + b_o),
// float32 throughout, every addition rounded to float32 in that order.  dnn_layer_kernel<ACT> is one layer: a float32
// GEMM on gfx950's exact-f32 matrix instruction v_mfma_f32_32x32x2_f32, which is bit for bit a k-ordered fmaf chain
// that starts from zero (one rounding per product), with bias, speaker row and activation in the epilogue.
//   block 256 threads = 4 waves, tile 128 rows x 128 columns x 32 k; wave (wm, wn) owns rows 64 wm .. + 63 and columns
//   64 wn .. + 63 as 2 x 2 accumulator tiles of 32 x 32 (64 registers);
//   A and W tiles go global -> registers -> LDS; the next tile's global loads are issued before the current tile's
//   MFMAs.  A is kept transposed in LDS ([k][row]) so that the 32 lanes of a half-wave read consecutive words for both
//   operands (lane l supplies A[row l & 31][k = l >> 5] and W[k = l >> 5][column l & 31]).
//   What lies beyond M, N or K is ZERO in LDS and is never read from memory: a zero product leaves an fma chain as it
//   is, so a row's result depends on that row of A and on W, b, sd alone -- not on its place in a tile, on the chunk
//   or on the batch around it.  Stores are guarded by bounds.
// Frames go through the layers in chunks of at most `max_chunk_frames` rows (65 536 unless the caller lowers it); the
// hidden activations ping-pong between two [chunk][max units] buffers of the batch's workspace (Batch::dnn).  The
// row -> utterance map is the batch's frame_utt, the speaker of an utterance a device copy of the caller's array.
// dnn_check_kernel flags non-finite inputs before the first layer; the output layer flags non-finite outputs;
// dnn_cost_kernel, one block per utterance, checks the speaker's variances, zeroes the rows of a flagged utterance and
// sums the cost in double in column_moments_kernel's fixed order (groups of 32 frames dealt to four waves, a lane per
// column, the columns by a tree over the lanes): the order depends on the utterance's length alone.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "batch.hpp"
#include "common.hpp"
#include "dnn.hpp"

namespace wm {

template <int ACT>
__global__ __launch_bounds__(256) void dnn_layer_kernel(DnnLayer p) {
  __shared__ __attribute__((aligned(16))) float As[kDnnBK * kDnnLd];   // [k][row]
  __shared__ __attribute__((aligned(16))) float Ws[kDnnBK * kDnnLd];   // [k][column]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile_m = (int)(blockIdx.x / (unsigned)p.tiles_n), tile_n = (int)blockIdx.x - tile_m * p.tiles_n;
  const int row0 = tile_m * kDnnBM, col0 = tile_n * kDnnBN;
  const int M = p.M, N = p.N, K = p.K;

  // this thread's part of a tile: A rows ar + 32 i at k ak .. ak + 3; W rows wk + 8 i at columns wc .. wc + 3
  const int ar = tid >> 3, ak = (tid & 7) * 4;
  const int wk = tid >> 5, wc = (tid & 31) * 4;
  float4 ra[4], rw[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = row0 + ar + 32 * i, k = k0 + ak;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (r < M && k < K) {
        const float* src = p.A + (int64_t)r * p.lda + k;
        if (p.a_vec && k + 3 < K) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          v.x = src[0];
          if (k + 1 < K) v.y = src[1];
          if (k + 2 < K) v.z = src[2];
          if (k + 3 < K) v.w = src[3];
        }
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + wk + 8 * i, c = col0 + wc;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (k < K && c < N) {
        const float* src = p.W + (int64_t)k * N + c;
        if (p.w_vec && c + 3 < N) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          v.x = src[0];
          if (c + 1 < N) v.y = src[1];
          if (c + 2 < N) v.z = src[2];
          if (c + 3 < N) v.w = src[3];
        }
      }
      rw[i] = v;
    }
  };

  dnn_f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

  fetch(0);
  const int half = lane >> 5, l31 = lane & 31;
  for (int k0 = 0; k0 < K; k0 += kDnnBK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* dst = As + ak * kDnnLd + ar + 32 * i;
      dst[0] = ra[i].x;
      dst[kDnnLd] = ra[i].y;
      dst[2 * kDnnLd] = ra[i].z;
      dst[3 * kDnnLd] = ra[i].w;
      *reinterpret_cast<float4*>(Ws + (wk + 8 * i) * kDnnLd + wc) = rw[i];
    }
    __syncthreads();
    if (k0 + kDnnBK < K) fetch(k0 + kDnnBK);
    const float* ap = As + half * kDnnLd + wm * 64 + l31;
    const float* bp = Ws + half * kDnnLd + wn * 64 + l31;
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

  // epilogue: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 tile
  const float inf = __builtin_inff();
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
        if (p.status != nullptr && !(fabsf(v) < inf)) {
          const int u = p.frame_utt[row];
          if ((p.status[u] & 1) == 0) atomicOr(p.status + u, 2);     // bit 1 was settled before the first layer
        }
        p.C[(int64_t)row * p.ldc + col] = v;
      }
    }
  }
}

// A wave per row: a non-finite value among the row's `width` columns sets `bit` in its utterance's status.
__global__ __launch_bounds__(256) void dnn_check_kernel(const float* __restrict__ x, int64_t ld, int width, int64_t rows,
                                                        const int* __restrict__ frame_utt, int* __restrict__ status,
                                                        int bit) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * ld;
  const float inf = __builtin_inff();
  bool bad = false;
  for (int c = lane; c < width; c += 64) bad |= !(fabsf(xr[c]) < inf);
  if (bad) atomicOr(status + frame_utt[row], bit);
}

// One block per utterance.  With a cost: the speaker's variances are checked (bit 2) and the cost is summed; always: a
// flagged utterance's rows of `out` become zeros and its cost 0.
__global__ __launch_bounds__(256) void dnn_cost_kernel(float* __restrict__ out, int64_t ld_out, const float* __restrict__ obs,
                                                       int64_t ld_obs, const float* __restrict__ variances,
                                                       const int* __restrict__ spk, int D,
                                                       const int64_t* __restrict__ f_off, int* __restrict__ status,
                                                       double* __restrict__ cost) {
#pragma clang fp contract(off)
  const int u = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int64_t fb = f_off[u];
  const int64_t T = f_off[u + 1] - fb;
  __shared__ int flag;
  __shared__ double part[4][64], red[2][64];
  const float inf = __builtin_inff();
  if (tid == 0) flag = T > 0 ? status[u] : 0;
  __syncthreads();
  const float* __restrict__ var = cost != nullptr ? variances + (int64_t)spk[u] * D : nullptr;
  if (cost != nullptr && T > 0) {
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
      for (int64_t e = tid; e < T * D; e += 256) out[(fb + e / D) * ld_out + e % D] = 0.0f;
    if (cost != nullptr && tid == 0) cost[u] = 0.0;
    return;
  }
  if (cost == nullptr) return;
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
      red[0][lane] = on ? ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) / v : 0.0;
      red[1][lane] = on ? log(v) : 0.0;
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
  if (tid == 0) cost[u] = 0.5 * (kLn2Pi + lnsum / (double)D + msum / ((double)T * (double)D));
}

// What WorldMi355AcousticModelForward refuses, on the host alone: no device call is made for a refused argument set.
int check_dnn(int n_utt, const WorldMi355AcousticModel* m, const float* x, int64_t ld_x, const int* spkr, const float* out,
              int64_t ld_out, const float* obs, int64_t ld_obs, const double* cost) {
  if (!m || !x || !out || !m->weights || !m->biases) return WM_ERR_BAD_ARG;
  if (m->n_layers < 0 || m->n_layers > kDnnMaxLayers || m->n_inputs < 1 || m->n_outputs < 1 || m->n_spkrs < 1)
    return WM_ERR_BAD_ARG;
  if (m->hidden_activation < 0 || m->hidden_activation > 3 || m->output_activation < 0 || m->output_activation > 3)
    return WM_ERR_BAD_ARG;
  if (m->n_layers > 0 && !m->units) return WM_ERR_BAD_ARG;
  if (m->max_chunk_frames < 0) return WM_ERR_BAD_ARG;
  for (int i = 0; i <= m->n_layers; ++i) {
    if (!m->weights[i] || !m->biases[i]) return WM_ERR_BAD_ARG;
    if (i < m->n_layers && (m->units[i] < 1 || (m->spkr_weights != nullptr && !m->spkr_weights[i]))) return WM_ERR_BAD_ARG;
  }
  if (spkr != nullptr)
    for (int u = 0; u < n_utt; ++u)
      if (spkr[u] < 0 || spkr[u] >= m->n_spkrs) return WM_ERR_BAD_ARG;
  if (ld_x < m->n_inputs || ld_out < m->n_outputs) return WM_ERR_BAD_ARG;
  if (cost != nullptr && (!obs || !m->variances)) return WM_ERR_BAD_ARG;
  if (cost != nullptr && ld_obs < m->n_outputs) return WM_ERR_BAD_ARG;
  return WM_OK;
}

void dnn_launch_layer(int act, const DnnLayer& L, hipStream_t st) {
  const int64_t blocks = (int64_t)((L.M + kDnnBM - 1) / kDnnBM) * L.tiles_n;
  const dim3 g((unsigned)blocks), t(256);
  switch (act) {
    case 0: hipLaunchKernelGGL((dnn_layer_kernel<0>), g, t, 0, st, L); break;
    case 1: hipLaunchKernelGGL((dnn_layer_kernel<1>), g, t, 0, st, L); break;
    case 2: hipLaunchKernelGGL((dnn_layer_kernel<2>), g, t, 0, st, L); break;
    default: hipLaunchKernelGGL((dnn_layer_kernel<3>), g, t, 0, st, L); break;
  }
}

void dnn_launch_check(hipStream_t st, const float* x, int64_t ld, int width, int64_t rows, const int* frame_utt, int* status,
                      int bit) {
  hipLaunchKernelGGL(dnn_check_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, ld, width, rows, frame_utt,
                     status, bit);
}

int launch_dnn(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const float* x, int64_t ld_x, const int* spkr,
               float* out, int64_t ld_out, const float* obs, int64_t ld_obs, double* cost, int* d_status) {
  if (const int rc = check_dnn(b.n_utt, &m, x, ld_x, spkr, out, ld_out, obs, ld_obs, cost)) return rc;
  if (b.total_f <= 0 || b.n_utt <= 0) return WM_OK;
  int64_t chunk = m.max_chunk_frames > 0 ? m.max_chunk_frames : kDnnChunk;
  chunk = chunk < kDnnMaxChunk ? chunk : kDnnMaxChunk;          // a chunk's tiles fit a one-dimensional grid
  chunk = chunk < b.total_f ? chunk : b.total_f;
  int max_units = 0;
  for (int i = 0; i < m.n_layers; ++i) max_units = max_units > m.units[i] ? max_units : m.units[i];
  for (int i = 0; i <= m.n_layers; ++i) {                       // a layer's tiles fit a one-dimensional grid
    const int64_t tiles_n = ((int64_t)(i == m.n_layers ? m.n_outputs : m.units[i]) + kDnnBN - 1) / kDnnBN;
    if ((chunk + kDnnBM - 1) / kDnnBM * tiles_n > (int64_t)0x7fffffff) return WM_ERR_BAD_ARG;
  }
  const int n_buf = m.n_layers >= 2 ? 2 : m.n_layers;
  const int64_t need = chunk * (int64_t)max_units;
  DnnWs* W = nullptr;                                    // (a training pass's DnnTrainWs serves as well)
  if (const int rc = grow_ws(b.dnn, st, W,
                             [&](const DnnWs& w) { return w.cap >= need && w.n_buf >= n_buf && w.cap_utt >= b.n_utt; },
                             [&](DnnWs& n) {
                               n.cap = need;
                               n.n_buf = n_buf;
                               n.cap_utt = b.n_utt;
                               for (int k = 0; k < n_buf; ++k)
                                 if (const int rc = wm_check(n.alloc(&n.h[k], sizeof(float) * (size_t)need))) return rc;
                               if (const int rc = wm_check(n.alloc(&n.spk, sizeof(int) * (size_t)b.n_utt))) return rc;
                               return wm_check(n.alloc(&n.status, sizeof(int) * (size_t)b.n_utt));
                             }))
    return rc;
  W->h_spk.resize((size_t)b.n_utt);
  for (int u = 0; u < b.n_utt; ++u) W->h_spk[(size_t)u] = spkr != nullptr ? spkr[u] : m.n_spkrs - 1;   // DNNSynthesis.py:139
  if (const int rc = wm_check(hipMemcpyAsync(W->spk, W->h_spk.data(), sizeof(int) * (size_t)b.n_utt, hipMemcpyHostToDevice, st)))
    return rc;
  if (d_status == nullptr) d_status = W->status;
  if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st))) return rc;
  {
    TimedScope ts_(b.ctx, st, "dnn_layer_kernel");
    dnn_launch_check(st, x, ld_x, m.n_inputs, b.total_f, b.d_frame_utt, d_status, 1);
    if (cost != nullptr) dnn_launch_check(st, obs, ld_obs, m.n_outputs, b.total_f, b.d_frame_utt, d_status, 1);
    for (int64_t r0 = 0; r0 < b.total_f; r0 += chunk) {
      const int64_t rows = b.total_f - r0 < chunk ? b.total_f - r0 : chunk;
      const float* A = x + r0 * ld_x;
      int64_t lda = ld_x;
      int K = m.n_inputs;
      for (int i = 0; i <= m.n_layers; ++i) {
        const bool last = i == m.n_layers;
        DnnLayer L;
        memset(&L, 0, sizeof(L));
        L.A = A;
        L.lda = lda;
        L.K = K;
        L.M = (int)rows;
        L.N = last ? m.n_outputs : m.units[i];
        L.W = m.weights[i];
        L.bias = m.biases[i];
        L.sd = !last && m.spkr_weights != nullptr ? m.spkr_weights[i] : nullptr;
        L.spk = W->spk;
        L.frame_utt = b.d_frame_utt + r0;
        L.C = last ? out + r0 * ld_out : W->h[i & 1];
        L.ldc = last ? ld_out : (int64_t)L.N;
        L.status = last ? d_status : nullptr;
        L.tiles_n = (L.N + kDnnBN - 1) / kDnnBN;
        L.a_vec = ((uintptr_t)L.A % 16 == 0 && L.lda % 4 == 0) ? 1 : 0;
        L.w_vec = ((uintptr_t)L.W % 16 == 0 && L.N % 4 == 0) ? 1 : 0;
        dnn_launch_layer(last ? m.output_activation : m.hidden_activation, L, st);
        A = L.C;
        lda = L.ldc;
        K = L.N;
      }
    }
  }
  {
    TimedScope ts_(b.ctx, st, "dnn_cost_kernel");
    hipLaunchKernelGGL(dnn_cost_kernel, dim3((unsigned)b.n_utt), dim3(256), 0, st, out, ld_out, obs, ld_obs, m.variances,
                       (const int*)W->spk, m.n_outputs, (const int64_t*)b.d_f_off, d_status, cost);
  }
  return wm_check(hipGetLastError());
}

}  // namespace wm
