// dnn.hpp -- what the acoustic model's forward pass (dnn.hip) and its training pass (dnn_train.hip) share: the tile
// conventions of the float32 GEMM, the activation codes, the layer kernel's arguments and the batch's workspace.  The
// kernels dnn_layer_kernel and dnn_check_kernel are dnn.hip's; the training pass reaches them through the launchers.
#pragma once
#include <stdint.h>

#include <vector>

#include "batch.hpp"

namespace wm {

constexpr int kDnnMaxLayers = 8;
constexpr int kDnnBM = 128, kDnnBN = 128, kDnnBK = 32;
constexpr int kDnnLd = 132;                                  // words per k row of either LDS tile (16-byte rows)
constexpr int64_t kDnnChunk = 65536, kDnnMaxChunk = (int64_t)1 << 20;
typedef float dnn_f32x16 __attribute__((ext_vector_type(16)));

// 0 linear, 1 sigmoid, 2 tanh, 3 ReLU (Config.pm.in:228).  expf and tanhf are the device library's (1 and 2 ulp), the
// addition and the division IEEE: the activation's own error stays under 8 * 2^-24 |value|.
template <int ACT> __device__ __forceinline__ float dnn_act(float v) {
  if (ACT == 1) return 1.0f / (1.0f + expf(-v));
  if (ACT == 2) return tanhf(v);
  if (ACT == 3) return v > 0.0f ? v : 0.0f;
  return v;
}

struct DnnLayer {
  const float* A;          // [M][K], row stride lda
  const float* W;          // [K][N], contiguous
  const float* bias;       // [N]
  const float* sd;         // null, or [n_spkrs][N]
  const int* spk;          // [n_utt], read with sd
  const int* frame_utt;    // of row 0 of this chunk
  float* C;                // [M][N], row stride ldc
  int* status;             // null, or [n_utt]: the output layer flags non-finite results (bit 2)
  int64_t lda, ldc;
  int M, N, K, tiles_n;
  int a_vec, w_vec;        // 16-byte loads are possible (base and stride aligned)
};

struct DnnWs : StageWs {
  float* h[2] = {nullptr, nullptr};
  int* spk = nullptr;
  int* status = nullptr;
  std::vector<int> h_spk;           // the pageable source of the upload: it outlives the call, and the next call rewrites
                                    // it without a wait -- a copy from pageable memory returns once the source has
                                    // been read or staged (as mspf.hip's h_tab and synthesis.hip's order rely on)
  int64_t cap = 0, cap_utt = 0;     // floats per buffer; utterances
  int n_buf = 0;
  bool train = false;               // a DnnTrainWs (dnn_train.hip): this struct with the training pass's buffers behind it
};

// dnn_layer_kernel<act> on L's tiles
void dnn_launch_layer(int act, const DnnLayer& L, hipStream_t st);
// dnn_check_kernel: a non-finite value among the `width` columns of a row sets `bit` in its utterance's status
void dnn_launch_check(hipStream_t st, const float* x, int64_t ld, int width, int64_t rows, const int* frame_utt, int* status,
                      int bit);

}  // namespace wm
