// capi.cpp -- the C-ABI of libworld_mi355.so.
//
// (1) WORLD's public API (include/world/*.h), one utterance per call, host
//     pointers in and out, exactly the reference's signatures
//     (externs/WORLD_v2/src/world/{dio,stonemask,cheaptrick,d4c,synthesis,harvest}.h).
//     Each call stages the utterance into HBM, runs the batch kernels with B = 1
//     and copies the result back.  There is NO CPU fallback: without a HIP device
//     the call aborts with a message, like the reference aborts on bad_alloc.
// (2) The batched device-pointer extension (include/world_mi355.h).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <mutex>
#include <vector>

#include "batch.hpp"
#include "common.hpp"
#include "world/cheaptrick.h"
#include "world/codec.h"
#include "world/d4c.h"
#include "world/dio.h"
#include "world/harvest.h"
#include "world/stonemask.h"
#include "world/synthesis.h"

namespace wm {
const char* last_error();
void set_error(const char* msg);
#ifdef WM_PHASE
int phase_read_d4c(unsigned long long* out32);
int phase_read_cheaptrick(unsigned long long* out32);
int phase_read_synthesis(unsigned long long* out32);
#endif
}  // namespace wm

using namespace wm;

// the drop-in entry points' failure handler (WorldMi355SetErrorHandler; see die() below)
// The handler and its argument are read and written as a pair under their own lock (not g_mu: die() runs while an
// entry point holds that one).
static std::mutex g_err_mu;
static WorldMi355ErrorHandler g_on_error = nullptr;
static void* g_on_error_user = nullptr;
static WorldMi355ErrorHandler error_handler(void** user) {
  std::lock_guard<std::mutex> lock(g_err_mu);
  *user = g_on_error_user;
  return g_on_error;
}

struct WorldMi355Context { Context c; };
struct WorldMi355Batch { Batch b; };

// How every batched entry point ends: a NULL batch is WM_ERR_BAD_ARG; otherwise on the batch's device, the launcher
// with the batch and its context's stream, the caller's.  Host-only checks (check_*) come before it, so a refused
// argument set makes no device call, hipGetDevice included.
template <class Launch, class... Args> static int on_batch(WorldMi355Batch* b, Launch launch, Args&&... args) {
  if (!b) return WM_ERR_BAD_ARG;
  OnDevice dev_(*b->b.ctx);
  return launch(b->b, b->b.ctx->stream, std::forward<Args>(args)...);
}

template <typename T> static int alloc_items(T** p, size_t count) {
  *p = nullptr;
  return wm_check(wm::dev_alloc(p, sizeof(T) * (count ? count : 1)));
}
template <typename T> static int upload(T** p, const std::vector<T>& v) {
  int rc = alloc_items(p, v.size());
  if (rc) return rc;
  if (v.empty()) return WM_OK;
  return wm_check(hipMemcpy(*p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
}

extern "C" {

const char* WorldMi355LastError(void) { return wm::last_error(); }

void WorldMi355DefaultParams(int fs, double frame_period, WorldMi355Params* p) {
  memset(p, 0, sizeof(*p));
  p->fs = fs;
  p->frame_period = frame_period;
  p->f0_floor = 71.0;            // analysis.cpp:111
  p->f0_ceil = 800.0;            // dio.cpp:652 (kCeilF0)
  p->channels_in_octave = 2.0;   // dio.cpp:651
  p->speed = 1;                  // analysis.cpp:106
  p->allowed_range = 0.1;        // analysis.cpp:116
  p->q1 = -0.15;                 // analysis.cpp:151
  p->fft_size = 0;
  p->d4c_threshold = 0.0;        // analysis.cpp:190
}

int WorldMi355CreateContext(int device, void* hip_stream, WorldMi355Context** out) {
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    wm::set_error("no HIP device visible: libworld_mi355 has no CPU path");
    return WM_ERR_NO_DEVICE;
  }
  int before = -1;
  (void)hipGetDevice(&before);
  if (device >= 0 && device != before) {
    int rc = wm_check(hipSetDevice(device));
    if (rc) return rc;
  }
  WorldMi355Context* h = new WorldMi355Context();
  Context& c = h->c;
  hipGetDevice(&c.device);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c.device) == hipSuccess) c.num_cu = prop.multiProcessorCount;
  c.frame_grid = c.num_cu * 16 * c.oversub;
  // NULL selects the legacy default stream (stream 0): it orders with every blocking stream, which
  // is what callers that allocate and copy with plain hipMemcpy / torch's default stream expect.
  c.stream = (hipStream_t)hip_stream;
  *out = h;
  // every entry point switches to its context's device itself (OnDevice): the caller's current device stays
  if (before >= 0 && before != c.device) (void)hipSetDevice(before);
  return WM_OK;
}

void WorldMi355DestroyContext(WorldMi355Context* h) {
  if (!h) return;
  Context& c = h->c;
  OnDevice dev_(c);
  hipStreamSynchronize(c.stream);
  if (c.fork) { hipStreamSynchronize(c.fork->side); hipStreamSynchronize(c.fork->aux); }
  if (c.split) hipStreamSynchronize(c.split->prep);
  c.timing_clear();
  wm::dev_free(c.d_rng);
  wm::dev_free(c.d_scratch);
  delete h;                            // the tables, the streams and events, the pinned counters: with their owners
}

int WorldMi355SetStream(WorldMi355Context* h, void* hip_stream) {
  OnDevice dev_(h->c);
  Context& c = h->c;
  int rc = wm_check(hipStreamSynchronize(c.stream));
  if (rc) return rc;
  c.stream = (hipStream_t)hip_stream;
  return WM_OK;
}

int WorldMi355Synchronize(WorldMi355Context* h) {
  OnDevice dev_(h->c);
  return wm_check(hipStreamSynchronize(h->c.stream));
}

int WorldMi355CreateBatch(WorldMi355Context* h, const WorldMi355Params* params, int n_utt,
                          const int* x_lengths, const int* f0_lengths, const int* y_lengths,
                          WorldMi355Batch** out) {
  *out = nullptr;
  if (!h || !params || n_utt <= 0 || (!x_lengths && !f0_lengths)) {
    wm::set_error("CreateBatch: bad argument");
    return WM_ERR_BAD_ARG;
  }
  OnDevice dev_(h->c);
  WorldMi355Batch* hb = new WorldMi355Batch();
  Batch& b = hb->b;
  b.ctx = &h->c;
  b.p = *params;
  if (b.p.fft_size == 0)   // GetFFTSizeForCheapTrick, cheaptrick.cpp:191-194
    b.p.fft_size = (int)pow(2.0, 1.0 + (int)(log(3.0 * b.p.fs / b.p.f0_floor + 1) / kLog2));
  b.n_utt = n_utt;
  b.x_len.assign(n_utt, 0); b.f0_len.assign(n_utt, 0); b.y_len.assign(n_utt, 0);
  b.x_off.assign(n_utt + 1, 0); b.f_off.assign(n_utt + 1, 0); b.y_off.assign(n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) {
    b.x_len[u] = x_lengths ? x_lengths[u] : 0;
    b.f0_len[u] = f0_lengths ? f0_lengths[u]
                             : (int)(1000.0 * b.x_len[u] / b.p.fs / b.p.frame_period) + 1;   // dio.cpp:638-640
    b.y_len[u] = y_lengths ? y_lengths[u]
                           : (int)((b.f0_len[u] - 1) * b.p.frame_period / 1000.0 * b.p.fs) + 1;   // synth.cpp:259
    if (b.x_len[u] < 0 || b.f0_len[u] <= 0 || b.y_len[u] < 0) {
      delete hb;
      wm::set_error("CreateBatch: negative length");
      return WM_ERR_BAD_ARG;
    }
    if (x_lengths && b.x_len[u] == 0) {
      // the reference's caller refuses a wav without samples (test/analysis.cpp:252-259); the kernels clamp their
      // loads into [0, x_length - 1], which an empty utterance does not have
      delete hb;
      wm::set_error("CreateBatch: an utterance has no samples");
      return WM_ERR_BAD_ARG;
    }
    b.x_off[u + 1] = b.x_off[u] + b.x_len[u];
    b.f_off[u + 1] = b.f_off[u] + b.f0_len[u];
    b.y_off[u + 1] = b.y_off[u] + b.y_len[u];
    b.max_x_len = imax(b.max_x_len, b.x_len[u]);
    b.max_f0_len = imax(b.max_f0_len, b.f0_len[u]);
    b.max_y_len = imax(b.max_y_len, b.y_len[u]);
  }
  b.total_x = b.x_off[n_utt]; b.total_f = b.f_off[n_utt]; b.total_y = b.y_off[n_utt];
  // One device allocation and one upload for every descriptor and per-frame work array of the batch (a batch of
  // one utterance is created per call by the per-utterance entry points: fourteen hipMallocs and seven blocking
  // copies were most of its cost).  Layout: 256-byte aligned sections; the first `init_bytes` are initialised
  // from a host image, the rest is scratch.
  const size_t n1 = (size_t)n_utt + 1, nf = (size_t)b.total_f;
  Sections take;
  const size_t o_xoff = take(8 * n1), o_foff = take(8 * n1), o_yoff = take(8 * n1);
  const size_t o_xlen = take(4 * (size_t)n_utt), o_flen = take(4 * (size_t)n_utt), o_ylen = take(4 * (size_t)n_utt);
  const size_t o_futt = take(4 * nf);
  const size_t init_bytes = take.at;
  const size_t o_rng = take(4 * nf), o_rng2 = take(4 * nf), o_ap0 = take(8 * nf), o_f0t = take(8 * nf);
  const size_t o_perm = take(4 * nf), o_pcnt = take(4 * (nf / 1024 + 2)), o_pn = take(4 * 4);
  const size_t o_rng_d = take(4 * nf), o_perm_d = take(4 * nf), o_pcnt_d = take(4 * (nf / 1024 + 2)), o_pn_d = take(4 * 4);
  std::vector<unsigned char> img(init_bytes, 0);
  memcpy(&img[o_xoff], b.x_off.data(), 8 * n1);
  memcpy(&img[o_foff], b.f_off.data(), 8 * n1);
  memcpy(&img[o_yoff], b.y_off.data(), 8 * n1);
  memcpy(&img[o_xlen], b.x_len.data(), 4 * (size_t)n_utt);
  memcpy(&img[o_flen], b.f0_len.data(), 4 * (size_t)n_utt);
  memcpy(&img[o_ylen], b.y_len.data(), 4 * (size_t)n_utt);
  {
    int* fu = reinterpret_cast<int*>(&img[o_futt]);
    for (int u = 0; u < n_utt; ++u)
      for (int64_t i = b.f_off[u]; i < b.f_off[u + 1]; ++i) fu[i] = u;
  }
  unsigned char* base = nullptr;
  int rc = wm_check(wm::dev_alloc(&base, take.at));
  if (!rc) b.d_arena = base;                     // freed with the batch
  if (!rc) rc = wm_check(hipMemcpy(base, img.data(), init_bytes, hipMemcpyHostToDevice));
  if (rc) {
    delete hb;
    return rc;
  }
  b.d_x_off = (int64_t*)(base + o_xoff); b.d_f_off = (int64_t*)(base + o_foff); b.d_y_off = (int64_t*)(base + o_yoff);
  b.d_x_len = (int*)(base + o_xlen); b.d_f0_len = (int*)(base + o_flen); b.d_y_len = (int*)(base + o_ylen);
  b.d_frame_utt = (int*)(base + o_futt);
  b.d_rng_off = (int*)(base + o_rng); b.d_rng_off2 = (int*)(base + o_rng2);
  b.d_ap0 = (double*)(base + o_ap0); b.d_f0_tmp = (double*)(base + o_f0t);
  b.d_perm = (int*)(base + o_perm); b.d_part_cnt = (int*)(base + o_pcnt); b.d_part_n = (int*)(base + o_pn);
  b.d_rng_off_d4c = (int*)(base + o_rng_d); b.d_perm_d4c = (int*)(base + o_perm_d);
  b.d_part_cnt_d4c = (int*)(base + o_pcnt_d); b.d_part_n_d4c = (int*)(base + o_pn_d);
  *out = hb;
  return WM_OK;
}

void WorldMi355DestroyBatch(WorldMi355Batch* hb) {
  if (!hb) return;
  Batch& b = hb->b;
  OnDevice dev_(*b.ctx);
  hipStreamSynchronize(b.ctx->stream);
  delete hb;
}

int64_t WorldMi355BatchTotalSamples(const WorldMi355Batch* b) { return b->b.total_x; }
int64_t WorldMi355BatchTotalFrames(const WorldMi355Batch* b) { return b->b.total_f; }
int64_t WorldMi355BatchTotalOutputSamples(const WorldMi355Batch* b) { return b->b.total_y; }
int WorldMi355BatchFftSize(const WorldMi355Batch* b) { return b->b.p.fft_size; }
const int64_t* WorldMi355BatchSampleOffsets(const WorldMi355Batch* b) { return b->b.x_off.data(); }
const int64_t* WorldMi355BatchFrameOffsets(const WorldMi355Batch* b) { return b->b.f_off.data(); }
const int64_t* WorldMi355BatchOutputOffsets(const WorldMi355Batch* b) { return b->b.y_off.data(); }

int WorldMi355Dio(WorldMi355Batch* b, const double* x, double* t, double* f0) {
  return on_batch(b, launch_dio, x, t, f0);
}
int WorldMi355StoneMask(WorldMi355Batch* b, const double* x, const double* t, const double* f0,
                        double* refined_f0) {
  return on_batch(b, launch_stonemask, x, t, f0, refined_f0);
}
int WorldMi355CheapTrick(WorldMi355Batch* b, const double* x, const double* t, const double* f0,
                         double* sp) {
  return on_batch(b, launch_cheaptrick, x, t, f0, sp);
}
int WorldMi355D4C(WorldMi355Batch* b, const double* x, const double* t, const double* f0, double* ap) {
  return on_batch(b, launch_d4c, x, t, f0, ap);
}
int WorldMi355Synthesis(WorldMi355Batch* b, const double* f0, const double* sp, const double* ap,
                        double* y) {
  return on_batch(b, launch_synthesis, f0, sp, ap, y);
}
int WorldMi355GetNumberOfAperiodicities(int fs) { return codec_num_aperiodicities(fs); }
int WorldMi355CodeSpectralEnvelope(WorldMi355Batch* b, const double* sp, int number_of_dimensions, double* coded) {
  return on_batch(b, launch_code_spectral_envelope, sp, number_of_dimensions, coded);
}
int WorldMi355DecodeSpectralEnvelope(WorldMi355Batch* b, const double* coded, int number_of_dimensions,
                                     double* sp) {
  return on_batch(b, launch_decode_spectral_envelope, coded, number_of_dimensions, sp);
}
int WorldMi355CodeAperiodicity(WorldMi355Batch* b, const double* ap, double* coded) {
  return on_batch(b, launch_code_aperiodicity, ap, coded);
}
int WorldMi355DecodeAperiodicity(WorldMi355Batch* b, const double* coded, double* ap) {
  return on_batch(b, launch_decode_aperiodicity, coded, ap);
}
int WorldMi355RecipeFeatures(WorldMi355Batch* b, const double* f0, const double* sp, const double* ap,
                             int spec_dim, int ap_dim, float* lf0, float* mgc, float* bap) {
  return on_batch(b, launch_recipe_features, f0, sp, ap, spec_dim, ap_dim, lf0, mgc, bap);
}
int WorldMi355RecipeDecode(WorldMi355Batch* b, const float* lf0, const float* mgc, const float* bap, int spec_dim,
                           int ap_dim, double* f0, double* sp, double* ap) {
  return on_batch(b, launch_recipe_decode, lf0, mgc, bap, spec_dim, ap_dim, f0, sp, ap);
}
void WorldMi355DefaultMcepOption(WorldMi355McepOption* o) {                     // SPTK's mcep / mgcep defaults
  if (!o) return;
  o->alpha = 0.35;
  o->order = 25;
  o->itr1 = 2;
  o->itr2 = 30;
  o->dd = 1e-3;
  o->etype = 0;
  o->e = 0.0;
  o->f = 1e-6;
  o->itype = 3;
}
int WorldMi355MelCepstrum(WorldMi355Batch* b, const double* spectrum, const WorldMi355McepOption* opt, double* mc,
                          int* status) {
  if (!b || !opt) return WM_ERR_BAD_ARG;
  if (const int rc = check_mel_cepstrum(b->b, spectrum, *opt, mc)) return rc;   // refused before any device call
  return on_batch(b, launch_mel_cepstrum, spectrum, *opt, mc, status);
}
int WorldMi355SptkFrames(int64_t n_samples, int frame_length, int frame_shift, int64_t* n_frames) {
  return sptk_frames(n_samples, frame_length, frame_shift, n_frames);
}
int WorldMi355SptkWindow(int type, int normalize, int length, double* w) {
  return sptk_window(type, normalize, length, w);
}
int WorldMi355MelCepstrumOfFrames(WorldMi355Batch* b, const double* frames, const WorldMi355McepOption* opt, double* mc,
                                  int* status) {
  if (!b || !opt) return WM_ERR_BAD_ARG;
  if (const int rc = check_mgcep(b->b, frames, false, nullptr, 0, 0, *opt, mc)) return rc;   // before any device call
  return on_batch(b, launch_mel_cepstrum_of_frames, frames, *opt, mc, status);
}
int WorldMi355MelCepstrumOfWaveform(WorldMi355Batch* b, const double* x, const double* window, int frame_length,
                                    int frame_shift, int pipe_float32, const WorldMi355McepOption* opt, double* mc,
                                    int* status) {
  if (!b || !opt) return WM_ERR_BAD_ARG;
  if (const int rc = check_mgcep(b->b, x, true, window, frame_length, frame_shift, *opt, mc)) return rc;
  return on_batch(b, launch_mel_cepstrum_of_waveform, x, window, frame_length, frame_shift, pipe_float32, *opt, mc,
                  status);
}
void WorldMi355DefaultMgc2spOption(WorldMi355Mgc2spOption* o) {                 // SPTK's mgc2sp defaults, ln |H| out
  if (!o) return;
  o->alpha = 0.35;
  o->gamma = 0.0;
  o->order = 25;
  o->out_format = 0;
}
int WorldMi355MelCepstrumToSpectrum(WorldMi355Batch* b, const double* mc, const WorldMi355Mgc2spOption* opt,
                                    double* spectrum, double* phase, int* status) {
  if (!b || !opt) return WM_ERR_BAD_ARG;
  if (const int rc = check_mgc2sp(b->b, mc, *opt, spectrum)) return rc;         // refused before any device call
  return on_batch(b, launch_mgc2sp, mc, *opt, spectrum, phase, status);
}
void WorldMi355DefaultMgcConvertOption(WorldMi355MgcConvertOption* o) {         // SPTK's mgc2mgc defaults
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->in_order = 25;
  o->out_order = 25;
}
int WorldMi355MelGeneralizedCepstrumConvert(WorldMi355Batch* b, const double* in, const WorldMi355MgcConvertOption* opt,
                                            double* out, int* status) {
  if (!b || !opt) return WM_ERR_BAD_ARG;
  if (const int rc = check_mgc2mgc(b->b.total_f, in, opt, out)) return rc;      // refused before any device call
  return on_batch(b, launch_mgc2mgc, in, *opt, out, status);
}
void WorldMi355DefaultLspOption(WorldMi355LspOption* o) {                       // lspcheck -r 0.1 -G 1e-10, SPTK's orders
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->order = 25;
  o->alpha = 0.35;
  o->gamma = -1.0;
  o->min_distance = 0.1;
  o->min_gain = 1e-10;
}
void WorldMi355DefaultLspPostfilterOption(WorldMi355LspPostfilterOption* o) {   // $pf_lsp 0.7, IMPLEN 4096
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->order = 25;
  o->alpha = 0.35;
  o->gamma = -1.0;
  o->min_distance = 0.1;
  o->min_gain = 1e-10;
  o->beta = 0.7;
  o->length = 4096;
}
int WorldMi355LspToLpc(WorldMi355Batch* b, const double* lsp, const WorldMi355LspOption* opt, double* lpc,
                       double* checked, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_lsp(b->b.total_f, lsp, opt, lpc, checked)) return rc;   // refused before any device call
  return on_batch(b, launch_lsp_to_lpc, lsp, *opt, lpc, checked, status);
}
int WorldMi355LspToMelGeneralizedCepstrum(WorldMi355Batch* b, const double* lsp, const WorldMi355LspOption* opt,
                                          int out_order, double out_alpha, double out_gamma, double* out, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_lsp_to_mgc(b->b.total_f, lsp, opt, out_order, out_alpha, out_gamma, out, status)) return rc;
  return on_batch(b, launch_lsp_to_mgc, lsp, *opt, out_order, out_alpha, out_gamma, out, status);
}
int WorldMi355LspPostfilter(WorldMi355Batch* b, const double* lsp, const WorldMi355LspPostfilterOption* opt, double* out,
                            double* ene1, double* ene2, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_lsp_postfilter(b->b.total_f, lsp, opt, out, ene1, ene2, status)) return rc;
  return on_batch(b, launch_lsp_postfilter, lsp, *opt, out, ene1, ene2, status);
}
void WorldMi355DefaultMlsaOption(WorldMi355MlsaOption* o) {                     // SPTK's mglsadf defaults, Pade order 4
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->alpha = 0.35;
  o->order = 25;
  o->pade_order = 4;
  o->frame_shift = 100;
}
int WorldMi355MlsaSamples(int n_frames, int frame_shift, int* n_samples) {
  return mlsa_samples(n_frames, frame_shift, n_samples);
}
int WorldMi355MlsaPade(int order, double* row) { return mlsa_pade(order, row); }
int WorldMi355MlsaNoise(int64_t n, double* out) { return mlsa_noise(n, out); }
int WorldMi355MlsaExcitation(WorldMi355Batch* b, const float* pitch, const double* lowpass, int n_low,
                             const double* highpass, int n_high, const WorldMi355MlsaOption* opt, double* e) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_mlsa(b->b, 1, pitch, nullptr, lowpass, n_low, highpass, n_high, opt, e, nullptr))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_mlsa_excitation, pitch, lowpass, n_low, highpass, n_high, *opt, e);
}
int WorldMi355MlsaFilter(WorldMi355Batch* b, const double* e, const float* mc, const WorldMi355MlsaOption* opt, double* y,
                         int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_mlsa(b->b, 2, nullptr, mc, nullptr, 0, nullptr, 0, opt, e, y)) return rc;
  return on_batch(b, launch_mlsa_filter, e, mc, *opt, y, status);
}
int WorldMi355MlsaSynthesis(WorldMi355Batch* b, const float* pitch, const float* mc, const double* lowpass, int n_low,
                            const double* highpass, int n_high, const WorldMi355MlsaOption* opt, double* y, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_mlsa(b->b, 3, pitch, mc, lowpass, n_low, highpass, n_high, opt, nullptr, y)) return rc;
  return on_batch(b, launch_mlsa_synthesis, pitch, mc, lowpass, n_low, highpass, n_high, *opt, y, status);
}
void WorldMi355DefaultDistortionOption(WorldMi355DistortionOption* o) {
  if (!o) return;
  o->voiced_above = -1.0e9;                                                     // the recipe's unvoiced value is -1e10
}
int WorldMi355DtwWorkspaceBytes(int n_utt, const int* a_lengths, const int* b_lengths, int64_t* bytes) {
  return dtw_workspace_bytes(n_utt, a_lengths, b_lengths, bytes);
}
int WorldMi355DtwAlign(WorldMi355Batch* b, const float* a, int64_t ld_a, const float* bs, int64_t ld_b, const int64_t* b_off,
                       int first, int count, int* path, int* path_len, double* cost, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_dtw(b->b, a, ld_a, bs, ld_b, b_off, first, count, path, path_len, cost))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_dtw_align, a, ld_a, bs, ld_b, b_off, first, count, path, path_len, cost, status);
}
int WorldMi355FeatureDistortion(WorldMi355Batch* b, const int* path, const int* path_len, const int64_t* b_off,
                                const unsigned char* b_mask, int n_groups, const WorldMi355DistortionGroup* groups,
                                const WorldMi355DistortionOption* opt, double* out) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_distortion(b->b, path, path_len, b_off, n_groups, groups, opt, out)) return rc;
  return on_batch(b, launch_feature_distortion, path, path_len, b_off, b_mask, n_groups, groups, *opt, out);
}
int WorldMi355ComposeCmp(WorldMi355Batch* b, int n_streams, const float* const* streams, const int* dims,
                         const int* n_windows, const double* const* const* windows,
                         const int* const* window_sizes, float* out) {
  if (const int rc = check_compose_cmp(n_streams, streams, dims, n_windows, windows, window_sizes, out)) return rc;
  return on_batch(b, launch_compose_cmp, n_streams, streams, dims, n_windows, windows, window_sizes, out);
}
void WorldMi355DefaultMlpgOption(WorldMi355MlpgOption* o) {                     // SPTK's mlpg: taps beyond the ends dropped
  if (!o) return;
  o->edge = 0;
  o->var_per_frame = 0;
  o->input_type = 0;
  o->unvoiced_value = -1.0e+10;
}
int WorldMi355ParameterGeneration(WorldMi355Batch* b, int n_streams, const float* const* mean, int64_t ld_mean,
                                  const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                                  const double* const* const* windows, const int* const* window_sizes,
                                  const float* const* msd, const WorldMi355MlpgOption* opt, float* const* out,
                                  int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_mlpg(n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes, opt, out))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_mlpg, n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes, msd,
                  *opt, out, status);
}
void WorldMi355DefaultGvOption(WorldMi355GvOption* o) {                         // configure.ac:808-880
  if (!o) return;
  o->max_iter = 50;
  o->scale = 1;
  o->epsilon = 1.0e-4;
  o->step_init = 1.0;
  o->step_inc = 1.2;
  o->step_dec = 0.5;
  o->hmm_weight = 1.0;
  o->gv_weight = 1.0;
}
int WorldMi355ParameterGenerationGv(WorldMi355Batch* b, int n_streams, const float* const* mean, int64_t ld_mean,
                                    const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                                    const double* const* const* windows, const int* const* window_sizes,
                                    const float* const* msd, const WorldMi355MlpgOption* opt,
                                    const float* const* gv_mean, const float* const* gv_var,
                                    const unsigned char* gv_mask, const WorldMi355GvOption* gv, float* const* out,
                                    double* info, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_mlpg(n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes, opt, out))
    return rc;                                                                  // refused before any device call
  if (const int rc = check_mlpg_gv(n_streams, dims, gv_mean, gv_var, gv)) return rc;
  return on_batch(b, launch_mlpg_gv, n_streams, mean, ld_mean, var, ld_var, dims, n_windows, windows, window_sizes, msd,
                  *opt, gv_mean, gv_var, gv_mask, *gv, out, info, status);
}
void WorldMi355DefaultTrajectoryOption(WorldMi355TrajectoryOption* o) {         // DNNDefine.py:248-249
  if (!o) return;
  o->edge = 0;
  o->msd_weight = 1.0;
  o->gv_weight = 1.0e-6;
}
int WorldMi355TrajectoryCost(WorldMi355Batch* b, int n_streams, const float* const* pred, const float* const* obs,
                             int64_t ld, const float* const* var, const float* const* gv_var, const int* dims,
                             const int* n_windows, const double* const* const* windows, const int* const* window_sizes,
                             const float* const* msd_pred, const float* const* msd_obs, const float* const* msd_var,
                             const WorldMi355TrajectoryOption* opt, double* cost, float* const* c,
                             float* const* grad_pred, float* const* grad_msd, int64_t ld_grad, double* grad_var,
                             int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_trj(n_streams, pred, obs, ld, var, gv_var, dims, n_windows, windows, window_sizes, msd_pred,
                               msd_obs, msd_var, opt, cost, grad_pred, grad_msd, ld_grad))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_trj, n_streams, pred, obs, ld, var, gv_var, dims, n_windows, windows, window_sizes,
                  msd_pred, msd_obs, msd_var, *opt, cost, c, grad_pred, grad_msd, ld_grad, grad_var, status);
}
int WorldMi355AcousticModelForward(WorldMi355Batch* b, const WorldMi355AcousticModel* m, const float* x, int64_t ld_x,
                                   const int* spkr, float* out, int64_t ld_out, const float* obs, int64_t ld_obs,
                                   double* cost, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_dnn(b->b.n_utt, m, x, ld_x, spkr, out, ld_out, obs, ld_obs, cost))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_dnn, *m, x, ld_x, spkr, out, ld_out, obs, ld_obs, cost, status);
}
int WorldMi355AcousticModelTrainForward(WorldMi355Batch* b, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop,
                                        const float* x, int64_t ld_x, const int* spkr, float* out, int64_t ld_out,
                                        const float* obs, int64_t ld_obs, double* cost, float* grad_out, int64_t ld_grad,
                                        double* grad_var, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_dnn_train_forward(b->b.n_utt, m, drop, x, ld_x, spkr, out, ld_out, obs, ld_obs, cost, grad_out,
                                             ld_grad, grad_var))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_dnn_train_forward, *m, drop, x, ld_x, spkr, out, ld_out, obs, ld_obs, cost, grad_out,
                  ld_grad, grad_var, status);
}
int WorldMi355AcousticModelBackward(WorldMi355Batch* b, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop,
                                    const float* x, int64_t ld_x, const int* spkr, const float* grad_out, int64_t ld_grad,
                                    float* const* grad_weights, float* const* grad_biases, float* const* grad_spkr_weights,
                                    int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_dnn_backward(b->b.n_utt, m, drop, x, ld_x, spkr, grad_out, ld_grad, grad_weights, grad_biases,
                                        grad_spkr_weights))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_dnn_backward, *m, drop, x, ld_x, spkr, grad_out, ld_grad, grad_weights, grad_biases,
                  grad_spkr_weights, status);
}
void WorldMi355DefaultOptimizerOption(int rule, WorldMi355OptimizerOption* o) {   // tf.train.*Optimizer's defaults (TF 1.x)
  if (!o) return;
  o->rule = rule;
  o->momentum = rule == 1 ? 0.9f : 0.0f;
  o->rho = rule == 3 ? 0.95f : 0.9f;
  o->beta1 = 0.9f;
  o->beta2 = 0.999f;
  o->epsilon = rule == 5 ? 1e-10f : 1e-8f;
  o->beta1_power = o->beta1;
  o->beta2_power = o->beta2;
}
int WorldMi355OptimizerStep(WorldMi355Context* h, const WorldMi355OptimizerOption* opt, int n_tensors, float* const* param,
                            const float* const* grad, float* const* slot0, float* const* slot1, const int64_t* count,
                            const float* rate, int* status) {
  if (!h) return WM_ERR_BAD_ARG;
  if (const int rc = check_optimizer_step(opt, n_tensors, param, grad, slot0, slot1, count, rate))
    return rc;                                                                  // refused before any device call
  OnDevice dev_(h->c);
  return launch_optimizer_step(h->c, h->c.stream, *opt, n_tensors, param, grad, slot0, slot1, count, rate, status);
}
void WorldMi355DefaultMcpfOption(WorldMi355McpfOption* o) {                     // SPTK's alpha and order, the recipe's beta and IMPLEN
  if (!o) return;
  o->alpha = 0.35;
  o->beta = 1.4;
  o->order = 25;
  o->length = 4096;
}
int WorldMi355MelCepstrumPostfilter(WorldMi355Batch* b, const double* mc, const WorldMi355McpfOption* opt, double* out,
                                    double* gain, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_mcpf(mc, opt, out)) return rc;                       // refused before any device call
  return on_batch(b, launch_mcpf, mc, *opt, out, gain, status);
}
int WorldMi355ModifyFeatures(WorldMi355Batch* b, const double* f0_scale, const double* formant_ratio, const double* f0,
                             const double* sp, double* f0_out, double* sp_out) {
  if (!b) return WM_ERR_BAD_ARG;
  if (const int rc = check_modify(b->b, f0_scale, formant_ratio, f0, sp, f0_out, sp_out)) return rc;   // before any device call
  return on_batch(b, launch_modify, f0_scale, formant_ratio, f0, sp, f0_out, sp_out);
}
void WorldMi355DefaultMspfOption(WorldMi355MspfOption* o) {                     // the recipe's $mspfLength, $mspfFFTLen, $mspfe{'mgc'}
  if (!o) return;
  o->frame_length = 25;
  o->fft_length = 64;
  o->emphasis = 1.0;
}
int WorldMi355MspfSegmentFrames(void) { return mspf_segment_frames(); }
int WorldMi355ColumnMeans(WorldMi355Batch* b, const double* x, int dim, double* mean) {
  if (const int rc = check_column_means(x, dim, mean)) return rc;               // refused before any device call
  return on_batch(b, launch_column_means, x, dim, mean);
}
int WorldMi355ModulationSpectrumPostfilter(WorldMi355Batch* b, const double* x, int dim, const WorldMi355MspfOption* opt,
                                           const double* mean_gen, const double* std_gen, const double* mean_nat,
                                           const double* std_nat, double* out, int* status) {
  if (const int rc = check_mspf(x, dim, opt, mean_gen, std_gen, mean_nat, std_nat, out)) return rc;
  return on_batch(b, launch_mspf, x, dim, *opt, mean_gen, std_gen, mean_nat, std_nat, out, status);
}
int WorldMi355ModulationSpectrumStats(WorldMi355Batch* b, const double* x, int dim, const WorldMi355MspfOption* opt,
                                      const double* mean, double* sum, double* sumsq, int64_t* n_frames) {
  if (const int rc = check_mspf_stats(x, dim, opt, sum, sumsq, n_frames)) return rc;
  return on_batch(b, launch_mspf_stats, x, dim, *opt, mean, sum, sumsq, n_frames);
}
int WorldMi355InterpolateGaps(WorldMi355Batch* b, const float* x, int dim, double ignore_value, float* out, float* voiced,
                               int* status) {
  if (const int rc = check_interpolate_gaps(x, dim, ignore_value, out)) return rc;   // refused before any device call
  return on_batch(b, launch_interpolate_gaps, x, dim, ignore_value, out, voiced, status);
}
int WorldMi355ComposeFfo(WorldMi355Batch* b, int n_streams, const float* const* streams, const int* dims,
                         const int* n_windows, const double* const* const* windows, const int* const* window_sizes,
                         const float* const* msd, float* out) {
  if (const int rc = check_compose_ffo(n_streams, streams, dims, n_windows, windows, window_sizes, out)) return rc;
  return on_batch(b, launch_compose_ffo, n_streams, streams, dims, n_windows, windows, window_sizes, msd, out);
}
int WorldMi355ColumnMoments(WorldMi355Batch* b, const float* x, int64_t ld, int width, const double* ignore_value,
                            int64_t* count, double* mean, double* m2) {
  if (const int rc = check_column_moments(x, ld, width, ignore_value, count, mean, m2)) return rc;
  return on_batch(b, launch_column_moments, x, ld, width, ignore_value, count, mean, m2);
}
int WorldMi355CreateLabelFeatureSet(WorldMi355Context* h, int n_features, const WorldMi355LabelFeature* features,
                                    WorldMi355LabelFeatureSet** out) {
  if (!out) return WM_ERR_BAD_ARG;
  *out = nullptr;
  if (!h) return WM_ERR_BAD_ARG;
  OnDevice dev_(h->c);
  LabelSet* s = nullptr;
  const int rc = label_set_create(h->c, n_features, features, &s);              // a refused config makes no device call
  *out = reinterpret_cast<WorldMi355LabelFeatureSet*>(s);
  return rc;
}
void WorldMi355DestroyLabelFeatureSet(WorldMi355LabelFeatureSet* set) {
  label_set_destroy(reinterpret_cast<LabelSet*>(set));
}
int WorldMi355LabelFeatureCount(const WorldMi355LabelFeatureSet* set) {
  return label_set_count(reinterpret_cast<const LabelSet*>(set));
}
int WorldMi355LabelFeatures(WorldMi355Batch* b, const WorldMi355LabelFeatureSet* set, const int* line_off, const int* start,
                            const int* end, const int* state_index, const char* const* name, const int* state_level,
                            float* out, int64_t ld_out, int* status) {
  if (!b) return WM_ERR_BAD_ARG;
  const LabelSet* s = reinterpret_cast<const LabelSet*>(set);
  if (const int rc = check_label_features(b->b, s, line_off, start, end, state_index, name, state_level, out, ld_out))
    return rc;                                                                  // refused before any device call
  return on_batch(b, launch_label_features, *s, line_off, start, end, state_index, name, state_level, out, ld_out,
                  status);
}
void WorldMi355HtkHeader(int n_frames, int sampling_rate, int frame_shift_samples, int bytes_per_frame,
                         int htk_type, unsigned char out12[12]) {              // addhtkheader.pl:60-75
  const int32_t a = n_frames, fs100 = (int32_t)(10000000.0 * frame_shift_samples / sampling_rate);
  const int16_t c = (int16_t)bytes_per_frame, d = (int16_t)htk_type;
  memcpy(out12, &a, 4);
  memcpy(out12 + 4, &fs100, 4);
  memcpy(out12 + 8, &c, 2);
  memcpy(out12 + 10, &d, 2);
}
int WorldMi355SamplesFromPcm16(WorldMi355Batch* b, const int16_t* pcm, double* x) {
  return on_batch(b, launch_pcm16_to_samples, pcm, x);
}
int WorldMi355SamplesToPcm16(WorldMi355Batch* b, const double* y, int16_t* pcm) {
  return on_batch(b, launch_samples_to_pcm16, y, pcm);
}
int WorldMi355Harvest(WorldMi355Batch* b, const double* x, double* t, double* f0) {
  return on_batch(b, launch_harvest, x, t, f0);
}
int WorldMi355Analyze(WorldMi355Batch* hb, const double* x, double* t, double* f0, double* sp,
                      double* ap) {
  return on_batch(hb, launch_analyze, x, t, f0, sp, ap);
}
int WorldMi355AnalyzeSynthesize(WorldMi355Batch* hb, const double* x, double* t, double* f0, double* sp,
                                double* ap, double* y) {
  return on_batch(hb, launch_analyze_synthesize, x, t, f0, sp, ap, y);
}
int WorldMi355BatchSetF0Estimator(WorldMi355Batch* hb, int estimator, int refine) {
  if (!hb || (estimator != WM_F0_DIO && estimator != WM_F0_HARVEST) || (refine != 0 && refine != 1) || hb->b.total_x <= 0) {
    wm::set_error("BatchSetF0Estimator: a batch with x_lengths, WM_F0_DIO or WM_F0_HARVEST, refine 0 or 1");
    return WM_ERR_BAD_ARG;
  }
  hb->b.f0_estimator = estimator;                // host state only: the next one-call form reads it (launch_f0)
  hb->b.f0_refine = refine;
  return WM_OK;
}
int WorldMi355BatchGetF0Estimator(const WorldMi355Batch* hb, int* estimator, int* refine) {
  if (!hb || !estimator || !refine) return WM_ERR_BAD_ARG;
  *estimator = hb->b.f0_estimator;
  *refine = hb->b.f0_refine;
  return WM_OK;
}
int WorldMi355HarvestWorkspaceBytes(const WorldMi355Params* p, int n_utt, const int* x_lengths, int64_t* bytes) {
  bool ok = p && x_lengths && bytes && n_utt > 0 && p->fs > 0 && p->f0_floor > 0.0 && p->f0_ceil > p->f0_floor;
  for (int u = 0; ok && u < n_utt; ++u) ok = x_lengths[u] > 0;
  if (!ok) {
    wm::set_error("HarvestWorkspaceBytes: bad argument");
    return WM_ERR_BAD_ARG;
  }
  return harvest_workspace_bytes(*p, n_utt, x_lengths, bytes);
}
int WorldMi355Vibrato(WorldMi355Batch* hb, const float* lf0, const int* seg_utt_off, const int* seg_start,
                      const int* seg_end, const double* seg_pitch, float* vib, float* lf0_out, int* n_too_long) {
  return on_batch(hb, launch_vibrato, lf0, seg_utt_off, seg_start, seg_end, seg_pitch, vib, lf0_out, n_too_long);
}
int WorldMi355UtteranceStatus(WorldMi355Batch* hb, const double* x, const double* f0, const double* sp,
                              const double* ap, int* status) {
  return on_batch(hb, launch_utterance_status, x, f0, sp, ap, status);
}
#ifdef WM_PHASE
// debug builds only (make EXTRA=-DWM_PHASE): the shader-clock totals of the phase marks of one translation unit
// (0 = d4c.hip, 1 = cheaptrick.hip, 2 = synthesis.hip), read and cleared
__attribute__((visibility("default"))) int WorldMi355DebugPhases(int unit, unsigned long long* out32) {
  return unit == 0 ? wm::phase_read_d4c(out32) : unit == 1 ? wm::phase_read_cheaptrick(out32) : wm::phase_read_synthesis(out32);
}
#endif
void WorldMi355SetErrorHandler(WorldMi355ErrorHandler handler, void* user) {
  std::lock_guard<std::mutex> lock(g_err_mu);
  g_on_error = handler;
  g_on_error_user = user;
}
int WorldMi355TimingEnable(WorldMi355Context* h, int on) {
  OnDevice dev_(h->c);
  Context& c = h->c;
  int rc = wm_check(hipStreamSynchronize(c.stream));
  c.timing_clear();
  c.timing = on != 0;
  return rc;
}
int WorldMi355TimingQuery(WorldMi355Context* h, const char* kernel, double* total_ms, int* launches) {
  OnDevice dev_(h->c);
  Context& c = h->c;
  int rc = wm_check(hipStreamSynchronize(c.stream));
  if (rc) return rc;
  *total_ms = 0.0;
  *launches = 0;
  auto it = c.timed.find(kernel);
  if (it == c.timed.end()) return WM_OK;
  for (auto& pr : it->second) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { *total_ms += ms; *launches += 1; }
  }
  return WM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// WORLD's own API: host pointers, one utterance, B = 1 batch.
// ---------------------------------------------------------------------------
namespace {

std::mutex g_mu;
WorldMi355Context* g_ctx = nullptr;

// A failure inside a drop-in entry point (no device, a HIP error, an unsupported size): the reference's functions
// return void, so by default it ends in a message on stderr and abort(), like the reference's own bad_alloc.  A host
// that would rather lose one utterance than the process installs a handler (WorldMi355SetErrorHandler): the failure
// then unwinds to the entry point, which calls the handler and returns with its outputs unspecified.
struct DropInError {
  const char* where;
  int code;
  WorldMi355ErrorHandler handler;   // the handler that was installed when the failure happened: a concurrent
  void* user;                       // WorldMi355SetErrorHandler(NULL) cannot make the failure vanish
};
[[noreturn]] void die(const char* where, int rc) {
  void* user = nullptr;
  if (WorldMi355ErrorHandler handler = error_handler(&user)) throw DropInError{where, rc, handler, user};
  fprintf(stderr, "libworld_mi355: %s failed (code %d): %s\n", where, rc, WorldMi355LastError());
  abort();
}

WorldMi355Context* default_context() {
  if (!g_ctx) {
    int rc = WorldMi355CreateContext(-1, nullptr, &g_ctx);
    if (rc) die("CreateContext", rc);
  }
  return g_ctx;
}

// ---- persistent workspace of the per-utterance entry points ------------------------------------------------
// The reference's API is stateless: every call brings host pointers and takes its results home.  Doing that
// literally -- a fresh batch, fresh device buffers and pageable copies per call -- cost 8 ms per utterance of 5 s,
// most of it allocation and staging rather than kernels.  What persists here between calls (per process, under the
// same mutex as the calls; nothing of it is visible to the caller):
//   * device buffers by role (x, t, f0, f0 out, sp, ap, coded, y), grow-only;
//   * one pinned staging buffer, grow-only: `double**` rows are gathered into / scattered from it, so the DMA
//     engine always sees pinned contiguous memory;
//   * the last few batches by (parameters, lengths): Dio, StoneMask, CheapTrick and D4C of one utterance, or the
//     same call on the next utterance of equal length, reuse descriptors and stage workspaces;
//   * a host copy of the last uploaded waveform: the four analysis calls of one utterance pass the same x, which
//     is then uploaded once (a memcmp of the samples decides, not the pointer).
enum Slot { kX, kT, kF0, kOut, kSp, kAp, kCoded, kY, kSlots };

struct Workspace {
  void* dev[kSlots] = {};
  size_t dev_cap[kSlots] = {};
  void* pinned = nullptr;
  size_t pinned_cap = 0;
  std::vector<double> x_copy;           // what dev[kX] holds
  bool x_valid = false;
  struct Entry { WorldMi355Params p; int xl, fl, yl; WorldMi355Batch* b; unsigned long stamp; };
  std::vector<Entry> cache;
  unsigned long clock = 0;

  double* device(Slot s, size_t n) {
    const size_t bytes = sizeof(double) * (n ? n : 1);
    if (bytes > dev_cap[s]) {
      if (s == kX) x_valid = false;
      if (dev[s]) wm::dev_free(dev[s]);
      dev[s] = nullptr;
      const size_t cap = bytes + bytes / 4;
      if (wm::dev_alloc(&dev[s], cap) != hipSuccess) die("hipMalloc", WM_ERR_HIP);
      dev_cap[s] = cap;
    }
    return (double*)dev[s];
  }
  // Pinned staging of one API call: regions are handed out one after another (no region is reused inside a call,
  // so no copy has to be waited for before the next argument is staged) and the call ends with finish(): ONE
  // stream synchronisation, then the host-side copies of the results.  Growing moves what the call has staged.
  size_t stage_at = 0;                   // doubles in use by the current call
  struct Pending { size_t off; double* flat; double** rows; size_t n; int n_rows, width; };
  std::vector<Pending> pending;
  double* stage(size_t n) {
    const size_t need = sizeof(double) * (stage_at + n + 8);
    if (need > pinned_cap) {
      if (hipStreamSynchronize(default_context()->c.stream) != hipSuccess) die("staging", WM_ERR_HIP);
      void* grown = nullptr;
      const size_t cap = need + need / 2;
      if (hipHostMalloc(&grown, cap, hipHostMallocDefault) != hipSuccess) die("hipHostMalloc", WM_ERR_HIP);
      if (pinned) {
        memcpy(grown, pinned, sizeof(double) * stage_at);
        (void)hipHostFree(pinned);
      }
      pinned = grown;
      pinned_cap = cap;
    }
    double* r = (double*)pinned + stage_at;
    stage_at += (n + 7) & ~(size_t)7;
    return r;
  }
  void finish() {
    if (hipStreamSynchronize(default_context()->c.stream) != hipSuccess) die("finish", WM_ERR_HIP);
    for (const Pending& q : pending) {
      const double* st = (const double*)pinned + q.off;
      if (q.flat) {
        if (q.n) memcpy(q.flat, st, sizeof(double) * q.n);
      } else {
        for (int i = 0; i < q.n_rows; ++i) memcpy(q.rows[i], st + (size_t)i * q.width, sizeof(double) * q.width);
      }
    }
    pending.clear();
    stage_at = 0;
  }
  WorldMi355Batch* batch(const WorldMi355Params& p, int xl, int fl, int yl) {
    ++clock;
    for (Entry& e : cache)
      if (e.xl == xl && e.fl == fl && e.yl == yl && memcmp(&e.p, &p, sizeof(p)) == 0) {
        e.stamp = clock;
        return e.b;
      }
    if (cache.size() >= 8) {                  // drop the least recently used
      size_t lru = 0;
      for (size_t i = 1; i < cache.size(); ++i)
        if (cache[i].stamp < cache[lru].stamp) lru = i;
      WorldMi355DestroyBatch(cache[lru].b);
      cache.erase(cache.begin() + (long)lru);
    }
    WorldMi355Batch* b = nullptr;
    int rc = WorldMi355CreateBatch(default_context(), &p, 1, xl >= 0 ? &xl : nullptr, fl >= 0 ? &fl : nullptr,
                                   yl >= 0 ? &yl : nullptr, &b);
    if (rc) die("CreateBatch", rc);
    Entry e;
    e.p = p; e.xl = xl; e.fl = fl; e.yl = yl; e.b = b; e.stamp = clock;
    cache.push_back(e);
    return b;
  }
};
// Never destroyed (a leaked singleton, like g_ctx): at process exit the HIP runtime may already be gone when static
// destructors run, and a destroyed cache whose batches are then unreachable is what a leak checker reports.
Workspace& g_ws = *new Workspace();

void drop_in_failed(const DropInError& e) {
  (void)hipDeviceSynchronize();               // nothing of the failed call may still write into the staging buffers
  g_ws.pending.clear();
  g_ws.stage_at = 0;
  g_ws.x_valid = false;
  e.handler(e.where, e.code, WorldMi355LastError(), e.user);
}

// A drop-in entry point's body: one call at a time, and a failure that unwinds from it (die() with a handler installed)
// ends in that handler.
template <class Body> void drop_in(Body body) {
  std::lock_guard<std::mutex> lock(g_mu);
  try {
    body();
  } catch (const DropInError& e) {
    drop_in_failed(e);
  }
}

hipStream_t ws_stream() { return default_context()->c.stream; }

// the upload stream of Synthesis(): its sp / ap rows travel beside the f0-only kernels, not behind them
struct Upload : Handles {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
};
const Upload* g_up = nullptr;            // made on first use and never destroyed, like g_ctx
const Upload& upload_stream() {
  if (!g_up) {
    std::unique_ptr<Upload> u(new Upload());
    if (u->Handles::stream(&u->stream) != hipSuccess || u->event(&u->done) != hipSuccess) die("upload stream", WM_ERR_HIP);
    g_up = u.release();
  }
  return *g_up;
}

void h2d(double* dst, const double* staged, size_t n, hipStream_t st = nullptr) {
  if (n && hipMemcpyAsync(dst, staged, sizeof(double) * n, hipMemcpyHostToDevice, st ? st : ws_stream()) != hipSuccess)
    die("H2D", WM_ERR_HIP);
}
// contiguous host array -> device slot through a staging region of this call (asynchronous: see Workspace::stage)
double* put(Slot s, const double* h, size_t n) {
  double* d = g_ws.device(s, n);
  double* st = g_ws.stage(n);
  if (n) memcpy(st, h, sizeof(double) * n);
  h2d(d, st, n);
  return d;
}
double* put_x(const double* x, size_t n) {
  if (g_ws.x_valid && g_ws.x_copy.size() == n && (n == 0 || memcmp(g_ws.x_copy.data(), x, sizeof(double) * n) == 0))
    return (double*)g_ws.dev[kX];
  g_ws.x_valid = false;
  double* d = put(kX, x, n);
  g_ws.x_copy.assign(x, x + n);
  g_ws.x_valid = true;
  return d;
}
double* put_rows(Slot s, const double* const* rows, int n_rows, int width, hipStream_t stream = nullptr) {
  const size_t n = (size_t)n_rows * width;
  double* d = g_ws.device(s, n);
  double* st = g_ws.stage(n);
  for (int i = 0; i < n_rows; ++i) memcpy(st + (size_t)i * width, rows[i], sizeof(double) * width);
  h2d(d, st, n, stream);
  return d;
}
// device -> a staging region (after the kernels on the stream); the host copy happens in finish()
size_t fetch(const double* d, size_t n) {
  double* st = g_ws.stage(n);
  const size_t off = (size_t)(st - (double*)g_ws.pinned);
  if (n && hipMemcpyAsync(st, d, sizeof(double) * n, hipMemcpyDeviceToHost, ws_stream()) != hipSuccess)
    die("D2H", WM_ERR_HIP);
  return off;
}
void get(const double* d, double* h, size_t n) {
  const size_t off = fetch(d, n);
  g_ws.pending.push_back({off, h, nullptr, n, 0, 0});
}
void get_rows(const double* d, double** rows, int n_rows, int width) {
  const size_t off = fetch(d, (size_t)n_rows * width);
  g_ws.pending.push_back({off, nullptr, rows, 0, n_rows, width});
}
void run_or_die(const char* where, int rc) {
  if (rc) die(where, rc);
}

// WORLD_MI355_TRACE=1: where the wall time of a drop-in call goes, to stderr (host staging / launches + kernels / the
// way back); synchronises after every stage, so the totals are somewhat above the untraced call's
struct CallTrace {
  bool on;
  double t0, last;
  const char* name;
  char line[256];
  int at = 0;
  static double now() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
  }
  explicit CallTrace(const char* n) : name(n) {
    static const bool enabled = getenv("WORLD_MI355_TRACE") && atoi(getenv("WORLD_MI355_TRACE")) != 0;
    on = enabled;
    if (on) t0 = last = now();
    line[0] = 0;
  }
  void mark(const char* what, bool sync = false) {
    if (!on) return;
    if (sync) (void)hipStreamSynchronize(ws_stream());
    const double t = now();
    at += snprintf(line + at, sizeof(line) - (size_t)at, " %s %.3f", what, t - last);
    last = t;
  }
  ~CallTrace() {
    if (on) fprintf(stderr, "[world_mi355] %s:%s | total %.3f ms\n", name, line, now() - t0);
  }
};

}  // namespace

extern "C" {

int GetSamplesForDIO(int fs, int x_length, double frame_period) {      // dio.cpp:638-640
  return (int)(1000.0 * x_length / fs / frame_period) + 1;
}
void InitializeDioOption(DioOption* option) {                           // dio.cpp:649-665
  option->channels_in_octave = 2.0;
  option->f0_ceil = 800.0;
  option->f0_floor = 71.0;
  option->frame_period = 5;
  option->speed = 1;
  option->allowed_range = 0.1;
}
void Dio(const double* x, int x_length, int fs, const DioOption* option, double* temporal_positions,
         double* f0) {
  drop_in([&] {
    WorldMi355Params p;
    WorldMi355DefaultParams(fs, option->frame_period, &p);
    p.f0_floor = option->f0_floor; p.f0_ceil = option->f0_ceil;
    p.channels_in_octave = option->channels_in_octave; p.speed = option->speed;
    p.allowed_range = option->allowed_range;
    p.fft_size = 1024;   // unused by DIO
    CallTrace tr("Dio");
    WorldMi355Batch* b = g_ws.batch(p, x_length, -1, -1);
    tr.mark("batch");
    const size_t nf = (size_t)WorldMi355BatchTotalFrames(b);
    double* dx = put_x(x, (size_t)x_length);
    tr.mark("stage");
    double* dt = g_ws.device(kT, nf);
    double* df = g_ws.device(kF0, nf);
    run_or_die("Dio", WorldMi355Dio(b, dx, dt, df));
    tr.mark("launch");
    tr.mark("kernels", true);
    get(dt, temporal_positions, nf);
    get(df, f0, nf);
    g_ws.finish();
    tr.mark("back");
  });
}

int GetSamplesForHarvest(int fs, int x_length, double frame_period) {  // harvest.cpp:1219-1221
  return (int)(1000.0 * x_length / fs / frame_period) + 1;
}
void InitializeHarvestOption(HarvestOption* option) {                   // harvest.cpp:1257-1262
  option->f0_ceil = 800.0;
  option->f0_floor = 71.0;
  option->frame_period = 5;
}
void Harvest(const double* x, int x_length, int fs, const HarvestOption* option,
             double* temporal_positions, double* f0) {
  drop_in([&] {
    WorldMi355Params p;
    WorldMi355DefaultParams(fs, option->frame_period, &p);
    p.f0_floor = option->f0_floor; p.f0_ceil = option->f0_ceil;
    p.fft_size = 1024;   // unused by Harvest
    WorldMi355Batch* b = g_ws.batch(p, x_length, -1, -1);
    const size_t nf = (size_t)WorldMi355BatchTotalFrames(b);
    double* dx = put_x(x, (size_t)x_length);
    double* dt = g_ws.device(kT, nf);
    double* df = g_ws.device(kF0, nf);
    run_or_die("Harvest", WorldMi355Harvest(b, dx, dt, df));
    get(dt, temporal_positions, nf);
    get(df, f0, nf);
    g_ws.finish();
  });
}

void StoneMask(const double* x, int x_length, int fs, const double* temporal_positions, const double* f0,
               int f0_length, double* refined_f0) {
  drop_in([&] {
    WorldMi355Params p;
    WorldMi355DefaultParams(fs, 5.0, &p);
    p.fft_size = 1024;   // unused by StoneMask
    WorldMi355Batch* b = g_ws.batch(p, x_length, f0_length, -1);
    double* dx = put_x(x, (size_t)x_length);
    double* dt = put(kT, temporal_positions, (size_t)f0_length);
    double* df = put(kF0, f0, (size_t)f0_length);
    double* dr = g_ws.device(kOut, (size_t)f0_length);
    run_or_die("StoneMask", WorldMi355StoneMask(b, dx, dt, df, dr));
    get(dr, refined_f0, (size_t)f0_length);
    g_ws.finish();
  });
}

int GetFFTSizeForCheapTrick(int fs, const CheapTrickOption* option) {   // cheaptrick.cpp:191-194
  return (int)pow(2.0, 1.0 + (int)(log(3.0 * fs / option->f0_floor + 1) / kLog2));
}
double GetF0FloorForCheapTrick(int fs, int fft_size) {                   // cheaptrick.cpp:196-198
  return 3.0 * fs / (fft_size - 3.0);
}
void InitializeCheapTrickOption(int fs, CheapTrickOption* option) {      // cheaptrick.cpp:230-239
  option->q1 = -0.15;
  option->f0_floor = 71.0;
  option->fft_size = GetFFTSizeForCheapTrick(fs, option);
}
void CheapTrick(const double* x, int x_length, int fs, const double* temporal_positions, const double* f0,
                int f0_length, const CheapTrickOption* option, double** spectrogram) {
  drop_in([&] {
    WorldMi355Params p;
    WorldMi355DefaultParams(fs, 5.0, &p);
    p.q1 = option->q1;
    p.fft_size = option->fft_size;
    const int w = option->fft_size / 2 + 1;
    CallTrace tr("CheapTrick");
    WorldMi355Batch* b = g_ws.batch(p, x_length, f0_length, -1);
    tr.mark("batch");
    double* dx = put_x(x, (size_t)x_length);
    double* dt = put(kT, temporal_positions, (size_t)f0_length);
    double* df = put(kF0, f0, (size_t)f0_length);
    tr.mark("stage");
    double* ds = g_ws.device(kSp, (size_t)f0_length * w);
    run_or_die("CheapTrick", WorldMi355CheapTrick(b, dx, dt, df, ds));
    tr.mark("launch");
    tr.mark("kernels", true);
    get_rows(ds, spectrogram, f0_length, w);
    g_ws.finish();
    tr.mark("back");
  });
}

void InitializeD4COption(D4COption* option) { option->threshold = 0.85; }   // d4c.cpp:399-401
void D4C(const double* x, int x_length, int fs, const double* temporal_positions, const double* f0,
         int f0_length, int fft_size, const D4COption* option, double** aperiodicity) {
  drop_in([&] {
    WorldMi355Params p;
    WorldMi355DefaultParams(fs, 5.0, &p);
    p.fft_size = fft_size;
    p.d4c_threshold = option->threshold;
    const int w = fft_size / 2 + 1;
    WorldMi355Batch* b = g_ws.batch(p, x_length, f0_length, -1);
    double* dx = put_x(x, (size_t)x_length);
    double* dt = put(kT, temporal_positions, (size_t)f0_length);
    double* df = put(kF0, f0, (size_t)f0_length);
    CallTrace tr("D4C");
    double* da = g_ws.device(kAp, (size_t)f0_length * w);
    run_or_die("D4C", WorldMi355D4C(b, dx, dt, df, da));
    tr.mark("launch");
    tr.mark("kernels", true);
    get_rows(da, aperiodicity, f0_length, w);
    g_ws.finish();
    tr.mark("back");
  });
}

// ---- world/codec.h --------------------------------------------------------------------------------
int GetNumberOfAperiodicities(int fs) { return codec_num_aperiodicities(fs); }   // codec.cpp:212-215

namespace {
// a frames-only batch: the codec needs fs, fft_size and the frame count
static WorldMi355Batch* codec_batch(int fs, int fft_size, int f0_length) {   // C linkage ignores the namespace
  WorldMi355Params p;
  WorldMi355DefaultParams(fs, 5.0, &p);
  p.fft_size = fft_size;
  return g_ws.batch(p, -1, f0_length, -1);
}
}  // namespace

void CodeSpectralEnvelope(const double* const* spectrogram, int f0_length, int fs, int fft_size,
                          int number_of_dimensions, double** coded_spectral_envelope) {
  drop_in([&] {
    const int w = fft_size / 2 + 1;
    WorldMi355Batch* b = codec_batch(fs, fft_size, f0_length);
    double* ds = put_rows(kSp, spectrogram, f0_length, w);
    double* dc = g_ws.device(kCoded, (size_t)f0_length * number_of_dimensions);
    run_or_die("CodeSpectralEnvelope", WorldMi355CodeSpectralEnvelope(b, ds, number_of_dimensions, dc));
    get_rows(dc, coded_spectral_envelope, f0_length, number_of_dimensions);
    g_ws.finish();
  });
}

void DecodeSpectralEnvelope(const double* const* coded_spectral_envelope, int f0_length, int fs, int fft_size,
                            int number_of_dimensions, double** spectrogram) {
  drop_in([&] {
    const int w = fft_size / 2 + 1;
    WorldMi355Batch* b = codec_batch(fs, fft_size, f0_length);
    double* dc = put_rows(kCoded, coded_spectral_envelope, f0_length, number_of_dimensions);
    double* ds = g_ws.device(kSp, (size_t)f0_length * w);
    run_or_die("DecodeSpectralEnvelope", WorldMi355DecodeSpectralEnvelope(b, dc, number_of_dimensions, ds));
    get_rows(ds, spectrogram, f0_length, w);
    g_ws.finish();
  });
}

void CodeAperiodicity(const double* const* aperiodicity, int f0_length, int fs, int fft_size,
                      int number_of_aperiodicities, double** coded_aperiodicity) {
  drop_in([&] {
    if (number_of_aperiodicities != codec_num_aperiodicities(fs))
      die("CodeAperiodicity: number_of_aperiodicities must be GetNumberOfAperiodicities(fs)", WM_ERR_BAD_ARG);
    const int w = fft_size / 2 + 1;
    WorldMi355Batch* b = codec_batch(fs, fft_size, f0_length);
    double* da = put_rows(kAp, aperiodicity, f0_length, w);
    double* dc = g_ws.device(kCoded, (size_t)f0_length * number_of_aperiodicities);
    run_or_die("CodeAperiodicity", WorldMi355CodeAperiodicity(b, da, dc));
    get_rows(dc, coded_aperiodicity, f0_length, number_of_aperiodicities);
    g_ws.finish();
  });
}

// Positional meaning of the reference's DEFINITION (codec.cpp:237-238): the 4th argument is the number
// of aperiodicities and the 5th the FFT size, whatever the header calls them.
void DecodeAperiodicity(const double* const* coded_aperiodicity, int f0_length, int fs, int arg4_number_of_aperiodicities,
                        int arg5_fft_size, double** aperiodicity) {
  drop_in([&] {
    const int nap = arg4_number_of_aperiodicities, fft_size = arg5_fft_size;
    if (nap != codec_num_aperiodicities(fs))
      die("DecodeAperiodicity: 4th argument must be GetNumberOfAperiodicities(fs) (codec.cpp:237-238)", WM_ERR_BAD_ARG);
    const int w = fft_size / 2 + 1;
    WorldMi355Batch* b = codec_batch(fs, fft_size, f0_length);
    double* dc = put_rows(kCoded, coded_aperiodicity, f0_length, nap);
    double* da = g_ws.device(kAp, (size_t)f0_length * w);
    run_or_die("DecodeAperiodicity", WorldMi355DecodeAperiodicity(b, dc, da));
    get_rows(da, aperiodicity, f0_length, w);
    g_ws.finish();
  });
}

void Synthesis(const double* f0, int f0_length, const double* const* spectrogram,
               const double* const* aperiodicity, int fft_size, double frame_period, int fs, int y_length,
               double* y) {
  drop_in([&] {
    WorldMi355Params p;
    WorldMi355DefaultParams(fs, frame_period, &p);
    p.fft_size = fft_size;
    const int w = fft_size / 2 + 1;
    CallTrace tr("Synthesis");
    WorldMi355Batch* b = g_ws.batch(p, -1, f0_length, y_length);
    tr.mark("batch");
    // f0 first, and the f0-only stage of Synthesis behind it (time base, pulse search: a latency chain as long as the
    // utterance); the rows of sp / ap are gathered into pinned memory and sent while that runs
    double* df = put(kF0, f0, (size_t)f0_length);
    double* dy = g_ws.device(kY, (size_t)y_length);
    {
      OnDevice dev_(b->b.ctx[0]);
      run_or_die("Synthesis", synthesis_begin(b->b, ws_stream(), df, dy));
    }
    tr.mark("begin");
    // (the device and pinned buffers are sized before anything of this call is in flight on the upload stream: growing
    // them synchronises the context's stream only)
    const size_t cells = (size_t)f0_length * w;
    (void)g_ws.device(kSp, cells);
    (void)g_ws.device(kAp, cells);
    (void)g_ws.stage(2 * cells + 16);
    g_ws.stage_at -= (2 * cells + 16 + 7) & ~(size_t)7;               // reserved, not taken
    const Upload& up = upload_stream();
    double* ds = put_rows(kSp, spectrogram, f0_length, w, up.stream);
    double* da = put_rows(kAp, aperiodicity, f0_length, w, up.stream);
    if (hipEventRecord(up.done, up.stream) != hipSuccess) die("upload", WM_ERR_HIP);
    tr.mark("stage");
    {
      OnDevice dev_(b->b.ctx[0]);
      run_or_die("Synthesis", synthesis_prepare_wait(b->b, ws_stream()));
      tr.mark("wait");
      if (hipStreamWaitEvent(ws_stream(), up.done, 0) != hipSuccess) die("upload", WM_ERR_HIP);
      run_or_die("Synthesis", synthesis_render(b->b, ws_stream(), ds, da, dy));
    }
    tr.mark("launch");
    tr.mark("kernels", true);
    get(dy, y, (size_t)y_length);
    g_ws.finish();
    tr.mark("back");
  });
}

}  // extern "C"
