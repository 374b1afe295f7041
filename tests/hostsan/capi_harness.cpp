// Drives the HOST layer of libworld_mi355 (csrc/capi.cpp, context.cpp and the host halves of the .hip units) under
// AddressSanitizer + UBSan against tests/hostsan/hip_stub.cpp, the way the reference's CLIs call it
// (test/analysis.cpp:93-203, test/synth.cpp:103-106): host pointers, `double**` rows allocated ONE BY ONE at their
// exact size (analysis.cpp:172-176) -- a scatter that is one element off lands in a red zone.  Kernels do not run in
// the stub, so nothing here checks arithmetic; what is checked is that every call returns, outputs are written and
// finite, the error-handler path unwinds cleanly, and the sanitizers stay silent.
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "world/cheaptrick.h"
#include "world/codec.h"
#include "world/d4c.h"
#include "world/dio.h"
#include "world/harvest.h"
#include "world/stonemask.h"
#include "world/synthesis.h"
#include "world_mi355.h"

extern "C" long HipStubMallocs();
extern "C" long HipStubLaunches();
extern "C" long HipStubCreations();
extern "C" long HipStubDevPtrs();
extern "C" void HipStubNextPulses(long index);
extern "C" void HipStubFailMallocAfter(long n);
namespace wm { void dev_cache_trim(size_t keep_bytes); }     // the library's block cache (csrc/batch.hpp)
extern "C" void HipStubTraceMark(const char* text);
extern "C" void HipStubTraceStream(const char* label, void* stream);

static int g_handler_calls = 0;
static void on_error(const char* where, int code, const char* message, void* user) {
  ++g_handler_calls;
  *(int*)user = code;
  fprintf(stderr, "handler: %s code %d: %s\n", where, code, message ? message : "");
}

struct Rows {                         // T rows of `width` doubles, each its own allocation, poisoned with NaN
  std::vector<double*> p;
  int width;
  Rows(int T, int w) : p((size_t)T), width(w) {
    for (auto& r : p) {
      r = new double[(size_t)w];
      for (int j = 0; j < w; ++j) r[j] = NAN;
    }
  }
  ~Rows() { for (auto r : p) delete[] r; }
  bool all_finite() const {
    for (auto r : p)
      for (int j = 0; j < width; ++j)
        if (!isfinite(r[j])) return false;
    return true;
  }
};

static int one_utterance(int fs, double seconds, double frame_period, int fft_override, bool harvest) {
  const int n = (int)(fs * seconds);
  std::vector<double> x((size_t)n);
  for (int i = 0; i < n; ++i) x[(size_t)i] = 0.3 * sin(2.0 * M_PI * 140.0 * i / fs) + 1e-3 * ((i * 2654435761u >> 16) % 1000 - 500) / 500.0;
  DioOption dopt;
  InitializeDioOption(&dopt);
  dopt.frame_period = frame_period;
  dopt.speed = 1;
  dopt.f0_floor = 71.0;
  dopt.allowed_range = 0.1;
  const int T = GetSamplesForDIO(fs, n, frame_period);
  std::vector<double> t((size_t)T, NAN), f0((size_t)T, NAN), rf0((size_t)T, NAN);
  if (harvest) {
    HarvestOption hopt;
    InitializeHarvestOption(&hopt);
    hopt.frame_period = frame_period;
    if (GetSamplesForHarvest(fs, n, frame_period) != T) return 10;
    Harvest(x.data(), n, fs, &hopt, t.data(), f0.data());
  } else {
    Dio(x.data(), n, fs, &dopt, t.data(), f0.data());
  }
  // kernels do not run: give the later stages a plausible contour (time axis and f0 as the analysis would)
  for (int i = 0; i < T; ++i) { t[(size_t)i] = i * frame_period / 1000.0; f0[(size_t)i] = (i % 7 == 0) ? 0.0 : 100.0 + (i % 50); }
  StoneMask(x.data(), n, fs, t.data(), f0.data(), T, rf0.data());
  CheapTrickOption copt;
  InitializeCheapTrickOption(fs, &copt);
  if (fft_override) copt.fft_size = fft_override;
  const int F = copt.fft_size, bins = F / 2 + 1;
  if (fft_override == 0 && F != GetFFTSizeForCheapTrick(fs, &copt)) return 11;
  Rows sp(T, bins), ap(T, bins);
  CheapTrick(x.data(), n, fs, t.data(), f0.data(), T, &copt, sp.p.data());
  D4COption aopt;
  InitializeD4COption(&aopt);
  aopt.threshold = 0.0;
  D4C(x.data(), n, fs, t.data(), f0.data(), T, F, &aopt, ap.p.data());
  if (!sp.all_finite() || !ap.all_finite()) return 12;      // every row written, none past its end (ASan)
  const int ylen = (int)((T - 1) * frame_period / 1000.0 * fs) + 1;
  std::vector<double> y((size_t)ylen, NAN);
  Synthesis(f0.data(), T, sp.p.data(), ap.p.data(), F, frame_period, fs, ylen, y.data());
  for (double v : y)
    if (!isfinite(v)) return 13;
  // the codec entry points the CLIs link (codec.h)
  const int nd = 50 < F / 4 ? 50 : F / 4, na = GetNumberOfAperiodicities(fs);
  Rows mgc(T, nd), sp2(T, bins);
  CodeSpectralEnvelope(sp.p.data(), T, fs, F, nd, mgc.p.data());
  DecodeSpectralEnvelope(mgc.p.data(), T, fs, F, nd, sp2.p.data());
  if (!mgc.all_finite() || !sp2.all_finite()) return 14;
  if (na > 0) {
    Rows bap(T, na), ap2(T, bins);
    CodeAperiodicity(ap.p.data(), T, fs, F, na, bap.p.data());
    DecodeAperiodicity(bap.p.data(), T, fs, na, F, ap2.p.data());   // the reference DEFINITION's order (codec.cpp:237-238)
    if (!bap.all_finite() || !ap2.all_finite()) return 15;
  }
  return 0;
}

// `capi_harness batched`: the multi-stream paths of the batched API on one context, for the stub's call trace
// (HIP_STUB_TRACE) and its injected creation failures.  Every step is marked in the trace; a step that fails is made
// once more and must then succeed (a failed set-up leaves nothing behind).  "Device" buffers are host vectors; sp / ap
// of the large batch are never read by the host layer and get no backing.  HIP_STUB_PULSES gives Synthesis pulses to
// render: `pulses` is the entry that a step's first launch of the counting kernel reports (a repeated step reports the same).
static int g_steps_failed = 0;
template <class Call> static bool step(const char* name, int pulses, Call call) {
  for (int attempt = 1; attempt <= 2; ++attempt) {
    HipStubNextPulses(pulses);
    char mark[96];
    snprintf(mark, sizeof(mark), "step %s attempt %d", name, attempt);
    HipStubTraceMark(mark);
    const int rc = call();
    printf("%s: rc %d\n", mark, rc);
    if (rc == 0) return true;
    ++g_steps_failed;
  }
  return false;
}
static int batched_sequence() {
  int last_code = 0;
  WorldMi355SetErrorHandler(on_error, &last_code);
  const int fs = 16000, F = 1024, bins = F / 2 + 1;
  WorldMi355Params p;
  WorldMi355DefaultParams(fs, 5.0, &p);
  WorldMi355Context* ctx = nullptr;
  if (WorldMi355CreateContext(-1, nullptr, &ctx) != 0 || !ctx) return 20;
  // the large batch: the split form of Synthesis wants 16 utterances and 4 Mi output samples (launch_synthesis)
  const int lens[3] = {9000, 16000, 4321}, small_f[2] = {200, 300};
  int big_f[16], big_y[16];
  int64_t big_tf = 0, big_ty = 0;
  for (int u = 0; u < 16; ++u) {
    big_y[u] = (1 << 18) + 4000 * ((u * 7) % 16);                         // not in order of length
    big_f[u] = (big_y[u] - 1) / 80 + 1;
    big_tf += big_f[u];
    big_ty += big_y[u];
  }
  if (big_ty < ((int64_t)4 << 20)) return 21;
  for (int round = 0; round < 2; ++round) {
    if (round == 1 && WorldMi355TimingEnable(ctx, 1) != 0) return 22;    // the streams TimedScope records on
    // the drop-in Synthesis(): its own context, its upload stream
    {
      const int T = 120, ylen = (T - 1) * 80 + 1;
      std::vector<double> f0((size_t)T, 120.0), y((size_t)ylen, NAN);
      Rows sp(T, bins), ap(T, bins);
      for (auto r : sp.p) for (int j = 0; j < bins; ++j) r[j] = 1.0;
      for (auto r : ap.p) for (int j = 0; j < bins; ++j) r[j] = 0.5;
      if (!step("drop-in Synthesis", 0, [&] {
            const int before = g_handler_calls;
            Synthesis(f0.data(), T, sp.p.data(), ap.p.data(), F, 5.0, fs, ylen, y.data());
            return g_handler_calls == before ? 0 : last_code;
          })) return 23;
    }
    WorldMi355Batch *b = nullptr, *bs = nullptr, *bb = nullptr;
    if (WorldMi355CreateBatch(ctx, &p, 3, lens, nullptr, nullptr, &b) != 0) return 24;
    if (WorldMi355CreateBatch(ctx, &p, 2, nullptr, small_f, nullptr, &bs) != 0) return 25;
    if (WorldMi355CreateBatch(ctx, &p, 16, nullptr, big_f, big_y, &bb) != 0) return 26;
    if (WorldMi355BatchFftSize(b) != F || WorldMi355BatchTotalOutputSamples(bb) != big_ty) return 27;
    const size_t tf = (size_t)WorldMi355BatchTotalFrames(b), tfs = (size_t)WorldMi355BatchTotalFrames(bs);
    std::vector<double> x((size_t)WorldMi355BatchTotalSamples(b), 0.1), t(tf), f0(tf), sp(tf * bins), ap(tf * bins);
    std::vector<double> y((size_t)WorldMi355BatchTotalOutputSamples(b));
    std::vector<double> f0s(tfs, 150.0), sps(tfs * bins, 1.0), aps(tfs * bins, 0.5);
    std::vector<double> ys((size_t)WorldMi355BatchTotalOutputSamples(bs)), f0b((size_t)big_tf, 110.0), yb((size_t)big_ty);
    const double* no_backing = f0b.data();                                  // sp / ap of the large batch: never read
    bool ok = step("Analyze 1", 0, [&] { return WorldMi355Analyze(b, x.data(), t.data(), f0.data(), sp.data(), ap.data()); });
    ok = ok && step("Analyze 2 (D4C's preparation beside CheapTrick)", 0,
                    [&] { return WorldMi355Analyze(b, x.data(), t.data(), f0.data(), sp.data(), ap.data()); });
    ok = ok && step("AnalyzeSynthesize 1", 1, [&] {
           return WorldMi355AnalyzeSynthesize(b, x.data(), t.data(), f0.data(), sp.data(), ap.data(), y.data());
         });
    ok = ok && step("AnalyzeSynthesize 2 (warm, overlapped)", 2, [&] {
           return WorldMi355AnalyzeSynthesize(b, x.data(), t.data(), f0.data(), sp.data(), ap.data(), y.data());
         });
    ok = ok && step("Synthesis in one part", 3, [&] { return WorldMi355Synthesis(bs, f0s.data(), sps.data(), aps.data(), ys.data()); });
    ok = ok && step("Synthesis in two parts", 4, [&] { return WorldMi355Synthesis(bb, f0b.data(), no_backing, no_backing, yb.data()); });
    HipStubTraceMark("end of round");
    if (!ok || WorldMi355Synchronize(ctx) != 0) return 28;
    WorldMi355DestroyBatch(b);
    WorldMi355DestroyBatch(bs);
    WorldMi355DestroyBatch(bb);
  }
  double ms = 0.0;
  int launches = 0;
  if (WorldMi355TimingQuery(ctx, "synth_ola_kernel", &ms, &launches) != 0 || launches == 0) return 29;
  WorldMi355DestroyContext(ctx);
  WorldMi355SetErrorHandler(nullptr, nullptr);
  printf("capi batched ok: %d failed steps, %ld creations, %ld device pointers, %ld launches\n", g_steps_failed,
         HipStubCreations(), HipStubDevPtrs(), HipStubLaunches());
  return 0;
}

// `capi_harness streams`: every entry point that queues device work, at tiny sizes, on a context whose stream is NOT the
// legacy default stream, for the rules of tests/stream_rules.py (checked in tests/test_sanitizers.py): nothing may be
// queued on stream 0, and a stream of the library's own is forked from the caller's and joined back into it within
// the call.  The trace starts with the
// names of the NULL stream and of the two caller streams ("# stream U s1"); "# caller U" says which one the context is
// on from there.  The last steps re-point the context (WorldMi355SetStream) and call once more.
template <class T> static T* dev(std::vector<std::vector<unsigned char>>& pool, size_t n, T fill) {
  pool.emplace_back((n ? n : 1) * sizeof(T));
  T* p = (T*)pool.back().data();
  for (size_t i = 0; i < n; ++i) p[i] = fill;
  return p;
}
static int stream_sequence() {
  int last_code = 0;
  WorldMi355SetErrorHandler(on_error, &last_code);
  hipStream_t U = nullptr, V = nullptr;
  if (hipStreamCreateWithFlags(&U, hipStreamNonBlocking) != hipSuccess || !U) return 40;
  if (hipStreamCreateWithFlags(&V, hipStreamNonBlocking) != hipSuccess || !V) return 40;
  HipStubTraceStream("null", nullptr);
  HipStubTraceStream("U", U);
  HipStubTraceStream("V", V);
  const int fs = 16000, F = 1024, bins = F / 2 + 1;
  WorldMi355Params p;
  WorldMi355DefaultParams(fs, 5.0, &p);
  WorldMi355Context* ctx = nullptr;
  if (WorldMi355CreateContext(-1, U, &ctx) != 0 || !ctx) return 41;
  HipStubTraceMark("caller U");
  std::vector<std::vector<unsigned char>> pool;
  const int lens[2] = {4800, 8000}, frames[3] = {5, 64, 33};
  int big_f[16], big_y[16];
  int64_t big_tf = 0, big_ty = 0;
  for (int u = 0; u < 16; ++u) {                                          // the split Synthesis, as in `batched`
    big_y[u] = (1 << 18) + 4000 * ((u * 7) % 16);
    big_f[u] = (big_y[u] - 1) / 80 + 1;
    big_tf += big_f[u];
    big_ty += big_y[u];
  }
  WorldMi355Batch *b = nullptr, *bf = nullptr, *bb = nullptr;
  if (WorldMi355CreateBatch(ctx, &p, 2, lens, nullptr, nullptr, &b) != 0) return 42;
  if (WorldMi355CreateBatch(ctx, &p, 3, nullptr, frames, nullptr, &bf) != 0) return 43;
  if (WorldMi355CreateBatch(ctx, &p, 16, nullptr, big_f, big_y, &bb) != 0) return 44;
  bool ok = true;
  for (int round = 0; round < 2 && ok; ++round) {                         // the second time with TimedScope's records
    if (round == 1 && WorldMi355TimingEnable(ctx, 1) != 0) return 47;
    {  // ---- WORLD and its codec on the analysis batch
      const size_t tx = (size_t)WorldMi355BatchTotalSamples(b), tf = (size_t)WorldMi355BatchTotalFrames(b);
      const size_t ty = (size_t)WorldMi355BatchTotalOutputSamples(b);
      const int nd = 20, na = WorldMi355GetNumberOfAperiodicities(fs), apd = 5;
      double *x = dev(pool, tx, 0.1), *t = dev(pool, tf, 0.0), *f0 = dev(pool, tf, 120.0), *rf0 = dev(pool, tf, 120.0);
      double *sp = dev(pool, tf * bins, 1.0), *ap = dev(pool, tf * bins, 0.5), *y = dev(pool, ty, 0.0);
      double *csp = dev(pool, tf * nd, 0.0), *cap = dev(pool, tf * (size_t)(na > 0 ? na : 1), 0.0);
      int16_t *pcm_in = dev(pool, tx, (int16_t)100), *pcm_out = dev(pool, ty, (int16_t)0);
      float *lf0 = dev(pool, tf, 4.8f), *mgc = dev(pool, tf * nd, 0.0f), *bap = dev(pool, tf * apd, 0.0f);
      int* ust = dev(pool, 2, 0);
      ok = ok && step("SamplesFromPcm16", 0, [&] { return WorldMi355SamplesFromPcm16(b, pcm_in, x); });
      ok = ok && step("Dio", 0, [&] { return WorldMi355Dio(b, x, t, f0); });
      ok = ok && step("Harvest", 0, [&] { return WorldMi355Harvest(b, x, t, f0); });
      for (size_t i = 0; i < tf; ++i) { t[i] = i * 0.005; f0[i] = (i % 7 == 0) ? 0.0 : 100.0 + (double)(i % 50); }
      ok = ok && step("StoneMask", 0, [&] { return WorldMi355StoneMask(b, x, t, f0, rf0); });
      ok = ok && step("CheapTrick", 0, [&] { return WorldMi355CheapTrick(b, x, t, f0, sp); });
      ok = ok && step("D4C", 0, [&] { return WorldMi355D4C(b, x, t, f0, ap); });
      ok = ok && step("Analyze (forked)", 0, [&] { return WorldMi355Analyze(b, x, t, f0, sp, ap); });
      ok = ok && step("AnalyzeSynthesize 1", 1, [&] { return WorldMi355AnalyzeSynthesize(b, x, t, f0, sp, ap, y); });
      ok = ok && step("AnalyzeSynthesize 2 (overlapped)", 2, [&] { return WorldMi355AnalyzeSynthesize(b, x, t, f0, sp, ap, y); });
      ok = ok && step("Synthesis in one part", 3, [&] { return WorldMi355Synthesis(b, f0, sp, ap, y); });
      ok = ok && step("SamplesToPcm16", 0, [&] { return WorldMi355SamplesToPcm16(b, y, pcm_out); });
      ok = ok && step("UtteranceStatus", 0, [&] { return WorldMi355UtteranceStatus(b, x, f0, sp, ap, ust); });
      ok = ok && step("CodeSpectralEnvelope", 0, [&] { return WorldMi355CodeSpectralEnvelope(b, sp, nd, csp); });
      ok = ok && step("DecodeSpectralEnvelope", 0, [&] { return WorldMi355DecodeSpectralEnvelope(b, csp, nd, sp); });
      ok = ok && step("CodeAperiodicity", 0, [&] { return WorldMi355CodeAperiodicity(b, ap, cap); });
      ok = ok && step("DecodeAperiodicity", 0, [&] { return WorldMi355DecodeAperiodicity(b, cap, ap); });
      ok = ok && step("RecipeFeatures", 0, [&] { return WorldMi355RecipeFeatures(b, f0, sp, ap, nd, apd, lf0, mgc, bap); });
      ok = ok && step("RecipeDecode", 0, [&] { return WorldMi355RecipeDecode(b, lf0, mgc, bap, nd, apd, f0, sp, ap); });
    }
    {  // ---- Synthesis in two parts: sp / ap of the large batch are never read by the host layer
      double *f0b = dev(pool, (size_t)big_tf, 110.0), *yb = dev(pool, (size_t)big_ty, 0.0);
      ok = ok && step("Synthesis in two parts", 4, [&] { return WorldMi355Synthesis(bb, f0b, f0b, f0b, yb); });
    }
    {  // ---- the recipe's stages on the frame batch (5, 64 and 33 frames)
      const size_t tf = (size_t)WorldMi355BatchTotalFrames(bf);
      const int nu = 3, dim = 2, nw = 3, row = dim * nw, order = 8, K = 33;
      std::vector<double> w0{1.0}, w1{-0.5, 0.0, 0.5}, w2{1.0, -2.0, 1.0};
      const double* wins[3] = {w0.data(), w1.data(), w2.data()};
      const int sizes3[3] = {1, 3, 3};
      const double* const* windows[1] = {wins};
      const int* sizes[1] = {sizes3};
      const int dims[1] = {dim}, nwin[1] = {nw};
      float *st32 = dev(pool, tf * dim, 0.5f), *cmp = dev(pool, tf * row, 0.5f), *ffo = dev(pool, tf * (row + 1), 0.5f);
      float *msd = dev(pool, tf, 1.0f), *gap = dev(pool, tf * dim, 0.5f), *voiced = dev(pool, tf, 0.0f);
      int *ust = dev(pool, nu, 0), *fst = dev(pool, tf, 0);
      const float* streams[1] = {st32};
      const float* msds[1] = {msd};
      ok = ok && step("ComposeCmp", 0, [&] { return WorldMi355ComposeCmp(bf, 1, streams, dims, nwin, windows, sizes, cmp); });
      ok = ok && step("ComposeFfo", 0, [&] { return WorldMi355ComposeFfo(bf, 1, streams, dims, nwin, windows, sizes, msds, ffo); });
      ok = ok && step("InterpolateGaps", 0, [&] { return WorldMi355InterpolateGaps(bf, st32, dim, -1e10, gap, voiced, ust); });
      int64_t* cnt = dev(pool, (size_t)nu * dim, (int64_t)0);
      double *mom1 = dev(pool, (size_t)nu * dim, 0.0), *mom2 = dev(pool, (size_t)nu * dim, 0.0);
      const double ignore = -1e10;
      ok = ok && step("ColumnMoments", 0, [&] { return WorldMi355ColumnMoments(bf, st32, dim, dim, &ignore, cnt, mom1, mom2); });
      double *x64 = dev(pool, tf * dim, 0.25), *o64 = dev(pool, tf * dim, 0.0), *um = dev(pool, (size_t)nu * dim, 0.0);
      ok = ok && step("ColumnMeans", 0, [&] { return WorldMi355ColumnMeans(bf, x64, dim, um); });
      double *spec = dev(pool, tf * bins, 1.0), *mc = dev(pool, tf * (order + 1), 0.1), *mc2 = dev(pool, tf * (order + 1), 0.0);
      double* gain = dev(pool, tf, 0.0);
      WorldMi355McepOption mo;
      WorldMi355DefaultMcepOption(&mo);
      mo.order = order;
      ok = ok && step("MelCepstrum", 0, [&] { return WorldMi355MelCepstrum(bf, spec, &mo, mc, fst); });
      WorldMi355Mgc2spOption go;
      WorldMi355DefaultMgc2spOption(&go);
      go.order = order;
      ok = ok && step("MelCepstrumToSpectrum", 0, [&] { return WorldMi355MelCepstrumToSpectrum(bf, mc, &go, spec, nullptr, fst); });
      WorldMi355McpfOption po;
      WorldMi355DefaultMcpfOption(&po);
      po.order = order;
      ok = ok && step("MelCepstrumPostfilter", 0, [&] { return WorldMi355MelCepstrumPostfilter(bf, mc, &po, mc2, gain, fst); });
      WorldMi355MspfOption so;
      WorldMi355DefaultMspfOption(&so);
      std::vector<double> tab_mean((size_t)dim * K, 0.0), tab_std((size_t)dim * K, 1.0);
      double *s1 = dev(pool, (size_t)dim * K, 0.0), *s2 = dev(pool, (size_t)dim * K, 0.0);
      int64_t n_frames = 0;
      ok = ok && step("ModulationSpectrumStats", 0,
                      [&] { return WorldMi355ModulationSpectrumStats(bf, x64, dim, &so, nullptr, s1, s2, &n_frames); });
      ok = ok && step("ModulationSpectrumPostfilter", 0, [&] {
             return WorldMi355ModulationSpectrumPostfilter(bf, x64, dim, &so, tab_mean.data(), tab_std.data(), tab_mean.data(),
                                                           tab_std.data(), o64, ust);
           });
      // parameter generation and the trajectory cost over compose_cmp's layout
      float *var = dev(pool, (size_t)row, 1.0f), *gv = dev(pool, (size_t)dim, 1.0f), *traj = dev(pool, tf * dim, 0.0f);
      float* gpred = dev(pool, tf * row, 0.0f);
      double *cost3 = dev(pool, (size_t)nu * 3, 0.0), *gvar = dev(pool, (size_t)nu * row, 0.0);
      const float *means[1] = {cmp}, *vars[1] = {var}, *gvs[1] = {gv};
      float *outs[1] = {traj}, *gpreds[1] = {gpred};
      WorldMi355MlpgOption lo;
      WorldMi355DefaultMlpgOption(&lo);
      ok = ok && step("ParameterGeneration", 0, [&] {
             return WorldMi355ParameterGeneration(bf, 1, means, row, vars, 0, dims, nwin, windows, sizes, nullptr, &lo, outs, ust);
           });
      // the same rows through a 15-tap window: a wider band, the workspace is replaced while the context may have work queued
      std::vector<double> w15(15, 0.0);
      for (int i = 0; i < 15; ++i) w15[(size_t)i] = (i - 7) / 28.0;
      const double* wins15[3] = {w0.data(), w15.data(), w2.data()};
      const int sizes15[3] = {1, 15, 3};
      const double* const* windows15[1] = {wins15};
      const int* sizes_15[1] = {sizes15};
      ok = ok && step("ParameterGeneration with 15 taps", 0, [&] {
             return WorldMi355ParameterGeneration(bf, 1, means, row, vars, 0, dims, nwin, windows15, sizes_15, nullptr, &lo, outs, ust);
           });
      WorldMi355TrajectoryOption to;
      WorldMi355DefaultTrajectoryOption(&to);
      ok = ok && step("TrajectoryCost", 0, [&] {
             return WorldMi355TrajectoryCost(bf, 1, means, means, row, vars, gvs, dims, nwin, windows, sizes, nullptr, nullptr,
                                             nullptr, &to, cost3, outs, gpreds, nullptr, row, gvar, ust);
           });
      // the acoustic model: 3 inputs, one hidden layer of 4 units, 2 outputs
      const int n_in = 3, n_hid = 4, n_out = 2, units[1] = {n_hid};
      float *W0 = dev(pool, (size_t)n_in * n_hid, 0.1f), *W1 = dev(pool, (size_t)n_hid * n_out, 0.1f);
      float *B0 = dev(pool, (size_t)n_hid, 0.0f), *B1 = dev(pool, (size_t)n_out, 0.0f), *mvar = dev(pool, (size_t)n_out, 1.0f);
      const float *weights[2] = {W0, W1}, *biases[2] = {B0, B1};
      WorldMi355AcousticModel am;
      memset(&am, 0, sizeof(am));
      am.n_layers = 1; am.n_inputs = n_in; am.n_outputs = n_out; am.n_spkrs = 1;
      am.hidden_activation = 2; am.output_activation = 0;
      am.units = units; am.weights = weights; am.biases = biases; am.variances = mvar;
      float *ax = dev(pool, tf * n_in, 0.5f), *aout = dev(pool, tf * n_out, 0.0f), *aobs = dev(pool, tf * n_out, 0.25f);
      float* gout = dev(pool, tf * n_out, 0.0f);
      double *acost = dev(pool, (size_t)nu, 0.0), *agvar = dev(pool, (size_t)nu * n_out, 0.0);
      ok = ok && step("AcousticModelForward", 0, [&] {
             return WorldMi355AcousticModelForward(bf, &am, ax, n_in, nullptr, aout, n_out, aobs, n_out, acost, ust);
           });
      WorldMi355Dropout drop = {0.8f, 1u, 0u};
      ok = ok && step("AcousticModelTrainForward", 0, [&] {
             return WorldMi355AcousticModelTrainForward(bf, &am, &drop, ax, n_in, nullptr, aout, n_out, aobs, n_out, acost, gout,
                                                        n_out, agvar, ust);
           });
      float *gW0 = dev(pool, (size_t)n_in * n_hid, 0.0f), *gW1 = dev(pool, (size_t)n_hid * n_out, 0.0f);
      float *gB0 = dev(pool, (size_t)n_hid, 0.0f), *gB1 = dev(pool, (size_t)n_out, 0.0f);
      float *gws[2] = {gW0, gW1}, *gbs[2] = {gB0, gB1};
      ok = ok && step("AcousticModelBackward", 0, [&] {
             return WorldMi355AcousticModelBackward(bf, &am, &drop, ax, n_in, nullptr, gout, n_out, gws, gbs, nullptr, ust);
           });
      WorldMi355OptimizerOption oo;
      WorldMi355DefaultOptimizerOption(4, &oo);
      float *m0 = dev(pool, (size_t)n_in * n_hid, 0.0f), *m1 = dev(pool, (size_t)n_hid * n_out, 0.0f);
      float *v0 = dev(pool, (size_t)n_in * n_hid, 0.0f), *v1 = dev(pool, (size_t)n_hid * n_out, 0.0f);
      float *params[2] = {W0, W1}, *slot0[2] = {m0, m1}, *slot1[2] = {v0, v1};
      const float* grads[2] = {gW0, gW1};
      const int64_t counts[2] = {n_in * n_hid, n_hid * n_out};
      const float rates[2] = {0.1f, 0.2f};
      int* ost = dev(pool, 2, 0);
      ok = ok && step("OptimizerStep", 0,
                      [&] { return WorldMi355OptimizerStep(ctx, &oo, 2, params, grads, slot0, slot1, counts, rates, ost); });
      // label features: two binary questions, a float one, a reserved one; four lines over the three utterances
      const WorldMi355LabelFeature feats[4] = {{0, "*-a+*", 0, 0}, {0, "*-b+*,*-c+*", 0, 0}, {1, "*/A:%d_*", 0, 10}, {6, nullptr, 0, 70}};
      WorldMi355LabelFeatureSet* set = nullptr;
      if (ok && WorldMi355CreateLabelFeatureSet(ctx, 4, feats, &set) != 0) return 45;
      const int line_off[4] = {0, 1, 3, 4}, lstart[4] = {0, 0, 30, 0}, lend[4] = {5, 30, 64, 33}, lstate[4] = {0, 0, 0, 0};
      const int level[3] = {0, 0, 0};
      const char* names_a[4] = {"x^x-a+b=c/A:3_1", "x^a-b+c=x/A:12_2", "a^b-c+x=x/A:0_3", "x^x-a+b=c/A:3_1"};
      const char* names_b[4] = {"x^x-c+b=a/A:7_1", "x^a-a+c=x/A:-2_2", "a^b-b+x=x/A:9_3", "x^x-c+b=a/A:7_1"};
      float* ffi = dev(pool, tf * 4, 0.0f);
      ok = ok && step("LabelFeatures", 0, [&] {
             return WorldMi355LabelFeatures(bf, set, line_off, lstart, lend, lstate, names_a, level, ffi, 4, ust);
           });
      ok = ok && step("LabelFeatures again (other names)", 0, [&] {
             return WorldMi355LabelFeatures(bf, set, line_off, lstart, lend, lstate, names_b, level, ffi, 4, ust);
           });
      WorldMi355DestroyLabelFeatureSet(set);
      float *vlf0 = dev(pool, tf, 5.0f), *vib = dev(pool, tf * 2, 0.0f), *vout = dev(pool, tf * 2, 0.0f);
      const int seg_off[4] = {0, 1, 2, 3}, seg_start[3] = {0, 0, 0}, seg_end[3] = {5, 64, 33};
      const double seg_pitch[3] = {220.0, 0.0, 180.0};
      int too_long = 0;
      ok = ok && step("Vibrato", 0,
                      [&] { return WorldMi355Vibrato(bf, vlf0, seg_off, seg_start, seg_end, seg_pitch, vib, vout, &too_long); });
    }
  }
  // ---- the context moves to V: everything from here on is V's, the side streams included
  ok = ok && step("SetStream", 0, [&] { return WorldMi355SetStream(ctx, V); });
  HipStubTraceMark("caller V");
  {
    const size_t tx = (size_t)WorldMi355BatchTotalSamples(b), tf = (size_t)WorldMi355BatchTotalFrames(b);
    double *x = dev(pool, tx, 0.1), *t = dev(pool, tf, 0.0), *f0 = dev(pool, tf, 120.0);
    double *sp = dev(pool, tf * bins, 1.0), *ap = dev(pool, tf * bins, 0.5), *y = dev(pool, (size_t)WorldMi355BatchTotalOutputSamples(b), 0.0);
    ok = ok && step("AnalyzeSynthesize after SetStream", 2, [&] { return WorldMi355AnalyzeSynthesize(b, x, t, f0, sp, ap, y); });
  }
  HipStubTraceMark("step teardown attempt 1");
  if (!ok || g_steps_failed || WorldMi355Synchronize(ctx) != 0) return 46;
  WorldMi355DestroyBatch(b);
  WorldMi355DestroyBatch(bf);
  WorldMi355DestroyBatch(bb);
  WorldMi355DestroyContext(ctx);
  (void)hipStreamDestroy(U);
  (void)hipStreamDestroy(V);
  WorldMi355SetErrorHandler(nullptr, nullptr);
  printf("capi streams ok: %ld launches\n", HipStubLaunches());
  return 0;
}

// `capi_harness grow`: the six stages that replace their batch workspace when a call needs a larger one (parameter
// generation, the trajectory cost, the acoustic model's forward and training passes, the modulation-spectrum postfilter,
// label features), each on a batch of its own, on a context whose stream is not the default one: a small call; a larger
// one whose device allocations fail (the block cache is emptied first, so the request reaches the stub's hipMalloc, which
// refuses from there on: HIP_STUB_FAIL_MALLOC_AFTER set mid-run) and which must return WM_ERR_HIP; the same call again,
// which must succeed; the small call again.  The larger sizes are at least four times the smaller, i.e. another size
// class of the cache.  No per-utterance status array is passed: a stage clears the caller's before it looks at its
// workspace, and the trace is read for "the wait comes before the call's first work" (tests/test_sanitizers.py).
template <class Small, class Large> static bool grow_case(const char* stage, Small small, Large large) {
  auto run = [&](const char* what, int want, auto& call) {
    char mark[96];
    snprintf(mark, sizeof(mark), "step %s: %s", stage, what);
    HipStubTraceMark(mark);
    const int rc = call();
    printf("%s: rc %d\n", mark, rc);
    return rc == want;
  };
  if (!run("small", WM_OK, small)) return false;
  wm::dev_cache_trim(0);
  HipStubFailMallocAfter(HipStubMallocs());
  const bool refused = run("larger, allocation fails", WM_ERR_HIP, large);
  HipStubFailMallocAfter(-1);
  return refused && run("larger again", WM_OK, large) && run("small again", WM_OK, small);
}
static int grow_sequence() {
  hipStream_t U = nullptr;
  if (hipStreamCreateWithFlags(&U, hipStreamNonBlocking) != hipSuccess || !U) return 60;
  HipStubTraceStream("null", nullptr);
  HipStubTraceStream("U", U);
  WorldMi355Params p;
  WorldMi355DefaultParams(16000, 5.0, &p);
  WorldMi355Context* ctx = nullptr;
  if (WorldMi355CreateContext(-1, U, &ctx) != 0 || !ctx) return 61;
  HipStubTraceMark("caller U");
  std::vector<std::vector<unsigned char>> pool;
  const int frames[3] = {5, 64, 33}, nu = 3, tf = 5 + 64 + 33;
  WorldMi355Batch* bs[6] = {};
  for (auto& b : bs)
    if (WorldMi355CreateBatch(ctx, &p, nu, nullptr, frames, nullptr, &b) != 0) return 62;
  // windows: static, delta, delta-delta; the delta window with 15 taps for the wider band
  std::vector<double> w0{1.0}, w1{-0.5, 0.0, 0.5}, w2{1.0, -2.0, 1.0}, w15(15, 0.0);
  for (int i = 0; i < 15; ++i) w15[(size_t)i] = (i - 7) / 28.0;
  const double *wins[3] = {w0.data(), w1.data(), w2.data()}, *wins15[3] = {w0.data(), w15.data(), w2.data()};
  const int sizes3[3] = {1, 3, 3}, sizes15[3] = {1, 15, 3};
  const double* const* windows[1] = {wins};
  const double* const* windows15[1] = {wins15};
  const int *sizes[1] = {sizes3}, *sizes_15[1] = {sizes15};
  const int nwin[1] = {3}, dims2[1] = {2}, dims8[1] = {8};
  float* data = dev(pool, (size_t)tf * 24, 0.5f);                          // rows of up to 8 columns x 3 windows
  float *var = dev(pool, 24, 1.0f), *gv = dev(pool, 8, 1.0f), *traj = dev(pool, (size_t)tf * 8, 0.0f);
  float* gpred = dev(pool, (size_t)tf * 24, 0.0f);
  const float *means[1] = {data}, *vars[1] = {var}, *gvs[1] = {gv};
  float *outs[1] = {traj}, *gpreds[1] = {gpred};
  bool ok = true;
  {  // parameter generation: 3 taps, then 15 (the shapes of `streams`)
    WorldMi355MlpgOption lo;
    WorldMi355DefaultMlpgOption(&lo);
    ok = ok && grow_case("ParameterGeneration", [&] {
           return WorldMi355ParameterGeneration(bs[0], 1, means, 6, vars, 0, dims2, nwin, windows, sizes, nullptr, &lo, outs, nullptr);
         }, [&] {
           return WorldMi355ParameterGeneration(bs[0], 1, means, 6, vars, 0, dims2, nwin, windows15, sizes_15, nullptr, &lo, outs, nullptr);
         });
  }
  {  // the trajectory cost: 2 columns, then 8
    WorldMi355TrajectoryOption to;
    WorldMi355DefaultTrajectoryOption(&to);
    double *cost3 = dev(pool, (size_t)nu * 3, 0.0), *gvar = dev(pool, (size_t)nu * 24, 0.0);
    auto call = [&](const int* dims, int row) {
      return WorldMi355TrajectoryCost(bs[1], 1, means, means, row, vars, gvs, dims, nwin, windows, sizes, nullptr, nullptr, nullptr,
                                      &to, cost3, outs, gpreds, nullptr, row, gvar, nullptr);
    };
    ok = ok && grow_case("TrajectoryCost", [&] { return call(dims2, 6); }, [&] { return call(dims8, 24); });
  }
  {  // the acoustic model, forward and training forward: one hidden layer of 4 units, then of 64
    const int n_in = 3, n_out = 2, units4[1] = {4}, units64[1] = {64};
    float *W0 = dev(pool, (size_t)n_in * 64, 0.1f), *W1 = dev(pool, (size_t)64 * n_out, 0.1f);
    float *B0 = dev(pool, 64, 0.0f), *B1 = dev(pool, (size_t)n_out, 0.0f), *mvar = dev(pool, (size_t)n_out, 1.0f);
    const float *weights[2] = {W0, W1}, *biases[2] = {B0, B1};
    WorldMi355AcousticModel am;
    memset(&am, 0, sizeof(am));
    am.n_layers = 1; am.n_inputs = n_in; am.n_outputs = n_out; am.n_spkrs = 1;
    am.hidden_activation = 2; am.output_activation = 0;
    am.weights = weights; am.biases = biases; am.variances = mvar;
    float *ax = dev(pool, (size_t)tf * n_in, 0.5f), *aout = dev(pool, (size_t)tf * n_out, 0.0f), *aobs = dev(pool, (size_t)tf * n_out, 0.25f);
    float* gout = dev(pool, (size_t)tf * n_out, 0.0f);
    double *acost = dev(pool, (size_t)nu, 0.0), *agvar = dev(pool, (size_t)nu * n_out, 0.0);
    WorldMi355Dropout drop = {0.8f, 1u, 0u};
    auto forward = [&](const int* units) {
      am.units = units;
      return WorldMi355AcousticModelForward(bs[2], &am, ax, n_in, nullptr, aout, n_out, aobs, n_out, acost, nullptr);
    };
    auto train = [&](const int* units) {
      am.units = units;
      return WorldMi355AcousticModelTrainForward(bs[3], &am, &drop, ax, n_in, nullptr, aout, n_out, aobs, n_out, acost, gout, n_out,
                                                 agvar, nullptr);
    };
    ok = ok && grow_case("AcousticModelForward", [&] { return forward(units4); }, [&] { return forward(units64); });
    ok = ok && grow_case("AcousticModelTrainForward", [&] { return train(units4); }, [&] { return train(units64); });
  }
  {  // the modulation-spectrum postfilter: 2 columns, then 64
    WorldMi355MspfOption so;
    WorldMi355DefaultMspfOption(&so);
    const int K = 33;
    std::vector<double> tab_mean((size_t)64 * K, 0.0), tab_std((size_t)64 * K, 1.0);
    double *x64 = dev(pool, (size_t)tf * 64, 0.25), *o64 = dev(pool, (size_t)tf * 64, 0.0);
    auto call = [&](int dim) {
      return WorldMi355ModulationSpectrumPostfilter(bs[4], x64, dim, &so, tab_mean.data(), tab_std.data(), tab_mean.data(),
                                                    tab_std.data(), o64, nullptr);
    };
    ok = ok && grow_case("ModulationSpectrumPostfilter", [&] { return call(2); }, [&] { return call(64); });
  }
  {  // label features: four lines over the three utterances, then a line per frame
    const WorldMi355LabelFeature feats[4] = {{0, "*-a+*", 0, 0}, {0, "*-b+*,*-c+*", 0, 0}, {1, "*/A:%d_*", 0, 10}, {6, nullptr, 0, 70}};
    WorldMi355LabelFeatureSet* set = nullptr;
    if (WorldMi355CreateLabelFeatureSet(ctx, 4, feats, &set) != 0) return 63;
    const char* names[4] = {"x^x-a+b=c/A:3_1", "x^a-b+c=x/A:12_2", "a^b-c+x=x/A:0_3", "x^x-a+b=c/A:3_1"};
    const int line_off[4] = {0, 1, 3, 4}, lstart[4] = {0, 0, 30, 0}, lend[4] = {5, 30, 64, 33}, lstate[4] = {0, 0, 0, 0};
    const int level[3] = {0, 0, 0}, line_off_f[4] = {0, 5, 5 + 64, tf};
    std::vector<int> fstart((size_t)tf), fend((size_t)tf), fstate((size_t)tf, 0);
    std::vector<const char*> fnames((size_t)tf);
    for (int u = 0, i = 0; u < nu; ++u)
      for (int k = 0; k < frames[u]; ++k, ++i) { fstart[(size_t)i] = k; fend[(size_t)i] = k + 1; fnames[(size_t)i] = names[i % 3]; }
    float* ffi = dev(pool, (size_t)tf * 4, 0.0f);
    ok = ok && grow_case("LabelFeatures", [&] {
           return WorldMi355LabelFeatures(bs[5], set, line_off, lstart, lend, lstate, names, level, ffi, 4, nullptr);
         }, [&] {
           return WorldMi355LabelFeatures(bs[5], set, line_off_f, fstart.data(), fend.data(), fstate.data(), fnames.data(), level, ffi, 4, nullptr);
         });
    HipStubTraceMark("step the feature set goes");
    WorldMi355DestroyLabelFeatureSet(set);
  }
  HipStubTraceMark("step teardown");
  if (!ok || WorldMi355Synchronize(ctx) != 0) return 65;
  for (auto b : bs) WorldMi355DestroyBatch(b);
  WorldMi355DestroyContext(ctx);
  (void)hipStreamDestroy(U);
  printf("capi grow ok: %ld device allocations, %ld launches\n", HipStubMallocs(), HipStubLaunches());
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "batched") == 0) return batched_sequence();
  if (argc > 1 && strcmp(argv[1], "streams") == 0) return stream_sequence();
  if (argc > 1 && strcmp(argv[1], "grow") == 0) return grow_sequence();
  int last_code = 0;
  if (getenv("HIP_STUB_DEVICES") && atoi(getenv("HIP_STUB_DEVICES")) == 0) {
    // no device: the drop-in entry points report to the handler and return (reference entry points are void)
    WorldMi355SetErrorHandler(on_error, &last_code);
    DioOption dopt;
    InitializeDioOption(&dopt);
    std::vector<double> x(8000, 0.1), t(401), f0(401);
    Dio(x.data(), 8000, 16000, &dopt, t.data(), f0.data());
    if (g_handler_calls != 1 || last_code == 0) { printf("no-device: handler calls %d code %d\n", g_handler_calls, last_code); return 1; }
    WorldMi355Context* ctx = nullptr;
    if (WorldMi355CreateContext(-1, nullptr, &ctx) == 0 || ctx) return 2;
    printf("capi no-device ok\n");
    return 0;
  }
  WorldMi355SetErrorHandler(on_error, &last_code);
  struct Case { int fs; double sec, fp; int fft; bool hv; } cases[] = {
      {16000, 1.30, 5.0, 0, false}, {16000, 0.21, 5.0, 0, false}, {16000, 0.75, 1.0, 0, true}, {22050, 0.40, 5.0, 0, false},
      {48000, 0.35, 5.0, 0, false}, {48000, 0.30, 5.0, 4096, false}, {8000, 0.50, 10.0, 0, false}, {16000, 0.033, 5.0, 0, false},
      {44100, 0.25, 5.0, 0, true}, {16000, 0.50, 5.0, 2048, false}};
  for (const Case& c : cases) {
    const int before = g_handler_calls;
    const int rc = one_utterance(c.fs, c.sec, c.fp, c.fft, c.hv);
    if (rc != 0 && g_handler_calls == before) {       // a failure must have gone through the handler, never silently
      printf("case fs %d %.3f s fp %.1f fft %d: rc %d without a handler call\n", c.fs, c.sec, c.fp, c.fft, rc);
      return 3;
    }
  }
  // what the library refuses, it refuses through the handler: an fft size it has no transform for, a sampling rate
  // whose D4C sizes differ, an empty utterance
  {
    const int before = g_handler_calls;
    std::vector<double> x(4000, 0.1), t(200, 0.0), f0(200, 120.0);
    for (int i = 0; i < 200; ++i) t[(size_t)i] = i * 0.005;
    CheapTrickOption copt;
    InitializeCheapTrickOption(16000, &copt);
    copt.fft_size = 300;                                    // not a power of two
    Rows sp(200, 151);
    CheapTrick(x.data(), 4000, 16000, t.data(), f0.data(), 200, &copt, sp.p.data());
    DioOption dopt;
    InitializeDioOption(&dopt);
    Dio(x.data(), 0, 16000, &dopt, t.data(), f0.data());    // empty
    if (g_handler_calls == before) { printf("refusals did not reach the handler\n"); return 4; }
    // a NULL batch is refused by every batched entry point, the older ones (Dio ... UtteranceStatus) included
    double* d = x.data();
    float* q = nullptr;
    const int null_batch[] = {
        WorldMi355Dio(nullptr, d, d, d), WorldMi355Harvest(nullptr, d, d, d), WorldMi355StoneMask(nullptr, d, d, d, d),
        WorldMi355CheapTrick(nullptr, d, d, d, d), WorldMi355D4C(nullptr, d, d, d, d), WorldMi355Synthesis(nullptr, d, d, d, d),
        WorldMi355Analyze(nullptr, d, d, d, d, d), WorldMi355AnalyzeSynthesize(nullptr, d, d, d, d, d, d),
        WorldMi355CodeSpectralEnvelope(nullptr, d, 20, d), WorldMi355DecodeSpectralEnvelope(nullptr, d, 20, d),
        WorldMi355CodeAperiodicity(nullptr, d, d), WorldMi355DecodeAperiodicity(nullptr, d, d),
        WorldMi355RecipeFeatures(nullptr, d, d, d, 20, 5, q, q, q), WorldMi355RecipeDecode(nullptr, q, q, q, 20, 5, d, d, d),
        WorldMi355SamplesFromPcm16(nullptr, nullptr, d), WorldMi355SamplesToPcm16(nullptr, d, nullptr),
        WorldMi355Vibrato(nullptr, q, nullptr, nullptr, nullptr, d, q, q, nullptr),
        WorldMi355UtteranceStatus(nullptr, d, d, d, d, nullptr)};
    for (int rc : null_batch)
      if (rc != WM_ERR_BAD_ARG) { printf("a NULL batch was answered with %d\n", rc); return 4; }
  }
  // the batched API: create, analyze into caller buffers, destroy -- and a context torn down with work behind it
  {
    WorldMi355Context* ctx = nullptr;
    const bool inject = getenv("HIP_STUB_FAIL_MALLOC_AFTER") != nullptr;       // allocation failures are the point then
    if (WorldMi355CreateContext(-1, nullptr, &ctx) != 0 || !ctx) return inject ? 0 : 5;
    WorldMi355Params p;
    WorldMi355DefaultParams(16000, 5.0, &p);
    const int lens[3] = {9000, 16000, 4321};
    WorldMi355Batch* b = nullptr;
    if (WorldMi355CreateBatch(ctx, &p, 3, lens, nullptr, nullptr, &b) != 0 || !b) {
      printf("CreateBatch: %s\n", WorldMi355LastError());
      if (!inject) return 6;
    }
    // the stream/window bundle of ComposeCmp: a valid one is read tap by tap at its exact sizes; a null window and a
    // window of 16 taps are refused on the host
    if (b) {
      const size_t tf = (size_t)WorldMi355BatchTotalFrames(b);
      std::vector<float> data(tf * 2, 0.5f), out(tf * 4, NAN);
      const float* streams[1] = {data.data()};
      const int dims[1] = {2}, nwin[1] = {2}, sizes_ok[2] = {1, 3}, sizes_16[2] = {1, 16};
      std::vector<double> w0(1, 1.0), w1{-0.5, 0.0, 0.5}, w16(16, 0.0);
      const double* wins_ok[2] = {w0.data(), w1.data()};
      const double* wins_null[2] = {w0.data(), nullptr};
      const double* wins_16[2] = {w0.data(), w16.data()};
      const double* const* windows[1] = {wins_ok};
      const int* sizes[1] = {sizes_ok};
      if (WorldMi355ComposeCmp(b, 1, streams, dims, nwin, windows, sizes, out.data()) != WM_OK) return 7;
      windows[0] = wins_null;
      if (WorldMi355ComposeCmp(b, 1, streams, dims, nwin, windows, sizes, out.data()) != WM_ERR_BAD_ARG) return 8;
      windows[0] = wins_16;
      sizes[0] = sizes_16;
      if (WorldMi355ComposeCmp(b, 1, streams, dims, nwin, windows, sizes, out.data()) != WM_ERR_BAD_ARG) return 9;
    }
    if (b) WorldMi355DestroyBatch(b);
    WorldMi355DestroyContext(ctx);
  }
  WorldMi355SetErrorHandler(nullptr, nullptr);
  printf("capi ok: %d handler calls, %ld device allocations, %ld launches\n", g_handler_calls, HipStubMallocs(), HipStubLaunches());
  return 0;
}
