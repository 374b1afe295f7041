// Drives the HOST layer of libworld_mi355 (csrc/capi.cpp, context.cpp and the host halves of the .hip units) under
// AddressSanitizer + UBSan against tests/hostsan/hip_stub.cpp, the way the reference's CLIs call it
// (test/analysis.cpp:93-203, test/synth.cpp:103-106): host pointers, `double**` rows allocated ONE BY ONE at their
// exact size (analysis.cpp:172-176) -- a scatter that is one element off lands in a red zone.  Kernels do not run in
// the stub, so nothing here checks arithmetic; what is checked is that every call returns, outputs are written and
// finite, the error-handler path unwinds cleanly, and the sanitizers stay silent.
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
extern "C" void HipStubTraceMark(const char* text);

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

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "batched") == 0) return batched_sequence();
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
