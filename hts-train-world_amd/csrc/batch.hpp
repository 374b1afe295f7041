// batch.hpp -- host-side state shared by the kernel launchers and the C ABI.
//
// Context : one per (process, device): the caller's HIP stream, the universal randn table
//           (matlabfunctions.cpp:247-277 as data), launch geometry.
// Batch   : one per set of utterances: lengths/offsets on host and device, the
//           frame->utterance map and the per-frame arrays several stages share,
//           and each stage's own workspace, built on its first use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/world_mi355.h"

namespace wm {

int wm_check(hipError_t e);   // maps to WM_ERR_HIP and records the message
void set_error(const char* msg);

// Device memory of batches and stage workspaces comes from a process-wide cache of freed blocks (context.cpp):
// the drop-in C API builds a batch per call signature, and hipMalloc / hipFree (which also synchronises the
// device) per utterance were a third of its latency.  A block goes back to the cache when it is freed and is
// handed out again for a request of its size class; callers free only memory whose users have finished or are
// ordered on the stream that will use it next (DestroyBatch synchronises its context's stream first).
hipError_t dev_alloc_bytes(void** p, size_t bytes);
void dev_free(void* p);
void dev_cache_trim(size_t keep_bytes);       // hipFree cached blocks until at most keep_bytes stay cached
size_t dev_alloc_size(size_t bytes);          // what a request of `bytes` takes from the device: its size class (host only)
template <class T> inline hipError_t dev_alloc(T** p, size_t bytes) { return dev_alloc_bytes((void**)p, bytes); }

struct NoCopy {                               // base of what frees or restores something in its destructor
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};

// Device blocks freed together with their owner: alloc() records what it hands out.  Every stage keeps the state it
// builds in one such struct, private to its .hip file and owned by the batch (Batch::dio ... ffi); a set-up builds it
// in a local and moves it into the batch only once every allocation, copy, launch and synchronisation has succeeded,
// so a failure leaves nothing half-built behind.  A stage whose needs vary from call to call keeps it with grow_ws().
struct StageWs : NoCopy {
  std::vector<void*> owned;
  template <class T> hipError_t alloc(T** p, size_t bytes) {
    const hipError_t e = dev_alloc(p, bytes);
    if (e == hipSuccess) owned.push_back(*p);
    return e;
  }
  virtual ~StageWs() {
    for (void* p : owned) dev_free(p);
  }
};

// The workspace of a stage that may need a larger one than the batch holds (a wider band, more rows, a training pass
// after a forward pass).  The one rule, for every such stage:
//   * a workspace that exists and fits -- fits(present) -- is used as it is;
//   * otherwise one that exists is released first, after a wait for `st`: an earlier call's kernels, queued on the
//     stream this call was given, may still use it.  The two never exist side by side;
//   * the new one is built in a local -- build(fresh) -> WM_OK -- and published only when every allocation has succeeded;
//   * a failed build returns its error and leaves the slot empty: the next call builds afresh.  (A failed wait returns
//     its error with the slot as it was.)
// `Held` is what the slot may hold where that is a base of Ws (the training pass finds the forward pass's DnnWs).
template <class Ws, class Held = Ws, class Fits, class Build>
int grow_ws(std::unique_ptr<StageWs>& slot, hipStream_t st, Ws*& out, Fits fits, Build build) {
  out = nullptr;
  if (slot) {
    if (fits(static_cast<const Held&>(*slot))) {
      out = static_cast<Ws*>(slot.get());
      return WM_OK;
    }
    if (const int rc = wm_check(hipStreamSynchronize(st))) return rc;
    slot.reset();
  }
  std::unique_ptr<Ws> fresh(new Ws());
  if (const int rc = build(*fresh)) return rc;
  out = fresh.get();
  slot = std::move(fresh);
  return WM_OK;
}

// Byte offsets of the sections of one allocation, 256-byte aligned and handed out one after another (an empty one
// still takes a slot); `at` is the size so far.
struct Sections {
  size_t at = 0;
  size_t operator()(size_t bytes) {
    const size_t o = at;
    at = (at + (bytes ? bytes : 8) + 255) & ~(size_t)255;
    return o;
  }
};

// A per-context table: its kind and that kind's parameters (compared exactly; unused ones 0), and its device blocks.
enum TableKind { kDioFilters, kD4cWindow, kDcRemover, kSmTwiddles };
struct TableKey {
  TableKind kind;
  double v[5];
  bool operator==(const TableKey& o) const {
    for (int i = 0; i < 5; ++i)
      if (!(v[i] == o.v[i])) return false;
    return kind == o.kind;
  }
};
struct Table : StageWs {
  TableKey key;
  void* d[3] = {nullptr, nullptr, nullptr};
};

// Streams and events that are created together and destroyed with their owner, in StageWs' idiom: a set-up creates them
// in a local and moves that into the context only when every creation has succeeded, so nothing half-made is ever seen.
struct Handles : NoCopy {
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> events;
  hipError_t stream(hipStream_t* s) { return keep(hipStreamCreateWithFlags(s, hipStreamNonBlocking), streams, *s); }
  hipError_t stream(hipStream_t* s, int prio) { return keep(hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio), streams, *s); }
  hipError_t event(hipEvent_t* e) { return keep(hipEventCreateWithFlags(e, hipEventDisableTiming), events, *e); }
  ~Handles() {
    for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
  }
 private:
  template <class T> static hipError_t keep(hipError_t e, std::vector<T>& v, T made) {
    if (e == hipSuccess) v.push_back(made);
    return e;
  }
};
// the one-call forms and Synthesis' render stage (Context::ensure_side)
struct SideStreams : Handles {
  hipStream_t side = nullptr;        // D4C's and Synthesis' preparation beside CheapTrick; the overlap-adds
  hipStream_t aux = nullptr;         // D4C's RARE launch (d4c_rare)
  hipEvent_t ev_f0 = nullptr, ev_prep = nullptr, ev_d4c = nullptr, ev_rare = nullptr;
  hipEvent_t ev_pulse[2] = {nullptr, nullptr}, ev_ola[2] = {nullptr, nullptr};   // synthesis_render's two response halves
};
// the split form of launch_synthesis, made when it first runs
struct SplitStreams : Handles {
  hipStream_t prep = nullptr;        // the f0-only kernels of the batch's second part
  hipEvent_t ev_call = nullptr, ev_prep_b = nullptr;
};
// {total pulses, largest per-utterance count} of the last Synthesis: two pinned, mapped integers the device writes
struct PulseInfo : NoCopy {
  int64_t* h = nullptr;
  int64_t* d = nullptr;              // the same memory as the device sees it
  ~PulseInfo() { (void)hipHostFree(h); }   // (of NULL: no-op)
};
// Driven by one thread at a time (with its batches): table, scratch, events and pulse counters are shared by all its calls.
struct Context {
  int device = 0;
  hipStream_t stream = nullptr;      // the CALLER's (CreateContext / SetStream), read by capi.cpp alone (and by
                                     // label_set_destroy, which has no caller to take one from): every launcher is
                                     // handed the stream it queues on as its argument `st`
  int num_cu = 256;
  int frame_grid = 256 * 8;          // upper bound on the workgroups of a grid-stride per-frame kernel
  int oversub = 6;                   // workgroups per resident slot of those kernels (persistent_grid): measured on
                                     // configs[1], round 2: 21.2 / 18.0 / 17.7 / 17.3 / 17.3 ms per step at 1 / 2 / 4 / 8 /
                                     // 16; end of round 3 (profiles/README.md, r03_d_bench_default.json): 15.0 / 14.2 / 14.1 /
                                     // 14.3 / 13.8 / 14.2 / 14.0 / 14.7 / 17.0 at 2 / 3 / 4 / 5 / 6 / 7 / 8 / 16 / 32 -- a
                                     // workgroup's start (twiddle bases, the blocking fill of the scalar pipe, its share
                                     // of the default rows) is worth most of a frame, a large share makes the last round
                                     // ragged
  uint32_t* d_rng = nullptr;         // universal randn table, uint32 sums
  int64_t rng_cap = 0;
  uint32_t rng_state[4] = {123456789u, 362436069u, 521288629u, 88675123u};   // matlabfunctions.cpp:247-250
  double* d_scratch = nullptr;       // growable scratch (synthesis responses)
  int64_t scratch_cap = 0;           // in doubles
  // grow (+ generate); `user` is the stream whose kernels may still read the old block: waited for before it is freed
  int ensure_rng(int64_t count, hipStream_t user);
  int ensure_scratch(int64_t doubles, hipStream_t user);
  std::unique_ptr<PulseInfo> pulse;      // made by Synthesis' first set-up on the context
  std::unique_ptr<SideStreams> fork;
  std::unique_ptr<SplitStreams> split;
  int ensure_side(), ensure_split(); // `fork` / `split`, created on first use
  // Tables that depend on a few parameters, not on the utterances (Dio's filters, D4C's Nuttall window, Synthesis' DC
  // remover, StoneMask's twiddles): built once per context and key and shared by every batch of the context (the
  // drop-in API makes a batch per utterance length: rebuilding them per batch was 0.1 - 0.3 ms of every call)
  std::vector<std::unique_ptr<Table>> tables;
  template <class Build> int table(const TableKey& key, const Table*& out, Build build);
  std::unique_ptr<StageWs> mlsa_noise;   // excite's Gaussian sequence g (mlsa.hip), grown by grow_ws' rule
  // optional per-kernel HIP-event timing (bench.py's roofline leg): see TimedScope
  bool timing = false;
  std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> timed;
  void timing_clear();
};

// The table of `key`, built by build(Table&) -> WM_OK on first use.  An entry that fails to build is freed, not kept.
template <class Build> int Context::table(const TableKey& key, const Table*& out, Build build) {
  for (const auto& t : tables)
    if (t->key == key) {
      out = t.get();
      return WM_OK;
    }
  std::unique_ptr<Table> t(new Table);
  t->key = key;
  const int rc = build(*t);
  if (rc) return rc;
  out = t.get();
  tables.push_back(std::move(t));
  return WM_OK;
}

// Grid of a grid-stride per-frame kernel: a small multiple (Context::oversub) of the workgroups that are resident
// at once.  Exactly the resident number gives every wave slot the same share when the kernel has the machine to
// itself, but then a slot that is busy with another stream's kernel when this one starts (the f0-only first part
// of Synthesis runs beside CheapTrick and D4C) delays a whole share by that much: the launch ends late by the
// overlap.  With a few workgroups per slot the hardware dispatcher hands the shares out as slots become free; the
// price is a last round that is not full (at most one share of 1 / oversub of a slot's work).
// The occupancy query is made once per (device, kernel, block size) -- a process may hold contexts on several GPUs --
// and remembered (context.cpp).  slot_get / slot_raise read and update an entry under the table's lock: two threads
// that drive contexts concurrently may both ask the runtime the first time, neither reads a half-written value.
int slot_get(int device, const void* kernel, int tag);                 // 0 = never set
int slot_raise(int device, const void* kernel, int tag, int value);    // entry = max(entry, value); returns the old entry
template <class K> inline int persistent_grid(const Context& c, K kernel, int block, int64_t items) {
  int per_cu = slot_get(c.device, (const void*)kernel, block);
  if (per_cu == 0) {
    int q = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kernel, block, 0) != hipSuccess || q < 1) q = 4;
    per_cu = q;
    (void)slot_raise(c.device, (const void*)kernel, block, q);
  }
  const int64_t g = (int64_t)c.num_cu * per_cu * c.oversub;
  return (int)(items < g ? items : g);
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize): once per (device, kernel), and again whenever a launch asks for more
// than the largest size granted so far (hv_refine_kernel's size varies with the batch).
template <class K> inline void allow_dynamic_lds(const Context& c, K kernel, int bytes) {
  if (slot_raise(c.device, (const void*)kernel, -1, bytes) >= bytes) return;
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// Every entry point that takes a batch or a context runs on the context's device, whatever device is current on
// the calling thread, and leaves the caller's current device as it found it.
struct OnDevice : NoCopy {
  int prev = -1;
  explicit OnDevice(const Context& c) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != c.device && hipSetDevice(c.device) == hipSuccess) prev = cur;
  }
  ~OnDevice() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// RAII bracket: records a start/stop event pair on `st`, the stream of the launches in its scope.
struct TimedScope {
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  TimedScope(Context* c, hipStream_t stream, const char* name) : st(stream) {
    if (!c->timing) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
    (void)hipEventRecord(a, st);
    c->timed[name].push_back(std::make_pair(a, b));
  }
  ~TimedScope() {
    if (b) (void)hipEventRecord(b, st);
  }
};

struct Batch {
  Context* ctx = nullptr;
  WorldMi355Params p{};
  int n_utt = 0;
  std::vector<int> x_len, f0_len, y_len;
  std::vector<int64_t> x_off, f_off, y_off;
  int64_t total_x = 0, total_f = 0, total_y = 0;
  int max_x_len = 0, max_f0_len = 0, max_y_len = 0;
  // device descriptors: sections of one allocation (d_arena), laid out by WorldMi355CreateBatch
  void* d_arena = nullptr;
  int64_t *d_x_off = nullptr, *d_f_off = nullptr, *d_y_off = nullptr;
  int *d_x_len = nullptr, *d_f0_len = nullptr, *d_y_len = nullptr;
  int* d_frame_utt = nullptr;        // [total_f]
  int* d_rng_off = nullptr;          // [total_f] per-frame randn offsets (CheapTrick / D4C phase 2)
  int* d_rng_off2 = nullptr;         // [total_f] D4C LoveTrain offsets
  double* d_ap0 = nullptr;           // [total_f] D4C LoveTrain result
  double* d_f0_tmp = nullptr;        // [total_f] raw DIO f0 before StoneMask
  int* d_perm = nullptr;             // [total_f] costly frames first (partition.hpp)
  int* d_part_cnt = nullptr;         // [total_f / 1024 + 2]
  int* d_part_n = nullptr;           // [4] number of listed frames
  // D4C's own offsets and lists: its preparation may run beside CheapTrick (d4c_prepare, d4c.hip)
  int* d_rng_off_d4c = nullptr;      // [total_f]
  int* d_perm_d4c = nullptr;         // [total_f]
  int* d_part_cnt_d4c = nullptr;     // [total_f / 1024 + 2]
  int* d_part_n_d4c = nullptr;       // [4]
  // each stage's own state, built on its first use (see StageWs): the struct is private to the stage's .hip file
  std::unique_ptr<StageWs> dio, d4c, syn, harvest, codec, vibrato, mlpg, mlpg_gv, mspf, trj, dnn, ffi, mgcep, mlsa, dtw, modify, lsp;
  bool syn_warm = false;                    // launch_analyze_synthesize has succeeded once on this batch
  // the f0 front end of the one-call forms (launch_f0; WorldMi355BatchSetF0Estimator): WM_F0_DIO or WM_F0_HARVEST, and
  // whether StoneMask follows it.  The stage entry points (WorldMi355Dio, WorldMi355Harvest, ...) do not read them.
  int f0_estimator = WM_F0_DIO;
  int f0_refine = 1;

  int64_t rng_bound_cheaptrick() const;
  int64_t rng_bound_d4c() const;
  int64_t rng_bound_synthesis() const;
  ~Batch() { dev_free(d_arena); }
};

// Kernel launchers (one translation unit each).  Whatever queues device work takes the stream it queues on, `st`,
// directly after its Batch& / Context&: the capi.cpp entry points pass the caller's (Context::stream), the one-call forms
// fork from `st` and join back into it, and a table or workspace built inside a stage is launched on and waited for on
// the `st` of the call that builds it.
int launch_dio(Batch& b, hipStream_t st, const double* d_x, double* d_t, double* d_f0);
int launch_harvest(Batch& b, hipStream_t st, const double* d_x, double* d_t, double* d_f0);
// What Harvest's set-up takes from the device for a batch of these sample counts (harvest.hip, HvPlan: the sizes the set-up
// itself allocates from).  Host only.  WM_ERR_UNSUPPORTED where the set-up would refuse the f0 range.
int harvest_workspace_bytes(const WorldMi355Params& p, int n_utt, const int* x_len, int64_t* bytes);
// the f0 front end of the one-call forms: the batch's estimator, and StoneMask behind it when the batch says so (context.cpp)
int launch_f0(Batch& b, hipStream_t st, const double* d_x, double* d_t, double* d_f0);
int launch_stonemask(Batch& b, hipStream_t st, const double* d_x, const double* d_t, const double* d_f0, double* d_out);
int launch_cheaptrick(Batch& b, hipStream_t st, const double* d_x, const double* d_t, const double* d_f0, double* d_sp);
int launch_d4c(Batch& b, hipStream_t st, const double* d_x, const double* d_t, const double* d_f0, double* d_ap);
int launch_analyze(Batch& b, hipStream_t st, const double* d_x, double* d_t, double* d_f0, double* d_sp, double* d_ap);
int launch_synthesis(Batch& b, hipStream_t st, const double* d_f0, const double* d_sp, const double* d_ap, double* d_y);
// the stages behind launch_d4c / launch_synthesis (context.cpp, the drop-in Synthesis())
int d4c_prepare(Batch& b, hipStream_t st, const double* d_x, const double* d_t, const double* d_f0);
int d4c_rare(Batch& b, hipStream_t st, const double* d_x, const double* d_t, const double* d_f0, double* d_ap);
int d4c_run(Batch& b, hipStream_t st, const double* d_x, const double* d_t, const double* d_f0, double* d_ap);
int synthesis_prepare(Batch& b, hipStream_t st, const double* d_f0, double* d_y);
int synthesis_begin(Batch& b, hipStream_t st, const double* d_f0, double* d_y);      // the f0-only kernels, queued
int synthesis_prepare_wait(Batch& b, hipStream_t st);                                 // their host round trip
int synthesis_render(Batch& b, hipStream_t st, const double* d_sp, const double* d_ap, double* d_y);
int launch_analyze_synthesize(Batch& b, hipStream_t st, const double* d_x, double* d_t, double* d_f0, double* d_sp,
                              double* d_ap, double* d_y);
int launch_utterance_status(Batch& b, hipStream_t st, const double* d_x, const double* d_f0, const double* d_sp,
                            const double* d_ap, int* d_status);
int launch_vibrato(Batch& b, hipStream_t st, const float* d_lf0, const int* seg_utt_off, const int* seg_start,
                   const int* seg_end, const double* seg_pitch, float* d_vib, float* d_lf0_out, int* n_too_long);
int launch_pcm16_to_samples(Batch& b, hipStream_t st, const int16_t* d_pcm, double* d_x);
int launch_samples_to_pcm16(Batch& b, hipStream_t st, const double* d_y, int16_t* d_pcm);
int codec_num_aperiodicities(int fs);
int launch_code_spectral_envelope(Batch& b, hipStream_t st, const double* d_sp, int ndim, double* d_coded);
int launch_decode_spectral_envelope(Batch& b, hipStream_t st, const double* d_coded, int ndim, double* d_sp);
int launch_code_aperiodicity(Batch& b, hipStream_t st, const double* d_ap, double* d_coded);
int launch_decode_aperiodicity(Batch& b, hipStream_t st, const double* d_coded, double* d_ap);
int check_compose_cmp(int n_streams, const float* const* d_data, const int* dims, const int* n_windows,
                      const double* const* const* windows, const int* const* window_sizes, const float* d_out);
int launch_compose_cmp(Batch& b, hipStream_t st, int n_streams, const float* const* d_data, const int* dims,
                       const int* n_windows, const double* const* const* windows, const int* const* window_sizes,
                       float* d_out);
int launch_recipe_features(Batch& b, hipStream_t st, const double* d_f0, const double* d_sp, const double* d_ap,
                           int spec_dim, int ap_dim, float* d_lf0, float* d_mgc, float* d_bap);
int launch_recipe_decode(Batch& b, hipStream_t st, const float* d_lf0, const float* d_mgc, const float* d_bap,
                         int spec_dim, int ap_dim, double* d_f0, double* d_sp, double* d_ap);
int check_mel_cepstrum(const Batch& b, const double* d_spec, const WorldMi355McepOption& opt, const double* d_mc);
int launch_mel_cepstrum(Batch& b, hipStream_t st, const double* d_spec, const WorldMi355McepOption& opt, double* d_mc,
                        int* d_status);
// mgcep.hip: mcep's itype 0 on rows of windowed frames, and on waveforms framed and windowed on the way in
int sptk_frames(int64_t n_samples, int frame_length, int frame_shift, int64_t* n_frames);
int sptk_window(int type, int normalize, int length, double* w);
int check_mgcep(const Batch& b, const double* d_in, bool waveform, const double* window, int frame_length,
                int frame_shift, const WorldMi355McepOption& opt, const double* d_mc);
int launch_mel_cepstrum_of_frames(Batch& b, hipStream_t st, const double* d_frames, const WorldMi355McepOption& opt,
                                  double* d_mc, int* d_status);
int launch_mel_cepstrum_of_waveform(Batch& b, hipStream_t st, const double* d_x, const double* window, int frame_length,
                                    int frame_shift, int pipe_float32, const WorldMi355McepOption& opt, double* d_mc,
                                    int* d_status);
int check_mgc2sp(const Batch& b, const double* d_mc, const WorldMi355Mgc2spOption& opt, const double* d_sp);
int launch_mgc2sp(Batch& b, hipStream_t st, const double* d_mc, const WorldMi355Mgc2spOption& opt, double* d_sp,
                  double* d_phase, int* d_status);
int check_mgc2mgc(int64_t total_rows, const double* d_in, const WorldMi355MgcConvertOption* opt, const double* d_out);
int launch_mgc2mgc(Batch& b, hipStream_t st, const double* d_in, const WorldMi355MgcConvertOption& opt, double* d_out,
                   int* d_status);
// the energy form: d_ene[row] = 1/2 ln sum_k c2[k]^2 of the row's conversion, NaN where the storing form flags the row
int launch_mgc2mgc_energy(Batch& b, hipStream_t st, const double* d_in, const WorldMi355MgcConvertOption& opt,
                          double* d_ene);
// lsp.hip: lspcheck | lsp2lpc, the way on to MGC rows, and postfiltering_lsp
int check_lsp(int64_t total_rows, const double* d_lsp, const WorldMi355LspOption* opt, const double* d_lpc,
              const double* d_checked);
int launch_lsp_to_lpc(Batch& b, hipStream_t st, const double* d_lsp, const WorldMi355LspOption& opt, double* d_lpc,
                      double* d_checked, int* d_status);
int check_lsp_to_mgc(int64_t total_rows, const double* d_lsp, const WorldMi355LspOption* opt, int out_order,
                     double out_alpha, double out_gamma, const double* d_out, const int* d_status);
int launch_lsp_to_mgc(Batch& b, hipStream_t st, const double* d_lsp, const WorldMi355LspOption& opt, int out_order,
                      double out_alpha, double out_gamma, double* d_out, int* d_status);
int check_lsp_postfilter(int64_t total_rows, const double* d_lsp, const WorldMi355LspPostfilterOption* opt,
                         const double* d_out, const double* d_ene1, const double* d_ene2, const int* d_status);
int launch_lsp_postfilter(Batch& b, hipStream_t st, const double* d_lsp, const WorldMi355LspPostfilterOption& opt,
                          double* d_out, double* d_ene1, double* d_ene2, int* d_status);
// mlsa.hip: excite | dfs | mglsadf.  mode bits of check_mlsa: 1 the excitation's arguments, 2 the filter's
int mlsa_samples(int n_frames, int frame_shift, int* n_samples);
int mlsa_pade(int order, double* row);
int mlsa_noise(int64_t n, double* out);
int check_mlsa(const Batch& b, int mode, const void* pitch, const void* mc, const double* lowpass, int n_low,
               const double* highpass, int n_high, const WorldMi355MlsaOption* opt, const void* e, const void* y);
int launch_mlsa_excitation(Batch& b, hipStream_t st, const float* d_pitch, const double* lowpass, int n_low,
                           const double* highpass, int n_high, const WorldMi355MlsaOption& opt, double* d_e);
int launch_mlsa_filter(Batch& b, hipStream_t st, const double* d_e, const float* d_mc, const WorldMi355MlsaOption& opt,
                       double* d_y, int* d_status);
int launch_mlsa_synthesis(Batch& b, hipStream_t st, const float* d_pitch, const float* d_mc, const double* lowpass,
                          int n_low, const double* highpass, int n_high, const WorldMi355MlsaOption& opt, double* d_y,
                          int* d_status);
// dtw.hip: alignment of two feature sequences per utterance and the distortion measures along a path
int dtw_workspace_bytes(int n_utt, const int* a_lengths, const int* b_lengths, int64_t* bytes);
int check_dtw(const Batch& b, const float* a, int64_t ld_a, const float* bs, int64_t ld_b, const int64_t* b_off, int first,
              int count, const int* path, const int* path_len, const double* cost);
int launch_dtw_align(Batch& b, hipStream_t st, const float* d_a, int64_t ld_a, const float* d_b, int64_t ld_b,
                     const int64_t* b_off, int first, int count, int* d_path, int* d_path_len, double* d_cost,
                     int* d_status);
int check_distortion(const Batch& b, const int* path, const int* path_len, const int64_t* b_off, int n_groups,
                     const WorldMi355DistortionGroup* groups, const WorldMi355DistortionOption* opt, const double* out);
int launch_feature_distortion(Batch& b, hipStream_t st, const int* d_path, const int* d_path_len, const int64_t* b_off,
                              const unsigned char* d_b_mask, int n_groups, const WorldMi355DistortionGroup* groups,
                              const WorldMi355DistortionOption& opt, double* d_out);
int check_mlpg(int n_streams, const float* const* mean, int64_t ld_mean, const float* const* var, int64_t ld_var,
               const int* dims, const int* n_windows, const double* const* const* windows,
               const int* const* window_sizes, const WorldMi355MlpgOption* opt, float* const* out);
int launch_mlpg(Batch& b, hipStream_t st, int n_streams, const float* const* mean, int64_t ld_mean,
                const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                const double* const* const* windows, const int* const* window_sizes, const float* const* msd,
                const WorldMi355MlpgOption& opt, float* const* out, int* d_status);
int launch_mlpg_flags(Batch& b, hipStream_t st, int n_streams, const float* const* mean, int64_t ld_mean,
                      const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                      const double* const* const* windows, const int* const* window_sizes, const float* const* msd,
                      const WorldMi355MlpgOption& opt, float* const* out, int* d_status, int* d_colflag);
int check_mlpg_gv(int n_streams, const int* dims, const float* const* gv_mean, const float* const* gv_var,
                  const WorldMi355GvOption* gv);
int launch_mlpg_gv(Batch& b, hipStream_t st, int n_streams, const float* const* mean, int64_t ld_mean,
                   const float* const* var, int64_t ld_var, const int* dims, const int* n_windows,
                   const double* const* const* windows, const int* const* window_sizes, const float* const* msd,
                   const WorldMi355MlpgOption& opt, const float* const* gv_mean, const float* const* gv_var,
                   const unsigned char* gv_mask, const WorldMi355GvOption& gv, float* const* out, double* info,
                   int* d_status);
int check_trj(int n_streams, const float* const* pred, const float* const* obs, int64_t ld, const float* const* var,
              const float* const* gv_var, const int* dims, const int* n_windows, const double* const* const* windows,
              const int* const* window_sizes, const float* const* msd_pred, const float* const* msd_obs,
              const float* const* msd_var, const WorldMi355TrajectoryOption* opt, const double* cost,
              float* const* grad_pred, float* const* grad_msd, int64_t ld_grad);
int launch_trj(Batch& b, hipStream_t st, int n_streams, const float* const* pred, const float* const* obs, int64_t ld,
               const float* const* var, const float* const* gv_var, const int* dims, const int* n_windows,
               const double* const* const* windows, const int* const* window_sizes, const float* const* msd_pred,
               const float* const* msd_obs, const float* const* msd_var, const WorldMi355TrajectoryOption& opt,
               double* cost, float* const* c, float* const* grad_pred, float* const* grad_msd, int64_t ld_grad,
               double* grad_var, int* d_status);
int check_dnn(int n_utt, const WorldMi355AcousticModel* m, const float* x, int64_t ld_x, const int* spkr, const float* out,
              int64_t ld_out, const float* obs, int64_t ld_obs, const double* cost);
int launch_dnn(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const float* x, int64_t ld_x, const int* spkr,
               float* out, int64_t ld_out, const float* obs, int64_t ld_obs, double* cost, int* d_status);
int check_dnn_train_forward(int n_utt, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop, const float* x,
                            int64_t ld_x, const int* spkr, const float* out, int64_t ld_out, const float* obs, int64_t ld_obs,
                            const double* cost, const float* grad_out, int64_t ld_grad, const double* grad_var);
int launch_dnn_train_forward(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const WorldMi355Dropout* drop,
                             const float* x, int64_t ld_x, const int* spkr, float* out, int64_t ld_out, const float* obs,
                             int64_t ld_obs, double* cost, float* grad_out, int64_t ld_grad, double* grad_var, int* d_status);
int check_dnn_backward(int n_utt, const WorldMi355AcousticModel* m, const WorldMi355Dropout* drop, const float* x,
                       int64_t ld_x, const int* spkr, const float* grad_out, int64_t ld_grad, float* const* grad_weights,
                       float* const* grad_biases, float* const* grad_spkr_weights);
int launch_dnn_backward(Batch& b, hipStream_t st, const WorldMi355AcousticModel& m, const WorldMi355Dropout* drop,
                        const float* x, int64_t ld_x, const int* spkr, const float* G, int64_t ld_g, float* const* gW,
                        float* const* gB, float* const* gS, int* d_status);
int check_optimizer_step(const WorldMi355OptimizerOption* opt, int n_tensors, float* const* param, const float* const* grad,
                         float* const* slot0, float* const* slot1, const int64_t* count, const float* rate);
int launch_optimizer_step(Context& c, hipStream_t st, const WorldMi355OptimizerOption& opt, int n_tensors, float* const* param,
                          const float* const* grad, float* const* slot0, float* const* slot1, const int64_t* count,
                          const float* rate, int* d_status);
int check_mcpf(const double* d_mc, const WorldMi355McpfOption* opt, const double* d_out);
int launch_mcpf(Batch& b, hipStream_t st, const double* d_mc, const WorldMi355McpfOption& opt, double* d_out,
                double* d_gain, int* d_status);
// modify.hip: F0 scaling and formant shift between analysis and synthesis; the factor arrays are HOST, one per utterance
int check_modify(const Batch& b, const double* f0_scale, const double* formant_ratio, const double* d_f0,
                 const double* d_sp, const double* d_f0_out, const double* d_sp_out);
int launch_modify(Batch& b, hipStream_t st, const double* f0_scale, const double* formant_ratio, const double* d_f0,
                  const double* d_sp, double* d_f0_out, double* d_sp_out);
int check_column_means(const double* d_x, int dim, const double* d_mean);
int launch_column_means(Batch& b, hipStream_t st, const double* d_x, int dim, double* d_mean);
int check_mspf(const double* d_x, int dim, const WorldMi355MspfOption* opt, const double* mean_gen, const double* std_gen,
               const double* mean_nat, const double* std_nat, const double* d_out);
int launch_mspf(Batch& b, hipStream_t st, const double* d_x, int dim, const WorldMi355MspfOption& opt,
                const double* mean_gen, const double* std_gen, const double* mean_nat, const double* std_nat,
                double* d_out, int* d_status);
int check_mspf_stats(const double* d_x, int dim, const WorldMi355MspfOption* opt, const double* d_sum,
                     const double* d_sumsq, const int64_t* n_frames);
int launch_mspf_stats(Batch& b, hipStream_t st, const double* d_x, int dim, const WorldMi355MspfOption& opt,
                      const double* d_mean, double* d_sum, double* d_sumsq, int64_t* n_frames);
int mspf_segment_frames();
int check_interpolate_gaps(const float* d_x, int dim, double ignore_value, const float* d_out);
int launch_interpolate_gaps(Batch& b, hipStream_t st, const float* d_x, int dim, double ignore_value, float* d_out,
                            float* d_voiced, int* d_status);
int check_compose_ffo(int n_streams, const float* const* d_data, const int* dims, const int* n_windows,
                      const double* const* const* windows, const int* const* window_sizes, const float* d_out);
int launch_compose_ffo(Batch& b, hipStream_t st, int n_streams, const float* const* d_data, const int* dims,
                       const int* n_windows, const double* const* const* windows, const int* const* window_sizes,
                       const float* const* d_msd, float* d_out);
int check_column_moments(const float* d_x, int64_t ld, int width, const double* ignore_value, const int64_t* d_count,
                         const double* d_mean, const double* d_m2);
int launch_column_moments(Batch& b, hipStream_t st, const float* d_x, int64_t ld, int width, const double* ignore_value,
                          int64_t* d_count, double* d_mean, double* d_m2);
struct LabelSet;                                    // a compiled question config and its device tables (ffi.hip)
int label_set_create(Context& c, int n_features, const WorldMi355LabelFeature* f, LabelSet** out);
void label_set_destroy(LabelSet* s);
int label_set_count(const LabelSet* s);
int check_label_features(const Batch& b, const LabelSet* set, const int* line_off, const int* start, const int* end,
                         const int* state_index, const char* const* name, const int* state_level, const float* d_out,
                         int64_t ld_out);
int launch_label_features(Batch& b, hipStream_t st, const LabelSet& set, const int* line_off, const int* start,
                          const int* end, const int* state_index, const char* const* name, const int* state_level,
                          float* d_out, int64_t ld_out, int* d_status);

}  // namespace wm
