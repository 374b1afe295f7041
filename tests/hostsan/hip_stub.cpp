// A stand-in for the HIP runtime, for the HOST layer of libworld_mi355 under AddressSanitizer / UBSan on a box without
// a GPU (tests/test_sanitizers.py).  Test infrastructure only: "device" memory is host heap (so a marshalling copy that
// is one byte too long is an ASan report), copies are memcpy, streams and events are tokens, and KERNELS DO NOT RUN --
// what a kernel would have written is the fill pattern of hipMalloc (finite doubles) or what a memset left.  The
// arithmetic is not under test here (tests/test_gpu_parity.py, on the device); the host side is: option validation,
// arena sizing, the `double**` gather / scatter of the drop-in entry points, the block cache, the error-handler path,
// and WHICH STREAM every call goes to: HIP_STUB_TRACE=file writes one line per call that carries a stream or an event.
//   HIP_STUB_DEVICES=0            a box without a device
//   HIP_STUB_FAIL_MALLOC_AFTER=n  every hipMalloc from the n-th on fails
//   HIP_STUB_FAIL_CREATE_AT=k     the k-th creation of a stream or of an untimed event fails, once
//   HIP_STUB_FAIL_DEVPTR_AT=k     the k-th hipHostGetDevicePointer fails, once
//   HIP_STUB_PULSES=t:m,t:m,...   the launches of synth_pulse_off_kernel report these pulse totals and per-utterance
//                                 maxima through their last argument, in turn (kernels do not run: it would be 0 : 0)
//   HIP_STUB_TRACE=file           see trace() below
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <stdio.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace {
std::atomic<int> g_device{0};
std::atomic<long> g_mallocs{0}, g_frees{0}, g_launches{0};
int g_devices = 1;                     // HIP_STUB_DEVICES=0: a box without a device
bool g_fail_malloc_after_set = false;
long g_fail_malloc_after = 0;
long g_fail_create_at = -1, g_fail_devptr_at = -1;
std::atomic<long> g_creations{0}, g_devptrs{0}, g_pulse_launches{0};
std::vector<std::pair<long, long>> g_pulses;
FILE* g_trace = nullptr;
struct Init {
  Init() {
    if (const char* e = getenv("HIP_STUB_DEVICES")) g_devices = atoi(e);
    if (const char* e = getenv("HIP_STUB_FAIL_MALLOC_AFTER")) { g_fail_malloc_after_set = true; g_fail_malloc_after = atol(e); }
    if (const char* e = getenv("HIP_STUB_FAIL_CREATE_AT")) g_fail_create_at = atol(e);
    if (const char* e = getenv("HIP_STUB_FAIL_DEVPTR_AT")) g_fail_devptr_at = atol(e);
    if (const char* e = getenv("HIP_STUB_PULSES"))
      for (long t = 0, m = 0; *e && sscanf(e, "%ld:%ld", &t, &m) == 2; e += strcspn(e, ","), e += *e == ',') g_pulses.push_back({t, m});
    if (const char* e = getenv("HIP_STUB_TRACE")) g_trace = fopen(e, "w");
  }
  ~Init() { if (g_trace) fclose(g_trace); }
} g_init;

// Streams and events are heap tokens that hold a serial number (an address may come back after a destroy, a number
// does not); the trace names them s<k> / e<k> in order of first appearance, the NULL stream included.
std::mutex g_trace_mu;
std::map<const void*, std::string>& kernel_names() {    // host function pointer -> device name (__hipRegisterFunction,
  static auto* m = new std::map<const void*, std::string>;   // which runs from other units' static constructors)
  return *m;
}
std::map<long, int> g_seen[2];
long g_serial = 0;
void* new_token() {
  if (g_creations++ == g_fail_create_at) return nullptr;
  long* t = (long*)malloc(sizeof(long));
  std::lock_guard<std::mutex> g(g_trace_mu);
  *t = ++g_serial;
  return t;
}
std::string ordinal(int kind, const void* token) {
  const long serial = token ? *(const long*)token : 0;
  const int k = g_seen[kind].emplace(serial, (int)g_seen[kind].size()).first->second;
  return (kind ? " e" : " s") + std::to_string(k);
}
// one line: the call, for a launch the kernel and its geometry, then the stream and the event if the call has one
void trace(const char* call, bool has_stream, hipStream_t s, hipEvent_t e = nullptr, const std::string& what = "") {
  if (!g_trace) return;
  std::lock_guard<std::mutex> g(g_trace_mu);
  std::string line = call + what;
  if (has_stream) line += ordinal(0, s);
  if (e) line += ordinal(1, e);
  fprintf(g_trace, "%s\n", line.c_str());
}
template <class T> hipError_t create(T* out) {
  *out = (T)new_token();
  return *out ? hipSuccess : hipErrorOutOfMemory;
}
}  // namespace

extern "C" {
long HipStubMallocs() { return g_mallocs.load(); }
long HipStubFrees() { return g_frees.load(); }
long HipStubLaunches() { return g_launches.load(); }
long HipStubCreations() { return g_creations.load(); }       // streams and untimed events asked for so far
long HipStubDevPtrs() { return g_devptrs.load(); }
void HipStubNextPulses(long index) { g_pulse_launches = index; }   // which entry of HIP_STUB_PULSES comes next
void HipStubFailMallocAfter(long n) {                        // HIP_STUB_FAIL_MALLOC_AFTER, set by the harness mid-run; n < 0: off
  g_fail_malloc_after_set = n >= 0;
  g_fail_malloc_after = n;
}
void HipStubTraceMark(const char* text) {                    // a line of the harness's own in the trace ("# ...")
  if (!g_trace) return;
  std::lock_guard<std::mutex> g(g_trace_mu);
  fprintf(g_trace, "# %s\n", text);
}
void HipStubTraceStream(const char* label, void* stream) {    // "# stream <label> s<k>": which trace name a stream of
  if (!g_trace) return;                                       // the harness has (NULL is the legacy default stream)
  std::lock_guard<std::mutex> g(g_trace_mu);
  fprintf(g_trace, "# stream %s%s\n", label, ordinal(0, stream).c_str());
}

hipError_t hipGetDeviceCount(int* n) { *n = g_devices; return g_devices > 0 ? hipSuccess : hipErrorNoDevice; }
hipError_t hipGetDevice(int* d) { *d = g_device.load(); return hipSuccess; }
hipError_t hipSetDevice(int d) { if (d < 0 || d >= g_devices) return hipErrorInvalidDevice; g_device = d; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) {
  memset(p, 0, sizeof(*p));
  p->multiProcessorCount = 256;
  strcpy(p->name, "hip_stub");
  return hipSuccess;
}
hipError_t hipDeviceSynchronize() { trace("hipDeviceSynchronize", false, nullptr); return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }

hipError_t hipMalloc(void** p, size_t bytes) {
  if (g_fail_malloc_after_set && g_mallocs.load() >= g_fail_malloc_after) { *p = nullptr; return hipErrorOutOfMemory; }
  ++g_mallocs;
  void* q = malloc(bytes ? bytes : 1);
  if (!q) return hipErrorOutOfMemory;
  // a finite pattern: what a kernel "wrote" (doubles 0.25, 0.5, ...; harmless as int32 / float too)
  double* d = (double*)q;
  for (size_t i = 0; i + 1 <= bytes / 8; ++i) d[i] = 0.25 * (double)(1 + (i & 1023));
  memset((char*)q + (bytes / 8) * 8, 0, bytes % 8);
  *p = q;
  return hipSuccess;
}
hipError_t hipFree(void* p) { if (p) ++g_frees; free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
  *p = calloc(1, bytes ? bytes : 1);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) {
  if (g_devptrs++ == g_fail_devptr_at) { *d = nullptr; return hipErrorInvalidValue; }
  *d = h;
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind) { if (n) memcpy(dst, src, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t s) { trace("hipMemcpyAsync", true, s); if (n) memmove(dst, src, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t s) { trace("hipMemsetAsync", true, s); if (n) memset(dst, v, n); return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return create(s); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return create(s); }
hipError_t hipStreamDestroy(hipStream_t s) { free((void*)s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { trace("hipStreamSynchronize", true, s); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { trace("hipStreamWaitEvent", true, s, e); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) {                   // TimedScope's: not among the injected failures
  long* t = (long*)malloc(sizeof(long));
  std::lock_guard<std::mutex> g(g_trace_mu);
  *t = ++g_serial;
  *e = (hipEvent_t)t;
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return create(e); }
hipError_t hipEventDestroy(hipEvent_t e) { free((void*)e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { trace("hipEventRecord", true, s, e); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { *n = 2; return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t, hipStream_t s) {
  ++g_launches;
  std::string name;
  {
    std::lock_guard<std::mutex> lock(g_trace_mu);
    auto it = kernel_names().find(f);
    if (it != kernel_names().end()) name = it->second;
  }
  char geo[96];
  snprintf(geo, sizeof(geo), " grid %u %u %u block %u %u %u", g.x, g.y, g.z, b.x, b.y, b.z);
  trace("launch ", true, s, nullptr, name + geo);
  if (!g_pulses.empty() && name.find("synth_pulse_off_kernel") != std::string::npos) {
    // (utts, cnt, n_list, base, off, info): what the host reads back from the mapped `info` after its round trip
    const auto& tm = g_pulses[(size_t)(g_pulse_launches++ % (long)g_pulses.size())];
    int64_t* info = *(int64_t**)args[5];
    info[0] = tm.first;
    info[1] = tm.second;
  }
  return hipSuccess;
}

// what the host halves of the .hip translation units reference for kernel registration and launches
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fun, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  std::lock_guard<std::mutex> g(g_trace_mu);
  kernel_names()[host_fun] = device_name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
static thread_local struct { dim3 g, b; size_t shm; hipStream_t st; } t_cfg;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t shm, hipStream_t st) { t_cfg.g = g; t_cfg.b = b; t_cfg.shm = shm; t_cfg.st = st; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* shm, hipStream_t* st) { *g = t_cfg.g; *b = t_cfg.b; *shm = t_cfg.shm; *st = t_cfg.st; return hipSuccess; }
}
