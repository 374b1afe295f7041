// ffi.hip -- the acoustic model's input rows from aligned labels: data/scripts/makefeature.pl on the device, the
// counterpart of `ffo` (make_train_data_dnn / make_gen_data_dnn, scripts/Training.pl:1677-1723).
//
// A question config is compiled once into a feature set (labelpat.hpp): the binary features' alternatives as
// bit-parallel programs, laid out so that one feature's alternatives are neighbours, and a four-byte column code per
// feature.  A call finds the distinct label names of its batch on the host, evaluates the few float features there
// (backtracking, capture) and launches two kernels.
//
// label_match_kernel: distinct names x binary features.  A workgroup is one wave and takes one name, whose bytes it
// copies to LDS once (every lane then reads the same byte: a broadcast, made a scalar by readfirstlane).  Its lanes take
// 64 alternatives at a time and step them through the name with labelpat::step; the per-character mask table is laid
// out [character][alternative], so the 64 lanes read 512 neighbouring bytes per character.  A feature's answer is the
// OR over its alternatives: a ballot of the verdicts, cut into segments at the ballot of "first alternative of a
// feature"; the segment's first lane writes the byte when the segment also ends in the group (ballot of "last
// alternative"), otherwise the wave carries the segment's OR into the next group of 64.  One writer per (name, feature):
// no atomics.
//
// ffi_rows_kernel: frames x features.  A wave takes a row: its utterance from the batch's frame map, its line by a
// 64-way search (one probe per lane, a ballot) through the utterance's prefix sums of end - start, then consecutive
// lanes write consecutive columns from three sources: the answer bytes, the float table, and the six reserved values
// computed in place (makefeature.pl:377-431) and normalised by labelpat::normalise.  Four columns per lane as one
// 16-byte store where ld_out and the pointer allow, else one by one: the values do not depend on the path.  Only
// columns [0, n_features) are written.  status[u] gathers bit 1 (a value was clamped: the script's "Out of range"
// warning) and bit 2 (a state-related reserved feature in a phoneme-level file) with one atomicOr per row that has
// any; OR does not depend on the order.
#include <string.h>

#include <string>
#include <unordered_map>

#include "batch.hpp"
#include "common.hpp"
#include "labelpat.hpp"

namespace wm {

namespace lp = labelpat;
typedef unsigned long long u64;

constexpr int kFfiFirst = 1, kFfiLast = 2;          // alternative flags
constexpr int kFfiClamped = 1, kFfiNoState = 2;     // status bits

__global__ __launch_bounds__(64) void label_match_kernel(
    const unsigned char* __restrict__ names, const int* __restrict__ name_off, const u64* __restrict__ consumes,
    const u64* __restrict__ run, const u64* __restrict__ skip, const u64* __restrict__ accept,
    const int* __restrict__ alt_feature, const int* __restrict__ alt_flags, int a_pad, int n_binary,
    unsigned char* __restrict__ answers) {
  __shared__ unsigned char sname[lp::kMaxName + 1];
  const int lane = (int)threadIdx.x;
  const int d = (int)blockIdx.x;
  const int off = name_off[d];
  const int len = imin(name_off[d + 1] - off, lp::kMaxName);
  for (int i = lane; i < len; i += 64) sname[i] = (unsigned char)imin((names[off + i] - lp::kFirstChar) & 0xff, lp::kChars - 1);   // checked on the host
  wave_sync();
  bool carry = false;                               // the OR so far of a feature whose alternatives began in an earlier group
  for (int a0 = 0; a0 < a_pad; a0 += 64) {
    const int a = a0 + lane;
    const u64 my_run = run[a], my_skip = skip[a];
    u64 dstate = lp::close_over(1, my_skip);
    int i = 0;
    for (; i + 4 <= len; i += 4) {                  // the loads do not depend on the state: four in flight
      const int c0 = __builtin_amdgcn_readfirstlane((int)sname[i]), c1 = __builtin_amdgcn_readfirstlane((int)sname[i + 1]);
      const int c2 = __builtin_amdgcn_readfirstlane((int)sname[i + 2]), c3 = __builtin_amdgcn_readfirstlane((int)sname[i + 3]);
      const u64 m0 = consumes[(int64_t)c0 * a_pad + a], m1 = consumes[(int64_t)c1 * a_pad + a];
      const u64 m2 = consumes[(int64_t)c2 * a_pad + a], m3 = consumes[(int64_t)c3 * a_pad + a];
      dstate = lp::step(dstate, m0, my_run, my_skip);
      dstate = lp::step(dstate, m1, my_run, my_skip);
      dstate = lp::step(dstate, m2, my_run, my_skip);
      dstate = lp::step(dstate, m3, my_run, my_skip);
    }
    for (; i < len; ++i) {
      const int c = __builtin_amdgcn_readfirstlane((int)sname[i]);
      dstate = lp::step(dstate, consumes[(int64_t)c * a_pad + a], my_run, my_skip);
    }
    const int feat = alt_feature[a], flags = alt_flags[a];       // padding: feature -1, accept 0, both flags
    const u64 hits = __ballot((dstate & accept[a]) != 0);
    const u64 firsts = __ballot((flags & kFfiFirst) != 0);
    const u64 lasts = __ballot((flags & kFfiLast) != 0);
    const u64 heads = firsts | 1;                                 // lane 0 heads the segment that continues a feature
    const u64 above = lane == 63 ? (u64)0 : heads & ~(((u64)2 << lane) - 1);
    const int end = above != 0 ? __builtin_ctzll(above) - 1 : 63; // the last lane of this lane's segment
    const u64 seg = (end == 63 ? ~(u64)0 : (((u64)2 << end) - 1)) & ~(((u64)1 << lane) - 1);
    const bool continued = (firsts & 1) == 0;                     // lane 0's alternative is not its feature's first
    const bool any = (hits & seg) != 0 || (lane == 0 && continued && carry);
    const bool complete = ((lasts >> end) & 1) != 0;
    if (((heads >> lane) & 1) != 0 && complete && feat >= 0) answers[(int64_t)d * n_binary + feat] = any ? 1 : 0;
    // the segment that holds lane 63, the same in every lane
    const int h63 = 63 - __builtin_clzll(heads);
    const bool any63 = (hits >> h63) != 0 || (h63 == 0 && continued && carry);
    carry = ((lasts >> 63) & 1) != 0 ? false : any63;
  }
}

struct FfiCol {                                     // a reserved column: its kind (2 .. 7), min and max
  int kind, unused, min, max;
};

struct FfiLines {                                   // per line of the batch, and per utterance
  const int64_t* row_off;                           // [n_lines + 1] the batch row a line begins at
  const int *start, *end, *state_index, *ph_start, *ph_end, *name_id;
  const int* line_off;                              // [n_utt + 1]
  const int* state_level;                           // [n_utt]
  const int* name_clamped;                          // [n_distinct] a float feature of the name was clamped
};

// A column's code: its kind in the top four bits, below them its index among the binary features, among the float
// ones, or -- kinds 2 .. 7 -- among the set's reserved columns (FfiCol: min and max).  Four bytes per column instead of
// a descriptor of sixteen: the codes and the answer bytes are what the kernel reads per value it writes.
constexpr int kFfiCodeShift = 28;
__device__ __forceinline__ float ffi_value(int code, const FfiCol* __restrict__ reserved,
                                           const unsigned char* __restrict__ ans_row, const float* __restrict__ flt_row,
                                           int sl, int j, int start, int end, int sidx, int ph_start, int ph_end, int& st) {
  const int kind = code >> kFfiCodeShift, index = code & ((1 << kFfiCodeShift) - 1);
  if (kind == 0) return ans_row[index] ? 1.0f : 0.0f;
  if (kind == 1) return flt_row[index];
  const FfiCol c = reserved[index];
  int64_t v;
  if (c.kind <= 5 && !sl) {                         // makefeature.pl:380-382 and its likes: the value is min
    st |= kFfiNoState;
    v = c.min;
  } else if (c.kind == 2) v = sidx;
  else if (c.kind == 3) v = (int64_t)c.max - sidx + c.min;
  else if (c.kind == 4) v = (int64_t)1 + j - start;
  else if (c.kind == 5) v = (int64_t)end - j;
  else if (c.kind == 6) v = (int64_t)1 + j - ph_start;
  else v = (int64_t)ph_end - j;
  int clamped = 0;
  const float r = lp::normalise(v, c.min, c.max, &clamped);
  if (clamped) st |= kFfiClamped;
  return r;
}

__global__ __launch_bounds__(256) void ffi_rows_kernel(const int* __restrict__ codes, const FfiCol* __restrict__ reserved,
                                                       int n_features, int n_binary, int n_float,
                                                       const unsigned char* __restrict__ answers,
                                                       const float* __restrict__ floats, FfiLines L,
                                                       const int* __restrict__ frame_utt, int64_t total_rows,
                                                       float* __restrict__ out, int64_t ld_out, int vec4,
                                                       int* __restrict__ status) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  for (int64_t t = wave; t < total_rows; t += n_waves) {
    const int u = frame_utt[t];
    // the last line of the utterance whose first row is <= t (lines have at least one row)
    int lo = L.line_off[u], hi = L.line_off[u + 1];
    while (hi - lo > 1) {
      const int stride = (hi - lo + 63) / 64;
      const int probe = lo + lane * stride;
      const u64 le = __ballot(probe < hi && L.row_off[probe] <= t);
      const int k = __builtin_popcountll(le) - 1;  // lane 0's probe is lo: always counted
      lo = lo + k * stride;
      hi = imin(hi, lo + stride);
    }
    const int line = lo;
    const int start = L.start[line], end = L.end[line], sidx = L.state_index[line];
    const int ph_start = L.ph_start[line], ph_end = L.ph_end[line], nid = L.name_id[line];
    const int sl = L.state_level[u];
    const int j = start + (int)(t - L.row_off[line]);
    const unsigned char* __restrict__ ans_row = answers + (int64_t)nid * n_binary;
    const float* __restrict__ flt_row = floats + (int64_t)nid * n_float;
    float* __restrict__ row = out + t * ld_out;
    int st = L.name_clamped[nid] ? kFfiClamped : 0;
    if (vec4) {
      const int n4 = n_features & ~3;
      for (int k = lane * 4; k < n4; k += 256) {
        const int4 c = *reinterpret_cast<const int4*>(codes + k);      // the table is an allocation of its own: aligned
        float4 v;
        v.x = ffi_value(c.x, reserved, ans_row, flt_row, sl, j, start, end, sidx, ph_start, ph_end, st);
        v.y = ffi_value(c.y, reserved, ans_row, flt_row, sl, j, start, end, sidx, ph_start, ph_end, st);
        v.z = ffi_value(c.z, reserved, ans_row, flt_row, sl, j, start, end, sidx, ph_start, ph_end, st);
        v.w = ffi_value(c.w, reserved, ans_row, flt_row, sl, j, start, end, sidx, ph_start, ph_end, st);
        *reinterpret_cast<float4*>(row + k) = v;
      }
      const int k = n4 + lane;
      if (k < n_features)
        row[k] = ffi_value(codes[k], reserved, ans_row, flt_row, sl, j, start, end, sidx, ph_start, ph_end, st);
    } else {
      for (int k = lane; k < n_features; k += 64)
        row[k] = ffi_value(codes[k], reserved, ans_row, flt_row, sl, j, start, end, sidx, ph_start, ph_end, st);
    }
    if (status != nullptr) {
      const int bits = (__ballot((st & kFfiClamped) != 0) != 0 ? kFfiClamped : 0) |
                       (__ballot((st & kFfiNoState) != 0) != 0 ? kFfiNoState : 0);
      if (lane == 0 && bits != 0) atomicOr(&status[u], bits);
    }
  }
}

// ---- the feature set: the compiled config and its device tables ---------------------------------------------------------
struct LabelSet : StageWs {
  Context* ctx = nullptr;
  lp::FeatureSet host;
  int a_pad = 0;                                    // alternatives rounded up to whole groups of 64
  u64 *d_consumes = nullptr, *d_run = nullptr, *d_skip = nullptr, *d_accept = nullptr;
  int *d_alt_feature = nullptr, *d_alt_flags = nullptr;
  int* d_codes = nullptr;                           // [n_features]
  FfiCol* d_reserved = nullptr;                     // the reserved columns' kind, min and max
};

int label_set_create(Context& c, int n_features, const WorldMi355LabelFeature* f, LabelSet** out) {
  *out = nullptr;
  const char* why = "";
  std::unique_ptr<LabelSet> S(new LabelSet());
  if (const int rc = lp::compile_feature_set(n_features, f, S->host, &why)) {     // refused before any device call
    set_error((std::string("CreateLabelFeatureSet: ") + why).c_str());
    return rc;
  }
  S->ctx = &c;
  const lp::FeatureSet& h = S->host;
  const int A = (int)h.alts.size();
  const int a_pad = A > 0 ? (A + 63) / 64 * 64 : 64;
  S->a_pad = a_pad;
  std::vector<u64> consumes((size_t)lp::kChars * a_pad, 0), run((size_t)a_pad, 0), skip((size_t)a_pad, 0), accept((size_t)a_pad, 0);
  std::vector<int> alt_feature((size_t)a_pad, -1), alt_flags((size_t)a_pad, kFfiFirst | kFfiLast);
  for (int a = 0; a < A; ++a) {
    lp::Program p;
    lp::build_program(h.alts[(size_t)a], p);
    for (int ch = 0; ch < lp::kChars; ++ch) consumes[(size_t)ch * a_pad + a] = p.consumes[ch];
    run[(size_t)a] = p.run;
    skip[(size_t)a] = p.skip;
    accept[(size_t)a] = p.accept;
    alt_feature[(size_t)a] = h.alt_feature[(size_t)a];
    alt_flags[(size_t)a] = (a == 0 || h.alt_feature[(size_t)a - 1] != h.alt_feature[(size_t)a] ? kFfiFirst : 0) |
                           (a == A - 1 || h.alt_feature[(size_t)a + 1] != h.alt_feature[(size_t)a] ? kFfiLast : 0);
  }
  if (h.features.size() >= ((size_t)1 << kFfiCodeShift)) {
    set_error("CreateLabelFeatureSet: too many features");
    return WM_ERR_BAD_ARG;
  }
  std::vector<int> codes;
  std::vector<FfiCol> reserved;
  for (const lp::Feature& ft : h.features) {
    codes.push_back((ft.kind << kFfiCodeShift) | (ft.kind <= 1 ? ft.index : (int)reserved.size()));
    if (ft.kind >= 2) reserved.push_back(FfiCol{ft.kind, 0, ft.min, ft.max});
  }
  if (reserved.empty()) reserved.push_back(FfiCol{0, 0, 0, 0});
  int rc = WM_OK;
  auto up = [&](auto** dst, const auto& v) {
    if (rc) return;
    const size_t bytes = sizeof(v[0]) * v.size();
    rc = wm_check(S->alloc(dst, bytes));
    if (!rc) rc = wm_check(hipMemcpy(*dst, v.data(), bytes, hipMemcpyHostToDevice));
  };
  up(&S->d_consumes, consumes);
  up(&S->d_run, run);
  up(&S->d_skip, skip);
  up(&S->d_accept, accept);
  up(&S->d_alt_feature, alt_feature);
  up(&S->d_alt_flags, alt_flags);
  up(&S->d_codes, codes);
  up(&S->d_reserved, reserved);
  if (rc) return rc;
  *out = S.release();
  return WM_OK;
}

void label_set_destroy(LabelSet* s) {
  if (s == nullptr) return;
  OnDevice dev_(*s->ctx);
  (void)hipStreamSynchronize(s->ctx->stream);       // a queued kernel may still read the tables
  delete s;
}

int label_set_count(const LabelSet* s) { return s != nullptr ? (int)s->host.features.size() : 0; }

// ---- the stage ------------------------------------------------------------------------------------------------------------
// What is refused on the host alone; no device call is made for a refused argument set.
int check_label_features(const Batch& b, const LabelSet* set, const int* line_off, const int* start, const int* end,
                         const int* state_index, const char* const* name, const int* state_level, const float* d_out,
                         int64_t ld_out) {
  auto refuse = [](int rc, const char* why) {
    set_error((std::string("LabelFeatures: ") + why).c_str());
    return rc;
  };
  if (!set || !line_off || !start || !end || !state_index || !name || !state_level || !d_out)
    return refuse(WM_ERR_BAD_ARG, "a NULL required pointer");
  if (set->ctx != b.ctx) return refuse(WM_ERR_BAD_ARG, "the feature set belongs to another context");
  if (ld_out < (int64_t)set->host.features.size()) return refuse(WM_ERR_BAD_ARG, "ld_out < n_features");
  if (line_off[0] != 0) return refuse(WM_ERR_BAD_ARG, "line_off[0] != 0");
  for (int u = 0; u < b.n_utt; ++u) {
    if (line_off[u + 1] < line_off[u]) return refuse(WM_ERR_BAD_ARG, "line_off decreases");
    int64_t rows = 0;
    for (int i = line_off[u]; i < line_off[u + 1]; ++i) {
      if (start[i] < 0 || end[i] <= start[i]) return refuse(WM_ERR_BAD_ARG, "a line with end <= start or start < 0");
      rows += (int64_t)end[i] - start[i];
      const char* why = "";
      if (const int rc = lp::check_name(name[i], &why)) return refuse(rc, why);
    }
    if (rows != b.f_off[(size_t)u + 1] - b.f_off[(size_t)u])
      return refuse(WM_ERR_BAD_ARG, "an utterance's lines do not add up to its frame count");
  }
  return WM_OK;
}

struct FfiWs : StageWs {                            // the batch's uploads of its last call (Batch::ffi)
  std::vector<unsigned char> image;                 // the host side of the upload: alive while the copy is queued
  unsigned char* d = nullptr;
  size_t cap = 0;
};

int launch_label_features(Batch& b, hipStream_t st, const LabelSet& set, const int* line_off, const int* start,
                          const int* end, const int* state_index, const char* const* name, const int* state_level,
                          float* d_out, int64_t ld_out, int* d_status) {
  if (const int rc = check_label_features(b, &set, line_off, start, end, state_index, name, state_level, d_out, ld_out))
    return rc;
  if (b.n_utt <= 0) return WM_OK;
  if (d_status != nullptr)
    if (const int rc = wm_check(hipMemsetAsync(d_status, 0, sizeof(int) * (size_t)b.n_utt, st))) return rc;
  if (b.total_f <= 0) return WM_OK;
  const lp::FeatureSet& h = set.host;
  const int n_lines = line_off[b.n_utt];
  const int nb = h.n_binary, nf = h.n_float;
  // distinct names, in order of first appearance; their float features
  std::unordered_map<std::string, int> seen;
  std::vector<int> name_id((size_t)n_lines), name_off(1, 0), name_clamped;
  std::vector<unsigned char> bytes;
  std::vector<float> floats;
  for (int i = 0; i < n_lines; ++i) {
    const size_t n = strlen(name[i]);
    auto it = seen.find(std::string(name[i], n));
    if (it == seen.end()) {
      const int d = (int)seen.size();
      it = seen.emplace(std::string(name[i], n), d).first;
      bytes.insert(bytes.end(), name[i], name[i] + n);
      name_off.push_back((int)bytes.size());
      floats.resize((size_t)(d + 1) * (size_t)nf);
      name_clamped.push_back(lp::float_features(h, name[i], n, floats.data() + (size_t)d * (size_t)nf));
    }
    name_id[(size_t)i] = it->second;
  }
  const int nd = (int)seen.size();
  // per line: its first batch row, and its phoneme's first line's start and last line's end (makefeature.pl:294-316)
  std::vector<int64_t> row_off((size_t)n_lines + 1, 0);
  std::vector<int> ph_start((size_t)n_lines), ph_end((size_t)n_lines);
  for (int u = 0; u < b.n_utt; ++u) {
    const int l0 = line_off[u], l1 = line_off[u + 1];
    for (int i = l0; i < l1; ++i) {
      row_off[(size_t)i + 1] = row_off[(size_t)i] + (end[i] - start[i]);
      const bool joins = state_level[u] && i > l0 && state_index[i - 1] < state_index[i];
      ph_start[(size_t)i] = joins ? ph_start[(size_t)i - 1] : start[i];
    }
    for (int i = l1 - 1; i >= l0; --i) {
      const bool joins = state_level[u] && i < l1 - 1 && state_index[i] < state_index[i + 1];
      ph_end[(size_t)i] = joins ? ph_end[(size_t)i + 1] : end[i];
    }
  }
  // one image, one upload: 256-byte aligned sections
  Sections take;
  const size_t nl = (size_t)n_lines, nu = (size_t)b.n_utt;
  const size_t o_row = take(8 * (nl + 1)), o_start = take(4 * nl), o_end = take(4 * nl), o_sidx = take(4 * nl);
  const size_t o_phs = take(4 * nl), o_phe = take(4 * nl), o_nid = take(4 * nl), o_loff = take(4 * (nu + 1));
  const size_t o_sl = take(4 * nu), o_ncl = take(4 * (size_t)nd), o_noff = take(4 * ((size_t)nd + 1));
  const size_t o_bytes = take(bytes.size()), o_flt = take(4 * floats.size());
  const size_t init_bytes = take.at;
  const size_t o_ans = take((size_t)nd * (size_t)nb);
  const size_t need = take.at;
  // A workspace that is kept has its host image rewritten below: an earlier call's copy may still read it, so this
  // call waits for `st` itself.  One that is replaced is waited for by grow_ws(): one wait per call either way.
  const bool kept = b.ffi && static_cast<const FfiWs&>(*b.ffi).cap >= need;
  if (kept)
    if (const int rc = wm_check(hipStreamSynchronize(st))) return rc;
  FfiWs* W = nullptr;
  if (const int rc = grow_ws(b.ffi, st, W, [&](const FfiWs&) { return kept; }, [&](FfiWs& n) {
        n.cap = need;
        return wm_check(n.alloc(&n.d, need));
      }))
    return rc;
  W->image.assign(init_bytes, 0);
  unsigned char* img = W->image.data();
  auto put = [&](size_t o, const void* src, size_t n) { if (n) memcpy(img + o, src, n); };
  put(o_row, row_off.data(), 8 * (nl + 1));
  put(o_start, start, 4 * nl);
  put(o_end, end, 4 * nl);
  put(o_sidx, state_index, 4 * nl);
  put(o_phs, ph_start.data(), 4 * nl);
  put(o_phe, ph_end.data(), 4 * nl);
  put(o_nid, name_id.data(), 4 * nl);
  put(o_loff, line_off, 4 * (nu + 1));
  put(o_sl, state_level, 4 * nu);
  put(o_ncl, name_clamped.data(), 4 * (size_t)nd);
  put(o_noff, name_off.data(), 4 * ((size_t)nd + 1));
  put(o_bytes, bytes.data(), bytes.size());
  put(o_flt, floats.data(), 4 * floats.size());
  unsigned char* base = W->d;
  if (const int rc = wm_check(hipMemcpyAsync(base, img, init_bytes, hipMemcpyHostToDevice, st))) return rc;
  unsigned char* d_ans = base + o_ans;
  if (nb > 0) {
    if (const int rc = wm_check(hipMemsetAsync(d_ans, 0, (size_t)nd * (size_t)nb, st))) return rc;   // a feature without alternatives
    TimedScope ts_(b.ctx, st, "label_match_kernel");
    hipLaunchKernelGGL(label_match_kernel, dim3((unsigned)nd), dim3(64), 0, st, base + o_bytes, (const int*)(base + o_noff),
                       set.d_consumes, set.d_run, set.d_skip, set.d_accept, set.d_alt_feature, set.d_alt_flags, set.a_pad, nb,
                       d_ans);
    if (const int rc = wm_check(hipGetLastError())) return rc;
  }
  FfiLines L;
  L.row_off = (const int64_t*)(base + o_row);
  L.start = (const int*)(base + o_start);
  L.end = (const int*)(base + o_end);
  L.state_index = (const int*)(base + o_sidx);
  L.ph_start = (const int*)(base + o_phs);
  L.ph_end = (const int*)(base + o_phe);
  L.name_id = (const int*)(base + o_nid);
  L.line_off = (const int*)(base + o_loff);
  L.state_level = (const int*)(base + o_sl);
  L.name_clamped = (const int*)(base + o_ncl);
  const int n_features = (int)h.features.size();
  const int vec4 = ld_out % 4 == 0 && ((uintptr_t)d_out & 15) == 0 ? 1 : 0;
  const int64_t blocks = (b.total_f + 3) / 4, cap = (int64_t)b.ctx->num_cu * 32;
  TimedScope ts_(b.ctx, st, "ffi_rows_kernel");
  hipLaunchKernelGGL(ffi_rows_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, st, set.d_codes, set.d_reserved, n_features,
                     nb, nf, d_ans, (const float*)(base + o_flt), L, b.d_frame_utt, b.total_f, d_out, ld_out, vec4, d_status);
  return wm_check(hipGetLastError());
}

}  // namespace wm
