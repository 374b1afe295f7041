// labelpat.hpp -- the wildcard patterns of a question config (data/scripts/makefeature.pl:456-496), host side.
//
// No HIP runtime: the whole layer is inline in this header, and labelpat.cpp -- a translation unit of its own, like
// fileio.cpp -- holds its one C entry point (WorldMi355LabelPatternMatch).  ffi.hip includes the header for the compiler,
// for the float features and for the step function its kernel shares with the host loop.
//
// The token language.  The script turns a pattern into a Perl regex by substitution: `*` becomes `.*`, `?` becomes `.?`
// (zero or one character, not exactly one), `+ | ^ $ [ ]` are escaped and everything else is left as it is, so `.`
// matches any one character; in a float pattern `%d` becomes `([+-]?[0-9]+)`.  Here the text between the braces
// becomes tokens: literal byte, any-one (`.`), optional-any (`?`), any-run (`*`), number (`%d`, float patterns only;
// in a binary pattern `%` and `d` are two literals, as in the script).  A binary pattern is split at its commas; an
// empty alternative is valid and matches no name (a name is never empty).  Refused (WM_ERR_UNSUPPORTED) are bytes
// outside 0x21-0x7E, the characters the script leaves active as regex syntax (backslash, parentheses, braces) and an
// alternative of more than 63 tokens.
//
// Two engines.  match_backtrack walks the tokens in Perl's order -- `.*`, `.?` and the digits of `%d` greedy, the first
// success decides what `%d` captures -- and remembers failed (token, position) pairs, so a pattern with many `*` costs
// tokens x length^2 at most; a remembered failure is a failure on every path, so the first success is the same one.
// It evaluates the float features (a few dozen per config, once per distinct name: host work, uploaded as a float32
// table).  A binary alternative also compiles to a bit-parallel program: state bit i = "tokens 0 .. i-1 are consumed",
// n + 1 <= 64 bits of one 64-bit word; per character a mask of the tokens that consume it; `any-run` keeps its own
// bit; the zero-width moves over runs of skippable tokens (`*`, `?`) are closed by ONE addition: adding the active
// skippable bits to the skippable mask carries through each run of ones up to the first state behind it (close_over).
// The bound: one add and three logic operations per character whatever the run lengths, against up to 63 shift-or
// rounds.  step() is what label_match_kernel and the host loop (engine 1) both call.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/world_mi355.h"

#if defined(__HIPCC__)
#define WM_LP_HD __host__ __device__
#else
#define WM_LP_HD
#endif

namespace wm {
namespace labelpat {

constexpr int kMaxTokens = 63;
constexpr int kMaxName = 1023;
constexpr int kFirstChar = 0x21, kLastChar = 0x7E;
constexpr int kChars = kLastChar - kFirstChar + 1;
constexpr int64_t kMaxSpan = (int64_t)1 << 20;                  // max - min: see the float32 argument in DESIGN.md

enum TokenKind { kLiteral = 0, kAnyOne = 1, kOptAny = 2, kAnyRun = 3, kNumber = 4 };
struct Token {
  uint8_t kind, byte;
};
typedef std::vector<Token> Alternative;

// ---- the shared step ------------------------------------------------------------------------------------------------
// d | every state reachable from an active state through skippable tokens: within a run of ones of `skip` the addition
// clears the bits from the lowest active one upwards and sets the bit behind the run; the changed bits are the closure.
WM_LP_HD inline uint64_t close_over(uint64_t d, uint64_t skip) { return d | ((skip + (d & skip)) ^ skip); }
// one character: `consumes` is the character's mask (literals that equal it, any-one, optional-any), `run` the any-run bits
WM_LP_HD inline uint64_t step(uint64_t d, uint64_t consumes, uint64_t run, uint64_t skip) {
  return close_over(((d & consumes) << 1) | (d & run), skip);
}

// makefeature.pl:442-454 and the output's float32: below min 0, above max 1 (*clamped set: the script's "Out of range"
// warning), else one rounding of the double quotient (equal to the script's text round trip for
// max - min <= 2^20)
WM_LP_HD inline float normalise(int64_t v, int min, int max, int* clamped) {
  if (v < (int64_t)min) {
    *clamped = 1;
    return 0.0f;
  }
  if (v > (int64_t)max) {
    *clamped = 1;
    return 1.0f;
  }
  return (float)((double)(v - (int64_t)min) / (double)((int64_t)max - (int64_t)min));
}

// ---- compiler ---------------------------------------------------------------------------------------------------------
inline bool byte_ok(unsigned char c) { return c >= kFirstChar && c <= kLastChar; }

// WM_OK, or WM_ERR_UNSUPPORTED with *why set.  A float pattern is one alternative; its `%d` count and commas are the
// caller's to check (compile_pattern below).
inline int compile_alternative(const char* s, size_t n, bool is_float, Alternative& out, const char** why) {
  out.clear();
  for (size_t i = 0; i < n; ++i) {
    const unsigned char c = (unsigned char)s[i];
    if (!byte_ok(c)) {
      *why = "a pattern byte outside 0x21-0x7E";
      return WM_ERR_UNSUPPORTED;
    }
    if (c == '\\' || c == '(' || c == ')' || c == '{' || c == '}') {
      *why = "a pattern holds one of \\ ( ) { }, which the script leaves active as regex syntax";
      return WM_ERR_UNSUPPORTED;
    }
    Token t;
    t.byte = c;
    if (c == '*') t.kind = kAnyRun;
    else if (c == '?') t.kind = kOptAny;
    else if (c == '.') t.kind = kAnyOne;
    else if (is_float && c == '%' && i + 1 < n && s[i + 1] == 'd') {
      t.kind = kNumber;
      ++i;
    } else t.kind = kLiteral;
    out.push_back(t);
    if ((int)out.size() > kMaxTokens) {
      *why = "an alternative of more than 63 tokens";
      return WM_ERR_UNSUPPORTED;
    }
  }
  return WM_OK;
}

// The text between the braces -> alternatives (a float pattern: exactly one, with exactly one number token).
inline int compile_pattern(const char* pattern, bool is_float, std::vector<Alternative>& out, const char** why) {
  out.clear();
  if (pattern == nullptr) {
    *why = "a NULL pattern";
    return WM_ERR_BAD_ARG;
  }
  const size_t n = strlen(pattern);
  if (is_float) {
    Alternative a;
    if (const int rc = compile_alternative(pattern, n, true, a, why)) return rc;
    int numbers = 0;
    for (const Token& t : a) numbers += t.kind == kNumber ? 1 : 0;
    if (numbers != 1 || memchr(pattern, ',', n) != nullptr) {       // the script dies at :152-160
      *why = "a float pattern needs exactly one %d and no comma";
      return WM_ERR_BAD_ARG;
    }
    out.push_back(a);
    return WM_OK;
  }
  size_t from = 0;
  for (size_t i = 0; i <= n; ++i) {
    if (i < n && pattern[i] != ',') continue;
    Alternative a;
    if (const int rc = compile_alternative(pattern + from, i - from, false, a, why)) return rc;
    out.push_back(a);
    from = i + 1;
  }
  return WM_OK;
}

// A label name as the stage takes it (the state suffix already cut): 1 .. 1023 bytes of 0x21-0x7E.
inline int check_name(const char* name, const char** why) {
  if (name == nullptr || name[0] == 0) {
    *why = "a NULL or empty label name";
    return WM_ERR_BAD_ARG;
  }
  const size_t n = strnlen(name, (size_t)kMaxName + 1);
  if (n > (size_t)kMaxName) {
    *why = "a label name longer than 1023 bytes";
    return WM_ERR_UNSUPPORTED;
  }
  for (size_t i = 0; i < n; ++i)
    if (!byte_ok((unsigned char)name[i])) {
      *why = "a label name byte outside 0x21-0x7E";
      return WM_ERR_UNSUPPORTED;
    }
  return WM_OK;
}

// ---- the backtracking matcher ---------------------------------------------------------------------------------------
struct Backtrack {
  const Token* tok;
  int n_tok;
  const unsigned char* s;
  int n;
  std::vector<uint8_t> failed;                        // [(n_tok + 1) x (n + 1)]
  int cap_from = -1, cap_to = -1;
  bool at(int ti, int si) {
    if (ti == n_tok) return si == n;
    uint8_t& f = failed[(size_t)ti * (size_t)(n + 1) + (size_t)si];
    if (f) return false;
    bool ok = false;
    const Token t = tok[ti];
    switch (t.kind) {
      case kLiteral: ok = si < n && s[si] == t.byte && at(ti + 1, si + 1); break;
      case kAnyOne: ok = si < n && at(ti + 1, si + 1); break;
      case kOptAny: ok = (si < n && at(ti + 1, si + 1)) || at(ti + 1, si); break;
      case kAnyRun:
        for (int k = n; k >= si && !ok; --k) ok = at(ti + 1, k);
        break;
      default: {                                      // [+-]?[0-9]+ : a sign in front must be taken, the digits greedy
        int p = si;
        if (p < n && (s[p] == '+' || s[p] == '-')) ++p;
        int d = 0;
        while (p + d < n && s[p + d] >= '0' && s[p + d] <= '9') ++d;
        for (int len = d; len >= 1 && !ok; --len)
          if (at(ti + 1, p + len)) {
            ok = true;
            cap_from = si;
            cap_to = p + len;
          }
      }
    }
    if (!ok) f = 1;
    return ok;
  }
};

// The captured text as an integer; more digits than an int holds saturate (the script goes on in double there; a
// saturated value is clamped by normalise() as the script's is, since max - min <= 2^20).
inline int capture_value(const unsigned char* s, int from, int to) {
  bool neg = false;
  int p = from;
  if (s[p] == '+' || s[p] == '-') neg = s[p++] == '-';
  int64_t v = 0;
  for (; p < to; ++p) {
    v = v * 10 + (s[p] - '0');
    if (v > (int64_t)1 << 40) v = (int64_t)1 << 40;
  }
  if (neg) v = -v;
  if (v > 2147483647) v = 2147483647;
  if (v < -2147483647 - 1) v = -2147483647 - 1;
  return (int)v;
}

inline bool match_backtrack(const Alternative& a, const char* name, size_t n, int* value) {
  Backtrack b;
  b.tok = a.data();
  b.n_tok = (int)a.size();
  b.s = (const unsigned char*)name;
  b.n = (int)n;
  b.failed.assign((size_t)(b.n_tok + 1) * (n + 1), 0);
  if (!b.at(0, 0)) return false;
  if (value != nullptr) *value = b.cap_from >= 0 ? capture_value(b.s, b.cap_from, b.cap_to) : 0;
  return true;
}

// ---- the bit-parallel program of a binary alternative -----------------------------------------------------------------
struct Program {
  uint64_t skip = 0, run = 0, accept = 0;
  uint64_t consumes[kChars];
};
inline void build_program(const Alternative& a, Program& p) {
  p.skip = p.run = 0;
  memset(p.consumes, 0, sizeof(p.consumes));
  for (size_t i = 0; i < a.size(); ++i) {
    const uint64_t bit = (uint64_t)1 << i;
    const Token t = a[i];
    if (t.kind == kAnyRun) {
      p.run |= bit;
      p.skip |= bit;
    } else if (t.kind == kLiteral) {
      p.consumes[t.byte - kFirstChar] |= bit;
    } else {                                          // any-one, optional-any
      for (int c = 0; c < kChars; ++c) p.consumes[c] |= bit;
      if (t.kind == kOptAny) p.skip |= bit;
    }
  }
  p.accept = (uint64_t)1 << a.size();
}
inline bool match_program(const Program& p, const char* name, size_t n) {
  uint64_t d = close_over(1, p.skip);
  for (size_t i = 0; i < n; ++i) d = step(d, p.consumes[(unsigned char)name[i] - kFirstChar], p.run, p.skip);
  return (d & p.accept) != 0;
}

// ---- a compiled config ----------------------------------------------------------------------------------------------
struct Feature {
  int kind = 0, min = 0, max = 0;
  int index = 0;                                      // among the binary features, or among the float ones
  int first_alt = 0, n_alt = 0;                       // binary: its alternatives in FeatureSet::alts
  Alternative number;                                 // float: its one alternative
};
struct FeatureSet {
  std::vector<Feature> features;
  std::vector<Alternative> alts;                      // every binary feature's, one feature's side by side
  std::vector<int> alt_feature;                       // the binary index of an alternative's feature
  int n_binary = 0, n_float = 0;
};

inline int compile_feature_set(int n_features, const WorldMi355LabelFeature* f, FeatureSet& out, const char** why) {
  if (n_features < 1 || f == nullptr) {
    *why = "no features";
    return WM_ERR_BAD_ARG;
  }
  out = FeatureSet();
  for (int k = 0; k < n_features; ++k) {
    Feature ft;
    ft.kind = f[k].kind;
    ft.min = f[k].min;
    ft.max = f[k].max;
    if (ft.kind < 0 || ft.kind > 7) {
      *why = "a feature kind outside 0 .. 7";
      return WM_ERR_BAD_ARG;
    }
    std::vector<Alternative> alts;
    if (ft.kind <= 1)
      if (const int rc = compile_pattern(f[k].pattern, ft.kind == 1, alts, why)) return rc;
    if (ft.kind >= 1) {
      if ((int64_t)ft.max <= (int64_t)ft.min) {
        *why = "max <= min";
        return WM_ERR_BAD_ARG;
      }
      if ((int64_t)ft.max - (int64_t)ft.min > kMaxSpan) {
        *why = "max - min above 2^20";
        return WM_ERR_BAD_ARG;
      }
    }
    if (ft.kind == 0) {
      ft.index = out.n_binary++;
      ft.first_alt = (int)out.alts.size();
      ft.n_alt = (int)alts.size();
      for (Alternative& a : alts) {
        out.alts.push_back(a);
        out.alt_feature.push_back(ft.index);
      }
    } else if (ft.kind == 1) {
      ft.index = out.n_float++;
      ft.number = alts[0];
    }
    out.features.push_back(ft);
  }
  return WM_OK;
}

// The float features of one name, in the set's float order; returns 1 when a value was clamped.
inline int float_features(const FeatureSet& set, const char* name, size_t n, float* out) {
  int clamped = 0;
  for (const Feature& ft : set.features) {
    if (ft.kind != 1) continue;
    int v = 0;
    out[ft.index] = match_backtrack(ft.number, name, n, &v) ? normalise(v, ft.min, ft.max, &clamped) : 0.0f;
  }
  return clamped;
}

}  // namespace labelpat
}  // namespace wm
