// The host-only pattern layer of the product (csrc/labelpat.hpp, csrc/labelpat.cpp: no HIP) under AddressSanitizer +
// UndefinedBehaviorSanitizer: tests/test_label_features_sanitized.py compiles this file together with labelpat.cpp by
// g++ and runs it.  argv[1] is a text file of "pattern<TAB>name<TAB>is_float<TAB>matched<TAB>value" lines (the
// fixture's patterns and names with the verdicts of the Python restatement): both engines must give them.  Then
// malformed patterns and names: every one refused with the expected code, none read out of bounds; the longest name
// and the longest alternative; a feature set compiled, its float features evaluated, its refusals.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "labelpat.hpp"

namespace wm {
static std::string g_msg;
void set_error(const char* msg) { g_msg = msg; }
}  // namespace wm

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, wm::g_msg.c_str()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static int probe(const std::string& patt, int is_float, const std::string& name, int engine, int* matched, int* value) {
  // exact-size heap copies: a read past either end is a report
  char* p = (char*)malloc(patt.size() + 1);
  char* n = (char*)malloc(name.size() + 1);
  memcpy(p, patt.c_str(), patt.size() + 1);
  memcpy(n, name.c_str(), name.size() + 1);
  const int rc = WorldMi355LabelPatternMatch(p, is_float, n, engine, matched, value);
  free(p);
  free(n);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<char> line(1 << 16);
  int cases = 0;
  while (fgets(line.data(), (int)line.size(), f)) {
    std::vector<std::string> field(1);
    for (const char* c = line.data(); *c && *c != '\n'; ++c) {
      if (*c == '\t') field.emplace_back();
      else field.back().push_back(*c);
    }
    CHECK(field.size() == 5);
    const int is_float = atoi(field[2].c_str()), want = atoi(field[3].c_str()), want_value = atoi(field[4].c_str());
    int m = -1, v = -1;
    CHECK(probe(field[0], is_float, field[1], 0, &m, &v) == WM_OK);
    CHECK(m == want && v == want_value);
    if (!is_float) {
      CHECK(probe(field[0], 0, field[1], 1, &m, &v) == WM_OK);
      CHECK(m == want && v == 0);
    }
    ++cases;
  }
  fclose(f);
  CHECK(cases > 1000);

  int m = 0, v = 0;
  const char* bad_patterns[] = {"a\\", "\\", "(", "a)", "{", "}", " ", "a\x01", "\x7f", "\xff*", "%d\\"};
  for (const char* p : bad_patterns)
    for (int engine = 0; engine < 2; ++engine) CHECK(probe(p, 0, "name", engine, &m, &v) == WM_ERR_UNSUPPORTED);
  CHECK(probe(std::string(64, '*'), 0, "a", 0, &m, &v) == WM_ERR_UNSUPPORTED);
  CHECK(probe(std::string(63, '*'), 0, "a", 1, &m, &v) == WM_OK && m == 1);
  CHECK(probe(std::string(63, '?') + ",a", 0, "a", 1, &m, &v) == WM_OK && m == 1);
  CHECK(probe("a," + std::string(64, 'a'), 0, "a", 0, &m, &v) == WM_ERR_UNSUPPORTED);   // refused before anything runs
  CHECK(probe("*", 0, std::string(1024, 'a'), 0, &m, &v) == WM_ERR_UNSUPPORTED);
  CHECK(probe("*", 0, "a b", 1, &m, &v) == WM_ERR_UNSUPPORTED);
  CHECK(probe("*", 0, "", 0, &m, &v) == WM_ERR_BAD_ARG);
  CHECK(WorldMi355LabelPatternMatch(nullptr, 0, "a", 0, &m, &v) == WM_ERR_BAD_ARG);
  CHECK(WorldMi355LabelPatternMatch("a", 0, nullptr, 0, &m, &v) == WM_ERR_BAD_ARG);
  CHECK(WorldMi355LabelPatternMatch("a", 0, "a", 0, nullptr, &v) == WM_ERR_BAD_ARG);
  CHECK(WorldMi355LabelPatternMatch("a", 0, "a", 0, &m, nullptr) == WM_OK && m == 1);
  CHECK(probe("a", 0, "a", 2, &m, &v) == WM_ERR_BAD_ARG && probe("a", 0, "a", -1, &m, &v) == WM_ERR_BAD_ARG);
  CHECK(probe("%d", 1, "5", 1, &m, &v) == WM_ERR_BAD_ARG);
  CHECK(probe("a", 1, "a", 0, &m, &v) == WM_ERR_BAD_ARG && probe("%d%d", 1, "11", 0, &m, &v) == WM_ERR_BAD_ARG);
  CHECK(probe("%d,", 1, "1", 0, &m, &v) == WM_ERR_BAD_ARG);
  CHECK(probe("%", 1, "%", 0, &m, &v) == WM_ERR_BAD_ARG);                               // a lone % at the end is a literal
  // the longest name against the worst patterns: remembered failures keep it polynomial
  const std::string longest = std::string(500, 'a') + std::string(523, 'b');
  std::string stars;
  for (int i = 0; i < 31; ++i) stars += "*a";
  CHECK(probe(stars + "*", 0, longest, 0, &m, &v) == WM_OK && m == 1);
  CHECK(probe(stars + "c", 0, longest, 0, &m, &v) == WM_OK && m == 0);
  CHECK(probe(stars + "c", 0, longest, 1, &m, &v) == WM_OK && m == 0);
  CHECK(probe(std::string(31, '?') + "*" + std::string(31, '?'), 0, longest, 1, &m, &v) == WM_OK && m == 1);
  CHECK(probe("*b%d", 1, longest + "-2147483648", 0, &m, &v) == WM_ERR_UNSUPPORTED);    // 1034 bytes
  CHECK(probe("*b%d", 1, longest.substr(0, 1012) + "-2147483648", 0, &m, &v) == WM_OK && m == 1 && v == -2147483647 - 1);
  CHECK(probe("*b%d", 1, longest.substr(0, 1003) + "99999999999999999999", 0, &m, &v) == WM_OK && v == 2147483647);
  CHECK(probe("*b%d", 1, longest.substr(0, 1003) + "-9999999999999999999", 0, &m, &v) == WM_OK && v == -2147483647 - 1);

  // a feature set: compile, evaluate, refuse
  using namespace wm::labelpat;
  const char* why = "";
  FeatureSet set;
  const WorldMi355LabelFeature ok[] = {{0, "*-a+*,,*-b+*", 0, 0}, {1, "*_%d", -3, 7}, {4, nullptr, 1, 5}, {0, "", 0, 0},
                                       {1, "*:%d?", 0, 1 << 20}, {7, nullptr, -5, 5}};
  CHECK(compile_feature_set(6, ok, set, &why) == WM_OK);
  CHECK(set.n_binary == 2 && set.n_float == 2 && set.alts.size() == 4 && set.features[3].n_alt == 1);
  float out[2] = {-1.0f, -1.0f};
  CHECK(float_features(set, "x-a+y:12_2", 10, out) == 0 && out[0] == 0.5f && out[1] == 0.0f);
  CHECK(float_features(set, "x:1048576", 9, out) == 0 && out[0] == 0.0f && out[1] == 1.0f);
  CHECK(float_features(set, "x:1048577_8", 11, out) == 1 && out[0] == 1.0f && out[1] == 0.0f);
  CHECK(float_features(set, "x:3_-4", 6, out) == 1 && out[0] == 0.0f);
  int clamped = 0;
  CHECK(normalise(-2147483647 - 1, 2147483647 - 5, 2147483647, &clamped) == 0.0f && clamped == 1);
  const WorldMi355LabelFeature bad[] = {{8, "a", 0, 1},        {-1, "a", 0, 1},          {0, nullptr, 0, 0},  {1, "%d", 3, 3},
                                        {1, "%d", 4, 3},       {5, nullptr, 0, 0},       {1, "%d", 0, (1 << 20) + 1},
                                        {2, nullptr, -2147483647 - 1, 2147483647}};
  for (const WorldMi355LabelFeature& b : bad) CHECK(compile_feature_set(1, &b, set, &why) == WM_ERR_BAD_ARG);
  const WorldMi355LabelFeature unsupported[] = {{0, "a(b", 0, 0}, {1, "a{%d", 0, 1}, {0, "a b", 0, 0}};
  for (const WorldMi355LabelFeature& b : unsupported) CHECK(compile_feature_set(1, &b, set, &why) == WM_ERR_UNSUPPORTED);
  CHECK(compile_feature_set(0, ok, set, &why) == WM_ERR_BAD_ARG && compile_feature_set(1, nullptr, set, &why) == WM_ERR_BAD_ARG);
  printf("labelpat ok: %d cases\n", cases);
  return 0;
}
