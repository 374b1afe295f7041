// labelpat.cpp -- the host-only probe of the label pattern layer (labelpat.hpp): one pattern against one name, by either
// engine.  No context, no HIP call: a caller can try a config with it, and the CPU tests drive both engines through it.
// Its own translation unit, like fileio.cpp; nothing else in the library refers to it (the layer itself is inline in
// the header, which ffi.hip includes).
#include "labelpat.hpp"

namespace wm {
void set_error(const char* msg);
}

extern "C" int WorldMi355LabelPatternMatch(const char* pattern, int is_float, const char* name, int engine, int* matched,
                                           int* value) {
  using namespace wm::labelpat;
  const char* why = "";
  if (matched == nullptr || engine < 0 || engine > 1 || (engine == 1 && is_float)) {
    wm::set_error("LabelPatternMatch: a NULL result, an engine other than 0 / 1, or a float pattern for engine 1");
    return WM_ERR_BAD_ARG;
  }
  *matched = 0;
  if (value != nullptr) *value = 0;
  std::vector<Alternative> alts;
  int rc = compile_pattern(pattern, is_float != 0, alts, &why);
  if (!rc) rc = check_name(name, &why);
  if (rc) {
    wm::set_error((std::string("LabelPatternMatch: ") + why).c_str());
    return rc;
  }
  const size_t n = strlen(name);
  for (const Alternative& a : alts) {                // makefeature.pl:352-362: the first alternative that matches decides
    bool hit;
    if (engine == 0) {
      int v = 0;
      hit = match_backtrack(a, name, n, &v);
      if (hit && value != nullptr) *value = v;
    } else {
      Program p;
      build_program(a, p);
      hit = match_program(p, name, n);
    }
    if (hit) {
      *matched = 1;
      break;
    }
  }
  return WM_OK;
}
