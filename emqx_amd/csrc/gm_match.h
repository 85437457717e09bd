// gm_match.h -- emqx_topic:match/2 on raw bytes, shared by the gfx950 kernels (k_verify,
// k_verify_scatter, k_rules) and the CPU harness that pins it to the oracle
// (tests/host_harness/match2_main.cpp, tests/test_match2_cpu.py).
#pragma once
#include "gm_common.h"

namespace gm {

template <class PA, class PB>
GM_HD bool bytes_equal(PA a, PB b, uint32_t len) {
  for (uint32_t i = 0; i < len; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// emqx_topic:match/2 (emqx_topic.erl:67-89) on raw bytes.  T and F are byte accessors over LDS
// or global memory.  A '+'/'#' word of T is compared literally, as match/2 does for wildcard
// names.  DOLLAR: the binary clauses (:70-73, a '$' name never matches a root wildcard); false
// for match/2 called on word lists, which skips them (emqx_authz_rule.erl:213-214).
template <bool DOLLAR = true, class PT, class PF>
GM_HD bool mqtt_match(PT T, uint32_t tl, PF F, uint32_t fl) {
  if (DOLLAR && tl > 0 && T[0] == '$' && fl > 0 && (F[0] == '+' || F[0] == '#')) return false;
  uint32_t i = 0, j = 0;  // start of the current topic / filter word
  for (;;) {
    uint32_t je = j;
    while (je < fl && F[je] != '/') ++je;
    const bool flast = (je == fl);
    const uint32_t flen = je - j;
    const bool fplus = (flen == 1 && F[j] == '+');
    const bool fhash = (flen == 1 && F[j] == '#');
    if (fhash && flast) {
      // match([H | T1], [H | T2]) (:78) is tried before match(_, ['#']) (:82): a word of T that
      // is itself '#' is taken as the equal word, and then T has to end with it
      if (i < tl && T[i] == '#' && (i + 1 == tl || T[i + 1] == '/')) return i + 1 == tl;
      return true;  // match(_, ['#']) -> true
    }
    if (i > tl) return false;         // match([], [_|_]) -> false
    uint32_t ie = i;
    while (ie < tl && T[ie] != '/') ++ie;
    bool eq = fplus;
    if (!eq && flen == ie - i) {
      eq = true;
      for (uint32_t q = 0; q < flen; ++q)
        if (T[i + q] != F[j + q]) {
          eq = false;
          break;
        }
    }
    if (!eq) return false;
    i = ie + 1;
    j = je + 1;
    if (flast) return i > tl;  // match([], []) -> true ; match([_|_], []) -> false
  }
}

}  // namespace gm
