// acl_main.cpp -- emqx_amd/csrc/gm_acl_match.h alone on the CPU (no HIP, no kernel, no C-ABI),
// built with ASan + UBSan by tests/test_acl_cpu.py: the list compiler (acl_rule_header,
// acl_compile_filter, rs_append), the client derivation (acl_client) and, per (request, record),
// the token predicates (acl_match_action, acl_match_who_tokens, acl_match_tokens,
// acl_needs_confirm) and the byte checks (acl_match_bytes, who-string equality), walked the way
// gm_acl.inc's lane walks the stream but over the whole stream at once, tiles' padding included.
//
//   acl_main INPUT          (acl_input.h)
// Output: one line per request, the first matching rule or "-", then
//   "STATS <filters> <tiles> <filters> <rules> <candidates> <removed> <deep names> <visited>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../emqx_amd/csrc/gm_acl_match.h"
#include "acl_input.h"

using namespace gm;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  AclInput in;
  if (!acl_read_input(argv[1], in)) return 2;
  const uint64_t mask = rs_test_mask(in.hash_bits);
  const uint32_t nfil = (uint32_t)in.ff.size();
  AclExact<uint8_t> fb(in.fb), wb(in.wb), nb(in.nb), cb(in.cb), ub(in.ub);

  std::vector<uint64_t> recs;
  uint32_t i = 0;
  for (uint32_t r = 0; r < in.n_rules; ++r) {
    uint64_t rec[ACL_FILTER_HDR + RS_MAX_LEVELS];
    const bool str = in.who[r] == ACL_WHO_USERNAME || in.who[r] == ACL_WHO_CLIENTID;
    rec[0] = acl_rule_header(in.perm[r], in.action[r], in.who[r], in.who[r] == ACL_WHO_HOST ? in.slot[r] : 0, r);
    rec[1] = str ? acl_value_token(wb.p + in.wo[r], in.wo[r + 1] - in.wo[r], mask) : 0;
    rs_append(recs, rec, ACL_RULE_WORDS);
    for (; i < nfil && in.fr[i] == r; ++i) {
      const uint32_t nw =
          acl_compile_filter(fb.p + in.fo[i], in.fo[i + 1] - in.fo[i], in.ff[i] == RS_F_EQ, r, i, mask, rec);
      if (nw < ACL_FILTER_HDR || nw > ACL_FILTER_HDR + RS_MAX_LEVELS || acl_step(rec[0]) != nw) return 3;
      rs_append(recs, rec, nw);
    }
  }
  AclExact<uint64_t> stream(recs);
  const uint32_t total = (uint32_t)recs.size();

  uint64_t cand = 0, removed = 0, deep_names = 0, visited = 0;
  std::vector<uint32_t> out(in.n, NONE);
  for (uint32_t t = 0; t < in.n; ++t) {
    const uint8_t* T = nb.p + in.no[t];
    const uint32_t tl = in.no[t + 1] - in.no[t], ci = in.client[t];
    if (ci >= in.n_clients) return 3;
    const uint8_t *C = cb.p + in.co[ci], *U = ub.p + in.uo[ci];
    const uint32_t cl = in.co[ci + 1] - in.co[ci], ul = in.uo[ci + 1] - in.uo[ci];
    const AclClient c = acl_client(C, cl, U, ul, in.cf[ci], mask);
    uint64_t tok[RS_MAX_LEVELS];
    uint32_t hw = 0;
    const uint32_t nl = rs_tokenize(T, tl, mask, RS_MAX_LEVELS, [&](uint32_t lv, uint64_t tk, uint32_t at, uint32_t len) {
      tok[lv] = tk;
      if (len == 1 && T[at] == '#') hw |= 1u << lv;
    });
    const bool deep = nl > RS_MAX_LEVELS;
    deep_names += deep;
    bool live = false;
    for (uint32_t tile = 0; tile < rs_n_tiles(total) && out[t] == NONE; ++tile) {
      const uint32_t span = rs_tile_span(tile, total);
      const uint64_t* S = stream.p + (size_t)tile * RS_TILE_WORDS;
      for (uint32_t p = 0; p < span && S[p] != RS_END;) {
        const uint64_t w0 = S[p];
        const uint32_t step = acl_step(w0);
        if (p + step > span) return 3;  // a record straddles a tile
        ++visited;
        if (acl_is_rule(w0)) {
          bool confirm = false;
          live = acl_match_action(acl_action(w0), in.req_action[t]) &&
                 acl_match_who_tokens(w0, S[p + 1], c, in.wbits[ci], &confirm);
          if (live && confirm) {
            ++cand;
            const uint32_t r = acl_rule(w0), wl = in.wo[r + 1] - in.wo[r];
            const bool usr = acl_who(w0) == ACL_WHO_USERNAME;
            live = wl == (usr ? ul : cl) && bytes_equal(wb.p + in.wo[r], usr ? U : C, wl);
            removed += !live;
          }
        } else if (live) {
          const uint64_t w1 = S[p + 1];
          bool ok = deep || acl_match_tokens(w0, w1, S + p + ACL_FILTER_HDR, nl, hw, c, [&](uint32_t l) { return tok[l]; });
          if (ok && (deep || acl_needs_confirm(w0, w1, c))) {
            ++cand;
            const uint32_t f = rs_filter(w0);
            ok = acl_match_bytes(T, tl, fb.p + in.fo[f], in.fo[f + 1] - in.fo[f], in.ff[f] == RS_F_EQ, C, cl, U, ul, c.flags);
            removed += !ok;
          }
          if (ok) {
            out[t] = rs_rule(w0);
            break;
          }
        }
        p += step;
      }
    }
  }
  for (uint32_t t = 0; t < in.n; ++t) {
    if (out[t] == NONE)
      puts("-");
    else
      printf("%u\n", out[t]);
  }
  printf("STATS %u %u %u %u %llu %llu %llu %llu\n", nfil, rs_n_tiles(total), nfil, in.n_rules,
         (unsigned long long)cand, (unsigned long long)removed, (unsigned long long)deep_names,
         (unsigned long long)visited);
  return 0;
}
