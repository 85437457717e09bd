// acl_dev_main.cpp -- the CPU gate of the ACL device path (DESIGN.md 6b "ACL lists"), built with
// ASan + UBSan by tests/test_acl_dev_host.py: every line of k_acl's device code
// (emqx_amd/csrc/gm_acl.inc, included unchanged behind hip_shim.h) and every byte of host code
// that sizes or addresses a device buffer (emqx_amd/csrc/gm_acl.cpp, included with
// GM_ACL_EXACT_ALLOC on the fake HIP runtime, so each "device" array is a malloc of exactly the
// bytes in use and an access one byte past it hits a redzone) runs here before it runs on a GPU.
// launch_acl runs a block the way the kernel body does: each phase function for lanes
// 0 .. WG - 1 in turn, phase by phase, which is what the __syncthreads() between them guarantee;
// the two LDS arrays are heap blocks of their exact size.  Everything is driven through the C-ABI
// (emqxgm_acl_create / set / match / tune / stats).
//
//   acl_dev_main INPUT          (acl_input.h)
// Output: one line per request, the first matching rule or "-", then
//   "STATS <filters> <tiles> <filters> <rules> <candidates> <removed> <deep names> <visited>".
// After the match the program also checks that malformed sets (a slot of 64, an unknown kind,
// action, permission or flag, descending rule order, a rule out of range, too many rules) return
// -EINVAL and leave the answers as they were, and that a request with a client index out of
// range or an action other than publish or subscribe is refused with -EINVAL.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "hip_shim.h"
#include "ruleset_shim.h"

#include "../../emqx_amd/csrc/gm_acl_match.h"
#include "../../emqx_amd/csrc/gm_kernels.h"
#include "acl_input.h"

namespace gm {
namespace {
#include "../../emqx_amd/csrc/gm_acl.inc"

#define ALL_LANES for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)

// k_acl's body for block b, the barriers turned into "every lane, then the next phase"
void run_block(const AclArgs& A, uint32_t b) {
  std::unique_ptr<uint64_t[]> tok(new uint64_t[RS_MAX_LEVELS * WG]);
  std::unique_ptr<uint64_t[]> tile(new uint64_t[RS_TILE_WORDS]);
  memset(tok.get(), 0xA5, sizeof(uint64_t) * RS_MAX_LEVELS * WG);  // LDS starts undefined
  memset(tile.get(), 0xA5, sizeof(uint64_t) * RS_TILE_WORDS);
  uint64_t *s_tok = tok.get(), *s_tile = tile.get();
  std::vector<AclLane> L(WG);
  blockIdx.x = b;
  ALL_LANES acl_ph_tokenize(A, L[threadIdx.x], s_tok);
  const uint32_t tiles = rs_n_tiles(A.total_words);
  for (uint32_t k = 0; k < tiles; ++k) {
    if (rs_tile_span(k, A.total_words) == 0) abort();
    ALL_LANES acl_ph_stage(A, k, s_tile);
    ALL_LANES acl_ph_walk(A, L[threadIdx.x], s_tok, s_tile);
  }
  ALL_LANES acl_ph_finish(A, L[threadIdx.x], s_tile);
  ALL_LANES acl_ph_counters(A, s_tile);
}
}  // namespace

hipError_t launch_acl(const AclArgs& a, hipStream_t) {
  if (a.n == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((uint64_t)a.n + WG - 1) / WG);
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; ++b) run_block(a, b);
  return hipSuccess;
}
}  // namespace gm

#define GM_ACL_EXACT_ALLOC 1
#include "../../emqx_amd/csrc/gm_acl.cpp"

#define CHECK(c, what)                       \
  do {                                       \
    if (!(c)) {                              \
      fprintf(stderr, "FAILED: %s\n", what); \
      return 1;                              \
    }                                        \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  AclInput in;
  if (!acl_read_input(argv[1], in)) return 2;
  // exact-size copies of the inputs: the C-ABI must not read past what it is given
  AclExact<uint8_t> fb(in.fb), wb(in.wb), nb(in.nb), cb(in.cb), ub(in.ub);
  AclExact<uint32_t> fo(in.fo), ff(in.ff), fr(in.fr), perm(in.perm), action(in.action), who(in.who), slot(in.slot),
      wo(in.wo), co(in.co), uo(in.uo), cf(in.cf), no(in.no), client(in.client), ract(in.req_action);
  AclExact<uint64_t> wbits(in.wbits);
  const uint32_t nfil = (uint32_t)in.ff.size(), nr = in.n_rules, nc = in.n_clients, n = in.n;

  emqxgm_acl_t* h = nullptr;
  CHECK(emqxgm_acl_create(0, in.hash_bits, &h) == 0, "create");
  CHECK(emqxgm_acl_tune(h, "counters", 1) == 0, "tune counters");
  if (in.pass_names) CHECK(emqxgm_acl_tune(h, "pass_names", (int64_t)in.pass_names) == 0, "tune pass_names");
  CHECK(emqxgm_acl_tune(h, "no_such_key", 1) == -EINVAL, "unknown tune key");
  CHECK(emqxgm_acl_tune(h, "timing", 1) == 0 && emqxgm_acl_tune(h, "kernel_us", 0) == 0, "tune timing");
  auto match = [&](std::vector<uint32_t>& out) {
    out.assign(n, 0xA5A5A5A5u);
    AclExact<uint32_t> o(out);
    const int rc = emqxgm_acl_match(h, nb.p, no.p, n, client.p, ract.p, cb.p, co.p, ub.p, uo.p, cf.p, wbits.p, nc, o.p);
    for (uint32_t i = 0; i < n; ++i) out[i] = o.p[i];
    return rc;
  };
  auto set = [&](const uint32_t* ff_, const uint32_t* fr_, const uint32_t* perm_, const uint32_t* action_,
                 const uint32_t* who_, const uint32_t* slot_, uint32_t n_rules) {
    return emqxgm_acl_set(h, fb.p, fo.p, ff_, fr_, nfil, perm_, action_, who_, slot_, wb.p, wo.p, n_rules);
  };
  std::vector<uint32_t> none, rows, again;
  // before any set: the empty list
  CHECK(match(none) == 0, "match on the empty list");
  for (uint32_t v : none) CHECK(v == EMQXGM_NONE, "the empty list gives no match");
  CHECK(set(ff.p, fr.p, perm.p, action.p, who.p, slot.p, nr) == 0, "set");
  CHECK(match(rows) == 0, "match");
  uint64_t st[8];
  CHECK(emqxgm_acl_stats(h, st) == 0, "stats");

  // malformed lists: -EINVAL, and the list in force keeps answering
  if (nr >= 1) {
    auto bad_rule = [&](const std::vector<uint32_t>& base, uint32_t v, int which) {
      std::vector<uint32_t> b = base;
      b[0] = v;
      AclExact<uint32_t> x(b);
      return set(ff.p, fr.p, which == 0 ? x.p : perm.p, which == 1 ? x.p : action.p, which == 2 ? x.p : who.p,
                 which == 3 ? x.p : slot.p, nr);
    };
    CHECK(bad_rule(in.perm, 2, 0) == -EINVAL, "unknown permission");
    CHECK(bad_rule(in.action, 0, 1) == -EINVAL && bad_rule(in.action, 4, 1) == -EINVAL, "unknown action");
    CHECK(bad_rule(in.who, 4, 2) == -EINVAL, "unknown who kind");
    CHECK(bad_rule(in.slot, 64, 3) == -EINVAL, "slot 64");
  }
  if (nfil >= 1) {
    std::vector<uint32_t> b = in.fr;
    b[0] = nr;  // out of range
    AclExact<uint32_t> x(b);
    CHECK(set(ff.p, x.p, perm.p, action.p, who.p, slot.p, nr) == -EINVAL, "rule out of range");
    std::vector<uint32_t> bf = in.ff;
    bf[0] = 2;  // EMQXGM_RULE_WORDS is not a flag of an ACL filter
    AclExact<uint32_t> y(bf);
    CHECK(set(y.p, fr.p, perm.p, action.p, who.p, slot.p, nr) == -EINVAL, "unknown flag");
  }
  if (nfil >= 2 && in.fr[0] != in.fr[nfil - 1]) {
    std::vector<uint32_t> b(in.fr.rbegin(), in.fr.rend());  // descending
    AclExact<uint32_t> x(b);
    CHECK(set(ff.p, x.p, perm.p, action.p, who.p, slot.p, nr) == -EINVAL, "descending rule order");
  }
  CHECK(emqxgm_acl_set(h, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, 65537) == -EINVAL,
        "too many rules");
  if (n >= 1) {
    std::vector<uint32_t> b = in.client, out(n, 7u);
    b[n - 1] = nc;  // out of range
    AclExact<uint32_t> x(b), o(out);
    CHECK(emqxgm_acl_match(h, nb.p, no.p, n, x.p, ract.p, cb.p, co.p, ub.p, uo.p, cf.p, wbits.p, nc, o.p) == -EINVAL,
          "client index out of range");
    std::vector<uint32_t> a = in.req_action;
    a[n - 1] = 3;  // EMQXGM_ACL_ALL is a rule's action, not a request's
    AclExact<uint32_t> y(a);
    CHECK(emqxgm_acl_match(h, nb.p, no.p, n, client.p, y.p, cb.p, co.p, ub.p, uo.p, cf.p, wbits.p, nc, o.p) == -EINVAL,
          "request action all");
    for (uint32_t i = 0; i < n; ++i) CHECK(o.p[i] == 7u, "a refused match writes nothing");
  }
  CHECK(match(again) == 0, "match after refused sets");
  CHECK(again == rows, "a refused set leaves the answers as they were");
  CHECK(emqxgm_acl_match(h, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, 0, nullptr) == 0,
        "n == 0 with no clients");
  emqxgm_acl_destroy(h);

  for (uint32_t v : rows) {
    if (v == EMQXGM_NONE)
      puts("-");
    else
      printf("%u\n", v);
  }
  printf("STATS");
  for (uint64_t v : st) printf(" %llu", (unsigned long long)v);
  printf("\n");
  return 0;
}
