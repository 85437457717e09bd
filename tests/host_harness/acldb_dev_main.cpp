// acldb_dev_main.cpp -- the CPU gate of the built-in database's device path (DESIGN.md 6b
// "Built-in database"), built with ASan + UBSan by tests/test_acldb_dev_host.py: every line of
// k_acldb's device code (emqx_amd/csrc/gm_acldb.inc, included unchanged behind hip_shim.h) and
// every byte of host code that sizes or addresses a device buffer (emqx_amd/csrc/gm_acldb.cpp,
// included with GM_ACLDB_EXACT_ALLOC on the fake HIP runtime, so each "device" array is a malloc
// of exactly the bytes in use and an access one byte past it hits a redzone) runs here before it
// runs on a GPU.  launch_acldb runs a block the way the kernel body does: each phase function for
// lanes 0 .. WG - 1 in turn, phase by phase, which is what the __syncthreads() between them
// guarantee; the two LDS arrays are heap blocks of their exact size.  Everything is driven
// through the C-ABI.
//
//   acldb_dev_main INPUT
// INPUT (text; byte strings in hex, "-" = empty) is the script of tests/acldb_cases.py:
//   hash_bits pass_names            (pass_names 0: the default)
//   n_clients, then per client "flags clientid username"
//   then operations until "E":
//     S kind key n_rules            emqxgm_acldb_store; then per rule "perm action filter"
//     M n_records                   emqxgm_acldb_store_many; per record "kind key n_rules" and its rules
//     D kind key | P | C            delete, purge, commit
//     T key value                   emqxgm_acldb_tune
//     R                             the refused calls, each of which must return -EINVAL
//     Q n                           emqxgm_acldb_match of n requests "client action name"
// Output per Q: one line per request, "perm src pos" or "-", then "STATS <the 18 values of
// emqxgm_acldb_stats>" and "COUNT <emqxgm_acldb_count>".
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "hip_shim.h"
#include "ruleset_shim.h"

#include "../../emqx_amd/csrc/gm_acldb_match.h"
#include "../../emqx_amd/csrc/gm_kernels.h"
#include "acl_input.h"

namespace gm {
namespace {
#include "../../emqx_amd/csrc/gm_acldb.inc"

#define ALL_LANES for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)

// k_acldb's body for block b, the barriers turned into "every lane, then the next phase"
void run_block(const AclDbArgs& A, uint32_t b) {
  std::unique_ptr<uint64_t[]> tok(new uint64_t[RS_MAX_LEVELS * WG]);
  std::unique_ptr<uint64_t[]> tile(new uint64_t[RS_TILE_WORDS]);
  memset(tok.get(), 0xA5, sizeof(uint64_t) * RS_MAX_LEVELS * WG);  // LDS starts undefined
  memset(tile.get(), 0xA5, sizeof(uint64_t) * RS_TILE_WORDS);
  uint64_t *s_tok = tok.get(), *s_tile = tile.get();
  std::vector<AdbLane> L(WG);
  blockIdx.x = b;
  ALL_LANES adb_ph_tokenize(A, L[threadIdx.x], s_tok);
  ALL_LANES adb_ph_lookup(A, L[threadIdx.x], s_tok, ADB_CLIENTID);
  ALL_LANES adb_ph_lookup(A, L[threadIdx.x], s_tok, ADB_USERNAME);
  const uint32_t tiles = rs_n_tiles(A.all_words);
  for (uint32_t k = 0; k < tiles; ++k) {
    if (rs_tile_span(k, A.all_words) == 0) abort();
    ALL_LANES adb_ph_stage(A, k, s_tile);
    ALL_LANES adb_ph_walk(A, L[threadIdx.x], s_tok, s_tile);
  }
  ALL_LANES adb_ph_finish(A, L[threadIdx.x], s_tok);
  ALL_LANES adb_ph_counters(A, s_tok);
}
}  // namespace

hipError_t launch_acldb(const AclDbArgs& a, hipStream_t) {
  if (a.n == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((uint64_t)a.n + WG - 1) / WG);
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; ++b) run_block(a, b);
  return hipSuccess;
}
}  // namespace gm

#define GM_ACLDB_EXACT_ALLOC 1
#include "../../emqx_amd/csrc/gm_acldb.cpp"

#define CHECK(c, what)                       \
  do {                                       \
    if (!(c)) {                              \
      fprintf(stderr, "FAILED: %s\n", what); \
      return 1;                              \
    }                                        \
  } while (0)

namespace {

// The rules of one or more records in the C-ABI's packed form.
struct Rules {
  std::vector<uint32_t> perm, action, fo{0};
  std::vector<uint8_t> fb;
  void read(std::ifstream& f, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) {
      uint32_t p, a;
      std::string hex;
      f >> p >> a >> hex;
      perm.push_back(p);
      action.push_back(a);
      acl_unhex(hex, fb, fo);
    }
  }
};

std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> b;
  std::vector<uint32_t> o;
  acl_unhex(h, b, o);
  return b;
}

// The refused calls; the database in force and what is pending stay as they are.
int refused(emqxgm_acldb_t* h) {
  const uint8_t key[2] = {'k', 'k'};
  const uint8_t fb[3] = {'a', '/', 'b'};
  const uint32_t perm[2] = {1, 0}, action[2] = {1, 3}, fo[3] = {0, 1, 3};
  const uint32_t bad_perm[2] = {1, 2}, act0[2] = {0, 1}, act4[2] = {1, 4}, desc[3] = {0, 2, 1};
  CHECK(emqxgm_acldb_store(h, 3, key, 2, perm, action, fb, fo, 2) == -EINVAL, "unknown kind");
  CHECK(emqxgm_acldb_store(h, 0, key, 2, bad_perm, action, fb, fo, 2) == -EINVAL, "unknown permission");
  CHECK(emqxgm_acldb_store(h, 0, key, 2, perm, act0, fb, fo, 2) == -EINVAL, "action 0");
  CHECK(emqxgm_acldb_store(h, 1, key, 2, perm, act4, fb, fo, 2) == -EINVAL, "action 4");
  CHECK(emqxgm_acldb_store(h, 2, key, 2, perm, action, fb, desc, 2) == -EINVAL, "descending offsets");
  CHECK(emqxgm_acldb_store(h, 0, nullptr, 2, perm, action, fb, fo, 2) == -EINVAL, "no key bytes");
  CHECK(emqxgm_acldb_delete(h, 3, key, 2) == -EINVAL, "delete of an unknown kind");
  {
    const uint32_t n = 65537;
    std::vector<uint32_t> p(n, 1), a(n, 3), o(n + 1, 0);
    AclExact<uint32_t> pe(p), ae(a), oe(o);
    CHECK(emqxgm_acldb_store(h, 0, key, 2, pe.p, ae.p, nullptr, oe.p, n) == -EINVAL, "65,537 rules");
    const uint32_t kind[1] = {0}, ko[2] = {0, 2}, ro[2] = {0, n};
    CHECK(emqxgm_acldb_store_many(h, 1, kind, key, ko, ro, pe.p, ae.p, nullptr, oe.p) == -EINVAL,
          "65,537 rules in store_many");
  }
  {
    // the second record is bad: the first is not stored either
    const uint32_t kind[2] = {0, 3}, ko[3] = {0, 1, 2}, ro[3] = {0, 1, 2};
    CHECK(emqxgm_acldb_store_many(h, 2, kind, key, ko, ro, perm, action, fb, fo) == -EINVAL, "store_many is all or nothing");
  }
  const uint32_t no[2] = {0, 3}, co[2] = {0, 2}, uo[2] = {0, 0}, cf[1] = {0};
  uint32_t out[3] = {7, 7, 7};
  const uint32_t c1[1] = {1}, c0[1] = {0}, a1[1] = {1}, a3[1] = {3};
  CHECK(emqxgm_acldb_match(h, fb, no, 1, c1, a1, key, co, key, uo, cf, 1, out, out + 1, out + 2) == -EINVAL,
        "client index out of range");
  CHECK(emqxgm_acldb_match(h, fb, no, 1, c0, a3, key, co, key, uo, cf, 1, out, out + 1, out + 2) == -EINVAL,
        "request action all");
  CHECK(out[0] == 7 && out[1] == 7 && out[2] == 7, "a refused match writes nothing");
  CHECK(emqxgm_acldb_tune(h, "no_such_key", 1) == -EINVAL, "unknown tune key");
  CHECK(emqxgm_acldb_tune(h, "rebuild_load_pct", 51) == -EINVAL && emqxgm_acldb_tune(h, "rebuild_load_pct", 0) == -EINVAL,
        "load beyond 1/2");
  CHECK(emqxgm_acldb_tune(h, "rebuild_garbage_pct", 0) == -EINVAL, "garbage percent 0");
  CHECK(emqxgm_acldb_tune(h, "pass_names", 0) == -EINVAL, "pass_names 0");
  CHECK(emqxgm_acldb_match(h, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                           nullptr, nullptr, nullptr) == 0,
        "n == 0 with no clients");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  uint32_t hash_bits = 0, n_clients = 0;
  uint64_t pass_names = 0;
  f >> hash_bits >> pass_names >> n_clients;
  std::vector<uint8_t> cbv, ubv;
  std::vector<uint32_t> cov{0}, uov{0}, cfv;
  for (uint32_t c = 0; c < n_clients; ++c) {
    uint32_t flags;
    std::string cid, usr;
    f >> flags >> cid >> usr;
    cfv.push_back(flags);
    acl_unhex(cid, cbv, cov);
    acl_unhex(usr, ubv, uov);
  }
  if (!f) return 2;
  // exact-size copies of the inputs: the C-ABI must not read past what it is given
  AclExact<uint8_t> cb(cbv), ub(ubv);
  AclExact<uint32_t> co(cov), uo(uov), cf(cfv);

  emqxgm_acldb_t* h = nullptr;
  CHECK(emqxgm_acldb_create(0, hash_bits, &h) == 0, "create");
  CHECK(emqxgm_acldb_tune(h, "counters", 1) == 0, "tune counters");
  if (pass_names) CHECK(emqxgm_acldb_tune(h, "pass_names", (int64_t)pass_names) == 0, "tune pass_names");
  CHECK(emqxgm_acldb_tune(h, "timing", 1) == 0 && emqxgm_acldb_tune(h, "kernel_us", 0) == 0, "tune timing");

  std::string op;
  while (f >> op && op != "E") {
    if (op == "S") {
      uint32_t kind, n;
      std::string key;
      f >> kind >> key >> n;
      Rules r;
      r.read(f, n);
      const std::vector<uint8_t> kb = unhex(key);
      AclExact<uint8_t> ke(kb), fbe(r.fb);
      AclExact<uint32_t> pe(r.perm), ae(r.action), oe(r.fo);
      CHECK(emqxgm_acldb_store(h, kind, ke.p, (uint32_t)kb.size(), pe.p, ae.p, fbe.p, oe.p, n) == 0, "store");
    } else if (op == "M") {
      uint32_t nrec;
      f >> nrec;
      Rules r;
      std::vector<uint32_t> kind, kov{0}, rov{0};
      std::vector<uint8_t> kbv;
      for (uint32_t i = 0; i < nrec; ++i) {
        uint32_t k, n;
        std::string key;
        f >> k >> key >> n;
        kind.push_back(k);
        acl_unhex(key, kbv, kov);
        r.read(f, n);
        rov.push_back((uint32_t)r.perm.size());
      }
      AclExact<uint8_t> ke(kbv), fbe(r.fb);
      AclExact<uint32_t> kd(kind), ko(kov), ro(rov), pe(r.perm), ae(r.action), oe(r.fo);
      CHECK(emqxgm_acldb_store_many(h, nrec, kd.p, ke.p, ko.p, ro.p, pe.p, ae.p, fbe.p, oe.p) == 0, "store_many");
    } else if (op == "D") {
      uint32_t kind;
      std::string key;
      f >> kind >> key;
      const std::vector<uint8_t> kb = unhex(key);
      AclExact<uint8_t> ke(kb);
      CHECK(emqxgm_acldb_delete(h, kind, ke.p, (uint32_t)kb.size()) == 0, "delete");
    } else if (op == "P") {
      CHECK(emqxgm_acldb_purge(h) == 0, "purge");
    } else if (op == "C") {
      CHECK(emqxgm_acldb_commit(h) == 0, "commit");
    } else if (op == "T") {
      std::string key;
      long long v;
      f >> key >> v;
      CHECK(emqxgm_acldb_tune(h, key.c_str(), v) == 0, "tune");
    } else if (op == "R") {
      if (refused(h)) return 1;
    } else if (op == "Q") {
      uint32_t n;
      f >> n;
      std::vector<uint8_t> nbv;
      std::vector<uint32_t> nov{0}, clv, acv;
      for (uint32_t t = 0; t < n; ++t) {
        uint32_t c, a;
        std::string hex;
        f >> c >> a >> hex;
        clv.push_back(c);
        acv.push_back(a);
        acl_unhex(hex, nbv, nov);
      }
      AclExact<uint8_t> nb(nbv);
      AclExact<uint32_t> no(nov), cl(clv), ac(acv);
      std::vector<uint32_t> fill(n, 0xA5A5A5A5u);
      AclExact<uint32_t> op_(fill), os(fill), oq(fill);
      CHECK(emqxgm_acldb_match(h, nb.p, no.p, n, cl.p, ac.p, cb.p, co.p, ub.p, uo.p, cf.p, n_clients, op_.p, os.p,
                               oq.p) == 0,
            "match");
      for (uint32_t t = 0; t < n; ++t) {
        if (op_.p[t] == EMQXGM_NONE) {
          CHECK(os.p[t] == EMQXGM_NONE && oq.p[t] == EMQXGM_NONE, "nomatch has no source");
          puts("-");
        } else {
          printf("%u %u %u\n", op_.p[t], os.p[t], oq.p[t]);
        }
      }
      uint64_t st[20], count = 0;
      CHECK(emqxgm_acldb_stats(h, st) == 0 && emqxgm_acldb_count(h, &count) == 0, "stats");
      printf("STATS");
      for (int i = 0; i < 18; ++i) printf(" %llu", (unsigned long long)st[i]);
      printf("\nCOUNT %llu\n", (unsigned long long)count);
    } else {
      return 2;
    }
    if (!f) return 2;
  }
  CHECK(op == "E", "the script ends with E");
  emqxgm_acldb_destroy(h);
  return 0;
}
