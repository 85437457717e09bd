// acldb_main.cpp -- emqx_amd/csrc/gm_acldb_match.h alone on the CPU (DESIGN.md 6b "Built-in
// database"), built with ASan + UBSan by tests/test_acldb_cpu.py: the probe, the run walk, the
// relative indices, and the malformed slots and runs that the C-ABI cannot build.  Every table,
// pool and offset array is a heap block of its exact size, so an index followed past one lands in
// a redzone.  The lookup phase of the kernel (gm_acldb.inc, included unchanged behind hip_shim.h)
// is run for single lanes where the contract is the phase's: a slot's key index is checked there.
//
//   acldb_main HASH_BITS KEY0 KEY1 KEY2 KEY3     (keys in hex: tests/acldb_cases.py chain_keys)
// Output, one line each, read by the test:
//   HOME h h h h            adb_home of the four keys in a table of ADB_MIN_SLOTS slots
//   SLOTS a b c d           the slots they took, stored in order (read back from the table)
//   FOUND a b c d / STEPS   each key's probe: the slot found and the slots looked at
//   DELETED s               key 1's slot after its delete, then FOUND / STEPS of keys 2 and 3
//   STATES ...              the table's slots: E empty, D deleted, 0..3 the key
//   AGAIN s                 the slot key 1 takes when stored again
//   WALK / BAD lines        see below
// Exit status 0 only when every check held.
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

#include "../../emqx_amd/csrc/gm_acldb_match.h"
#include "../../emqx_amd/csrc/gm_kernels.h"
#include "acl_input.h"

namespace gm {
namespace {
#include "../../emqx_amd/csrc/gm_acldb.inc"
}  // namespace
}  // namespace gm

using namespace gm;

#define CHECK(c, what)                       \
  do {                                       \
    if (!(c)) {                              \
      fprintf(stderr, "FAILED: %s\n", what); \
      return 1;                              \
    }                                        \
  } while (0)

namespace {

typedef std::vector<uint8_t> Bytes;

// The probe as the kernel's lookup phase does it: the next slot with the token, confirmed on the
// key's bytes when the token is hashed.  *steps: slots looked at; *hits: token hits.
uint32_t find(const AdbSlot* tab, uint64_t mask, uint64_t tok, const std::vector<Bytes>& keys, const Bytes& key,
              uint64_t* steps, uint32_t* hits) {
  uint64_t i = adb_home(tok, mask);
  uint32_t at;
  *steps = 0;
  *hits = 0;
  while ((at = adb_probe_next(tab, mask, tok, &i, steps)) != NONE) {
    ++*hits;
    if (!(tok & TOK_HASHED) || keys[tab[at].key] == key) break;
  }
  return at;
}

// Where an insert of the token goes: the first deleted slot of its chain, else the empty one.
uint32_t free_slot(const AdbSlot* tab, uint64_t mask, uint64_t tok) {
  uint32_t first = NONE;
  for (uint64_t i = adb_home(tok, mask), n = 0; n <= mask; ++n, i = (i + 1) & mask) {
    if (tab[i].tok == ADB_DELETED && first == NONE) first = (uint32_t)i;
    if (tab[i].tok == ADB_EMPTY) return first == NONE ? (uint32_t)i : first;
  }
  return first;
}

struct Rule {
  uint32_t perm, action;
  const char* filter;
};

// A record pool of the runs `recs` with their filters, as gm_acldb.cpp lays them out.
struct Pool {
  std::vector<uint64_t> words;
  std::vector<uint8_t> fb;
  std::vector<uint32_t> fo{0};
  std::vector<uint32_t> starts;
  uint64_t test_mask = 0;
  void add(const std::vector<Rule>& rules) {
    starts.push_back((uint32_t)words.size());
    const size_t h = words.size();
    words.push_back(0);
    for (uint32_t k = 0; k < rules.size(); ++k) {
      uint64_t rec[ADB_RULE_WORDS_MAX];
      uint32_t skip = 0;
      const uint32_t len = (uint32_t)strlen(rules[k].filter);
      const uint32_t nw = adb_compile_rule(rules[k].perm, rules[k].action, (const uint8_t*)rules[k].filter, len, k,
                                           test_mask, rec, &skip);
      words.insert(words.end(), rec, rec + nw);
      fb.insert(fb.end(), rules[k].filter + skip, rules[k].filter + len);
      fo.push_back((uint32_t)fb.size());
    }
    words[h] = adb_run_header((uint32_t)(words.size() - h), (uint32_t)(fo.size() - 1 - rules.size()));
  }
};

// Walks run `start` of an exact-size copy of `words`; every visit must be in bounds.  Returns
// -1 when a visit was out of bounds, else visits * 2 + (the walk's verdict).
int walk(const std::vector<uint64_t>& words, uint32_t start, uint32_t n_filters, std::vector<uint32_t>* seen) {
  AclExact<uint64_t> pool(words);
  bool oob = false;
  int visits = 0;
  const bool ok = adb_walk_run((const uint64_t*)pool.p, (uint64_t)words.size(), start, n_filters,
                               [&](uint32_t k, uint64_t r0, const uint64_t* rec, uint32_t f) {
                                 ++visits;
                                 if (f >= n_filters || acl_rule(r0) != k || rs_rule(rec[0]) != k || rs_filter(rec[0]) != k)
                                   oob = true;
                                 if (seen) seen->push_back(f);
                                 return false;
                               });
  return oob ? -1 : visits * 2 + (ok ? 1 : 0);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const uint64_t test_mask = rs_test_mask((uint32_t)atoi(argv[1]));
  std::vector<Bytes> keys;
  for (int i = 2; i < 6; ++i) {
    Bytes b;
    std::vector<uint32_t> o;
    acl_unhex(argv[i], b, o);
    keys.push_back(b);
  }
  // ---- the probe: a chain of four that wraps, a delete in its middle, the key stored again ----
  const uint64_t mask = ADB_MIN_SLOTS - 1;
  std::unique_ptr<AdbSlot[]> tab(new AdbSlot[ADB_MIN_SLOTS]);
  for (uint32_t i = 0; i < ADB_MIN_SLOTS; ++i) tab[i] = AdbSlot{ADB_EMPTY, 0, 0};
  uint64_t tok[4];
  uint32_t slot[4];
  printf("HOME");
  for (uint32_t k = 0; k < 4; ++k) {
    tok[k] = acl_value_token(keys[k].data(), (uint32_t)keys[k].size(), test_mask);
    CHECK(tok[k] != ADB_EMPTY && tok[k] != ADB_DELETED, "a token is no mark");
    printf(" %llu", (unsigned long long)adb_home(tok[k], mask));
  }
  printf("\n");
  for (uint32_t k = 0; k < 4; ++k) {
    slot[k] = free_slot(tab.get(), mask, tok[k]);
    CHECK(slot[k] != NONE, "a free slot");
    tab[slot[k]] = AdbSlot{tok[k], 100 + k, k};
  }
  auto states = [&]() {
    printf("STATES");
    for (uint32_t i = 0; i < ADB_MIN_SLOTS; ++i) {
      if (tab[i].tok == ADB_EMPTY) printf(" E");
      else if (tab[i].tok == ADB_DELETED) printf(" D");
      else printf(" %u", tab[i].key);
    }
    printf("\n");
  };
  auto probe_all = [&](uint32_t from) {
    uint64_t steps[4];
    uint32_t at[4], hits;
    for (uint32_t k = from; k < 4; ++k) at[k] = find(tab.get(), mask, tok[k], keys, keys[k], &steps[k], &hits);
    printf("FOUND");
    for (uint32_t k = from; k < 4; ++k) printf(" %d", at[k] == NONE ? -1 : (int)at[k]);
    printf("\nSTEPS");
    for (uint32_t k = from; k < 4; ++k) printf(" %llu", (unsigned long long)steps[k]);
    printf("\n");
  };
  printf("SLOTS %u %u %u %u\n", slot[0], slot[1], slot[2], slot[3]);
  states();
  probe_all(0);
  {
    // a key that is not stored: the probe ends at the empty slot past the chain
    uint64_t steps;
    uint32_t hits;
    const Bytes absent = {'n', 'o'};
    const uint64_t t = acl_value_token(absent.data(), 2u, test_mask);
    const uint32_t at = find(tab.get(), mask, t, keys, absent, &steps, &hits);
    CHECK(at == NONE && steps <= ADB_MIN_SLOTS, "an absent key ends at an empty slot");
  }
  tab[slot[1]].tok = ADB_DELETED;
  printf("DELETED %u\n", slot[1]);
  states();
  {
    uint64_t steps;
    uint32_t hits;
    CHECK(find(tab.get(), mask, tok[1], keys, keys[1], &steps, &hits) == NONE, "the deleted key is gone");
  }
  probe_all(2);
  const uint32_t again = free_slot(tab.get(), mask, tok[1]);
  tab[again] = AdbSlot{tok[1], 101, 1};
  printf("AGAIN %u\n", again);
  states();
  probe_all(0);
  {
    // a full table with no empty slot and no such token: the probe stops after mask + 1 slots
    std::unique_ptr<AdbSlot[]> full(new AdbSlot[ADB_MIN_SLOTS]);
    for (uint32_t i = 0; i < ADB_MIN_SLOTS; ++i) full[i] = AdbSlot{ADB_DELETED, 0, 0};
    uint64_t i = adb_home(tok[0], mask), steps = 0;
    CHECK(adb_probe_next(full.get(), mask, tok[0], &i, &steps) == NONE && steps == ADB_MIN_SLOTS, "a probe is bounded");
  }

  // ---- the run walk and the relative indices ----
  Pool P;
  P.test_mask = test_mask;
  P.add({{1, 3, "a/+"}, {0, 1, "eq a/b"}, {1, 2, "c/${clientid}/#"}});
  P.add({});
  P.add({{0, 3, "x"}, {1, 1, "y/#"}});
  const uint32_t nf = (uint32_t)P.fo.size() - 1;
  CHECK(nf == 5, "five filters");
  std::vector<uint32_t> seen;
  CHECK(walk(P.words, P.starts[0], nf, &seen) == 3 * 2 + 1 && seen == std::vector<uint32_t>({0, 1, 2}), "run 0");
  seen.clear();
  CHECK(walk(P.words, P.starts[1], nf, &seen) == 1 && seen.empty(), "the empty run");
  seen.clear();
  CHECK(walk(P.words, P.starts[2], nf, &seen) == 2 * 2 + 1 && seen == std::vector<uint32_t>({3, 4}), "run 2");
  // run 2's records carry positions 0 and 1, not 3 and 4: the fields are relative to the run
  CHECK(acl_rule(P.words[P.starts[2] + 1]) == 0 && rs_filter(P.words[P.starts[2] + 3]) == 0, "relative fields");
  printf("WALK ok\n");

  // ---- malformed runs: the walk says so before it follows anything ----
  const uint32_t s2 = P.starts[2];
  struct Bad {
    const char* what;
    std::vector<uint64_t> words;
    uint32_t start, n_filters;
    int want;  // visits before the walk gives up, * 2 (the verdict is false)
  };
  std::vector<Bad> bad;
  auto mutate = [&](const char* what, size_t at, uint64_t v, int want, uint32_t start, uint32_t n_filters) {
    Bad b{what, P.words, start, n_filters, want};
    b.words[at] = v;
    bad.push_back(b);
  };
  bad.push_back(Bad{"a run that starts at the pool's end", P.words, (uint32_t)P.words.size(), nf, 0});
  bad.push_back(Bad{"a run that starts past the pool's end", P.words, 0xFFFFFFF0u, nf, 0});
  mutate("a run longer than the pool", s2, adb_run_header((uint32_t)(P.words.size() - s2) + 1, 3), 0, s2, nf);
  mutate("a run of no words", s2, adb_run_header(0, 3), 0, s2, nf);
  mutate("a run cut inside its last record", s2, adb_run_header((uint32_t)(P.words.size() - s2) - 1, 3), 2, s2, nf);
  mutate("a run cut inside a rule header", s2, adb_run_header(2, 3), 0, s2, nf);
  mutate("a rule field that is not the position", s2 + 1, acl_rule_header(0, 3, ACL_WHO_ALL, 0, 1), 0, s2, nf);
  mutate("a rule header of another who kind", s2 + 1, acl_rule_header(0, 3, ACL_WHO_CLIENTID, 0, 0), 0, s2, nf);
  mutate("a filter record where a rule header is due", s2 + 1, P.words[s2 + 3], 0, s2, nf);
  mutate("a rule header where a filter record is due", s2 + 3, P.words[s2 + 1], 0, s2, nf);
  mutate("the end mark where a filter record is due", s2 + 3, RS_END, 0, s2, nf);
  {
    const uint64_t w0 = P.words[s2 + 3];
    mutate("a filter field that is not the position", s2 + 3,
           rs_header(rs_levels(w0), rs_flags(w0), 0, 1, rs_plus(w0)), 0, s2, nf);
    mutate("a rule field of the filter record that is not the position", s2 + 3,
           rs_header(rs_levels(w0), rs_flags(w0), 1, 0, rs_plus(w0)), 0, s2, nf);
    mutate("more levels than the run has words", s2 + 3, rs_header(16, rs_flags(w0), 0, 0, rs_plus(w0)), 0, s2, nf);
  }
  mutate("a filter base at the offset array's end", s2, adb_run_header((uint32_t)(P.words.size() - s2), nf), 0, s2, nf);
  mutate("a filter base far past the offset array", s2, adb_run_header((uint32_t)(P.words.size() - s2), 0xFFFFFFFFu), 0,
         s2, nf);
  bad.push_back(Bad{"the second filter at the offset array's end", P.words, s2, 4, 2});
  for (const Bad& b : bad) {
    const int got = walk(b.words, b.start, b.n_filters, nullptr);
    if (got != b.want) {
      fprintf(stderr, "FAILED: %s: got %d, want %d\n", b.what, got, b.want);
      return 1;
    }
    printf("BAD %s\n", b.what);
  }

  // ---- malformed slots through the kernel's lookup phase: the error word, no answer, no read
  // past an array (every one is of exact size) ----
  {
    const Bytes name = {'x'}, cid = keys[0];
    const std::vector<uint32_t> no = {0, 1}, cl = {0}, ac = {ACL_PUBLISH}, co = {0, (uint32_t)cid.size()}, uo = {0, 0},
                                cf = {ACL_C_USR_UNDEF};
    const Bytes none;
    AclExact<uint8_t> nb(name), cb(cid), ub(none), fb(P.fb), kb(keys[0]);
    AclExact<uint32_t> noe(no), cle(cl), ace(ac), coe(co), uoe(uo), cfe(cf), fo(P.fo);
    const std::vector<uint32_t> kov = {0, (uint32_t)keys[0].size()};
    AclExact<uint32_t> ko(kov);
    AclExact<uint64_t> pool(P.words);
    struct Case {
      const char* what;
      AdbSlot slot;
      uint32_t want_bad, want_perm;
    };
    const Case cases[] = {
        {"a well-formed slot", AdbSlot{tok[0], s2, 0}, 0, ACL_DENY},
        {"a key index at the key array's end", AdbSlot{tok[0], s2, 1}, 1, NONE},
        {"a key index far past the key array", AdbSlot{tok[0], s2, 0xFFFFFFFFu}, 1, NONE},
        {"a run at the pool's end", AdbSlot{tok[0], (uint32_t)P.words.size(), 0}, 1, NONE},
        {"a run far past the pool", AdbSlot{tok[0], 0xFFFFFFF0u, 0}, 1, NONE},
    };
    for (const Case& c : cases) {
      std::vector<AdbSlot> tv(ADB_MIN_SLOTS, AdbSlot{ADB_EMPTY, 0, 0});
      tv[adb_home(tok[0], mask)] = c.slot;
      AclExact<AdbSlot> t0(tv);
      std::vector<AdbSlot> ev(ADB_MIN_SLOTS, AdbSlot{ADB_EMPTY, 0, 0});
      AclExact<AdbSlot> t1(ev);
      AclDbArgs A;
      A.nb = nb.p, A.no = noe.p, A.client = cle.p, A.action = ace.p, A.n = 1;
      A.cb = cb.p, A.co = coe.p, A.ub = ub.p, A.uo = uoe.p, A.cf = cfe.p, A.n_clients = 1;
      A.tab[0] = t0.p, A.tab[1] = t1.p, A.tmask[0] = A.tmask[1] = mask;
      A.pool = pool.p, A.pool_words = P.words.size();
      A.fb = fb.p, A.fo = fo.p, A.n_filters = nf;
      A.kb = kb.p, A.ko = ko.p, A.n_keys = 1;
      A.test_mask = test_mask;
      std::unique_ptr<uint64_t[]> s_tok(new uint64_t[RS_MAX_LEVELS * WG]);
      AdbLane L;
      blockIdx.x = 0;
      threadIdx.x = 0;
      adb_ph_tokenize(A, L, s_tok.get());
      adb_ph_lookup(A, L, s_tok.get(), ADB_CLIENTID);
      adb_ph_lookup(A, L, s_tok.get(), ADB_USERNAME);
      if (L.bad != c.want_bad || L.perm != c.want_perm) {
        fprintf(stderr, "FAILED: %s: bad %u perm %u\n", c.what, L.bad, L.perm);
        return 1;
      }
      printf("SLOT %s\n", c.what);
    }
  }
  return 0;
}
