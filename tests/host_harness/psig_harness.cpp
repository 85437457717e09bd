// psig_harness.cpp -- TEST INFRASTRUCTURE: the lent-signature invariant of the edge table
// (gm_common.h "Lent signatures") after a full build and after every step of a delta churn.
//
// Built by tests/test_psig_host.py (tests/host_build.py) under ASan + UBSan against the fake HIP
// runtime of this directory, like harness.cpp; the rig is harness_rig.h's.  It runs no SlotWalk
// (harness_walk.h): the filter it guards only removes probes, so the rows of the plain reader
// are the check.  After every commit it scans every live node's
// slot in the committed device tables (the root's half in the arguments and the root's own
// signature included):
//   * the slot equals what the model gives for its node (a delta left no stale slot behind);
//   * CF_LIT set: the signature field is the node's own -- 0 for a keyed node, else its stored
//     signature, which contains the class of every live literal child;
//   * CF_LIT clear: the field is 0 without a '+' child, else it contains the class of every live
//     literal child of the '+' child (a clear bit must be exact: the walk drops the probe).
// and walks every probe topic on the CPU with the reader that ignores lent bits
// (harness_walk.h), whose rows must stay equal to the oracle's.
// Prints "OK <commits> <delta commits> <slots scanned> <lending slots> <row checks>".
#include "harness_rig.h"

namespace {

uint64_t g_slots = 0, g_lending = 0;

struct Rig : RigBase {
  using RigBase::RigBase;
  // the node at the end of a path that is in the trie
  uint32_t node(const std::string& path) {
    const uint32_t c = node_of(path);
    CHECK(c != NONE, "no node at '%s'", path.c_str());
    return c;
  }
  // the committed slot of node c (the root's half: the arguments); nullptr for the root
  const uint4* slot(uint32_t c, uint4 tmp[2]) {
    const TrieModel& m = h->tm;
    const DevIndex& ix = h->cur->ix;
    if (m.slot[c] == ROOTH) {
      tmp[0] = ix.rh0;
      tmp[1] = ix.rh1;
      return tmp;
    }
    return ix.edges + SLOT_U4 * m.slot[c];
  }
  uint32_t field(uint32_t c) {
    if (c == 0) return h->cur->ix.root_sig;
    uint4 tmp[2];
    return slot(c, tmp)[0].z >> SIG_SHIFT;
  }

  void scan(const char* what) {
    const TrieModel& m = h->tm;
    const DevIndex& ix = h->cur->ix;
    CHECK(m.valid, "%s: no model", what);
    const uint32_t n = (uint32_t)m.parent.size();
    auto alive = [&](uint32_t c) { return c == 0 || m.slot[c] != DEAD; };
    std::vector<uint32_t> kids(n, 0);  // classes of the live literal children
    for (uint32_t y = 1; y < n; ++y)
      if (alive(y) && m.tok[y] != PLUS_TOK) kids[m.parent[y]] |= sig_bit(m.tok[y]);
    for (uint32_t c = 0; c < n; ++c) {
      if (!alive(c)) continue;
      uint32_t cf, fld;
      if (c == 0) {
        cf = ix.root_cf;
        fld = ix.root_sig;
        CHECK(cf == m.cf(0), "%s: root cf", what);
      } else {
        uint4 tmp[2], want[2];
        const uint4* q = slot(c, tmp);
        m.node_slot(c, want);
        CHECK(memcmp(q, want, sizeof want) == 0, "%s: node %u: stale slot", what, c);
        CHECK((q[0].z & CF_ID_MASK) == (m.half[c] ? FAT_ID : m.parent[c]), "%s: node %u: parent word",
              what, c);
        cf = q[0].w;
        fld = q[0].z >> SIG_SHIFT;
      }
      ++g_slots;
      CHECK(((cf & CF_LIT) != 0) == (m.nlit[c] != 0) && ((cf & CF_PLUS) != 0) == (m.pchild[c] != 0),
            "%s: node %u: child flags", what, c);
      if (cf & CF_LIT) {
        // today's value: the node's own signature, or the keyed flag
        CHECK(fld == (m.keyed[c] ? 0u : (uint32_t)m.sig[c]), "%s: node %u: own field %02x", what, c, fld);
        CHECK(m.keyed[c] || (fld & kids[c]) == kids[c], "%s: node %u: own classes", what, c);
      } else if (!m.pchild[c]) {
        CHECK(fld == 0u, "%s: node %u: field %02x without a '+' child", what, c, fld);
      } else {
        const uint32_t k = kids[m.pchild[c]];
        CHECK((fld & k) == k, "%s: node %u: lent field %02x misses classes %02x", what, c, fld, k);
        g_lending += k != 0;
      }
    }
  }

  // commit, then every check; delta: the commit must have patched the tables in place
  void step(const char* what, bool delta = true) {
    commit(what, delta);
    scan(what);
    // (no SlotWalk here: the rows are the plain reader's, which ignores lent bits)
    rows(what, [](const std::string&, const std::vector<uint32_t>&) {});
  }
};

// A cfg3-shaped trie (workloads/gen.cpp gen_cfg3: 4 sites x 8 devices, its five patterns) and
// the churn of its device states.
void run_cfg3(uint32_t hash_bits, int keyed_mode, int fat) {
  Rig r(hash_bits, keyed_mode, fat);
  const bool exact = hash_bits == 0;  // (collision tokens merge nodes: no per-node assertions)
  std::mt19937_64 rng(7 + hash_bits);
  auto dev = [](int s, int j) { return S(s * 1000 + j); };
  std::set<std::string> fs;
  for (int s = 0; s < 4; ++s)
    for (int j = 0; j < 8; ++j) {
      const std::string site = "site/" + S(s), d = dev(s, j);
      if (j != 5) fs.insert(site + "/device/" + d + "/#");
      if (rng() % 2) fs.insert("site/+/device/" + d + "/#");
      // devices 0..3: some D/+/k; 4: none (gains and loses its '+' child below); 5: only D/+/k;
      // 6: literal children beside the '+' child (a keyed parent at "keyed" 2); 7: a fat node
      if (j < 4 || j == 5)
        for (int k = 0; k < 16; ++k)
          if (rng() % 4 == 0 || k == j) fs.insert(site + "/device/" + d + "/+/" + S(k));
      if (j == 6) {
        fs.insert(site + "/device/" + d + "/a/z");
        fs.insert(site + "/device/" + d + "/b/z");
        fs.insert(site + "/device/" + d + "/+/5");
        fs.insert(site + "/device/" + d + "/+/11");
      }
      if (j == 7) fs.insert(site + "/device/" + d + "/only/+/7");
    }
  for (int s = 0; s < 4; ++s)
    for (int m = 0; m < 32; m += 1 + (int)(rng() % 5)) {
      fs.insert("site/" + S(s) + "/device/+/m" + S(m));
      fs.insert("site/" + S(s) + "/+/+/m" + S((m + 3) % 32));
    }
  for (const auto& f : fs) r.add(f);
  for (int s = 0; s < 4; ++s)
    for (int j = 0; j < 8; ++j)
      for (int k = 0; k < 16; k += 3) {
        const std::string p = "site/" + S(s) + "/device/" + dev(s, j);
        r.topics.push_back(p + "/m" + S((k * 5 + j) % 32) + "/" + S(k));
      }
  for (int k = 0; k < 16; ++k) r.topics.push_back("site/0/device/" + dev(0, 0) + "/m1/" + S(k));
  for (const char* w : {"new", "lit", "x", "only", "other", "z", "q7", "q8", "q9", "q10", "q11", "q12"}) {
    r.topics.push_back("site/0/device/" + dev(0, 0) + "/m1/" + w);
    r.topics.push_back("site/0/device/" + dev(0, 1) + "/" + w + "/x");
    r.topics.push_back("site/2/device/" + dev(2, 7) + "/only/" + w + "/7");
    r.topics.push_back("site/2/device/" + dev(2, 7) + "/" + w);
  }
  r.topics.push_back("site/0/device/" + dev(0, 0));
  r.topics.push_back("site/0/device/" + dev(0, 0) + "/m1");
  r.topics.push_back("site/0/device/" + dev(0, 0) + "/m1/3/deeper");
  r.topics.push_back("site/0/device/" + dev(0, 0) + "/m1/3/deeper/still");
  r.topics.push_back("site/1/device/" + dev(1, 6) + "/a/z");
  r.topics.push_back("site/1/device/" + dev(1, 6) + "/c/5");
  r.topics.push_back("site/1/device/" + dev(1, 6) + "/c/11");
  r.topics.push_back("$site/0/device/0/m1/3");
  r.topics.push_back("site/+/device/0/m1/3");
  r.step("full build", false);
  CHECK(g_lending > 0, "no slot lends a signature");

  // -- a literal child under an existing D/+: a word of a class the lent field does not have yet
  {
    const std::string D = "site/0/device/" + dev(0, 0);
    const uint32_t c = r.node(D);
    std::string w;
    for (int i = 7; i < 13 && w.empty(); ++i)
      if (!(r.field(c) & sig_bit(r.word_tok("q" + S(i))))) w = "q" + S(i);
    if (exact) {
      CHECK(c && r.h->tm.nlit[c] == 0 && r.h->tm.pchild[c], "D shape");
      CHECK(!w.empty(), "no word of a class that is still clear");
    }
    if (w.empty()) w = "q7";
    r.add(D + "/+/" + w);
    r.step("literal child under D/+");
    if (exact) CHECK(r.field(c) & sig_bit(r.word_tok(w)), "the new child's class is not lent");
    r.del(D + "/+/" + w);
    r.step("literal child under D/+ deleted");
  }
  // -- a literal-less D gains its first literal child (the field is its own again), loses it
  {
    const std::string D = "site/0/device/" + dev(0, 1);
    const uint32_t c = r.node(D);
    const uint32_t lent = r.field(c);
    if (exact) CHECK(c && r.h->tm.nlit[c] == 0 && lent != 0, "D shape");
    r.add(D + "/lit/x");
    r.step("first literal child");
    if (exact) CHECK(r.field(c) == sig_bit(r.word_tok("lit")), "own signature after the first literal child");
    r.del(D + "/lit/x");
    r.step("last literal child deleted");
    if (exact) CHECK(r.field(c) == lent, "lent signature back after the last literal child");
  }
  // -- the '+' child comes and goes
  {
    const std::string D = "site/0/device/" + dev(0, 4);
    const uint32_t c = r.node(D);
    if (exact) CHECK(c && r.h->tm.pchild[c] == 0 && r.field(c) == 0, "D shape");
    r.add(D + "/+/3");
    r.step("'+' child added");
    if (exact) CHECK(r.field(c) == sig_bit(r.word_tok("3")), "a new '+' child's signature is lent");
    r.del(D + "/+/3");
    r.step("'+' child deleted");
    if (exact) CHECK(r.field(c) == 0, "no '+' child, no lent bits");
    r.add(D + "/+/4");  // (a new '+' node: the old one's bits must not come back)
    r.step("'+' child added again");
    if (exact) CHECK(r.field(c) == sig_bit(r.word_tok("4")), "the new '+' child's signature");
  }
  // -- a keyed parent loses all its literal children: it lends, it does not write the keyed 0
  {
    const std::string D = "site/1/device/" + dev(1, 6);
    const uint32_t c = r.node(D);
    if (exact && keyed_mode == 2) CHECK(c && r.h->tm.keyed[c] && r.field(c) == 0, "keyed D");
    r.del(D + "/a/z");
    r.del(D + "/b/z");
    r.step("keyed parent without literal children");
    if (exact) {
      CHECK(r.h->tm.nlit[c] == 0 && (keyed_mode != 2 || r.h->tm.keyed[c]), "D shape");
      CHECK(r.field(c) == (sig_bit(r.word_tok("5")) | sig_bit(r.word_tok("11"))), "a keyed node lends");
    }
    r.add(D + "/a/z");
    r.step("keyed parent with a literal child again");
    if (exact && keyed_mode == 2) CHECK(r.field(c) == 0, "keyed flag back");
  }
  // -- a fat node and its half: the half lends in FAT_ID | field; then the half moves out
  {
    const std::string D = "site/2/device/" + dev(2, 7);
    const uint32_t c = r.node(D), g = r.node(D + "/only");
    if (exact && fat) {
      CHECK(c && g && r.h->tm.fchild[c] == g && r.h->tm.half[g], "no fat node");
      CHECK(r.field(g) == sig_bit(r.word_tok("7")), "the half lends");
    }
    r.add(D + "/only/+/9");
    r.step("literal child under a half's '+' child");
    if (exact) CHECK(r.field(g) == (sig_bit(r.word_tok("7")) | sig_bit(r.word_tok("9"))), "the half's lent bits");
    r.add(D + "/other");
    r.step("the half moves out");
    if (exact) CHECK(!r.h->tm.half[g] && r.field(g) == (sig_bit(r.word_tok("7")) | sig_bit(r.word_tok("9"))),
                     "the moved half still lends");
  }
  // -- and a full build of the churned registry
  CHECK(emqxgm_tune(r.h, "fat_buckets", fat) == 0, "tune");  // (invalidates the model)
  r.step("full rebuild", false);
}

// A root without literal children whose '+' child has some: root_sig lends.
void run_root(uint32_t hash_bits) {
  Rig r(hash_bits, 1, 1);
  const bool exact = hash_bits == 0;
  for (const char* f : {"+/a", "+/b/#", "+/+/c", "+/a/+/d", "#"}) r.add(f);
  for (const char* t : {"x/a", "x/q", "x/b/y", "x/y/c", "$x/a", "x", "x/a/y/d", "x/zz", "lit/q", "lit/a",
                        "+/a", "x/a/y/e"})
    r.topics.push_back(t);
  r.step("root build", false);
  if (exact) {
    CHECK(r.h->tm.nlit[0] == 0 && !(r.h->cur->ix.root_cf & CF_LIT), "root shape");
    CHECK(r.field(0) == (sig_bit(r.word_tok("a")) | sig_bit(r.word_tok("b"))), "the root lends");
  }
  r.add("+/zz");
  r.step("literal child under the root's '+' child");
  if (exact) CHECK(r.field(0) & sig_bit(r.word_tok("zz")), "root_sig follows");
  r.add("lit/q");
  r.step("the root's first literal child");
  if (exact) CHECK((r.h->cur->ix.root_cf & CF_LIT) && r.field(0) == sig_bit(r.word_tok("lit")), "root's own");
  r.del("lit/q");
  r.step("the root's last literal child deleted");
  if (exact) CHECK(!(r.h->cur->ix.root_cf & CF_LIT) && (r.field(0) & sig_bit(r.word_tok("zz"))), "root lends again");
}

}  // namespace

int main() {
  run_cfg3(0, 2, 1);  // every eligible node keyed
  run_cfg3(0, 1, 1);
  run_cfg3(0, 2, 0);  // no fat buckets
  run_cfg3(3, 2, 1);  // 3-bit collision tokens
  run_root(0);
  run_root(3);
  printf("OK %llu %llu %llu %llu %llu\n", (unsigned long long)g_commits, (unsigned long long)g_deltas,
         (unsigned long long)g_slots, (unsigned long long)g_lending, (unsigned long long)g_rows);
  return 0;
}
