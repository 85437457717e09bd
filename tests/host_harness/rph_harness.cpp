// rph_harness.cpp -- TEST INFRASTRUCTURE: the root's '+' half (gm_kernels.h DevIndex::rp0/rp1) and
// the shared line of keyed siblings (gm_walk.inc SHARE), on the CPU.
//
// Built by tests/test_rph_host.py (tests/host_build.py) under ASan + UBSan against the fake HIP
// runtime of this directory, like psig_harness.cpp; the rig is harness_rig.h's, the restated walk
// harness_walk.h's SlotWalk, run with the switches rp and ks in all four combinations and with
// lent and cb off.  After a full build and after every step of a delta churn it checks that
//   * rp0/rp1 is absent, or equals node_slot of the only live literal child H of the '+' child p
//     of the root's half G -- and equals H's slot in the committed table (the copy is a cache);
//     where a step says so, that it is present (a build with one such child) or absent (a second
//     literal child under G/+ clears it in that same commit);
//   * the restatement of k_walk's iteration -- two probe slots filled from the LIFO, one bucket per
//     slot and round trip, resolves in slot order, then the late match -- returns the same rows
//     with the two rules on and off, equal to the rows of the reader that knows neither
//     (harness_walk.h CpuWalk) and to the oracle's.
// Prints "OK <commits> <delta commits> <copies present> <copy hits> <shared items> <row checks>".
#include "harness_rig.h"

namespace {

uint64_t g_present = 0, g_rp_hits = 0, g_shared = 0;
uint64_t g_loads[2] = {0, 0}, g_iters[2] = {0, 0};

struct Rig : RigBase {
  Rig(uint32_t hb, int keyed_mode, int fat_mode) : RigBase(hb, keyed_mode, fat_mode) {
    // the rules' tune keys: accepted values, rejected values
    CHECK(emqxgm_tune(h, "root_plus_half", 0) == 0 && emqxgm_tune(h, "root_plus_half", 1) == 0 &&
              emqxgm_tune(h, "root_plus_half", 2) != 0, "tune root_plus_half");
    CHECK(emqxgm_tune(h, "keyed_share", 0) == 0 && emqxgm_tune(h, "keyed_share", 1) == 0 &&
              emqxgm_tune(h, "keyed_share", -1) != 0, "tune keyed_share");
  }

  // want: 1 the copy must be there, 0 it must be absent, -1 either (absent is always correct)
  void copy(const char* what, int want) {
    const TrieModel& m = h->tm;
    const DevIndex& ix = h->cur->ix;
    CHECK(m.valid, "%s: no model", what);
    const uint32_t nn = (uint32_t)m.parent.size();
    const uint32_t g = m.fchild[0], p = g ? m.pchild[g] : 0u;
    uint32_t kids = 0, H = 0;
    if (p)
      for (uint32_t c = 1; c < nn; ++c)
        if (m.slot[c] != DEAD && m.parent[c] == p && m.tok[c] != PLUS_TOK) {
          ++kids;
          H = c;
        }
    const bool present = ix.rp0.z != NONE;
    if (present) {
      CHECK(g && p && kids == 1, "%s: a copy with %u literal children under G/+", what, kids);
      uint4 wantsl[2];
      m.node_slot(H, wantsl);
      const uint4 got[2] = {ix.rp0, ix.rp1};
      CHECK(memcmp(got, wantsl, sizeof got) == 0, "%s: the copy is not node_slot(H)", what);
      CHECK(m.slot[H] != ROOTH && memcmp(got, ix.edges + SLOT_U4 * m.slot[H], sizeof got) == 0,
            "%s: the copy differs from H's slot in the table", what);
      CHECK((ix.rp0.z & CF_ID_MASK) == p, "%s: the copy's parent word", what);
      ++g_present;
    }
    if (hash_bits == 0) {  // (collision tokens merge nodes: no per-node expectations)
      if (want == 1) CHECK(present, "%s: no copy (G %u, p %u, %u literal children, root nlit %u)", what, g, p, kids, m.nlit[0]);
      if (want == 0) CHECK(!present, "%s: a copy that should be gone", what);
    }
  }

  // The restated walk with its two rules on and off, one at a time and together.  Lent
  // signatures and closed buckets stay off in all four: mode 0 stands for production with tune
  // "plus_sig" 0, "closed_buckets" 0, "root_plus_half" 0, "keyed_share" 0, mode 3 for the same
  // with the last two at 1 -- so the loads and iterations compared are these two rules' alone.
  void walks(const char* what, const std::string& topic, const std::vector<uint32_t>& base) {
    for (int mode = 0; mode < 4; ++mode) {
      WalkRules rules(h->cur->ix);
      rules.lent = rules.cb = false;
      rules.rp = (mode & 1) != 0;
      rules.ks = (mode & 2) != 0;
      const SlotWalk sw = slot_walk(rules, what, topic, base, ("rules " + S(mode)).c_str());
      if (mode == 0 || mode == 3) {
        g_loads[mode == 3] += sw.loads;
        g_iters[mode == 3] += sw.iters;
      }
      if (mode == 3) {
        g_rp_hits += sw.rp_hits;
        g_shared += sw.shared;
      }
    }
  }

  void step(const char* what, int want, bool delta = true) {
    if (!fat && want == 1) want = 0;  // without fat buckets the root has no half, so no copy
    commit(what, delta);
    copy(what, want);
    rows(what, [&](const std::string& t, const std::vector<uint32_t>& base) { walks(what, t, base); });
  }
};

// A cfg3-shaped trie (4 sites x 8 devices, its five patterns): G = site, p = site/+, H =
// site/+/device, and the churn of H's slot and of p's literal children.
void run_cfg3(uint32_t hash_bits, int keyed_mode, int fat) {
  Rig r(hash_bits, keyed_mode, fat);
  std::mt19937_64 rng(11 + hash_bits);
  auto dev = [](int s, int j) { return S(s * 1000 + j); };
  std::set<std::string> fs;
  for (int s = 0; s < 4; ++s)
    for (int j = 0; j < 8; ++j) {
      const std::string site = "site/" + S(s), d = dev(s, j);
      if (j != 5) fs.insert(site + "/device/" + d + "/#");
      if (rng() % 2 || j == 0) fs.insert("site/+/device/" + d + "/#");  // (j == 0: both edges of D)
      if (j == 1) fs.erase("site/+/device/" + d + "/#");                 // only the first
      if (j < 4 || j == 5)
        for (int k = 0; k < 16; ++k)
          if (rng() % 4 == 0 || k == j) fs.insert(site + "/device/" + d + "/+/" + S(k));
    }
  for (int j = 8; j < 12; ++j) fs.insert("site/+/device/" + dev(0, j) + "/#");  // only the second
  for (int s = 0; s < 4; ++s)
    for (int m = 0; m < 32; m += 1 + (int)(rng() % 5)) {
      fs.insert("site/" + S(s) + "/device/+/m" + S(m));
      fs.insert("site/" + S(s) + "/+/+/m" + S((m + 3) % 32));
    }
  for (const auto& f : fs) r.add(f);
  for (int s = 0; s < 4; ++s)
    for (int j = 0; j < 12; ++j)
      for (int k = 0; k < 16; k += 5) {
        const std::string p = "site/" + S(s) + "/device/" + dev(j < 8 ? s : 0, j);
        r.topics.push_back(p + "/m" + S((k * 5 + j) % 32) + "/" + S(k));
      }
  for (const char* t : {"site", "site/0", "site/0/device", "site/0/other", "site/0/device/0", "site/9/device/0/m1/3",
                        "site/0/device/0/m1/3/a/b", "site/0/device/0/m1/3/a/b/c/d/e/f/g/h/i/j/k",
                        "site/0/ext/0/m1/3", "site/0/ext", "site/0/ext/x/m3", "$site/0/device/0/m1/3", "$site",
                        "site/+/device/0/m1/3", "other/0/device/0/m1/3", "site/0/device/nodev/m1/3"})
    r.topics.push_back(t);
  r.step("full build", 1, false);
  if (hash_bits == 0 && keyed_mode == 2 && fat) {
    const TrieModel& m = r.h->tm;
    const uint32_t H = m.lone.at(m.pchild[m.fchild[0]]);
    CHECK(m.keyed[H], "site/+/device is not keyed");
  }

  // -- H's slot changes: the copy follows in the same commit
  r.add("site/+/device/#");
  r.step("H gains a '#' filter", 1);
  r.add("site/+/device");
  r.step("H gains a terminal filter", 1);
  r.del("site/+/device/#");
  r.step("H keeps terminal filters only", 1);
  r.add("site/+/device/+/deep");
  r.step("H gains a '+' child", 1);
  r.add("site/+/device/fresh/#");
  r.step("H gains a literal child", 1);
  // -- a second literal child under G/+: the copy goes in that commit; back to one: absent or right
  r.add("site/+/ext/+/m3");
  r.step("H gains a sibling", 0);
  r.add("site/+/ext2");
  r.step("a third literal child", 0);
  r.del("site/+/ext2");
  r.step("back to two", 0);
  r.del("site/+/ext/+/m3");
  r.step("H loses the sibling", -1);
  r.del("site/+/device");
  r.step("H loses its terminal filter", -1);
  // -- the root's half goes (a second first-level word), and a full build of the churned registry
  r.add("other/+/device/7/#");
  r.step("the root's half moves out", 0);
  CHECK(emqxgm_tune(r.h, "fat_buckets", fat) == 0, "tune");  // (invalidates the model)
  r.step("full rebuild, two first-level words", 0, false);
  r.del("other/+/device/7/#");
  r.step("one first-level word again", -1);
  CHECK(emqxgm_tune(r.h, "fat_buckets", fat) == 0, "tune");
  r.step("full rebuild", 1, false);
}

// G/+ with no literal child, one that comes by a delta, then p itself going and coming.
void run_small(uint32_t hash_bits) {
  Rig r(hash_bits, 2, 1);
  for (const char* f : {"a/b/c", "a/b/#", "a/+", "a/+/+/z", "a/#"}) r.add(f);
  for (const char* t : {"a", "a/b", "a/b/c", "a/x", "a/x/h", "a/x/h/z", "a/b/h/z", "a/x/h/q/r", "$a/x/h", "b/x/h",
                        "a/x/h2", "a/x/h2/w", "a/x/y/z"})
    r.topics.push_back(t);
  r.step("no literal child under G/+", 0, false);
  r.add("a/+/h");
  r.step("the first literal child comes by a delta", 1);
  r.add("a/+/h/#");
  r.step("H gains a '#' filter (it ends topics of 3 levels with both)", 1);
  r.add("a/+/h2/w");
  r.step("a second literal child", 0);
  r.del("a/+/h2/w");
  r.del("a/+/h");
  r.del("a/+/h/#");
  r.step("all literal children gone", 0);
  r.add("a/+/h2/w");
  r.step("one again, a new node", 1);
  r.del("a/+");
  r.del("a/+/+/z");
  r.del("a/+/h2/w");
  r.step("the '+' child gone", 0);
  r.add("a/+/k/#");
  r.step("a new '+' child with one literal child", 1);
}

}  // namespace

int main() {
  run_cfg3(0, 2, 1);  // every eligible node keyed: site/S/device and site/+/device share D's line
  run_cfg3(0, 1, 1);
  run_cfg3(0, 2, 0);  // no fat buckets: no root half, no copy
  run_cfg3(3, 2, 1);  // 3-bit collision tokens: full home buckets, chains
  run_small(0);
  run_small(3);
  CHECK(g_present > 0 && g_rp_hits > 0 && g_shared > 0, "a rule never applied");
  // the rules only ever remove loads and iterations
  CHECK(g_loads[1] < g_loads[0] && g_iters[1] <= g_iters[0], "loads %llu -> %llu, iterations %llu -> %llu",
        (unsigned long long)g_loads[0], (unsigned long long)g_loads[1], (unsigned long long)g_iters[0],
        (unsigned long long)g_iters[1]);
  fprintf(stderr, "loads %llu -> %llu, lane iterations %llu -> %llu\n", (unsigned long long)g_loads[0],
          (unsigned long long)g_loads[1], (unsigned long long)g_iters[0], (unsigned long long)g_iters[1]);
  printf("OK %llu %llu %llu %llu %llu %llu\n", (unsigned long long)g_commits, (unsigned long long)g_deltas,
         (unsigned long long)g_present, (unsigned long long)g_rp_hits, (unsigned long long)g_shared,
         (unsigned long long)g_rows);
  return 0;
}
