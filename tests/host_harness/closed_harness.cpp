// closed_harness.cpp -- TEST INFRASTRUCTURE: closed edge buckets (gm_common.h EDGE_CLOSED), on the CPU.
//
// Built by tests/test_closed_host.py (tests/host_build.py) under ASan + UBSan against the fake HIP
// runtime of this directory, like rph_harness.cpp, and run directly; the rig is harness_rig.h's, the
// restated walk harness_walk.h's SlotWalk, run with the switch cb off and on and with lent, rp
// and ks as the committed index has them (all on).  A cfg3 miniature and a random
// cfg2-like trie are built -- plain and with 3-bit collision tokens, keyed on / auto, fat buckets
// on / off -- and churned by delta commits: inserts whose home bucket is full and closed (the
// word is chosen by its edge_home), deletes, re-inserts into the TOMB slots, a fat half moving
// out, a node gaining and losing its '+' child while its bucket is closed, a background full
// build with catch-up, a snapshot save and load with further deltas.  After every commit:
//   * every live slot of the committed table equals node_slot of its node (model and table
//     agree), and the model's owner array names that node;
//   * no bucket on a live edge's chain before its slot carries a mark or a closed bit;
//   * a mark sits only on a live slot whose node has no '+' child, in a bucket the model has
//     closed; the copies in the arguments carry none that a reader could take for one;
//   * the rows of the plain reader (harness_walk.h CpuWalk), of the restatement of k_walk's
//     iteration with the rule on and off, and of the oracle are equal.
// Prints "OK <commits> <delta commits> <buckets opened by a delta> <inserts past a closed full
// bucket> <lookups stopped at a closed bucket> <row checks>".
#include <unistd.h>

#include <atomic>
#include <thread>

#include "harness_rig.h"

namespace {

uint64_t g_opened = 0, g_past = 0, g_stops = 0, g_marks = 0;
uint64_t g_loads[2] = {0, 0}, g_iters[2] = {0, 0};

// The restated walk as production runs it on the rig's handle -- lent signatures on, "root_plus_half"
// and "keyed_share" as the committed index has them (1) -- with tune "closed_buckets" 0 / 1.
WalkRules closed_rules(const DevIndex& ix, bool on) {
  WalkRules rules(ix);
  rules.cb = on;
  return rules;
}

struct Rig : RigBase {
  std::mt19937_64 rng{5};

  Rig(uint32_t hb, int keyed_mode, int fat_mode) : RigBase(hb, keyed_mode, fat_mode) { tune_key(); }
  // the rule's tune key: accepted values, rejected values
  void tune_key() {
    CHECK(emqxgm_tune(h, "closed_buckets", 0) == 0 && emqxgm_tune(h, "closed_buckets", 1) == 0 &&
              emqxgm_tune(h, "closed_buckets", 2) != 0 && emqxgm_tune(h, "closed_buckets", -1) != 0,
          "tune closed_buckets");
  }

  // every proper prefix of a live filter that ends at a node (its words before a trailing '#')
  std::vector<std::string> prefixes() {
    std::set<std::string> ps;
    for (const auto& f : live) {
      for (size_t i = 0; i <= f.size(); ++i)
        if (i == f.size() || f[i] == '/') {
          const std::string p = f.substr(0, i);
          if (p.size() >= 1 && p.back() != '#') ps.insert(p);
        }
    }
    return std::vector<std::string>(ps.begin(), ps.end());
  }
  bool live_slot(const uint4* q) const { return q[0].z != NONE && q[0].z != TOMB; }
  bool bucket_full(uint64_t b) const {
    const uint4* q = h->cur->ix.edges + SLOT_U4 * EBUCKET * b;
    return live_slot(q) && live_slot(q + SLOT_U4);
  }

  // ---- the invariants of a committed index ----
  void marks(const char* what) {
    const TrieModel& tm = h->tm;
    const DevIndex& ix = h->cur->ix;
    CHECK(tm.valid, "%s: no model", what);
    CHECK(tm.open.size() >= tm.nbk / 64 + 1 && tm.owner.size() == tm.ecap, "%s: bitmap sizes", what);
    const uint32_t nn = (uint32_t)tm.parent.size();
    std::vector<uint32_t> at(tm.ecap, NONE);
    for (uint32_t c = 1; c < nn; ++c) {
      if (tm.slot[c] == DEAD || tm.slot[c] == ROOTH) continue;
      at[tm.slot[c]] = c;
      uint4 want[2];
      tm.node_slot(c, want);
      CHECK(memcmp(want, ix.edges + SLOT_U4 * tm.slot[c], sizeof want) == 0,
            "%s: node %u: its slot in the table is not node_slot", what, c);
      if (tm.half[c]) continue;
      // no mark and no closed bit on the chain before the slot
      for (uint64_t b = tm.home(tm.parent[c], tm.tok[c]); b != tm.slot[c] / EBUCKET; b = (b + 1) & (tm.nbk - 1)) {
        const uint4* q = ix.edges + SLOT_U4 * EBUCKET * b;
        CHECK(bit(tm.open, b), "%s: node %u lies past bucket %llu, which the model has closed", what, c,
              (unsigned long long)b);
        CHECK(!slot_closed(q[0].w, q[1].w, 0) && !slot_closed(q[SLOT_U4].w, q[SLOT_U4 + 1].w, 0),
              "%s: node %u lies past the marked bucket %llu", what, c, (unsigned long long)b);
      }
    }
    for (uint64_t i = 0; i < tm.ecap; ++i) {
      const uint4* q = ix.edges + SLOT_U4 * i;
      CHECK(tm.owner[i] == at[i], "%s: slot %llu: owner", what, (unsigned long long)i);
      CHECK(live_slot(q) == (at[i] != NONE), "%s: slot %llu: live in the table, not in the model", what,
            (unsigned long long)i);
      if (!slot_closed(q[0].w, q[1].w, 0)) continue;
      CHECK(at[i] != NONE, "%s: a mark on the dead slot %llu", what, (unsigned long long)i);
      CHECK(!tm.pchild[at[i]] && !(q[0].w & CF_PLUS), "%s: a mark on a slot with a '+' child", what);
      CHECK(!bit(tm.open, i / EBUCKET), "%s: a mark in a bucket the model has open", what);
      ++g_marks;
    }
    // the copies in the arguments: the root's half has no bucket; the '+' half's copy equals its
    // table slot (rph_harness) and is never probed for a chain
    CHECK(ix.rh1.w != EDGE_CLOSED || (ix.rh0.w & CF_PLUS), "%s: a mark on the root's half", what);
  }

  // the invariants, then the rows: the plain reader's, the restated walk's with the rule off and
  // on (closed_rules), the oracle's
  void checks(const char* what) {
    marks(what);
    rows(what, [&](const std::string& t, const std::vector<uint32_t>& base) {
      for (int on = 0; on < 2; ++on) {
        const SlotWalk sw = slot_walk(closed_rules(h->cur->ix, on != 0), what, t, base,
                                      on ? "closed_buckets 1" : "closed_buckets 0");
        CHECK(on || sw.stops == 0, "%s: the rule applied while off", what);
        g_loads[on] += sw.loads;
        g_iters[on] += sw.iters;
        if (on) g_stops += sw.stops;
      }
    });
  }

  // commit and check; delta: the commit must be a delta commit (with collision tokens one may be
  // declined -- two filters at one node -- and built in full).  Returns the buckets the delta
  // opened, -1 after a full build.
  int64_t step(const char* what, bool delta = true) {
    const std::vector<uint64_t> open0 = h->tm.valid ? h->tm.open : std::vector<uint64_t>();
    int64_t opened = -1;
    if (commit(what, delta)) {
      opened = 0;
      CHECK(open0.size() == h->tm.open.size(), "%s: bitmap resized by a delta", what);
      for (size_t i = 0; i < open0.size(); ++i) {
        CHECK((open0[i] & ~h->tm.open[i]) == 0, "%s: a delta closed a bucket", what);
        opened += __builtin_popcountll(h->tm.open[i] & ~open0[i]);
      }
      g_opened += (uint64_t)opened;
    }
    checks(what);
    return opened;
  }

  // A filter "<P>/<word>/#" whose new edge (P, word) has a full, closed home bucket: the delta
  // commit must place it past that bucket and open it.  The word is searched by its edge_home.
  // Returns the filter added ("" when no parent and word lead to such a bucket).
  std::string insert_past(const char* what) {
    TrieModel& tm = h->tm;
    const std::vector<std::string> ps = prefixes();
    for (int tries = 0; tries < 40000; ++tries) {
      const std::string& P = ps[rng() % ps.size()];
      if (P.find('#') != std::string::npos || (P.find('+') != std::string::npos && tries < 20000)) continue;
      const uint32_t par = node_of(P);
      if (par == NONE || par == 0 || tm.fchild[par]) continue;  // (a fat parent: its half would move first)
      const std::string w = "q" + S(rng() % 100000);
      const uint64_t tok = word_tok(w);
      if (tm.emap.find(par, tok)) continue;
      const uint64_t b = tm.home(par, tok);
      if (!bucket_full(b) || bit(tm.open, b)) continue;
      const std::string f = P + "/" + w + "/#";
      if (live.count(f)) continue;
      add(f);
      topics.push_back(P + "/" + w + "/leaf");
      const int64_t opened = step(what);
      if (opened < 0) return f;  // (built in full: another table)
      const uint32_t c = node_of(P + "/" + w);
      CHECK(c != NONE && h->tm.slot[c] / EBUCKET != b, "%s: the edge did not go past bucket %llu", what,
            (unsigned long long)b);
      CHECK(opened >= 1 && bit(h->tm.open, b), "%s: bucket %llu stayed closed", what, (unsigned long long)b);
      ++g_past;
      return f;
    }
    return "";
  }

  // a node without a '+' child whose slot carries a mark gains one and loses it again
  void plus_child_flip(const char* what) {
    const std::vector<std::string> ps = prefixes();
    for (const std::string& P : ps) {
      if (P.find('+') != std::string::npos) continue;
      const uint32_t x = node_of(P);
      const TrieModel& tm = h->tm;
      if (x == NONE || x == 0 || tm.pchild[x] || tm.slot[x] == DEAD || tm.slot[x] == ROOTH) continue;
      const uint4* q = h->cur->ix.edges + SLOT_U4 * tm.slot[x];
      if (!slot_closed(q[0].w, q[1].w, 0) || !bucket_full(tm.slot[x] / EBUCKET)) continue;
      const std::string f = P + "/+/flip";
      if (live.count(f)) continue;
      add(f);
      topics.push_back(P + "/any/flip");
      if (step((std::string(what) + ": a '+' child comes").c_str()) < 0) return;
      q = h->cur->ix.edges + SLOT_U4 * h->tm.slot[x];
      CHECK((q[0].w & CF_PLUS) && !slot_closed(q[0].w, q[1].w, 0), "%s: the mark stayed under CF_PLUS", what);
      del(f);
      if (step((std::string(what) + ": the '+' child goes").c_str()) < 0) return;
      q = h->cur->ix.edges + SLOT_U4 * h->tm.slot[x];
      CHECK(slot_closed(q[0].w, q[1].w, 0), "%s: the mark did not come back", what);
      return;
    }
    CHECK(hash_bits != 0, "%s: no marked node in a full bucket", what);
  }

  // a fat node takes a second literal child: its half moves out to its own hash position
  void half_moves_out(const char* what) {
    if (!fat) return;
    const std::vector<std::string> ps = prefixes();
    for (const std::string& P : ps) {
      const uint32_t x = node_of(P);
      if (x == NONE || x == 0 || !h->tm.fchild[x]) continue;
      const uint32_t g = h->tm.fchild[x];
      const std::string f = P + "/second/#";
      add(f);
      topics.push_back(P + "/second/leaf");
      if (step(what) >= 0 && hash_bits == 0)
        CHECK(!h->tm.fchild[x] && !h->tm.half[g] && h->tm.slot[g] != DEAD, "%s: the half did not move", what);
      return;
    }
    CHECK(hash_bits != 0, "%s: no fat node", what);
  }

  // a bulk too large for a delta builds in the background; changes committed meanwhile are
  // replayed onto the new tables at the install
  void background_build(const char* what) {
    CHECK(emqxgm_tune(h, "bg_build", 1) == 0 && emqxgm_tune(h, "delta_max", 16) == 0 &&
              emqxgm_tune(h, "delta_commit", 1) == 0 && emqxgm_tune(h, "bg_delay_ms", 300) == 0,
          "tune");
    emqxgm_stats st0{};
    emqxgm_get_stats(h, &st0);
    for (int i = 0; i < 40; ++i) add("bulk/" + S(i % 5) + "/b" + S(i) + "/#");
    topics.push_back("bulk/3/b8/x");
    std::atomic<bool> done{false};
    std::thread committer([&] {
      CHECK(emqxgm_commit(h, nullptr) == 0, "bulk commit: %s", h->err.c_str());
      done = true;
    });
    auto in_flight = [&]() {
      std::lock_guard<std::mutex> g(h->wmu);
      return h->builds_done < h->builds_started;
    };
    for (int k = 0; !in_flight(); ++k) {
      CHECK(!done && k < 200000, "%s: the bulk commit did not build in the background", what);
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    // (delta commits beside the build: small, patched into the tables readers have)
    for (int i = 0; i < 4; ++i) {
      add("during/" + S(i) + "/#");
      CHECK(emqxgm_commit(h, nullptr) == 0, "commit during the build: %s", h->err.c_str());
    }
    del("during/1/#");
    CHECK(emqxgm_commit(h, nullptr) == 0, "commit during the build: %s", h->err.c_str());
    topics.push_back("during/2/x");
    topics.push_back("during/1/x");
    committer.join();
    emqxgm_stats st{};
    emqxgm_get_stats(h, &st);
    // (with collision tokens a small commit may be declined as a delta and wait for the install)
    CHECK(st.bg_builds > st0.bg_builds && (hash_bits != 0 || st.catchup_changes > st0.catchup_changes),
          "%s (hash bits %u keyed %d fat %d): builds %llu, catch-up changes %llu", what, hash_bits, keyed, fat,
          (unsigned long long)(st.bg_builds - st0.bg_builds),
          (unsigned long long)(st.catchup_changes - st0.catchup_changes));
    ++g_commits;
    checks(what);
    CHECK(emqxgm_tune(h, "bg_build", 0) == 0 && emqxgm_tune(h, "delta_max", 0) == 0 &&
              emqxgm_tune(h, "delta_commit", 2) == 0 && emqxgm_tune(h, "bg_delay_ms", 0) == 0,
          "tune");
  }

  // save, load into a fresh handle, go on with that one
  void snapshot(const char* what) {
    char path[] = "/tmp/closed_harness_XXXXXX";
    const int fd = mkstemp(path);
    CHECK(fd >= 0, "mkstemp");
    close(fd);
    CHECK(emqxgm_snapshot_save(h, path) == 0, "%s: save: %s", what, h->err.c_str());
    const std::vector<uint64_t> open0 = h->tm.open;
    counted += deltas();
    emqxgm_destroy(h);
    make_handle(true);
    tune_key();
    CHECK(emqxgm_snapshot_load(h, path) == 0, "%s: load: %s", what, h->err.c_str());
    unlink(path);
    // the loaded bits are derived from the placement: never a bucket closed that an edge passes
    // (marks checks that), and nothing open that the saved model had closed
    CHECK(open0.size() == h->tm.open.size(), "%s: bitmap size", what);
    for (size_t i = 0; i < open0.size(); ++i)
      CHECK((h->tm.open[i] & ~open0[i]) == 0, "%s: the load opened a bucket", what);
    checks(what);
  }

  void churn() {
    step("full build", false);
    std::vector<std::string> added;
    for (int i = 0; i < 3; ++i) {
      const std::string f = insert_past("an insert past a full closed bucket");
      if (!f.empty()) added.push_back(f);
    }
    CHECK(!added.empty(), "no parent and word with a full closed home bucket");
    // deletes (TOMB slots in buckets that stay open), then the same edges again: into the TOMBs
    std::vector<std::string> some(live.begin(), live.end());
    std::shuffle(some.begin(), some.end(), rng);
    some.resize(std::min<size_t>(some.size(), 12));
    for (const auto& f : some) del(f);
    step("deletes");
    for (const auto& f : added)
      if (live.count(f)) del(f);
    step("the displaced edges go");
    for (const auto& f : some) add(f);
    step("re-inserts into TOMB slots");
    for (const auto& f : added) add(f);
    step("the displaced edges come back");
    insert_past("a second round past a full closed bucket");
    half_moves_out("a fat half moves out");
    plus_child_flip("a '+' child under a closed bucket");
    background_build("a background build with catch-up");
    insert_past("past a full closed bucket of the background build");
    snapshot("a snapshot round trip");
    insert_past("past a full closed bucket after the load");
    some.assign(live.begin(), live.end());
    std::shuffle(some.begin(), some.end(), rng);
    some.resize(std::min<size_t>(some.size(), 8));
    for (const auto& f : some) del(f);
    step("deletes after the load");
    for (const auto& f : some) add(f);
    step("re-inserts after the load");
    CHECK(emqxgm_tune(h, "fat_buckets", fat) == 0, "tune");  // (invalidates the model)
    step("a full rebuild of the churned registry", false);
  }
};

// The cfg3 miniature: 6 sites x 40 devices, the workload's five patterns; topics with device
// ids of the own site, of another site and of none.
void run_cfg3(uint32_t hash_bits, int keyed_mode, int fat) {
  Rig r(hash_bits, keyed_mode, fat);
  std::mt19937_64 rng(11 + hash_bits);
  auto dev = [](int s, int j) { return S(s * 1000 + j); };
  for (int s = 0; s < 6; ++s)
    for (int j = 0; j < 40; ++j) {
      const std::string site = "site/" + S(s), d = dev(s, j);
      if (j % 7 != 5) r.add(site + "/device/" + d + "/#");
      if (rng() % 2) r.add("site/+/device/" + d + "/#");
      if (j % 3 == 0)
        for (int k = 0; k < 8; ++k)
          if (rng() % 3 == 0 || k == j % 8) r.add(site + "/device/" + d + "/+/" + S(k));
    }
  for (int s = 0; s < 6; ++s)
    for (int mm = 0; mm < 32; mm += 1 + (int)(rng() % 5)) {
      r.add("site/" + S(s) + "/device/+/m" + S(mm));
      r.add("site/" + S(s) + "/+/+/m" + S((mm + 3) % 32));
    }
  for (int s = 0; s < 6; ++s)
    for (int j = 0; j < 60; j += 3) {
      // (j >= 40: a device id no site has -- the absent probes the rule is for)
      const std::string p = "site/" + S(s) + "/device/" + dev(j % 2 ? s : (s + 1) % 6, j);
      r.topics.push_back(p + "/m" + S(j % 32) + "/" + S(j % 8));
    }
  for (const char* t : {"site", "site/0", "site/0/device", "site/0/other", "site/9/device/0/m1/3",
                        "site/0/device/0/m1/3/a/b/c/d/e/f/g/h/i/j/k", "$site/0/device/0/m1/3", "$site",
                        "site/+/device/0/m1/3", "other/0/device/0/m1/3", "site/0/device/nodev/m1/3"})
    r.topics.push_back(t);
  r.churn();
}

// A random cfg2-like trie: deep filters over a small vocabulary with '+' levels and '#' ends;
// a third of the topic words are in no filter.
void run_random(uint32_t hash_bits, int keyed_mode, int fat) {
  Rig r(hash_bits, keyed_mode, fat);
  std::mt19937_64 rng(23 + hash_bits + 7 * keyed_mode + fat);
  auto word = [&](int lvl) { return "w" + S(lvl) + "_" + S(rng() % (3 + 2 * lvl)); };
  for (int i = 0; i < 700; ++i) {
    const int depth = 2 + (int)(rng() % 6);
    std::string f;
    for (int l = 0; l < depth; ++l) {
      if (l) f += "/";
      f += (l > 0 && rng() % 5 == 0) ? std::string("+") : word(l);
    }
    if (rng() % 3 == 0) f += "/#";
    r.add(f);
  }
  for (int i = 0; i < 220; ++i) {
    const int depth = 2 + (int)(rng() % 7);
    std::string t;
    for (int l = 0; l < depth; ++l) {
      if (l) t += "/";
      t += rng() % 3 == 0 ? "absent" + S(rng() % 50) : word(l);
    }
    r.topics.push_back(t);
  }
  r.churn();
}

// closed_harness --count FILTERS TOPICS: the bucket loads and lane iterations of the census walk
// (one line per filter / topic in the files; every eligible parent keyed, as the device tests
// build their miniatures), with the rule off and on.  A lane's iteration count as k_walk counts
// it: the iteration that creates the root state counts even when it fills no slot.
int count(const char* ffile, const char* tfile) {
  Rig r(0, 2, 1);
  auto lines = [](const char* path) {
    std::vector<std::string> v;
    FILE* f = fopen(path, "r");
    CHECK(f, "open %s", path);
    char buf[4096];
    while (fgets(buf, sizeof buf, f)) {
      std::string l(buf);
      while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
      v.push_back(l);
    }
    fclose(f);
    return v;
  };
  for (const auto& f : lines(ffile)) r.add(f);
  r.topics = lines(tfile);
  r.step("full build", false);
  fprintf(stderr, "%zu nodes, %llu buckets\n", r.h->tm.parent.size(), (unsigned long long)r.h->tm.nbk);
  uint64_t loads[2] = {0, 0}, iters[2] = {0, 0}, stops = 0;
  for (const auto& t : r.topics)
    for (int on = 0; on < 2; ++on) {
      SlotWalk sw(r.h->cur->ix, closed_rules(r.h->cur->ix, on != 0));
      sw.run(t, r.h->test_mask);
      loads[on] += sw.loads;
      iters[on] += sw.walked ? std::max<uint64_t>(sw.iters, 1) : 0;
      stops += sw.stops;
    }
  printf("COUNT %llu %llu %llu %llu %llu\n", (unsigned long long)loads[0], (unsigned long long)iters[0],
         (unsigned long long)loads[1], (unsigned long long)iters[1], (unsigned long long)stops);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "--count") return count(argv[2], argv[3]);
  for (uint32_t hb : {0u, 3u})
    for (int keyed_mode : {2, 1})
      for (int fat : {1, 0}) {
        run_cfg3(hb, keyed_mode, fat);
        run_random(hb, keyed_mode, fat);
      }
  CHECK(g_commits > 0 && g_deltas > 0 && g_opened > 0 && g_past > 0 && g_stops > 0 && g_marks > 0,
        "a count is zero: commits %llu deltas %llu opened %llu past %llu stops %llu marks %llu",
        (unsigned long long)g_commits, (unsigned long long)g_deltas, (unsigned long long)g_opened,
        (unsigned long long)g_past, (unsigned long long)g_stops, (unsigned long long)g_marks);
  // the rule only ever removes loads and iterations
  CHECK(g_loads[1] < g_loads[0] && g_iters[1] <= g_iters[0], "loads %llu -> %llu, iterations %llu -> %llu",
        (unsigned long long)g_loads[0], (unsigned long long)g_loads[1], (unsigned long long)g_iters[0],
        (unsigned long long)g_iters[1]);
  fprintf(stderr, "loads %llu -> %llu, lane iterations %llu -> %llu\n", (unsigned long long)g_loads[0],
          (unsigned long long)g_loads[1], (unsigned long long)g_iters[0], (unsigned long long)g_iters[1]);
  printf("OK %llu %llu %llu %llu %llu %llu\n", (unsigned long long)g_commits, (unsigned long long)g_deltas,
         (unsigned long long)g_opened, (unsigned long long)g_past, (unsigned long long)g_stops,
         (unsigned long long)g_rows);
  return 0;
}
