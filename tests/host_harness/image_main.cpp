// image_main.cpp -- TEST INFRASTRUCTURE: the bytes the kernels read, commit by commit.
//
// Built by tests/test_table_image_host.py (tests/host_build.py) under ASan + UBSan against the
// fake HIP runtime of this directory, like harness.cpp.  One engine is driven through a fixed,
// seeded script, and after every commit one line is printed: a 64-bit FNV-1a digest of everything
// the committed index (h->cur->ix) lets a kernel read -- the edge slots, both regions of the exact
// table, the multi lists, the tn side array, the verify bits, the overflow bits and the scalar
// fields of DevIndex (the root's fields and carried halves, masks, flags, bounds; no pointers).
// The lines are compared with tests/golden/table_images.json, recorded at the commit before the
// host model's placement and path code moved into gm_model.h: a change of the host code that
// leaves the table layout alone leaves every line alone.
//
// The script (vocabulary and filter shapes of harness.cpp: ~1500 filters of depth 1 to 6) runs
// four times -- word_hash_bits 0 and 3, crossed with keyed 1 and 2 -- each time on a fresh engine
// that builds in the caller's thread (bg_build 0: one thread, one order):
//   * one full build of the filters whose first level is "a", '+' or '#', so that the root has
//     one literal child, carried in the arguments (the root's fat half);
//   * delta commits (delta_commit 2: every delta that fits is patched) of mixed trie and
//     route-key adds and deletes over all the filters, until at least 24 were patched; the first
//     registers 40000 names that are members of nothing, past the verify bits' headroom;
//   * half-way, a digest of the file emqxgm_snapshot_save writes (with route keys and trie
//     filters only it holds the registry and the model, nothing else);
//   * with delta_commit 0, one more full build of the churned registry.
// Usage: image_main <scratch dir> [--print]
//   --print: the lines as the JSON list that tests/golden/table_images.json holds under "lines".
#include <stdarg.h>

#include "harness_walk.h"

namespace {

struct Fnv {
  uint64_t x = FNV_OFF;
  void raw(const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) x = fnv_step(x, b[i]);
  }
  template <class T>
  void pod(const T& v) {
    raw(&v, sizeof v);
  }
};

uint64_t image(emqxgm* h) {
  const DevIndex& ix = h->cur->ix;
  const TrieModel& m = h->tm;
  CHECK(m.valid, "no model after a commit");
  Fnv d;
  d.raw(ix.edges, (ix.emask + 1) * EBUCKET * SLOT_U4 * sizeof(uint4));
  d.raw(ix.exact, (ix.xmask + 1 + ix.xwmask + 1) * XBUCKET * XENT_U4 * sizeof(uint4));
  d.raw(ix.multi, m.multi.size() * 4);
  d.raw(ix.tn_of, m.tn_cap * 4);
  d.raw(ix.fvbits, m.fv_cap * 4);
  d.raw(ix.xovf, m.xovf.size() * 8);
  d.pod(ix.emask);
  d.pod(ix.root_cf);
  d.pod(ix.root_hf);
  d.pod(ix.root_pcf);
  d.pod(ix.root_phf);
  d.pod(ix.root_sig);
  for (const uint4* q : {&ix.rh0, &ix.rh1, &ix.rp0, &ix.rp1})
    for (uint32_t v : {q->x, q->y, q->z, q->w}) d.pod(v);
  d.pod(ix.xmask);
  d.pod(ix.xwbase);
  d.pod(ix.xwmask);
  d.pod(ix.test_mask);
  d.pod(ix.full_mask);
  d.pod(ix.max_depth);
  d.pod(ix.fid_bound);
  for (bool b : {ix.trie_empty, ix.plain_empty, ix.wild_empty, ix.needs_verify}) d.pod((uint8_t)b);
  d.pod(ix.leafp_mask);
  d.pod(ix.psig_off);
  d.pod(ix.rp_on);
  d.pod(ix.ks_on);
  d.pod(ix.cb_on);
  return d.x;
}

uint64_t file_digest(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  CHECK(f != nullptr, "open %s", path.c_str());
  Fnv d;
  char buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) d.raw(buf, k);
  fclose(f);
  return d.x;
}

std::vector<std::string> g_lines;

void line(const char* fmt, ...) {
  char b[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  g_lines.push_back(b);
}

void run(uint32_t hash_bits, int keyed_mode, const std::string& dir) {
  std::mt19937_64 rng(1000 + 10 * hash_bits + (uint64_t)keyed_mode);
  auto rnd = [&](uint64_t k) { return (uint64_t)(rng() % k); };
  const char* vocab[] = {"a", "b", "", "$x", "c", "dd", "sensor", "long-level-name", "device-0001"};
  auto word = [&]() { return std::string(vocab[rnd(9)]); };
  std::vector<std::string> filters;
  std::set<std::string> seen;
  while (filters.size() < 1500) {
    const uint32_t d = 1 + (uint32_t)rnd(6);
    std::string f;
    for (uint32_t i = 0; i < d; ++i) {
      if (i) f += '/';
      const uint64_t r = rnd(100);
      f += (i + 1 == d && r < 15) ? "#" : (r < 40 ? "+" : word());
    }
    if (seen.insert(f).second) filters.push_back(f);
  }

  emqxgm_cfg cfg{};
  cfg.word_hash_bits = hash_bits;
  emqxgm_t* h = nullptr;
  CHECK(emqxgm_create(&cfg, &h) == 0, "create");
  CHECK(emqxgm_tune(h, "keyed", keyed_mode) == 0 && emqxgm_tune(h, "bg_build", 0) == 0 &&
            emqxgm_tune(h, "delta_commit", 2) == 0,
        "tune");
  std::set<std::string> in_trie, keys;
  auto trie = [&](const std::string& f, bool on) {
    const uint8_t* p = (const uint8_t*)f.data();
    if (on)
      CHECK(emqxgm_trie_insert(h, p, (uint32_t)f.size(), nullptr) == 0, "ins");
    else
      CHECK(emqxgm_trie_delete(h, p, (uint32_t)f.size()) == 0, "del");
    if (on) in_trie.insert(f); else in_trie.erase(f);
  };
  auto key = [&](const std::string& f, bool on) {
    const uint8_t* p = (const uint8_t*)f.data();
    if (on == (keys.count(f) != 0)) return;  // one ref per key
    if (on)
      CHECK(emqxgm_route_ref(h, p, (uint32_t)f.size(), nullptr) == 0, "ref");
    else
      CHECK(emqxgm_route_unref(h, p, (uint32_t)f.size()) == 0, "unref");
    if (on) keys.insert(f); else keys.erase(f);
  };
  uint64_t n_commit = 0;
  auto commit = [&]() {
    emqxgm_stats s0{}, s1{};
    emqxgm_get_stats(h, &s0);
    CHECK(emqxgm_commit(h, nullptr) == 0, "commit: %s", h->err.c_str());
    emqxgm_get_stats(h, &s1);
    const bool delta = s1.delta_commits == s0.delta_commits + 1;
    const bool full = s1.full_commits == s0.full_commits + 1;  // neither: nothing had changed
    line("h%u k%d commit %llu %s %016llx", hash_bits, keyed_mode, (unsigned long long)n_commit++,
         delta ? "delta" : full ? "full" : "none", (unsigned long long)image(h));
    return delta;
  };

  // ---- the full build: the root's only literal child is "a" ----
  for (const std::string& f : filters) {
    if (!(f[0] == '+' || f[0] == '#' || (f[0] == 'a' && (f.size() == 1 || f[1] == '/')))) continue;
    const uint64_t r = rnd(4);
    if (r < 3) trie(f, true);
    if (r >= 2) key(f, true);
  }
  CHECK(!commit(), "the first commit is a full build");
  CHECK(h->tm.fchild[0] != 0, "the root has no fat half");

  // ---- delta commits ----
  const uint64_t want = 24;
  uint64_t deltas = 0;
  bool snapped = false;
  for (int round = 0; round < 600 && deltas < want; ++round) {
    if (round == 0) {
      // names registered past the verify bits' headroom, members of nothing
      for (int i = 0; i < 40000; ++i) {
        const std::string f = "bulk/" + std::to_string(i);
        CHECK(emqxgm_route_ref(h, (const uint8_t*)f.data(), (uint32_t)f.size(), nullptr) == 0, "ref");
        CHECK(emqxgm_route_unref(h, (const uint8_t*)f.data(), (uint32_t)f.size()) == 0, "unref");
      }
    }
    // collision tokens put several keys on one node, which a delta declines: small rounds there
    const int ops = (int)(1 + rnd(hash_bits ? 4 : 120));
    for (int k = 0; k < ops; ++k) {
      const std::string& f = filters[rnd(filters.size())];
      switch (rnd(8)) {
        case 0:
        case 1:
        case 2: trie(f, true); break;
        case 3:
        case 4: trie(f, false); break;
        case 5:
        case 6: key(f, true); break;
        default: key(f, false); break;
      }
    }
    if (commit()) ++deltas;
    if (!snapped && deltas == want / 2) {
      const std::string snap = dir + "/image_" + std::to_string(hash_bits) + "_" +
                               std::to_string(keyed_mode) + ".snap";
      CHECK(emqxgm_snapshot_save(h, snap.c_str()) == 0, "save: %s", h->err.c_str());
      line("h%u k%d snapshot %016llx", hash_bits, keyed_mode, (unsigned long long)file_digest(snap));
      remove(snap.c_str());
      snapped = true;
    }
  }
  CHECK(deltas >= want && snapped, "only %llu delta commits", (unsigned long long)deltas);

  // ---- the churned registry, built in full ----
  CHECK(emqxgm_tune(h, "delta_commit", 0) == 0, "tune");
  trie(filters[0], in_trie.count(filters[0]) == 0);
  CHECK(!commit(), "delta_commit 0 builds in full");
  emqxgm_destroy(h);
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const bool print = argc > 2 && std::string(argv[2]) == "--print";
  for (uint32_t hb : {0u, 3u})
    for (int keyed_mode : {1, 2}) run(hb, keyed_mode, dir);
  if (print) printf("[\n");
  for (size_t i = 0; i < g_lines.size(); ++i)
    printf(print ? "  \"%s\"%s\n" : "%s%s\n", g_lines[i].c_str(), print && i + 1 < g_lines.size() ? "," : "");
  if (print) printf("]\n");
  return 0;
}
