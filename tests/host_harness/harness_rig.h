// harness_rig.h -- TEST INFRASTRUCTURE shared by the walk-rule harnesses (psig_harness.cpp,
// rph_harness.cpp, closed_harness.cpp): an engine handle that patches every delta that fits, the
// oracle beside it, and the row comparison every commit of theirs ends with.  A harness derives
// its Rig from RigBase and adds its own invariant scan, its step() and its churn.
#pragma once
#include "harness_walk.h"

namespace {

uint64_t g_commits = 0, g_deltas = 0, g_rows = 0;

std::string S(uint64_t v) { return std::to_string(v); }

struct RigBase {
  emqxgm_t* h = nullptr;
  Oracle orc;
  std::set<std::string> live;  // the filters in the trie
  std::vector<std::string> topics;
  uint32_t hash_bits = 0;
  int keyed = 1, fat = 1;
  uint64_t counted = 0;  // delta commits of handles this rig has dropped

  RigBase(uint32_t hb, int keyed_mode, int fat_mode) : hash_bits(hb), keyed(keyed_mode), fat(fat_mode) {
    make_handle();
  }
  ~RigBase() {
    g_deltas += counted + deltas();
    emqxgm_destroy(h);
  }
  // for_load: the handle stays fresh (the fat_buckets tune marks a handle changed, and a
  // snapshot loads into a fresh one only)
  void make_handle(bool for_load = false) {
    emqxgm_cfg cfg{};
    cfg.word_hash_bits = hash_bits;
    CHECK(emqxgm_create(&cfg, &h) == 0, "create");
    CHECK(emqxgm_tune(h, "keyed", keyed) == 0, "tune keyed");
    if (for_load)
      h->fat_mode = (uint32_t)fat;
    else
      CHECK(emqxgm_tune(h, "fat_buckets", fat) == 0, "tune fat");
    CHECK(emqxgm_tune(h, "delta_commit", 2) == 0, "tune delta");  // every delta that fits is patched
  }
  void add(const std::string& f) {
    CHECK(emqxgm_trie_insert(h, (const uint8_t*)f.data(), (uint32_t)f.size(), nullptr) == 0, "ins");
    orc.add(f, 1);
    live.insert(f);
  }
  void del(const std::string& f) {
    CHECK(emqxgm_trie_delete(h, (const uint8_t*)f.data(), (uint32_t)f.size()) == 0, "del");
    ref_trie_delete(orc.r, (const uint8_t*)f.data(), (uint32_t)f.size());
    live.erase(f);
  }
  uint64_t deltas() {
    emqxgm_stats st{};
    emqxgm_get_stats(h, &st);
    return st.delta_commits;
  }
  // commits; delta: the commit must have patched the tables in place (collision tokens put
  // several keys on one node: such a delta is declined and built in full).  True after a delta
  // commit.
  bool commit(const char* what, bool delta) {
    const uint64_t d0 = deltas();
    CHECK(emqxgm_commit(h, nullptr) == 0, "%s: commit: %s", what, h->err.c_str());
    ++g_commits;
    if (delta && hash_bits == 0) CHECK(deltas() == d0 + 1, "%s: not a delta commit", what);
    return delta && deltas() == d0 + 1;
  }

  std::vector<uint64_t> tokens(const std::string& s, std::vector<uint8_t>& plus) {
    std::vector<uint64_t> tk;
    std::vector<uint8_t> hs;
    bool hashed;
    tokenize((const uint8_t*)s.data(), (uint32_t)s.size(), h->test_mask, tk, plus, hs, hashed);
    return tk;
  }
  // the model's node at the end of a path of words ("+" = the '+' edge, "" = the root); NONE
  // when the path is not in the trie
  uint32_t node_of(const std::string& path) {
    if (path.empty()) return 0;
    std::vector<uint8_t> pl;
    const std::vector<uint64_t> tk = tokens(path, pl);
    uint32_t cur = 0;
    for (size_t w = 0; w < tk.size(); ++w) {
      const uint32_t* v = h->tm.emap.find(cur, pl[w] ? PLUS_TOK : tk[w]);
      if (!v) return NONE;
      cur = *v;
    }
    return cur;
  }
  uint64_t word_tok(const std::string& word) {
    std::vector<uint8_t> pl;
    return tokens(word, pl)[0];
  }

  // Every topic through the plain reader (CpuWalk): its filters, verified by mqtt_match where
  // fvbits asks for it, equal the oracle's by name.  each(topic, ids) gets the plain reader's
  // ids, sorted: there a harness runs its SlotWalk modes against them.
  template <class Each>
  void rows(const char* what, Each each) {
    std::string tb;
    std::vector<uint32_t> toff(1, 0);
    for (const auto& t : topics) {
      tb += t;
      toff.push_back((uint32_t)tb.size());
    }
    std::vector<uint64_t> row(topics.size() + 1);
    std::vector<uint32_t> rex(topics.size());
    uint32_t* ids = nullptr;
    uint64_t nids = 0;
    ref_match_batch(orc.r, (const uint8_t*)tb.data(), toff.data(), topics.size(), 1, row.data(), &ids,
                    &nids, rex.data());
    const DevIndex& ix = h->cur->ix;
    for (size_t i = 0; i < topics.size(); ++i) {
      CpuWalk w(ix);
      std::vector<uint32_t> base = w.run(topics[i], h->test_mask);
      std::sort(base.begin(), base.end());
      each(topics[i], base);
      std::vector<std::string> gs, ws;
      for (uint32_t f : base) {
        const bool verify = (ix.fvbits[f >> 5] >> (f & 31)) & 1u;
        const std::string fs = filter_str(h, f);
        if (!verify || mqtt_match(topics[i], fs)) gs.push_back(fs);
      }
      for (uint64_t j = row[i]; j < row[i + 1]; ++j) ws.push_back(orc.names[ids[j]]);
      std::sort(gs.begin(), gs.end());
      std::sort(ws.begin(), ws.end());
      CHECK(gs == ws, "%s: topic '%s': %zu vs %zu filters", what, topics[i].c_str(), gs.size(), ws.size());
      ++g_rows;
    }
    ref_free(ids);
  }
  // one SlotWalk run of a rows() hook: its ids must be the plain reader's
  SlotWalk slot_walk(const WalkRules& rules, const char* what, const std::string& topic,
                     const std::vector<uint32_t>& base, const char* mode) {
    SlotWalk sw(h->cur->ix, rules);
    std::vector<uint32_t> got = sw.run(topic, h->test_mask);
    std::sort(got.begin(), got.end());
    CHECK(got == base, "%s: topic '%s': %s: %zu ids, the plain reader %zu", what, topic.c_str(), mode,
          got.size(), base.size());
    return sw;
  }
};

}  // namespace
