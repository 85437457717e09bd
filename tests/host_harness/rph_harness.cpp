// rph_harness.cpp -- TEST INFRASTRUCTURE: the root's '+' half (gm_kernels.h DevIndex::rp0/rp1) and
// the shared line of keyed siblings (gm_walk.inc SHARE), on the CPU.
//
// Built by tests/test_rph_host.py with g++ -fsanitize=address,undefined against the fake HIP
// runtime of this directory, like psig_harness.cpp.  After a full build and after every step of a
// delta churn it checks that
//   * rp0/rp1 is absent, or equals node_slot of the only live literal child H of the '+' child p
//     of the root's half G -- and equals H's slot in the committed table (the copy is a cache);
//     where a step says so, that it is present (a build with one such child) or absent (a second
//     literal child under G/+ clears it in that same commit);
//   * a restatement of k_walk's iteration -- two probe slots filled from the LIFO, one bucket per
//     slot and round trip, resolves in slot order, then the late match -- returns the same rows
//     with the two rules on and off, equal to the rows of the reader that knows neither
//     (harness_walk.h, unchanged) and to the oracle's.
// Prints "OK <commits> <delta commits> <copies present> <copy hits> <shared items> <row checks>".
#include "harness_walk.h"

namespace {

uint64_t g_commits = 0, g_deltas = 0, g_present = 0, g_rp_hits = 0, g_shared = 0, g_rows = 0;
uint64_t g_loads[2] = {0, 0}, g_iters[2] = {0, 0};

// k_walk's iteration restated: the fill and resolve order of gm_walk.inc with NS = 2 slots.
struct SlotWalk {
  const DevIndex& ix;
  const bool rp_on, ks_on;
  std::vector<uint64_t> toks;
  uint32_t n = 0;
  bool dollar = false;
  std::vector<uint32_t> out;
  std::vector<std::pair<uint32_t, uint32_t>> stk;  // (node | item kind, level)
  uint64_t loads = 0, iters = 0, rp_hits = 0, shared = 0;
  static constexpr uint32_t IT_PLUS = 0x80000000u, IT_TN = 0x40000000u;
  static constexpr uint32_t IT_KEYED = IT_PLUS | IT_TN, IT_KIND = IT_PLUS | IT_TN;
  struct Slot {
    bool busy = false, side = false;
    uint32_t cur = 0, k = 0;
    uint64_t key = 0, ia = 0;
  };

  SlotWalk(const DevIndex& x, bool rp, bool ks) : ix(x), rp_on(rp), ks_on(ks) {}
  void em(uint32_t v) {
    if (v == NONE) return;
    if (v & LIST_MULTI) {
      const uint32_t i = v & ~LIST_MULTI, c = ix.multi[i];
      for (uint32_t j = 0; j < c; ++j) out.push_back(ix.multi[i + 1 + j]);
    } else {
      out.push_back(v);
    }
  }
  uint32_t strip(uint32_t cf, uint32_t d) const {
    const uint32_t h = cf_depth_code(cf & ix.leafp_mask);
    return (h != 0u && (int)(n - d) > (int)h) ? (cf & ~(CF_LIT | CF_PLUS)) : cf;
  }
  void visit(uint32_t cf, uint32_t hf, uint32_t tw, uint32_t d, bool lit, uint32_t kind = 0) {
    if (hf != NONE) em(hf);
    if (d == n) {
      if (cf & CF_TW) em(tw);
      if (lit && (cf & CF_TN) && dollar && n == 1) stk.push_back({IT_TN | (cf & CF_ID_MASK), d});
    } else if (cf & CF_LIT) {
      stk.push_back({(cf & CF_ID_MASK) | kind, d});
    }
  }
  // rp: 1 = the root's state, 2 = its fat half's (gm_walk.inc create RP)
  void create(uint32_t cf, uint32_t hf, uint32_t tw, uint32_t sig, uint32_t pcf, uint32_t phf,
              uint32_t d, bool plus_ok, bool lit, bool fat = false, const uint4* h = nullptr,
              uint32_t rp = 0) {
    const bool keyed = sig == 0u && (cf & CF_LIT);
    cf = strip(cf, d);
    const uint64_t wtok = d < REC_TOKS ? (d < n ? toks[d] : 0ull) : 0ull;
    const bool fat_go = fat && (cf & CF_LIT) && d < n && d < REC_TOKS &&
                        (uint32_t)wtok == h[0].x && (uint32_t)(wtok >> 32) == h[0].y;
    if (fat || (!keyed && d < REC_TOKS && !(sig & sig_bit(wtok)))) cf &= ~CF_LIT;
    pcf = strip(pcf, d + 1);
    visit(cf, hf, tw, d, lit, keyed ? IT_KEYED : 0u);
    if (fat_go)
      create(h[0].w, h[1].x, h[1].y, h[0].z >> SIG_SHIFT, h[1].z, h[1].w, d + 1, true, true, false,
             nullptr, rp == 1 ? 2u : 0u);
    if (!plus_ok || d >= n || !(cf & CF_PLUS)) return;
    const bool ptw = (pcf & CF_PTW) != 0;
    if (d + 1 == n && (pcf & CF_TW) && !ptw) {
      stk.push_back({IT_PLUS | (cf & CF_ID_MASK), d});
      return;
    }
    const uint32_t rpz = rp_on ? ix.rp0.z : NONE;  // (launch_walk: the tune masks the copy)
    const bool r = rp == 2 && (rpz & CF_ID_MASK) == (pcf & CF_ID_MASK) && (pcf & CF_LIT) && d + 1 < n;
    if (r) pcf &= ~CF_LIT;
    visit(pcf & ~CF_PTW, ptw ? NONE : phf, ptw ? phf : NONE, d + 1, false);
    if (r && (uint32_t)toks[d + 1] == ix.rp0.x && (uint32_t)(toks[d + 1] >> 32) == ix.rp0.y) {
      ++rp_hits;
      create(ix.rp0.w, ix.rp1.x, ix.rp1.y, ix.rp0.z >> SIG_SHIFT, ix.rp1.z, ix.rp1.w, d + 2, true, true);
    }
    if (d + 1 < n && (pcf & CF_PLUS)) stk.push_back({IT_PLUS | (pcf & CF_ID_MASK), d + 1});
  }
  // one bucket against (node, key): 1 hit (s, fat, hh filled), 0 an empty slot, -1 full of others
  int bucket(uint64_t b, uint32_t node, uint64_t key, uint4 s[2], bool& fat, uint4 hh[2]) const {
    const uint4* q = ix.edges + SLOT_U4 * EBUCKET * b;
    for (uint32_t j = 0; j < EBUCKET; ++j)
      if ((q[SLOT_U4 * j].z & CF_ID_MASK) == node && q[SLOT_U4 * j].x == (uint32_t)key &&
          q[SLOT_U4 * j].y == (uint32_t)(key >> 32)) {
        s[0] = q[SLOT_U4 * j];
        s[1] = q[SLOT_U4 * j + 1];
        fat = j == 0 && (q[SLOT_U4].z & CF_ID_MASK) == FAT_ID;
        if (fat) {
          hh[0] = q[SLOT_U4];
          hh[1] = q[SLOT_U4 + 1];
        }
        return 1;
      }
    return (q[0].z == NONE || q[SLOT_U4].z == NONE) ? 0 : -1;
  }
  std::vector<uint32_t> run(const std::string& topic, uint64_t test_mask) {
    std::vector<uint8_t> pl, hs;
    bool hashed;
    tokenize((const uint8_t*)topic.data(), (uint32_t)topic.size(), test_mask, toks, pl, hs, hashed);
    n = (uint32_t)toks.size();
    out.clear();
    stk.clear();
    for (size_t i = 0; i < n; ++i)
      if (pl[i] || hs[i]) return out;
    if (ix.trie_empty) return out;
    dollar = !topic.empty() && topic[0] == '$';
    const uint4 rh[2] = {ix.rh0, ix.rh1};
    create(ix.root_cf, dollar ? NONE : ix.root_hf, NONE, ix.root_sig, ix.root_pcf, ix.root_phf, 0,
           !dollar, false, (ix.rh0.z & CF_ID_MASK) == FAT_ID, rh, 1);
    Slot P[2];
    while (!stk.empty() || P[0].busy || P[1].busy) {
      ++iters;
      CHECK(iters < 100000, "topic '%s': the walk does not end", topic.c_str());
      // ---- fill ----
      uint32_t shk = NONE;
      bool stop = false;
      for (uint32_t j = 0; j < 2; ++j) {
        Slot& p = P[j];
        if (p.busy || stk.empty() || stop) continue;
        if (j > 0 && shk != NONE && (stk.back().first & IT_KIND) == IT_KEYED && stk.back().second == shk) {
          stop = true;  // a keyed sibling of slot 0's probe stays on the stack
          continue;
        }
        const auto it = stk.back();
        stk.pop_back();
        const uint32_t kind = it.first & IT_KIND;
        p.busy = true;
        p.cur = it.first;
        p.k = it.second;
        p.side = kind == IT_TN || (kind != IT_PLUS && it.second >= REC_TOKS);
        if (kind == IT_PLUS) p.key = PLUS_TOK;
        else if (kind != IT_TN) p.key = toks[it.second];
        if (j == 0 && ks_on && kind == IT_KEYED && it.second < REC_TOKS) shk = it.second;
        if (!p.side) p.ia = edge_home(it.first & CF_ID_MASK, p.key, ix.emask, kind == IT_KEYED);
      }
      const size_t sh_lo = (shk != NONE && !stk.empty()) ? stk.size() - 1 : stk.size();
      const uint64_t line0 = P[0].ia;  // slot 0's line of this round trip
      for (uint32_t j = 0; j < 2; ++j) loads += P[j].busy && !P[j].side;
      // ---- resolve ----
      for (uint32_t j = 0; j < 2; ++j) {
        Slot& p = P[j];
        if (!p.busy) continue;
        if (p.side) {
          p.side = false;
          if ((p.cur & IT_KIND) == IT_TN) {
            p.busy = false;
            em(ix.tn_of[p.cur & CF_ID_MASK]);
          } else {
            p.ia = edge_home(p.cur & CF_ID_MASK, p.key, ix.emask, (p.cur & IT_KIND) == IT_KEYED);
          }
          continue;
        }
        uint4 s[2], hh[2];
        bool fat = false;
        const int r = bucket(p.ia, p.cur & CF_ID_MASK, p.key, s, fat, hh);
        if (r == 1) {
          p.busy = false;
          create(s[0].w, s[1].x, s[1].y, s[0].z >> SIG_SHIFT, s[1].z, s[1].w, p.k + 1, true,
                 (p.cur & IT_KIND) != IT_PLUS, fat, hh);
        } else if (r == 0) {
          p.busy = false;
        } else {
          p.ia = (p.ia + 1) & ix.emask;
        }
      }
      // ---- the late match: the first keyed item of slot 0's level against slot 0's line ----
      if (shk != NONE) {
        for (size_t i = sh_lo; i < stk.size(); ++i) {
          if ((stk[i].first & IT_KIND) != IT_KEYED || stk[i].second != shk) continue;
          const uint32_t node = stk[i].first & CF_ID_MASK;
          CHECK(edge_home(node, toks[shk], ix.emask, true) == line0, "keyed siblings, two homes");
          uint4 s[2], hh[2];
          bool fat = false;
          const int r = bucket(line0, node, toks[shk], s, fat, hh);
          if (r != -1) {
            ++shared;
            stk[i] = stk.back();
            stk.pop_back();
          }
          if (r == 1)
            create(s[0].w, s[1].x, s[1].y, s[0].z >> SIG_SHIFT, s[1].z, s[1].w, shk + 1, true, true, fat, hh);
          break;
        }
      }
    }
    return out;
  }
};

struct Rig {
  emqxgm_t* h = nullptr;
  Oracle orc;
  std::vector<std::string> topics;
  uint32_t hash_bits = 0;
  int fat = 1;

  Rig(uint32_t hb, int keyed_mode, int fat_mode) : hash_bits(hb), fat(fat_mode) {
    emqxgm_cfg cfg{};
    cfg.word_hash_bits = hb;
    CHECK(emqxgm_create(&cfg, &h) == 0, "create");
    CHECK(emqxgm_tune(h, "keyed", keyed_mode) == 0, "tune keyed");
    CHECK(emqxgm_tune(h, "fat_buckets", fat) == 0, "tune fat");
    CHECK(emqxgm_tune(h, "delta_commit", 2) == 0, "tune delta");
    // the new keys: accepted values, rejected values
    CHECK(emqxgm_tune(h, "root_plus_half", 0) == 0 && emqxgm_tune(h, "root_plus_half", 1) == 0 &&
              emqxgm_tune(h, "root_plus_half", 2) != 0, "tune root_plus_half");
    CHECK(emqxgm_tune(h, "keyed_share", 0) == 0 && emqxgm_tune(h, "keyed_share", 1) == 0 &&
              emqxgm_tune(h, "keyed_share", -1) != 0, "tune keyed_share");
  }
  ~Rig() {
    g_deltas += deltas();
    emqxgm_destroy(h);
  }
  void add(const std::string& f) {
    CHECK(emqxgm_trie_insert(h, (const uint8_t*)f.data(), (uint32_t)f.size(), nullptr) == 0, "ins");
    orc.add(f, 1);
  }
  void del(const std::string& f) {
    CHECK(emqxgm_trie_delete(h, (const uint8_t*)f.data(), (uint32_t)f.size()) == 0, "del");
    ref_trie_delete(orc.r, (const uint8_t*)f.data(), (uint32_t)f.size());
  }
  uint64_t deltas() {
    emqxgm_stats st{};
    emqxgm_get_stats(h, &st);
    return st.delta_commits;
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

  void rows(const char* what) {
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
      for (int mode = 0; mode < 4; ++mode) {
        SlotWalk sw(ix, (mode & 1) != 0, (mode & 2) != 0);
        std::vector<uint32_t> got = sw.run(topics[i], h->test_mask);
        std::sort(got.begin(), got.end());
        CHECK(got == base, "%s: topic '%s': rules %d: %zu ids, the plain reader %zu", what,
              topics[i].c_str(), mode, got.size(), base.size());
        if (mode == 0 || mode == 3) {
          g_loads[mode == 3] += sw.loads;
          g_iters[mode == 3] += sw.iters;
        }
        if (mode == 3) {
          g_rp_hits += sw.rp_hits;
          g_shared += sw.shared;
        }
      }
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

  void step(const char* what, int want, bool delta = true) {
    if (!fat && want == 1) want = 0;  // without fat buckets the root has no half, so no copy
    const uint64_t d0 = deltas();
    CHECK(emqxgm_commit(h, nullptr) == 0, "%s: commit: %s", what, h->err.c_str());
    ++g_commits;
    if (delta && hash_bits == 0) CHECK(deltas() == d0 + 1, "%s: not a delta commit", what);
    copy(what, want);
    rows(what);
  }
};

std::string S(uint64_t v) { return std::to_string(v); }

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
