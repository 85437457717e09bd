// recparts_main.cpp -- TEST INFRASTRUCTURE: topic records stored and loaded in the parts the
// index can read (gm_common.h rec_parts), on the CPU under ASan + UBSan.
//
// Built by tests/test_rec_parts_host.py (tests/host_build.py) against the fake HIP runtime of this
// directory and run directly.  emqx_amd/csrc/gm_tok.inc is included unchanged behind hip_shim.h,
// as tok_main.cpp includes it; its three constants from gm_kernels.hip come from
// build/tok_consts.inc.  Three parts:
//   1. rec_parts(max_depth) for max_depth 0..10, printed ("parts ...") for the test to compare.
//   2. The round trip of a 64-topic block and of a ragged tail (101 topics) for each supported
//      part count, plain and non-temporal stores: every topic is tokenised by gm_tok.inc's
//      tok_words, stored by its store_rec and loaded by gm_common.h's rec_load / rec_tokens -- the
//      walk's loader.  The record and header arrays are heap blocks of exactly the sizes the
//      engine allocates and are filled with a sentinel first: tokens below 2P come back, the rest
//      read 0, the header word is equal, wbase is there exactly when P = REC_U4, and what the mode
//      does not store (the fourth part, or the header array) still holds the sentinel.
//   3. The property the partial records rest on: the walk reads level token k only for
//      k < max_depth.  harness_walk.h's SlotWalk iteration is run with the tokens from level
//      max_depth on zeroed (ZeroedWalk below restates SlotWalk::run's loop around that one change;
//      create, bucket and visit are SlotWalk's own) and must give the rows of SlotWalk with full
//      tokens, which harness_rig.h compares with the plain reader's and the oracle's.  A cfg3
//      miniature and a random trie are churned by full builds and delta commits: deletions that
//      leave max_depth where it was, deltas that deepen the index from 6 to 7 and 8 levels (one
//      of them ending in an empty level, whose token is 0 like a token not stored), a rebuild
//      that makes it shallow again.  Checked after every commit, every rule of WalkRules on.
// Prints "OK <commits> <delta commits> <row checks> <topics walked at 3 parts> <at 4 parts>
// <tokens zeroed>".
#include "harness_rig.h"

#include "hip_shim.h"

namespace gm {
namespace {
#include "build/tok_consts.inc"
inline uint32_t lane_id() { return threadIdx.x & 63u; }
inline uint32_t mbcnt64(uint64_t) { return 0u; }
#include "../../emqx_amd/csrc/gm_tok.inc"
}  // namespace
}  // namespace gm

namespace {

uint64_t g_p3 = 0, g_p4 = 0, g_zeroed = 0;

// ---- 1. the table ----
void parts_table() {
  printf("parts");
  for (uint32_t d = 0; d <= 10; ++d) {
    const uint32_t p = rec_parts(d);
    CHECK(p >= REC_PARTS_MIN && p <= REC_U4, "rec_parts(%u) = %u", d, p);
    CHECK((p == REC_U4) == (d >= REC_TOKS), "rec_parts(%u) = %u: all parts exactly from %u levels on", d, p, REC_TOKS);
    CHECK(2 * p >= std::min(d, REC_TOKS), "rec_parts(%u) = %u: a readable token is not stored", d, p);
    printf(" %u", p);
  }
  printf("\n");
}

// ---- 2. store / load round trip ----
struct Heap {  // a heap block of exactly `bytes` bytes (ASan guards both ends)
  uint8_t* p;
  size_t bytes;
  explicit Heap(size_t b) : p((uint8_t*)malloc(b)), bytes(b) { memset(p, 0xA5, b); }
  ~Heap() { free(p); }
  Heap(const Heap&) = delete;
};

std::vector<std::string> trip_topics(uint32_t n) {
  std::mt19937_64 rng(77 + n);
  std::vector<std::string> ts = {"", "/", "$", "$SYS/a", "a/+/b", "a//b///c", "w1/w2/w3/w4/w5/w6/w7",
                                 "seven77/eight888/x", "a/b/c/d/e/f/g/h/i/j", "a/b/c/d/e/seven77",
                                 "a/b/c/d/e/eight888", "a/b/c/d/e/f/eight888/h"};
  while (ts.size() < n) {
    const uint32_t depth = 1 + (uint32_t)(rng() % 9);
    std::string t;
    for (uint32_t l = 0; l < depth; ++l) {
      if (l) t += "/";
      const uint32_t len = (uint32_t)(rng() % 10);  // 0..9 bytes: empty, inline and hashed words
      for (uint32_t i = 0; i < len; ++i) t.push_back((char)('a' + rng() % 26));
    }
    ts.push_back(t);
  }
  ts.resize(n);
  return ts;
}

void round_trip(uint32_t n, uint32_t P, bool nt) {
  const std::vector<std::string> topics = trip_topics(n);
  const uint32_t blocks = (n + REC_BLOCK - 1) / REC_BLOCK;
  Heap rec((size_t)blocks * REC_BLOCK * REC_U4 * sizeof(uint4));  // ensure_scratch's size
  Heap hdr((size_t)n * 4);
  uint4* R = (uint4*)rec.p;
  uint32_t* H = (uint32_t*)hdr.p;
  gm::TokArgs A{};
  A.rec = R;
  A.hdr = P >= REC_U4 ? nullptr : H;  // gm_kernels.hip launch_tok
  A.nt_rec = nt;
  std::vector<std::vector<uint64_t>> want(n);
  std::vector<uint32_t> whd(n), wwb(n);
  uint32_t ob = 0;
  for (uint32_t t = 0; t < n; ++t) {
    const std::string& s = topics[t];
    uint64_t tk[REC_TOKS] = {0, 0, 0, 0, 0, 0, 0};
    std::vector<uint64_t>& all = want[t];
    auto dst = [&](uint32_t k, uint64_t tok) {
      if (k < REC_TOKS) tk[k] = tok;
      all.push_back(tok);
    };
    uint32_t flags = 0;
    const uint32_t nwd = gm::tok_words(gm::GlobBytes{(const uint8_t*)s.data()}, (uint32_t)s.size(), 0, dst, flags);
    wwb[t] = ob + t;  // k_tok: off[t] + t
    whd[t] = nwd | (flags << 24);
    gm::store_rec(A, t, tk, wwb[t], whd[t]);
    ob += (uint32_t)s.size();
  }
  const uint4 ZERO4 = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t t = 0; t < n; ++t) {
    uint4 a = ZERO4, b = ZERO4, c = ZERO4, d = ZERO4;  // (k_walk: nr0..nr3 start as zeros)
    if (P >= REC_U4)
      rec_load<true>((const uint4*)R, (const uint32_t*)nullptr, t, a, b, c, d);
    else
      rec_load<false>((const uint4*)R, (const uint32_t*)H, t, a, b, c, d);
    uint64_t tk[REC_TOKS];
    rec_tokens(a, b, c, d, tk);
    for (uint32_t k = 0; k < REC_TOKS; ++k) {
      const uint64_t w = (k < 2 * P && k < want[t].size()) ? want[t][k] : 0ull;
      CHECK(tk[k] == w, "n %u P %u nt %d topic %u token %u: %llx, want %llx", n, P, (int)nt, t, k,
            (unsigned long long)tk[k], (unsigned long long)w);
    }
    CHECK(d.w == whd[t], "n %u P %u topic %u: header %x, want %x", n, P, t, d.w, whd[t]);
    CHECK(d.z == (P >= REC_U4 ? wwb[t] : 0u), "n %u P %u topic %u: wbase %u", n, P, t, d.z);
  }
  // what the mode does not store is untouched, and so is the unused tail of the last block
  for (uint32_t bl = 0; bl < blocks; ++bl)
    for (uint32_t c = 0; c < REC_U4; ++c)
      for (uint32_t i = 0; i < REC_BLOCK; ++i) {
        const uint32_t t = bl * REC_BLOCK + i;
        const uint4& v = R[(size_t)bl * REC_BLOCK * REC_U4 + c * REC_BLOCK + i];
        const bool stored = t < n && c < P;
        const bool sent = v.x == 0xA5A5A5A5u && v.y == 0xA5A5A5A5u && v.z == 0xA5A5A5A5u && v.w == 0xA5A5A5A5u;
        CHECK(stored || sent, "n %u P %u: part %u of slot %u was written", n, P, c, t);
      }
  if (P >= REC_U4)
    for (uint32_t t = 0; t < n; ++t) CHECK(H[t] == 0xA5A5A5A5u, "n %u: header array written with full records", n);
}

// ---- 3. the walk reads no token from level max_depth on ----
// SlotWalk::run's loop with toks[k] = 0 for k >= from (SlotWalk::run tokenises inside, so the one
// change cannot be handed to it): fill, resolve and late match as harness_walk.h has them.
struct ZeroedWalk : SlotWalk {
  using SlotWalk::SlotWalk;
  std::vector<uint32_t> run_zeroed(const std::string& topic, uint64_t test_mask, uint32_t from) {
    if (!begin(topic, test_mask)) return out;
    for (uint32_t k = from; k < n; ++k) {
      g_zeroed += toks[k] != 0;
      toks[k] = 0;
    }
    const uint4 rh[2] = {ix.rh0, ix.rh1};
    create(ix.root_cf, dollar ? NONE : ix.root_hf, NONE, ix.root_sig, ix.root_pcf, ix.root_phf, 0,
           !dollar, false, (ix.rh0.z & CF_ID_MASK) == FAT_ID, rh, 1);
    Slot P[2];
    while (!stk.empty() || P[0].busy || P[1].busy) {
      ++iters;
      CHECK(iters < 100000, "topic '%s': the walk does not end", topic.c_str());
      uint32_t shk = NONE;
      bool stop = false;
      for (uint32_t j = 0; j < 2; ++j) {
        Slot& p = P[j];
        if (p.busy || stk.empty() || stop) continue;
        if (j > 0 && shk != NONE && (stk.back().first & IT_KIND) == IT_KEYED && stk.back().second == shk) {
          stop = true;
          continue;
        }
        const auto it = stk.back();
        stk.pop_back();
        const uint32_t kind = it.first & IT_KIND;
        p.busy = true;
        p.cur = it.first;
        p.k = it.second;
        p.side = kind == IT_TN || (kind != IT_PLUS && it.second >= REC_TOKS);
        // the claim itself: a literal item's level has a stored token
        CHECK(kind == IT_PLUS || kind == IT_TN || it.second < from, "topic '%s': a literal item of level %u, tokens from %u",
              topic.c_str(), it.second, from);
        if (kind == IT_PLUS) p.key = PLUS_TOK;
        else if (kind != IT_TN) p.key = toks[it.second];
        if (j == 0 && rules.ks && kind == IT_KEYED && it.second < REC_TOKS) shk = it.second;
        if (!p.side) p.ia = edge_home(it.first & CF_ID_MASK, p.key, ix.emask, kind == IT_KEYED);
      }
      const size_t sh_lo = (shk != NONE && !stk.empty()) ? stk.size() - 1 : stk.size();
      const uint64_t line0 = P[0].ia;
      for (uint32_t j = 0; j < 2; ++j) loads += P[j].busy && !P[j].side;
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
      if (shk != NONE) {
        for (size_t i = sh_lo; i < stk.size(); ++i) {
          if ((stk[i].first & IT_KIND) != IT_KEYED || stk[i].second != shk) continue;
          const uint32_t node = stk[i].first & CF_ID_MASK;
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

struct Rig : RigBase {
  Rig(uint32_t hb, int keyed_mode, int fat_mode) : RigBase(hb, keyed_mode, fat_mode) {
    CHECK(emqxgm_tune(h, "rec_parts", 0) == 0 && emqxgm_tune(h, "rec_parts", 4) == 0 &&
              emqxgm_tune(h, "rec_parts", 3) != 0 && emqxgm_tune(h, "rec_parts", 5) != 0 &&
              emqxgm_tune(h, "rec_parts", -1) != 0 && emqxgm_tune(h, "rec_parts", 0) == 0,
          "tune rec_parts");
  }
  uint32_t depth() const { return h->cur->ix.max_depth; }
  // commit, then the rows: plain reader = oracle (rows), SlotWalk with full tokens = plain
  // reader (slot_walk), SlotWalk with the tokens from max_depth on zeroed = the same, its loads
  // and iterations included.  want_depth: the committed max_depth (0: not asserted)
  void step(const char* what, bool delta, uint32_t want_depth) {
    // (with collision tokens a delta may be declined and built in full: another depth)
    const bool as_asked = commit(what, delta) == delta;
    const DevIndex& ix = h->cur->ix;
    if (want_depth && as_asked) CHECK(ix.max_depth == want_depth, "%s: max_depth %u, want %u", what, ix.max_depth, want_depth);
    const uint32_t P = rec_parts(ix.max_depth);
    const WalkRules rules(ix);
    CHECK(rules.lent && rules.rp && rules.ks && rules.cb, "%s: a walk rule is off", what);
    rows(what, [&](const std::string& t, const std::vector<uint32_t>& base) {
      const SlotWalk sw = slot_walk(rules, what, t, base, "full tokens");
      ZeroedWalk zw(ix, rules);
      std::vector<uint32_t> got = zw.run_zeroed(t, h->test_mask, ix.max_depth);
      std::sort(got.begin(), got.end());
      CHECK(got == base, "%s: topic '%s': tokens zeroed from level %u: %zu ids, full tokens %zu", what,
            t.c_str(), ix.max_depth, got.size(), base.size());
      CHECK(zw.loads == sw.loads && zw.iters == sw.iters && zw.shared == sw.shared && zw.rp_hits == sw.rp_hits,
            "%s: topic '%s': loads %llu / %llu, iterations %llu / %llu", what, t.c_str(),
            (unsigned long long)zw.loads, (unsigned long long)sw.loads, (unsigned long long)zw.iters,
            (unsigned long long)sw.iters);
      (P >= REC_U4 ? g_p4 : g_p3) += 1;
    });
  }
};

void deepen_and_back(Rig& r, const std::string& p6, uint32_t base_depth) {
  // p6: a live path of base_depth - 1 levels to hang deeper filters under
  std::mt19937_64 rng(3);
  r.step("full build", false, base_depth);
  // deletions and re-inserts that leave max_depth where it was, the deepest filters among them
  std::vector<std::string> some(r.live.begin(), r.live.end());
  std::shuffle(some.begin(), some.end(), rng);
  some.resize(std::min<size_t>(some.size(), 10));
  for (const auto& f : r.live)
    if ((uint32_t)std::count(f.begin(), f.end(), '/') + 1 == base_depth && f.back() != '#' && some.size() < 40)
      some.push_back(f);
  std::sort(some.begin(), some.end());
  some.erase(std::unique(some.begin(), some.end()), some.end());
  for (const auto& f : some) r.del(f);
  r.step("deletes", true, base_depth);
  for (const auto& f : some) r.add(f);
  r.step("re-inserts", true, base_depth);
  // one level deeper, ending in an empty level (its token is 0, as a token not stored reads)
  std::string f7 = p6, f8;
  for (uint32_t l = base_depth - 1; l < 6; ++l) f7 += "/x" + S(l);
  const std::string g7 = "+" + f7.substr(f7.find('/'));  // the same path under the root's '+'
  r.add(f7 + "/");            // 7 levels, the last one empty
  r.add(f7 + "/seven77");     // 7 levels, a 7-byte word
  r.add(g7 + "/");            // (wildcard filters: the ones emqx_trie:match returns)
  r.add(g7 + "/seven77");
  r.topics.push_back(f7 + "/");
  r.topics.push_back(f7 + "/seven77");
  r.topics.push_back(f7 + "/other");
  r.topics.push_back(f7);
  r.step("a delta to 7 levels", true, 7);
  f8 = f7 + "/eight888/last";  // 8 levels: the 8-byte word is hashed, the last level comes from wh
  r.add(f8);
  r.add(f7 + "/+/last");
  r.add(g7 + "/eight888/last");
  r.topics.push_back(f8);
  r.topics.push_back(f7 + "/eight888/nolast");
  r.topics.push_back(f7 + "/eight888/last/deeper");
  r.step("a delta to 8 levels", true, 8);
  // the deep filters go: a delta leaves max_depth, a rebuild brings the shallow index back
  for (const std::string& f : {f7 + "/", f7 + "/seven77", g7 + "/", g7 + "/seven77", f8, f7 + "/+/last",
                               g7 + "/eight888/last"})
    r.del(f);
  r.step("the deep filters go", true, 8);
  CHECK(emqxgm_tune(r.h, "fat_buckets", r.fat) == 0, "tune");  // (invalidates the model)
  r.step("a full rebuild", false, base_depth);
  r.add(f7 + "/");
  r.step("7 levels again, into the rebuilt tables", true, 7);
}

// the cfg3 miniature of closed_harness.cpp: six levels
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
      const std::string p = "site/" + S(s) + "/device/" + dev(j % 2 ? s : (s + 1) % 6, j);
      r.topics.push_back(p + "/m" + S(j % 32) + "/" + S(j % 8));
      if (j % 9 == 0) r.topics.push_back(p + "/m" + S(j % 32) + "/" + S(j % 8) + "/seventh/eighth");
    }
  for (const char* t : {"site", "site/0", "site/0/device", "site/0/other", "site/9/device/0/m1/3",
                        "site/0/device/0/m1/3/a/b/c/d/e/f/g/h/i/j/k", "$site/0/device/0/m1/3", "$site",
                        "site/+/device/0/m1/3", "other/0/device/0/m1/3", "site/0/device/nodev/m1/3",
                        "site/0/device/0/m1/", "site/0/device/0//3", "site/0/device/0/m1/3/"})
    r.topics.push_back(t);
  deepen_and_back(r, "site/0/device/0/m1", 6);
}

// a random trie of at most five levels ('#' ends aside), then deepened the same way
void run_random(uint32_t hash_bits, int keyed_mode, int fat) {
  Rig r(hash_bits, keyed_mode, fat);
  std::mt19937_64 rng(29 + hash_bits + 7 * keyed_mode + fat);
  auto word = [&](int lvl) { return "w" + S(lvl) + "_" + S(rng() % (3 + 2 * lvl)); };
  r.add("w0_0/w1_0/w2_0/w3_0/w4_0");  // five levels for certain
  for (int i = 0; i < 400; ++i) {
    const int depth = 2 + (int)(rng() % 4);
    std::string f;
    for (int l = 0; l < depth; ++l) {
      if (l) f += "/";
      f += (l > 0 && rng() % 5 == 0) ? std::string("+") : word(l);
    }
    if (rng() % 3 == 0 && depth < 5) f += "/#";
    r.add(f);
  }
  for (int i = 0; i < 160; ++i) {
    const int depth = 1 + (int)(rng() % 9);
    std::string t;
    for (int l = 0; l < depth; ++l) {
      if (l) t += "/";
      t += rng() % 4 == 0 ? "absent" + S(rng() % 50) : word(std::min(l, 4));
    }
    r.topics.push_back(t);
  }
  deepen_and_back(r, "w0_0/w1_0/w2_0/w3_0", 5);
}

}  // namespace

int main() {
  parts_table();
  for (uint32_t n : {64u, 101u, 1u, 63u, 65u, 129u})
    for (uint32_t P = REC_PARTS_MIN; P <= REC_U4; ++P)
      for (int nt = 0; nt < 2; ++nt) round_trip(n, P, nt != 0);
  for (uint32_t hb : {0u, 3u})
    for (int keyed_mode : {2, 1})
      for (int fat : {1, 0}) {
        run_cfg3(hb, keyed_mode, fat);
        run_random(hb, keyed_mode, fat);
      }
  CHECK(g_commits > g_deltas && g_deltas > 0 && g_rows > 0 && g_p3 > 0 && g_p4 > 0 && g_zeroed > 0,
        "a count is zero: commits %llu deltas %llu rows %llu p3 %llu p4 %llu zeroed %llu",
        (unsigned long long)g_commits, (unsigned long long)g_deltas, (unsigned long long)g_rows,
        (unsigned long long)g_p3, (unsigned long long)g_p4, (unsigned long long)g_zeroed);
  printf("OK %llu %llu %llu %llu %llu %llu\n", (unsigned long long)g_commits, (unsigned long long)g_deltas,
         (unsigned long long)g_rows, (unsigned long long)g_p3, (unsigned long long)g_p4,
         (unsigned long long)g_zeroed);
  return 0;
}
