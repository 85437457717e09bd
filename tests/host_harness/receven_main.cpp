// receven_main.cpp -- TEST HARNESS, not product code: even-elided topic records (gm_common.h:
// two parts {tok1, tok3} {tok4, tok5} and a header bit for each of the words 0 and 2, for an
// index whose literal edges of level 0, and those of level 2, each carry at most one token), on
// the CPU under ASan + UBSan.
//
// Built by tests/test_rec_even_host.py (tests/host_build.py) against the fake HIP runtime of this
// directory, with emqx_amd/csrc/gm_tok.inc included unchanged behind hip_shim.h (as tok_main.cpp
// and recparts_main.cpp have it) and gm_engine.cpp through harness_rig.h.  A stand-alone program,
// run directly.  It checks
//   1. The round trip k_tok's store_rec<EVEN> -> the walk's rec_load_even ->
//      rec_tokens_even, for 1, 63, 64, 65 and 129 topics, plain and non-temporal stores, with
//      c_0 / c_2 inline words, an 8-byte (hashed) c_2, and a level without a token (c = 0): tokens
//      1, 3, 4, 5 and the header word's count and flags exact, T_EQ0 / T_EQ2 set exactly for the
//      topics whose word is there and equal to c_k, tok0 / tok2 rebuilt as c_k for those and 0 for
//      the others (a word one byte off, empty, missing, of 8 bytes), tok6 and wbase 0, part 2,
//      part 3 and the tail of the last block untouched.
//   2. The level state of the host model (TrieModel::lev_st / lev_tok, DevIndex's copy) through a
//      seeded churn of full builds, delta commits, deletions, rebuilds and a snapshot load over
//      indexes of 1 to 8 levels, with inline and collision-test tokens, keyed and fat nodes on and
//      off.  After every commit the state equals one recomputed from the live filters, or is
//      higher where a deletion would have lowered it; within deltas it never moves backwards; a
//      full build and a snapshot load make it exact.  And where a pass would take the form
//      (neither level "many", three parts), the restated walk (harness_walk.h SlotWalk's
//      iteration) fed with tokens that went through store_rec and rec_tokens_even returns the
//      rows of the plain reader -- which rows() holds against the oracle's.
#include <unistd.h>

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

uint64_t g_even = 0, g_three = 0, g_rebuilt0 = 0, g_kept = 0, g_loads = 0;

struct Heap {  // a heap block of exactly `bytes` bytes (ASan guards both ends)
  uint8_t* p;
  size_t bytes;
  explicit Heap(size_t b) : p((uint8_t*)malloc(b)), bytes(b) { memset(p, 0xA5, b); }
  ~Heap() { free(p); }
  Heap(const Heap&) = delete;
};

// a topic's tokens and header word as k_tok computes them (test_mask: collision tokens)
uint32_t tok_topic(const std::string& s, uint64_t test_mask, uint64_t (&tk)[REC_TOKS], std::vector<uint64_t>& all) {
  for (uint64_t& v : tk) v = 0;
  all.clear();
  auto dst = [&](uint32_t k, uint64_t tok) {
    if (k < REC_TOKS) tk[k] = tok;
    all.push_back(tok);
  };
  uint32_t flags = 0;
  const uint32_t nwd = gm::tok_words(gm::GlobBytes{(const uint8_t*)s.data()}, (uint32_t)s.size(), test_mask, dst, flags);
  return nwd | (flags << 24);
}
uint64_t word_token_of(const std::string& w) {
  uint64_t tk[REC_TOKS];
  std::vector<uint64_t> all;
  tok_topic(w, 0, tk, all);
  return tk[0];
}

// ---- 1. store / load round trip ----
std::vector<std::string> trip_topics(uint32_t n, const std::string& w0, const std::string& w2) {
  std::mt19937_64 rng(91 + n);
  auto off_by_one = [](std::string w) {
    w.back() = (char)(w.back() + 1);
    return w;
  };
  std::vector<std::string> ts = {
      w0 + "/7/" + w2 + "/9/m/3", w0, w0 + "/7", w0 + "/7/" + w2, "", "/", "//" + w2, w0 + "//" + w2,
      off_by_one(w0) + "/7/" + w2 + "/9", w0 + "/7/" + off_by_one(w2) + "/9", "/7/" + w2, w0 + "/7//9",
      "eight888/7/" + w2 + "/9", w0 + "/7/eight888/9", "$SYS/" + w0, "$" + w0 + "/7/" + w2,
      w0 + "/+/" + w2 + "/#", w0 + "/7/" + w2 + "/9/m/3/seventh/eighth/ninth", w2 + "/7/" + w0 + "/9"};
  while (ts.size() < n) {
    const uint32_t depth = 1 + (uint32_t)(rng() % 9);
    std::string t;
    for (uint32_t l = 0; l < depth; ++l) {
      if (l) t += "/";
      const uint32_t r = (uint32_t)(rng() % 4);
      if (l == 0 && r) t += r == 3 ? off_by_one(w0) : w0;
      else if (l == 2 && r) t += r == 3 ? off_by_one(w2) : w2;
      else {
        const uint32_t len = (uint32_t)(rng() % 10);  // 0..9 bytes: empty, inline and hashed words
        for (uint32_t i = 0; i < len; ++i) t.push_back((char)('a' + rng() % 26));
      }
    }
    ts.push_back(t);
  }
  ts.resize(n);
  return ts;
}

void round_trip(uint32_t n, bool nt, const std::string& w0, const std::string& w2, bool have0, bool have2) {
  const std::vector<std::string> topics = trip_topics(n, w0, w2);
  const uint64_t c0 = have0 ? word_token_of(w0) : 0ull, c2 = have2 ? word_token_of(w2) : 0ull;
  CHECK((!have0 || c0 != 0) && (!have2 || c2 != 0), "a level token of 0");
  const uint32_t blocks = (n + REC_BLOCK - 1) / REC_BLOCK;
  Heap rec((size_t)blocks * REC_BLOCK * REC_U4 * sizeof(uint4));  // ensure_scratch's size
  Heap hdr((size_t)n * 4);
  uint4* R = (uint4*)rec.p;
  uint32_t* H = (uint32_t*)hdr.p;
  gm::TokArgs A{};
  A.rec = R;
  A.hdr = H;
  A.nt_rec = nt;
  A.c0 = c0;
  A.c2 = c2;
  std::vector<std::vector<uint64_t>> want(n);
  std::vector<uint32_t> whd(n);
  uint32_t ob = 0;
  for (uint32_t t = 0; t < n; ++t) {
    uint64_t tk[REC_TOKS];
    whd[t] = tok_topic(topics[t], 0, tk, want[t]);
    gm::store_rec<true>(A, t, tk, ob + t, whd[t]);
    ob += (uint32_t)topics[t].size();
  }
  const uint4 ZERO4 = make_uint4(0u, 0u, 0u, 0u);
  auto words = [](const std::string& s) {
    std::vector<std::string> w(1);
    for (char ch : s)
      if (ch == '/') w.emplace_back();
      else w.back().push_back(ch);
    return w;
  };
  for (uint32_t t = 0; t < n; ++t) {
    uint4 a = ZERO4, b = ZERO4, c = ZERO4, d = ZERO4;  // (k_walk: nr0..nr3 start as zeros)
    rec_load_even((const uint4*)R, (const uint32_t*)H, t, a, b, d);
    uint64_t tk[REC_TOKS];
    rec_tokens_even(a, b, d.w, c0, c2, tk);
    // the bits from the topic's bytes, not from its tokens
    const std::vector<std::string> w = words(topics[t]);
    const bool eq0 = have0 && w[0] == w0, eq2 = have2 && w.size() > 2 && w[2] == w2;
    const uint32_t hd = whd[t] | (eq0 ? T_EQ0 << 24 : 0u) | (eq2 ? T_EQ2 << 24 : 0u);
    CHECK(d.w == hd, "n %u nt %d topic %u '%s': header %x, want %x", n, (int)nt, t, topics[t].c_str(), d.w, hd);
    CHECK((d.w & 0xFFFFFFu) == w.size() && ((d.w >> 24) & (T_WILD | T_DOLLAR)) == (whd[t] >> 24),
          "n %u topic %u: count or flags", n, t);
    for (uint32_t k : {1u, 3u, 4u, 5u}) {
      const uint64_t x = k < want[t].size() ? want[t][k] : 0ull;
      CHECK(tk[k] == x, "n %u nt %d topic %u token %u: %llx, want %llx", n, (int)nt, t, k,
            (unsigned long long)tk[k], (unsigned long long)x);
    }
    CHECK(tk[0] == (eq0 ? c0 : 0ull) && tk[2] == (eq2 ? c2 : 0ull), "n %u topic %u '%s': tok0 %llx tok2 %llx",
          n, t, topics[t].c_str(), (unsigned long long)tk[0], (unsigned long long)tk[2]);
    if (eq0) CHECK(tk[0] == want[t][0], "topic %u: c0 is not the word's token", t);
    if (eq2) CHECK(tk[2] == want[t][2], "topic %u: c2 is not the word's token", t);
    CHECK(tk[6] == 0 && d.x == 0 && d.y == 0 && d.z == 0 && c.x == 0 && c.y == 0 && c.z == 0 && c.w == 0,
          "n %u topic %u: tok6, wbase or the third part read", n, t);
    g_rebuilt0 += (!eq0 && !want[t].empty() && want[t][0] != 0) + (!eq2 && want[t].size() > 2 && want[t][2] != 0);
    g_kept += eq0 + eq2;
  }
  // parts 2 and 3 are untouched, and so is the unused tail of the last block
  for (uint32_t bl = 0; bl < blocks; ++bl)
    for (uint32_t c = 0; c < REC_U4; ++c)
      for (uint32_t i = 0; i < REC_BLOCK; ++i) {
        const uint32_t t = bl * REC_BLOCK + i;
        const uint4& v = R[(size_t)bl * REC_BLOCK * REC_U4 + c * REC_BLOCK + i];
        const bool stored = t < n && c < REC_PARTS_EVEN;
        const bool sent = v.x == 0xA5A5A5A5u && v.y == 0xA5A5A5A5u && v.z == 0xA5A5A5A5u && v.w == 0xA5A5A5A5u;
        CHECK(stored || sent, "n %u: part %u of slot %u was written", n, c, t);
      }
}

// ---- 2. the level state through a churn, and the walk on reconstructed tokens ----
// SlotWalk::run's loop on tokens that went through the even-elided record (SlotWalk::run
// tokenises inside, so the one change cannot be handed to it): fill, resolve and late match as
// harness_walk.h has them.
struct EvenWalk : SlotWalk {
  using SlotWalk::SlotWalk;
  std::vector<uint32_t> run_even(const std::string& topic, uint64_t test_mask) {
    if (!begin(topic, test_mask)) return out;
    {
      // the topic's record as k_tok stores it and k_walk's activation block reads it
      uint64_t tk[REC_TOKS];
      std::vector<uint64_t> all;
      const uint32_t hd = tok_topic(topic, test_mask, tk, all);
      CHECK(all.size() == n, "topic '%s': %zu tokens, the host tokeniser %u", topic.c_str(), all.size(), n);
      for (uint32_t k = 0; k < n; ++k) CHECK(all[k] == toks[k], "topic '%s': token %u", topic.c_str(), k);
      Heap rec((size_t)REC_BLOCK * REC_U4 * sizeof(uint4));
      Heap hdr(4);
      gm::TokArgs A{};
      A.rec = (uint4*)rec.p;
      A.hdr = (uint32_t*)hdr.p;
      A.c0 = ix.lev_st[0] == LEV_ONE ? ix.lev_tok[0] : 0ull;  // gm_kernels.hip launch_tok / launch_walk
      A.c2 = ix.lev_st[1] == LEV_ONE ? ix.lev_tok[1] : 0ull;
      gm::store_rec<true>(A, 0, tk, 0, hd);
      const uint4 Z = make_uint4(0u, 0u, 0u, 0u);
      uint4 a = Z, b = Z, d = Z;
      rec_load_even((const uint4*)rec.p, (const uint32_t*)hdr.p, 0u, a, b, d);
      uint64_t rk[REC_TOKS];
      rec_tokens_even(a, b, d.w, A.c0, A.c2, rk);
      CHECK((d.w & 0xFFFFFFu) == n, "topic '%s': header count", topic.c_str());
      for (uint32_t k = 0; k < n && k < REC_TOKS; ++k) {
        g_rebuilt0 += rk[k] != toks[k];
        toks[k] = rk[k];
      }
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

struct Lev {
  uint32_t st[2] = {LEV_NONE, LEV_NONE};
  uint64_t tok[2] = {0, 0};
};

struct Rig : RigBase {
  Lev prev;
  Rig(uint32_t hb, int keyed_mode, int fat_mode) : RigBase(hb, keyed_mode, fat_mode) {
    CHECK(emqxgm_tune(h, "rec_even", 0) == 0 && emqxgm_tune(h, "rec_even", 2) != 0 &&
              emqxgm_tune(h, "rec_even", -1) != 0 && emqxgm_tune(h, "rec_even", 1) == 0,
          "tune rec_even");
  }
  // the state from the live filters alone: the tokens of their literal words 0 and 2 (a trailing
  // '#' is no level)
  Lev scratch() {
    Lev L;
    std::set<uint64_t> seen[2];
    for (const std::string& f : live) {
      std::vector<uint8_t> pl;
      const std::vector<uint64_t> tk = tokens(f, pl);
      const size_t len = f.back() == '#' && (f.size() == 1 || f[f.size() - 2] == '/') ? tk.size() - 1 : tk.size();
      for (uint32_t i = 0; i < 2; ++i)
        if (2 * i < len && !pl[2 * i]) seen[i].insert(tk[2 * i]);
    }
    for (uint32_t i = 0; i < 2; ++i) {
      L.st[i] = seen[i].empty() ? LEV_NONE : (seen[i].size() > 1 || *seen[i].begin() == 0) ? LEV_MANY : LEV_ONE;
      L.tok[i] = L.st[i] == LEV_ONE ? *seen[i].begin() : 0;
    }
    return L;
  }
  // exact: the commit was a full build or a snapshot load
  void check_state(const char* what, bool was_delta) {
    const DevIndex& ix = h->cur->ix;
    const Lev want = scratch();
    for (uint32_t i = 0; i < 2; ++i) {
      const uint32_t st = ix.lev_st[i];
      CHECK(st == h->tm.lev_st[i] && st <= LEV_MANY, "%s: level %u: index %u, model %u", what, 2 * i, st, h->tm.lev_st[i]);
      CHECK(ix.lev_tok[i] == (st == LEV_ONE ? h->tm.lev_tok[i] : 0ull), "%s: level %u: token", what, 2 * i);
      CHECK(st != LEV_ONE || ix.lev_tok[i] != 0, "%s: level %u: one token, 0", what, 2 * i);
      // never below what the live filters need; equal after a full build
      CHECK(st >= want.st[i], "%s: level %u: state %u, the live filters need %u", what, 2 * i, st, want.st[i]);
      if (st == LEV_ONE && want.st[i] == LEV_ONE)
        CHECK(ix.lev_tok[i] == want.tok[i], "%s: level %u: token %llx, live %llx", what, 2 * i,
              (unsigned long long)ix.lev_tok[i], (unsigned long long)want.tok[i]);
      if (!was_delta)
        CHECK(st == want.st[i], "%s: level %u: state %u after a full build, want %u", what, 2 * i, st, want.st[i]);
      else
        CHECK(st >= prev.st[i] && (st != LEV_ONE || prev.st[i] != LEV_ONE || ix.lev_tok[i] == prev.tok[i]),
              "%s: level %u: state %u after %u within deltas", what, 2 * i, st, prev.st[i]);
      prev.st[i] = st;
      prev.tok[i] = ix.lev_tok[i];
    }
  }
  void walks(const char* what) {
    const DevIndex& ix = h->cur->ix;
    const WalkRules rules(ix);
    CHECK(rules.lent && rules.rp && rules.ks && rules.cb, "%s: a walk rule is off", what);
    // pass_enqueue's condition, the walk variant aside
    const bool even = rec_parts(ix.max_depth) == REC_PARTS_MIN && ix.lev_st[0] != LEV_MANY && ix.lev_st[1] != LEV_MANY;
    rows(what, [&](const std::string& t, const std::vector<uint32_t>& base) {
      const SlotWalk sw = slot_walk(rules, what, t, base, "full tokens");
      if (!even) {
        ++g_three;
        return;
      }
      EvenWalk ew(ix, rules);
      std::vector<uint32_t> got = ew.run_even(t, h->test_mask);
      std::sort(got.begin(), got.end());
      CHECK(got == base, "%s: topic '%s': reconstructed tokens: %zu ids, full tokens %zu", what, t.c_str(),
            got.size(), base.size());
      // (a reconstructed 0 may fall into another signature class than the word it stands for:
      // a probe more or a probe less, never a row; counted)
      g_loads += ew.loads > sw.loads ? ew.loads - sw.loads : sw.loads - ew.loads;
      ++g_even;
    });
  }
  void step(const char* what, bool delta) {
    const bool was_delta = commit(what, delta);
    check_state(what, was_delta);
    walks(what);
  }
  void rebuild(const char* what) {
    CHECK(emqxgm_tune(h, "fat_buckets", fat) == 0, "tune");  // (invalidates the model)
    prev = Lev();
    step(what, false);
  }
  void snapshot(const char* what) {
    char path[] = "/tmp/receven_main_XXXXXX";
    const int fd = mkstemp(path);
    CHECK(fd >= 0, "mkstemp");
    close(fd);
    CHECK(emqxgm_snapshot_save(h, path) == 0, "%s: save: %s", what, h->err.c_str());
    counted += deltas();
    emqxgm_destroy(h);
    make_handle(true);
    CHECK(emqxgm_snapshot_load(h, path) == 0, "%s: load: %s", what, h->err.c_str());
    unlink(path);
    ++g_commits;
    check_state(what, false);  // derived from the node arrays: exact for the live edges
    walks(what);
  }
};

// an index of `depth` levels shaped site/<s>/device/<d>/m<k>/<j>/x/y, cut at `depth`
void run_depth(uint32_t depth, uint32_t hash_bits, int keyed_mode, int fat) {
  Rig r(hash_bits, keyed_mode, fat);
  std::mt19937_64 rng(5 + 13 * depth + hash_bits + 7 * keyed_mode + fat);
  auto cut = [&](const std::string& s, uint32_t d) {
    size_t pos = 0;
    for (uint32_t l = 0; l < d; ++l) {
      pos = s.find('/', pos);
      if (pos == std::string::npos) return s;
      ++pos;
    }
    return s.substr(0, pos - 1);
  };
  const char* wc2 = depth % 2 ? "device88" : "device";  // odd depths: c_2 is an 8-byte (hashed) word
  auto full = [&](int s, int d, int k, int j) {
    return "site/" + S(s) + "/" + wc2 + "/" + S(d) + "/m" + S(k) + "/" + S(j) + "/x/y";
  };
  for (int s = 0; s < 4; ++s)
    for (int d = 0; d < 18; ++d) {
      r.add(cut(full(s, 100 * s + d, d % 5, d % 3), depth));
      if (depth > 2 && rng() % 2) r.add(cut("site/+/" + std::string(wc2) + "/" + S(100 * s + d) + "/+/" + S(d % 3) + "/x/y", depth));
      if (depth > 3 && rng() % 3 == 0) r.add(cut(full(s, 100 * s + d, d % 5, d % 3), depth - 1) + "/#");
      if (depth > 1 && rng() % 4 == 0) r.add(cut("+/" + S(s) + "/+/" + S(100 * s + d) + "/m" + S(d % 5), depth));
    }
  for (int s = 0; s < 5; ++s)
    for (int d = 0; d < 18; d += 2) {
      const std::string t = full(s, 100 * (d % 3 ? s : (s + 1) % 4) + d, d % 5, d % 3);
      r.topics.push_back(cut(t, 1 + (uint32_t)(rng() % 9)));
      r.topics.push_back(cut(t, depth));
    }
  for (const std::string t : {std::string(""), std::string("/"), std::string("site"), std::string("sitf/0/") + wc2 + "/0/m0/0",
                              std::string("site/0/devicf/0/m0/0"), std::string("site/0/") + wc2 + "9/0/m0/0",
                              std::string("/0/") + wc2 + "/0/m0/0", std::string("site/0//0/m0/0"),
                              std::string("eight888/0/") + wc2 + "/0/m0/0", std::string("site/0/eight888/0/m0/0"),
                              std::string("$SYS"), std::string("$SYS/0/") + wc2 + "/0", std::string("$site/0/") + wc2 + "/0/m0/0",
                              std::string("site/+/") + wc2 + "/0", std::string("other/0/") + wc2 + "/0/m0/0",
                              std::string("site/0/other/0/m0/0"), std::string("site/0"), std::string("site/0/") + wc2})
    r.topics.push_back(t);
  r.add("#");  // (no level: every name that is no '$' name has a row, which the oracle's batch call needs)
  r.step("full build", false);
  // deletions and re-inserts that leave the levels' tokens where they are
  std::vector<std::string> some(r.live.begin(), r.live.end());
  some.erase(std::find(some.begin(), some.end(), "#"));
  std::shuffle(some.begin(), some.end(), rng);
  some.resize(std::min<size_t>(some.size(), 12));
  for (const auto& f : some) r.del(f);
  r.step("deletes", true);
  for (const auto& f : some) r.add(f);
  r.step("re-inserts", true);
  // a second token at level 0, by a delta: many from here; its deletion leaves the state
  const std::string o0 = cut("other/0/" + std::string(wc2) + "/0/m0/0/x/y", depth);
  r.add(o0);
  r.step("a second token at level 0", true);
  r.del(o0);
  r.step("and gone again", true);
  r.rebuild("a rebuild lowers level 0");
  if (depth >= 3) {
    const std::string o2 = cut("site/0/other/0/m0/0/x/y", depth);
    r.add(o2);
    r.step("a second token at level 2", true);
    r.del(o2);
    r.step("and gone again", true);
    r.snapshot("a snapshot load lowers level 2");
    // under the root's '+' child too: a literal edge of level 2 all the same
    const std::string p2 = cut("+/0/third/0/m0/0/x/y", depth);
    r.add(p2);
    r.step("a second token at level 2 under +", true);
    r.del(p2);
    r.rebuild("a rebuild lowers level 2");
  }
  // a '$' name's key of level 0 (tn) is a literal edge of level 0
  r.add("$SYS");
  r.step("a tn key of level 0", true);
  r.del("$SYS");
  r.rebuild("and rebuilt without it");
  // the empty word at level 0: its token is 0 without collision tokens -- many, though one
  for (const std::string& f : std::vector<std::string>(r.live.begin(), r.live.end()))
    if (f != "#") r.del(f);
  r.add(cut("/0/" + std::string(wc2) + "/0/m0/0/x/y", depth));
  r.add(cut("/+/" + std::string(wc2) + "/1/m0/0/x/y", depth));
  r.topics.push_back(cut("/0/" + std::string(wc2) + "/0/m0/0/x/y", depth));
  r.topics.push_back(cut("/0/" + std::string(wc2) + "/1/m0/0/x/y", depth));
  r.step("only the empty word at level 0", true);
  r.rebuild("and rebuilt");
  if (hash_bits == 0) CHECK(r.h->cur->ix.lev_st[0] == LEV_MANY, "depth %u: the empty word counts as many", depth);
  // filters of one and two levels only: level 2 has no token at all
  for (const std::string& f : std::vector<std::string>(r.live.begin(), r.live.end()))
    if (f != "#") r.del(f);
  r.add("site");
  r.add("site/+");
  r.add("site/7");
  r.add("site/#");
  r.rebuild("one and two levels");
  CHECK(r.h->cur->ix.lev_st[1] == LEV_NONE && r.h->cur->ix.lev_st[0] == LEV_ONE, "depth %u: none at level 2", depth);
}

}  // namespace

int main() {
  for (uint32_t n : {1u, 63u, 64u, 65u, 129u})
    for (int nt = 0; nt < 2; ++nt) {
      round_trip(n, nt != 0, "site", "device", true, true);
      round_trip(n, nt != 0, "site", "device88", true, true);   // c_2 an 8-byte (hashed) word
      round_trip(n, nt != 0, "site", "device", true, false);    // level 2 without a token
      round_trip(n, nt != 0, "site", "device", false, false);   // neither
    }
  for (uint32_t depth = 1; depth <= 8; ++depth)
    for (uint32_t hb : {0u, 3u})
      for (int keyed_mode : {2, 1})
        for (int fat : {1, 0}) run_depth(depth, hb, keyed_mode, fat);
  CHECK(g_commits > g_deltas && g_deltas > 0 && g_rows > 0 && g_even > 0 && g_three > 0 && g_rebuilt0 > 0 && g_kept > 0,
        "a count is zero: commits %llu deltas %llu rows %llu even %llu three %llu rebuilt %llu kept %llu",
        (unsigned long long)g_commits, (unsigned long long)g_deltas, (unsigned long long)g_rows,
        (unsigned long long)g_even, (unsigned long long)g_three, (unsigned long long)g_rebuilt0,
        (unsigned long long)g_kept);
  printf("OK %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)g_commits, (unsigned long long)g_deltas,
         (unsigned long long)g_rows, (unsigned long long)g_even, (unsigned long long)g_three,
         (unsigned long long)g_rebuilt0, (unsigned long long)g_loads);
  return 0;
}
