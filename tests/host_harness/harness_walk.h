// harness_walk.h -- TEST INFRASTRUCTURE shared by the host harnesses (harness.cpp, bg_harness.cpp
// and, through harness_rig.h, psig_harness.cpp, rph_harness.cpp, closed_harness.cpp): the
// engine's host code itself (gm_engine.cpp, included), the walk of gm_walk.inc and the probe of
// k_exact restated on the CPU over the committed tables, emqx_topic:match/2 on strings, and the
// oracle's C++ restatement (oracle/ref_trie.cpp) as the checker.
//
// Two readers of the committed edge table live here, and only here:
//   * CpuWalk, the plain reader: one probe after the other, every bucket of a chain up to an
//     empty slot, and none of the walk's rules;
//   * SlotWalk, the one restatement of k_walk's iteration (two probe slots, one bucket per slot
//     and round trip), with the rules of gm_walk.inc behind the switches of WalkRules: lent
//     signatures, the root's '+' half, the shared line of keyed siblings, closed buckets.
// They share what WalkBase holds -- tokens, the item stack, what a state lists -- and nothing
// that creates a state's children or probes the table: a harness compares the rows of one with
// the rows of the other.
#pragma once
#include <stdio.h>

#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_engine.cpp"

extern "C" {
void* ref_create(int compact);
void ref_destroy(void* h);
int ref_add_many(void* h, const uint8_t* bytes, const uint64_t* off, uint64_t n, const uint8_t* kind);
int ref_trie_delete(void* h, const uint8_t* p, uint32_t len);
int ref_route_delete(void* h, const uint8_t* p, uint32_t len);
int ref_match_batch(void* h, const uint8_t* tb, const uint32_t* toff, uint64_t n, int threads,
                    uint64_t* row, uint32_t** ids_out, uint64_t* n_ids, uint32_t* exact);
void ref_free(void* p);
}

namespace {

#define CHECK(c, ...)                                             \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
      fprintf(stderr, __VA_ARGS__);                               \
      fprintf(stderr, "\n");                                      \
      exit(1);                                                    \
    }                                                             \
  } while (0)

// emqx_topic:match/2 on bytes (gm_kernels.hip mqtt_match, the '$' clauses included)
bool mqtt_match(const std::string& t, const std::string& f) {
  if (!t.empty() && t[0] == '$' && !f.empty() && (f[0] == '+' || f[0] == '#')) return false;
  std::vector<std::string> tw, fw;
  auto split = [](const std::string& s, std::vector<std::string>& w) {
    size_t a = 0;
    for (size_t i = 0; i <= s.size(); ++i)
      if (i == s.size() || s[i] == '/') {
        w.push_back(s.substr(a, i - a));
        a = i + 1;
      }
  };
  split(t, tw);
  split(f, fw);
  for (size_t i = 0; i < fw.size(); ++i) {
    if (fw[i] == "#" && i + 1 == fw.size()) return true;
    if (i >= tw.size()) return false;
    if (fw[i] != "+" && fw[i] != tw[i]) return false;
  }
  return tw.size() == fw.size();
}

std::string filter_str(emqxgm* h, uint32_t id) {
  // the registry lock, as the engine's readers take it (a commit may move the arrays: r06
  // reserves room for the deltas ahead)
  std::shared_lock<std::shared_mutex> g(h->pmu);
  const Filter& f = h->filters[id];
  return std::string((const char*)h->pool.data() + f.off, f.len);
}

// What the two readers below share: a topic's tokens, the item stack, what a state lists.
struct WalkBase {
  const DevIndex& ix;
  std::vector<uint64_t> toks;
  uint32_t n = 0;
  bool dollar = false;
  std::vector<uint32_t> out;
  std::vector<std::pair<uint32_t, uint32_t>> stk;  // (node | item kind, level)
  static constexpr uint32_t IT_PLUS = 0x80000000u, IT_TN = 0x40000000u;
  static constexpr uint32_t IT_KEYED = IT_PLUS | IT_TN, IT_KIND = IT_PLUS | IT_TN;

  explicit WalkBase(const DevIndex& x) : ix(x) {}
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
  // tokenises the topic and clears the output; false when no walk starts: a wildcard topic
  // name -> [] (emqx_trie.erl:157-166), or an empty trie
  bool begin(const std::string& topic, uint64_t test_mask) {
    std::vector<uint8_t> pl, hs;
    bool hashed;
    tokenize((const uint8_t*)topic.data(), (uint32_t)topic.size(), test_mask, toks, pl, hs, hashed);
    n = (uint32_t)toks.size();
    out.clear();
    stk.clear();
    for (size_t i = 0; i < n; ++i)
      if (pl[i] || hs[i]) return false;
    if (ix.trie_empty) return false;
    dollar = !topic.empty() && topic[0] == '$';
    return true;
  }
};

// The walk of gm_walk.inc over the committed tables, on the CPU: the plain reader.
struct CpuWalk : WalkBase {
  using WalkBase::WalkBase;
  // fat: the state's only literal child comes with it in {h0, h1} (gm_common.h FAT_ID)
  void create(uint32_t cf, uint32_t hf, uint32_t tw, uint32_t sig, uint32_t pcf, uint32_t phf,
              uint32_t d, bool plus_ok, bool lit, bool fat = false, const uint4* h = nullptr) {
    const bool keyed = sig == 0u && (cf & CF_LIT);  // gm_common.h edge_home
    cf = strip(cf, d);
    const uint64_t wtok = d < REC_TOKS ? (d < n ? toks[d] : 0ull) : 0ull;
    const bool fat_go = fat && (cf & CF_LIT) && d < n && d < REC_TOKS &&
                        (uint32_t)wtok == h[0].x && (uint32_t)(wtok >> 32) == h[0].y;
    if (fat || (!keyed && d < REC_TOKS && !(sig & sig_bit(wtok)))) cf &= ~CF_LIT;
    pcf = strip(pcf, d + 1);
    visit(cf, hf, tw, d, lit, keyed ? IT_KEYED : 0u);
    if (fat_go)
      create(h[0].w, h[1].x, h[1].y, h[0].z >> SIG_SHIFT, h[1].z, h[1].w, d + 1, true, true);
    if (!plus_ok || d >= n || !(cf & CF_PLUS)) return;
    const bool ptw = (pcf & CF_PTW) != 0;  // the carried copy holds the child's tw, no hf
    if (d + 1 == n && (pcf & CF_TW) && !ptw) {
      stk.push_back({IT_PLUS | (cf & CF_ID_MASK), d});
      return;
    }
    visit(pcf & ~CF_PTW, ptw ? NONE : phf, ptw ? phf : NONE, d + 1, false);
    if (d + 1 < n && (pcf & CF_PLUS)) stk.push_back({IT_PLUS | (pcf & CF_ID_MASK), d + 1});
  }
  // the edge slot of (node, key): probes buckets like k_walk (a bucket with an empty slot ends)
  // fat: the hit is a bucket's first slot and the second holds its fat half (copied to h)
  bool probe(uint32_t node, uint64_t key, bool keyed, uint4 s[2], bool& fat, uint4 h[2]) const {
    for (uint64_t b = edge_home(node, key, ix.emask, keyed);; b = (b + 1) & ix.emask) {
      bool empty = false;
      for (uint32_t j = 0; j < EBUCKET; ++j) {
        const uint4* q = ix.edges + SLOT_U4 * (EBUCKET * b + j);
        if ((q[0].z & CF_ID_MASK) == node && q[0].x == (uint32_t)key &&
            q[0].y == (uint32_t)(key >> 32)) {
          s[0] = q[0];
          s[1] = q[1];
          fat = j == 0 && (q[SLOT_U4].z & CF_ID_MASK) == FAT_ID;
          if (fat) {
            h[0] = q[SLOT_U4];
            h[1] = q[SLOT_U4 + 1];
          }
          return true;
        }
        empty = empty || q[0].z == NONE;
      }
      if (empty) return false;
    }
  }
  std::vector<uint32_t> run(const std::string& topic, uint64_t test_mask) {
    if (!begin(topic, test_mask)) return out;
    const uint4 rh[2] = {ix.rh0, ix.rh1};
    create(ix.root_cf, dollar ? NONE : ix.root_hf, NONE, ix.root_sig, ix.root_pcf, ix.root_phf, 0,
           !dollar, false, (ix.rh0.z & CF_ID_MASK) == FAT_ID, rh);
    while (!stk.empty()) {
      const auto it = stk.back();
      stk.pop_back();
      const uint32_t kind = it.first & IT_KIND;
      if (kind == IT_TN) {
        em(ix.tn_of[it.first & CF_ID_MASK]);
        continue;
      }
      const uint32_t node = it.first & CF_ID_MASK, k = it.second;
      const uint64_t key = kind == IT_PLUS ? PLUS_TOK : toks[k];
      uint4 s[2], hh[2];
      bool fat = false;
      const bool hit = probe(node, key, kind == IT_KEYED, s, fat, hh);
      if (getenv("HH_TRACE")) fprintf(stderr, "probe node %u k %u plus %d -> %d fat %d\n", node, k, (it.first & IT_PLUS) ? 1 : 0, hit ? 1 : 0, fat ? 1 : 0);
      if (hit)
        create(s[0].w, s[1].x, s[1].y, s[0].z >> SIG_SHIFT, s[1].z, s[1].w, k + 1, true,
               kind != IT_PLUS, fat, hh);
    }
    return out;
  }
};

// The rules of gm_walk.inc that SlotWalk has, each behind a switch.  The defaults are the
// committed index's, as launch_walk reads them (gm_kernels.hip); a harness overrides the ones it
// compares.
struct WalkRules {
  bool lent;  // lent signatures drop literal probes under a carried '+' child (tune "plus_sig")
  bool rp;    // the root's '+' half rides in the arguments (tune "root_plus_half")
  bool ks;    // keyed siblings of one level are decided from one line (tune "keyed_share")
  bool cb;    // a missed lookup ends at a closed bucket (tune "closed_buckets")
  explicit WalkRules(const DevIndex& ix)
      : lent(ix.psig_off == 0u), rp(ix.rp_on != 0u), ks(ix.ks_on != 0u), cb(ix.cb_on != 0u) {}
};

// k_walk's iteration restated: the fill and resolve order of gm_walk.inc with NS = 2 slots, as
// the compact one-lane-per-topic walks and the census have it.
struct SlotWalk : WalkBase {
  const WalkRules rules;
  uint64_t loads = 0, iters = 0;  // bucket loads, iterations of the lane
  uint64_t stops = 0;             // lookups ended at a closed bucket
  uint64_t rp_hits = 0;           // states created from the copy rp0/rp1
  uint64_t shared = 0;            // keyed siblings decided from slot 0's line
  bool walked = false;  // the topic reached the walk (not a wildcard name, the trie not empty)
  struct Slot {
    bool busy = false, side = false;
    uint32_t cur = 0, k = 0;
    uint64_t key = 0, ia = 0;
  };

  SlotWalk(const DevIndex& x, const WalkRules& r) : WalkBase(x), rules(r) {}
  explicit SlotWalk(const DevIndex& x) : SlotWalk(x, WalkRules(x)) {}
  // rp: 1 = the root's state, 2 = its fat half's (gm_walk.inc create RP)
  void create(uint32_t cf, uint32_t hf, uint32_t tw, uint32_t sig, uint32_t pcf, uint32_t phf,
              uint32_t d, bool plus_ok, bool lit, bool fat = false, const uint4* h = nullptr,
              uint32_t rp = 0) {
    const bool keyed = sig == 0u && (cf & CF_LIT);
    // (lent signatures, gm_common.h: with CF_LIT clear the field summarises the '+' child's children)
    const uint32_t lent = ((cf & CF_LIT) || !rules.lent) ? 0x3Fu : sig;
    cf = strip(cf, d);
    const uint64_t wtok = d < REC_TOKS ? (d < n ? toks[d] : 0ull) : 0ull;
    const uint64_t ptok = d + 1 < n ? toks[d + 1] : 0ull;
    const bool fat_go = fat && (cf & CF_LIT) && d < n && d < REC_TOKS &&
                        (uint32_t)wtok == h[0].x && (uint32_t)(wtok >> 32) == h[0].y;
    if (fat || (!keyed && d < REC_TOKS && !(sig & sig_bit(wtok)))) cf &= ~CF_LIT;
    pcf = strip(pcf, d + 1);
    if (d + 1 < REC_TOKS && !(lent & sig_bit(ptok))) pcf &= ~CF_LIT;
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
    const uint32_t rpz = rules.rp ? ix.rp0.z : NONE;  // (launch_walk: the tune masks the copy)
    const bool r = rp == 2 && (rpz & CF_ID_MASK) == (pcf & CF_ID_MASK) && (pcf & CF_LIT) && d + 1 < n;
    if (r) pcf &= ~CF_LIT;
    visit(pcf & ~CF_PTW, ptw ? NONE : phf, ptw ? phf : NONE, d + 1, false);
    if (r && (uint32_t)toks[d + 1] == ix.rp0.x && (uint32_t)(toks[d + 1] >> 32) == ix.rp0.y) {
      ++rp_hits;
      create(ix.rp0.w, ix.rp1.x, ix.rp1.y, ix.rp0.z >> SIG_SHIFT, ix.rp1.z, ix.rp1.w, d + 2, true, true);
    }
    if (d + 1 < n && (pcf & CF_PLUS)) stk.push_back({IT_PLUS | (pcf & CF_ID_MASK), d + 1});
  }
  // one bucket against (node, key): 1 hit (s, fat, hh filled), 0 the chain ends here (an empty
  // slot, or -- rules.cb -- a closed bucket), -1 full of others: on to the next bucket
  int bucket(uint64_t b, uint32_t node, uint64_t key, uint4 s[2], bool& fat, uint4 hh[2]) {
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
    if (q[0].z == NONE || q[SLOT_U4].z == NONE) return 0;
    const uint32_t off = rules.cb ? 0u : 1u;
    if (slot_closed(q[0].w, q[1].w, off) || slot_closed(q[SLOT_U4].w, q[SLOT_U4 + 1].w, off)) {
      ++stops;
      return 0;
    }
    return -1;
  }
  std::vector<uint32_t> run(const std::string& topic, uint64_t test_mask) {
    if (!begin(topic, test_mask)) return out;
    walked = true;
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
        if (j == 0 && rules.ks && kind == IT_KEYED && it.second < REC_TOKS) shk = it.second;
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

// k_exact's lookup over the committed exact table
uint32_t cpu_exact(const DevIndex& ix, const std::string& t, bool wild) {
  if (wild ? ix.wild_empty : ix.plain_empty) return NONE;
  const uint32_t len = (uint32_t)t.size();
  const uint64_t fh = key_hash((const uint8_t*)t.data(), len, ix.full_mask);
  const uint64_t base = wild ? ix.xwbase : 0, mask = wild ? ix.xwmask : ix.xmask;
  uint64_t b = base + exact_slot(fh, mask);
  for (;;) {
    for (uint32_t j = 0; j < XBUCKET; ++j) {
      const uint4* e = ix.exact + XENT_U4 * (XBUCKET * b + j);
      if (e[0].y == NONE) return NONE;
      if (e[0].y == TOMB || e[0].x != (uint32_t)(fh >> 32) || e[0].z != len) continue;
      uint32_t w[5] = {0, 0, 0, 0, 0};
      memcpy(w, t.data(), std::min<uint32_t>(len, XINL));
      const uint32_t inl[5] = {e[0].w, e[1].x, e[1].y, e[1].z, e[1].w};
      if (memcmp(w, inl, sizeof w) != 0) continue;
      const uint8_t* fp = ix.fbytes + ix.foff[e[0].y];
      if (len > XINL && memcmp(fp + XINL, t.data() + XINL, len - XINL) != 0) continue;
      return e[0].y;
    }
    if (!((ix.xovf[b >> 5] >> (b & 31)) & 1u)) return NONE;
    b = base + ((b - base + 1) & mask);
  }
}

struct Oracle {
  void* r = ref_create(1);
  std::vector<std::string> names;  // oracle id -> bytes
  std::set<std::string> known;
  ~Oracle() { ref_destroy(r); }
  void add(const std::string& s, uint8_t kind) {
    if (known.insert(s).second) names.push_back(s);
    const uint64_t off[2] = {0, s.size()};
    ref_add_many(r, (const uint8_t*)s.data(), off, 1, &kind);
  }
};

bool is_wild_s(const std::string& s) { return is_wild((const uint8_t*)s.data(), (uint32_t)s.size()); }

}  // namespace
