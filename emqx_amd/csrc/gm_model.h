// gm_model.h -- the host model of the device index, for gm_engine.cpp: the tokeniser, the host
// trie and the one statement of each placement rule k_walk and k_exact take on faith (first free
// or TOMB slot on the chain, the mark on a full bucket passed, open buckets, fat and keyed nodes,
// the root's carried halves).  Full builds, delta commits and snapshot loads all go through it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "gm_common.h"
#include "gm_kernels.h"

namespace gm {
namespace {

uint64_t pow2_at_least(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

template <class V>
void sort_unique(V& v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}

// key_hash's mask for emqxgm_cfg::full_hash_bits
inline uint64_t full_mask(uint32_t bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }

inline bool bit(const std::vector<uint64_t>& b, uint64_t i) { return (b[i >> 6] >> (i & 63)) & 1; }
inline void bset(std::vector<uint64_t>& b, uint64_t i) { b[i >> 6] |= 1ull << (i & 63); }
inline void bclr(std::vector<uint64_t>& b, uint64_t i) { b[i >> 6] &= ~(1ull << (i & 63)); }

// The placement rule of both tables: the first free or TOMB position among the n of bucket b,
// taken in the bitmaps (used: the positions ever taken); ~0: the bucket is full of live entries.
inline uint64_t take_in_bucket(std::vector<uint64_t>& occ, std::vector<uint64_t>& tomb, uint64_t b,
                               uint32_t n, uint64_t& used) {
  for (uint64_t q = b * n; q < (b + 1) * n; ++q) {
    if (!bit(occ, q)) {
      bset(occ, q);
      used += 1;
      return q;
    }
    if (bit(tomb, q)) {
      bclr(tomb, q);
      return q;
    }
  }
  return ~0ull;
}

// Open-addressing map (parent node, level token) -> child node (host-side trie; kept between
// commits for delta commits, so it also erases: a freed entry becomes a TOMB that lookups pass).
struct EdgeMap {
  struct Ent {
    uint64_t tok;
    uint32_t parent;  // NONE = empty, TOMB = erased
    uint32_t child;
  };
  std::vector<Ent> ents;
  uint64_t mask = 0, used = 0;  // used counts erased entries too
  void init(uint64_t expect) {
    const uint64_t cap = pow2_at_least(std::max<uint64_t>(16, expect * 2));
    ents.assign(cap, Ent{0, NONE, 0});
    mask = cap - 1;
    used = 0;
  }
  void grow() {
    std::vector<Ent> old;
    old.swap(ents);
    ents.assign(old.size() * 2, Ent{0, NONE, 0});
    mask = ents.size() - 1;
    used = 0;
    bool ins;
    for (const Ent& e : old)
      if (e.parent != NONE && e.parent != TOMB) *get_or_insert(e.parent, e.tok, ins) = e.child;
  }
  // returns pointer to the child slot; inserted=true if new
  uint32_t* get_or_insert(uint32_t parent, uint64_t tok, bool& inserted) {
    if ((used + 1) * 2 > mask + 1) grow();
    uint64_t i = edge_slot(parent, tok, mask), free_at = ~0ull;
    for (;;) {
      Ent& e = ents[i];
      if (e.parent == parent && e.tok == tok) {
        inserted = false;
        return &e.child;
      }
      if (e.parent == TOMB && free_at == ~0ull) free_at = i;
      if (e.parent == NONE) {
        if (free_at == ~0ull) {
          free_at = i;
          ++used;
        }
        Ent& f = ents[free_at];
        f.parent = parent;
        f.tok = tok;
        inserted = true;
        return &f.child;
      }
      i = (i + 1) & mask;
    }
  }
  uint32_t* find(uint32_t parent, uint64_t tok) {
    if (ents.empty()) return nullptr;
    for (uint64_t i = edge_slot(parent, tok, mask);; i = (i + 1) & mask) {
      Ent& e = ents[i];
      if (e.parent == parent && e.tok == tok) return &e.child;
      if (e.parent == NONE) return nullptr;
    }
  }
  bool erase(uint32_t parent, uint64_t tok) {
    uint32_t* c = find(parent, tok);
    if (!c) return false;
    Ent* e = (Ent*)((uint8_t*)c - offsetof(Ent, child));
    e->parent = TOMB;
    return true;
  }
};

// Level tokens of a filter/topic string, exactly as the device tokenizer computes them.
// is_plus/is_hash flag words that are exactly '+' / '#'; `hashed` = some literal word got a
// hashed token (its trie pairs need byte verification).
void tokenize(const uint8_t* p, uint32_t len, uint64_t test_mask, std::vector<uint64_t>& toks,
              std::vector<uint8_t>& is_plus, std::vector<uint8_t>& is_hash, bool& hashed) {
  toks.clear();
  is_plus.clear();
  is_hash.clear();
  hashed = false;
  uint32_t s = 0;
  for (uint32_t i = 0; i <= len; ++i) {
    if (i == len || p[i] == '/') {
      const uint32_t wl = i - s;
      uint64_t packed = 0, fnv = FNV_OFF;
      for (uint32_t q = 0; q < wl; ++q) {
        if (q < 8) packed |= (uint64_t)p[s + q] << (8 * q);
        fnv = fnv_step(fnv, p[s + q]);
      }
      const bool pl = (wl == 1 && p[s] == '+');
      const bool hs = (wl == 1 && p[s] == '#');
      const uint64_t tok = word_token(packed, fnv, wl, test_mask);
      toks.push_back(tok);
      is_plus.push_back(pl);
      is_hash.push_back(hs);
      if (!pl && !hs && (tok & TOK_HASHED)) hashed = true;
      s = i + 1;
    }
  }
}

// A filter's way through the trie: the edge tokens of its levels, PLUS_TOK for a '+' level.  A
// trailing '#' is no level: the filter hangs off the node before it (hash_last).  Filled again
// and again (resolve): a commit allocates one.
struct Path {
  std::vector<uint64_t> tok;  // [0, len): the edges; a trailing '#' word stays behind them
  std::vector<uint8_t> is_plus, is_hash;
  size_t len = 0;
  bool hash_last = false, hashed = false;  // hashed: tokenize's (trie pairs need verification)
};
void resolve(const uint8_t* p, uint32_t len, uint64_t test_mask, Path& path) {
  tokenize(p, len, test_mask, path.tok, path.is_plus, path.is_hash, path.hashed);
  path.hash_last = path.is_hash.back();
  path.len = path.hash_last ? path.tok.size() - 1 : path.tok.size();  // '#' last: the parent node
  for (size_t w = 0; w < path.len; ++w)
    if (path.is_plus[w]) path.tok[w] = PLUS_TOK;
}

// Node-level filter list during the build: NONE, a single fid, or LIST_MULTI|index.
struct ListBuild {
  std::vector<std::vector<uint32_t>> lists;
  void add(uint32_t& slot, uint32_t fid) {
    if (slot == NONE) {
      slot = fid;
    } else if (slot & LIST_MULTI) {
      lists[slot & ~LIST_MULTI].push_back(fid);
    } else {
      lists.push_back({slot, fid});
      slot = LIST_MULTI | (uint32_t)(lists.size() - 1);
    }
  }
};

constexpr uint64_t DEAD = ~0ull;  // TrieModel::slot of the root and of removed nodes
constexpr uint64_t ROOTH = ~1ull; // TrieModel::slot of the root's fat half (kernel arguments)

// edge slots a delta commit rewrites: slot -> node (NONE: TOMB)
using EdgePatch = std::unordered_map<uint64_t, uint32_t>;

// Host model of the committed trie and exact table, kept so that a commit with a small delta
// patches the device tables in place (commit_delta) instead of rebuilding them.  A slot's 32 B
// are a function of its node's state (node_slot), so only positions and occupancy are mirrored.
struct TrieModel {
  bool valid = false;  // false: the next commit is a full build
  EdgeMap emap;
  // per node (root = 0): hf/tw/tn are NONE, a filter id, or LIST_MULTI | multi[] position
  std::vector<uint32_t> parent, ref, nlit, pchild, hf, tw, tn;
  std::vector<uint8_t> sig;    // gm_common.h sig_bit classes of the node's literal children
  std::vector<uint8_t> hcode;  // depth code (gm_common.h CF_H0/CF_H1): exact at a full build,
                               // only reset to 0 (unbounded) by delta commits
  std::vector<uint64_t> tok;
  std::vector<uint64_t> slot;       // edge slot of the node's incoming edge (DEAD: root/removed,
                                    // ROOTH: the root's fat half, carried in the arguments)
  // fat buckets (gm_common.h FAT_ID): fchild = the node's only literal child when that child's
  // slot is the second half of the node's bucket (the root's: the arguments), else 0; half = the
  // node is such a child
  std::vector<uint32_t> fchild;
  std::vector<uint8_t> half;
  std::vector<uint8_t> keyed;  // the node's children are placed by token (gm_common.h edge_home)
  // the only literal child of a depth-2 '+' node (G/+ for a first-level node G), kept while that
  // node has exactly one: set when its nlit becomes 1, dropped when it becomes 2 or a literal
  // child goes (after a deletion back to one it stays absent until the next full build; absent
  // is always correct).  Feeds root_plus_half; not part of a snapshot (lone_rebuild).
  std::unordered_map<uint32_t, uint32_t> lone;
  std::vector<uint64_t> occ, tomb;  // bitmaps over edge slots: used (live or TOMB), TOMB
  // closed buckets (gm_common.h EDGE_CLOSED).  open: a bit per bucket, set when some edge whose
  // chain passes the bucket was placed beyond it -- exact after a full build and a snapshot load
  // (closed_rebuild), only ever set by delta commits (a deletion leaves it).  owner: the node of
  // each slot's live edge (NONE: empty or TOMB), so that a delta commit that opens a bucket can
  // re-emit the slots that carried its mark.  Neither is part of a snapshot.
  std::vector<uint64_t> open;
  std::vector<uint32_t> owner;
  uint64_t nbk = 0, ecap = 0, n_occ = 0, n_edges = 0, tn_cap = 0, fv_cap = 0;
  std::vector<uint32_t> fvbits;
  std::vector<uint32_t> multi;  // [count, fid...] lists of nodes shared by several filters
  bool needs_verify = false;
  uint32_t max_depth = 0;
  // The tokens the walk can compare a topic's word 0 ([0]) and word 2 ([1]) against: those of the
  // literal edges of that level under any parent (keyed edges, fat halves and the root's carried
  // slots are nodes like the rest; a `tn` key of level 0 hangs off such an edge).  A state
  // (gm_common.h LEV_NONE / LEV_ONE / LEV_MANY) and, for LEV_ONE, the token: exact after a full
  // build and a snapshot load (lev_rebuild), only ever raised by delta commits (a deletion
  // leaves it, as with `sig` and `hcode`).  Token 0, the empty word, counts as many: the walk
  // reads a word that differs from the one token as 0.  Not part of a snapshot.
  uint32_t lev_st[2] = {LEV_NONE, LEV_NONE};
  uint64_t lev_tok[2] = {0, 0};
  uint64_t n_trie = 0, n_route = 0;
  uint64_t n_nodes0 = 0, fv_words0 = 0;  // nodes / verify words at the build (headroom used since)
  // exact route keys: entry per committed key, bitmaps over entries.  Two regions of one
  // table: plain (non-wildcard) keys in buckets [0, xcap_p), wildcard keys in [xcap_p,
  // xcap_p + xcap_w); a name can only equal a key of its own kind (same bytes, same words).
  std::vector<uint32_t> xpos;
  std::vector<uint64_t> xocc, xtomb, xovf;  // xovf: a bit per bucket (gm_common.h)
  uint64_t xcap_p = 0, xcap_w = 0, x_occ_p = 0, x_occ_w = 0, n_route_p = 0, n_route_w = 0;
  uint64_t xbase(bool w) const { return w ? xcap_p : 0; }
  uint64_t xcapr(bool w) const { return w ? xcap_w : xcap_p; }
  uint64_t& xoccr(bool w) { return w ? x_occ_w : x_occ_p; }
  uint64_t& nroute(bool w) { return w ? n_route_w : n_route_p; }
  // home bucket of a key hash in its region, and the next bucket of its probe sequence
  uint64_t xhome(bool w, uint64_t fh) const { return xbase(w) + exact_slot(fh, xcapr(w) - 1); }
  uint64_t xnext(bool w, uint64_t b) const {
    return xbase(w) + ((b - xbase(w) + 1) & (xcapr(w) - 1));
  }
  // device tables patched in place (owned by emqxgm::o_tab)
  uint32_t *d_edges = nullptr, *d_exact = nullptr, *d_tn = nullptr, *d_fv = nullptr,
           *d_xovf = nullptr;

  uint32_t cf(uint32_t i) const {  // gm_common.h cf: id | flags
    uint32_t f = i;
    if (nlit[i]) f |= CF_LIT;
    if (pchild[i]) f |= CF_PLUS;
    if (tw[i] != NONE) f |= CF_TW;
    if (tn[i] != NONE) f |= CF_TN;
    return cf_with_depth_code(f, hcode[i]);
  }
  // The signature field of c's slot (gm_common.h "Child signature"): c's own literal children's
  // classes, 0 for a keyed node with literal children (the keyed flag) -- and, when c has no
  // literal child (CF_LIT clear, its own signature unused), the classes of the literal children
  // of c's '+' child, lent to the walk (a keyed node that lost its last literal child lends
  // them too: a 0 there would rule out every child of the '+' node).  A '+' node is never keyed.
  uint32_t sig_field(uint32_t c) const {
    if (nlit[c]) return keyed[c] ? 0u : (uint32_t)sig[c];
    return pchild[c] ? (uint32_t)sig[pchild[c]] : 0u;
  }
  void node_slot(uint32_t c, uint4* sl) const {  // the 2 x uint4 of c's incoming edge
    const uint32_t p = pchild[c];
    sl[0] = make_uint4((uint32_t)tok[c], (uint32_t)(tok[c] >> 32),
                       (half[c] ? FAT_ID : parent[c]) | (sig_field(c) << SIG_SHIFT), cf(c));
    sl[1] = make_uint4(hf[c], tw[c], p ? pcf(p) : 0u, p ? phf(p) : closed_mark(c));
  }
  // s1.w of a slot whose node has no '+' child: EDGE_CLOSED while its bucket is closed (the
  // root's half, carried in the arguments, has no bucket)
  uint32_t closed_mark(uint32_t c) const {
    const uint64_t s = slot[c];
    if (s == DEAD || s == ROOTH || (s / EBUCKET >> 6) >= open.size()) return NONE;
    return (open[s / EBUCKET >> 6] >> (s / EBUCKET & 63)) & 1 ? NONE : EDGE_CLOSED;
  }
  // open and owner from the placement: every bucket from an edge's home up to its slot's is
  // open (a fat half sits in its parent's bucket, on no chain of its own).  False: some slot is
  // not on its edge's chain (a corrupt snapshot).
  bool closed_rebuild() {
    open.assign(nbk / 64 + 1, 0ull);
    owner.assign(ecap, NONE);
    for (uint32_t c = 1; c < parent.size(); ++c) {
      if (slot[c] == DEAD || slot[c] == ROOTH) continue;
      if (slot[c] >= ecap || owner[slot[c]] != NONE) return false;
      owner[slot[c]] = c;
      if (half[c]) continue;
      uint64_t b = home(parent[c], tok[c]), steps = 0;
      for (; b != slot[c] / EBUCKET; b = (b + 1) & (nbk - 1)) {
        if (++steps >= nbk) return false;
        open[b >> 6] |= 1ull << (b & 63);
      }
    }
    return true;
  }
  // the carried copy of '+' child p (gm_common.h CF_PTW): its '#' filter, or -- when it has
  // none -- its terminal filters, flagged
  bool ptw(uint32_t p) const { return hf[p] == NONE && tw[p] != NONE; }
  uint32_t pcf(uint32_t p) const { return cf(p) | (ptw(p) ? CF_PTW : 0u); }
  uint32_t phf(uint32_t p) const { return ptw(p) ? tw[p] : hf[p]; }
  uint32_t new_node(uint32_t par, uint64_t t) {
    const uint32_t c = (uint32_t)parent.size();
    parent.push_back(par);
    tok.push_back(t);
    ref.push_back(0);
    nlit.push_back(0);
    pchild.push_back(0);
    hf.push_back(NONE);
    tw.push_back(NONE);
    tn.push_back(NONE);
    hcode.push_back(0);
    sig.push_back(0);
    slot.push_back(DEAD);
    fchild.push_back(0);
    half.push_back(0);
    keyed.push_back(0);
    if (par != NONE) child_added(par, c);
    return c;
  }
  // where a filter hangs at its path's end node: '#' filters, other wildcards, plain names
  uint32_t& end_field(uint32_t node, const Path& path, bool wild) {
    return path.hash_last ? hf[node] : wild ? tw[node] : tn[node];
  }
  // the nodes of path's levels that are in the trie, after the root (fewer than path.len + 1:
  // the levels from there on are not)
  void follow(const Path& path, std::vector<uint32_t>& nodes) {
    nodes.assign(1, 0u);
    for (size_t w = 0; w < path.len; ++w) {
      const uint32_t* v = emap.find(nodes.back(), path.tok[w]);
      if (!v) break;
      nodes.push_back(*v);
    }
  }
  // home bucket of the edge (par, t): a keyed parent's literal children by token, its '+' child
  // (probed by IT_PLUS items, never keyed) like every other edge
  uint64_t home(uint32_t par, uint64_t t) const {
    return edge_home(par, t, nbk - 1, keyed[par] != 0 && t != PLUS_TOK);
  }
  // The slot of a new edge (par, t), the first its bucket chain offers (gm_common.h "edge slots").
  // With `opened` (a delta commit) a full bucket the edge passes is no longer closed (gm_common.h
  // EDGE_CLOSED): its `open` bit is set and the bucket listed, for the slots that carried its mark
  // to be written again.  A full build derives `open` from the whole placement (closed_rebuild).
  uint64_t place_edge(uint32_t par, uint64_t t, std::vector<uint64_t>* opened) {
    for (uint64_t b = home(par, t);; b = (b + 1) & (nbk - 1)) {
      const uint64_t q = take_in_bucket(occ, tomb, b, EBUCKET, n_occ);
      if (q != ~0ull) return q;
      if (opened && !bit(open, b)) {
        bset(open, b);
        opened->push_back(b);
      }
    }
  }
  // Node n's edge leaves its slot (the node goes, or a fat half moves out), which becomes TOMB;
  // the root's half (ROOTH) has none.  The caller gives slot[n] its new value.
  void free_edge(uint32_t n, EdgePatch& epatch) {
    if (slot[n] == ROOTH) return;
    bset(tomb, slot[n]);
    epatch[slot[n]] = NONE;
    owner[slot[n]] = NONE;
  }
  // The entry of a new route key of hash fh in its region (w: wildcard keys), the first its
  // bucket chain offers.  A full bucket the key goes on past gets its xovf bit (gm_common.h); a
  // delta commit collects the 32-bit words of the bits newly set (ovf_words) to patch them.
  uint64_t place_key(bool w, uint64_t fh, std::vector<uint32_t>* ovf_words) {
    for (uint64_t b = xhome(w, fh);; b = xnext(w, b)) {
      const uint64_t q = take_in_bucket(xocc, xtomb, b, XBUCKET, xoccr(w));
      if (q != ~0ull) return q;
      if (!bit(xovf, b)) {
        bset(xovf, b);
        if (ovf_words) ovf_words->push_back((uint32_t)(b >> 5));
      }
    }
  }
  // node c's slot as the walk's arguments carry one (c = 0: none, s0.z = NONE)
  void carried(uint32_t c, uint4& s0, uint4& s1) const {
    uint4 sl[2] = {make_uint4(0u, 0u, NONE, 0u), make_uint4(0u, 0u, 0u, 0u)};
    if (c) node_slot(c, sl);
    s0 = sl[0];
    s1 = sl[1];
  }
  // the root's fat half (rh0.z = NONE: none)
  void root_half(DevIndex& x) const { carried(fchild[0], x.rh0, x.rh1); }
  // the walk's copy of the slot of the only literal child H of the root's half's '+' child
  // (gm_kernels.h rp0/rp1), derived wherever root_half is, so it follows every change of H's slot
  // in the same commit; rp0.z = NONE: none.  (H is at depth 3 under a '+' node: never fat, never
  // a half; checked all the same.)
  void root_plus_half(DevIndex& x) const {
    const uint32_t g = fchild[0], p = g ? pchild[g] : 0u;
    uint32_t hn = 0;
    if (p && nlit[p] == 1) {
      const auto it = lone.find(p);
      if (it != lone.end() && slot[it->second] != DEAD && parent[it->second] == p &&
          !half[it->second] && !fchild[it->second])
        hn = it->second;
    }
    carried(hn, x.rp0, x.rp1);
  }
  // What the index holds of the model outside the tables: the root's fields and carried halves,
  // the flags and bounds the passes size and skip their work by.  Every commit ends with it.
  void root_fields(DevIndex& x) const {
    const uint32_t root_p = pchild[0];
    x.root_cf = cf(0);
    x.root_sig = sig_field(0);
    x.root_hf = hf[0];
    x.root_pcf = root_p ? pcf(root_p) : 0u;
    x.root_phf = root_p ? phf(root_p) : NONE;
    root_half(x);
    root_plus_half(x);
    x.needs_verify = needs_verify;
    x.max_depth = max_depth;
    for (uint32_t i = 0; i < 2; ++i) {
      x.lev_st[i] = lev_st[i];
      x.lev_tok[i] = lev_st[i] == LEV_ONE ? lev_tok[i] : 0ull;
    }
    x.fid_bound = (uint64_t)fv_cap * 32;
    x.trie_empty = (n_trie == 0);
    x.plain_empty = (n_route_p == 0);
    x.wild_empty = (n_route_w == 0);
  }
  bool lone_parent(uint32_t par) const {  // a depth-2 '+' node
    return par != 0 && tok[par] == PLUS_TOK && parent[par] != 0 && parent[parent[par]] == 0;
  }
  // the level (0 or 2, as an index of lev_st) whose words node par's literal children are
  // compared against, or 2: another level
  uint32_t lev_index(uint32_t par) const {
    if (par == 0) return 0;
    return parent[par] != 0 && parent[parent[par]] == 0 ? 1u : 2u;
  }
  void lev_note(uint32_t par, uint64_t t) {  // a literal edge (par, t): none -> one -> many
    const uint32_t i = lev_index(par);
    if (i >= 2 || lev_st[i] == LEV_MANY) return;
    if (t == 0 || (lev_st[i] == LEV_ONE && lev_tok[i] != t)) {
      lev_st[i] = LEV_MANY;
    } else {
      lev_st[i] = LEV_ONE;
      lev_tok[i] = t;
    }
  }
  void lev_rebuild() {  // from the node arrays (a snapshot load)
    lev_st[0] = lev_st[1] = LEV_NONE;
    lev_tok[0] = lev_tok[1] = 0;
    for (uint32_t c = 1; c < parent.size(); ++c)
      if (slot[c] != DEAD && tok[c] != PLUS_TOK) lev_note(parent[c], tok[c]);
  }
  void child_added(uint32_t par, uint32_t c) {  // new_node: c hangs under par
    if (tok[c] == PLUS_TOK) {
      pchild[par] = c;
      return;
    }
    lev_note(par, tok[c]);
    nlit[par] += 1;
    sig[par] |= (uint8_t)sig_bit(tok[c]);
    if (!lone_parent(par)) return;
    if (nlit[par] == 1)
      lone[par] = c;
    else
      lone.erase(par);
  }
  void lit_removed(uint32_t par) {  // a literal child of par went
    if (lone_parent(par)) lone.erase(par);
  }
  void lone_rebuild() {  // from the node arrays (a snapshot load)
    lone.clear();
    for (uint32_t c = 1; c < parent.size(); ++c)
      if (slot[c] != DEAD && tok[c] != PLUS_TOK && lone_parent(parent[c]) && nlit[parent[c]] == 1)
        lone[parent[c]] = c;
  }
  // a filter was added along path[0] = root .. path[m] (its end node; hash_last: a '#' filter
  // hanging off path[m]): a code its ancestors can no longer guarantee is reset to unbounded
  void widen_codes(const std::vector<uint32_t>& path, bool hash_last,
                   std::vector<uint32_t>& dirty) {
    const size_t m = path.size() - 1;
    for (size_t i = 0; i < m; ++i) {
      const uint32_t x = path[i];
      if (hcode[x] && (hash_last || m - i > hcode[x])) {
        hcode[x] = 0;
        dirty.push_back(x);
      }
    }
  }
};

// Token-keyed parents (gm_common.h edge_home) of a full build.  mode 1: parents with at least
// KEYED_MIN_FANOUT literal children, none of whose child tokens is the child of more than
// KEYED_MAX_SHARE candidates and at most 1/16 of them of more than EBUCKET (their edges then
// share one bucket per token; the few crowded tokens only lengthen their own chains -- on cfg3 the
// device ids 0..9999 are also site numbers, children of `site`); mode 2 (tests): every eligible
// parent; 0: none.  Never the root or a node reached by a '+' edge.
constexpr uint32_t KEYED_MIN_FANOUT = 16;
constexpr uint32_t KEYED_MAX_SHARE = 8;
void select_keyed(TrieModel& m, uint32_t mode) {
  const size_t nn = m.parent.size();
  m.keyed.assign(nn, 0u);
  if (mode == 0) return;
  auto eligible = [&](uint32_t x) {
    return x != 0 && m.tok[x] != PLUS_TOK && m.nlit[x] > 0 &&
           (mode == 2 || m.nlit[x] >= KEYED_MIN_FANOUT);
  };
  if (mode == 2) {
    for (uint32_t x = 1; x < nn; ++x) m.keyed[x] = eligible(x) ? 1 : 0;
    return;
  }
  // child tokens of the candidates, counted by sorting
  std::vector<uint64_t> toks;
  for (uint32_t c = 1; c < nn; ++c)
    if (m.tok[c] != PLUS_TOK && eligible(m.parent[c])) toks.push_back(m.tok[c]);
  if (toks.empty()) return;
  std::sort(toks.begin(), toks.end());
  std::vector<std::pair<uint64_t, uint32_t>> crowded;  // tokens under more than EBUCKET candidates
  for (size_t i = 0; i < toks.size();) {
    size_t j = i;
    while (j < toks.size() && toks[j] == toks[i]) ++j;
    if (j - i > EBUCKET) crowded.emplace_back(toks[i], (uint32_t)std::min<size_t>(j - i, ~0u));
    i = j;
  }
  std::vector<uint32_t> n_crowded(nn, 0);
  std::vector<uint8_t> ok(nn, 0);
  for (uint32_t x = 1; x < nn; ++x) ok[x] = eligible(x) ? 1 : 0;
  for (uint32_t c = 1; c < nn; ++c) {
    const uint32_t p = m.parent[c];
    if (!ok[p] || m.tok[c] == PLUS_TOK) continue;
    auto it = std::lower_bound(crowded.begin(), crowded.end(), std::make_pair(m.tok[c], 0u));
    if (it == crowded.end() || it->first != m.tok[c]) continue;
    if (it->second > KEYED_MAX_SHARE) ok[p] = 0;
    else n_crowded[p] += 1;
  }
  for (uint32_t x = 1; x < nn; ++x) m.keyed[x] = ok[x] && n_crowded[x] * 16 <= m.nlit[x];
}

}  // namespace
}  // namespace gm
