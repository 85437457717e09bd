// gm_ruleset_match.h -- compiled topic-rule filters and the per-(name, filter) predicate on
// level tokens, for rule lists that return every matching rule per name (the
// rule engine's get_rules_for_topic/1, egress bridges, exhook and trace filters).  Plain
// functions with no HIP call, written so that a device kernel and a host program run the same
// code: k_ruleset (gm_ruleset.inc) and the host side of the emqxgm_ruleset_* C-ABI
// (gm_ruleset.cpp) on the device path, tests/host_harness/ruleset_main.cpp and
// ruleset_dev_main.cpp (the kernel's phases, lane by lane) on the CPU.
//
// A filter of a rule is compiled once into a record of 64-bit words:
//   word 0   header: levels (5 bits) | RS_* flags (6) | rule index (16) | filter index (20) |
//            '+' mask (16: bit l set = level l is a '+')
//   word 1.. one level token per level (word_token of the level's word; PLUS_TOK for a '+')
// The kind of a level is its '+' mask bit (literal or '+'); a final '#' is the header's RS_HASH
// flag and takes no level word, so `levels` counts the words before it.  A filter with more
// than RS_MAX_LEVELS such words is RS_DEEP and carries no level word: no name of at most
// RS_MAX_LEVELS levels can match it, and deeper names are matched on their bytes.
// Records are laid out in tiles of RS_TILE_WORDS words (sized as one LDS tile); a record
// never straddles a tile, and a tile that is not full ends in RS_END.
#pragma once
#include <stdint.h>

#include "gm_common.h"

namespace gm {

constexpr uint32_t RS_MAX_LEVELS = 16;   // name levels tokenised; filter levels in a record
constexpr uint32_t RS_TILE_WORDS = 1024; // 8 KB of records per LDS tile
constexpr uint64_t RS_END = ~0ull;       // levels field 31: never a record header

constexpr uint32_t RS_DOLLAR = 1u;    // match/2 on binaries: the '$' clauses apply
constexpr uint32_t RS_ROOTWILD = 2u;  // the filter's first byte is '+' or '#'
constexpr uint32_t RS_HASH = 4u;      // the filter's last word is '#'
constexpr uint32_t RS_HASHED = 8u;    // some level token is a hash: a token hit needs the bytes
constexpr uint32_t RS_EQ = 16u;       // {eq, Filter}: word-list equality, wildcards literal
constexpr uint32_t RS_DEEP = 32u;     // more than RS_MAX_LEVELS levels

constexpr uint32_t RS_F_EQ = 1u;      // emqx_gpumatch.h EMQXGM_RULE_EQ
constexpr uint32_t RS_F_WORDS = 2u;   // EMQXGM_RULE_WORDS

GM_HD uint32_t rs_levels(uint64_t hdr) { return (uint32_t)hdr & 31u; }
GM_HD uint32_t rs_flags(uint64_t hdr) { return (uint32_t)(hdr >> 5) & 63u; }
GM_HD uint32_t rs_rule(uint64_t hdr) { return (uint32_t)(hdr >> 11) & 0xFFFFu; }
GM_HD uint32_t rs_filter(uint64_t hdr) { return (uint32_t)(hdr >> 27) & 0xFFFFFu; }
GM_HD uint32_t rs_plus(uint64_t hdr) { return (uint32_t)(hdr >> 47) & 0xFFFFu; }
GM_HD uint64_t rs_header(uint32_t levels, uint32_t flags, uint32_t rule, uint32_t filter,
                         uint32_t plus) {
  return (uint64_t)levels | ((uint64_t)flags << 5) | ((uint64_t)rule << 11) |
         ((uint64_t)filter << 27) | ((uint64_t)plus << 47);
}
// Tiles of a record stream of total_words words, and the words of tile k that the stream holds
// (a short last tile: the rest of the LDS tile is set to RS_END).
GM_HD uint32_t rs_n_tiles(uint32_t total_words) { return (total_words + RS_TILE_WORDS - 1) / RS_TILE_WORDS; }
GM_HD uint32_t rs_tile_span(uint32_t k, uint32_t total_words) {
  const uint64_t b = (uint64_t)k * RS_TILE_WORDS;
  if (b >= total_words) return 0;
  return total_words - b < RS_TILE_WORDS ? (uint32_t)(total_words - b) : RS_TILE_WORDS;
}
GM_HD uint64_t rs_test_mask(uint32_t hash_bits) { return hash_bits ? (1ull << hash_bits) - 1 : 0; }

// emqx_topic:words/1 over bytes b[0 .. len): put(level, token, start, length) for each of the
// first `max` words.  Returns the number of words, or max + 1 as soon as there are more.
template <class PB, class PUT>
GM_HD uint32_t rs_tokenize(PB b, uint32_t len, uint64_t test_mask, uint32_t max, PUT put) {
  uint64_t packed = 0, fnv = FNV_OFF;
  uint32_t wl = 0, lv = 0;
  for (uint32_t i = 0;; ++i) {
    if (i < len) {
      const uint32_t c = b[i];
      if (c != '/') {
        if (wl < TOK_INLINE_MAX) packed |= (uint64_t)c << (8 * wl);
        fnv = fnv_step(fnv, c);
        ++wl;
        continue;
      }
    }
    if (lv == max) return max + 1;
    put(lv, word_token(packed, fnv, wl, test_mask), i - wl, wl);
    ++lv;
    if (i >= len) return lv;
    packed = 0, fnv = FNV_OFF, wl = 0;
  }
}

// Compiles one filter (flag: 0, RS_F_WORDS or RS_F_EQ) of rule `rule` into out[0 .. return):
// at most 1 + RS_MAX_LEVELS words.
GM_HD uint32_t rs_compile(const uint8_t* f, uint32_t len, uint32_t flag, uint32_t rule,
                          uint32_t filter, uint64_t test_mask, uint64_t* out) {
  const bool eq = (flag & RS_F_EQ) != 0;
  uint32_t flags = eq ? RS_EQ : 0u, plus = 0;
  if (!eq && !(flag & RS_F_WORDS)) flags |= RS_DOLLAR;
  if (len > 0 && (f[0] == '+' || f[0] == '#')) flags |= RS_ROOTWILD;
  uint64_t tok[RS_MAX_LEVELS + 1];
  bool last_hash = false;
  uint32_t nw = rs_tokenize(f, len, test_mask, RS_MAX_LEVELS + 1,
                            [&](uint32_t lv, uint64_t t, uint32_t s, uint32_t wl) {
                              const bool one = !eq && wl == 1;
                              last_hash = one && f[s] == '#';
                              if (one && f[s] == '+') {
                                t = PLUS_TOK;
                                plus |= 1u << lv;
                              }
                              tok[lv] = t;
                            });
  // a '#' is the multi-level wildcard only as the last word (a '#' elsewhere is a literal word)
  if (nw <= RS_MAX_LEVELS + 1 && last_hash) {
    flags |= RS_HASH;
    --nw;
  }
  if (nw > RS_MAX_LEVELS) {
    out[0] = rs_header(0, flags | RS_DEEP, rule, filter, 0);
    return 1;
  }
  plus &= (1u << nw) - 1;
  for (uint32_t l = 0; l < nw; ++l) {
    out[1 + l] = tok[l];
    if (!((plus >> l) & 1u) && (tok[l] & TOK_HASHED)) flags |= RS_HASHED;
  }
  out[0] = rs_header(nw, flags, rule, filter, plus);
  return 1 + nw;
}

// Appends a compiled record to the tiled record stream (host only; V: a vector of uint64_t).
// A reader walks a tile from its first word: header, skip 1 + rs_levels(header) words, until
// the tile's end or RS_END.
template <class V>
inline void rs_append(V& recs, const uint64_t* rec, uint32_t n_words) {
  const uint32_t used = (uint32_t)(recs.size() % RS_TILE_WORDS);
  if (used && used + n_words > RS_TILE_WORDS) recs.resize(recs.size() + (RS_TILE_WORDS - used), RS_END);
  recs.insert(recs.end(), rec, rec + n_words);
}

// emqx_topic:match/2 of a tokenised name (n_levels <= RS_MAX_LEVELS words, token of level l =
// name_tok(l); dollar: its first byte is '$'; hash_words: bit l set = its word l is exactly "#")
// against the record {hdr, lv[]}: one token compare per literal level.  match/2 tries
// match([H | T1], [H | T2]) before match(_, ['#']) (emqx_topic.erl:78-83), so a name whose word
// at a filter's final '#' is itself "#" matches only if it ends there: a/#/c does not match a/#.
// True for a filter with RS_HASHED is a candidate only (two long words may share a token): the
// caller confirms it on the bytes.
template <class NT>
GM_HD bool rs_match_tokens(uint64_t hdr, const uint64_t* lv, uint32_t n_levels, bool dollar,
                           uint32_t hash_words, NT name_tok) {
  const uint32_t fl = rs_levels(hdr), fg = rs_flags(hdr), plus = rs_plus(hdr);
  if (fg & RS_DEEP) return false;
  if (dollar && (fg & (RS_DOLLAR | RS_ROOTWILD)) == (RS_DOLLAR | RS_ROOTWILD)) return false;
  if (fg & RS_HASH) {
    if (n_levels < fl || (n_levels > fl + 1 && ((hash_words >> fl) & 1u))) return false;
  } else if (n_levels != fl) {
    return false;
  }
  for (uint32_t l = 0; l < fl; ++l)
    if (!((plus >> l) & 1u) && lv[l] != name_tok(l)) return false;
  return true;
}

}  // namespace gm
