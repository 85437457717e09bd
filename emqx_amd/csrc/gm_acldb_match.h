// gm_acldb_match.h -- the built-in authorization database keyed by client (DESIGN.md 6b "Built-in
// database"): emqx_authz_mnesia's one record per principal (apps/emqx_authz/src/
// emqx_authz_mnesia.erl:41-58), found by key and walked rule by rule (:98-120, :222-229).  Plain
// functions with no HIP call, written so that a device kernel and a host program run the same
// code: k_acldb (gm_acldb.inc) and the host side of the emqxgm_acldb_* C-ABI (gm_acldb.cpp) on the
// device path, tests/host_harness/acldb_main.cpp and acldb_dev_main.cpp on the CPU.  Built on
// gm_acl_match.h: its rule header, filter records, client words and predicates are used as they
// are.
//
// Key tables: one open-addressing table (linear probing, a power of two of 16-byte slots) per key
// kind.  A slot is {token of the key's bytes (acl_value_token), first word of the key's run in
// the record pool, index of the key in the key-offset array}.  ADB_EMPTY and ADB_DELETED are
// values no token takes (bit 63 clear and a length field of 64: an inline token's length is at
// most 7).  A probe starts at adb_home(token) and stops at an empty slot; a hit on a hashed token
// (keys longer than TOK_INLINE_MAX bytes, every key in the collision-test mode) is confirmed on
// the key's bytes and the probe goes on when they differ.
//
// Record pool: 64-bit words.  A key's run is contiguous:
//   word 0   run header: words of the run, this one included (32 bits) | base of the run's
//            filters in the filter-offset array (32)
//   then per rule, in list order: the ACL rule header of gm_acl_match.h (2 words, who = all) and
//            one filter record.  The rule field of both and the filter field of the record are
//            relative to the run: rule k of the record has k in all three, and its filter's bytes
//            are filter base + k of the filter-offset array.
// A lane reads its own run from global memory word after word, so a run needs no tile rule.  The
// `all` record is not in the pool: it is a tiled stream as in gm_acl_match.h (rs_append), staged
// through LDS by the whole block, with the same relative fields.
#pragma once
#include <stdint.h>

#include "gm_acl_match.h"

namespace gm {

constexpr uint32_t ADB_CLIENTID = 0, ADB_USERNAME = 1, ADB_ALL = 2;  // EMQXGM_ACLDB_*; the source
constexpr uint64_t ADB_EMPTY = 1ull << 62;
constexpr uint64_t ADB_DELETED = (1ull << 62) | 1ull;
constexpr uint32_t ADB_MIN_SLOTS = 8;
constexpr uint32_t ADB_MAX_RULES = 65536;  // per record: the 16-bit rule field
constexpr uint32_t ADB_RULE_WORDS_MAX = ACL_RULE_WORDS + ACL_FILTER_HDR + RS_MAX_LEVELS;

struct alignas(16) AdbSlot {
  uint64_t tok;
  uint32_t run;  // first word of the key's run in the record pool
  uint32_t key;  // key bytes: kb[ko[key] .. ko[key + 1])
};

GM_HD uint64_t adb_home(uint64_t tok, uint64_t mask) { return fmix64(tok + 0x2545f4914f6cdd1dull) & mask; }
GM_HD uint64_t adb_run_header(uint32_t words, uint32_t fbase) { return (uint64_t)words | ((uint64_t)fbase << 32); }
GM_HD uint32_t adb_run_words(uint64_t h) { return (uint32_t)h; }
GM_HD uint32_t adb_run_fbase(uint64_t h) { return (uint32_t)(h >> 32); }

// Compiles rule k of a record (perm, action, topic filter f: "eq F" is {eq, F}, compile_topic/1
// emqx_authz_rule.erl:98-99) into out[0 .. return): at most ADB_RULE_WORDS_MAX words.  *skip =
// bytes of the prefix that the filter's stored bytes leave out.
GM_HD uint32_t adb_compile_rule(uint32_t perm, uint32_t action, const uint8_t* f, uint32_t len, uint32_t k,
                                uint64_t test_mask, uint64_t* out, uint32_t* skip) {
  const bool eq = len >= 3 && f[0] == 'e' && f[1] == 'q' && f[2] == ' ';
  *skip = eq ? 3u : 0u;
  out[0] = acl_rule_header(perm, action, ACL_WHO_ALL, 0, k);
  out[1] = 0;
  return ACL_RULE_WORDS + acl_compile_filter(f + *skip, len - *skip, eq, k, k, test_mask, out + ACL_RULE_WORDS);
}

// The next slot from *i on whose token is `tok`, or NONE at the empty slot that ends the chain (or
// after `mask + 1` slots); *i is left past the slot returned, *steps counts the slots looked at.
// A probe of a key starts with *i = adb_home(tok, mask) and *steps = 0; a hit on a hashed token is
// confirmed on the key's bytes by the caller, who calls again when they differ.
template <class PS>
GM_HD uint32_t adb_probe_next(PS tab, uint64_t mask, uint64_t tok, uint64_t* i, uint64_t* steps) {
  while (*steps <= mask) {
    const uint64_t at = *i;
    const uint64_t t = tab[at].tok;
    ++*steps;
    *i = (at + 1) & mask;
    if (t == ADB_EMPTY) return NONE;
    if (t == tok) return (uint32_t)at;  // (ADB_DELETED is no token)
  }
  return NONE;
}

// Walks the run that starts at pool[start]: visit(k, rule header, filter record, absolute filter
// index) for rule k = 0, 1, .. until visit returns true.  False for a malformed run, found before
// any index of it is followed: a run or a record past the pool's or the run's end, a record that
// is not (rule header of `all`, filter record), a rule or filter field other than the rule's
// position, a filter index outside the filter-offset array.
template <class PW, class VISIT>
GM_HD bool adb_walk_run(PW pool, uint64_t pool_words, uint32_t start, uint32_t n_filters, VISIT visit) {
  if (start >= pool_words) return false;
  const uint64_t h = pool[start];
  const uint32_t len = adb_run_words(h), fbase = adb_run_fbase(h);
  if (len < 1 || (uint64_t)start + len > pool_words) return false;
  uint32_t k = 0;
  for (uint32_t p = 1; p < len; ++k) {
    if (len - p < ACL_RULE_WORDS + ACL_FILTER_HDR) return false;
    const uint64_t r0 = pool[start + p], w0 = pool[start + p + ACL_RULE_WORDS];
    if (!acl_is_rule(r0) || acl_who(r0) != ACL_WHO_ALL || acl_rule(r0) != k) return false;
    if (rs_levels(w0) > RS_MAX_LEVELS) return false;  // a rule header, RS_END or no record at all
    const uint32_t step = ACL_RULE_WORDS + ACL_FILTER_HDR + rs_levels(w0);
    if (len - p < step) return false;
    if (rs_rule(w0) != k || rs_filter(w0) != k || (uint64_t)fbase + k >= n_filters) return false;
    if (visit(k, r0, &pool[start + p + ACL_RULE_WORDS], fbase + k)) return true;
    p += step;
  }
  return true;
}

}  // namespace gm
