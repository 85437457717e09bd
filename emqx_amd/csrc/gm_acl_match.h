// gm_acl_match.h -- compiled ACL rule lists with client placeholders and the per-(name, client,
// record) predicate on level tokens (DESIGN.md 6b "ACL lists"): emqx_authz_rule:matches/4
// (apps/emqx_authz/src/emqx_authz_rule.erl:125-215) with feed_var/2 (:217-230).  Plain functions
// with no HIP call, written so that a device kernel and a host program run the same code: k_acl
// (gm_acl.inc) and the host side of the emqxgm_acl_* C-ABI (gm_acl.cpp) on the device path,
// tests/host_harness/acl_main.cpp and acl_dev_main.cpp (the kernel's phases, lane by lane) on
// the CPU.  Built on gm_ruleset_match.h: its tokeniser, word_token, the clause logic of
// rs_match_tokens and the tile rules are used as they are; the ACL stream has words of its own.
//
// The stream is a sequence of records of 64-bit words, rule by rule, in list order:
//   rule header (ACL_RULE_WORDS = 2 words), then the rule's filter records.
//   rule header word 0: 30 in the levels field (never a filter record: those have at most
//            RS_MAX_LEVELS, and RS_END has 31) | permission (1 bit) | action (2) | who kind (2) |
//            host slot (6) | rule index (16, which is also the index of the rule's who string)
//   rule header word 1: the who string's token (acl_value_token; kinds USERNAME and CLIENTID)
//   filter record word 0: the header of gm_ruleset_match.h (rs_header; RS_EQ or word-list
//            semantics, never RS_DOLLAR: emqx_authz_rule calls match/2 on word lists, :212-215)
//   filter record word 1: ${clientid} level mask (16 bits) | ${username} level mask (16) << 16 |
//            ACL_W1_LITHASHED: a level that is neither '+' nor a placeholder has a hashed token
//   filter record word 2..: one level token per level, as in gm_ruleset_match.h
// No record straddles a tile of RS_TILE_WORDS words and a tile that is not full ends in RS_END
// (rs_append).  A reader walks a tile from word 0 with acl_step.
//
// feed_var/2 puts the client's id or username in as one binary word, and emqx_topic:words/1
// makes atoms of a name's words "", "+" and "#" and never yields a word with a '/'.  So a fed
// value that is empty, "+", "#" or holds a '/' equals no name word (ACL_C_*_NOWORD), it is never
// a wildcard, and which levels of a filter are wildcards does not depend on the client.  With the
// value undefined the placeholder stays the literal word (:221-222, :225-226).
#pragma once
#include <stdint.h>

#include "gm_match.h"
#include "gm_ruleset_match.h"

namespace gm {

constexpr uint32_t ACL_RULE_MARK = 30;  // levels field of a rule header
constexpr uint32_t ACL_RULE_WORDS = 2;
constexpr uint32_t ACL_FILTER_HDR = 2;  // words of a filter record before its level tokens

constexpr uint32_t ACL_DENY = 0, ACL_ALLOW = 1;                  // emqx_gpumatch.h EMQXGM_ACL_*
constexpr uint32_t ACL_PUBLISH = 1, ACL_SUBSCRIBE = 2, ACL_ALL = 3;  // a request has one bit
constexpr uint32_t ACL_WHO_ALL = 0, ACL_WHO_USERNAME = 1, ACL_WHO_CLIENTID = 2, ACL_WHO_HOST = 3;
constexpr uint32_t ACL_HOST_SLOTS = 64;

constexpr uint32_t ACL_C_CID_UNDEF = 1u;   // EMQXGM_ACL_NO_CLIENTID: clientid => undefined
constexpr uint32_t ACL_C_USR_UNDEF = 2u;   // EMQXGM_ACL_NO_USERNAME
constexpr uint32_t ACL_C_CID_NOWORD = 4u;  // derived: the client id equals no name word
constexpr uint32_t ACL_C_USR_NOWORD = 8u;

constexpr uint64_t ACL_W1_LITHASHED = 1ull << 32;

constexpr uint32_t ACL_PH_LEN = 11;  // emqx_placeholder.hrl:31-33
GM_HD const char* acl_ph_clientid() { return "${clientid}"; }
GM_HD const char* acl_ph_username() { return "${username}"; }

GM_HD uint64_t acl_rule_header(uint32_t perm, uint32_t action, uint32_t who, uint32_t slot, uint32_t rule) {
  return (uint64_t)ACL_RULE_MARK | ((uint64_t)perm << 5) | ((uint64_t)action << 6) | ((uint64_t)who << 8) |
         ((uint64_t)slot << 10) | ((uint64_t)rule << 16);
}
GM_HD bool acl_is_rule(uint64_t w0) { return rs_levels(w0) == ACL_RULE_MARK; }
GM_HD uint32_t acl_perm(uint64_t w0) { return (uint32_t)(w0 >> 5) & 1u; }
GM_HD uint32_t acl_action(uint64_t w0) { return (uint32_t)(w0 >> 6) & 3u; }
GM_HD uint32_t acl_who(uint64_t w0) { return (uint32_t)(w0 >> 8) & 3u; }
GM_HD uint32_t acl_slot(uint64_t w0) { return (uint32_t)(w0 >> 10) & 63u; }
GM_HD uint32_t acl_rule(uint64_t w0) { return (uint32_t)(w0 >> 16) & 0xFFFFu; }
GM_HD uint32_t acl_cid_mask(uint64_t w1) { return (uint32_t)w1 & 0xFFFFu; }
GM_HD uint32_t acl_usr_mask(uint64_t w1) { return (uint32_t)(w1 >> 16) & 0xFFFFu; }
// Words of the record that starts with w0 (not RS_END).
GM_HD uint32_t acl_step(uint64_t w0) { return acl_is_rule(w0) ? ACL_RULE_WORDS : ACL_FILTER_HDR + rs_levels(w0); }

// Token of a whole value (a client id, a username, a rule's who string): word_token over all its
// bytes, a '/' included.  For a value that can be a name word it is that word's level token.
template <class PB>
GM_HD uint64_t acl_value_token(PB b, uint32_t len, uint64_t test_mask) {
  uint64_t packed = 0, fnv = FNV_OFF;
  for (uint32_t i = 0; i < len; ++i) {
    const uint32_t c = b[i];
    if (i < TOK_INLINE_MAX) packed |= (uint64_t)c << (8 * i);
    fnv = fnv_step(fnv, c);
  }
  return word_token(packed, fnv, len, test_mask);
}

// A fed value that equals no name word: empty, "+", "#", or with a '/' in it.
template <class PB>
GM_HD bool acl_value_noword(PB b, uint32_t len) {
  if (len == 0 || (len == 1 && (b[0] == '+' || b[0] == '#'))) return true;
  for (uint32_t i = 0; i < len; ++i)
    if (b[i] == '/') return true;
  return false;
}

// What a request's lane needs of its client: derived once per lane (or per client).
struct AclClient {
  uint64_t cid_tok = 0, usr_tok = 0;
  uint32_t flags = 0;  // ACL_C_*
};
template <class PB>
GM_HD AclClient acl_client(PB cid, uint32_t cl, PB usr, uint32_t ul, uint32_t undef_flags, uint64_t test_mask) {
  AclClient c;
  c.flags = undef_flags & (ACL_C_CID_UNDEF | ACL_C_USR_UNDEF);
  if (!(c.flags & ACL_C_CID_UNDEF)) {
    c.cid_tok = acl_value_token(cid, cl, test_mask);
    if (acl_value_noword(cid, cl)) c.flags |= ACL_C_CID_NOWORD;
  }
  if (!(c.flags & ACL_C_USR_UNDEF)) {
    c.usr_tok = acl_value_token(usr, ul, test_mask);
    if (acl_value_noword(usr, ul)) c.flags |= ACL_C_USR_NOWORD;
  }
  return c;
}

template <class PB>
GM_HD bool acl_word_is(PB w, uint32_t len, const char* ph) {
  if (len != ACL_PH_LEN) return false;
  for (uint32_t i = 0; i < ACL_PH_LEN; ++i)
    if ((uint8_t)w[i] != (uint8_t)ph[i]) return false;
  return true;
}

// Compiles one filter (eq: {eq, F} or "eq F" with the prefix taken off by the caller) of rule
// `rule` into out[0 .. return): at most ACL_FILTER_HDR + RS_MAX_LEVELS words.  pattern/1
// (:109-110) is decided here: a non-eq filter one of whose words is exactly a placeholder.
GM_HD uint32_t acl_compile_filter(const uint8_t* f, uint32_t len, bool eq, uint32_t rule, uint32_t filter,
                                  uint64_t test_mask, uint64_t* out) {
  uint64_t rec[1 + RS_MAX_LEVELS];
  const uint32_t nw = rs_compile(f, len, eq ? RS_F_EQ : RS_F_WORDS, rule, filter, test_mask, rec);
  const uint32_t fl = rs_levels(rec[0]), plus = rs_plus(rec[0]);
  uint32_t cm = 0, um = 0;
  if (!eq && !(rs_flags(rec[0]) & RS_DEEP))
    rs_tokenize(f, len, test_mask, RS_MAX_LEVELS, [&](uint32_t lv, uint64_t, uint32_t s, uint32_t wl) {
      if (lv >= fl) return;
      if (acl_word_is(f + s, wl, acl_ph_clientid())) cm |= 1u << lv;
      if (acl_word_is(f + s, wl, acl_ph_username())) um |= 1u << lv;
    });
  uint64_t w1 = (uint64_t)cm | ((uint64_t)um << 16);
  for (uint32_t l = 0; l < fl; ++l)
    if (!(((plus | cm | um) >> l) & 1u) && (rec[1 + l] & TOK_HASHED)) w1 |= ACL_W1_LITHASHED;
  out[0] = rec[0];
  out[1] = w1;
  for (uint32_t l = 0; l + 1 < nw; ++l) out[2 + l] = rec[1 + l];
  return nw + 1;
}

// match_action/2 (:147-150): the request's one bit against the rule's bits.
GM_HD bool acl_match_action(uint32_t rule_action, uint32_t req_action) { return (rule_action & req_action) != 0; }

// The token side of match_who/2 (:152-200) for the kinds decided here.  *confirm: the answer
// true rests on a hashed token and the caller compares the bytes.
GM_HD bool acl_match_who_tokens(uint64_t w0, uint64_t who_tok, const AclClient& c, uint64_t who_bits,
                                bool* confirm) {
  *confirm = false;
  switch (acl_who(w0)) {
    case ACL_WHO_ALL:
      return true;
    case ACL_WHO_HOST:
      return ((who_bits >> acl_slot(w0)) & 1ull) != 0;
    case ACL_WHO_USERNAME:
      if ((c.flags & ACL_C_USR_UNDEF) || c.usr_tok != who_tok) return false;
      break;
    default:
      if ((c.flags & ACL_C_CID_UNDEF) || c.cid_tok != who_tok) return false;
      break;
  }
  *confirm = (who_tok & TOK_HASHED) != 0;
  return true;
}

// Whether a token hit of this record for this client has to be confirmed on the bytes.
GM_HD bool acl_needs_confirm(uint64_t w0, uint64_t w1, const AclClient& c) {
  if (rs_flags(w0) & RS_EQ) return (rs_flags(w0) & RS_HASHED) != 0;
  if (w1 & ACL_W1_LITHASHED) return true;
  // an undefined value leaves the placeholder word itself (11 bytes: a hashed token)
  if (acl_cid_mask(w1) && ((c.flags & ACL_C_CID_UNDEF) || (c.cid_tok & TOK_HASHED))) return true;
  if (acl_usr_mask(w1) && ((c.flags & ACL_C_USR_UNDEF) || (c.usr_tok & TOK_HASHED))) return true;
  return false;
}

// match_topic/2 (:212-215) of a tokenised name against the filter record {w0, w1, lv[]} with the
// client's values fed into the placeholder levels: rs_match_tokens with those levels left out,
// then one token compare per placeholder level.  True is a candidate when acl_needs_confirm.
template <class NT>
GM_HD bool acl_match_tokens(uint64_t w0, uint64_t w1, const uint64_t* lv, uint32_t n_levels, uint32_t hash_words,
                            const AclClient& c, NT name_tok) {
  const uint32_t cm = acl_cid_mask(w1), um = acl_usr_mask(w1);
  if (!rs_match_tokens(w0 | ((uint64_t)(cm | um) << 47), lv, n_levels, false, hash_words, name_tok)) return false;
  if (!(cm | um)) return true;
  if (cm && (c.flags & (ACL_C_CID_UNDEF | ACL_C_CID_NOWORD)) == ACL_C_CID_NOWORD) return false;
  if (um && (c.flags & (ACL_C_USR_UNDEF | ACL_C_USR_NOWORD)) == ACL_C_USR_NOWORD) return false;
  const uint32_t fl = rs_levels(w0);
  for (uint32_t l = 0; l < fl; ++l) {
    if ((cm >> l) & 1u) {
      if (((c.flags & ACL_C_CID_UNDEF) ? lv[l] : c.cid_tok) != name_tok(l)) return false;
    } else if ((um >> l) & 1u) {
      if (((c.flags & ACL_C_USR_UNDEF) ? lv[l] : c.usr_tok) != name_tok(l)) return false;
    }
  }
  return true;
}

// match_topic/2 on the bytes, with feed_var/2 done here: emqx_topic:match/2 on word lists (no
// '$' clauses) of name T against filter F whose words ${clientid} / ${username} are replaced by
// the client's value unless that is undefined.  A fed value is a binary: it equals a name word
// only when that word is not "", "+" or "#" (atoms) and has the same bytes; it is never a
// wildcard.  eq: word-list equality, which is equality of the bytes.
template <class PT, class PF, class PC>
GM_HD bool acl_match_bytes(PT T, uint32_t tl, PF F, uint32_t fl, bool eq, PC cid, uint32_t cl, PC usr,
                           uint32_t ul, uint32_t cflags) {
  if (eq) return tl == fl && bytes_equal(T, F, fl);
  uint32_t i = 0, j = 0;  // start of the current name / filter word
  for (;;) {
    uint32_t je = j;
    while (je < fl && F[je] != '/') ++je;
    const bool flast = (je == fl);
    const uint32_t flen = je - j;
    const bool fplus = (flen == 1 && F[j] == '+');
    const bool fhash = (flen == 1 && F[j] == '#');
    if (fhash && flast) {
      // match([H | T1], [H | T2]) before match(_, ['#']) (emqx_topic.erl:78-83)
      if (i < tl && T[i] == '#' && (i + 1 == tl || T[i + 1] == '/')) return i + 1 == tl;
      return true;
    }
    if (i > tl) return false;  // match([], [_|_])
    uint32_t ie = i;
    while (ie < tl && T[ie] != '/') ++ie;
    const uint32_t wl = ie - i;
    bool same = fplus;
    if (!same) {
      const bool fc = !(cflags & ACL_C_CID_UNDEF) && acl_word_is(F + j, flen, acl_ph_clientid());
      const bool fu = !fc && !(cflags & ACL_C_USR_UNDEF) && acl_word_is(F + j, flen, acl_ph_username());
      if (fc || fu) {
        const uint32_t vl = fc ? cl : ul;
        same = vl == wl && wl > 0 && !(wl == 1 && (T[i] == '+' || T[i] == '#')) &&
               bytes_equal(T + i, fc ? cid : usr, vl);
      } else {
        same = flen == wl && bytes_equal(T + i, F + j, flen);
      }
    }
    if (!same) return false;
    i = ie + 1;
    j = je + 1;
    if (flast) return i > tl;  // match([], []) ; match([_|_], [])
  }
}

}  // namespace gm
