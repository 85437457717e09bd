// gm_admit_match.h -- the admission checks of one topic name or topic filter on its raw bytes
// (DESIGN.md 6b "Admission"): emqx_topic:validate/2 (apps/emqx/src/emqx_topic.erl:98-130),
// emqx_topic:parse/1 (:206-233) and the clauses of emqx_mqtt_caps:do_check_pub /
// do_check_sub (apps/emqx/src/emqx_mqtt_caps.erl:94-105, 134-152).  Plain functions with no HIP
// call, written so that a device kernel and a host program run the same code: k_admit
// (gm_admit.inc) on the device, tests/host_harness/admit_dev_main.cpp (the kernel's phases, lane by
// lane) and tools/admit_host_bench.cpp on the CPU.
//
// The bytes of an item are read through a reader R with R.w8(i) = the 8 bytes at byte i of the
// item, little-endian (bytes at or past the item's end hold anything; a reader touches no memory
// word that holds none of the item's bytes, AdmGlob, or stays inside the LDS tile, AdmLds).
//
// validate/2 in one pass, 8 bytes at a time.  A word of 8 bytes is tested for '/', '#', '+', NUL
// and bytes >= 0x80 together; one with none of them (and nothing pending) only adds to the length
// of the current level.  One without a byte >= 0x80 visits its special bytes only (adm_ascii);
// only a word with a byte >= 0x80, or one that starts inside a sequence, is walked code point by
// code point (adm_codepoints).  Carried from word to word (AdmScan): the current level's length
// (0, 1, 2+), whether its first byte is '+' or '#', the bytes a UTF-8 sequence still expects with
// the range of the next one (RFC 3629: E0 A0..BF, ED 80..9F, F0 90..BF, F4 80..8F), the first
// verdict, the '/' count and whether some level is exactly '+' or '#'.
//
// The first event of a level decides (validate3, :125-130, matches code point by code point from
// the left): '#', '+' or NUL as a code point is topic_invalid_char; bytes that <<_/utf8>> does not
// accept are function_clause at the position where the sequence starts, so "E2 82 #" is
// function_clause and "# E2 82" topic_invalid_char.  A '/' inside a sequence ends the level
// (binary:split runs first, :159) and leaves a truncated sequence in it.  A level that is exactly
// '#' and not the last ends validate2 with 'topic_invalid_#' (:116-117); levels behind the first
// verdict are not examined, but still counted (levels/1, wildcard/1 read the whole item).
#pragma once
#include <stdint.h>

#include "gm_common.h"

#if defined(__HIPCC__)
#define GM_HD_MEMBER __host__ __device__ __forceinline__
#else
#define GM_HD_MEMBER inline
#endif

namespace gm {

// validate verdicts (emqx_gpumatch.h EMQXGM_ADMIT_V_*)
constexpr uint32_t ADM_V_OK = 0, ADM_V_EMPTY = 1, ADM_V_TOO_LONG = 2, ADM_V_NAME_ERROR = 3, ADM_V_HASH = 4,
                   ADM_V_CHAR = 5, ADM_V_FUNCTION_CLAUSE = 6;
constexpr uint32_t ADM_P_OK = 0, ADM_P_INVALID = 1;  // parse verdicts
// record word 0: validate | parse << 8 | caps reason << 16 | flags
constexpr uint32_t ADM_F_WILDCARD = 1u << 24, ADM_F_SHARED = 1u << 25, ADM_F_EXCLUSIVE = 1u << 26,
                   ADM_F_EXCL_LOOKUP = 1u << 27;
constexpr uint32_t ADM_NAME = 0, ADM_FILTER = 1;  // modes
// per-item input flags
constexpr uint32_t ADM_IN_QOS = 3u, ADM_IN_RETAIN = 4u, ADM_IN_HAS_SHARE = 8u;
constexpr uint32_t ADM_MAX_TOPIC_LEN = 65535;  // ?MAX_TOPIC_LEN
constexpr uint32_t ADM_MAX_ZONES = 256;
// a zone's caps as the kernel reads them: {max_topic_levels, max_qos_allowed | ADM_C_* bits}
constexpr uint32_t ADM_C_QOS = 0xFFu, ADM_C_RETAIN = 1u << 8, ADM_C_WILDCARD = 1u << 9, ADM_C_SHARED = 1u << 10,
                   ADM_C_EXCLUSIVE = 1u << 11;
// reason codes (apps/emqx/include/emqx_mqtt.hrl:173-192)
constexpr uint32_t ADM_RC_TOPIC_FILTER_INVALID = 0x8F, ADM_RC_TOPIC_NAME_INVALID = 0x90,
                   ADM_RC_RETAIN_NOT_SUPPORTED = 0x9A, ADM_RC_QOS_NOT_SUPPORTED = 0x9B,
                   ADM_RC_SHARED_NOT_SUPPORTED = 0x9E, ADM_RC_WILDCARD_NOT_SUPPORTED = 0xA2;
constexpr uint32_t ADM_RAISES = 0x100;  // emqxgm_admit_reason: parse raises inside handle_in

// ---- readers ----

// An item in global (or host) memory: aligned 8-byte words, only those that hold a byte of it.
struct AdmGlob {
  const uint8_t* p;
  uint32_t len;
  GM_HD_MEMBER uint64_t w8(uint32_t i) const {
    const uintptr_t a = (uintptr_t)(p + i);
    const uint64_t* q = (const uint64_t*)(a & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)(a & 7u);
    const uint64_t lo = q[0];
    if (sh == 0) return lo;
    const uint64_t hi = (8u - sh < len - i) ? q[1] : 0ull;
    return (lo >> (8 * sh)) | (hi << (64 - 8 * sh));
  }
};

// An item in an LDS tile of dwords (gm_tok.inc stage_tile): `s` = its byte offset in the tile.
// Three aligned dwords, funnel-shifted; the tile has a spare chunk behind its last byte.
struct AdmLds {
  const uint32_t* w;
  uint32_t s;
  GM_HD_MEMBER uint64_t w8(uint32_t i) const {
    const uint32_t x = s + i, wi = x >> 2, sh = 8 * (x & 3u);
    const uint64_t ab = ((uint64_t)w[wi + 1] << 32) | w[wi], bc = ((uint64_t)w[wi + 2] << 32) | w[wi + 1];
    return ((uint64_t)(uint32_t)(bc >> sh) << 32) | (uint32_t)(ab >> sh);
  }
};

// 0x80 in every byte of x that is zero (exact: no borrow between bytes).
GM_HD uint64_t adm_zero_bytes(uint64_t x) {
  constexpr uint64_t L = 0x7F7F7F7F7F7F7F7Full;
  return ~(((x & L) + L) | x | L);
}
GM_HD uint64_t adm_rep(uint32_t b) { return 0x0101010101010101ull * b; }

// ---- parse/1 ----

struct AdmParse {
  uint32_t verdict = ADM_P_OK;
  uint32_t off = 0;          // where the returned topic starts in the item
  uint32_t share_len = NONE; // length of the share name taken from the string
  uint32_t flags = 0;        // ADM_F_SHARED | ADM_F_EXCLUSIVE
  uint32_t slashes = 0;      // '/' in front of `off`: levels(topic) = levels(item) - slashes
};

template <class R>
GM_HD bool adm_has_prefix(const R r, uint32_t len, uint32_t at, uint64_t first8, uint32_t n, uint64_t rest) {
  if (len - at < n) return false;
  if (n <= 8) return ((r.w8(at) ^ first8) & (n == 8 ? ~0ull : ((1ull << (8 * n)) - 1))) == 0;
  return r.w8(at) == first8 && ((r.w8(at + 8) ^ rest) & ((1ull << (8 * (n - 8))) - 1)) == 0;
}
constexpr uint64_t ADM_SHARE8 = 0x002F657261687324ull;  // "$share/"
constexpr uint64_t ADM_EXCL8 = 0x6973756C63786524ull;   // "$exclusi"
constexpr uint64_t ADM_EXCL3 = 0x00000000002F6576ull;   // "ve/"

// emqx_topic:parse({Item, Options}), Options with `share` iff has_share (emqx_topic.erl:212-233).
template <class R>
GM_HD AdmParse adm_parse(const R r, uint32_t len, bool has_share) {
  AdmParse P;
  if (has_share) P.flags |= ADM_F_SHARED;
  if (adm_has_prefix(r, len, 0, ADM_SHARE8, 7, 0)) {
    if (has_share) {  // :213-214
      P.verdict = ADM_P_INVALID;
      return P;
    }
    // binary:split(Rest, <<"/">>) and binary:match(ShareName, [<<"+">>, <<"#">>]) (:216-223): the
    // first '/', '+' or '#' behind the prefix decides -- a '/' ends the share name
    uint32_t at = NONE;
    for (uint32_t i = 7; i < len && at == NONE; i += 8) {
      const uint64_t v = r.w8(i);
      uint64_t z = adm_zero_bytes(v ^ adm_rep('/')) | adm_zero_bytes(v ^ adm_rep('+')) | adm_zero_bytes(v ^ adm_rep('#'));
      if (len - i < 8) z &= (1ull << (8 * (len - i))) - 1;
      if (z) at = i + ((uint32_t)__builtin_ctzll(z) >> 3);
    }
    if (at == NONE || (uint8_t)(r.w8(at)) != '/') {
      P.verdict = ADM_P_INVALID;
      return P;
    }
    P.share_len = at - 7;
    P.off = at + 1;
    P.flags |= ADM_F_SHARED;
    P.slashes = 2;
    // parse(Filter, Options#{share => ShareName}): the first clause again, then '$exclusive/'
    if (adm_has_prefix(r, len, P.off, ADM_SHARE8, 7, 0)) {
      P.verdict = ADM_P_INVALID;
      return P;
    }
  }
  if (adm_has_prefix(r, len, P.off, ADM_EXCL8, 11, ADM_EXCL3)) {  // :225-231
    if (len - P.off == 11) {
      P.verdict = ADM_P_INVALID;
      return P;
    }
    P.off += 11;
    P.flags |= ADM_F_EXCLUSIVE;
    P.slashes += 1;
  }
  return P;
}

// ---- validate/2, levels/1 and wildcard/1 in one pass ----

struct AdmScan {
  uint32_t verdict = ADM_V_OK;  // the first one
  uint32_t slashes = 0;
  uint32_t wild = 0;      // some level is exactly '+' or '#'
  uint32_t wl = 0;        // bytes of the current level: 0, 1, 2 = more
  uint32_t w0 = 0;        // the level's first byte when that is '+' or '#', else 0
  uint32_t need = 0;      // continuation bytes the open sequence still expects
  uint32_t lo = 0x80, hi = 0xBF;  // the range of the next one
};

// The scan's state changes are written as selected values, never as stores under a condition: the
// compiler turned "store to this field or to that one" into a selected address and kept the state
// in scratch memory.
GM_HD void adm_verdict_if(AdmScan& S, bool c, uint32_t v) {
  S.verdict = (c && S.verdict == ADM_V_OK) ? v : S.verdict;
  S.need = c ? 0u : S.need;
}
GM_HD void adm_verdict(AdmScan& S, uint32_t v) { adm_verdict_if(S, true, v); }

// g > 0 bytes that are none of '/', '#', '+', NUL and below 0x80, with no sequence open.
GM_HD void adm_plain(AdmScan& S, uint32_t g) {
  adm_verdict_if(S, S.wl == 1 && S.w0 != 0, ADM_V_CHAR);  // '+x': the '+' at its head is a code point of the level
  S.wl = S.wl + g > 2 ? 2 : S.wl + g;
}

// One byte below 0x80 that is '/', '#', '+' or NUL, with no sequence open.
GM_HD void adm_special(AdmScan& S, uint32_t b) {
  const bool slash = b == '/';
  const bool one = S.wl == 1 && S.w0 != 0;  // the level so far is exactly '+' or '#'
  const bool head = b != 0 && S.wl == 0;    // '+' or '#' at a level's head: no event unless the level goes on
  // '/': a level that is '#' and not the last; else '#', '+' or NUL inside a level
  adm_verdict_if(S, slash ? (one && S.w0 == '#') : !head, slash ? ADM_V_HASH : ADM_V_CHAR);
  S.wild |= (slash && one) ? 1u : 0u;
  S.slashes += slash ? 1u : 0u;
  S.w0 = slash ? 0u : head ? b : S.w0;
  S.wl = slash ? 0u : S.wl + 1 > 2 ? 2 : S.wl + 1;
}

// A word of nb bytes without a byte >= 0x80, no sequence open: its special bytes (z: 0x80 per
// byte) and the runs between them.
GM_HD void adm_ascii(AdmScan& S, uint64_t v, uint64_t z, uint32_t nb) {
  uint32_t pos = 0;
  while (z) {
    const uint32_t k = (uint32_t)__builtin_ctzll(z) >> 3;
    z &= z - 1;
    if (k > pos) adm_plain(S, k - pos);
    adm_special(S, (uint32_t)(v >> (8 * k)) & 0xFFu);
    pos = k + 1;
  }
  if (nb > pos) adm_plain(S, nb - pos);
}

// A word of nb bytes code point by code point (<<C/utf8, _/binary>>, RFC 3629).
GM_HD void adm_codepoints(AdmScan& S, uint64_t v, uint32_t nb) {
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t b = (uint32_t)(v >> (8 * k)) & 0xFFu;
    if (S.need) {
      if (b >= S.lo && b <= S.hi) {
        --S.need;
        S.lo = 0x80;
        S.hi = 0xBF;
        continue;  // (the level has two bytes or more already)
      }
      adm_verdict(S, ADM_V_FUNCTION_CLAUSE);  // truncated: the byte starts over below
    }
    if (b < 0x80) {
      if (b == '/' || b == '#' || b == '+' || b == 0) adm_special(S, b);
      else adm_plain(S, 1);
      continue;
    }
    adm_plain(S, 1);
    if (S.verdict != ADM_V_OK) continue;  // behind the first verdict nothing is decoded
    // (values, not conditional stores into S: those became a selected address and put S in scratch)
    const uint32_t need = (b >= 0xC2 && b <= 0xDF) ? 1u : (b >= 0xE0 && b <= 0xEF) ? 2u : (b >= 0xF0 && b <= 0xF4) ? 3u : 0u;
    if (need == 0) {
      adm_verdict(S, ADM_V_FUNCTION_CLAUSE);  // 80..C1, F5..FF
      continue;
    }
    S.need = need;
    S.lo = b == 0xE0 ? 0xA0u : b == 0xF0 ? 0x90u : 0x80u;  // overlong forms
    S.hi = b == 0xED ? 0x9Fu : b == 0xF4 ? 0x8Fu : 0xBFu;  // surrogates; above U+10FFFF
  }
}

// The item's len (1 .. ADM_MAX_TOPIC_LEN) bytes: S.verdict is validate2's (:111-123), S.slashes
// and S.wild are the whole item's.
template <class R>
GM_HD void adm_scan(const R r, uint32_t len, AdmScan& S) {
  for (uint32_t i = 0; i < len; i += 8) {
    const uint32_t nb = len - i < 8 ? len - i : 8u;
    uint64_t v = r.w8(i);
    if (nb < 8) {  // bytes past the end read as 'a'
      const uint64_t m = (1ull << (8 * nb)) - 1;
      v = (v & m) | (adm_rep('a') & ~m);
    }
    const uint64_t high = v & adm_rep(0x80);
    if (high || S.need) {
      adm_codepoints(S, v, nb);
      continue;
    }
    const uint64_t z = adm_zero_bytes(v ^ adm_rep('/')) | adm_zero_bytes(v ^ adm_rep('#')) |
                       adm_zero_bytes(v ^ adm_rep('+')) | adm_zero_bytes(v);
    if (z == 0 && !(S.wl == 1 && S.w0)) {
      S.wl = 2;
      continue;
    }
    adm_ascii(S, v, z, nb);
  }
  if (S.need) adm_verdict(S, ADM_V_FUNCTION_CLAUSE);  // the item ends inside a sequence
  if (S.wl == 1 && S.w0) S.wild = 1;                  // a last '#' or '+' is no event
}

// ---- caps ----

// do_check_pub (emqx_mqtt_caps.erl:94-105).
GM_HD uint32_t adm_caps_pub(uint32_t levels, uint32_t in_flags, uint32_t cap_levels, uint32_t cap_bits) {
  if (cap_levels > 0 && levels > cap_levels) return ADM_RC_TOPIC_NAME_INVALID;
  if ((in_flags & ADM_IN_QOS) > (cap_bits & ADM_C_QOS)) return ADM_RC_QOS_NOT_SUPPORTED;
  if ((in_flags & ADM_IN_RETAIN) && !(cap_bits & ADM_C_RETAIN)) return ADM_RC_RETAIN_NOT_SUPPORTED;
  return 0;
}

// do_check_sub (:134-152); ADM_F_EXCL_LOOKUP in the answer: the clause that asks
// emqx_exclusive_subscription was reached (:144-150).
GM_HD uint32_t adm_caps_sub(uint32_t levels, uint32_t flags, uint32_t cap_levels, uint32_t cap_bits) {
  if (cap_levels > 0 && levels > cap_levels) return ADM_RC_TOPIC_FILTER_INVALID;
  if ((flags & ADM_F_WILDCARD) && !(cap_bits & ADM_C_WILDCARD)) return ADM_RC_WILDCARD_NOT_SUPPORTED;
  if ((flags & ADM_F_SHARED) && !(cap_bits & ADM_C_SHARED)) return ADM_RC_SHARED_NOT_SUPPORTED;
  if ((flags & ADM_F_EXCLUSIVE) && !(cap_bits & ADM_C_EXCLUSIVE)) return ADM_RC_TOPIC_FILTER_INVALID;
  return (flags & ADM_F_EXCLUSIVE) ? ADM_F_EXCL_LOOKUP : 0u;
}

// ---- one item ----

struct AdmRecord {
  uint32_t w0, levels, off, share_len;
};

// What the offsets decide before a byte is read.
GM_HD uint32_t adm_length_verdict(uint32_t len) {
  return len == 0 ? ADM_V_EMPTY : len > ADM_MAX_TOPIC_LEN ? ADM_V_TOO_LONG : ADM_V_OK;
}

// The record of an item from its parse (FILTER; a default AdmParse for NAME), its scan (not run
// for an empty or too long item) and its zone's caps.
GM_HD AdmRecord adm_record(uint32_t mode, uint32_t len, const AdmParse& P, const AdmScan& S, uint32_t in_flags,
                           uint32_t cap_levels, uint32_t cap_bits) {
  uint32_t v = adm_length_verdict(len);
  if (v == ADM_V_OK) v = S.verdict;
  if (v == ADM_V_OK && mode == ADM_NAME && S.wild) v = ADM_V_NAME_ERROR;  // :105-109
  AdmRecord r{v | (P.verdict << 8), 0u, 0u, NONE};
  if (P.verdict != ADM_P_OK) return r;
  r.off = P.off;  // parse's answer is a function of the bytes alone
  r.share_len = P.share_len;
  if (len > ADM_MAX_TOPIC_LEN) {  // levels, wildcard and caps: not run
    r.w0 |= P.flags;
    return r;
  }
  r.levels = S.slashes + 1 - P.slashes;
  uint32_t flags = P.flags | (S.wild ? ADM_F_WILDCARD : 0u), rc;
  if (mode == ADM_NAME) {
    rc = adm_caps_pub(r.levels, in_flags, cap_levels, cap_bits);
  } else {
    rc = adm_caps_sub(r.levels, flags, cap_levels, cap_bits);
    flags |= rc & ADM_F_EXCL_LOOKUP;
    rc &= 0xFFu;
  }
  r.w0 |= (rc << 16) | flags;
  return r;
}

// The channel's first failure (emqxgm_admit_reason): emqx_packet:check/1, then parse inside
// handle_in, then the caps.
GM_HD uint32_t adm_reason(uint32_t mode, uint32_t w0) {
  if (w0 & 0xFFu) return mode == ADM_NAME ? ADM_RC_TOPIC_NAME_INVALID : ADM_RC_TOPIC_FILTER_INVALID;
  if ((w0 >> 8) & 0xFFu) return ADM_RAISES;
  return (w0 >> 16) & 0xFFu;
}

}  // namespace gm
