// gm_share_match.h -- shared subscriptions: which member of a group gets a message (DESIGN.md 6b
// "Shared subscriptions"): emqx_shared_sub's bag of {Group, Topic, SubPid} (apps/emqx/src/
// emqx_shared_sub.erl:104-117), found by (Group, Topic) (subscribers/2, :391-392) and picked from
// by the group's strategy (pick/6, :309-379).  Plain functions with no HIP call, written so that a
// device kernel and a host program run the same code: k_share (gm_share.inc) and the host side of
// the emqxgm_share_* C-ABI (gm_share.cpp) on the device path, tests/host_harness/
// share_dev_main.cpp on the CPU.
//
// Key table: one open-addressing table (linear probing, a power of two of 16-byte slots, at most
// half full with deleted marks counted).  A slot is {tag of (group, key_hash of the topic's bytes),
// first word of the key's run in the member pool, index of the key}.  SH_EMPTY and SH_DELETED have
// bit 63 set, which no tag has.  A probe starts at sh_home(tag) and stops at an empty slot; every
// hit on a tag is confirmed on the key's group and bytes and the probe goes on when they differ:
// no answer rests on a hash.
//
// Keys: key k has the group kg[k] and the bytes kb[ko[k] .. ko[k + 1]).
//
// Member pool: 32-bit words.  A key's run is contiguous:
//   words 0..3   {n_all, n_local, strategy, 0}
//   then         the n_all member handles in subscribe order, bit 31 set for a local member
//   then         the n_local local handles in that order (bit 31 set too)
// so a pick of the `local` strategy is one load like every other pick.
#pragma once
#include <stdint.h>

#include "gm_common.h"
#include "gm_match.h"

namespace gm {

// EMQXGM_SHARE_*: the strategies of emqx_shared_sub.erl:78-85 ...
constexpr uint32_t SH_RANDOM = 0, SH_ROUND_ROBIN = 1, SH_RR_PER_GROUP = 2, SH_STICKY = 3, SH_LOCAL = 4,
                   SH_HASH_CLIENTID = 5, SH_HASH_TOPIC = 6, SH_STRATEGIES = 7;
// ... and the status of an answer
constexpr uint32_t SH_PICKED = 0, SH_NO_SUBSCRIBERS = 1, SH_HOST_STRATEGY = 2, SH_COUNTER_PENDING = 3,
                   SH_MALFORMED = 4,  // (never leaves the library: the call returns -EIO)
                   SH_NOT_SHARED = 5;  // k_pubshare: the entry's dest is a node, nothing was picked
constexpr uint32_t SH_LOCAL_BIT = 1u << 31;
constexpr uint32_t DEST_GROUP_BIT = 1u << 31;  // EMQXGM_DEST_GROUP: the dest of an aggre entry is a group
constexpr uint32_t SH_HDR_WORDS = 4;
constexpr uint64_t SH_EMPTY = 1ull << 63;
constexpr uint64_t SH_DELETED = (1ull << 63) | 1ull;
constexpr uint32_t SH_MIN_SLOTS = 8;

struct alignas(16) ShSlot {
  uint64_t tag;
  uint32_t run;  // first word of the key's run in the member pool
  uint32_t key;  // group kg[key], bytes kb[ko[key] .. ko[key + 1])
};

// tag_mask 0 is production (63 bits); 1..16 kept bits give the tests chains of equal tags.
GM_HD uint64_t sh_tag_mask(uint32_t hash_bits) { return hash_bits ? (1ull << hash_bits) - 1 : ~SH_EMPTY; }
GM_HD uint64_t sh_tag(uint32_t group, uint64_t topic_hash, uint64_t tag_mask) {
  return fmix64(topic_hash ^ ((uint64_t)group * 0x9e3779b97f4a7c15ull)) & tag_mask;
}
GM_HD uint64_t sh_key_tag(uint32_t group, const uint8_t* topic, uint32_t len, uint64_t tag_mask) {
  return sh_tag(group, key_hash(topic, len, ~0ull), tag_mask);
}
GM_HD uint64_t sh_home(uint64_t tag, uint64_t mask) { return fmix64(tag + 0x2545f4914f6cdd1dull) & mask; }

// The next slot from *i on whose tag is `tag`, or NONE at the empty slot that ends the chain (or
// after `mask + 1` slots); *i is left past the slot returned, *steps counts the slots looked at.
// A probe of a key starts with *i = sh_home(tag, mask) and *steps = 0; the caller confirms the
// hit (sh_confirm) and calls again when it fails.
template <class PS>
GM_HD uint32_t sh_probe_next(PS tab, uint64_t mask, uint64_t tag, uint64_t* i, uint64_t* steps) {
  while (*steps <= mask) {
    const uint64_t at = *i;
    const uint64_t t = tab[at].tag;
    ++*steps;
    *i = (at + 1) & mask;
    if (t == SH_EMPTY) return NONE;
    if (t == tag) return (uint32_t)at;  // (SH_DELETED is no tag)
  }
  return NONE;
}

// Whether key `key` (< n_keys, checked by the caller) is (group, topic bytes).
GM_HD bool sh_confirm(const uint32_t* kg, const uint32_t* ko, const uint8_t* kb, uint32_t key, uint32_t group,
                      const uint8_t* topic, uint32_t len) {
  if (kg[key] != group) return false;
  const uint32_t k0 = ko[key], kl = ko[key + 1] - k0;
  return kl == len && bytes_equal(kb + k0, topic, len);
}

// Whether the run at pool[run] lies inside the pool and is well formed; its header into *n_all,
// *n_local, *strategy.  Checked before any word of the run is followed.
GM_HD bool sh_read_run(const uint32_t* pool, uint64_t pool_words, uint32_t run, uint32_t* n_all, uint32_t* n_local,
                       uint32_t* strategy) {
  if ((uint64_t)run + SH_HDR_WORDS > pool_words) return false;
  *n_all = pool[run];
  *n_local = pool[run + 1];
  *strategy = pool[run + 2];
  if (*n_local > *n_all || *strategy >= SH_STRATEGIES) return false;
  return (uint64_t)run + SH_HDR_WORDS + *n_all + *n_local <= pool_words;
}
GM_HD uint32_t sh_run_words(uint32_t n_all, uint32_t n_local) { return SH_HDR_WORDS + n_all + n_local; }

struct ShDecision {
  uint32_t status;  // SH_*
  uint32_t pos;     // SH_PICKED: the word of the run, counted from its first, that holds the member
  uint32_t state;   // the round_robin state to hand back
};

// pick/6 for a first dispatch (FailedSubs = #{}) over a key of n_all members, n_local of them
// local.  hc = erlang:phash2(ClientId), ht = erlang:phash2(SourceTopic), draw = 32 random bits
// that stand in for rand:uniform(Count) as 1 + draw rem Count, state = the caller's round_robin
// state or NONE for undefined.
//   do_pick([], ..) -> false                                                        (:334-335)
//   sticky: the stuck pid's liveness is the caller's, so the caller decides         (:309-329)
//   pick_subscriber(.., [Sub]) -> Sub, before any strategy, no state touched        (:346-347)
//   local: the local members if there are any, else all, then as random            (:348-354)
//   random, hash_clientid, hash_topic                                               (:359-364)
//   round_robin: (N + 1) rem Count, or the draw when undefined; Rem goes back       (:365-372)
//   round_robin_per_group: the counter step is the host's (sh_counter_step)         (:373-379)
GM_HD ShDecision sh_decide(uint32_t n_all, uint32_t n_local, uint32_t strategy, uint32_t hc, uint32_t ht,
                           uint32_t draw, uint32_t state) {
  ShDecision d{SH_PICKED, SH_HDR_WORDS, state};
  if (n_all == 0) {
    d.status = SH_NO_SUBSCRIBERS;
    return d;
  }
  if (strategy == SH_STICKY) {
    d.status = SH_HOST_STRATEGY;
    return d;
  }
  if (n_all == 1) return d;
  switch (strategy) {
    case SH_RANDOM:
      d.pos = SH_HDR_WORDS + draw % n_all;
      break;
    case SH_HASH_CLIENTID:
      d.pos = SH_HDR_WORDS + hc % n_all;
      break;
    case SH_HASH_TOPIC:
      d.pos = SH_HDR_WORDS + ht % n_all;
      break;
    case SH_LOCAL:
      if (n_local == 0) d.pos = SH_HDR_WORDS + draw % n_all;
      else if (n_local == 1) d.pos = SH_HDR_WORDS + n_all;
      else d.pos = SH_HDR_WORDS + n_all + draw % n_local;
      break;
    case SH_ROUND_ROBIN:
      d.state = state == NONE ? draw % n_all : (uint32_t)(((uint64_t)state + 1) % n_all);
      d.pos = SH_HDR_WORDS + d.state;
      break;
    case SH_RR_PER_GROUP:
      d.status = SH_COUNTER_PENDING;
      break;
    default:
      d.status = SH_MALFORMED;
      break;
  }
  return d;
}

// ets:update_counter(Key, {2, 1, Count, 1}, {Key, 0}) (:377-379): c + 1, or 1 when that exceeds
// Count; an absent counter reads 0.  The value is both the new counter and Nth.
GM_HD uint32_t sh_counter_step(uint32_t c, uint32_t count) { return c >= count ? 1u : c + 1u; }

}  // namespace gm
