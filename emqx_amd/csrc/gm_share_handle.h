// gm_share_handle.h -- the shared-subscription handle (gm_share.cpp) as the library's own files see
// it: gm_share.cpp, which owns it, and gm_pubshare.cpp, whose publish entry picks from its tables
// inside the engine's pass.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/emqx_gpumatch.h"
#include "gm_internal.h"
#include "gm_kernels.h"
#include "gm_share_match.h"

namespace gm {

struct ShBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// A pool: its host mirror, its device array and how many elements of the mirror the device has.
template <class T>
struct ShPool {
  std::vector<T> h;
  ShBuf d;
  size_t dev_n = 0;
};

struct ShTable {
  std::vector<ShSlot> h;
  ShBuf d;
  uint64_t live = 0, tomb = 0;
  std::vector<uint32_t> touched;  // slots changed since the last upload
  bool whole = true;              // the device has no copy of this table's size
};

enum { SH_OP_SUB, SH_OP_UNSUB, SH_OP_DOWN, SH_OP_STRATEGY };
struct ShOp {
  uint32_t op = 0, group = 0, sub = 0, arg = 0;  // arg: the local flag or the strategy
  size_t t0 = 0;                                 // the topic in ptb
  uint32_t tl = 0;
};

// What the pending mutations make of one (group, topic, sub): seq orders it against a pending
// subscriber_down of the sub.
struct ShTriple {
  uint32_t seq = 0;
  int state = -1;  // -1 absent, 0 subscribed remote, 1 subscribed local
};

// scratch: the pass's groups, topics, offsets, hc, ht, draw, state, answers; the error word; a
// publish pass's state list (st_ptr, st_group, st_filter, st_value)
enum { SH_GR, SH_RB, SH_RO, SH_HC, SH_HT, SH_DR, SH_ST, SH_OUT, SH_CTL, SH_SP, SH_SG, SH_SF, SH_SV, SH_SLOTS };

}  // namespace gm

struct emqxgm_share {
  std::mutex mu;
  int32_t device = 0;
  hipStream_t stream = nullptr;
  uint64_t tag_mask = 0;
  // committed
  gm::ShTable tab;
  gm::ShPool<uint32_t> pool, ko, kg;
  gm::ShPool<uint8_t> kb;
  std::vector<uint32_t> pool_touched;  // header words rewritten in place since the last upload
  std::vector<uint32_t> krun;          // per key: its run, NONE once the key is gone (host only)
  std::vector<uint32_t> ctr;           // per key: the round_robin_per_group counter, NONE if none
  std::unordered_map<std::string, uint32_t> orphan_ctr;  // counters of keys without members
  std::unordered_map<uint32_t, uint32_t> gstrat;
  uint32_t def_strat = gm::SH_ROUND_ROBIN;  // emqx_schema.erl: shared_subscription_strategy
  uint64_t members = 0, live_words = 0, garbage_words = 0, load_rebuilds = 0, garbage_rebuilds = 0, growths = 0,
           max_chain = 0;
  // pending
  bool broken = false;  // a commit failed half way: the device arrays and the mirror disagree
  std::vector<gm::ShOp> pend;
  std::vector<uint8_t> ptb;
  std::unordered_map<std::string, gm::ShTriple> ptri;
  std::unordered_map<uint32_t, uint32_t> pdown;
  // tuning, scratch
  uint64_t pass_names = 1ull << 20;
  uint32_t load_pct = 50, garbage_pct = 100;
  bool timing = false, stage_lds = true;  // MEASUREMENTS.md r16
  hipEvent_t ev[2] = {nullptr, nullptr};
  double kernel_ms = 0;
  gm::ShBuf sc[gm::SH_SLOTS];
  std::vector<uint32_t> h_off;
  std::vector<uint32_t> h_pub;  // emqxgm_publish_shared_batch: the call's answers, 4 words per entry
};

namespace gm {

// What a publish pass passes per topic (emqxgm_publish_shared_batch's arrays, whole).
struct PubShareIn {
  const uint32_t *hc = nullptr, *ht = nullptr, *draw = nullptr;
  const uint32_t *st_ptr = nullptr, *st_group = nullptr, *st_filter = nullptr, *st_value = nullptr;
};
constexpr size_t SH_CTL_BYTES = 8;
// Scratch slot `slot` (SH_*) of at least `bytes`, regrown after a wait for the handle's stream.
int share_grow(emqxgm_share* a, int slot, uint64_t bytes);
// The committed tables as a kernel takes them.
void share_tables(const emqxgm_share* a, ShareTables& A);
// The round_robin_per_group steps of the np answers at o, in their order: every
// SH_COUNTER_PENDING answer takes the next value of its key's counter and becomes a pick
// (emqxgm_share_pick's passes and share_pub_pass's both end in this).
int share_counter_steps(emqxgm_share* a, uint32_t* o, uint64_t np);
// The pick of every entry of one chunk of a publish pass (k_pubshare) into a->h_pub, then the
// round_robin_per_group counter steps in entry order.  a->mu is held by the caller.
int share_pub_pass(emqxgm_share* a, const gm_pub_chunk& c, const PubShareIn& in);

}  // namespace gm
