// gm_share.cpp -- host side of the shared-subscription membership resident on the device (k_share,
// gm_share.inc): the pending mutations, the incremental commit, the full rebuild, the pass driver,
// the round_robin_per_group counter step and the emqxgm_share_* C-ABI of include/
// emqx_gpumatch.h.  A handle of its own, beside the engine, the retainer, the rule set, the ACL
// list and the ACL database.
//
// Reference: emqx_shared_sub (apps/emqx/src/emqx_shared_sub.erl): subscribe/3 and unsubscribe/3
// (:416-431), cleanup_down/1 (:509-519), strategy/1 (:159-164), pick/6 (:309-379),
// maybe_insert_round_robin_count/1 and maybe_delete_round_robin_count/1 (:484-494).
//
// The host keeps a mirror of every device array (gm_share_match.h: the key table, the member
// pool, key bytes, offsets and groups).  A commit applies the pending mutations, in call order, to
// the member lists of the keys they touch; then each touched key's new run is appended to the pool
// and its slot patched, the run it replaces is counted as garbage, and a key whose list became
// empty leaves SH_DELETED in its slot.  A strategy change rewrites the strategy word of the runs
// of that group's keys in place.  Then only what changed goes to the device: the appended tails of
// the pools (a pool grows with slack; growing is a new allocation and a device-to-device copy),
// the rewritten header words and the touched slots as 16-byte copies on the handle's stream.  A
// full rebuild compacts the pools and rehashes the table into a fresh mirror that is uploaded
// whole; it runs when an insert would take the table's used slots (deleted ones included) past
// "rebuild_load_pct" of its slots, or when the garbage words pass "rebuild_garbage_pct" percent of
// the live ones.  The mirror changes before the uploads: a commit that fails on the device marks
// the handle broken, and every later call returns -EIO.  A pick holds the handle's mutex for its
// passes, so a commit never runs beside a kernel.
//
// The round_robin_per_group counters live here, one per key, and the host takes their step after
// the device pass (sh_counter_step): requests of one call on one key take consecutive values in
// request order, with one writer.  The handle itself is declared in gm_share_handle.h, which
// gm_pubshare.cpp (the pick inside the publish pass) shares: it takes the tables, a scratch slot
// and the counter steps from here (share_tables, share_grow, share_counter_steps).
//
// With -DGM_SHARE_EXACT_ALLOC every device array is exactly the bytes in use (no floor, no growth
// slack): tests/host_harness/share_dev_main.cpp runs this file and the kernel's phases on the CPU
// under ASan, where a read or write one byte past any array then lands in a redzone.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/emqx_gpumatch.h"
#include "gm_common.h"
#include "gm_kernels.h"
#include "gm_share_handle.h"
#include "gm_share_match.h"

using namespace gm;

namespace {

// A key a commit touches: its member list and counter as the mutations leave them.
struct ShWork {
  std::vector<uint32_t> m;  // handles, SH_LOCAL_BIT for a local member
  uint32_t ctr = NONE;      // NONE: no counter
  bool changed = false;
};

constexpr uint64_t SH_PASS_MAX = 1ull << 28;
constexpr uint64_t SH_INDEX_MAX = 0xFFFFFFF0ull;  // pool words, keys, key bytes
constexpr size_t SH_PATCH_MAX = 256;              // touched slots or words beyond this: one copy
constexpr uint32_t SH_HANDLE_MAX = 1u << 31;      // member and group handles are below this

std::string sh_key(uint32_t group, const uint8_t* topic, uint32_t len) {
  std::string k((const char*)&group, 4);
  if (len) k.append((const char*)topic, len);
  return k;
}

#define SHCHK(expr)                        \
  do {                                     \
    if ((expr) != hipSuccess) return -EIO; \
  } while (0)

void sh_free(ShBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b = ShBuf();
}

int sh_upload(const void* src, size_t bytes, ShBuf& b) {
  sh_free(b);
  if (!bytes) return 0;
  SHCHK(hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  SHCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

// The device array of a pool follows its mirror: grown when the mirror no longer fits (a new
// allocation and a device-to-device copy of what the device has), then the mirror's new tail.
template <class T>
int sh_sync(emqxgm_share* s, ShPool<T>& p) {
  const size_t need = p.h.size() * sizeof(T);
#ifdef GM_SHARE_EXACT_ALLOC
  const bool grow = need != p.d.bytes;
  const size_t cap = need;
#else
  const bool grow = need > p.d.bytes;
  const size_t cap = std::max<size_t>(need + need / 2, 256);
#endif
  if (grow) {
    ShBuf nb;
    if (cap) {
      SHCHK(hipMalloc(&nb.p, cap));
      nb.bytes = cap;
    }
    if (p.dev_n) {
      if (hipMemcpy(nb.p, p.d.p, p.dev_n * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) {
        sh_free(nb);
        return -EIO;
      }
      ++s->growths;
    }
    sh_free(p.d);
    p.d = nb;
  }
  if (p.h.size() > p.dev_n)
    SHCHK(hipMemcpy((T*)p.d.p + p.dev_n, p.h.data() + p.dev_n, (p.h.size() - p.dev_n) * sizeof(T),
                    hipMemcpyHostToDevice));
  p.dev_n = p.h.size();
  return 0;
}

template <class T>
void sh_drop(ShPool<T>& p) {
  sh_free(p.d);
  p.dev_n = 0;
}

// The member pool: its tail, then the header words rewritten among the words the device had.
int sh_sync_pool(emqxgm_share* s) {
  const size_t had = s->pool.dev_n;
  const int rc = sh_sync(s, s->pool);
  if (rc) return rc;
  if (s->pool_touched.size() > SH_PATCH_MAX) {
    if (had) SHCHK(hipMemcpy(s->pool.d.p, s->pool.h.data(), had * 4, hipMemcpyHostToDevice));
  } else {
    for (uint32_t w : s->pool_touched)
      if (w < had)
        SHCHK(hipMemcpyAsync((uint32_t*)s->pool.d.p + w, &s->pool.h[w], 4, hipMemcpyHostToDevice, s->stream));
  }
  s->pool_touched.clear();
  return 0;
}

int sh_sync_table(emqxgm_share* s, ShTable& t) {
  if (t.whole) {
    const int rc = sh_upload(t.h.data(), t.h.size() * sizeof(ShSlot), t.d);
    if (rc) return rc;
  } else if (t.touched.size() > SH_PATCH_MAX) {
    SHCHK(hipMemcpy(t.d.p, t.h.data(), t.h.size() * sizeof(ShSlot), hipMemcpyHostToDevice));
  } else {
    for (uint32_t i : t.touched)
      SHCHK(hipMemcpyAsync((ShSlot*)t.d.p + i, &t.h[i], sizeof(ShSlot), hipMemcpyHostToDevice, s->stream));
  }
  t.whole = false;
  t.touched.clear();
  return 0;
}

// Slots for `keys` keys at the handle's load limit.
uint64_t sh_slots_for(const emqxgm_share* s, uint64_t keys) {
  uint64_t want = (keys * 100 + s->load_pct - 1) / s->load_pct, n = SH_MIN_SLOTS;
  while (n < want) n <<= 1;
  return n;
}

void sh_table_reset(ShTable& t, uint64_t slots) {
  t.h.assign(slots, ShSlot{SH_EMPTY, 0, 0});
  t.live = t.tomb = 0;
  t.touched.clear();
  t.whole = true;
}

// The slot of (group, topic), or NONE; *free_at = where an insert of the key goes (the first
// deleted slot of its chain, else the empty slot that ends it).
uint32_t sh_find(const emqxgm_share* s, uint32_t group, const uint8_t* topic, uint32_t len, uint32_t* free_at) {
  const ShTable& t = s->tab;
  const uint64_t mask = t.h.size() - 1;
  const uint64_t tag = sh_key_tag(group, topic, len, s->tag_mask);
  uint64_t i = sh_home(tag, mask);
  *free_at = NONE;
  for (uint64_t step = 0; step <= mask; ++step, i = (i + 1) & mask) {
    const ShSlot& e = t.h[i];
    if (e.tag == SH_EMPTY) {
      if (*free_at == NONE) *free_at = (uint32_t)i;
      return NONE;
    }
    if (e.tag == SH_DELETED) {
      if (*free_at == NONE) *free_at = (uint32_t)i;
      continue;
    }
    if (e.tag != tag) continue;
    if (sh_confirm(s->kg.h.data(), s->ko.h.data(), s->kb.h.data(), e.key, group, topic, len)) return (uint32_t)i;
  }
  return NONE;
}

void sh_touch(ShTable& t, uint32_t i) {
  if (!t.whole && t.touched.size() <= SH_PATCH_MAX) t.touched.push_back(i);
}

uint32_t sh_strategy(const emqxgm_share* s, uint32_t group) {
  auto it = s->gstrat.find(group);
  return it == s->gstrat.end() ? s->def_strat : it->second;
}

uint32_t sh_words_at(const emqxgm_share* s, uint32_t run) {
  return sh_run_words(s->pool.h[run], s->pool.h[run + 1]);
}

// Appends the run of members m (in order, SH_LOCAL_BIT on the local ones) to pool.
uint32_t sh_append_run(std::vector<uint32_t>& pool, const uint32_t* m, uint32_t n, uint32_t strategy) {
  const uint32_t run = (uint32_t)pool.size();
  uint32_t n_local = 0;
  for (uint32_t i = 0; i < n; ++i) n_local += (m[i] & SH_LOCAL_BIT) != 0;
  const uint32_t hdr[SH_HDR_WORDS] = {n, n_local, strategy, 0};
  pool.insert(pool.end(), hdr, hdr + SH_HDR_WORDS);
  pool.insert(pool.end(), m, m + n);
  for (uint32_t i = 0; i < n; ++i)
    if (m[i] & SH_LOCAL_BIT) pool.push_back(m[i]);
  return run;
}

// Compacts the pools and rehashes the table (sized for `extra` more keys) into a fresh mirror;
// everything is uploaded whole by the commit that called it.  Keys are renumbered.
void sh_rebuild(emqxgm_share* s, uint64_t extra) {
  std::vector<uint32_t> npool, nko{0}, nkg, nkrun, nctr;
  std::vector<uint8_t> nkb;
  npool.reserve((size_t)s->live_words);
  ShTable& t = s->tab;
  std::vector<ShSlot> nh(sh_slots_for(s, t.live + extra), ShSlot{SH_EMPTY, 0, 0});
  const uint64_t mask = nh.size() - 1;
  s->max_chain = 0;
  for (const ShSlot& e : t.h) {
    if (e.tag == SH_EMPTY || e.tag == SH_DELETED) continue;
    const uint32_t n_all = s->pool.h[e.run];
    ShSlot ns{e.tag, 0, (uint32_t)nkg.size()};
    ns.run = sh_append_run(npool, s->pool.h.data() + e.run + SH_HDR_WORDS, n_all, s->pool.h[e.run + 2]);
    nkb.insert(nkb.end(), s->kb.h.begin() + s->ko.h[e.key], s->kb.h.begin() + s->ko.h[e.key + 1]);
    nko.push_back((uint32_t)nkb.size());
    nkg.push_back(s->kg.h[e.key]);
    nkrun.push_back(ns.run);
    nctr.push_back(s->ctr[e.key]);
    uint64_t i = sh_home(e.tag, mask), chain = 1;
    for (; nh[i].tag != SH_EMPTY; i = (i + 1) & mask) ++chain;
    nh[i] = ns;
    s->max_chain = std::max(s->max_chain, chain);
  }
  t.h.swap(nh);
  t.tomb = 0;
  t.touched.clear();
  t.whole = true;
  s->pool.h.swap(npool);
  s->kb.h.swap(nkb);
  s->ko.h.swap(nko);
  s->kg.h.swap(nkg);
  s->krun.swap(nkrun);
  s->ctr.swap(nctr);
  sh_drop(s->pool);
  sh_drop(s->kb);
  sh_drop(s->ko);
  sh_drop(s->kg);
  s->pool_touched.clear();
  s->live_words = s->pool.h.size();
  s->garbage_words = 0;
}

void sh_clear_pending(emqxgm_share* s) {
  s->pend.clear();
  s->ptb.clear();
  s->ptri.clear();
  s->pdown.clear();
}

// Whether (group, topic, sub) is subscribed once the pending mutations are applied: -1 no,
// 0 as a remote member, 1 as a local one.
int sh_triple_state(const emqxgm_share* s, uint32_t group, const uint8_t* topic, uint32_t len, uint32_t sub) {
  std::string k3 = sh_key(group, topic, len);
  k3.append((const char*)&sub, 4);
  const auto dn = s->pdown.find(sub);
  const auto it = s->ptri.find(k3);
  if (it != s->ptri.end() && (dn == s->pdown.end() || dn->second < it->second.seq)) return it->second.state;
  if (dn != s->pdown.end()) return -1;
  uint32_t free_at;
  const uint32_t at = sh_find(s, group, topic, len, &free_at);
  if (at == NONE) return -1;
  const uint32_t run = s->tab.h[at].run, n_all = s->pool.h[run];
  for (uint32_t i = 0; i < n_all; ++i) {
    const uint32_t m = s->pool.h[run + SH_HDR_WORDS + i];
    if ((m & ~SH_LOCAL_BIT) == sub) return (m & SH_LOCAL_BIT) ? 1 : 0;
  }
  return -1;
}

void sh_pend(emqxgm_share* s, uint32_t op, uint32_t group, const uint8_t* topic, uint32_t len, uint32_t sub,
             uint32_t arg) {
  ShOp e;
  e.op = op;
  e.group = group;
  e.sub = sub;
  e.arg = arg;
  e.t0 = s->ptb.size();
  e.tl = len;
  if (len) s->ptb.insert(s->ptb.end(), topic, topic + len);
  const uint32_t seq = (uint32_t)s->pend.size() + 1;
  if (op == SH_OP_SUB || op == SH_OP_UNSUB) {
    std::string k3 = sh_key(group, topic, len);
    k3.append((const char*)&sub, 4);
    s->ptri[k3] = ShTriple{seq, op == SH_OP_SUB ? (int)(arg != 0) : -1};
  } else if (op == SH_OP_DOWN) {
    s->pdown[sub] = seq;
  }
  s->pend.push_back(e);
}

// The key's list and counter as committed, into the commit's working set on first touch.
ShWork& sh_load(emqxgm_share* s, std::unordered_map<std::string, ShWork>& work, std::vector<std::string>& order,
                uint32_t group, const uint8_t* topic, uint32_t len) {
  const std::string k = sh_key(group, topic, len);
  auto it = work.find(k);
  if (it != work.end()) return it->second;
  ShWork w;
  uint32_t free_at;
  const uint32_t at = sh_find(s, group, topic, len, &free_at);
  if (at != NONE) {
    const ShSlot& e = s->tab.h[at];
    const uint32_t* m = s->pool.h.data() + e.run + SH_HDR_WORDS;
    w.m.assign(m, m + s->pool.h[e.run]);
    w.ctr = s->ctr[e.key];
  } else {
    const auto oc = s->orphan_ctr.find(k);
    if (oc != s->orphan_ctr.end()) w.ctr = oc->second;
  }
  order.push_back(k);
  return work.emplace(k, std::move(w)).first->second;
}

// unsubscribe/3 and cleanup_down/1 for one key: the member out of the list, then
// maybe_delete_round_robin_count/1 (:489-494).
void sh_remove(emqxgm_share* s, ShWork& w, uint32_t group, uint32_t sub) {
  for (size_t i = 0; i < w.m.size(); ++i)
    if ((w.m[i] & ~SH_LOCAL_BIT) == sub) {
      w.m.erase(w.m.begin() + i);
      w.changed = true;
      break;
    }
  if (w.m.empty() && sh_strategy(s, group) == SH_RR_PER_GROUP) w.ctr = NONE;
}

// Applies the pending mutations to the mirror and sends what changed to the device.
int sh_commit(emqxgm_share* s) {
  // the bounds of every 32-bit index, before anything changes: a mutation touches at most one new
  // key, and the rewritten runs hold at most every member now and every pending one, twice
  const uint64_t add_words = (uint64_t)s->pend.size() * (SH_HDR_WORDS + 2);
  if (s->pool.h.size() + 2 * s->members + add_words > SH_INDEX_MAX || s->ko.h.size() + s->pend.size() > SH_INDEX_MAX ||
      s->kb.h.size() + s->ptb.size() > SH_INDEX_MAX)
    return -ENOMEM;
  if (hipSetDevice(s->device) != hipSuccess) return -EIO;
  SHCHK(hipStreamSynchronize(s->stream));
  std::unordered_map<std::string, ShWork> work;
  std::vector<std::string> order;
  bool strategies = false;
  for (const ShOp& e : s->pend) {
    const uint8_t* topic = e.tl ? s->ptb.data() + e.t0 : (const uint8_t*)"";
    if (e.op == SH_OP_STRATEGY) {
      if (e.group == NONE) s->def_strat = e.arg;
      else s->gstrat[e.group] = e.arg;
      strategies = true;
    } else if (e.op == SH_OP_SUB) {
      ShWork& w = sh_load(s, work, order, e.group, topic, e.tl);
      bool present = false;
      for (uint32_t m : w.m) present |= (m & ~SH_LOCAL_BIT) == e.sub;
      if (!present) {
        w.m.push_back(e.sub | (e.arg ? SH_LOCAL_BIT : 0u));
        w.changed = true;
      }
      // maybe_insert_round_robin_count/1 (:484-487): a duplicate subscribe resets it too
      if (sh_strategy(s, e.group) == SH_RR_PER_GROUP) w.ctr = 0;
    } else if (e.op == SH_OP_UNSUB) {
      sh_remove(s, sh_load(s, work, order, e.group, topic, e.tl), e.group, e.sub);
    } else {
      // cleanup_down/1 (:509-519) matches the whole bag on the pid; so does this
      for (uint32_t k = 0; k < s->krun.size(); ++k) {
        const uint32_t run = s->krun[k];
        if (run == NONE) continue;
        const uint32_t n_all = s->pool.h[run];
        for (uint32_t i = 0; i < n_all; ++i)
          if ((s->pool.h[run + SH_HDR_WORDS + i] & ~SH_LOCAL_BIT) == e.sub) {
            (void)sh_load(s, work, order, s->kg.h[k], s->kb.h.data() + s->ko.h[k], s->ko.h[k + 1] - s->ko.h[k]);
            break;
          }
      }
      for (const std::string& k : order) {
        ShWork& w = work[k];
        bool has = false;
        for (uint32_t m : w.m) has |= (m & ~SH_LOCAL_BIT) == e.sub;
        uint32_t group;
        memcpy(&group, k.data(), 4);
        if (has) sh_remove(s, w, group, e.sub);
      }
    }
  }
  uint64_t left = 0;  // keys the working set will add
  for (const std::string& k : order) {
    uint32_t group, free_at;
    memcpy(&group, k.data(), 4);
    if (!work[k].m.empty() && sh_find(s, group, (const uint8_t*)k.data() + 4, (uint32_t)k.size() - 4, &free_at) == NONE)
      ++left;
  }
  // the first load of an empty table sizes it once; that is no rebuild
  if (s->tab.live == 0 && s->tab.tomb == 0 && sh_slots_for(s, left) > s->tab.h.size())
    sh_table_reset(s->tab, sh_slots_for(s, left));
  ShTable& t = s->tab;
  for (const std::string& k : order) {
    ShWork& w = work[k];
    uint32_t group, free_at = NONE;
    memcpy(&group, k.data(), 4);
    const uint8_t* topic = (const uint8_t*)k.data() + 4;
    const uint32_t len = (uint32_t)k.size() - 4;
    uint32_t at = sh_find(s, group, topic, len, &free_at);
    if (at != NONE) {
      const uint32_t key = t.h[at].key;
      s->ctr[key] = w.ctr;
      if (!w.changed) continue;
      const uint32_t old_run = t.h[at].run, old_words = sh_words_at(s, old_run);
      s->garbage_words += old_words;
      s->live_words -= old_words;
      s->members -= s->pool.h[old_run];
      if (w.m.empty()) {
        t.h[at].tag = SH_DELETED;
        --t.live;
        ++t.tomb;
        s->krun[key] = NONE;
        s->ctr[key] = NONE;
        if (w.ctr != NONE) s->orphan_ctr[k] = w.ctr;
      } else {
        const uint32_t run = sh_append_run(s->pool.h, w.m.data(), (uint32_t)w.m.size(), sh_strategy(s, group));
        s->live_words += sh_words_at(s, run);
        s->members += w.m.size();
        t.h[at].run = run;
        s->krun[key] = run;
      }
      sh_touch(t, at);
      continue;
    }
    if (w.m.empty()) {  // still no such key: only its counter may have changed
      if (w.ctr == NONE) s->orphan_ctr.erase(k);
      else s->orphan_ctr[k] = w.ctr;
      continue;
    }
    --left;
    const bool takes_empty = free_at == NONE || t.h[free_at].tag == SH_EMPTY;
    if (free_at == NONE || (takes_empty && (t.live + t.tomb + 1) * 100 > t.h.size() * s->load_pct)) {
      sh_rebuild(s, left + 1);
      ++s->load_rebuilds;
      at = sh_find(s, group, topic, len, &free_at);
    }
    const uint32_t run = sh_append_run(s->pool.h, w.m.data(), (uint32_t)w.m.size(), sh_strategy(s, group));
    s->live_words += sh_words_at(s, run);
    s->members += w.m.size();
    const uint64_t tag = sh_key_tag(group, topic, len, s->tag_mask);
    if (t.h[free_at].tag == SH_DELETED) --t.tomb;
    t.h[free_at] = ShSlot{tag, run, (uint32_t)s->kg.h.size()};
    if (len) s->kb.h.insert(s->kb.h.end(), topic, topic + len);
    s->ko.h.push_back((uint32_t)s->kb.h.size());
    s->kg.h.push_back(group);
    s->krun.push_back(run);
    s->ctr.push_back(w.ctr);
    s->orphan_ctr.erase(k);
    ++t.live;
    sh_touch(t, free_at);
    const uint64_t mask = t.h.size() - 1;
    s->max_chain = std::max<uint64_t>(s->max_chain, ((free_at - sh_home(tag, mask)) & mask) + 1);
  }
  sh_clear_pending(s);
  // a strategy change rewrites the strategy word of that group's runs, in place
  if (strategies) {
    for (uint32_t k = 0; k < s->krun.size(); ++k) {
      const uint32_t run = s->krun[k];
      if (run == NONE) continue;
      const uint32_t want = sh_strategy(s, s->kg.h[k]);
      if (s->pool.h[run + 2] == want) continue;
      s->pool.h[run + 2] = want;
      if (s->pool_touched.size() <= SH_PATCH_MAX) s->pool_touched.push_back(run + 2);
    }
  }
  if (s->garbage_words && s->garbage_words * 100 > s->live_words * s->garbage_pct) {
    sh_rebuild(s, 0);
    ++s->garbage_rebuilds;
  }
  int rc = 0;
  if ((rc = sh_sync_pool(s)) || (rc = sh_sync(s, s->kb)) || (rc = sh_sync(s, s->ko)) || (rc = sh_sync(s, s->kg)) ||
      (rc = sh_sync_table(s, s->tab)))
    return rc;
  SHCHK(hipStreamSynchronize(s->stream));
  return 0;
}

}  // namespace

// Scratch slot of at least `bytes` (exactly `bytes` with GM_SHARE_EXACT_ALLOC).
int gm::share_grow(emqxgm_share* a, int slot, uint64_t bytes) {
  ShBuf& b = a->sc[slot];
#ifdef GM_SHARE_EXACT_ALLOC
  if (b.p && b.bytes == bytes) return 0;
  const uint64_t cap = bytes;
#else
  if (b.p && b.bytes >= bytes) return 0;
  const uint64_t cap = std::max<uint64_t>(bytes + bytes / 2, 4096);
#endif
  SHCHK(hipStreamSynchronize(a->stream));
  sh_free(b);
  if (!cap) return 0;
  SHCHK(hipMalloc(&b.p, cap));
  b.bytes = cap;
  return 0;
}

namespace {

int sh_put(emqxgm_share* a, int slot, const void* src, uint64_t bytes) {
  const int rc = share_grow(a, slot, bytes);
  if (rc) return rc;
  if (bytes) SHCHK(hipMemcpyAsync(a->sc[slot].p, src, bytes, hipMemcpyHostToDevice, a->stream));
  return 0;
}

// The round_robin_per_group steps of the np answers at o, in their order: every
// SH_COUNTER_PENDING answer takes the next value of its key's counter and becomes a pick.
}  // namespace

int gm::share_counter_steps(emqxgm_share* a, uint32_t* o, uint64_t np) {
  for (uint64_t i = 0; i < np; ++i) {
    uint32_t* r = o + (size_t)i * 4;
    if (r[1] != SH_COUNTER_PENDING) continue;
    const uint32_t key = r[3];
    if (key >= a->krun.size() || a->krun[key] == NONE) return -EIO;
    const uint32_t run = a->krun[key], count = a->pool.h[run];
    const uint32_t nth = sh_counter_step(a->ctr[key] == NONE ? 0u : a->ctr[key], count);
    a->ctr[key] = nth;
    r[0] = a->pool.h[run + SH_HDR_WORDS + nth - 1] & ~SH_LOCAL_BIT;
    r[1] = SH_PICKED;
    r[3] = count;
  }
  return 0;
}

// The committed tables as a kernel takes them.
void gm::share_tables(const emqxgm_share* a, ShareTables& A) {
  A.tab = a->tab.d.p;
  A.tmask = a->tab.h.size() - 1;
  A.pool = (const uint32_t*)a->pool.d.p;
  A.pool_words = a->pool.dev_n;
  A.kb = (const uint8_t*)a->kb.d.p;
  A.ko = (const uint32_t*)a->ko.d.p;
  A.kg = (const uint32_t*)a->kg.d.p;
  A.n_keys = (uint32_t)a->kg.dev_n;
  A.tag_mask = a->tag_mask;
}

namespace {

// One pass: requests [lo, hi) of the call; then the host's counter steps, in request order.
int sh_pass(emqxgm_share* a, const uint32_t* groups, const uint8_t* bytes, const uint32_t* offsets, const uint32_t* hc,
            const uint32_t* ht, const uint32_t* draw, const uint32_t* state, uint32_t lo, uint32_t hi, uint32_t* out) {
  const uint32_t np = hi - lo, o0 = offsets[lo];
  const uint64_t nbytes = offsets[hi] - o0;
  hipStream_t st = a->stream;
  SHCHK(hipStreamSynchronize(st));  // h_off is reused
  a->h_off.resize((size_t)np + 1);
  for (uint32_t i = 0; i <= np; ++i) a->h_off[i] = offsets[lo + i] - o0;
  int rc = 0;
  if ((rc = sh_put(a, SH_GR, groups + lo, (uint64_t)np * 4)) ||
      (rc = sh_put(a, SH_RB, nbytes ? bytes + o0 : nullptr, nbytes)) ||
      (rc = sh_put(a, SH_RO, a->h_off.data(), ((uint64_t)np + 1) * 4)) ||
      (rc = sh_put(a, SH_HC, hc + lo, (uint64_t)np * 4)) || (rc = sh_put(a, SH_HT, ht + lo, (uint64_t)np * 4)) ||
      (rc = sh_put(a, SH_DR, draw + lo, (uint64_t)np * 4)) || (rc = sh_put(a, SH_ST, state + lo, (uint64_t)np * 4)) ||
      (rc = share_grow(a, SH_OUT, (uint64_t)np * 16)) || (rc = share_grow(a, SH_CTL, SH_CTL_BYTES)))
    return rc;
  auto B = [&](int k) { return a->sc[k].p; };
  SHCHK(hipMemsetAsync(B(SH_CTL), 0, SH_CTL_BYTES, st));
  ShareArgs A;
  A.group = (const uint32_t*)B(SH_GR);
  A.rb = (const uint8_t*)B(SH_RB);
  A.ro = (const uint32_t*)B(SH_RO);
  A.hc = (const uint32_t*)B(SH_HC);
  A.ht = (const uint32_t*)B(SH_HT);
  A.draw = (const uint32_t*)B(SH_DR);
  A.state = (const uint32_t*)B(SH_ST);
  A.n = np;
  share_tables(a, A);
  A.out = (uint4*)B(SH_OUT);
  A.err = (uint32_t*)B(SH_CTL);
  A.stage = a->stage_lds;
  const bool timed = a->timing && a->ev[1];
  if (timed) SHCHK(hipEventRecord(a->ev[0], st));
  SHCHK(launch_share(A, st));
  if (timed) SHCHK(hipEventRecord(a->ev[1], st));
  uint32_t ctl[SH_CTL_BYTES / 4];
  uint32_t* o = out + (size_t)lo * 4;
  SHCHK(hipMemcpyAsync(o, A.out, (size_t)np * 16, hipMemcpyDeviceToHost, st));
  SHCHK(hipMemcpyAsync(ctl, B(SH_CTL), SH_CTL_BYTES, hipMemcpyDeviceToHost, st));
  SHCHK(hipStreamSynchronize(st));
  if (ctl[0] != 0) return -EIO;
  if (timed) {
    float ms = 0.f;
    SHCHK(hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
    a->kernel_ms += ms;
  }
  return share_counter_steps(a, o, np);
}

}  // namespace

extern "C" {

int emqxgm_share_create(int32_t device, uint32_t hash_bits, emqxgm_share_t** out) {
  if (!out) return -EINVAL;
  *out = nullptr;
  if (hash_bits > 16) return -EINVAL;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -ENODEV;
  emqxgm_share* s = new (std::nothrow) emqxgm_share();
  if (!s) return -ENOMEM;
  s->device = device;
  s->tag_mask = sh_tag_mask(hash_bits);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
    delete s;
    return -EIO;
  }
  sh_table_reset(s->tab, SH_MIN_SLOTS);
  s->ko.h.assign(1, 0u);
  const int rc = emqxgm_share_commit(s);  // lays out the empty table
  if (rc) {
    emqxgm_share_destroy(s);
    return rc;
  }
  *out = s;
  return 0;
}

void emqxgm_share_destroy(emqxgm_share_t* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  sh_free(s->tab.d);
  sh_free(s->pool.d);
  sh_free(s->kb.d);
  sh_free(s->ko.d);
  sh_free(s->kg.d);
  for (ShBuf& b : s->sc) sh_free(b);
  for (hipEvent_t e : s->ev)
    if (e) (void)hipEventDestroy(e);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

int emqxgm_share_subscribe(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len, uint32_t sub,
                           uint32_t local) {
  if (!s || (len && !topic) || group >= SH_HANDLE_MAX || sub >= SH_HANDLE_MAX || local > 1) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  const int st = sh_triple_state(s, group, topic, len, sub);
  if (st >= 0 && st != (int)local) return -EINVAL;
  sh_pend(s, SH_OP_SUB, group, topic, len, sub, local);
  return 0;
}

int emqxgm_share_unsubscribe(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len, uint32_t sub) {
  if (!s || (len && !topic) || group >= SH_HANDLE_MAX || sub >= SH_HANDLE_MAX) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  sh_pend(s, SH_OP_UNSUB, group, topic, len, sub, 0);
  return 0;
}

int emqxgm_share_subscriber_down(emqxgm_share_t* s, uint32_t sub) {
  if (!s || sub >= SH_HANDLE_MAX) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  sh_pend(s, SH_OP_DOWN, 0, nullptr, 0, sub, 0);
  return 0;
}

int emqxgm_share_set_strategy(emqxgm_share_t* s, uint32_t group, uint32_t strategy) {
  if (!s || (group >= SH_HANDLE_MAX && group != NONE) || strategy >= SH_STRATEGIES) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  sh_pend(s, SH_OP_STRATEGY, group, nullptr, 0, 0, strategy);
  return 0;
}

int emqxgm_share_commit(emqxgm_share_t* s) {
  if (!s) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->broken) return -EIO;
  const int rc = sh_commit(s);
  // the mirror is changed before the uploads: after a failed one no call may use the handle
  if (rc && rc != -ENOMEM) s->broken = true;
  return rc;
}

int emqxgm_share_pick(emqxgm_share_t* s, uint32_t n, const uint32_t* groups, const uint8_t* key_bytes,
                      const uint32_t* key_offsets, const uint32_t* hc, const uint32_t* ht, const uint32_t* draw,
                      const uint32_t* state, uint32_t* out) {
  if (!s) return -EINVAL;
  if (n == 0) return 0;
  if (!groups || !key_offsets || !hc || !ht || !draw || !state || !out) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (key_offsets[i + 1] < key_offsets[i] || groups[i] >= SH_HANDLE_MAX) return -EINVAL;
  if (key_offsets[n] != key_offsets[0] && !key_bytes) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->broken) return -EIO;
  if (hipSetDevice(s->device) != hipSuccess) return -EIO;
  const uint64_t cap = std::min<uint64_t>(s->pass_names, SH_PASS_MAX);
  for (uint64_t lo = 0; lo < n; lo += cap) {
    const uint32_t hi = (uint32_t)std::min<uint64_t>(n, lo + cap);
    const int rc = sh_pass(s, groups, key_bytes, key_offsets, hc, ht, draw, state, (uint32_t)lo, hi, out);
    if (rc) return rc;
  }
  return 0;
}

int emqxgm_share_members(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len, uint32_t* out,
                         uint32_t cap, uint32_t* n_out) {
  if (!s || !n_out || (len && !topic) || (cap && !out)) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->broken) return -EIO;
  uint32_t free_at;
  const uint32_t at = sh_find(s, group, topic, len, &free_at);
  *n_out = 0;
  if (at == NONE) return 0;
  const uint32_t run = s->tab.h[at].run, n_all = s->pool.h[run];
  *n_out = n_all;
  for (uint32_t i = 0; i < n_all && i < cap; ++i) out[i] = s->pool.h[run + SH_HDR_WORDS + i];
  return 0;
}

int emqxgm_share_counter(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len, uint32_t* out) {
  if (!s || !out || (len && !topic)) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->broken) return -EIO;
  uint32_t free_at, c = NONE;
  const uint32_t at = sh_find(s, group, topic, len, &free_at);
  if (at != NONE) {
    c = s->ctr[s->tab.h[at].key];
  } else {
    const auto it = s->orphan_ctr.find(sh_key(group, topic, len));
    if (it != s->orphan_ctr.end()) c = it->second;
  }
  *out = c;
  return 0;
}

int emqxgm_share_tune(emqxgm_share_t* s, const char* key, int64_t value) {
  if (!s || !key) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  if (strcmp(key, "pass_names") == 0) {
    if (value < 1) return -EINVAL;
    s->pass_names = (uint64_t)value;
    return 0;
  }
  if (strcmp(key, "timing") == 0) {
    if (value && !s->ev[1]) {
      if (hipSetDevice(s->device) != hipSuccess) return -EIO;
      for (hipEvent_t& e : s->ev)
        if (!e) SHCHK(hipEventCreate(&e));
    }
    s->timing = value != 0;
    s->kernel_ms = 0;
    return 0;
  }
  if (strcmp(key, "stage_lds") == 0) {
    s->stage_lds = value != 0;
    return 0;
  }
  if (strcmp(key, "kernel_us") == 0) {
    const double us = s->kernel_ms * 1000.0;
    return us > 2147483647.0 ? 2147483647 : (int)us;
  }
  if (strcmp(key, "rebuild_load_pct") == 0) {
    if (value < 1 || value > 50) return -EINVAL;
    s->load_pct = (uint32_t)value;
    return 0;
  }
  if (strcmp(key, "rebuild_garbage_pct") == 0) {
    if (value < 1 || value > 1000000) return -EINVAL;
    s->garbage_pct = (uint32_t)value;
    return 0;
  }
  return -EINVAL;
}

int emqxgm_share_stats(emqxgm_share_t* s, uint64_t out[12]) {
  if (!s || !out) return -EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  uint64_t counters = s->orphan_ctr.size();
  for (uint32_t c : s->ctr) counters += c != NONE;
  out[0] = s->tab.live;
  out[1] = s->tab.h.size();
  out[2] = s->tab.tomb;
  out[3] = s->max_chain;
  out[4] = s->members;
  out[5] = s->live_words;
  out[6] = s->garbage_words;
  out[7] = s->load_rebuilds;
  out[8] = s->garbage_rebuilds;
  out[9] = s->growths;
  out[10] = counters;
  out[11] = s->pend.size();
  return 0;
}

}  // extern "C"
