// gm_acldb.cpp -- host side of the built-in authorization database resident on the device
// (k_acldb, gm_acldb.inc): the record compiler, the pending mutations, the incremental commit, the
// full rebuild, the pass driver and the emqxgm_acldb_* C-ABI of include/emqx_gpumatch.h.  A handle
// of its own, beside the engine, the retainer, the rule set and the ACL list.
//
// Reference: emqx_authz_mnesia (apps/emqx_authz/src/emqx_authz_mnesia.erl): authorize/4 (:98-120),
// store_rules/2, delete_rules/1, purge_rules/0 and record_count/0 (:132-173), do_authorize/4
// (:222-229) over emqx_authz_rule:compile/1 and match/4.
//
// The host keeps a mirror of every device array (gm_acldb_match.h: two key tables, the record
// pool, filter bytes and offsets, key bytes and offsets, the `all` stream).  A commit applies the
// pending mutations to the mirror: a new or replaced run is appended to the pools with its filter
// and key bytes, its slot is patched, the run it replaces is counted as garbage, a delete leaves
// ADB_DELETED in the slot.  Then only what changed goes to the device: the appended tails of the
// pools (a pool grows with slack; growing is a new allocation and a device-to-device copy) and
// the touched slots as 16-byte copies on the handle's stream.  A full rebuild compacts the pools
// and rehashes both tables into a fresh mirror that is uploaded whole; it runs when an insert
// would take a table's used slots (deleted ones included) past "rebuild_load_pct" of its slots,
// or when the garbage words pass "rebuild_garbage_pct" percent of the live ones (the words of a
// replaced `all` stream count as garbage too: its filter bytes stay in the pools until then).  The
// mirror changes before the uploads: a commit that fails on the device marks the handle broken, and
// every later commit and match returns -EIO instead of pairing the mirror's sizes with old arrays.
// Sizing the
// tables of an empty database for its first load is not a rebuild.  A match holds the handle's
// mutex for its passes, so a commit never runs beside a kernel.
//
// With -DGM_ACLDB_EXACT_ALLOC every device array is exactly the bytes in use (no floor, no growth
// slack): tests/host_harness/acldb_dev_main.cpp runs this file and the kernel's phases on the CPU
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
#include "gm_acldb_match.h"
#include "gm_common.h"
#include "gm_kernels.h"

using namespace gm;

namespace {

struct AdbBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// A pool: its host mirror, its device array and how many elements of the mirror the device has.
template <class T>
struct AdbPool {
  std::vector<T> h;
  AdbBuf d;
  size_t dev_n = 0;
};

struct AdbTable {
  std::vector<AdbSlot> h;
  AdbBuf d;
  uint64_t live = 0, tomb = 0;
  std::vector<uint32_t> touched;  // slots changed since the last upload
  bool whole = true;              // the device has no copy of this table's size
};

// A pending store or delete: its key in pkb, its compiled rules in pw, its filters in pfb / pfl.
struct AdbPend {
  uint32_t kind = 0;
  bool del = false, dead = false;  // dead: a later mutation of the same key replaced it
  size_t key0 = 0, w0 = 0, fb0 = 0, fl0 = 0;
  uint32_t klen = 0, nw = 0, n_rules = 0;
};

// scratch: the pass's names, clients, actions and answers; the call's client table; the control
// words
enum { ADB_NB, ADB_NO, ADB_CL, ADB_AC, ADB_OP, ADB_OS, ADB_OQ, ADB_CB, ADB_CO, ADB_UB, ADB_UO, ADB_CF, ADB_CTL,
       ADB_SLOTS };
constexpr size_t ADB_CTL_BYTES = 48;  // 5 x u64 counters, then the error word (and a pad word)
constexpr uint64_t ADB_PASS_MAX = 1ull << 31;
constexpr uint64_t ADB_INDEX_MAX = 0xFFFFFFF0ull;  // pool words, filters, keys, filter and key bytes
constexpr size_t ADB_PATCH_MAX = 256;              // touched slots beyond this: the table in one copy

}  // namespace

struct emqxgm_acldb {
  std::mutex mu;
  int32_t device = 0;
  hipStream_t stream = nullptr;
  uint64_t test_mask = 0;
  // committed
  AdbTable tab[2];
  AdbPool<uint64_t> pool;
  AdbPool<uint8_t> fb, kb;
  AdbPool<uint32_t> fo, ko;
  std::vector<uint64_t> all_h;
  AdbBuf all_d;
  bool all_present = false, all_dirty = true;
  uint32_t all_fbase = 0, all_rules = 0;
  uint64_t live_words = 0, garbage_words = 0, rebuilds = 0, growths = 0, max_chain = 0;
  // pending
  bool broken = false;  // a commit failed half way: the device arrays and the mirror disagree
  bool purge = false;
  std::vector<AdbPend> pend;
  std::vector<uint8_t> pkb, pfb;
  std::vector<uint64_t> pw;
  std::vector<uint32_t> pfl;
  std::unordered_map<std::string, uint32_t> pidx[3];
  // tuning, counters, scratch
  uint64_t pass_names = 1ull << 20;
  uint32_t load_pct = 50, garbage_pct = 100;
  bool counters = false;
  uint64_t ctr[5] = {0, 0, 0, 0, 0};
  bool timing = false;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double kernel_ms = 0;
  AdbBuf sc[ADB_SLOTS];
  std::vector<uint32_t> h_off;
};

namespace {

#define ADBCHK(expr)                       \
  do {                                     \
    if ((expr) != hipSuccess) return -EIO; \
  } while (0)

void adb_free(AdbBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b = AdbBuf();
}

// The device array of `bytes` bytes of src, exactly (a table, the `all` stream).
int adb_upload(const void* src, size_t bytes, AdbBuf& b) {
  adb_free(b);
  if (!bytes) return 0;
  ADBCHK(hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  ADBCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

// The device array of a pool follows its mirror: grown when the mirror no longer fits (a new
// allocation and a device-to-device copy of what the device has), then the mirror's new tail.
template <class T>
int adb_sync(emqxgm_acldb* db, AdbPool<T>& p) {
  const size_t need = p.h.size() * sizeof(T);
#ifdef GM_ACLDB_EXACT_ALLOC
  const bool grow = need != p.d.bytes;
  const size_t cap = need;
#else
  const bool grow = need > p.d.bytes;
  const size_t cap = std::max<size_t>(need + need / 2, 256);
#endif
  if (grow) {
    AdbBuf nb;
    if (cap) {
      ADBCHK(hipMalloc(&nb.p, cap));
      nb.bytes = cap;
    }
    if (p.dev_n) {
      if (hipMemcpy(nb.p, p.d.p, p.dev_n * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) {
        adb_free(nb);
        return -EIO;
      }
      ++db->growths;
    }
    adb_free(p.d);
    p.d = nb;
  }
  if (p.h.size() > p.dev_n)
    ADBCHK(hipMemcpy((T*)p.d.p + p.dev_n, p.h.data() + p.dev_n, (p.h.size() - p.dev_n) * sizeof(T),
                     hipMemcpyHostToDevice));
  p.dev_n = p.h.size();
  return 0;
}

template <class T>
void adb_drop(AdbPool<T>& p) {
  adb_free(p.d);
  p.dev_n = 0;
}

int adb_sync_table(emqxgm_acldb* db, AdbTable& t) {
  if (t.whole) {
    const int rc = adb_upload(t.h.data(), t.h.size() * sizeof(AdbSlot), t.d);
    if (rc) return rc;
  } else if (t.touched.size() > ADB_PATCH_MAX) {
    ADBCHK(hipMemcpy(t.d.p, t.h.data(), t.h.size() * sizeof(AdbSlot), hipMemcpyHostToDevice));
  } else {
    for (uint32_t i : t.touched)
      ADBCHK(hipMemcpyAsync((AdbSlot*)t.d.p + i, &t.h[i], sizeof(AdbSlot), hipMemcpyHostToDevice, db->stream));
  }
  t.whole = false;
  t.touched.clear();
  return 0;
}

uint64_t adb_pow2(uint64_t v) {
  uint64_t s = ADB_MIN_SLOTS;
  while (s < v) s <<= 1;
  return s;
}

// Slots for `keys` keys at the handle's load limit.
uint64_t adb_slots_for(const emqxgm_acldb* db, uint64_t keys) {
  return adb_pow2((keys * 100 + db->load_pct - 1) / db->load_pct);
}

void adb_table_reset(AdbTable& t, uint64_t slots) {
  t.h.assign(slots, AdbSlot{ADB_EMPTY, 0, 0});
  t.live = t.tomb = 0;
  t.touched.clear();
  t.whole = true;
}

// The slot of (kind, key), or NONE; *free_at = where an insert of the key goes (the first deleted
// slot of its chain, else the empty slot that ends it), *chain = slots looked at.
uint32_t adb_find(const emqxgm_acldb* db, uint32_t kind, uint64_t tok, const uint8_t* key, uint32_t klen,
                  uint32_t* free_at, uint32_t* chain) {
  const AdbTable& t = db->tab[kind];
  const uint64_t mask = t.h.size() - 1;
  uint64_t i = adb_home(tok, mask);
  *free_at = NONE;
  *chain = 0;
  for (uint64_t step = 0; step <= mask; ++step, i = (i + 1) & mask) {
    const AdbSlot& s = t.h[i];
    ++*chain;
    if (s.tok == ADB_EMPTY) {
      if (*free_at == NONE) *free_at = (uint32_t)i;
      return NONE;
    }
    if (s.tok == ADB_DELETED) {
      if (*free_at == NONE) *free_at = (uint32_t)i;
      continue;
    }
    if (s.tok != tok) continue;
    const uint32_t k0 = db->ko.h[s.key], kl = db->ko.h[s.key + 1] - k0;
    if (kl == klen && (klen == 0 || memcmp(db->kb.h.data() + k0, key, klen) == 0)) return (uint32_t)i;
  }
  return NONE;
}

void adb_touch(AdbTable& t, uint32_t i) {
  if (!t.whole && t.touched.size() <= ADB_PATCH_MAX) t.touched.push_back(i);
}

// Compacts the pools and rehashes both tables (sized for extra[kind] more keys) into a fresh
// mirror; everything is uploaded whole by the commit that called it.
void adb_rebuild(emqxgm_acldb* db, const uint64_t extra[2]) {
  std::vector<uint64_t> npool;
  std::vector<uint8_t> nfb, nkb;
  std::vector<uint32_t> nfo{0}, nko{0};
  npool.reserve((size_t)db->live_words);
  db->max_chain = 0;
  for (uint32_t kind = 0; kind < 2; ++kind) {
    AdbTable& t = db->tab[kind];
    std::vector<AdbSlot> nh(adb_slots_for(db, t.live + extra[kind]), AdbSlot{ADB_EMPTY, 0, 0});
    const uint64_t mask = nh.size() - 1;
    for (const AdbSlot& s : t.h) {
      if (s.tok == ADB_EMPTY || s.tok == ADB_DELETED) continue;
      const uint64_t hdr = db->pool.h[s.run];
      const uint32_t len = adb_run_words(hdr), fbase = adb_run_fbase(hdr);
      uint32_t rules = 0;
      (void)adb_walk_run(db->pool.h.data(), db->pool.h.size(), s.run, (uint32_t)(db->fo.h.size() - 1),
                         [&](uint32_t, uint64_t, const uint64_t*, uint32_t) {
                           ++rules;
                           return false;
                         });
      AdbSlot ns{s.tok, (uint32_t)npool.size(), (uint32_t)(nko.size() - 1)};
      npool.push_back(adb_run_header(len, (uint32_t)(nfo.size() - 1)));
      npool.insert(npool.end(), db->pool.h.begin() + s.run + 1, db->pool.h.begin() + s.run + len);
      for (uint32_t k = 0; k < rules; ++k) {
        nfb.insert(nfb.end(), db->fb.h.begin() + db->fo.h[fbase + k], db->fb.h.begin() + db->fo.h[fbase + k + 1]);
        nfo.push_back((uint32_t)nfb.size());
      }
      nkb.insert(nkb.end(), db->kb.h.begin() + db->ko.h[s.key], db->kb.h.begin() + db->ko.h[s.key + 1]);
      nko.push_back((uint32_t)nkb.size());
      uint64_t i = adb_home(s.tok, mask), chain = 1;
      for (; nh[i].tok != ADB_EMPTY; i = (i + 1) & mask) ++chain;
      nh[i] = ns;
      db->max_chain = std::max(db->max_chain, chain);
    }
    t.h.swap(nh);
    t.tomb = 0;
    t.touched.clear();
    t.whole = true;
  }
  const uint32_t afb = (uint32_t)(nfo.size() - 1);
  for (uint32_t k = 0; k < db->all_rules; ++k) {
    nfb.insert(nfb.end(), db->fb.h.begin() + db->fo.h[db->all_fbase + k],
               db->fb.h.begin() + db->fo.h[db->all_fbase + k + 1]);
    nfo.push_back((uint32_t)nfb.size());
  }
  db->all_fbase = afb;
  db->pool.h.swap(npool);
  db->fb.h.swap(nfb);
  db->fo.h.swap(nfo);
  db->kb.h.swap(nkb);
  db->ko.h.swap(nko);
  adb_drop(db->pool);
  adb_drop(db->fb);
  adb_drop(db->fo);
  adb_drop(db->kb);
  adb_drop(db->ko);
  db->live_words = db->pool.h.size() + db->all_h.size();
  db->garbage_words = 0;
}

void adb_clear_pending(emqxgm_acldb* db) {
  db->pend.clear();
  db->pkb.clear();
  db->pfb.clear();
  db->pw.clear();
  db->pfl.clear();
  for (auto& m : db->pidx) m.clear();
}

bool adb_rules_ok(const uint32_t* perm, const uint32_t* action, const uint8_t* fbytes, const uint32_t* foff,
                  uint32_t lo, uint32_t hi) {
  if (hi < lo || hi - lo > ADB_MAX_RULES) return false;
  if (hi > lo && (!perm || !action || !foff)) return false;
  for (uint32_t k = lo; k < hi; ++k) {
    if (perm[k] > ACL_ALLOW || action[k] < ACL_PUBLISH || action[k] > ACL_ALL) return false;
    if (foff[k + 1] < foff[k] || (foff[k + 1] > foff[k] && !fbytes)) return false;
  }
  return true;
}

// One validated mutation into the pending lists (the handle's mutex is held).
void adb_pend(emqxgm_acldb* db, uint32_t kind, bool del, const uint8_t* key, uint32_t klen, const uint32_t* perm,
              const uint32_t* action, const uint8_t* fbytes, const uint32_t* foff, uint32_t lo, uint32_t hi) {
  if (kind == ADB_ALL) klen = 0;
  AdbPend e;
  e.kind = kind;
  e.del = del;
  e.key0 = db->pkb.size();
  e.klen = klen;
  if (klen) db->pkb.insert(db->pkb.end(), key, key + klen);
  e.w0 = db->pw.size();
  e.fb0 = db->pfb.size();
  e.fl0 = db->pfl.size();
  for (uint32_t k = lo; k < hi; ++k) {
    uint64_t rec[ADB_RULE_WORDS_MAX];
    const uint32_t len = foff[k + 1] - foff[k];
    const uint8_t* f = len ? fbytes + foff[k] : (const uint8_t*)"";
    uint32_t skip = 0;
    const uint32_t nw = adb_compile_rule(perm[k], action[k], f, len, k - lo, db->test_mask, rec, &skip);
    db->pw.insert(db->pw.end(), rec, rec + nw);
    db->pfb.insert(db->pfb.end(), f + skip, f + len);
    db->pfl.push_back(len - skip);
  }
  e.nw = (uint32_t)(db->pw.size() - e.w0);
  e.n_rules = hi - lo;
  const std::string ks(klen ? (const char*)key : "", klen);
  auto it = db->pidx[kind].find(ks);
  if (it != db->pidx[kind].end()) {
    db->pend[it->second].dead = true;
    it->second = (uint32_t)db->pend.size();
  } else {
    db->pidx[kind].emplace(ks, (uint32_t)db->pend.size());
  }
  db->pend.push_back(e);
}

// The pending `all` record into the tiled stream.
void adb_apply_all(emqxgm_acldb* db, const AdbPend& e) {
  // the stream it replaces, and with it its filter bytes and offsets, is garbage until a rebuild
  db->garbage_words += db->all_h.size();
  db->live_words -= db->all_h.size();
  db->all_h.clear();
  db->all_dirty = true;
  db->all_present = !e.del;
  db->all_rules = e.n_rules;
  db->all_fbase = (uint32_t)(db->fo.h.size() - 1);
  const uint64_t* w = db->pw.data() + e.w0;
  for (uint32_t p = 0; p < e.nw;) {
    rs_append(db->all_h, w + p, ACL_RULE_WORDS);
    p += ACL_RULE_WORDS;
    const uint32_t step = acl_step(w[p]);
    rs_append(db->all_h, w + p, step);
    p += step;
  }
  db->live_words += db->all_h.size();
}

void adb_append_filters(emqxgm_acldb* db, const AdbPend& e) {
  size_t at = e.fb0;
  for (uint32_t k = 0; k < e.n_rules; ++k) {
    const uint32_t fl = db->pfl[e.fl0 + k];
    db->fb.h.insert(db->fb.h.end(), db->pfb.begin() + at, db->pfb.begin() + at + fl);
    db->fo.h.push_back((uint32_t)db->fb.h.size());
    at += fl;
  }
}

// Applies the pending mutations to the mirror and sends what changed to the device.
int adb_commit(emqxgm_acldb* db) {
  // the bounds of every 32-bit index, before anything changes
  if (db->pool.h.size() + db->pw.size() + db->pend.size() > ADB_INDEX_MAX ||
      db->fo.h.size() + db->pfl.size() > ADB_INDEX_MAX || db->fb.h.size() + db->pfb.size() > ADB_INDEX_MAX ||
      db->ko.h.size() + db->pend.size() > ADB_INDEX_MAX || db->kb.h.size() + db->pkb.size() > ADB_INDEX_MAX)
    return -ENOMEM;
  if (hipSetDevice(db->device) != hipSuccess) return -EIO;
  ADBCHK(hipStreamSynchronize(db->stream));
  if (db->purge) {
    for (AdbTable& t : db->tab) adb_table_reset(t, ADB_MIN_SLOTS);
    db->pool.h.clear();
    db->fb.h.clear();
    db->kb.h.clear();
    db->fo.h.assign(1, 0u);
    db->ko.h.assign(1, 0u);
    adb_drop(db->pool);
    adb_drop(db->fb);
    adb_drop(db->fo);
    adb_drop(db->kb);
    adb_drop(db->ko);
    db->all_h.clear();
    db->all_present = false;
    db->all_dirty = true;
    db->all_rules = db->all_fbase = 0;
    db->live_words = db->garbage_words = db->max_chain = 0;
    db->purge = false;
  }
  uint64_t left[2] = {0, 0};  // pending stores per kind not yet applied
  for (const AdbPend& e : db->pend)
    if (!e.dead && !e.del && e.kind < ADB_ALL) ++left[e.kind];
  // the first load of an empty database sizes its tables once; that is no rebuild
  for (uint32_t kind = 0; kind < 2; ++kind) {
    AdbTable& t = db->tab[kind];
    if (t.live == 0 && t.tomb == 0 && adb_slots_for(db, left[kind]) > t.h.size())
      adb_table_reset(t, adb_slots_for(db, left[kind]));
  }
  for (const AdbPend& e : db->pend) {
    if (e.dead) continue;
    if (e.kind == ADB_ALL) {
      adb_apply_all(db, e);
      if (!e.del) adb_append_filters(db, e);
      continue;
    }
    const uint8_t* key = db->pkb.data() + e.key0;
    const uint64_t tok = acl_value_token(e.klen ? key : (const uint8_t*)"", e.klen, db->test_mask);
    uint32_t free_at = NONE, chain = 0;
    uint32_t at = adb_find(db, e.kind, tok, key, e.klen, &free_at, &chain);
    if (e.del) {
      if (at != NONE) {
        AdbTable& t = db->tab[e.kind];
        const uint64_t old = adb_run_words(db->pool.h[t.h[at].run]);
        db->garbage_words += old;
        db->live_words -= old;
        t.h[at].tok = ADB_DELETED;
        --t.live;
        ++t.tomb;
        adb_touch(t, at);
      }
      continue;
    }
    --left[e.kind];
    if (at == NONE) {
      AdbTable& t0 = db->tab[e.kind];
      const bool takes_empty = free_at == NONE || t0.h[free_at].tok == ADB_EMPTY;
      if (free_at == NONE || (takes_empty && (t0.live + t0.tomb + 1) * 100 > t0.h.size() * db->load_pct)) {
        uint64_t extra[2] = {left[0], left[1]};
        ++extra[e.kind];
        adb_rebuild(db, extra);
        ++db->rebuilds;
        at = adb_find(db, e.kind, tok, key, e.klen, &free_at, &chain);
      }
    }
    AdbTable& t = db->tab[e.kind];
    const uint32_t run = (uint32_t)db->pool.h.size();
    db->pool.h.push_back(adb_run_header(1 + e.nw, (uint32_t)(db->fo.h.size() - 1)));
    db->pool.h.insert(db->pool.h.end(), db->pw.begin() + e.w0, db->pw.begin() + e.w0 + e.nw);
    adb_append_filters(db, e);
    db->live_words += 1 + e.nw;
    if (at != NONE) {
      const uint64_t old = adb_run_words(db->pool.h[t.h[at].run]);
      db->garbage_words += old;
      db->live_words -= old;
      t.h[at].run = run;
      adb_touch(t, at);
    } else {
      if (t.h[free_at].tok == ADB_DELETED) --t.tomb;
      t.h[free_at] = AdbSlot{tok, run, (uint32_t)(db->ko.h.size() - 1)};
      if (e.klen) db->kb.h.insert(db->kb.h.end(), key, key + e.klen);
      db->ko.h.push_back((uint32_t)db->kb.h.size());
      ++t.live;
      adb_touch(t, free_at);
      // the key's own chain: its home to the slot it took
      const uint64_t mask = t.h.size() - 1;
      db->max_chain = std::max<uint64_t>(db->max_chain, ((free_at - adb_home(tok, mask)) & mask) + 1);
    }
  }
  adb_clear_pending(db);
  if (db->garbage_words && db->garbage_words * 100 > db->live_words * db->garbage_pct) {
    const uint64_t none[2] = {0, 0};
    adb_rebuild(db, none);
    ++db->rebuilds;
  }
  int rc = 0;
  if ((rc = adb_sync(db, db->pool)) || (rc = adb_sync(db, db->fb)) || (rc = adb_sync(db, db->fo)) ||
      (rc = adb_sync(db, db->kb)) || (rc = adb_sync(db, db->ko)) || (rc = adb_sync_table(db, db->tab[0])) ||
      (rc = adb_sync_table(db, db->tab[1])))
    return rc;
  if (db->all_dirty) {
    if ((rc = adb_upload(db->all_h.data(), db->all_h.size() * 8, db->all_d))) return rc;
    db->all_dirty = false;
  }
  ADBCHK(hipStreamSynchronize(db->stream));
  return 0;
}

// Scratch slot of at least `bytes` (exactly `bytes` with GM_ACLDB_EXACT_ALLOC).
int adb_grow(emqxgm_acldb* a, int slot, uint64_t bytes) {
  AdbBuf& b = a->sc[slot];
#ifdef GM_ACLDB_EXACT_ALLOC
  if (b.p && b.bytes == bytes) return 0;
  const uint64_t cap = bytes;
#else
  if (b.p && b.bytes >= bytes) return 0;
  const uint64_t cap = std::max<uint64_t>(bytes + bytes / 2, 4096);
#endif
  ADBCHK(hipStreamSynchronize(a->stream));
  adb_free(b);
  ADBCHK(hipMalloc(&b.p, cap));
  b.bytes = cap;
  return 0;
}

int adb_put(emqxgm_acldb* a, int slot, const void* src, uint64_t bytes) {
  const int rc = adb_grow(a, slot, bytes);
  if (rc) return rc;
  if (bytes) ADBCHK(hipMemcpyAsync(a->sc[slot].p, src, bytes, hipMemcpyHostToDevice, a->stream));
  return 0;
}

// offsets [lo .. hi] rebased to 0 into h_off, then into `slot` (h_off is reused: the stream is
// drained first).
int adb_put_offsets(emqxgm_acldb* a, int slot, const uint32_t* offsets, uint32_t lo, uint32_t hi) {
  ADBCHK(hipStreamSynchronize(a->stream));
  const uint32_t m = hi - lo + 1, o0 = offsets[lo];
  a->h_off.resize(m);
  for (uint32_t i = 0; i < m; ++i) a->h_off[i] = offsets[lo + i] - o0;
  return adb_put(a, slot, a->h_off.data(), (uint64_t)m * 4);
}

int adb_put_clients(emqxgm_acldb* a, const uint8_t* cb, const uint32_t* co, const uint8_t* ub, const uint32_t* uo,
                    const uint32_t* cf, uint32_t n) {
  static const uint32_t zero = 0;
  int rc = 0;
  const uint32_t cbytes = n ? co[n] - co[0] : 0, ubytes = n ? uo[n] - uo[0] : 0;
  if ((rc = adb_put(a, ADB_CB, cbytes ? cb + co[0] : nullptr, cbytes)) ||
      (rc = adb_put(a, ADB_UB, ubytes ? ub + uo[0] : nullptr, ubytes)) || (rc = adb_put(a, ADB_CF, cf, (uint64_t)n * 4)))
    return rc;
  if (n == 0) {
    if ((rc = adb_put(a, ADB_CO, &zero, 4)) || (rc = adb_put(a, ADB_UO, &zero, 4))) return rc;
  } else if ((rc = adb_put_offsets(a, ADB_CO, co, 0, n)) || (rc = adb_put_offsets(a, ADB_UO, uo, 0, n))) {
    return rc;
  }
  ADBCHK(hipStreamSynchronize(a->stream));
  return 0;
}

// One pass: requests [lo, hi) of the call.
int adb_pass(emqxgm_acldb* a, const uint8_t* bytes, const uint32_t* offsets, const uint32_t* client,
             const uint32_t* action, uint32_t n_clients, uint32_t lo, uint32_t hi, uint32_t* out_perm,
             uint32_t* out_src, uint32_t* out_pos) {
  const uint32_t np = hi - lo;
  const uint32_t o0 = offsets[lo];
  const uint64_t nbytes = offsets[hi] - o0;
  hipStream_t s = a->stream;
  int rc = 0;
  if ((rc = adb_put(a, ADB_NB, nbytes ? bytes + o0 : nullptr, nbytes)) ||
      (rc = adb_put_offsets(a, ADB_NO, offsets, lo, hi)) || (rc = adb_put(a, ADB_CL, client + lo, (uint64_t)np * 4)) ||
      (rc = adb_put(a, ADB_AC, action + lo, (uint64_t)np * 4)) || (rc = adb_grow(a, ADB_OP, (uint64_t)np * 4)) ||
      (rc = adb_grow(a, ADB_OS, (uint64_t)np * 4)) || (rc = adb_grow(a, ADB_OQ, (uint64_t)np * 4)) ||
      (rc = adb_grow(a, ADB_CTL, ADB_CTL_BYTES)))
    return rc;
  auto B = [&](int k) { return a->sc[k].p; };
  ADBCHK(hipMemsetAsync(B(ADB_CTL), 0, ADB_CTL_BYTES, s));
  AclDbArgs A;
  A.nb = (const uint8_t*)B(ADB_NB);
  A.no = (const uint32_t*)B(ADB_NO);
  A.client = (const uint32_t*)B(ADB_CL);
  A.action = (const uint32_t*)B(ADB_AC);
  A.n = np;
  A.cb = (const uint8_t*)B(ADB_CB);
  A.co = (const uint32_t*)B(ADB_CO);
  A.ub = (const uint8_t*)B(ADB_UB);
  A.uo = (const uint32_t*)B(ADB_UO);
  A.cf = (const uint32_t*)B(ADB_CF);
  A.n_clients = n_clients;
  for (uint32_t k = 0; k < 2; ++k) {
    A.tab[k] = a->tab[k].d.p;
    A.tmask[k] = a->tab[k].h.size() - 1;
  }
  A.pool = (const uint64_t*)a->pool.d.p;
  A.pool_words = a->pool.dev_n;
  A.all = (const uint64_t*)a->all_d.p;
  A.all_words = (uint32_t)a->all_h.size();
  A.all_fbase = a->all_fbase;
  A.all_rules = a->all_rules;
  A.fb = (const uint8_t*)a->fb.d.p;
  A.fo = (const uint32_t*)a->fo.d.p;
  A.n_filters = (uint32_t)(a->fo.dev_n - 1);
  A.kb = (const uint8_t*)a->kb.d.p;
  A.ko = (const uint32_t*)a->ko.d.p;
  A.n_keys = (uint32_t)(a->ko.dev_n - 1);
  A.test_mask = a->test_mask;
  A.out_perm = (uint32_t*)B(ADB_OP);
  A.out_src = (uint32_t*)B(ADB_OS);
  A.out_pos = (uint32_t*)B(ADB_OQ);
  A.err = (uint32_t*)((uint8_t*)B(ADB_CTL) + 40);
  A.ctr = a->counters ? (unsigned long long*)B(ADB_CTL) : nullptr;
  const bool timed = a->timing && a->ev[1];
  if (timed) ADBCHK(hipEventRecord(a->ev[0], s));
  ADBCHK(launch_acldb(A, s));
  if (timed) ADBCHK(hipEventRecord(a->ev[1], s));
  uint64_t ctl[ADB_CTL_BYTES / 8];
  ADBCHK(hipMemcpyAsync(out_perm + lo, A.out_perm, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  ADBCHK(hipMemcpyAsync(out_src + lo, A.out_src, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  ADBCHK(hipMemcpyAsync(out_pos + lo, A.out_pos, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  ADBCHK(hipMemcpyAsync(ctl, B(ADB_CTL), ADB_CTL_BYTES, hipMemcpyDeviceToHost, s));
  ADBCHK(hipStreamSynchronize(s));
  if ((uint32_t)ctl[5] != 0) return -EIO;
  if (timed) {
    float ms = 0.f;
    ADBCHK(hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
    a->kernel_ms += ms;
  }
  for (int c = 0; c < 5; ++c) a->ctr[c] += ctl[c];
  return 0;
}

bool adb_offsets_ok(const uint32_t* off, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

}  // namespace

extern "C" {

int emqxgm_acldb_create(int32_t device, uint32_t word_hash_bits, emqxgm_acldb_t** out) {
  if (!out) return -EINVAL;
  *out = nullptr;
  if (word_hash_bits > 62) return -EINVAL;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -ENODEV;
  emqxgm_acldb* db = new (std::nothrow) emqxgm_acldb();
  if (!db) return -ENOMEM;
  db->device = device;
  db->test_mask = rs_test_mask(word_hash_bits);
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess) {
    delete db;
    return -EIO;
  }
  db->purge = true;  // the first commit lays out the empty database
  const int rc = emqxgm_acldb_commit(db);
  if (rc) {
    emqxgm_acldb_destroy(db);
    return rc;
  }
  *out = db;
  return 0;
}

void emqxgm_acldb_destroy(emqxgm_acldb_t* db) {
  if (!db) return;
  (void)hipSetDevice(db->device);
  if (db->stream) (void)hipStreamSynchronize(db->stream);
  for (AdbTable& t : db->tab) adb_free(t.d);
  adb_free(db->pool.d);
  adb_free(db->fb.d);
  adb_free(db->fo.d);
  adb_free(db->kb.d);
  adb_free(db->ko.d);
  adb_free(db->all_d);
  for (AdbBuf& b : db->sc) adb_free(b);
  for (hipEvent_t e : db->ev)
    if (e) (void)hipEventDestroy(e);
  if (db->stream) (void)hipStreamDestroy(db->stream);
  delete db;
}

int emqxgm_acldb_store(emqxgm_acldb_t* db, uint32_t kind, const uint8_t* key, uint32_t klen, const uint32_t* perm,
                       const uint32_t* action, const uint8_t* filter_bytes, const uint32_t* filter_offsets,
                       uint32_t n_rules) {
  if (!db || kind > ADB_ALL || (kind != ADB_ALL && klen && !key)) return -EINVAL;
  if (!adb_rules_ok(perm, action, filter_bytes, filter_offsets, 0, n_rules)) return -EINVAL;
  std::lock_guard<std::mutex> g(db->mu);
  adb_pend(db, kind, false, key, klen, perm, action, filter_bytes, filter_offsets, 0, n_rules);
  return 0;
}

int emqxgm_acldb_store_many(emqxgm_acldb_t* db, uint32_t n_records, const uint32_t* kind, const uint8_t* key_bytes,
                            const uint32_t* key_offsets, const uint32_t* rule_offsets, const uint32_t* perm,
                            const uint32_t* action, const uint8_t* filter_bytes, const uint32_t* filter_offsets) {
  if (!db) return -EINVAL;
  if (n_records == 0) return 0;
  if (!kind || !key_offsets || !rule_offsets) return -EINVAL;
  for (uint32_t i = 0; i < n_records; ++i) {
    if (kind[i] > ADB_ALL || key_offsets[i + 1] < key_offsets[i]) return -EINVAL;
    if (kind[i] != ADB_ALL && key_offsets[i + 1] > key_offsets[i] && !key_bytes) return -EINVAL;
    if (!adb_rules_ok(perm, action, filter_bytes, filter_offsets, rule_offsets[i], rule_offsets[i + 1])) return -EINVAL;
  }
  std::lock_guard<std::mutex> g(db->mu);
  db->pend.reserve(db->pend.size() + n_records);
  for (uint32_t i = 0; i < n_records; ++i)
    adb_pend(db, kind[i], false, key_bytes ? key_bytes + key_offsets[i] : nullptr, key_offsets[i + 1] - key_offsets[i],
             perm, action, filter_bytes, filter_offsets, rule_offsets[i], rule_offsets[i + 1]);
  return 0;
}

int emqxgm_acldb_delete(emqxgm_acldb_t* db, uint32_t kind, const uint8_t* key, uint32_t klen) {
  if (!db || kind > ADB_ALL || (kind != ADB_ALL && klen && !key)) return -EINVAL;
  std::lock_guard<std::mutex> g(db->mu);
  adb_pend(db, kind, true, key, klen, nullptr, nullptr, nullptr, nullptr, 0, 0);
  return 0;
}

int emqxgm_acldb_purge(emqxgm_acldb_t* db) {
  if (!db) return -EINVAL;
  std::lock_guard<std::mutex> g(db->mu);
  adb_clear_pending(db);
  db->purge = true;
  return 0;
}

int emqxgm_acldb_commit(emqxgm_acldb_t* db) {
  if (!db) return -EINVAL;
  std::lock_guard<std::mutex> g(db->mu);
  if (db->broken) return -EIO;
  const int rc = adb_commit(db);
  // the mirror is changed before the uploads: after a failed one no match may use the handle
  if (rc && rc != -ENOMEM) db->broken = true;
  return rc;
}

int emqxgm_acldb_count(emqxgm_acldb_t* db, uint64_t* out) {
  if (!db || !out) return -EINVAL;
  std::lock_guard<std::mutex> g(db->mu);
  int64_t c = db->purge ? 0 : (int64_t)(db->tab[0].live + db->tab[1].live + (db->all_present ? 1 : 0));
  for (const AdbPend& e : db->pend) {
    if (e.dead) continue;
    bool exists = false;
    if (!db->purge) {
      if (e.kind == ADB_ALL) {
        exists = db->all_present;
      } else {
        const uint8_t* key = db->pkb.data() + e.key0;
        uint32_t free_at, chain;
        exists = adb_find(db, e.kind, acl_value_token(e.klen ? key : (const uint8_t*)"", e.klen, db->test_mask), key,
                          e.klen, &free_at, &chain) != NONE;
      }
    }
    if (e.del && exists) --c;
    if (!e.del && !exists) ++c;
  }
  *out = (uint64_t)c;
  return 0;
}

int emqxgm_acldb_match(emqxgm_acldb_t* db, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                       const uint32_t* client, const uint32_t* action, const uint8_t* clientid_bytes,
                       const uint32_t* clientid_offsets, const uint8_t* username_bytes,
                       const uint32_t* username_offsets, const uint32_t* client_flags, uint32_t n_clients,
                       uint32_t* out_perm, uint32_t* out_src, uint32_t* out_pos) {
  if (!db || (n && (!offsets || !client || !action || !out_perm || !out_src || !out_pos))) return -EINVAL;
  if (n_clients && (!clientid_offsets || !username_offsets || !client_flags)) return -EINVAL;
  if (n && !adb_offsets_ok(offsets, n)) return -EINVAL;
  if (n && offsets[n] != offsets[0] && !bytes) return -EINVAL;
  if (n_clients) {
    if (!adb_offsets_ok(clientid_offsets, n_clients) || !adb_offsets_ok(username_offsets, n_clients)) return -EINVAL;
    if (clientid_offsets[n_clients] != clientid_offsets[0] && !clientid_bytes) return -EINVAL;
    if (username_offsets[n_clients] != username_offsets[0] && !username_bytes) return -EINVAL;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (client[i] >= n_clients || (action[i] != ACL_PUBLISH && action[i] != ACL_SUBSCRIBE)) return -EINVAL;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> g(db->mu);
  if (db->broken) return -EIO;
  if (hipSetDevice(db->device) != hipSuccess) return -EIO;
  int rc = adb_put_clients(db, clientid_bytes, clientid_offsets, username_bytes, username_offsets, client_flags,
                           n_clients);
  if (rc) return rc;
  const uint64_t cap = std::min<uint64_t>(db->pass_names, ADB_PASS_MAX);
  for (uint64_t lo = 0; lo < n; lo += cap) {
    const uint32_t hi = (uint32_t)std::min<uint64_t>(n, lo + cap);
    if ((rc = adb_pass(db, bytes, offsets, client, action, n_clients, (uint32_t)lo, hi, out_perm, out_src, out_pos)))
      return rc;
  }
  return 0;
}

int emqxgm_acldb_tune(emqxgm_acldb_t* db, const char* key, int64_t value) {
  if (!db || !key) return -EINVAL;
  std::lock_guard<std::mutex> g(db->mu);
  if (strcmp(key, "pass_names") == 0) {
    if (value < 1) return -EINVAL;
    db->pass_names = (uint64_t)value;
    return 0;
  }
  if (strcmp(key, "counters") == 0) {
    db->counters = value != 0;
    for (uint64_t& c : db->ctr) c = 0;
    return 0;
  }
  if (strcmp(key, "timing") == 0) {
    if (value && !db->ev[1]) {
      if (hipSetDevice(db->device) != hipSuccess) return -EIO;
      for (hipEvent_t& e : db->ev)
        if (!e) ADBCHK(hipEventCreate(&e));
    }
    db->timing = value != 0;
    db->kernel_ms = 0;
    return 0;
  }
  if (strcmp(key, "kernel_us") == 0) {
    const double us = db->kernel_ms * 1000.0;
    return us > 2147483647.0 ? 2147483647 : (int)us;
  }
  if (strcmp(key, "rebuild_load_pct") == 0) {
    if (value < 1 || value > 50) return -EINVAL;
    db->load_pct = (uint32_t)value;
    return 0;
  }
  if (strcmp(key, "rebuild_garbage_pct") == 0) {
    if (value < 1 || value > 1000000) return -EINVAL;
    db->garbage_pct = (uint32_t)value;
    return 0;
  }
  return -EINVAL;
}

int emqxgm_acldb_stats(emqxgm_acldb_t* db, uint64_t out[20]) {
  if (!db || !out) return -EINVAL;
  std::lock_guard<std::mutex> g(db->mu);
  for (uint32_t k = 0; k < 2; ++k) {
    out[3 * k] = db->tab[k].live;
    out[3 * k + 1] = db->tab[k].h.size();
    out[3 * k + 2] = db->tab[k].tomb;
  }
  out[6] = db->max_chain;
  out[7] = db->all_rules;
  out[8] = db->live_words;
  out[9] = db->garbage_words;
  out[10] = db->rebuilds;
  out[11] = db->growths;
  for (int c = 0; c < 5; ++c) out[12 + c] = db->ctr[c];
  out[17] = rs_n_tiles((uint32_t)db->all_h.size());
  out[18] = out[19] = 0;
  return 0;
}

}  // extern "C"
