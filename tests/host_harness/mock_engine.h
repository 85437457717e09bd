// mock_engine.h -- TEST INFRASTRUCTURE: the engine entry points emqx_amd/csrc/gm_async.cpp is a
// layer over (emqxgm_host_alloc / _free, emqxgm_match_batch_submit_filters / _wait_filters, ...),
// as a mock whose "device pass" is the oracle's C++ restatement of emqx_trie:match/1 + the
// route-key lookup (oracle/ref_trie.cpp, emqx_trie.erl:282-348, emqx_router.erl:141-146), with the
// real engine's contract enforced: at most EMQXGM_HOST_PIPES tickets in flight per handle (-EBUSY
// beyond), a result's buffers valid only until ticket + EMQXGM_HOST_PIPES is submitted (the mock
// then poisons them, so a layer that reads a released result reports garbage and fails the
// check), and waits that take a random while.
//
// Included by exactly one translation unit of a program: tests/host_harness/async_harness.cpp
// (the layer alone; the index is the global g_filters / g_ref) and, with MOCK_ENGINE_FULL defined
// first, tests/host_harness/nif_driver_mock.cpp (the NIF on the fake erl_nif runtime).
//
// MOCK_ENGINE_FULL adds emqxgm_create / _destroy / _tune and the membership calls: route_set,
// _set_many, _set_batch, _dests_batch, sync_begin / _end, commit, trie_member, route_member,
// trie_empty record into a set of route keys per engine, and a commit rebuilds the engine's
// oracle trie from the set; filter ids are the positions in the sorted committed set.  Its publish
// pass (emqxgm_publish_batch) has a fixed fan-out, a function of the matched filter ids alone: for
// each matched filter id f, in match_routes order (the exact key, then the trie row),
//     entry (f, node f % 3); if f is odd, entry (f, EMQXGM_DEST_GROUP | f % 2);
//     delivery (f, subscriber f % 5).
// Every call there returns g_stub_rc while that is not 0 (the driver's `rc` line).
#pragma once
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/emqx_gpumatch.h"
#include "../../emqx_amd/csrc/gm_internal.h"

extern "C" {
void* ref_create(int compact);
void ref_destroy(void* h);
int ref_add_many(void* h, const uint8_t* bytes, const uint64_t* off, uint64_t n, const uint8_t* kind);
int ref_match_batch(void* h, const uint8_t* tb, const uint32_t* toff, uint64_t n, int threads,
                    uint64_t* row, uint32_t** ids_out, uint64_t* n_ids, uint32_t* exact);
void ref_free(void* p);
}

#define CHECK(c, ...)                                             \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
      fprintf(stderr, __VA_ARGS__);                               \
      fprintf(stderr, "\n");                                      \
      abort();                                                    \
    }                                                             \
  } while (0)

namespace {

std::vector<std::string> g_filters;  // oracle ids = registration order
void* g_ref = nullptr;
std::mutex g_ref_mu;  // ref_match_batch is a reader, but keep the oracle single-threaded

struct MockPipe {
  uint64_t ticket = 0;
  int state = 0;  // 0 free / taken, 1 in flight
  std::vector<uint32_t> row, fid, exact, foff;
  std::vector<uint8_t> fb;
};

}  // namespace

struct emqxgm {
  std::mutex mu;
  MockPipe p[EMQXGM_HOST_PIPES];
  uint64_t next = 1;
  std::atomic<uint64_t> busy{0};
  std::atomic<int> stale{0};     // the engine's health mark (emqxgm_mark_stale)
  std::atomic<int> hang_us{0};   // health mode: waits stall this long (a hung device)
  // MOCK_ENGINE_FULL: the engine's own index (else the global one)
  void* ref = nullptr;
  std::vector<std::string> filters;    // committed, sorted: ids
  std::map<std::string, uint32_t> set; // pending route keys -> the sync generation that set them
  uint32_t gen = 0;
  uint64_t epoch = 0;
  uint32_t local_node = 0;
  // the publish pass's result (valid until the handle's next one)
  std::vector<uint64_t> route_ptr, deliver_ptr;
  std::vector<uint32_t> route_filter, route_dest, deliver_filter, deliver_sub;
};

namespace {
void* mock_ref(emqxgm* h) { return h->ref ? h->ref : g_ref; }
const std::vector<std::string>& mock_filters(emqxgm* h) { return h->ref ? h->filters : g_filters; }
}  // namespace

#ifdef MOCK_ENGINE_FULL
extern "C" int g_stub_rc;
int g_stub_rc = 0;
#define MOCK_RC()                      \
  do {                                 \
    if (g_stub_rc) return g_stub_rc;   \
  } while (0)
#else
#define MOCK_RC() \
  do {            \
  } while (0)
#endif

extern "C" {

void* emqxgm_host_alloc(emqxgm_t*, uint64_t bytes) { return malloc(bytes ? bytes : 1); }
int emqxgm_mark_stale(emqxgm_t* h, int) {
  h->stale.store(1);
  return 0;
}
void emqxgm_host_free(emqxgm_t*, void* p) { free(p); }

int emqxgm_match_batch_submit_filters(emqxgm_t* h, const uint8_t* bytes, const uint32_t* off,
                                      uint32_t n, uint64_t* ticket) {
  MOCK_RC();
  if (h->stale.load()) return -ESTALE;  // the real engine refuses a stale index's windows
  std::lock_guard<std::mutex> g(h->mu);
  const uint64_t tk = h->next;
  MockPipe& p = h->p[tk % EMQXGM_HOST_PIPES];
  if (p.state == 1) {
    h->busy++;
    return -EBUSY;
  }
  // the previous result of this pipe is overwritten now: poison it first (a reader of a released
  // result then sees garbage)
  std::fill(p.row.begin(), p.row.end(), 0xDEADBEEFu);
  std::fill(p.fid.begin(), p.fid.end(), 0xDEADBEEFu);
  std::fill(p.foff.begin(), p.foff.end(), 0xDEADBEEFu);
  std::fill(p.fb.begin(), p.fb.end(), (uint8_t)0xEE);
  CHECK(off[0] == 0, "offsets[0]");
  std::vector<uint64_t> row(n + 1);
  uint32_t* ids = nullptr;
  uint64_t nid = 0;
  p.exact.assign(n, 0);
  {
    std::lock_guard<std::mutex> r(g_ref_mu);
    ref_match_batch(mock_ref(h), bytes, off, n, 1, row.data(), &ids, &nid, p.exact.data());
    p.row.assign(row.begin(), row.end());
    p.fid.assign(ids, ids + nid);
    ref_free(ids);
    p.foff.assign(1, 0);
    p.fb.clear();
    const std::vector<std::string>& fs = mock_filters(h);
    for (uint32_t id : p.fid) {
      p.fb.insert(p.fb.end(), fs[id].begin(), fs[id].end());
      p.foff.push_back((uint32_t)p.fb.size());
    }
  }
  p.ticket = tk;
  p.state = 1;
  h->next += 1;
  *ticket = tk;
  return 0;
}

}  // extern "C"
int gm_stale(emqxgm_t* h) { return h->stale.load(); }
// the engine's buffers sized for the layer's windows (nothing to size in the mock)
int gm_reserve_windows(emqxgm_t* h, uint32_t n, uint64_t) { return h && n ? 0 : -EINVAL; }
// the layer's window submit (gm_engine.cpp skips the offsets check there; the mock checks them)
int gm_submit_window(emqxgm_t* h, const uint8_t* bytes, const uint32_t* off, uint32_t n,
                     uint64_t* ticket) {
  for (uint32_t i = 0; i < n; ++i) CHECK(off[i + 1] >= off[i], "window offsets increase");
  return emqxgm_match_batch_submit_filters(h, bytes, off, n, ticket);
}
extern "C" {

std::atomic<int> g_hang{0};  // health mode: every wait blocks while set (a hung device)

int emqxgm_match_batch_wait_filters(emqxgm_t* h, uint64_t ticket, emqxgm_batch_out* out,
                                    const uint32_t** foff, const uint8_t** fbytes) {
  // the "device" takes a while; the layer must not hold its own lock meanwhile
  thread_local std::mt19937 rng(std::hash<std::thread::id>()(std::this_thread::get_id()));
  std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));
  while (g_hang.load()) std::this_thread::sleep_for(std::chrono::microseconds(200));
  std::lock_guard<std::mutex> g(h->mu);
  MockPipe& p = h->p[ticket % EMQXGM_HOST_PIPES];
  if (ticket == 0 || p.ticket != ticket || p.state != 1) return -ENOENT;
  p.state = 0;
  out->n = (uint32_t)p.exact.size();
  out->n_pairs = (uint32_t)p.fid.size();
  out->row_ptr = p.row.data();
  out->filter_id = p.fid.data();
  out->exact_id = p.exact.data();
  *foff = p.foff.data();
  *fbytes = p.fb.data();
  return 0;
}

#ifdef MOCK_ENGINE_FULL
int emqxgm_abi_version(void) { return EMQXGM_ABI_VERSION; }

int emqxgm_create(const emqxgm_cfg* cfg, emqxgm_t** out) {
  MOCK_RC();
  if (!cfg || !out) return -EINVAL;
  emqxgm* h = new emqxgm();
  h->ref = ref_create(1);
  *out = h;
  return 0;
}

void emqxgm_destroy(emqxgm_t* h) {
  if (!h) return;
  ref_destroy(h->ref);
  delete h;
}

int emqxgm_tune(emqxgm_t* h, const char* key, int64_t) {
  MOCK_RC();
  return h && (!strcmp(key, "spin_us") || !strcmp(key, "bg_build")) ? 0 : -EINVAL;
}

int emqxgm_get_stats(emqxgm_t*, emqxgm_stats* st) {
  MOCK_RC();
  memset(st, 0, sizeof *st);
  return 0;
}

int emqxgm_get_health(emqxgm_t* h, emqxgm_health_t* out) {
  memset(out, 0, sizeof *out);
  return h->stale.load();
}

int emqxgm_set_local_node(emqxgm_t* h, uint32_t node) {
  MOCK_RC();
  h->local_node = node;
  return 0;
}

static bool mock_wild(const std::string& f) {
  return f.find('+') != std::string::npos || f.find('#') != std::string::npos;
}

int emqxgm_commit(emqxgm_t* h, uint64_t* epoch) {
  MOCK_RC();
  std::vector<std::string> fs;
  std::vector<uint8_t> fb, kind;
  std::vector<uint64_t> fo{0};
  for (auto& kv : h->set) {  // a std::map: sorted
    fs.push_back(kv.first);
    fb.insert(fb.end(), kv.first.begin(), kv.first.end());
    fo.push_back(fb.size());
    kind.push_back(mock_wild(kv.first) ? 3 : 2);
  }
  void* r = ref_create(1);
  ref_add_many(r, fb.data(), fo.data(), fs.size(), kind.data());
  {
    std::lock_guard<std::mutex> g(g_ref_mu);
    ref_destroy(h->ref);
    h->ref = r;
    h->filters.swap(fs);
  }
  h->epoch += 1;
  if (epoch) *epoch = h->epoch;
  return 0;
}

int emqxgm_route_set(emqxgm_t* h, const uint8_t* f, uint32_t len, int present) {
  MOCK_RC();
  const std::string s((const char*)f, len);
  if (present) h->set[s] = h->gen;
  else h->set.erase(s);
  return 0;
}

int emqxgm_route_set_many(emqxgm_t* h, const uint8_t* bytes, const uint64_t* off, uint64_t n, int present) {
  MOCK_RC();
  for (uint64_t i = 0; i < n; ++i) emqxgm_route_set(h, bytes + off[i], (uint32_t)(off[i + 1] - off[i]), present);
  return 0;
}

int emqxgm_route_set_batch(emqxgm_t* h, const uint8_t* bytes, const uint64_t* off, const uint8_t* present,
                           uint64_t n, uint32_t flags, uint64_t* epoch) {
  MOCK_RC();
  for (uint64_t i = 0; i < n; ++i)
    emqxgm_route_set(h, bytes + off[i], (uint32_t)(off[i + 1] - off[i]), present ? present[i] : 1);
  if (epoch) *epoch = h->epoch;
  return (flags & EMQXGM_SET_COMMIT) ? emqxgm_commit(h, epoch) : 0;
}

// a filter is a route key while it has a dest; the dests themselves are the fixed fan-out above
int emqxgm_route_dests_batch(emqxgm_t* h, const uint8_t* bytes, const uint64_t* off, uint64_t n,
                             const uint32_t* dptr, const uint32_t* node, const uint32_t* group,
                             uint32_t flags, uint64_t* epoch) {
  MOCK_RC();
  for (uint64_t i = 0; i < n; ++i) {
    for (uint32_t j = dptr[i]; j < dptr[i + 1]; ++j) CHECK(node[j] != EMQXGM_NONE || group[j] != EMQXGM_NONE, "dest %u", j);
    emqxgm_route_set(h, bytes + off[i], (uint32_t)(off[i + 1] - off[i]), dptr[i + 1] > dptr[i]);
  }
  if (epoch) *epoch = h->epoch;
  return (flags & EMQXGM_SET_COMMIT) ? emqxgm_commit(h, epoch) : 0;
}

int emqxgm_subscribers_batch(emqxgm_t* h, const uint8_t*, const uint64_t* off, uint64_t n, const uint32_t* sptr,
                             const uint32_t* subs, uint32_t flags, uint64_t* epoch) {
  MOCK_RC();
  uint64_t sum = 0;  // every array read to its end: a short one is a sanitizer report
  for (uint64_t i = 0; i < n; ++i) {
    CHECK(off[i + 1] >= off[i] && sptr[i + 1] >= sptr[i], "offsets of filter %llu", (unsigned long long)i);
    for (uint32_t j = sptr[i]; j < sptr[i + 1]; ++j) sum += subs[j];
  }
  (void)sum;
  if (epoch) *epoch = h->epoch;
  return (flags & EMQXGM_SET_COMMIT) ? emqxgm_commit(h, epoch) : 0;
}

int emqxgm_route_sync_begin(emqxgm_t* h, uint32_t* gen) {
  MOCK_RC();
  *gen = ++h->gen;
  return 0;
}

int emqxgm_route_sync_end(emqxgm_t* h, uint32_t gen, uint64_t* removed) {
  MOCK_RC();
  if (gen != h->gen) return -ESTALE;
  uint64_t n = 0;
  for (auto it = h->set.begin(); it != h->set.end();)
    if (it->second != gen) {
      it = h->set.erase(it);
      ++n;
    } else {
      ++it;
    }
  if (removed) *removed = n;
  return 0;
}

static bool mock_committed(emqxgm_t* h, const uint8_t* f, uint32_t len) {
  return std::binary_search(h->filters.begin(), h->filters.end(), std::string((const char*)f, len));
}
int emqxgm_route_member(emqxgm_t* h, const uint8_t* f, uint32_t len) {
  MOCK_RC();
  return mock_committed(h, f, len);
}
int emqxgm_trie_member(emqxgm_t* h, const uint8_t* f, uint32_t len) {
  MOCK_RC();
  return mock_committed(h, f, len) && mock_wild(std::string((const char*)f, len));
}
int emqxgm_trie_empty(emqxgm_t* h) {
  MOCK_RC();
  for (auto& f : h->filters)
    if (mock_wild(f)) return 0;
  return 1;
}

int emqxgm_publish_batch(emqxgm_t* h, const uint8_t* bytes, const uint32_t* off, uint32_t n, emqxgm_publish_out* out) {
  MOCK_RC();
  std::vector<uint64_t> row(n + 1);
  std::vector<uint32_t> exact(n, 0);
  uint32_t* ids = nullptr;
  uint64_t nid = 0;
  {
    std::lock_guard<std::mutex> r(g_ref_mu);
    ref_match_batch(h->ref, bytes, off, n, 1, row.data(), &ids, &nid, exact.data());
  }
  h->route_ptr.assign(1, 0);
  h->deliver_ptr.assign(1, 0);
  h->route_filter.clear();
  h->route_dest.clear();
  h->deliver_filter.clear();
  h->deliver_sub.clear();
  auto fan = [&](uint32_t f) {
    h->route_filter.push_back(f);
    h->route_dest.push_back(f % 3);
    if (f & 1) {
      h->route_filter.push_back(f);
      h->route_dest.push_back(EMQXGM_DEST_GROUP | (f % 2));
    }
    h->deliver_filter.push_back(f);
    h->deliver_sub.push_back(f % 5);
  };
  for (uint32_t i = 0; i < n; ++i) {
    if (exact[i] != EMQXGM_NONE) fan(exact[i]);
    for (uint64_t j = row[i]; j < row[i + 1]; ++j) fan(ids[j]);
    h->route_ptr.push_back(h->route_filter.size());
    h->deliver_ptr.push_back(h->deliver_filter.size());
  }
  ref_free(ids);
  out->n = n;
  out->n_routes = h->route_filter.size();
  out->n_deliveries = h->deliver_filter.size();
  out->route_ptr = h->route_ptr.data();
  out->route_filter = h->route_filter.data();
  out->route_dest = h->route_dest.data();
  out->deliver_ptr = h->deliver_ptr.data();
  out->deliver_filter = h->deliver_filter.data();
  out->deliver_sub = h->deliver_sub.data();
  return 0;
}

int emqxgm_filters_copy(emqxgm_t* h, const uint32_t* ids, uint64_t n, uint8_t* buf, uint64_t cap, uint64_t* offsets) {
  MOCK_RC();
  std::lock_guard<std::mutex> g(g_ref_mu);
  uint64_t at = 0;
  offsets[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const std::string& f = h->filters[ids[i]];
    if (at + f.size() <= cap) memcpy(buf + at, f.data(), f.size());
    at += f.size();
    offsets[i + 1] = at;
  }
  return at > cap ? -ENOSPC : 0;
}
#endif  // MOCK_ENGINE_FULL

}  // extern "C"
