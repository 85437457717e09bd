// nif_driver_mock.cpp -- TEST INFRASTRUCTURE: what tests/host_harness/nif_driver.c is linked with
// on the CPU (tests/test_nif_host.py) below the real async layer (emqx_amd/csrc/gm_async.cpp):
// the oracle-backed mock engine with its membership calls and its fixed publish fan-out
// (mock_engine.h, MOCK_ENGINE_FULL), and a null stub for every other emqxgm_* the NIF calls
// (retain, rules, ruleset, acl, acldb, share, snapshot).
//
// Null stubs: a *_create succeeds unless g_stub_create_rc is set; every other call returns
// g_stub_rc (the driver's `rc` line), and with 0 an empty result of the right shape (one empty row
// per request, none / nomatch / no_subscribers per request), every input array read to its end so
// that a short one is a sanitizer report.  retain_tune knows its two keys and refuses others.
#define MOCK_ENGINE_FULL
#include "mock_engine.h"

extern "C" int g_stub_create_rc;
int g_stub_create_rc = 0;

namespace {
struct Rows {  // n empty rows
  std::vector<uint64_t> ptr;
  std::vector<uint32_t> ids;
  const uint64_t* rows(uint32_t n) {
    ptr.assign((size_t)n + 1, 0);
    ids.assign(1, 0);
    return ptr.data();
  }
};
uint64_t touch(const uint8_t* bytes, const uint32_t* off, uint32_t n) {
  uint64_t s = 0;
  for (uint32_t i = 0; i < n; ++i) {
    CHECK(off[i + 1] >= off[i], "offsets of item %u", i);
    for (uint32_t j = off[i]; j < off[i + 1]; ++j) s += bytes[j];
  }
  return s;
}
template <class T>
uint64_t touch(const T* v, uint64_t n) {
  uint64_t s = 0;
  for (uint64_t i = 0; i < n; ++i) s += v[i];
  return s;
}
volatile uint64_t g_sink;
}  // namespace

struct emqxgm_retain { Rows r; };
struct emqxgm_ruleset { Rows r; };
struct emqxgm_acl { int x; };
struct emqxgm_acldb { int x; };
struct emqxgm_share { int x; };

extern "C" {

int emqxgm_snapshot_save(emqxgm_t*, const char* path) { g_sink = strlen(path); return g_stub_rc; }
int emqxgm_snapshot_load(emqxgm_t*, const char* path) { g_sink = strlen(path); return g_stub_rc; }

int emqxgm_match_rules(emqxgm_t*, const uint8_t* nb, const uint32_t* no, uint32_t n, const uint8_t* rb,
                       const uint32_t* ro, const uint32_t* rf, uint32_t nr, uint32_t* out) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(nb, no, n) + touch(rb, ro, nr) + touch(rf, nr);
  for (uint32_t i = 0; i < n; ++i) out[i] = EMQXGM_NONE;
  return 0;
}

// ---- retainer ----
int emqxgm_retain_create(int32_t, emqxgm_retain_t** out) {
  if (g_stub_create_rc) return g_stub_create_rc;
  *out = new emqxgm_retain();
  return 0;
}
void emqxgm_retain_destroy(emqxgm_retain_t* r) { delete r; }
int emqxgm_retain_set_indices(emqxgm_retain_t*, const uint32_t* pos, const uint32_t* off, uint32_t n) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(pos, off[n]);
  return 0;
}
int emqxgm_retain_store(emqxgm_retain_t*, const uint8_t* t, uint32_t len, uint64_t, uint32_t* id) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(t, len);
  *id = 0;
  return 0;
}
int emqxgm_retain_store_ts(emqxgm_retain_t* r, const uint8_t* t, uint32_t len, uint64_t e, uint64_t, uint32_t* id) {
  return emqxgm_retain_store(r, t, len, e, id);
}
int emqxgm_retain_delete(emqxgm_retain_t*, const uint8_t* t, uint32_t len) {
  g_sink = touch(t, len);
  return g_stub_rc;
}
int emqxgm_retain_clean(emqxgm_retain_t*) { return g_stub_rc; }
int emqxgm_retain_commit(emqxgm_retain_t*) { return g_stub_rc; }
int emqxgm_retain_tune(emqxgm_retain_t*, const char* key, int64_t) {
  if (g_stub_rc) return g_stub_rc;
  return !strcmp(key, "delta_max") || !strcmp(key, "max_retained_messages") ? 0 : -EINVAL;
}
int emqxgm_retain_topic(emqxgm_retain_t*, uint32_t, const uint8_t**, uint32_t*) { return -ENOENT; }
int emqxgm_retain_match(emqxgm_retain_t* r, const uint8_t* b, const uint32_t* o, uint32_t n, uint64_t,
                        emqxgm_retain_out* out) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(b, o, n);
  out->n = n;
  out->n_ids = 0;
  out->ptr = r->r.rows(n);
  out->id = r->r.ids.data();
  return 0;
}
int emqxgm_retain_match_limit(emqxgm_retain_t* r, const uint8_t* b, const uint32_t* o, uint32_t n, uint64_t now,
                              const uint32_t* limit, emqxgm_retain_cursor* cur, emqxgm_retain_out* out) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(limit, n) + touch((const uint8_t*)cur, sizeof(*cur) * (uint64_t)n);
  return emqxgm_retain_match(r, b, o, n, now, out);
}
int emqxgm_retain_clear_expired(emqxgm_retain_t* r, uint64_t, const uint32_t** ids, uint64_t* n) {
  if (g_stub_rc) return g_stub_rc;
  r->r.rows(0);
  *ids = r->r.ids.data();
  *n = 0;
  return 0;
}
int emqxgm_retain_delete_matching(emqxgm_retain_t* r, const uint8_t* f, uint32_t len, const uint32_t** ids, uint64_t* n) {
  g_sink = touch(f, len);
  return emqxgm_retain_clear_expired(r, 0, ids, n);
}
int emqxgm_retain_page_read(emqxgm_retain_t* r, const uint8_t* f, uint32_t len, uint64_t, uint64_t, uint64_t,
                            const uint32_t** ids, uint64_t* n) {
  if (f) g_sink = touch(f, len);
  return emqxgm_retain_clear_expired(r, 0, ids, n);
}

// ---- rule sets ----
int emqxgm_ruleset_create(int32_t, uint32_t, emqxgm_ruleset_t** out) {
  if (g_stub_create_rc) return g_stub_create_rc;
  *out = new emqxgm_ruleset();
  return 0;
}
void emqxgm_ruleset_destroy(emqxgm_ruleset_t* r) { delete r; }
int emqxgm_ruleset_set(emqxgm_ruleset_t*, const uint8_t* fb, const uint32_t* fo, const uint32_t* fg,
                       const uint32_t* fr, uint32_t nf, uint32_t nr) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(fb, fo, nf) + touch(fg, nf);
  for (uint32_t i = 0; i < nf; ++i) CHECK(fr[i] < nr, "filter %u of rule %u of %u", i, fr[i], nr);
  return 0;
}
int emqxgm_ruleset_match(emqxgm_ruleset_t* r, const uint8_t* b, const uint32_t* o, uint32_t n, emqxgm_ruleset_out* out) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(b, o, n);
  out->n = n;
  out->n_ids = 0;
  out->ptr = r->r.rows(n);
  out->rule = r->r.ids.data();
  return 0;
}

// ---- ACL lists ----
int emqxgm_acl_create(int32_t, uint32_t, emqxgm_acl_t** out) {
  if (g_stub_create_rc) return g_stub_create_rc;
  *out = new emqxgm_acl();
  return 0;
}
void emqxgm_acl_destroy(emqxgm_acl_t* a) { delete a; }
int emqxgm_acl_set(emqxgm_acl_t*, const uint8_t* fb, const uint32_t* fo, const uint32_t* fg, const uint32_t* fr,
                   uint32_t nf, const uint32_t* perm, const uint32_t* action, const uint32_t* who,
                   const uint32_t* slot, const uint8_t* wb, const uint32_t* wo, uint32_t nr) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(fb, fo, nf) + touch(fg, nf) + touch(perm, nr) + touch(action, nr) + touch(who, nr) +
           touch(slot, nr) + (wo[nr] ? touch(wb, wo, nr) : 0);
  for (uint32_t i = 0; i < nf; ++i) CHECK(fr[i] < nr, "filter %u of rule %u of %u", i, fr[i], nr);
  return 0;
}
int emqxgm_acl_match(emqxgm_acl_t*, const uint8_t* b, const uint32_t* o, uint32_t n, const uint32_t* client,
                     const uint32_t* action, const uint8_t* cb, const uint32_t* co, const uint8_t* ub,
                     const uint32_t* uo, const uint32_t* cf, const uint64_t* wbits, uint32_t nc, uint32_t* out) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(b, o, n) + touch(action, n) + touch(cb, co, nc) + touch(ub, uo, nc) + touch(cf, nc) + touch(wbits, nc);
  for (uint32_t i = 0; i < n; ++i) {
    if (client[i] >= nc) return -EINVAL;
    out[i] = EMQXGM_NONE;
  }
  return 0;
}

// ---- the ACL database ----
int emqxgm_acldb_create(int32_t, uint32_t, emqxgm_acldb_t** out) {
  if (g_stub_create_rc) return g_stub_create_rc;
  *out = new emqxgm_acldb();
  return 0;
}
void emqxgm_acldb_destroy(emqxgm_acldb_t* d) { delete d; }
int emqxgm_acldb_store(emqxgm_acldb_t*, uint32_t, const uint8_t* key, uint32_t klen, const uint32_t* perm,
                       const uint32_t* action, const uint8_t* fb, const uint32_t* fo, uint32_t nr) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(key, klen) + touch(perm, nr) + touch(action, nr) + touch(fb, fo, nr);
  return 0;
}
int emqxgm_acldb_delete(emqxgm_acldb_t*, uint32_t, const uint8_t* key, uint32_t klen) {
  g_sink = touch(key, klen);
  return g_stub_rc;
}
int emqxgm_acldb_purge(emqxgm_acldb_t*) { return g_stub_rc; }
int emqxgm_acldb_commit(emqxgm_acldb_t*) { return g_stub_rc; }
int emqxgm_acldb_match(emqxgm_acldb_t*, const uint8_t* b, const uint32_t* o, uint32_t n, const uint32_t* client,
                       const uint32_t* action, const uint8_t* cb, const uint32_t* co, const uint8_t* ub,
                       const uint32_t* uo, const uint32_t* cf, uint32_t nc, uint32_t* perm, uint32_t* src,
                       uint32_t* pos) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(b, o, n) + touch(action, n) + touch(cb, co, nc) + touch(ub, uo, nc) + touch(cf, nc);
  for (uint32_t i = 0; i < n; ++i) {
    if (client[i] >= nc) return -EINVAL;
    perm[i] = src[i] = pos[i] = EMQXGM_NONE;
  }
  return 0;
}

// ---- shared subscriptions ----
int emqxgm_share_create(int32_t, uint32_t, emqxgm_share_t** out) {
  if (g_stub_create_rc) return g_stub_create_rc;
  *out = new emqxgm_share();
  return 0;
}
void emqxgm_share_destroy(emqxgm_share_t* s) { delete s; }
int emqxgm_share_subscribe(emqxgm_share_t*, uint32_t, const uint8_t* t, uint32_t len, uint32_t, uint32_t) {
  g_sink = touch(t, len);
  return g_stub_rc;
}
int emqxgm_share_unsubscribe(emqxgm_share_t*, uint32_t, const uint8_t* t, uint32_t len, uint32_t) {
  g_sink = touch(t, len);
  return g_stub_rc;
}
int emqxgm_share_subscriber_down(emqxgm_share_t*, uint32_t) { return g_stub_rc; }
int emqxgm_share_set_strategy(emqxgm_share_t*, uint32_t, uint32_t) { return g_stub_rc; }
int emqxgm_share_commit(emqxgm_share_t*) { return g_stub_rc; }
int emqxgm_share_pick(emqxgm_share_t*, uint32_t n, const uint32_t* groups, const uint8_t* kb, const uint32_t* ko,
                      const uint32_t* hc, const uint32_t* ht, const uint32_t* draw, const uint32_t* state,
                      uint32_t* out) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(groups, n) + touch(kb, ko, n) + touch(hc, n) + touch(ht, n) + touch(draw, n) + touch(state, n);
  for (uint32_t i = 0; i < n; ++i) {
    out[4 * i] = EMQXGM_NONE;
    out[4 * i + 1] = EMQXGM_SHARE_NO_SUBSCRIBERS;
    out[4 * i + 2] = state[i];
    out[4 * i + 3] = 0;
  }
  return 0;
}
int emqxgm_share_members(emqxgm_share_t*, uint32_t, const uint8_t* t, uint32_t len, uint32_t*, uint32_t, uint32_t* n) {
  if (g_stub_rc) return g_stub_rc;
  g_sink = touch(t, len);
  *n = 0;
  return 0;
}

}  // extern "C"
