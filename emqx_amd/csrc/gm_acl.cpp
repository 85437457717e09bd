// gm_acl.cpp -- host side of ACL lists that return the first matching rule per request (k_acl,
// gm_acl.inc): the list compiler run at emqxgm_acl_set, the pass driver and the emqxgm_acl_*
// C-ABI of include/emqx_gpumatch.h.  A handle of its own, beside the engine, the retainer and
// the rule set.
//
// Reference: emqx_authz_rule:compile/1 and matches/4 (apps/emqx_authz/src/emqx_authz_rule.erl:
// 61-110, 125-230), called by emqx_authz_file:authorize/4 (emqx_authz_file.erl:64-65) and rule by
// rule by emqx_authz_mnesia:authorize/4 (emqx_authz_mnesia.erl:98-120, 222-229).
//
// Every device array is an allocation of its own.  With -DGM_ACL_EXACT_ALLOC each is exactly the
// bytes in use (no floor, no growth slack): tests/host_harness/acl_dev_main.cpp runs this file
// and the kernel's phases on the CPU under ASan, where a read or write one byte past any array
// then lands in a redzone.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/emqx_gpumatch.h"
#include "gm_acl_match.h"
#include "gm_common.h"
#include "gm_kernels.h"

using namespace gm;

namespace {

struct AclBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// The resident list: six device arrays and what the host knows about them.
struct AclList {
  AclBuf recs, fb, fo, ff, wb, wo;
  uint32_t total_words = 0, n_filters = 0, n_rules = 0;
};

// scratch: the pass's names, clients, actions and answers; the call's client table; the control
// words
enum { ACL_NB, ACL_NO, ACL_CL, ACL_AC, ACL_OUT, ACL_CB, ACL_CO, ACL_UB, ACL_UO, ACL_CF, ACL_WBITS, ACL_CTL,
       ACL_SLOTS };
constexpr size_t ACL_CTL_BYTES = 40;  // 4 x u64 counters, then the error word (and a pad word)
constexpr uint64_t ACL_PASS_MAX = 1ull << 31;

}  // namespace

struct emqxgm_acl {
  std::mutex mu;
  int32_t device = 0;
  hipStream_t stream = nullptr;
  uint64_t test_mask = 0;
  AclList cur;
  uint64_t pass_names = 1ull << 20;
  bool counters = false;
  uint64_t ctr[4] = {0, 0, 0, 0};  // since the last set
  bool timing = false;             // tune "timing": HIP events around the launch of a pass
  hipEvent_t ev[2] = {nullptr, nullptr};
  double kernel_ms = 0;  // since timing was turned on
  AclBuf sc[ACL_SLOTS];
  std::vector<uint32_t> h_off;
};

namespace {

#define ACLCHK(expr)                       \
  do {                                     \
    if ((expr) != hipSuccess) return -EIO; \
  } while (0)

void acl_free(AclBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b = AclBuf();
}

void acl_free_list(AclList& l) {
  acl_free(l.recs);
  acl_free(l.fb);
  acl_free(l.fo);
  acl_free(l.ff);
  acl_free(l.wb);
  acl_free(l.wo);
}

int acl_upload(const void* src, size_t bytes, AclBuf& b) {
#ifdef GM_ACL_EXACT_ALLOC
  const size_t cap = bytes;
#else
  const size_t cap = std::max<size_t>(16, bytes);
#endif
  ACLCHK(hipMalloc(&b.p, cap));
  b.bytes = cap;
  if (bytes) ACLCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

// Scratch slot of at least `bytes` (exactly `bytes` with GM_ACL_EXACT_ALLOC).
int acl_grow(emqxgm_acl* a, int slot, uint64_t bytes) {
  AclBuf& b = a->sc[slot];
#ifdef GM_ACL_EXACT_ALLOC
  if (b.p && b.bytes == bytes) return 0;
  const uint64_t cap = bytes;
#else
  if (b.p && b.bytes >= bytes) return 0;
  const uint64_t cap = std::max<uint64_t>(bytes + bytes / 2, 4096);
#endif
  ACLCHK(hipStreamSynchronize(a->stream));
  acl_free(b);
  ACLCHK(hipMalloc(&b.p, cap));
  b.bytes = cap;
  return 0;
}

// Slot `slot` holds src[0 .. bytes) (asynchronous on the handle's stream).
int acl_put(emqxgm_acl* a, int slot, const void* src, uint64_t bytes) {
  const int rc = acl_grow(a, slot, bytes);
  if (rc) return rc;
  if (bytes) ACLCHK(hipMemcpyAsync(a->sc[slot].p, src, bytes, hipMemcpyHostToDevice, a->stream));
  return 0;
}

// offsets [lo .. hi] rebased to 0 into h_off, then into `slot`.  The copy is asynchronous and
// h_off is reused, so the stream is drained first.
int acl_put_offsets(emqxgm_acl* a, int slot, const uint32_t* offsets, uint32_t lo, uint32_t hi) {
  ACLCHK(hipStreamSynchronize(a->stream));
  const uint32_t m = hi - lo + 1, o0 = offsets[lo];
  a->h_off.resize(m);
  for (uint32_t i = 0; i < m; ++i) a->h_off[i] = offsets[lo + i] - o0;
  return acl_put(a, slot, a->h_off.data(), (uint64_t)m * 4);
}

struct AclTable {
  const uint8_t *cb, *ub;
  const uint32_t *co, *uo, *cf;
  const uint64_t* wbits;
  uint32_t n;
};

// The call's client table into its scratch slots.
int acl_put_clients(emqxgm_acl* a, const AclTable& t) {
  static const uint32_t zero = 0;
  int rc = 0;
  const uint32_t cbytes = t.n ? t.co[t.n] - t.co[0] : 0, ubytes = t.n ? t.uo[t.n] - t.uo[0] : 0;
  if ((rc = acl_put(a, ACL_CB, cbytes ? t.cb + t.co[0] : nullptr, cbytes)) ||
      (rc = acl_put(a, ACL_UB, ubytes ? t.ub + t.uo[0] : nullptr, ubytes)) ||
      (rc = acl_put(a, ACL_CF, t.cf, (uint64_t)t.n * 4)) || (rc = acl_put(a, ACL_WBITS, t.wbits, (uint64_t)t.n * 8)))
    return rc;
  if (t.n == 0) {
    if ((rc = acl_put(a, ACL_CO, &zero, 4)) || (rc = acl_put(a, ACL_UO, &zero, 4))) return rc;
    ACLCHK(hipStreamSynchronize(a->stream));
    return 0;
  }
  if ((rc = acl_put_offsets(a, ACL_CO, t.co, 0, t.n)) || (rc = acl_put_offsets(a, ACL_UO, t.uo, 0, t.n))) return rc;
  ACLCHK(hipStreamSynchronize(a->stream));
  return 0;
}

// One pass: requests [lo, hi) of the call.
int acl_pass(emqxgm_acl* a, const uint8_t* bytes, const uint32_t* offsets, const uint32_t* client,
             const uint32_t* action, uint32_t n_clients, uint32_t lo, uint32_t hi, uint32_t* out_rule) {
  const uint32_t np = hi - lo;
  const uint32_t o0 = offsets[lo];
  const uint64_t nbytes = offsets[hi] - o0;
  hipStream_t s = a->stream;
  int rc = 0;
  if ((rc = acl_put(a, ACL_NB, nbytes ? bytes + o0 : nullptr, nbytes)) ||
      (rc = acl_put_offsets(a, ACL_NO, offsets, lo, hi)) || (rc = acl_put(a, ACL_CL, client + lo, (uint64_t)np * 4)) ||
      (rc = acl_put(a, ACL_AC, action + lo, (uint64_t)np * 4)) || (rc = acl_grow(a, ACL_OUT, (uint64_t)np * 4)) ||
      (rc = acl_grow(a, ACL_CTL, ACL_CTL_BYTES)))
    return rc;
  auto B = [&](int k) { return a->sc[k].p; };
  ACLCHK(hipMemsetAsync(B(ACL_CTL), 0, ACL_CTL_BYTES, s));
  const AclList& l = a->cur;
  AclArgs A;
  A.nb = (const uint8_t*)B(ACL_NB);
  A.no = (const uint32_t*)B(ACL_NO);
  A.client = (const uint32_t*)B(ACL_CL);
  A.action = (const uint32_t*)B(ACL_AC);
  A.n = np;
  A.cb = (const uint8_t*)B(ACL_CB);
  A.co = (const uint32_t*)B(ACL_CO);
  A.ub = (const uint8_t*)B(ACL_UB);
  A.uo = (const uint32_t*)B(ACL_UO);
  A.cf = (const uint32_t*)B(ACL_CF);
  A.wbits = (const uint64_t*)B(ACL_WBITS);
  A.n_clients = n_clients;
  A.recs = (const uint64_t*)l.recs.p;
  A.total_words = l.total_words;
  A.fb = (const uint8_t*)l.fb.p;
  A.fo = (const uint32_t*)l.fo.p;
  A.ff = (const uint32_t*)l.ff.p;
  A.n_filters = l.n_filters;
  A.wb = (const uint8_t*)l.wb.p;
  A.wo = (const uint32_t*)l.wo.p;
  A.n_rules = l.n_rules;
  A.test_mask = a->test_mask;
  A.out = (uint32_t*)B(ACL_OUT);
  A.err = (uint32_t*)((uint8_t*)B(ACL_CTL) + 32);
  A.ctr = a->counters ? (unsigned long long*)B(ACL_CTL) : nullptr;
  const bool timed = a->timing && a->ev[1];
  if (timed) ACLCHK(hipEventRecord(a->ev[0], s));
  ACLCHK(launch_acl(A, s));
  if (timed) ACLCHK(hipEventRecord(a->ev[1], s));
  uint64_t ctl[ACL_CTL_BYTES / 8];
  ACLCHK(hipMemcpyAsync(out_rule + lo, A.out, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  ACLCHK(hipMemcpyAsync(ctl, B(ACL_CTL), ACL_CTL_BYTES, hipMemcpyDeviceToHost, s));
  ACLCHK(hipStreamSynchronize(s));
  if ((uint32_t)ctl[4] != 0) return -EIO;
  if (timed) {
    float ms = 0.f;
    ACLCHK(hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
    a->kernel_ms += ms;
  }
  for (int c = 0; c < 4; ++c) a->ctr[c] += ctl[c];
  return 0;
}

bool acl_offsets_ok(const uint32_t* off, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

}  // namespace

extern "C" {

int emqxgm_acl_create(int32_t device, uint32_t word_hash_bits, emqxgm_acl_t** out) {
  if (!out) return -EINVAL;
  *out = nullptr;
  if (word_hash_bits > 62) return -EINVAL;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -ENODEV;
  emqxgm_acl* a = new (std::nothrow) emqxgm_acl();
  if (!a) return -ENOMEM;
  a->device = device;
  a->test_mask = rs_test_mask(word_hash_bits);
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess) {
    delete a;
    return -EIO;
  }
  int rc = emqxgm_acl_set(a, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, 0);
  if (rc) {
    emqxgm_acl_destroy(a);
    return rc;
  }
  *out = a;
  return 0;
}

void emqxgm_acl_destroy(emqxgm_acl_t* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  acl_free_list(a->cur);
  for (AclBuf& b : a->sc) acl_free(b);
  for (hipEvent_t e : a->ev)
    if (e) (void)hipEventDestroy(e);
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

int emqxgm_acl_set(emqxgm_acl_t* a, const uint8_t* filter_bytes, const uint32_t* filter_offsets,
                   const uint32_t* filter_flags, const uint32_t* filter_rule, uint32_t n_filters,
                   const uint32_t* rule_perm, const uint32_t* rule_action, const uint32_t* rule_who,
                   const uint32_t* rule_slot, const uint8_t* who_bytes, const uint32_t* who_offsets,
                   uint32_t n_rules) {
  if (!a || n_rules > 65536u || n_filters > (1u << 20)) return -EINVAL;
  if (n_filters && (!filter_offsets || !filter_flags || !filter_rule)) return -EINVAL;
  if (n_rules && (!rule_perm || !rule_action || !rule_who || !rule_slot || !who_offsets)) return -EINVAL;
  for (uint32_t i = 0; i < n_filters; ++i) {
    if (filter_offsets[i + 1] < filter_offsets[i]) return -EINVAL;
    if (filter_flags[i] != 0 && filter_flags[i] != RS_F_EQ) return -EINVAL;
    if (filter_rule[i] >= n_rules || (i && filter_rule[i] < filter_rule[i - 1])) return -EINVAL;
  }
  for (uint32_t r = 0; r < n_rules; ++r) {
    if (rule_perm[r] > ACL_ALLOW || rule_action[r] < ACL_PUBLISH || rule_action[r] > ACL_ALL) return -EINVAL;
    if (rule_who[r] > ACL_WHO_HOST || rule_slot[r] >= ACL_HOST_SLOTS) return -EINVAL;
    if (who_offsets[r + 1] < who_offsets[r]) return -EINVAL;
  }
  const uint32_t o0 = n_filters ? filter_offsets[0] : 0;
  const uint32_t nbytes = n_filters ? filter_offsets[n_filters] - o0 : 0;
  const uint32_t w0 = n_rules ? who_offsets[0] : 0;
  const uint32_t wbytes = n_rules ? who_offsets[n_rules] - w0 : 0;
  if ((nbytes && !filter_bytes) || (wbytes && !who_bytes)) return -EINVAL;
  // compile: per rule its header, then one record per filter, in filter order, tiled
  std::vector<uint64_t> recs;
  std::vector<uint32_t> fo((size_t)n_filters + 1, 0), ff((size_t)n_filters, 0), wo((size_t)n_rules + 1, 0);
  uint32_t i = 0;
  for (uint32_t r = 0; r < n_rules; ++r) {
    const uint32_t kind = rule_who[r];
    const bool str = kind == ACL_WHO_USERNAME || kind == ACL_WHO_CLIENTID;
    const uint32_t wl = who_offsets[r + 1] - who_offsets[r];
    uint64_t rec[ACL_FILTER_HDR + RS_MAX_LEVELS];
    rec[0] = acl_rule_header(rule_perm[r], rule_action[r], kind, kind == ACL_WHO_HOST ? rule_slot[r] : 0, r);
    rec[1] = str ? acl_value_token(wl ? who_bytes + who_offsets[r] : (const uint8_t*)"", wl, a->test_mask) : 0;
    rs_append(recs, rec, ACL_RULE_WORDS);
    wo[r + 1] = who_offsets[r + 1] - w0;
    for (; i < n_filters && filter_rule[i] == r; ++i) {
      const uint8_t* fp = nbytes ? filter_bytes + filter_offsets[i] : (const uint8_t*)"";
      const bool eq = filter_flags[i] == RS_F_EQ;
      const uint32_t nw =
          acl_compile_filter(fp, filter_offsets[i + 1] - filter_offsets[i], eq, r, i, a->test_mask, rec);
      rs_append(recs, rec, nw);
      fo[i + 1] = filter_offsets[i + 1] - o0;
      ff[i] = eq ? RS_F_EQ : RS_F_WORDS;
    }
  }
  std::lock_guard<std::mutex> g(a->mu);
  if (hipSetDevice(a->device) != hipSuccess) return -EIO;
  AclList nl;
  nl.total_words = (uint32_t)recs.size();
  nl.n_filters = n_filters;
  nl.n_rules = n_rules;
  int rc = 0;
  if ((rc = acl_upload(recs.data(), recs.size() * 8, nl.recs)) ||
      (rc = acl_upload(nbytes ? filter_bytes + o0 : nullptr, nbytes, nl.fb)) ||
      (rc = acl_upload(fo.data(), fo.size() * 4, nl.fo)) || (rc = acl_upload(ff.data(), ff.size() * 4, nl.ff)) ||
      (rc = acl_upload(wbytes ? who_bytes + w0 : nullptr, wbytes, nl.wb)) ||
      (rc = acl_upload(wo.data(), wo.size() * 4, nl.wo))) {
    acl_free_list(nl);
    return rc;
  }
  if (hipStreamSynchronize(a->stream) != hipSuccess) {
    acl_free_list(nl);
    return -EIO;
  }
  AclList old = a->cur;
  a->cur = nl;
  acl_free_list(old);
  for (uint64_t& c : a->ctr) c = 0;
  return 0;
}

int emqxgm_acl_match(emqxgm_acl_t* a, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                     const uint32_t* client, const uint32_t* action, const uint8_t* clientid_bytes,
                     const uint32_t* clientid_offsets, const uint8_t* username_bytes,
                     const uint32_t* username_offsets, const uint32_t* client_flags, const uint64_t* who_bits,
                     uint32_t n_clients, uint32_t* out_rule) {
  if (!a || (n && (!offsets || !client || !action || !out_rule))) return -EINVAL;
  if (n_clients && (!clientid_offsets || !username_offsets || !client_flags || !who_bits)) return -EINVAL;
  if (n && !acl_offsets_ok(offsets, n)) return -EINVAL;
  if (n && offsets[n] != offsets[0] && !bytes) return -EINVAL;
  if (n_clients) {
    if (!acl_offsets_ok(clientid_offsets, n_clients) || !acl_offsets_ok(username_offsets, n_clients)) return -EINVAL;
    if (clientid_offsets[n_clients] != clientid_offsets[0] && !clientid_bytes) return -EINVAL;
    if (username_offsets[n_clients] != username_offsets[0] && !username_bytes) return -EINVAL;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (client[i] >= n_clients || (action[i] != ACL_PUBLISH && action[i] != ACL_SUBSCRIBE)) return -EINVAL;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> g(a->mu);
  if (hipSetDevice(a->device) != hipSuccess) return -EIO;
  const AclTable tab = {clientid_bytes, username_bytes, clientid_offsets, username_offsets, client_flags, who_bits,
                        n_clients};
  int rc = acl_put_clients(a, tab);
  if (rc) return rc;
  const uint64_t cap = std::min<uint64_t>(a->pass_names, ACL_PASS_MAX);
  for (uint64_t lo = 0; lo < n; lo += cap) {
    const uint32_t hi = (uint32_t)std::min<uint64_t>(n, lo + cap);
    if ((rc = acl_pass(a, bytes, offsets, client, action, n_clients, (uint32_t)lo, hi, out_rule))) return rc;
  }
  return 0;
}

int emqxgm_acl_tune(emqxgm_acl_t* a, const char* key, int64_t value) {
  if (!a || !key) return -EINVAL;
  std::lock_guard<std::mutex> g(a->mu);
  if (strcmp(key, "pass_names") == 0) {
    if (value < 1) return -EINVAL;
    a->pass_names = (uint64_t)value;
    return 0;
  }
  if (strcmp(key, "counters") == 0) {
    a->counters = value != 0;
    return 0;
  }
  if (strcmp(key, "timing") == 0) {
    if (value && !a->ev[1]) {
      if (hipSetDevice(a->device) != hipSuccess) return -EIO;
      for (hipEvent_t& e : a->ev)
        if (!e) ACLCHK(hipEventCreate(&e));
    }
    a->timing = value != 0;
    a->kernel_ms = 0;
    return 0;
  }
  // read-only key: the kernel time summed since "timing" was set, in microseconds
  if (strcmp(key, "kernel_us") == 0) {
    const double us = a->kernel_ms * 1000.0;
    return us > 2147483647.0 ? 2147483647 : (int)us;
  }
  return -EINVAL;
}

int emqxgm_acl_stats(emqxgm_acl_t* a, uint64_t out[8]) {
  if (!a || !out) return -EINVAL;
  std::lock_guard<std::mutex> g(a->mu);
  out[0] = a->cur.n_filters;
  out[1] = rs_n_tiles(a->cur.total_words);
  out[2] = a->cur.n_filters;
  out[3] = a->cur.n_rules;
  for (int c = 0; c < 4; ++c) out[4 + c] = a->ctr[c];
  return 0;
}

}  // extern "C"
