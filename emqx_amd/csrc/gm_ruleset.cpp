// gm_ruleset.cpp -- host side of rule sets that return every matching rule per name
// (k_ruleset, gm_ruleset.inc): the list compiler run at emqxgm_ruleset_set, the pass driver and
// the emqxgm_ruleset_* C-ABI of include/emqx_gpumatch.h.  A handle of its own, beside the engine
// and the retainer.
//
// Reference: emqx_rule_engine:get_rules_for_topic/1 (apps/emqx_rule_engine/src/
// emqx_rule_engine.erl:198-204) with emqx_plugin_libs_rule:can_topic_match_oneof/2
// (emqx_plugin_libs_rule.erl:340-346), emqx_bridge:get_matched_egress_bridges/1
// (emqx_bridge.erl:342-382), and the exhook / trace filters (emqx_exhook_server.erl:361,
// emqx_trace_handler.erl:138).
//
// Every device array is an allocation of its own.  With -DGM_RULESET_EXACT_ALLOC each is exactly
// the bytes in use (no floor, no growth slack): tests/host_harness/ruleset_dev_main.cpp runs this
// file and the kernel's phases on the CPU under ASan, where a read or write one byte past any
// array then lands in a redzone.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/emqx_gpumatch.h"
#include "gm_common.h"
#include "gm_kernels.h"
#include "gm_ruleset_match.h"

using namespace gm;

namespace {

struct RsBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// The resident list: four device arrays and what the host knows about them.
struct RsList {
  RsBuf recs, fb, fo, ff;
  uint32_t total_words = 0, n_filters = 0, n_rules = 0;
};

enum { RS_NB, RS_NO, RS_CNT, RS_ROW, RS_TMP, RS_CTL, RS_RULE, RS_SLOTS };
constexpr size_t RS_CTL_BYTES = 40;  // 4 x u64 counters, then the error word (and a pad word)
constexpr uint64_t RS_PASS_MAX = 1ull << 31;

}  // namespace

struct emqxgm_ruleset {
  std::mutex mu;
  int32_t device = 0;
  hipStream_t stream = nullptr;
  uint64_t test_mask = 0;
  RsList cur;
  uint64_t n_records = 0;
  uint64_t pass_names = 1ull << 20;
  bool counters = false;
  uint64_t ctr[4] = {0, 0, 0, 0};  // since the last set
  bool timing = false;             // tune "timing": HIP events around the two launches of a pass
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  double count_ms = 0, fill_ms = 0;  // since timing was turned on
  RsBuf sc[RS_SLOTS];
  std::vector<uint32_t> h_off, h_row32, h_rule;
  std::vector<uint64_t> h_ptr;
};

namespace {

#define RSCHK(expr)                        \
  do {                                     \
    if ((expr) != hipSuccess) return -EIO; \
  } while (0)

void rs_free(RsBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b = RsBuf();
}

void rs_free_list(RsList& l) {
  rs_free(l.recs);
  rs_free(l.fb);
  rs_free(l.fo);
  rs_free(l.ff);
}

int rs_upload(const void* src, size_t bytes, RsBuf& b) {
#ifdef GM_RULESET_EXACT_ALLOC
  const size_t cap = bytes;
#else
  const size_t cap = std::max<size_t>(16, bytes);
#endif
  RSCHK(hipMalloc(&b.p, cap));
  b.bytes = cap;
  if (bytes) RSCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

// Scratch slot of at least `bytes` (exactly `bytes` with GM_RULESET_EXACT_ALLOC).
int rs_grow(emqxgm_ruleset* r, int slot, uint64_t bytes) {
  RsBuf& b = r->sc[slot];
#ifdef GM_RULESET_EXACT_ALLOC
  if (b.p && b.bytes == bytes) return 0;
  const uint64_t cap = bytes;
#else
  if (b.p && b.bytes >= bytes) return 0;
  const uint64_t cap = std::max<uint64_t>(bytes + bytes / 2, 4096);
#endif
  RSCHK(hipStreamSynchronize(r->stream));
  rs_free(b);
  RSCHK(hipMalloc(&b.p, cap));
  b.bytes = cap;
  return 0;
}

// One pass: names [a, b) of the call, at most 2^32 - 1 row entries by the caller's choice of b.
int rs_pass(emqxgm_ruleset* r, const uint8_t* bytes, const uint32_t* offsets, uint32_t a, uint32_t b,
            uint64_t& n_ids) {
  const uint32_t np = b - a;
  const uint32_t o0 = offsets[a];
  const uint64_t nbytes = offsets[b] - o0;
  hipStream_t s = r->stream;
  r->h_off.resize((size_t)np + 1);
  for (uint32_t i = 0; i <= np; ++i) r->h_off[i] = offsets[a + i] - o0;
  int rc = 0;
  if ((rc = rs_grow(r, RS_NB, nbytes)) || (rc = rs_grow(r, RS_NO, ((uint64_t)np + 1) * 4)) ||
      (rc = rs_grow(r, RS_CNT, (uint64_t)np * 4)) || (rc = rs_grow(r, RS_ROW, ((uint64_t)np + 1) * 4)) ||
      (rc = rs_grow(r, RS_TMP, (uint64_t)scan_tmp_words(np) * 4)) || (rc = rs_grow(r, RS_CTL, RS_CTL_BYTES)))
    return rc;
  auto B = [&](int k) { return r->sc[k].p; };
  RSCHK(hipMemsetAsync(B(RS_CTL), 0, RS_CTL_BYTES, s));
  if (nbytes) RSCHK(hipMemcpyAsync(B(RS_NB), bytes + o0, nbytes, hipMemcpyHostToDevice, s));
  RSCHK(hipMemcpyAsync(B(RS_NO), r->h_off.data(), ((size_t)np + 1) * 4, hipMemcpyHostToDevice, s));
  const RsList& l = r->cur;
  RulesetArgs A;
  A.nb = (const uint8_t*)B(RS_NB);
  A.no = (const uint32_t*)B(RS_NO);
  A.n = np;
  A.recs = (const uint64_t*)l.recs.p;
  A.total_words = l.total_words;
  A.fb = (const uint8_t*)l.fb.p;
  A.fo = (const uint32_t*)l.fo.p;
  A.ff = (const uint32_t*)l.ff.p;
  A.n_filters = l.n_filters;
  A.test_mask = r->test_mask;
  A.cnt = (uint32_t*)B(RS_CNT);
  A.err = (uint32_t*)((uint8_t*)B(RS_CTL) + 32);
  A.ctr = r->counters ? (unsigned long long*)B(RS_CTL) : nullptr;
  uint32_t* row = (uint32_t*)B(RS_ROW);
  const bool timed = r->timing && r->ev[3];
  if (timed) RSCHK(hipEventRecord(r->ev[0], s));
  RSCHK(launch_ruleset(A, false, s));
  if (timed) RSCHK(hipEventRecord(r->ev[1], s));
  RSCHK(launch_ruleset_ptr(A.cnt, row, np, (uint32_t*)B(RS_TMP), nullptr, s));
  uint32_t total = 0;
  RSCHK(hipMemcpyAsync(&total, row + np, 4, hipMemcpyDeviceToHost, s));
  RSCHK(hipStreamSynchronize(s));
  if ((rc = rs_grow(r, RS_RULE, (uint64_t)total * 4))) return rc;
  A.cnt = nullptr;
  A.ctr = nullptr;
  A.row = row;
  A.rule = (uint32_t*)B(RS_RULE);
  if (timed) RSCHK(hipEventRecord(r->ev[2], s));
  RSCHK(launch_ruleset(A, true, s));
  if (timed) RSCHK(hipEventRecord(r->ev[3], s));
  r->h_row32.resize((size_t)np + 1);
  r->h_rule.resize(n_ids + total);
  uint64_t ctl[RS_CTL_BYTES / 8];
  RSCHK(hipMemcpyAsync(r->h_row32.data(), row, ((size_t)np + 1) * 4, hipMemcpyDeviceToHost, s));
  if (total)
    RSCHK(hipMemcpyAsync(r->h_rule.data() + n_ids, A.rule, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  RSCHK(hipMemcpyAsync(ctl, B(RS_CTL), RS_CTL_BYTES, hipMemcpyDeviceToHost, s));
  RSCHK(hipStreamSynchronize(s));
  if ((uint32_t)ctl[4] != 0 || r->h_row32[np] != total) return -EIO;
  if (timed) {
    float c = 0.f, f = 0.f;
    RSCHK(hipEventElapsedTime(&c, r->ev[0], r->ev[1]));
    RSCHK(hipEventElapsedTime(&f, r->ev[2], r->ev[3]));
    r->count_ms += c;
    r->fill_ms += f;
  }
  for (int c = 0; c < 4; ++c) r->ctr[c] += ctl[c];
  for (uint32_t i = 0; i <= np; ++i) r->h_ptr[a + i] = n_ids + r->h_row32[i];
  n_ids += total;
  return 0;
}

}  // namespace

extern "C" {

int emqxgm_ruleset_create(int32_t device, uint32_t word_hash_bits, emqxgm_ruleset_t** out) {
  if (!out) return -EINVAL;
  *out = nullptr;
  if (word_hash_bits > 62) return -EINVAL;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -ENODEV;
  emqxgm_ruleset* r = new (std::nothrow) emqxgm_ruleset();
  if (!r) return -ENOMEM;
  r->device = device;
  r->test_mask = rs_test_mask(word_hash_bits);
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) {
    delete r;
    return -EIO;
  }
  int rc = emqxgm_ruleset_set(r, nullptr, nullptr, nullptr, nullptr, 0, 0);
  if (rc) {
    emqxgm_ruleset_destroy(r);
    return rc;
  }
  *out = r;
  return 0;
}

void emqxgm_ruleset_destroy(emqxgm_ruleset_t* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  rs_free_list(r->cur);
  for (RsBuf& b : r->sc) rs_free(b);
  for (hipEvent_t e : r->ev)
    if (e) (void)hipEventDestroy(e);
  if (r->stream) (void)hipStreamDestroy(r->stream);
  delete r;
}

int emqxgm_ruleset_set(emqxgm_ruleset_t* r, const uint8_t* filter_bytes, const uint32_t* filter_offsets,
                       const uint32_t* filter_flags, const uint32_t* filter_rule, uint32_t n_filters,
                       uint32_t n_rules) {
  if (!r || n_rules > 65536u || n_filters > (1u << 20)) return -EINVAL;
  if (n_filters && (!filter_offsets || !filter_flags || !filter_rule)) return -EINVAL;
  for (uint32_t i = 0; i < n_filters; ++i) {
    if (filter_offsets[i + 1] < filter_offsets[i]) return -EINVAL;
    const uint32_t fg = filter_flags[i];
    if (fg != 0 && fg != RS_F_EQ && fg != RS_F_WORDS) return -EINVAL;
    if (filter_rule[i] >= n_rules || (i && filter_rule[i] < filter_rule[i - 1])) return -EINVAL;
  }
  const uint32_t o0 = n_filters ? filter_offsets[0] : 0;
  const uint32_t nbytes = n_filters ? filter_offsets[n_filters] - o0 : 0;
  if (nbytes && !filter_bytes) return -EINVAL;
  // compile: one record per filter, in filter order, tiled
  std::vector<uint64_t> recs;
  std::vector<uint32_t> fo((size_t)n_filters + 1, 0), ff(filter_flags, filter_flags + n_filters);
  for (uint32_t i = 0; i < n_filters; ++i) {
    uint64_t rec[1 + RS_MAX_LEVELS];
    const uint8_t* fp = nbytes ? filter_bytes + filter_offsets[i] : (const uint8_t*)"";
    const uint32_t nw = rs_compile(fp, filter_offsets[i + 1] - filter_offsets[i],
                                   filter_flags[i], filter_rule[i], i, r->test_mask, rec);
    rs_append(recs, rec, nw);
    fo[i + 1] = filter_offsets[i + 1] - o0;
  }
  std::lock_guard<std::mutex> g(r->mu);
  if (hipSetDevice(r->device) != hipSuccess) return -EIO;
  RsList nl;
  nl.total_words = (uint32_t)recs.size();
  nl.n_filters = n_filters;
  nl.n_rules = n_rules;
  int rc = 0;
  if ((rc = rs_upload(recs.data(), recs.size() * 8, nl.recs)) ||
      (rc = rs_upload(nbytes ? filter_bytes + o0 : nullptr, nbytes, nl.fb)) ||
      (rc = rs_upload(fo.data(), fo.size() * 4, nl.fo)) || (rc = rs_upload(ff.data(), ff.size() * 4, nl.ff))) {
    rs_free_list(nl);
    return rc;
  }
  if (hipStreamSynchronize(r->stream) != hipSuccess) {
    rs_free_list(nl);
    return -EIO;
  }
  RsList old = r->cur;
  r->cur = nl;
  rs_free_list(old);
  r->n_records = n_filters;
  for (uint64_t& c : r->ctr) c = 0;
  return 0;
}

int emqxgm_ruleset_match(emqxgm_ruleset_t* r, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                         emqxgm_ruleset_out* out) {
  if (!r || !out || (n && !offsets)) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return -EINVAL;
  if (n && offsets[n] != offsets[0] && !bytes) return -EINVAL;
  std::lock_guard<std::mutex> g(r->mu);
  r->h_ptr.assign((size_t)n + 1, 0);
  r->h_rule.clear();
  out->n = n;
  out->n_ids = 0;
  out->ptr = r->h_ptr.data();
  out->rule = r->h_rule.data();
  if (n == 0) return 0;
  if (hipSetDevice(r->device) != hipSuccess) return -EIO;
  // a pass's 32-bit row pointers cannot overflow: names x rules <= 2^32 - 1
  const uint64_t cap = std::min<uint64_t>(
      std::min<uint64_t>(r->pass_names, RS_PASS_MAX), 0xFFFFFFFFull / std::max<uint32_t>(r->cur.n_rules, 1u));
  uint64_t n_ids = 0;
  for (uint64_t a = 0; a < n; a += cap) {
    const uint32_t b = (uint32_t)std::min<uint64_t>(n, a + cap);
    const int rc = rs_pass(r, bytes, offsets, (uint32_t)a, b, n_ids);
    if (rc) {
      r->h_rule.clear();
      return rc;
    }
  }
  out->n_ids = n_ids;
  out->ptr = r->h_ptr.data();
  out->rule = r->h_rule.data();
  return 0;
}

int emqxgm_ruleset_tune(emqxgm_ruleset_t* r, const char* key, int64_t value) {
  if (!r || !key) return -EINVAL;
  std::lock_guard<std::mutex> g(r->mu);
  if (strcmp(key, "pass_names") == 0) {
    if (value < 1) return -EINVAL;
    r->pass_names = (uint64_t)value;
    return 0;
  }
  if (strcmp(key, "counters") == 0) {
    r->counters = value != 0;
    return 0;
  }
  if (strcmp(key, "timing") == 0) {
    if (value && !r->ev[3]) {
      if (hipSetDevice(r->device) != hipSuccess) return -EIO;
      for (hipEvent_t& e : r->ev)
        if (!e) RSCHK(hipEventCreate(&e));
    }
    r->timing = value != 0;
    r->count_ms = r->fill_ms = 0;
    return 0;
  }
  // read-only keys: the kernel time summed since "timing" was set, in microseconds
  if (strcmp(key, "count_us") == 0 || strcmp(key, "fill_us") == 0) {
    const double us = (key[0] == 'c' ? r->count_ms : r->fill_ms) * 1000.0;
    return us > 2147483647.0 ? 2147483647 : (int)us;
  }
  return -EINVAL;
}

int emqxgm_ruleset_stats(emqxgm_ruleset_t* r, uint64_t out[8]) {
  if (!r || !out) return -EINVAL;
  std::lock_guard<std::mutex> g(r->mu);
  out[0] = r->n_records;
  out[1] = rs_n_tiles(r->cur.total_words);
  out[2] = r->cur.n_filters;
  out[3] = r->cur.n_rules;
  for (int c = 0; c < 4; ++c) out[4 + c] = r->ctr[c];
  return 0;
}

}  // extern "C"
