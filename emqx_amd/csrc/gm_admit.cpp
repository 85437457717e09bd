// gm_admit.cpp -- host side of the admission pass (k_admit, gm_admit.inc): the handle, the pass
// driver and the emqxgm_admit_* C-ABI of include/emqx_gpumatch.h.  A handle of its own, beside the
// engine, the retainer, the rule set, the ACL list, the ACL database and the shared subscriptions.
//
// Reference: emqx_topic:validate/2 and parse/1 (apps/emqx/src/emqx_topic.erl:98-130, 206-233),
// emqx_mqtt_caps:check_pub/2 and check_sub/3 (apps/emqx/src/emqx_mqtt_caps.erl:74-152).
//
// The pass is stateless: nothing is resident but scratch, which grows on the handle's stream.  A
// call is cut into passes of at most "pass_items" items and ADM_PASS_BYTES bytes (an item larger
// than that is a pass of its own); a pass's bytes are copied to the start of the byte scratch (plus
// "byte_base", 0..15, a test hook that moves the pass through the alignments of a 16-B chunk), whose
// capacity is a whole number of 16-B chunks with one to spare behind the last byte: stage_tile
// reads whole chunks, and the chunk at the pass's end even for a tile of empty items.
//
// With -DGM_ADMIT_EXACT_ALLOC every device array is exactly the bytes in use (no growth slack):
// tests/host_harness/admit_dev_main.cpp runs this file and the kernel's phases on the CPU under
// ASan, where a read or write one byte past any array then lands in a redzone.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/emqx_gpumatch.h"
#include "gm_admit_match.h"
#include "gm_common.h"
#include "gm_kernels.h"

using namespace gm;

static_assert(EMQXGM_ADMIT_NAME == ADM_NAME && EMQXGM_ADMIT_FILTER == ADM_FILTER, "modes");
static_assert(EMQXGM_ADMIT_V_FUNCTION_CLAUSE == ADM_V_FUNCTION_CLAUSE && EMQXGM_ADMIT_V_EMPTY_TOPIC == ADM_V_EMPTY &&
                  EMQXGM_ADMIT_V_TOO_LONG == ADM_V_TOO_LONG && EMQXGM_ADMIT_V_NAME_ERROR == ADM_V_NAME_ERROR &&
                  EMQXGM_ADMIT_V_INVALID_HASH == ADM_V_HASH && EMQXGM_ADMIT_V_INVALID_CHAR == ADM_V_CHAR,
              "validate verdicts");
static_assert(EMQXGM_ADMIT_WILDCARD == ADM_F_WILDCARD && EMQXGM_ADMIT_SHARED == ADM_F_SHARED &&
                  EMQXGM_ADMIT_EXCLUSIVE == ADM_F_EXCLUSIVE && EMQXGM_ADMIT_EXCL_LOOKUP == ADM_F_EXCL_LOOKUP,
              "record flags");
static_assert(EMQXGM_ADMIT_IN_RETAIN == ADM_IN_RETAIN && EMQXGM_ADMIT_IN_HAS_SHARE == ADM_IN_HAS_SHARE &&
                  EMQXGM_ADMIT_RAISES == ADM_RAISES && EMQXGM_ADMIT_MAX_ZONES == ADM_MAX_ZONES,
              "input flags");

namespace {

enum { AD_BYTES, AD_OFF, AD_FLAGS, AD_ZONE, AD_CAPS, AD_OUT, AD_CTL, AD_SLOTS };

struct AdBuf {
  void* p = nullptr;
  uint64_t bytes = 0;
};

constexpr uint64_t ADM_PASS_BYTES = 1ull << 30;
constexpr uint64_t ADM_PASS_ITEMS = 1ull << 22;

}  // namespace

struct emqxgm_admit {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  AdBuf sc[AD_SLOTS];
  std::vector<uint32_t> h_off;  // a pass's offsets from its first byte
  std::vector<uint32_t> h_out;  // the call's records
  uint64_t pass_items = ADM_PASS_ITEMS;
  uint32_t byte_base = 0;
  bool force_global = false, timing = false;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double kernel_ms = 0;
  uint64_t calls = 0, items = 0, bytes = 0, passes = 0, growths = 0;
};

namespace {

#define ADCHK(expr)                        \
  do {                                     \
    if ((expr) != hipSuccess) return -EIO; \
  } while (0)

void ad_free(AdBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b = AdBuf();
}

// Scratch slot of at least `bytes` (exactly `bytes` with GM_ADMIT_EXACT_ALLOC).
int ad_grow(emqxgm_admit* a, int slot, uint64_t bytes) {
  AdBuf& b = a->sc[slot];
#ifdef GM_ADMIT_EXACT_ALLOC
  if (b.p && b.bytes == bytes) return 0;
  const uint64_t cap = bytes;
#else
  if (b.p && b.bytes >= bytes) return 0;
  const uint64_t cap = (std::max<uint64_t>(bytes + bytes / 2, 4096) + 15) & ~15ull;
#endif
  ADCHK(hipStreamSynchronize(a->stream));
  if (b.p) ++a->growths;
  ad_free(b);
  if (!cap) return 0;
  ADCHK(hipMalloc(&b.p, cap));
  b.bytes = cap;
  return 0;
}

int ad_put(emqxgm_admit* a, int slot, const void* src, uint64_t bytes) {
  const int rc = ad_grow(a, slot, bytes);
  if (rc) return rc;
  if (bytes) ADCHK(hipMemcpyAsync(a->sc[slot].p, src, bytes, hipMemcpyHostToDevice, a->stream));
  return 0;
}

uint2 ad_pack_caps(const emqxgm_admit_caps& c) {
  return make_uint2(c.max_topic_levels, (uint32_t)c.max_qos_allowed | (c.retain_available ? ADM_C_RETAIN : 0u) |
                                            (c.wildcard_subscription ? ADM_C_WILDCARD : 0u) |
                                            (c.shared_subscription ? ADM_C_SHARED : 0u) |
                                            (c.exclusive_subscription ? ADM_C_EXCLUSIVE : 0u));
}

// One pass: items [lo, hi) of the call.
int ad_pass(emqxgm_admit* a, uint32_t mode, const uint8_t* bytes, const uint32_t* offsets, const uint8_t* in_flags,
            const uint8_t* zone, uint32_t n_zones, uint32_t lo, uint32_t hi) {
  const uint32_t np = hi - lo, o0 = offsets[lo];
  const uint64_t nbytes = offsets[hi] - o0;
  hipStream_t st = a->stream;
  ADCHK(hipStreamSynchronize(st));  // h_off is reused
  a->h_off.resize((size_t)np + 1);
  for (uint32_t i = 0; i <= np; ++i) a->h_off[i] = offsets[lo + i] - o0;
  // whole 16-B chunks, and one behind the last byte (the file comment)
  const uint64_t cap = ((a->byte_base + nbytes + 15) & ~15ull) + 16;
  int rc = 0;
  if ((rc = ad_grow(a, AD_BYTES, cap)) || (rc = ad_put(a, AD_OFF, a->h_off.data(), ((uint64_t)np + 1) * 4)) ||
      (rc = ad_put(a, AD_FLAGS, in_flags ? in_flags + lo : nullptr, in_flags ? np : 0)) ||
      (rc = ad_put(a, AD_ZONE, zone ? zone + lo : nullptr, zone ? np : 0)) ||
      (rc = ad_grow(a, AD_OUT, (uint64_t)np * 16)) || (rc = ad_grow(a, AD_CTL, 4)))
    return rc;
  uint8_t* d_bytes = (uint8_t*)a->sc[AD_BYTES].p + a->byte_base;
  if (nbytes) ADCHK(hipMemcpyAsync(d_bytes, bytes + o0, nbytes, hipMemcpyHostToDevice, st));
  ADCHK(hipMemsetAsync(a->sc[AD_CTL].p, 0, 4, st));
  AdmitArgs A;
  A.bytes = d_bytes;
  A.off = (const uint32_t*)a->sc[AD_OFF].p;
  A.n = np;
  A.nbytes = (uint32_t)nbytes;
  A.mode = mode;
  A.in_flags = in_flags ? (const uint8_t*)a->sc[AD_FLAGS].p : nullptr;
  A.zone = zone ? (const uint8_t*)a->sc[AD_ZONE].p : nullptr;
  A.caps = (const uint2*)a->sc[AD_CAPS].p;
  A.n_zones = n_zones;
  A.out = (uint4*)a->sc[AD_OUT].p;
  A.err = (uint32_t*)a->sc[AD_CTL].p;
  A.force_global = a->force_global;
  const bool timed = a->timing && a->ev[1];
  if (timed) ADCHK(hipEventRecord(a->ev[0], st));
  ADCHK(launch_admit(A, st));
  if (timed) ADCHK(hipEventRecord(a->ev[1], st));
  uint32_t ctl = 0;
  ADCHK(hipMemcpyAsync(a->h_out.data() + (size_t)lo * 4, A.out, (size_t)np * 16, hipMemcpyDeviceToHost, st));
  ADCHK(hipMemcpyAsync(&ctl, a->sc[AD_CTL].p, 4, hipMemcpyDeviceToHost, st));
  ADCHK(hipStreamSynchronize(st));
  if (ctl != 0) return -EIO;
  if (timed) {
    float ms = 0.f;
    ADCHK(hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
    a->kernel_ms += ms;
  }
  ++a->passes;
  return 0;
}

}  // namespace

extern "C" {

int emqxgm_admit_create(int32_t device, emqxgm_admit_t** out) {
  if (!out) return -EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -ENODEV;
  emqxgm_admit* a = new (std::nothrow) emqxgm_admit();
  if (!a) return -ENOMEM;
  a->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess) {
    delete a;
    return -EIO;
  }
  *out = a;
  return 0;
}

void emqxgm_admit_destroy(emqxgm_admit_t* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  for (AdBuf& b : a->sc) ad_free(b);
  for (hipEvent_t e : a->ev)
    if (e) (void)hipEventDestroy(e);
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

int emqxgm_admit_batch(emqxgm_admit_t* a, uint32_t mode, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                       const uint8_t* in_flags, const uint8_t* zone, const emqxgm_admit_caps* caps, uint32_t n_zones,
                       const uint32_t** out) {
  if (!a || !out || mode > ADM_FILTER || !caps || n_zones < 1 || n_zones > ADM_MAX_ZONES) return -EINVAL;
  *out = nullptr;
  if (n && !offsets) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i] || (zone && zone[i] >= n_zones)) return -EINVAL;
  if (n && offsets[n] != offsets[0] && !bytes) return -EINVAL;
  for (uint32_t z = 0; z < n_zones; ++z)
    if (caps[z].max_qos_allowed > 2) return -EINVAL;
  std::lock_guard<std::mutex> g(a->mu);
  if (hipSetDevice(a->device) != hipSuccess) return -EIO;
  ++a->calls;
  a->h_out.assign((size_t)n * 4, NONE);
  *out = a->h_out.data();
  if (n == 0) return 0;
  uint2 packed[ADM_MAX_ZONES];
  for (uint32_t z = 0; z < n_zones; ++z) packed[z] = ad_pack_caps(caps[z]);
  int rc = ad_put(a, AD_CAPS, packed, (uint64_t)n_zones * sizeof(uint2));
  if (rc) return rc;
  ADCHK(hipStreamSynchronize(a->stream));  // `packed` is on this stack
  for (uint32_t lo = 0; lo < n;) {
    uint32_t hi = lo + 1;
    while (hi < n && hi - lo < a->pass_items && (uint64_t)offsets[hi + 1] - offsets[lo] <= ADM_PASS_BYTES) ++hi;
    if ((rc = ad_pass(a, mode, bytes, offsets, in_flags, zone, n_zones, lo, hi))) return rc;
    lo = hi;
  }
  a->items += n;
  a->bytes += offsets[n] - offsets[0];
  return 0;
}

uint32_t emqxgm_admit_reason(uint32_t mode, const uint32_t* rec) { return adm_reason(mode, rec[0]); }

int emqxgm_admit_tune(emqxgm_admit_t* a, const char* key, int64_t value) {
  if (!a || !key) return -EINVAL;
  std::lock_guard<std::mutex> g(a->mu);
  if (strcmp(key, "pass_items") == 0) {
    if (value < 1) return -EINVAL;
    a->pass_items = (uint64_t)value;
    return 0;
  }
  if (strcmp(key, "force_global") == 0) {
    a->force_global = value != 0;
    return 0;
  }
  if (strcmp(key, "byte_base") == 0) {
    if (value < 0 || value > 15) return -EINVAL;
    a->byte_base = (uint32_t)value;
    return 0;
  }
  if (strcmp(key, "timing") == 0) {
    if (value && !a->ev[1]) {
      if (hipSetDevice(a->device) != hipSuccess) return -EIO;
      for (hipEvent_t& e : a->ev)
        if (!e) ADCHK(hipEventCreate(&e));
    }
    a->timing = value != 0;
    a->kernel_ms = 0;
    return 0;
  }
  if (strcmp(key, "kernel_us") == 0) {
    const double us = a->kernel_ms * 1000.0;
    return us > 2147483647.0 ? 2147483647 : (int)us;
  }
  return -EINVAL;
}

int emqxgm_admit_stats(emqxgm_admit_t* a, uint64_t out[6]) {
  if (!a || !out) return -EINVAL;
  std::lock_guard<std::mutex> g(a->mu);
  out[0] = a->calls;
  out[1] = a->items;
  out[2] = a->bytes;
  out[3] = a->passes;
  out[4] = a->growths;
  out[5] = (uint64_t)(a->kernel_ms * 1000.0);
  return 0;
}

}  // extern "C"
