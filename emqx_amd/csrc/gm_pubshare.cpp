// gm_pubshare.cpp -- emqxgm_publish_shared_batch (include/emqx_gpumatch.h): the publish pass of the
// engine (gm_engine.cpp gm_publish_hooked) with the shared-subscription pick of every aggre entry
// (k_pubshare, gm_pubshare.inc; share_pub_pass below, which ends in gm_share.cpp's counter steps)
// run per chunk before the engine lets its index epoch go.  DESIGN.md 6b "The pick
// inside the publish".
//
// Reference: emqx_broker:route/2 and do_route/2 (apps/emqx/src/emqx_broker.erl:262-282),
// emqx_shared_sub:dispatch/3 and pick/6 (emqx_shared_sub.erl:138-157, 309-379).
//
// Locks: the engine's (taken by gm_publish_hooked), then the share handle's, taken at the first
// chunk and held to the end of the call, so that no share commit runs beside a kernel or between
// the chunks of one call and the counter steps of a call are taken together.
#include <errno.h>

#include <mutex>

#include "../../include/emqx_gpumatch.h"
#include "gm_internal.h"
#include "gm_kernels.h"
#include "gm_share_handle.h"

using namespace gm;

#define SHCHK(expr)                        \
  do {                                     \
    if ((expr) != hipSuccess) return -EIO; \
  } while (0)

int gm::share_pub_pass(emqxgm_share* a, const gm_pub_chunk& c, const PubShareIn& in) {
  hipStream_t st = (hipStream_t)c.stream;
  const uint32_t m = c.m, nr = c.n_routes;
  a->h_pub.resize((size_t)(c.rbase + nr) * 4);
  if (nr == 0) return 0;
  int rc = 0;
  const uint32_t s0 = in.st_ptr ? in.st_ptr[c.i0] : 0u, ns = in.st_ptr ? in.st_ptr[c.i0 + m] - s0 : 0u;
  if (in.st_ptr) {
    a->h_off.resize((size_t)m + 1);  // st_ptr rebased to the chunk (every earlier pass was waited for)
    for (uint32_t i = 0; i <= m; ++i) a->h_off[i] = in.st_ptr[c.i0 + i] - s0;
  }
  // the copies go on the pass's stream, which the engine waits on before the next chunk: a scratch
  // slot is never regrown under a kernel
  auto put = [&](int slot, const uint32_t* src, uint64_t words) -> int {
    const int r = share_grow(a, slot, words * 4);
    if (r) return r;
    if (words) SHCHK(hipMemcpyAsync(a->sc[slot].p, src, words * 4, hipMemcpyHostToDevice, st));
    return 0;
  };
  if ((rc = put(SH_HC, in.hc + c.i0, m)) || (rc = put(SH_HT, in.ht + c.i0, m)) || (rc = put(SH_DR, in.draw + c.i0, m)) ||
      (in.st_ptr && ((rc = put(SH_SP, a->h_off.data(), (uint64_t)m + 1)) || (rc = put(SH_SG, in.st_group + s0, ns)) ||
                     (rc = put(SH_SF, in.st_filter + s0, ns)) || (rc = put(SH_SV, in.st_value + s0, ns)))) ||
      (rc = share_grow(a, SH_OUT, (uint64_t)nr * 16)) || (rc = share_grow(a, SH_CTL, SH_CTL_BYTES)))
    return rc;
  auto B = [&](int k) { return a->sc[k].p; };
  SHCHK(hipMemsetAsync(B(SH_CTL), 0, SH_CTL_BYTES, st));
  PubShareArgs A;
  share_tables(a, A);
  A.rp = c.rp;
  A.o_rf = c.o_rf;
  A.o_rd = c.o_rd;
  A.n = m;
  A.n_routes = nr;
  A.fbytes = c.fbytes;
  A.foff = c.foff;
  A.n_filters = c.n_filters;
  A.pool_bytes = c.pool_bytes;
  A.hc = (const uint32_t*)B(SH_HC);
  A.ht = (const uint32_t*)B(SH_HT);
  A.draw = (const uint32_t*)B(SH_DR);
  if (in.st_ptr) {
    A.st_ptr = (const uint32_t*)B(SH_SP);
    A.st_group = (const uint32_t*)B(SH_SG);
    A.st_filter = (const uint32_t*)B(SH_SF);
    A.st_value = (const uint32_t*)B(SH_SV);
  }
  A.out = (uint4*)B(SH_OUT);
  A.err = (uint32_t*)B(SH_CTL);
  const bool timed = a->timing && a->ev[1];
  if (timed) SHCHK(hipEventRecord(a->ev[0], st));
  SHCHK(launch_pubshare(A, st));
  if (timed) SHCHK(hipEventRecord(a->ev[1], st));
  uint32_t ctl[SH_CTL_BYTES / 4];
  uint32_t* o = a->h_pub.data() + (size_t)c.rbase * 4;
  SHCHK(hipMemcpyAsync(o, A.out, (size_t)nr * 16, hipMemcpyDeviceToHost, st));
  SHCHK(hipMemcpyAsync(ctl, B(SH_CTL), SH_CTL_BYTES, hipMemcpyDeviceToHost, st));
  SHCHK(hipStreamSynchronize(st));
  if (ctl[0] != 0) return -EIO;
  if (timed) {
    float ms = 0.f;
    SHCHK(hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
    a->kernel_ms += ms;
  }
  return share_counter_steps(a, o, nr);
}


namespace {

struct PubShareCall {
  emqxgm_share* s;
  PubShareIn in;
  std::unique_lock<std::mutex> lock;
};

int pubshare_chunk(void* ctx, const gm_pub_chunk* c) {
  PubShareCall& call = *(PubShareCall*)ctx;
  if (!call.lock.owns_lock()) {
    call.lock = std::unique_lock<std::mutex>(call.s->mu);
    if (call.s->broken) return -EIO;
    call.s->h_pub.clear();
  }
  return share_pub_pass(call.s, *c, call.in);
}

}  // namespace

extern "C" int emqxgm_publish_shared_batch(emqxgm_t* h, emqxgm_share_t* s, const uint8_t* bytes,
                                           const uint32_t* offsets, uint32_t n, const uint32_t* hc,
                                           const uint32_t* ht, const uint32_t* draw, const uint32_t* st_ptr,
                                           const uint32_t* st_group, const uint32_t* st_filter,
                                           const uint32_t* st_value, emqxgm_publish_shared_out* out) {
  if (!h || !s || !out || (n && (!offsets || !hc || !ht || !draw))) return -EINVAL;
  if (gm_engine_device(h) != s->device) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return -EINVAL;
  if (st_ptr) {
    for (uint32_t i = 0; i < n; ++i)
      if (st_ptr[i + 1] < st_ptr[i]) return -EINVAL;
    const uint32_t s0 = n ? st_ptr[0] : 0u, s1 = n ? st_ptr[n] : 0u;
    if (s1 > s0 && (!st_group || !st_filter || !st_value)) return -EINVAL;
    for (uint32_t i = s0; i < s1; ++i)
      if (st_group[i] >= (1u << 31)) return -EINVAL;
  }
  {
    std::lock_guard<std::mutex> g(s->mu);
    if (s->broken) return -EIO;
  }
  PubShareCall call;
  call.s = s;
  call.in.hc = hc;
  call.in.ht = ht;
  call.in.draw = draw;
  call.in.st_ptr = st_ptr;
  call.in.st_group = st_group;
  call.in.st_filter = st_filter;
  call.in.st_value = st_value;
  const int rc = gm_publish_hooked(h, bytes, offsets, n, &out->pub, pubshare_chunk, &call);
  if (rc) return rc;
  if (!call.lock.owns_lock()) {  // no topics: nothing was asked of the share handle
    std::lock_guard<std::mutex> g(s->mu);
    s->h_pub.clear();
  }
  out->share = s->h_pub.data();
  return 0;
}
