// pubshare_dev_main.cpp -- the CPU gate of the pick inside the publish (DESIGN.md 6b "The pick
// inside the publish"), built with ASan + UBSan by tests/test_pubshare_dev_host.py: every line of
// k_pubshare's device code (emqx_amd/csrc/gm_pubshare.inc over gm_share.inc, included unchanged
// behind hip_shim.h) and the host code that drives it (emqx_amd/csrc/gm_pubshare.cpp's
// share_pub_pass and gm_share.cpp's counter steps, included with GM_SHARE_EXACT_ALLOC on the fake
// HIP runtime, so each "device" array is a malloc of exactly the bytes in use) runs here before it
// runs on a GPU.
// launch_pubshare runs a block the way the kernel body does: each phase function for lanes
// 0 .. WG - 1 in turn, phase by phase, which is what the __syncthreads() between them guarantee.
// The share tables are built by gm_share.cpp through the C-ABI; the fan-out's entry arrays and the
// index's string pool, which the engine would leave on the device, are written by this program in
// allocations of exactly the bytes in use.
//
//   pubshare_dev_main INPUT        the script of tests/pubshare_cases.py (input_text)
//   pubshare_dev_main --structures what the C-ABI cannot build, fed to the kernel's phases: each
//                                  must set the error word and follow nothing
// INPUT (text; byte strings in hex, "-" = empty): "hash_bits chunk" (chunk 0: a call is one pass,
// else passes of `chunk` topics), then operations until "E":
//   S group topic sub local | U group topic sub | G group strategy | C
//   P n n_filters has_states   then one line of n_filters filters, then per topic
//                              "hc ht draw n_entries n_states {filter dest}* {group filter value}*"
// Output: per P one line "member status state count" per entry, in entry order.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "hip_shim.h"

#include "../../emqx_amd/csrc/gm_kernels.h"
#include "../../emqx_amd/csrc/gm_share_match.h"
#include "acl_input.h"

namespace gm {
constexpr uint32_t WG = 256;  // gm_kernels.hip
namespace {
#include "../../emqx_amd/csrc/gm_share.inc"
#include "../../emqx_amd/csrc/gm_pubshare.inc"

#define ALL_LANES for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)

// k_pubshare's body for block b, the barriers turned into "every lane, then the next phase".
// tamper_pos != NONE: every lane's member position is set to it before the last phase.
void run_block(const PubShareArgs& A, uint32_t b, uint32_t tamper_pos) {
  std::vector<PsLane> L(WG);
  blockIdx.x = b;
  ALL_LANES ps_ph_owner(A, L[threadIdx.x]);
  ALL_LANES ps_ph_key(A, L[threadIdx.x]);
  ALL_LANES ps_ph_probe(A, L[threadIdx.x]);
  ALL_LANES ps_ph_header(A, L[threadIdx.x]);
  ALL_LANES ps_ph_decide(A, L[threadIdx.x]);
  if (tamper_pos != NONE) ALL_LANES L[threadIdx.x].s.d.pos = tamper_pos;
  ALL_LANES ps_ph_out(A, L[threadIdx.x]);
}

uint32_t g_tamper_pos = NONE;
}  // namespace

hipError_t launch_pubshare(const PubShareArgs& a, hipStream_t) {
  if (a.n_routes == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((uint64_t)a.n_routes + WG - 1) / WG);
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; ++b) run_block(a, b, g_tamper_pos);
  return hipSuccess;
}
// this program makes no emqxgm_share_pick call (tests/host_harness/share_dev_main.cpp does)
hipError_t launch_share(const ShareArgs&, hipStream_t) { return hipErrorUnknown; }
}  // namespace gm

#define GM_SHARE_EXACT_ALLOC 1
#include "../../emqx_amd/csrc/gm_share.cpp"
#include "../../emqx_amd/csrc/gm_pubshare.cpp"

// There is no engine in this program: it calls share_pub_pass with chunks of its own, and
// emqxgm_publish_shared_batch, which gm_pubshare.cpp also holds, is never called.
int gm_publish_hooked(emqxgm_t*, const uint8_t*, const uint32_t*, uint32_t, emqxgm_publish_out*, gm_pub_chunk_fn, void*) {
  return -ENOSYS;
}
int gm_engine_device(emqxgm_t*) { return -1; }

#define CHECK(c, what)                       \
  do {                                       \
    if (!(c)) {                              \
      fprintf(stderr, "FAILED: %s\n", what); \
      return 1;                              \
    }                                        \
  } while (0)

namespace {

std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> b;
  std::vector<uint32_t> o;
  acl_unhex(h, b, o);
  return b;
}

// ---- what the C-ABI cannot build ------------------------------------------------------------
// One publish pass of one topic with one entry, every array an exact-size copy.
struct Rig {
  std::vector<gm::ShSlot> tab;
  std::vector<uint32_t> pool, ko, kg;
  std::vector<uint8_t> kb;
  uint64_t tag_mask = 0;
  std::vector<uint32_t> rp{0, 1}, o_rf{0}, o_rd{0x80000001u};
  std::vector<uint8_t> fbytes{'k', '/', 'a', 'k', '/', 'b'};
  std::vector<uint64_t> foff{0, 3, 6};
  uint64_t n_filters = 2, pool_bytes = 6;
  uint32_t n_routes = 1;
};

struct Answer {
  uint32_t w[4];
  uint32_t err;
};

Answer ask(const Rig& r, uint32_t draw, uint32_t tamper_pos = gm::NONE) {
  std::vector<uint32_t> dr{draw}, zero{0};
  AclExact<uint8_t> kb(r.kb), fbytes(r.fbytes);
  AclExact<uint64_t> foff(r.foff);
  AclExact<uint32_t> rp(r.rp), o_rf(r.o_rf), o_rd(r.o_rd), d(dr), z(zero), pool(r.pool), ko(r.ko), kg(r.kg);
  AclExact<gm::ShSlot> tab(r.tab);
  std::vector<uint4> outv(1, make_uint4(9, 9, 9, 9));
  AclExact<uint4> out(outv);
  std::vector<uint32_t> errv(1, 0);
  AclExact<uint32_t> err(errv);
  gm::PubShareArgs A;
  A.tab = tab.p;
  A.tmask = r.tab.size() - 1;
  A.pool = pool.p;
  A.pool_words = r.pool.size();
  A.kb = kb.p;
  A.ko = ko.p;
  A.kg = kg.p;
  A.n_keys = (uint32_t)r.kg.size();
  A.tag_mask = r.tag_mask;
  A.rp = rp.p;
  A.o_rf = o_rf.p;
  A.o_rd = o_rd.p;
  A.n = 1;
  A.n_routes = r.n_routes;
  A.fbytes = fbytes.p;
  A.foff = foff.p;
  A.n_filters = r.n_filters;
  A.pool_bytes = r.pool_bytes;
  A.hc = A.ht = z.p;
  A.draw = d.p;
  A.out = out.p;
  A.err = err.p;
  gm::g_tamper_pos = tamper_pos;
  (void)gm::launch_pubshare(A, nullptr);
  gm::g_tamper_pos = gm::NONE;
  return Answer{{out.p[0].x, out.p[0].y, out.p[0].z, out.p[0].w}, err.p[0]};
}

int structures() {
  using namespace gm;
  // the tables of two keys, built by the library; their mirrors are what the device holds
  emqxgm_share_t* h = nullptr;
  CHECK(emqxgm_share_create(0, 0, &h) == 0, "create");
  const uint8_t ka[3] = {'k', '/', 'a'}, kb[3] = {'k', '/', 'b'};
  CHECK(emqxgm_share_set_strategy(h, 1, SH_RANDOM) == 0, "strategy");
  CHECK(emqxgm_share_subscribe(h, 1, ka, 3, 100, 0) == 0 && emqxgm_share_subscribe(h, 1, ka, 3, 101, 1) == 0 &&
            emqxgm_share_subscribe(h, 1, kb, 3, 200, 1) == 0 && emqxgm_share_commit(h) == 0,
        "two keys");
  Rig r;
  r.tab = h->tab.h;
  r.pool = h->pool.h;
  r.ko = h->ko.h;
  r.kg = h->kg.h;
  r.kb = h->kb.h;
  r.tag_mask = h->tag_mask;
  emqxgm_share_destroy(h);
  uint32_t slot_a = NONE;
  for (uint32_t i = 0; i < r.tab.size(); ++i)
    if (r.tab[i].tag != SH_EMPTY && r.tab[i].tag != SH_DELETED && r.ko[r.tab[i].key] == 0) slot_a = i;
  CHECK(slot_a != NONE, "the slot of (1, k/a)");
  const uint32_t run_a = r.tab[slot_a].run;
  {
    const Answer a = ask(r, 1);
    CHECK(!a.err && a.w[0] == 101 && a.w[1] == SH_PICKED && a.w[3] == 2, "the rig itself is well formed");
    Rig x = r;
    x.o_rf[0] = 1;
    const Answer b = ask(x, 1);
    CHECK(!b.err && b.w[0] == 200 && b.w[1] == SH_PICKED && b.w[3] == 1, "the second filter's key");
    x = r;
    x.o_rd[0] = 0x80000002u;
    const Answer c = ask(x, 1);
    CHECK(!c.err && c.w[0] == NONE && c.w[1] == SH_NO_SUBSCRIBERS && c.w[3] == 0, "the same bytes, another group");
    // a node entry answers NOT_SHARED and nothing of it is followed, not even its filter id
    x = r;
    x.o_rd[0] = 7;
    x.o_rf[0] = 0xFFFFFFFFu;
    const Answer d = ask(x, 1);
    CHECK(!d.err && d.w[0] == NONE && d.w[1] == SH_NOT_SHARED && d.w[2] == NONE && d.w[3] == 0, "a node entry");
  }
  struct Bad {
    const char* what;
    void (*make)(Rig&, uint32_t slot, uint32_t run);
    uint32_t tamper;
  };
  const Bad bad[] = {
      {"a filter id at n_filters", [](Rig& x, uint32_t, uint32_t) { x.o_rf[0] = 2; }, NONE},
      {"a filter id past n_filters", [](Rig& x, uint32_t, uint32_t) { x.o_rf[0] = 3; }, NONE},
      {"a filter id of 2^32 - 1", [](Rig& x, uint32_t, uint32_t) { x.o_rf[0] = 0xFFFFFFFFu; }, NONE},
      {"a decreasing foff", [](Rig& x, uint32_t, uint32_t) { x.foff[0] = 4; }, NONE},
      {"a string longer than 2^32 - 1", [](Rig& x, uint32_t, uint32_t) { x.foff[1] = 1ull << 33; }, NONE},
      {"a string past the string pool", [](Rig& x, uint32_t, uint32_t) { x.foff[1] = 7; }, NONE},
      {"rows that do not cover the entry", [](Rig& x, uint32_t, uint32_t) { x.rp[1] = 0; }, NONE},
      {"a key index past the key array", [](Rig& x, uint32_t s, uint32_t) { x.tab[s].key = (uint32_t)x.kg.size(); }, NONE},
      {"a key index of 2^32 - 1", [](Rig& x, uint32_t s, uint32_t) { x.tab[s].key = 0xFFFFFFFFu; }, NONE},
      {"a run that starts in the pool's last words", [](Rig& x, uint32_t s, uint32_t) { x.tab[s].run = (uint32_t)x.pool.size() - 2; }, NONE},
      {"a run that starts past the pool", [](Rig& x, uint32_t s, uint32_t) { x.tab[s].run = 0xFFFFFFF0u; }, NONE},
      {"members past the pool", [](Rig& x, uint32_t, uint32_t run) { x.pool[run] = 1000000; }, NONE},
      {"n_local > n_all", [](Rig& x, uint32_t, uint32_t run) { x.pool[run + 1] = 3; }, NONE},
      {"a strategy code out of range", [](Rig& x, uint32_t, uint32_t run) { x.pool[run + 2] = SH_STRATEGIES; }, NONE},
      {"a member position past the run", [](Rig&, uint32_t, uint32_t) {}, SH_HDR_WORDS + 3},
      {"a member position near 2^32", [](Rig&, uint32_t, uint32_t) {}, 0xFFFFFFF0u},
  };
  for (const Bad& b : bad) {
    Rig x = r;
    b.make(x, slot_a, run_a);
    const Answer a = ask(x, 1, b.tamper);
    CHECK(a.err == 1 && a.w[0] == NONE && a.w[1] == SH_MALFORMED, b.what);
  }
  puts("structures ok");
  return 0;
}

// One "P" of the script: the call in passes of `chunk` topics through share_pub_pass.
int publish(emqxgm_share_t* h, std::ifstream& f, uint32_t chunk) {
  uint32_t n, nf, has_states;
  f >> n >> nf >> has_states;
  std::vector<uint8_t> fbv;
  std::vector<uint32_t> fo32{0};
  for (uint32_t i = 0; i < nf; ++i) {
    std::string hex;
    f >> hex;
    acl_unhex(hex, fbv, fo32);
  }
  std::vector<uint64_t> fov(fo32.begin(), fo32.end());
  std::vector<uint32_t> hcv, htv, drv, rpv{0}, rfv, rdv, spv{0}, sgv, sfv, svv;
  for (uint32_t t = 0; t < n; ++t) {
    uint32_t hc, ht, dr, ne, ns;
    f >> hc >> ht >> dr >> ne >> ns;
    hcv.push_back(hc);
    htv.push_back(ht);
    drv.push_back(dr);
    for (uint32_t j = 0; j < ne; ++j) {
      uint32_t fid, d;
      f >> fid >> d;
      rfv.push_back(fid);
      rdv.push_back(d);
    }
    rpv.push_back((uint32_t)rfv.size());
    for (uint32_t j = 0; j < ns; ++j) {
      uint32_t g, fid, v;
      f >> g >> fid >> v;
      sgv.push_back(g);
      sfv.push_back(fid);
      svv.push_back(v);
    }
    spv.push_back((uint32_t)sgv.size());
  }
  if (!f) return 2;
  AclExact<uint8_t> fbytes(fbv);
  AclExact<uint64_t> foff(fov);
  AclExact<uint32_t> hc(hcv), ht(htv), dr(drv), sp(spv), sg(sgv), sf(sfv), sv(svv);
  gm::PubShareIn in;
  in.hc = hc.p;
  in.ht = ht.p;
  in.draw = dr.p;
  if (has_states) {
    in.st_ptr = sp.p;
    in.st_group = sg.p;
    in.st_filter = sf.p;
    in.st_value = sv.p;
  }
  std::lock_guard<std::mutex> g(h->mu);
  h->h_pub.clear();
  const uint32_t step = chunk ? chunk : std::max(n, 1u);
  for (uint32_t i0 = 0; i0 < n; i0 += step) {
    const uint32_t m = std::min(step, n - i0), e0 = rpv[i0], e1 = rpv[i0 + m];
    // the chunk's entry arrays as the fan-out leaves them: rows from 0, exactly the entries
    std::vector<uint32_t> rpc(m + 1);
    for (uint32_t i = 0; i <= m; ++i) rpc[i] = rpv[i0 + i] - e0;
    AclExact<uint32_t> rp(rpc), o_rf(std::vector<uint32_t>(rfv.begin() + e0, rfv.begin() + e1)),
        o_rd(std::vector<uint32_t>(rdv.begin() + e0, rdv.begin() + e1));
    const gm_pub_chunk c = {nullptr, i0, m, e1 - e0, e0, rp.p, o_rf.p, o_rd.p, fbytes.p, foff.p, nf, fbv.size()};
    CHECK(gm::share_pub_pass(h, c, in) == 0, "share_pub_pass");
  }
  CHECK(h->h_pub.size() == rfv.size() * 4, "four words per entry");
  for (size_t j = 0; j < rfv.size(); ++j)
    printf("%u %u %u %u\n", h->h_pub[4 * j], h->h_pub[4 * j + 1], h->h_pub[4 * j + 2], h->h_pub[4 * j + 3]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (strcmp(argv[1], "--structures") == 0) return structures();
  std::ifstream f(argv[1]);
  uint32_t hash_bits = 0, chunk = 0;
  f >> hash_bits >> chunk;
  if (!f) return 2;
  emqxgm_share_t* h = nullptr;
  CHECK(emqxgm_share_create(0, hash_bits, &h) == 0, "create");
  CHECK(emqxgm_share_tune(h, "timing", 1) == 0, "tune timing");
  std::string op;
  while (f >> op && op != "E") {
    if (op == "S" || op == "U") {
      uint32_t g, sub, local = 0;
      std::string hex;
      f >> g >> hex >> sub;
      if (op == "S") f >> local;
      const std::vector<uint8_t> tb = unhex(hex);
      AclExact<uint8_t> te(tb);
      if (op == "S") CHECK(emqxgm_share_subscribe(h, g, te.p, (uint32_t)tb.size(), sub, local) == 0, "subscribe");
      else CHECK(emqxgm_share_unsubscribe(h, g, te.p, (uint32_t)tb.size(), sub) == 0, "unsubscribe");
    } else if (op == "G") {
      uint32_t g, strat;
      f >> g >> strat;
      CHECK(emqxgm_share_set_strategy(h, g, strat) == 0, "set_strategy");
    } else if (op == "C") {
      CHECK(emqxgm_share_commit(h) == 0, "commit");
    } else if (op == "P") {
      if (int rc = publish(h, f, chunk)) return rc;
    } else {
      return 2;
    }
    if (!f) return 2;
  }
  CHECK(op == "E", "the script ends with E");
  emqxgm_share_destroy(h);
  return 0;
}
