// share_dev_main.cpp -- the CPU gate of the shared-subscription device path (DESIGN.md 6b "Shared
// subscriptions"), built with ASan + UBSan by tests/test_share_dev_host.py: every line of k_share's
// device code (emqx_amd/csrc/gm_share.inc, included unchanged behind hip_shim.h) and every byte of
// host code that sizes or addresses a device buffer (emqx_amd/csrc/gm_share.cpp, included with
// GM_SHARE_EXACT_ALLOC on the fake HIP runtime, so each "device" array is a malloc of exactly the
// bytes in use and an access one byte past it hits a redzone) runs here before it runs on a GPU.
// launch_share runs a block the way the kernel body does: each phase function for lanes
// 0 .. WG - 1 in turn, phase by phase, which is what the __syncthreads() between them guarantee.
//
//   share_dev_main INPUT        the script of tests/share_cases.py, through the C-ABI
//   share_dev_main --structures what the C-ABI cannot build, fed to the kernel's phases directly:
//                               a chain that wraps the table's end, a deleted slot inside a chain,
//                               a key stored again after its delete, and out-of-range values, each
//                               refused before it is followed
// INPUT (text; byte strings in hex, "-" = empty): "hash_bits pass_names" (pass_names 0: the
// default), then operations until "E":
//   S group topic sub local | U group topic sub | D sub | G group strategy | C | T key value
//   R                         the refused calls, each of which must return -EINVAL
//   Q n                       emqxgm_share_pick of n requests "group topic hc ht draw state"
//   M group topic | K group topic | X     members, counter, stats
// Output: per Q one line "member status state count" per request; "M n handles..", "K counter",
// "STATS <the 12 values of emqxgm_share_stats>".
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <memory>
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

#define ALL_LANES for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)

// k_share's body for block b, the barriers turned into "every lane, then the next phase".
// tamper_pos != NONE: every lane's member position is set to it before the last phase.
void run_block(const ShareArgs& A, uint32_t b, uint32_t tamper_pos) {
  std::vector<ShLane> L(WG);
  std::unique_ptr<uint8_t[]> keys(A.stage ? new uint8_t[SH_STAGE_BYTES] : nullptr);
  if (A.stage) memset(keys.get(), 0xA5, SH_STAGE_BYTES);  // LDS starts undefined
  blockIdx.x = b;
  if (A.stage) ALL_LANES sh_ph_stage(A, keys.get());
  ALL_LANES sh_ph_hash(A, L[threadIdx.x], keys.get());
  ALL_LANES sh_ph_probe(A, L[threadIdx.x]);
  ALL_LANES sh_ph_header(A, L[threadIdx.x]);
  ALL_LANES sh_ph_decide(A, L[threadIdx.x]);
  if (tamper_pos != NONE) ALL_LANES L[threadIdx.x].d.pos = tamper_pos;
  ALL_LANES sh_ph_member(A, L[threadIdx.x]);
}

uint32_t g_tamper_pos = NONE;
}  // namespace

hipError_t launch_share(const ShareArgs& a, hipStream_t) {
  if (a.n == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((uint64_t)a.n + WG - 1) / WG);
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; ++b) run_block(a, b, g_tamper_pos);
  return hipSuccess;
}
}  // namespace gm

#define GM_SHARE_EXACT_ALLOC 1
#include "../../emqx_amd/csrc/gm_share.cpp"

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

// The refused calls; the table in force and what is pending stay as they are.
int refused(emqxgm_share_t* h) {
  const uint8_t t[3] = {'r', '/', 't'};
  const uint32_t big = 1u << 31;
  CHECK(emqxgm_share_subscribe(h, 1, t, 3, big, 1) == -EINVAL, "member handle 2^31");
  CHECK(emqxgm_share_subscribe(h, big, t, 3, 1, 1) == -EINVAL, "group handle 2^31");
  CHECK(emqxgm_share_subscribe(h, 1, nullptr, 3, 1, 1) == -EINVAL, "no topic bytes");
  CHECK(emqxgm_share_subscribe(h, 1, t, 3, 1, 2) == -EINVAL, "local flag 2");
  CHECK(emqxgm_share_unsubscribe(h, 1, t, 3, big) == -EINVAL, "unsubscribe of handle 2^31");
  CHECK(emqxgm_share_subscriber_down(h, 0xFFFFFFFFu) == -EINVAL, "down of handle 2^32 - 1");
  CHECK(emqxgm_share_set_strategy(h, 1, 7) == -EINVAL, "strategy 7");
  CHECK(emqxgm_share_set_strategy(h, big, 1) == -EINVAL, "strategy of group 2^31");
  // the other local flag, against a pending subscribe and against a committed one
  uint64_t st0[12], st1[12];
  CHECK(emqxgm_share_stats(h, st0) == 0, "stats");
  CHECK(emqxgm_share_subscribe(h, 0x7FFFFFF0u, t, 3, 5, 1) == 0, "a pending subscribe");
  CHECK(emqxgm_share_subscribe(h, 0x7FFFFFF0u, t, 3, 5, 0) == -EINVAL, "the other local flag, pending");
  CHECK(emqxgm_share_subscribe(h, 0x7FFFFFF0u, t, 3, 5, 1) == 0, "the same flag again");
  CHECK(emqxgm_share_unsubscribe(h, 0x7FFFFFF0u, t, 3, 5) == 0, "and out again");
  CHECK(emqxgm_share_subscribe(h, 0x7FFFFFF0u, t, 3, 5, 0) == 0, "after the unsubscribe either flag");
  CHECK(emqxgm_share_unsubscribe(h, 0x7FFFFFF0u, t, 3, 5) == 0, "and out");
  CHECK(emqxgm_share_stats(h, st1) == 0 && st1[11] == st0[11] + 5, "five mutations pending, none applied");
  const uint32_t g1[1] = {1}, gbig[1] = {big}, ko[2] = {0, 3}, desc[2] = {3, 0}, z[1] = {0};
  uint32_t out[4] = {7, 7, 7, 7};
  CHECK(emqxgm_share_pick(h, 1, gbig, t, ko, z, z, z, z, out) == -EINVAL, "pick of group 2^31");
  CHECK(emqxgm_share_pick(h, 1, g1, t, desc, z, z, z, z, out) == -EINVAL, "descending offsets");
  CHECK(emqxgm_share_pick(h, 1, g1, nullptr, ko, z, z, z, z, out) == -EINVAL, "no key bytes");
  CHECK(emqxgm_share_pick(h, 1, g1, t, ko, z, z, z, nullptr, out) == -EINVAL, "no state array");
  CHECK(out[0] == 7 && out[1] == 7 && out[2] == 7 && out[3] == 7, "a refused pick writes nothing");
  CHECK(emqxgm_share_pick(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0, "n == 0");
  CHECK(emqxgm_share_tune(h, "no_such_key", 1) == -EINVAL, "unknown tune key");
  CHECK(emqxgm_share_tune(h, "rebuild_load_pct", 51) == -EINVAL && emqxgm_share_tune(h, "rebuild_load_pct", 0) == -EINVAL,
        "load beyond 1/2");
  CHECK(emqxgm_share_tune(h, "rebuild_garbage_pct", 0) == -EINVAL, "garbage percent 0");
  CHECK(emqxgm_share_tune(h, "pass_names", 0) == -EINVAL, "pass_names 0");
  emqxgm_share_t* none = nullptr;
  CHECK(emqxgm_share_create(0, 17, &none) == -EINVAL && !none, "17 hash bits");
  return 0;
}

// ---- what the C-ABI cannot build ------------------------------------------------------------
struct Rig {
  std::vector<gm::ShSlot> tab;
  std::vector<uint32_t> pool, ko{0}, kg;
  std::vector<uint8_t> kb;
  uint64_t tag_mask = gm::sh_tag_mask(0);
  uint32_t add_key(uint32_t group, const std::string& t) {
    kb.insert(kb.end(), t.begin(), t.end());
    ko.push_back((uint32_t)kb.size());
    kg.push_back(group);
    return (uint32_t)kg.size() - 1;
  }
  uint32_t add_run(std::vector<uint32_t> m, uint32_t strategy) {
    return sh_append_run(pool, m.data(), (uint32_t)m.size(), strategy);
  }
};

struct Answer {
  uint32_t w[4];
  uint32_t err;
};

// One request (group, topic, draw) through the kernel's phases on exact-size copies of the rig.
Answer ask(const Rig& r, uint32_t group, const std::string& topic, uint32_t draw, uint32_t tamper_pos = gm::NONE) {
  std::vector<uint8_t> rbv(topic.begin(), topic.end());
  std::vector<uint32_t> rov{0, (uint32_t)topic.size()}, one{group}, dr{draw}, zero{0}, st{gm::NONE};
  AclExact<uint8_t> rb(rbv), kb(r.kb);
  AclExact<uint32_t> ro(rov), g(one), d(dr), z(zero), s(st), pool(r.pool), ko(r.ko), kg(r.kg);
  AclExact<gm::ShSlot> tab(r.tab);
  std::vector<uint4> outv(1, make_uint4(9, 9, 9, 9));
  AclExact<uint4> out(outv);
  std::vector<uint32_t> errv(1, 0);
  AclExact<uint32_t> err(errv);
  gm::ShareArgs A;
  A.group = g.p;
  A.rb = rb.p;
  A.ro = ro.p;
  A.hc = A.ht = z.p;
  A.draw = d.p;
  A.state = s.p;
  A.n = 1;
  A.tab = tab.p;
  A.tmask = r.tab.size() - 1;
  A.pool = pool.p;
  A.pool_words = r.pool.size();
  A.kb = kb.p;
  A.ko = ko.p;
  A.kg = kg.p;
  A.n_keys = (uint32_t)r.kg.size();
  A.tag_mask = r.tag_mask;
  A.out = out.p;
  A.err = err.p;
  gm::g_tamper_pos = tamper_pos;
  (void)gm::launch_share(A, nullptr);
  gm::g_tamper_pos = gm::NONE;
  return Answer{{out.p[0].x, out.p[0].y, out.p[0].z, out.p[0].w}, err.p[0]};
}

int structures() {
  using namespace gm;
  Rig r;
  r.tab.assign(8, ShSlot{SH_EMPTY, 0, 0});
  // three keys of group 1 whose home is the table's last slot
  std::vector<std::string> t;
  for (uint32_t i = 0; t.size() < 3 && i < 100000; ++i) {
    const std::string c = "w/" + std::to_string(i);
    if (sh_home(sh_key_tag(1, (const uint8_t*)c.data(), (uint32_t)c.size(), r.tag_mask), 7) == 7) t.push_back(c);
  }
  CHECK(t.size() == 3, "three keys with home 7");
  auto tag = [&](const std::string& c) { return sh_key_tag(1, (const uint8_t*)c.data(), (uint32_t)c.size(), r.tag_mask); };
  const uint32_t at[3] = {7, 0, 1};
  for (uint32_t k = 0; k < 3; ++k) {
    const uint32_t key = r.add_key(1, t[k]);
    r.tab[at[k]] = ShSlot{tag(t[k]), r.add_run({100 + k, (200 + k) | SH_LOCAL_BIT}, SH_RANDOM), key};
  }
  // a chain that wraps the table's end
  for (uint32_t k = 0; k < 3; ++k) {
    const Answer a = ask(r, 1, t[k], 1);
    CHECK(!a.err && a.w[0] == 200 + k && a.w[1] == SH_PICKED && a.w[3] == 2, "a key past the table's end");
    const Answer b = ask(r, 2, t[k], 1);
    CHECK(!b.err && b.w[0] == NONE && b.w[1] == SH_NO_SUBSCRIBERS && b.w[3] == 0, "the same bytes, another group");
  }
  // a deleted slot between a key's home and its slot
  r.tab[0].tag = SH_DELETED;
  CHECK(ask(r, 1, t[0], 0).w[0] == 100 && ask(r, 1, t[2], 0).w[0] == 102, "past a deleted slot");
  CHECK(ask(r, 1, t[1], 0).w[1] == SH_NO_SUBSCRIBERS, "the deleted key");
  // the key stored again after its delete, at the chain's end
  r.tab[2] = ShSlot{tag(t[1]), r.add_run({300}, SH_HASH_TOPIC), 1};
  {
    const Answer a = ask(r, 1, t[1], 5);
    CHECK(!a.err && a.w[0] == 300 && a.w[1] == SH_PICKED && a.w[3] == 1, "stored again after its delete");
  }
  // a full table without an empty slot ends the probe after mask + 1 steps
  {
    Rig f = r;
    for (ShSlot& s : f.tab)
      if (s.tag == SH_EMPTY) s.tag = SH_DELETED;
    const Answer a = ask(f, 1, "w/absent", 0);
    CHECK(!a.err && a.w[1] == SH_NO_SUBSCRIBERS, "a table with no empty slot");
  }
  // out-of-range values, each refused before it is followed (an access would hit a redzone)
  const uint32_t run7 = r.tab[7].run;
  struct Bad {
    const char* what;
    void (*make)(Rig&, uint32_t);
    uint32_t tamper;
  };
  const Bad bad[] = {
      {"a run that starts in the pool's last words", [](Rig& x, uint32_t) { x.tab[7].run = (uint32_t)x.pool.size() - 2; }, NONE},
      {"a run that starts past the pool", [](Rig& x, uint32_t) { x.tab[7].run = 0xFFFFFFF0u; }, NONE},
      {"members past the pool", [](Rig& x, uint32_t run) { x.pool[run] = 1000000; }, NONE},
      {"members near 2^32", [](Rig& x, uint32_t run) { x.pool[run] = 0xFFFFFFFFu; x.pool[run + 1] = 0xFFFFFFFFu; }, NONE},
      {"n_local > n_all", [](Rig& x, uint32_t run) { x.pool[run + 1] = 3; }, NONE},
      {"a strategy code out of range", [](Rig& x, uint32_t run) { x.pool[run + 2] = SH_STRATEGIES; }, NONE},
      {"a key index past the key array", [](Rig& x, uint32_t) { x.tab[7].key = (uint32_t)x.kg.size(); }, NONE},
      {"a key index of 2^32 - 1", [](Rig& x, uint32_t) { x.tab[7].key = 0xFFFFFFFFu; }, NONE},
      {"a member position past the run", [](Rig&, uint32_t) {}, SH_HDR_WORDS + 3},
      {"a member position near 2^32", [](Rig&, uint32_t) {}, 0xFFFFFFF0u},
  };
  for (const Bad& b : bad) {
    Rig x = r;
    b.make(x, run7);
    const Answer a = ask(x, 1, t[0], 1, b.tamper);
    CHECK(a.err == 1 && a.w[0] == NONE && a.w[1] == SH_MALFORMED, b.what);
  }
  CHECK(!ask(r, 1, t[0], 1).err, "the rig itself is well formed");
  puts("structures ok");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (strcmp(argv[1], "--structures") == 0) return structures();
  std::ifstream f(argv[1]);
  uint32_t hash_bits = 0;
  uint64_t pass_names = 0;
  f >> hash_bits >> pass_names;
  if (!f) return 2;
  emqxgm_share_t* h = nullptr;
  CHECK(emqxgm_share_create(0, hash_bits, &h) == 0, "create");
  if (pass_names) CHECK(emqxgm_share_tune(h, "pass_names", (int64_t)pass_names) == 0, "tune pass_names");
  CHECK(emqxgm_share_tune(h, "timing", 1) == 0 && emqxgm_share_tune(h, "kernel_us", 0) == 0, "tune timing");
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
    } else if (op == "D") {
      uint32_t sub;
      f >> sub;
      CHECK(emqxgm_share_subscriber_down(h, sub) == 0, "subscriber_down");
    } else if (op == "G") {
      uint32_t g, strat;
      f >> g >> strat;
      CHECK(emqxgm_share_set_strategy(h, g, strat) == 0, "set_strategy");
    } else if (op == "C") {
      CHECK(emqxgm_share_commit(h) == 0, "commit");
    } else if (op == "T") {
      std::string key;
      long long v;
      f >> key >> v;
      CHECK(emqxgm_share_tune(h, key.c_str(), v) == 0, "tune");
    } else if (op == "R") {
      if (refused(h)) return 1;
    } else if (op == "Q") {
      uint32_t n;
      f >> n;
      std::vector<uint8_t> kbv;
      std::vector<uint32_t> kov{0}, gv, hcv, htv, drv, stv;
      for (uint32_t i = 0; i < n; ++i) {
        uint32_t g, hc, ht, dr, st;
        std::string hex;
        f >> g >> hex >> hc >> ht >> dr >> st;
        gv.push_back(g);
        hcv.push_back(hc);
        htv.push_back(ht);
        drv.push_back(dr);
        stv.push_back(st);
        acl_unhex(hex, kbv, kov);
      }
      AclExact<uint8_t> kb(kbv);
      AclExact<uint32_t> ko(kov), g(gv), hc(hcv), ht(htv), dr(drv), st(stv);
      std::vector<uint32_t> fill((size_t)n * 4, 0xA5A5A5A5u);
      AclExact<uint32_t> out(fill);
      CHECK(emqxgm_share_pick(h, n, g.p, kb.p, ko.p, hc.p, ht.p, dr.p, st.p, out.p) == 0, "pick");
      for (uint32_t i = 0; i < n; ++i) printf("%u %u %u %u\n", out.p[4 * i], out.p[4 * i + 1], out.p[4 * i + 2], out.p[4 * i + 3]);
    } else if (op == "M" || op == "K") {
      uint32_t g;
      std::string hex;
      f >> g >> hex;
      const std::vector<uint8_t> tb = unhex(hex);
      AclExact<uint8_t> te(tb);
      if (op == "K") {
        uint32_t c = 0;
        CHECK(emqxgm_share_counter(h, g, te.p, (uint32_t)tb.size(), &c) == 0, "counter");
        printf("K %u\n", c);
      } else {
        uint32_t n = 0;
        CHECK(emqxgm_share_members(h, g, te.p, (uint32_t)tb.size(), nullptr, 0, &n) == 0, "members (count)");
        std::vector<uint32_t> fill(n, 0);
        AclExact<uint32_t> m(fill);
        uint32_t n2 = 0;
        CHECK(emqxgm_share_members(h, g, te.p, (uint32_t)tb.size(), m.p, n, &n2) == 0 && n2 == n, "members");
        printf("M %u", n);
        for (uint32_t i = 0; i < n; ++i) printf(" %u", m.p[i]);
        printf("\n");
      }
    } else if (op == "X") {
      uint64_t st[12];
      CHECK(emqxgm_share_stats(h, st) == 0, "stats");
      printf("STATS");
      for (int i = 0; i < 12; ++i) printf(" %llu", (unsigned long long)st[i]);
      printf("\n");
    } else {
      return 2;
    }
    if (!f) return 2;
  }
  CHECK(op == "E", "the script ends with E");
  emqxgm_share_destroy(h);
  return 0;
}
