// admit_dev_main.cpp -- the CPU gate of the admission pass (DESIGN.md 6b "Admission"), built with
// ASan + UBSan by tests/test_admit_dev_host.py: every line of k_admit's device code
// (emqx_amd/csrc/gm_admit.inc and gm_admit_match.h, with stage_tile of gm_tok.inc, included
// unchanged behind hip_shim.h) and every byte of host code that sizes or addresses a device buffer
// (emqx_amd/csrc/gm_admit.cpp, included with GM_ADMIT_EXACT_ALLOC on the fake HIP runtime, so each
// "device" array is a malloc of exactly the bytes in use and an access one byte past it hits a
// redzone) runs here before it runs on a GPU.  launch_admit runs a block the way the kernel body
// does: each phase function for lanes 0 .. WG - 1 in turn, phase by phase, which is what the
// __syncthreads() between them guarantee.  The LDS tile is a heap block of exactly
// TILE_CHUNKS * 16 bytes, filled with '#' before every block (stale bytes past an item's end are
// the worst ones for the scan).  WG, TILE_BYTES and TILE_CHUNKS come from build/tok_consts.inc,
// which the test cuts out of gm_kernels.hip.
//
//   admit_dev_main INPUT      batches through the C-ABI; per batch
//                             "B mode force_global byte_base pass_items n_zones n has_flags has_zones",
//                             n_zones lines "levels qos retain wildcard shared exclusive", n lines
//                             "hex flags zone" ("-" = empty); "E" ends the input
//   admit_dev_main --refused  the refused calls and what the kernel itself refuses to follow
// Output: per item "w0 levels off share_len reason", per batch "END".
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "hip_shim.h"

#include "../../emqx_amd/csrc/gm_kernels.h"
#include "../../emqx_amd/csrc/gm_admit_match.h"
#include "acl_input.h"

namespace gm {
namespace {
#include "build/tok_consts.inc"
inline uint32_t lane_id() { return threadIdx.x & 63u; }
inline uint32_t mbcnt64(uint64_t) { return 0u; }
#include "../../emqx_amd/csrc/gm_tok.inc"
#include "../../emqx_amd/csrc/gm_admit.inc"

#define ALL_LANES for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)

uint32_t g_tiled_blocks = 0, g_global_blocks = 0;

// k_admit's body for block b, the barriers turned into "every lane, then the next phase".
void run_block(const AdmitArgs& A, uint32_t b) {
  std::vector<AdmLane> L(WG);
  uint4* s_buf = (uint4*)aligned_alloc(16, TILE_CHUNKS * 16);
  uint2* s_caps = (uint2*)malloc(ADM_MAX_ZONES * sizeof(uint2));
  memset(s_buf, '#', TILE_CHUNKS * 16);  // LDS starts undefined
  memset(s_caps, 0xA5, ADM_MAX_ZONES * sizeof(uint2));
  blockIdx.x = b;
  ALL_LANES adm_ph_stage(A, L[threadIdx.x], s_buf, s_caps);
  for (uint32_t i = 1; i < WG; ++i)
    if (L[i].tiled != L[0].tiled) abort();  // the lanes of a block decide alike
  ++(L[0].tiled ? g_tiled_blocks : g_global_blocks);
  ALL_LANES adm_ph_scan(A, L[threadIdx.x], s_buf, s_caps);
  ALL_LANES adm_ph_store(A, L[threadIdx.x]);
  threadIdx.x = 0;
  free(s_caps);
  free(s_buf);
}
}  // namespace

hipError_t launch_admit(const AdmitArgs& a, hipStream_t) {
  if (a.n == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((uint64_t)a.n + WG - 1) / WG);
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; ++b) run_block(a, b);
  return hipSuccess;
}
}  // namespace gm

#define GM_ADMIT_EXACT_ALLOC 1
#include "../../emqx_amd/csrc/gm_admit.cpp"

#define CHECK(c, what)                       \
  do {                                       \
    if (!(c)) {                              \
      fprintf(stderr, "FAILED: %s\n", what); \
      return 1;                              \
    }                                        \
  } while (0)

namespace {

int refused() {
  emqxgm_admit_t* h = nullptr;
  CHECK(emqxgm_admit_create(0, &h) == 0, "create");
  emqxgm_admit_caps c{65535, 2, 1, 1, 1, 0, {0, 0, 0}};
  const uint8_t t[3] = {'a', '/', 'b'};
  const uint32_t up[2] = {0, 3}, down[3] = {0, 3, 2};
  const uint8_t z1[1] = {1};
  const uint32_t* out = nullptr;
  CHECK(emqxgm_admit_batch(h, 2, t, up, 1, nullptr, nullptr, &c, 1, &out) == -EINVAL, "mode 2");
  CHECK(emqxgm_admit_batch(h, 0, t, down, 2, nullptr, nullptr, &c, 1, &out) == -EINVAL, "decreasing offsets");
  CHECK(emqxgm_admit_batch(h, 0, t, up, 1, nullptr, z1, &c, 1, &out) == -EINVAL, "zone 1 of 1");
  CHECK(emqxgm_admit_batch(h, 0, t, up, 1, nullptr, nullptr, nullptr, 1, &out) == -EINVAL, "no caps");
  CHECK(emqxgm_admit_batch(h, 0, t, up, 1, nullptr, nullptr, &c, 0, &out) == -EINVAL, "0 zones");
  CHECK(emqxgm_admit_batch(h, 0, t, up, 1, nullptr, nullptr, &c, 257, &out) == -EINVAL, "257 zones");
  CHECK(emqxgm_admit_batch(h, 0, nullptr, up, 1, nullptr, nullptr, &c, 1, &out) == -EINVAL, "no bytes");
  CHECK(emqxgm_admit_batch(h, 0, t, up, 1, nullptr, nullptr, &c, 1, nullptr) == -EINVAL, "no out");
  emqxgm_admit_caps q3 = c;
  q3.max_qos_allowed = 3;
  CHECK(emqxgm_admit_batch(h, 0, t, up, 1, nullptr, nullptr, &q3, 1, &out) == -EINVAL, "max_qos_allowed 3");
  CHECK(emqxgm_admit_batch(h, 0, nullptr, nullptr, 0, nullptr, nullptr, &c, 1, &out) == 0, "n == 0");
  CHECK(emqxgm_admit_tune(h, "no_such_key", 1) == -EINVAL, "unknown tune key");
  CHECK(emqxgm_admit_tune(h, "byte_base", 16) == -EINVAL, "byte_base 16");
  CHECK(emqxgm_admit_tune(h, "pass_items", 0) == -EINVAL, "pass_items 0");
  CHECK(emqxgm_admit_batch(h, 0, t, up, 1, nullptr, nullptr, &c, 1, &out) == 0 && out && out[0] == 0 && out[1] == 2,
        "the handle still answers");
  emqxgm_admit_destroy(h);
  // what the C-ABI refuses before a launch, fed to the kernel's phases directly: each sets the
  // error word, is not followed (an access would hit a redzone) and leaves a record of all ones
  struct Bad {
    const char* what;
    std::vector<uint32_t> off;
    std::vector<uint8_t> zone;
  };
  const Bad bad[] = {{"an offset past the bytes", {0, 3, 4000}, {0, 0}},
                     {"a decreasing offset", {0, 3, 1}, {0, 0}},
                     {"offsets near 2^32", {0, 0xFFFFFFF0u, 0xFFFFFFF8u}, {0, 0}},
                     {"a first offset past the bytes", {100, 101, 102}, {0, 0}},
                     {"a zone past the table", {0, 1, 3}, {0, 1}}};
  for (int fg = 0; fg < 2; ++fg)
    for (const Bad& b : bad) {
      std::vector<uint8_t> bv(32, '/');
      uint8_t* bytes = (uint8_t*)aligned_alloc(16, 32);
      memcpy(bytes, bv.data(), 32);
      memcpy(bytes, t, 3);
      AclExact<uint32_t> off(b.off);
      AclExact<uint8_t> zone(b.zone);
      std::vector<uint2> cv(1, make_uint2(65535, 2));
      AclExact<uint2> caps(cv);
      std::vector<uint4> ov(2, make_uint4(9, 9, 9, 9));
      AclExact<uint4> o(ov);
      std::vector<uint32_t> ev(1, 0);
      AclExact<uint32_t> err(ev);
      gm::AdmitArgs A;
      A.bytes = bytes;
      A.off = off.p;
      A.n = 2;
      A.nbytes = 3;
      A.mode = 1;
      A.zone = zone.p;
      A.caps = caps.p;
      A.n_zones = 1;
      A.out = o.p;
      A.err = err.p;
      A.force_global = fg != 0;
      (void)gm::launch_admit(A, nullptr);
      const bool ones = (o.p[0].x == gm::NONE && o.p[0].y == gm::NONE) || (o.p[1].x == gm::NONE && o.p[1].y == gm::NONE);
      free(bytes);
      CHECK(err.p[0] == 1 && ones, b.what);
    }
  puts("refused ok");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (strcmp(argv[1], "--refused") == 0) return refused();
  std::ifstream f(argv[1]);
  emqxgm_admit_t* h = nullptr;
  CHECK(emqxgm_admit_create(0, &h) == 0, "create");
  CHECK(emqxgm_admit_tune(h, "timing", 1) == 0 && emqxgm_admit_tune(h, "kernel_us", 0) == 0, "tune timing");
  std::string op;
  while (f >> op && op != "E") {
    CHECK(op == "B", "a batch starts with B");
    uint32_t mode, fg, base, n_zones, n, has_flags, has_zones;
    uint64_t pass_items;
    f >> mode >> fg >> base >> pass_items >> n_zones >> n >> has_flags >> has_zones;
    CHECK((bool)f && n_zones >= 1 && n_zones <= 256, "batch header");
    std::vector<emqxgm_admit_caps> cv(n_zones);
    for (emqxgm_admit_caps& c : cv) {
      uint32_t lv, q, r, w, s, x;
      f >> lv >> q >> r >> w >> s >> x;
      c = emqxgm_admit_caps{lv, (uint8_t)q, (uint8_t)r, (uint8_t)w, (uint8_t)s, (uint8_t)x, {0, 0, 0}};
    }
    std::vector<uint8_t> bv, fv, zv;
    std::vector<uint32_t> ov{0};
    for (uint32_t i = 0; i < n; ++i) {
      std::string hex;
      uint32_t fl, zn;
      f >> hex >> fl >> zn;
      acl_unhex(hex, bv, ov);
      fv.push_back((uint8_t)fl);
      zv.push_back((uint8_t)zn);
    }
    CHECK((bool)f, "batch items");
    AclExact<uint8_t> bytes(bv), flags(fv), zones(zv);
    AclExact<uint32_t> off(ov);
    AclExact<emqxgm_admit_caps> caps(cv);
    CHECK(emqxgm_admit_tune(h, "force_global", fg) == 0 && emqxgm_admit_tune(h, "byte_base", base) == 0 &&
              emqxgm_admit_tune(h, "pass_items", pass_items ? (int64_t)pass_items : (1ll << 22)) == 0,
          "tune");
    const uint32_t* out = nullptr;
    gm::g_tiled_blocks = gm::g_global_blocks = 0;
    CHECK(emqxgm_admit_batch(h, mode, bytes.p, off.p, n, has_flags ? flags.p : nullptr, has_zones ? zones.p : nullptr,
                             caps.p, n_zones, &out) == 0,
          "admit_batch");
    CHECK(!fg || gm::g_tiled_blocks == 0, "force_global stages no tile");
    for (uint32_t i = 0; i < n; ++i)
      printf("%u %u %u %u %u\n", out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3],
             emqxgm_admit_reason(mode, out + 4 * i));
    printf("END %u %u\n", gm::g_tiled_blocks, gm::g_global_blocks);
  }
  CHECK(op == "E", "the input ends with E");
  uint64_t st[6];
  CHECK(emqxgm_admit_stats(h, st) == 0 && st[0] > 0, "stats");
  emqxgm_admit_destroy(h);
  return 0;
}
