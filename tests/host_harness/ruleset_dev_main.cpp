// ruleset_dev_main.cpp -- the CPU gate of the rule-set device path, built with
// ASan + UBSan by tests/test_ruleset_dev_host.py: every line of k_ruleset's device code
// (emqx_amd/csrc/gm_ruleset.inc, included unchanged behind hip_shim.h) and every byte of host
// code that sizes or addresses a device buffer (emqx_amd/csrc/gm_ruleset.cpp, included with
// GM_RULESET_EXACT_ALLOC on the fake HIP runtime, so each "device" array is a malloc of exactly
// the bytes in use and an access one byte past it hits a redzone) runs here before it runs on a
// GPU.  launch_ruleset runs a block the way the kernel body does: each phase function for lanes
// 0 .. WG - 1 in turn, phase by phase, which is what the __syncthreads() between them guarantee;
// the two LDS arrays are heap blocks of their exact size.  launch_ruleset_ptr is a CPU prefix
// sum.  Everything is driven through the C-ABI (emqxgm_ruleset_create / set / match / stats).
//
//   ruleset_dev_main INPUT
// INPUT (text; byte strings in hex, "-" = empty), the format of ruleset_main.cpp with a
// pass_names line:
//   hash_bits
//   pass_names            (0: the default)
//   n_rules, then per rule: n_filters, then per filter: "flag hex"
//   n_names, then one name per line
// Output: one line per name with its matching rules as reported, then
//   "STATS <records> <tiles> <filters> <rules> <candidates> <removed> <deep names> <visited>".
// After the match the program also checks that a malformed set (descending rule order, a rule
// out of range, an unknown flag) returns -EINVAL and leaves the answers as they were.
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
#include "ruleset_shim.h"

#include "../../emqx_amd/csrc/gm_kernels.h"
#include "../../emqx_amd/csrc/gm_match.h"
#include "../../emqx_amd/csrc/gm_ruleset_match.h"

namespace gm {
namespace {
#include "../../emqx_amd/csrc/gm_ruleset.inc"

#define ALL_LANES for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)

// k_ruleset<FILL>'s body for block b, the barriers turned into "every lane, then the next phase"
template <bool FILL>
void run_block(const RulesetArgs& A, uint32_t b) {
  std::unique_ptr<uint64_t[]> tok(new uint64_t[RS_MAX_LEVELS * WG]);
  std::unique_ptr<uint64_t[]> tile(new uint64_t[RS_TILE_WORDS]);
  memset(tok.get(), 0xA5, sizeof(uint64_t) * RS_MAX_LEVELS * WG);  // LDS starts undefined
  memset(tile.get(), 0xA5, sizeof(uint64_t) * RS_TILE_WORDS);
  uint64_t *s_tok = tok.get(), *s_tile = tile.get();
  std::vector<RsLane> L(WG);
  blockIdx.x = b;
  ALL_LANES rs_ph_tokenize<FILL>(A, L[threadIdx.x], s_tok);
  const uint32_t tiles = rs_n_tiles(A.total_words);
  for (uint32_t k = 0; k < tiles; ++k) {
    if (rs_tile_span(k, A.total_words) == 0) abort();
    ALL_LANES rs_ph_stage(A, k, s_tile);
    ALL_LANES rs_ph_walk<FILL>(A, L[threadIdx.x], s_tok, s_tile);
  }
  ALL_LANES rs_ph_finish<FILL>(A, L[threadIdx.x], s_tile);
  ALL_LANES rs_ph_counters<FILL>(A, s_tile);
}
}  // namespace

hipError_t launch_ruleset(const RulesetArgs& a, bool fill, hipStream_t) {
  if (a.n == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)(((uint64_t)a.n + WG - 1) / WG);
  gridDim.x = grid;
  for (uint32_t b = 0; b < grid; ++b) {
    if (fill)
      run_block<true>(a, b);
    else
      run_block<false>(a, b);
  }
  return hipSuccess;
}

hipError_t launch_ruleset_ptr(const uint32_t* cnt, uint32_t* row, uint32_t n, uint32_t*, uint32_t* total_dst,
                              hipStream_t) {
  uint32_t acc = 0;
  for (uint32_t i = 0; i < n; ++i) {
    row[i] = acc;
    acc += cnt[i];
  }
  row[n] = acc;
  if (total_dst) *total_dst = acc;
  return hipSuccess;
}
}  // namespace gm

#define GM_RULESET_EXACT_ALLOC 1
#include "../../emqx_amd/csrc/gm_ruleset.cpp"

static std::string unhex(const std::string& h) {
  std::string o;
  if (h == "-") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return o;
}

#define CHECK(c, what)                             \
  do {                                             \
    if (!(c)) {                                    \
      fprintf(stderr, "FAILED: %s\n", what);       \
      return 1;                                    \
    }                                              \
  } while (0)

static std::vector<std::vector<uint32_t>> rows_of(const emqxgm_ruleset_out& o) {
  std::vector<std::vector<uint32_t>> rows(o.n);
  for (uint32_t i = 0; i < o.n; ++i) rows[i].assign(o.rule + o.ptr[i], o.rule + o.ptr[i + 1]);
  return rows;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  uint32_t hash_bits = 0, n_rules = 0, n_names = 0;
  uint64_t pass_names = 0;
  in >> hash_bits >> pass_names >> n_rules;
  std::vector<uint8_t> fb, nb;
  std::vector<uint32_t> fo(1, 0), ff, fr, no(1, 0);
  for (uint32_t r = 0; r < n_rules; ++r) {
    uint32_t nf = 0;
    in >> nf;
    for (uint32_t k = 0; k < nf; ++k) {
      uint32_t flag;
      std::string hex;
      in >> flag >> hex;
      const std::string f = unhex(hex);
      fb.insert(fb.end(), f.begin(), f.end());
      fo.push_back((uint32_t)fb.size());
      ff.push_back(flag);
      fr.push_back(r);
    }
  }
  in >> n_names;
  for (uint32_t t = 0; t < n_names; ++t) {
    std::string hex;
    in >> hex;
    const std::string name = unhex(hex);
    nb.insert(nb.end(), name.begin(), name.end());
    no.push_back((uint32_t)nb.size());
  }
  if (!in) return 2;
  // exact-size copies of the inputs too: the C-ABI must not read past what it is given
  std::unique_ptr<uint8_t[]> nbx(new uint8_t[nb.size()]), fbx(new uint8_t[fb.size()]);
  if (!nb.empty()) memcpy(nbx.get(), nb.data(), nb.size());
  if (!fb.empty()) memcpy(fbx.get(), fb.data(), fb.size());
  const uint32_t nfil = (uint32_t)ff.size();

  emqxgm_ruleset_t* h = nullptr;
  CHECK(emqxgm_ruleset_create(0, hash_bits, &h) == 0, "create");
  CHECK(emqxgm_ruleset_tune(h, "counters", 1) == 0, "tune counters");
  if (pass_names) CHECK(emqxgm_ruleset_tune(h, "pass_names", (int64_t)pass_names) == 0, "tune pass_names");
  CHECK(emqxgm_ruleset_tune(h, "no_such_key", 1) == -EINVAL, "unknown tune key");
  CHECK(emqxgm_ruleset_tune(h, "timing", 1) == 0 && emqxgm_ruleset_tune(h, "count_us", 0) == 0, "tune timing");
  emqxgm_ruleset_out o;
  // before any set: the empty list
  CHECK(emqxgm_ruleset_match(h, nbx.get(), no.data(), n_names, &o) == 0, "match on the empty list");
  CHECK(o.n == n_names && o.n_ids == 0, "empty list gives empty rows");
  CHECK(emqxgm_ruleset_set(h, fbx.get(), fo.data(), ff.data(), fr.data(), nfil, n_rules) == 0, "set");
  CHECK(emqxgm_ruleset_match(h, nbx.get(), no.data(), n_names, &o) == 0, "match");
  CHECK(o.n == n_names && o.ptr[0] == 0 && o.ptr[n_names] == o.n_ids, "row pointers");
  const std::vector<std::vector<uint32_t>> rows = rows_of(o);
  uint64_t st[8];
  CHECK(emqxgm_ruleset_stats(h, st) == 0, "stats");

  // malformed lists: -EINVAL, and the list in force keeps answering
  if (nfil >= 1) {
    std::vector<uint32_t> bad = fr;
    bad[0] = n_rules;  // out of range
    CHECK(emqxgm_ruleset_set(h, fbx.get(), fo.data(), ff.data(), bad.data(), nfil, n_rules) == -EINVAL,
          "rule out of range");
    std::vector<uint32_t> bf = ff;
    bf[0] = 3;
    CHECK(emqxgm_ruleset_set(h, fbx.get(), fo.data(), bf.data(), fr.data(), nfil, n_rules) == -EINVAL,
          "unknown flag");
  }
  if (nfil >= 2 && fr[0] != fr[nfil - 1]) {
    std::vector<uint32_t> bad(fr.rbegin(), fr.rend());  // descending
    CHECK(emqxgm_ruleset_set(h, fbx.get(), fo.data(), ff.data(), bad.data(), nfil, n_rules) == -EINVAL,
          "descending rule order");
  }
  CHECK(emqxgm_ruleset_set(h, nullptr, nullptr, nullptr, nullptr, 0, 65537) == -EINVAL, "too many rules");
  CHECK(emqxgm_ruleset_match(h, nbx.get(), no.data(), n_names, &o) == 0, "match after refused sets");
  CHECK(rows_of(o) == rows, "a refused set leaves the answers as they were");
  CHECK(emqxgm_ruleset_match(h, nullptr, nullptr, 0, &o) == 0 && o.n == 0 && o.n_ids == 0 && o.ptr[0] == 0,
        "n == 0");
  emqxgm_ruleset_destroy(h);

  for (const auto& row : rows) {
    std::string line;
    for (uint32_t r : row) line += (line.empty() ? "" : " ") + std::to_string(r);
    puts(line.c_str());
  }
  printf("STATS");
  for (uint64_t v : st) printf(" %llu", (unsigned long long)v);
  printf("\n");
  return 0;
}
