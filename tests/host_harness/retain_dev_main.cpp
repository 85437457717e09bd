// retain_dev_main.cpp -- the CPU gate of the retained-topic store, built with
// ASan + UBSan by tests/test_retain_dev_host.py as a stand-alone program: the device code of
// emqx_amd/csrc/gm_retain.inc (included unchanged behind hip_shim.h) and the host code behind
// the emqxgm_retain_* C-ABI (emqx_amd/csrc/gm_retain.cpp, included with GM_RETAIN_EXACT_ALLOC
// on the fake HIP runtime below, so each "device" array is a malloc of exactly the bytes in use
// and an access one byte past it hits a redzone) run here before they run on a GPU.
//  * launch_retain_walk, launch_retain_ptr, launch_retain_win: the kernels whole, lane by lane
//    (their lanes are independent).
//  * launch_retain_runs: k_retain_runs unchanged, 64 lanes per wave in two rounds -- the first
//    records every lane's vote at each __ballot, the second runs the lanes again with the
//    ballots of all 64 (the loop trip counts are the same in every lane of a wave).
//  * launch_retain_runs_win: the per-lane functions rw_open / rw_live / rw_put for lanes
//    0 .. 63 in turn, phase by phase, with the ballot computed between the phases, in the loop
//    of k_retain_runs_win.
//  * launch_scan is a CPU prefix sum, launch_patch a memcpy.
//
//   retain_dev_main FILE      (FILE "-": standard input; one answer per command, flushed)
// Commands (byte strings in hex, "-" = empty, "*" = NULL), answers in ():
//   indices K, then K lines "m p1 .. pm"        (K rc)
//   tune KEY VALUE | delete HEX | clean | commit  (K rc)
//   store HEX EXPIRY TS                         (S rc id)
//   size (Z n) | read HEX NOW (D rc) | stats (T full delta base_topics delta_topics)
//   match NOW N, then N lines HEX               (E rc | N lines "R hex.." then "N n_ids")
//   limit NOW N, then N lines "HEX LIMIT SLOT"  (E rc | N lines "R hex..", N lines
//                                                "C gen phase at", then "N n_ids")
//   setcur SLOT GEN PHASE AT                    (K 0)      cursors live in numbered slots
//   clear NOW | delmatch HEX | page HEX|* PAGE LIMIT NOW   (I rc hex..)
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "hip_shim.h"

// ---- the fake HIP runtime: "device" memory is malloc'ed, poisoned, exactly as large as asked
struct ihipStream_t {
  int dummy;
};
hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
const char* hipGetErrorString(hipError_t) { return "fake hip error"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t bytes) {
  *p = malloc(bytes ? bytes : 1);
  if (*p && bytes) memset(*p, 0xA5, bytes);  // device memory starts undefined
  return *p ? hipSuccess : hipErrorUnknown;
}
hipError_t hipFree(void* p) {
  free(p);
  return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
  if (n) memmove(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t) {
  return hipMemcpy(d, s, n, k);
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
  if (n) memset(d, v, n);
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = new ihipStream_t();
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  delete s;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
struct ihipEvent_t {
  int dummy;
};
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = new ihipEvent_t();
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  delete e;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 0.f;
  return hipSuccess;
}

// ---- the wave's ballot for kernels run whole (k_retain_runs): record, then replay
namespace {
enum { BALLOT_OWN, BALLOT_RECORD, BALLOT_REPLAY } g_ballot_mode = BALLOT_OWN;
std::vector<uint64_t> g_votes;
size_t g_vote_at = 0;

uint64_t rt_ballot(int v) {
  const uint32_t lane = threadIdx.x & 63;
  if (g_ballot_mode == BALLOT_RECORD) {
    if (g_vote_at == g_votes.size()) g_votes.push_back(0);
    g_votes[g_vote_at++] |= (uint64_t)(v ? 1 : 0) << lane;
    return 0;
  }
  if (g_ballot_mode == BALLOT_REPLAY) {
    if (g_vote_at >= g_votes.size()) abort();  // the lanes of a wave disagree on the trip count
    return g_votes[g_vote_at++];
  }
  return v ? 1ull << lane : 0ull;
}
unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
  const unsigned long long old = *p;
  *p = old + v;
  return old;
}
}  // namespace
#define __ballot rt_ballot

#include "../../emqx_amd/csrc/gm_common.h"
#include "../../emqx_amd/csrc/gm_kernels.h"

namespace gm {
constexpr uint32_t WG = 256;  // gm_kernels.hip
namespace {
#include "../../emqx_amd/csrc/gm_retain.inc"

// a small grid, so that the waves' stride loops over the runs take several rounds
uint32_t small_grid(uint64_t lanes) {
  const uint64_t b = (lanes + WG - 1) / WG;
  return (uint32_t)(b < 1 ? 1 : (b > 3 ? 3 : b));
}

template <class F>
void each_lane(uint32_t grid, F f) {
  gridDim.x = grid;
  for (blockIdx.x = 0; blockIdx.x < grid; ++blockIdx.x)
    for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x) f();
}
}  // namespace

uint32_t scan_tmp_words(uint32_t) { return 1; }

hipError_t launch_scan(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t*, uint32_t* total_dst,
                       hipStream_t) {
  uint32_t acc = 0;
  for (uint32_t i = 0; i < n; ++i) {
    out[i] = acc;
    acc += in[i];
  }
  out[n] = acc;
  if (total_dst) *total_dst = acc;
  return hipSuccess;
}

hipError_t launch_patch(const PatchEnt* ents, uint32_t n, const uint32_t* src, hipStream_t) {
  for (uint32_t e = 0; e < n; ++e) memcpy((void*)(uintptr_t)ents[e].dst, src + ents[e].s, 4u * ents[e].w);
  return hipSuccess;
}

hipError_t launch_retain_walk(const RetainDev& st, const uint8_t* fb, const uint32_t* fo, uint32_t n,
                              const uint8_t* tail, uint4* frames, uint32_t max_plus, uint32_t* cnt,
                              const uint32_t* cnt_in, const uint32_t* rbase, const uint32_t* rshift,
                              bool delta, uint2* runs, bool fill, hipStream_t) {
  if (n == 0) return hipSuccess;
  RetainArgs a{fb, fo, n, st.rn, st.redge, st.rmask, st.rch, st.rw, st.pool, tail, frames, max_plus,
               cnt, cnt_in, rbase, rshift, delta ? RUN_DELTA : 0u, runs};
  each_lane((n + WG - 1) / WG, [&] {
    if (fill)
      k_retain_walk<true>(a);
    else
      k_retain_walk<false>(a);
  });
  return hipSuccess;
}

hipError_t launch_retain_ptr(const uint32_t* rbase, const uint32_t* abase, uint32_t n, uint32_t* ptr,
                             hipStream_t) {
  each_lane(n / WG + 1, [&] { k_retain_ptr(rbase, abase, n, ptr); });
  return hipSuccess;
}

hipError_t launch_retain_win(const uint32_t* rbase, const uint32_t* abase, const uint32_t* limit,
                             uint32_t n, uint32_t* tot, uint32_t* win, hipStream_t) {
  if (n == 0) return hipSuccess;
  each_lane((n + WG - 1) / WG, [&] { k_retain_win(rbase, abase, limit, n, tot, win); });
  return hipSuccess;
}

hipError_t launch_retain_runs(const RetainDev& base, const RetainDev& delta, const uint2* runs,
                              uint32_t nr, uint64_t now, uint32_t* acnt, const uint32_t* abase,
                              uint32_t* out, unsigned long long* total, bool fill, hipStream_t) {
  if (nr == 0) return hipSuccess;
  RunArgs a{runs, nr, base.sexp, base.sid, delta.sexp, delta.sid, now, acnt, abase, out, total};
  // the recording round: the count pass (it casts the same votes) into scratch of its own
  std::vector<uint32_t> scratch(nr);
  unsigned long long scratch_total = 0;
  RunArgs rec = a;
  rec.acnt = scratch.data();
  rec.total = &scratch_total;
  const uint32_t grid = small_grid((uint64_t)nr * 64);
  gridDim.x = grid;
  for (blockIdx.x = 0; blockIdx.x < grid; ++blockIdx.x)
    for (uint32_t wave = 0; wave < WG / 64; ++wave) {
      g_votes.clear();
      g_ballot_mode = BALLOT_RECORD;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        threadIdx.x = wave * 64 + lane;
        g_vote_at = 0;
        k_retain_runs<false>(rec);
      }
      g_ballot_mode = BALLOT_REPLAY;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        threadIdx.x = wave * 64 + lane;
        g_vote_at = 0;
        if (fill)
          k_retain_runs<true>(a);
        else
          k_retain_runs<false>(a);
        if (g_vote_at != g_votes.size()) abort();
      }
      g_ballot_mode = BALLOT_OWN;
    }
  return hipSuccess;
}

namespace {
// k_retain_runs_win<FILL>'s body for run r: each per-lane function for lanes 0 .. 63 in turn,
// the ballot between them
template <bool FILL>
void run_wave_win(const RunWinArgs& A, uint32_t r) {
  RwRun R[64];
  for (uint32_t lane = 0; lane < 64; ++lane) R[lane] = rw_open<FILL>(A, r);
  for (uint32_t lane = 1; lane < 64; ++lane)
    if (memcmp(&R[lane].f, &R[0].f, sizeof(uint32_t)) != 0 || R[lane].lo != R[0].lo) abort();
  if (FILL && R[0].rank >= R[0].w) return;
  uint32_t c = 0;
  for (uint32_t b = R[0].lo; b < R[0].hi; b += 64) {
    bool live[64];
    uint64_t m = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      live[lane] = rw_live(R[lane], b + lane, A.now);
      m |= (uint64_t)live[lane] << lane;
    }
    if (FILL)
      for (uint32_t lane = 0; lane < 64; ++lane)
        rw_put(A, R[lane], b + lane, live[lane],
               R[lane].rank + c + __builtin_popcountll(m & ((1ull << lane) - 1)));
    c += __builtin_popcountll(m);
    if (FILL && R[0].rank + c >= R[0].w) break;
  }
  if (!FILL) {
    A.acnt[r] = c;
    *A.total += c;
  }
}
}  // namespace

hipError_t launch_retain_runs_win(const RetainDev& base, const RetainDev& delta, const uint2* runs,
                                  uint32_t nr, uint64_t now, const RetainWin& w, bool fill,
                                  hipStream_t) {
  if (nr == 0 || w.n == 0) return hipSuccess;
  RunWinArgs a{runs,       nr,        w.rbase, w.n,    w.rb,    w.rd,  base.sexp, base.sid,
               delta.sexp, delta.sid, now,     w.acnt, w.abase, w.win, w.wptr,    w.out,
               w.last,     w.total};
  for (uint32_t r = 0; r < nr; ++r) {
    if (fill)
      run_wave_win<true>(a, r);
    else
      run_wave_win<false>(a, r);
  }
  return hipSuccess;
}
}  // namespace gm

#undef __ballot
#define GM_RETAIN_EXACT_ALLOC 1
#include "../../emqx_amd/csrc/gm_retain.cpp"

static std::string unhex(const std::string& h) {
  std::string o;
  if (h == "-" || h == "*") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return o;
}

static std::string hex_of(const uint8_t* p, uint32_t n) {
  static const char* d = "0123456789abcdef";
  std::string o;
  for (uint32_t i = 0; i < n; ++i) {
    o.push_back(d[p[i] >> 4]);
    o.push_back(d[p[i] & 15]);
  }
  return n ? o : "-";
}

static std::string topic_hex(emqxgm_retain_t* h, uint32_t id) {
  const uint8_t* p = nullptr;
  uint32_t n = 0;
  if (emqxgm_retain_topic(h, id, &p, &n) != 0) return "?";
  return hex_of(p, n);
}

// exact-size copy of a byte string: the C-ABI must not read past what it is given
struct Exact {
  uint8_t* p;
  explicit Exact(const std::string& s) : p(new uint8_t[s.size()]) {
    if (!s.empty()) memcpy(p, s.data(), s.size());
  }
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
};

static void print_rows(emqxgm_retain_t* h, const emqxgm_retain_out& o) {
  for (uint32_t i = 0; i < o.n; ++i) {
    std::string line = "R";
    for (uint64_t k = o.ptr[i]; k < o.ptr[i + 1]; ++k) line += " " + topic_hex(h, o.id[k]);
    puts(line.c_str());
  }
}

static void print_ids(emqxgm_retain_t* h, int rc, const uint32_t* ids, uint64_t n) {
  std::string line = "I " + std::to_string(rc);
  for (uint64_t k = 0; rc == 0 && k < n; ++k) line += " " + topic_hex(h, ids[k]);
  puts(line.c_str());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream file;
  const bool use_stdin = strcmp(argv[1], "-") == 0;
  if (!use_stdin) file.open(argv[1]);
  std::istream& in = use_stdin ? std::cin : file;
  emqxgm_retain_t* h = nullptr;
  if (emqxgm_retain_create(0, &h) != 0) return 1;
  std::map<uint32_t, emqxgm_retain_cursor> slots;
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "indices") {
      uint32_t k = 0;
      in >> k;
      std::vector<uint32_t> pos, off(1, 0);
      for (uint32_t i = 0; i < k; ++i) {
        uint32_t m = 0, p = 0;
        in >> m;
        for (uint32_t j = 0; j < m; ++j) {
          in >> p;
          pos.push_back(p);
        }
        off.push_back((uint32_t)pos.size());
      }
      printf("K %d\n", emqxgm_retain_set_indices(h, pos.data(), off.data(), k));
    } else if (cmd == "tune") {
      std::string key;
      long long v = 0;
      in >> key >> v;
      printf("K %d\n", emqxgm_retain_tune(h, key.c_str(), v));
    } else if (cmd == "store") {
      std::string hx;
      unsigned long long e = 0, ts = 0;
      in >> hx >> e >> ts;
      const std::string t = unhex(hx);
      Exact x(t);
      uint32_t id = 0xFFFFFFFFu;
      const int rc = emqxgm_retain_store_ts(h, x.p, (uint32_t)t.size(), e, ts, &id);
      printf("S %d %u\n", rc, id);
    } else if (cmd == "delete") {
      std::string hx;
      in >> hx;
      const std::string t = unhex(hx);
      Exact x(t);
      printf("K %d\n", emqxgm_retain_delete(h, x.p, (uint32_t)t.size()));
    } else if (cmd == "clean") {
      printf("K %d\n", emqxgm_retain_clean(h));
    } else if (cmd == "commit") {
      printf("K %d\n", emqxgm_retain_commit(h));
    } else if (cmd == "size") {
      uint64_t n = 0;
      emqxgm_retain_size(h, &n);
      printf("Z %llu\n", (unsigned long long)n);
    } else if (cmd == "read") {
      std::string hx;
      unsigned long long now = 0;
      in >> hx >> now;
      const std::string t = unhex(hx);
      Exact x(t);
      uint32_t id = 0;
      printf("D %d\n", emqxgm_retain_read(h, x.p, (uint32_t)t.size(), now, &id));
    } else if (cmd == "stats") {
      uint64_t st[4] = {0, 0, 0, 0};
      emqxgm_retain_stats(h, st);
      printf("T %llu %llu %llu %llu\n", (unsigned long long)st[0], (unsigned long long)st[1],
             (unsigned long long)st[2], (unsigned long long)st[3]);
    } else if (cmd == "match" || cmd == "limit") {
      const bool lim = cmd == "limit";
      unsigned long long now = 0;
      uint32_t n = 0;
      in >> now >> n;
      std::string bytes;
      std::vector<uint32_t> off(1, 0), limits, slot_of;
      for (uint32_t i = 0; i < n; ++i) {
        std::string hx;
        in >> hx;
        bytes += unhex(hx);
        off.push_back((uint32_t)bytes.size());
        if (lim) {
          uint32_t l = 0, sl = 0;
          in >> l >> sl;
          limits.push_back(l);
          slot_of.push_back(sl);
        }
      }
      Exact x(bytes);
      emqxgm_retain_out o;
      int rc;
      // exact-size arrays for the limits and the cursors too
      std::vector<uint32_t> lim_x(limits);
      std::vector<emqxgm_retain_cursor> cur;
      if (lim) {
        for (uint32_t i = 0; i < n; ++i) cur.push_back(slots[slot_of[i]]);  // (a new slot is zeroed)
        cur.shrink_to_fit();
        lim_x.shrink_to_fit();
        rc = emqxgm_retain_match_limit(h, x.p, off.data(), n, now, lim_x.data(), cur.data(), &o);
      } else {
        rc = emqxgm_retain_match(h, x.p, off.data(), n, now, &o);
      }
      if (rc != 0) {
        printf("E %d\n", rc);
      } else {
        if (o.n != n || o.ptr[0] != 0 || o.ptr[n] != o.n_ids) return 1;
        print_rows(h, o);
        if (lim)
          for (uint32_t i = 0; i < n; ++i) {
            slots[slot_of[i]] = cur[i];
            printf("C %llu %u %u\n", (unsigned long long)cur[i].gen, cur[i].phase, cur[i].at);
          }
        printf("N %llu\n", (unsigned long long)o.n_ids);
      }
    } else if (cmd == "setcur") {
      uint32_t sl = 0;
      unsigned long long gen = 0;
      emqxgm_retain_cursor c;
      in >> sl >> gen >> c.phase >> c.at;
      c.gen = gen;
      slots[sl] = c;
      printf("K 0\n");
    } else if (cmd == "clear") {
      unsigned long long now = 0;
      in >> now;
      const uint32_t* ids = nullptr;
      uint64_t n = 0;
      const int rc = emqxgm_retain_clear_expired(h, now, &ids, &n);
      print_ids(h, rc, ids, n);
    } else if (cmd == "delmatch") {
      std::string hx;
      in >> hx;
      const std::string t = unhex(hx);
      Exact x(t);
      const uint32_t* ids = nullptr;
      uint64_t n = 0;
      const int rc = emqxgm_retain_delete_matching(h, x.p, (uint32_t)t.size(), &ids, &n);
      print_ids(h, rc, ids, n);
    } else if (cmd == "page") {
      std::string hx;
      unsigned long long page = 0, limit = 0, now = 0;
      in >> hx >> page >> limit >> now;
      const std::string t = unhex(hx);
      Exact x(t);
      const uint32_t* ids = nullptr;
      uint64_t n = 0;
      const int rc = emqxgm_retain_page_read(h, hx == "*" ? nullptr : x.p, (uint32_t)t.size(), page, limit,
                                             now, &ids, &n);
      print_ids(h, rc, ids, n);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
    fflush(stdout);
    if (!in) return 2;
  }
  emqxgm_retain_destroy(h);
  return 0;
}
