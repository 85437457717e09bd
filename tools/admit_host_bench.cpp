// admit_host_bench.cpp -- the CPU yardstick of tools/admit_bench.py: gm_admit_match.h (the code
// k_admit runs per item) compiled for the host, over a packed batch, on T threads.
//   admit_host_bench FILE MODE THREADS REPS
// FILE: u32 n, u32 offsets[n + 1], then the bytes (padded to a multiple of 8 by the writer).
// Prints "best_ms checksum".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <thread>
#include <vector>

#include "../emqx_amd/csrc/gm_admit_match.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t mode = (uint32_t)atoi(argv[2]);
  const int threads = atoi(argv[3]), reps = atoi(argv[4]);
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  std::vector<uint32_t> off((size_t)n + 1);
  if (fread(off.data(), 4, off.size(), f) != off.size()) return 2;
  std::vector<uint64_t> words(((size_t)off[n] + 7) / 8 + 1);
  if (off[n] && fread(words.data(), 1, off[n], f) != off[n]) return 2;
  fclose(f);
  const uint8_t* bytes = (const uint8_t*)words.data();
  std::vector<gm::AdmRecord> out(n);
  auto work = [&](uint32_t lo, uint32_t hi) {
    for (uint32_t t = lo; t < hi; ++t) {
      const uint32_t len = off[t + 1] - off[t];
      const gm::AdmGlob R{bytes + off[t], len};
      gm::AdmParse P;
      gm::AdmScan S;
      if (mode == gm::ADM_FILTER) P = gm::adm_parse(R, len, false);
      if (gm::adm_length_verdict(len) == gm::ADM_V_OK) gm::adm_scan(R, len, S);
      out[t] = gm::adm_record(mode, len, P, S, 0, 65535, 2 | gm::ADM_C_RETAIN | gm::ADM_C_WILDCARD | gm::ADM_C_SHARED);
    }
  };
  double best = 1e30;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int k = 0; k < threads; ++k)
      th.emplace_back(work, (uint32_t)((uint64_t)n * k / threads), (uint32_t)((uint64_t)n * (k + 1) / threads));
    for (auto& t : th) t.join();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms < best) best = ms;
  }
  uint64_t sum = 0;
  for (const gm::AdmRecord& r : out) sum += r.w0 + r.levels + r.off;
  printf("%.3f %llu\n", best, (unsigned long long)sum);
  return 0;
}
