// match2_main.cpp -- mqtt_match of emqx_amd/csrc/gm_match.h (the matcher of k_rules, k_verify and
// k_verify_scatter) on the CPU (no HIP), built with ASan + UBSan by tests/test_match2_cpu.py.
// Every string sits in a heap block of exactly its length, so a read past either end is reported.
//
//   match2_main INPUT
// INPUT (text; byte strings in hex, "-" = empty):
//   n_names, then one name per line
//   n_filters, then one filter per line
// Output: two lines per filter, the bit row ('0'/'1' per name) of mqtt_match<true> (match/2 on
// binaries) and of mqtt_match<false> (match/2 on word lists).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_match.h"

struct Str {
  std::unique_ptr<uint8_t[]> p;
  uint32_t len = 0;
};

static Str unhex(const std::string& h) {
  Str s;
  if (h != "-") s.len = (uint32_t)(h.size() / 2);
  s.p.reset(new uint8_t[s.len]);
  for (uint32_t i = 0; i < s.len; ++i) s.p[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
  return s;
}

static bool read_list(std::ifstream& in, std::vector<Str>& out) {
  uint32_t n = 0;
  in >> n;
  for (uint32_t i = 0; i < n && in; ++i) {
    std::string hex;
    in >> hex;
    out.push_back(unhex(hex));
  }
  return (bool)in;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::vector<Str> names, filters;
  if (!read_list(in, names) || !read_list(in, filters)) return 2;
  std::string bin(names.size(), '0'), wl(names.size(), '0');
  for (const Str& f : filters) {
    for (size_t t = 0; t < names.size(); ++t) {
      const uint8_t* T = names[t].p.get();
      const uint8_t* F = f.p.get();
      bin[t] = gm::mqtt_match<true>(T, names[t].len, F, f.len) ? '1' : '0';
      wl[t] = gm::mqtt_match<false>(T, names[t].len, F, f.len) ? '1' : '0';
    }
    puts(bin.c_str());
    puts(wl.c_str());
  }
  return 0;
}
