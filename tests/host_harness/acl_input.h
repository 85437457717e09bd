// acl_input.h -- TEST INFRASTRUCTURE: the input file of the two ACL host programs (acl_main.cpp,
// acl_dev_main.cpp), in emqxgm_acl_set's and emqxgm_acl_match's own terms.  Text; byte strings
// in hex, "-" = empty:
//   hash_bits pass_names            (pass_names 0: the default)
//   n_rules, then per rule: "perm action who slot who_string n_filters", then per filter "flag hex"
//   n_clients, then per client: "flags clientid username who_bits"
//   n_requests, then per request: "client action name"
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <fstream>
#include <string>
#include <vector>

struct AclInput {
  uint32_t hash_bits = 0;
  uint64_t pass_names = 0;
  std::vector<uint8_t> fb, wb, nb, cb, ub;
  std::vector<uint32_t> fo{0}, ff, fr, perm, action, who, slot, wo{0};
  std::vector<uint32_t> co{0}, uo{0}, cf, no{0}, client, req_action;
  std::vector<uint64_t> wbits;
  uint32_t n_rules = 0, n_clients = 0, n = 0;
};

static inline void acl_unhex(const std::string& h, std::vector<uint8_t>& bytes, std::vector<uint32_t>& off) {
  if (h != "-")
    for (size_t i = 0; i + 1 < h.size(); i += 2) bytes.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  off.push_back((uint32_t)bytes.size());
}

static inline bool acl_read_input(const char* path, AclInput& in) {
  std::ifstream f(path);
  f >> in.hash_bits >> in.pass_names >> in.n_rules;
  for (uint32_t r = 0; r < in.n_rules; ++r) {
    uint32_t p, a, w, s, nf;
    std::string hex;
    f >> p >> a >> w >> s >> hex >> nf;
    in.perm.push_back(p);
    in.action.push_back(a);
    in.who.push_back(w);
    in.slot.push_back(s);
    acl_unhex(hex, in.wb, in.wo);
    for (uint32_t k = 0; k < nf; ++k) {
      uint32_t flag;
      f >> flag >> hex;
      acl_unhex(hex, in.fb, in.fo);
      in.ff.push_back(flag);
      in.fr.push_back(r);
    }
  }
  f >> in.n_clients;
  for (uint32_t c = 0; c < in.n_clients; ++c) {
    uint32_t flags;
    uint64_t bits;
    std::string cid, usr;
    f >> flags >> cid >> usr >> bits;
    in.cf.push_back(flags);
    acl_unhex(cid, in.cb, in.co);
    acl_unhex(usr, in.ub, in.uo);
    in.wbits.push_back(bits);
  }
  f >> in.n;
  for (uint32_t t = 0; t < in.n; ++t) {
    uint32_t c, a;
    std::string hex;
    f >> c >> a >> hex;
    in.client.push_back(c);
    in.req_action.push_back(a);
    acl_unhex(hex, in.nb, in.no);
  }
  return (bool)f;
}

// An exact-size heap copy of a vector (a read one element past it hits an ASan redzone; the
// vector's own capacity may be larger than its size).
template <class T>
struct AclExact {
  T* p;
  explicit AclExact(const std::vector<T>& v) : p(new T[v.size()]) {
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  }
  ~AclExact() { delete[] p; }
  AclExact(const AclExact&) = delete;
  AclExact& operator=(const AclExact&) = delete;
};
