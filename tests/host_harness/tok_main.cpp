// tok_main.cpp -- TEST INFRASTRUCTURE: the per-lane functions of emqx_amd/csrc/gm_tok.inc
// themselves (not a restatement) on the CPU, under ASan + UBSan, over the case batches of
// tests/tok_cases.py.  Built and driven by tests/test_tok_host.py (tests/host_build.py); the file
// is included unchanged behind hip_shim.h, its three constants that live in gm_kernels.hip (WG,
// TILE_BYTES, TILE_CHUNKS) come from build/tok_consts.inc, which the test cuts out of that file.
//
// Memory is laid out so that a read the kernels must not make trips ASan:
//   * the LDS tile is a heap block of exactly TILE_CHUNKS * 16 bytes, filled with '/' before
//     every tile (stale bytes past a tile's end are the worst ones for next_slash);
//   * a batch's bytes live in a heap block with exactly what the engine guarantees around a
//     batch: emqxgm_match_batch copies it to the start of d_in_bytes and the host pipes to the
//     start of their d_bytes, both hipMalloc'ed (aligned far beyond 16 bytes) with a capacity
//     rounded up to a multiple of 16 (ensure_input, host_pipe_reserve), so the 16-B chunks that
//     stage_tile reads -- it reads whole chunks, up to 15 bytes either side of a tile by design
//     -- end inside the allocation; the copy-through k_tok reads a pinned window the same way
//     (emqxgm_host_alloc rounds its size up to a multiple of 16 too) and stores the chunks into
//     the pipe's d_bytes.  A caller-owned buffer (emqxgm_match_device) has to be
//     readable over the aligned 16-B chunks that hold its first and last byte
//     (include/emqx_gpumatch.h); `base` = its address residue: the block starts `base` bytes in
//     front of the batch and ends at the next multiple of 16 behind it.  The padding holds '/'.
//
// Input (argv[1]): commands, strings as hex lines ("-" = empty):
//   tok <base> <test_mask> <n>, n topics       -> "tile <k> <sh> <fits>" per 256-topic tile and,
//       per topic, "R <t> <levels> <flags> <7 record tokens> <deep tokens>" from tok_words_rec
//       (fitting tiles) and "W ..." from tok_words
//   probe <full_hash_bits> <kinds> <base> <nk> <nn>, nk keys, nn names -> "probe <lookups>":
//       every name through exact_lookup over global memory, exact_lookup over the staged LDS
//       tile, exact_lookup_wild, k_xhash + exact_probe and k_exact_owned (parts 1..3) against a
//       std::map of the keys; a difference ends the program
// Prints "consts ..." first and "OK" last; before the commands it checks that ensure_input and
// host_pipe_reserve really give capacities of whole 16-B chunks (run_caps).
#include "harness_rig.h"

#include "hip_shim.h"

namespace gm {
namespace {
#include "build/tok_consts.inc"
inline uint32_t lane_id() { return threadIdx.x & 63u; }
inline uint32_t mbcnt64(uint64_t) { return 0u; }
#include "../../emqx_amd/csrc/gm_tok.inc"
}  // namespace
}  // namespace gm

namespace {

constexpr uint64_t SENT = 0x5E5E5E5E5E5E5E5Eull;  // a token-array slot nothing wrote

std::string unhex(const std::string& s) {
  if (s == "-") return std::string();
  std::string o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((char)std::stoi(s.substr(i, 2), nullptr, 16));
  return o;
}

std::vector<std::string> read_strings(FILE* f, size_t n) {
  std::vector<std::string> v;
  char* line = nullptr;
  size_t cap = 0;
  for (size_t i = 0; i < n; ++i) {
    const ssize_t len = getline(&line, &cap, f);
    CHECK(len > 0, "input ends early");
    std::string s(line, (size_t)len);
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    v.push_back(unhex(s));
  }
  free(line);
  return v;
}

// A packed batch in a heap block of its own (see the file comment).
struct Packed {
  uint8_t* block = nullptr;
  uint8_t* bytes = nullptr;
  size_t cap = 0;
  std::vector<uint32_t> off;
  Packed(const std::vector<std::string>& ts, uint32_t base) : off(1, 0) {
    size_t n = 0;
    for (const auto& t : ts) n += t.size();
    cap = std::max<size_t>((base + n + 15) & ~(size_t)15, 16);
    block = (uint8_t*)aligned_alloc(16, cap);
    memset(block, '/', cap);
    bytes = block + base;
    for (const auto& t : ts) {
      if (!t.empty()) memcpy(bytes + off.back(), t.data(), t.size());  // (memcpy(_, null, 0) is UB)
      off.push_back(off.back() + (uint32_t)t.size());
    }
  }
  ~Packed() { free(block); }
  Packed(const Packed&) = delete;
};

struct Lds {
  uint4* buf;
  Lds() : buf((uint4*)aligned_alloc(16, TILE_CHUNKS * 16)) {}
  ~Lds() { free(buf); }
  // stage_tile by the 256 lanes of a block; every lane must decide alike
  template <bool CP>
  bool stage(const Packed& P, uint32_t B0, uint32_t B1, uint32_t& sh, uint8_t* cp = nullptr) {
    memset(buf, '/', TILE_CHUNKS * 16);
    bool tiled = false;
    for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x) {
      uint32_t s = 0;
      const bool f = stage_tile<CP>(P.bytes, B0, B1, buf, s, cp);
      if (threadIdx.x == 0) {
        sh = s;
        tiled = f;
      }
      CHECK(f == tiled && s == sh, "lanes disagree on a tile");
    }
    threadIdx.x = 0;
    return tiled;
  }
};

void print_tokens(char path, uint32_t t, uint32_t nwd, uint32_t flags, const uint64_t (&tk)[REC_TOKS],
                  const std::vector<uint64_t>& wh, uint32_t wb) {
  printf("%c %u %u %u", path, t, nwd, flags);
  for (uint32_t k = 0; k < REC_TOKS; ++k) printf(" %llx", (unsigned long long)tk[k]);
  for (uint32_t k = REC_TOKS; k < nwd; ++k) printf(" %llx", (unsigned long long)wh[wb + k]);
  printf("\n");
}

void run_tok(const std::vector<std::string>& topics, uint32_t base, uint64_t mask) {
  const Packed P(topics, base);
  const Packed C(topics, base);  // the copy-through target: the same offsets, '/' everywhere
  memset(C.block, '/', C.cap);
  Lds lds;
  const uint32_t* s32 = (const uint32_t*)lds.buf;
  const uint32_t n = (uint32_t)topics.size();
  // token k >= REC_TOKS of topic t lives at wh[off[t] + t + k]: no two topics share a slot
  std::vector<uint64_t> wh((size_t)P.off[n] + n + 1, SENT);
  for (uint32_t t0 = 0; t0 < n; t0 += WG) {
    const uint32_t t1 = std::min(t0 + WG, n), B0 = P.off[t0], B1 = P.off[t1];
    uint32_t sh = 0, sh2 = 0;
    const bool tiled = lds.stage<false>(P, B0, B1, sh);
    CHECK(lds.stage<true>(P, B0, B1, sh2, C.bytes) == tiled && sh2 == sh, "copy-through staging");
    printf("tile %u %u %d\n", t0 / WG, sh, (int)tiled);
    if (tiled) CHECK(memcmp(C.bytes + B0, P.bytes + B0, B1 - B0) == 0, "copy-through bytes of tile %u", t0 / WG);
    for (uint32_t t = t0; t < t1; ++t) {
      const uint32_t ob = P.off[t], len = P.off[t + 1] - ob, wb = ob + t;
      auto deep = [&](uint32_t k, uint64_t tok) {
        CHECK(k >= REC_TOKS && (size_t)wb + k < wh.size(), "deep token %u of topic %u", k, t);
        CHECK(wh[wb + k] == SENT, "token slot %u written twice", wb + k);
        wh[wb + k] = tok;
      };
      uint32_t flags = 0;
      if (tiled) {
        uint64_t tk[REC_TOKS] = {0, 0, 0, 0, 0, 0, 0};
        const uint32_t nwd = tok_words_rec(s32, sh + (ob - B0), len, mask, tk, deep, flags);
        print_tokens('R', t, nwd, flags, tk, wh, wb);
        for (uint32_t k = REC_TOKS; k < nwd; ++k) wh[wb + k] = SENT;
      }
      uint64_t tk[REC_TOKS] = {0, 0, 0, 0, 0, 0, 0};
      auto dst = [&](uint32_t k, uint64_t tok) {
        if (k < REC_TOKS)
          tk[k] = tok;
        else
          deep(k, tok);
      };
      const uint32_t nwd = tok_words(GlobBytes{P.bytes + ob}, len, mask, dst, flags);
      print_tokens('W', t, nwd, flags, tk, wh, wb);
    }
  }
}

ExactArgs exact_args(const DevIndex& ix) {  // gm_kernels.hip exact_args
  ExactArgs x;
  x.xseq = 1;
  x.exact = ix.exact;
  x.xovf = ix.xovf;
  x.xmask = ix.xmask;
  x.xwbase = ix.xwbase;
  x.xwmask = ix.xwmask;
  x.fbytes = ix.fbytes;
  x.foff = ix.foff;
  x.full_mask = ix.full_mask;
  return x;
}

uint64_t run_probe(uint32_t bits, const std::string& kinds, uint32_t base,
                   const std::vector<std::string>& keys, const std::vector<std::string>& names) {
  emqxgm_t* h = nullptr;
  emqxgm_cfg cfg{};
  cfg.full_hash_bits = bits;
  CHECK(emqxgm_create(&cfg, &h) == 0, "create");
  std::map<std::string, uint32_t> ids;
  for (const auto& k : keys) {
    uint32_t id = NONE;
    CHECK(emqxgm_route_ref(h, (const uint8_t*)k.data(), (uint32_t)k.size(), &id) == 0, "route_ref");
    ids[k] = id;
  }
  CHECK(emqxgm_commit(h, nullptr) == 0, "commit: %s", h->err.c_str());
  const DevIndex& ix = h->cur->ix;
  CHECK(ix.plain_empty == (kinds == "wild") && ix.wild_empty == (kinds == "plain"), "regions of '%s'", kinds.c_str());
  const ExactArgs X = exact_args(ix);
  const Packed P(names, base);
  const uint32_t n = (uint32_t)names.size();
  uint64_t lookups = 0;
  std::vector<uint32_t> want(n), mark(n);
  std::vector<uint8_t> wild(n);
  for (uint32_t t = 0; t < n; ++t) {
    const auto it = ids.find(names[t]);
    want[t] = it == ids.end() ? NONE : it->second;
    uint32_t flags = 0;
    tok_words(GlobBytes{P.bytes + P.off[t]}, P.off[t + 1] - P.off[t], 0, [](uint32_t, uint64_t) {}, flags);
    wild[t] = (flags & T_WILD) != 0;
    mark[t] = wild[t] ? X_WILDPEND : NONE;  // what k_tok<DEFER> leaves for k_exact / k_xhash
  }
  auto same = [&](const char* what, uint32_t t, uint32_t got) {
    CHECK(got == want[t], "%s: name %u (%zu bytes) at residue %u: id %u, the key map says %u (%u-bit hashes, %s keys)",
          what, t, names[t].size(), (base + P.off[t]) & 15u, got, want[t], bits, kinds.c_str());
    ++lookups;
  };
  Lds lds;
  const uint32_t* s32 = (const uint32_t*)lds.buf;
  // k_exact: runs when there are plain keys; a wildcard name without wildcard keys is decided
  if (!ix.plain_empty)
    for (uint32_t t0 = 0; t0 < n; t0 += WG) {
      const uint32_t t1 = std::min(t0 + WG, n), B0 = P.off[t0], B1 = P.off[t1];
      uint32_t sh = 0;
      const bool tiled = lds.stage<false>(P, B0, B1, sh);
      CHECK(tiled, "a probe tile does not fit");
      for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t ob = P.off[t], len = P.off[t + 1] - ob;
        if (wild[t] && ix.wild_empty) continue;
        same("exact_lookup over global memory", t, exact_lookup(X, P.bytes, ob, len, wild[t] != 0));
        same("exact_lookup over the LDS tile", t,
             exact_lookup(X, P.bytes, ob, len, wild[t] != 0, LdsTopicWords(s32, sh + (ob - B0), len)));
      }
    }
  // k_tok's own probe of a wildcard name
  if (!ix.wild_empty)
    for (uint32_t t = 0; t < n; ++t)
      if (wild[t]) same("exact_lookup_wild", t, exact_lookup_wild(X, P.bytes, P.off[t], P.off[t + 1] - P.off[t]));
  if (!ix.plain_empty) {
    // k_xhash, the kernel itself (its lanes are independent), then k_exact_part's probe
    std::vector<uint32_t> xid(mark);
    std::vector<uint2> xh(n);
    blockIdx.x = 0;
    gridDim.x = 1;
    for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)
      k_xhash(P.bytes, P.off.data(), n, xid.data(), X, ix.wild_empty, xh.data());
    threadIdx.x = 0;
    for (uint32_t t = 0; t < n; ++t) {
      if (wild[t] && ix.wild_empty) {
        CHECK(xid[t] == NONE && xh[t].x == NONE, "k_xhash: a decided wildcard name");
        continue;
      }
      const uint32_t ob = P.off[t], len = P.off[t + 1] - ob;
      const uint64_t fh = key_hash((const uint8_t*)names[t].data(), len, ix.full_mask);  // the host's hash
      CHECK(xh[t].y == (uint32_t)(fh >> 32), "k_xhash: name %u (%u bytes): h32 differs from key_hash's", t, len);
      const TopicWords T(P.bytes, ob, len);
      uint32_t tw[XINL / 4];
      for (uint32_t k = 0; k < XINL / 4; ++k) tw[k] = 4 * k < len ? (T(k) & len_mask(len, k)) : 0u;
      const bool w = xh[t].x >= X.xwbase;
      CHECK(w == (wild[t] != 0), "k_xhash: region of name %u", t);
      same("k_xhash + exact_probe", t,
           exact_probe(X, T, len, w ? X.xwbase : 0ull, w ? X.xwmask : X.xmask, xh[t].x, xh[t].y, tw));
    }
    // k_exact_owned, the kernel itself: the owner answers, the others say NONE
    std::vector<uint64_t> off64(P.off.begin(), P.off.end());
    for (uint32_t parts = 1; parts <= 3; ++parts) {
      std::vector<uint32_t> own(n);
      CHECK(emqxgm_key_owners(h, P.bytes, off64.data(), n, parts, own.data()) == 0, "key_owners");
      for (uint32_t part = 0; part < parts; ++part) {
        std::vector<uint32_t> out(n, 0x12345678u);
        for (threadIdx.x = 0; threadIdx.x < WG; ++threadIdx.x)
          k_exact_owned(P.bytes, P.off.data(), n, out.data(), X, parts, part);
        threadIdx.x = 0;
        for (uint32_t t = 0; t < n; ++t) {
          const uint32_t w = (own[t] == part && !wild[t]) ? want[t] : NONE;
          CHECK(out[t] == w, "k_exact_owned: name %u (%zu bytes), part %u of %u (owner %u): id %u, want %u", t,
                names[t].size(), part, parts, own[t], out[t], w);
          ++lookups;
        }
      }
    }
  }
  emqxgm_destroy(h);
  return lookups;
}

// The guarantee the Packed blocks above rest on: the engine's own topic-byte buffers hold whole
// 16-B chunks whatever size asked for them (odd sizes, growing: a capacity is only replaced by a
// larger one).
void run_caps() {
  emqxgm_t* h = nullptr;
  emqxgm_cfg cfg{};
  CHECK(emqxgm_create(&cfg, &h) == 0, "create");
  for (uint64_t bytes : {1ull, 1000003ull, (1ull << 20) + 1, 3000001ull, 7654321ull}) {
    CHECK(ensure_input(h, bytes, 2) == 0, "ensure_input");
    CHECK(h->in_bytes_cap >= bytes && h->in_bytes_cap % 16 == 0, "d_in_bytes: %llu bytes for %llu",
          (unsigned long long)h->in_bytes_cap, (unsigned long long)bytes);
    emqxgm::HostPipe& p = h->hpipes[0];
    CHECK(host_pipe_reserve(h, p, 1, bytes, 1) == 0, "host_pipe_reserve");
    CHECK(p.bytes_cap >= bytes && p.bytes_cap % 16 == 0, "a host pipe's d_bytes: %llu bytes for %llu",
          (unsigned long long)p.bytes_cap, (unsigned long long)bytes);
  }
  emqxgm_destroy(h);
}

}  // namespace

int main(int argc, char** argv) {
  CHECK(argc == 2, "usage: %s <commands>", argv[0]);
  FILE* f = fopen(argv[1], "r");
  CHECK(f, "cannot open %s", argv[1]);
  printf("consts %u %u %u %u %u %u\n", TILE_BYTES, TILE_CHUNKS, REC_TOKS, TOK_INLINE_MAX, XINL, WG);
  run_caps();
  char cmd[16], kinds[16];
  while (fscanf(f, "%15s", cmd) == 1) {
    if (!strcmp(cmd, "tok")) {
      unsigned base = 0, n = 0;
      unsigned long long mask = 0;
      CHECK(fscanf(f, "%u %llx %u\n", &base, &mask, &n) == 3, "tok header");
      printf("tok %u %llx %u\n", base, mask, n);
      run_tok(read_strings(f, n), base, mask);
    } else if (!strcmp(cmd, "probe")) {
      unsigned bits = 0, base = 0, nk = 0, nn = 0;
      CHECK(fscanf(f, "%u %15s %u %u %u\n", &bits, kinds, &base, &nk, &nn) == 5, "probe header");
      const std::vector<std::string> keys = read_strings(f, nk);
      const std::vector<std::string> names = read_strings(f, nn);
      printf("probe %u %s %u %llu\n", bits, kinds, base,
             (unsigned long long)run_probe(bits, kinds, base, keys, names));
    } else {
      CHECK(false, "unknown command '%s'", cmd);
    }
  }
  fclose(f);
  printf("OK\n");
  return 0;
}
