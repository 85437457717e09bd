// gm_ruleset.inc -- every matching rule per name against a resident rule list (included by
// gm_kernels.hip; DESIGN.md 6b).
//
// The loops that keep every match, run once per publish beside the route match:
//   * emqx_rule_engine:get_rules_for_topic/1 (apps/emqx_rule_engine/src/emqx_rule_engine.erl:
//     198-204): a rule matches when any of its `from` filters does
//     (emqx_plugin_libs_rule:can_topic_match_oneof/2, emqx_plugin_libs_rule.erl:340-346);
//   * emqx_bridge:get_matched_egress_bridges/1 (emqx_bridge.erl:342-382);
//   * the exhook and trace topic filters (emqx_exhook_server.erl:361, emqx_trace_handler.erl:138).
//
// One lane per name, block b owns names [WG b, WG b + WG).  A lane tokenises its name once into
// LDS (level-major: a wave reads one level as consecutive 8-byte words), then the block stages
// the compiled records (gm_ruleset_match.h) tile by tile into LDS and every lane walks the tile
// from word 0 -- all lanes read the same record words (a broadcast), so the loop is wave-uniform.
// A token hit on a filter with a hashed word, and every record for a name deeper than
// RS_MAX_LEVELS, is confirmed on the bytes: no result rests on a hash.  Records lie in filter
// order with a rule's filters adjacent, so a lane keeps the last rule it reported and drops a
// second hit of the same rule: rows come out ascending, each rule once.  Count pass, scan
// (launch_ruleset_ptr), fill pass.
//
// The kernel body is a sequence of per-lane phase functions separated by __syncthreads() and
// nothing else; tests/host_harness/ruleset_dev_main.cpp runs each phase for all WG lanes of a
// block before the next, which reproduces the barriers, under ASan + UBSan.  Every lane walks
// every barrier: a lane past the last name skips the work inside the phases.

constexpr uint32_t RS_CTR_CAND = 0;     // candidates sent to the byte check
constexpr uint32_t RS_CTR_REMOVED = 1;  // candidates the byte check removed
constexpr uint32_t RS_CTR_DEEP = 2;     // names deeper than RS_MAX_LEVELS
constexpr uint32_t RS_CTR_VISITED = 3;  // records visited (names x records)
constexpr uint32_t RS_CTRS = 4;
static_assert(RS_CTRS * WG <= RS_TILE_WORDS, "the counters are reduced through the record tile");
static_assert(RS_TILE_WORDS % WG == 0, "a lane stages RS_TILE_WORDS / WG words of a tile");

// What a lane keeps in registers from phase to phase.
struct RsLane {
  uint32_t t, active;
  uint32_t n0, tl;                        // the name's bytes: nb[n0 .. n0 + tl)
  uint32_t n_levels, dollar, hash_words;  // rs_tokenize / rs_match_tokens
  uint32_t last_rule, k;                  // the last rule reported, rules reported so far
  uint32_t r0, rlen;                      // fill: the lane's row
  uint32_t bad;
  uint32_t c_cand, c_removed, c_visited;
};

template <bool FILL>
__device__ __forceinline__ void rs_ph_tokenize(const RulesetArgs& A, RsLane& L, uint64_t* s_tok) {
  L.t = blockIdx.x * WG + threadIdx.x;
  L.active = L.t < A.n;
  L.n0 = L.tl = L.n_levels = L.dollar = L.hash_words = 0;
  L.last_rule = NONE;
  L.k = L.r0 = L.rlen = L.bad = 0;
  L.c_cand = L.c_removed = L.c_visited = 0;
  if (!L.active) return;
  L.n0 = A.no[L.t];
  L.tl = A.no[L.t + 1] - L.n0;
  const uint8_t* T = A.nb + L.n0;
  uint32_t hw = 0;
  L.n_levels = rs_tokenize(T, L.tl, A.test_mask, RS_MAX_LEVELS,
                           [&](uint32_t lv, uint64_t tk, uint32_t at, uint32_t len) {
                             s_tok[lv * WG + threadIdx.x] = tk;
                             if (len == 1 && T[at] == '#') hw |= 1u << lv;
                           });
  L.hash_words = hw;
  L.dollar = L.tl > 0 && T[0] == '$';
  if (FILL) {
    L.r0 = A.row[L.t];
    L.rlen = A.row[L.t + 1] - L.r0;
  }
}

// Tile k of the record stream into LDS; a short last tile ends in RS_END.
__device__ __forceinline__ void rs_ph_stage(const RulesetArgs& A, uint32_t k, uint64_t* s_tile) {
  const uint32_t span = rs_tile_span(k, A.total_words);
  const uint64_t base = (uint64_t)k * RS_TILE_WORDS;
  for (uint32_t i = threadIdx.x; i < RS_TILE_WORDS; i += WG)
    s_tile[i] = i < span ? A.recs[base + i] : RS_END;
}

// The byte check of name L against filter f, by the filter's flag.
__device__ __forceinline__ bool rs_confirm(const RulesetArgs& A, RsLane& L, uint32_t f) {
  if (f >= A.n_filters) {
    L.bad = 1;
    return false;
  }
  const uint32_t f0 = A.fo[f], fl = A.fo[f + 1] - f0, fg = A.ff[f];
  const uint8_t* T = A.nb + L.n0;
  const uint8_t* F = A.fb + f0;
  if (fg & RS_F_EQ) return L.tl == fl && bytes_equal(T, F, fl);
  if (fg & RS_F_WORDS) return mqtt_match<false>(T, L.tl, F, fl);
  return mqtt_match<true>(T, L.tl, F, fl);
}

template <bool FILL>
__device__ __forceinline__ void rs_ph_walk(const RulesetArgs& A, RsLane& L, const uint64_t* s_tok,
                                           const uint64_t* s_tile) {
  if (!L.active) return;
  const bool deep = L.n_levels > RS_MAX_LEVELS;
  for (uint32_t p = 0; p < RS_TILE_WORDS;) {
    const uint64_t hdr = s_tile[p];
    if (hdr == RS_END) break;
    const uint32_t step = 1 + rs_levels(hdr);
    if (p + step > RS_TILE_WORDS) {  // no record straddles a tile (rs_append)
      L.bad = 1;
      break;
    }
    ++L.c_visited;
    const uint32_t rule = rs_rule(hdr);
    if (rule != L.last_rule) {  // else: a further filter of a rule already reported
      bool ok = deep || rs_match_tokens(hdr, s_tile + p + 1, L.n_levels, L.dollar != 0, L.hash_words,
                                        [&](uint32_t l) { return s_tok[l * WG + threadIdx.x]; });
      if (ok && (deep || (rs_flags(hdr) & RS_HASHED))) {
        ++L.c_cand;
        ok = rs_confirm(A, L, rs_filter(hdr));
        L.c_removed += !ok;
      }
      if (ok) {
        if (FILL) {
          if (L.k < L.rlen)
            A.rule[L.r0 + L.k] = rule;
          else
            L.bad = 1;  // more hits than the count pass found: never outside the row
        }
        L.last_rule = rule;
        ++L.k;
      }
    }
    p += step;
  }
}

// The lane's result; with counters on, its four counts go to LDS (the record tile is free now).
template <bool FILL>
__device__ __forceinline__ void rs_ph_finish(const RulesetArgs& A, RsLane& L, uint64_t* s_tile) {
  if (L.active) {
    if (!FILL)
      A.cnt[L.t] = L.k;
    else if (L.k != L.rlen)
      L.bad = 1;
  }
  if (L.bad) *A.err = 1u;
  if (!FILL && A.ctr) {
    s_tile[RS_CTR_CAND * WG + threadIdx.x] = L.c_cand;
    s_tile[RS_CTR_REMOVED * WG + threadIdx.x] = L.c_removed;
    s_tile[RS_CTR_DEEP * WG + threadIdx.x] = L.active && L.n_levels > RS_MAX_LEVELS;
    s_tile[RS_CTR_VISITED * WG + threadIdx.x] = L.c_visited;
  }
}

// Lane c < RS_CTRS of each wave adds up counter c of its wave's 64 lanes: one atomic per wave
// and counter.
template <bool FILL>
__device__ __forceinline__ void rs_ph_counters(const RulesetArgs& A, const uint64_t* s_tile) {
  if (FILL || !A.ctr) return;
  const uint32_t c = threadIdx.x & 63u, w0 = threadIdx.x & ~63u;
  if (c >= RS_CTRS) return;
  unsigned long long sum = 0;
  for (uint32_t i = 0; i < 64; ++i) sum += s_tile[c * WG + w0 + i];
  if (sum) atomicAdd(&A.ctr[c], sum);
}

template <bool FILL>
__global__ __launch_bounds__(WG) void k_ruleset(RulesetArgs A) {
  __shared__ uint64_t s_tok[RS_MAX_LEVELS * WG];  // [level][lane], 32 KB
  __shared__ uint64_t s_tile[RS_TILE_WORDS];      // 8 KB
  RsLane L;
  rs_ph_tokenize<FILL>(A, L, s_tok);
  __syncthreads();
  const uint32_t tiles = rs_n_tiles(A.total_words);
  for (uint32_t k = 0; k < tiles; ++k) {
    rs_ph_stage(A, k, s_tile);
    __syncthreads();
    rs_ph_walk<FILL>(A, L, s_tok, s_tile);
    __syncthreads();
  }
  rs_ph_finish<FILL>(A, L, s_tile);
  __syncthreads();
  rs_ph_counters<FILL>(A, s_tile);
}
