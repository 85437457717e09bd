// gm_acl.inc -- the first matching ACL rule per request against a resident rule list (included by
// gm_kernels.hip; DESIGN.md 6b "ACL lists").
//
// emqx_authz_rule:matches/4 (apps/emqx_authz/src/emqx_authz_rule.erl:125-133) over match/4
// (:135-145): rules in order; within a rule match_action/2 (:147-150), then match_who/2
// (:152-200), then match_topics/3 (:202-210) with feed_var/2 (:217-230).  It is what
// emqx_authz_file:authorize/4 (emqx_authz_file.erl:64-65) and, one rule at a time,
// emqx_authz_mnesia:authorize/4 (emqx_authz_mnesia.erl:98-120, 222-229) run per publish and
// subscribe.
//
// One lane per request (client, publish | subscribe, name), block b owns requests
// [WG b, WG b + WG).  A lane tokenises its name once into LDS (level-major, as k_ruleset does)
// and derives its client's words {client-id token, username token, flags} from the call's client
// table itself: the derivation is one pass over at most two short strings, and a kernel of its
// own per call would cost a launch for work that hides behind the name's tokenising.  Then the
// block stages the record stream (gm_acl_match.h) tile by tile into LDS and every lane walks the
// tile from word 0: all lanes read the same record words (a broadcast), the loop is wave-uniform
// and only the byte check diverges.  A rule header sets the lane's "rule live" bit from action and
// who; a filter record of a live rule that matches -- confirmed on the bytes wherever the hit
// rests on a hashed token or the name is deeper than RS_MAX_LEVELS -- fixes the lane's answer,
// and the lane skips the rest.  One u32 per request; one pass.
//
// The kernel body is a sequence of per-lane phase functions separated by barriers and nothing
// else; tests/host_harness/acl_dev_main.cpp runs each phase for all WG lanes of a block before
// the next, under ASan + UBSan.  Every lane walks every barrier: a lane with its answer, or past
// the last request, skips the work inside the phases.  There is no block-wide early exit: its
// vote would take LDS of its own, and the 256 bytes are what separates four blocks per CU from
// three (40 KB of LDS per block, 160 KB per CU).

constexpr uint32_t ACL_CTR_CAND = 0;     // candidates sent to a byte check (who strings included)
constexpr uint32_t ACL_CTR_REMOVED = 1;  // candidates the byte check removed
constexpr uint32_t ACL_CTR_DEEP = 2;     // names deeper than RS_MAX_LEVELS
constexpr uint32_t ACL_CTR_VISITED = 3;  // records visited (rule headers and filter records)
constexpr uint32_t ACL_CTRS = 4;
static_assert(ACL_CTRS * WG <= RS_TILE_WORDS, "the counters are reduced through the record tile");
static_assert(RS_TILE_WORDS % WG == 0, "a lane stages RS_TILE_WORDS / WG words of a tile");

// What a lane keeps in registers from phase to phase.
struct AclLane {
  uint32_t t, active;
  uint32_t n0, tl;               // the name's bytes: nb[n0 .. n0 + tl)
  uint32_t n_levels, hash_words; // rs_tokenize / rs_match_tokens
  uint32_t action;               // ACL_PUBLISH or ACL_SUBSCRIBE
  uint32_t c0, cl, u0, ul;       // the client's id cb[c0 .. c0 + cl) and username ub[u0 .. u0 + ul)
  AclClient c;
  uint64_t who_bits;
  uint32_t live, ans;            // the current rule passed action and who; the answer (NONE: pending)
  uint32_t bad;
  uint32_t c_cand, c_removed, c_visited;
};

__device__ __forceinline__ void acl_ph_tokenize(const AclArgs& A, AclLane& L, uint64_t* s_tok) {
  L.t = blockIdx.x * WG + threadIdx.x;
  L.active = L.t < A.n;
  L.n0 = L.tl = L.n_levels = L.hash_words = L.action = 0;
  L.c0 = L.cl = L.u0 = L.ul = 0;
  L.c = AclClient();
  L.who_bits = 0;
  L.live = 0;
  L.ans = NONE;
  L.bad = 0;
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
  L.action = A.action[L.t];
  const uint32_t ci = A.client[L.t];
  if (ci >= A.n_clients || (L.action != ACL_PUBLISH && L.action != ACL_SUBSCRIBE)) {
    L.bad = 1;  // the host checks both before it launches
    L.active = 0;
    return;
  }
  L.c0 = A.co[ci];
  L.cl = A.co[ci + 1] - L.c0;
  L.u0 = A.uo[ci];
  L.ul = A.uo[ci + 1] - L.u0;
  L.c = acl_client(A.cb + L.c0, L.cl, A.ub + L.u0, L.ul, A.cf[ci], A.test_mask);
  L.who_bits = A.wbits[ci];
}

// Tile k of the record stream into LDS; a short last tile ends in RS_END.
__device__ __forceinline__ void acl_ph_stage(const AclArgs& A, uint32_t k, uint64_t* s_tile) {
  const uint32_t span = rs_tile_span(k, A.total_words);
  const uint64_t base = (uint64_t)k * RS_TILE_WORDS;
  for (uint32_t i = threadIdx.x; i < RS_TILE_WORDS; i += WG)
    s_tile[i] = i < span ? A.recs[base + i] : RS_END;
}

// The byte check of rule `rule`'s who string against the lane's client.
__device__ __forceinline__ bool acl_confirm_who(const AclArgs& A, AclLane& L, uint32_t rule, uint32_t kind) {
  if (rule >= A.n_rules) {
    L.bad = 1;
    return false;
  }
  const uint32_t w0 = A.wo[rule], wl = A.wo[rule + 1] - w0;
  if (kind == ACL_WHO_USERNAME) return wl == L.ul && bytes_equal(A.wb + w0, A.ub + L.u0, wl);
  return wl == L.cl && bytes_equal(A.wb + w0, A.cb + L.c0, wl);
}

// The byte check of the lane's name against filter f with the lane's client fed in.
__device__ __forceinline__ bool acl_confirm(const AclArgs& A, AclLane& L, uint32_t f) {
  if (f >= A.n_filters) {
    L.bad = 1;
    return false;
  }
  const uint32_t f0 = A.fo[f], fl = A.fo[f + 1] - f0;
  return acl_match_bytes(A.nb + L.n0, L.tl, A.fb + f0, fl, (A.ff[f] & RS_F_EQ) != 0, A.cb + L.c0, L.cl,
                         A.ub + L.u0, L.ul, L.c.flags);
}

__device__ __forceinline__ void acl_ph_walk(const AclArgs& A, AclLane& L, const uint64_t* s_tok,
                                            const uint64_t* s_tile) {
  if (!L.active || L.ans != NONE) return;
  const bool deep = L.n_levels > RS_MAX_LEVELS;
  for (uint32_t p = 0; p < RS_TILE_WORDS;) {
    const uint64_t w0 = s_tile[p];
    if (w0 == RS_END) break;
    const uint32_t step = acl_step(w0);
    if (p + step > RS_TILE_WORDS) {  // no record straddles a tile (rs_append)
      L.bad = 1;
      break;
    }
    ++L.c_visited;
    if (acl_is_rule(w0)) {
      bool confirm = false;
      bool ok = acl_match_action(acl_action(w0), L.action) &&
                acl_match_who_tokens(w0, s_tile[p + 1], L.c, L.who_bits, &confirm);
      if (ok && confirm) {
        ++L.c_cand;
        ok = acl_confirm_who(A, L, acl_rule(w0), acl_who(w0));
        L.c_removed += !ok;
      }
      L.live = ok;
    } else if (L.live) {
      const uint64_t w1 = s_tile[p + 1];
      bool ok = deep || acl_match_tokens(w0, w1, s_tile + p + ACL_FILTER_HDR, L.n_levels, L.hash_words, L.c,
                                         [&](uint32_t l) { return s_tok[l * WG + threadIdx.x]; });
      if (ok && (deep || acl_needs_confirm(w0, w1, L.c))) {
        ++L.c_cand;
        ok = acl_confirm(A, L, rs_filter(w0));
        L.c_removed += !ok;
      }
      if (ok) {
        L.ans = rs_rule(w0);
        break;
      }
    }
    p += step;
  }
}

// The lane's result; with counters on, its four counts go to LDS (the record tile is free now).
__device__ __forceinline__ void acl_ph_finish(const AclArgs& A, AclLane& L, uint64_t* s_tile) {
  if (L.t < A.n) A.out[L.t] = L.ans;
  if (L.bad) *A.err = 1u;
  if (A.ctr) {
    s_tile[ACL_CTR_CAND * WG + threadIdx.x] = L.c_cand;
    s_tile[ACL_CTR_REMOVED * WG + threadIdx.x] = L.c_removed;
    s_tile[ACL_CTR_DEEP * WG + threadIdx.x] = L.active && L.n_levels > RS_MAX_LEVELS;
    s_tile[ACL_CTR_VISITED * WG + threadIdx.x] = L.c_visited;
  }
}

// Lane c < ACL_CTRS of each wave adds up counter c of its wave's 64 lanes: one atomic per wave
// and counter.
__device__ __forceinline__ void acl_ph_counters(const AclArgs& A, const uint64_t* s_tile) {
  if (!A.ctr) return;
  const uint32_t c = threadIdx.x & 63u, w0 = threadIdx.x & ~63u;
  if (c >= ACL_CTRS) return;
  unsigned long long sum = 0;
  for (uint32_t i = 0; i < 64; ++i) sum += s_tile[c * WG + w0 + i];
  if (sum) atomicAdd(&A.ctr[c], sum);
}

__global__ __launch_bounds__(WG) void k_acl(AclArgs A) {
  __shared__ uint64_t s_tok[RS_MAX_LEVELS * WG];  // [level][lane], 32 KB
  __shared__ uint64_t s_tile[RS_TILE_WORDS];      // 8 KB
  AclLane L;
  acl_ph_tokenize(A, L, s_tok);
  __syncthreads();
  const uint32_t tiles = rs_n_tiles(A.total_words);
  for (uint32_t k = 0; k < tiles; ++k) {
    acl_ph_stage(A, k, s_tile);
    __syncthreads();
    acl_ph_walk(A, L, s_tok, s_tile);
    __syncthreads();
  }
  acl_ph_finish(A, L, s_tile);
  __syncthreads();
  acl_ph_counters(A, s_tile);
}
