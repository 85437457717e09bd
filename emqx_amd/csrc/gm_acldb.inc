// gm_acldb.inc -- emqx_authz_mnesia:authorize/4 per request against the resident built-in database
// (included by gm_kernels.hip; DESIGN.md 6b "Built-in database").
//
// authorize/4 (apps/emqx_authz/src/emqx_authz_mnesia.erl:98-120) reads the record keyed by the
// client's id, the one keyed by its username and the `all` record, and do_authorize/4 (:222-229)
// takes the first rule of clientid ++ username ++ all that matches, each rule compiled as
// {Permission, all, Action, [TopicFilter]}.
//
// One lane per request (client, publish | subscribe, name), block b owns requests
// [WG b, WG b + WG).  A lane tokenises its name into LDS and derives its client's words as k_acl
// does (gm_acl.inc).  It then probes the client-id table with the id's token and walks the run it
// finds from global memory: the slot is one 16-byte load, the run's words are consecutive, so a
// lane streams its own record and nothing of any other client's.  Lanes still undecided do the
// same with the username.  Last, the block stages the `all` stream tile by tile through LDS and
// the lanes still undecided walk it, exactly as k_acl walks its list.  The work of a request is
// its client's own rules plus the `all` rules, whatever the number of keys.
//
// A key hit on a hashed token is confirmed on the key's bytes, a filter hit wherever k_acl
// confirms one.  A lane that meets a malformed run, slot or record sets the error word and never
// follows the index (adb_ph_lookup, adb_walk_run).
//
// The kernel body is a sequence of per-lane phase functions separated by barriers and nothing
// else; tests/host_harness/acldb_dev_main.cpp runs each phase for all WG lanes of a block before
// the next, under ASan + UBSan.  Every lane walks every barrier.  LDS is k_acl's: 32 KB of tokens
// and the 8 KB tile, four blocks per CU.

constexpr uint32_t ADB_CTR_KEY = 0;        // key hits sent to the byte check
constexpr uint32_t ADB_CTR_KEY_REMOVED = 1;
constexpr uint32_t ADB_CTR_CAND = 2;       // filter candidates sent to the byte check
constexpr uint32_t ADB_CTR_REMOVED = 3;
constexpr uint32_t ADB_CTR_DEEP = 4;       // names deeper than RS_MAX_LEVELS
constexpr uint32_t ADB_CTRS = 5;
static_assert(ADB_CTRS * WG <= RS_MAX_LEVELS * WG, "the counters are reduced through the token array");

struct AdbLane {
  uint32_t t, active;
  uint32_t n0, tl;
  uint32_t n_levels, hash_words;
  uint32_t action;
  uint32_t c0, cl, u0, ul;
  AclClient c;
  uint32_t perm, src, pos;  // the answer (perm NONE: pending)
  uint32_t live, cur_perm;  // `all` tiles: the current rule passed its action; its permission
  uint32_t bad;
  uint32_t c_key, c_key_removed, c_cand, c_removed;
};

__device__ __forceinline__ void adb_ph_tokenize(const AclDbArgs& A, AdbLane& L, uint64_t* s_tok) {
  L.t = blockIdx.x * WG + threadIdx.x;
  L.active = L.t < A.n;
  L.n0 = L.tl = L.n_levels = L.hash_words = L.action = 0;
  L.c0 = L.cl = L.u0 = L.ul = 0;
  L.c = AclClient();
  L.perm = L.src = L.pos = NONE;
  L.live = L.cur_perm = 0;
  L.bad = 0;
  L.c_key = L.c_key_removed = L.c_cand = L.c_removed = 0;
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
}

// Whether the filter record {w0, w1, lv[]} (absolute filter index f) matches the lane's name with
// the lane's client fed in: the tokens, then the bytes where k_acl confirms.
__device__ __forceinline__ bool adb_filter(const AclDbArgs& A, AdbLane& L, const uint64_t* s_tok, uint64_t w0,
                                           uint64_t w1, const uint64_t* lv, uint32_t f) {
  const bool deep = L.n_levels > RS_MAX_LEVELS;
  bool ok = deep || acl_match_tokens(w0, w1, lv, L.n_levels, L.hash_words, L.c,
                                     [&](uint32_t l) { return s_tok[l * WG + threadIdx.x]; });
  if (ok && (deep || acl_needs_confirm(w0, w1, L.c))) {
    ++L.c_cand;
    if (f >= A.n_filters) {
      L.bad = 1;
      return false;
    }
    const uint32_t f0 = A.fo[f], fl = A.fo[f + 1] - f0;
    ok = acl_match_bytes(A.nb + L.n0, L.tl, A.fb + f0, fl, (rs_flags(w0) & RS_EQ) != 0, A.cb + L.c0, L.cl,
                         A.ub + L.u0, L.ul, L.c.flags);
    L.c_removed += !ok;
  }
  return ok;
}

// The record keyed by the lane's client id (kind ADB_CLIENTID) or username (ADB_USERNAME).
__device__ __forceinline__ void adb_ph_lookup(const AclDbArgs& A, AdbLane& L, const uint64_t* s_tok, uint32_t kind) {
  if (!L.active || L.perm != NONE) return;
  const bool usr = kind == ADB_USERNAME;
  if (L.c.flags & (usr ? ACL_C_USR_UNDEF : ACL_C_CID_UNDEF)) return;
  const uint64_t tok = usr ? L.c.usr_tok : L.c.cid_tok;
  const uint8_t* v = usr ? A.ub + L.u0 : A.cb + L.c0;
  const uint32_t vl = usr ? L.ul : L.cl;
  const AdbSlot* tab = (const AdbSlot*)A.tab[kind];
  const uint64_t mask = A.tmask[kind];
  uint64_t i = adb_home(tok, mask), steps = 0;
  uint32_t at;
  while ((at = adb_probe_next(tab, mask, tok, &i, &steps)) != NONE) {
    const uint32_t key = tab[at].key;
    if (key >= A.n_keys) {  // never followed
      L.bad = 1;
      return;
    }
    if (!(tok & TOK_HASHED)) break;
    ++L.c_key;
    const uint32_t k0 = A.ko[key], kl = A.ko[key + 1] - k0;
    if (kl == vl && bytes_equal(A.kb + k0, v, vl)) break;
    ++L.c_key_removed;
  }
  if (at == NONE) return;
  const bool ok = adb_walk_run(A.pool, A.pool_words, tab[at].run, A.n_filters,
                               [&](uint32_t k, uint64_t r0, const uint64_t* rec, uint32_t f) {
                                 if (!acl_match_action(acl_action(r0), L.action)) return false;
                                 if (!adb_filter(A, L, s_tok, rec[0], rec[1], rec + ACL_FILTER_HDR, f)) return false;
                                 L.perm = acl_perm(r0);
                                 L.src = kind;
                                 L.pos = k;
                                 return true;
                               });
  if (!ok) L.bad = 1;
}

// Tile k of the `all` stream into LDS; a short last tile ends in RS_END.
__device__ __forceinline__ void adb_ph_stage(const AclDbArgs& A, uint32_t k, uint64_t* s_tile) {
  const uint32_t span = rs_tile_span(k, A.all_words);
  const uint64_t base = (uint64_t)k * RS_TILE_WORDS;
  for (uint32_t i = threadIdx.x; i < RS_TILE_WORDS; i += WG) s_tile[i] = i < span ? A.all[base + i] : RS_END;
}

__device__ __forceinline__ void adb_ph_walk(const AclDbArgs& A, AdbLane& L, const uint64_t* s_tok,
                                            const uint64_t* s_tile) {
  if (!L.active || L.perm != NONE) return;
  for (uint32_t p = 0; p < RS_TILE_WORDS;) {
    const uint64_t w0 = s_tile[p];
    if (w0 == RS_END) break;
    const uint32_t step = acl_step(w0);
    if (p + step > RS_TILE_WORDS) {  // no record straddles a tile (rs_append)
      L.bad = 1;
      break;
    }
    if (acl_is_rule(w0)) {
      L.live = acl_who(w0) == ACL_WHO_ALL && acl_match_action(acl_action(w0), L.action);
      L.cur_perm = acl_perm(w0);
    } else if (L.live) {
      const uint32_t k = rs_rule(w0);
      if (k >= A.all_rules || rs_filter(w0) != k) {
        L.bad = 1;
        break;
      }
      if (adb_filter(A, L, s_tok, w0, s_tile[p + 1], s_tile + p + ACL_FILTER_HDR, A.all_fbase + k)) {
        L.perm = L.cur_perm;
        L.src = ADB_ALL;
        L.pos = k;
        break;
      }
    }
    p += step;
  }
}

// The lane's result; with counters on, its counts go to LDS (the tokens are not read again).
__device__ __forceinline__ void adb_ph_finish(const AclDbArgs& A, AdbLane& L, uint64_t* s_tok) {
  if (L.t < A.n) {
    A.out_perm[L.t] = L.perm;
    A.out_src[L.t] = L.src;
    A.out_pos[L.t] = L.pos;
  }
  if (L.bad) *A.err = 1u;
  if (A.ctr) {
    s_tok[ADB_CTR_KEY * WG + threadIdx.x] = L.c_key;
    s_tok[ADB_CTR_KEY_REMOVED * WG + threadIdx.x] = L.c_key_removed;
    s_tok[ADB_CTR_CAND * WG + threadIdx.x] = L.c_cand;
    s_tok[ADB_CTR_REMOVED * WG + threadIdx.x] = L.c_removed;
    s_tok[ADB_CTR_DEEP * WG + threadIdx.x] = L.active && L.n_levels > RS_MAX_LEVELS;
  }
}

// Lane c < ADB_CTRS of each wave adds up counter c of its wave's 64 lanes.
__device__ __forceinline__ void adb_ph_counters(const AclDbArgs& A, const uint64_t* s_tok) {
  if (!A.ctr) return;
  const uint32_t c = threadIdx.x & 63u, w0 = threadIdx.x & ~63u;
  if (c >= ADB_CTRS) return;
  unsigned long long sum = 0;
  for (uint32_t i = 0; i < 64; ++i) sum += s_tok[c * WG + w0 + i];
  if (sum) atomicAdd(&A.ctr[c], sum);
}

__global__ __launch_bounds__(WG) void k_acldb(AclDbArgs A) {
  __shared__ uint64_t s_tok[RS_MAX_LEVELS * WG];  // [level][lane], 32 KB
  __shared__ uint64_t s_tile[RS_TILE_WORDS];      // 8 KB
  AdbLane L;
  adb_ph_tokenize(A, L, s_tok);
  __syncthreads();
  adb_ph_lookup(A, L, s_tok, ADB_CLIENTID);
  __syncthreads();
  adb_ph_lookup(A, L, s_tok, ADB_USERNAME);
  __syncthreads();
  const uint32_t tiles = rs_n_tiles(A.all_words);
  for (uint32_t k = 0; k < tiles; ++k) {
    adb_ph_stage(A, k, s_tile);
    __syncthreads();
    adb_ph_walk(A, L, s_tok, s_tile);
    __syncthreads();
  }
  adb_ph_finish(A, L, s_tok);
  __syncthreads();
  adb_ph_counters(A, s_tok);
}
