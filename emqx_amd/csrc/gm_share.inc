// gm_share.inc -- emqx_shared_sub:pick/6 per request against the resident membership table
// (included by gm_kernels.hip; DESIGN.md 6b "Shared subscriptions").
//
// One lane per request (group, topic, hc, ht, draw, round_robin state), block b owns requests
// [WG b, WG b + WG).  The block first copies its requests' topic bytes, which are contiguous, into
// LDS when they fit SH_STAGE_BYTES (k_share<true>, the default; MEASUREMENTS.md r16 has the A/B
// against hashing them from global memory, k_share<false>).  A lane hashes its topic's bytes,
// probes the key table with the tag of
// (group, hash), confirms the group and the bytes of every slot whose tag matches, reads the four
// header words of the key's run, decides with sh_decide (gm_share_match.h) and loads the one
// member word the decision names.  Output per request is four u32 in one 16-byte store:
//   {member handle | NONE, SH_* status, round_robin state out, Count | key index when the counter
//    step is pending}.
// The round_robin_per_group counter step is the host's (gm_share.cpp): requests of one call on the
// same key take consecutive counter values in request order, which lanes cannot give each other
// without a segmented sort of the batch.
//
// A lane that finds a key index, a run or a member position out of bounds sets the error word and
// follows nothing.  The kernel body is a sequence of per-lane phase functions separated by
// barriers and nothing else; tests/host_harness/share_dev_main.cpp runs each phase for all WG
// lanes of a block before the next, under ASan + UBSan.  No atomics, no block waits for another;
// LDS holds the staged topic bytes and nothing else.
//
// The probe, the header, the decision and the member load are written over a key given as pointer
// and length (sh_probe_key .. sh_member_answer): k_share's phases call them with the request's
// bytes, k_pubshare's (gm_pubshare.inc) with a filter's bytes in the index's string pool.

struct ShLane {
  uint32_t t, active;
  uint32_t group, k0, kl;
  uint64_t tag;
  uint32_t run, key;  // NONE: no such key
  uint32_t n_all, n_local, strategy;
  ShDecision d;
  uint32_t bad;
};

constexpr uint32_t SH_STAGE_BYTES = 16384;

// With A.stage: the topics of the block's requests, contiguous in rb, into LDS when they fit.
__device__ __forceinline__ void sh_ph_stage(const ShareArgs& A, uint8_t* s_keys) {
  const uint32_t t0 = blockIdx.x * WG, t1 = min(t0 + WG, A.n);
  const uint32_t b0 = A.ro[t0], nb = A.ro[t1] - b0;
  if (nb > SH_STAGE_BYTES) return;
  for (uint32_t i = threadIdx.x; i < nb; i += WG) s_keys[i] = A.rb[b0 + i];
}

// ---- the phase bodies over a key given as pointer and length: k_share's phases below and
// k_pubshare's (gm_pubshare.inc) call these, so a pick is decided by one copy of the code ----

__device__ __forceinline__ void sh_lane_reset(ShLane& L) {
  L.t = L.active = 0;
  L.group = L.k0 = L.kl = 0;
  L.tag = 0;
  L.run = L.key = NONE;
  L.n_all = L.n_local = L.strategy = 0;
  L.d = ShDecision{SH_NO_SUBSCRIBERS, 0, NONE};
  L.bad = 0;
}

// The slot of (L.group, key bytes) by L.tag: L.run and L.key, or both NONE.
__device__ __forceinline__ void sh_probe_key(const ShareTables& T, ShLane& L, const uint8_t* key, uint32_t len) {
  const ShSlot* tab = (const ShSlot*)T.tab;
  uint64_t i = sh_home(L.tag, T.tmask), steps = 0;
  uint32_t at;
  while ((at = sh_probe_next(tab, T.tmask, L.tag, &i, &steps)) != NONE) {
    const uint32_t k = tab[at].key;
    if (k >= T.n_keys) {  // never followed
      L.bad = 1;
      return;
    }
    if (sh_confirm(T.kg, T.ko, T.kb, k, L.group, key, len)) break;
  }
  if (at == NONE) return;
  L.run = tab[at].run;
  L.key = tab[at].key;
}

__device__ __forceinline__ void sh_header_run(const ShareTables& T, ShLane& L) {
  if (!sh_read_run(T.pool, T.pool_words, L.run, &L.n_all, &L.n_local, &L.strategy)) {
    L.bad = 1;
    L.run = NONE;
  }
}

__device__ __forceinline__ void sh_decide_run(ShLane& L, uint32_t hc, uint32_t ht, uint32_t draw) {
  L.d = sh_decide(L.n_all, L.n_local, L.strategy, hc, ht, draw, L.d.state);
  if (L.d.status == SH_MALFORMED) L.bad = 1;
}

// The bounds check of the member position, the error word, and an active lane's answer.
__device__ __forceinline__ uint4 sh_member_answer(const ShareTables& T, ShLane& L, uint32_t* err) {
  if (L.active && !L.bad && L.run != NONE && L.d.status == SH_PICKED &&
      L.d.pos >= sh_run_words(L.n_all, L.n_local))
    L.bad = 1;  // a member position past the run: never followed
  if (L.bad) *err = 1u;
  uint32_t member = NONE, aux = L.n_all;
  if (L.bad) {
    L.d.status = SH_MALFORMED;
  } else if (L.active && L.run != NONE) {
    if (L.d.status == SH_PICKED) member = T.pool[L.run + L.d.pos] & ~SH_LOCAL_BIT;
    if (L.d.status == SH_COUNTER_PENDING) aux = L.key;
  }
  return make_uint4(member, L.d.status, L.d.state, aux);
}

// ---- k_share's phases ----

__device__ __forceinline__ void sh_ph_hash(const ShareArgs& A, ShLane& L, const uint8_t* s_keys) {
  sh_lane_reset(L);
  L.t = blockIdx.x * WG + threadIdx.x;
  L.active = L.t < A.n;
  if (!L.active) return;
  L.group = A.group[L.t];
  L.k0 = A.ro[L.t];
  L.kl = A.ro[L.t + 1] - L.k0;
  L.d.state = A.state[L.t];
  const uint32_t t0 = blockIdx.x * WG, t1 = min(t0 + WG, A.n);
  const uint32_t b0 = A.ro[t0];
  if (s_keys && A.ro[t1] - b0 <= SH_STAGE_BYTES) L.tag = sh_key_tag(L.group, s_keys + (L.k0 - b0), L.kl, A.tag_mask);
  else L.tag = sh_key_tag(L.group, A.rb + L.k0, L.kl, A.tag_mask);
}

__device__ __forceinline__ void sh_ph_probe(const ShareArgs& A, ShLane& L) {
  if (!L.active) return;
  sh_probe_key(A, L, A.rb + L.k0, L.kl);
}

__device__ __forceinline__ void sh_ph_header(const ShareArgs& A, ShLane& L) {
  if (!L.active || L.bad || L.run == NONE) return;
  sh_header_run(A, L);
}

__device__ __forceinline__ void sh_ph_decide(const ShareArgs& A, ShLane& L) {
  if (!L.active || L.bad || L.run == NONE) return;
  sh_decide_run(L, A.hc[L.t], A.ht[L.t], A.draw[L.t]);
}

__device__ __forceinline__ void sh_ph_member(const ShareArgs& A, ShLane& L) {
  const uint4 r = sh_member_answer(A, L, A.err);
  if (L.active) A.out[L.t] = r;
}

template <bool STAGE>
__global__ __launch_bounds__(WG) void k_share(ShareArgs A) {
  __shared__ uint8_t s_keys[STAGE ? SH_STAGE_BYTES : 1];
  ShLane L;
  if (STAGE) {
    sh_ph_stage(A, s_keys);
    __syncthreads();
  }
  sh_ph_hash(A, L, STAGE ? s_keys : nullptr);
  __syncthreads();
  sh_ph_probe(A, L);
  __syncthreads();
  sh_ph_header(A, L);
  __syncthreads();
  sh_ph_decide(A, L);
  __syncthreads();
  sh_ph_member(A, L);
}
