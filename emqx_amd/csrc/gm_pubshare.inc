// gm_pubshare.inc -- emqx_shared_sub:dispatch/3's pick for every aggre entry of a publish pass
// (included by gm_kernels.hip after gm_share.inc; DESIGN.md 6b "The pick inside the publish").
//
// emqx_broker:route/2 (apps/emqx/src/emqx_broker.erl:262-282) hands each {To, Group} entry of
// aggre/1 to emqx_shared_sub:dispatch/3, which looks up the members of (Group, To) and picks one
// (emqx_shared_sub.erl:138-157, 309-379).  k_pubshare runs after k_fanout<FILL> on the same stream
// and the same index epoch and reads the entries where the fan-out left them: one lane per entry e
// of [0, n_routes).  The lane finds its topic t (rp[t] <= e < rp[t + 1]) by a binary search of rp,
// takes the group from o_rd[e] and the key's bytes from the index's string pool (filter o_rf[e]),
// looks the publisher's round_robin state for (group, filter) up in topic t's slice of the state
// list, and then runs the pick of gm_share.inc: the same probe, header, decision and member load,
// called with the key's pointer and length.  The keys of a block lie anywhere in the string pool,
// so they are hashed from global memory; there is no LDS staging as in k_share.
//
// Output per entry is one 16-byte store, {member | NONE, SH_* status, state out, Count | key index
// when the counter step is pending}; an entry whose dest is a node answers {NONE, SH_NOT_SHARED,
// NONE, 0}.  The round_robin_per_group counter step stays the host's (gm_share.cpp
// share_counter_steps), in entry order.
//
// A lane that finds a topic, a filter id, a string-pool range, a key index, a run or a member
// position out of bounds sets the error word and follows nothing.  The body is a sequence of
// per-lane phase functions separated by barriers and nothing else, as k_share's;
// tests/host_harness/pubshare_dev_main.cpp runs each phase for all WG lanes of a block before the
// next, under ASan + UBSan.  No atomics, no LDS, no block waits for another.

struct PsLane {
  ShLane s;       // s.t: the topic that owns the entry; s.active: a group entry with a sound key
  uint32_t e, f;  // the entry, its filter id
  uint32_t in;    // e < n_routes
  const uint8_t* key;
};

// The topic t with rp[t] <= e < rp[t + 1]; empty rows may lie anywhere.  n past the last row
// when rp does not cover e (never followed).
__device__ __forceinline__ uint32_t ps_owner(const uint32_t* rp, uint32_t n, uint32_t e) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (rp[mid + 1] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void ps_ph_owner(const PubShareArgs& A, PsLane& L) {
  sh_lane_reset(L.s);
  L.e = blockIdx.x * WG + threadIdx.x;
  L.f = NONE;
  L.key = nullptr;
  L.in = L.e < A.n_routes;
  if (!L.in) return;
  const uint32_t d = A.o_rd[L.e];
  if (!(d & DEST_GROUP_BIT)) return;  // {To, Node}: nothing to pick
  L.s.group = d & ~DEST_GROUP_BIT;
  L.s.t = ps_owner(A.rp, A.n, L.e);
  if (L.s.t >= A.n || A.rp[L.s.t] > L.e) {
    L.s.bad = 1;
    return;
  }
  L.s.active = 1;
}

// The key's bytes in the string pool, the publisher's state for (group, filter), the tag.
__device__ __forceinline__ void ps_ph_key(const PubShareArgs& A, PsLane& L) {
  if (!L.s.active) return;
  L.f = A.o_rf[L.e];
  if (L.f >= A.n_filters) {  // never followed
    L.s.bad = 1;
    L.s.active = 0;
    return;
  }
  const uint64_t b0 = A.foff[L.f], b1 = A.foff[L.f + 1];
  if (b1 < b0 || b1 - b0 > 0xFFFFFFFFull || b1 > A.pool_bytes) {
    L.s.bad = 1;
    L.s.active = 0;
    return;
  }
  L.key = A.fbytes + b0;
  L.s.kl = (uint32_t)(b1 - b0);
  if (A.st_ptr) {
    // the publisher's process dictionary, passed whole: the first (group, filter) pair wins
    for (uint32_t i = A.st_ptr[L.s.t], i1 = A.st_ptr[L.s.t + 1]; i < i1; ++i)
      if (A.st_group[i] == L.s.group && A.st_filter[i] == L.f) {
        L.s.d.state = A.st_value[i];
        break;
      }
  }
  L.s.tag = sh_key_tag(L.s.group, L.key, L.s.kl, A.tag_mask);
}

__device__ __forceinline__ void ps_ph_probe(const PubShareArgs& A, PsLane& L) {
  if (!L.s.active) return;
  sh_probe_key(A, L.s, L.key, L.s.kl);
}

__device__ __forceinline__ void ps_ph_header(const PubShareArgs& A, PsLane& L) {
  if (!L.s.active || L.s.bad || L.s.run == NONE) return;
  sh_header_run(A, L.s);
}

__device__ __forceinline__ void ps_ph_decide(const PubShareArgs& A, PsLane& L) {
  if (!L.s.active || L.s.bad || L.s.run == NONE) return;
  sh_decide_run(L.s, A.hc[L.s.t], A.ht[L.s.t], A.draw[L.s.t]);
}

__device__ __forceinline__ void ps_ph_out(const PubShareArgs& A, PsLane& L) {
  const uint4 r = sh_member_answer(A, L.s, A.err);
  if (!L.in) return;
  const bool shared = (A.o_rd[L.e] & DEST_GROUP_BIT) != 0;
  A.out[L.e] = shared ? r : make_uint4(NONE, SH_NOT_SHARED, NONE, 0u);
}

__global__ __launch_bounds__(WG) void k_pubshare(PubShareArgs A) {
  PsLane L;
  ps_ph_owner(A, L);
  __syncthreads();
  ps_ph_key(A, L);
  __syncthreads();
  ps_ph_probe(A, L);
  __syncthreads();
  ps_ph_header(A, L);
  __syncthreads();
  ps_ph_decide(A, L);
  __syncthreads();
  ps_ph_out(A, L);
}
