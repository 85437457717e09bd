// gm_admit.inc -- k_admit: emqx_topic:validate/2, emqx_topic:parse/1 and the caps clauses of
// emqx_mqtt_caps per item of a batch of names or filters (included by gm_kernels.hip; DESIGN.md
// 6b "Admission").  The per-item code is gm_admit_match.h's, shared with the host.
//
// One lane per item, block b owns items [WG b, WG b + WG).  The block stages its items' packed
// bytes in LDS with stage_tile (gm_tok.inc) and each lane scans its item there, 8 bytes at a
// time; a tile that does not fit (any tile with a 64 KB item) reads global memory through
// AdmGlob, with the same results.  The zones' caps are staged once per block.  Output is one
// 16-byte store per item: {validate | parse << 8 | caps reason << 16 | flags, levels, topic
// offset, share-name length}.
//
// The kernel body is a sequence of per-lane phase functions separated by barriers and nothing
// else, and every lane walks every barrier; tests/host_harness/admit_dev_main.cpp runs each phase
// for all WG lanes of a block before the next, under ASan + UBSan.  No atomics.  An offset that
// decreases or points past the pass's bytes, or a zone past the table, sets the error word and is
// never followed: the item's record is all ones.

struct AdmLane {
  uint32_t t, active;
  uint32_t ob, len;
  uint32_t in_flags, zone;
  uint32_t tiled, s;  // the block's tile fits LDS; the item's byte offset in the tile
  uint32_t bad;
  AdmRecord r;
};

// The lane's offsets, flags and zone; the zones' caps and the tile's bytes into LDS.
__device__ __forceinline__ void adm_ph_stage(const AdmitArgs& A, AdmLane& L, uint4* s_buf, uint2* s_caps) {
  const uint32_t t0 = blockIdx.x * WG, t1 = min(t0 + WG, A.n);
  L.t = t0 + threadIdx.x;
  L.active = L.t < t1;
  L.bad = 0;
  L.ob = L.len = L.in_flags = L.zone = L.tiled = L.s = 0;
  L.r = AdmRecord{NONE, NONE, NONE, NONE};
  if (threadIdx.x < A.n_zones) s_caps[threadIdx.x] = A.caps[threadIdx.x];
  const uint32_t B0 = A.off[t0], B1 = A.off[t1];
  const bool tile_ok = B0 <= B1 && B1 <= A.nbytes;  // (block-uniform)
  if (L.active) {
    const uint32_t ob = A.off[L.t], oe = A.off[L.t + 1];
    if (ob > oe || oe > A.nbytes || !tile_ok || ob < B0 || oe > B1) {
      L.bad = 1;
    } else {
      L.ob = ob;
      L.len = oe - ob;
    }
    if (A.in_flags) L.in_flags = A.in_flags[L.t];
    if (A.zone) L.zone = A.zone[L.t];
    if (L.zone >= A.n_zones) L.bad = 1;
  }
  if (!tile_ok || A.force_global) return;
  uint32_t sh;
  L.tiled = stage_tile(A.bytes, B0, B1, s_buf, sh);
  L.s = sh + (L.ob - B0);
}

// The item's parse and scan, from LDS or from global memory, and its record.
__device__ __forceinline__ void adm_ph_scan(const AdmitArgs& A, AdmLane& L, const uint4* s_buf, const uint2* s_caps) {
  if (!L.active || L.bad) return;
  AdmParse P;
  AdmScan S;
  const bool scan = adm_length_verdict(L.len) == ADM_V_OK;
  if (L.tiled) {
    const AdmLds R{(const uint32_t*)s_buf, L.s};
    if (A.mode == ADM_FILTER) P = adm_parse(R, L.len, (L.in_flags & ADM_IN_HAS_SHARE) != 0);
    if (scan) adm_scan(R, L.len, S);
  } else {
    const AdmGlob R{A.bytes + L.ob, L.len};
    if (A.mode == ADM_FILTER) P = adm_parse(R, L.len, (L.in_flags & ADM_IN_HAS_SHARE) != 0);
    if (scan) adm_scan(R, L.len, S);
  }
  const uint2 c = s_caps[L.zone];
  L.r = adm_record(A.mode, L.len, P, S, L.in_flags, c.x, c.y);
}

__device__ __forceinline__ void adm_ph_store(const AdmitArgs& A, const AdmLane& L) {
  if (!L.active) return;
  if (L.bad) *A.err = 1u;
  A.out[L.t] = make_uint4(L.r.w0, L.r.levels, L.r.off, L.r.share_len);
}

static_assert(WG >= ADM_MAX_ZONES, "one lane stages one zone's caps");

__global__ __launch_bounds__(WG) void k_admit(AdmitArgs A) {
  __shared__ uint4 s_buf[TILE_CHUNKS];
  __shared__ uint2 s_caps[ADM_MAX_ZONES];
  AdmLane L;
  adm_ph_stage(A, L, s_buf, s_caps);
  __syncthreads();
  adm_ph_scan(A, L, s_buf, s_caps);
  __syncthreads();
  adm_ph_store(A, L);
}
