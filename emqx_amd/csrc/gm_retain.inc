// gm_retain.inc -- reverse match for the retainer: subscription filters -> stored retained
// topics (included by gm_kernels.hip).  SURVEY 8f rank 4.
//
// emqx_retainer_mnesia:match_messages/3 (apps/emqx_retainer/src/emqx_retainer_mnesia.erl:185-195)
// selects the stored messages whose topic word list matches the ETS pattern condition/1 of the
// filter (emqx_retainer_index.erl:97-112): '+' any one word, a last '#' any tail (including
// none), every other word itself; no '$' rule; expiry 0 or > Now (search_table/3, :300-330).
// With index specs configured (the reference's default) search_table/3 matches the index keys
// of the best-scoring index instead (condition/2, emqx_retainer_index.erl:174-200); the host
// (gm_retain.cpp plan_filters) turns that into this walk's terms: a filter cut after its first
// '#', and a per-filter open tail -- when the filter ends before the index's positions do, the
// index part of the pattern stays open, so topics up to `tail` words longer than the filter are
// selected too (any words there).
//
// Store layout (gm_retain.cpp, rebuilt at commit): the stored topics sorted in word order form a
// trie whose nodes are numbered in preorder, so the topics under a node are one contiguous run
// [tb, te) of the sorted order, and a node that is itself a topic is the first of its run.
//   node v: rn[v] = {tb | RTERM, te, c0, c1}; its children (ascending) are rch[c0 .. c1)
//   rw[v] = {pool offset, length} of v's word (checked bytewise when its token is hashed)
//   edge slots: 16 B {tok.lo, tok.hi, parent, child}, (parent, token) key as in the match trie
// A walk over one filter is a DFS: a literal word follows one edge, '+' iterates the children
// (a frame per '+' level), a last '#' selects the whole run of the node, the end of the filter
// selects the node itself if it is a topic.  Runs come out in ascending topic order.  Then
// runs are expanded to topic ids (expired and deleted ones dropped) by one wave per run.
//
// Two stores answer together: the base (built at a full commit) and a small delta store of the
// topics stored since (rebuilt at every commit); a filter's runs are its base runs, then its
// delta runs (tagged RUN_DELTA).  Deleting or re-storing a base topic patches its expiry word
// (RDEAD = deleted), so small changes never rebuild the base.

constexpr uint32_t RTERM = 0x80000000u;
constexpr uint32_t RUN_DELTA = 0x80000000u;  // run lo bit: a run of the delta store
constexpr uint64_t RDEAD = ~0ull;            // expiry word of a deleted base topic

struct RetainArgs {
  const uint8_t* fb;     // filters
  const uint32_t* fo;    // [n+1]
  uint32_t n;
  const uint4* rn;       // nodes
  const uint4* redge;    // edge slots
  uint64_t rmask;        // edge slots - 1
  const uint32_t* rch;   // children lists
  const uint2* rw;       // node words
  const uint8_t* pool;   // topic bytes
  const uint8_t* tail;   // [n] open index tail per filter (words), or null (none)
  uint4* frames;         // [n * max_plus] DFS frames {cursor, end, next pos, tail left}
  uint32_t max_plus;     // frames per filter: its '+' words + its tail
  uint32_t* cnt;         // [n] runs per filter (count pass)
  const uint32_t* cnt_in; // count pass: added to this store's runs (base counts), or null
  const uint32_t* rbase; // [n+1] scanned cnt (fill pass)
  const uint32_t* rshift; // fill pass: runs written after this many (base counts), or null
  uint32_t tag;          // RUN_DELTA for the delta store, else 0
  uint2* runs;           // [runs] {lo | tag, hi}
};

// Child of v by the word f[p, e), or NONE.
__device__ __forceinline__ uint32_t retain_child(const RetainArgs& A, uint32_t v, const uint8_t* f,
                                                 uint32_t p, uint32_t e) {
  uint64_t packed = 0, fnv = FNV_OFF;
  for (uint32_t q = p; q < e; ++q) {
    const uint32_t b = f[q];
    if (q - p < 8) packed |= (uint64_t)b << (8 * (q - p));
    fnv = fnv_step(fnv, b);
  }
  const uint32_t wl = e - p;
  const uint64_t tok = word_token(packed, fnv, wl, 0);
  for (uint64_t i = edge_slot(v, tok, A.rmask);; i = (i + 1) & A.rmask) {
    const uint4 s = A.redge[i];
    if (s.z == NONE) return NONE;
    if (s.z != v || s.x != (uint32_t)tok || s.y != (uint32_t)(tok >> 32)) continue;
    if (!(tok & TOK_HASHED)) return s.w;
    const uint2 w = A.rw[s.w];  // hashed token: the word itself decides
    if (w.y != wl) continue;
    bool eq = true;
    for (uint32_t q = 0; eq && q < wl; ++q) eq = (A.pool[w.x + q] == f[p + q]);
    if (eq) return s.w;
  }
}

template <bool FILL>
__global__ __launch_bounds__(WG) void k_retain_walk(RetainArgs A) {
  const uint32_t fi = blockIdx.x * WG + threadIdx.x;
  if (fi >= A.n) return;
  const uint8_t* f = A.fb + A.fo[fi];
  const uint32_t fl = A.fo[fi + 1] - A.fo[fi];
  uint4* fr = A.frames + (uint64_t)fi * A.max_plus;
  uint32_t depth = 0, runs = 0;
  uint32_t w = FILL ? A.rbase[fi] + (A.rshift ? A.rshift[fi] : 0u) : 0u;
  uint32_t v = 0, p = 0;  // state: node v, the filter's next word starts at byte p
  uint32_t rem = A.tail ? A.tail[fi] : 0u;  // tail levels left once every word is consumed
  auto emit = [&](uint32_t lo, uint32_t hi) {
    if (FILL) A.runs[w++] = make_uint2(lo | A.tag, hi);
    ++runs;
  };
  for (;;) {
    bool live = true;
    while (live) {
      if (p > fl) {  // all words consumed: the node itself, if it is a stored topic
        const uint4 nd = A.rn[v];
        if (nd.x & RTERM) emit(nd.x & ~RTERM, (nd.x & ~RTERM) + 1);
        // an open index tail: every child, down to `rem` more levels (preorder keeps the runs
        // ascending)
        if (rem > 0 && nd.z < nd.w && depth < A.max_plus)
          fr[depth++] = make_uint4(nd.z, nd.w, fl + 1, rem - 1);
        live = false;
        break;
      }
      uint32_t e = p;
      while (e < fl && f[e] != '/') ++e;
      if (e - p == 1 && f[p] == '#') {  // '#': the whole run (only as the last word)
        if (e == fl) {
          const uint4 nd = A.rn[v];
          emit(nd.x & ~RTERM, nd.y);
        }
        live = false;
      } else if (e - p == 1 && f[p] == '+') {
        const uint4 nd = A.rn[v];
        if (nd.z < nd.w && depth < A.max_plus) fr[depth++] = make_uint4(nd.z, nd.w, e + 1, rem);
        live = false;  // children are taken from the frame below
      } else {
        const uint32_t c = retain_child(A, v, f, p, e);
        if (c == NONE) {
          live = false;
        } else {
          v = c;
          p = e + 1;
        }
      }
    }
    // next child of the innermost '+' frame with children left
    while (depth > 0 && fr[depth - 1].x >= fr[depth - 1].y) --depth;
    if (depth == 0) break;
    uint4 t = fr[depth - 1];
    v = A.rch[t.x];
    p = t.z;
    rem = t.w;
    t.x += 1;
    fr[depth - 1] = t;
  }
  if (!FILL) A.cnt[fi] = runs + (A.cnt_in ? A.cnt_in[fi] : 0u);
}

struct RunArgs {
  const uint2* runs;
  uint32_t nr;
  const uint64_t* sexp0;  // base store: expiry per sorted position (RDEAD: deleted)
  const uint32_t* sid0;   //   topic id per sorted position
  const uint64_t* sexp1;  // delta store
  const uint32_t* sid1;
  uint64_t now;
  uint32_t* acnt;         // [nr] live ids per run (count pass)
  const uint32_t* abase;  // [nr+1] scanned acnt (fill pass)
  uint32_t* out;
  unsigned long long* total;
};

// One wave per run: count (or write, in order) the ids of its live topics.
template <bool FILL>
__global__ __launch_bounds__(WG) void k_retain_runs(RunArgs A) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * WG + threadIdx.x) >> 6;
  const uint32_t nw = (gridDim.x * WG) >> 6;
  for (uint32_t r = wave; r < A.nr; r += nw) {
    const uint2 run = A.runs[r];
    const bool dl = (run.x & RUN_DELTA) != 0;
    const uint64_t* sexp = dl ? A.sexp1 : A.sexp0;
    const uint32_t* sid = dl ? A.sid1 : A.sid0;
    const uint32_t lo = run.x & ~RUN_DELTA;
    uint32_t c = 0, o = FILL ? A.abase[r] : 0u;
    for (uint32_t b = lo; b < run.y; b += 64) {
      const uint32_t i = b + lane;
      bool live = i < run.y;
      if (live) {
        const uint64_t e = sexp[i];
        live = e != RDEAD && (e == 0 || e > A.now);
      }
      const uint64_t m = __ballot(live);
      if (FILL && live) A.out[o + __popcll(m & ((1ull << lane) - 1))] = sid[i];
      o += __popcll(m);
      c += __popcll(m);
    }
    if (!FILL && lane == 0) {
      A.acnt[r] = c;
      atomicAdd(A.total, (unsigned long long)c);
    }
  }
}

// ptr[f] = abase[rbase[f]] (first id of filter f), ptr[n] = ids in all
__global__ __launch_bounds__(WG) void k_retain_ptr(const uint32_t* rbase, const uint32_t* abase,
                                                   uint32_t n, uint32_t* ptr) {
  const uint32_t f = blockIdx.x * WG + threadIdx.x;
  if (f <= n) ptr[f] = abase[rbase[f]];
}

// ---- limited reads (emqxgm_retain_match_limit): a window of each filter's ids ----
// The dispatcher reads retained messages batch_read_number at a time through a cursor
// (emqx_retainer_mnesia.erl:185-202, qlc_next_answers/2 :384-397).  The walk produces the runs
// as for the unlimited match; k_retain_runs_win then looks only at the part of each run at or
// after its filter's resume position (host-computed from the cursor: rb[f] in the base store,
// rd[f] in the delta store; the store's size skips the store), and the fill pass writes only
// the first win[f] live ids of filter f.  A live id's rank in its filter is its global rank
// (abase) minus abase[rbase[f]], so the walk needs no output beyond the runs.
//
// Written as per-lane functions with the wave's ballot between them (rw_open, rw_live, rw_put):
// the kernel below is their only device caller, and the host harness
// (tests/host_harness/retain_dev_main.cpp) runs the same functions for lanes 0 .. 63 in turn
// with the ballot computed between the phases.

struct RunWinArgs {
  const uint2* runs;
  uint32_t nr;
  const uint32_t* rbase;  // [n+1] first run of each filter
  uint32_t n;
  const uint32_t* rb;     // [n] resume position in the base store
  const uint32_t* rd;     // [n] resume position in the delta store
  const uint64_t* sexp0;  // base store
  const uint32_t* sid0;
  const uint64_t* sexp1;  // delta store
  const uint32_t* sid1;
  uint64_t now;
  uint32_t* acnt;         // [nr] live ids of each clipped run (count pass)
  const uint32_t* abase;  // [nr+1] scanned acnt (fill pass)
  const uint32_t* win;    // [n] ids to write per filter (fill pass)
  const uint32_t* wptr;   // [n+1] scanned win: the output rows
  uint32_t* out;
  uint2* last;            // [n] {RUN_DELTA or 0, sorted position} of the id of rank win - 1
  unsigned long long* total;  // count pass: live ids of all clipped runs (the ranks are 32-bit)
};

// One clipped run as its wave sees it (the same in every lane).
struct RwRun {
  const uint64_t* sexp;
  const uint32_t* sid;
  uint32_t f;     // the run's filter
  uint32_t tag;   // RUN_DELTA or 0
  uint32_t lo, hi;  // clipped positions [lo, hi)
  uint32_t rank;  // fill: rank in the filter of the run's first live id
  uint32_t w;     // fill: the filter's window
};

// The filter of run r: the last f with rbase[f] <= r (filters without runs repeat their
// neighbour's rbase and are passed over).  r < rbase[n].
__device__ __forceinline__ uint32_t rw_filter(const uint32_t* rbase, uint32_t n, uint32_t r) {
  uint32_t lo = 0, hi = n;  // rbase[lo] <= r < rbase[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (rbase[mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

template <bool FILL>
__device__ __forceinline__ RwRun rw_open(const RunWinArgs& A, uint32_t r) {
  RwRun R;
  const uint2 run = A.runs[r];
  R.f = rw_filter(A.rbase, A.n, r);
  R.tag = run.x & RUN_DELTA;
  R.sexp = R.tag ? A.sexp1 : A.sexp0;
  R.sid = R.tag ? A.sid1 : A.sid0;
  const uint32_t from = R.tag ? A.rd[R.f] : A.rb[R.f];
  R.lo = run.x & ~RUN_DELTA;
  if (R.lo < from) R.lo = from;
  R.hi = run.y;
  R.rank = 0;
  R.w = 0;
  if (FILL) {
    R.rank = A.abase[r] - A.abase[A.rbase[R.f]];
    R.w = A.win[R.f];
  }
  return R;
}

// Is position i of the run a live topic (one coalesced 8-byte load per lane)?
__device__ __forceinline__ bool rw_live(const RwRun& R, uint32_t i, uint64_t now) {
  if (i >= R.hi) return false;
  const uint64_t e = R.sexp[i];
  return e != RDEAD && (e == 0 || e > now);
}

// Fill: a live lane whose rank is inside the window writes its id; the window's last rank
// also leaves where it was found.
__device__ __forceinline__ void rw_put(const RunWinArgs& A, const RwRun& R, uint32_t i, bool live,
                                       uint32_t rank) {
  if (!live || rank >= R.w) return;
  A.out[A.wptr[R.f] + rank] = R.sid[i];
  if (rank + 1 == R.w) A.last[R.f] = make_uint2(R.tag, i);
}

// One wave per run, as k_retain_runs.
template <bool FILL>
__global__ __launch_bounds__(WG) void k_retain_runs_win(RunWinArgs A) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * WG + threadIdx.x) >> 6;
  const uint32_t nw = (gridDim.x * WG) >> 6;
  for (uint32_t r = wave; r < A.nr; r += nw) {
    RwRun R = rw_open<FILL>(A, r);
    if (FILL && R.rank >= R.w) continue;  // past the window: no expiry word is read
    uint32_t c = 0;
    for (uint32_t b = R.lo; b < R.hi; b += 64) {
      const uint32_t i = b + lane;
      const bool live = rw_live(R, i, A.now);
      const uint64_t m = __ballot(live);
      if (FILL) rw_put(A, R, i, live, R.rank + c + __popcll(m & ((1ull << lane) - 1)));
      c += __popcll(m);
      if (FILL && R.rank + c >= R.w) break;
    }
    if (!FILL && lane == 0) {
      A.acnt[r] = c;
      atomicAdd(A.total, (unsigned long long)c);
    }
  }
}

// Per filter: tot = live ids at or after its cursor, win = min(limit, tot) (limit 0: all).
__device__ __forceinline__ void rw_window(const uint32_t* rbase, const uint32_t* abase,
                                          const uint32_t* limit, uint32_t f, uint32_t* tot,
                                          uint32_t* win) {
  const uint32_t t = abase[rbase[f + 1]] - abase[rbase[f]];
  const uint32_t l = limit[f];
  tot[f] = t;
  win[f] = (l != 0 && l < t) ? l : t;
}

__global__ __launch_bounds__(WG) void k_retain_win(const uint32_t* rbase, const uint32_t* abase,
                                                   const uint32_t* limit, uint32_t n, uint32_t* tot,
                                                   uint32_t* win) {
  const uint32_t f = blockIdx.x * WG + threadIdx.x;
  if (f < n) rw_window(rbase, abase, limit, f, tot, win);
}
