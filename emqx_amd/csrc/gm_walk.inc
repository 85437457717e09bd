// gm_walk.inc -- the persistent trie-walk kernel (included by gm_kernels.hip).
//
// emqx_trie:match_compact/5 (apps/emqx/src/emqx_trie.erl:327-348) restated over the hashed trie:
// for a topic w0/../w(n-1), every trie node reachable by following, level by level, the literal
// edge of the topic's word or the '+' edge (never the root '+' for a '$' topic, :282-289) is a
// matched state; each matched node contributes its "path/#" filters, and the nodes reached after
// the last level contribute the filters that end there.  Every matched node is visited exactly
// once per topic (edges are keyed on the exact parent id), so rows carry no duplicates.
//
// Mapping.  One lane owns one topic at a time.  Its pending work is a LIFO of probe items
// (node, level, literal | '+' | tn), kept in LDS.  Every loop iteration costs the wave ONE
// memory round trip, in which each lane runs up to WSLOTS probes of its topic at once, one
// 64-B bucket (two 32-B edge slots) each (a probe on a collision chain stays in its slot to the
// next iteration).  A resolved probe creates the child state: its filters are emitted and its
// own probe items pushed.  The slot also carries the child's '+' child {cf, hf} (gm_common.h "edge slots"), so
// that state is created on the spot without a probe of its own, unless its terminal filters
// are needed (then one '+' probe fetches them).  Level tokens 0..6 come from the 64-B topic
// record (kept in LDS per lane), deeper ones from the token array.  Matches are appended
// with one wave-wide scan per flush into wave-private chunks of the staging buffer (stored by
// position, whole lines per store); ranks within a topic follow the (deterministic) order of
// emission.
//
// Why 32-B slots: a slot load is a per-lane-divergent access, and the CU's vector memory path
// (TA/TCP/TD) processes every 16-B load instruction lane by lane; with 64-B slots (4 loads)
// that path was ~75% busy (TD_TD_BUSY, profiles/r01) while HBM was far from its limit.

constexpr uint32_t WSLOTS = 2;             // probes in flight per lane per iteration
constexpr uint32_t PAIR_WSLOTS = 2;        // ... per lane of a pair walk (r05: 1 and 3 slower)
// the pair walk ends lookups at closed buckets too (r10: compiled out like LENT / RP / SHARE --
// the pair walk is bound by its instruction count and was not measured with the rule)
constexpr bool WALK_CLOSED_PAIR = false;
// probe items per lane kept in LDS: STK (a k_walk template parameter) = WALK_STK_SHALLOW or
// WALK_STK_DEEP (gm_kernels.h); the spilling variant continues in global memory
constexpr uint32_t EMX = 8;                // emissions per lane per flush (<= 2 + 3 + 3, below)
constexpr uint32_t IT_PLUS = 0x80000000u;  // probe item kinds (in the node word): '+' edge,
constexpr uint32_t IT_TN = 0x40000000u;    //   non-wildcard keys of a node (side array),
constexpr uint32_t IT_KEYED = IT_PLUS | IT_TN;  // a literal child of a keyed node (gm_common.h
                                                //   edge_home); neither bit: a literal child
constexpr uint32_t IT_KIND = IT_PLUS | IT_TN;
constexpr uint32_t EM_MULTI = 0x80000000u; // emission entry is a multi[] list index
// Compact probe items (CPT variants): one 32-bit word, node id (CF_ID_MASK) | kind (IT_PLUS /
// IT_TN) | level in bits 26..29 -- half the LDS of {node, level} pairs, so the shallow stack
// holds 12 items at four blocks per CU and the deep one 24 at three.  An item past the stack or
// of a level >= CPT_LEVELS flags the lane (the batch is redone one variant up, as for a full
// stack: only an index with filters of 16+ levels can produce such an item).
constexpr uint32_t CPT_SHIFT = 26;
constexpr uint32_t CPT_LEVELS = 16;
static_assert(CF_ID_MASK == (1u << CPT_SHIFT) - 1 && (IT_TN >> CPT_SHIFT) == 16u,
              "compact items: level bits between the id and the kinds");

struct WalkArgs {
  const uint4* rec;     // REC_U4 parts per topic, in blocks of 64 topics part-major (rec_at)
  const uint32_t* hdr;  // per topic n_words | flags << 24, when the pass stored fewer parts
  const uint64_t* wh;   // level tokens
  const uint4* edges;
  uint64_t emask;
  const uint32_t* multi;
  const uint32_t* tn_of; // per node: non-wildcard trie keys ending there (id / multi / NONE)
  uint32_t root_cf, root_hf;
  uint32_t root_pcf, root_phf;  // root's '+' child {cf, hf} (cf 0: none)
  uint32_t n;
  uint32_t* ctl;
  uint32_t* cnt;
  uint3* stg;           // staged pairs {topic, filter, rank} (12 B) in CH-slot chunks per wave
  StgFmt fmt;           //   or packed 8-B words (fmt.pk)
  uint32_t* chk;        // per chunk: slots filled (the chunk's first chk[c] slots hold pairs)
  uint32_t pcap;        // a multiple of CH
  uint2* spill;         // probe items beyond STK: [depth - STK][lanes]
  uint32_t spill_items; // spill entries per lane
  uint32_t lanes;
  uint32_t tblk;        // topics claimed per wave per atomic (smaller for small batches)
  uint32_t leafp_mask;  // CF_HMASK (depth-code pruning, gm_common.h) or 0
  uint32_t psig_off;    // 0, or 0x3F: lent signatures pass every class (tune "plus_sig" 0)
  uint32_t stat_chunks; // waves owning a static first chunk of staged pairs (chunk = wave), or 0
  uint32_t static_claim;  // 1: k_tok started the claim counters past each wave's first block
  uint32_t static_one;  // 1: at most one topic per lane of the grid -- lane gl walks topic gl,
                        // no claims (the atomics of a claim loop dominate small batches)
  uint32_t root_sig;    // the root's child signature
  uint4 rh0, rh1;       // the root's fat half (rh0.z low bits FAT_ID), or rh0.z = NONE
  uint4 rp0, rp1;       // the slot of the only literal child of the half's '+' child (create RP),
                        // or rp0.z = NONE (none, more than one, or tune "root_plus_half" 0)
  uint32_t keyed_share; // 1: keyed siblings of a level share the loaded line (tune "keyed_share")
  uint32_t closed_off;  // 0, or 1: closed-bucket marks are ignored (tune "closed_buckets" 0;
                        // gm_common.h slot_closed)
  unsigned long long* census;  // [0] states, [1] slot loads, [2] lane iters, [3] wave iters,
                               // then per wave {start, claims exhausted, end} (wall clock)
  uint64_t c0, c2;      // the even-elided reader (REC_REVEN): the one token of the literal edges
                        // of level 0 / level 2, 0: none (read in the activation block only)
};

// Topic t's 64-B record (gm_common.h rec_at): lanes holding consecutive topics load whole lines
// per instruction (r06; topic-major, each 16-B load of the wave touched a line per lane, on the
// vector memory path the walk is bound by -- TD busy 89% at cfg3).  r05: non-temporal loads
// measured slower (profiles/r05/ab_nt).
// (One address and the parts at immediate offsets of 1 KB: a separate 64-bit address per part,
// for a fully part-major layout, cost the walk 6 VGPRs, past 128.)
// REC (a k_walk template parameter, gm_common.h REC_R*): REC_RFULL, the pass stored all REC_U4
// parts; REC_R3, REC_PARTS_MIN parts and the header word in A.hdr (gm_common.h rec_parts,
// rec_load) -- one line per 64 topics less to request, and the registers of tok6 and wbase are
// constants; REC_REVEN, the even-elided form's two parts and the header word (rec_load_even) --
// another line less, and one prefetched uint4 (c) stays a constant.
template <uint32_t REC>
__device__ __forceinline__ void load_rec(const WalkArgs& A, uint32_t t, uint4& a, uint4& b, uint4& c,
                                         uint4& d) {
  if constexpr (REC == REC_REVEN)
    rec_load_even(A.rec, A.hdr, t, a, b, d);
  else
    rec_load<REC == REC_RFULL>(A.rec, A.hdr, t, a, b, c, d);
}

struct WaveOut {  // wave-uniform cursor into this wave's reserved chunk of staged pairs
  uint32_t pos, end;
};

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t& total) {
  const uint32_t lane = lane_id();
  uint32_t x = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  total = __builtin_amdgcn_readlane(x, 63);  // wave-uniform (SGPR)
  return x - v;
}

// Records how many slots of the wave's current chunk it filled (chk[chunk]); the rest of the
// chunk is never read (k_verify / k_scatter walk chunk by chunk up to the fill), so nothing is
// written there.
__device__ __forceinline__ void close_chunk(const WaveOut& o, const WalkArgs& A) {
  if (o.end != 0 && o.end <= A.pcap && lane_id() == 0) A.chk[(o.end - CH) / CH] = o.pos - (o.end - CH);
}

// Make room for `need` more slots in the wave's chunk (wave-uniform).
__device__ __forceinline__ void reserve(uint32_t need, WaveOut& o, const WalkArgs& A) {
  if (o.pos + need <= o.end) return;
  close_chunk(o, A);
  uint32_t base = 0;
  if (lane_id() == 0) base = atomicAdd(&A.ctl[CTL_PAIR_TOP], CH);
  base = __builtin_amdgcn_readfirstlane(base);  // every lane is active here
  o.pos = base;
  o.end = base + CH;
}

// PKO (the pair walk): packed only, no wide path compiled in -- the runtime choice cost the pair
// variant 10 VGPRs, 121 -> 131, one wave per SIMD (cfg1's walk 37 -> 51 us: its 782 blocks no
// longer fit at once).  A pass that must stage wide runs the one-lane-per-topic walk.
template <bool PKO = false>
__device__ __forceinline__ void put(uint32_t i, uint32_t t, uint32_t f, uint32_t r,
                                    const WalkArgs& A) {
  if (i >= A.pcap) return;
  // (the walk's ranks carry no reject bit.  A rank past the field is masked: unmasked it would
  // carry into the filter id, which k_verify and k_scatter use as an index before the host sees
  // CTL_PKOVF and redoes the pass wide)
  if (PKO || A.fmt.pk)  // (wave-uniform)
    ((uint64_t*)A.stg)[i] = ((uint64_t)t << A.fmt.tsh) | ((uint64_t)f << A.fmt.fsh) |
                            ((uint64_t)(r & A.fmt.rmask) << 1);
  else
    A.stg[i] = make_uint3(t, f, r);
}

// One emission round for a single id per lane (multi-list path).
template <bool PKO = false>
__device__ __forceinline__ void emit1(bool v, uint32_t t, uint32_t f, uint32_t& rank, WaveOut& o,
                                      const WalkArgs& A) {
  const uint64_t m = __ballot(v);
  if (m == 0) return;
  reserve((uint32_t)__popcll(m), o, A);
  if (v) {
    put<PKO>(o.pos + mbcnt64(m), t, f, rank, A);
    ++rank;
  }
  o.pos += (uint32_t)__popcll(m);
}

// Emit every id of a multi[] list (filters sharing one trie node by level-token collision).
template <bool PKO = false>
__device__ __forceinline__ void emit_multi(bool has, uint32_t idx, uint32_t t, uint32_t& rank,
                                           WaveOut& o, const WalkArgs& A) {
  if (__ballot(has) == 0) return;
  const uint32_t cntm = has ? A.multi[idx] : 0u;
  for (uint32_t j = 0; __ballot(has && j < cntm) != 0; ++j) {
    const bool v = has && j < cntm;
    emit1<PKO>(v, t, v ? A.multi[idx + 1 + j] : 0u, rank, o, A);
  }
}

// Per-lane walk context shared by the helpers below.
struct Lane {
  uint32_t tid, gl;
  uint32_t tcol;  // the s_tw column of the lane's topic (its own; a pair's: the leading lane's)
  uint32_t n, fl, sp, ne;
  uint32_t np;  // entries of s_em[0, min(ne, EMX)) that are plain ids (not multi[] lists)
  uint32_t cls; // sig_class of the topic's record tokens, 3 bits per level (set at activation)
  bool overflow;
};

// The LDS item stack of a variant: 8-B {node | kind, level} items, or compact 32-bit ones (CPT)
template <bool CPT>
struct ItemT {
  using type = uint2;
};
template <>
struct ItemT<true> {
  using type = uint32_t;
};

struct Probe {
  bool busy, side;  // side: this iteration loads a side word (deep level token / tn list)
  uint32_t cur;     // node id | item kind
  uint32_t k;       // level probed
  uint64_t key, ia; // ia: bucket index
  uint64_t skey;    // side word as loaded (its own register: see the issue phase)
  uint4 s0, s1, t0, t1;  // the bucket's two slots
};

template <bool SPILL, uint32_t STK, bool CPT>
__device__ __forceinline__ void push_item(Lane& L, typename ItemT<CPT>::type (*s_stk)[WG],
                                          const WalkArgs& A, uint32_t node, uint32_t k) {
  if constexpr (CPT) {
    if (L.sp < STK && k < CPT_LEVELS) {
      s_stk[L.sp][L.tid] = node | (k << CPT_SHIFT);
      ++L.sp;
    } else {
      L.overflow = true;  // the engine re-runs the batch one variant up: never dropped
    }
  } else {
    if (L.sp < STK) {
      s_stk[L.sp][L.tid] = make_uint2(node, k);
    } else if (SPILL && L.sp - STK < A.spill_items) {
      // non-temporal (a spilled item is read back once): also keeps this store from being
      // merged with the LDS store above into one generic (FLAT) store, whose completion waits
      // would drain every outstanding global load of the wave
      __builtin_nontemporal_store(((uint64_t)k << 32) | node,
                                  (uint64_t*)(A.spill + (uint64_t)(L.sp - STK) * A.lanes + L.gl));
    } else {
      L.overflow = true;  // the engine re-runs the batch with (a larger) spill: never dropped
      return;
    }
    ++L.sp;
  }
}

__device__ __forceinline__ void em(Lane& L, uint32_t (*s_em)[WG], uint32_t v) {
  if (L.ne < EMX) {
    s_em[L.ne][L.tid] = v;
    L.np += (v & EM_MULTI) ? 0u : 1u;
  }
  ++L.ne;
}
__device__ __forceinline__ void em_list(Lane& L, uint32_t (*s_em)[WG], uint32_t v) {
  em(L, s_em, (v & LIST_MULTI) ? (EM_MULTI | (v & ~LIST_MULTI)) : v);
}

// A matched trie state at depth d: its '#' filters, its terminal filters when d == n (and,
// fetched by a tn item, the non-wildcard keys for a single-level '$' topic reached by a literal
// edge, emqx_trie.erl:287), and a literal probe item for level d when it has literal children
// -- unless its depth code says every filter below it ends within h levels and the topic has
// more than h words left (n - d > h): nothing below can match, so no child is expanded.
// A state's flags with its child flags dropped in that case (a select, not a branch: extra
// branches around push_item's LDS-or-spill store make the compiler merge the two address
// spaces into one generic store).
__device__ __forceinline__ uint32_t leaf_strip(uint32_t mask, uint32_t n, uint32_t cf, uint32_t d) {
  const uint32_t h = cf_depth_code(cf & mask);
  return (h != 0u && (int)(n - d) > (int)h) ? (cf & ~(CF_LIT | CF_PLUS)) : cf;
}
template <bool SPILL, uint32_t STK, bool CPT>
__device__ __forceinline__ void visit(Lane& L, typename ItemT<CPT>::type (*s_stk)[WG], uint32_t (*s_em)[WG],
                                      const WalkArgs& A, uint32_t cf, uint32_t hf, uint32_t tw,
                                      uint32_t d, bool lit, uint32_t kind = 0u) {
  if (hf != NONE) em(L, s_em, hf);  // a multi[] index carries LIST_MULTI == EM_MULTI
  if (d == L.n) {
    if (cf & CF_TW) em_list(L, s_em, tw);
    if (lit && (cf & CF_TN) && (L.fl & T_DOLLAR) && L.n == 1)
      push_item<SPILL, STK, CPT>(L, s_stk, A, IT_TN | (cf & CF_ID_MASK), d);
  } else if (cf & CF_LIT) {
    push_item<SPILL, STK, CPT>(L, s_stk, A, (cf & CF_ID_MASK) | kind, d);
  }
}

// State `cf` at depth d plus its carried '+' child {pcf, phf} at depth d+1.  The carried copy
// holds the child's '#' filter, or, flagged CF_PTW (gm_common.h), its terminal filters when it
// has no '#' filter; only a child with both, when its terminal filters are needed (d+1 == n),
// takes a '+' probe to fetch its full slot.  Its own '+' child is always a '+' probe.
// `plus_ok` = false drops the '+' child (the root of a '$' topic, emqx_trie.erl:282-289).
// `sig` = the state's child signature (gm_common.h sig_bit): when word d's class bit is clear no
// literal child can match it, so the literal probe is dropped (a select on CF_LIT).  Levels
// past the record's tokens are not filtered.  With CF_LIT clear in `cf` the field is lent to the
// carried '+' child (gm_common.h): it summarises that child's literal children, and the literal
// probe under it is dropped the same way when word d+1's class bit is clear.
// `fat`: the state's only literal child G comes with it (gm_common.h FAT_ID: the second half of
// the state's bucket, or the root's half in the arguments), {h0, h1} = G's slot.  Its literal
// children are then never probed by hash: G's state is created here, in the same round trip,
// when word d equals G's token (fat states have d <= FAT_MAX_DEPTH < REC_TOKS), and nothing is
// when it does not.
// LENT = false compiles the lent-signature filter out and keeps r06's per-state code (the own
// filter from a sig_bit of the token): the pair walk, which runs where the walk is bound by its
// instruction count (small batches, indexes whose walks outgrow a lane's stack: cfg1, cfg2), lost
// 1-2% to the filter's instructions in every form measured (MEASUREMENTS r07) and meets few
// such probes; the one-lane-per-topic walks and the census have it.
// RP (the root's '+' half, with LENT in the same walks): 1 = the root's state, which hands 2 to
// its fat half G's.  G's carried '+' child p then takes no literal item when p's literal children
// are one node H alone and the arguments carry H's slot (A.rp0/rp1, a copy: H keeps its slot in
// the table, and "absent" is always right): word d+1 against H's token decides here what the
// probe (p, word d+1) would have found a round trip later -- the same hot line for every topic
// of a batch (cfg3: site/+ -> device).  H's state is created exactly as a resolved probe's.
template <bool SPILL, uint32_t STK, bool CPT, bool FAT = false, bool LENT = true, uint32_t RP = 0>
__device__ __forceinline__ void create(Lane& L, typename ItemT<CPT>::type (*s_stk)[WG], uint32_t (*s_em)[WG],
                                       const uint64_t (*s_tw)[WG], const WalkArgs& A,
                                       uint32_t cf, uint32_t hf, uint32_t tw, uint32_t sig,
                                       uint32_t pcf, uint32_t phf, uint32_t d, bool plus_ok,
                                       bool lit, uint32_t& states, bool fat = false,
                                       uint4 h0 = uint4{}, uint4 h1 = uint4{}) {
  fat = FAT && fat;
  // a keyed state (CF_LIT with signature 0, gm_common.h edge_home): its children are placed by
  // token and not summarised by class
  const bool keyed = sig == 0u && (cf & CF_LIT);
  // the carried '+' child's signature (from the unstripped cf): lent, or unknown (every class)
  const uint32_t lent = ((cf & CF_LIT) ? 0x3Fu : sig) | A.psig_off;
  cf = leaf_strip(A.leafp_mask, L.n, cf, d);
  // a fat state's literal child: its token against word d (exact), else the signature filter
  const uint64_t wtok = s_tw[d < REC_TOKS ? d : REC_TOKS - 1][L.tcol];
  const bool fat_go = fat && (cf & CF_LIT) && d < L.n && d < REC_TOKS &&
                      (uint32_t)wtok == h0.x && (uint32_t)(wtok >> 32) == h0.y;
  // sig_bit of words d and d+1, from the classes computed once per topic (a sig_bit per state
  // is two multiplies); past the record's tokens the classes read 0 and the filters below do
  // not apply
  const uint32_t cw = L.cls >> (3u * min(d, REC_TOKS));
  const uint32_t wbit = LENT ? 1u << (cw & 7u) : sig_bit(wtok), pbit = 1u << ((cw >> 3) & 7u);
  cf = (fat || (!keyed && d < REC_TOKS && !(sig & wbit))) ? (cf & ~CF_LIT) : cf;
  pcf = leaf_strip(A.leafp_mask, L.n, pcf, d + 1);
  // The carried '+' child at depth d+1 loses its literal probe when word d+1's class is not
  // among its literal children's (a select, as above).  No `d + 1 < n` guard is needed: this
  // function returns before it expands the carried child when d >= n, and at d + 1 == n
  // visit() takes its `d == n` branch and never looks at CF_LIT (word n's token reads 0).  A
  // change to either must bring the guard back.
  if constexpr (LENT) pcf = (d + 1 < REC_TOKS && !(lent & pbit)) ? (pcf & ~CF_LIT) : pcf;
  visit<SPILL, STK, CPT>(L, s_stk, s_em, A, cf, hf, tw, d, lit, keyed ? IT_KEYED : 0u);
  states += 1;
  if (FAT && fat_go)
    create<SPILL, STK, CPT, false, LENT, (RP == 1 ? 2u : 0u)>(L, s_stk, s_em, s_tw, A, h0.w, h1.x, h1.y,
                                                             h0.z >> SIG_SHIFT, h1.z, h1.w, d + 1,
                                                             true, true, states);
  if (!plus_ok || d >= L.n || !(cf & CF_PLUS)) return;
  const bool ptw = (pcf & CF_PTW) != 0;
  if (d + 1 == L.n && (pcf & CF_TW) && !ptw) {
    push_item<SPILL, STK, CPT>(L, s_stk, A, IT_PLUS | (cf & CF_ID_MASK), d);
    return;
  }
  // (RP: the copy is p's child -- its parent word says so -- and p would take a literal item)
  bool rp = false;
  if constexpr (RP == 2) {
    rp = (A.rp0.z & CF_ID_MASK) == (pcf & CF_ID_MASK) && (pcf & CF_LIT) && d + 1 < L.n;
    pcf = rp ? (pcf & ~CF_LIT) : pcf;
  }
  visit<SPILL, STK, CPT>(L, s_stk, s_em, A, pcf & ~CF_PTW, ptw ? NONE : phf, ptw ? phf : NONE, d + 1, false);
  states += 1;
  if constexpr (RP == 2) {
    const uint64_t ptok = s_tw[d + 1 < REC_TOKS ? d + 1 : REC_TOKS - 1][L.tcol];
    if (rp && (uint32_t)ptok == A.rp0.x && (uint32_t)(ptok >> 32) == A.rp0.y)
      create<SPILL, STK, CPT, false, LENT>(L, s_stk, s_em, s_tw, A, A.rp0.w, A.rp1.x, A.rp1.y,
                                           A.rp0.z >> SIG_SHIFT, A.rp1.z, A.rp1.w, d + 2, true, true,
                                           states);
  }
  if (d + 1 < L.n && (pcf & CF_PLUS))
    push_item<SPILL, STK, CPT>(L, s_stk, A, IT_PLUS | (pcf & CF_ID_MASK), d + 1);
}

// SPILL = false (production): the item stack lives in LDS only, so popping never touches
// global memory (a generic LDS-or-global pop compiles to a FLAT load, which drains every
// outstanding memory operation); a lane that outgrows it flags CTL_ERR and the engine redoes
// the batch with SPILL = true, whose stack continues in global memory.
// LDS of a walk block with a stack of STK items per lane (s_stk, s_em, s_tw; s_dep aside)
constexpr uint32_t walk_lds_bytes(uint32_t stk, bool cpt = false) {
  return WG * (stk * (cpt ? 4u : 8u) + EMX * 4u + REC_TOKS * 8u);
}

// WSLOTS probe slots per lane: more slots cost registers, hence resident waves, and the walk is
// bound by the memory system's request rate (r01: 3 slots slower); for one-topic-per-lane
// batches 4 slots were measured too (r03: cfg1 -6%, cfg3 64k +19%; off -- they changed only
// the emission order, never a row's set: r04 tools/ws_order_check.py).
//
// PAIR (r05, small batches only: static_one with two lanes per topic).  A batch of at most half
// a grid's lanes leaves the SIMDs at ~1.5 waves each (cfg1: 100k topics), where an iteration's
// dependent LDS and memory latencies are not hidden and the walk is its lanes' longest chains.
// Lanes 2i and 2i+1 then walk topic i together, four probes in flight per topic: each keeps its
// own item stack and emission list, and at every fill a lane with a free slot and an empty stack
// takes items from the top of its partner's (after the partner's own pops).  The pair's rank
// counter stays equal in both lanes: at a flush the leading lane's ids come first.  Everything the
// pair exchanges is one DPP move between neighbouring lanes (no LDS round trip).  The emission
// order of a topic is then a function of the topic and the index, as without pairs, but a
// different one: rows are sets (emqx_trie:match/1 is tested with lists:sort).
__device__ __forceinline__ uint32_t pair_xchg(uint32_t v) {
  // quad_perm [1, 0, 3, 2]: lane i reads lane i ^ 1 (both lanes of a pair are always active here)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}


// SHARE (r09; the compact one-lane-per-topic walks).  An IT_KEYED item's home bucket is a hash of
// its level's token alone (gm_common.h edge_home), so the keyed items of one topic at one level
// probe the same line (cfg3: site/+/device -> D and site/S/device -> D).  When slot 0 is filled
// with a keyed probe at its home, a keyed item of the same level on top of the stack is not given
// a slot of its own: it stays there, and after the resolves the first such item on the stack from
// that point up -- those pushed by this iteration's resolves included -- is decided from slot 0's
// line, still in its registers: found -> its child state is created now; the bucket has an empty
// slot -> no such child; a full bucket of other keys -> the item stays and is probed the ordinary
// way from its home.  One item per lane and iteration (a loop over all of them, with its flush,
// cost the cfg3 kernel a wave per SIMD: MEASUREMENTS r09); a further sibling takes its own probe.
// Only slot 0 anchors a shared line: its fields are read at a constant index (a select between
// two P[] fields puts the array into scratch).  A slot that has moved along a chain is not at an
// item's home and shares nothing.
template <bool CENSUS, bool SPILL, uint32_t STK, bool CPT = false, bool PAIR = false, uint32_t REC = REC_RFULL>
__global__ __launch_bounds__(WG) void k_walk(WalkArgs A) {
  static_assert(REC != REC_REVEN || (!SPILL && !PAIR), "the even-elided reader: the one-lane LDS-only walks");
  static_assert(!(CPT && SPILL), "compact items live in LDS only");
  static_assert(!PAIR || (CPT && !SPILL && !CENSUS), "pairs: the compact LDS-only production walk");
  constexpr uint32_t NS = PAIR ? PAIR_WSLOTS : WSLOTS;  // probe slots per lane
  constexpr bool SHARE = CPT && !PAIR;
  constexpr uint32_t RP = PAIR ? 0u : 1u;  // (the pair walk: compiled out, as LENT is)
  constexpr bool CLOSED = WALK_CLOSED_PAIR || !PAIR;  // closed buckets (gm_common.h EDGE_CLOSED)
  __shared__ typename ItemT<CPT>::type s_stk[STK][WG];
  __shared__ uint32_t s_em[EMX][WG];
  __shared__ uint64_t s_tw[REC_TOKS][WG];  // the lane's topic's level tokens 0..6
  const uint4 ZERO4 = make_uint4(0u, 0u, 0u, 0u);

  Lane L;
  L.tid = threadIdx.x;
  L.gl = blockIdx.x * WG + L.tid;
  L.tcol = PAIR ? (L.tid & ~1u) : L.tid;
  const bool lead = !PAIR || (L.tid & 1u) == 0u;
  L.n = 0;
  L.fl = 0;
  L.sp = 0;
  L.ne = 0;
  L.np = 0;
  L.cls = 0;
  L.overflow = false;
  // topic context (t = NONE: idle) and the next topic, its record prefetched ahead
  uint32_t t = NONE, wb = 0, rank = 0;
  uint32_t nxt = NONE;
  uint4 nr0 = ZERO4, nr1 = ZERO4, nr2 = ZERO4, nr3 = ZERO4;

  Probe P[NS];
#pragma unroll
  for (uint32_t j = 0; j < NS; ++j) {
    P[j].busy = false;
    P[j].side = false;
    P[j].cur = 0;
    P[j].k = 0;
    P[j].key = 0;
    P[j].skey = 0;
    P[j].ia = 0;
    P[j].s0 = P[j].s1 = P[j].t0 = P[j].t1 = ZERO4;
  }

  uint32_t q_next = 0, q_end = 0;
  uint32_t cs = blockIdx.x % WALK_SHARDS, out_seen = 0;  // claim shard, shards seen out (wave-uniform)
  if (A.static_claim && !A.static_one) {
    // this wave's first topic block: block r of its shard, claimed by k_tok's counter start
    const uint32_t lo = (uint32_t)((uint64_t)A.n * cs / WALK_SHARDS);
    const uint32_t hi = (uint32_t)((uint64_t)A.n * (cs + 1) / WALK_SHARDS);
    const uint64_t r = (uint64_t)(blockIdx.x / WALK_SHARDS) * (WG / 64) + (threadIdx.x >> 6);
    const uint64_t b = r * A.tblk;
    if (b < hi - lo) {
      q_next = lo + (uint32_t)b;
      q_end = (uint32_t)std::min<uint64_t>(lo + b + A.tblk, hi);
    }
  }
  bool done = false;
  // the wave's first chunk of staged pairs is its own (no atomic at its first flush: every wave
  // reaches that flush within the first iterations, and one hot counter serialises)
  const uint32_t wv = L.gl >> 6;
  WaveOut o{wv < A.stat_chunks ? wv * CH : 0u, wv < A.stat_chunks ? (wv + 1) * CH : 0u};
  uint32_t c_states = 0, c_loads = 0, c_liters = 0, c_witers = 0;
  unsigned long long* wt = CENSUS ? A.census + CENSUS_HDR + 3 * (L.gl >> 6) : nullptr;
  __shared__ uint32_t s_dep[2 * CENSUS_DEPTHS];  // census: bucket loads per level and kind
  if (CENSUS) {
    for (uint32_t i = threadIdx.x; i < 2 * CENSUS_DEPTHS; i += WG) s_dep[i] = 0;
    __syncthreads();
  }
  if (CENSUS && lane_id() == 0) wt[0] = wall_clock64();
  bool was_done = false;

  for (;;) {
    L.ne = 0;
    L.np = 0;
    // ---- activate: an idle lane takes its prefetched topic and creates the root state ----
    if (t == NONE && nxt != NONE) {
      t = nxt;
      nxt = NONE;
      wb = nr3.z;  // (0 without the last part: no item of a level >= REC_TOKS then)
      L.n = nr3.w & 0xFFFFFFu;
      L.fl = nr3.w >> 24;
      rank = 0;
      L.sp = 0;
      if (L.fl & T_WILD) {  // emqx_trie.erl:157-166: wildcard topic name -> []
        A.cnt[t] = 0;
        t = NONE;
      } else {
        uint64_t tk[REC_TOKS];
        if constexpr (REC == REC_REVEN)  // tok0 / tok2 from their header bits: c_k or 0
          rec_tokens_even(nr0, nr1, nr3.w, A.c0, A.c2, tk);
        else
          rec_tokens(nr0, nr1, nr2, nr3, tk);
        L.cls = 0;
#pragma unroll
        for (uint32_t k = 0; k < REC_TOKS; ++k) {
          s_tw[k][L.tcol] = tk[k];
          if constexpr (!PAIR) L.cls |= sig_class(tk[k]) << (3u * k);  // (create's LENT)
        }
        const bool dollar = (L.fl & T_DOLLAR) != 0;
        // the root: no root '#' and no root '+' for a '$' topic (emqx_trie.erl:282-289); a
        // pair's root state is its leading lane's (the partner takes items from it)
        if (lead)
          create<SPILL, STK, CPT, true, !PAIR, RP>(L, s_stk, s_em, s_tw, A, A.root_cf, dollar ? NONE : A.root_hf, NONE,
                        A.root_sig, A.root_pcf,
                        A.root_phf, 0, !dollar, false, c_states,
                        (A.rh0.z & CF_ID_MASK) == FAT_ID, A.rh0, A.rh1);
      }
    }
    // ---- prefetch: lanes without a next topic claim one from the wave's block ----
    if (A.static_one && !done) {
      if ((PAIR ? L.gl >> 1 : L.gl) < A.n) {
        nxt = PAIR ? L.gl >> 1 : L.gl;
        load_rec<REC>(A, nxt, nr0, nr1, nr2, nr3);
      }
      done = true;
    }
    // (a pair: its leading lane claims, the partner follows below)
    uint64_t mi = __ballot(lead && nxt == NONE);
    while (mi != 0 && !done) {
      const uint32_t avail = q_end - q_next;
      if (avail == 0) {
        // shard cs holds topics [lo, hi)
        const uint32_t lo = (uint32_t)((uint64_t)A.n * cs / WALK_SHARDS);
        const uint32_t hi = (uint32_t)((uint64_t)A.n * (cs + 1) / WALK_SHARDS);
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(&A.ctl[CTL_CLAIM0 + CTL_CLAIM_STRIDE * cs], A.tblk);
        base = __builtin_amdgcn_readfirstlane(base);  // every lane is active here
        if (base >= hi - lo) {
          // shard cs is out.  The one claim that ran it out (base in [size, size + tblk)) posts
          // that in CTL_SHARDS_OUT; a wave then moves on to a shard nobody has seen run out, by
          // one load instead of one atomic per exhausted shard (at the end of a pass every
          // wave otherwise queued on all 8 counters).  Done once every shard is seen out, by
          // the posted bits or by this wave's own failed claims (a bit is only ever set after
          // a failed claim, so no topic is left unclaimed).
          out_seen |= 1u << cs;
          uint32_t posted = 0;
          if (lane_id() == 0) {
            if (base < hi - lo + A.tblk) atomicOr(&A.ctl[CTL_SHARDS_OUT], 1u << cs);
            posted = __hip_atomic_load(&A.ctl[CTL_SHARDS_OUT], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
          }
          const uint32_t m = (__builtin_amdgcn_readfirstlane(posted) | out_seen) & ((1u << WALK_SHARDS) - 1);
          if (m == (1u << WALK_SHARDS) - 1) {
            done = true;
            break;
          }
          do cs = (cs + 1) % WALK_SHARDS; while ((m >> cs) & 1u);
          continue;
        }
        q_next = lo + base;
        q_end = min(lo + base + A.tblk, hi);
        continue;
      }
      const uint32_t r = mbcnt64(mi);
      if (lead && nxt == NONE && r < avail) {
        nxt = q_next + r;
        load_rec<REC>(A, nxt, nr0, nr1, nr2, nr3);  // consumed when this lane next idles
      }
      q_next += min((uint32_t)__popcll(mi), avail);
      mi = __ballot(lead && nxt == NONE);
    }
    if constexpr (PAIR) {
      if (!A.static_one) {  // the partner takes its leading lane's claim (same record)
        const uint32_t ln = pair_xchg(nxt);
        if (!lead && nxt == NONE && ln != NONE) {
          nxt = ln;
          load_rec<REC>(A, nxt, nr0, nr1, nr2, nr3);
        }
      }
    }
    if (CENSUS && done && !was_done) {
      was_done = true;
      if (lane_id() == 0) wt[1] = wall_clock64();
    }
    const bool active = (t != NONE);
    // wave-uniform exit (readfirstlane tells the compiler so: a divergent-looking break lets
    // paths skip the register "uses" below and costs vmcnt drains at the loop head)
    if (__ballot(active || nxt != NONE) == 0 && __builtin_amdgcn_readfirstlane(done ? 1u : 0u)) break;

    // ---- fill idle probe slots from the item stack (a pair: then from the partner's) ----
    uint32_t own_pos = L.sp, st_pos = 0, own_left = L.sp, st_left = 0;
    if constexpr (PAIR) {
      uint32_t fr = 0;
#pragma unroll
      for (uint32_t j = 0; j < NS; ++j) fr += (active && !P[j].busy) ? 1u : 0u;
      const uint32_t own = min(fr, L.sp);
      const uint32_t psp = pair_xchg(L.sp), pfr = pair_xchg(fr);
      const uint32_t pown = min(pfr, psp);
      own_left = own;
      st_left = min(fr - own, psp - pown);  // taken from the top of the partner's stack
      st_pos = psp - pown;
      L.sp -= own + min(pfr - pown, L.sp - own);  // (and what the partner takes from mine)
      __builtin_amdgcn_wave_barrier();  // the partner's pushes of the last iteration are in LDS
    }
    // SHARE: the level of slot 0's keyed probe when it is filled here, at its home (else NONE),
    // and the stack position from which the items are matched against its line after the resolves
    uint32_t shk = NONE, sh_lo = 0;
#pragma unroll
    for (uint32_t j = 0; j < NS; ++j) {
      Probe& p = P[j];
      if constexpr (SHARE) {
        // a keyed sibling of slot 0's probe stays on the stack (and so does everything below it)
        if (j > 0 && active && !p.busy && own_left > 0 && shk != NONE) {
          const uint32_t v = s_stk[own_pos - 1][L.tid];
          if ((v & IT_KIND) == IT_KEYED && ((v >> CPT_SHIFT) & 0xFu) == shk) own_left = 0;
        }
      }
      if (active && !p.busy && (own_left > 0 || st_left > 0)) {
        uint32_t pos, col = L.tid;
        if (own_left > 0) {
          pos = --own_pos;
          --own_left;
        } else {
          pos = --st_pos;
          --st_left;
          col = L.tid ^ 1u;
        }
        if constexpr (!PAIR) L.sp = pos;
        uint2 it;
        if constexpr (CPT) {
          const uint32_t v = s_stk[pos][col];
          it = make_uint2(v & ~(0xFu << CPT_SHIFT), (v >> CPT_SHIFT) & 0xFu);
          if constexpr (SHARE)
            if (j == 0) shk = (A.keyed_share && (v & IT_KIND) == IT_KEYED && it.y < REC_TOKS) ? it.y : NONE;
        } else if (!SPILL || L.sp < STK) {
          it = s_stk[L.sp][L.tid];
        } else {
          const uint64_t v = __builtin_nontemporal_load(
              (const uint64_t*)(A.spill + (uint64_t)(L.sp - STK) * A.lanes + L.gl));
          it = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        }
        p.busy = true;
        p.cur = it.x;
        p.k = it.y;
        p.side = false;
        const uint32_t kind = it.x & IT_KIND;
        if (kind == IT_PLUS) {
          p.key = PLUS_TOK;
        } else if (kind == IT_TN) {
          p.side = true;  // loads the node's tn list word
        } else if (it.y < REC_TOKS) {
          p.key = s_tw[it.y][L.tcol];
        } else {
          p.side = true;  // deep level: fetch its token this iteration, probe the next
        }
        if (!p.side) p.ia = edge_home(it.x & CF_ID_MASK, p.key, A.emask, kind == IT_KEYED);
      }
    }
    if constexpr (SHARE) sh_lo = (shk != NONE && L.sp > 0) ? L.sp - 1 : L.sp;
    // ---- one memory round trip: every slot issues its load, branch-free (an idle slot loads
    // slot 0, an always-cached line, and ignores it): with the loads of all slots in one basic
    // block the compiler keeps them in flight together instead of draining vmcnt between ----
#pragma unroll
    for (uint32_t j = 0; j < NS; ++j) {
      Probe& p = P[j];
      const bool ld = p.busy && !p.side;
      const uint4* q = A.edges + SLOT_U4 * EBUCKET * (ld ? p.ia : 0ull);
      p.s0 = q[0];
      p.s1 = q[1];
      p.t0 = q[2];
      p.t1 = q[3];
      if (CENSUS && ld) {
        c_loads += 1u;
        atomicAdd(&s_dep[min(p.k, CENSUS_DEPTHS - 1) + ((p.cur & IT_KIND) == IT_PLUS ? CENSUS_DEPTHS : 0u)], 1u);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < NS; ++j) {
      Probe& p = P[j];
      if (p.busy && p.side) {  // rare: levels >= REC_TOKS, tn lists
        if ((p.cur & IT_KIND) == IT_TN)
          p.skey = A.tn_of[p.cur & CF_ID_MASK];
        else
          p.skey = A.wh[wb + p.k];
      }
    }
    if (CENSUS) {
      c_liters += active ? 1u : 0u;
      c_witers += 1u;
    }

    // ---- emission: the ids listed in s_em since the last flush, by one wave scan (into the
    // wave's chunk of staged pairs, ranks in list order), multi[] lists after ----
    auto flush = [&]() {
      const uint32_t ne = min(L.ne, EMX);
      const uint32_t plain = L.np;  // counted as listed (r04: a read-back loop cost an LDS
                                    // round trip per entry, for no measurable walk time)
      const bool any_multi = __ballot(plain != ne) != 0;
      // a pair's ids: the leading lane's first, then the partner's
      const uint32_t pp = PAIR ? pair_xchg(plain) : 0u;
      const uint32_t rk = rank + (lead ? 0u : pp);
      // at most one id per lane: the scan is a ballot and a bit count (no shuffle chain)
      const bool single = __ballot(plain > 1) == 0;
      uint32_t tot = 0, ex = 0;
      if (single) {
        const uint64_t m = __ballot(plain != 0);
        ex = mbcnt64(m);
        tot = (uint32_t)__popcll(m);
      } else if (!any_multi) {
        // (the rounds below need only the total: ballots, no scan)
        for (uint32_t q = 0; q < EMX; ++q) {
          const uint64_t m = __ballot(plain > q);
          if (m == 0) break;
          tot += (uint32_t)__popcll(m);
        }
      } else {
        ex = wave_excl_scan(plain, tot);
      }
      if (tot) {
        reserve(tot, o, A);
        if (!any_multi && single) {
          // at most one id per lane (the common case when matches are few per topic): each lane
          // stores its own at its place in the scan, no owner search
          if (plain) put<PAIR>(o.pos + ex, t, s_em[0][L.tid], rk, A);
        } else if (!any_multi) {
          // In rounds: in round q every lane with more than q ids stores its q-th, the round's
          // pairs side by side (whole lines per store).  A pair carries its rank, so the order of
          // a chunk's slots is free.  (Until r06 the slots were filled by position, each lane
          // finding a slot's owner by a 5-step binary search of shuffles: a chain of dependent
          // LDS-crossbar round trips in every such flush, the latency a small batch's walk pays.)
          uint32_t pos = o.pos;
          for (uint32_t q = 0; q < EMX; ++q) {  // (wave-uniform exit)
            const uint64_t m = __ballot(plain > q);
            if (m == 0) break;
            if (plain > q) put<PAIR>(pos + mbcnt64(m), t, s_em[q][L.tid], rk + q, A);
            pos += (uint32_t)__popcll(m);
          }
        } else {
          const uint32_t base = o.pos + ex;
          uint32_t q = 0;
          for (uint32_t j = 0; j < ne; ++j) {
            const uint32_t v = s_em[j][L.tid];
            if (!(v & EM_MULTI)) {
              put<PAIR>(base + q, t, v, rk + q, A);
              ++q;
            }
          }
        }
        rank += plain + pp;
        o.pos += tot;
      }
      if (any_multi) {  // rare: ids shared by several filters (a pair: one lane after the other)
#pragma unroll
        for (uint32_t pass = 0; pass < (PAIR ? 2u : 1u); ++pass) {
          const bool mine = !PAIR || ((pass == 0) == lead);
          for (uint32_t j = 0; __ballot(j < ne) != 0; ++j) {
            const uint32_t v = (j < ne) ? s_em[j][L.tid] : 0u;
            const bool m = mine && (j < ne) && (v & EM_MULTI);
            emit_multi<PAIR>(m, v & ~EM_MULTI, t, rank, o, A);
          }
          if constexpr (PAIR) {
            const uint32_t pr = pair_xchg(rank);
            if (!mine) rank = pr;
          }
        }
      }
      if (L.ne > EMX) L.overflow = true;
      L.ne = 0;
      L.np = 0;
    };

    // ---- resolve: hit -> create the child state(s); empty slot -> no child; else next slot ----
    // One flush per iteration: a lane lists at most 8 ids per iteration -- its new topic's root
    // state ('#' filter, carried '+' child's '#' filter) and, per slot, a resolved child
    // ('#' filter, terminal filters, carried '+' child's '#' filter) or one tn list.
    // A state that brings its fat half lists up to 2 + 3 ids (its own '#' filter and carried
    // '+' child's, then the half's three), the new topic's root with the root's half as many --
    // and, when the half's '+' child's only child comes from the arguments (create RP: topics of
    // 3 and more levels, so the half lists no terminal filters), 2 + 2 + 3 from an empty list:
    // before a slot is resolved the wave flushes if some lane could pass EMX.
    static_assert(EMX >= 5 + 3, "a flush must hold a slot's emissions after a partial list");
#pragma unroll
    for (uint32_t j = 0; j < NS; ++j) {
      Probe& p = P[j];
      if (__ballot(L.ne + 5u > EMX) != 0) flush();
      if (!p.busy) continue;
      if (p.side) {
        p.side = false;
        if ((p.cur & IT_KIND) == IT_TN) {  // the keys of a single-level '$' topic's node (:287)
          p.busy = false;
          if ((uint32_t)p.skey != NONE) em_list(L, s_em, (uint32_t)p.skey);
        } else {
          p.key = p.skey;
          p.ia = edge_home(p.cur & CF_ID_MASK, p.key, A.emask, (p.cur & IT_KIND) == IT_KEYED);
        }
        continue;
      }
      const uint32_t node = p.cur & CF_ID_MASK;
      // s0 = {tok.lo, tok.hi, parent, cf}: the key is (parent, token), exactly.  Fields are
      // copied to scalars before any select: a select between two fields of P[] makes the
      // compiler keep the whole array in scratch memory.
      const uint4 a0 = p.s0, a1 = p.s1, b0 = p.t0, b1 = p.t1;
      const uint32_t klo = (uint32_t)p.key, khi = (uint32_t)(p.key >> 32);
      const bool ha = (a0.z & CF_ID_MASK) == node && a0.x == klo && a0.y == khi;
      const bool hb = (b0.z & CF_ID_MASK) == node && b0.x == klo && b0.y == khi;
      if (ha || hb) {
        p.busy = false;
        const uint32_t ccf = ha ? a0.w : b0.w, chf = ha ? a1.x : b1.x;
        const uint32_t ctw = ha ? a1.y : b1.y, cpcf = ha ? a1.z : b1.z;
        const uint32_t cphf = ha ? a1.w : b1.w;
        const uint32_t csig = (ha ? a0.z : b0.z) >> SIG_SHIFT;
        // a fat node sits in the first half of its bucket, its only literal child in the second
        const bool fat = ha && (b0.z & CF_ID_MASK) == FAT_ID;
        create<SPILL, STK, CPT, true, !PAIR>(L, s_stk, s_em, s_tw, A, ccf, chf, ctw, csig, cpcf, cphf, p.k + 1,
                                 true, (p.cur & IT_KIND) != IT_PLUS, c_states, fat, b0, b1);
      } else if (a0.z == NONE || b0.z == NONE ||
                 (CLOSED && (slot_closed(a0.w, a1.w, A.closed_off) || slot_closed(b0.w, b1.w, A.closed_off)))) {
        // (a closed bucket, gm_common.h EDGE_CLOSED: nothing on this chain was placed past it)
        p.busy = false;
      } else {
        p.ia = (p.ia + 1) & A.emask;
      }
    }

    // ---- SHARE: the keyed items of slot 0's level against slot 0's line ----
    if constexpr (SHARE) {
      // (one item per lane: the first found; a create lists up to 5 ids, so the flush check
      // comes first.  A second sibling, rare, is probed the ordinary way.)
      uint32_t node = NONE, fi = 0;
      if (shk != NONE) {
        for (uint32_t i = sh_lo; i < L.sp; ++i) {
          const uint32_t v = s_stk[i][L.tid];
          if ((v & IT_KIND) == IT_KEYED && ((v >> CPT_SHIFT) & 0xFu) == shk) {
            node = v & CF_ID_MASK;
            fi = i;
            break;
          }
        }
      }
      if (__ballot(node != NONE) != 0) {
        if (__ballot(L.ne + 5u > EMX) != 0) flush();
        if (node != NONE) {
          const uint4 a0 = P[0].s0, a1 = P[0].s1, b0 = P[0].t0, b1 = P[0].t1;
          const uint32_t klo = (uint32_t)P[0].key, khi = (uint32_t)(P[0].key >> 32);
          const bool ha = (a0.z & CF_ID_MASK) == node && a0.x == klo && a0.y == khi;
          const bool hb = (b0.z & CF_ID_MASK) == node && b0.x == klo && b0.y == khi;
          if (ha || hb || a0.z == NONE || b0.z == NONE ||
              (CLOSED && (slot_closed(a0.w, a1.w, A.closed_off) || slot_closed(b0.w, b1.w, A.closed_off)))) {
            // decided by this line (a closed bucket of other keys: the sibling is absent as
            // well): the item leaves the stack (the top one takes its place)
            --L.sp;
            s_stk[fi][L.tid] = s_stk[L.sp][L.tid];
          }
          // (else a full bucket of other keys with an edge placed past it: the item stays, for
          // a probe of its own)
          if (ha || hb) {
            const uint32_t ccf = ha ? a0.w : b0.w, chf = ha ? a1.x : b1.x;
            const uint32_t ctw = ha ? a1.y : b1.y, cpcf = ha ? a1.z : b1.z;
            const uint32_t cphf = ha ? a1.w : b1.w;
            const uint32_t csig = (ha ? a0.z : b0.z) >> SIG_SHIFT;
            const bool fat = ha && (b0.z & CF_ID_MASK) == FAT_ID;
            create<SPILL, STK, CPT, true, !PAIR>(L, s_stk, s_em, s_tw, A, ccf, chf, ctw, csig, cpcf, cphf,
                                                 shk + 1, true, true, c_states, fat, b0, b1);
          }
        }
      }
    }

    // The prefetched record and every slot's data (an idle slot's dummy load included) are
    // complete by now; saying so keeps the compiler from draining vmcnt (stores included)
    // wherever it later reuses those registers.
    if constexpr (REC == REC_REVEN)  // (nr2 and the rest of nr3 are never loaded: constants)
      asm volatile("" ::"v"(nr0.x), "v"(nr0.y), "v"(nr0.z), "v"(nr0.w), "v"(nr1.x), "v"(nr1.y),
                   "v"(nr1.z), "v"(nr1.w), "v"(nr3.w));
    else
      asm volatile("" ::"v"(nr0.x), "v"(nr0.y), "v"(nr0.z), "v"(nr0.w), "v"(nr1.x), "v"(nr1.y),
                   "v"(nr1.z), "v"(nr1.w), "v"(nr2.x), "v"(nr2.y), "v"(nr2.z), "v"(nr2.w),
                   "v"(nr3.x), "v"(nr3.y), "v"(nr3.z), "v"(nr3.w));
#pragma unroll
    for (uint32_t j = 0; j < NS; ++j)
      asm volatile("" ::"v"(P[j].s0.x), "v"(P[j].s1.x), "v"(P[j].s0.w), "v"(P[j].s1.w),
                   "v"(P[j].s0.y), "v"(P[j].s1.y), "v"(P[j].s0.z), "v"(P[j].s1.z),
                   "v"(P[j].t0.x), "v"(P[j].t1.x), "v"(P[j].t0.w), "v"(P[j].t1.w),
                   "v"(P[j].t0.y), "v"(P[j].t1.y), "v"(P[j].t0.z), "v"(P[j].t1.z));

    flush();

    // ---- topic done when no probe is in flight and no item is pending ----
    bool idle = (L.sp == 0);
#pragma unroll
    for (uint32_t j = 0; j < NS; ++j) idle = idle && !P[j].busy;
    if constexpr (PAIR) idle = idle && pair_xchg(idle ? 1u : 0u) != 0u;
    if (active && idle) {
      if (lead) A.cnt[t] = rank;
      if (lead && (PAIR || A.fmt.pk) && rank > A.fmt.rmask + 1u) A.ctl[CTL_PKOVF] = 1u;
      t = NONE;
    }
  }
  close_chunk(o, A);
  if (__ballot(L.overflow) != 0 && lane_id() == 0) atomicOr(&A.ctl[CTL_ERR], 1u);
  if (CENSUS) {
    atomicAdd(&A.census[0], (unsigned long long)c_states);
    atomicAdd(&A.census[1], (unsigned long long)c_loads);
    atomicAdd(&A.census[2], (unsigned long long)c_liters);
    if (lane_id() == 0) atomicAdd(&A.census[3], (unsigned long long)c_witers);
    if (lane_id() == 0) wt[2] = wall_clock64();
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * CENSUS_DEPTHS; i += WG)
      if (s_dep[i]) atomicAdd(&A.census[CENSUS_N + i], (unsigned long long)s_dep[i]);
  }
}
