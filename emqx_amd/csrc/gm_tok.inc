// gm_tok.inc -- the tokenizer kernel and the exact route-key probe (included by gm_kernels.hip).
//
// emqx_topic:tokens/1 + words/1 (apps/emqx/src/emqx_topic.erl:155-169): every '/' splits, no
// trimming, "" -> [''].  One 256-thread workgroup takes a tile of 256 topics:
//   1. their packed bytes are staged in LDS with coalesced 16-B loads;
//   2. each lane computes its level tokens (gm_common.h word_token), the wildcard flag
//      (emqx_topic:wildcard/1, :54-64), the '$' flag (emqx_trie.erl:282) and the whole-topic
//      hash, and writes its topic record: header + the first REC_TOKS tokens, which is
//      all the walk reads for topics of up to 7 levels -- of its 64 B only the parts the
//      committed index can read (gm_common.h rec_parts).  A deeper topic writes its levels
//      >= REC_TOKS to the token array at off[t] + t (no counters: a topic has <= len + 1 levels).
// The kernel issues no atomics: a single hot counter serialises at ~88 updates/us chip-wide.
//   3. the exact route-key probe: when the committed index has plain (non-wildcard) route keys,
//      every name probes them in k_exact (below), a kernel of its own with few registers and
//      many waves, so the tokenizer keeps its occupancy; k_tok then only marks wildcard names
//      (X_WILDPEND).  Without plain keys the rare wildcard name probes the wildcard-key region
//      right here.
// Tiles whose bytes do not fit in LDS (very long topics) read global memory; same results.

// Stages the packed bytes [B0, B1) into s_buf; returns false when the tile does not fit (the
// caller then reads global memory).  `sh` = offset of B0 in s_buf.  `cp` (copy-through, see
// TokArgs): the staged chunks are also stored there, at the same offsets.
template <bool CP = false>
__device__ __forceinline__ bool stage_tile(const uint8_t* bytes, uint32_t B0, uint32_t B1,
                                           uint4* s_buf, uint32_t& sh, uint8_t* cp = nullptr) {
  const uintptr_t p0 = (uintptr_t)(bytes + B0);
  sh = (uint32_t)(p0 & 15u);
  const uint32_t nch = (sh + (B1 - B0) + 15u) >> 4;
  if (nch + 1 > TILE_CHUNKS) return false;  // one chunk of slack: load8 reads past the end
  const uint4* q = (const uint4*)(bytes + B0 - sh);  // keep the global address space
  // all of a lane's chunk loads in flight at once, then the LDS writes; both unconditional
  // (past the tile a lane re-reads chunk 0 and writes the spare last chunk, which holds no
  // tile bytes) so that the compiler cannot sink each load next to its write
  constexpr uint32_t PER = (TILE_CHUNKS + WG - 1) / WG;
  uint4 v[PER];
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    const uint32_t c = threadIdx.x + j * WG;
    v[j] = q[c < nch ? c : 0u];
  }
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    const uint32_t c = threadIdx.x + j * WG;
    s_buf[c < nch ? c : TILE_CHUNKS - 1] = v[j];
  }
  if (CP) {
    uint4* w = (uint4*)(cp + B0 - sh);  // 16-B aligned like `bytes` (the engine checks)
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {
      const uint32_t c = threadIdx.x + j * WG;
      if (c < nch) w[c] = v[j];
    }
  }
  return true;
}

// Byte accessor over global memory.
struct GlobBytes {
  const uint8_t* p;
  __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return p[i]; }
};

struct TokArgs {
  const uint8_t* bytes;
  const uint32_t* off;
  uint32_t n;
  uint32_t* nw;
  uint64_t* wh;
  uint4* rec;           // records in blocks of 64 topics, part-major (gm_common.h rec_at)
  uint32_t* exact_id;
  uint32_t* ctl;
  uint64_t test_mask;
  uint32_t pair_top0;  // CTL_PAIR_TOP at the walk's start: the walk's static chunks (or 0)
  uint32_t* rej;       // per-topic reject counts to zero (verifying passes), or null
  uint32_t claim0[WALK_SHARDS];  // walk claim counters' start values (static first claims)
  bool wild_empty;  // no committed wildcard route key
  // copy-through (small host windows): bytes / off point into pinned host memory, read over
  // PCIe once here, and the kernel stores what it read into the pass's device copies cp_bytes /
  // cp_off (the later kernels' inputs) -- no DMA copy, and no copy-to-kernel dependency, in
  // front of the pass; null otherwise
  uint8_t* cp_bytes;
  uint32_t* cp_off;
  uint32_t* ctl_host;  // the host mirror of ctl: its CTL_LEGACY is zeroed here (k_scatter<true>
                       // mirrors every other word; scatter blocks set this one), or null
  bool nt_rec;  // records stored non-temporally (batches of at least TOK_NT_MIN topics)
  uint32_t* hdr;  // null: all REC_U4 record parts are stored (gm_common.h rec_parts); else
                  // REC_PARTS_MIN, and the header word n_words | flags << 24 of topic t at hdr[t]
  // the even-elided form (gm_common.h; k_tok's EVEN instantiations, hdr set): parts {tok1, tok3}
  // {tok4, tok5}, and T_EQ0 / T_EQ2 in the header word for a word 0 / 2 whose token is c0 / c2
  // (0: the level has no token).  The other instantiations never read them.
  uint64_t c0, c2;
};

// Batches from which k_tok stores its records non-temporally: 128 MB of records and up do not
// stay in the caches until the walk reads them (the other pass's kernels run in between), and
// plain stores evict the walk's edge lines (r05, cfg3 4M topics, 3 alternating runs each:
// walk 0.330 -> 0.324 ms, 9.49 -> 9.59 G topics/s; 1M topics: even, so smaller batches and the
// NIF's windows keep plain stores; profiles/r05/ab_ntst/).  The walk's loads stay plain (r05:
// non-temporal loads too were slower, profiles/r05/ab_nt/).
constexpr uint32_t TOK_NT_MIN = 2u << 20;

// Exact route-key probe: emqx_router:lookup_routes(Topic) (emqx_router.erl:155-157) is an
// ets:lookup on the route bag, keyed by the filter string -- wildcard strings included (:143).
// A name equal to a key has the key's words, so it is a wildcard string iff the key is one:
// plain names probe only the region of plain keys, wildcard names only the region of wildcard
// keys (an IoT tree whose routes are all wildcard filters needs no probe for its publishes).
// Buckets are one 64-B line of two 32-B entries carrying the key's first XINL bytes
// (gm_common.h "Exact route-key table"): a key of up to XINL bytes is found or ruled out by the
// line(s) of its bucket chain alone; a longer one is confirmed against the string pool.

// A topic's bytes as little-endian dwords read straight from global memory: word(k) holds bytes
// 4k .. 4k+3 of the topic (bytes past its end are garbage, callers mask them).  Only dwords that
// hold bytes of the topic are read.
struct TopicWords {
  const uint32_t* w;  // dword-aligned base
  uint32_t b;         // byte offset of the topic from w
  uint32_t last;      // index of the dword holding the topic's last byte
  __device__ __forceinline__ TopicWords(const uint8_t* bytes, uint32_t ob, uint32_t len) {
    const uintptr_t p = (uintptr_t)bytes;
    w = (const uint32_t*)(p & ~(uintptr_t)3);
    b = ob + (uint32_t)(p & 3u);
    last = len ? (b + len - 1) >> 2 : b >> 2;
  }
  __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
    const uint32_t x = b + 4 * k, i = x >> 2;
    return __builtin_amdgcn_alignbyte(w[min(i + 1, last)], w[min(i, last)], x & 3u);
  }
};

struct ExactArgs {
  const uint4* exact;  // XBUCKET x XENT_U4 uint4 per bucket
  const uint32_t* xovf;  // overflow bit per bucket
  uint64_t xmask;      // plain-key region: bucket count - 1 (region starts at bucket 0)
  uint64_t xwbase;     // wildcard-key region: first bucket
  uint64_t xwmask;     // wildcard-key region: bucket count - 1
  const uint8_t* fbytes;
  const uint64_t* foff;
  uint64_t full_mask;
  uint32_t xseq;  // CTL_XHIT is set to this pass's sequence number (the word is never cleared)
};

__device__ __forceinline__ uint32_t len_mask(uint32_t len, uint32_t k) {
  const uint32_t nb = len > 4 * k ? len - 4 * k : 0u;
  return nb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nb)) - 1u);
}

// The probe of a hashed name: its chain from home bucket `bk` (in the region at `base`, `mask`),
// comparing h32 and the first XINL bytes (tw) inline; a longer key is confirmed against the
// string pool a dword at a time (T: the name's dwords).  r06: the confirmation compared byte by
// byte with an early exit, two dependent loads per byte -- every hit of a name longer than XINL
// was a chain of ~2 x (len - 20) round trips (cfg2's probe: 33 load instructions per wave).
template <class W>
__device__ __forceinline__ uint32_t exact_probe(const ExactArgs& A, const W& T, uint32_t len,
                                                uint64_t base, uint64_t mask, uint64_t bk,
                                                uint32_t h32, const uint32_t (&tw)[XINL / 4]) {
  for (;;) {
    const uint4* q = A.exact + XBUCKET * XENT_U4 * bk;
    const uint4 e[XBUCKET * XENT_U4] = {q[0], q[1], q[2], q[3]};
    const uint32_t ovf = A.xovf[bk >> 5];  // issued with the bucket line
#pragma unroll
    for (uint32_t j = 0; j < XBUCKET; ++j) {
      const uint4 e0 = e[XENT_U4 * j], e1 = e[XENT_U4 * j + 1];
      if (e0.y == NONE) return NONE;  // an empty entry ends the chain
      if (e0.y != TOMB && e0.x == h32 && e0.z == len && e0.w == tw[0] && e1.x == tw[1] &&
          e1.y == tw[2] && e1.z == tw[3] && e1.w == tw[4]) {
        uint32_t diff = 0;
        if (len > XINL) {  // a long key: the rest of its bytes from the string pool
          const TopicWords F(A.fbytes + A.foff[e0.y], 0u, len);
          for (uint32_t k = XINL / 4; 4 * k < len; ++k) diff |= (T(k) ^ F(k)) & len_mask(len, k);
        }
        if (diff == 0) return e0.y;
      }
    }
    if (!((ovf >> (bk & 31)) & 1u)) return NONE;  // nothing placed past this bucket
    bk = base + ((bk - base + 1) & mask);
  }
}

// The same dwords of a topic staged in LDS (k_exact's tiles): `b` = the topic's byte offset in
// the tile buffer.
struct LdsTopicWords {
  const uint32_t* w;
  uint32_t b, last;
  __device__ __forceinline__ LdsTopicWords(const uint32_t* s32, uint32_t b_, uint32_t len)
      : w(s32), b(b_), last(len ? (b_ + len - 1) >> 2 : b_ >> 2) {}
  __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
    const uint32_t x = b + 4 * k, i = x >> 2;
    return __builtin_amdgcn_alignbyte(w[min(i + 1, last)], w[min(i, last)], x & 3u);
  }
};

// Route key equal to the topic bytes [ob, ob + len) of `bytes` (wild: probe the wildcard-key
// region), or NONE.  T reads the topic's dwords (from global memory, or from an LDS tile).
template <class W = TopicWords>
__device__ __forceinline__ uint32_t exact_lookup(const ExactArgs& A, const uint8_t* bytes,
                                                 uint32_t ob, uint32_t len, bool wild,
                                                 const W& T) {
  uint32_t a, c, tw[XINL / 4];
  key_hash_init(len, a, c);
#pragma unroll
  for (uint32_t k = 0; k < XINL / 4; ++k) {
    tw[k] = 4 * k < len ? (T(k) & len_mask(len, k)) : 0u;
    if (4 * k < len) key_hash_word(tw[k], a, c);
  }
  for (uint32_t k = XINL / 4; 4 * k < len; ++k) key_hash_word(T(k) & len_mask(len, k), a, c);
  const uint64_t fh = key_hash_final(a, c, A.full_mask);
  const uint64_t base = wild ? A.xwbase : 0ull, mask = wild ? A.xwmask : A.xmask;
  return exact_probe(A, T, len, base, mask, base + exact_slot(fh, mask), (uint32_t)(fh >> 32), tw);
}
__device__ __forceinline__ uint32_t exact_lookup(const ExactArgs& A, const uint8_t* bytes,
                                                 uint32_t ob, uint32_t len, bool wild) {
  return exact_lookup(A, bytes, ob, len, wild, TopicWords(bytes, ob, len));
}
static_assert(XINL == 20 && XBUCKET * XENT_U4 == 4, "exact_lookup reads one 4 x 16-B bucket");
// The tokenizer's rare wildcard-name probe: the same lookup written for few live registers
// (byte loop, one 16-B entry word at a time), so it does not cost the tokenizer occupancy.
__device__ __forceinline__ uint32_t exact_lookup_wild(const ExactArgs& A, const uint8_t* bytes,
                                                      uint32_t ob, uint32_t len) {
  const uint8_t* p = bytes + ob;
  const uint64_t fh = key_hash(p, len, A.full_mask);
  const uint32_t h32 = (uint32_t)(fh >> 32);
  uint64_t bk = A.xwbase + exact_slot(fh, A.xwmask);
  for (;;) {
    const uint4* q = A.exact + XBUCKET * XENT_U4 * bk;
    for (uint32_t j = 0; j < XBUCKET; ++j) {
      const uint4 e0 = q[XENT_U4 * j];
      if (e0.y == NONE) return NONE;
      if (e0.y == TOMB || e0.x != h32 || e0.z != len) continue;
      const uint8_t* fp = A.fbytes + A.foff[e0.y];
      bool eq = true;
      for (uint32_t i = 0; i < len && eq; ++i) eq = p[i] == fp[i];
      if (eq) return e0.y;
    }
    if (!((A.xovf[bk >> 5] >> (bk & 31)) & 1u)) return NONE;
    bk = A.xwbase + ((bk - A.xwbase + 1) & A.xwmask);
  }
}

// Tokens of one topic.  Writes token k to dst(k); returns the topic hash state and flags.
template <class P, class D>
__device__ __forceinline__ uint32_t tok_words(P p, uint32_t len, uint64_t test_mask, D dst,
                                              uint32_t& flags) {
  uint64_t packed = 0;
  uint32_t k = 0, wlen = 0, ws = 0;
  flags = (len > 0 && p[0] == '$') ? T_DOLLAR : 0u;
  for (uint32_t i = 0; i <= len; ++i) {  // i == len is the final separator
    const uint32_t c = (i < len) ? p[i] : (uint32_t)'/';
    if (c == '/') {
      if (wlen == 1 && (packed == '+' || packed == '#')) flags |= T_WILD;
      uint64_t fnv = FNV_OFF;
      if (wlen > TOK_INLINE_MAX || test_mask)  // hashed token: long word (or test mode)
        for (uint32_t q = ws; q < i; ++q) fnv = fnv_step(fnv, p[q]);
      const uint64_t tok = word_token(packed, fnv, wlen, test_mask);
      dst(k, tok);
      ++k;
      packed = 0;
      wlen = 0;
      ws = i + 1;
    } else {
      if (wlen < 8) packed |= (uint64_t)c << (8 * wlen);
      ++wlen;
    }
  }
  return k;  // levels
}

// First '/' at or after byte x (< e) of an LDS tile, or e.  One aligned dword per step.
__device__ __forceinline__ uint32_t next_slash(const uint32_t* w, uint32_t x, uint32_t e) {
  while (x < e) {
    const uint32_t wi = x >> 2;
    const uint32_t y = w[wi] ^ 0x2F2F2F2Fu;
    uint32_t z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);  // 0x80 per '/'
    z &= 0xFFFFFFFFu << (8 * (x & 3u));
    if (z) {
      const uint32_t p = (wi << 2) + ((uint32_t)__builtin_ctz(z) >> 3);
      return p < e ? p : e;
    }
    x = (wi + 1) << 2;
  }
  return e;
}

// The len (<= 8) bytes at byte x of an LDS tile, little-endian, higher bytes zero.
__device__ __forceinline__ uint64_t load8(const uint32_t* w, uint32_t x, uint32_t len) {
  const uint32_t wi = x >> 2, sh = x & 3u;
  const uint32_t a = w[wi], b = w[wi + 1], c = w[wi + 2];
  const uint32_t lo = __builtin_amdgcn_alignbyte(b, a, sh);
  const uint32_t hi = __builtin_amdgcn_alignbyte(c, b, sh);
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  return len >= 8 ? v : (v & ((1ull << (8 * len)) - 1ull));
}

// One word of an LDS tile starting at byte x: its token (gm_common.h word_token); `we` = the byte
// after it (its '/', or e).  Sets T_WILD for a word that is exactly '+' or '#'.
__device__ __forceinline__ uint64_t lds_word(const uint32_t* w, uint32_t x, uint32_t e,
                                             uint64_t test_mask, uint32_t& we, uint32_t& flags) {
  we = next_slash(w, x, e);
  const uint32_t wl = we - x;
  const uint64_t packed = load8(w, x, wl < 8 ? wl : 8u);
  if (wl == 1 && (packed == '+' || packed == '#')) flags |= T_WILD;
  uint64_t fnv = FNV_OFF;
  if (wl > TOK_INLINE_MAX || test_mask)  // hashed token: long word (or test mode)
    for (uint32_t q = x; q < we; ++q) fnv = fnv_step(fnv, (w[q >> 2] >> (8 * (q & 3u))) & 0xFFu);
  return word_token(packed, fnv, wl, test_mask);
}

// tok_words over an LDS tile, word by word instead of byte by byte: the per-word work (token,
// hash fold) runs once per word with the lanes of a wave in step, and a word's bytes are one
// funnel-shifted 8-byte read.  The first REC_TOKS tokens land in fixed registers (the word loop
// is unrolled over them: a dynamic index into the token array cost every word a shuffle of all
// seven); deeper tokens go to deep(k, token).  Same results as tok_words.
template <class D>
__device__ __forceinline__ uint32_t tok_words_rec(const uint32_t* w, uint32_t s, uint32_t len,
                                                  uint64_t test_mask, uint64_t (&tk)[REC_TOKS],
                                                  D deep, uint32_t& flags) {
  const uint32_t e = s + len;
  flags = (len > 0 && (w[s >> 2] >> (8 * (s & 3u)) & 0xFFu) == '$') ? T_DOLLAR : 0u;
  uint32_t x = s, n = 0;
  bool more = true;  // a topic has at least one word ("" -> [''])
#pragma unroll
  for (uint32_t k = 0; k < REC_TOKS; ++k) {
    if (more) {
      uint32_t we;
      tk[k] = lds_word(w, x, e, test_mask, we, flags);
      n = k + 1;
      more = we < e;
      x = we + 1;
    }
  }
  for (uint32_t k = REC_TOKS; more; ++k) {
    uint32_t we;
    deep(k, lds_word(w, x, e, test_mask, we, flags));
    n = k + 1;
    more = we < e;
    x = we + 1;
  }
  return n;
}


// Topic t's record (gm_common.h rec_at): all REC_U4 parts {tok0, tok1} {tok2, tok3} {tok4, tok5}
// {tok6, wbase, header}, or (A.hdr set) the first REC_PARTS_MIN and the header word to hdr[t]
// (lanes of consecutive topics fill whole lines there too), or (EVEN) the even-elided form's
// two parts {tok1, tok3} {tok4, tok5} and the header word with T_EQ0 / T_EQ2: 44 B per topic
// with nw and exact_id instead of 60.  (EVEN is a template parameter, of k_tok too: as a
// run-time branch it took k_tok<0,0> from 62 to 65 VGPRs, past the 64 at which two of its waves
// fit a SIMD beside three of the walk's, and the pipelined cfg3 step lost 2%: MEASUREMENTS r17.)
// Non-temporal for large batches
// (nt_rec: records are read back once, by the walk, and would evict its edges).
template <bool EVEN = false>
__device__ __forceinline__ void store_rec(const TokArgs& A, uint32_t t, const uint64_t (&tk)[REC_TOKS],
                                          uint32_t wb, uint32_t hd) {
  uint4* q = rec_at(A.rec, t);
  constexpr uint32_t S = REC_BLOCK;
  const bool full = A.hdr == nullptr;  // (wave-uniform)
  if constexpr (EVEN) {  // two parts, words 0 and 2 as a bit each in the header word
    hd |= (A.c0 != 0 && tk[0] == A.c0 ? T_EQ0 << 24 : 0u) | (A.c2 != 0 && tk[2] == A.c2 ? T_EQ2 << 24 : 0u);
    const uint4 e0 = make_uint4((uint32_t)tk[1], (uint32_t)(tk[1] >> 32), (uint32_t)tk[3], (uint32_t)(tk[3] >> 32));
    const uint4 e1 = make_uint4((uint32_t)tk[4], (uint32_t)(tk[4] >> 32), (uint32_t)tk[5], (uint32_t)(tk[5] >> 32));
    if (A.nt_rec) {
      typedef unsigned int u4v __attribute__((ext_vector_type(4)));
      __builtin_nontemporal_store(u4v{e0.x, e0.y, e0.z, e0.w}, (u4v*)q);
      __builtin_nontemporal_store(u4v{e1.x, e1.y, e1.z, e1.w}, (u4v*)(q + S));
      __builtin_nontemporal_store(hd, A.hdr + t);
    } else {
      q[0] = e0;
      q[S] = e1;
      A.hdr[t] = hd;
    }
    return;
  }
  const uint4 r0 = make_uint4((uint32_t)tk[0], (uint32_t)(tk[0] >> 32), (uint32_t)tk[1], (uint32_t)(tk[1] >> 32));
  const uint4 r1 = make_uint4((uint32_t)tk[2], (uint32_t)(tk[2] >> 32), (uint32_t)tk[3], (uint32_t)(tk[3] >> 32));
  const uint4 r2 = make_uint4((uint32_t)tk[4], (uint32_t)(tk[4] >> 32), (uint32_t)tk[5], (uint32_t)(tk[5] >> 32));
  const uint4 r3 = make_uint4((uint32_t)tk[6], (uint32_t)(tk[6] >> 32), wb, hd);
  if (A.nt_rec) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(u4v{r0.x, r0.y, r0.z, r0.w}, (u4v*)q);
    __builtin_nontemporal_store(u4v{r1.x, r1.y, r1.z, r1.w}, (u4v*)(q + S));
    __builtin_nontemporal_store(u4v{r2.x, r2.y, r2.z, r2.w}, (u4v*)(q + 2 * S));
    if (full)
      __builtin_nontemporal_store(u4v{r3.x, r3.y, r3.z, r3.w}, (u4v*)(q + 3 * S));
    else
      __builtin_nontemporal_store(hd, A.hdr + t);
  } else {
    q[0] = r0;
    q[S] = r1;
    q[2 * S] = r2;
    if (full)
      q[3 * S] = r3;
    else
      A.hdr[t] = hd;
  }
}

// DEFER = the committed index has plain route keys: k_exact runs every name's probe after this
// kernel, which only marks wildcard names (exact_id = X_WILDPEND, probed in the wildcard-key
// region there).  Otherwise a wildcard name probes the wildcard-key region here (rare).
// CP = copy-through (TokArgs cp_*): its own instantiation -- the extra stores in the default
// kernel cost the cfg3 tokenizer 35% (r04: 0.087 -> 0.117 ms)
// EVEN = the pass moves even-elided records (store_rec).
template <bool DEFER, bool CP, bool EVEN = false>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(6))) void k_tok(TokArgs A, ExactArgs X) {
  __shared__ uint4 s_buf[TILE_CHUNKS];
  const uint32_t tid = threadIdx.x;
  const uint32_t* s32 = (const uint32_t*)s_buf;
  // the pass's control words start here (no memset launch): zero, but CTL_PAIR_TOP past the
  // walk's static chunks; CTL_XHIT is left alone (other blocks may set it already: it holds a
  // pass sequence number, X.xseq)
  if (blockIdx.x == 0 && tid == 0 && A.ctl_host) A.ctl_host[CTL_LEGACY] = 0u;
  if (blockIdx.x == 0)
    for (uint32_t i = tid; i < CTL_N; i += WG) {
      const uint32_t cs = (i - CTL_CLAIM0) / CTL_CLAIM_STRIDE;
      const bool claim = i >= CTL_CLAIM0 && (i - CTL_CLAIM0) % CTL_CLAIM_STRIDE == 0 && cs < WALK_SHARDS;
      if (i != CTL_XHIT)
        A.ctl[i] = i == CTL_PAIR_TOP ? A.pair_top0 : claim ? A.claim0[cs] : 0u;
    }
  for (uint32_t t0 = blockIdx.x * WG; t0 < A.n; t0 += gridDim.x * WG) {
    const uint32_t t1 = min(t0 + WG, A.n);
    const uint32_t B0 = A.off[t0], B1 = A.off[t1];
    const uint32_t t = t0 + tid;
    // the lane's own offsets load in the same round trip as the tile
    const uint32_t tc = t < t1 ? t : t1 - 1;
    const uint32_t ob = A.off[tc], oe = A.off[tc + 1];
    if (CP && t < t1) {
      A.cp_off[t] = ob;
      if (t + 1 == A.n) A.cp_off[A.n] = oe;
    }
    uint32_t sh;
    const bool tiled = stage_tile<CP>(A.bytes, B0, B1, s_buf, sh, A.cp_bytes);
    __syncthreads();
    if (tiled) {
      // Records are stored in blocks of 64 topics, part-major (gm_common.h rec_at): part c of a
      // wave's topics is one contiguous 1-KB run, so each of a lane's four 16-B stores is a
      // full-line store of the wave
      // (r06; until then records were topic-major and went out through LDS to the same effect).
      // The rare wildcard-name probe reads the topic's bytes from global memory.
      uint64_t tk[REC_TOKS] = {0, 0, 0, 0, 0, 0, 0};
      uint32_t flags = 0, nwd = 0, hit = NONE;
      // token k >= REC_TOKS of this topic lives at wh[wb + k]: a topic has at most len + 1
      // levels, so off[t] + t is a collision-free base without any counter
      const uint32_t b = ob, len = oe - ob, wb = b + t;
      if (t < t1) {
        auto deep = [&](uint32_t k, uint64_t tok) { A.wh[wb + k] = tok; };
        nwd = tok_words_rec(s32, sh + (b - B0), len, A.test_mask, tk, deep, flags);
      }
      __syncthreads();  // every lane is done with the tile's bytes
      if (t < t1) {
        A.nw[t] = nwd;
        store_rec<EVEN>(A, t, tk, wb, nwd | (flags << 24));
        if (flags & T_WILD) {
          if (DEFER)
            hit = X_WILDPEND;
          else if (!A.wild_empty)
            hit = exact_lookup_wild(X, A.bytes, b, len);
          if (hit < X_WILDPEND) A.ctl[CTL_XHIT] = X.xseq;  // rare: a wildcard name's key
        }
        A.exact_id[t] = hit;
        if (A.rej) A.rej[t] = 0u;
      }
    } else if (t < t1) {
      // a tile too long for LDS (very long topics): bytes from global memory, records direct
      const uint32_t b = ob, len = oe - ob, wb = b + t;
      if (CP)
        for (uint32_t i = 0; i < len; ++i) A.cp_bytes[b + i] = A.bytes[b + i];
      uint64_t tk0 = 0, tk1 = 0, tk2 = 0, tk3 = 0, tk4 = 0, tk5 = 0, tk6 = 0;
      auto dst = [&](uint32_t k, uint64_t tok) {
        switch (k) {
          case 0: tk0 = tok; break;
          case 1: tk1 = tok; break;
          case 2: tk2 = tok; break;
          case 3: tk3 = tok; break;
          case 4: tk4 = tok; break;
          case 5: tk5 = tok; break;
          case 6: tk6 = tok; break;
          default: A.wh[wb + k] = tok;
        }
      };
      uint32_t flags, hit = NONE;
      const GlobBytes P{A.bytes + b};
      const uint32_t nwd = tok_words(P, len, A.test_mask, dst, flags);
      A.nw[t] = nwd;
      const uint64_t tk[REC_TOKS] = {tk0, tk1, tk2, tk3, tk4, tk5, tk6};
      store_rec<EVEN>(A, t, tk, wb, nwd | (flags << 24));
      if (flags & T_WILD) {
        if (DEFER)
          hit = X_WILDPEND;
        else if (!A.wild_empty)
          hit = exact_lookup_wild(X, A.bytes, b, len);
        if (hit < X_WILDPEND) A.ctl[CTL_XHIT] = X.xseq;
      }
      A.exact_id[t] = hit;
      if (A.rej) A.rej[t] = 0u;
    }
    __syncthreads();
  }
}

// ---- the probe over a table far beyond the TLB's reach (100M keys: 8.6 GB) ----
// Random lines over 8 GiB come at a third of the rate of a 2 GiB table (profiles/r02/
// gather_tlb.txt: 17 vs 52 G/s) when every wave draws from the whole table -- and at the 2 GiB
// rate when each workgroup draws from one range of at most ~2 GiB, whichever workgroups share a
// range (r05, tools/gather_bench.hip part mode, profiles/r05/gather_part.txt: 8 GiB in ranges
// of 1-2 GiB 47-49 G/s, 16 GiB in 2-GiB ranges 44 G/s).  The partitioned probe (an option,
// emqxgm_tune("exact_range_kb"): on cfg4 it is slower than k_exact, gm_kernels.hip
// XRANGE_MIN_TABLE): k_xhash hashes every name once ({home bucket, h32}, streamed out), and workgroup
// b probes, of its slice of the names, those whose home bucket lies in range b % R.  A wave
// scans XPART_SCAN x 64 names' homes, queues the ones in its range in LDS, then probes the queue
// one name per lane, so the probes run on (nearly) full waves.  Nothing is reordered: every
// name's exact id is written where it was.

// {home bucket, h32} of every name; a wildcard name with no wildcard keys is decided (NONE)
// and gets a home no range holds.
__global__ __launch_bounds__(WG) void k_xhash(const uint8_t* bytes, const uint32_t* off, uint32_t n,
                                              uint32_t* exact_id, ExactArgs X, bool wild_empty,
                                              uint2* xh) {
  for (uint32_t t = blockIdx.x * WG + threadIdx.x; t < n; t += gridDim.x * WG) {
    const uint32_t ob = off[t], len = off[t + 1] - ob;
    const bool wild = exact_id[t] == X_WILDPEND;
    if (wild && wild_empty) {
      exact_id[t] = NONE;
      xh[t] = make_uint2(NONE, 0u);
      continue;
    }
    const TopicWords T(bytes, ob, len);
    uint32_t a, c;
    key_hash_init(len, a, c);
    for (uint32_t k = 0; 4 * k < len; ++k) key_hash_word(T(k) & len_mask(len, k), a, c);
    const uint64_t fh = key_hash_final(a, c, X.full_mask);
    const uint64_t bk = wild ? X.xwbase + exact_slot(fh, X.xwmask) : exact_slot(fh, X.xmask);
    xh[t] = make_uint2((uint32_t)bk, (uint32_t)(fh >> 32));
  }
}

constexpr uint32_t XPART_SCAN = 8;  // 64-name groups a wave scans before it probes its queue

// gridDim.x = R x G: workgroup b takes bucket range b % R ([r * rb, r * rb + rb); a chain may
// run on past its end) and name slice b / R of G (split over its waves).
__global__ __launch_bounds__(WG) void k_exact_part(const uint8_t* bytes, const uint32_t* off,
                                                   uint32_t n, uint32_t* exact_id, ExactArgs X,
                                                   const uint2* xh, uint32_t R, uint32_t rb,
                                                   uint32_t* ctl) {
  constexpr uint32_t WAVES = WG / 64;
  __shared__ uint32_t s_q[WAVES][XPART_SCAN * 64];
  const uint32_t r = blockIdx.x % R, g = blockIdx.x / R, G = gridDim.x / R;
  const uint64_t lo = (uint64_t)r * rb, hi = lo + rb;
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t nw = (uint64_t)G * WAVES, wi = (uint64_t)g * WAVES + wv;
  const uint32_t t0 = (uint32_t)(n * wi / nw), t1 = (uint32_t)(n * (wi + 1) / nw);
  uint32_t* q = s_q[wv];
  bool any = false;
  for (uint32_t c = t0; c < t1; c += XPART_SCAN * 64) {
    // the homes of the next XPART_SCAN x 64 names, all loads in flight, then the queue
    uint32_t home[XPART_SCAN];
#pragma unroll
    for (uint32_t k = 0; k < XPART_SCAN; ++k) {
      const uint32_t t = c + k * 64 + lane;
      home[k] = t < t1 ? xh[t].x : NONE;
    }
    uint32_t nq = 0;
#pragma unroll
    for (uint32_t k = 0; k < XPART_SCAN; ++k) {
      const bool in = home[k] != NONE && home[k] >= lo && home[k] < hi;
      const uint64_t m = __ballot(in);
      if (in) q[nq + mbcnt64(m)] = c + k * 64 + lane;
      nq += (uint32_t)__popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (uint32_t j = lane; j < nq; j += 64) {
      const uint32_t t = q[j];
      const uint2 h = xh[t];
      const uint32_t ob = off[t], len = off[t + 1] - ob;
      const TopicWords T(bytes, ob, len);
      uint32_t tw[XINL / 4];
#pragma unroll
      for (uint32_t k = 0; k < XINL / 4; ++k) tw[k] = 4 * k < len ? (T(k) & len_mask(len, k)) : 0u;
      const bool wild = h.x >= X.xwbase;  // the wildcard-key region follows the plain one
      const uint64_t base = wild ? X.xwbase : 0ull, mask = wild ? X.xwmask : X.xmask;
      const uint32_t id = exact_probe(X, T, len, base, mask, h.x, h.y, tw);
      exact_id[t] = id;
      any |= id != NONE;
    }
    __builtin_amdgcn_wave_barrier();  // the queue's reads are done before the next scan writes it
  }
  if (__syncthreads_or(any) && threadIdx.x == 0) ctl[CTL_XHIT] = X.xseq;  // one store per block
}

// Every name's route-key probe when the index has plain route keys (after k_tok<true>): one lane
// per topic, one line per bucket of its chain (gm_common.h "Exact route-key table").  A block
// takes a tile of 256 names and stages their packed bytes in LDS with coalesced 16-B loads (as
// k_tok does) before hashing them: read straight from global memory, every dword of a name was
// two lane-divergent loads on the vector memory path (r06, one box: cfg2's 1M names 61.7 ->
// 47.3 us, cfg4's 87.1 -> 83.8 us; profiles/r06/exact/).  Tiles too long for LDS read global
// memory.
__global__ __launch_bounds__(WG) void k_exact(const uint8_t* bytes, const uint32_t* off,
                                              uint32_t n, uint32_t* exact_id, ExactArgs X,
                                              bool wild_empty, uint32_t* ctl) {
  __shared__ uint4 s_buf[TILE_CHUNKS];
  const uint32_t* s32 = (const uint32_t*)s_buf;
  bool any = false;
  for (uint32_t t0 = blockIdx.x * WG; t0 < n; t0 += gridDim.x * WG) {  // (block-uniform)
    const uint32_t t1 = min(t0 + WG, n), t = t0 + threadIdx.x;
    const uint32_t B0 = off[t0], B1 = off[t1];
    const uint32_t tc = t < t1 ? t : t1 - 1;
    const uint32_t ob = off[tc], len = off[tc + 1] - ob;
    const bool wild = exact_id[tc] == X_WILDPEND;
    uint32_t sh;
    const bool tiled = stage_tile(bytes, B0, B1, s_buf, sh);
    __syncthreads();
    if (t < t1) {
      uint32_t id = NONE;
      if (!(wild && wild_empty))
        id = tiled ? exact_lookup(X, bytes, ob, len, wild, LdsTopicWords(s32, sh + (ob - B0), len))
                   : exact_lookup(X, bytes, ob, len, wild);
      exact_id[t] = id;
      any |= id != NONE;
    }
    __syncthreads();  // every lane is done with the tile
  }
  if (__syncthreads_or(any) && threadIdx.x == 0) ctl[CTL_XHIT] = X.xseq;  // one store per block
}

// The route-key probe of the names one key shard owns (the key-partitioned layout of cfg4,
// DESIGN.md 5, SURVEY 8e): a name's owner is the high half of its key hash mod `parts`
// (emqxgm_key_owners); a name owned elsewhere gets NONE without a probe.  Only the plain-key
// region is probed: a wildcard name never equals a plain key (its wildcard-key probe is the
// topic-block match's, whose shard holds every wildcard key).
__global__ __launch_bounds__(WG) void k_exact_owned(const uint8_t* bytes, const uint32_t* off,
                                                    uint32_t n, uint32_t* exact_id, ExactArgs X,
                                                    uint32_t parts, uint32_t part) {
  for (uint32_t t = blockIdx.x * WG + threadIdx.x; t < n; t += gridDim.x * WG) {
    const uint32_t ob = off[t], len = off[t + 1] - ob;
    const TopicWords T(bytes, ob, len);
    uint32_t a, c, tw[XINL / 4];
    key_hash_init(len, a, c);
#pragma unroll
    for (uint32_t k = 0; k < XINL / 4; ++k) {
      tw[k] = 4 * k < len ? (T(k) & len_mask(len, k)) : 0u;
      if (4 * k < len) key_hash_word(tw[k], a, c);
    }
    for (uint32_t k = XINL / 4; 4 * k < len; ++k) key_hash_word(T(k) & len_mask(len, k), a, c);
    const uint64_t fh = key_hash_final(a, c, X.full_mask);
    uint32_t id = NONE;
    if ((uint32_t)(fh >> 32) % parts == part)
      id = exact_probe(X, T, len, 0ull, X.xmask, exact_slot(fh, X.xmask), (uint32_t)(fh >> 32), tw);
    exact_id[t] = id;
  }
}
