// gm_common.h -- layout constants and token/hash functions shared by the host index builder
// and the gfx950 kernels.  The device index layout is described in DESIGN.md "Data layout".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GM_HD __host__ __device__ __forceinline__
#else
#define GM_HD static inline
#endif

namespace gm {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t TOMB = 0xFFFFFFFEu;  // deleted slot / exact entry (delta commits)

// ---- level tokens ---------------------------------------------------------------------
// A level token identifies one topic level (emqx_topic:words/1 element).  A word of at most
// 7 bytes is packed injectively: bytes little-endian in bits 0..55, length in bits 56..62,
// bit 63 clear -- two different short words can never share a token, so trie edges over
// short words are exact.  A longer word gets bit 63 set and a 63-bit hash; only filters with
// such a word need the byte verification pass.  '+' has a token no word can have.
constexpr uint64_t TOK_HASHED = 1ull << 63;
constexpr uint64_t PLUS_TOK = 0x7FFFFFFFFFFFFFFFull;  // length field 127: impossible for a word
constexpr uint32_t TOK_INLINE_MAX = 7;

constexpr uint64_t FNV_OFF = 0xcbf29ce484222325ull;
constexpr uint64_t FNV_PRIME = 0x100000001b3ull;

GM_HD uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

GM_HD uint64_t fnv_step(uint64_t h, uint32_t b) { return (h ^ b) * FNV_PRIME; }

// Token of a finished word: `packed` = its first bytes little-endian, `fnv` = FNV-1a state
// over all its bytes, `len` = its length.  `test_mask` != 0 selects the collision-test mode in
// which every word is hashed and only the masked bits of the hash are kept.
GM_HD uint64_t word_token(uint64_t packed, uint64_t fnv, uint32_t len, uint64_t test_mask) {
  if (test_mask) return TOK_HASHED | (fmix64(fnv) & test_mask);
  if (len <= TOK_INLINE_MAX) return packed | ((uint64_t)len << 56);
  return TOK_HASHED | (fmix64(fnv) >> 1);
}

// Route-key hash (exact table): over the key's bytes taken as little-endian 32-bit words, the
// last one zero-padded, in two 32-bit multiply-rotate lanes folded through fmix64.  It needs
// only the bytes (not the level tokens), so the device issues the table probe before it
// tokenises.  `mask` keeps fewer bits in the collision tests.
GM_HD void key_hash_init(uint32_t len, uint32_t& a, uint32_t& b) {
  a = 0x9747b28cu ^ len;
  b = 0x85ebca6bu + len;
}
GM_HD void key_hash_word(uint32_t w, uint32_t& a, uint32_t& b) {
  a ^= w * 0xcc9e2d51u;
  a = ((a << 15) | (a >> 17)) * 5u + 0xe6546b64u;
  b += w * 0x1b873593u;
  b = ((b << 13) | (b >> 19)) * 0x85ebca6bu ^ 0xc2b2ae35u;
}
GM_HD uint64_t key_hash_final(uint32_t a, uint32_t b, uint64_t mask) {
  return fmix64(((uint64_t)a << 32) | b) & mask;
}
GM_HD uint64_t key_hash(const uint8_t* p, uint32_t len, uint64_t mask) {
  uint32_t a, b;
  key_hash_init(len, a, b);
  for (uint32_t i = 0; i < len; i += 4) {
    uint32_t w = 0;
    for (uint32_t j = 0; j < 4 && i + j < len; ++j) w |= (uint32_t)p[i + j] << (8 * j);
    key_hash_word(w, a, b);
  }
  return key_hash_final(a, b, mask);
}

// ---- edge slots -------------------------------------------------------------------------
// 32 B per slot, 2 x uint4, one slot per trie edge (parent --level token--> child C):
//   s0 = {tok.lo, tok.hi, parent, cf}       key = (parent node id, level token), exact
//   s1 = {hf, tw, p.cf, p.hf}
//   cf  = C's node id (26 bits) | C's flags (4 bits) | C's depth code (2 bits)
//   hf  = filter id of "C_path/#", NONE, or LIST_MULTI | index into the multi[] list pool
//   tw  = wildcard filter(s) ending exactly at C (fid, or LIST_MULTI|multi index)
//   p   = C's '+' child {cf, hf} (cf = 0 if there is none; node 0 is the root, never a child),
//         carried so that the walk expands it without a probe.  The rest of p (its terminal
//         filters, its own '+' child) comes from the (C, '+') slot when the walk needs it.
// Non-wildcard trie keys ending at a node (only single-level '$' topics read them,
// emqx_trie.erl:287) live in a per-node side array.  An empty slot has parent == NONE; a slot
// freed by a delta commit has parent == TOMB (never a node id, not empty: lookups go on).
// Slots come in 64-B buckets of EBUCKET (one line: a probe loads and checks both slots, so a
// collision inside the bucket costs no extra round trip); an edge goes to the first free slot
// of its home bucket (edge_slot) or of the buckets after it, and a lookup stops at a bucket
// with a free slot -- or at a closed one (EDGE_CLOSED below: s1.w of a slot whose child has no
// '+' child, where p.hf has no reader).
constexpr uint32_t SLOT_U4 = 2;
constexpr uint32_t EBUCKET = 2;
constexpr uint32_t EDGE_SLACK = 4;  // slots >= 4 x edges (load <= 1/4): fewer bucket overflows
constexpr uint32_t CF_ID_BITS = 26;
constexpr uint32_t CF_ID_MASK = (1u << CF_ID_BITS) - 1;
constexpr uint32_t MAX_NODES = CF_ID_MASK - 2;  // ids stay below FAT_ID and TOMB's / NONE's low 26 bits
// Fat buckets (path compression of single-literal-child nodes).  A node C at depth 2, 4 or 6,
// reached by a literal edge, whose only literal child is G, takes a whole bucket: C's slot in
// the bucket's first half and G's slot in its second half, whose parent word is FAT_ID | G's
// signature (FAT_ID is never a node id, so no key probe matches the half).  G has no slot at
// its own hash position: a walk that resolves C finds G in the line it already loaded and, when
// the topic's word equals G's token, creates G's state in the same round trip; otherwise C has
// no matching literal child.  The root's only literal child, when it has one, is carried in
// the kernel arguments the same way.  A delta commit that gives a fat node a second literal
// child moves the half to its own hash position (the half's slot becomes TOMB), so a bucket
// holds a half exactly when its first node's literal children are that half alone.
constexpr uint32_t FAT_ID = CF_ID_MASK - 2;  // = MAX_NODES: no id; TOMB and NONE have low bits ..FE, ..FF
constexpr uint32_t FAT_MAX_DEPTH = 6;  // C's word (level depth(C)) is a record token (< REC_TOKS)
// Child signature: the top 6 bits of a slot's parent word (parent ids use 26) hold a 1-bit-per-
// class summary of the child's literal children's level tokens (class = sig_bit(token)); the
// walk does not probe a literal child whose token's class bit is clear.  Bits are only ever
// added (a delta commit ORs a new child in, deletions leave them), so a clear bit is exact.
// Lent signatures: a child C without literal children (CF_LIT clear in cf) has no use for the
// field, so it holds the signature of C's '+' child instead (0: C has none) -- the carried
// '+' child p has no bits to spare in p.cf, and the walk, which creates p's state without a probe,
// drops the literal probe under p when the next word's class bit is clear (cfg3: the k of
// site/S/device/D/+/k under a device D that has only '+' below it).  With CF_LIT set the field
// is C's own (0: keyed, below).  The same rule holds for a fat half's word (FAT_ID | field), the
// root's half in the kernel arguments and the root's own signature.  A reader that ignores lent
// bits is still exact: they only ever drop probes that find nothing.
// Closed buckets (r10).  A bucket is closed when no live edge whose chain (the buckets from its
// home to its slot) starts at or passes through it sits beyond it: a lookup that finds neither
// its key nor an empty slot there ends with "no such child" instead of loading the next bucket.
// The mark lives in the bucket's own line: s1.w of a live slot whose child has no '+' child
// (CF_PLUS clear in its cf, so no reader looks at the carried p.hf) holds EDGE_CLOSED instead of
// NONE while its bucket is closed.  Every such slot of the bucket carries it, the halves of a fat
// bucket included; a bucket whose children all have a '+' child goes unmarked, and so do empty
// slots, TOMB slots and the copies in the kernel arguments.  A reader tests CF_PLUS first (the
// value alone could be a p.hf).  Marks are taken away in the commit that places an edge past
// the bucket and come back only with a full build or a snapshot load, which derive them from the
// placement (tune "closed_buckets" 0: the walk ignores them).  A reader that ignores the mark is
// still exact: it only ever ends chains that find nothing.
constexpr uint32_t EDGE_CLOSED = 0xFFFFFFFCu;
constexpr uint32_t SIG_SHIFT = CF_ID_BITS;
constexpr uint32_t SIG_CLASSES = 6;
GM_HD uint32_t sig_class(uint64_t tok) {
  return (uint32_t)(((((tok * 0x9E3779B97F4A7C15ull) >> 32) & 0xFFFFFFFFull) * SIG_CLASSES) >> 32);
}
GM_HD uint32_t sig_bit(uint64_t tok) { return 1u << sig_class(tok); }
// Depth code h of the child C (bits CF_H0 | CF_H1 = h & 1, h & 2): every filter strictly below
// C ends within h levels of C and none of them is a '#' filter, so a topic with more than h
// words left after C cannot match anything below it and the walk does not expand C's children.
// h = 0: unbounded (a '#' below, deeper filters, or unknown).  Exact at a full build; a delta
// commit only ever resets codes to 0.
constexpr uint32_t CF_H0 = 1u << 26;
constexpr uint32_t CF_LIT = 1u << 27;   // child has literal (non-'+') children
constexpr uint32_t CF_PLUS = 1u << 28;  // child has a '+' child
constexpr uint32_t CF_H1 = 1u << 29;
constexpr uint32_t CF_HMASK = CF_H0 | CF_H1;
GM_HD uint32_t cf_depth_code(uint32_t cf) { return ((cf >> 26) & 1u) | ((cf >> 28) & 2u); }
GM_HD uint32_t cf_with_depth_code(uint32_t cf, uint32_t h) {
  return (cf & ~CF_HMASK) | ((h & 1u) << 26) | ((h & 2u) << 28);
}
constexpr uint32_t CF_TW = 1u << 30;    // child terminates >=1 wildcard filter
constexpr uint32_t CF_TN = 1u << 31;    // child terminates >=1 non-wildcard trie key
// In the carried copy of a '+' child's cf (p.cf) bit 31 means something else: a '+' node never
// ends a non-wildcard key (a path through '+' is a wildcard filter), so CF_TN is free there and
// CF_PTW says "p.hf holds the child's terminal filters (tw), it has no '#' filter": the walk then
// emits them without a '+' probe.
constexpr uint32_t CF_PTW = 1u << 31;
constexpr uint32_t LIST_MULTI = 0x80000000u;  // tw/tn value is a multi[] index
// The closed mark of a slot {.., cf}, {.., .., .., phf} (EDGE_CLOSED above); `off` = 0, or 1 when
// marks are ignored (bit 0 of EDGE_CLOSED is clear, so the comparison then never holds).
GM_HD bool slot_closed(uint32_t cf, uint32_t phf, uint32_t off) {
  return !(cf & CF_PLUS) && (phf | off) == EDGE_CLOSED;
}

GM_HD uint64_t edge_slot(uint32_t parent, uint64_t tok, uint64_t mask) {
  return fmix64(tok ^ ((uint64_t)parent * 0x9e3779b97f4a7c15ull)) & mask;
}
// Token-keyed parents.  The home bucket of a child edge (P, t) is edge_slot(P, t) -- or, when P
// is KEYED and t a literal word (not '+'), a hash of t alone, so the edges of the parents that share a child token share a
// line: on cfg3 site/S/device/D and site/+/device/D (D a global device id, one site's) sit in
// one bucket, and the walk's second probe of D is an L1/L2 hit instead of an HBM miss (r04).
// A full build keys the parents with many literal children whose every child token is the child
// of at most EBUCKET keyed parents (tune "keyed"); a node reached by a '+' edge or the root is
// never keyed (the walk creates those states without their slot).  The flag travels in the
// parent's slot as an impossible signature: CF_LIT with sig 0 (every literal child of an
// unkeyed node sets its class bit), so a keyed node's children are never filtered by class.
GM_HD uint64_t edge_home(uint32_t parent, uint64_t tok, uint64_t mask, bool keyed) {
  return keyed ? (fmix64(tok + 0x5851f42d4c957f2dull) & mask) : edge_slot(parent, tok, mask);
}
// Exact route-key table: 64-B buckets (one line) of XBUCKET 32-B entries, filled in order
// (linear probing over buckets); exact_slot gives the home bucket.  An entry carries the key's
// first XINL bytes, so a probe for a key of up to XINL bytes is decided by the one line it loads
// (no dependent load of a verification record):
//   e0 = {h32 (high half of the key hash), fid, len, key bytes 0..3}
//   e1 = {key bytes 4..7, 8..11, 12..15, 16..19}   (zero past len)
// A longer key's inline prefix and hash filter the candidates and its full bytes (verification
// record / string pool) confirm.  An empty entry has fid == NONE, a deleted one fid == TOMB.
// A bit per bucket (xovf) says whether some key whose probe passed it was placed beyond it: a
// probe that finds neither its key nor an empty entry in a bucket goes on only if the bit is
// set, so a miss costs its home bucket's line (plus the bit word, loaded beside it) even when
// that bucket is full.  Bits are only set (a delta commit may leave one set after deletions).
constexpr uint32_t XBUCKET = 2;
constexpr uint32_t XENT_U4 = 2;
constexpr uint32_t XINL = 20;
GM_HD uint64_t exact_slot(uint64_t fh, uint64_t mask) { return fmix64(fh + 0x632be59bd9b4e019ull) & mask; }
// k_tok's exact_id marker for a wildcard name whose route-key probe k_exact still has to run
constexpr uint32_t X_WILDPEND = 0xFFFFFFFDu;

// Filter verification record (64 B per filter id): {u32 len, 60 bytes of the filter}; the
// bytes of longer filters are read from the string pool.
constexpr uint32_t VREC = 64;
constexpr uint32_t VINL = 60;

// Per-topic record written by the tokenizer, 64 B = REC_U4 x uint4 parts:
//   {tok0, tok1} {tok2, tok3} {tok4, tok5} {tok6.lo, tok6.hi, wbase, n_words | flags << 24}
// (tokens past the last level are 0); level tokens from REC_TOKS on are read from the token
// array at wbase.  Topics have at most 32,768 levels (65,535 bytes).  Stored in blocks of
// REC_BLOCK topics, part-major within a block (r06): part c of topic t at uint4 index
// (t / 64) * 256 + c * 64 + t % 64, so a wave's lanes, holding consecutive topics, read and write
// whole lines per 16-B access, and one address with immediate offsets of 1 KB reaches every part.
// A scratch of n topics holds ceil(n / 64) whole blocks.
// A pass stores and loads only the parts its index can read (rec_parts below): the walk reads
// level token k only where the index has a literal edge at level k, that is for k < max_depth,
// and wbase only for levels from REC_TOKS on.  With fewer than REC_U4 parts the header word
// n_words | flags << 24 travels in a u32 per topic beside the records (Scratch::hdr), the
// block stride stays REC_U4 parts, and the walk takes the tokens not stored as 0.
// The even-elided form (r17; a pass over an index whose literal edges of level 0, and those of
// level 2, each carry at most one token c_k != 0: `site/<id>/device/<id>/...`): all the walk can
// learn from word k of such a level is whether it equals c_k, so the record is two parts,
//   {tok1, tok3} {tok4, tok5}
// and the header word carries T_EQ0 / T_EQ2 (word k is present and its token is c_k).  The walk
// rebuilds tok0 / tok2 as c_k or 0 when it activates the topic (rec_tokens_even): no edge of the
// level carries 0, and only equality with edge tokens, bucket homes computed from them and
// signature classes (which decide probes, never rows) depend on a level token.
constexpr uint32_t REC_U4 = 4;
constexpr uint32_t REC_BLOCK = 64;
constexpr uint32_t REC_TOKS = 7;
constexpr uint32_t REC_PARTS_MIN = 3;  // rec_parts' least: the walk's readers are 3 parts, all 4,
                                       // and the even-elided form's 2 (REC_R3 / RFULL / REVEN below)
template <class T>
GM_HD T* rec_at(T* rec, uint32_t t) {
  return rec + (uint64_t)(t / REC_BLOCK) * (REC_BLOCK * REC_U4) + (t % REC_BLOCK);
}
// Parts a pass over an index whose deepest filter has max_depth levels stores and loads:
// ceil(min(max_depth, REC_TOKS) / 2), at least REC_PARTS_MIN; REC_U4 from 7 levels on (tok6, and
// wbase for the levels past it, live in the last part).
GM_HD uint32_t rec_parts(uint32_t max_depth) {
  const uint32_t p = ((max_depth < REC_TOKS ? max_depth : REC_TOKS) + 1u) / 2u;
  return p < REC_PARTS_MIN ? REC_PARTS_MIN : p;
}
// The walk's load of topic t's record into {a, b, c, d} (U4 = uint4).  FULL: all REC_U4 parts,
// the header in d.w and wbase in d.z.  Otherwise REC_PARTS_MIN parts and the header word from
// hdr[t] into d.w: d.x, d.y and d.z keep what the caller put there (0: tok6 and wbase read 0).
template <bool FULL, class U4>
GM_HD void rec_load(const U4* rec, const uint32_t* hdr, uint32_t t, U4& a, U4& b, U4& c, U4& d) {
  const U4* q = rec_at(rec, t);
  a = q[0];
  b = q[REC_BLOCK];
  c = q[2 * REC_BLOCK];
  if (FULL)
    d = q[3 * REC_BLOCK];
  else
    d.w = hdr[t];
}
// Level tokens 0 .. REC_TOKS - 1 of a loaded record.
template <class U4>
GM_HD void rec_tokens(const U4& a, const U4& b, const U4& c, const U4& d, uint64_t (&tk)[REC_TOKS]) {
  tk[0] = ((uint64_t)a.y << 32) | a.x;
  tk[1] = ((uint64_t)a.w << 32) | a.z;
  tk[2] = ((uint64_t)b.y << 32) | b.x;
  tk[3] = ((uint64_t)b.w << 32) | b.z;
  tk[4] = ((uint64_t)c.y << 32) | c.x;
  tk[5] = ((uint64_t)c.w << 32) | c.z;
  tk[6] = ((uint64_t)d.y << 32) | d.x;
}
constexpr uint32_t T_WILD = 1u;    // some level is exactly '+' or '#'  -> trie result []
constexpr uint32_t T_DOLLAR = 2u;  // first byte is '$' -> no root '+'/'#' (emqx_trie.erl:282)
constexpr uint32_t T_EQ0 = 4u;     // even-elided records only: word 0 is there and its token is c_0,
constexpr uint32_t T_EQ2 = 8u;     //   word 2 and c_2

// The tokens of the literal edges of one level, as the host model keeps them for levels 0 and 2
// (TrieModel::lev, DevIndex::lev_st): none, one (c_k != 0), many (or the one token is 0, the
// empty word).  Delta commits only move it upwards.
enum : uint32_t { LEV_NONE = 0, LEV_ONE = 1, LEV_MANY = 2 };
// The record readers of k_walk (its REC template parameter): REC_PARTS_MIN parts and the header
// array, all REC_U4 parts, or the two parts of the even-elided form and the header array.
enum : uint32_t { REC_R3 = 0, REC_RFULL = 1, REC_REVEN = 2 };
constexpr uint32_t REC_PARTS_EVEN = 2;

// The even-elided form's load of topic t's record: parts {tok1, tok3} into a, {tok4, tok5} into
// b, the header word into d.w; c and the rest of d keep what the caller put there (0).
template <class U4>
GM_HD void rec_load_even(const U4* rec, const uint32_t* hdr, uint32_t t, U4& a, U4& b, U4& d) {
  const U4* q = rec_at(rec, t);
  a = q[0];
  b = q[REC_BLOCK];
  d.w = hdr[t];
}
// Its level tokens: tok0 / tok2 rebuilt from the header's T_EQ0 / T_EQ2 and the pass's c0 / c2
// (0: the level has no literal edge; the bit is clear then), tok6 reads 0.
template <class U4>
GM_HD void rec_tokens_even(const U4& a, const U4& b, uint32_t hd, uint64_t c0, uint64_t c2,
                           uint64_t (&tk)[REC_TOKS]) {
  tk[0] = ((hd >> 24) & T_EQ0) ? c0 : 0ull;
  tk[1] = ((uint64_t)a.y << 32) | a.x;
  tk[2] = ((hd >> 24) & T_EQ2) ? c2 : 0ull;
  tk[3] = ((uint64_t)a.w << 32) | a.z;
  tk[4] = ((uint64_t)b.y << 32) | b.x;
  tk[5] = ((uint64_t)b.w << 32) | b.z;
  tk[6] = 0ull;
}

}  // namespace gm
