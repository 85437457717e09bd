/*
 * emqx_gpumatch.h -- C-ABI of the MI355X-native batched MQTT topic-matching engine.
 *
 * This is the drop-in boundary for the publish-time match path of EMQX 5.0.14
 * (fengyangdi/emqx).  Plain pointers and sizes only; no torch/HIP types.  Each entry point
 * names the reference interface it replaces (paths relative to the reference checkout):
 *
 *   emqxgm_trie_insert   <- emqx_trie:insert/1        apps/emqx/src/emqx_trie.erl:113-127
 *   emqxgm_trie_delete   <- emqx_trie:delete/1        apps/emqx/src/emqx_trie.erl:130-144
 *   emqxgm_trie_empty    <- emqx_trie:empty/0         apps/emqx/src/emqx_trie.erl:172-178
 *   emqxgm_trie_member   <- emqx_trie:lookup_topic/2  apps/emqx/src/emqx_trie.erl:267-271
 *   emqxgm_route_ref     <- route-bag key insert      apps/emqx/src/emqx_router_utils.erl:31-39
 *   emqxgm_route_unref   <- route-bag key delete      apps/emqx/src/emqx_router_utils.erl:48-71
 *   emqxgm_route_set     <- the same membership rule as a state, for a mirror of the committed
 *                           route table (emqx_router_utils.erl:34-39, 57-71; emqx_router.erl:72-92)
 *   emqxgm_async_match   <- emqx_trie:match/1 called from every publisher process at once
 *                           (emqx_broker.erl:218-232 -> emqx_router.erl:141-153, read_concurrency
 *                           tables emqx_trie.erl:70-75): the NIF's match_async/3
 *   emqxgm_commit        <- mnesia/mria commit point  (snapshot swap; readers never see partial
 *                           state; emqx_router_utils.erl:74-135 is where writes commit)
 *   emqxgm_match_batch   <- emqx_trie:match/1 + emqx_router:match_routes/1 over a batch of
 *                           published topics        apps/emqx/src/emqx_trie.erl:147-169,
 *                                                    apps/emqx/src/emqx_router.erl:141-157,
 *                           tokenising per emqx_topic:words/1 (emqx_topic.erl:155-169)
 *   emqxgm_match_device  <- the same with topic bytes / results resident in HBM
 *   emqxgm_filter_bytes  <- filter id -> filter binary (the trie returns binaries)
 *   emqxgm_route_add     <- emqx_router:do_add_route/2    apps/emqx/src/emqx_router.erl:124-138
 *   emqxgm_route_delete  <- emqx_router:do_delete_route/2 apps/emqx/src/emqx_router.erl:171-179
 *   emqxgm_subscriber_add/delete <- the local emqx_subscriber bag (emqx_broker.erl:150-214)
 *   emqxgm_publish_batch <- emqx_broker:publish/1 -> route(aggre(match_routes(Topic)))
 *                           apps/emqx/src/emqx_broker.erl:218-300, dispatch/2 :326-355
 *
 * Result semantics (bit-exact with the reference, SURVEY.md 8a/8a'):
 *   for topic t, trie row = { f in trie : emqx_trie:match(t) returns f }  (no duplicates;
 *   [] for a wildcard topic name), exact_id[t] = id of the route key equal to t's bytes (or
 *   EMQXGM_NONE).  match_routes(t) = routes(exact) ++ routes(row).  Row order is
 *   deterministic for a given committed index, but callers should treat it as a set, as the
 *   reference tests do (lists:sort).
 *
 * Return codes: 0 on success, or a negative errno: -EINVAL (bad argument), -ENOMEM (host or
 * device allocation failed), -EIO (device/HIP failure), -ENOENT (unknown id), -E2BIG (index
 * exceeds the device layout limits: 2^27 trie nodes, 2^31 filters).  There is no CPU fallback:
 * a device failure is reported, never silently recomputed on the host.
 *
 * Ownership: input buffers are borrowed for the duration of the call (the pipelined forms:
 * until the matching _wait returns).  Output arrays in emqxgm_out / emqxgm_dev_out are owned by
 * the engine and stay valid until the next match call on the same handle or emqxgm_destroy;
 * pipelined results as documented at their _submit.  Device inputs (emqxgm_match_device*) must
 * be complete in HBM when the call is made: the engine's streams do not wait for the caller's
 * (synchronise the stream that produced them first); the host-in forms copy their input
 * themselves.
 *
 * Threading (the reference reads with read_concurrency while writers commit in mria
 * transactions, emqx_trie.erl:70-75, emqx_router_utils.erl:74-135):
 *   - writers (insert/delete/route/subscriber calls, emqxgm_commit) are serialised by one writer
 *     lock; a full build of a large registry runs in a background thread without it (r05):
 *     meanwhile commits are delta patches of the current index, emqxgm_commit returns once the
 *     build is installed (changes made before it started show with it), and
 *     emqxgm_route_set_batch(.., EMQXGM_SET_COMMIT) returns as soon as its own changes show;
 *   - every match call reads the last committed epoch and never waits for a writer: a commit
 *     builds the next index beside the current one (a full build: seconds at 10M filters) and
 *     swaps it in atomically; a small delta is patched in place on the device, ordered on the GPU
 *     after the passes already enqueued and before every later one.  A pass that started before
 *     the swap completes against the epoch it started on;
 *   - match calls serialise among themselves (one pass context per call kind); filter_bytes,
 *     filter_copy, lookup_id, trie_member and trie_empty only take a shared read lock.
 */
#ifndef EMQX_GPUMATCH_H
#define EMQX_GPUMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMQXGM_NONE 0xFFFFFFFFu
#define EMQXGM_DEST_GROUP 0x80000000u /* dest handle bit: a shared-subscription group */
#define EMQXGM_RULE_EQ 1u    /* rule flag: {eq, Filter} -- the name must equal the filter */
#define EMQXGM_RULE_WORDS 2u /* rule flag: match/2 on word lists (no '$' clauses) */
#define EMQXGM_ABI_VERSION 13
#define EMQXGM_SET_COMMIT 1u /* emqxgm_route_set_batch: visible before the call returns */

typedef struct emqxgm emqxgm_t;

typedef struct emqxgm_cfg {
  int32_t device;          /* HIP device ordinal */
  uint32_t word_hash_bits; /* bits kept of each 37-bit level token (0 = 37, production);
                              small values only to force collisions in tests */
  uint32_t full_hash_bits; /* bits kept of the 64-bit whole-topic hash (exact table); 64 */
  uint32_t batch_max;      /* topics per device pass of emqxgm_match_batch (0 = 4Mi) */
  uint32_t walk_wg_per_cu; /* persistent walk workgroups per CU (0 = default) */
  uint32_t reject_cap;     /* verification rejects handled in-line per batch (0 = 1Mi);
                              beyond it a batch is redone on the compaction path */
  uint32_t reserved[2];
} emqxgm_cfg;

typedef struct emqxgm_out { /* host-resident result of emqxgm_match_batch */
  uint32_t n;               /* topics */
  uint64_t n_pairs;         /* total trie matches */
  const uint64_t* row_ptr;  /* [n+1] CSR offsets into filter_id */
  const uint32_t* filter_id;/* [n_pairs] matched trie filter ids */
  const uint32_t* exact_id; /* [n] route key equal to the topic, or EMQXGM_NONE */
} emqxgm_out;

typedef struct emqxgm_dev_out { /* device-resident result of emqxgm_match_device */
  uint32_t n;
  uint32_t n_pairs;
  const uint32_t* row_ptr;  /* device [n+1] */
  const uint32_t* filter_id;/* device [n_pairs] */
  const uint32_t* exact_id; /* device [n] */
  const uint32_t* n_words;  /* device [n] level count per topic (emqx_topic:levels/1) */
} emqxgm_dev_out;

typedef struct emqxgm_stats {
  uint64_t epoch;
  uint64_t n_filters;       /* ids ever assigned */
  uint64_t n_trie_filters;  /* committed trie members */
  uint64_t n_route_keys;    /* committed route keys */
  uint64_t n_nodes;         /* trie nodes (incl. root) */
  uint64_t n_edges;
  uint64_t edge_slots;
  uint64_t exact_slots;
  uint64_t device_bytes;    /* bytes of the committed device index */
  uint32_t max_depth;       /* deepest trie filter (levels) */
  uint32_t legacy_batches;  /* batches redone on the compaction path (many rejects) */
  uint64_t batches, topics, pairs;
  uint64_t rejected_pairs;  /* staged pairs rejected by byte verification (hash collisions) */
  uint64_t reruns;          /* passes redone (staging growth or legacy path) */
  double walk_ms;           /* summed walk-kernel time (HIP events), if profiling is on */
  uint64_t walk_launches;
  double total_ms;          /* summed device time of whole match passes, if profiling is on */
  uint64_t full_commits;    /* commits that rebuilt the device index */
  uint64_t delta_commits;   /* commits that patched it in place (small deltas) */
  double last_commit_ms;    /* host wall time of the last commit (build/patch + upload) */
  double tok_ms;            /* summed tokenizer-kernel time (HIP events), if profiling is on */
  uint64_t tok_launches;
  double exact_ms;          /* summed exact route-key probe time (k_exact; 0 without plain keys) */
  uint64_t keyed_nodes;     /* trie nodes whose literal children are placed by token */
  uint64_t buffer_grows;    /* pass scratch / host-pipe buffers reallocated (each a stall) */
  uint64_t sync_gathers;    /* host windows whose filter block outgrew its estimate (finished
                               synchronously in the wait) */
  uint64_t bg_builds;       /* full builds run in the background, beside the writers (r05) */
  uint64_t bg_waits;        /* commits that waited for one: the current tables could not take
                               their delta */
  double last_build_ms;     /* wall time of the last full build (background: start to ready) */
  uint64_t catchup_changes; /* filters replayed onto the last background build at its install */
  uint64_t even_passes;     /* passes enqueued with even-elided topic records (tune "rec_even") */
} emqxgm_stats;

int emqxgm_abi_version(void);
int emqxgm_create(const emqxgm_cfg* cfg, emqxgm_t** out);
void emqxgm_destroy(emqxgm_t* h);

/* Index mutation (applies to the pending state; visible to match after emqxgm_commit). */
int emqxgm_trie_insert(emqxgm_t* h, const uint8_t* filter, uint32_t len, uint32_t* id);
int emqxgm_trie_delete(emqxgm_t* h, const uint8_t* filter, uint32_t len);
int emqxgm_route_ref(emqxgm_t* h, const uint8_t* filter, uint32_t len, uint32_t* id);
int emqxgm_route_unref(emqxgm_t* h, const uint8_t* filter, uint32_t len);
/* Bulk forms: n filters packed in bytes, filter i = bytes[offsets[i] .. offsets[i+1]). */
int emqxgm_trie_insert_many(emqxgm_t* h, const uint8_t* bytes, const uint64_t* offsets,
                            uint64_t n, uint32_t* ids /* nullable */);
int emqxgm_route_ref_many(emqxgm_t* h, const uint8_t* bytes, const uint64_t* offsets,
                          uint64_t n, uint32_t* ids /* nullable */);
int emqxgm_commit(emqxgm_t* h, uint64_t* epoch /* nullable */);
/* Health of the index (r06; SURVEY 5 "Failure detection").  The reference's route writes abort in
 * the caller when they fail (mria transactions, emqx_router_utils.erl:114-118); here the caller's
 * tables already hold a change when the device refuses it, so the engine fails CLOSED: a commit
 * that fails (emqxgm_commit, or the commit of an EMQXGM_SET_COMMIT set), a set that fails half-way
 * (-E2BIG) and emqxgm_mark_stale (the host saw a timeout or a failed window) mark the index
 * STALE, and every match entry (emqxgm_match_batch*, _match_device*, emqxgm_publish_batch, the
 * windows of the concurrent entry) returns -ESTALE until a repair -- the caller answers from its
 * own tables (the reference path) meanwhile, so no answer ever comes from an index that lacks a
 * change the caller made.  Repair: a successful emqxgm_commit clears the mark when no mark came
 * during it, every EMQXGM_STALE_RESYNC mark has a full resync (emqxgm_route_sync_begin .. _end)
 * begun after it, and an event on each of the engine's streams completes within "probe_ms"
 * (emqxgm_tune, 2000 default).  emqxgm_commit returns -ESTALE (-ETIMEDOUT: the probe) while the
 * index stays stale after its commit.  emqxgm_get_health returns the stale bits (0 = healthy). */
#define EMQXGM_STALE_COMMIT 1u /* a commit failed: the pending registry holds the change */
#define EMQXGM_STALE_RESYNC 2u /* the registry may lack changes: a full resync must follow */
typedef struct emqxgm_health_s {
  uint32_t stale;     /* EMQXGM_STALE_* bits; 0 = healthy */
  int32_t last_error; /* the last mark's errno (negative) */
  uint64_t marks;     /* times marked */
  uint64_t repairs;   /* times a repair cleared the marks */
  uint64_t refused;   /* match calls refused with -ESTALE */
} emqxgm_health_t;
int emqxgm_get_health(emqxgm_t* h, emqxgm_health_t* out);
/* The host's report (a window that timed out or failed): EMQXGM_STALE_RESYNC with errno err. */
int emqxgm_mark_stale(emqxgm_t* h, int err);
/* Index snapshot (the reference rebuilds its ram_copies route tables at start,
 * emqx_router.erl:78-92): _save commits pending changes and writes the committed registry (filter
 * strings, trie / route-key membership, routes, subscribers) and the host model of the device
 * index to `path`; _load restores them into a fresh handle of the same configuration and
 * publishes the index without rebuilding it (the device tables are generated from the model).
 * -EBUSY: the handle is not fresh; -EINVAL: not a snapshot of this configuration. */
int emqxgm_snapshot_save(emqxgm_t* h, const char* path);
int emqxgm_snapshot_load(emqxgm_t* h, const char* path);
/* Level-triggered route-key membership, for a mirror of the committed route table (the NIF's sync
 * process): present != 0 makes `filter` a route key and, when it is a wildcard filter
 * (emqx_topic:wildcard/1), a trie member; present == 0 removes both -- the state
 * emqx_router_utils.erl:34-39, 57-71 keeps (a route key exists while its filter has a route, a
 * wildcard filter is in the trie while it has one).  Idempotent: the index converges to the
 * route table's state whatever the number and order of the calls that told it so.  It overrides
 * the refcount emqxgm_route_ref / _unref keep: a mirror uses this call alone.  Visible after
 * emqxgm_commit. */
int emqxgm_route_set(emqxgm_t* h, const uint8_t* filter, uint32_t len, int present);
int emqxgm_route_set_many(emqxgm_t* h, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                          int present);
/* The same for n filters at once, each with its own state (present[i] != 0; present == NULL: all
 * present), and with flags EMQXGM_SET_COMMIT a commit that makes them visible to every match
 * started after the call returns: the writing node's subscribe / unsubscribe path (SURVEY 8b's
 * post-maybe_trans hook: the reference's subscriber has its route before SUBACK,
 * emqx_broker.erl:163-168, 484-486 -> emqx_router.erl:124-138) and the mirror's batched events.
 * It never waits for a full build: while one runs in the background, the changes are patched
 * into the index the readers have now (a delta commit) and replayed onto the new index when it
 * is installed.  It waits only when the current tables cannot take the delta (a table at its
 * load bound while the rebuild that grows it runs; emqxgm_stats.bg_waits counts them).  Full
 * builds of registries of at least emqxgm_tune("bg_build") filters run in the background. */
int emqxgm_route_set_batch(emqxgm_t* h, const uint8_t* bytes, const uint64_t* offsets,
                           const uint8_t* present, uint64_t n, uint32_t flags, uint64_t* epoch);
/* A full resync (the mirror's start and its periodic anti-entropy pass): _begin starts generation
 * *gen; every emqxgm_route_set(.., 1) until _end marks its filter; _end(gen) sets every route key
 * that was not marked absent (*removed of them).  -ESTALE if another _begin came in between. */
int emqxgm_route_sync_begin(emqxgm_t* h, uint32_t* gen);
int emqxgm_route_sync_end(emqxgm_t* h, uint32_t gen, uint64_t* removed /* nullable */);
/* 1 if `filter` is a committed route key (emqx_router:has_routes/1 of the committed index), 0 if
 * not. */
int emqxgm_route_member(emqxgm_t* h, const uint8_t* filter, uint32_t len);
/* 1 if the committed trie holds no filter, 0 otherwise (emqx_trie:empty/0). */
int emqxgm_trie_empty(emqxgm_t* h);
/* 1 if the committed trie holds exactly this filter key (emqx_trie:lookup_topic/2,
 * emqx_trie.erl:267-271), 0 otherwise. */
int emqxgm_trie_member(emqxgm_t* h, const uint8_t* filter, uint32_t len);

int emqxgm_lookup_id(emqxgm_t* h, const uint8_t* filter, uint32_t len, uint32_t* id);
/* Pointer to filter id's bytes in the engine's registry: valid until the next call that adds a
 * filter string or commits (insert / route / subscriber calls may grow the registry, and a commit
 * reserves room for the deltas ahead).  Prefer the copies. */
int emqxgm_filter_bytes(emqxgm_t* h, uint32_t id, const uint8_t** p, uint32_t* len);
/* Copy of filter id's bytes into buf (cap bytes): *len = its length; -ENOSPC if cap < *len. */
int emqxgm_filter_copy(emqxgm_t* h, uint32_t id, uint8_t* buf, uint32_t cap, uint32_t* len);
/* The filters ids[0..n) packed into buf: filter i = buf[offsets[i] .. offsets[i+1]) (offsets has
 * n+1 entries).  -ENOSPC if cap is too small (offsets[n] = the bytes needed). */
int emqxgm_filters_copy(emqxgm_t* h, const uint32_t* ids, uint64_t n, uint8_t* buf, uint64_t cap,
                        uint64_t* offsets);

/* Match n topics: topic i = bytes[offsets[i] .. offsets[i+1]), offsets has n+1 entries. */
int emqxgm_match_batch(emqxgm_t* h, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                       emqxgm_out* out);
/* Same, with bytes/offsets already in HBM on the handle's device; results stay in HBM.
 * bytes_len = offsets[n] (passed so the engine never has to read it back).
 * The kernels read the batch in aligned 16-byte chunks: the chunks that hold its first and its
 * last byte are read whole, so up to 15 bytes in front of d_bytes and behind d_bytes + bytes_len
 * (never a chunk that holds no byte of the batch) must be readable device memory; their values
 * do not matter.  A batch anywhere inside an allocation whose start and size are multiples of
 * 16 bytes satisfies this.  The same holds for emqxgm_match_device_submit and
 * emqxgm_exact_owned_device (aligned 4-byte words there). */
int emqxgm_match_device(emqxgm_t* h, const uint8_t* d_bytes, const uint32_t* d_offsets,
                        uint32_t n, uint64_t bytes_len, emqxgm_dev_out* out);

/* Pipelined form of emqxgm_match_device for a stream of batches (the reference's publishers
 * call match_routes concurrently, emqx_broker.erl:231; a batcher in front of the NIF hands the
 * engine one batch after another).  _submit enqueues the whole pass for one batch and returns
 * at once with a ticket; _wait(ticket) completes it (redoing it synchronously in the rare case
 * of a staging overflow or deep walk) and returns the device-resident result.  Up to
 * EMQXGM_PIPES passes are in flight per handle, each on its own HIP stream and scratch, so one
 * batch's walk tail overlaps the next batch's tokenizer and walk.  Ticket k's result lives in
 * pipe k % EMQXGM_PIPES and stays valid until ticket k + EMQXGM_PIPES is submitted; submitting
 * it before ticket k was waited for returns -EBUSY.  The caller keeps d_bytes/d_offsets alive
 * until the wait.  A commit first completes every pass in flight (results stay retrievable).
 * Results are identical to emqxgm_match_device's. */
#ifndef EMQXGM_PIPES
#define EMQXGM_PIPES 2
#endif
/* EMQXGM_PIPES of the library's build (a caller compiled against another header asks). */
int emqxgm_device_pipes(void);

/* Pinned (page-locked) host memory on the handle's device, for the caller's topic staging: a
 * batcher that packs its window into it gets full-speed H2D copies from emqxgm_match_batch.
 * The size is rounded up to a multiple of 16 bytes.  NULL on failure.  emqxgm_host_free
 * releases it. */
void* emqxgm_host_alloc(emqxgm_t* h, uint64_t bytes);
void emqxgm_host_free(emqxgm_t* h, void* p);
int emqxgm_match_device_submit(emqxgm_t* h, const uint8_t* d_bytes, const uint32_t* d_offsets,
                               uint32_t n, uint64_t bytes_len, uint64_t* ticket);
int emqxgm_match_device_wait(emqxgm_t* h, uint64_t ticket, emqxgm_dev_out* out);

/* Pipelined host-in / host-out form of emqxgm_match_batch: the call a NIF batcher makes (the
 * reference's publishers call match_routes concurrently from every scheduler,
 * emqx_broker.erl:231).  _submit enqueues, on one of EMQXGM_HOST_PIPES streams, the copy of the
 * batch into HBM, the whole device pass and the copy of its result into pinned host memory, and
 * returns at once; _wait(ticket) completes it.  With several tickets in flight one batch's
 * upload, another's pass and a third's download overlap.  The batch: n <= cfg.batch_max topics,
 * topic i = bytes[offsets[i] .. offsets[i+1]), offsets[0] == 0 and non-decreasing (-EINVAL
 * otherwise, checked on the host before anything is enqueued); bytes and
 * offsets stay untouched until the wait (pinned memory from emqxgm_host_alloc gives full-speed
 * copies).  The result (batch-local u32 row pointers, trie filter ids, exact ids) lives in
 * pinned buffers of the pipe and stays valid until ticket + EMQXGM_HOST_PIPES is submitted;
 * submitting that ticket before this one was waited for returns -EBUSY.  When no topic of the
 * batch equals a route key, exact_id points at an all-EMQXGM_NONE buffer of the pipe (same
 * lifetime) and no exact id crossed PCIe.  Results are identical to emqxgm_match_batch's. */
#define EMQXGM_HOST_PIPES 3
typedef struct emqxgm_batch_out {
  uint32_t n;
  uint32_t n_pairs;
  const uint32_t* row_ptr;   /* [n+1] offsets into filter_id */
  const uint32_t* filter_id; /* [n_pairs] matched trie filter ids */
  const uint32_t* exact_id;  /* [n] route key equal to the topic, or EMQXGM_NONE */
} emqxgm_batch_out;
int emqxgm_match_batch_submit(emqxgm_t* h, const uint8_t* bytes, const uint32_t* offsets,
                              uint32_t n, uint64_t* ticket);
int emqxgm_match_batch_wait(emqxgm_t* h, uint64_t ticket, emqxgm_batch_out* out);
/* _wait, plus the bytes of every matched pair's filter, gathered on the device from its copy of
 * the string pool and copied into pinned buffers of the pipe (same lifetime as the result): pair
 * j's filter is fbytes[foff[j] .. foff[j+1]), foff has n_pairs + 1 entries.  What a NIF needs to
 * build each caller's filter binaries without touching the host registry per pair. */
int emqxgm_match_batch_wait_filters(emqxgm_t* h, uint64_t ticket, emqxgm_batch_out* out,
                                    const uint32_t** foff, const uint8_t** fbytes);
/* _submit for a ticket that will be completed with _wait_filters: the filter-byte gather and the
 * copies of every result array (filter ids, byte offsets, bytes, exact ids) are enqueued behind
 * the pass -- packed on the device into one block that one copy brings into pinned memory --
 * sized by the pairs and bytes per topic of the pipe's recent windows (x1.2), so that
 * _wait_filters takes one stream synchronisation instead of four; a window beyond those sizes is
 * finished there synchronously.  Same arguments, errors and results as _submit + _wait_filters
 * (the NIF batcher core submits its windows this way).  A window of at most "zc_topics" topics
 * (emqxgm_tune; 65536 default) and 8 MiB whose bytes and offsets are pinned memory
 * (emqxgm_host_alloc) goes without DMA copies: the tokenizer reads it over PCIe and the result
 * block is written straight into the pipe's pinned buffer (r04: 16k-topic windows 150 -> 114 us
 * one at a time).  Either way bytes / offsets stay untouched until the wait.  Such a window
 * (bytes 16-byte aligned, or it takes the copies) is read in whole 16-byte chunks, up to 15 bytes
 * past bytes + offsets[n]: those bytes must be part of the pinned buffer.  emqxgm_host_alloc
 * rounds its size up to a multiple of 16, so a window that fills its buffer satisfies this. */
int emqxgm_match_batch_submit_filters(emqxgm_t* h, const uint8_t* bytes, const uint32_t* offsets,
                                      uint32_t n, uint64_t* ticket);

/* ---- publish fan-out (emqx_broker.erl:218-355) -------------------------------------------
 * Routes with dest identity: a plain route {Filter, Node} passes group = EMQXGM_NONE; a shared-
 * subscription route {Filter, {Group, Node}} passes both (handles < 2^31, chosen by the caller).
 * Like emqx_router:do_add_route/do_delete_route, the first route of a wildcard filter inserts it
 * into the trie and its last one removes it, the route key exists while the filter has a route
 * (the same refcount as emqxgm_route_ref), and adding an existing route or deleting an absent
 * one is a no-op.  Visible after emqxgm_commit, like every mutation. */
int emqxgm_route_add(emqxgm_t* h, const uint8_t* filter, uint32_t len, uint32_t node,
                     uint32_t group);
int emqxgm_route_delete(emqxgm_t* h, const uint8_t* filter, uint32_t len, uint32_t node,
                        uint32_t group);
/* node() of this broker: aggre entries {To, local_node} are dispatched to local subscribers. */
int emqxgm_set_local_node(emqxgm_t* h, uint32_t node);
/* The local subscriber bag (filter -> subscriber handle); duplicates / absent deletes: no-op. */
int emqxgm_subscriber_add(emqxgm_t* h, const uint8_t* filter, uint32_t len, uint32_t sub);
int emqxgm_subscriber_delete(emqxgm_t* h, const uint8_t* filter, uint32_t len, uint32_t sub);
/* Level-triggered forms for a mirror of the committed tables (the NIF's sync process and the
 * writing node's hook, r05): filter i = bytes[offsets[i] .. offsets[i+1]) gets exactly the dests
 * (node[j], group[j]) for j in [dptr[i], dptr[i+1]) -- its rows of the emqx_route bag,
 * emqx_router.erl:72-92: group = EMQXGM_NONE for a node dest, else the {Group, Node} dest --
 * and its route key / wildcard trie membership while it has any (emqxgm_route_set's rule);
 * or exactly the local subscribers subs[sptr[i] .. sptr[i+1]) (the emqx_subscriber bag,
 * emqx_broker.erl:150-214, 546-552).  Duplicates are ignored.  flags EMQXGM_SET_COMMIT: visible
 * before the call returns, as emqxgm_route_set_batch. */
int emqxgm_route_dests_batch(emqxgm_t* h, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                             const uint32_t* dptr, const uint32_t* node, const uint32_t* group,
                             uint32_t flags, uint64_t* epoch);
int emqxgm_subscribers_batch(emqxgm_t* h, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                             const uint32_t* sptr, const uint32_t* subs, uint32_t flags,
                             uint64_t* epoch);

typedef struct emqxgm_publish_out { /* host-resident result of emqxgm_publish_batch */
  uint32_t n;
  uint64_t n_routes;              /* aggre entries of the whole batch */
  uint64_t n_deliveries;          /* local dispatches of the whole batch */
  const uint64_t* route_ptr;      /* [n+1] topic i's entries: [route_ptr[i], route_ptr[i+1]) */
  const uint32_t* route_filter;   /* To of each entry (filter id) */
  const uint32_t* route_dest;     /* node handle, or EMQXGM_DEST_GROUP | group handle */
  const uint64_t* deliver_ptr;    /* [n+1] topic i's local dispatches */
  const uint32_t* deliver_filter; /* the filter (To) a dispatch goes through */
  const uint32_t* deliver_sub;    /* the subscriber it reaches */
} emqxgm_publish_out;

/* emqx_broker:publish/1 for a batch of topics: the aggre/1 entries of match_routes(Topic)
 * (node dests as {To, Node}, shared dests as {To, Group} with each group once per filter) and
 * the local dispatches of the entries {To, local_node} (every subscriber of To).  Entries of a
 * topic come in match_routes order (exact key first, then the trie row); callers treat them as
 * the set the reference's route/2 folds over. */
int emqxgm_publish_batch(emqxgm_t* h, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                         emqxgm_publish_out* out);

/* First rule matching each name, for the scalar emqx_topic:match/2 loops outside the router:
 * emqx_authz_rule:match_topics/3 (apps/emqx_authz/src/emqx_authz_rule.erl:201-214: rules in
 * order, {eq, F} by equality, others by match/2 on word lists -> EMQXGM_RULE_WORDS) and
 * emqx_rewrite:match_and_rewrite/3 (apps/emqx_modules/src/emqx_rewrite.erl:145-150: match/2 on
 * binaries, flags 0).  names / rules: packed bytes + [n+1] / [n_rules+1] offsets on the host;
 * out[i] = index of the first matching rule, or EMQXGM_NONE.  Independent of the index. */
int emqxgm_match_rules(emqxgm_t* h, const uint8_t* name_bytes, const uint32_t* name_offsets,
                       uint32_t n, const uint8_t* rule_bytes, const uint32_t* rule_offsets,
                       const uint32_t* rule_flags, uint32_t n_rules, uint32_t* out);

/* ---- retained-message store: reverse match (filter -> stored topics) ----
 * The retainer's mnesia backend (apps/emqx_retainer/src/emqx_retainer_mnesia.erl) on the
 * device: topics of retained messages (the messages stay with the caller) with their expiry
 * times, and match_messages/3 (:185-195) for batches of subscription filters.  The selected set
 * is search_table/3's (:300-330): with index specs configured (emqxgm_retain_set_indices; the
 * default is the reference's ?DEFAULT_INDICES [[1,2,3],[1,3],[2,3],[3]],
 * emqx_retainer_schema.erl:24-29) the index path of the best-scoring index (select_index/2 and
 * condition/2, emqx_retainer_index.erl:83-91, 141-200), including its open index tail (a/+
 * also selects a/x/y under [1,2,3]); with none, or when no index scores, the full scan of
 * condition/1 (:97-112: '+' any word, a last '#' any tail).  No '$' rule; expiry 0 or > now.
 * Mutations are visible after emqxgm_retain_commit. */
typedef struct emqxgm_retain emqxgm_retain_t;
int emqxgm_retain_create(int32_t device, emqxgm_retain_t** out);
void emqxgm_retain_destroy(emqxgm_retain_t* r);
/* store_retained/2 (:138-152): insert or overwrite; expiry_ms 0 = never; *id = stable id */
int emqxgm_retain_store(emqxgm_retain_t* r, const uint8_t* topic, uint32_t len,
                        uint64_t expiry_ms, uint32_t* id);
/* delete_message/2 of one topic (:166-170, delete_message_by_topic/2 :345-349); absent: no-op */
int emqxgm_retain_delete(emqxgm_retain_t* r, const uint8_t* topic, uint32_t len);
int emqxgm_retain_clean(emqxgm_retain_t* r); /* clean/1 (:241-244) */
int emqxgm_retain_commit(emqxgm_retain_t* r);
/* Committed state = a base store plus a small delta store of the topics stored since the base
 * was built; re-storing or deleting a base topic patches it in place.  "delta_max": delta topics
 * before a commit rebuilds the base (-1 = max(4096, base / 16), 0 = rebuild at every commit).
 * "max_retained_messages": the table-full limit of emqxgm_retain_store_ts (0 = none).
 * "timing": see emqxgm_retain_timing. */
int emqxgm_retain_tune(emqxgm_retain_t* r, const char* key, int64_t value);
/* The retainer's index specs (retainer.backend.index_specs, config_indices/0 of
 * emqx_retainer_mnesia.erl:424-425): spec i = positions pos[offsets[i] .. offsets[i+1]), each
 * >= 1 and strictly ascending; n = 0 selects the full scan only (index_specs = []).  -EINVAL on a
 * malformed spec (then the specs are unchanged).  Applies to the next emqxgm_retain_match. */
int emqxgm_retain_set_indices(emqxgm_retain_t* r, const uint32_t* pos, const uint32_t* offsets,
                              uint32_t n);
/* out = {full rebuilds, delta commits, base topics (incl. deleted), delta topics} */
int emqxgm_retain_stats(emqxgm_retain_t* r, uint64_t out[4]);
/* size/1 (:246-247): committed topics */
int emqxgm_retain_size(emqxgm_retain_t* r, uint64_t* n);
/* read_message/2 (:182-183, read_messages/1 :372-382: expiry 0 or >= now), committed state:
 * 1 and *id if the topic is stored and live, 0 if not */
int emqxgm_retain_read(emqxgm_retain_t* r, const uint8_t* topic, uint32_t len, uint64_t now_ms,
                       uint32_t* id);
int emqxgm_retain_topic(emqxgm_retain_t* r, uint32_t id, const uint8_t** p, uint32_t* len);
typedef struct emqxgm_retain_out { /* host-resident, valid until the next call on r */
  uint32_t n;
  uint64_t n_ids;
  const uint64_t* ptr; /* [n+1]: filter i selects id[ptr[i] .. ptr[i+1]) */
  const uint32_t* id;  /* topic ids: a filter's base-store topics, then its delta-store topics,
                          each ascending in topic word order */
} emqxgm_retain_out;
/* match_messages/3 for a batch of filters (packed bytes + [n+1] offsets on the host) */
int emqxgm_retain_match(emqxgm_retain_t* r, const uint8_t* bytes, const uint32_t* offsets,
                        uint32_t n, uint64_t now_ms, emqxgm_retain_out* out);

/* match_messages/3 with {Cursor, BatchNum} (:185-202, qlc_next_answers/2 :384-397): the
 * dispatcher's flow control (emqx_retainer_dispatcher.erl:242-257) reads batch_read_number
 * messages at a time.  A filter's ids come in emqxgm_retain_match's order (base topics in word
 * order, then delta topics in word order); a call returns, per filter, the first limit[i] live
 * ids at or after cur[i] (limit 0: all of them) and advances cur[i].  Only the windows are
 * computed into the output and downloaded.
 *  * A zeroed cursor starts.  phase becomes DONE when nothing live remains after the window at
 *    this call -- one call earlier than qlc_next_answers/2 reports `closed` when exactly N
 *    answers remain (it then needs one more, empty, read); the rows delivered are the same.
 *    An entry that comes in DONE or STALE yields an empty row and stays as it is.
 *  * A cursor belongs to one base generation (gen = full rebuilds at its first call): base
 *    positions are stable while the base is only patched.  After a full rebuild or a clean the
 *    entry comes back STALE with an empty row and the caller restarts that filter; the other
 *    entries proceed and the call returns 0.  A delta cursor resumes by bytes: after the topic
 *    `at` in the current delta store's word order, whether or not it is still stored.
 *  * While no full rebuild intervenes, a topic that is selected and untouched from the first
 *    page to the last is returned exactly once; no topic is returned twice; a topic stored
 *    meanwhile may or may not be seen -- what a qlc cursor over a fixed ets table gives.
 *  * -EINVAL, before anything is launched: an unknown phase, a BASE cursor with `at` past the
 *    base store's size, a DELTA cursor whose `at` is no topic id.  -E2BIG: the windows together
 *    hold 2^32 ids or more, or (ranks are 32-bit) so many live ids remain after the cursors. */
enum { EMQXGM_RC_START = 0, EMQXGM_RC_BASE = 1, EMQXGM_RC_DELTA = 2, EMQXGM_RC_DONE = 3,
       EMQXGM_RC_STALE = 4 };
typedef struct emqxgm_retain_cursor {
  uint64_t gen;   /* base generation the cursor belongs to */
  uint32_t phase; /* EMQXGM_RC_* */
  uint32_t at;    /* BASE: next sorted position of the base store;
                     DELTA: id of the last delta topic returned */
} emqxgm_retain_cursor;
int emqxgm_retain_match_limit(emqxgm_retain_t* r, const uint8_t* bytes, const uint32_t* offsets,
                              uint32_t n, uint64_t now_ms, const uint32_t* limit /* [n], 0 = all */,
                              emqxgm_retain_cursor* cur /* [n], in/out, zeroed = start */,
                              emqxgm_retain_out* out);
/* With emqxgm_retain_tune "timing" = 1: HIP-event times in ms of the last
 * emqxgm_retain_match_limit's own launches -- {count pass of k_retain_runs_win, the scans and
 * k_retain_win between the passes (two host round trips included), fill pass}. */
int emqxgm_retain_timing(emqxgm_retain_t* r, double out[3]);
/* store_retained/2 with #message.timestamp (kept in the host registry, for page_read);
 * emqxgm_retain_store is this call with ts_ms = 0.  With emqxgm_retain_tune
 * "max_retained_messages" = L > 0 (is_table_full/0 and is_new_topic/1, :141, :409-419): a topic
 * that is not stored, while L or more are (expired but uncleared ones count, table_size/0),
 * returns -ENOSPC and changes nothing; storing a stored topic again always succeeds.  0: no limit. */
int emqxgm_retain_store_ts(emqxgm_retain_t* r, const uint8_t* topic, uint32_t len,
                           uint64_t expiry_ms, uint64_t ts_ms, uint32_t* id);
/* clear_expired/1 (:154-164): deletes every stored topic with expiry != 0 and expiry < now_ms
 * (strictly, :161; the match keeps > now, the read >= now), commits, and returns their ids
 * (valid until the next call on r): the caller deletes those messages from its own table. */
int emqxgm_retain_clear_expired(emqxgm_retain_t* r, uint64_t now_ms, const uint32_t** ids,
                                uint64_t* n);
/* delete_message/2 (:166-180): commits pending changes; a wildcard filter deletes every topic
 * search_table(Tokens, 0) selects (:172), any other the topic itself; commits; returns the ids
 * deleted (valid until the next call on r). */
int emqxgm_retain_delete_matching(emqxgm_retain_t* r, const uint8_t* filter, uint32_t len,
                                  const uint32_t** ids, uint64_t* n);
/* page_read/4 (:204-238), the dashboard listing: commits; filter NULL = '#' on the full scan
 * (search_table(undefined, ['#'], Now), :209), else the filter through the configured indices;
 * the selected ids in a stable sort by timestamp (compare_message/2, :364-365), entries
 * [(page-1)*limit, page*limit) of them.  page = 0 or limit = 0: -EINVAL.  Host sort. */
int emqxgm_retain_page_read(emqxgm_retain_t* r, const uint8_t* filter, uint32_t len, uint64_t page,
                            uint64_t limit, uint64_t now_ms, const uint32_t** ids, uint64_t* n);

/* ---- rule sets: every matching rule per name, against a resident list ----
 * The loops that keep every match, run once per publish beside the route match:
 * emqx_rule_engine:get_rules_for_topic/1 (apps/emqx_rule_engine/src/emqx_rule_engine.erl:198-204;
 * a rule matches when any of its `from` filters does, emqx_plugin_libs_rule.erl:340-346),
 * emqx_bridge:get_matched_egress_bridges/1 (emqx_bridge.erl:342-382), and the exhook and trace
 * topic filters (emqx_exhook_server.erl:361, emqx_trace_handler.erl:138: one filter per rule).
 * The list is compiled once at emqxgm_ruleset_set and stays on the device; a match tokenises
 * each name once and confirms on the bytes whatever rests on a hashed word.  word_hash_bits is
 * the test knob of emqxgm_cfg.word_hash_bits (0 = production).  Limits: 65,536 rules and 2^20
 * filters per list. */
typedef struct emqxgm_ruleset emqxgm_ruleset_t;
int emqxgm_ruleset_create(int32_t device, uint32_t word_hash_bits, emqxgm_ruleset_t** out);
void emqxgm_ruleset_destroy(emqxgm_ruleset_t* r);
/* Replaces the whole list.  Filter i = filter_bytes[filter_offsets[i] .. filter_offsets[i+1])
 * with flags 0 (match/2 on binaries) | EMQXGM_RULE_WORDS | EMQXGM_RULE_EQ, belonging to rule
 * filter_rule[i]; the filters of one rule are adjacent: filter_rule is non-decreasing and
 * < n_rules.  A rule may have no filter.  -EINVAL beyond the limits or on malformed offsets,
 * flags or rule order; the previous list then stays in force. */
int emqxgm_ruleset_set(emqxgm_ruleset_t* r, const uint8_t* filter_bytes,
                       const uint32_t* filter_offsets, const uint32_t* filter_flags,
                       const uint32_t* filter_rule, uint32_t n_filters, uint32_t n_rules);
typedef struct emqxgm_ruleset_out { /* host-resident, valid until the next call on r */
  uint32_t n;
  uint64_t n_ids;
  const uint64_t* ptr;  /* [n+1] */
  const uint32_t* rule; /* name i matches rule[ptr[i] .. ptr[i+1]), ascending, each once */
} emqxgm_ruleset_out;
/* names: packed bytes + [n+1] offsets on the host.  -EIO if the device reports a row that the
 * count and the fill pass disagree on. */
int emqxgm_ruleset_match(emqxgm_ruleset_t* r, const uint8_t* bytes, const uint32_t* offsets,
                         uint32_t n, emqxgm_ruleset_out* out);
/* "pass_names": names per device pass (default 1 Mi; never more than (2^32 - 1) / n_rules, so a
 * pass's 32-bit row pointers cannot overflow); "counters": 1 = the count pass keeps the four
 * counters of emqxgm_ruleset_stats; "timing": 1 = HIP events around the count and the fill
 * kernel of every pass (tools/ruleset_bench.py), setting it clears the sums, which the read-only
 * keys "count_us" / "fill_us" return in microseconds (>= 0, the value is ignored) */
int emqxgm_ruleset_tune(emqxgm_ruleset_t* r, const char* key, int64_t value);
/* out = {records, record tiles, filters, rules, candidates sent to the byte check, candidates it
 * removed, names deeper than 16 levels, records visited}; the last four since the last set */
int emqxgm_ruleset_stats(emqxgm_ruleset_t* r, uint64_t out[8]);

/* ---- ACL lists: the first matching authz rule per request, against a resident list ----
 * emqx_authz_rule:matches/4 (apps/emqx_authz/src/emqx_authz_rule.erl:125-133): an ordered list of
 * {Permission, Who, Action, TopicFilters}; the first rule whose action (match_action/2, :147-150),
 * principal (match_who/2, :152-200) and any topic filter (match_topics/3, :202-210) match decides.
 * It is emqx_authz_file:authorize/4 (emqx_authz_file.erl:64-65) and, with one rule per record
 * entry, emqx_authz_mnesia:authorize/4 (emqx_authz_mnesia.erl:98-120, 222-229).  Filters are
 * {eq, F} (word-list equality, compile_topic/1 :98-101) or match by emqx_topic:match/2 on word
 * lists (:212-215; EMQXGM_RULE_WORDS semantics); a filter with a word that is exactly
 * ${clientid} or ${username} is a pattern (pattern/1, :109-110) and gets the request's client fed
 * in on the device (feed_var/2, :217-230): the value is one binary word, so an empty value, "+",
 * "#" or a value with a '/' equals no name word, and an undefined value leaves the placeholder a
 * literal word.  The device decides the principals all, {username, {eq, U}} and
 * {clientid, {eq, C}} (byte equality; an undefined value never matches); every other principal
 * (regexes, ipaddr, ipaddrs, 'and', 'or') is one of 64 host slots that the caller evaluates once
 * per client.  No answer rests on a hash.  Limits: 65,536 rules and 2^20 filters per list. */
#define EMQXGM_ACL_DENY 0u
#define EMQXGM_ACL_ALLOW 1u
#define EMQXGM_ACL_PUBLISH 1u   /* action of a rule or a request */
#define EMQXGM_ACL_SUBSCRIBE 2u
#define EMQXGM_ACL_ALL 3u       /* action of a rule only */
#define EMQXGM_ACL_WHO_ALL 0u
#define EMQXGM_ACL_WHO_USERNAME 1u /* {username, {eq, who string}} */
#define EMQXGM_ACL_WHO_CLIENTID 2u /* {clientid, {eq, who string}} */
#define EMQXGM_ACL_WHO_HOST 3u     /* host slot rule_slot[r] < 64 */
#define EMQXGM_ACL_NO_CLIENTID 1u  /* client flag: clientid => undefined */
#define EMQXGM_ACL_NO_USERNAME 2u  /* client flag: username => undefined */
typedef struct emqxgm_acl emqxgm_acl_t;
int emqxgm_acl_create(int32_t device, uint32_t word_hash_bits, emqxgm_acl_t** out);
void emqxgm_acl_destroy(emqxgm_acl_t* a);
/* Replaces the whole list (compile/1, :61-71).  Filter i = filter_bytes[filter_offsets[i] ..
 * filter_offsets[i+1]) with flag EMQXGM_RULE_EQ or 0, belonging to rule filter_rule[i]
 * (non-decreasing, < n_rules; a rule with no filter never matches, :202-203).  Rule r has
 * rule_perm[r] (EMQXGM_ACL_DENY | ALLOW), rule_action[r] (PUBLISH | SUBSCRIBE | ALL),
 * rule_who[r] (EMQXGM_ACL_WHO_*), rule_slot[r] (< 64; read for WHO_HOST) and the who string
 * who_bytes[who_offsets[r] .. who_offsets[r+1]) (read for WHO_USERNAME and WHO_CLIENTID).
 * -EINVAL beyond the limits or on malformed offsets, flags, rule order, kinds or a slot of 64
 * or more; the previous list then stays in force. */
int emqxgm_acl_set(emqxgm_acl_t* a, const uint8_t* filter_bytes, const uint32_t* filter_offsets,
                   const uint32_t* filter_flags, const uint32_t* filter_rule, uint32_t n_filters,
                   const uint32_t* rule_perm, const uint32_t* rule_action, const uint32_t* rule_who,
                   const uint32_t* rule_slot, const uint8_t* who_bytes, const uint32_t* who_offsets,
                   uint32_t n_rules);
/* matches/4 for a batch of requests: name i = bytes[offsets[i] .. offsets[i+1]) (a topic, or the
 * filter of a subscribe, taken as words), client[i] an index into the call's client table,
 * action[i] = EMQXGM_ACL_PUBLISH | SUBSCRIBE.  The client table: client ids and usernames as
 * packed bytes + [n_clients+1] offsets, client_flags[c] (EMQXGM_ACL_NO_*: the value is undefined
 * and its bytes are ignored), who_bits[c] (bit k set: client c satisfies host slot k).
 * out_rule[i] = the first matching rule or EMQXGM_NONE.  -EINVAL, before anything is launched,
 * on a client index out of range or an action other than publish or subscribe. */
int emqxgm_acl_match(emqxgm_acl_t* a, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                     const uint32_t* client, const uint32_t* action, const uint8_t* clientid_bytes,
                     const uint32_t* clientid_offsets, const uint8_t* username_bytes,
                     const uint32_t* username_offsets, const uint32_t* client_flags,
                     const uint64_t* who_bits, uint32_t n_clients, uint32_t* out_rule);
/* "pass_names": requests per device pass (default 1 Mi); "counters": 1 = keep the four counters
 * of emqxgm_acl_stats; "timing": 1 = HIP events around the kernel of every pass
 * (tools/acl_bench.py), setting it clears the sum, which the read-only key "kernel_us" returns in
 * microseconds (>= 0, the value is ignored) */
int emqxgm_acl_tune(emqxgm_acl_t* a, const char* key, int64_t value);
/* out = {filter records, record tiles, filters, rules, candidates sent to a byte check,
 * candidates it removed, names deeper than 16 levels, records visited}; the last four since the
 * last set */
int emqxgm_acl_stats(emqxgm_acl_t* a, uint64_t out[8]);

/* ---- the built-in authorization database, resident on the device -------------
 * emqx_authz_mnesia (apps/emqx_authz/src/emqx_authz_mnesia.erl): one record per principal, keyed
 * {clientid, C}, {username, U} or all (:41-58), each an ordered list of
 * {Permission, Action, TopicFilter}.  authorize/4 (:98-120) reads the record of the request's
 * client id, the one of its username and the all record, and the first rule of
 * clientid ++ username ++ all that matches decides (do_authorize/4, :222-229, each rule compiled
 * as {Permission, all, Action, [TopicFilter]} by emqx_authz_rule:compile/1).  Keys are compared by
 * byte equality over any bytes (the empty key included); the same bytes as a client id and as a
 * username are two keys.  An undefined client id or username skips that read.  A filter that
 * begins with "eq " is {eq, F} (compile_topic/1, emqx_authz_rule.erl:98-99); the placeholder feed
 * and the topic match are those of the ACL lists above.  No answer rests on a hash.  A request
 * costs its client's own rules plus the all rules, whatever the number of keys.  Limits: 65,536
 * rules per record; the database as a whole has none below 2^32 pool words, filters and keys.
 * Mutations (store, delete, purge) are pending until emqxgm_acldb_commit and invisible before. */
#define EMQXGM_ACLDB_CLIENTID 0u /* key kind; also the source of an answer */
#define EMQXGM_ACLDB_USERNAME 1u
#define EMQXGM_ACLDB_ALL 2u
typedef struct emqxgm_acldb emqxgm_acldb_t;
int emqxgm_acldb_create(int32_t device, uint32_t word_hash_bits, emqxgm_acldb_t** out);
void emqxgm_acldb_destroy(emqxgm_acldb_t* db);
/* store_rules/2 (:132-150): replaces the record of (kind, key) by n_rules rules, rule k =
 * {perm[k] (EMQXGM_ACL_DENY | ALLOW), action[k] (PUBLISH | SUBSCRIBE | ALL), filter
 * filter_bytes[filter_offsets[k] .. filter_offsets[k+1])}.  The key is ignored for
 * EMQXGM_ACLDB_ALL.  A record with no rules answers like an absent one and counts in
 * emqxgm_acldb_count.  -EINVAL on a bad kind, permission, action or offsets or more than 65,536
 * rules; nothing is then pending from the call. */
int emqxgm_acldb_store(emqxgm_acldb_t* db, uint32_t kind, const uint8_t* key, uint32_t klen,
                       const uint32_t* perm, const uint32_t* action, const uint8_t* filter_bytes,
                       const uint32_t* filter_offsets, uint32_t n_rules);
/* The same for n_records records at once, in order: record i has kind[i], the key
 * key_bytes[key_offsets[i] .. key_offsets[i+1]) and the rules rule_offsets[i] ..
 * rule_offsets[i+1] of perm / action / filter_offsets.  All or nothing. */
int emqxgm_acldb_store_many(emqxgm_acldb_t* db, uint32_t n_records, const uint32_t* kind,
                            const uint8_t* key_bytes, const uint32_t* key_offsets,
                            const uint32_t* rule_offsets, const uint32_t* perm, const uint32_t* action,
                            const uint8_t* filter_bytes, const uint32_t* filter_offsets);
/* delete_rules/1 (:152-164); deleting an absent key is a no-op. */
int emqxgm_acldb_delete(emqxgm_acldb_t* db, uint32_t kind, const uint8_t* key, uint32_t klen);
/* purge_rules/0 (:166-169): drops every record and everything pending before the call. */
int emqxgm_acldb_purge(emqxgm_acldb_t* db);
/* Makes the pending mutations visible.  New and replaced runs are appended to the device pools
 * and their table slots patched; a full rebuild (compaction and rehash) runs when a key table
 * would pass the load "rebuild_load_pct" or the garbage words pass "rebuild_garbage_pct" percent
 * of the live ones (the words of the all stream count like pool words).  After a commit that
 * failed with -EIO the handle answers -EIO to every commit and match: destroy it. */
int emqxgm_acldb_commit(emqxgm_acldb_t* db);
/* record_count/0 (:171-173): committed records as they will be after the pending mutations. */
int emqxgm_acldb_count(emqxgm_acldb_t* db, uint64_t* out);
/* authorize/4 for a batch: requests and the client table as in emqxgm_acl_match (without
 * who_bits).  Per request: out_perm = EMQXGM_ACL_DENY | ALLOW or EMQXGM_NONE for nomatch, out_src
 * = EMQXGM_ACLDB_* of the deciding record, out_pos = the deciding rule's position in it (both
 * EMQXGM_NONE for nomatch).  -EINVAL, before anything is launched, on a client index out of range
 * or an action other than publish or subscribe; -EIO when a lane found a malformed run. */
int emqxgm_acldb_match(emqxgm_acldb_t* db, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                       const uint32_t* client, const uint32_t* action, const uint8_t* clientid_bytes,
                       const uint32_t* clientid_offsets, const uint8_t* username_bytes,
                       const uint32_t* username_offsets, const uint32_t* client_flags,
                       uint32_t n_clients, uint32_t* out_perm, uint32_t* out_src, uint32_t* out_pos);
/* "pass_names", "counters", "timing" and the read-only "kernel_us" as emqxgm_acl_tune;
 * "rebuild_load_pct" (1..50, default 50: a table's used slots, deleted ones included, in percent
 * of its slots) and "rebuild_garbage_pct" (>= 1, default 100) */
int emqxgm_acldb_tune(emqxgm_acldb_t* db, const char* key, int64_t value);
/* out = {client-id records, slots, deleted slots, username records, slots, deleted slots, the
 * longest probe chain of a stored key, rules of the all record, live words (pool and all
 * stream), garbage words, full rebuilds, pool growths, key hits sent to the byte check, key hits it removed,
 * filter candidates sent to the byte check, candidates it removed, names deeper than 16 levels,
 * tiles of the all record, 0, 0}; the five counters since "counters" was last set */
int emqxgm_acldb_stats(emqxgm_acldb_t* db, uint64_t out[20]);

/* ---- shared subscriptions: which member of a group gets a message -------------
 * emqx_shared_sub (apps/emqx/src/emqx_shared_sub.erl): a bag of {Group, Topic, SubPid} (:104-117);
 * subscribers/2 (:391-392) gives a key's members in subscribe order and pick/6 (:309-379) applies
 * the group's strategy (strategy/1, :159-164).  This handle answers the first dispatch
 * (dispatch/3, FailedSubs = #{}) of a batch of {To, Group} entries of emqx_broker:publish/1
 * (emqx_broker.erl:270-275, EMQXGM_DEST_GROUP | group in emqxgm_publish_batch's answers).  Groups
 * and members are handles below 2^31 that the caller assigns.  Keys (group, topic) are compared by
 * byte equality over any bytes: the empty topic, "+", "#" and "a/#" are keys like any other.  No
 * answer rests on a hash.  Redispatch after a nack (dispatch/4 with FailedSubs) and the ack
 * protocol stay with the caller.  Mutations (subscribe, unsubscribe, subscriber_down,
 * set_strategy) are pending, in call order, until emqxgm_share_commit and invisible before. */
#define EMQXGM_SHARE_RANDOM 0u /* strategy/0 (:78-85) */
#define EMQXGM_SHARE_ROUND_ROBIN 1u /* the default of a new handle, as emqx_schema's */
#define EMQXGM_SHARE_ROUND_ROBIN_PER_GROUP 2u
#define EMQXGM_SHARE_STICKY 3u
#define EMQXGM_SHARE_LOCAL 4u
#define EMQXGM_SHARE_HASH_CLIENTID 5u
#define EMQXGM_SHARE_HASH_TOPIC 6u
#define EMQXGM_SHARE_PICKED 0u /* status of an answer */
#define EMQXGM_SHARE_NO_SUBSCRIBERS 1u
#define EMQXGM_SHARE_HOST_STRATEGY 2u /* sticky: the caller decides, from emqxgm_share_members */
#define EMQXGM_SHARE_LOCAL_MEMBER 0x80000000u /* emqxgm_share_members: bit of a local member */
typedef struct emqxgm_share emqxgm_share_t;
/* hash_bits 0 is production; 1..16 keeps that many bits of a key's tag (collision tests). */
int emqxgm_share_create(int32_t device, uint32_t hash_bits, emqxgm_share_t** out);
void emqxgm_share_destroy(emqxgm_share_t* s);
/* subscribe/3 (:416-425): appends sub to the members of (group, topic); a triple already present
 * keeps its position.  Either way a group whose strategy is round_robin_per_group at that moment
 * has the key's counter set to 0 (maybe_insert_round_robin_count/1, :484-487).  local: whether
 * the member is on this node (erlang:node(Pid) =:= node(), :349).  -EINVAL on a handle >= 2^31 or
 * a triple subscribed (committed or pending) with the other local flag. */
int emqxgm_share_subscribe(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len,
                           uint32_t sub, uint32_t local);
/* unsubscribe/3 (:426-431): removes the triple; a later subscribe appends at the end.  A key whose
 * last member leaves is absent, and its counter is deleted if the group's strategy is
 * round_robin_per_group at that moment (maybe_delete_round_robin_count/1, :489-494). */
int emqxgm_share_unsubscribe(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len,
                             uint32_t sub);
/* cleanup_down/1 (:509-519): removes sub from every key. */
int emqxgm_share_subscriber_down(emqxgm_share_t* s, uint32_t sub);
/* strategy/1 (:159-164): the strategy of a group, or with group = EMQXGM_NONE the default for
 * groups that have none set.  -EINVAL on a strategy code out of range. */
int emqxgm_share_set_strategy(emqxgm_share_t* s, uint32_t group, uint32_t strategy);
/* Makes the pending mutations visible.  Rewritten member runs and new keys are appended to the
 * device pools and their table slots patched; a full rebuild (compaction and rehash) runs when the
 * key table would pass the load "rebuild_load_pct" or the garbage words pass "rebuild_garbage_pct"
 * percent of the live ones.  After a commit that failed with -EIO the handle answers -EIO to every
 * later call: destroy it. */
int emqxgm_share_commit(emqxgm_share_t* s);
/* pick/6 for n requests: request i is on the key (groups[i], key_bytes[key_offsets[i] ..
 * key_offsets[i+1])) with hc[i] = erlang:phash2(ClientId), ht[i] = erlang:phash2(SourceTopic),
 * draw[i] = 32 random bits (the member is 1 + draw rem Count where the reference calls
 * rand:uniform(Count)) and state[i] = the publisher's round_robin state for the key
 * (erlang:get({shared_sub_round_robin, Group, Topic}), :367) or EMQXGM_NONE for undefined.
 * out[4i..4i+3] = {member handle or EMQXGM_NONE, EMQXGM_SHARE_* status, round_robin state to
 * store (state[i] unchanged unless round_robin ran over two or more members), Count = the key's
 * members}.  A key of one member answers that member before any strategy (:346-347).
 * round_robin_per_group requests of one call on one key take consecutive counter values in
 * request order (:373-379).  -EINVAL, before anything is launched, on non-monotone offsets or a
 * group >= 2^31; -EIO when a lane found a malformed table or run. */
int emqxgm_share_pick(emqxgm_share_t* s, uint32_t n, const uint32_t* groups, const uint8_t* key_bytes,
                      const uint32_t* key_offsets, const uint32_t* hc, const uint32_t* ht,
                      const uint32_t* draw, const uint32_t* state, uint32_t* out);
/* emqx_broker:publish/1 through route/2 for a batch of topics (emqx_broker.erl:262-282): what
 * emqxgm_publish_batch answers, and for every aggre/1 entry of it the member that
 * emqx_shared_sub:dispatch/3 sends a {To, Group} entry to (emqx_shared_sub.erl:138-157, 309-379),
 * picked in the same device pass against the index epoch the match and the fan-out read.  The key
 * of entry j is (route_dest[j] without EMQXGM_DEST_GROUP, the bytes of filter route_filter[j]).
 * hc[i], ht[i] and draw[i] are topic i's, as emqxgm_share_pick's.  The publisher's round_robin
 * states of topic i (its process dictionary, :365-372, passed whole) are the triples
 * [st_ptr[i], st_ptr[i+1]) of (st_group, st_filter, st_value): group handle, filter id of To,
 * state; the first pair that matches an entry is its state in, no match is undefined; st_ptr NULL:
 * every state is undefined.  out->pub is exactly emqxgm_publish_batch's answer; out->share holds
 * four words per entry, in the entries' order, with emqxgm_share_pick's meaning, and
 * {EMQXGM_NONE, EMQXGM_SHARE_NOT_SHARED, EMQXGM_NONE, 0} for an entry whose dest is a node.  It
 * stays valid until the next call with s.  round_robin_per_group entries of one call on one key
 * take consecutive counter values in entry order (topic order, then the entries of a topic).
 * -EINVAL, before anything is launched, on a null handle or per-topic array, handles on different
 * devices, non-monotone offsets or st_ptr, or a st_group >= 2^31; -ESTALE as emqxgm_publish_batch;
 * -EIO when the share handle is broken or a lane found a malformed table, run or string-pool
 * range.  Locks: the engine's, then the share handle's, held to the end of the counter steps. */
#define EMQXGM_SHARE_NOT_SHARED 5u /* status of an entry whose dest is a node */
typedef struct emqxgm_publish_shared_out {
  emqxgm_publish_out pub; /* exactly what emqxgm_publish_batch answers */
  const uint32_t* share;  /* [4 * pub.n_routes], entry j at share[4j..4j+3] */
} emqxgm_publish_shared_out;
int emqxgm_publish_shared_batch(emqxgm_t* h, emqxgm_share_t* s, const uint8_t* bytes,
                                const uint32_t* offsets, uint32_t n, const uint32_t* hc,
                                const uint32_t* ht, const uint32_t* draw, const uint32_t* st_ptr,
                                const uint32_t* st_group, const uint32_t* st_filter,
                                const uint32_t* st_value, emqxgm_publish_shared_out* out);
/* subscribers/2 (:391-392): *n_out = the committed members of (group, topic), the first
 * min(cap, *n_out) into out in order, EMQXGM_SHARE_LOCAL_MEMBER set on the local ones.  From the
 * host mirror: no device call. */
int emqxgm_share_members(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len,
                         uint32_t* out, uint32_t cap, uint32_t* n_out);
/* The key's round_robin_per_group counter, EMQXGM_NONE when it has none (for tests). */
int emqxgm_share_counter(emqxgm_share_t* s, uint32_t group, const uint8_t* topic, uint32_t len,
                         uint32_t* out);
/* "pass_names" (requests per launch), "timing" and the read-only "kernel_us" as emqxgm_acl_tune;
 * "rebuild_load_pct" (1..50, default 50) and "rebuild_garbage_pct" (>= 1, default 100);
 * "stage_lds" (default 1: a block's topics go through LDS before they are hashed; 0 hashes them
 * from global memory, the slower side of the A/B in MEASUREMENTS.md r16) */
int emqxgm_share_tune(emqxgm_share_t* s, const char* key, int64_t value);
/* out = {keys, table slots, deleted slots, the longest probe chain of a stored key, members, live
 * pool words, garbage words, rebuilds forced by the table's load, rebuilds forced by garbage, pool
 * growths, counters held, pending mutations} */
int emqxgm_share_stats(emqxgm_share_t* s, uint64_t out[12]);

/* ---- admission: validate/2, parse/1 and the caps checks per name or filter -----------------
 * The steps of the channel in front of the match, for a batch of PUBLISH topic names or SUBSCRIBE
 * topic filters, on their raw bytes (any bytes: nothing is assumed to be UTF-8):
 *   EMQXGM_ADMIT_NAME    emqx_packet:check/1 -> emqx_topic:validate(name, Topic)
 *                        (apps/emqx/src/emqx_packet.erl:254-260, emqx_topic.erl:98-130), then
 *                        emqx_mqtt_caps:check_pub/2 (emqx_channel.erl:647,1850-1860,
 *                        emqx_mqtt_caps.erl:74-105);
 *   EMQXGM_ADMIT_FILTER  validate_topic_filters (emqx_packet.erl:267-273,411-420), then
 *                        emqx_topic:parse/1 (emqx_channel.erl:510,2087-2089,
 *                        emqx_topic.erl:206-233), then emqx_mqtt_caps:check_sub/3
 *                        (emqx_channel.erl:801,1885-1886, emqx_mqtt_caps.erl:107-152).
 * Stateless: a handle owns a stream and scratch only.  Per item one record of four words:
 *   rec[0]  validate verdict (EMQXGM_ADMIT_V_*) | parse verdict << 8 (0 ok, 1
 *           {invalid_topic_filter, _}) | caps reason code << 16 (0 ok, else the reference's byte,
 *           emqx_mqtt.hrl:173-192) | EMQXGM_ADMIT_WILDCARD | _SHARED | _EXCLUSIVE | _EXCL_LOOKUP
 *   rec[1]  levels/1 of the name, or of the topic parse/1 returned
 *   rec[2]  byte offset of the topic parse/1 returned inside the item (0 for a name)
 *   rec[3]  length of the share name parse/1 took from the string (it starts at byte 7), or
 *           EMQXGM_NONE
 * The three results are independent: parse is reported whatever validate said (NAME: 0), and the
 * caps are checked on the parsed topic whatever validate said.  validate is of the raw item.  A
 * sequence that <<_/utf8>> does not accept (RFC 3629: overlong forms, surrogates, above U+10FFFF,
 * lone continuation bytes, truncated sequences) in a word validate3 examines is
 * EMQXGM_ADMIT_V_FUNCTION_CLAUSE, as the reference ends in function_clause there.  For an item
 * whose parse failed, rec[1] and rec[2] are 0, rec[3] EMQXGM_NONE and no caps reason or flag is
 * set; for an item of more than 65535 bytes levels, wildcard and caps are not run (rec[1] 0, no
 * reason, no _WILDCARD or _EXCL_LOOKUP) and parse's answer stands (rec[2], rec[3], _SHARED,
 * _EXCLUSIVE).  EMQXGM_ADMIT_SHARED: the options carry `share` (from the string
 * or from EMQXGM_ADMIT_IN_HAS_SHARE).  EMQXGM_ADMIT_EXCL_LOOKUP: the zone has
 * exclusive_subscription and the filter is exclusive -- the reference asks
 * emqx_exclusive_subscription:check_subscribe/2 (emqx_mqtt_caps.erl:144-150), the caller must. */
#define EMQXGM_ADMIT_NAME 0u
#define EMQXGM_ADMIT_FILTER 1u
#define EMQXGM_ADMIT_V_OK 0u
#define EMQXGM_ADMIT_V_EMPTY_TOPIC 1u
#define EMQXGM_ADMIT_V_TOO_LONG 2u
#define EMQXGM_ADMIT_V_NAME_ERROR 3u
#define EMQXGM_ADMIT_V_INVALID_HASH 4u /* 'topic_invalid_#' */
#define EMQXGM_ADMIT_V_INVALID_CHAR 5u
#define EMQXGM_ADMIT_V_FUNCTION_CLAUSE 6u
#define EMQXGM_ADMIT_WILDCARD (1u << 24)
#define EMQXGM_ADMIT_SHARED (1u << 25)
#define EMQXGM_ADMIT_EXCLUSIVE (1u << 26)
#define EMQXGM_ADMIT_EXCL_LOOKUP (1u << 27)
#define EMQXGM_ADMIT_IN_RETAIN 4u    /* in_flags: bits 0-1 are the QoS */
#define EMQXGM_ADMIT_IN_HAS_SHARE 8u /* in_flags: the options passed to parse/1 carry `share` */
#define EMQXGM_ADMIT_RAISES 0x100u   /* emqxgm_admit_reason: parse/1 raises inside handle_in */
#define EMQXGM_ADMIT_MAX_ZONES 256u
/* A zone's caps (emqx_mqtt_caps.erl:61-72 has the defaults: 65535, 2, true, true, true, false;
 * max_topic_levels 0 = no limit, :94-96). */
typedef struct emqxgm_admit_caps {
  uint32_t max_topic_levels;
  uint8_t max_qos_allowed;
  uint8_t retain_available;
  uint8_t wildcard_subscription;
  uint8_t shared_subscription;
  uint8_t exclusive_subscription;
  uint8_t reserved[3];
} emqxgm_admit_caps;
typedef struct emqxgm_admit emqxgm_admit_t;
int emqxgm_admit_create(int32_t device, emqxgm_admit_t** out);
void emqxgm_admit_destroy(emqxgm_admit_t* a);
/* One batch of n items of one mode: item i is bytes[offsets[i] .. offsets[i+1]) (host memory).
 * in_flags[i] (null: all 0) = QoS | EMQXGM_ADMIT_IN_RETAIN | EMQXGM_ADMIT_IN_HAS_SHARE; zone[i]
 * (null: all 0) = the row of caps[n_zones] (1..256 rows) the item is checked against.  *out = the
 * records, four words per item, in host memory of the handle, valid until the next call on a.
 * Larger batches are cut into passes internally.  -EINVAL, before anything is launched, on
 * decreasing offsets, a zone >= n_zones, n_zones out of range or a max_qos_allowed above 2; -EIO
 * when a device call failed or a lane found an offset or zone out of bounds. */
int emqxgm_admit_batch(emqxgm_admit_t* a, uint32_t mode, const uint8_t* bytes,
                       const uint32_t* offsets, uint32_t n, const uint8_t* in_flags,
                       const uint8_t* zone, const emqxgm_admit_caps* caps, uint32_t n_zones,
                       const uint32_t** out);
/* The first failure in the order the channel takes them, from one record: NAME: any validate
 * error is 16#90 (emqx_channel.erl:647 after emqx_packet:check/1), then the caps reason; FILTER:
 * any validate error is 16#8F, then EMQXGM_ADMIT_RAISES for a parse failure, then the caps
 * reason; 0 = admitted.  No device call. */
uint32_t emqxgm_admit_reason(uint32_t mode, const uint32_t* rec);
/* "pass_items" (items per launch), "timing" and the read-only "kernel_us" as emqxgm_acl_tune;
 * "force_global" (1: no LDS tile, every item is read from global memory; same records);
 * "byte_base" (0..15, tests: the residue of a pass's first byte in its 16-B chunk). */
int emqxgm_admit_tune(emqxgm_admit_t* a, const char* key, int64_t value);
/* out = {calls, items, bytes, passes, scratch growths, kernel microseconds (timing on)} */
int emqxgm_admit_stats(emqxgm_admit_t* a, uint64_t out[6]);

/* ---- single-driver batcher core: publish windows over the host pipes ---------------------
 * A caller that batches topics itself (one thread adding, flushing and collecting; bench.py's
 * window sweep) packs them into a window in pinned host memory, submits a full window (or one
 * that is due) with emqxgm_match_batch_submit_filters, and on collection reads every topic's trie
 * row with its filter bytes (gathered on the device).  Up to EMQXGM_HOST_PIPES windows are in
 * flight; a window's result stays valid until that many more windows are flushed.  Collect waits
 * without the batcher's lock.  The NIF uses the concurrent entry below (emqxgm_async_*), which
 * any number of threads call one topic at a time (emqx_broker.erl:218-232,
 * emqx_trie.erl:147-169). */
typedef struct emqxgm_batcher emqxgm_batcher_t;
typedef struct emqxgm_batcher_cfg {
  uint32_t window_topics; /* topics per window (0 = 65,536; <= the engine's batch_max) */
  uint32_t window_bytes;  /* topic bytes per window (0 = 64 x window_topics) */
  uint32_t window_us;     /* a non-empty window is due this long after its first topic (0 = 50) */
  uint32_t reserved;
} emqxgm_batcher_cfg;
typedef struct emqxgm_window_out {
  uint32_t n;                 /* topics in the window, in the order they were added */
  uint32_t n_pairs;
  const uint64_t* tag;        /* [n] the caller's tag of each topic (e.g. its waiter) */
  const uint32_t* row;        /* [n+1] topic i's trie filters are pairs row[i] .. row[i+1] */
  const uint32_t* filter_id;  /* [n_pairs] */
  const uint32_t* foff;       /* [n_pairs + 1] pair j's filter bytes: fbytes[foff[j] .. foff[j+1]) */
  const uint8_t* fbytes;
  const uint32_t* exact_id;   /* [n] route key equal to the topic, or EMQXGM_NONE */
  uint64_t flush_ns, done_ns; /* CLOCK_MONOTONIC at the flush and when the result was complete */
} emqxgm_window_out;
int emqxgm_batcher_create(emqxgm_t* h, const emqxgm_batcher_cfg* cfg, emqxgm_batcher_t** out);
void emqxgm_batcher_destroy(emqxgm_batcher_t* b);
/* Appends a topic to the open window (*slot = its index there).  Returns 1 when the window is
 * now full (flush it before the next add), 0 otherwise; -E2BIG for a topic longer than a window,
 * -ENOSPC when the open window is full, -EINVAL. */
int emqxgm_batcher_add(emqxgm_batcher_t* b, const uint8_t* topic, uint32_t len, uint64_t tag,
                       uint32_t* slot);
/* Appends topics bytes[offsets[i] .. offsets[i+1]) for i in [0, n) (tag tag0 + i) until the
 * open window is full; returns how many were added (>= 0), or -EINVAL / -E2BIG as _add.  A
 * batcher process that drains several callers at once packs them with one call. */
int emqxgm_batcher_add_many(emqxgm_batcher_t* b, const uint8_t* bytes, const uint32_t* offsets,
                            uint32_t n, uint64_t tag0);
/* 1 when the open window holds topics and its first one was added window_us or more before
 * now_ns (CLOCK_MONOTONIC), else 0. */
int emqxgm_batcher_due(emqxgm_batcher_t* b, uint64_t now_ns);
/* Submits the open window and opens an empty one; *window = the window's id (0: it was empty,
 * nothing submitted).  -EBUSY when EMQXGM_HOST_PIPES windows are flushed and not collected. */
int emqxgm_batcher_flush(emqxgm_batcher_t* b, uint64_t* window);
/* Completes window `window` (flushed; the oldest first is cheapest) and returns its result,
 * read in place from the host pipe's pinned buffers: valid until EMQXGM_HOST_PIPES more windows
 * are flushed (collecting it again before that returns the same result). */
int emqxgm_batcher_collect(emqxgm_batcher_t* b, uint64_t window, emqxgm_window_out* out);

/* ---- concurrent publish entry: one topic per call from any number of threads ------------------
 * The reference matches every publish in the publisher's own process, on every scheduler at once
 * (emqx_broker:publish/1 -> emqx_router:match_routes/1 -> emqx_trie:match/1,
 * emqx_broker.erl:218-232, emqx_router.erl:141-153, read_concurrency ETS emqx_trie.erl:70-75).
 * emqxgm_async_match is what those processes call through the NIF (match_async/3): it appends the
 * topic to the open window in pinned memory and returns at once; a flusher thread submits a
 * window when it is full or window_us after its first topic, over the handles' host pipes (round
 * robin over the handles with a pipe free: one handle per GPU, each holding the whole index), and
 * one completer thread per handle waits for its windows in order and calls `cb` once per window
 * (from that thread; the windows of different handles concurrently).  The window passed to `cb`
 * is valid during the call only.  Every accepted call is reported exactly once, unless cancelled
 * first.  Errors of emqxgm_async_match: -E2BIG (longer than a window, or more than max_levels
 * levels), -EBUSY (every window full or in flight), -ESTALE (every handle's index is stale: see
 * "Health"), -EINVAL: the caller answers those itself.  Windows go to handles that are not stale;
 * a window whose handle is (or becomes) stale is reported with status -ESTALE.
 * A layer created with EMQXGM_ASYNC_PUBLISH answers each call with emqx_broker:publish/1's
 * routing instead (emqx_broker.erl:218-300: the aggre/1 entries of match_routes(Topic) and the
 * local dispatches, dispatch/2 :326-355, from the engine's fan-out tables): the completer runs
 * emqxgm_publish_batch for the window (the handle's publish results are then reused by it, so a
 * handle serves one publish layer). */
#define EMQXGM_TAG_CANCELLED 0xFFFFFFFFFFFFFFFFull /* never a caller's tag */
typedef struct emqxgm_async emqxgm_async_t;
typedef struct emqxgm_async_cfg {
  uint32_t window_topics;  /* topics per window (0 = 65,536; <= every handle's batch_max) */
  uint32_t window_bytes;   /* topic bytes per window (0 = 64 x window_topics) */
  uint32_t window_us;      /* a window is submitted at most this long after its first topic (0 = 50) */
  uint32_t max_levels;     /* calls for topics with more levels: -E2BIG (0 = no limit) */
  uint32_t queued_windows; /* full windows that may wait for a pipe (0 = 2) */
  uint32_t flags;          /* EMQXGM_ASYNC_PUBLISH: windows are answered with the publish
                              fan-out (emqxgm_publish_batch) instead of trie rows */
  uint32_t deliver_threads;/* 0 or 1: each completer calls cb once per window; k > 1: a window
                              of at least 2,048 calls is reported in up to k parts of >= 1,024
                              calls, `cb` running concurrently on the completer and k - 1 pool
                              threads (a view per part: n, tag, owner, row / exact_id /
                              route_ptr / deliver_ptr offset to the part; pair and entry indices
                              stay absolute).  For a caller whose per-call report is costly (the
                              NIF: terms + enif_send), so one thread does not bound the rate */
  uint32_t fail_threshold; /* 0: no health counting (the default); k > 0: k consecutive failures
                              -- calls cancelled while still pending (a caller that timed out) or
                              windows that failed other than -ESTALE -- mark every handle stale
                              (emqxgm_mark_stale), so a hung GPU costs the callers in flight one
                              timeout each and every later call is refused at once (-ESTALE) until
                              the index is repaired.  A window answered resets the count. */
} emqxgm_async_cfg;
#define EMQXGM_ASYNC_PUBLISH 1u
/* flags: a window is sealed and submitted as soon as a pipe is free and no sealed window waits,
 * instead of window_us after its first call.  An idle layer then answers a call in one pass; a
 * loaded one still grows its windows while every pipe is busy (the pipes' pace sets their size). */
#define EMQXGM_ASYNC_EAGER 2u
typedef struct emqxgm_async_window {
  int status;               /* 0, or the negative errno the window's pass failed with (no result) */
  uint32_t n;               /* calls in the window, in the order they were made */
  uint32_t n_pairs;
  uint32_t device_index;    /* the handle that matched it */
  const uint64_t* tag;      /* [n] each call's tag (EMQXGM_TAG_CANCELLED: cancelled, skip it) */
  const uint64_t* owner;    /* [n] each call's owner (e.g. the calling process) */
  const uint32_t* row;      /* [n+1] call i's trie filters are pairs row[i] .. row[i+1] */
  const uint32_t* filter_id;/* [n_pairs] */
  const uint32_t* foff;     /* [n_pairs + 1] pair j's filter bytes: fbytes[foff[j] .. foff[j+1]) */
  const uint8_t* fbytes;
  const uint32_t* exact_id; /* [n] route key equal to the topic, or EMQXGM_NONE */
  uint64_t first_ns, flush_ns, done_ns; /* CLOCK_MONOTONIC: first call, submit, result complete */
  /* EMQXGM_ASYNC_PUBLISH layers (row .. exact_id are then unset): the window's
   * emqxgm_publish_batch result -- call i's aggre/1 entries are [route_ptr[i], route_ptr[i+1])
   * (filter id To, dest handle), its local dispatches [deliver_ptr[i], deliver_ptr[i+1])
   * (filter id To, subscriber handle) -- and the bytes of each entry's To:
   * rfbytes[rfoff[j] .. rfoff[j+1]) (rfoff has n_routes + 1 entries) */
  uint64_t n_routes, n_deliveries;
  const uint64_t* route_ptr;
  const uint32_t* route_filter;
  const uint32_t* route_dest;
  const uint64_t* deliver_ptr;
  const uint32_t* deliver_filter;
  const uint32_t* deliver_sub;
  const uint64_t* rfoff;
  const uint8_t* rfbytes;
} emqxgm_async_window;
typedef void (*emqxgm_async_cb)(void* user, const emqxgm_async_window* w);
int emqxgm_async_create(emqxgm_t* const* hs, uint32_t n_handles, const emqxgm_async_cfg* cfg,
                        emqxgm_async_cb cb, void* user, emqxgm_async_t** out);
/* Stops taking calls, submits and reports every accepted one, then frees the layer. */
void emqxgm_async_destroy(emqxgm_async_t* a);
int emqxgm_async_match(emqxgm_async_t* a, const uint8_t* topic, uint32_t len, uint64_t tag,
                       uint64_t owner);
/* 1: the call (tag, owner) was still pending and will never be reported; 0: it was reported
 * already (when its window is being reported right now, this waits until that is done) or is
 * unknown.  A caller that timed out cancels, and on 0 finds the report delivered. */
int emqxgm_async_cancel(emqxgm_async_t* a, uint64_t tag, uint64_t owner);
/* out = {calls accepted, windows submitted, calls reported, -EBUSY refusals, cancelled, -E2BIG
 * refusals (levels), windows failed, windows outstanding} */
int emqxgm_async_stats(emqxgm_async_t* a, uint64_t out[8]);
/* out = {handles stale now, timeouts counted (pending calls cancelled), failed windows counted,
 * calls refused with -ESTALE}.  Returns out[0]. */
int emqxgm_async_health(emqxgm_async_t* a, uint64_t out[4]);

/* ---- handle registry: the 32-bit names of dest and subscriber terms, reused (r06) ----------
 * The engine's fan-out tables name nodes, shared-subscription groups and subscribers by handles
 * the caller chooses (emqxgm_route_dests_batch / _subscribers_batch); the NIF maps them back to
 * terms.  A broker whose clients reconnect sees a new subscriber pid per connection, so handles
 * must be reused or the tables grow without bound (the reference's subscriber_down/1 removes every
 * trace of a pid, emqx_broker.erl:361-380, emqx_broker_helper.erl:133-165).  A handle may be
 * reused only when no answer can still name it for its old term: the caller releases it after the
 * commit that removed it from every list (its lists were set without it and committed), and the
 * registry hands it out again only once every window the layers had submitted before the release
 * has been reported (windows submitted later read an epoch without it).  _alloc: a quiesced
 * released handle of `kind`, else the next never-used number (-E2BIG past EMQXGM_HANDLE_MAX);
 * _release: -ENOENT if not allocated; _stats: {numbers made, allocated, released and waiting for
 * their windows, free}.  Thread-safe.  A released subscriber's lists must all have been committed
 * without it; a full resync (emqxgm_route_sync_begin .. _end) clears every subscriber list it did
 * not set, so a topic whose last subscriber left cannot keep a reused number. */
#define EMQXGM_HANDLE_KINDS 3 /* 0 node, 1 group, 2 subscriber */
#define EMQXGM_HANDLE_MAX 0x7FFFFFFFu
typedef struct emqxgm_handles emqxgm_handles_t;
int emqxgm_handles_create(emqxgm_async_t* const* layers, uint32_t n_layers, emqxgm_handles_t** out);
void emqxgm_handles_destroy(emqxgm_handles_t* r);
int emqxgm_handles_alloc(emqxgm_handles_t* r, uint32_t kind, uint32_t* handle);
int emqxgm_handles_release(emqxgm_handles_t* r, uint32_t kind, uint32_t handle);
int emqxgm_handles_stats(emqxgm_handles_t* r, uint32_t kind, uint64_t out[4]);
/* every allocated handle of every kind released at once (a restarted mirror whose own table of
 * them was lost; its resync then rewrites every list) */
int emqxgm_handles_reset(emqxgm_handles_t* r);

/* ---- filter-sharded layout over several GPUs (the subscription set partitioned by
 * filter, the topic batch broadcast, the per-GPU match lists gathered to one GPU) ----
 * emqxgm_export copies a device-resident result (emqxgm_match_device / _wait) into the caller's
 * device buffers (row [n+1], fid [n_pairs], exact [n]), mapping filter and exact ids through
 * id_map (device u32 array, local id -> global id; NULL = identity; NONE stays NONE).
 * emqxgm_merge merges `parts` such results of one batch (rows/fids/exacts: host arrays of device
 * pointers) into one CSR on the handle's device: topic t's row is shard 0's row, then shard 1's,
 * ...; its exact id the one shard's that has it.  out_fid holds the sum of the parts' pairs;
 * *n_pairs = that sum.  Both calls return when the device work is complete. */
int emqxgm_export(emqxgm_t* h, const emqxgm_dev_out* r, const uint32_t* id_map, uint32_t* row,
                  uint32_t* fid, uint32_t* exact);
int emqxgm_merge(emqxgm_t* h, uint32_t parts, const uint32_t* const* rows,
                 const uint32_t* const* fids, const uint32_t* const* exacts, uint32_t n,
                 uint32_t* out_row, uint32_t* out_fid, uint32_t* out_exact, uint32_t* n_pairs);

/* The key-partitioned layout of a route-key-heavy index (cfg4: 100M exact keys, DESIGN.md 5,
 * SURVEY 8e's alternative): the plain route keys are split over `parts` engines by key hash
 * (emqxgm_key_owners: owner[i] of packed key i, a function of its bytes and the engine's
 * full_hash_bits only), each engine also holding every wildcard filter.  A batch's names are
 * probed each by its owner only: emqxgm_exact_owned_device writes to d_out (device, n u32) the
 * owned names' route-key ids and EMQXGM_NONE for the others, without a probe (the trie walk of a
 * topic and its wildcard-key probe are its topic block's, emqxgm_match_device on that block). */
int emqxgm_key_owners(emqxgm_t* h, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                      uint32_t parts, uint32_t* owner);
int emqxgm_exact_owned_device(emqxgm_t* h, const uint8_t* d_bytes, const uint32_t* d_offsets,
                              uint32_t n, uint32_t parts, uint32_t part, uint32_t* d_out);

/* The compact wire form of a shard's result for the exchange to the root:
 *   cnt  per-topic pair counts: n u8 (255 = in ovf), or with EMQXGM_WIRE_CNT2 two bit planes per
 *        64 topics (16 B per 64 topics, 2 bits a topic; 3 = in ovf) -- for sparse results;
 *   fid  the pairs' ids mapped through id_map (NULL = identity): n_pairs u32, or with
 *        EMQXGM_WIRE_ID24 (every id < 2^24) n_pairs u16 low halves then n_pairs u8 high bytes;
 *   xs   (topic, exact id) u32 pairs of the topics that equal a route key;
 *   ovf  (topic, count) u32 pairs of the counts the count width cannot hold.
 * xs and ovf are device arrays of 2 x n u32; counts[0] / counts[1] = their entries.
 * emqxgm_merge_wire merges `parts` such results (host arrays of device pointers, flags and
 * lengths) into one CSR exactly as emqxgm_merge does.  Both return when the device work is
 * complete. */
#define EMQXGM_WIRE_CNT2 1u
#define EMQXGM_WIRE_ID24 2u
int emqxgm_export_wire(emqxgm_t* h, const emqxgm_dev_out* r, const uint32_t* id_map,
                       uint32_t flags, void* cnt, void* fid, uint32_t* xs, uint32_t* ovf,
                       uint32_t counts[2]);
int emqxgm_merge_wire(emqxgm_t* h, uint32_t parts, const uint32_t* flags, const void* const* cnts,
                      const void* const* fids, const uint32_t* n_pairs_part,
                      const uint32_t* const* xss, const uint32_t* n_xs, const uint32_t* const* ovfs,
                      const uint32_t* n_ovf, uint32_t n, uint32_t* out_row, uint32_t* out_fid,
                      uint32_t* out_exact, uint32_t* n_pairs);

/* Diagnostic pass (instrumented walk kernel, not the production launch): runs the device
 * match and returns out[0] = trie states matched (SURVEY 8d S(t) summed over the batch),
 * out[1] = edge slots loaded, out[2] = pairs, out[3] = levels (words) in the batch,
 * out[4] = walk iterations summed over busy lanes, out[5] = walk iterations summed over
 * wavefronts (one memory round trip each). */
int emqxgm_walk_census(emqxgm_t* h, const uint8_t* d_bytes, const uint32_t* d_offsets,
                       uint32_t n, uint64_t bytes_len, uint64_t out[6]);
/* The last census pass's edge-bucket loads by probed level: out[d] literal probes of level d,
 * out[16 + d] '+' probes (levels >= 15 lumped into 15).  Returns the number of counters (32). */
int emqxgm_walk_census_levels(emqxgm_t* h, uint64_t* out, uint32_t n_out);

int emqxgm_set_profiling(emqxgm_t* h, int on);
/* Runtime tuning knobs: "walk_wg_per_cu" (persistent walk workgroups per CU); "leaf_prune"
 * (1 default: depth-code pruning in the walk, 0 off); "plus_sig" (1 default: the walk drops the
 * literal probe under a carried '+' child whose lent signature rules the next word
 * out; 0: lent signatures are ignored, an A/B -- from the next pass on, no rebuild; the pair walk
 * is built without this filter: it runs batches of at most half the walk grid's
 * lanes, every batch of an index whose walks outgrew a lane's shallow stack, and every batch at
 * "walk_pair" 2; emqxgm_walk_census always runs a one-lane walk with the filter, so for such
 * passes it counts slightly fewer loads than the production kernel issues);
 * "root_plus_half" (1 default: when the root's only literal child G rides in the walk's arguments
 * and G's '+' child has exactly one literal child H, a copy of H's slot rides there too and the walk
 * decides (G/+, word 2) from it without a probe; 0: the copy is ignored) and "keyed_share"
 * (1 default: the keyed items of one topic at one level, which share a home bucket, are decided
 * from one loaded line; 0: each takes a probe of its own) -- both A/B switches from the next pass
 * on, no rebuild, same rows either way (a row's order may differ); like "plus_sig" they act in the
 * one-lane-per-topic walks and the census, and the pair walk is built without them;
 * "closed_buckets" (1 default: a lookup that finds neither its edge nor an empty slot in a bucket
 * ends there when the bucket's line says that no edge was placed past it; 0: the marks
 * are ignored and every such lookup goes on to the next bucket -- an A/B switch like the two above,
 * from the next pass on, same rows; the pair walk is built without the rule);
 * "rec_parts" (0 default: a pass's tokenizer stores, and its walk loads, only the 16-B parts of
 * each 64-B topic record that the committed index can read -- three of four, and a 4-B header
 * word, while no trie filter has 7 levels or more; 4: full records always -- an A/B
 * switch from the next pass on, same rows, same order, every walk variant and the census);
 * "rec_even" (1 default: a three-part pass over an index whose literal edges of level 0, and those
 * of level 2, each carry at most one token (`site/<id>/device/<id>/...`) moves even-elided records,
 * two parts {tok1, tok3} {tok4, tok5} and a header bit for each of the words 0 and 2, DESIGN.md 3,
 * where its walk has the reader: the one-lane-per-topic walks and the census, not the pair walk
 * or the spilling one; 0: three parts -- an A/B switch from the next pass on, same rows;
 * emqxgm_stats::even_passes counts the passes enqueued in the form; "rec_parts" 4 overrides it);
 * "host_out" (host pipes copy results to the
 * host with hipMemcpyAsync, 0 default, or with a kernel writing host memory, 1);
 * "walk_pair" (1 default: a batch of at most half the walk grid's lanes is walked by two lanes
 * per topic; 0: one lane per topic); "exact_range_kb" (0 default: one route-key probe pass over the whole table; > 0: the probe
 * runs in passes over bucket ranges of that many KiB, so that the lines in flight share page
 * translations -- measured slower on a 100M-key table, kept as an option); "delta_commit": 0 = every commit rebuilds the index, 1 = small deltas are patched in place
 * (default), 2 = every delta that fits the tables' load bounds is patched in place; "delta_max":
 * the changes a delta commit takes in mode 1 (0 default = max(4096, (trie members + route keys)
 * / 8));
 * "fat_buckets": 1 (default) = single-literal-child nodes keep their child in their own bucket
 * line, 0 = none (A/B runs), from the next full build on (the next commit);
 * "roctx": 1 = roctx ranges around passes, waits and commits and a marker at each kernel launch
 * (rocprofv3 --marker-trace; also EMQXGM_ROCTX=1 at create), 0 (default) = none;
 * "keyed": token-keyed trie parents from the next full build: 1 (default) =
 * automatic, 0 = none, 2 = every eligible node (tests); "zc_topics": the largest pinned window
 * of _submit_filters that goes without DMA copies (65536 default, 0 = always copies); "spin_us":
 * host pipes' waits poll the pass's completion for up to this long before they block (200
 * default, 0 = block at once); "bg_build": full builds of registries of at least this many
 * filters run in a background thread while commits keep patching the current index (16384
 * default, 0 = every full build blocks the writers, as before r05); "bg_delay_ms": a background
 * build holds its install back this long (tests: a build in flight on demand); "rebuild" (1):
 * start a background full build of the registry now without waiting for it (-EBUSY: one is in
 * flight; it also compacts the tables' deleted slots); "probe_ms": a repair's bounded wait for
 * the engine's streams (2000 default).  Fault injection (tests of "Health"): "fail_commits" (n):
 * the next n commits fail before they change anything, with errno "fail_errno" (EIO default);
 * "hang_ms": every host-pipe wait and publish pass stalls this long first (0 default).
 * "stage_rank_bits": caps the rank field of the packed pair staging (tests of the wide redo a
 * topic with more pairs than the field holds takes; 0 default = as wide as fits). */
int emqxgm_tune(emqxgm_t* h, const char* key, int64_t value);
int emqxgm_get_stats(emqxgm_t* h, emqxgm_stats* st);
/* Last HIP error string seen by the handle (for diagnostics). */
const char* emqxgm_last_error(emqxgm_t* h);

#ifdef __cplusplus
}
#endif
#endif /* EMQX_GPUMATCH_H */
