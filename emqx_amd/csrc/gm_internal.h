// gm_internal.h -- entry points of the engine (gm_engine.cpp) that only the library's own layers
// use (the concurrent publish entry, gm_async.cpp); not part of the C-ABI.  The async layer's
// host harness (tests/host_harness/async_harness.cpp) defines them over its mock engine.
#pragma once
#include <stdint.h>

#include "../../include/emqx_gpumatch.h"

// emqxgm_match_batch_submit_filters for a window whose offsets the caller built increasing
// (no O(n) check)
int gm_submit_window(emqxgm_t* h, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                     uint64_t* ticket);
// every host pipe of h sized for windows of n topics / nb bytes (no reallocation later)
int gm_reserve_windows(emqxgm_t* h, uint32_t n, uint64_t nb);
// whether h's index is stale (include/emqx_gpumatch.h "Health"): one atomic load, per call
int gm_stale(emqxgm_t* h);

// One chunk (at most batch_max topics) of a publish pass, as the engine leaves it on the device
// after the fan-out's fill: what a layer that answers the chunk's entries in the same pass reads
// (gm_pubshare.cpp).  The index arrays are those of the epoch the match and the fan-out read,
// which the engine holds until the hook returns.
typedef struct gm_pub_chunk {
  void* stream;             /* hipStream_t of the pass */
  uint32_t i0, m;           /* topics [i0, i0 + m) of the call */
  uint32_t n_routes;        /* aggre entries of the chunk */
  uint64_t rbase;           /* aggre entries of the call before this chunk */
  const uint32_t* rp;       /* [m+1] device: entries of topic i0 + t are [rp[t], rp[t+1]) */
  const uint32_t* o_rf;     /* [n_routes] device: entry filter ids */
  const uint32_t* o_rd;     /* [n_routes] device: entry dests */
  const uint8_t* fbytes;    /* device: the index's filter string pool, pool_bytes of it */
  const uint64_t* foff;     /* [n_filters+1] device */
  uint64_t n_filters, pool_bytes;
} gm_pub_chunk;
typedef int (*gm_pub_chunk_fn)(void* ctx, const gm_pub_chunk* c);
// emqxgm_publish_batch with fn(ctx, chunk) called per chunk, on the calling thread under the
// engine's lock, after the fill was enqueued and before the epoch is released; a non-zero return
// ends the call with it.  fn NULL: emqxgm_publish_batch itself.
int gm_publish_hooked(emqxgm_t* h, const uint8_t* bytes, const uint32_t* offsets, uint32_t n,
                      emqxgm_publish_out* out, gm_pub_chunk_fn fn, void* ctx);
// the device h was created on
int gm_engine_device(emqxgm_t* h);
