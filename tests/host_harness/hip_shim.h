// hip_shim.h -- TEST INFRASTRUCTURE: the HIP device keywords and the few builtins that
// emqx_amd/csrc/gm_tok.inc mentions, defined away or as plain C++, so that a host harness
// (tok_main.cpp) includes the file unchanged and calls its per-lane functions one lane at a time.
// Included after the fake runtime's <hip/hip_runtime.h> (uint4, make_uint4).  Nothing here runs
// lanes in step: a kernel that synchronises its workgroup (__syncthreads, ballots) compiles, and
// only kernels whose lanes are independent (k_xhash, k_exact_owned) may be called whole, in a loop
// over threadIdx.x.
#pragma once
#include <stdint.h>
#include <string.h>

#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(n)
// store_rec's 16-B vector type: GCC spells the attribute vector_size(bytes)
#define ext_vector_type(n) vector_size(4 * (n))
#define __builtin_nontemporal_store shim_nontemporal_store
#define __builtin_amdgcn_alignbyte shim_alignbyte
#define __builtin_amdgcn_wave_barrier() ((void)0)
#define __builtin_amdgcn_fence(order, scope) ((void)0)

struct shim_dim3 {
  uint32_t x = 0, y = 0, z = 0;
};
static shim_dim3 threadIdx, blockIdx;
static shim_dim3 gridDim = {1, 1, 1};

// v_alignbyte_b32: bytes sh .. sh + 3 of the 8-byte value {hi, lo}
static inline uint32_t shim_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3u)));
}
template <class V>
static inline void shim_nontemporal_store(V v, V* p) {
  memcpy(p, &v, sizeof v);  // (a record part is 4-byte aligned here, the vector type asks for 16)
}
static inline uint32_t min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// one lane at a time: a workgroup barrier is nothing, a vote is the lane's own
static inline void __syncthreads() {}
static inline int __syncthreads_or(int v) { return v; }
static inline uint64_t __ballot(int v) { return v ? 1ull : 0ull; }
static inline int __popcll(uint64_t v) { return __builtin_popcountll(v); }
