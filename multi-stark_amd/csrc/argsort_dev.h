// The sorting permutation of a circuit's rows, the part that is the same text in both fields (ms_witness_argsort in argsort.hip,
// msbb_witness_argsort in bb_argsort.hip; the algorithm is described at the top of argsort.hip): the tile and round constants,
// the LDS count that a wave with one digit adds once, the sum of the histogram slots, and the three launches of a digit pass -
// per-tile counts, one-workgroup offsets, the ballot-ranked scatter. Include it from a .hip file only; everything lives in an
// unnamed namespace, so each translation unit compiles the kernels it launches for itself.
//   What a field brings: the key word K of as_count_k / as_scatter_k (u64: a Goldilocks cell as it lies in the trace; u32: the
// canonical value of a BabyBear cell), the number of 8-bit digits in it (the HIST words of as_hist_sum_k are digits x 256), and
// its own histogram / extraction, gather and final kernels, which know the layout of the trace.
#pragma once
#include "msamd.h"

namespace msamd {
namespace {

constexpr u32 AS_THREADS = 256, AS_STEPS = 16, AS_TILE = AS_THREADS * AS_STEPS, AS_WAVES = AS_THREADS / 64, AS_SLOTS = AS_STEPS * AS_WAVES;
constexpr u32 AS_BITS = 8, AS_RADIX = 1u << AS_BITS;
constexpr u32 AS_OFF_THREADS = 1024, AS_OFF_PER = 4, AS_OFF_ROUND = AS_OFF_THREADS * AS_OFF_PER, AS_OFF_WAVES = AS_OFF_THREADS / 64;
constexpr u32 AS_HIST_GROUPS = 256, AS_MAX_KEYS = 8;

// one more row with digit d in the LDS histogram h; every lane of the wave calls this. A wave whose valid rows all share the digit
// adds once (constant digits are the common case, and 64 atomics on one word serialise)
__device__ __forceinline__ void as_lds_count(u32* h, u32 d, bool valid) {
  const u32 lane = threadIdx.x & 63;
  const unsigned long long act = __ballot(valid);
  if (!act) return;
  const u32 lead = (u32)__ffsll((long long)act) - 1;
  const u32 d0 = (u32)__shfl((int)d, (int)lead, 64);
  const unsigned long long same = __ballot(valid && d == d0);
  if (same == act) {
    if (lane == lead) atomicAdd(&h[d0], (u32)__popcll(act));
  } else if (valid) {
    atomicAdd(&h[d], 1u);
  }
}

// hist[k][i] = the sum over column k's `groups` slots of HIST words; one thread per (k, i)
template <u32 HIST>
__global__ __launch_bounds__(AS_THREADS) void as_hist_sum_k(const u32* slots, u32 groups, u32 total, u32* hist) {
  const u32 i = blockIdx.x * AS_THREADS + threadIdx.x;
  if (i >= total) return;
  const u32 k = i / HIST, w = i % HIST;
  u32 s = 0;
  for (u32 g = 0; g < groups; g++) s += slots[(size_t(k) * groups + g) * HIST + w];
  hist[i] = s;
}

template <class K>
__global__ __launch_bounds__(AS_THREADS) void as_count_k(const K* keys, size_t n, u32 shift, u32 n_tiles, u32* counts) {
  __shared__ u32 h[AS_RADIX];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (u32 j = 0; j < AS_STEPS; j++) {
    const size_t r = size_t(blockIdx.x) * AS_TILE + j * AS_THREADS + threadIdx.x;
    const bool valid = r < n;
    as_lds_count(h, valid ? (u32)(keys[r] >> shift) & (AS_RADIX - 1) : 0, valid);
  }
  __syncthreads();
  counts[size_t(threadIdx.x) * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// counts -> their exclusive prefix sums, in place; one workgroup, AS_OFF_ROUND counts per round
__global__ __launch_bounds__(AS_OFF_THREADS) void as_offsets_k(u32* counts, size_t total) {
  __shared__ u32 sm[AS_OFF_WAVES];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 carry = 0;
  for (size_t base = 0; base < total; base += AS_OFF_ROUND) {
    const size_t i0 = base + size_t(threadIdx.x) * AS_OFF_PER;
    u32 v[AS_OFF_PER], s = 0;
#pragma unroll
    for (u32 q = 0; q < AS_OFF_PER; q++) {
      v[q] = i0 + q < total ? counts[i0 + q] : 0;
      s += v[q];
    }
    u32 inc = s;
    for (u32 d = 1; d < 64; d <<= 1) {
      const u32 up = (u32)__shfl_up((int)inc, d, 64);  // (every lane takes part in the shuffle)
      if (lane >= d) inc += up;
    }
    if (lane == 63) sm[wave] = inc;
    __syncthreads();
    u32 before = 0, round_total = 0;
    for (u32 k = 0; k < AS_OFF_WAVES; k++) {
      const u32 w = sm[k];
      if (k < wave) before += w;
      round_total += w;
    }
    u32 x = carry + before + inc - s;
#pragma unroll
    for (u32 q = 0; q < AS_OFF_PER; q++) {
      if (i0 + q < total) counts[i0 + q] = x;
      x += v[q];
    }
    carry += round_total;
    __syncthreads();
  }
}

// idx_in nullptr: the pairs are in row order (index = position); keys_out nullptr: the keys are not needed again
template <class K>
__global__ __launch_bounds__(AS_THREADS) void as_scatter_k(const K* keys_in, const u32* idx_in, size_t n, u32 shift, u32 n_tiles, const u32* offsets,
                                                           K* keys_out, u32* idx_out) {
  __shared__ uint16_t cnt[AS_SLOTS * AS_RADIX];  // [slot][digit]: the slot's rows with that digit (at most 64), then their prefix over the slots
  __shared__ u32 first[AS_RADIX];                // where the tile's first pair with that digit goes
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    u32* z = reinterpret_cast<u32*>(cnt);
    for (u32 i = threadIdx.x; i < AS_SLOTS * AS_RADIX / 2; i += AS_THREADS) z[i] = 0;
  }
  first[threadIdx.x] = offsets[size_t(threadIdx.x) * n_tiles + blockIdx.x];
  __syncthreads();
  const size_t r0 = size_t(blockIdx.x) * AS_TILE + threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1;
  K key[AS_STEPS];
  u32 rank[AS_STEPS];
#pragma unroll
  for (u32 j = 0; j < AS_STEPS; j++) {
    const size_t r = r0 + j * AS_THREADS;
    const bool valid = r < n;
    key[j] = valid ? keys_in[r] : 0;
    const u32 d = (u32)(key[j] >> shift) & (AS_RADIX - 1);
    unsigned long long eq = __ballot(valid);  // the valid lanes whose digit equals this lane's
#pragma unroll
    for (u32 b = 0; b < AS_BITS; b++) {
      const bool bit = (d >> b) & 1;
      const unsigned long long with = __ballot(bit);
      eq &= bit ? with : ~with;
    }
    rank[j] = (u32)__popcll(eq & below);
    if (valid && rank[j] == 0) cnt[(j * AS_WAVES + wave) * AS_RADIX + d] = (uint16_t)__popcll(eq);
  }
  __syncthreads();
  {
    u32 run = 0;  // digit threadIdx.x along its slots, in row order
    for (u32 s = 0; s < AS_SLOTS; s++) {
      const u32 c = cnt[s * AS_RADIX + threadIdx.x];
      cnt[s * AS_RADIX + threadIdx.x] = (uint16_t)run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (u32 j = 0; j < AS_STEPS; j++) {
    const size_t r = r0 + j * AS_THREADS;
    if (r >= n) continue;
    const u32 d = (u32)(key[j] >> shift) & (AS_RADIX - 1);
    const size_t pos = size_t(first[d]) + cnt[(j * AS_WAVES + wave) * AS_RADIX + d] + rank[j];
    if (pos >= n) continue;  // (cannot happen: the offsets are the prefix sums of these very counts)
    idx_out[pos] = idx_in ? idx_in[r] : (u32)r;
    if (keys_out) keys_out[pos] = key[j];
  }
}

}  // namespace
}  // namespace msamd
