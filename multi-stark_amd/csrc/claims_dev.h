// The compaction behind a claim program with a `keep` expression (ms_witness_claims_fill in fill.hip; the definition is in
// include/mstark.h, "CLAIM PROGRAMS"), templated on the word the claims are stored in, as argsort_dev.h is on its field. Include
// it from a .hip file only; everything lives in an unnamed namespace.
//
// The evaluation pass (fill_k) leaves a temporary of rows x (W + 1) words, row-major: the W elements of row r and, in column W,
// its keep flag. The kept rows go, in ascending row order, to dst as rows of W words. A tile is CL_TILE = 256 threads x 4 rows,
// and wave v of a tile owns the 256 consecutive rows from tile * 1024 + v * 256 on, as four rounds of 64: lane l looks at the
// flag of row base + 64 j + l, so a ballot is the flags of 64 consecutive rows and a popcount their number.
//   (a) claims_count_k    per tile: the number of kept rows - ballots and popcounts per wave, the four wave totals joined in LDS
//   (b) claims_offsets_k  ONE workgroup: exclusive prefix of the tile counts, 256 per round with the carry behind the round,
//                         and the total
//   (c) claims_scatter_k  per tile: the ballots again; a kept row's rank inside its wave is the popcount of the earlier rounds
//                         plus mbcnt of its own, and the row's number goes to list[rank] in LDS. Then the wave copies
//                         count x W words: lane l takes the flat words l, l + 64, ... of the wave's output, word f being
//                         element f % W of kept row list[f / W] - consecutive lanes write consecutive words whatever W is and
//                         read consecutive words of one row (of two rows where a row ends), so a 49-word claim is copied as
//                         fast as a 4-word one. The quotient is never divided out again: k and c advance by 64 / W and 64 % W.
// The phases are ordered by the launches; no workgroup waits for another, and no position depends on the order in which atomics
// land (there are none). rows <= CL_TILE takes (c) alone, which then also leaves the total.
// Bytes, with S = sizeof(Word): the pass writes S (W + 1) per row; (a) reads S per row (the flag; a sector of 32 bytes where W + 1
// >= 4), (c) reads S per row again and S W per kept row and writes S W per kept row; counts and offsets are 16 bytes per tile.
#pragma once
#include "msamd.h"

namespace msamd {
namespace {

constexpr u32 CL_THREADS = 256, CL_ROWS = 4, CL_TILE = CL_THREADS * CL_ROWS, CL_WAVES = CL_THREADS / 64, CL_WAVE_ROWS = 64 * CL_ROWS;

template <class Word>
struct ClParams {
  const Word* tmp;     // rows x (W + 1), the flag in column W
  Word* dst;           // kept x W
  u64* counts;         // per tile (a) -> (b)
  u64* offsets;        // per tile: kept rows in front of it (nullptr: one tile, 0)
  u64* total;          // where the number of kept rows goes: (b), or (c) of a single tile (nullable)
  size_t rows;
  u32 W, n_tiles;
};

// the flags of the wave's round j as a ballot (row = first + 64 j + lane; rows from p.rows on are not kept)
template <class Word>
__device__ __forceinline__ u64 cl_ballot(const ClParams<Word>& p, size_t first, u32 j, u32 lane, bool& mine) {
  const size_t r = first + 64 * j + lane;
  mine = r < p.rows && p.tmp[r * (size_t(p.W) + 1) + p.W] != 0;
  return __ballot(mine);
}

template <class Word>
__global__ __launch_bounds__(CL_THREADS) void claims_count_k(ClParams<Word> p) {
  __shared__ u32 wave_cnt[CL_WAVES];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t first = blockIdx.x * size_t(CL_TILE) + wave * CL_WAVE_ROWS;
  u32 cnt = 0;
  for (u32 j = 0; j < CL_ROWS; j++) {
    bool mine;
    cnt += __popcll(cl_ballot(p, first, j, lane, mine));
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 t = 0;
    for (u32 k = 0; k < CL_WAVES; k++) t += wave_cnt[k];
    p.counts[blockIdx.x] = t;
  }
}

template <class Word>
__global__ __launch_bounds__(CL_THREADS) void claims_offsets_k(ClParams<Word> p) {  // one workgroup
  __shared__ u64 wave_sum[CL_WAVES];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 carry = 0;  // kept rows in front of the round's first tile
  for (u32 t0 = 0; t0 < p.n_tiles; t0 += CL_THREADS) {
    const u32 t = t0 + threadIdx.x;
    const u64 mine = t < p.n_tiles ? p.counts[t] : 0;
    u64 inc = mine;
    for (u32 d = 1; d < 64; d <<= 1) {
      const u64 up = (u64)__shfl_up((unsigned long long)inc, d, 64);  // (every lane takes part in the shuffle)
      if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
    for (u32 k = 0; k < CL_WAVES; k++) {
      if (k < wave) before += wave_sum[k];
      all += wave_sum[k];
    }
    if (t < p.n_tiles) p.offsets[t] = carry + before + inc - mine;
    carry += all;
    __syncthreads();  // (wave_sum is written again by the next round)
  }
  if (threadIdx.x == 0) *p.total = carry;
}

template <class Word>
__global__ __launch_bounds__(CL_THREADS) void claims_scatter_k(ClParams<Word> p) {
  __shared__ u32 wave_cnt[CL_WAVES];
  __shared__ uint16_t list[CL_WAVES][CL_WAVE_ROWS];  // per wave: its kept rows, counted from the wave's first row, ascending
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t first = blockIdx.x * size_t(CL_TILE) + wave * CL_WAVE_ROWS;
  u32 cnt = 0;
  for (u32 j = 0; j < CL_ROWS; j++) {
    bool mine;
    const u64 b = cl_ballot(p, first, j, lane, mine);
    const u32 rank = cnt + __builtin_amdgcn_mbcnt_hi((u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0));  // kept rows of the wave before this one
    if (mine) list[wave][rank] = (uint16_t)(64 * j + lane);
    cnt += __popcll(b);
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();  // (the list is read by other lanes than wrote it)
  u64 base = p.offsets ? p.offsets[blockIdx.x] : 0;
  u32 tile_cnt = 0;
  for (u32 k = 0; k < CL_WAVES; k++) {
    if (k < wave) base += wave_cnt[k];
    tile_cnt += wave_cnt[k];
  }
  if (p.total && !p.offsets && threadIdx.x == 0) *p.total = tile_cnt;  // a single tile: no launch (b)
  const u32 W = p.W, words = cnt * W;  // (at most 256 x 2^16 = 2^24)
  const size_t pitch = size_t(W) + 1;
  const Word* in = p.tmp + first * pitch;
  Word* out = p.dst + base * W;
  const u32 dk = 64 / W, dc = 64 % W;
  u32 k = lane / W, c = lane % W;
  for (u32 f = lane; f < words; f += 64) {
    out[f] = in[list[wave][k] * pitch + c];
    k += dk, c += dc;
    if (c >= W) c -= W, k++;
  }
}

// offs[k] = base + k * W for k < count: the offsets of `count - 1` claims of W elements behind `base` elements, and their end
__global__ __launch_bounds__(256) void claims_arith_offsets_k(u64* offs, u64 base, u64 W, size_t count) {
  const size_t k = blockIdx.x * size_t(256) + threadIdx.x;
  if (k < count) offs[k] = base + k * W;
}

}  // namespace
}  // namespace msamd
