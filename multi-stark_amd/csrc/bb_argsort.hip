// The sorting permutation of a circuit's rows for the BabyBear configuration (msbb_witness_argsort; the definition is the
// "sorting permutation" section of include/mstark.h read over p = 2^31 - 2^27 + 1, what differs is listed in
// include/mstark_bb.h). The algorithm is argsort.hip's - a least-significant-digit radix sort over (key, row index) pairs with
// 8-bit digits, the LAST key column first, all histograms in front of the one host wait, digits in which all n rows agree
// skipped, three launches per pass that runs, no atomic to global memory - and the count, offsets and scatter kernels are the
// same text (argsort_dev.h), instantiated here with a 32-bit key word. What the layout and the field change:
//   - the trace is a column-major matrix of Montgomery words with a leading dimension: cell (r, c) is buf[c * ld + r]. The order
//     is that of the CANONICAL integers in [0, p), so every read of a key goes through bb_from_monty, and the keys that are
//     sorted are canonical u32 below 2^31: FOUR digits per key column where the other field has eight. The top digit never
//     exceeds 0x78, which needs no special case;
//   - bas_hist_k, one launch per key column, reads trace[col * ld + r] - contiguous 4-byte loads - and counts the four digit
//     histograms in LDS, 4 x 256 counts, 4 KB per column and workgroup; the launch for the last key column also writes the
//     canonical keys out, which is its extraction;
//   - bas_gather_k pulls an earlier key column out in the current order, keys[t] = bb_from_monty(trace[col * ld + idx[t]]): 4
//     bytes of index read contiguously, a scattered 4-byte load, 4 bytes written;
//   - keys and indices are separate u32 buffers. Bytes per row and pass: the count launch reads the 4-byte key, the scatter reads
//     key and index and writes both, 16 more - 20 bytes, 16 in the first pass of the call (indices are the row numbers and are not
//     read) and 16 in the last pass of a column (its keys are not written); plus 2 x 4 bytes per 16 rows for the counts;
//   - bas_final_k stores Montgomery words: PERM bb_to_monty(idx[t]) at trace[dst * ld + t], contiguous across a wave; RANK
//     bb_to_monty(t) at trace[dst * ld + idx[t]]. Every cell once; heights are at most 2^27 < p, so every row index is a canonical
//     value. The witness holds no lookup values: nothing follows;
//   - temporaries of the call: two key and two index buffers (4 bytes x n each: 16 bytes x n), 1024 bytes per tile for the
//     counts, and 4 KB per key column and workgroup of bas_hist_k (at most 256 workgroups) plus 4 KB per key column for the
//     histograms. The sorting buffers but the first key buffer are taken behind the host wait, and only if a pass runs; all are
//     taken before dst is written.
#include <algorithm>
#include <string>

#include "argsort_dev.h"
#include "bb_host.h"

namespace msbb {

namespace {

using namespace msamd;  // the constants and kernels of argsort_dev.h, K_WITNESS_ARGSORT

constexpr const char* BAS_CALL = "msbb_witness_argsort";
constexpr u32 BAS_DIGITS = 32 / AS_BITS, BAS_HIST = BAS_DIGITS * AS_RADIX;

// col: the key column, n Montgomery words
__global__ __launch_bounds__(AS_THREADS) void bas_hist_k(const u32* col, size_t n, u32 n_tiles, u32* keys_out, u32* slots) {
  __shared__ u32 h[BAS_HIST];
  for (u32 i = threadIdx.x; i < BAS_HIST; i += AS_THREADS) h[i] = 0;
  __syncthreads();
  for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    for (u32 j = 0; j < AS_STEPS; j++) {
      const size_t r = size_t(tile) * AS_TILE + j * AS_THREADS + threadIdx.x;
      const bool valid = r < n;
      const u32 key = valid ? bb_from_monty(col[r]) : 0;
      if (valid && keys_out) keys_out[r] = key;
#pragma unroll
      for (u32 dg = 0; dg < BAS_DIGITS; dg++) as_lds_count(h + dg * AS_RADIX, (key >> (dg * AS_BITS)) & (AS_RADIX - 1), valid);
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < BAS_HIST; i += AS_THREADS) slots[size_t(blockIdx.x) * BAS_HIST + i] = h[i];
}

__global__ __launch_bounds__(AS_THREADS) void bas_gather_k(const u32* col, const u32* idx, size_t n, u32* keys_out) {
  const size_t t = size_t(blockIdx.x) * AS_THREADS + threadIdx.x;
  if (t >= n) return;
  const size_t r = idx ? idx[t] : t;
  if (r < n) keys_out[t] = bb_from_monty(col[r]);
}

// dst: the destination column, n words
__global__ __launch_bounds__(AS_THREADS) void bas_final_k(const u32* idx, size_t n, u32* dst, u32 rank) {
  const size_t t = size_t(blockIdx.x) * AS_THREADS + threadIdx.x;
  if (t >= n) return;
  const size_t i = idx ? idx[t] : t;
  if (i >= n) return;  // (cannot happen: idx is a permutation of the rows)
  if (rank)
    dst[i] = bb_to_monty((u32)t);
  else
    dst[t] = bb_to_monty((u32)i);
}

}  // namespace

void sort_info(u64 out4[4]) { out4[0] = AS_TILE, out4[1] = AS_BITS, out4[2] = AS_OFF_ROUND, out4[3] = AS_MAX_KEYS; }

void witness_argsort(BSystem& sys, BWitness& wit, size_t ci, const uint32_t* key_columns, size_t n_keys, uint32_t dst, uint32_t what,
                     u64 summary[4]) {
  Ctx& ctx = *sys.ctx;
  const std::string name(BAS_CALL);
  auto fail = [&](const std::string& text) -> void { throw std::runtime_error(name + ": " + text); };
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C || wit.traces.size() != C) fail("the witness does not belong to this system");
  if (wit.host_resident) fail("takes a device-resident witness (msbb_witness_create, msbb_witness_create_device)");
  if (ci >= C) fail("circuit " + std::to_string(ci) + " is out of range");
  const size_t n = wit.heights[ci];
  if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
  const BCircuit& c = sys.circuits[ci];
  BMat& tr = wit.traces[ci];
  if (!tr.buf.p || tr.h != n || tr.w != c.main_width || tr.ld < n) fail("the circuit has no trace on this device");
  if (n_keys < 1 || n_keys > AS_MAX_KEYS) fail(std::to_string(n_keys) + " key columns: between 1 and " + std::to_string(AS_MAX_KEYS) + " are taken");
  for (size_t k = 0; k < n_keys; k++) {
    if (key_columns[k] >= c.main_width)
      fail("key column " + std::to_string(key_columns[k]) + " is beyond main_width " + std::to_string(c.main_width));
    if (key_columns[k] == dst) fail("dst column " + std::to_string(dst) + " is among the keys");
  }
  if (dst >= c.main_width) fail("dst column " + std::to_string(dst) + " is beyond main_width " + std::to_string(c.main_width));
  if (what > 1) fail("what = " + std::to_string(what) + " is neither MS_SORT_PERM (0) nor MS_SORT_RANK (1)");
  // (the witness-making calls refuse a trace taller than the two-adicity allows, so no witness reaches this; it is what makes
  // every row index a canonical value)
  if (n > (size_t(1) << BB_TWO_ADICITY)) fail("height " + std::to_string(n) + " is above 2^27");

  const u32 m = (u32)n_keys, n_tiles = (u32)((n + AS_TILE - 1) / AS_TILE), groups = std::min(n_tiles, AS_HIST_GROUPS);
  const unsigned row_blocks = (unsigned)((n + AS_THREADS - 1) / AS_THREADS);

  // every column's digit histograms; the last key column is written out on the way. Then the one host wait
  DBuf<u32> keys_a(ctx, n);
  DBuf<u32> slots(ctx, size_t(m) * groups * BAS_HIST), d_hist(ctx, size_t(m) * BAS_HIST);
  for (u32 k = 0; k < m; k++)
    hipLaunchKernelGGL(bas_hist_k, dim3(groups), dim3(AS_THREADS), 0, ctx.stream, tr.col(key_columns[k]), n, n_tiles, k == m - 1 ? keys_a.p : nullptr,
                       slots.p + size_t(k) * groups * BAS_HIST);
  hipLaunchKernelGGL(as_hist_sum_k<BAS_HIST>, dim3(m * BAS_HIST / AS_THREADS), dim3(AS_THREADS), 0, ctx.stream, slots.p, groups, m * BAS_HIST, d_hist.p);
  HIP_CHECK(hipGetLastError());
  std::vector<u32> hist(size_t(m) * BAS_HIST);
  ctx.d2h(hist.data(), d_hist.p, hist.size() * sizeof(u32));

  // a digit in which all n rows share one value moves nothing
  std::vector<std::vector<u32>> digits(m);
  size_t run = 0;
  for (u32 k = 0; k < m; k++)
    for (u32 dg = 0; dg < BAS_DIGITS; dg++) {
      const u32* h = hist.data() + (size_t(k) * BAS_DIGITS + dg) * AS_RADIX;
      if (std::find(h, h + AS_RADIX, (u32)n) == h + AS_RADIX) digits[k].push_back(dg), run++;
    }
  summary[0] = n, summary[1] = m, summary[2] = run, summary[3] = size_t(m) * BAS_DIGITS - run;

  hipEvent_t ev = ctx.prof_begin(K_WITNESS_ARGSORT);
  DBuf<u32> keys_b, idx_a, idx_b, counts;
  if (run) {
    keys_b = DBuf<u32>(ctx, n);
    idx_a = DBuf<u32>(ctx, n), idx_b = DBuf<u32>(ctx, n);
    counts = DBuf<u32>(ctx, size_t(AS_RADIX) * n_tiles);
  }
  const u32* idx = nullptr;  // the current order (nullptr: row order)
  for (u32 k = m; k-- > 0;) {
    if (digits[k].empty()) continue;
    if (k != m - 1) hipLaunchKernelGGL(bas_gather_k, dim3(row_blocks), dim3(AS_THREADS), 0, ctx.stream, tr.col(key_columns[k]), idx, n, keys_a.p);
    u32 *in = keys_a.p, *out = keys_b.p;
    for (size_t q = 0; q < digits[k].size(); q++) {
      const u32 shift = digits[k][q] * AS_BITS;
      const bool last = q + 1 == digits[k].size();
      u32* idx_out = idx == idx_a.p ? idx_b.p : idx_a.p;
      hipLaunchKernelGGL(as_count_k<u32>, dim3(n_tiles), dim3(AS_THREADS), 0, ctx.stream, in, n, shift, n_tiles, counts.p);
      hipLaunchKernelGGL(as_offsets_k, dim3(1), dim3(AS_OFF_THREADS), 0, ctx.stream, counts.p, size_t(AS_RADIX) * n_tiles);
      hipLaunchKernelGGL(as_scatter_k<u32>, dim3(n_tiles), dim3(AS_THREADS), 0, ctx.stream, in, idx, n, shift, n_tiles, counts.p, last ? nullptr : out, idx_out);
      idx = idx_out;
      std::swap(in, out);
    }
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(bas_final_k, dim3(row_blocks), dim3(AS_THREADS), 0, ctx.stream, idx, n, tr.col(dst), what);
  HIP_CHECK(hipGetLastError());
  ctx.prof_end(K_WITNESS_ARGSORT, ev, double(n) * (20.0 * double(run) + 8.0));
}

}  // namespace msbb
