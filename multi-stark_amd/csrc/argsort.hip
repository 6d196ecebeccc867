// The sorting permutation of a circuit's rows, made on the device (ms_witness_argsort; the definition is in include/mstark.h): row i
// comes before row j iff (trace[i][k_0], .., trace[i][k_{m-1}], i) is lexicographically smaller, cells compared as unsigned 64-bit
// integers. The row index is the last component, so the order is total and the result unique: a stable sort. Main column dst
// receives the permutation (MS_SORT_PERM: the row at sorted position t) or its inverse (MS_SORT_RANK: the position of row r).
//
// A least-significant-digit radix sort over (key, row index) pairs, 8-bit digits, the LAST key column first; row indices are u32
// (heights up to 2^31). All launches go to the context's stream and launches order the phases: no workgroup waits for another
// inside a kernel, and there is no atomic to global memory. LDS atomics only add up plain counts; every position a pair is stored
// at is a function of the input alone.
//   Histograms (in front of the host wait). as_hist_k, one launch per key column: workgroups walk tiles of T = 4096 rows, read the
// column out of the row-major trace at a stride of main_width words and count all eight digit histograms in LDS (a wave whose 64
// rows share a digit adds once); each workgroup leaves its 8 x 256 counts in a slot of its own. The launch for the last key
// column - the one sorted first, in row order - also writes the column out contiguously: its extraction. as_hist_sum_k, one
// launch for all columns, adds the slots up. A histogram does not depend on the order of the rows, which is why all of them can be
// taken before anything is sorted, and the host reads them in ONE copy: the call's one host wait. The host skips every digit in
// which all n rows share one value: a byte-valued column costs one pass, a 20-bit address three, a constant column none.
//   Extraction. For every other key column with a digit to sort, as_gather_k pulls the column out in the current order,
// keys[t] = trace[idx[t]][k] (8 bytes read at a stride, 4 + 8 contiguous).
//   A digit pass that runs: three launches.
//     (a) as_count_k    one workgroup per tile: the tile's digit counts into the digit-major array counts[digit * tiles + tile]
//     (b) as_offsets_k  ONE workgroup of 1024 threads turns the 256 x tiles counts into exclusive offsets in place, R = 4096 counts
//                       per round with a carry from round to round (ms_sort_info tells T and R)
//     (c) as_scatter_k  one workgroup per tile recomputes the stable local ranks and stores each pair once. The tile is walked in
//                       16 steps of 256 consecutive rows, a wave taking 64 of them: 64 (step, wave) slots in row order. Inside a
//                       wave the rank is found by matching digits with eight ballots - the mask of the lanes with an equal digit,
//                       then the popcount of the lanes below; the lowest lane of each mask leaves its popcount in the LDS table
//                       [slot][digit] (16-bit entries, 32 KB). Thread d then runs along digit d's 64 slots in slot order, which
//                       joins the waves' counts in wave order; position = offset of (digit, tile) + slot prefix + rank in the wave.
//   Bytes per row and pass: (a) reads the 8-byte key; (c) reads key and index and writes them, 24 more - 32 bytes, 28 in the first
// pass of the call (indices are the row numbers and are not read) and 24 in the last pass of a column (its keys are not needed
// again and are not written); plus 2 x 4 bytes per 16 rows for the counts.
//   Final. as_final_k writes dst - trace[t][dst] = idx[t], or trace[idx[t]][dst] = t - 4 bytes read, 8 written at a stride, each
// cell once. Held lookup values of the circuit are recomputed behind it, as ms_witness_fill does.
//   Temporaries of the call: two key buffers (8 bytes x n each) and two index buffers (4 bytes x n each), 1024 bytes per tile for
// the counts, and 8 KB per key column and workgroup of as_hist_k (at most 256 workgroups) plus 8 KB per key column for the
// histograms. The sorting buffers but the first key buffer are taken behind the host wait, and only if a pass runs.
#include <algorithm>

#include "argsort_dev.h"
#include "host.h"
#include "program.h"

namespace msamd {
namespace {

// (the constants, as_lds_count, as_hist_sum_k, as_count_k, as_offsets_k and as_scatter_k are argsort_dev.h's, shared with
// bb_argsort.hip; the key word here is the u64 cell as it lies in the trace)
constexpr const char* AS_CALL = "ms_witness_argsort";
constexpr u32 AS_DIGITS = 64 / AS_BITS, AS_HIST = AS_DIGITS * AS_RADIX;

__global__ __launch_bounds__(AS_THREADS) void as_hist_k(const u64* trace, u32 main_w, u32 col, size_t n, u32 n_tiles, u64* keys_out, u32* slots) {
  __shared__ u32 h[AS_HIST];
  for (u32 i = threadIdx.x; i < AS_HIST; i += AS_THREADS) h[i] = 0;
  __syncthreads();
  for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    for (u32 j = 0; j < AS_STEPS; j++) {
      const size_t r = size_t(tile) * AS_TILE + j * AS_THREADS + threadIdx.x;
      const bool valid = r < n;
      const u64 key = valid ? trace[r * main_w + col] : 0;
      if (valid && keys_out) keys_out[r] = key;
#pragma unroll
      for (u32 dg = 0; dg < AS_DIGITS; dg++) as_lds_count(h + dg * AS_RADIX, (u32)(key >> (dg * AS_BITS)) & (AS_RADIX - 1), valid);
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < AS_HIST; i += AS_THREADS) slots[size_t(blockIdx.x) * AS_HIST + i] = h[i];
}

__global__ __launch_bounds__(AS_THREADS) void as_gather_k(const u64* trace, u32 main_w, u32 col, const u32* idx, size_t n, u64* keys_out) {
  const size_t t = size_t(blockIdx.x) * AS_THREADS + threadIdx.x;
  if (t >= n) return;
  const size_t r = idx ? idx[t] : t;
  if (r < n) keys_out[t] = trace[r * main_w + col];
}

__global__ __launch_bounds__(AS_THREADS) void as_final_k(const u32* idx, size_t n, u64* trace, u32 main_w, u32 dst, u32 rank) {
  const size_t t = size_t(blockIdx.x) * AS_THREADS + threadIdx.x;
  if (t >= n) return;
  const size_t i = idx ? idx[t] : t;
  if (i >= n) return;  // (cannot happen: idx is a permutation of the rows)
  if (rank)
    trace[i * main_w + dst] = t;
  else
    trace[t * main_w + dst] = i;
}

}  // namespace

void sort_info(u64 out4[4]) { out4[0] = AS_TILE, out4[1] = AS_BITS, out4[2] = AS_OFF_ROUND, out4[3] = AS_MAX_KEYS; }

void witness_argsort(HSystem& sys, HWitness& wit, size_t ci, const uint32_t* key_columns, size_t n_keys, uint32_t dst, uint32_t what,
                     u64 summary[4]) {
  Ctx& ctx = *sys.ctx;
  const std::string name(AS_CALL);
  auto fail = [&](const std::string& text) -> void { throw std::runtime_error(name + ": " + text); };
  const size_t C = sys.circuits.size();
  if (wit.sys != &sys || wit.heights.size() != C) fail("the witness does not belong to this system");
  if (wit.host_resident) fail("takes a device-resident witness (ms_witness_create, ms_witness_create_device, the generators)");
  if (wit.has_remote) fail("this witness lacks traces that another rank computes");
  if (ci >= C) fail("circuit " + std::to_string(ci) + " is out of range");
  const size_t n = wit.heights[ci];
  if (!n) fail("circuit " + std::to_string(ci) + " is inactive (height 0)");
  if (!wit.traces[ci].p) fail("the circuit has no trace on this device");
  const HCircuit& c = sys.circuits[ci];
  if (n_keys < 1 || n_keys > AS_MAX_KEYS) fail(std::to_string(n_keys) + " key columns: between 1 and " + std::to_string(AS_MAX_KEYS) + " are taken");
  for (size_t k = 0; k < n_keys; k++) {
    if (key_columns[k] >= c.main_width)
      fail("key column " + std::to_string(key_columns[k]) + " is beyond main_width " + std::to_string(c.main_width));
    if (key_columns[k] == dst) fail("dst column " + std::to_string(dst) + " is among the keys");
  }
  if (dst >= c.main_width) fail("dst column " + std::to_string(dst) + " is beyond main_width " + std::to_string(c.main_width));
  if (what > 1) fail("what = " + std::to_string(what) + " is neither MS_SORT_PERM (0) nor MS_SORT_RANK (1)");
  if (n > (size_t(1) << 31)) fail("height " + std::to_string(n) + " is above 2^31");
  DLookups& lk = wit.lookups[ci];
  const bool held = lk.mult.p != nullptr;
  if (held && (!c.prefix_on_device || c.prefix_prog.n_slots * 64 * 8 > 64 * 1024))
    fail("the witness holds lookup values for circuit " + std::to_string(ci) + " and its lookup prefix does not fit the device sweep");

  const u32 W = (u32)c.main_width, m = (u32)n_keys, n_tiles = (u32)((n + AS_TILE - 1) / AS_TILE), groups = std::min(n_tiles, AS_HIST_GROUPS);
  const unsigned row_blocks = (unsigned)((n + AS_THREADS - 1) / AS_THREADS);
  u64* trace = wit.traces[ci].p;

  // every column's digit histograms; the last key column is written out on the way. Then the one host wait
  DBuf<u64> keys_a(ctx, n);
  DBuf<u32> slots(ctx, size_t(m) * groups * AS_HIST), d_hist(ctx, size_t(m) * AS_HIST);
  for (u32 k = 0; k < m; k++)
    hipLaunchKernelGGL(as_hist_k, dim3(groups), dim3(AS_THREADS), 0, ctx.stream, trace, W, key_columns[k], n, n_tiles, k == m - 1 ? keys_a.p : nullptr,
                       slots.p + size_t(k) * groups * AS_HIST);
  hipLaunchKernelGGL(as_hist_sum_k<AS_HIST>, dim3(m * AS_HIST / AS_THREADS), dim3(AS_THREADS), 0, ctx.stream, slots.p, groups, m * AS_HIST, d_hist.p);
  HIP_CHECK(hipGetLastError());
  std::vector<u32> hist(size_t(m) * AS_HIST);
  ctx.d2h(hist.data(), d_hist.p, hist.size() * sizeof(u32));

  // a digit in which all n rows share one value moves nothing
  std::vector<std::vector<u32>> digits(m);
  size_t run = 0;
  for (u32 k = 0; k < m; k++)
    for (u32 dg = 0; dg < AS_DIGITS; dg++) {
      const u32* h = hist.data() + (size_t(k) * AS_DIGITS + dg) * AS_RADIX;
      if (std::find(h, h + AS_RADIX, (u32)n) == h + AS_RADIX) digits[k].push_back(dg), run++;
    }
  summary[0] = n, summary[1] = m, summary[2] = run, summary[3] = size_t(m) * AS_DIGITS - run;

  hipEvent_t ev = ctx.prof_begin(K_WITNESS_ARGSORT);
  DBuf<u64> keys_b;
  DBuf<u32> idx_a, idx_b, counts;
  if (run) {
    keys_b = DBuf<u64>(ctx, n);
    idx_a = DBuf<u32>(ctx, n), idx_b = DBuf<u32>(ctx, n);
    counts = DBuf<u32>(ctx, size_t(AS_RADIX) * n_tiles);
  }
  const u32* idx = nullptr;  // the current order (nullptr: row order)
  for (u32 k = m; k-- > 0;) {
    if (digits[k].empty()) continue;
    if (k != m - 1) hipLaunchKernelGGL(as_gather_k, dim3(row_blocks), dim3(AS_THREADS), 0, ctx.stream, trace, W, key_columns[k], idx, n, keys_a.p);
    u64 *in = keys_a.p, *out = keys_b.p;
    for (size_t q = 0; q < digits[k].size(); q++) {
      const u32 shift = digits[k][q] * AS_BITS;
      const bool last = q + 1 == digits[k].size();
      u32* idx_out = idx == idx_a.p ? idx_b.p : idx_a.p;
      hipLaunchKernelGGL(as_count_k<u64>, dim3(n_tiles), dim3(AS_THREADS), 0, ctx.stream, in, n, shift, n_tiles, counts.p);
      hipLaunchKernelGGL(as_offsets_k, dim3(1), dim3(AS_OFF_THREADS), 0, ctx.stream, counts.p, size_t(AS_RADIX) * n_tiles);
      hipLaunchKernelGGL(as_scatter_k<u64>, dim3(n_tiles), dim3(AS_THREADS), 0, ctx.stream, in, idx, n, shift, n_tiles, counts.p, last ? nullptr : out, idx_out);
      idx = idx_out;
      std::swap(in, out);
    }
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(as_final_k, dim3(row_blocks), dim3(AS_THREADS), 0, ctx.stream, idx, n, trace, W, dst, what);
  HIP_CHECK(hipGetLastError());
  ctx.prof_end(K_WITNESS_ARGSORT, ev, double(n) * (32.0 * double(run) + 12.0));
  // SystemWitness::from_stage_1 again for the values the witness holds (checked above: the sweep fits)
  if (held && !lookup_values_device(ctx, c.prefix_prog, trace, c.pre_width ? c.d_preprocessed.p : nullptr, n, c.main_width, c.pre_width, c.args_width,
                                    lk.mult.p, lk.args.p))
    fail("internal error (the lookup prefix was found to fit and does not)");
}

}  // namespace msamd
