// The bench workload's witness generated in HBM: build_witness + build_claims of
// /root/reference/benches/multi_stark.rs:171-238 for the system [ByteTable, U32Add]. Row i of the adder is
// (x bytes, y bytes, z = x + y mod 2^32 bytes, carry, 1) with x, y the (i+1)-th states of two xorshift32 streams; the
// byte table's column counts the 12 bytes of every row; claim i = [1, x, y, z]. xorshift32 is linear over GF(2), so a
// thread jumps to the state before its first row with the precomputed powers T^(2^j) of the step matrix and then walks
// its rows - no H2D of the 117 MB trace or the 33 MB of claims for synthetic runs.
#include <algorithm>
#include <array>
#include <cstring>

#include "host.h"

namespace msamd {

namespace {

struct XsJump {
  u32 m[32][32];  // m[j][c] = T^(2^j) e_c
};

__host__ __device__ inline u32 xs_step(u32 a) {
  a ^= a << 13;
  a ^= a >> 17;
  a ^= a << 5;
  return a;
}
__device__ inline u32 xs_apply(const u32* __restrict__ col, u32 v) {
  u32 r = 0;
#pragma unroll
  for (int c = 0; c < 32; c++) r ^= (v >> c) & 1u ? col[c] : 0u;
  return r;
}

constexpr int GEN_ROWS = 16;  // consecutive rows per thread
__global__ __launch_bounds__(256) void u32_add_bench_k(const XsJump* __restrict__ jump, u32 a0, u32 b0, size_t num_adds, size_t height,
                                                       u64* __restrict__ add /* height x 14 */, unsigned long long* __restrict__ byte /* 256 */,
                                                       u64* __restrict__ claims /* num_adds x 4 */) {
  __shared__ unsigned int hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const size_t first = (blockIdx.x * size_t(blockDim.x) + threadIdx.x) * GEN_ROWS;
  u32 a = a0, b = b0;
  for (int j = 0; j < 32; j++)
    if ((first >> j) & 1) {
      a = xs_apply(jump->m[j], a);
      b = xs_apply(jump->m[j], b);
    }
  for (int k = 0; k < GEN_ROWS; k++) {
    const size_t i = first + k;
    if (i >= height) break;
    u64* row = add + i * 14;
    if (i < num_adds) {
      a = xs_step(a);
      b = xs_step(b);
      const u64 s = (u64)a + (u64)b;
      const u32 z = (u32)s;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const u32 xb = (a >> (8 * q)) & 0xff, yb = (b >> (8 * q)) & 0xff, zb = (z >> (8 * q)) & 0xff;
        row[q] = xb;
        row[4 + q] = yb;
        row[8 + q] = zb;
        atomicAdd(&hist[xb], 1u);
        atomicAdd(&hist[yb], 1u);
        atomicAdd(&hist[zb], 1u);
      }
      row[12] = s >> 32;
      row[13] = 1;
      u64* c = claims + i * 4;
      c[0] = 1;
      c[1] = a;
      c[2] = b;
      c[3] = z;
    } else {
#pragma unroll
      for (int q = 0; q < 14; q++) row[q] = 0;  // padding rows (benches/multi_stark.rs:196-199)
    }
  }
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(&byte[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

__global__ void claim_offsets_k(u64* __restrict__ offs, size_t n) {
  const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
  if (i <= n) offs[i] = 4 * i;
}

}  // namespace

std::unique_ptr<HWitness> witness_u32_add_bench(HSystem& sys, size_t num_adds, u32 a0, u32 b0) {
  Ctx& ctx = *sys.ctx;
  HIP_CHECK(hipSetDevice(ctx.device));
  if (sys.circuits.size() != 2 || sys.circuits[0].main_width != 1 || sys.circuits[0].pre_height != 256 || sys.circuits[1].main_width != 14 ||
      sys.circuits[1].pre_width != 0)
    throw std::runtime_error("witness_u32_add_bench: the system is not [ByteTable, U32Add]");
  if (num_adds == 0 || num_adds > (size_t(1) << NTT_MAX_LOG)) throw std::runtime_error("witness_u32_add_bench: bad size");
  size_t height = 1;
  while (height < num_adds) height <<= 1;
  // powers of the step matrix: column c of T^(2^(j+1)) = T^(2^j) applied to column c of T^(2^j)
  std::unique_ptr<XsJump> jump(new XsJump());
  for (int c = 0; c < 32; c++) jump->m[0][c] = xs_step(1u << c);
  for (int j = 1; j < 32; j++)
    for (int c = 0; c < 32; c++) {
      u32 v = jump->m[j - 1][c], r = 0;
      for (int k = 0; k < 32; k++)
        if ((v >> k) & 1u) r ^= jump->m[j - 1][k];
      jump->m[j][c] = r;
    }
  DBuf<XsJump> d_jump(ctx, 1);
  ctx.h2d(d_jump.p, jump.get(), sizeof(XsJump));
  std::vector<DBuf<u64>> traces(2);
  traces[0] = DBuf<u64>(ctx, 256);
  traces[1] = DBuf<u64>(ctx, height * 14);
  DBuf<u64> d_offs(ctx, num_adds + 1), d_data(ctx, num_adds * 4);
  HIP_CHECK(hipMemsetAsync(traces[0].p, 0, 256 * 8, ctx.stream));
  const size_t threads = (height + GEN_ROWS - 1) / GEN_ROWS;
  hipLaunchKernelGGL(u32_add_bench_k, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx.stream, (const XsJump*)d_jump.p, a0, b0,
                     num_adds, height, traces[1].p, reinterpret_cast<unsigned long long*>(traces[0].p), d_data.p);
  hipLaunchKernelGGL(claim_offsets_k, dim3((unsigned)((num_adds + 256) / 256)), dim3(256), 0, ctx.stream, d_offs.p, num_adds);
  HIP_CHECK(hipGetLastError());
  ctx.sync();  // `jump` may go
  return witness_from_device(sys, std::move(traces), {256, height}, std::move(d_offs), std::move(d_data), num_adds, num_adds * 4);
}

// ---------------------------------------------------------------------------------------------------------------------
// The BLAKE3 compression system's witness generated in HBM: Blake3CompressionClaims::witness of
// src/test_circuits/blake3.rs:1511-2213 (blake3_circuit.py::blake3_witness cell for cell) for n claims of the compression
// circuit. With H = n rounded up to a power of two every row of every lower circuit sits at a closed-form index, so the
// reference's work lists are not needed:
//   compression  H x 2625     row c < n real, the rest zero
//   G            64 H x 81    row 56 c + 8 r + j for every compression row (a padding row sends 56 zero tuples: [1, 0..]);
//                             the last 8 H rows zero
//   u32 xor      512 H x 13   16 c + k from the compression rows, then 16 H + 4 g + {d0t, b0t, d1t, b1t} for all 64 H G rows
//   u32 add      512 H x 14   6 g + {a0t, a0, c0, a1t, a1, c1} for all 64 H G rows
//   rotations    64 H         one row per G row
//   byte pairs   65536 x 2    column 0: four byte triples per xor row, column 1: eight pairs per add row, two per rot8 / rot16
//                             row - matrix padding rows included
// b3_compress_k (one wave per compression row) runs the rounds and leaves the 56 G tuples and 16 xor triples of its row in a
// u32 scratch, which is also the argument list of the compression circuit's 73 lookups: the kernel writes that circuit's
// LookupValues itself (its prefix is the one that does not fit the device sweep). b3_expand_k derives 64 G rows per
// workgroup and everything below them. Rows are staged as words in LDS and written with consecutive lanes on consecutive
// cells. Byte-pair counts: global atomics from the rows of real compressions only; rows known to be zero are counted in
// closed form by the host, and hits of bin (0, 0) are summed per workgroup first.
namespace {

constexpr u32 B3_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
constexpr int B3_ROW_WORDS = 656;    // state_in 32 | 56 x (a b c d mx my a1 d1 c1 b1) | 16 x (left right xor) | state_out 16
constexpr int B3_SCRATCH = 608;      // the middle two parts
constexpr int B3_G0 = 32, B3_X0 = 592, B3_OUT0 = 640;
constexpr int B3_COMP_W = 2625, B3_COMP_LOOKUPS = 73, B3_COMP_ARGS = 49 + 56 * 11 + 16 * 4, B3_CLAIM = 49;
constexpr int B3_GROWS = 64;         // G rows per workgroup of b3_expand_k

__host__ __device__ inline u32 b3_byte(u32 x, int i) { return (x >> (8 * i)) & 0xffu; }

// one G application: the 20 words of a G-function row after its multiplicity (:1806-1904)
// a b c d mx my | a0t a0 d0t d0 c0 b0t b0 a1t a1 d1t d1 c1 b1t b1
__host__ __device__ inline void b3_g(const u32 in[6], u32 w[20]) {
  for (int i = 0; i < 6; i++) w[i] = in[i];
  w[6] = in[0] + in[1];
  w[7] = w[6] + in[4];
  w[8] = in[3] ^ w[7];
  w[9] = b3_rotr(w[8], 16);
  w[10] = in[2] + w[9];
  w[11] = in[1] ^ w[10];
  w[12] = b3_rotr(w[11], 12);
  w[13] = w[7] + w[12];
  w[14] = w[13] + in[5];
  w[15] = w[9] ^ w[14];
  w[16] = b3_rotr(w[15], 8);
  w[17] = w[10] + w[16];
  w[18] = w[12] ^ w[17];
  w[19] = b3_rotr(w[18], 7);
}
// the seven rounds on the 32-word state (in place). rec (nullable): 10 words per G application, in the column order of the
// compression circuit (a b c d mx my | a1 d1 c1 b1)
__host__ __device__ inline void b3_rounds(u32* st, u32* rec) {
  constexpr int perm[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  for (int r = 0; r < 7; r++) {
    for (int j = 0; j < 8; j++) {
      const int s = j >> 2, a = j & 3, b = 4 + ((j + s) & 3), c = 8 + ((j + 2 * s) & 3), d = 12 + ((j + 3 * s) & 3);
      const u32 in[6] = {st[a], st[b], st[c], st[d], st[16 + 2 * j], st[17 + 2 * j]};
      u32 w[20];
      b3_g(in, w);
      st[a] = w[14];
      st[b] = w[19];
      st[c] = w[17];
      st[d] = w[16];
      if (rec) {
        for (int i = 0; i < 6; i++) rec[i] = in[i];
        rec[6] = w[14];
        rec[7] = w[16];
        rec[8] = w[17];
        rec[9] = w[19];
        rec += 10;
      }
    }
    if (r < 6) {
      u32 m[16];
#pragma unroll
      for (int i = 0; i < 16; i++) m[i] = st[16 + perm[i]];
#pragma unroll
      for (int i = 0; i < 16; i++) st[16 + i] = m[i];
    }
  }
}

// value of column `col` of a row [multiplicity, words little-endian byte by byte]
__device__ inline u64 b3_cell(const u32* words, int col, u32 multiplicity) {
  return col == 0 ? multiplicity : b3_byte(words[(col - 1) >> 2], (col - 1) & 3);
}
// one more pair (i, j) for column `col` of the byte-pair table; bin 0 is summed per workgroup
__device__ inline void b3_count(unsigned long long* __restrict__ u8, int col, u32 i, u32 j, unsigned& zeros) {
  const u32 bin = 256 * i + j;
  if (bin == 0)
    zeros++;
  else
    atomicAdd(&u8[2 * bin + col], 1ull);
}

// one wave per compression row c < H
__global__ __launch_bounds__(64) void b3_compress_k(const u32* __restrict__ states_in /* n x 32 */, size_t n, u64* __restrict__ comp /* H x 2625 */,
                                                    u64* __restrict__ xor_rows /* first 16 H rows x 13 */, u32* __restrict__ scratch /* H x 608 */,
                                                    u64* __restrict__ claims /* n x 49 */, u32* __restrict__ states_out /* n x 16 */,
                                                    u64* __restrict__ mult /* H x 73 */, u64* __restrict__ args /* H x 729 */,
                                                    unsigned long long* __restrict__ u8 /* 65536 x 2 */) {
  __shared__ u32 w[B3_ROW_WORDS];
  __shared__ u32 st[32];
  __shared__ unsigned zero_hits;
  const size_t c = blockIdx.x;
  const int t = threadIdx.x;
  const bool real = c < n;
  for (int i = t; i < B3_ROW_WORDS; i += 64) w[i] = real && i < 32 ? states_in[c * 32 + i] : 0u;
  if (t == 0) zero_hits = 0;
  __syncthreads();
  if (real && t == 0) {
    for (int i = 0; i < 32; i++) st[i] = w[i];
    b3_rounds(st, w + B3_G0);
    for (int i = 0; i < 8; i++) {  // (:1770-1796) state[i] ^= state[i + 8], then state[i + 8] ^= cv[i]
      u32* x = w + B3_X0 + 6 * i;
      x[0] = st[i];
      x[1] = st[i + 8];
      x[2] = st[i] ^ st[i + 8];
      x[3] = st[i + 8];
      x[4] = w[i];
      x[5] = st[i + 8] ^ w[i];
      w[B3_OUT0 + i] = x[2];
      w[B3_OUT0 + 8 + i] = x[5];
    }
  }
  __syncthreads();
  // the compression row
  u64* row = comp + c * B3_COMP_W;
  for (int k = t; k < B3_COMP_W; k += 64) row[k] = b3_cell(w, k, real);
  for (int i = t; i < B3_SCRATCH; i += 64) scratch[c * B3_SCRATCH + i] = w[B3_G0 + i];
  // its 16 u32-xor rows, and their byte triples
  unsigned zeros = 0;
  for (int e = t; e < 16 * 13; e += 64) {
    const int r = e / 13, col = e % 13;
    const u32* x = w + B3_X0 + 3 * r;
    xor_rows[c * (16 * 13) + e] = b3_cell(x, col, 1);
    if (real && col >= 1 && col <= 4) b3_count(u8, 0, b3_byte(x[0], col - 1), b3_byte(x[1], col - 1), zeros);
  }
  // the circuit's own LookupValues (what host_lookup_values computes from the row): one pull of the claim, 56 pushes to the
  // G-function channel, 16 to the u32-xor channel
  for (int j = t; j < B3_COMP_LOOKUPS; j += 64) mult[c * B3_COMP_LOOKUPS + j] = j == 0 ? (real ? GL_P - 1 : 0) : 1;
  for (int i = t; i < B3_COMP_ARGS; i += 64) {
    u64 v;
    if (i < 49) {
      v = i == 0 ? 9 : i < 33 ? w[i - 1] : w[B3_OUT0 + i - 33];
    } else if (i < 49 + 56 * 11) {
      const int k = (i - 49) / 11, q = (i - 49) % 11;
      v = q == 0 ? 8 : w[B3_G0 + 10 * k + q - 1];
    } else {
      const int k = (i - 49 - 56 * 11) / 4, q = (i - 49 - 56 * 11) % 4;
      v = q == 0 ? 1 : w[B3_X0 + 3 * k + q - 1];
    }
    args[c * B3_COMP_ARGS + i] = v;
  }
  if (real) {
    if (t < B3_CLAIM) claims[c * B3_CLAIM + t] = t == 0 ? 9 : t < 33 ? w[t - 1] : w[B3_OUT0 + t - 33];
    if (t < 16) states_out[c * 16 + t] = w[B3_OUT0 + t];
  }
  if (zeros) atomicAdd(&zero_hits, zeros);
  __syncthreads();
  if (t == 0 && zero_hits) atomicAdd(&u8[0], (unsigned long long)zero_hits);
}

// 64 consecutive G rows per workgroup, and the rows of u32 xor / u32 add / the rotations they send work to
__global__ __launch_bounds__(256) void b3_expand_k(const u32* __restrict__ scratch, size_t n, size_t H, u64* __restrict__ g_tr, u64* __restrict__ xor_tr,
                                                   u64* __restrict__ add_tr, u64* __restrict__ rot8, u64* __restrict__ rot16, u64* __restrict__ rot12,
                                                   u64* __restrict__ rot7, unsigned long long* __restrict__ u8) {
  // operands of the six additions and four xors of a G row, as indices into its 20 words (blake3_witness: the order in which the
  // G-function circuit appends to the work lists)
  constexpr unsigned char ADD[6][3] = {{0, 1, 6}, {6, 4, 7}, {2, 9, 10}, {7, 12, 13}, {13, 5, 14}, {10, 16, 17}};
  constexpr unsigned char XOR[4][3] = {{3, 7, 8}, {1, 10, 11}, {9, 14, 15}, {12, 17, 18}};
  __shared__ u32 w[B3_GROWS][21];
  __shared__ unsigned char live[B3_GROWS], counted[B3_GROWS];
  __shared__ unsigned zero_hits[2];
  const int t = threadIdx.x;
  const size_t g0 = size_t(blockIdx.x) * B3_GROWS;
  if (t < 2) zero_hits[t] = 0;
  if (t < B3_GROWS) {
    const size_t g = g0 + t;
    u32 in[6] = {0, 0, 0, 0, 0, 0}, v[20];
    const bool has_tuple = g < 56 * H;  // the last 8 H rows of G are padding: they send all-zero work
    if (has_tuple) {
      const u32* s = scratch + (g / 56) * B3_SCRATCH + (g % 56) * 10;
      for (int i = 0; i < 6; i++) in[i] = s[i];
    }
    b3_g(in, v);
    for (int i = 0; i < 20; i++) w[t][i] = v[i];
    live[t] = has_tuple;
    counted[t] = has_tuple && g / 56 < n;  // everything else is known to be zero and is counted in closed form
  }
  __syncthreads();
  unsigned z0 = 0, z1 = 0;
  for (int e = t; e < B3_GROWS * 81; e += 256) {
    const int r = e / 81, col = e % 81;
    g_tr[g0 * 81 + e] = b3_cell(w[r], col, live[r]);
  }
  for (int e = t; e < B3_GROWS * 6 * 14; e += 256) {
    const int ar = e / 14, col = e % 14, r = ar / 6, op = ar % 6;
    const u32 x = w[r][ADD[op][0]], y = w[r][ADD[op][1]], z = w[r][ADD[op][2]];
    u64 v;
    if (col < 4) {
      v = b3_byte(x, col);
      if (counted[r]) b3_count(u8, 1, (u32)v, b3_byte(y, col), z1);
    } else if (col < 8) {
      v = b3_byte(y, col - 4);
    } else if (col < 12) {
      v = b3_byte(z, col - 8);
      if (counted[r]) b3_count(u8, 1, (u32)v, 0, z1);
    } else {
      v = col == 12 ? ((u64)x + y) >> 32 : 1;
    }
    add_tr[g0 * (6 * 14) + e] = v;
  }
  for (int e = t; e < B3_GROWS * 4 * 13; e += 256) {
    const int xr = e / 13, col = e % 13, r = xr / 4, op = xr % 4;
    const u32 x = w[r][XOR[op][0]], y = w[r][XOR[op][1]], z = w[r][XOR[op][2]];
    const u32 src = col < 5 ? x : col < 9 ? y : z;
    xor_tr[(16 * H + 4 * g0) * 13 + e] = col == 0 ? 1 : b3_byte(src, (col - 1) & 3);
    if (counted[r] && col >= 1 && col <= 4) b3_count(u8, 0, b3_byte(x, col - 1), b3_byte(y, col - 1), z0);
  }
  for (int e = t; e < B3_GROWS * 9; e += 256) {  // rotations by whole bytes: [1, value, rotated]; byte pairs (0, 2), (1, 3) of the value
    const int r = e / 9, col = e % 9;
    const u32 v16[2] = {w[r][8], w[r][9]}, v8[2] = {w[r][15], w[r][16]};
    rot16[g0 * 9 + e] = b3_cell(v16, col, 1);
    rot8[g0 * 9 + e] = b3_cell(v8, col, 1);
    if (counted[r] && (col == 1 || col == 2)) {
      b3_count(u8, 1, b3_byte(v16[0], col - 1), b3_byte(v16[0], col + 1), z1);
      b3_count(u8, 1, b3_byte(v8[0], col - 1), b3_byte(v8[0], col + 1), z1);
    }
  }
  for (int e = t; e < B3_GROWS * 25; e += 256) {  // by 12 and 7 bits: [1, value, rotated, 2^k, 2^(32-k), value >> k, value mod 2^k]
    const int r = e / 25, col = e % 25;
    const u32 a = w[r][11], b = w[r][18];
    const u32 v12[6] = {a, w[r][12], 1u << 12, 1u << 20, a >> 12, a & 0xfffu}, v7[6] = {b, w[r][19], 1u << 7, 1u << 25, b >> 7, b & 0x7fu};
    rot12[g0 * 25 + e] = b3_cell(v12, col, 1);
    rot7[g0 * 25 + e] = b3_cell(v7, col, 1);
  }
  if (z0) atomicAdd(&zero_hits[0], z0);
  if (z1) atomicAdd(&zero_hits[1], z1);
  __syncthreads();
  if (t < 2 && zero_hits[t]) atomicAdd(&u8[t], (unsigned long long)zero_hits[t]);
}

__global__ void b3_claim_offsets_k(u64* __restrict__ offs, size_t n, u64* __restrict__ u8, u64 zero_triples, u64 zero_pairs) {
  const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
  if (i <= n) offs[i] = B3_CLAIM * i;
  if (i == 0) {  // the byte pairs of every row that is zero whatever the claims are (the table was cleared before)
    u8[0] = zero_triples;
    u8[1] = zero_pairs;
  }
}

}  // namespace

size_t blake3_compression_states(const uint8_t* data, size_t len, u32* states_in, size_t cap_rows, uint8_t* digest32) {
  struct Node {
    u32 cv[8], words[16];
    u64 counter;
    u32 block_len, flags;
  };
  size_t rows = 0;
  auto run = [&](const Node& nd, u32 extra_flags, u32* cv_out) {
    u32 st[32];
    for (int i = 0; i < 8; i++) st[i] = nd.cv[i];
    for (int i = 0; i < 4; i++) st[8 + i] = B3_IV[i];
    st[12] = (u32)nd.counter;
    st[13] = (u32)(nd.counter >> 32);
    st[14] = nd.block_len;
    st[15] = nd.flags | extra_flags;
    for (int i = 0; i < 16; i++) st[16 + i] = nd.words[i];
    if (rows < cap_rows) memcpy(states_in + rows * 32, st, sizeof(st));
    rows++;
    b3_rounds(st, nullptr);
    for (int i = 0; i < 8; i++) cv_out[i] = st[i] ^ st[i + 8];
  };
  auto words_of = [](const uint8_t* p, size_t n, u32* w) {
    uint8_t b[64] = {0};
    if (n) memcpy(b, p, n);
    for (int i = 0; i < 16; i++) w[i] = (u32)b[4 * i] | (u32)b[4 * i + 1] << 8 | (u32)b[4 * i + 2] << 16 | (u32)b[4 * i + 3] << 24;
  };
  auto parent = [](const u32* left, const u32* right) {
    Node p;
    for (int i = 0; i < 8; i++) p.cv[i] = B3_IV[i], p.words[i] = left[i], p.words[8 + i] = right[i];
    p.counter = 0;
    p.block_len = 64;
    p.flags = B3_PARENT;
    return p;
  };
  const size_t n_chunks = len ? (len + 1023) / 1024 : 1;
  std::vector<std::array<u32, 8>> stack;  // chaining values of the complete sub-trees to the left
  Node node;
  for (size_t ci = 0; ci < n_chunks; ci++) {
    const uint8_t* chunk = data + ci * 1024;
    const size_t clen = std::min<size_t>(1024, len - ci * 1024), n_blocks = clen ? (clen + 63) / 64 : 1;
    Node blk;
    for (int i = 0; i < 8; i++) blk.cv[i] = B3_IV[i];
    blk.counter = ci;
    for (size_t bi = 0; bi + 1 < n_blocks; bi++) {
      words_of(chunk + 64 * bi, 64, blk.words);
      blk.block_len = 64;
      blk.flags = bi == 0 ? B3_CHUNK_START : 0;
      u32 cv[8];
      run(blk, 0, cv);
      memcpy(blk.cv, cv, sizeof(cv));
    }
    const size_t last_len = clen - 64 * (n_blocks - 1);
    words_of(chunk + 64 * (n_blocks - 1), last_len, blk.words);
    blk.block_len = (u32)last_len;
    blk.flags = (n_blocks == 1 ? B3_CHUNK_START : 0) | B3_CHUNK_END;
    if (ci + 1 < n_chunks) {  // a complete chunk with input behind it: its chaining value joins the stack of sub-tree roots
      std::array<u32, 8> cv;
      run(blk, 0, cv.data());
      for (size_t total = ci + 1; (total & 1) == 0; total >>= 1) {
        const Node p = parent(stack.back().data(), cv.data());
        stack.pop_back();
        run(p, 0, cv.data());
      }
      stack.push_back(cv);
    } else {
      node = blk;
    }
  }
  while (!stack.empty()) {
    u32 right[8];
    run(node, 0, right);
    node = parent(stack.back().data(), right);
    stack.pop_back();
  }
  node.counter = 0;
  u32 out[8];
  run(node, B3_ROOT, out);
  if (digest32)
    for (int i = 0; i < 8; i++)
      for (int k = 0; k < 4; k++) digest32[4 * i + k] = (uint8_t)(out[i] >> (8 * k));
  return rows;
}

std::unique_ptr<HWitness> witness_blake3_compressions(HSystem& sys, size_t n, const u32* states_in, u32* states_out) {
  Ctx& ctx = *sys.ctx;
  HIP_CHECK(hipSetDevice(ctx.device));
  static const size_t widths[9] = {2, 13, 14, 9, 9, 25, 25, 81, B3_COMP_W}, lookups[9] = {2, 5, 9, 3, 3, 1, 1, 15, B3_COMP_LOOKUPS};
  bool shape = sys.circuits.size() == 9;
  for (size_t ci = 0; ci < 9 && shape; ci++) {
    const HCircuit& c = sys.circuits[ci];
    shape = c.main_width == widths[ci] && c.num_lookups == lookups[ci] && c.pre_width == (ci == 0 ? 3u : 0u);
  }
  if (!shape || sys.circuits[0].pre_height != 65536 || sys.circuits[8].args_width != (size_t)B3_COMP_ARGS)
    throw std::runtime_error("witness_blake3_compressions: the system is not the nine-circuit BLAKE3 compression system");
  if (!states_in) throw std::runtime_error("witness_blake3_compressions: null states_in");
  // the u32 traces are the tallest: 512 H rows. Refused before anything is allocated.
  const u64 lb = sys.params.log_blowup;
  const unsigned max_log = lb >= TW_LOG ? 0 : std::min<unsigned>(NTT_MAX_LOG, TW_LOG - (unsigned)lb);
  if (n == 0 || n > ((size_t(1) << max_log) >> 9)) throw std::runtime_error("witness_blake3_compressions: bad size (no claims, or the u32 traces would exceed the supported height)");
  size_t H = 1;
  while (H < n) H <<= 1;
  const std::vector<size_t> heights = {65536, 512 * H, 512 * H, 64 * H, 64 * H, 64 * H, 64 * H, 64 * H, H};
  std::vector<DBuf<u64>> traces(9);
  for (size_t ci = 0; ci < 9; ci++) traces[ci] = DBuf<u64>(ctx, heights[ci] * widths[ci]);
  std::vector<ReadyLookups> ready(9);
  ready[8].mult = DBuf<u64>(ctx, H * B3_COMP_LOOKUPS);
  ready[8].args = DBuf<u64>(ctx, H * B3_COMP_ARGS);
  DBuf<u32> d_in(ctx, n * 32), d_out(ctx, n * 16), d_scratch(ctx, H * B3_SCRATCH);
  DBuf<u64> d_offs(ctx, n + 1), d_data(ctx, n * B3_CLAIM);
  ctx.h2d(d_in.p, states_in, n * 32 * sizeof(u32));
  // rows no kernel writes: u32 xor beyond 272 H, u32 add beyond 384 H
  HIP_CHECK(hipMemsetAsync(traces[0].p, 0, 65536 * 2 * 8, ctx.stream));
  HIP_CHECK(hipMemsetAsync(traces[1].p + 272 * H * 13, 0, 240 * H * 13 * 8, ctx.stream));
  HIP_CHECK(hipMemsetAsync(traces[2].p + 384 * H * 14, 0, 128 * H * 14 * 8, ctx.stream));
  // Only rows below a real compression fire atomics: 16 + 4 x 56 xor rows, 6 x 56 add rows and 56 rows of rot8 and of rot16 per
  // claim. All other rows of the three matrices hold zero bytes, whatever the claims: four (0, 0, 0) triples per xor row, eight
  // (0, 0) pairs per add row, two per rotation row.
  const u64 zero_triples = 4 * (512 * (u64)H - 240 * (u64)n), zero_pairs = 8 * (512 * (u64)H - 336 * (u64)n) + 2 * 2 * (64 * (u64)H - 56 * (u64)n);
  hipLaunchKernelGGL(b3_claim_offsets_k, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, ctx.stream, d_offs.p, n, traces[0].p, zero_triples, zero_pairs);
  unsigned long long* u8 = reinterpret_cast<unsigned long long*>(traces[0].p);
  hipLaunchKernelGGL(b3_compress_k, dim3((unsigned)H), dim3(64), 0, ctx.stream, (const u32*)d_in.p, n, traces[8].p, traces[1].p, d_scratch.p, d_data.p,
                     d_out.p, ready[8].mult.p, ready[8].args.p, u8);
  hipLaunchKernelGGL(b3_expand_k, dim3((unsigned)H), dim3(256), 0, ctx.stream, (const u32*)d_scratch.p, n, H, traces[7].p, traces[1].p, traces[2].p,
                     traces[3].p, traces[4].p, traces[5].p, traces[6].p, u8);
  HIP_CHECK(hipGetLastError());
  if (states_out)
    ctx.d2h(states_out, d_out.p, n * 16 * sizeof(u32));
  else
    ctx.sync();  // the scratch and the inputs may go
  return witness_from_device(sys, std::move(traces), heights, std::move(d_offs), std::move(d_data), n, n * B3_CLAIM, &ready);
}

}  // namespace msamd
