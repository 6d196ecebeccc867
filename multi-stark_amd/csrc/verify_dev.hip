// Kernels of batched verification (verify_dev.h). Two launches per batch:
//   verify_queries_k  one thread per (proof, query): reduced openings, FRI fold chain, final polynomial - the per-query
//                     arithmetic of verifier.hip::pcs_verify restated with the same field functions (gl_dev.h is shared by
//                     host and device, so the results are the same field elements). Writes every FRI round's leaf row.
//   verify_paths_k    one thread per Merkle path (input rounds, FRI rounds, ms_mmcs_verify_batch openings): a dependent
//                     chain of BLAKE3 compressions per thread, wide across threads.
// Every index used here was derived by the host from lengths it had checked; a refused proof contributes no thread.
#include "b3_dev.h"
#include "verify_dev.h"

namespace msamd {

namespace {

constexpr u32 B3_WHOLE = B3_CHUNK_START | B3_CHUNK_END | B3_ROOT;  // a message of one block: what compress2 hashes

__device__ __forceinline__ void b3_pair(const u32 l[8], const u32 r[8], u32 flags, u32 out[8]) {
  u32 m[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    m[i] = l[i];
    m[8 + i] = r[i];
  }
  b3_iv(out);
  b3_compress(out, m, 0, 64, flags);
}

// stack[l] with l only known at run time, without indexing registers: compare-and-select over the (unrolled) levels
__device__ __forceinline__ void stack_get(const u32 (&st)[VB_STACK][8], u32 l, u32 out[8]) {
#pragma unroll
  for (u32 k = 0; k < VB_STACK; k++)
#pragma unroll
    for (int i = 0; i < 8; i++)
      out[i] = (k == 0 || l == k) ? st[k][i] : out[i];
}
__device__ __forceinline__ void stack_put(u32 (&st)[VB_STACK][8], u32 l, const u32 v[8]) {
#pragma unroll
  for (u32 k = 0; k < VB_STACK; k++)
#pragma unroll
    for (int i = 0; i < 8; i++)
      st[k][i] = l == k ? v[i] : st[k][i];
}

// BLAKE3 of n canonical little-endian u64 words (n <= VB_MAX_GROUP_WORDS), chunk tree included. A finished chunk is merged
// with the complete left subtrees of equal size at once (the set bits of the chunk count say which stack levels are full),
// which is what the lazy merge of the specification amounts to as long as more input follows.
__device__ __forceinline__ void hash_words(const u64* w, u32 n, u32 cv[8]) {
  u32 st[VB_STACK][8];
#pragma unroll
  for (u32 k = 0; k < VB_STACK; k++)
#pragma unroll
    for (int i = 0; i < 8; i++) st[k][i] = 0;
  const u32 nchunks = n ? (n + 127) >> 7 : 1;
#pragma unroll 1
  for (u32 c = 0; c < nchunks; c++) {
    b3_iv(cv);
    const u32 cw = n - 128 * c < 128 ? n - 128 * c : 128;  // words of this chunk (0 only for the empty message)
    const u32 nblocks = cw ? (cw + 7) >> 3 : 1;
#pragma unroll 1
    for (u32 b = 0; b < nblocks; b++) {
      const u32 bw = cw - 8 * b < 8 ? cw - 8 * b : 8;
      const u64* src = w + 128 * (size_t)c + 8 * b;
      u32 m[16];
#pragma unroll
      for (u32 k = 0; k < 8; k++) {
        const u64 v = k < bw ? src[k] : 0;
        m[2 * k] = (u32)v;
        m[2 * k + 1] = (u32)(v >> 32);
      }
      u32 flags = b == 0 ? B3_CHUNK_START : 0;
      if (b + 1 == nblocks) flags |= B3_CHUNK_END | (nchunks == 1 ? B3_ROOT : 0);
      b3_compress(cv, m, c, bw * 8, flags);
    }
    if (c + 1 < nchunks) {
      u32 l = 0;
#pragma unroll 1
      while ((c >> l) & 1) {
        u32 left[8], out[8];
        stack_get(st, l, left);
        b3_pair(left, cv, B3_PARENT, out);
#pragma unroll
        for (int i = 0; i < 8; i++) cv[i] = out[i];
        l++;
      }
      stack_put(st, l, cv);
    }
  }
  if (nchunks > 1) {
    const u32 before = nchunks - 1;  // chunks in front of the last one: its set bits are the full stack levels
    const u32 top = 31 - __clz(before);
#pragma unroll 1
    for (u32 l = 0; l <= top; l++) {
      if (!((before >> l) & 1)) continue;
      u32 left[8], out[8];
      stack_get(st, l, left);
      b3_pair(left, cv, B3_PARENT | (l == top ? B3_ROOT : 0), out);
#pragma unroll
      for (int i = 0; i < 8; i++) cv[i] = out[i];
    }
  }
}

__device__ __forceinline__ void load_digest(const Digest* d, u32 out[8]) {
  const uint4* p = reinterpret_cast<const uint4*>(d);  // (the digest section is 64-byte aligned, digests 32 bytes apart)
  const uint4 a = p[0], b = p[1];
  out[0] = a.x, out[1] = a.y, out[2] = a.z, out[3] = a.w;
  out[4] = b.x, out[5] = b.y, out[6] = b.z, out[7] = b.w;
}

__global__ __launch_bounds__(256) void verify_paths_k(GVDev d, u32 n_items) {
  const u32 t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_items) return;
  const VPathItem it = d.items[t];
  const u32* grp = d.u32s + it.grp_off;
  const u64* vals = d.words + it.vals_off;
  u32 root[8];
#pragma unroll
  for (int i = 0; i < 8; i++) root[i] = 0;
#pragma unroll 1
  for (u32 k = 0; k <= it.n_levels; k++) {
    if (k) {
      u32 sib[8], l[8], r[8];
      load_digest(d.digs + it.sib_off + (k - 1), sib);
      const bool right = (it.index >> (k - 1)) & 1;  // this node is the right child
#pragma unroll
      for (int i = 0; i < 8; i++) {
        l[i] = right ? sib[i] : root[i];
        r[i] = right ? root[i] : sib[i];
      }
      b3_pair(l, r, B3_WHOLE, root);
    }
    const u32 g = grp[k];
    if (g) {  // the matrices of this height: the leaf (k = 0), or a group injected as compress2(root, hash(group))
      u32 h[8];
      hash_words(vals, g - 1, h);
      vals += g - 1;
      if (k) {
        u32 out[8];
        b3_pair(root, h, B3_WHOLE, out);
#pragma unroll
        for (int i = 0; i < 8; i++) root[i] = out[i];
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) root[i] = h[i];
      }
    }
  }
  u32 cap[8];
  load_digest(d.digs + it.cap_off + (it.index >> it.n_levels), cap);
  u32 diff = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) diff |= cap[i] ^ root[i];
  if (diff) atomicOr(d.fail + it.flag, 1u);
}

__global__ __launch_bounds__(256) void verify_queries_k(GVDev d, u32 n_queries) {
  const u32 t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_queries) return;
  const GVProofDesc& P = d.proofs[d.qmap[t]];
  const u32 q = t - P.query0;
  const u64* blk = d.words + P.blk_off + (u64)q * P.blk_stride;
  const u64 index = blk[0];
  const u32 log_gmax = P.log_gmax;
  const E2 alpha = P.alpha;
  bool bad = false;
  // reduced openings per LDE height: alpha powers run across the matrices of one height (round -> matrix -> point -> column)
  E2* ro = d.ro + P.ro_off + (u64)q * P.n_heights;
#pragma unroll 1
  for (u32 s = 0; s < P.n_heights; s++) {
    const VHeightDesc H = d.heights[P.height_off + s];
    const u64 rev = bitrev64(index >> (log_gmax - H.lh), H.lh);
    const u64 x = gl_mul(GL_GEN, gl_pow(gl_two_adic_generator(H.lh), rev));
    E2 apow = e2(1), acc = e2(0);
#pragma unroll 1
    for (u32 mi = 0; mi < H.n_mats; mi++) {
      const VMatDesc M = d.mats[H.mat_off + mi];
      const E2* pv = d.ext + M.pv_off;
      const u64* row = blk + M.row_off;
#pragma unroll 1
      for (u32 p = 0; p < M.n_points; p++) {
        const E2 quot = e2_inv(e2_sub(pv[0], e2(x)));
#pragma unroll 1
        for (u32 c = 0; c < M.width; c++) {
          const E2 diff = e2_sub(pv[1 + c], e2(row[c]));
          acc = e2_add(acc, e2_mul(e2_mul(apow, diff), quot));
          apow = e2_mul(apow, alpha);
        }
        pv += 1 + M.width;
      }
    }
    ro[s] = acc;
  }
  u32 n_chain = P.n_heights;
  if (P.zero_slot != ~0u) {  // a height-1 trace gives a constant polynomial: its reduced opening must vanish
    if (!e2_is_zero(ro[P.zero_slot])) bad = true;
    n_chain--;
  }
  E2 folded = ro[0];
  u32 hp = 1, log_height = log_gmax;
  u64 idx = index;
  const E2* sib = d.ext + P.sib_off + (u64)q * P.sib_stride;
  u64* frow = d.words + P.fri_off + (u64)q * P.fri_stride;
#pragma unroll 1
  for (u32 i = 0; i < P.n_rounds; i++) {
    const u32 la = d.u32s[P.arity_off + i];
    const E2 beta = d.ext[P.beta_off + i];
    const u32 log_folded_height = log_height - la;
    E2 next;
    if (la == 1) {
      const u64 pair = idx >> 1;
      const E2 s0 = sib[0];
      const E2 e0 = (idx & 1) ? s0 : folded, e1 = (idx & 1) ? folded : s0;
      frow[0] = e0.c0, frow[1] = e0.c1, frow[2] = e1.c0, frow[3] = e1.c1;
      idx = pair;
      // fold_row: the line through (x0, e0), (-x0, e1) evaluated at beta
      const u64 x0 = gl_pow(gl_two_adic_generator(log_folded_height + 1), bitrev64(idx, log_folded_height));
      const u64 x1 = gl_neg(x0);
      const E2 slope = e2_mul_base(e2_sub(e1, e0), gl_inv(gl_sub(x1, x0)));
      next = e2_add(e0, e2_mul(e2_sub(beta, e2(x0)), slope));
      sib += 1;
      frow += 4;
    } else {
      // barycentric form over the coset x <w>, w of order 2^la (see pcs_verify)
      const u32 m = 1u << la;
      const u32 own = (u32)idx & (m - 1);
      const u64 row = idx >> la;
      idx = row;
      const u64 x = gl_pow(gl_two_adic_generator(log_height), bitrev64(row, log_folded_height));
      const u64 wm = gl_two_adic_generator(la);
      E2 sum = e2(0), at_point = e2(0);
      bool hit = false;
      u32 k = 0;
#pragma unroll 1
      for (u32 j = 0; j < m; j++) {
        const E2 e = j == own ? folded : sib[k++];
        frow[2 * j] = e.c0, frow[2 * j + 1] = e.c1;
        if (hit) continue;
        const u64 h = gl_mul(x, gl_pow(wm, bitrev64(j, la)));
        const E2 dd = e2_sub(beta, e2(h));
        if (e2_is_zero(dd)) {  // beta is one of the row's points
          at_point = e;
          hit = true;
        } else {
          sum = e2_add(sum, e2_mul(e2_mul_base(e, h), e2_inv(dd)));
        }
      }
      if (hit) {
        next = at_point;
      } else {
        const u64 xm = gl_pow(x, m);
        const E2 z = e2_sub(e2_exp_pow2(beta, la), e2(xm));
        next = e2_mul(e2_mul_base(z, gl_inv(gl_mul(xm, (u64)m))), sum);
      }
      sib += m - 1;
      frow += 2 * m;
    }
    folded = next;
    log_height = log_folded_height;
    if (hp < n_chain && d.heights[P.height_off + hp].lh == log_height) {
      folded = e2_add(folded, e2_mul(e2_exp_pow2(beta, la), ro[hp]));  // roll-in factor beta^(2^la)
      hp++;
    }
  }
  const u64 x = gl_pow(gl_two_adic_generator(log_gmax), bitrev64(idx, log_gmax));
  E2 eval = e2(0);
#pragma unroll 1
  for (u32 k = P.n_final; k-- > 0;) eval = e2_add(e2_mul_base(eval, x), d.ext[P.final_off + k]);
  if (!(eval.c0 == folded.c0 && eval.c1 == folded.c1)) bad = true;
  if (bad) atomicOr(d.fail + P.flag, 1u);
}

}  // namespace

void verify_batch_launch(Ctx& ctx, const GVDev& d, size_t n_queries, size_t n_items, double path_bytes) {
  if (n_queries) {
    hipEvent_t ev = ctx.prof_begin(K_OTHER);
    hipLaunchKernelGGL(verify_queries_k, dim3((unsigned)((n_queries + 255) / 256)), dim3(256), 0, ctx.stream, d, (u32)n_queries);
    HIP_CHECK(hipGetLastError());
    ctx.prof_end(K_OTHER, ev, 0.0);
  }
  if (n_items) {
    hipEvent_t ev = ctx.prof_begin(K_COMPRESS);
    hipLaunchKernelGGL(verify_paths_k, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, ctx.stream, d, (u32)n_items);
    HIP_CHECK(hipGetLastError());
    ctx.prof_end(K_COMPRESS, ev, path_bytes);
  }
}

}  // namespace msamd
