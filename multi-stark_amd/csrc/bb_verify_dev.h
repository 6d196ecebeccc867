// Device side of batched verification for the BabyBear / Poseidon2 configuration (msbb_verify_batch,
// msbb_mmcs_verify_batch): the BabyBear instance of the flat arrays of verify_batch.h, which the host builds from proofs whose
// shape it has already checked, and the bodies of the two kernels that consume them. No kernel ever sees proof bytes: every
// offset and length is derived from lengths the collector of verify_batch.h has validated. The bodies are __host__ __device__
// like the field functions of bb_dev.h they are written with, so the same text can be run on the host against
// bb_verifier.hip::pcs_verify (one "thread" per call).
#pragma once
#include "bb_dev.h"
#include "verify_batch.h"

namespace msbb {

using BVPathItem = msamd::VPathItem;
using BVMatDesc = msamd::VMatDesc;
using BVHeightDesc = msamd::VHeightDesc;
using BVProofDesc = msamd::VProofDesc<E4>;
// words in Montgomery form, as they stand in the proof
struct BVDev : msamd::VDev<u32, E4, Digest8> {
  const Poseidon2* perm;  // the system's (or the context's) round constants, already in device memory
};
static_assert(sizeof(BVProofDesc) == 112 && std::is_trivially_copyable<BVProofDesc>::value, "BVProofDesc layout");
static_assert(sizeof(BVDev) == 96 && std::is_trivially_copyable<BVDev>::value, "BVDev layout");

#if defined(__HIP_DEVICE_COMPILE__)
#define BBV_FLAG_OR(p, v) atomicOr((p), (v))
#else
#define BBV_FLAG_OR(p, v) (*(p) |= (v))
#endif

BB_HD u32 bbv_bitrev(u32 x, unsigned bits) {  // bits <= 27 (the two-adicity); 0 bits -> 0
  u32 r = 0;
  for (unsigned i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
}

// PaddingFreeSponge<Perm,16,8,8> over n words: the state starts zeroed, every block overwrites its first min(8, remaining)
// words and is permuted; a short last block leaves the tail as it was. The state streams: no bound on n.
BB_HD void bbv_hash_words(const Poseidon2& perm, const u32* w, u32 n, u32 st[16]) {
#pragma unroll
  for (int j = 0; j < 16; j++) st[j] = 0;
#pragma unroll 1
  for (u32 i = 0; i < n; i += 8) {
    const u32 k = n - i < 8 ? n - i : 8;
#pragma unroll
    for (u32 j = 0; j < 8; j++)
      if (j < k) st[j] = w[i + j];
    bb_poseidon2(perm, st);
  }
}

// one Merkle path: bbv_paths_k's thread t
BB_HD void bbv_path_body(const BVDev& d, u32 t) {
  const BVPathItem it = d.items[t];
  const Poseidon2& perm = *d.perm;
  const u32* grp = d.u32s + it.grp_off;
  const u32* vals = d.words + it.vals_off;
  u32 root[8];
#pragma unroll
  for (int i = 0; i < 8; i++) root[i] = 0;
#pragma unroll 1
  for (u32 k = 0; k <= it.n_levels; k++) {
    u32 st[16];
    if (k) {  // TruncatedPermutation<Perm,2,8,16> of (left, right)
      const Digest8 sib = d.digs[it.sib_off + (k - 1)];
      const bool right = (it.index >> (k - 1)) & 1;  // this node is the right child
#pragma unroll
      for (int i = 0; i < 8; i++) {
        st[i] = right ? sib.w[i] : root[i];
        st[8 + i] = right ? root[i] : sib.w[i];
      }
      bb_poseidon2(perm, st);
#pragma unroll
      for (int i = 0; i < 8; i++) root[i] = st[i];
    }
    const u32 g = grp[k];
    if (g) {  // the matrices of this height: the leaf (k = 0), or a group injected as compress(root, hash(group))
      bbv_hash_words(perm, vals, g - 1, st);
      vals += g - 1;
      if (k) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          st[8 + i] = st[i];
          st[i] = root[i];
        }
        bb_poseidon2(perm, st);
      }
#pragma unroll
      for (int i = 0; i < 8; i++) root[i] = st[i];
    }
  }
  const Digest8 cap = d.digs[it.cap_off + (it.index >> it.n_levels)];
  u32 diff = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) diff |= cap.w[i] ^ root[i];
  if (diff) BBV_FLAG_OR(d.fail + it.flag, 1u);
}

// one query of one proof: bbv_queries_k's thread t. The arithmetic of bb_verifier.hip::pcs_verify's query loop.
BB_HD void bbv_query_body(const BVDev& d, u32 t) {
  const BVProofDesc& P = d.proofs[d.qmap[t]];
  const u32 q = t - P.query0;
  const u32* blk = d.words + P.blk_off + (u64)q * P.blk_stride;
  const u32 index = blk[0];
  const u32 log_gmax = P.log_gmax;
  const E4 alpha = P.alpha;
  const u32 gen = bb_to_monty(BB_GENERATOR);
  bool bad = false;
  // reduced openings per LDE height: alpha powers run across the matrices of one height (round -> matrix -> point -> column)
  E4* ro = d.ro + P.ro_off + (u64)q * P.n_heights;
#pragma unroll 1
  for (u32 s = 0; s < P.n_heights; s++) {
    const BVHeightDesc H = d.heights[P.height_off + s];
    const u32 rev = bbv_bitrev(index >> (log_gmax - H.lh), H.lh);
    const u32 x = bb_mul(gen, bb_pow(bb_two_adic_generator(H.lh), rev));
    E4 apow = e4_one(), acc = e4_zero();
#pragma unroll 1
    for (u32 mi = 0; mi < H.n_mats; mi++) {
      const BVMatDesc M = d.mats[H.mat_off + mi];
      const E4* pv = d.ext + M.pv_off;
      const u32* row = blk + M.row_off;
#pragma unroll 1
      for (u32 p = 0; p < M.n_points; p++) {
        E4 den = pv[0];
        den.c[0] = bb_sub(den.c[0], x);
        if (!(den.c[0] | den.c[1] | den.c[2] | den.c[3])) bad = true;  // the opening point lies on the domain: refused
        const E4 quot = e4_inv(den);
#pragma unroll 1
        for (u32 c = 0; c < M.width; c++) {
          E4 diff = pv[1 + c];
          diff.c[0] = bb_sub(diff.c[0], row[c]);
          acc = e4_add(acc, e4_mul(e4_mul(apow, diff), quot));
          apow = e4_mul(apow, alpha);
        }
        pv += 1 + M.width;
      }
    }
    ro[s] = acc;
  }
  u32 n_chain = P.n_heights;
  if (P.zero_slot != ~0u) {  // a height-1 trace gives a constant polynomial: its reduced opening must vanish
    const E4 z = ro[P.zero_slot];
    if (z.c[0] | z.c[1] | z.c[2] | z.c[3]) bad = true;
    n_chain--;
  }
  E4 folded = ro[0];
  u32 hp = 1, log_height = log_gmax;
  u32 idx = index;
  const E4* sib = d.ext + P.sib_off + (u64)q * P.sib_stride;
  u32* frow = d.words + P.fri_off + (u64)q * P.fri_stride;
#pragma unroll 1
  for (u32 i = 0; i < P.n_rounds; i++) {
    const u32 la = d.u32s[P.arity_off + i];
    const E4 beta = d.ext[P.beta_off + i];
    const u32 log_folded_height = log_height - la;
    const u32 m = 1u << la;
    const u32 own = idx & (m - 1);
    const u32 row = idx >> la;
    idx = row;
    E4 next;
    if (la == 1) {
      const E4 s0 = sib[0];
      const E4 e0 = own ? s0 : folded, e1 = own ? folded : s0;
#pragma unroll
      for (int k = 0; k < 4; k++) frow[k] = e0.c[k], frow[4 + k] = e1.c[k];
      // fold_row: the line through (x0, e0), (-x0, e1) evaluated at beta; x0 = w^bitrev(idx) on the subgroup
      const u32 x0 = bb_pow(bb_two_adic_generator(log_folded_height + 1), bbv_bitrev(idx, log_folded_height));
      const u32 x1 = bb_neg(x0);
      const E4 slope = e4_mul_base(e4_sub(e1, e0), bb_inv(bb_sub(x1, x0)));
      E4 bx = beta;
      bx.c[0] = bb_sub(bx.c[0], x0);
      next = e4_add(e0, e4_mul(bx, slope));
    } else {
      // barycentric form over the coset x <w>, w of order 2^la (see pcs_verify)
      const u32 x = bb_pow(bb_two_adic_generator(log_height), bbv_bitrev(row, log_folded_height));
      const u32 wm = bb_two_adic_generator(la);
      E4 sum = e4_zero(), at_point = e4_zero();
      bool hit = false;
      u32 k = 0;
#pragma unroll 1
      for (u32 j = 0; j < m; j++) {
        const E4 e = j == own ? folded : sib[k++];
#pragma unroll
        for (int c = 0; c < 4; c++) frow[4 * j + c] = e.c[c];
        if (hit) continue;
        const u32 h = bb_mul(x, bb_pow(wm, bbv_bitrev(j, la)));
        E4 dd = beta;
        dd.c[0] = bb_sub(dd.c[0], h);
        if (!(dd.c[0] | dd.c[1] | dd.c[2] | dd.c[3])) {  // beta is one of the row's points
          at_point = e;
          hit = true;
        } else {
          sum = e4_add(sum, e4_mul(e4_mul_base(e, h), e4_inv(dd)));
        }
      }
      if (hit) {
        next = at_point;
      } else {
        const u32 xm = bb_pow(x, m);
        E4 z = e4_exp_pow2(beta, la);
        z.c[0] = bb_sub(z.c[0], xm);
        next = e4_mul(e4_mul_base(z, bb_inv(bb_mul(xm, bb_to_monty(m)))), sum);
      }
    }
    sib += m - 1;
    frow += 4 * m;
    folded = next;
    log_height = log_folded_height;
    if (hp < n_chain && d.heights[P.height_off + hp].lh == log_height) {
      folded = e4_add(folded, e4_mul(e4_exp_pow2(beta, la), ro[hp]));  // roll-in factor beta^(2^la)
      hp++;
    }
  }
  const u32 x = bb_pow(bb_two_adic_generator(log_gmax), bbv_bitrev(idx, log_gmax));
  E4 eval = e4_zero();
#pragma unroll 1
  for (u32 k = P.n_final; k-- > 0;) eval = e4_add(e4_mul_base(eval, x), d.ext[P.final_off + k]);
  if (!e4_eq(eval, folded)) bad = true;
  if (bad) BBV_FLAG_OR(d.fail + P.flag, 1u);
}

}  // namespace msbb
