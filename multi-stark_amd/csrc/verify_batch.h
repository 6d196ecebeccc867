// Batched verification, the half that is the same text in both fields (ms_verify_batch / ms_mmcs_verify_batch in
// verifier.hip, msbb_verify_batch / msbb_mmcs_verify_batch in bb_verifier.hip): the flat arrays the device reads, the host
// collector that fills them, and the flush loop. A field describes itself by a plain traits struct F:
//   using Word / Ext / Dig      base-field word, extension element, digest
//   using Dev                   the kernels' argument: VDev<Word, Ext, Dig>, with the field's own tail members already set
//   ext_words, two_adicity      words per extension element; the largest log2 of a subgroup order
//   max_group_words             how many words of one height the path kernel hashes into one leaf or injected group
//   unopened_width_mismatch     what a matrix opened at no point, with another row width in a later query, means (COLLECT_*)
//   launch(ctx, dev, n_queries, n_items, path_bytes)
// and, for the flush loop, the host side of one proof: Prepared (constructed from the system), prepare, fri, pcs_verify, ood.
//
// The host keeps what is serial or cheap - parsing, verify_shape, the transcript replay, both proof-of-work checks, the query
// indices, the arity schedule and the out-of-domain check - and makes EVERY structural check of pcs_verify before a value is
// read. What remains per query (reduced openings, fold chain, final polynomial) and per Merkle path goes to the device as flat
// arrays whose offsets all come from the lengths validated here; a proof refused on the host adds nothing to them.
#pragma once
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <type_traits>
#include <vector>

#include "msamd.h"

namespace msamd {

// the VerificationError variants of the reference (src/verifier.rs:176-192) as include/mstark.h numbers them
enum : int { V_OK = 0, V_INVALID_OPENING = 2, V_INVALID_SHAPE = 3, V_INVALID_SYSTEM = 4, V_OOD_MISMATCH = 5, V_UNBALANCED = 6 };

// ---------------------------------------------------------------- what the kernels read
// MerkleTreeMmcs::verify_batch of one opening. The rows lie in walk order (stable sort by descending height) at
// words[vals_off ..); u32s[grp_off + k], k = 0 .. n_levels, is 1 + the word count of the matrices whose height is
// max_height >> k (0: none at that level; entry 0 is the leaf and always present).
struct VPathItem {
  u64 vals_off, index;
  u32 sib_off;   // digs: n_levels siblings, bottom-up
  u32 cap_off;   // digs: the cap; entry index >> n_levels is compared
  u32 grp_off, n_levels;
  u32 flag;      // fail[flag] |= 1 when the opening is refused
  u32 fri_row;   // host side only: vals_off counts from the FRI leaf rows (resolved by vbatch_seal before the upload)
};

struct VMatDesc {
  u32 row_off;   // words from the query's block to this matrix's opened row
  u32 width, n_points;
  u32 pv_off;    // ext: per point its z, then `width` claimed values
};
struct VHeightDesc {
  u32 lh;        // log2 of the LDE height
  u32 mat_off, n_mats;  // mats: the matrices of this height in round -> matrix order
  u32 pad;
};
// one proof's query arithmetic; every query of the proof is one thread
template <class Ext>
struct VProofDesc {
  Ext alpha;
  u64 blk_off, blk_stride;  // words: per query its index, then the opened input rows
  u64 fri_off, fri_stride;  // words: per query the FRI leaf rows, written by the arithmetic kernel for the path kernel
  u64 ro_off;               // ro: per query n_heights reduced openings (scratch of the arithmetic kernel)
  u32 sib_off, sib_stride;  // ext: per query the FRI sibling values of all rounds
  u32 beta_off;             // ext: one beta per round
  u32 final_off, n_final;   // ext: the final polynomial
  u32 arity_off;            // u32s: log_arity per round
  u32 height_off, n_heights;  // heights, descending; the first is log_gmax
  u32 zero_slot;            // the height whose reduced opening must vanish (always the last one), or ~0
  u32 n_rounds, log_gmax, query0, flag;
};

template <class Word, class Ext, class Dig>
struct VDev {
  const VPathItem* items;
  const VProofDesc<Ext>* proofs;
  const VMatDesc* mats;
  const VHeightDesc* heights;
  const u32* u32s;
  const u32* qmap;     // global query -> proof descriptor
  const Ext* ext;
  const Dig* digs;
  u32* fail;
  Word* words;         // uploaded words as they stand in the proof, then the FRI leaf rows
  Ext* ro;
};

// the layouts the kernels were compiled against: a change here is a change of the kernel arguments and of every upload
static_assert(sizeof(VPathItem) == 40 && std::is_trivially_copyable<VPathItem>::value, "VPathItem layout");
static_assert(sizeof(VMatDesc) == 16 && std::is_trivially_copyable<VMatDesc>::value, "VMatDesc layout");
static_assert(sizeof(VHeightDesc) == 16 && std::is_trivially_copyable<VHeightDesc>::value, "VHeightDesc layout");

// ---------------------------------------------------------------- the host collector
struct Dim {
  size_t w, h;
};

enum { PLAN_OK = 0, PLAN_REFUSED, PLAN_TOO_WIDE };
struct PathPlan {
  std::vector<size_t> order;  // the matrices in walk order: stable by descending height
  std::vector<u32> groups;    // per level 0 .. path_len: 1 + words of the matrices of height max >> level, 0 = none
  unsigned log_max = 0;
};
// everything mmcs_verify_batch refuses without hashing (PLAN_REFUSED), and the walk order of what it would hash; PLAN_TOO_WIDE
// where the path kernel could not hash what it accepts
template <class F>
int mmcs_plan(const std::vector<Dim>& dims, size_t capn, size_t path_len, PathPlan& pl) {
  if (dims.empty()) return PLAN_REFUSED;
  pl.order.resize(dims.size());
  for (size_t i = 0; i < dims.size(); i++) {
    pl.order[i] = i;
    if (dims[i].h == 0 || (dims[i].h & (dims[i].h - 1))) return PLAN_REFUSED;
  }
  std::stable_sort(pl.order.begin(), pl.order.end(), [&](size_t a, size_t b) { return dims[a].h > dims[b].h; });
  pl.log_max = log2_strict(dims[pl.order[0]].h);
  if (capn == 0 || (capn & (capn - 1))) return PLAN_REFUSED;
  const unsigned ch = log2_strict(capn);
  if (ch > pl.log_max || path_len != pl.log_max - ch) return PLAN_REFUSED;
  std::vector<u64> gw(path_len + 1, 0);
  std::vector<uint8_t> present(path_len + 1, 0);
  for (size_t i : pl.order) {
    const size_t k = pl.log_max - log2_strict(dims[i].h);
    if (k > path_len) return PLAN_REFUSED;  // shorter than the cap layer: never injected (pos != order.size())
    gw[k] += dims[i].w;
    present[k] = 1;
  }
  pl.groups.assign(path_len + 1, 0);
  for (size_t k = 0; k <= path_len; k++) {
    if (gw[k] > F::max_group_words) return PLAN_TOO_WIDE;
    if (present[k]) pl.groups[k] = 1 + (u32)gw[k];
  }
  return PLAN_OK;
}

template <class F>
struct VBatch {
  using Word = typename F::Word;
  using Ext = typename F::Ext;
  using Dig = typename F::Dig;
  std::vector<Word> words;
  std::vector<Ext> ext;
  std::vector<Dig> digs;
  std::vector<u32> u32s, qmap;
  std::vector<VPathItem> items;
  std::vector<VProofDesc<Ext>> proofs;
  std::vector<VMatDesc> mats;
  std::vector<VHeightDesc> heights;
  size_t n_flags = 0, fri_words = 0, ro_count = 0;
  double path_bytes = 0;
  size_t bytes() const {
    return (words.size() + fri_words) * sizeof(Word) + (ext.size() + ro_count) * sizeof(Ext) + digs.size() * sizeof(Dig) +
           (u32s.size() + qmap.size()) * 4 + items.size() * sizeof(VPathItem);
  }
};
static const size_t VB_FLUSH_BYTES = size_t(256) << 20;  // a batch larger than this goes to the device in several parts

// the FRI leaf rows live behind the uploaded words: settle the offsets that count from them
template <class F>
void vbatch_seal(VBatch<F>& B) {
  for (auto& it : B.items)
    if (it.fri_row) {
      it.vals_off += B.words.size();
      it.fri_row = 0;
    }
  for (auto& p : B.proofs) p.fri_off += B.words.size();
}

template <class T>
size_t vb_place(size_t& off, size_t count) {
  off = (off + 63) & ~size_t(63);
  const size_t at = off;
  off += count * sizeof(T);
  return at;
}

// upload, two launches, one read-back: fail[flag] != 0 where a device check of that flag's owner failed. `d` arrives with the
// field's own members set; the array pointers are filled in here.
template <class F>
void vbatch_run(Ctx& ctx, typename F::Dev d, VBatch<F>& B, std::vector<u32>& fail) {
  using Word = typename F::Word;
  using Ext = typename F::Ext;
  using Dig = typename F::Dig;
  using Proof = VProofDesc<Ext>;
  fail.assign(B.n_flags, 0);
  if (B.items.empty() && B.qmap.empty()) return;
  vbatch_seal(B);
  size_t off = 0;
  const size_t at_items = vb_place<VPathItem>(off, B.items.size()), at_proofs = vb_place<Proof>(off, B.proofs.size());
  const size_t at_mats = vb_place<VMatDesc>(off, B.mats.size()), at_heights = vb_place<VHeightDesc>(off, B.heights.size());
  const size_t at_u32s = vb_place<u32>(off, B.u32s.size()), at_qmap = vb_place<u32>(off, B.qmap.size());
  const size_t at_ext = vb_place<Ext>(off, B.ext.size()), at_digs = vb_place<Dig>(off, B.digs.size());
  const size_t at_fail = vb_place<u32>(off, B.n_flags), at_words = vb_place<Word>(off, B.words.size());
  const size_t up = off;
  off += B.fri_words * sizeof(Word);
  const size_t at_ro = vb_place<Ext>(off, B.ro_count);
  size_t total = 4096;
  while (total < off) total <<= 1;  // few distinct sizes: the context's pool keeps blocks by exact size
  if (ctx.verify_stage_cap < up) {
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    if (ctx.verify_stage) (void)hipHostFree(ctx.verify_stage);
    ctx.verify_stage = nullptr;
    ctx.verify_stage_cap = 0;
    size_t cap = size_t(1) << 20;
    while (cap < up) cap <<= 1;
    HIP_CHECK(hipHostMalloc((void**)&ctx.verify_stage, cap, hipHostMallocDefault));
    ctx.verify_stage_cap = cap;
  }
  uint8_t* st = ctx.verify_stage;
  auto put = [&](size_t at, const void* src, size_t n) {
    if (n) memcpy(st + at, src, n);
  };
  put(at_items, B.items.data(), B.items.size() * sizeof(VPathItem));
  put(at_proofs, B.proofs.data(), B.proofs.size() * sizeof(Proof));
  put(at_mats, B.mats.data(), B.mats.size() * sizeof(VMatDesc));
  put(at_heights, B.heights.data(), B.heights.size() * sizeof(VHeightDesc));
  put(at_u32s, B.u32s.data(), B.u32s.size() * 4);
  put(at_qmap, B.qmap.data(), B.qmap.size() * 4);
  put(at_ext, B.ext.data(), B.ext.size() * sizeof(Ext));
  put(at_digs, B.digs.data(), B.digs.size() * sizeof(Dig));
  memset(st + at_fail, 0, B.n_flags * 4);
  put(at_words, B.words.data(), B.words.size() * sizeof(Word));
  DBuf<uint8_t> dev(ctx, total);
  HIP_CHECK(hipMemcpyAsync(dev.p, st, up, hipMemcpyHostToDevice, ctx.stream));
  d.items = (const VPathItem*)(dev.p + at_items);
  d.proofs = (const Proof*)(dev.p + at_proofs);
  d.mats = (const VMatDesc*)(dev.p + at_mats);
  d.heights = (const VHeightDesc*)(dev.p + at_heights);
  d.u32s = (const u32*)(dev.p + at_u32s);
  d.qmap = (const u32*)(dev.p + at_qmap);
  d.ext = (const Ext*)(dev.p + at_ext);
  d.digs = (const Dig*)(dev.p + at_digs);
  d.fail = (u32*)(dev.p + at_fail);
  d.words = (Word*)(dev.p + at_words);
  d.ro = (Ext*)(dev.p + at_ro);
  F::launch(ctx, d, B.qmap.size(), B.items.size(), B.path_bytes);
  ctx.d2h(fail.data(), d.fail, B.n_flags * 4);  // the call's one host wait (the staging buffer is free again after it)
}

template <class F>
void vb_add_item(VBatch<F>& B, const PathPlan& pl, u64 vals_off, bool fri_row, u64 index, u32 sib_off, u32 cap_off, u32 grp_off, u32 flag) {
  VPathItem it;
  it.vals_off = vals_off;
  it.index = index;
  it.sib_off = sib_off;
  it.cap_off = cap_off;
  it.grp_off = grp_off;
  it.n_levels = (u32)(pl.groups.size() - 1);
  it.flag = flag;
  it.fri_row = fri_row ? 1 : 0;  // resolved by vbatch_seal
  B.items.push_back(it);
  double w = 0;
  for (u32 g : pl.groups) w += g ? g - 1 : 0;
  B.path_bytes += sizeof(typename F::Word) * w + 32.0 * (it.n_levels + 1);
}

// ---------------------------------------------------------------- the transcript up to the query loop
// What TwoAdicFriPcs::verify / verify_fri (p3-fri 0.5.1) draw from the transcript before the first query index, and every
// check they make on the way: false = refused. The order of the observations, samples and refusals is the protocol's.
template <class Ext>
struct FriReplay {
  Ext alpha;
  std::vector<unsigned> arities;  // log_arity per commit-phase round
  unsigned log_gmax = 0;          // log2 of the tallest input's LDE height
  std::vector<Ext> betas;
};
template <class F, class Params, class Rounds, class Proof, class Challenger>
bool fri_replay(const Params& prm, const Rounds& rounds, const Proof& proof, Challenger& ch, FriReplay<typename F::Ext>& out) {
  for (auto& r : rounds)
    for (auto& m : r.mats)
      for (auto& pv : m)
        for (auto& y : *pv.second) ch.observe_ext(y);
  out.alpha = ch.sample_ext();
  const size_t nrounds = proof.commits.size();
  if (proof.pow.size() != nrounds) return false;
  // every query repeats the rounds' arities; the first one's place the tallest input, and each is checked by the caller against
  // what the prover had to choose (p3-fri compute_log_arity_for_round) once the input heights are known
  out.arities.assign(nrounds, 1);
  if (!proof.queries.empty()) {
    if (proof.queries[0].steps.size() != nrounds) return false;
    for (size_t i = 0; i < nrounds; i++) out.arities[i] = proof.queries[0].steps[i].log_arity;
  }
  out.log_gmax = (unsigned)(prm.log_blowup + prm.log_final_poly_len);
  for (unsigned a : out.arities) {
    if (a > prm.max_log_arity) return false;
    out.log_gmax += a;
  }
  if (out.log_gmax > F::two_adicity) return false;  // no subgroup of that order
  out.betas.clear();
  for (size_t i = 0; i < nrounds; i++) {
    ch.observe_cap(proof.commits[i]);
    if (!ch.check_witness((unsigned)prm.commit_pow_bits, proof.pow[i])) return false;
    out.betas.push_back(ch.sample_ext());
  }
  if (proof.final_poly.size() != (size_t(1) << prm.log_final_poly_len)) return false;
  for (auto& c : proof.final_poly) ch.observe_ext(c);
  if (proof.queries.size() != prm.num_queries) return false;
  return ch.check_witness((unsigned)prm.query_pow_bits, proof.query_pow);
}

// ---------------------------------------------------------------- one proof into the batch
// pcs_verify with the per-query arithmetic and the Merkle paths left to the device.
//   COLLECT_REFUSED  pcs_verify returns false here, whatever the values are (nothing was added to B)
//   COLLECT_QUEUED   the verdict is B's flag `flag` after vbatch_run
//   COLLECT_HOST     the flat layout cannot hold this proof although pcs_verify may accept it: the caller runs pcs_verify
//                    itself (nothing was added to B). See F::unopened_width_mismatch; no prover output has this form.
// Widths are fixed by the first query. A later query whose row has another width is refused where the matrix is opened at some
// point (pcs_verify compares the width with the opened values'); where it is opened at none, the field decides.
enum { COLLECT_REFUSED = 0, COLLECT_QUEUED, COLLECT_HOST };
template <class F, class Params, class Rounds, class Proof, class Challenger>
int pcs_collect(const Params& prm, const Rounds& rounds, const Proof& proof, Challenger& ch, VBatch<F>& B, u32 flag) {
  using Word = typename F::Word;
  using Ext = typename F::Ext;
  const unsigned lb = (unsigned)prm.log_blowup;
  FriReplay<Ext> fr;
  if (!fri_replay<F>(prm, rounds, proof, ch, fr)) return COLLECT_REFUSED;
  const std::vector<unsigned>& arities = fr.arities;
  const unsigned log_gmax = fr.log_gmax;
  const size_t nrounds = arities.size();
  const unsigned log_final_height = (unsigned)(lb + prm.log_final_poly_len);
  const size_t nq = proof.queries.size(), R = rounds.size();
  if (nq == 0) return COLLECT_QUEUED;  // nothing is queried: pcs_verify accepts here as well (the flag stays clear)
  std::vector<size_t> index(nq);
  for (size_t q = 0; q < nq; q++) index[q] = ch.sample_bits(log_gmax);

  // ---- the input rounds' structure, from the first query
  struct RoundPlan {
    PathPlan pl;
    unsigned log_bmax = 0;
    std::vector<size_t> width, row_off;  // per matrix: words, and where its row lies in a query's block
    size_t words = 0, path_len = 0;
  };
  std::vector<RoundPlan> rp(R);
  const auto& q0 = proof.queries[0];
  if (q0.inputs.size() != R) return COLLECT_REFUSED;
  size_t blk = 1;  // word 0 of a query's block is its index
  std::map<unsigned, std::vector<std::pair<size_t, size_t>>, std::greater<unsigned>> by_height;  // (round, matrix) in ro's order
  for (size_t ri = 0; ri < R; ri++) {
    const auto& r = rounds[ri];
    const auto& bo = q0.inputs[ri];
    RoundPlan& P = rp[ri];
    if (bo.rows.size() != r.mats.size()) return COLLECT_REFUSED;
    std::vector<Dim> dims;
    for (size_t mi = 0; mi < r.mats.size(); mi++) {
      dims.push_back(Dim{bo.rows[mi].size(), size_t(1) << (r.log_n[mi] + lb)});
      P.log_bmax = std::max(P.log_bmax, r.log_n[mi] + lb);
      P.width.push_back(bo.rows[mi].size());
      for (auto& pv : r.mats[mi])
        if (pv.second->size() != bo.rows[mi].size()) return COLLECT_REFUSED;
      by_height[r.log_n[mi] + lb].push_back({ri, mi});
    }
    if (P.log_bmax > log_gmax) return COLLECT_REFUSED;
    P.path_len = bo.path.size();
    if (mmcs_plan<F>(dims, r.commit.size(), P.path_len, P.pl) != PLAN_OK) return COLLECT_REFUSED;
    P.row_off.resize(dims.size());
    for (size_t i : P.pl.order) {
      P.row_off[i] = blk + P.words;
      P.words += dims[i].w;
    }
    blk += P.words;
  }
  // ---- heights of the reduced openings, descending, and the fold chain's schedule
  std::vector<unsigned> hs;
  for (auto& kv : by_height) hs.push_back(kv.first);
  const bool zero_rule = by_height.count(lb) && log_final_height >= lb && lb < log_gmax;  // lb is the lowest height: the last slot
  const size_t n_chain = hs.size() - (zero_rule ? 1 : 0);
  if (n_chain == 0 || hs[0] != log_gmax) return COLLECT_REFUSED;
  struct StepPlan {
    PathPlan pl;
    size_t path_len = 0, row_off = 0, sib_off = 0;
    unsigned shift = 0;  // the round's row index is the query index >> shift
  };
  std::vector<StepPlan> sp(nrounds);
  size_t fri_stride = 0, sib_stride = 0;
  {
    size_t hp = 1;
    unsigned lh = log_gmax, shift = 0;
    for (size_t i = 0; i < nrounds; i++) {
      const unsigned la = arities[i];
      if (lh <= log_final_height) return COLLECT_REFUSED;
      unsigned want = std::min<unsigned>((unsigned)prm.max_log_arity, lh - log_final_height);
      if (hp < n_chain) want = std::min(want, lh - hs[hp]);
      if (la != want) return COLLECT_REFUSED;
      lh -= la;
      shift += la;
      const size_t m = size_t(1) << la;
      sp[i].path_len = q0.steps[i].path.size();
      sp[i].shift = shift;
      sp[i].row_off = fri_stride;
      sp[i].sib_off = sib_stride;
      if (mmcs_plan<F>({Dim{F::ext_words * m, size_t(1) << lh}}, proof.commits[i].size(), sp[i].path_len, sp[i].pl) != PLAN_OK)
        return COLLECT_REFUSED;
      fri_stride += F::ext_words * m;
      sib_stride += m - 1;
      if (hp < n_chain && hs[hp] == lh) hp++;
    }
    if (hp != n_chain) return COLLECT_REFUSED;
  }
  // ---- every query has that structure
  for (auto& qp : proof.queries) {
    if (qp.inputs.size() != R || qp.steps.size() != nrounds) return COLLECT_REFUSED;
    for (size_t ri = 0; ri < R; ri++) {
      const auto& bo = qp.inputs[ri];
      if (bo.rows.size() != rp[ri].width.size()) return COLLECT_REFUSED;
      for (size_t mi = 0; mi < bo.rows.size(); mi++)
        if (bo.rows[mi].size() != rp[ri].width[mi]) return rounds[ri].mats[mi].empty() ? F::unopened_width_mismatch : COLLECT_REFUSED;
      if (bo.path.size() != rp[ri].path_len) return COLLECT_REFUSED;
    }
    for (size_t i = 0; i < nrounds; i++) {
      const auto& st = qp.steps[i];
      if (st.log_arity != arities[i] || st.siblings.size() != (size_t(1) << arities[i]) - 1 || st.path.size() != sp[i].path_len)
        return COLLECT_REFUSED;
    }
  }

  // ---- accepted so far: append
  VProofDesc<Ext> D;
  memset(&D, 0, sizeof(D));
  D.alpha = fr.alpha;
  D.blk_off = B.words.size();
  D.blk_stride = blk;
  D.fri_off = B.fri_words;  // (vbatch_seal adds the uploaded words in front)
  D.fri_stride = fri_stride;
  D.ro_off = B.ro_count;
  D.sib_stride = (u32)sib_stride;
  D.n_rounds = (u32)nrounds;
  D.log_gmax = log_gmax;
  D.query0 = (u32)B.qmap.size();
  D.flag = flag;
  D.n_heights = (u32)hs.size();
  D.zero_slot = zero_rule ? (u32)(hs.size() - 1) : ~u32(0);
  D.height_off = (u32)B.heights.size();
  for (unsigned lh : hs) {
    auto& list = by_height[lh];
    VHeightDesc H;
    H.lh = lh;
    H.mat_off = (u32)B.mats.size();
    H.n_mats = (u32)list.size();
    H.pad = 0;
    B.heights.push_back(H);
    for (auto& rm : list) {
      const auto& pts = rounds[rm.first].mats[rm.second];
      VMatDesc M;
      M.row_off = (u32)rp[rm.first].row_off[rm.second];
      M.width = (u32)rp[rm.first].width[rm.second];
      M.n_points = (u32)pts.size();
      M.pv_off = (u32)B.ext.size();
      B.mats.push_back(M);
      for (auto& pv : pts) {
        B.ext.push_back(pv.first);
        B.ext.insert(B.ext.end(), pv.second->begin(), pv.second->end());
      }
    }
  }
  D.beta_off = (u32)B.ext.size();
  B.ext.insert(B.ext.end(), fr.betas.begin(), fr.betas.end());
  D.final_off = (u32)B.ext.size();
  D.n_final = (u32)proof.final_poly.size();
  B.ext.insert(B.ext.end(), proof.final_poly.begin(), proof.final_poly.end());
  D.arity_off = (u32)B.u32s.size();
  for (unsigned a : arities) B.u32s.push_back(a);
  std::vector<u32> grp_in(R), cap_in(R), grp_fri(nrounds), cap_fri(nrounds);
  for (size_t ri = 0; ri < R; ri++) {
    grp_in[ri] = (u32)B.u32s.size();
    B.u32s.insert(B.u32s.end(), rp[ri].pl.groups.begin(), rp[ri].pl.groups.end());
    cap_in[ri] = (u32)B.digs.size();
    B.digs.insert(B.digs.end(), rounds[ri].commit.begin(), rounds[ri].commit.end());
  }
  for (size_t i = 0; i < nrounds; i++) {
    grp_fri[i] = (u32)B.u32s.size();
    B.u32s.insert(B.u32s.end(), sp[i].pl.groups.begin(), sp[i].pl.groups.end());
    cap_fri[i] = (u32)B.digs.size();
    B.digs.insert(B.digs.end(), proof.commits[i].begin(), proof.commits[i].end());
  }
  D.sib_off = (u32)B.ext.size();
  const u32 proof_slot = (u32)B.proofs.size();
  for (size_t q = 0; q < nq; q++) {
    const auto& qp = proof.queries[q];
    B.words.push_back((Word)index[q]);
    for (size_t ri = 0; ri < R; ri++) {
      const auto& bo = qp.inputs[ri];
      const u64 vals_off = B.words.size();
      for (size_t i : rp[ri].pl.order) B.words.insert(B.words.end(), bo.rows[i].begin(), bo.rows[i].end());
      const u32 sib = (u32)B.digs.size();
      B.digs.insert(B.digs.end(), bo.path.begin(), bo.path.end());
      vb_add_item(B, rp[ri].pl, vals_off, false, index[q] >> (log_gmax - rp[ri].log_bmax), sib, cap_in[ri], grp_in[ri], flag);
    }
    for (size_t i = 0; i < nrounds; i++) {
      const auto& st = qp.steps[i];
      B.ext.insert(B.ext.end(), st.siblings.begin(), st.siblings.end());
      const u32 sib = (u32)B.digs.size();
      B.digs.insert(B.digs.end(), st.path.begin(), st.path.end());
      vb_add_item(B, sp[i].pl, B.fri_words + q * fri_stride + sp[i].row_off, true, index[q] >> sp[i].shift, sib, cap_fri[i], grp_fri[i], flag);
    }
    B.qmap.push_back(proof_slot);
  }
  B.fri_words += nq * fri_stride;
  B.ro_count += nq * hs.size();
  B.proofs.push_back(D);
  return COLLECT_QUEUED;
}

// ---------------------------------------------------------------- the flush loop
// verdicts[i] = what the field's verify() returns for proof i. `dev` carries the field's own kernel arguments.
template <class F, class System>
void verify_batch_run(System& sys, const typename F::Dev& dev, size_t n_proofs, const u64* n_claims, const u64* const* claim_offsets,
                      const typename F::Word* const* claim_data, const uint8_t* const* proofs, const u64* proof_lens, int32_t* verdicts) {
  Ctx& ctx = *sys.ctx;
  HIP_CHECK(hipSetDevice(ctx.device));
  static const u64 no_offsets[1] = {0};
  VBatch<F> B;
  std::vector<std::pair<size_t, int>> waiting;  // (proof, its out-of-domain verdict): the device decides between that and 2
  std::vector<u32> fail;
  auto flush = [&]() {
    B.n_flags = waiting.size();
    vbatch_run<F>(ctx, dev, B, fail);
    for (size_t k = 0; k < waiting.size(); k++) verdicts[waiting[k].first] = fail[k] ? V_INVALID_OPENING : waiting[k].second;
    waiting.clear();
    B = VBatch<F>();
  };
  for (size_t i = 0; i < n_proofs; i++) {
    const u64* offs = n_claims[i] ? claim_offsets[i] : no_offsets;
    typename F::Prepared P(sys);
    const int v = F::prepare(sys, (size_t)n_claims[i], offs, claim_data ? claim_data[i] : nullptr, proofs[i], (size_t)proof_lens[i], P);
    if (v != V_OK) {
      verdicts[i] = v;
      continue;
    }
    const auto at_pcs = P.ch;
    const int c = pcs_collect<F>(sys.params, P.rounds, F::fri(P), P.ch, B, (u32)waiting.size());
    if (c == COLLECT_HOST) {
      auto ch = at_pcs;
      verdicts[i] = F::pcs_verify(sys, P, ch) ? F::ood(sys, P) : V_INVALID_OPENING;
      continue;
    }
    if (c == COLLECT_REFUSED) {
      verdicts[i] = V_INVALID_OPENING;
      continue;
    }
    waiting.push_back({i, F::ood(sys, P)});
    if (B.bytes() > VB_FLUSH_BYTES) flush();
  }
  flush();
}

}  // namespace msamd
