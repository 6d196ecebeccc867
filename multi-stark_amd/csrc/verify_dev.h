// Device side of batched verification (ms_verify_batch, ms_mmcs_verify_batch): the flat arrays the host builds from
// proofs whose shape it has already checked, and the two launches that consume them. No kernel ever sees proof bytes:
// every offset and length below is derived from lengths verifier.hip has validated.
#pragma once
#include "msamd.h"

namespace msamd {

// one leaf or injected group is hashed inside a thread with a chunk stack held in registers: 2^VB_STACK chunks at most
static constexpr unsigned VB_STACK = 6;
static constexpr u32 VB_MAX_GROUP_WORDS = 128u << VB_STACK;

// MerkleTreeMmcs::verify_batch of one opening. The rows lie in walk order (stable sort by descending height) at
// words[vals_off ..); groups[grp_off + k], k = 0 .. n_levels, is 1 + the word count of the matrices whose height is
// max_height >> k (0: none at that level; entry 0 is the leaf and always present).
struct VPathItem {
  u64 vals_off, index;
  u32 sib_off;   // digs: n_levels siblings, bottom-up
  u32 cap_off;   // digs: the cap; entry index >> n_levels is compared
  u32 grp_off, n_levels;
  u32 flag;      // fail[flag] |= 1 when the opening is refused
  u32 pad;
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
struct VProofDesc {
  E2 alpha;
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

struct VDev {
  const VPathItem* items;
  const VProofDesc* proofs;
  const VMatDesc* mats;
  const VHeightDesc* heights;
  const u32* u32s;
  const u32* qmap;     // global query -> proof descriptor
  const E2* ext;
  const Digest* digs;
  u32* fail;
  u64* words;          // uploaded words, then the FRI leaf rows
  E2* ro;
};

// the arithmetic launch over n_queries threads (K_OTHER), then the path launch over n_items threads (K_COMPRESS)
void verify_batch_launch(Ctx& ctx, const VDev& d, size_t n_queries, size_t n_items, double path_bytes);

}  // namespace msamd
