// Device side of batched verification (ms_verify_batch, ms_mmcs_verify_batch): the Goldilocks / BLAKE3 instance of the flat
// arrays of verify_batch.h, which the host builds from proofs whose shape it has already checked, and the two launches that
// consume them. No kernel ever sees proof bytes: every offset and length is derived from lengths the collector of
// verify_batch.h has validated.
#pragma once
#include "msamd.h"
#include "verify_batch.h"

namespace msamd {

// one leaf or injected group is hashed inside a thread with a chunk stack held in registers: 2^VB_STACK chunks at most
static constexpr unsigned VB_STACK = 6;
static constexpr u32 VB_MAX_GROUP_WORDS = 128u << VB_STACK;

using GVProofDesc = VProofDesc<E2>;
using GVDev = VDev<u64, E2, Digest>;
static_assert(sizeof(GVProofDesc) == 112 && std::is_trivially_copyable<GVProofDesc>::value, "GVProofDesc layout");
static_assert(sizeof(GVDev) == 88 && std::is_trivially_copyable<GVDev>::value, "GVDev layout");

// the arithmetic launch over n_queries threads (K_OTHER), then the path launch over n_items threads (K_COMPRESS)
void verify_batch_launch(Ctx& ctx, const GVDev& d, size_t n_queries, size_t n_items, double path_bytes);

}  // namespace msamd
