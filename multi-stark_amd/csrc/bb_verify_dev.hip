// Kernels of batched verification for the BabyBear / Poseidon2 configuration (bb_verify_dev.h). Two launches per batch:
//   bbv_queries_k  one thread per (proof, query): reduced openings, FRI fold chain, final polynomial - the per-query
//                  arithmetic of bb_verifier.hip::pcs_verify restated with the same field functions (bb_dev.h is shared by
//                  host and device, so the results are the same field elements). Writes every FRI round's leaf row.
//   bbv_paths_k    one thread per Merkle path (input rounds, FRI rounds, msbb_mmcs_verify_batch openings): a dependent
//                  chain of Poseidon2 permutations per thread, wide across threads (leaf_hash_k in bb_kernels.hip is the
//                  precedent for a whole permutation per thread).
// Every index used here was derived by the host from lengths it had checked; a refused proof contributes no thread.
#include "bb.h"
#include "bb_verify_dev.h"

namespace msbb {

namespace {

__global__ __launch_bounds__(256) void bbv_paths_k(BVDev d, u32 n_items) {
  const u32 t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_items) return;
  bbv_path_body(d, t);
}

__global__ __launch_bounds__(256) void bbv_queries_k(BVDev d, u32 n_queries) {
  const u32 t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_queries) return;
  bbv_query_body(d, t);
}

}  // namespace

void bbv_launch(Ctx& ctx, const BVDev& d, size_t n_queries, size_t n_items, double path_bytes) {
  if (n_queries) {
    hipEvent_t ev = ctx.prof_begin(msamd::K_OTHER);
    hipLaunchKernelGGL(bbv_queries_k, dim3((unsigned)((n_queries + 255) / 256)), dim3(256), 0, ctx.stream, d, (u32)n_queries);
    HIP_CHECK(hipGetLastError());
    ctx.prof_end(msamd::K_OTHER, ev, 0.0);
  }
  if (n_items) {
    hipEvent_t ev = ctx.prof_begin(msamd::K_COMPRESS);
    hipLaunchKernelGGL(bbv_paths_k, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, ctx.stream, d, (u32)n_items);
    HIP_CHECK(hipGetLastError());
    ctx.prof_end(msamd::K_COMPRESS, ev, path_bytes);
  }
}

}  // namespace msbb
