// Traces that start in DEVICE memory (ms_witness_create_device / msbb_witness_create_device, ingest.hip): the host-side
// checks of a caller's ms_dev_matrix, the ordering behind the caller's stream, and the launchers that copy a strided view
// into the layout a witness stores while checking every element against the field modulus.
#pragma once
#include <string>

#include "../../include/mstark.h"
#include "msamd.h"

namespace msamd {

struct IngestView {  // a checked ms_dev_matrix: element (r, c) at base + (r * row_stride + c * col_stride) * elem_bytes
  const void* base = nullptr;
  size_t h = 0, w = 0;
  unsigned elem_bytes = 0;
  size_t row_stride = 0, col_stride = 0;
};
// Everything that can be decided about one matrix without a launch (throws with the circuit's number): elem_bytes one of
// 1 / 2 / 4 / 8 and at most max_elem_bytes, strides > 0, an extent that fits 63 bits, a pointer aligned to elem_bytes that
// hipPointerGetAttributes reports as device memory of the context's device, and a view that lies inside the allocation
// hipMemGetAddressRange reports around it. m.height must be > 0.
IngestView ingest_check(Ctx& ctx, const ms_dev_matrix& m, size_t circuit, size_t width, unsigned max_elem_bytes);
// the same pointer checks for a plain array of `bytes` bytes (device-resident claims)
void ingest_check_device_range(Ctx& ctx, const void* p, size_t bytes, size_t align, const std::string& what);
// producer_stream != nullptr: the context's stream waits for everything queued on it so far (an event, no host wait)
void ingest_wait_for_producer(Ctx& ctx, void* producer_stream);
// "non-canonical trace value: circuit 1, row 5, column 3" for the flat index r * w + c
std::string ingest_offender_text(size_t circuit, u64 flat, size_t w);

// Launches only, on ctx.stream. *bad (device, initialised to all-ones by the caller) takes the smallest flat index r * w + c
// of an element >= the modulus (atomicMin); only elements of the full width can be: 8 bytes for Goldilocks, 4 for BabyBear.
// Goldilocks: out = h x w row-major u64 (HWitness::traces).
void ingest_goldilocks(Ctx& ctx, const IngestView& v, u64* out_rowmajor, u64* bad);
// BabyBear: out = column-major u32 in Montgomery form with leading dimension h (what bb_upload_rows leaves in a BMat); elem_bytes <= 4
void ingest_babybear(Ctx& ctx, const IngestView& v, u32* out_colmajor_monty, u64* bad);

}  // namespace msamd
