// Witness traces from device memory (ms_witness_create_device, msbb_witness_create_device): one pass that reads a strided
// view of 1 / 2 / 4 / 8-byte unsigned elements, checks every element against the field modulus and writes the layout the
// witness stores - row-major u64 for Goldilocks (HWitness::traces), column-major Montgomery u32 for BabyBear (BMat).
//
// The kernels are written for the OUTPUT's axes: F is its contiguous ("fast") axis, S the other one, output element (s, f) at
// out[s * F + f] and its source at in[s * ss + f * fs]. Goldilocks: S = rows, F = columns; BabyBear: S = columns, F = rows.
// Three forms, so that reads and writes are both coalesced whichever way the source lies:
//   vec     fs == 1, 16-byte loads: base, row pitch and row length are multiples of 16 bytes (a contiguous source is one long row)
//   tiled   ss == 1: the source runs along S; 64 x 64 tiles turned in LDS, rows padded by one element (the standard +1 pad:
//           the turned read of 8-byte words walks 65 words = banks 2 l, 2 l + 1 per lane - conflict-free per 32-lane half)
//   plain   everything else: one output element per thread (writes coalesced; reads as the strides allow)
// All are grid-strided with 64-bit indices. An offender is reported as the smallest flat index r * w + c: every thread keeps
// its own minimum and ends with at most one 64-bit atomicMin. Only what lies inside the view is read.
#include <algorithm>

#include "bb_dev.h"
#include "ingest.h"

namespace msamd {

namespace {

struct IngestArgs {
  const void* in;
  void* out;
  size_t S, F;    // output axes: slow, fast (contiguous)
  size_t ss, fs;  // source strides along them, in elements
  size_t h, w;    // the matrix (for the offender's flat index)
  unsigned long long* bad;
};

struct GlIngest {
  typedef u64 Out;
  static constexpr bool kColMajorOut = false;
  static constexpr unsigned kFullBytes = 8;
  template <class In>
  static __device__ __forceinline__ bool bad(In v) { return sizeof(In) == 8 && (u64)v >= GL_P; }
  static __device__ __forceinline__ Out conv(u64 v) { return v; }
};
struct BbIngest {
  typedef u32 Out;
  static constexpr bool kColMajorOut = true;
  static constexpr unsigned kFullBytes = 4;
  template <class In>
  static __device__ __forceinline__ bool bad(In v) { return sizeof(In) == 4 && (u32)v >= msbb::BB_P; }
  static __device__ __forceinline__ Out conv(u64 v) { return msbb::bb_to_monty((u32)v); }
};

// output index o = s * F + f -> r * w + c (the order in which the caller counts)
template <class Fd>
__device__ __forceinline__ unsigned long long flat_of(const IngestArgs& a, size_t o) {
  return Fd::kColMajorOut ? (unsigned long long)((o % a.h) * a.w + o / a.h) : (unsigned long long)o;
}
__device__ __forceinline__ void report(unsigned long long* bad, unsigned long long worst) {
  if (worst != ~0ull) atomicMin(bad, worst);
}

template <class In, class Fd>
__global__ __launch_bounds__(256) void ingest_vec_k(IngestArgs a) {
  typedef typename Fd::Out Out;
  constexpr unsigned PER = 16 / sizeof(In), NQ = PER * sizeof(Out) / 16;
  const In* __restrict__ in = static_cast<const In*>(a.in);
  Out* __restrict__ out = static_cast<Out*>(a.out);
  const size_t vpr = a.F / PER, total = a.S * vpr, step = size_t(gridDim.x) * blockDim.x;
  unsigned long long worst = ~0ull;
  for (size_t v = blockIdx.x * size_t(blockDim.x) + threadIdx.x; v < total; v += step) {
    const size_t s = a.S == 1 ? 0 : v / vpr, j = v - s * vpr;
    union {
      uint4 q;
      In e[PER];
    } src;
    src.q = *reinterpret_cast<const uint4*>(in + s * a.ss + j * PER);
    union {
      uint4 q[NQ];
      Out e[PER];
    } dst;
    const size_t o = s * a.F + j * PER;
#pragma unroll
    for (unsigned k = 0; k < PER; k++) {
      if (Fd::bad(src.e[k])) worst = min(worst, flat_of<Fd>(a, o + k));
      dst.e[k] = Fd::conv((u64)src.e[k]);
    }
    uint4* d = reinterpret_cast<uint4*>(out + o);
#pragma unroll
    for (unsigned k = 0; k < NQ; k++) d[k] = dst.q[k];
  }
  report(a.bad, worst);
}

template <class In, class Fd>
__global__ __launch_bounds__(256) void ingest_tiled_k(IngestArgs a) {
  typedef typename Fd::Out Out;
  __shared__ Out tile[64][65];
  const In* __restrict__ in = static_cast<const In*>(a.in);
  Out* __restrict__ out = static_cast<Out*>(a.out);
  const size_t ts = (a.S + 63) / 64, tf = (a.F + 63) / 64, tiles = ts * tf;
  unsigned long long worst = ~0ull;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const size_t s0 = (t % ts) * 64, f0 = (t / ts) * 64;
    const unsigned ns = (unsigned)((a.S - s0) < 64 ? (a.S - s0) : 64), nf = (unsigned)((a.F - f0) < 64 ? (a.F - f0) : 64);
    for (unsigned idx = threadIdx.x; idx < ns * nf; idx += blockDim.x) {  // lanes along S: where the source is contiguous
      const unsigned fl = idx / ns, sl = idx % ns;
      const In v = in[(s0 + sl) + (f0 + fl) * a.fs];
      if (Fd::bad(v)) worst = min(worst, flat_of<Fd>(a, (s0 + sl) * a.F + f0 + fl));
      tile[fl][sl] = Fd::conv((u64)v);
    }
    __syncthreads();
    for (unsigned idx = threadIdx.x; idx < ns * nf; idx += blockDim.x) {  // lanes along F: where the output is contiguous
      const unsigned sl = idx / nf, fl = idx % nf;
      out[(s0 + sl) * a.F + f0 + fl] = tile[fl][sl];
    }
    __syncthreads();
  }
  report(a.bad, worst);
}

template <class In, class Fd>
__global__ __launch_bounds__(256) void ingest_plain_k(IngestArgs a) {
  typedef typename Fd::Out Out;
  const In* __restrict__ in = static_cast<const In*>(a.in);
  Out* __restrict__ out = static_cast<Out*>(a.out);
  const size_t total = a.S * a.F, step = size_t(gridDim.x) * blockDim.x;
  unsigned long long worst = ~0ull;
  for (size_t o = blockIdx.x * size_t(blockDim.x) + threadIdx.x; o < total; o += step) {
    const size_t s = a.S == 1 ? 0 : o / a.F, f = o - s * a.F;
    const In v = in[s * a.ss + f * a.fs];
    if (Fd::bad(v)) worst = min(worst, flat_of<Fd>(a, o));
    out[o] = Fd::conv((u64)v);
  }
  report(a.bad, worst);
}

constexpr size_t MAX_BLOCKS = 4096;  // grid-strided beyond: 256 CUs x 16 workgroups of four waves
unsigned grid_for(size_t items) { return (unsigned)std::max<size_t>(1, std::min(MAX_BLOCKS, (items + 255) / 256)); }

template <class In, class Fd>
void launch(Ctx& ctx, const IngestView& v, typename Fd::Out* out, u64* bad) {
  IngestArgs a;
  a.in = v.base;
  a.out = out;
  a.h = v.h, a.w = v.w;
  a.bad = reinterpret_cast<unsigned long long*>(bad);
  if (Fd::kColMajorOut)
    a.S = v.w, a.F = v.h, a.ss = v.col_stride, a.fs = v.row_stride;
  else
    a.S = v.h, a.F = v.w, a.ss = v.row_stride, a.fs = v.col_stride;
  // an axis of one element has no stride
  if (a.F == 1) a.fs = 1;
  if (a.S == 1) a.ss = 0;
  if (a.fs == 1 && a.S > 1 && a.ss == a.F) {  // contiguous: one long row
    a.F *= a.S;
    a.S = 1;
    a.ss = 0;
  }
  constexpr size_t PER = 16 / sizeof(In);
  const dim3 block(256);
  if (a.fs == 1 && a.F % PER == 0 && (reinterpret_cast<uintptr_t>(v.base) & 15) == 0 && (a.ss * sizeof(In)) % 16 == 0)
    hipLaunchKernelGGL((ingest_vec_k<In, Fd>), dim3(grid_for(a.S * (a.F / PER))), block, 0, ctx.stream, a);
  else if (a.fs != 1 && a.ss == 1)
    hipLaunchKernelGGL((ingest_tiled_k<In, Fd>), dim3((unsigned)std::min(MAX_BLOCKS, ((a.S + 63) / 64) * ((a.F + 63) / 64))), block, 0,
                       ctx.stream, a);
  else
    hipLaunchKernelGGL((ingest_plain_k<In, Fd>), dim3(grid_for(a.S * a.F)), block, 0, ctx.stream, a);
  HIP_CHECK(hipGetLastError());
}

template <class Fd>
void ingest(Ctx& ctx, const IngestView& v, typename Fd::Out* out, u64* bad) {
  if (v.h == 0 || v.w == 0) return;
  if (v.elem_bytes > Fd::kFullBytes) throw std::runtime_error("ingest: element wider than the field's word");
  hipEvent_t ev = ctx.prof_begin(K_TRANSPOSE);
  switch (v.elem_bytes) {
    case 1: launch<uint8_t, Fd>(ctx, v, out, bad); break;
    case 2: launch<uint16_t, Fd>(ctx, v, out, bad); break;
    case 4: launch<uint32_t, Fd>(ctx, v, out, bad); break;
    case 8: launch<std::conditional_t<Fd::kFullBytes == 8, uint64_t, uint32_t>, Fd>(ctx, v, out, bad); break;  // (8: Goldilocks only, checked above)
    default: throw std::runtime_error("ingest: elem_bytes must be 1, 2, 4 or 8");
  }
  ctx.prof_end(K_TRANSPOSE, ev, double(v.h) * double(v.w) * double(v.elem_bytes + sizeof(typename Fd::Out)));
}

}  // namespace

void ingest_goldilocks(Ctx& ctx, const IngestView& v, u64* out_rowmajor, u64* bad) { ingest<GlIngest>(ctx, v, out_rowmajor, bad); }
void ingest_babybear(Ctx& ctx, const IngestView& v, u32* out_colmajor_monty, u64* bad) { ingest<BbIngest>(ctx, v, out_colmajor_monty, bad); }

// ------------------------------------------------------------------ host side: what is decided before any launch
void ingest_check_device_range(Ctx& ctx, const void* p, size_t bytes, size_t align, const std::string& what) {
  if (!p) throw std::runtime_error(what + ": null pointer");
  if (reinterpret_cast<uintptr_t>(p) % align) throw std::runtime_error(what + ": pointer not aligned to " + std::to_string(align) + " bytes");
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();  // (an address the runtime has never seen: plain host memory)
  if (e != hipSuccess || attr.type != hipMemoryTypeDevice)
    throw std::runtime_error(what + ": not a pointer to device memory");
  if (attr.device != ctx.device)
    throw std::runtime_error(what + ": device memory of device " + std::to_string(attr.device) + ", the context runs on device " +
                             std::to_string(ctx.device));
  // the allocation around it: the view must lie inside (no launch ever reads what the driver cannot vouch for)
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();
    throw std::runtime_error(what + ": the driver does not know the allocation this pointer belongs to");
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base), at = reinterpret_cast<uintptr_t>(p);
  if (at < lo || bytes > size || at - lo > size - bytes)
    throw std::runtime_error(what + ": reaches " + std::to_string(at - lo + bytes) + " bytes into an allocation of " + std::to_string(size));
}

IngestView ingest_check(Ctx& ctx, const ms_dev_matrix& m, size_t circuit, size_t width, unsigned max_elem_bytes) {
  const std::string what = "device trace of circuit " + std::to_string(circuit);
  const unsigned eb = m.elem_bytes;
  if (!(eb == 1 || eb == 2 || eb == 4 || eb == 8) || eb > max_elem_bytes)
    throw std::runtime_error(what + ": elem_bytes must be one of 1, 2, 4" + (max_elem_bytes >= 8 ? ", 8" : "") + " (got " + std::to_string(eb) + ")");
  if (m.row_stride <= 0 || m.col_stride <= 0) throw std::runtime_error(what + ": strides must be positive");
  if (!m.ptr) throw std::runtime_error(what + ": null pointer with height " + std::to_string(m.height));
  IngestView v;
  v.base = m.ptr;
  v.h = (size_t)m.height, v.w = width;
  v.elem_bytes = eb;
  v.row_stride = (size_t)m.row_stride, v.col_stride = (size_t)m.col_stride;
  // (h - 1) * row_stride + (w - 1) * col_stride + 1 elements, in bytes, below 2^63
  unsigned long long a = 0, b = 0, n = 0;
  const bool over = __builtin_mul_overflow((unsigned long long)(v.h - 1), (unsigned long long)v.row_stride, &a) ||
                    __builtin_mul_overflow((unsigned long long)(width ? width - 1 : 0), (unsigned long long)v.col_stride, &b) ||
                    __builtin_add_overflow(a, b, &n) || __builtin_add_overflow(n, 1ull, &n) || __builtin_mul_overflow(n, (unsigned long long)eb, &n) ||
                    (n >> 63) != 0;
  if (over) throw std::runtime_error(what + ": height, width and strides overflow the address space");
  ingest_check_device_range(ctx, m.ptr, width ? (size_t)n : 0, eb, what);
  return v;
}

void ingest_wait_for_producer(Ctx& ctx, void* producer_stream) {
  if (!producer_stream) return;
  hipEvent_t ev = nullptr;
  HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(producer_stream));
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx.stream, ev, 0);
  (void)hipEventDestroy(ev);  // (released by the runtime once the wait has been passed)
  HIP_CHECK(e);
}

std::string ingest_offender_text(size_t circuit, u64 flat, size_t w) {
  return "non-canonical trace value: circuit " + std::to_string(circuit) + ", row " + std::to_string(flat / w) + ", column " +
         std::to_string(flat % w);
}

}  // namespace msamd
