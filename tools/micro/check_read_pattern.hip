// Does staging a tile of rows through LDS pay for a thread-per-row sweep over a ROW-MAJOR trace (csrc/check_dev.h with check.hip's view)?
//   hipcc -O3 --offload-arch=gfx950 -o check_read_pattern tools/micro/check_read_pattern.hip && ./check_read_pattern [log2 rows = 20]
// Both kernels read every word of row r and row (r + 1) mod n once per thread, as the check's leaf loads do, fold them into one
// word per row and write it: `direct` loads straight from global memory (lane k reads address base + k * width: strided),
// `staged` has the workgroup copy its 257 rows into LDS with consecutive lanes on consecutive words and reads the tile instead
// (rows padded to an odd number of words: 64-bit LDS reads at an odd stride do not conflict). Device events, 3 warm-up and 20
// timed launches each, alternating; the sums of the two forms are compared.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned long long u64;
#define CK(e)                                                                  \
  do {                                                                         \
    hipError_t _e = (e);                                                       \
    if (_e != hipSuccess) {                                                    \
      fprintf(stderr, "%s at line %d\n", hipGetErrorString(_e), __LINE__);     \
      return 1;                                                                \
    }                                                                          \
  } while (0)

__global__ __launch_bounds__(256) void direct_k(const u64* __restrict__ t, size_t n, unsigned w, u64* __restrict__ out) {
  const size_t r = blockIdx.x * size_t(256) + threadIdx.x;
  if (r >= n) return;
  const size_t rn = r + 1 == n ? 0 : r + 1;
  u64 acc = 0;
  for (unsigned c = 0; c < w; c++) acc += t[r * w + c] * 3 + t[rn * w + c];
  out[r] = acc;
}

__global__ __launch_bounds__(256) void staged_k(const u64* __restrict__ t, size_t n, unsigned w, u64* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) u64 tile[];  // 257 rows of pw words
  const unsigned pw = w | 1;
  const size_t r0 = blockIdx.x * size_t(256);
  const size_t rows = n - r0 < 256 ? n - r0 : 256;            // rows of this workgroup; one more is staged for the window
  const size_t words = (rows + 1) * w;
  for (size_t i = threadIdx.x; i < words; i += 256) {
    const size_t lr = i / w, c = i - lr * w;
    size_t gr = r0 + lr;
    if (gr >= n) gr -= n;                                     // the wrap row of the last workgroup
    tile[lr * pw + c] = t[gr * w + c];
  }
  __syncthreads();
  if (threadIdx.x >= rows) return;
  const u64* cur = tile + size_t(threadIdx.x) * pw;
  u64 acc = 0;
  for (unsigned c = 0; c < w; c++) acc += cur[c] * 3 + cur[pw + c];
  out[r0 + threadIdx.x] = acc;
}

int main(int argc, char** argv) {
  const unsigned log_n = argc > 1 ? (unsigned)atoi(argv[1]) : 20;
  if (log_n < 8 || log_n > 24) return 2;
  const size_t n = size_t(1) << log_n;
  const unsigned widths[] = {3, 14, 30};  // (257 rows of 31 words are 63.7 KB: the widest tile below 64 KB)
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  for (unsigned w : widths) {
    std::vector<u64> h(n * w);
    u64 s = 0x9E3779B97F4A7C15ull + w;
    for (auto& x : h) {
      s ^= s << 13, s ^= s >> 7, s ^= s << 17;
      x = s;
    }
    u64 *d, *o0, *o1;
    CK(hipMalloc(&d, n * w * 8));
    CK(hipMalloc(&o0, n * 8));
    CK(hipMalloc(&o1, n * 8));
    CK(hipMemcpy(d, h.data(), n * w * 8, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)((n + 255) / 256);
    const size_t lds = size_t(257) * (w | 1) * 8;
    float ms[2] = {0, 0};
    for (int it = 0; it < 23; it++) {
      for (int k = 0; k < 2; k++) {
        CK(hipEventRecord(a));
        if (k == 0)
          hipLaunchKernelGGL(direct_k, dim3(grid), dim3(256), 0, 0, d, n, w, o0);
        else
          hipLaunchKernelGGL(staged_k, dim3(grid), dim3(256), lds, 0, d, n, w, o1);
        CK(hipGetLastError());
        CK(hipEventRecord(b));
        CK(hipEventSynchronize(b));
        float t;
        CK(hipEventElapsedTime(&t, a, b));
        if (it >= 3) ms[k] += t / 20;
      }
    }
    std::vector<u64> r0(n), r1(n);
    CK(hipMemcpy(r0.data(), o0, n * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(r1.data(), o1, n * 8, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) bad += r0[i] != r1[i];
    const double gb = double(n) * w * 8 / 1e9;
    printf("2^%u rows x %2u columns (%.0f MB): direct %.4f ms (%.0f GB/s)   staged %.4f ms (%.0f GB/s, %zu B of LDS)   mismatches %zu\n", log_n, w, gb * 1e3,
           ms[0], gb / ms[0] * 1e3, ms[1], gb / ms[1] * 1e3, lds, bad);
    CK(hipFree(d));
    CK(hipFree(o0));
    CK(hipFree(o1));
    if (bad) return 3;
  }
  return 0;
}
