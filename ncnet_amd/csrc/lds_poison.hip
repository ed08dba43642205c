// Test support for the LDS poison tier (tests/test_gpu_lds_poison.py).
//
// LDS is not cleared between dispatches: a kernel that reads a word it did not
// write in the same launch sees what an earlier kernel left there.  lds_poison
// fills the whole LDS of every CU with a chosen 32-bit pattern right before a
// kernel under test, lds_probe copies a workgroup's uninitialised LDS out so
// the test can check that the fill really is what the next dispatch sees.
#include "common.h"
#include "launchers.h"

namespace ncnet {

constexpr int LDS_ALL = 160 * 1024;   // bytes of LDS per CU (gfx950)

// One workgroup owns all of a CU's LDS (so at most one is resident per CU) and
// writes every word with plain ds_write_b32; volatile keeps the stores, which
// nothing in this kernel reads back.
__global__ __launch_bounds__(256, 1) void lds_poison_kernel(uint32_t pattern) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  volatile uint32_t* w = (volatile uint32_t*)smem;
  for (int i = threadIdx.x; i < LDS_ALL / 4; i += 256) w[i] = pattern;
}

// out[g][i] = word i of workgroup g's LDS as the dispatch found it, i < n_words
__global__ __launch_bounds__(256, 1) void lds_probe_kernel(int* __restrict__ out, int n_words) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const volatile int* w = (const volatile int*)smem;
  int* o = out + (size_t)blockIdx.x * n_words;
  for (int i = threadIdx.x; i < n_words; i += 256) o[i] = w[i];
}

}  // namespace ncnet

using namespace ncnet;

extern "C" int ncnet_lds_poison(unsigned int pattern, int rounds, hipStream_t stream) {
  if (rounds < 1 || rounds > 64) return -3;
  const int ncu = device_num_cus();
  hipLaunchKernelGGL(lds_poison_kernel, dim3((unsigned)(ncu * rounds)), dim3(256), (size_t)LDS_ALL, stream,
                     (uint32_t)pattern);
  return (int)hipGetLastError();
}

extern "C" int ncnet_lds_probe(int* out, int G, int n_words, int lds_bytes, hipStream_t stream) {
  if (G < 1 || lds_bytes < 4 || lds_bytes > LDS_ALL || lds_bytes % 4 || n_words < 1 || n_words > lds_bytes / 4)
    return -3;
  hipLaunchKernelGGL(lds_probe_kernel, dim3((unsigned)G), dim3(256), (size_t)lds_bytes, stream, out, n_words);
  return (int)hipGetLastError();
}
