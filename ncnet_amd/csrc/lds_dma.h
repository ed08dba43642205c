// The LDS-DMA idiom of the gfx950 kernels, in one place (included by common.h).
//
// LDS-DMA of 16 B per lane (global_load_lds_dwordx4 / buffer_load_dwordx4 ..
// lds) issued from inline asm.  The compiler's waitcnt pass cannot prove that
// an LDS-DMA misses a later ds_read_b64_tr_b16 (intrinsic reads carry no alias
// info), so with the builtin it drains EVERY in-flight DMA (s_waitcnt vmcnt(0))
// before the first transposed read -- the next step's prefetch is serialised
// with the compute.  Issued from asm the DMA is invisible to that pass; the
// kernel then owns the wait: dma_wait*<N> below before reading what landed.
// (Extra in-flight asm ops only make the compiler's own vmcnt waits stricter,
// never weaker: completion is in issue order.)
//
// Visible or invisible is a per-kernel decision.  The builtin form
// (__builtin_amdgcn_global_load_lds in conv16v2 / v3 / f8, wgrad16v2,
// corr_gemm_v2 / f8v2 and conv2d v2; __builtin_amdgcn_raw_ptr_buffer_load_lds
// in conv16v4 and nc_fused) is for kernels that read what landed with plain
// LDS loads, or that want the compiler's waits (some still count their own
// with dma_wait*<N>); the asm form here is for the rest: conv2d v3, conv1x16,
// wgrad1x16, cout1_taps, wgrad16v3 / v4 / p.
//
// The contract every user of the asm form keeps:
//  * each wave issues a FIXED number of DMA instructions per stage, whatever
//    the runtime geometry, so `dma_wait<N>` with N = the instructions of the
//    stages that may still fly means "everything older has landed".  A lane
//    with nothing to fetch stays off (exec never empty), reads zeros through a
//    0-record descriptor, or the whole instruction goes to a trash KiB of LDS;
//  * completion is in issue order, so a counted wait never needs to know
//    which stage an instruction belonged to;
//  * M0 (the wave-uniform LDS destination) is set by the helper right before
//    the instruction; kernels using this issue no other M0-based instruction.
#pragma once

// compile-time loop: f(std::integral_constant<int, B>{}) ... f(<E - 1>)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// 32-bit LDS byte address of a generic pointer into LDS
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
// The LDS address as it goes into M0.  The optimizer keeps a wave-uniform
// address in a scalar register; the -O1 debug build does not, and an "s"
// operand then assembles as `s_mov_b32 m0, vNN`, so there the uniform value is
// read from the first lane.  (Unconditionally, the readfirstlane of a cast
// generic pointer breaks instruction selection at -O3.)
__device__ __forceinline__ uint32_t lds_m0(uint32_t lds) {
#ifdef NCNET_DEBUG
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)lds);
#else
  return lds;
#endif
}

// global DMA: lane's 16 B at gsrc -> LDS byte address lds + 16 * lane
__device__ __forceinline__ void dma16_lds(const void* gsrc, uint32_t lds) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_m0(lds))
               : "memory", "m0");
}
__device__ __forceinline__ void dma16_lds(const void* gsrc, const void* lds_dst) { dma16_lds(gsrc, lds_addr(lds_dst)); }

// buffer DMA (offen): lane's 16 B at byte offset voff of the resource; offsets
// at or past num_records land as zeros.  make_rsrc: base, 48-bit base hi,
// num_records = nbytes, raw 32-bit dword format.
// RFL: read the (wave-uniform) words from the first lane, which tells the
// compiler they are scalar.  conv1x.hip passes false: its descriptors are
// built from values the compiler already holds in scalar registers, and the
// extra readfirstlanes change its register allocation.
typedef int i32x4 __attribute__((ext_vector_type(4)));
template <bool RFL = true>
__device__ __forceinline__ i32x4 make_rsrc(const void* base, uint32_t nbytes) {
  const uint64_t b = (uint64_t)base;
  i32x4 r = {(int)(uint32_t)b, (int)((uint32_t)(b >> 32) & 0xffffu), (int)nbytes, 0x00020000};
  if constexpr (RFL) {
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = __builtin_amdgcn_readfirstlane(r[i]);
  }
  return r;
}
__device__ __forceinline__ void bdma16_lds(const i32x4& rs, uint32_t voff, uint32_t lds) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(rs),
               "s"(lds_m0(lds))
               : "memory", "m0");
}

// Counted waits: at most N of this wave's vector-memory ops (asm DMAs
// included) still in flight.  dma_wait<N>: the wait alone (a wave reading only
// its own DMAs); dma_wait_barrier<N>: + workgroup barrier; dma_wait_lds_barrier<N>:
// also this wave's LDS ops (its reads of the buffer the next stage overwrites).
template <int N>
__device__ __forceinline__ void dma_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void dma_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void dma_wait_lds_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
__device__ __forceinline__ void asm_barrier_vm0() { dma_wait_lds_barrier<0>(); }

// LDS swizzles of the GEMM-like kernels (16-byte chunks, conflict-free
// ds_read_b128 of 16 consecutive rows at one chunk column).
// 64-byte rows (4 chunks): the DMA rings of corr_gemm_v2 and conv2d v2
__device__ __forceinline__ int swz(int r) { return (r & 1) ^ ((r >> 1) & 2); }
__device__ __forceinline__ uint32_t roff(int row, int chunk) { return (uint32_t)(row * 64 + ((chunk ^ swz(row)) << 4)); }
// 128-byte rows (8 chunks): conv2d v1 / v3.  chunk ^ ((row >> 1) & 7): the 16
// rows of a lane group land on 16 distinct 16-B bank slots (chunk ^ (row & 7)
// put rows r and r + 8 on one slot)
__device__ __forceinline__ uint32_t toff(int row, int chunk) { return (uint32_t)(row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4)); }
