// Backward of the fused correlation + 2x2x2x2 max-pool (corr_gemm_pool2, csrc/corr.hip)
// into the features, for relocalized training with a trainable trunk.
//
// Rows are in 2x2-block order (row = 4 * pooled cell + sub).  Pooled cell (I, J) of
// volume v took its maximum at A sub-row a and B sub-row b of the code byte
// (di<<6 | dj<<4 | dk<<2 | dl, a = 2 di + dj, b = 2 dk + dl; only the low bit of each
// field is read, so every byte names a row inside its block), hence
//   gA[n][4I + a] += g[v,I,J] * fb[bmap[v]][4J + b]   over J and the v with amap[v] == n,
//   gB[n][4J + b] += g[v,I,J] * fa[amap[v]][4I + a]   over I and the v with bmap[v] == n.
// Per volume that is a GEMM G . F whose left operand G [rows, reduced rows] has one
// non-zero per 4 x 4 block.  It runs on v_mfma_f32_16x16x32_bf16 as D^T = F^T . G^T:
//  * the A operand is the feature matrix of the reduced side, read with one 16-byte
//    load per lane from a transposed copy [image, K, ldr] (ldr = the reduced rows
//    rounded up to 32, zero filled), so a lane's 8 consecutive reduced rows are
//    contiguous;
//  * the B operand is G^T, generated in registers: a lane's 8 reduced rows are two
//    4-row blocks, i.e. two (g, code) pairs; g is rounded to bf16 (RNE) and placed at
//    the block's reduced sub-row when the code's output sub-row is the lane's row,
//    else the block is zero.  G is never materialised;
//  * the accumulator lane holds 4 consecutive channels of one output row: one
//    16-byte store.
// A workgroup (4 waves, 2 x 2) owns a 128-row x 128-channel tile of ONE output image
// and walks that image's volumes in the order of the host-built list with the same
// accumulators: every output element is written exactly once, no atomics, and the
// result does not depend on the launch (bit-identical runs).  An image without
// volumes gets zeros.  No LDS: the operands of an image (a few MB) stay in L2.
// The two directions are the two instantiations: DIR 0 gA (g indexed [out, red]),
// DIR 1 gB (g indexed [red, out], the generated operand is G^T).
#include "common.h"
#include "launchers.h"

namespace ncnet {

namespace cpb {
constexpr int TC = 4, TR = 4;            // a wave's 16-channel feature / 16-row generated fragments
constexpr int BR = 2 * 16 * TR, BC = 2 * 16 * TC;   // workgroup tile: 2 x 2 waves
}  // namespace cpb

struct PoolBwdArgs {
  const bf16* ft;          // [nother, K, ldr]: transposed features of the reduced side
  const float* g;          // [V, NI, NJ]
  const uint8_t* code;     // [V, NI, NJ]
  const int* off;          // [nout + 1]: the output image's slice of vol
  const int* vol;          // [V]: volumes grouped by output image
  const int* omap;         // [V]: image of the reduced side
  float* out;              // [nout, R, K]
  int V, nout, nother;
  int R, NR, ldr, K;       // output rows, reduced 4-row blocks, padded reduced rows, channels
  int NI, NJ;              // pooled grid sizes of g / code
  int tiles_r, tiles_c;
};

template <int DIR>
__global__ __launch_bounds__(256, 2) void corr_pool2_bwd_kernel(PoolBwdArgs p) {
  constexpr int TC = cpb::TC, TR = cpb::TR;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tc = bid % p.tiles_c; bid /= p.tiles_c;
  const int tr = bid % p.tiles_r;
  const int n = bid / p.tiles_r;
  const int row0 = tr * cpb::BR + (wave >> 1) * (16 * TR), kc0 = tc * cpb::BC + (wave & 1) * (16 * TC);

  // generated operand: the lane's output row of fragment j, its block and sub-row
  bool r_ok[TR];
  int g_base[TR], sub_out[TR];
  const int g_step = DIR == 0 ? 1 : p.NJ;            // g index step per reduced block
#pragma unroll
  for (int j = 0; j < TR; ++j) {
    const int orow = row0 + j * 16 + fr;
    r_ok[j] = orow < p.R;
    g_base[j] = DIR == 0 ? (orow >> 2) * p.NJ : (orow >> 2);
    sub_out[j] = orow & 3;
  }
  // feature operand: K % 16 == 0, a 16-channel fragment is inside or outside
  bool c_ok[TC];
  uint32_t f_off[TC];     // 32-bit element offsets from wave-uniform bases (the launcher bounds them)
#pragma unroll
  for (int i = 0; i < TC; ++i) {
    c_ok[i] = kc0 + i * 16 < p.K;
    f_off[i] = (uint32_t)(c_ok[i] ? kc0 + i * 16 + fr : 0) * (uint32_t)p.ldr + 8u * fq;
  }

  struct Raw {
    u32x4 f[TC];
    float g[TR][2];
    int c[TR][2];
  };
  const uint32_t vsz = (uint32_t)p.NI * (uint32_t)p.NJ, fsz = (uint32_t)p.K * (uint32_t)p.ldr;
  f32x4 acc[TC][TR];
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int j = 0; j < TR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int e0 = min(max(p.off[n], 0), p.V), e1 = min(max(p.off[n + 1], e0), p.V);
  for (int e = e0; e < e1; ++e) {
    // list entries are validated on the host; a bad one is skipped, never dereferenced
    const int v = p.vol[e];
    if ((unsigned)v >= (unsigned)p.V) continue;
    const int om = p.omap[v];
    if ((unsigned)om >= (unsigned)p.nother) continue;
    const bf16* ft = p.ft + (size_t)om * fsz;
    const float* gv = p.g + (size_t)v * vsz;
    const uint8_t* cv = p.code + (size_t)v * vsz;

    auto load = [&](int k0, Raw& r) {
#pragma unroll
      for (int i = 0; i < TC; ++i) {
        const uint32_t o = f_off[i] + (uint32_t)k0;
        r.f[i] = (c_ok[i] && NCNET_OK(o + 8 <= fsz)) ? *(const u32x4*)(ft + o) : u32x4{0u, 0u, 0u, 0u};
      }
      const int rb0 = (k0 >> 2) + 2 * fq;
#pragma unroll
      for (int j = 0; j < TR; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int rb = rb0 + t;
          const uint32_t o = (uint32_t)(g_base[j] + rb * g_step);
          const bool ok = r_ok[j] && rb < p.NR && NCNET_OK(o < vsz);
          r.g[j][t] = ok ? gv[o] : 0.f;
          r.c[j][t] = ok ? (int)cv[o] : 0;
        }
    };
    auto compute = [&](const Raw& r) {
      u32x4 gf[TR];
#pragma unroll
      for (int j = 0; j < TR; ++j) {
        uint32_t w[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int c = r.c[j][t];
          const int ca = ((c >> 5) & 2) | ((c >> 4) & 1), cb = ((c >> 1) & 2) | (c & 1);
          const int so = DIR == 0 ? ca : cb, sr = DIR == 0 ? cb : ca;
          const uint32_t gb = so == sub_out[j] ? (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)r.g[j][t]) : 0u;
          const uint32_t half = gb << ((sr & 1) * 16);
          w[2 * t] = (sr & 2) ? 0u : half;
          w[2 * t + 1] = (sr & 2) ? half : 0u;
        }
        gf[j] = u32x4{w[0], w[1], w[2], w[3]};
      }
#pragma unroll
      for (int j = 0; j < TR; ++j)
#pragma unroll
        for (int i = 0; i < TC; ++i) acc[i][j] = mfma16u(r.f[i], gf[j], acc[i][j]);
    };

    // two register sets in turn: the loads of step s + 1 are issued before the MFMAs of step s
    Raw ra, rb;
    load(0, ra);
    for (int k0 = 0; k0 < p.ldr; k0 += 64) {
      const bool odd = k0 + 32 < p.ldr;
      if (odd) load(k0 + 32, rb);
      compute(ra);
      if (odd) {
        if (k0 + 64 < p.ldr) load(k0 + 64, ra);
        compute(rb);
      }
    }
  }

  // accumulator: rows = channels 4 fq + r of fragment i, column = output row fr of fragment j
#pragma unroll
  for (int j = 0; j < TR; ++j) {
    const int orow = row0 + j * 16 + fr;
#pragma unroll
    for (int i = 0; i < TC; ++i) {
      const size_t o = ((size_t)n * p.R + orow) * p.K + kc0 + i * 16 + 4 * fq;
      if (r_ok[j] && c_ok[i] && NCNET_OK(o + 4 <= (size_t)p.nout * p.R * p.K)) *(f32x4*)(p.out + o) = acc[i][j];
    }
  }
}

}  // namespace ncnet

using namespace ncnet;

extern "C" int ncnet_corr_pool2_bwd(const void* ft, const float* g, const uint8_t* code, const int* off,
                                    const int* vol, const int* omap, float* out, int V, int nout, int nother, int dir,
                                    int hA, int wA, int hB, int wB, int K, int ldr, hipStream_t stream) {
  if ((hA & 1) || (wA & 1) || (hB & 1) || (wB & 1) || hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0) return -3;
  if (K <= 0 || K % 16 != 0 || V < 0 || nout < 0 || nother < 0 || (dir != 0 && dir != 1)) return -3;
  if (!aligned16(ft) || !aligned16(out)) return -3;   // 16-byte operand loads and output stores
  const int M = hA * wA, N = hB * wB;
  PoolBwdArgs p{};
  p.ft = (const bf16*)ft; p.g = g; p.code = code; p.off = off; p.vol = vol; p.omap = omap; p.out = out;
  p.V = V; p.nout = nout; p.nother = nother;
  p.R = dir == 0 ? M : N;
  p.NR = (dir == 0 ? N : M) / 4;
  if (ldr % 32 != 0 || ldr < 4 * p.NR) return -3;
  p.ldr = ldr; p.K = K;
  p.NI = M / 4; p.NJ = N / 4;
  p.tiles_r = cdiv(p.R, cpb::BR); p.tiles_c = cdiv(K, cpb::BC);
  const long long blocks = (long long)nout * p.tiles_r * p.tiles_c;
  // the kernel's per-image / per-volume element offsets are 32-bit
  if ((long long)K * ldr > 0x7fffffffLL || (long long)p.NI * p.NJ > 0x7fffffffLL) return -1;
  if (blocks == 0) return 0;
  if (blocks > 0x7fffffffLL) return -1;
  dim3 grid((unsigned)blocks), block(256);
  dispatch_int<0, 1>(dir, [&](auto dc) {   // dir is 0 or 1 (checked above)
    hipLaunchKernelGGL((corr_pool2_bwd_kernel<decltype(dc)::value>), grid, block, 0, stream, p);
  });
  return (int)hipGetLastError();
}
