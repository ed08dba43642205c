// Dense pose verification on the GPU (the batched form of
// ncnet_amd/eval/pose_verification.py; host side: eval/pose_verification_gpu.py).
//
// pv_render: z-buffer projection of ONE scan through C poses at once
// (points_to_perspective for every pose of a batch).  Three passes, integer
// atomics only, so a result does not depend on the order the lanes arrive in:
//   depth   one lane per point (grid-stride), inner loop over the launch's
//           poses, which sit in LDS (every lane reads the same pose: a
//           broadcast read): a point is read from HBM once for all poses.
//           p = KP (X, 1) in fp64, kept when z > 1e-9 and floor(p0 / z),
//           floor(p1 / z) fall inside the image -- tested on the floored
//           doubles, so NaN, Inf and huge values drop out by comparison and
//           nothing out of range is ever converted to an integer.  Then an
//           atomicMin of z's bit pattern (positive doubles order like their
//           bits) into zbuf[c][pixel], which starts at the bits of +inf.
//   resolve the same projection (same inline function, same bits); a point
//           whose z bits equal zbuf does an atomicMax of its index into
//           winner[c][pixel] (starts at -1): among points of one pixel with
//           bit-identical depth the highest index wins.
//   gather  one lane per (pose, pixel): synth = rgb[winner] or NaN, flag.
// A plain read of zbuf / winner before each atomic skips the ones that cannot
// change the cell (both only move one way, so a stale read is merely
// conservative).  A launch takes at most PMAX poses; the host loops.
//
// pv_desc_err: the second half of dense_sift + root_sift + the descriptor
// distance, fused.  Inputs are the pooled orientation maps [B, 8, H, W] of the
// query side and the synthetic side.  One wave per (candidate, keypoint); lane
// l owns entries l and l + 64 of the 128 (entry = (by * 4 + bx) * 8 + ori):
// gather -> L2 normalise -> clamp 0.2 -> L2 normalise -> L1 normalise -> sqrt
// for both sides, then sqrt(sum (a - b)^2), all reductions by wave shuffles.
// The [B, n, 128] descriptors are never written.  err is NaN where flag is
// false at the keypoint.
//
// Every loop's trip count is fixed by the launch arguments (points, poses);
// none depends on the data.
#include "common.h"
#include "launchers.h"

namespace ncnet {
namespace pv {

constexpr int PMAX = 32;          // poses per render launch (3 KB of LDS)
constexpr int WG = 256;
constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

// Pixel of point (x, y, z) under pose kp (row-major 3 x 4), and the bit pattern
// of its depth.  false: behind the camera, outside the image, or not finite.
__device__ __forceinline__ bool project(const double* kp, double x, double y, double z, int h, int w, int& pix,
                                        unsigned long long& zbits) {
  const double p0 = fma(kp[0], x, fma(kp[1], y, fma(kp[2], z, kp[3])));
  const double p1 = fma(kp[4], x, fma(kp[5], y, fma(kp[6], z, kp[7])));
  const double p2 = fma(kp[8], x, fma(kp[9], y, fma(kp[10], z, kp[11])));
  if (!(p2 > 1e-9)) return false;
  const double u = floor(p0 / p2), v = floor(p1 / p2);
  if (!(u >= 0.0 && u < (double)w && v >= 0.0 && v < (double)h)) return false;
  pix = (int)v * w + (int)u;
  zbits = (unsigned long long)__double_as_longlong(p2);
  return true;
}

template <bool RESOLVE>
__global__ __launch_bounds__(WG) void pv_points_kernel(const double* __restrict__ xyz, long long N,
                                                       const double* __restrict__ KP, int C, int h, int w,
                                                       unsigned long long* __restrict__ zbuf,
                                                       int* __restrict__ winner) {
  __shared__ double s_kp[PMAX * 12];
  for (int i = threadIdx.x; i < C * 12; i += WG) s_kp[i] = KP[i];
  __syncthreads();
  const long long hw = (long long)h * w;
  const long long stride = (long long)gridDim.x * WG;
  for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < N; i += stride) {
    if (!NCNET_OK(i >= 0 && i < N)) continue;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    for (int c = 0; c < C; ++c) {
      int pix;
      unsigned long long zb;
      if (!project(s_kp + 12 * c, x, y, z, h, w, pix, zb)) continue;
      if (!NCNET_OK(pix >= 0 && (long long)pix < hw)) continue;
      const long long cell = (long long)c * hw + pix;
      if constexpr (!RESOLVE) {
        if (zb < zbuf[cell]) atomicMin(zbuf + cell, zb);
      } else {
        if (zb == zbuf[cell] && (int)i > winner[cell]) atomicMax(winner + cell, (int)i);
      }
    }
  }
}

__global__ __launch_bounds__(WG) void pv_gather_kernel(const float* __restrict__ rgb, long long N,
                                                       const int* __restrict__ winner, long long cells,
                                                       float* __restrict__ synth, uint8_t* __restrict__ flag) {
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  if (t >= cells) return;
  int wi = winner[t];
  if (!NCNET_OK(wi >= -1 && (long long)wi < N)) wi = -1;
  const float nan = __builtin_nanf("");
  float r = nan, g = nan, b = nan;
  if (wi >= 0) {
    r = rgb[3 * (long long)wi];
    g = rgb[3 * (long long)wi + 1];
    b = rgb[3 * (long long)wi + 2];
  }
  synth[3 * t] = r;
  synth[3 * t + 1] = g;
  synth[3 * t + 2] = b;
  flag[t] = wi >= 0;
}

// RootSIFT of one descriptor held two entries per lane (dense_sift's
// normalisation chain, then root_sift's)
__device__ __forceinline__ void root_sift(float& a0, float& a1) {
  float n = sqrtf(wave_sum(a0 * a0 + a1 * a1));
  n = fmaxf(n, 1e-12f);
  a0 = fminf(a0 / n, 0.2f);
  a1 = fminf(a1 / n, 0.2f);
  n = sqrtf(wave_sum(a0 * a0 + a1 * a1));
  n = fmaxf(n, 1e-12f);
  a0 /= n;
  a1 /= n;
  const float s = fmaxf(wave_sum(fabsf(a0) + fabsf(a1)), 1e-12f);
  a0 = sqrtf(a0 / s);
  a1 = sqrtf(a1 / s);
}

constexpr int SIZE = 8, STEP = 4, FIRST = 2 * SIZE - 1;      // dense_sift(size 8, step 4)

__global__ __launch_bounds__(WG) void pv_desc_err_kernel(const float* __restrict__ oq, const float* __restrict__ os,
                                                         const uint8_t* __restrict__ flag, int B, int H, int W, int ny,
                                                         int nx, float* __restrict__ err) {
  const int lane = lane_id();
  const long long n = (long long)ny * nx;
  const long long item = (long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);    // wave-uniform
  if (item >= (long long)B * n) return;
  const int b = (int)(item / n), k = (int)(item % n);
  const int y = FIRST + STEP * (k / nx), x = FIRST + STEP * (k % nx);
  const long long hw = (long long)H * W;
  if (!NCNET_OK(y >= 0 && y < H && x >= 0 && x < W)) return;
  if (!flag[b * hw + (long long)y * W + x]) {
    if (lane == 0) err[item] = __builtin_nanf("");
    return;
  }
  float a[2], s[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = lane + 64 * j;
    const int iy = e >> 5, ix = (e >> 3) & 3, ori = e & 7;
    // bin centres at -12, -4, 4, 12 px from the keypoint, clamped to the image
    const int yy = min(max(y + SIZE * iy - 12, 0), H - 1);
    const int xx = min(max(x + SIZE * ix - 12, 0), W - 1);
    const long long off = ((long long)b * 8 + ori) * hw + (long long)yy * W + xx;
    const bool ok = NCNET_OK(off >= 0 && off < (long long)B * 8 * hw);
    a[j] = ok ? oq[off] : 0.f;
    s[j] = ok ? os[off] : 0.f;
  }
  root_sift(a[0], a[1]);
  root_sift(s[0], s[1]);
  const float d0 = a[0] - s[0], d1 = a[1] - s[1];
  const float e2 = wave_sum(d0 * d0 + d1 * d1);
  if (lane == 0) err[item] = sqrtf(e2);
}

}  // namespace pv
}  // namespace ncnet

using namespace ncnet::pv;

extern "C" int ncnet_pv_pmax() { return PMAX; }

extern "C" int ncnet_pv_render(const double* xyz, const float* rgb, long long N, const double* KP, int C, int h, int w,
                               unsigned long long* zbuf, int* winner, float* synth, uint8_t* flag,
                               hipStream_t stream) {
  if (C <= 0) return 0;
  if (C > PMAX || h < 1 || w < 1 || N < 0) return -1;
  const long long cells = (long long)C * h * w;
  if (N > 0) {
    const long long want = (N + WG - 1) / WG, cap = 8ll * device_num_cus();
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(pv_points_kernel<false>, dim3(grid), dim3(WG), 0, stream, xyz, N, KP, C, h, w, zbuf, winner);
    hipLaunchKernelGGL(pv_points_kernel<true>, dim3(grid), dim3(WG), 0, stream, xyz, N, KP, C, h, w, zbuf, winner);
  }
  hipLaunchKernelGGL(pv_gather_kernel, dim3((unsigned)((cells + WG - 1) / WG)), dim3(WG), 0, stream, rgb, N, winner,
                     cells, synth, flag);
  return (int)hipGetLastError();
}

extern "C" int ncnet_pv_desc_err(const float* oq, const float* os, const uint8_t* flag, int B, int H, int W, int ny,
                                 int nx, float* err, hipStream_t stream) {
  const long long items = (long long)B * ny * nx;
  if (items <= 0) return 0;
  const int wpb = WG / 64;
  hipLaunchKernelGGL(pv_desc_err_kernel, dim3((unsigned)((items + wpb - 1) / wpb)), dim3(WG), 0, stream, oq, os, flag,
                     B, H, W, ny, nx, err);
  return (int)hipGetLastError();
}
