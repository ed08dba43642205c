// Backbone epilogues for the frozen-trunk execution plan (models/backbones.py
// FrozenResNetPlan).  MIOpen's bf16 NHWC convolutions add a bias in a separate
// pass and PyTorch then runs ReLU / residual add as further passes (~7 full
// activation round trips per bottleneck).  The plan routes 1x1 convolutions
// to hipBLASLt GEMMs (bias + ReLU in the GEMM epilogue, residual as the C
// operand) and finishes everything else with this single in-place pass:
//
//   Y[r, c] = act(Y[r, c] + b[c])          (bf16 rows of C channels, fp32 bias)
#include "common.h"
#include "launchers.h"

namespace ncnet {

// 8 channels (16 B) per thread; C % 8 == 0.  F16: Y is IEEE half.
template <bool RELU, bool F16>
__global__ __launch_bounds__(256) void bias_act_kernel(uint16_t* __restrict__ Y, const float* __restrict__ b,
                                                       long long n8, int C8) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n8) return;
  const int c0 = (int)(e % C8) * 8;
  u32x4 v = *(const u32x4*)(Y + e * 8);
  const f32x4 b0 = *(const f32x4*)(b + c0), b1 = *(const f32x4*)(b + c0 + 4);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t w = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 2 * q + h;
      float x = s162f<F16>((uint16_t)(v[q] >> (16 * h))) + (k < 4 ? b0[k] : b1[k - 4]);
      if (RELU) x = fmaxf(x, 0.f);
      w |= (uint32_t)f2s16<F16>(x) << (16 * h);
    }
    v[q] = w;
  }
  *(u32x4*)(Y + e * 8) = v;
}

// Stem finish: Y = act(maxpool_{k,s,p}(X) + b) in ONE pass over the stem conv
// output (NHWC, C % 8 == 0).  Equal to maxpool(act(X + b)) bit for bit:
// x -> round(act(x + b)) is monotonic per channel, so it commutes with max,
// and padded taps are skipped (MaxPool2d pads with -inf).  Replaces an
// in-place bias_act pass + PyTorch's max_pool2d (three full-size activation
// passes -> one read of the conv output; 2.9 -> ~0.4 ms per 11 images at 3200 px).
template <bool RELU, bool F16>
__global__ __launch_bounds__(256) void maxpool_bias_act_kernel(const uint16_t* __restrict__ X, uint16_t* __restrict__ Y,
                                                               const float* __restrict__ b, int N, int H, int W, int C8,
                                                               int Ho, int Wo, int k, int st, int pad) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)N * Ho * Wo * C8;
  if (e >= total) return;
  const int c8 = (int)(e % C8);
  long long r = e / C8;
  const int wo = (int)(r % Wo); r /= Wo;
  const int ho = (int)(r % Ho);
  const int n = (int)(r / Ho);
  float m[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) m[q] = -INFINITY;
  const int h0 = ho * st - pad, w0 = wo * st - pad;
  for (int dh = 0; dh < k; ++dh) {
    const int h = h0 + dh;
    if (h < 0 || h >= H) continue;
    for (int dw = 0; dw < k; ++dw) {
      const int w = w0 + dw;
      if (w < 0 || w >= W) continue;
      const u32x4 v = *(const u32x4*)(X + ((((size_t)n * H + h) * W + w) * C8 + c8) * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        m[2 * q] = fmaxf(m[2 * q], s162f<F16>((uint16_t)(v[q] & 0xffffu)));
        m[2 * q + 1] = fmaxf(m[2 * q + 1], s162f<F16>((uint16_t)(v[q] >> 16)));
      }
    }
  }
  const f32x4 b0 = *(const f32x4*)(b + c8 * 8), b1 = *(const f32x4*)(b + c8 * 8 + 4);
  u32x4 out;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t wv = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kk = 2 * q + h;
      float x = m[kk] + (kk < 4 ? b0[kk] : b1[kk - 4]);
      if (RELU) x = fmaxf(x, 0.f);
      wv |= (uint32_t)f2s16<F16>(x) << (16 * h);
    }
    out[q] = wv;
  }
  *(u32x4*)(Y + e * 8) = out;
}

// ---------------------------------------------------------------------------
// bf16x3 (fp32-accurate) trunk helpers (FrozenResNetPlan in float32): the
// activations are [N, H, W, 2C] bf16 with hi = bf16(x) in channels [0, C) and
// lo = bf16(x - hi) in [C, 2C); the convs run on conv2d_nhwc_v3's X3 mode.

// Stem im2col: fp32 NHWC image [N, H, W, Cin] -> A [N*Ho*Wo, 2 KP] pairs with
// k = (kh * KW + kw) * Cin + c (the channels-last weight order), zero for
// padding taps and k >= KH*KW*Cin (KP % 8 == 0).  One thread = 8 k.
__global__ __launch_bounds__(256) void stem_im2col_x3_kernel(const float* __restrict__ X, uint16_t* __restrict__ A,
                                                             int N, int H, int W, int Cin, int KH, int KW, int st,
                                                             int pad, int Ho, int Wo, int KP) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int kp8 = KP / 8;
  const long long total = (long long)N * Ho * Wo * kp8;
  if (e >= total) return;
  const int k0 = (int)(e % kp8) * 8;
  long long r = e / kp8;
  const int wo = (int)(r % Wo); r /= Wo;
  const int ho = (int)(r % Ho);
  const int n = (int)(r / Ho);
  const int K = KH * KW * Cin;
  u32x4 oh, ol;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t wh = 0, wl = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = k0 + 2 * q + h;
      float v = 0.f;
      if (k < K) {
        const int c = k % Cin, t = k / Cin, kw = t % KW, kh = t / KW;
        const int hi = ho * st - pad + kh, wi = wo * st - pad + kw;
        if (hi >= 0 && hi < H && wi >= 0 && wi < W) v = X[(((size_t)n * H + hi) * W + wi) * Cin + c];
      }
      const uint16_t hb = f2s16<false>(v);
      wh |= (uint32_t)hb << (16 * h);
      wl |= (uint32_t)f2s16<false>(v - s162f<false>(hb)) << (16 * h);
    }
    oh[q] = wh; ol[q] = wl;
  }
  const size_t row = ((size_t)n * Ho + ho) * Wo + wo;
  *(u32x4*)(A + row * 2 * KP + k0) = oh;
  *(u32x4*)(A + row * 2 * KP + KP + k0) = ol;
}

// k x k / stride max-pool of hi/lo pairs (the value is hi + lo in fp32;
// padded taps skipped as MaxPool2d's -inf padding), X [N,H,W,2C] -> Y [N,Ho,Wo,2C].
__global__ __launch_bounds__(256) void maxpool_x3_kernel(const uint16_t* __restrict__ X, uint16_t* __restrict__ Y,
                                                         int N, int H, int W, int C, int Ho, int Wo, int k, int st,
                                                         int pad) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C8 = C / 8;
  const long long total = (long long)N * Ho * Wo * C8;
  if (e >= total) return;
  const int c8 = (int)(e % C8);
  long long r = e / C8;
  const int wo = (int)(r % Wo); r /= Wo;
  const int ho = (int)(r % Ho);
  const int n = (int)(r / Ho);
  float m[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) m[q] = -INFINITY;
  const int h0 = ho * st - pad, w0 = wo * st - pad;
  for (int dh = 0; dh < k; ++dh) {
    const int h = h0 + dh;
    if (h < 0 || h >= H) continue;
    for (int dw = 0; dw < k; ++dw) {
      const int w = w0 + dw;
      if (w < 0 || w >= W) continue;
      const uint16_t* px = X + (((size_t)n * H + h) * W + w) * 2 * C + c8 * 8;
      const u32x4 vh = *(const u32x4*)px, vl = *(const u32x4*)(px + C);
#pragma unroll
      for (int q = 0; q < 8; ++q)
        m[q] = fmaxf(m[q], s162f<false>((uint16_t)(vh[q >> 1] >> (16 * (q & 1)))) +
                               s162f<false>((uint16_t)(vl[q >> 1] >> (16 * (q & 1)))));
    }
  }
  u32x4 oh, ol;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t wh = 0, wl = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float v = m[2 * q + h];
      const uint16_t hb = f2s16<false>(v);
      wh |= (uint32_t)hb << (16 * h);
      wl |= (uint32_t)f2s16<false>(v - s162f<false>(hb)) << (16 * h);
    }
    oh[q] = wh; ol[q] = wl;
  }
  uint16_t* py = Y + (((size_t)n * Ho + ho) * Wo + wo) * 2 * C + c8 * 8;
  *(u32x4*)py = oh;
  *(u32x4*)(py + C) = ol;
}

// hi/lo pairs [rows, 2C] -> fp32 [rows, C] (hi + lo)
__global__ __launch_bounds__(256) void x3_to_f32_kernel(const uint16_t* __restrict__ X, float* __restrict__ Y,
                                                        long long rows, int C) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C8 = C / 8;
  if (e >= rows * C8) return;
  const long long r = e / C8;
  const int c8 = (int)(e % C8);
  const uint16_t* px = X + r * 2 * C + c8 * 8;
  const u32x4 vh = *(const u32x4*)px, vl = *(const u32x4*)(px + C);
  f32x4 a, b;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a[q] = s162f<false>((uint16_t)(vh[q >> 1] >> (16 * (q & 1)))) + s162f<false>((uint16_t)(vl[q >> 1] >> (16 * (q & 1))));
    b[q] = s162f<false>((uint16_t)(vh[2 + (q >> 1)] >> (16 * (q & 1)))) +
           s162f<false>((uint16_t)(vl[2 + (q >> 1)] >> (16 * (q & 1))));
  }
  *(f32x4*)(Y + r * C + c8 * 8) = a;
  *(f32x4*)(Y + r * C + c8 * 8 + 4) = b;
}

// Sanitizer-tier self test: out[0] = 1 in release; in the debug build the
// check fails on purpose (n >= 0), prints its NCNET_CHECK line and out[0] = 0.
__global__ void debug_selftest_kernel(int* out, int n) {
  if (threadIdx.x == 0) out[0] = NCNET_OK(n < 0) ? 1 : 0;
}

}  // namespace ncnet

using namespace ncnet;

extern "C" int ncnet_debug_selftest(int* out, hipStream_t stream) {
  hipLaunchKernelGGL(debug_selftest_kernel, dim3(1), dim3(64), 0, stream, out, 1);
  return (int)hipGetLastError();
}

extern "C" int ncnet_bias_act(void* Y, const float* b, long long rows, int C, int relu, int f16, hipStream_t stream) {
  if (C % 8) return -1;
  const long long n8 = rows * (C / 8);
  if (n8 == 0) return 0;
  dim3 grid((unsigned)((n8 + 255) / 256)), block(256);
  uint16_t* y = (uint16_t*)Y;
  dispatch_bool(relu != 0, [&](auto rc) {
    dispatch_bool(f16 != 0, [&](auto hc) {
      hipLaunchKernelGGL((bias_act_kernel<decltype(rc)::value, decltype(hc)::value>), grid, block, 0, stream, y, b, n8,
                         C / 8);
    });
  });
  return (int)hipGetLastError();
}

extern "C" int ncnet_maxpool_bias_act(const void* X, void* Y, const float* b, int N, int H, int W, int C, int Ho,
                                      int Wo, int k, int stride, int pad, int relu, int f16, hipStream_t stream) {
  if (C % 8 || k < 1 || stride < 1 || pad < 0 || 2 * pad > k) return -1;
  const long long total = (long long)N * Ho * Wo * (C / 8);
  if (total == 0) return 0;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const uint16_t* x = (const uint16_t*)X; uint16_t* y = (uint16_t*)Y;
  dispatch_bool(relu != 0, [&](auto rc) {
    dispatch_bool(f16 != 0, [&](auto hc) {
      hipLaunchKernelGGL((maxpool_bias_act_kernel<decltype(rc)::value, decltype(hc)::value>), grid, block, 0, stream, x,
                         y, b, N, H, W, C / 8, Ho, Wo, k, stride, pad);
    });
  });
  return (int)hipGetLastError();
}

extern "C" int ncnet_stem_im2col_x3(const float* X, void* A, int N, int H, int W, int Cin, int KH, int KW, int stride,
                                    int pad, int Ho, int Wo, int KP, hipStream_t stream) {
  if (KP % 8 || KP < KH * KW * Cin) return -1;
  const long long total = (long long)N * Ho * Wo * (KP / 8);
  if (total == 0) return 0;
  hipLaunchKernelGGL(stem_im2col_x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, X,
                     (uint16_t*)A, N, H, W, Cin, KH, KW, stride, pad, Ho, Wo, KP);
  return (int)hipGetLastError();
}

extern "C" int ncnet_maxpool_x3(const void* X, void* Y, int N, int H, int W, int C, int Ho, int Wo, int k, int stride,
                                int pad, hipStream_t stream) {
  if (C % 8 || k < 1 || stride < 1 || pad < 0 || 2 * pad > k) return -1;
  const long long total = (long long)N * Ho * Wo * (C / 8);
  if (total == 0) return 0;
  hipLaunchKernelGGL(maxpool_x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                     (const uint16_t*)X, (uint16_t*)Y, N, H, W, C, Ho, Wo, k, stride, pad);
  return (int)hipGetLastError();
}

extern "C" int ncnet_x3_to_f32(const void* X, float* Y, long long rows, int C, hipStream_t stream) {
  if (C % 8) return -1;
  const long long total = rows * (C / 8);
  if (total == 0) return 0;
  hipLaunchKernelGGL(x3_to_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                     (const uint16_t*)X, Y, rows, C);
  return (int)hipGetLastError();
}

// gather_bf16: out[i] = bf16(src[idx[i]]) (0 where idx[i] < 0) -- the per-step
// weight packs as one launch (ops/packing.py gather_pack)
// (an index past the source -- nsrc elements -- also reads as 0: never a fault)
__global__ __launch_bounds__(256) void gather_bf16_kernel(const float* __restrict__ src, const int* __restrict__ idx,
                                                          __bf16* __restrict__ out, long long n, long long nsrc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = idx[i];
  out[i] = (__bf16)(j >= 0 && j < nsrc ? src[j] : 0.f);
}
extern "C" int ncnet_gather_bf16(const float* src, const int* idx, void* out, long long n, long long nsrc,
                                 hipStream_t s) {
  hipLaunchKernelGGL(gather_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, idx, (__bf16*)out, n,
                     nsrc);
  return (int)hipGetLastError();
}

// reduce_cols: per segment s, for every source column j < N_s
//   dst_s[map_s(j)] = sum_{r < R_s} src_s[r * N_s + j]
// map = idx_s[j] (a layout permutation; < 0 drops the column) or j (idx null);
// the weight-gradient partials of the NeighConsensus layers reduced and laid
// out in the checkpoint layout in one launch (ops/nc/layers.py
// reduce_partials).  A block owns 64 column quads; its 4 row slices sum rows
// r = slice (mod 4) and are combined in a fixed order through LDS, so the
// result is the same on every run.
struct RedSeg {
  const float* src;
  float* dst;
  const int* idx;
  int R, N;
  int blk0;         // first block of this segment
  long long ndst;   // dst elements: a map entry past them is dropped (never a fault)
};
struct RedSegs { RedSeg s[4]; int nseg; };

__global__ __launch_bounds__(256) void reduce_cols_kernel(RedSegs a) {
  __shared__ f32x4 part[4][64];
  int si = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (k < a.nseg && (int)blockIdx.x >= a.s[k].blk0) si = k;
  const RedSeg sg = a.s[si];
  const int cq = ((int)blockIdx.x - sg.blk0) * 64 + (threadIdx.x & 63);
  const int slice = threadIdx.x >> 6;
  const int nq = sg.N >> 2;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (cq < nq) {
    const f32x4* src = (const f32x4*)sg.src + cq;
    f32x4 acc1 = acc;
    int r = slice;
    for (; r + 4 < sg.R; r += 8) {
      acc += src[(size_t)r * nq];
      acc1 += src[(size_t)(r + 4) * nq];
    }
    if (r < sg.R) acc += src[(size_t)r * nq];
    acc += acc1;
  }
  part[slice][threadIdx.x & 63] = acc;
  __syncthreads();
  if (slice == 0 && cq < nq) {
    const f32x4 t = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = cq * 4 + e;
      const int o = sg.idx ? sg.idx[j] : j;
      if (o >= 0 && o < sg.ndst) sg.dst[o] = t[e];
    }
  }
}

extern "C" int ncnet_reduce_cols(const float* const* src, float* const* dst, const int* const* idx, const int* R,
                                 const int* N, const long long* ndst, int nseg, hipStream_t s) {
  if (nseg < 1 || nseg > 4) return -2;
  RedSegs a{};
  a.nseg = nseg;
  int blk = 0;
  for (int k = 0; k < nseg; ++k) {
    if (N[k] % 4 || R[k] < 1) return -3;
    a.s[k] = RedSeg{src[k], dst[k], idx[k], R[k], N[k], blk, ndst[k]};
    blk += (N[k] / 4 + 63) / 64;
  }
  hipLaunchKernelGGL(reduce_cols_kernel, dim3((unsigned)blk), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
