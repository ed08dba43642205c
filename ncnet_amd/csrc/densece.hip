// Dense correspondence cross-entropy on a 1-channel correlation volume viewed
// as x [B, R = hA*wA (A cells), C = hB*wB (B cells)] fp32 (ops/loss.py
// warp_loss_from_corr; the contract is ops/reference.py dense_ce).
//
// Both views of a pair are affine warps of one image, so every cell of one
// view has a closed-form position in the other.  warp_maps [B, 2, 12] fp64
// holds, per image and side (0: the A cells, 1: the B cells), two affine maps
// (m00, m01, c0, m10, m11, c1) on unit coordinates: entries 0..5 into the
// other view, 6..11 into the source image.  A cell is valid when both images
// of its centre lie in [0, 1]^2; its target is four cells of the other grid
// with bilinear weights (the mapping of kploss.hip kp_axis).  With V_r the
// weights of valid A cell r on the B grid and U_m those of valid B cell m on
// the A grid:
//   loss = 1/2 (sum_r -V_r . log_softmax(x[r, :]) / max(1, N_A)
//               + sum_m -U_m . log_softmax(x[:, m]) / max(1, N_B))
//
//  * densece_table_kernel: one thread per (image, side, cell): cells, weights
//    and the valid flag, struct-of-arrays [B, 2, 4, n] / [B, 2, n] with
//    n = max(R, C), so neighbouring threads of the backward read neighbouring
//    entries.  Entries past a side's cell count and invalid cells are zero.
//  * densece_fwd_kernel: one thread per (image, side, cell): the line's
//    log-sum-exp from the stats2d statistics (max + log sum exp) and the term
//    lse - sum_k w_k x[cell_k] (four gathers); for an invalid cell the term is
//    0 and the stored log-sum-exp +inf.
//  * densece_reduce: one wave per (image, side) sums terms and valid flags in
//    double (lane-strided, xor tree), then one wave over those partials writes
//    out[3] = (loss, 1 / (2 max(1, N_A)), 1 / (2 max(1, N_B))), which stay on
//    the device for the backward.  Fixed order, no atomics.
//  * densece_bwd_kernel: elementwise over the flat volume, four consecutive
//    elements per thread (16-byte access; a lane's elements may straddle a
//    row, so (r, m) is derived per element); every element of gx is written
//    exactly once:
//      gx[r, m] = g (validA_r (exp(x - lseA_r) - V_r(m)) / (2 N_A)
//                    + validB_m (exp(x - lseB_m) - U_m(r)) / (2 N_B))
//    V_r(m) / U_m(r) by comparing m with row r's four cells and r with column
//    m's four cells (coinciding cells add up).  An invalid line needs no flag:
//    its log-sum-exp is +inf (exp gives 0) and its weights are 0.  Per element
//    the kernel reads the column's first and last cell and log-sum-exp; the
//    other cells and the weights only where the index lies between them.
#include "common.h"
#include "launchers.h"

namespace ncnet {

constexpr int DC_THREADS = 256;

// cells i0, i1 and the fraction f of unit coordinate q on an n-cell axis:
// u = clamp(q (n - 1), 0, n - 1).  fmax / fmin drop a NaN, so the cells are in
// range for any input.
__device__ __forceinline__ void dc_axis(double q, int n, int& i0, int& i1, float& f) {
  double u = q * (double)(n - 1);
  u = fmin(fmax(u, 0.0), (double)(n - 1));
  i0 = min((int)floor(u), max(n - 2, 0));
  i1 = min(i0 + 1, n - 1);
  f = (float)(u - (double)i0);
}

__device__ __forceinline__ bool dc_in_unit(double v) { return v >= 0.0 && v <= 1.0; }

// grid: ceil(B * 2 * n / DC_THREADS) workgroups, thread id = (b * 2 + side) * n + t
__global__ __launch_bounds__(DC_THREADS) void densece_table_kernel(const double* __restrict__ maps, int B, int hA,
                                                                   int wA, int hB, int wB, int n,
                                                                   int* __restrict__ cells, float* __restrict__ wts,
                                                                   int* __restrict__ valid) {
  const long long idx = (long long)blockIdx.x * DC_THREADS + threadIdx.x;
  if (idx >= (long long)B * 2 * n) return;
  const int t = (int)(idx % n);
  const long long bs = idx / n;                        // b * 2 + side
  const int side = (int)(bs & 1);
  const int h = side ? hB : hA, w = side ? wB : wA;    // this side's grid
  const int gh = side ? hA : hB, gw = side ? wA : wB;  // the other grid
  int c[4] = {0, 0, 0, 0};
  float wt[4] = {0.f, 0.f, 0.f, 0.f};
  int ok = 0;
  if (t < h * w) {
    // the oracle's roundings (ops/reference.py dense_targets): no fused multiply-adds in the mapping
#pragma clang fp contract(off)
    const double* m = maps + bs * 12;
    const int i = t / w, j = t - i * w;
    const double ux = w > 1 ? (double)j / (double)(w - 1) : 0.0;
    const double uy = h > 1 ? (double)i / (double)(h - 1) : 0.0;
    const double qx = m[0] * ux + m[1] * uy + m[2], qy = m[3] * ux + m[4] * uy + m[5];
    const double sx = m[6] * ux + m[7] * uy + m[8], sy = m[9] * ux + m[10] * uy + m[11];
    ok = (dc_in_unit(qx) && dc_in_unit(qy) && dc_in_unit(sx) && dc_in_unit(sy)) ? 1 : 0;
    if (ok) {
      int i0, i1, j0, j1;
      float fi, fj;
      dc_axis(qy, gh, i0, i1, fi);
      dc_axis(qx, gw, j0, j1, fj);
      c[0] = i0 * gw + j0; wt[0] = (1.f - fi) * (1.f - fj);
      c[1] = i0 * gw + j1; wt[1] = (1.f - fi) * fj;
      c[2] = i1 * gw + j0; wt[2] = fi * (1.f - fj);
      c[3] = i1 * gw + j1; wt[3] = fi * fj;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cells[(bs * 4 + k) * n + t] = c[k];
    wts[(bs * 4 + k) * n + t] = wt[k];
  }
  valid[bs * n + t] = ok;
}

// grid and thread id as densece_table_kernel
__global__ __launch_bounds__(DC_THREADS) void densece_fwd_kernel(
    const float* __restrict__ x, const int* __restrict__ cells, const float* __restrict__ wts,
    const int* __restrict__ valid, const float* __restrict__ rmax, const float* __restrict__ rse,
    const float* __restrict__ cmax, const float* __restrict__ cse, int B, int R, int C, int n,
    float* __restrict__ lse, float* __restrict__ term) {
  const long long idx = (long long)blockIdx.x * DC_THREADS + threadIdx.x;
  if (idx >= (long long)B * 2 * n) return;
  const int t = (int)(idx % n);
  const long long bs = idx / n;
  const int side = (int)(bs & 1);
  const long long b = bs >> 1;
  const int ns = side ? C : R;                         // this side's cells
  const int no = side ? R : C;                         // the other side's
  float l = INFINITY, tm = 0.f;                        // +inf: what the backward reads for a line without a term
  if (t < ns && valid[bs * n + t]) {
    l = side ? cmax[b * C + t] + logf(cse[b * C + t]) : rmax[b * R + t] + logf(rse[b * R + t]);
    const float* xb = x + (size_t)b * R * C;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cells[(bs * 4 + k) * n + t];
      if (!NCNET_OK(c >= 0 && c < no)) continue;
      acc += wts[(bs * 4 + k) * n + t] * (side ? xb[(size_t)c * C + t] : xb[(size_t)t * C + c]);
    }
    tm = l - acc;
  }
  lse[idx] = l;
  term[idx] = tm;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid: B * 2 workgroups of one wave: part[(b * 2 + side) * 2] = (sum of terms, number of valid cells)
__global__ __launch_bounds__(64) void densece_partial_kernel(const float* __restrict__ term,
                                                             const int* __restrict__ valid, int n,
                                                             double* __restrict__ part) {
  const long long bs = blockIdx.x;
  double s = 0.0, c = 0.0;
  for (int t = threadIdx.x; t < n; t += 64) {
    s += (double)term[bs * n + t];
    c += (double)valid[bs * n + t];
  }
  s = wave_sum_f64(s);
  c = wave_sum_f64(c);
  if (threadIdx.x == 0) { part[bs * 2] = s; part[bs * 2 + 1] = c; }
}

// one wave: out = (loss, 1 / (2 max(1, N_A)), 1 / (2 max(1, N_B)))
__global__ __launch_bounds__(64) void densece_final_kernel(const double* __restrict__ part, int B,
                                                           float* __restrict__ out) {
  double sa = 0.0, ca = 0.0, sb = 0.0, cb = 0.0;
  for (int b = threadIdx.x; b < B; b += 64) {
    sa += part[(size_t)b * 4]; ca += part[(size_t)b * 4 + 1];
    sb += part[(size_t)b * 4 + 2]; cb += part[(size_t)b * 4 + 3];
  }
  sa = wave_sum_f64(sa); ca = wave_sum_f64(ca);
  sb = wave_sum_f64(sb); cb = wave_sum_f64(cb);
  if (threadIdx.x == 0) {
    const double ka = 1.0 / (2.0 * fmax(ca, 1.0)), kb = 1.0 / (2.0 * fmax(cb, 1.0));
    out[0] = (float)(sa * ka + sb * kb);
    out[1] = (float)ka;
    out[2] = (float)kb;
  }
}

// What the backward reads per line (row r: side 0, column m: side 1): the first and the last of its four
// cells -- c[0] <= c[1], c[2] <= c[3], so only an index inside [c0, c3] can meet one of them -- and its
// log-sum-exp, +inf for an invalid line (exp(x - inf) = 0 and its weights are 0: no term, no flag to read).
struct DcKey { int c0, c3; float lse; };

__device__ __forceinline__ DcKey dc_key(const int* __restrict__ cells, const float* __restrict__ lse, long long bs,
                                        int n, int t) {
  DcKey q;
  q.c0 = cells[(bs * 4) * n + t];
  q.c3 = cells[(bs * 4 + 3) * n + t];
  q.lse = lse[bs * n + t];
  return q;
}

// the weight of line t on cell i of the other grid (coinciding cells add up); the table is read only
// where i falls into the line's cell range: about one grid row of the plane
__device__ __forceinline__ float dc_weight(const DcKey& q, const int* __restrict__ cells,
                                           const float* __restrict__ wts, long long bs, int n, int t, int i) {
  float w = 0.f;
  if (i >= q.c0 && i <= q.c3) {
    const int c1 = cells[(bs * 4 + 1) * n + t], c2 = cells[(bs * 4 + 2) * n + t];
    w += q.c0 == i ? wts[(bs * 4) * n + t] : 0.f;
    w += c1 == i ? wts[(bs * 4 + 1) * n + t] : 0.f;
    w += c2 == i ? wts[(bs * 4 + 2) * n + t] : 0.f;
    w += q.c3 == i ? wts[(bs * 4 + 3) * n + t] : 0.f;
  }
  return w;
}

// grid: ceil(ceil(total / 4) / DC_THREADS) workgroups; thread i owns elements 4 i .. 4 i + 3 of the flat volume.
// VEC: x and gx are 16-byte aligned (one 16-byte load and store per full group; the tail group is scalar).
template <bool VEC>
__global__ __launch_bounds__(DC_THREADS) void densece_bwd_kernel(
    const float* __restrict__ x, const int* __restrict__ cells, const float* __restrict__ wts,
    const float* __restrict__ lse, const float* __restrict__ scales, const float* __restrict__ gscale,
    float* __restrict__ gx, long long total, int R, int C, int n) {
  const long long e0 = ((long long)blockIdx.x * DC_THREADS + threadIdx.x) * 4;
  if (e0 >= total) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const float ka = scales[1] * gs, kb = scales[2] * gs;
  long long b;
  int r, m;
  if (total <= 0xffffffffLL) {                         // 32-bit divisions (total is uniform)
    const unsigned e = (unsigned)e0, rc = (unsigned)R * (unsigned)C;
    const unsigned bq = e / rc, rem = e - bq * rc;
    b = bq;
    r = (int)(rem / (unsigned)C);
    m = (int)(rem - (unsigned)r * (unsigned)C);
  } else {
    const long long RC = (long long)R * C;
    b = e0 / RC;
    const long long rem = e0 - b * RC;
    r = (int)(rem / C);
    m = (int)(rem - (long long)r * C);
  }
  const int cnt = (int)((total - e0) < 4 ? (total - e0) : 4);
  float xv[4] = {0.f, 0.f, 0.f, 0.f}, g[4];
  if (VEC && cnt == 4) {
    const float4 q = *(const float4*)(x + e0);
    xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) xv[k] = x[e0 + k];
  }
  DcKey row = dc_key(cells, lse, b * 2, n, r);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < cnt) {
      const DcKey col = dc_key(cells, lse, b * 2 + 1, n, m);
      const float V = dc_weight(row, cells, wts, b * 2, n, r, m);
      const float U = dc_weight(col, cells, wts, b * 2 + 1, n, m, r);
      g[k] = ka * (__expf(xv[k] - row.lse) - V) + kb * (__expf(xv[k] - col.lse) - U);
      if (++m == C) {                                  // the next element starts a row (of the next image after the last row)
        m = 0;
        if (++r == R) { r = 0; ++b; }
        if (k + 1 < cnt) row = dc_key(cells, lse, b * 2, n, r);
      }
    }
  }
  if (VEC && cnt == 4) {
    *(float4*)(gx + e0) = make_float4(g[0], g[1], g[2], g[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) gx[e0 + k] = g[k];
  }
}

}  // namespace ncnet

using namespace ncnet;

// The launchers' contracts are in launchers.h.
static inline long long dc_cdiv(long long a, long long b) { return (a + b - 1) / b; }
static inline bool dc_geometry_ok(int B, int R, int C, int n) {
  return B >= 1 && R >= 1 && C >= 1 && n == (R > C ? R : C) &&
         dc_cdiv((long long)B * 2 * n, DC_THREADS) <= 0x7fffffffLL;
}
extern "C" int ncnet_densece_table(const double* maps, int B, int hA, int wA, int hB, int wB, int n, int* cells,
                                   float* wts, int* valid, hipStream_t s) {
  if (hA < 1 || wA < 1 || hB < 1 || wB < 1) return -3;
  if ((long long)hA * wA > 0x7fffffffLL || (long long)hB * wB > 0x7fffffffLL) return -1;
  if (!dc_geometry_ok(B, hA * wA, hB * wB, n)) return -3;
  const unsigned nblk = (unsigned)dc_cdiv((long long)B * 2 * n, DC_THREADS);
  hipLaunchKernelGGL(densece_table_kernel, dim3(nblk), dim3(DC_THREADS), 0, s, maps, B, hA, wA, hB, wB, n, cells, wts,
                     valid);
  return (int)hipGetLastError();
}
extern "C" int ncnet_densece_fwd(const float* x, const int* cells, const float* wts, const int* valid,
                                 const float* rmax, const float* rse, const float* cmax, const float* cse, int B, int R,
                                 int C, int n, float* lse, float* term, hipStream_t s) {
  if (!dc_geometry_ok(B, R, C, n)) return -3;
  const unsigned nblk = (unsigned)dc_cdiv((long long)B * 2 * n, DC_THREADS);
  hipLaunchKernelGGL(densece_fwd_kernel, dim3(nblk), dim3(DC_THREADS), 0, s, x, cells, wts, valid, rmax, rse, cmax, cse,
                     B, R, C, n, lse, term);
  return (int)hipGetLastError();
}
extern "C" int ncnet_densece_reduce(const float* term, const int* valid, int B, int n, double* part, float* out,
                                    hipStream_t s) {
  if (B < 1 || n < 1 || (long long)B * 2 > 0x7fffffffLL) return -3;
  hipLaunchKernelGGL(densece_partial_kernel, dim3((unsigned)(B * 2)), dim3(64), 0, s, term, valid, n, part);
  hipLaunchKernelGGL(densece_final_kernel, dim3(1), dim3(64), 0, s, part, B, out);
  return (int)hipGetLastError();
}
extern "C" int ncnet_densece_bwd(const float* x, const int* cells, const float* wts, const float* lse,
                                 const float* scales, const float* gscale, float* gx, int B, int R, int C, int n,
                                 hipStream_t s) {
  if (!dc_geometry_ok(B, R, C, n)) return -3;
  const long long total = (long long)B * R * C;
  const long long nblk = dc_cdiv(dc_cdiv(total, 4), DC_THREADS);
  if (nblk > 0x7fffffffLL) return -1;
  dispatch_bool(aligned16(x) && aligned16(gx), [&](auto vec) {
    hipLaunchKernelGGL((densece_bwd_kernel<decltype(vec)::value>), dim3((unsigned)nblk), dim3(DC_THREADS), 0, s, x,
                       cells, wts, lse, scales, gscale, gx, total, R, C, n);
  });
  return (int)hipGetLastError();
}
