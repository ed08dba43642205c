// Keypoint-supervised loss on a 1-channel correlation volume viewed as
// x [B, R = hA*wA (A cells), C = hB*wB (B cells)] fp32 (ops/loss.py
// strong_loss_from_corr; the contract is ops/reference.py keypoint_ce).
//
// A keypoint pair (source point on image A, target point on image B) becomes
// four cells a_k with bilinear weights u_k on the A grid and four cells b_k
// with weights v_k on the B grid, by the mapping the PCK evaluation uses
// (eval/point_tnf.py normalize_axis).  Per valid keypoint:
//   s[m] = sum_k u_k x[a_k, m],  L_ab = -sum_k v_k log_softmax(s)[b_k]
//   t[r] = sum_k v_k x[r, b_k],  L_ba = -sum_k u_k log_softmax(t)[a_k]
//   loss = sum (L_ab + L_ba) / (2 max(1, Nvalid))
//
//  * kploss_fwd_kernel: one workgroup per (image, keypoint, direction).  It
//    builds the cell / weight table from the raw points, forms the blended
//    line (s: four contiguous rows; t: four strided columns) and keeps a
//    running (max, sum exp) per thread -- one pass over global memory -- merged
//    in a fixed order; writes the log-sum-exp, the loss term and the table.
//  * kploss_reduce_kernel: one workgroup, fixed tree: the scalar loss and
//    1 / (2 max(1, Nvalid)), which stays on the device for the backward.
//  * kploss_bwd_kernel: one workgroup per (image, tile of rows); every element
//    of gx [B, R, C] is written exactly once (no atomics, no pre-zeroing), the
//    A -> B terms and then the B -> A terms summed in keypoint order:
//      gx[r, m] = g / (2 Nvalid) * sum_n [ U_n(r) (softmax(s_n)[m] - V_n(m))
//                                          + (softmax(t_n)[r] - U_n(r)) V_n(m) ]
//    with s_n[m] / t_n[r] recomputed from x (four loads each).
#include "common.h"
#include "launchers.h"

namespace ncnet {

constexpr int KP_MAXN = 64;      // keypoints per image (the binding raises above it)
constexpr int KP_THREADS = 256;
constexpr int KP_ROWS = 5;       // rows per backward workgroup (625 = 125 x 5 at the training plane)
constexpr int KP_CHUNK = 640;    // columns of the row tile staged in LDS at a time (one chunk at C = 625)

// cells i0, i1 and the fraction f of 1-based pixel coordinate p on an n-cell
// axis of an image `size` pixels long: u = clamp((normalize_axis(p, size) + 1) / 2 (n - 1), 0, n - 1).
// In double (a handful of operations per workgroup), so the table does not
// depend on fp32 rounding of the mapping; fmax / fmin drop a NaN, so the
// cells are in range for any input.
__device__ __forceinline__ void kp_axis(float p, float size, int n, int& i0, int& i1, float& f) {
  const double pn = ((double)p - 1.0 - ((double)size - 1.0) / 2.0) * 2.0 / ((double)size - 1.0);
  double u = (pn + 1.0) / 2.0 * (double)(n - 1);
  u = fmin(fmax(u, 0.0), (double)(n - 1));
  i0 = min((int)floor(u), max(n - 2, 0));
  i1 = min(i0 + 1, n - 1);
  f = (float)(u - (double)i0);
}

struct KpTable { int a[4], b[4]; float u[4], v[4]; int valid; };

__device__ __forceinline__ void kp_cells(float px, float py, float h, float w, int gh, int gw, int* cell, float* wt) {
  int i0, i1, j0, j1;
  float fi, fj;
  kp_axis(py, h, gh, i0, i1, fi);
  kp_axis(px, w, gw, j0, j1, fj);
  cell[0] = i0 * gw + j0; wt[0] = (1.f - fi) * (1.f - fj);
  cell[1] = i0 * gw + j1; wt[1] = (1.f - fi) * fj;
  cell[2] = i1 * gw + j0; wt[2] = fi * (1.f - fj);
  cell[3] = i1 * gw + j1; wt[3] = fi * fj;
}

// running (max, sum exp(. - max)) of a softmax line
struct MS { float m, s; };
__device__ __forceinline__ MS ms_push(MS a, float x) {
  if (x > a.m) { a.s = a.s * __expf(a.m - x) + 1.f; a.m = x; }
  else a.s += __expf(x - a.m);
  return a;
}
__device__ __forceinline__ MS ms_merge(MS a, MS b) {
  MS r;
  r.m = fmaxf(a.m, b.m);
  r.s = (a.s == 0.f ? 0.f : a.s * __expf(a.m - r.m)) + (b.s == 0.f ? 0.f : b.s * __expf(b.m - r.m));
  return r;
}

// grid: B * N * 2 workgroups, block id = (b * N + n) * 2 + dir
// (dir 0: A -> B over the C columns, 1: B -> A over the R rows)
template <bool VEC>
__global__ __launch_bounds__(KP_THREADS) void kploss_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ sp, const float* __restrict__ tp,
    const float* __restrict__ ssz, const float* __restrict__ tsz, int B, int N, int hA, int wA, int hB, int wB,
    int* __restrict__ cells, float* __restrict__ wts, int* __restrict__ valid, float* __restrict__ lse,
    float* __restrict__ term) {
  __shared__ float wm[KP_THREADS / 64], wsum[KP_THREADS / 64];
  const int R = hA * wA, C = hB * wB;
  const int dir = blockIdx.x & 1;
  const int bn = blockIdx.x >> 1;
  const int b = bn / N, n = bn - b * N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  const float sx = sp[((size_t)b * 2 + 0) * N + n], sy = sp[((size_t)b * 2 + 1) * N + n];
  const float tx = tp[((size_t)b * 2 + 0) * N + n], ty = tp[((size_t)b * 2 + 1) * N + n];
  KpTable t;
  t.valid = (sx != -1.f && sy != -1.f && tx != -1.f && ty != -1.f) ? 1 : 0;
  kp_cells(sx, sy, ssz[b * 3 + 0], ssz[b * 3 + 1], hA, wA, t.a, t.u);
  kp_cells(tx, ty, tsz[b * 3 + 0], tsz[b * 3 + 1], hB, wB, t.b, t.v);
  if (!t.valid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { t.a[k] = 0; t.b[k] = 0; t.u[k] = 0.f; t.v[k] = 0.f; }
  }
  if (dir == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cells[(size_t)bn * 8 + k] = t.a[k]; cells[(size_t)bn * 8 + 4 + k] = t.b[k];
      wts[(size_t)bn * 8 + k] = t.u[k]; wts[(size_t)bn * 8 + 4 + k] = t.v[k];
    }
    valid[bn] = t.valid;
  }
  if (!t.valid) {                                      // workgroup-uniform
    if (threadIdx.x == 0) { lse[(size_t)bn * 2 + dir] = 0.f; term[(size_t)bn * 2 + dir] = 0.f; }
    return;
  }
  const float* xb = x + (size_t)b * R * C;
  MS st{-INFINITY, 0.f};
  if (dir == 0) {
    const float* r0 = xb + (size_t)t.a[0] * C;
    const float* r1 = xb + (size_t)t.a[1] * C;
    const float* r2 = xb + (size_t)t.a[2] * C;
    const float* r3 = xb + (size_t)t.a[3] * C;
    if constexpr (VEC) {                               // C % 4 == 0: every row base is 16-byte aligned
      for (int m = threadIdx.x * 4; m < C; m += KP_THREADS * 4) {
        if (!NCNET_OK(m + 3 < C)) break;
        const float4 q0 = *(const float4*)(r0 + m), q1 = *(const float4*)(r1 + m);
        const float4 q2 = *(const float4*)(r2 + m), q3 = *(const float4*)(r3 + m);
        st = ms_push(st, t.u[0] * q0.x + t.u[1] * q1.x + t.u[2] * q2.x + t.u[3] * q3.x);
        st = ms_push(st, t.u[0] * q0.y + t.u[1] * q1.y + t.u[2] * q2.y + t.u[3] * q3.y);
        st = ms_push(st, t.u[0] * q0.z + t.u[1] * q1.z + t.u[2] * q2.z + t.u[3] * q3.z);
        st = ms_push(st, t.u[0] * q0.w + t.u[1] * q1.w + t.u[2] * q2.w + t.u[3] * q3.w);
      }
    } else {                                           // the four rows differ in alignment: scalar loads
      for (int m = threadIdx.x; m < C; m += KP_THREADS)
        st = ms_push(st, t.u[0] * r0[m] + t.u[1] * r1[m] + t.u[2] * r2[m] + t.u[3] * r3[m]);
    }
  } else {
    for (int r = threadIdx.x; r < R; r += KP_THREADS) {
      const float* xr = xb + (size_t)r * C;
      st = ms_push(st, t.v[0] * xr[t.b[0]] + t.v[1] * xr[t.b[1]] + t.v[2] * xr[t.b[2]] + t.v[3] * xr[t.b[3]]);
    }
  }
  // fixed-order merge: xor tree inside the wave, then the waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MS ot;
    ot.m = __shfl_xor(st.m, o, 64);
    ot.s = __shfl_xor(st.s, o, 64);
    st = ms_merge(st, ot);
  }
  if (lane == 0) { wm[wave] = st.m; wsum[wave] = st.s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    MS a{wm[0], wsum[0]};
#pragma unroll
    for (int w = 1; w < KP_THREADS / 64; ++w) a = ms_merge(a, MS{wm[w], wsum[w]});
    const float l = a.m + __logf(a.s);
    float acc = 0.f;
    if (dir == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += t.u[j] * xb[(size_t)t.a[j] * C + t.b[k]];
        acc += t.v[k] * (s - l);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += t.v[j] * xb[(size_t)t.a[k] * C + t.b[j]];
        acc += t.u[k] * (s - l);
      }
    }
    lse[(size_t)bn * 2 + dir] = l;
    term[(size_t)bn * 2 + dir] = -acc;
  }
}

// out[0] = sum(term) / (2 max(1, Nvalid)), out[1] = 1 / (2 max(1, Nvalid)); one workgroup, fixed order
__global__ __launch_bounds__(KP_THREADS) void kploss_reduce_kernel(const float* __restrict__ term,
                                                                   const int* __restrict__ valid, int BN,
                                                                   float* __restrict__ out) {
  __shared__ float ps[KP_THREADS / 64];
  __shared__ int pc[KP_THREADS / 64];
  float acc = 0.f;
  int cnt = 0;
  for (int e = threadIdx.x; e < BN; e += KP_THREADS) {
    acc += term[(size_t)e * 2] + term[(size_t)e * 2 + 1];
    cnt += valid[e];
  }
  acc = wave_sum(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) { ps[threadIdx.x >> 6] = acc; pc[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    int c = 0;
#pragma unroll
    for (int w = 0; w < KP_THREADS / 64; ++w) { s += ps[w]; c += pc[w]; }
    const float scale = 1.f / (2.f * (float)max(c, 1));
    out[0] = s * scale;
    out[1] = scale;
  }
}

// grid: B * ceil(R / KP_ROWS) workgroups, KP_ROWS consecutive rows of one image each.
// Set-up, once per workgroup (one exposed round of global loads): the image's
// table; for every (row, keypoint) U_n(r) and q_n(r) = softmax(t_n)[r] - U_n(r)
// (four loads of x); per row the keypoints whose A cells hit it, collected in
// keypoint order by a wave ballot (most rows have none); and the chains of
// B-cell entries that share a column.  Then, per chunk of KP_CHUNK columns, the
// tile is staged in LDS: every thread evaluates the A -> B terms of the hit
// keypoints for its columns (zero elsewhere); the B -> A terms q_n v_k -- non-zero
// only in the keypoints' 4 N B cells -- are added by one thread per (row,
// distinct column), the entries of a column chained in keypoint order so that
// coinciding cells add up in a fixed order; and the tile (contiguous in gx) is
// written out scaled.
__global__ __launch_bounds__(KP_THREADS) void kploss_bwd_kernel(
    const float* __restrict__ x, const int* __restrict__ cells, const float* __restrict__ wts,
    const int* __restrict__ valid, const float* __restrict__ lse, const float* __restrict__ scale,
    const float* __restrict__ gscale, float* __restrict__ gx, int N, int R, int C, int ntile) {
  // the image's keypoints, in index order: A / B cells and weights, lse of s_n and of t_n
  __shared__ int s_a[KP_MAXN][4], s_b[KP_MAXN][4];
  __shared__ float s_u[KP_MAXN][4], s_v[KP_MAXN][4];
  __shared__ float s_ls[KP_MAXN], s_lt[KP_MAXN];
  __shared__ int s_valid[KP_MAXN];
  // B-cell entries e = 4 n + k: column (-1: invalid keypoint), whether e is the first
  // entry of its column, and the next entry of the same column (-1: none)
  __shared__ int e_col[4 * KP_MAXN], e_first[4 * KP_MAXN], e_next[4 * KP_MAXN];
  // per row of the tile: U_n(r), the entries' values q_n v_k, the hit list
  __shared__ float s_U[KP_ROWS][KP_MAXN], e_val[KP_ROWS][4 * KP_MAXN];
  __shared__ int s_hl[KP_ROWS][KP_MAXN], s_nh[KP_ROWS];
  __shared__ float acc[KP_ROWS][KP_CHUNK];
  const int b = blockIdx.x / ntile;
  const int r0 = (blockIdx.x - b * ntile) * KP_ROWS;
  const int nrows = min(KP_ROWS, R - r0);
  const int tid = threadIdx.x;
  const int NE = 4 * N;
  const float* xb = x + (size_t)b * R * C;
  if (tid < N) {
    const size_t bn = (size_t)b * N + tid;
    const int vld = valid[bn];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int a = cells[bn * 8 + k], bc = cells[bn * 8 + 4 + k];
      if (!NCNET_OK(a >= 0 && a < R)) a = 0;
      if (!NCNET_OK(bc >= 0 && bc < C)) bc = 0;
      s_a[tid][k] = a; s_b[tid][k] = bc;
      s_u[tid][k] = wts[bn * 8 + k]; s_v[tid][k] = wts[bn * 8 + 4 + k];
      e_col[4 * tid + k] = vld ? bc : -1;
    }
    s_ls[tid] = lse[bn * 2]; s_lt[tid] = lse[bn * 2 + 1]; s_valid[tid] = vld;
  }
  __syncthreads();
  for (int idx = tid; idx < nrows * N; idx += KP_THREADS) {
    const int row = idx / N, n = idx - row * N, r = r0 + row;
    float U = 0.f, q = 0.f;
    if (s_valid[n]) {
#pragma unroll
      for (int k = 0; k < 4; ++k) U += s_a[n][k] == r ? s_u[n][k] : 0.f;
      const float* xr = xb + (size_t)r * C;
      const float tr = s_v[n][0] * xr[s_b[n][0]] + s_v[n][1] * xr[s_b[n][1]] + s_v[n][2] * xr[s_b[n][2]] +
                       s_v[n][3] * xr[s_b[n][3]];
      q = __expf(tr - s_lt[n]) - U;
    }
    s_U[row][n] = U;
#pragma unroll
    for (int k = 0; k < 4; ++k) e_val[row][4 * n + k] = q * s_v[n][k];
  }
  if (tid < NE) {
    // one pass over all entries with no early exit, so the (broadcast) LDS reads pipeline
    const int col = e_col[tid];
    int first = col >= 0, next = 0x7fffffff;
#pragma unroll 8
    for (int e = 0; e < NE; ++e) {
      const bool same = e_col[e] == col;
      first &= !(same && e < tid);
      next = (same && e > tid) ? min(next, e) : next;
    }
    e_first[tid] = first; e_next[tid] = (col >= 0 && next < NE) ? next : -1;
  }
  if (tid >= KP_THREADS - 64) {                        // the last wave: one lane per keypoint (N <= 64)
    const int n = tid - (KP_THREADS - 64);
    for (int row = 0; row < nrows; ++row) {
      int hit = 0;
      if (n < N && s_valid[n]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) hit |= s_a[n][k] == r0 + row;
      }
      const unsigned long long mask = __ballot(hit);
      if (hit) s_hl[row][__popcll(mask & ((1ull << n) - 1ull))] = n;   // keypoint order
      if (n == 0) s_nh[row] = __popcll(mask);
    }
  }
  __syncthreads();
  const float gs = scale[0] * (gscale ? gscale[0] : 1.f);
  float* gt = gx + (size_t)b * R * C + (size_t)r0 * C;  // the tile: nrows contiguous rows
  for (int c0 = 0; c0 < C; c0 += KP_CHUNK) {
    const int cn = min(KP_CHUNK, C - c0);
    for (int row = 0; row < nrows; ++row) {
      const int nh = s_nh[row];                        // workgroup-uniform
      for (int i = tid; i < cn; i += KP_THREADS) {
        const int m = c0 + i;
        float g = 0.f;
        for (int h = 0; h < nh; ++h) {
          const int n = s_hl[row][h];
          float V = 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) V += s_b[n][k] == m ? s_v[n][k] : 0.f;
          const float s = s_u[n][0] * xb[(size_t)s_a[n][0] * C + m] + s_u[n][1] * xb[(size_t)s_a[n][1] * C + m] +
                          s_u[n][2] * xb[(size_t)s_a[n][2] * C + m] + s_u[n][3] * xb[(size_t)s_a[n][3] * C + m];
          g += s_U[row][n] * (__expf(s - s_ls[n]) - V);
        }
        acc[row][i] = g;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nrows * NE; idx += KP_THREADS) {
      const int row = idx / NE, e = idx - row * NE;
      if (!e_first[e]) continue;
      const int col = e_col[e];
      if (col < c0 || col >= c0 + cn) continue;
      float t = e_val[row][e];
      for (int f = e_next[e]; f >= 0; f = e_next[f]) t += e_val[row][f];
      acc[row][col - c0] += t;
    }
    __syncthreads();
    for (int row = 0; row < nrows; ++row)
      for (int i = tid; i < cn; i += KP_THREADS) gt[(size_t)row * C + c0 + i] = acc[row][i] * gs;
    if (c0 + KP_CHUNK < C) __syncthreads();            // acc is reused by the next chunk
  }
}

}  // namespace ncnet

using namespace ncnet;

// The launchers' contracts are in launchers.h.
extern "C" int ncnet_kploss_fwd(const float* x, const float* sp, const float* tp, const float* ssz, const float* tsz,
                                int B, int N, int hA, int wA, int hB, int wB, int* cells, float* wts, int* valid,
                                float* lse, float* term, float* out, hipStream_t s) {
  if (B < 1 || N < 1 || N > KP_MAXN || hA < 1 || wA < 1 || hB < 1 || wB < 1) return -3;
  if ((long long)B * N * 2 > 0x7fffffffLL) return -1;
  const int C = hB * wB;
  dispatch_bool(C % 4 == 0, [&](auto vc) {
    hipLaunchKernelGGL((kploss_fwd_kernel<decltype(vc)::value>), dim3((unsigned)(B * N * 2)), dim3(KP_THREADS), 0, s, x,
                       sp, tp, ssz, tsz, B, N, hA, wA, hB, wB, cells, wts, valid, lse, term);
  });
  hipLaunchKernelGGL(kploss_reduce_kernel, dim3(1), dim3(KP_THREADS), 0, s, term, valid, B * N, out);
  return (int)hipGetLastError();
}
extern "C" int ncnet_kploss_bwd(const float* x, const int* cells, const float* wts, const int* valid, const float* lse,
                                const float* scale, const float* gscale, float* gx, int B, int N, int R, int C,
                                hipStream_t s) {
  if (B < 1 || N < 1 || N > KP_MAXN || R < 1 || C < 1) return -3;
  if ((long long)B * R > 0x7fffffffLL) return -1;
  const int ntile = cdiv(R, KP_ROWS);
  hipLaunchKernelGGL(kploss_bwd_kernel, dim3((unsigned)(B * ntile)), dim3(KP_THREADS), 0, s, x, cells, wts, valid, lse,
                     scale, gscale, gx, N, R, C, ntile);
  return (int)hipGetLastError();
}
