// Batched P3P LO-RANSAC for the InLoc localization back end (the GPU form of
// ncnet_amd/eval/localization.py p3p / p3p_ransac, fp64 throughout).
//
// p3p: Grunert's quartic in v = s3 / s1 with the validity filters of the numpy
// solver (real root, den, s1sq > 0, u > 0, v > 0, degenerate triangle -> no
// solution).  The quartic is solved in closed form (depressed quartic split
// into two quadratics through the largest real root of the resolvent cubic)
// and every root is polished by a fixed number of Newton steps on the original
// coefficients.  The rigid transform comes from two orthonormal frames, one
// spanned by the world triangle and one by the camera-frame triangle; the
// numpy solver's Kabsch / SVD gives the same pose because the triangles are
// congruent.  No loop in this file has a data-dependent trip count except the
// passes over a problem's points, which are bounded by the point count.
//
// p3p_ransac_batch: one 256-lane workgroup per problem (a persistent loop when
// the grid is smaller than the batch).  A round = every lane draws one minimal
// sample (counter-based hash of (key, round, lane, draw): no state, so a
// problem's result depends only on its data and its key), solves it and scores
// its <= 4 poses against ALL points of the problem.  Points live in LDS as
// (unit ray, X) = 6 doubles; every lane reads the same point in the same
// cycle, a broadcast read without bank conflicts.  Problems of <= TILE points
// are staged once; larger ones are tiled through LDS on every pass.  A
// workgroup max-reduction over (count, lowest lane, lowest solution) picks the
// round's winner; a winner that beats the best so far is kept, the inlier mask
// and the compacted inlier list are rebuilt, lo_iters local-optimisation
// samples are drawn from that list, and the adaptive bound
// need = log(1 - confidence) / log(1 - w^3) is re-evaluated.  The number of
// rounds is bounded by ceil(max_iters / 256), fixed at launch.
#include "common.h"
#include "launchers.h"

namespace ncnet {
namespace pnp {

constexpr int WG = 256;        // lanes per problem
constexpr int TILE = 1024;     // points per LDS staging (48 KB of doubles)
constexpr int NEWTON = 3;      // polishing steps per quartic root

#define PNP_HD __host__ __device__ __forceinline__

struct Pose { double r[9]; double t[3]; };   // row-major R, X_cam = R X + t

PNP_HD double dot3(const double* a, const double* b) {
  return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2]));
}
PNP_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// largest real root of U^3 + b U^2 + c U + d
PNP_HD double cubic_largest_root(double b, double c, double d) {
  const double b3 = b * (1.0 / 3.0);
  const double P = c - b * b3;
  const double Q = 2.0 * b3 * b3 * b3 - b3 * c + d;
  const double D = 0.25 * Q * Q + P * P * P * (1.0 / 27.0);
  double w;
  if (D > 0.0) {
    double A = cbrt(0.5 * fabs(Q) + sqrt(D));
    A = Q > 0.0 ? -A : A;
    w = A != 0.0 ? A - P / (3.0 * A) : 0.0;
  } else {
    const double m = sqrt(fmax(-P * (1.0 / 3.0), 0.0));
    double arg = m > 0.0 ? -Q / (2.0 * m * m * m) : 0.0;
    arg = fmin(1.0, fmax(-1.0, arg));
    w = 2.0 * m * cos(acos(arg) * (1.0 / 3.0));
  }
  double U = w - b3;
#pragma unroll
  for (int it = 0; it < NEWTON; ++it) {
    const double f = fma(fma(U + b, U, c), U, d);
    const double fp = fma(fma(3.0, U, 2.0 * b), U, c);
    if (fabs(fp) > 1e-300) {
      const double Un = U - f / fp;
      // stay on the largest root: a step that moves left past a flat spot is dropped
      if (Un == Un && fabs(Un - U) <= 0.5 * (fabs(U) + fabs(b) + 1.0)) U = Un;
    }
  }
  return U;
}

// real roots of a4 v^4 + a3 v^3 + a2 v^2 + a1 v + a0 in 4 fixed slots (two per
// quadratic factor); bit s of the result marks slot s as a real root.  A
// complex pair whose imaginary part is below 1e-6 max(1, |re|) counts as a
// real double root, as the numpy solver's filter on np.roots does.
PNP_HD unsigned quartic_real_roots(double a4, double a3, double a2, double a1, double a0,
                                                       double* v) {
  const double ia = 1.0 / a4;
  const double b = a3 * ia, c = a2 * ia, d = a1 * ia, e = a0 * ia;
  const double b2 = b * b;
  const double p = c - 0.375 * b2;
  const double q = 0.125 * b2 * b - 0.5 * b * c + d;
  const double r = (-3.0 * b2 * b2 + 256.0 * e - 64.0 * b * d + 16.0 * b2 * c) * (1.0 / 256.0);
  // (y^2 + u y + vv)(y^2 - u y + tt) with U = u^2 a root of the resolvent cubic
  double U = cubic_largest_root(2.0 * p, p * p - 4.0 * r, -q * q);
  U = fmax(U, 0.0);
  const double u = sqrt(U);
  double qu;                                            // q / u, finite as u -> 0
  if (U > 1e-18 * fmax(1.0, fmax(p * p, fabs(r)))) qu = q / u;
  else qu = copysign(sqrt(fmax(0.0, fma(U, U, fma(2.0 * p, U, p * p - 4.0 * r)))), q);
  const double tt = 0.5 * (p + U + qu), vv = 0.5 * (p + U - qu);
  const double shift = -0.25 * b;
  unsigned valid = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double lin = h == 0 ? u : -u, cst = h == 0 ? vv : tt;      // y^2 + lin y + cst
    double disc = lin * lin - 4.0 * cst;
    const double re = -0.5 * lin + shift;
    const bool real = disc >= -4e-12 * fmax(1.0, re * re);
    disc = fmax(disc, 0.0);
    const double sq = sqrt(disc);
    const double y0 = -0.5 * (lin + (lin >= 0.0 ? sq : -sq));
    const double y1 = y0 != 0.0 ? cst / y0 : 0.5 * (-lin + (lin >= 0.0 ? sq : -sq));
    v[2 * h] = y0 + shift;
    v[2 * h + 1] = y1 + shift;
    if (real) valid |= 3u << (2 * h);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    double x = v[s];
#pragma unroll
    for (int it = 0; it < NEWTON; ++it) {
      const double f = fma(fma(fma(fma(a4, x, a3), x, a2), x, a1), x, a0);
      const double fp = fma(fma(fma(4.0 * a4, x, 3.0 * a3), x, 2.0 * a2), x, a1);
      const double xn = x - f / fp;
      if (fabs(fp) > 1e-300 && xn == xn && fabs(xn - x) <= 1e-3 * (fabs(x) + 1.0)) x = xn;
    }
    // a slot that is no root of the quartic (a failed factorisation) is dropped
    const double x2 = x * x;
    const double f = fma(fma(fma(fma(a4, x, a3), x, a2), x, a1), x, a0);
    const double scale = fabs(a4) * x2 * x2 + fabs(a3 * x) * x2 + fabs(a2) * x2 + fabs(a1 * x) + fabs(a0);
    if (!(fabs(f) <= 1e-9 * scale)) valid &= ~(1u << s);
    v[s] = x;
  }
  return valid;
}

// f: 3 unit bearing vectors, X: 3 world points (row k = point k).  Fills up to 4
// poses in fixed slots and returns the mask of the valid slots.
PNP_HD unsigned p3p(const double f[3][3], const double X[3][3], Pose* out) {
  double e12[3], e13[3], e23[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e12[k] = X[1][k] - X[0][k];
    e13[k] = X[2][k] - X[0][k];
    e23[k] = X[2][k] - X[1][k];
  }
  const double a2 = dot3(e23, e23), b2 = dot3(e13, e13), c2 = dot3(e12, e12);
  if (!(fmin(a2, fmin(b2, c2)) >= 1e-12)) return 0;
  // world frame; a collinear triangle spans none
  double w1[3], w2[3], w3[3];
  const double il = 1.0 / sqrt(c2);
#pragma unroll
  for (int k = 0; k < 3; ++k) w1[k] = e12[k] * il;
  cross3(w1, e13, w3);
  const double n3 = dot3(w3, w3);
  if (!(n3 > 1e-18 * b2)) return 0;
  const double i3 = 1.0 / sqrt(n3);
#pragma unroll
  for (int k = 0; k < 3; ++k) w3[k] *= i3;
  cross3(w3, w1, w2);

  const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
  const double ib2 = 1.0 / b2;
  const double p = (a2 - c2) * ib2, q = (a2 + c2) * ib2;
  const double ca2 = ca * ca, cg2 = cg * cg;
  const double A4 = (p - 1.0) * (p - 1.0) - 4.0 * c2 * ib2 * ca2;
  const double A3 = 4.0 * (p * (1.0 - p) * cb - (1.0 - q) * ca * cg + 2.0 * c2 * ib2 * ca2 * cb);
  const double A2 = 2.0 * (p * p - 1.0 + 2.0 * p * p * cb * cb + 2.0 * (b2 - c2) * ib2 * ca2 - 4.0 * q * ca * cb * cg +
                           2.0 * (b2 - a2) * ib2 * cg2);
  const double A1 = 4.0 * (-p * (1.0 + p) * cb + 2.0 * a2 * ib2 * cg2 * cb - (1.0 - q) * ca * cg);
  const double A0 = (1.0 + p) * (1.0 + p) - 4.0 * a2 * ib2 * cg2;
  double v[4];
  unsigned valid = quartic_real_roots(A4, A3, A2, A1, A0, v);

  double xm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) xm[k] = (X[0][k] + X[1][k] + X[2][k]) * (1.0 / 3.0);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double vs = v[s];
    const double den = 2.0 * (cg - vs * ca);
    const double u = ((p - 1.0) * vs * vs - 2.0 * p * cb * vs + 1.0 + p) / den;
    const double s1sq = b2 / (1.0 + vs * vs - 2.0 * vs * cb);
    const bool good = fabs(den) >= 1e-12 && s1sq > 0.0 && u > 0.0 && vs > 0.0;
    const double s1 = sqrt(fmax(s1sq, 0.0));
    double d[3] = {s1, u * s1, vs * s1};
    // polish the three depths on the law-of-cosines system itself (u above divides by
    // den, which loses digits when den is small): Newton steps with the 3 x 3 adjugate
#pragma unroll
    for (int it = 0; it < NEWTON; ++it) {
      const double F0 = d[1] * d[1] + d[2] * d[2] - 2.0 * d[1] * d[2] * ca - a2;
      const double F1 = d[0] * d[0] + d[2] * d[2] - 2.0 * d[0] * d[2] * cb - b2;
      const double F2 = d[0] * d[0] + d[1] * d[1] - 2.0 * d[0] * d[1] * cg - c2;
      const double j01 = 2.0 * (d[1] - d[2] * ca), j02 = 2.0 * (d[2] - d[1] * ca);
      const double j10 = 2.0 * (d[0] - d[2] * cb), j12 = 2.0 * (d[2] - d[0] * cb);
      const double j20 = 2.0 * (d[0] - d[1] * cg), j21 = 2.0 * (d[1] - d[0] * cg);
      // J = [[0, j01, j02], [j10, 0, j12], [j20, j21, 0]]
      const double det = j01 * j12 * j20 + j02 * j10 * j21;
      const double id = 1.0 / det;
      const double e0 = (-j12 * j21 * F0 + j02 * j21 * F1 + j01 * j12 * F2) * id;
      const double e1 = (j12 * j20 * F0 - j02 * j20 * F1 + j02 * j10 * F2) * id;
      const double e2 = (j10 * j21 * F0 + j01 * j20 * F1 - j01 * j10 * F2) * id;
      const double lim = 1e-2 * (d[0] + d[1] + d[2]);
      if (fabs(e0) <= lim && fabs(e1) <= lim && fabs(e2) <= lim) {      // false for NaN / inf steps
        d[0] -= e0;
        d[1] -= e1;
        d[2] -= e2;
      }
    }
    double Y[3][3], ym[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) Y[j][k] = f[j][k] * d[j];
    double g12[3], g13[3], c1[3], c2v[3], c3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g12[k] = Y[1][k] - Y[0][k];
      g13[k] = Y[2][k] - Y[0][k];
      ym[k] = (Y[0][k] + Y[1][k] + Y[2][k]) * (1.0 / 3.0);
    }
    const double i1 = 1.0 / sqrt(dot3(g12, g12));
#pragma unroll
    for (int k = 0; k < 3; ++k) c1[k] = g12[k] * i1;
    cross3(c1, g13, c3);
    const double i3c = 1.0 / sqrt(dot3(c3, c3));
#pragma unroll
    for (int k = 0; k < 3; ++k) c3[k] *= i3c;
    cross3(c3, c1, c2v);
    Pose& P = out[s];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        P.r[3 * i + j] = fma(c1[i], w1[j], fma(c2v[i], w2[j], c3[i] * w3[j]));
        finite = finite && (P.r[3 * i + j] - P.r[3 * i + j] == 0.0);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      P.t[i] = ym[i] - dot3(&P.r[3 * i], xm);
      finite = finite && (P.t[i] - P.t[i] == 0.0);
    }
    if (!(good && finite && d[0] > 0.0 && d[1] > 0.0 && d[2] > 0.0)) valid &= ~(1u << s);
  }
  return valid;
}

// the inlier test of angular_errors(): angle(f, R X + t) < thr with the point in
// front of the camera, as f . Y > cos(thr) |Y| without the arccos (0 < thr < pi/2;
// ct2 = cos(thr)^2).  Written with explicit fma so that every call site rounds alike.
__device__ __forceinline__ bool is_inlier(const Pose& P, const double* pt, double ct2) {
  const double x0 = pt[3], x1 = pt[4], x2 = pt[5];
  const double y0 = fma(P.r[0], x0, fma(P.r[1], x1, fma(P.r[2], x2, P.t[0])));
  const double y1 = fma(P.r[3], x0, fma(P.r[4], x1, fma(P.r[5], x2, P.t[1])));
  const double y2 = fma(P.r[6], x0, fma(P.r[7], x1, fma(P.r[8], x2, P.t[2])));
  const double d = fma(pt[0], y0, fma(pt[1], y1, pt[2] * y2));
  const double m = fma(y0, y0, fma(y1, y1, y2 * y2));
  return y2 > 0.0 && d > 0.0 && d * d > ct2 * m;
}

// (unit ray, X) of global point i
__device__ __forceinline__ void load_point(const double* __restrict__ rays, const double* __restrict__ X, long long i,
                                           double* pt) {
  const double a = rays[3 * i], b = rays[3 * i + 1], c = rays[3 * i + 2];
  const double inv = 1.0 / sqrt(fma(a, a, fma(b, b, c * c)));
  pt[0] = a * inv;
  pt[1] = b * inv;
  pt[2] = c * inv;
  pt[3] = X[3 * i];
  pt[4] = X[3 * i + 1];
  pt[5] = X[3 * i + 2];
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
// counter-based draw: uniform 32 bits from (key, stream, round, lane, draw)
__device__ __forceinline__ uint32_t draw32(uint64_t key, uint32_t stream, uint32_t round, uint32_t lane, uint32_t k) {
  const uint64_t ctr = ((uint64_t)round << 32) | ((uint64_t)stream << 24) | ((uint64_t)lane << 8) | k;
  return (uint32_t)(mix64(mix64(key + 0x9E3779B97F4A7C15ull) ^ (ctr * 0xD6E8FEB86659FD93ull + 0x9E3779B97F4A7C15ull)) >> 32);
}
// 3 distinct indices in [0, n), n >= 3, without rejection: the k-th index is drawn
// from the n - k values left and shifted past the earlier ones
__device__ __forceinline__ void sample3(uint64_t key, uint32_t stream, uint32_t round, uint32_t lane, int n, int* idx) {
  int i0 = (int)(((uint64_t)draw32(key, stream, round, lane, 0) * (uint64_t)n) >> 32);
  int i1 = (int)(((uint64_t)draw32(key, stream, round, lane, 1) * (uint64_t)(n - 1)) >> 32);
  int i2 = (int)(((uint64_t)draw32(key, stream, round, lane, 2) * (uint64_t)(n - 2)) >> 32);
  if (i1 >= i0) ++i1;
  const int lo = min(i0, i1), hi = max(i0, i1);
  if (i2 >= lo) ++i2;
  if (i2 >= hi) ++i2;
  idx[0] = i0; idx[1] = i1; idx[2] = i2;
}

struct Shared {
  double pts[TILE * 6];
  Pose best;
  Pose cand;
  unsigned long long red[WG / 64];
  int wtot[WG / 64];
};

// stage points [t0, t0 + cnt) of the problem at off0 into LDS
__device__ __forceinline__ void stage(Shared& sh, const double* __restrict__ rays, const double* __restrict__ X,
                                      long long off0, int t0, int cnt) {
  for (int i = threadIdx.x; i < cnt; i += WG) load_point(rays, X, off0 + t0 + i, &sh.pts[6 * i]);
}

// Every lane scores its 4 pose slots against all n points; cnt[s] = inliers of slot s.
// All WG lanes call this (it holds barriers when the points are tiled).
__device__ __forceinline__ void score4(Shared& sh, const double* __restrict__ rays, const double* __restrict__ X,
                                       long long off0, int n, bool resident, const Pose* P, double ct2, int* cnt) {
  cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
  for (int t0 = 0; t0 < n; t0 += TILE) {
    const int m = min(TILE, n - t0);
    if (!resident) {
      __syncthreads();
      stage(sh, rays, X, off0, t0, m);
      __syncthreads();
    }
#pragma unroll 2
    for (int i = 0; i < m; ++i) {
      const double* pt = &sh.pts[6 * i];
#pragma unroll
      for (int s = 0; s < 4; ++s) cnt[s] += is_inlier(P[s], pt, ct2) ? 1 : 0;
    }
  }
}

// mask + ordered inlier list of sh.best; returns the inlier count (all lanes)
__device__ __forceinline__ int compact(Shared& sh, const double* __restrict__ rays, const double* __restrict__ X,
                                       long long off0, int n, bool resident, double ct2, uint8_t* __restrict__ mask,
                                       int* __restrict__ list) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  __syncthreads();                                      // sh.best is written
  const Pose P = sh.best;
  for (int t0 = 0; t0 < n; t0 += TILE) {
    const int m = min(TILE, n - t0);
    if (!resident) {
      __syncthreads();
      stage(sh, rays, X, off0, t0, m);
      __syncthreads();
    }
    for (int c0 = 0; c0 < m; c0 += WG) {
      const int i = c0 + (int)threadIdx.x;
      const bool in = i < m && is_inlier(P, &sh.pts[6 * i], ct2);
      const unsigned long long bal = __ballot(in);
      if (lane == 0) sh.wtot[wave] = __popcll(bal);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < WG / 64; ++w) {
        before += w < wave ? sh.wtot[w] : 0;
        total += sh.wtot[w];
      }
      if (i < m) {
        mask[off0 + t0 + i] = in ? 1 : 0;
        if (in) list[off0 + base + before + __popcll(bal & ((1ull << lane) - 1ull))] = t0 + i;
      }
      base += total;
      __syncthreads();
    }
  }
  return base;
}

// workgroup winner of a round: most inliers, ties to the lowest (lane, slot).
// Returns the packed key of the winner (count << 32 | ~(lane * 4 + slot)) to all lanes.
__device__ __forceinline__ unsigned long long reduce_best(Shared& sh, const int* cnt, unsigned valid) {
  unsigned long long k = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (valid & (1u << s)) {
      const unsigned long long ks = ((unsigned long long)(unsigned)cnt[s] << 32) | (0xFFFFFFFFu - (threadIdx.x * 4 + s));
      k = ks > k ? ks : k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o, 64);
    k = other > k ? other : k;
  }
  __syncthreads();                                      // sh.red of the previous reduction is read
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = k;
  __syncthreads();
  unsigned long long r = 0;
#pragma unroll
  for (int w = 0; w < WG / 64; ++w) r = sh.red[w] > r ? sh.red[w] : r;
  return r;
}

// one batch of hypotheses: lane draws a sample (from all points, or from the
// inlier list when lo), solves, scores, and the workgroup winner lands in
// sh.cand.  Returns the winner's inlier count to all lanes (0: no valid pose).
__device__ __forceinline__ int hypotheses(Shared& sh, const double* __restrict__ rays, const double* __restrict__ X,
                                          const int* list, long long off0, int n, int pool, bool lo,
                                          bool active, uint64_t key, uint32_t round, uint32_t lane_id, bool resident,
                                          double ct2) {
  Pose P[4];
  unsigned valid = 0;
  if (active) {
    int idx[3];
    sample3(key, lo ? 1u : 0u, round, lane_id, pool, idx);
    double f[3][3], Xs[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      int i = idx[j];
      if (lo) i = list[off0 + i];
      if (!NCNET_OK(i >= 0 && i < n)) i = 0;
      double pt[6];
      load_point(rays, X, off0 + i, pt);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        f[j][k] = pt[k];
        Xs[j][k] = pt[3 + k];
      }
    }
    valid = p3p(f, Xs, P);
  }
  if (!valid) {
    // idle lanes score a zero pose (depth 0: never an inlier) in step with the others
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int k = 0; k < 9; ++k) P[s].r[k] = 0.0;
      P[s].t[0] = P[s].t[1] = P[s].t[2] = 0.0;
    }
  }
  int cnt[4];
  score4(sh, rays, X, off0, n, resident, P, ct2, cnt);
  const unsigned long long win = reduce_best(sh, cnt, valid);
  if (win == 0) return 0;
  const unsigned who = 0xFFFFFFFFu - (unsigned)(win & 0xFFFFFFFFull);
  if (threadIdx.x == (who >> 2)) {
    const unsigned s = who & 3u;
    Pose w = P[0];
    if (s == 1) w = P[1];
    if (s == 2) w = P[2];
    if (s == 3) w = P[3];
    sh.cand = w;
  }
  return (int)(win >> 32);
}

__global__ __launch_bounds__(WG) void p3p_ransac_kernel(const double* __restrict__ rays, const double* __restrict__ X,
                                                         const int* __restrict__ offsets,
                                                         const long long* __restrict__ keys, int B, long long N,
                                                         double ct2, int max_iters, int max_rounds, double log1mc,
                                                         int lo_iters, int lo_rounds, double* __restrict__ Pout,
                                                         int* __restrict__ ninl, uint8_t* __restrict__ mask,
                                                         int* __restrict__ list, int* __restrict__ rounds_out) {
  __shared__ Shared sh;
  const double qnan = __builtin_nan("");
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const long long off0 = offsets[b];
    long long nn = (long long)offsets[b + 1] - off0;
    if (!NCNET_OK(off0 >= 0 && nn >= 0 && off0 + nn <= N)) nn = 0;
    const int n = (int)nn;
    const uint64_t key = (uint64_t)keys[b];
    const bool resident = n <= TILE;
    __syncthreads();                                    // the previous problem is done with sh
    if (threadIdx.x < 12) ((double*)&sh.best)[threadIdx.x] = qnan;
    if (resident) stage(sh, rays, X, off0, 0, n);
    __syncthreads();
    int best = 0, round = 0;
    long long need = max_iters;
    if (n >= 3) {
      for (round = 0; round < max_rounds; ++round) {
        if ((long long)round * WG >= need) break;        // need <= max_iters; the same in every lane
        const bool active = (long long)round * WG + threadIdx.x < max_iters;
        int c = hypotheses(sh, rays, X, list, off0, n, n, false, active, key, (uint32_t)round, threadIdx.x, resident, ct2);
        if (c > best) {                                  // c is workgroup-uniform
          __syncthreads();
          if (threadIdx.x < 12) ((double*)&sh.best)[threadIdx.x] = ((double*)&sh.cand)[threadIdx.x];
          best = compact(sh, rays, X, off0, n, resident, ct2, mask, list);
          // local optimisation: lo_iters minimal samples from the inliers, kept when they add inliers
          for (int lr = 0; lr < lo_rounds; ++lr) {
            if (best < 4) break;
            const bool la = lr * WG + (int)threadIdx.x < lo_iters;
            c = hypotheses(sh, rays, X, list, off0, n, best, true, la, key, (uint32_t)round,
                           (uint32_t)(lr * WG) + threadIdx.x, resident, ct2);
            if (c > best) {
              __syncthreads();
              if (threadIdx.x < 12) ((double*)&sh.best)[threadIdx.x] = ((double*)&sh.cand)[threadIdx.x];
              best = compact(sh, rays, X, off0, n, resident, ct2, mask, list);
            }
          }
          const double w = (double)best / (double)n;
          const double lg = log(fmax(1e-12, 1.0 - w * w * w));
          const double nd = lg < 0.0 ? ceil(log1mc / lg) : (double)max_iters;      // w^3 below 1 ulp: no bound
          need = nd < (double)max_iters ? (long long)nd : (long long)max_iters;   // NaN / inf -> max_iters
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 12) {                            // [R | t] row-major 3 x 4 from Pose's r[9], t[3]
      const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
      Pout[(size_t)b * 12 + threadIdx.x] = j < 3 ? sh.best.r[3 * i + j] : sh.best.t[i];
    }
    if (threadIdx.x == 0) {
      ninl[b] = best;
      if (rounds_out) rounds_out[b] = round;
    }
  }
}

// test entry point of the minimal solver: one lane per triplet
__global__ __launch_bounds__(64) void p3p_solve_kernel(const double* __restrict__ rays, const double* __restrict__ X,
                                                        int M, double* __restrict__ Pout, int* __restrict__ nsol) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M) return;
  double f[3][3], Xs[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double pt[6];
    load_point(rays, X, (long long)m * 3 + j, pt);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      f[j][k] = pt[k];
      Xs[j][k] = pt[3 + k];
    }
  }
  Pose P[4];
  const unsigned valid = p3p(f, Xs, P);
  const double qnan = __builtin_nan("");
  double* o = Pout + (size_t)m * 48;
  int k = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (valid & (1u << s)) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o[k * 12 + 4 * i + j] = P[s].r[3 * i + j];
        o[k * 12 + 4 * i + 3] = P[s].t[i];
      }
      ++k;
    }
  }
  for (int e = k * 12; e < 48; ++e) o[e] = qnan;
  nsol[m] = k;
}

}  // namespace pnp
}  // namespace ncnet

using namespace ncnet::pnp;

extern "C" int ncnet_p3p_solve(const double* rays, const double* X, int M, double* P, int* nsol, hipStream_t stream) {
  if (M <= 0) return 0;
  hipLaunchKernelGGL(p3p_solve_kernel, dim3((unsigned)cdiv(M, 64)), dim3(64), 0, stream, rays, X, M, P, nsol);
  return (int)hipGetLastError();
}

extern "C" int ncnet_p3p_ransac_batch(const double* rays, const double* X, const int* offsets, const long long* keys,
                                      int B, long long N, double cos_thr, int max_iters, double confidence,
                                      int lo_iters, double* P, int* ninl, uint8_t* mask, int* list, int* rounds,
                                      hipStream_t stream) {
  if (B <= 0) return 0;
  const int max_rounds = cdiv(max_iters, WG), lo_rounds = cdiv(lo_iters, WG);
  const double log1mc = log(1.0 - confidence);          // -inf at confidence 1: never stops early
  const int grid = B < 16 * device_num_cus() ? B : 16 * device_num_cus();
  hipLaunchKernelGGL(p3p_ransac_kernel, dim3((unsigned)grid), dim3(WG), 0, stream, rays, X, offsets, keys, B, N,
                     cos_thr * cos_thr, max_iters, max_rounds, log1mc, lo_iters, lo_rounds, P, ninl, mask, list, rounds);
  return (int)hipGetLastError();
}
