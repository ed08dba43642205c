// The one declaration of every extern "C" ncnet_* kernel launcher.
//
// Each csrc/*.hip file that defines a launcher includes this header, so a
// definition whose parameter list drifts from the declaration fails to compile
// ("conflicting types"); bindings.cpp includes it to call them.  It compiles
// under hipcc and under the plain host compiler: raw pointers and scalars only,
// no device types.
//
// Return code of every launcher (unless its comment says otherwise):
//    0   launched (or nothing to do), else the HIP error code of the launch;
//   -1   no kernel instantiation or launch geometry for this shape;
//   -2   unsupported kernel size;
//   -3   bad argument.
// (ncnet_ijpack / ncnet_ijsum report an unsupported kernel size as -1;
// ncnet_nc_fused_k3* use -2 bad tiling, -3 LDS over budget, -4 plane too large
// for 32-bit byte offsets; ncnet_gemm_lt returns other negative codes for
// hipBLASLt failures.)
//
// Volumes are channels-last [V,I,J,K,L,16] bf16 unless stated; "elements" are
// counts of the tensor's dtype.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

extern "C" {

// ---- launcher tuning (csrc/conv4d_fwd.hip) --------------------------------
// Tuning switch `name` (common.h NcnetTuning): returns its previous value and,
// when set != 0, stores `value`.  INT32_MIN for an unknown name.
int ncnet_set_tuning(const char* name, int value, int set);

// ---- Conv4d 16 -> 16 forward (csrc/conv4d_fwd.hip) ------------------------
// X [V,I,J,K,L,16] (all KS*KS planes (i+di-P, j+dj-P)), or npg > 0: group-planes
// mode -- X holds npg input groups [npg][V,I,J,K,L,16] and
// Y = sum_s conv_(dk,dl)(X[s] plane (i,j), Wp plane s): the (di, dj) offsets
// live in the channels (ij encoding, csrc/jshift.hip) or s indexes 16-channel
// input blocks of a wider layer.  Wp [planes][nq = ceil(KS*KS / 2)][64][8].
// epi: 0 none -> bf16, 1 bias + ReLU -> bf16, 2 ReLU mask M -> bf16,
//      4 fp32 channel-planar [nco,V,I,J,K,L] (first nco <= 16 output channels).
// epi | 64 (KS 3 / 5, epi 1 or 2): the bf16x3 layer, X_lo = X + xlo,
// Wp = [hi planes; lo planes], split output Y / Y + ylo (elements).
int ncnet_conv16_fwd(const void* X, const void* Wp, const float* bias, const void* M, void* Y, int V, int I, int J,
                     int K, int L, int KS, int epi, int npg, int nco, long long xlo, long long ylo,
                     hipStream_t stream);

// Cout = 1 layer (16 input channels) in output-plane-block mode: Y fp32
// [V,I,J,K,L] = act(bias + conv(X, W)); Wp [(KS+3)^2 relative planes][nq][64][8]
// (ops/packing.py blk_out_weights).  x3 != 0 (KS 3 / 5): the bf16x3 layer,
// X_lo = X + xlo (elements), Wp = [hi; lo] planes.
int ncnet_conv16_blk_fwd(const void* X, const void* Wp, const float* bias, float* Y, int V, int I, int J, int K, int L,
                         int KS, int relu, int x3, long long xlo, hipStream_t stream);

// fp8 (OCP e4m3) inference Conv4d 16 -> 16: X / Wp fp8 (weights * wscale), oscale = 1 / wscale;
// epi 1 (Y fp8 = relu(oscale * acc + bias)) or 4 (Y fp32 planar [nco,V,I,J,K,L]), else -2.
int ncnet_conv16f8_fwd(const void* X, const void* Wp, const float* bias, void* Y, int V, int I, int J, int K, int L,
                       int KS, int epi, int npg, int nco, float oscale, hipStream_t stream);

// ---- Conv4d weight gradients (csrc/conv4d_wgrad.hip) ----------------------
// wgrad16v2.  part: [2 * ngroups][KS*KS (dj_center 0) or 1 (dj_center 2: plane-only)][KS*KS][16 ci][16 co]
// fp32 (one row per voxel-chunk half); partb: [2 * ngroups][16].
int ncnet_wgrad16(const void* X, const void* G, float* part, float* partb, int V, int I, int J, int K, int L, int KS,
                  int ngroups, int dj_center, hipStream_t stream);

// wgrad16p (plane-only, whole-plane tiles: K, L <= 25): X [nsets][V,I,J,K,L,16]
// (set stride xstride elements), G [ngg][...] (stride gstride), ngg 1 or 2;
// part [2 * ngroups][nsets * ngg][KS*KS][16][16], partb [2 * ngroups][nsets * ngg][16].
int ncnet_wgrad16p(const void* X, const void* G, float* part, float* partb, int V, int I, int J, int K, int L, int KS,
                   int ngroups, int nsets, int ngg, long long xstride, long long gstride, hipStream_t stream);

// wgrad16v3 / v4 (sliding G ring, all (di, dj), KS 3 / 5): ngroups column groups
// per dj; part / partb as ncnet_wgrad16 with dj_center 0.
int ncnet_wgrad16v3(const void* X, const void* G, float* part, float* partb, int V, int I, int J, int K, int L, int KS,
                    int ngroups, hipStream_t stream);

// ---- ij encoding (csrc/jshift.hip) ----------------------------------------
// X [V,I,J,K,L] (bf16 / fp32) -> S [ceil(KS*KS / 16)][V,I,J,K,L,16] bf16, or OCP fp8 e4m3 (s_fp8); sgn +1 / -1.
int ncnet_ijpack(const void* X, int x_is_bf16, void* S, int V, int I, int J, int K, int L, int KS, int sgn, int s_fp8,
                 hipStream_t stream);
// Z [KS*KS,V,I,J,K,L] fp32 (channel-planar by combo q = di*KS + dj) -> y [V,I,J,K,L] fp32; bias [1] or null.
int ncnet_ijsum(const float* Z, const float* bias, float* y, int V, int I, int J, int K, int L, int KS, int relu,
                int sgn, hipStream_t stream);

// ---- 1-channel Conv4d on padded planes (csrc/conv1x.hip) ------------------
// padded-plane geometry of a (K, L) plane for kernel size KS: *lp = row length, *ppl = elements per plane
int ncnet_pad_geom(int K, int L, int KS, int* lp, int* ppl);
// x: [V, R, C] fp32 or bf16 (x_is_bf16); planes of x (trans 0: N = V*R planes of
// [I2, J2]) or of its A<->B swap (trans 1: N = V*C planes) into y [N, PPL] bf16,
// whose halo the caller zeroed.
int ncnet_pad_planes(const void* x, int x_is_bf16, void* y, int V, int R, int C, int I2, int J2, int KS, int trans,
                     hipStream_t s);
// 1 -> 16 layer: Xp padded planes [V*I*J][PPL], Wa A fragments [KS*KS][64][8], Y [V,I,J,K,L,16];
// epi 1 (bias + ReLU) or 2 (ReLU mask M), else -3.  epi | 4: the bf16x3 layer
// (X_lo = Xp + xlo, Wa = [hi; lo] fragment sets, Y_lo = Y + ylo, elements).
int ncnet_conv1x16(const void* Xp, const void* Wa, const float* bias, const void* M, void* Y, int V, int I, int J,
                   int K, int L, int KS, int epi, int nt_store, long long xlo, long long ylo, hipStream_t s);
// D bf16 [V,I,J,K,L,16], X1 padded planes [V*I*J][PPL]; part fp32
// [G][KS*KS taps][32 combos][16] (one partial per workgroup, G <= the CU count; G < 1: -2),
// partb fp32 [G][16] (sum of D; null: none).
int ncnet_wgrad1x16(const void* Dp, const void* X1p, float* part, float* partb, int G, int V, int I, int J, int K,
                    int L, int KS, hipStream_t s);

// ---- Cout = 1 layer, taps as MFMA rows (csrc/cout1.hip) -------------------
// Y fp32 [V,I,J,K,L] = act(bias + conv(X, W)) for a 16 -> 1 layer; Wt: the tap-row
// A fragments [KS*KS][64][8] (ops/packing.py cout1_taps_weights).  -1: the
// caller keeps the output-plane-block kernel.
int ncnet_cout1_taps_fwd(const void* X, const void* Wt, const float* bias, float* Y, int V, int I, int J, int K, int L,
                         int KS, int relu, hipStream_t s);

// ---- fused NC stack 1 -> 16 -> 1, k = 3 (csrc/nc_fused.hip) ---------------
// X bf16 [V,I,J,K,L]; W1p / W2p bf16 [5][64][8] (pack_w16_planes of the ij layer weights);
// b1 fp32 [16], b2 fp32 [1]; Y fp32 [V,I,J,K,L]; tile (TK, TL), R planes and IR rows per workgroup.
// f16: X / W1p / W2p are IEEE half (f16 MFMA, f16 hidden activation).
int ncnet_nc_fused_k3(const void* X, const void* W1p, const float* b1, const void* W2p, const float* b2, float* Y,
                      int V, int I, int J, int K, int L, int R, int IR, int TK, int TL, int f16, hipStream_t stream);
// fp8 fused stack: X bf16; W1a / W2a [64] x 32 B MX fragments of taps 0..7,
// W1b / W2b [64] x 8 B fragments of tap 8 (e4m3, weights * sw).  Scales: sx (X),
// inv1 = 1 / (sw1 sx), sh (hidden), inv2 = 1 / (sw2 sh).
int ncnet_nc_fused_k3_f8(const void* X, const void* W1a, const void* W1b, const float* b1, const void* W2a,
                         const void* W2b, const float* b2, float* Y, int V, int I, int J, int K, int L, int R, int IR,
                         int TK, int TL, float sx, float inv1, float sh, float inv2, hipStream_t stream);

// ---- feature trunk (csrc/conv2d.hip, csrc/gemm_lt.hip, csrc/epilogue.hip) -
// NHWC implicit-GEMM conv with fused bias (+ residual R) (+ ReLU): X [N,H,Wd,Cin],
// W [Cout,KH,KW,Cin], R / Y [N,Ho,Wo,Cout] bf16 (f16: IEEE half); Cin, Cout % 64 == 0.
int ncnet_conv2d_nhwc(const void* X, const void* W, const float* bias, const void* R, void* Y, int N, int H, int Wd,
                      int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, int f16, hipStream_t stream);
// bf16x3 (fp32-accurate) conv: X [N,H,W,2 Cin] = [hi | lo] bf16 pairs, W [Cout][KH][KW][3 Cin]
// = [W_hi | W_hi | W_lo], R / Y [.., 2 Cout] pairs, bias fp32.
int ncnet_conv2d_nhwc_x3(const void* X, const void* W, const float* bias, const void* R, void* Y, int N, int H, int Wd,
                         int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, hipStream_t stream);
// Y [m, cout] = act(X [m, cin] W^T + bias + R) through hipBLASLt.  tune != 0: time
// every heuristic candidate once for this shape (not while the stream is
// being captured) and keep the fastest.
int ncnet_gemm_lt(const void* X, const void* W, const float* bias, const void* R, void* Y, int m, int cin, int cout,
                  int relu, int f16, int tune, hipStream_t st);
// In place Y = act(Y + b): Y [rows, C] 16-bit (f16: IEEE half, else bf16), b fp32 [C], C % 8 == 0.
int ncnet_bias_act(void* Y, const float* b, long long rows, int C, int relu, int f16, hipStream_t stream);
// Y = act(maxpool(X) + b): X [N, H, W, C] (NHWC, 16-bit), Y [N, Ho, Wo, C]; b fp32 [C]; C % 8 == 0.
int ncnet_maxpool_bias_act(const void* X, void* Y, const float* b, int N, int H, int W, int C, int Ho, int Wo, int k,
                           int stride, int pad, int relu, int f16, hipStream_t stream);
// fp32 NHWC image -> stem im2col pairs A [N*Ho*Wo, 2 KP] bf16 (KP % 8 == 0, KP >= KH*KW*Cin)
int ncnet_stem_im2col_x3(const float* X, void* A, int N, int H, int W, int Cin, int KH, int KW, int stride, int pad,
                         int Ho, int Wo, int KP, hipStream_t stream);
// max-pool of [hi | lo] pairs: X [N,H,W,2C] -> Y [N,Ho,Wo,2C] bf16, C % 8 == 0
int ncnet_maxpool_x3(const void* X, void* Y, int N, int H, int W, int C, int Ho, int Wo, int k, int stride, int pad,
                     hipStream_t stream);
// X [rows, 2C] bf16 [hi | lo] pairs -> Y [rows, C] fp32, C % 8 == 0
int ncnet_x3_to_f32(const void* X, float* Y, long long rows, int C, hipStream_t stream);
// out[i] = bf16(src[idx[i]]), i < n (0 where idx[i] < 0 or >= nsrc: never a fault)
int ncnet_gather_bf16(const float* src, const int* idx, void* out, long long n, long long nsrc, hipStream_t s);
// nseg <= 4 segments (else -2): dst_s[map_s(j)] = sum_{r < R_s} src_s[r * N_s + j], map = idx_s[j]
// (< 0 or >= ndst_s drops the column) or j (idx_s null); N_s % 4 == 0, R_s >= 1 (else -3).
int ncnet_reduce_cols(const float* const* src, float* const* dst, const int* const* idx, const int* R, const int* N,
                      const long long* ndst, int nseg, hipStream_t s);
// Sanitizer-tier self test: out[0] = 1 in release, 0 (after an NCNET_CHECK line) in the debug build.
int ncnet_debug_selftest(int* out, hipStream_t stream);

// ---- LDS poison tier, test support (csrc/lds_poison.hip) ------------------
// Fill all 160 KiB of LDS of every CU with `pattern`: rounds (1..64, else -3) x CU-count
// workgroups that each own a whole CU's LDS.
int ncnet_lds_poison(unsigned int pattern, int rounds, hipStream_t stream);
// out int32 [G, n_words]: the first n_words words of each of G workgroups' uninitialised
// dynamic LDS of lds_bytes (a multiple of 4, <= 163840; n_words <= lds_bytes / 4; else -3).
int ncnet_lds_probe(int* out, int G, int n_words, int lds_bytes, hipStream_t stream);

// ---- correlation (csrc/corr.hip) ------------------------------------------
// y dtype: bf16 (fp8_scale == 0; ylo: optional low half) or OCP fp8 e4m3 scaled by fp8_scale.
// y_f16: y is IEEE half (no lo half, no fp8).  inv_norm [rows] or null.
int ncnet_l2norm_rows(const void* x, int x_is_bf16, void* y, float* inv_norm, int rows, int C, float fp8_scale,
                      void* ylo, int y_f16, hipStream_t stream);
int ncnet_l2norm_rows_bwd(const float* x, const float* g, const float* inv_norm, float* gx, int rows, int C,
                          hipStream_t stream);
// C[b] = A[amap[b]] . B[bmap[b]]^T (maps null: b); sA / sB / sC batch strides in elements;
// out_bf16 selects a 16-bit C (else fp32).
// fp8_out_scale != 0: A, B are OCP fp8 e4m3 and C = fp8_out_scale * (A . B^T).
// f16: A, B (and a 16-bit C) are IEEE half.
int ncnet_corr_gemm(const void* A, const void* B, void* C, const int* amap, const int* bmap, int batch, int M, int N,
                    int K, long long sA, long long sB, long long sC, int out_bf16, float fp8_out_scale, int f16,
                    hipStream_t stream);
// Fused correlation + 2x2x2x2 max-pool.  A rows / B rows must be in
// 2x2-block order; hA, wA, hB, wB even.  Volume b pools A[amap[b]] . B[bmap[b]]^T
// (maps null: b); batch = the number of volumes.
int ncnet_corr_gemm_pool2(const void* A, const void* B, float* pool_val, uint8_t* pool_idx, const int* amap,
                          const int* bmap, int batch, int hA, int wA, int hB, int wB, int K, long long sA, long long sB,
                          float fp8_out_scale, int f16, hipStream_t stream);

// ---- backward of the pooled correlation (csrc/corrpool_bwd.hip) -----------
// One direction of the feature gradient of ncnet_corr_gemm_pool2; rows in 2x2-block
// order, M = hA wA, N = hB wB, g fp32 / code uint8 [V, M/4, N/4] (code as the pool
// writes it; only the low bit of each 2-bit field is read).
//   dir 0: out[n][4I + a] = sum g[v,I,J] * fb[omap[v]][4J + b] over J and the volumes of image n,
//   dir 1: out[n][4J + b] = sum g[v,I,J] * fa[omap[v]][4I + a] over I and the volumes of image n,
// out fp32 [nout, M (dir 0) or N (dir 1), K], every element written once (zeros for an
// image without volumes), fixed summation order.  ft: the OTHER side's features
// transposed, bf16 [nother, K, ldr], ldr % 32 == 0 and >= that side's rows, zero
// past them.  g enters the MFMA rounded to bf16.  Volumes of output image n:
// vol[off[n] .. off[n + 1]) (off [nout + 1], vol [V], device int32, built and
// validated on the host); omap [V]: each volume's image on the other side.  An
// out-of-range list entry is skipped, never dereferenced.  K % 16 == 0 and ft, out
// 16-byte aligned (else -3).
int ncnet_corr_pool2_bwd(const void* ft, const float* g, const uint8_t* code, const int* off, const int* vol,
                         const int* omap, float* out, int V, int nout, int nother, int dir, int hA, int wA, int hB,
                         int wB, int K, int ldr, hipStream_t stream);

// ---- correlation-volume ops (csrc/volume.hip) -----------------------------
// x [rows, C] fp32 -> per-row max, first argmax (arg or null) and se (or null):
// sum_kind 1 sum exp(x - max), 2 plain sum
int ncnet_stats_rows(const float* x, float* mx, int* arg, float* se, long long rows, int C, int sum_kind,
                     hipStream_t s);
// x [V,R,C] -> per-column stats [V,C].  work: nullptr (nchunk = 1) or 3 * V * nchunk * C floats of partials.
int ncnet_stats_cols(const float* x, float* mx, int* arg, float* se, int V, int R, int C, float* work, int nchunk,
                     int sum_kind, hipStream_t s);
// row and column stats in one pass: work = 3 * V * (nct * R + nrt * C) floats of partials
// (nrt = ceil(R / 64), nct = ceil(C / 256)).  sum_kind 0: max / argmax only (rse, cse ignored).
// 16-byte loads when C % 4 == 0 and x is 16-byte aligned, else scalar loads (any alignment).
int ncnet_stats2d(const float* x, float* rmx, int* rarg, float* rse, float* cmx, int* carg, float* cse, int V, int R,
                  int C, float* work, int sum_kind, hipStream_t s);
// one volume's bidirectional match candidates from its column (B cells) and row (A cells)
// stats: m [N,5], sc [N] fp32, key [N] int64, N = fs1*fs2 + fs3*fs4; code: packed 2-bit offsets or null
int ncnet_match_candidates(const float* cmx, const float* cse, const int* carg, const float* rmx, const float* rse,
                           const int* rarg, const uint8_t* code, int fs1, int fs2, int fs3, int fs4, int k, float* m,
                           float* sc, long long* key, hipStream_t s);
// mutual matching; outputs optional (null).  x_f16: out_x / out_xt IEEE half (else bf16).
// pad_ks > 0: out_x / out_xt are padded bf16 planes for kernel size pad_ks (I2 x J2 = R, K2 x L2 = C)
int ncnet_mm_apply(const float* c, const float* rmax, const float* cmax, float* out_f32, void* out_x, void* out_xt,
                   int V, int R, int C, float eps, int x_f16, int pad_ks, int I2, int J2, int K2, int L2,
                   hipStream_t s);
// work: nullptr (separate row / column passes) or V * (ceil(C/256) * R + ceil(R/64) * C) floats (one pass;
// 16-byte loads when C % 4 == 0 and c, g are 16-byte aligned, else scalar loads)
int ncnet_mm_bwd(const float* c, const float* g, const float* rmax, const int* rarg, const float* cmax,
                 const int* carg, float* rsum, float* csum, float* gc, int V, int R, int C, float eps, float* work,
                 hipStream_t s);
// z [2*Vh, R, C] (second half stored as [C, R]) -> y [Vh, R, C]
int ncnet_combine_fwd(const float* z, float* y, int Vh, int R, int C, hipStream_t s);
// gz (and gzl, the bf16x3 low half, or null) bf16 in z's layout
int ncnet_combine_bwd(const float* g, const float* z, void* gz, void* gzl, int Vh, int R, int C, hipStream_t s);
// norm: 1 'softmax', 2 'l1' (eps), 0 none -- rse / cse from stats with the matching sum_kind; gscale [1] or null
int ncnet_softmax_max_bwd(const float* x, const float* rmax, const int* rarg, const float* rse, const float* cmax,
                          const int* carg, const float* cse, const float* wr, const float* wc, float* gx, int V, int R,
                          int C, int norm, float eps, const float* gscale, hipStream_t s);
// weak-loss score value out [1] fp32 from the row / column stats
int ncnet_score_sum(const float* rmax, const float* rse, const float* cmax, const float* cse, const float* wr,
                    const float* wc, int V, int R, int C, int norm, float eps, float* out, hipStream_t s);
// x [V,I,J,K,L] -> y fp32, code uint8 [V,I/ks,J/ks,K/ks,L/ks]; 1 <= ks <= 4
int ncnet_maxpool4d(const void* x, int x_is_bf16, float* y, uint8_t* code, int V, int I, int J, int K, int L, int ks,
                    hipStream_t s);
// x [V,R,C] -> y [V,C,R]; elem_bytes 2 or 4
int ncnet_transpose(const void* x, void* y, int elem_bytes, int V, int R, int C, hipStream_t s);

// ---- keypoint-supervised loss (csrc/kploss.hip) ---------------------------
// x [B, R = hA*wA, C = hB*wB] fp32; sp / tp [B, 2, N] (x, y) 1-based pixels, -1 padded; ssz / tsz
// [B, 3] (h, w, channels); 1 <= N <= 64 (else -3).  Writes the keypoint table (cells int32 [B, N, 8]
// = four A cells then four B cells, wts fp32 [B, N, 8] likewise, valid int32 [B, N]), lse / term
// [B, N, 2] (direction 0 A -> B, 1 B -> A; 0 for invalid keypoints) and out [2] =
// (loss, 1 / (2 max(1, Nvalid))).
int ncnet_kploss_fwd(const float* x, const float* sp, const float* tp, const float* ssz, const float* tsz, int B,
                     int N, int hA, int wA, int hB, int wB, int* cells, float* wts, int* valid, float* lse,
                     float* term, float* out, hipStream_t s);
// gx [B, R, C] = gscale[0] (or 1: null) * scale[0] * dloss/dx from the forward's table and lse;
// every element is written.
int ncnet_kploss_bwd(const float* x, const int* cells, const float* wts, const int* valid, const float* lse,
                     const float* scale, const float* gscale, float* gx, int B, int N, int R, int C, hipStream_t s);

// ---- dense correspondence loss (csrc/densece.hip) ---------------------------
// maps fp64 [B, 2, 12]: per image and side (0: the A cells, 1: the B cells) two affine maps (m00, m01, c0,
// m10, m11, c1) on unit coordinates, entries 0..5 into the other view, 6..11 into the source image.
// Writes the struct-of-arrays table with n = max(hA*wA, hB*wB): cells int32 / wts fp32 [B, 2, 4, n] (side 0:
// cells of the B grid, side 1: of the A grid), valid int32 [B, 2, n]; zero past a side's cell count and for
// invalid cells.
int ncnet_densece_table(const double* maps, int B, int hA, int wA, int hB, int wB, int n, int* cells, float* wts,
                        int* valid, hipStream_t s);
// x [B, R, C] fp32 with the table above and the stats2d statistics (sum_kind 1) rmax / rse [B, R],
// cmax / cse [B, C]: lse [B, 2, n] = max + log(se) per row / column, term [B, 2, n] = lse - sum_k w_k x[cell_k]
// (for an invalid cell and past a side's cell count: term 0, lse +inf, which is what the backward reads).
int ncnet_densece_fwd(const float* x, const int* cells, const float* wts, const int* valid, const float* rmax,
                      const float* rse, const float* cmax, const float* cse, int B, int R, int C, int n, float* lse,
                      float* term, hipStream_t s);
// term / valid [B, 2, n] -> out [3] = (loss, 1 / (2 max(1, N_A)), 1 / (2 max(1, N_B))); part: 4 B doubles of
// workspace.  Fixed order (one wave per (image, side), then one wave).
int ncnet_densece_reduce(const float* term, const int* valid, int B, int n, double* part, float* out, hipStream_t s);
// gx [B, R, C] = gscale[0] (or 1: null) * dloss/dx from the table (cells, wts), lse and scales = the forward's out [3];
// every element is written.  16-byte access when x and gx are 16-byte aligned, else scalar.
int ncnet_densece_bwd(const float* x, const int* cells, const float* wts, const float* lse,
                      const float* scales, const float* gscale, float* gx, int B, int R, int C, int n, hipStream_t s);

// ---- guarded flat Adam (csrc/optim.hip) -----------------------------------
// g may be longer than p (trailing loss-indicator slot); count / skipped int32 [1], step fp32 [1].
int ncnet_nonfinite_count(const float* g, long long n, int* count, hipStream_t s);
int ncnet_adam_masked(float* p, float* g, float* m, float* v, long long n, const int* count, const float* step,
                      float lr, float b1, float b2, float eps, float wd, float gscale, hipStream_t s);
int ncnet_adam_finalize(float* step, int* count, int* skipped, hipStream_t s);

// ---- data preparation (csrc/dataprep.hip) ---------------------------------
// Batched resize + normalise of packed HWC uint8 images: src bytes (device), meta int64 [B, 3] =
// (byte offset, H, W) (device), out fp32 [B, 3, oh, ow]; mean / stdv: 3 host floats each.
int ncnet_resize_norm_u8(const void* src, const long long* meta, float* out, int B, int oh, int ow, const float* mean,
                         const float* stdv, hipStream_t stream);
// The same with a per-image affine sampling map and gain / bias: params fp32 [B, 8] = (a0..a5, gain, bias) (device).
int ncnet_warp_norm_u8(const void* src, const long long* meta, const float* params, float* out, int B, int oh, int ow,
                       const float* mean, const float* stdv, hipStream_t stream);

// ---- P3P LO-RANSAC (csrc/pnp.hip) -----------------------------------------
// rays / X [M, 3, 3] fp64 -> P [M, 4, 3, 4] (valid poses first, NaN after), nsol [M]
int ncnet_p3p_solve(const double* rays, const double* X, int M, double* P, int* nsol, hipStream_t stream);
// rays / X [N, 3] fp64, offsets [B + 1] int32, keys [B] int64; P [B, 3, 4] fp64,
// ninl [B] int32, mask [N] uint8 (zeroed by the caller), list [N] int32 workspace,
// rounds [B] int32 or null.  cos_thr = cos(thr_rad), 0 < thr_rad < pi / 2.
int ncnet_p3p_ransac_batch(const double* rays, const double* X, const int* offsets, const long long* keys, int B,
                           long long N, double cos_thr, int max_iters, double confidence, int lo_iters, double* P,
                           int* ninl, uint8_t* mask, int* list, int* rounds, hipStream_t stream);

// ---- dense pose verification (csrc/pv.hip) --------------------------------
// poses per ncnet_pv_render launch (not a return code)
int ncnet_pv_pmax();
// xyz [N, 3] fp64, rgb [N, 3] fp32, KP [C, 3, 4] fp64 with C <= ncnet_pv_pmax();
// zbuf [C, h * w] u64 preset to the bits of +inf, winner [C, h * w] int32 preset to -1;
// synth [C, h, w, 3] fp32, flag [C, h, w] bytes.  C * h * w < 2^31, N < 2^31.
int ncnet_pv_render(const double* xyz, const float* rgb, long long N, const double* KP, int C, int h, int w,
                    unsigned long long* zbuf, int* winner, float* synth, uint8_t* flag, hipStream_t stream);
// oq / os [B, 8, H, W] fp32, flag [B, H, W] bytes, err [B, ny * nx] fp32
int ncnet_pv_desc_err(const float* oq, const float* os, const uint8_t* flag, int B, int H, int W, int ny, int nx,
                      float* err, hipStream_t stream);

}  // extern "C"
