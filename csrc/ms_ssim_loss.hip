// Multi-scale SSIM loss on the device (gfx950): loss = 1 - mean_{n,c} prod_j f_j^{w_j}, forward
// and a fused backward, for the two separable windows of ssim_loss.hip ("uniform7", "gauss11";
// same covariance factor, C1 / C2 and continuous model-range semantics).  Scale 1 is the input,
// scale j + 1 the 2 x 2 average pool of scale j (a trailing odd row / column is dropped).  Per
// (n, c), f_j (j < M) is the mean over the valid window origins of cs = A2 / B2 and f_M the
// mean of S = A1 A2 / (B1 B2), in the notation of ssim_loss.hip.  An (n, c) with any f_j <= 0
// has ms = 0 and an exactly zero gradient.  fp32 math, plain vector stores, no atomics.
//
// Derivatives of cs with respect to the three moments x enters (f the covariance factor):
//   dcs/dE[xy] = 2 f / B2,   dcs/dE[xx] = -f cs / B2,   dcs/dm = 2 f (m cs - n) / B2
// (those of S are in ssim_loss.hip).  cs and S are symmetric in (x, y): the gradient of y is
// the same chain with the images swapped.
//
// Forward, one launch per scale.  One workgroup = a 16 x 64 PIXEL tile of one (n, c); the
// grid covers every pixel, not only the window origins, because the workgroup that filters
// scale j also writes its 8 x 32 piece of scale j + 1 (x and y, fp32) from the pixels it has
// staged: every scale is read from HBM once and there is no pooling pass.  It stages the tile
// plus the K - 1 halo below / right as fp32 through the input strides, filters, and writes one
// partial sum of cs (of S at the last scale) over its valid origins.
//
// Finalize, one launch.  One wave per (n, c) sums that pair's partials of every scale in a
// fixed order (double), forms ms and the backward coefficients
//   coef[j][n][c] = -w_j ms / (f_j N C count_j)      (0 where any f_j <= 0)
// and the term 1 - ms, which the project's fixed-order sum reduces to the scalar loss.
//
// Backward, one launch per scale, coarsest first.  One workgroup = a 24 x 32 pixel tile.  It
// stages x and y with a 2 (K - 1) halo, recomputes the moments of the (24 + K - 1) x
// (32 + K - 1) origins whose windows touch its pixels (nothing per origin reaches HBM),
// evaluates (a, b, c) = d cs / d (m, E[xx], E[xy]) there (of S at the last scale; zero at
// origins that are not valid windows), applies the transposed separable filter and writes
//   G_j = gout coef_j[n,c] (W*a + 2 x W*b + y W*c) + 1/4 G_{j+1}[r/2, c/2]
// (the second term only where the parent pixel exists): the average pool's adjoint is folded
// into the next finer launch.  G_j is fp32 for j >= 2 and in x's dtype and layout for j = 1.
//
// Filter core.  ssim_loss.hip reads LDS K times per output and plane in every pass.  Here a
// thread owns a short run of SEG consecutive outputs of one row (horizontal passes) or one
// column (vertical passes) and slides over its SEG + K - 1 inputs: each input is read from
// LDS once and added with tap g[t] into the accumulator of output (input - t), all indices
// compile-time constants after unrolling, so the accumulators are registers and exactly K FMAs
// are spent per output and plane.  A ring of K accumulators walking a whole row or column would
// leave most of the 256 threads idle (a tile has 26 .. 44 rows and 32 .. 74 columns); the runs
// are therefore as short as keeps (rows or columns) x runs <= 256 (3 .. 9 outputs), shorter
// than K, which makes the ring a plain array of SEG accumulators.  LDS reads per output and
// plane fall from K to (SEG + K - 1) / SEG: 3.5 in the forward's vertical pass (was 11).
//
// LDS row strides.  Vertical passes: the lanes of a wave are consecutive columns of one run,
// conflict-free at any stride.  Horizontal passes: the lanes are (row i, run q) with q fastest
// and read word i * stride + q * SEG + s; every stride is ODD (the even tile width + 1), so
// rows i and i + 1 start an odd number of banks apart.  In the forward (SEG 8, 8 runs per row,
// 8 rows per wave) bank = 8 q + (i * stride mod 64) and i * stride mod 8 runs through all
// residues: all 64 lanes hit different banks.  The backward's runs (5 .. 9) leave some 2-way
// conflicts.
//
// Backward tile.  24 x 32 pixels recompute 34 x 42 / 768 = 1.86 origins per pixel for gauss11
// (1.48 for uniform7; ssim_loss.hip: 2.13) and is the largest tile whose planes fit 64 KB:
// x, y staged (2 planes) + 5 moment planes + 3 coefficient planes.  For gauss11 that needs the
// coefficient planes to overlay the staged images (dead once the moments are filtered; a
// thread keeps its own three pixels of x and y in registers), 56.5 KB; uniform7 fits without
// the overlay, 55.1 KB.  The transposed filter's intermediate overlays the moment planes.
#include "ssim_dev.h"

namespace p2p {

constexpr int MS_MAXM = 5;
constexpr int MF_H = 16, MF_W = 64;   // forward tile (pixels == window origins)
constexpr int MB_H = 24, MB_W = 32;   // backward tile (pixels)
constexpr int MS_LDS_LIMIT = 64 * 1024;

constexpr int ms_cdiv(int a, int b) { return (a + b - 1) / b; }
// shortest run such that lines x runs-per-line fits the 256 threads
constexpr int ms_seg(int lines, int outs) {
  int s = 1;
  while (lines * ms_cdiv(outs, s) > 256) ++s;
  return s;
}

struct MsArgs {
  const void* x;          // this scale's images (scale 1: the inputs; else the fp32 pyramid)
  const void* y;
  Strides4 xs, ys;        // of x and y
  int N, C, H, W, tiles_h, tiles_w;
  SsimWindow w;
  // forward
  float* px;              // next scale's x, y: fp32 [N, C, H / 2, W / 2] (unused at the last scale)
  float* py;
  float* ws;              // one partial per workgroup, [N * C][tiles_h * tiles_w]
  // backward
  void* dx;               // G of this scale
  Strides4 ds;
  const float* gpar;      // G of the next scale, fp32 [N, C, H / 2, W / 2], or null
  const float* coef;      // [N * C] of this scale
  const float* gout;      // dL/dloss on the device
};

struct MsFinArgs {
  const float* ws;
  long off[MS_MAXM];      // first partial of scale j
  int tiles[MS_MAXM];     // partials per (n, c)
  double inv_count[MS_MAXM];
  double w[MS_MAXM];
  int M, NC;
  float *ms, *coef, *term;
};

// horizontal K-tap filter of the five moments, sliding: staged [IH][OW + K - 1] (stride LS) ->
// hm[5][IH][OW] (stride PS).  One thread = SEG outputs of one row.
template <int K, int IH, int OW, int LS, int PS, int SEG>
P2P_SSIM_DEV void ms_hpass(const MsArgs& m, const float* lx, const float* ly, float* hm) {
  constexpr int NSEG = ms_cdiv(OW, SEG), IW = OW + K - 1;
  constexpr bool RAGGED = NSEG * SEG != OW;
  static_assert(IH * NSEG <= 256, "one run per thread");
  const int e = threadIdx.x;
  if (e >= IH * NSEG) return;
  const int q = e % NSEG, i = e / NSEG, j0 = q * SEG;
  float acc[5][SEG];
#pragma unroll
  for (int p = 0; p < 5; ++p)
#pragma unroll
    for (int o = 0; o < SEG; ++o) acc[p][o] = 0.f;
#pragma unroll
  for (int s = 0; s < SEG + K - 1; ++s) {
    const int j = RAGGED ? min(j0 + s, IW - 1) : j0 + s;   // past the row: feeds no kept output
    const float u = lx[i * LS + j], v = ly[i * LS + j];
    const float h[5] = {u, v, u * u, v * v, u * v};
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const int o = s - t;
      if (o >= 0 && o < SEG) {
#pragma unroll
        for (int p = 0; p < 5; ++p) acc[p][o] = fmaf(m.w.g[t], h[p], acc[p][o]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < SEG; ++o)
    if (!RAGGED || j0 + o < OW) {
#pragma unroll
      for (int p = 0; p < 5; ++p) hm[(p * IH + i) * PS + j0 + o] = acc[p][o];
    }
}

// vertical K-tap filter of the planes hm[5][IH][.] (stride PS), sliding down column j from row
// i0: the moments of the SEG origins (i0 .. i0 + SEG - 1, j)
template <int K, int IH, int PS, int SEG>
P2P_SSIM_DEV void ms_vpass(const MsArgs& m, const float* hm, int i0, int j, float acc[SEG][5]) {
#pragma unroll
  for (int o = 0; o < SEG; ++o)
#pragma unroll
    for (int p = 0; p < 5; ++p) acc[o][p] = 0.f;
#pragma unroll
  for (int s = 0; s < SEG + K - 1; ++s) {
    const int i = min(i0 + s, IH - 1);   // past the planes: feeds no kept origin
    float h[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) h[p] = hm[(p * IH + i) * PS + j];
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const int o = s - t;
      if (o >= 0 && o < SEG) {
#pragma unroll
        for (int p = 0; p < 5; ++p) acc[o][p] = fmaf(m.w.g[t], h[p], acc[o][p]);
      }
    }
  }
}

template <typename T, int K, bool LAST>
__global__ void P2P_SCALAR_F32 __launch_bounds__(256) ms_ssim_fwd_kernel(MsArgs m) {
  constexpr int IH = MF_H + K - 1, IW = MF_W + K - 1;
  constexpr int LS = IW + 1, PS = MF_W + 1;    // odd strides: see the file header
  constexpr int HSEG = 8, VSEG = MF_H * MF_W / 256;
  static_assert(LS % 2 == 1 && PS % 2 == 1 && MF_H % 2 == 0 && MF_W % 2 == 0, "odd strides, even tile");
  static_assert(MF_W == 64 && VSEG * 256 == MF_H * MF_W, "one wave per run of rows");
  __shared__ float lx[IH * LS], ly[IH * LS];
  __shared__ float hm[5 * IH * PS];
  __shared__ float red[4];
  static_assert(sizeof(float) * (2 * IH * LS + 5 * IH * PS + 4) <= MS_LDS_LIMIT, "forward LDS footprint");
  const int tid = threadIdx.x;
  const int n = blockIdx.z, c = blockIdx.y / m.tiles_h, ty = blockIdx.y % m.tiles_h;
  const int r0 = ty * MF_H, c0 = blockIdx.x * MF_W;
  const T* X = static_cast<const T*>(m.x) + n * m.xs.n + c * m.xs.c;
  const T* Y = static_cast<const T*>(m.y) + n * m.ys.n + c * m.ys.c;

  ssim_stage<T, IH, IW, LS>(m, X, Y, r0, c0, lx, ly);
  __syncthreads();
  if (!LAST) {
    // this tile's piece of the next scale; a pooled pixel inside H / 2 x W / 2 has all four
    // parents inside the image (and the tile: its corner is even)
    const int H2 = m.H >> 1, W2 = m.W >> 1;
    const long base = ((long)n * m.C + c) * H2 * W2;
    for (int e = tid; e < (MF_H / 2) * (MF_W / 2); e += 256) {
      const int pi = e / (MF_W / 2), pj = e % (MF_W / 2), pr = r0 / 2 + pi, pc = c0 / 2 + pj;
      if (pr < H2 && pc < W2) {
        const int o = 2 * pi * LS + 2 * pj;
        m.px[base + (long)pr * W2 + pc] = 0.25f * ((lx[o] + lx[o + 1]) + (lx[o + LS] + lx[o + LS + 1]));
        m.py[base + (long)pr * W2 + pc] = 0.25f * ((ly[o] + ly[o + 1]) + (ly[o + LS] + ly[o + LS + 1]));
      }
    }
  }
  // (halo columns / rows past the image are zeros and only feed origins that are not valid)
  ms_hpass<K, IH, MF_W, LS, PS, HSEG>(m, lx, ly, hm);
  __syncthreads();
  const int j = tid & 63, i0 = (tid >> 6) * VSEG;
  float s[VSEG][5];
  ms_vpass<K, IH, PS, VSEG>(m, hm, i0, j, s);
  float acc = 0.f;
#pragma unroll
  for (int o = 0; o < VSEG; ++o)
    if (r0 + i0 + o <= m.H - K && c0 + j <= m.W - K) acc += ssim_point<LAST>(s[o], m.w);
  acc = warp_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const long blk = (((long)n * m.C + c) * m.tiles_h + ty) * m.tiles_w + blockIdx.x;
    m.ws[blk] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

__device__ __forceinline__ double ms_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per (n, c): f_j, ms, 1 - ms and the backward coefficients
__global__ void __launch_bounds__(256) ms_ssim_finalize_kernel(MsFinArgs a) {
  const int nc = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (nc >= a.NC) return;
  double f[MS_MAXM], ms = 1.0;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < MS_MAXM; ++j) {
    if (j >= a.M) break;
    const float* p = a.ws + a.off[j] + (long)nc * a.tiles[j];
    double s = 0.0;
    for (int t = lane; t < a.tiles[j]; t += 64) s += (double)p[t];
    f[j] = ms_wave_sum(s) * a.inv_count[j];
    ok = ok && f[j] > 0.0;
  }
#pragma unroll
  for (int j = 0; j < MS_MAXM; ++j)
    if (j < a.M) ms *= ok ? pow(f[j], a.w[j]) : 0.0;
  if (lane != 0) return;
  a.ms[nc] = (float)ms;
  a.term[nc] = (float)(1.0 - ms);
#pragma unroll
  for (int j = 0; j < MS_MAXM; ++j)
    if (j < a.M) a.coef[(long)j * a.NC + nc] = ok ? (float)(-a.w[j] * ms / (f[j] * a.NC) * a.inv_count[j]) : 0.f;
}

template <typename T, int K, bool LAST>
__global__ void P2P_SCALAR_F32 __launch_bounds__(256) ms_ssim_bwd_kernel(MsArgs m) {
  constexpr int R = K - 1;
  constexpr int OH = MB_H + R, OW = MB_W + R;   // origins whose windows touch the tile
  constexpr int IH = OH + R, IW = OW + R;       // inputs those origins read
  constexpr int LS = IW + 1, PS = OW + 1, CS = OW + 1, TS = MB_W + 1;   // odd strides
  constexpr int HSEG = ms_seg(IH, OW);          // moments, horizontal: runs of one row
  constexpr int NV = 256 / OW, VSEG = ms_cdiv(OH, NV);   // moments, vertical: runs of one column
  constexpr int TSEG = ms_seg(OH, MB_W), NT = ms_cdiv(MB_W, TSEG);   // transposed, horizontal
  constexpr int PV = MB_H * MB_W / 256;         // transposed, vertical: pixels per thread
  constexpr int A_F = 2 * IH * LS, B_F = 5 * IH * PS, C_F = 3 * OH * CS;
  constexpr bool OVERLAY = C_F <= A_F;          // coefficient planes over the staged images
  static_assert(LS % 2 == 1 && PS % 2 == 1 && MB_W == 32 && PV * 256 == MB_H * MB_W, "strides and tile");
  static_assert(NV * VSEG >= OH && NV * OW <= 256 && OH * NT <= 256, "one run per thread");
  static_assert(3 * OH * TS <= B_F, "the transposed filter's planes overlay the moment planes");
  __shared__ float lds[A_F + B_F + (OVERLAY ? 0 : C_F)];
  static_assert(sizeof(lds) <= MS_LDS_LIMIT, "backward LDS footprint");
  float *lx = lds, *ly = lds + IH * LS, *hm = lds + A_F, *th = hm;
  float* cf = OVERLAY ? lds : hm + B_F;
  const int tid = threadIdx.x;
  const int n = blockIdx.z, c = blockIdx.y / m.tiles_h, ty = blockIdx.y % m.tiles_h;
  const int p0r = ty * MB_H, p0c = blockIdx.x * MB_W;   // first pixel of the tile
  const int br = p0r - R, bc = p0c - R;                 // first origin == first staged input
  const T* X = static_cast<const T*>(m.x) + n * m.xs.n + c * m.xs.c;
  const T* Y = static_cast<const T*>(m.y) + n * m.ys.n + c * m.ys.c;

  ssim_stage<T, IH, IW, LS>(m, X, Y, br, bc, lx, ly);
  __syncthreads();
  // this thread's pixels (column pj, rows pi0 .. pi0 + PV - 1), kept before cf may overlay them
  const int pj = tid & 31, pi0 = (tid >> 5) * PV;
  float xv[PV], yv[PV];
#pragma unroll
  for (int u = 0; u < PV; ++u) {
    xv[u] = lx[(pi0 + u + R) * LS + pj + R];
    yv[u] = ly[(pi0 + u + R) * LS + pj + R];
  }
  ms_hpass<K, IH, OW, LS, PS, HSEG>(m, lx, ly, hm);
  __syncthreads();
  if (tid < NV * OW) {
    const int j = tid % OW, i0 = (tid / OW) * VSEG, gc = bc + j;
    float s[VSEG][5];
    ms_vpass<K, IH, PS, VSEG>(m, hm, i0, j, s);
#pragma unroll
    for (int o = 0; o < VSEG; ++o) {
      const int i = i0 + o, gr = br + i;
      if (i >= OH) break;
      float a = 0.f, b = 0.f, cc = 0.f;
      if (gr >= 0 && gr <= m.H - K && gc >= 0 && gc <= m.W - K) ssim_point_grad<LAST>(s[o], m.w, a, b, cc);
      cf[(0 * OH + i) * CS + j] = a; cf[(1 * OH + i) * CS + j] = b; cf[(2 * OH + i) * CS + j] = cc;
    }
  }
  __syncthreads();
  // transposed filter, horizontal: pixel column p takes origin column p + R - t with tap t;
  // sliding over the origin columns j0 .. j0 + TSEG + R - 1 of one row
  if (tid < OH * NT) {
    const int q = tid % NT, i = tid / NT, j0 = q * TSEG;
    float acc[3][TSEG];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int o = 0; o < TSEG; ++o) acc[p][o] = 0.f;
#pragma unroll
    for (int s = 0; s < TSEG + R; ++s) {
      const int j = min(j0 + s, OW - 1);   // past the row: feeds no kept pixel
      const float h[3] = {cf[(0 * OH + i) * CS + j], cf[(1 * OH + i) * CS + j], cf[(2 * OH + i) * CS + j]};
#pragma unroll
      for (int t = 0; t < K; ++t) {
        const int o = s - R + t;
        if (o >= 0 && o < TSEG) {
#pragma unroll
          for (int p = 0; p < 3; ++p) acc[p][o] = fmaf(m.w.g[t], h[p], acc[p][o]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < TSEG; ++o)
      if (j0 + o < MB_W) {
#pragma unroll
        for (int p = 0; p < 3; ++p) th[(p * OH + i) * TS + j0 + o] = acc[p][o];
      }
  }
  __syncthreads();
  // ... vertical, sliding down the thread's column, then G = scale (A + 2 x B + y C) + parent / 4
  float acc[3][PV];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int o = 0; o < PV; ++o) acc[p][o] = 0.f;
#pragma unroll
  for (int s = 0; s < PV + R; ++s) {
    const float h[3] = {th[(0 * OH + pi0 + s) * TS + pj], th[(1 * OH + pi0 + s) * TS + pj],
                        th[(2 * OH + pi0 + s) * TS + pj]};
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const int o = s - R + t;
      if (o >= 0 && o < PV) {
#pragma unroll
        for (int p = 0; p < 3; ++p) acc[p][o] = fmaf(m.w.g[t], h[p], acc[p][o]);
      }
    }
  }
  const float scale = m.gout[0] * m.coef[n * m.C + c];
  const int H2 = m.H >> 1, W2 = m.W >> 1, col = p0c + pj;
  const float* P = m.gpar ? m.gpar + ((long)n * m.C + c) * H2 * W2 : nullptr;
  T* D = static_cast<T*>(m.dx) + n * m.ds.n + c * m.ds.c;
#pragma unroll
  for (int u = 0; u < PV; ++u) {
    const int r = p0r + pi0 + u;
    if (r >= m.H || col >= m.W) continue;
    float v = scale * (acc[0][u] + 2.f * xv[u] * acc[1][u] + yv[u] * acc[2][u]);
    if (P && (r >> 1) < H2 && (col >> 1) < W2) v += 0.25f * P[(long)(r >> 1) * W2 + (col >> 1)];
    D[r * m.ds.h + col * m.ds.w] = (T)v;
  }
}

// the shapes the op accepts: 1 <= M <= 5 scales, the coarsest still holds one window, and the
// finest scale's grid of TH-row tiles fits
static bool ms_shape_ok(int N, int C, int H, int W, int K, int M, int TH) {
  if (K == 0 || M < 1 || M > MS_MAXM || !ssim_grid_ok(N, C, ms_cdiv(H, TH))) return false;
  return ((H < W ? H : W) >> (M - 1)) >= K;
}

// contiguous fp32 NCHW: the pyramid and the coarser scales' gradients
static Strides4 ms_dense(int C, int h, int w) { return {(long)C * h * w, (long)h * w, w, 1}; }

template <bool FWD>
static void ms_launch(int K, int dtype, bool last, const MsArgs& m, hipStream_t st) {
  if (FWD && last) P2P_SSIM_LAUNCH(ms_ssim_fwd_kernel, K, dtype, m, st, , true);
  else if (FWD) P2P_SSIM_LAUNCH(ms_ssim_fwd_kernel, K, dtype, m, st, , false);
  else if (last) P2P_SSIM_LAUNCH(ms_ssim_bwd_kernel, K, dtype, m, st, , true);
  else P2P_SSIM_LAUNCH(ms_ssim_bwd_kernel, K, dtype, m, st, , false);
}

}  // namespace p2p

// floats of the fp32 pyramid: scales 2 .. M, x then y of each, [N, C, H_j, W_j]
extern "C" long p2p_ms_ssim_pyr(int N, int C, int H, int W, int M) {
  long n = 0;
  for (int j = 1; j < M; ++j) n += 2L * N * C * (H >> j) * (W >> j);
  return n;
}

// floats of forward workspace: the partials of every scale, the N * C terms 1 - ms and 256
// for the two-stage final sum
extern "C" long p2p_ms_ssim_ws(int N, int C, int H, int W, int M) {
  long n = 0;
  for (int j = 0; j < M; ++j)
    n += (long)N * C * (((H >> j) + p2p::MF_H - 1) / p2p::MF_H) * (((W >> j) + p2p::MF_W - 1) / p2p::MF_W);
  return n + (long)N * C + 256;
}

// dtype: 0 = fp32, 1 = bf16.  strides[8] = (n, c, h, w) of x, then of y.  weights[M].
// Writes the pyramid, ms[N * C], coef[M][N * C] and loss[0].
extern "C" int p2p_ms_ssim_fwd(const void* x, const void* y, int dtype, const long* strides, int N, int C, int H,
                               int W, int window, double data_range, const double* weights, int M, float* pyr,
                               float* ws, float* ms, float* coef, float* loss, hipStream_t st) {
  using namespace p2p;
  MsArgs m{};
  const int K = ssim_window(window, data_range, m.w);
  if (!ms_shape_ok(N, C, H, W, K, M, MF_H)) return -1;
  MsFinArgs fin{};
  fin.ws = ws; fin.M = M; fin.NC = N * C;
  m.N = N; m.C = C;
  m.x = x; m.y = y;
  m.xs = strides4(strides); m.ys = strides4(strides + 4);
  long woff = 0;
  for (int j = 0; j < M; ++j) {
    const int h = H >> j, w = W >> j, h2 = h >> 1, w2 = w >> 1;
    const long sz2 = (long)N * C * h2 * w2;
    m.H = h; m.W = w;
    m.tiles_h = ms_cdiv(h, MF_H);
    m.tiles_w = ms_cdiv(w, MF_W);
    m.ws = ws + woff;
    m.px = pyr; m.py = pyr + sz2;
    ms_launch<true>(K, j == 0 ? dtype : 0, j == M - 1, m, st);
    fin.off[j] = woff;
    fin.tiles[j] = m.tiles_h * m.tiles_w;
    fin.inv_count[j] = 1.0 / ((double)(h - K + 1) * (w - K + 1));
    fin.w[j] = weights[j];
    woff += (long)N * C * fin.tiles[j];
    // the next scale reads what this one pooled
    m.x = m.px; m.y = m.py;
    m.xs = m.ys = ms_dense(C, h2, w2);
    pyr += 2 * sz2;
  }
  fin.ms = ms; fin.coef = coef; fin.term = ws + woff;
  hipLaunchKernelGGL(ms_ssim_finalize_kernel, dim3((N * C + 3) / 4), dim3(256), 0, st, fin);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  return p2p_sum_fixed(fin.term, (long)N * C, (float)(1.0 / ((double)N * C)), loss, st);
}

// strides[12] = (n, c, h, w) of x, of y, then of dx.  dx = dL/dx; for dL/dy pass the images
// swapped and swap = 1 (the pyramid's y planes are then the differentiated ones).
// gtmp: N * C * sum_{j >= 2} H_j W_j floats for the coarser scales' gradients.
extern "C" int p2p_ms_ssim_bwd(const void* x, const void* y, int dtype, const long* strides, int N, int C, int H,
                               int W, int window, double data_range, int M, const float* pyr, int swap,
                               const float* coef, const float* gout, float* gtmp, void* dx, hipStream_t st) {
  using namespace p2p;
  MsArgs m{};
  const int K = ssim_window(window, data_range, m.w);
  if (!ms_shape_ok(N, C, H, W, K, M, MB_H)) return -1;
  m.N = N; m.C = C; m.gout = gout;
  // offsets of scale j's pair in the pyramid and of its gradient in gtmp (j >= 1)
  long poff[MS_MAXM] = {0}, goff[MS_MAXM] = {0};
  for (int j = 1; j < M; ++j) {
    const long sz = (long)N * C * (H >> j) * (W >> j);
    if (j + 1 < M) { poff[j + 1] = poff[j] + 2 * sz; goff[j + 1] = goff[j] + sz; }
  }
  for (int j = M - 1; j >= 0; --j) {
    const int h = H >> j, w = W >> j;
    m.H = h; m.W = w;
    m.tiles_h = ms_cdiv(h, MB_H);
    m.tiles_w = ms_cdiv(w, MB_W);
    m.coef = coef + (long)j * N * C;
    m.gpar = j + 1 < M ? gtmp + goff[j + 1] : nullptr;
    if (j == 0) {
      m.x = x; m.y = y; m.dx = dx;
      m.xs = strides4(strides); m.ys = strides4(strides + 4); m.ds = strides4(strides + 8);
    } else {
      const long sz = (long)N * C * h * w;
      const float *p0 = pyr + poff[j], *p1 = p0 + sz;
      m.x = swap ? p1 : p0; m.y = swap ? p0 : p1; m.dx = gtmp + goff[j];
      m.xs = m.ys = m.ds = ms_dense(C, h, w);
    }
    ms_launch<false>(K, j == 0 ? dtype : 0, j == M - 1, m, st);
  }
  return (int)hipGetLastError();
}
