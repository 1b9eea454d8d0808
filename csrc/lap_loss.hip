// Laplacian-pyramid L1 loss on the device (gfx950): loss = sum_j mean_{n,c,pixels} |b_j| over
// the M bands of d = x - y, forward and backward.  g_0 = d; g_{j+1} = D g_j with D the separable
// binomial k = [1, 4, 6, 4, 1] / 16 on the edge-replicated image (indices clamped), sampled at
// even rows and columns; U doubles each axis, per axis with clamped indices
//   up[2i] = (g[i-1] + 6 g[i] + g[i+1]) / 8,   up[2i+1] = (g[i] + g[i+1]) / 2;
// b_j = g_j - U g_{j+1} for j < M - 1 and b_{M-1} = g_{M-1}.  H and W are multiples of 2^(M-1),
// so every level halves exactly.  fp32 math, plain vector stores, no atomics, no host sync.
//
// The operator is linear in d, so one difference image is enough (the SSIM pyramids carry x
// and y), and |.| is the only nonlinearity: its derivative sign(b_j) (sign(0) = 0) is all the
// backward needs.  What lives between the passes is the int8 sign pyramid, 4/3 byte per pixel.
//
// Forward, one launch per level.  One workgroup = an even-aligned LT_H x LT_W tile of level j
// of one (n, c).  It stages g_j with a 4-pixel halo as fp32 through clamped indices (the edge
// replication; level 0 forms x - y on the way in through the input strides), runs the
// horizontal then the vertical 5-tap pass at even positions, which leaves the
// (LT_H / 2 + 2) x (LT_W / 2 + 2) piece of g_{j+1} around the tile in LDS, stores the interior
// of that piece as the next level (fp32: every level is read from HBM once and there is no
// pooling pass), applies U in polyphase form out of LDS, stores sign(b_j) and reduces |b_j| to
// one partial per workgroup, scaled by c_j = 1 / (N C H_j W_j).  A piece entry outside the
// level is the CLAMPED ENTRY of g_{j+1} (the entry of the clamped index, recomputed from the
// staged halo), not a filter over clamped g_j: that is what U reads in the oracle.  The launch
// of level M - 1 only takes |g|, its sign and the partial.  The partials of all levels go
// through the project's fixed-order sum.
//
// Backward, one launch per level, coarsest first:
//   T_j = c_j s_j - U^T (c_{j-1} s_{j-1}) + D^T T_{j+1}
// (the U^T term absent at j = 0, the D^T term at j = M - 1); dL/dx = gout T_0.  One workgroup =
// an LT_H x LT_W tile of T_j.  It stages the (2 LT_H + 4) x (2 LT_W + 4) int8 signs of the
// finer level and the (LT_H / 2 + 2) x (LT_W / 2 + 2) fp32 piece of T_{j+1}, both zero outside
// their level, and applies the two adjoints separably, rows then columns.  Per axis, with n
// the length of the coarse side:
//   (U^T s)[q] = sum_{t=0..4} 2 k[t] s[2q - 2 + t]
//                + (q == 0) s[0] / 8 + (q == n - 1) (s[2n - 2] / 8 + s[2n - 1] / 2)
//   (D^T T)[r] = (T[m - 1] + 6 T[m] + T[m + 1]) / 16  (r = 2m),  (T[m] + T[m + 1]) / 4  (r = 2m + 1)
//                + (r == 0) 5 T[0] / 16 + (r == 2n - 1) T[n - 1] / 16
// The extra terms are the taps that the clamped borders fold onto the first and last entry
// (checked against the oracle's autograd, n = 1 included, where both folds hit one entry).
// T_j is fp32 scratch for j >= 1; the j = 0 launch writes gout T_0 in x's dtype and layout and
// dy = -dx in the same store loop when y needs it.
//
// LDS: forward 19.4 KB, backward 33.4 KB (static_asserts below); the rows a wave reads in the
// passes are consecutive words, so the strides need no padding.
#include "ssim_dev.h"

namespace p2p {

constexpr int LAP_MAXM = 6;
constexpr int LT_H = 32, LT_W = 64;                      // tile of a level (pixels), even
constexpr int LP_H = LT_H / 2 + 2, LP_W = LT_W / 2 + 2;   // piece of the next coarser level
constexpr int LF_H = LT_H + 8, LF_W = LT_W + 8;           // forward: tile + 4-pixel halo
constexpr int LS_H = 2 * LT_H + 4, LS_W = 2 * LT_W + 4;   // backward: signs of the finer level
constexpr int LAP_LDS_LIMIT = 64 * 1024;
static_assert(LT_H % 2 == 0 && LT_W % 2 == 0 && LT_H * LT_W % 256 == 0, "even tile, whole passes");

struct LapArgs {
  const void* x;          // level 0: the images; else g_j, dense fp32 (y unused)
  const void* y;
  Strides4 xs, ys;
  int N, C, H, W, tiles_h, tiles_w;   // H, W of this level
  float cj;               // 1 / (N C H W) of this level
  // forward
  float* next;            // g_{j+1}, dense fp32 [N, C, H / 2, W / 2]
  signed char* sign;      // s_j, dense [N, C, H, W]
  float* ws;              // one partial per workgroup
  // backward
  const signed char* fine;   // s_{j-1}, dense [N, C, 2H, 2W]
  float cf;               // c_{j-1}
  const float* coarse;    // T_{j+1}, dense fp32 [N, C, H / 2, W / 2]
  const float* gout;
  void* dx;               // T_j: fp32 scratch (j >= 1) or the gradient of x (j = 0)
  void* dy;               // j = 0: -dx, or null
  Strides4 ds;
};

P2P_SSIM_DEV int lap_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// block sum of the 256 threads' values in a fixed order, valid in thread 0
P2P_SSIM_DEV float lap_block_sum(float v, float* red) {
  v = warp_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// d = x - y at level 0, g_j else
template <typename T, bool FIRST>
P2P_SSIM_DEV float lap_load(const LapArgs& m, const T* X, const T* Y, int r, int c) {
  const float u = (float)X[r * m.xs.h + c * m.xs.w];
  return FIRST ? u - (float)Y[r * m.ys.h + c * m.ys.w] : u;
}

template <typename T, bool FIRST, bool LAST>
__global__ void P2P_SCALAR_F32 __launch_bounds__(256) lap_fwd_kernel(LapArgs m) {
  __shared__ float lg[LAST ? 1 : LF_H * LF_W];    // staged g_j
  __shared__ float lh[LAST ? 1 : LF_H * LP_W];    // after the horizontal pass
  __shared__ float lp[LAST ? 1 : LP_H * LP_W];    // piece of g_{j+1}
  __shared__ float red[4];
  static_assert(sizeof(float) * (LF_H * LF_W + LF_H * LP_W + LP_H * LP_W + 4) <= LAP_LDS_LIMIT,
                "forward LDS footprint");
  const int tid = threadIdx.x;
  const int n = blockIdx.z, c = blockIdx.y / m.tiles_h, ty = blockIdx.y % m.tiles_h;
  const int r0 = ty * LT_H, c0 = blockIdx.x * LT_W;
  const T* X = static_cast<const T*>(m.x) + n * m.xs.n + c * m.xs.c;
  const T* Y = FIRST ? static_cast<const T*>(m.y) + n * m.ys.n + c * m.ys.c : nullptr;
  signed char* S = m.sign + ((long)n * m.C + c) * m.H * m.W;
  float acc = 0.f;

  if (LAST) {
    for (int e = tid; e < LT_H * LT_W; e += 256) {
      const int r = r0 + e / LT_W, col = c0 + e % LT_W;
      if (r >= m.H || col >= m.W) continue;
      const float b = lap_load<T, FIRST>(m, X, Y, r, col);
      S[(long)r * m.W + col] = (signed char)((b > 0.f) - (b < 0.f));
      acc += fabsf(b);
    }
  } else {
    const int H2 = m.H >> 1, W2 = m.W >> 1;
    // g_j on rows r0 - 4 .. r0 + LT_H + 3, clamped into the level (edge replication)
    for (int e = tid; e < LF_H * LF_W; e += 256) {
      const int r = lap_clamp(r0 - 4 + e / LF_W, m.H), col = lap_clamp(c0 - 4 + e % LF_W, m.W);
      lg[e] = lap_load<T, FIRST>(m, X, Y, r, col);
    }
    __syncthreads();
    // piece column b is entry clamp(c0 / 2 - 1 + b) of g_{j+1}: its taps are the level's
    // columns 2p - 2 .. 2p + 2, staged columns 2p - c0 + 2 .. (inside the halo for every b)
    for (int e = tid; e < LF_H * LP_W; e += 256) {
      const int i = e / LP_W, b = e % LP_W;
      const float* g = lg + i * LF_W + 2 * lap_clamp(c0 / 2 - 1 + b, W2) - c0 + 2;
      lh[e] = ((g[0] + g[4]) + 4.f * (g[1] + g[3]) + 6.f * g[2]) * (1.f / 16.f);
    }
    __syncthreads();
    float* NX = m.next + ((long)n * m.C + c) * H2 * W2;
    for (int e = tid; e < LP_H * LP_W; e += 256) {
      const int a = e / LP_W, b = e % LP_W, pr = r0 / 2 - 1 + a, pc = c0 / 2 - 1 + b;
      const float* h = lh + (2 * lap_clamp(pr, H2) - r0 + 2) * LP_W + b;
      const float v = ((h[0] + h[4 * LP_W]) + 4.f * (h[LP_W] + h[3 * LP_W]) + 6.f * h[2 * LP_W]) * (1.f / 16.f);
      lp[e] = v;
      // the interior of the piece is this tile's part of the next level
      if (a >= 1 && a <= LT_H / 2 && b >= 1 && b <= LT_W / 2 && pr < H2 && pc < W2) NX[(long)pr * W2 + pc] = v;
    }
    __syncthreads();
    // b_j = g_j - U g_{j+1}: pixel (i, j) reads piece rows i / 2 .. i / 2 + 2 (entry i / 2 + 1
    // is its parent), columns likewise; even and odd positions take different taps
    for (int e = tid; e < LT_H * LT_W; e += 256) {
      const int i = e / LT_W, j = e % LT_W, r = r0 + i, col = c0 + j;
      if (r >= m.H || col >= m.W) continue;
      const float* p = lp + (i / 2) * LP_W + j / 2;
      float h[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float* q = p + a * LP_W;
        h[a] = (j & 1) ? (q[1] + q[2]) * 0.5f : ((q[0] + q[2]) + 6.f * q[1]) * 0.125f;
      }
      const float up = (i & 1) ? (h[1] + h[2]) * 0.5f : ((h[0] + h[2]) + 6.f * h[1]) * 0.125f;
      const float b = lg[(i + 4) * LF_W + j + 4] - up;
      S[(long)r * m.W + col] = (signed char)((b > 0.f) - (b < 0.f));
      acc += fabsf(b);
    }
  }
  acc = lap_block_sum(acc, red);
  if (tid == 0) {
    const long blk = (((long)n * m.C + c) * m.tiles_h + ty) * m.tiles_w + blockIdx.x;
    m.ws[blk] = acc * m.cj;
  }
}

// UT: the U^T term exists (j > 0); DT: the D^T term exists (j < M - 1); OUT: j == 0
template <typename T, bool UT, bool DT, bool OUT>
__global__ void P2P_SCALAR_F32 __launch_bounds__(256) lap_bwd_kernel(LapArgs m) {
  __shared__ signed char ls[UT ? LS_H * LS_W : 4];   // s_{j-1}, rows 2 r0 - 2 ..
  __shared__ float lu[UT ? LS_H * LT_W : 1];          // ... after the horizontal U^T
  __shared__ float lt[DT ? LP_H * LP_W : 1];          // T_{j+1}, rows r0 / 2 - 1 ..
  __shared__ float ld[DT ? LP_H * LT_W : 1];          // ... after the horizontal D^T
  static_assert(LS_H * LS_W + sizeof(float) * (LS_H * LT_W + LP_H * LP_W + LP_H * LT_W) <= LAP_LDS_LIMIT,
                "backward LDS footprint");
  const int tid = threadIdx.x;
  const int n = blockIdx.z, c = blockIdx.y / m.tiles_h, ty = blockIdx.y % m.tiles_h;
  const int r0 = ty * LT_H, c0 = blockIdx.x * LT_W;
  const long plane = (long)n * m.C + c;

  if (UT) {
    const int HF = 2 * m.H, WF = 2 * m.W;
    const signed char* F = m.fine + plane * HF * WF;
    for (int e = tid; e < LS_H * LS_W; e += 256) {
      const int r = 2 * r0 - 2 + e / LS_W, col = 2 * c0 - 2 + e % LS_W;
      ls[e] = (r >= 0 && r < HF && col >= 0 && col < WF) ? F[(long)r * WF + col] : (signed char)0;
    }
  }
  if (DT) {
    const int H2 = m.H >> 1, W2 = m.W >> 1;
    const float* P = m.coarse + plane * H2 * W2;
    for (int e = tid; e < LP_H * LP_W; e += 256) {
      const int r = r0 / 2 - 1 + e / LP_W, col = c0 / 2 - 1 + e % LP_W;
      lt[e] = (r >= 0 && r < H2 && col >= 0 && col < W2) ? P[(long)r * W2 + col] : 0.f;
    }
  }
  __syncthreads();
  if (UT) {
    // staged column 2 j + t is the fine column 2 q - 2 + t of q = c0 + j
    for (int e = tid; e < LS_H * LT_W; e += 256) {
      const int i = e / LT_W, j = e % LT_W, q = c0 + j;
      const signed char* s = ls + i * LS_W + 2 * j;
      float v = (float)(s[0] + 4 * s[1] + 6 * s[2] + 4 * s[3] + s[4]);
      if (q == 0) v += (float)s[2];
      if (q == m.W - 1) v += (float)(s[2] + 4 * s[3]);
      lu[e] = q < m.W ? v * 0.125f : 0.f;
    }
  }
  if (DT) {
    // staged column j / 2 + 1 is entry m = r / 2 of r = c0 + j
    for (int e = tid; e < LP_H * LT_W; e += 256) {
      const int i = e / LT_W, j = e % LT_W, r = c0 + j;
      const float* t = lt + i * LP_W + j / 2;
      float v = (j & 1) ? 4.f * (t[1] + t[2]) : (t[0] + t[2]) + 6.f * t[1];
      if (r == 0) v += 5.f * t[1];
      if (r == m.W - 1) v += t[1];
      ld[e] = r < m.W ? v * (1.f / 16.f) : 0.f;
    }
  }
  __syncthreads();
  const signed char* S = m.sign + plane * m.H * m.W;
  const float go = OUT ? m.gout[0] : 1.f;
  T* DX = static_cast<T*>(m.dx) + n * m.ds.n + c * m.ds.c;
  T* DY = OUT && m.dy ? static_cast<T*>(m.dy) + n * m.ds.n + c * m.ds.c : nullptr;
  for (int e = tid; e < LT_H * LT_W; e += 256) {
    const int i = e / LT_W, j = e % LT_W, r = r0 + i, col = c0 + j;
    if (r >= m.H || col >= m.W) continue;
    float v = m.cj * (float)S[(long)r * m.W + col];
    if (UT) {
      const float* u = lu + 2 * i * LT_W + j;
      float a = (u[0] + u[4 * LT_W]) + 4.f * (u[LT_W] + u[3 * LT_W]) + 6.f * u[2 * LT_W];
      if (r == 0) a += u[2 * LT_W];
      if (r == m.H - 1) a += u[2 * LT_W] + 4.f * u[3 * LT_W];
      v -= m.cf * (a * 0.125f);
    }
    if (DT) {
      const float* t = ld + (i / 2) * LT_W + j;
      float a = (i & 1) ? 4.f * (t[LT_W] + t[2 * LT_W]) : (t[0] + t[2 * LT_W]) + 6.f * t[LT_W];
      if (r == 0) a += 5.f * t[LT_W];
      if (r == m.H - 1) a += t[LT_W];
      v += a * (1.f / 16.f);
    }
    v *= go;
    const long o = r * m.ds.h + col * m.ds.w;
    DX[o] = (T)v;
    if (DY) DY[o] = (T)(-v);
  }
}

static bool lap_shape_ok(int N, int C, int H, int W, int M) {
  if (M < 1 || M > LAP_MAXM || H < 1 || W < 1 || !ssim_grid_ok(N, C, (H + LT_H - 1) / LT_H)) return false;
  const int mask = (1 << (M - 1)) - 1;
  return !(H & mask) && !(W & mask) && (long)N * C * H * W < (1L << 40);
}

static Strides4 lap_dense(int C, int h, int w) { return {(long)C * h * w, (long)h * w, w, 1}; }

static void lap_tiles(LapArgs& m, int N, int C, int h, int w) {
  m.H = h; m.W = w;
  m.tiles_h = (h + LT_H - 1) / LT_H;
  m.tiles_w = (w + LT_W - 1) / LT_W;
  m.cj = (float)(1.0 / ((double)N * C * h * w));
}

template <bool LAST>
static void lap_launch_fwd(int dtype, bool first, const LapArgs& m, hipStream_t st) {
  const dim3 grid(m.tiles_w, m.C * m.tiles_h, m.N), block(256);
  if (!first) hipLaunchKernelGGL((lap_fwd_kernel<float, false, LAST>), grid, block, 0, st, m);
  else if (dtype == 1) hipLaunchKernelGGL((lap_fwd_kernel<bf16, true, LAST>), grid, block, 0, st, m);
  else hipLaunchKernelGGL((lap_fwd_kernel<float, true, LAST>), grid, block, 0, st, m);
}

template <typename T, bool OUT>
static void lap_launch_bwd(bool ut, bool dt, const LapArgs& m, hipStream_t st) {
  const dim3 grid(m.tiles_w, m.C * m.tiles_h, m.N), block(256);
  if (ut && dt) hipLaunchKernelGGL((lap_bwd_kernel<T, true, true, OUT>), grid, block, 0, st, m);
  else if (ut) hipLaunchKernelGGL((lap_bwd_kernel<T, true, false, OUT>), grid, block, 0, st, m);
  else if (dt) hipLaunchKernelGGL((lap_bwd_kernel<T, false, true, OUT>), grid, block, 0, st, m);
  else hipLaunchKernelGGL((lap_bwd_kernel<T, false, false, OUT>), grid, block, 0, st, m);
}

}  // namespace p2p

// bytes of the sign pyramid: levels 0 .. M - 1, [N, C, H_j, W_j] int8 each
extern "C" long p2p_lap_signs(int N, int C, int H, int W, int M) {
  long n = 0;
  for (int j = 0; j < M; ++j) n += (long)N * C * (H >> j) * (W >> j);
  return n;
}

// floats of scratch for the levels 1 .. M - 1 (g_j in the forward, T_j in the backward)
extern "C" long p2p_lap_pyr(int N, int C, int H, int W, int M) {
  long n = 1;   // never empty
  for (int j = 1; j < M; ++j) n += (long)N * C * (H >> j) * (W >> j);
  return n;
}

// floats of forward workspace: one partial per workgroup of every level and 256 for the
// two-stage final sum
extern "C" long p2p_lap_ws(int N, int C, int H, int W, int M) {
  long n = 0;
  for (int j = 0; j < M; ++j)
    n += (long)N * C * (((H >> j) + p2p::LT_H - 1) / p2p::LT_H) * (((W >> j) + p2p::LT_W - 1) / p2p::LT_W);
  return n + 256;
}

// dtype: 0 = fp32, 1 = bf16.  strides[8] = (n, c, h, w) of x, then of y.  Writes the sign
// pyramid and loss[0]; pyr and ws are scratch.
extern "C" int p2p_lap_fwd(const void* x, const void* y, int dtype, const long* strides, int N, int C, int H, int W,
                           int M, float* pyr, signed char* signs, float* ws, float* loss, hipStream_t st) {
  using namespace p2p;
  if (!lap_shape_ok(N, C, H, W, M)) return -1;
  LapArgs m{};
  m.N = N; m.C = C;
  m.x = x; m.y = y;
  m.xs = strides4(strides); m.ys = strides4(strides + 4);
  long woff = 0;
  for (int j = 0; j < M; ++j) {
    const int h = H >> j, w = W >> j;
    lap_tiles(m, N, C, h, w);
    m.ws = ws + woff;
    m.sign = signs;
    m.next = pyr;
    if (j == M - 1) lap_launch_fwd<true>(dtype, j == 0, m, st);
    else lap_launch_fwd<false>(dtype, j == 0, m, st);
    woff += (long)N * C * m.tiles_h * m.tiles_w;
    signs += (long)N * C * h * w;
    // the next level reads what this one filtered
    m.x = pyr; m.y = nullptr;
    m.xs = m.ys = lap_dense(C, h >> 1, w >> 1);
    pyr += (long)N * C * (h >> 1) * (w >> 1);
  }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  return p2p_sum_fixed(ws, woff, 1.f, loss, st);
}

// strides[4] = (n, c, h, w) of dx (and dy).  dx = gout dL/dx, dy = -dx or null.  tmp: the
// p2p_lap_pyr floats for T_j, j >= 1.
extern "C" int p2p_lap_bwd(const signed char* signs, const float* gout, int dtype, const long* strides, int N, int C,
                           int H, int W, int M, float* tmp, void* dx, void* dy, hipStream_t st) {
  using namespace p2p;
  if (!lap_shape_ok(N, C, H, W, M)) return -1;
  long soff[LAP_MAXM] = {0}, toff[LAP_MAXM] = {0};   // of s_j, and of T_j in tmp (j >= 1)
  for (int j = 1; j < M; ++j) {
    soff[j] = soff[j - 1] + (long)N * C * (H >> (j - 1)) * (W >> (j - 1));
    if (j >= 2) toff[j] = toff[j - 1] + (long)N * C * (H >> (j - 1)) * (W >> (j - 1));
  }
  LapArgs m{};
  m.N = N; m.C = C; m.gout = gout;
  for (int j = M - 1; j >= 0; --j) {
    const int h = H >> j, w = W >> j;
    lap_tiles(m, N, C, h, w);
    m.sign = const_cast<signed char*>(signs) + soff[j];
    const bool ut = j > 0, dt = j < M - 1;
    if (ut) {
      m.fine = signs + soff[j - 1];
      m.cf = (float)(1.0 / ((double)N * C * (2.0 * h) * (2.0 * w)));
    }
    if (dt) m.coarse = tmp + toff[j + 1];
    if (j > 0) {
      m.dx = tmp + toff[j]; m.dy = nullptr;
      m.ds = lap_dense(C, h, w);
      lap_launch_bwd<float, false>(ut, dt, m, st);
    } else {
      m.dx = dx; m.dy = dy;
      m.ds = strides4(strides);
      if (dtype == 1) lap_launch_bwd<bf16, true>(ut, dt, m, st);
      else lap_launch_bwd<float, true>(ut, dt, m, st);
    }
  }
  return (int)hipGetLastError();
}
