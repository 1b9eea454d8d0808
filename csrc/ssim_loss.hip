// Differentiable SSIM loss on the device (gfx950): loss = 1 - mean SSIM(x, y), forward and
// a fused backward, for the two separable windows "uniform7" (7x7 box, sample covariance
// 49/48 -- the window of the metric in metrics.hip) and "gauss11" (11x11, sigma 1.5, Wang
// et al.).  Unlike metrics.hip this is the CONTINUOUS SSIM of the model-range values as
// they are (no clamp, no uint8 levels: those have zero gradient); fp32 math throughout.
//
// Per valid window origin, with E[.] the window-weighted mean and f the covariance factor:
//   m = E[x], n = E[y], vx = f (E[xx] - m^2), vy = f (E[yy] - n^2), vxy = f (E[xy] - m n)
//   A1 = 2 m n + C1, A2 = 2 vxy + C2, B1 = m^2 + n^2 + C1, B2 = vx + vy + C2
//   S  = A1 A2 / (B1 B2)
// Derivatives with respect to the three moments x enters (E[y], E[yy] held fixed):
//   c = dS/dE[xy] = 2 f A1 / (B1 B2)
//   b = dS/dE[xx] = -f S / B2
//   a = dS/dm     = 2 n (A2 - f A1) / (B1 B2) - 2 m S (1 / B1 - f / B2)
//       (dA1/dm = 2 n, dA2/dm = -2 f n, dB1/dm = 2 m, dB2/dm = -2 f m)
// and, since dE[x]/dx(p) = w, dE[xx]/dx(p) = 2 x(p) w, dE[xy]/dx(p) = y(p) w,
//   dL/dx(p) = -gout / count * ( W*(a)(p) + 2 x(p) W*(b)(p) + y(p) W*(c)(p) )
// with W* the adjoint of the valid window filter.  S is symmetric in (x, y): the gradient of
// y is the same kernel with the two images swapped.
//
// Forward: one workgroup = 16 x 64 window origins of one (n, c).  It stages the x and y
// rectangle plus the K-1 halo into LDS as fp32 (strided reads: NHWC bf16, channel-padded
// and NCHW fp32 inputs all work in place), filters the five moments x, y, xx, yy, xy
// horizontally into LDS planes, vertically into registers, and reduces 1 - S by wave
// shuffle and LDS to one partial per workgroup; the partials are summed in a fixed order
// (bitwise reproducible, no atomics).
//
// Backward: one workgroup = 16 x 32 input pixels.  Nothing per-origin is ever written to
// HBM: the workgroup stages x and y with a 2(K-1) halo, recomputes the moments of the
// (16+K-1) x (32+K-1) origins whose windows touch its pixels, evaluates a, b, c there
// (zero at origins that are not valid windows), applies the transposed separable filter
// through LDS (the horizontal pass reuses the moment planes) and writes dx in the
// gradient's dtype and layout.  gout is read on the device.
//
// Every LDS plane is dense with the row stride of the pass that reads it column-wise, so
// the lanes of a wave (consecutive columns) hit consecutive banks in the vertical passes.
#include "ssim_dev.h"

namespace p2p {

constexpr int SF_H = 16, SF_W = 64;   // forward tile (window origins)
constexpr int SB_H = 16, SB_W = 32;   // backward tile (input pixels)
constexpr int SL_LDS_LIMIT = 64 * 1024;

struct SsimArgs {
  const void* x;
  const void* y;
  void* dx;
  Strides4 xs, ys, ds;    // of x, y and dx
  int N, C, H, W, tiles_h, tiles_w;
  SsimWindow w;
  float inv_count;
  float* ws;              // forward: one partial per workgroup
  const float* gout;      // backward: dL/dloss on the device
};

// horizontal K-tap filter of the five moments: staged [IH][OW + K - 1] -> hm[5][IH][OW]
template <int K, int IH, int OW>
__device__ __forceinline__ void ssim_hpass(const SsimArgs& m, const float* lx, const float* ly, float* hm) {
  constexpr int IW = OW + K - 1;
  for (int e = threadIdx.x; e < IH * OW; e += 256) {
    const int i = e / OW, j = e % OW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const float u = lx[i * IW + j + t], v = ly[i * IW + j + t], w = m.w.g[t];
      const float wu = w * u, wv = w * v;
      s0 += wu; s1 += wv; s2 += wu * u; s3 += wv * v; s4 += wu * v;
    }
    hm[0 * IH * OW + e] = s0; hm[1 * IH * OW + e] = s1; hm[2 * IH * OW + e] = s2;
    hm[3 * IH * OW + e] = s3; hm[4 * IH * OW + e] = s4;
  }
}

// vertical K-tap filter at origin (i, j) of the planes hm[5][IH][OW]
template <int K, int IH, int OW>
__device__ __forceinline__ void ssim_vpass(const SsimArgs& m, const float* hm, int i, int j, float s[5]) {
#pragma unroll
  for (int q = 0; q < 5; ++q) s[q] = 0.f;
#pragma unroll
  for (int t = 0; t < K; ++t)
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] += m.w.g[t] * hm[q * IH * OW + (i + t) * OW + j];
}

template <typename T, int K>
__global__ void P2P_SCALAR_F32 __launch_bounds__(256) ssim_loss_fwd_kernel(SsimArgs m) {
  constexpr int IH = SF_H + K - 1, IW = SF_W + K - 1;
  __shared__ float lx[IH * IW], ly[IH * IW];
  __shared__ float hm[5 * IH * SF_W];
  __shared__ float red[4];
  static_assert(sizeof(float) * (2 * IH * IW + 5 * IH * SF_W + 4) <= SL_LDS_LIMIT, "forward LDS footprint");
  const int tid = threadIdx.x;
  const int n = blockIdx.z, c = blockIdx.y / m.tiles_h, ty = blockIdx.y % m.tiles_h;
  const int r0 = ty * SF_H, c0 = blockIdx.x * SF_W;
  const T* X = static_cast<const T*>(m.x) + n * m.xs.n + c * m.xs.c;
  const T* Y = static_cast<const T*>(m.y) + n * m.ys.n + c * m.ys.c;

  ssim_stage<T, IH, IW, IW>(m, X, Y, r0, c0, lx, ly);
  __syncthreads();
  // (halo columns / rows past the image are zeros and only feed origins that are not valid)
  ssim_hpass<K, IH, SF_W>(m, lx, ly, hm);
  __syncthreads();
  float acc = 0.f;
  for (int e = tid; e < SF_H * SF_W; e += 256) {
    const int i = e / SF_W, j = e % SF_W;
    if (r0 + i > m.H - K || c0 + j > m.W - K) continue;
    float s[5];
    ssim_vpass<K, IH, SF_W>(m, hm, i, j, s);
    acc += 1.f - ssim_point<true>(s, m.w);
  }
  acc = warp_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const long blk = (((long)n * m.C + c) * m.tiles_h + ty) * m.tiles_w + blockIdx.x;
    m.ws[blk] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

template <typename T, int K>
__global__ void P2P_SCALAR_F32 __launch_bounds__(256) ssim_loss_bwd_kernel(SsimArgs m) {
  constexpr int R = K - 1;
  constexpr int OH = SB_H + R, OW = SB_W + R;   // origins whose windows touch the tile
  constexpr int IH = OH + R, IW = OW + R;       // inputs those origins read
  __shared__ float lx[IH * IW], ly[IH * IW];
  __shared__ float hm[5 * IH * OW];             // moment planes, then th[3][OH][SB_W]
  __shared__ float cf[3 * OH * OW];             // a, b, c per origin
  static_assert(sizeof(float) * (2 * IH * IW + 5 * IH * OW + 3 * OH * OW) <= SL_LDS_LIMIT,
                "backward LDS footprint");
  static_assert(3 * OH * SB_W <= 5 * IH * OW, "transposed-filter planes reuse the moment planes");
  const int tid = threadIdx.x;
  const int n = blockIdx.z, c = blockIdx.y / m.tiles_h, ty = blockIdx.y % m.tiles_h;
  const int p0r = ty * SB_H, p0c = blockIdx.x * SB_W;   // first pixel of the tile
  const int br = p0r - R, bc = p0c - R;                 // first origin == first staged input
  const T* X = static_cast<const T*>(m.x) + n * m.xs.n + c * m.xs.c;
  const T* Y = static_cast<const T*>(m.y) + n * m.ys.n + c * m.ys.c;

  ssim_stage<T, IH, IW, IW>(m, X, Y, br, bc, lx, ly);
  __syncthreads();
  ssim_hpass<K, IH, OW>(m, lx, ly, hm);
  __syncthreads();
  for (int e = tid; e < OH * OW; e += 256) {
    const int i = e / OW, j = e % OW, gr = br + i, gc = bc + j;
    float a = 0.f, b = 0.f, cc = 0.f;
    if (gr >= 0 && gr <= m.H - K && gc >= 0 && gc <= m.W - K) {
      float s[5];
      ssim_vpass<K, IH, OW>(m, hm, i, j, s);
      ssim_point_grad<true>(s, m.w, a, b, cc);
    }
    cf[0 * OH * OW + e] = a; cf[1 * OH * OW + e] = b; cf[2 * OH * OW + e] = cc;
  }
  __syncthreads();
  // transposed filter, horizontal: pixel column pj takes origin column pj + R - t with tap t
  float* th = hm;
  for (int e = tid; e < OH * SB_W; e += 256) {
    const int i = e / SB_W, pj = e % SB_W;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const int o = i * OW + pj + R - t;
      const float w = m.w.g[t];
      s0 += w * cf[0 * OH * OW + o]; s1 += w * cf[1 * OH * OW + o]; s2 += w * cf[2 * OH * OW + o];
    }
    th[0 * OH * SB_W + e] = s0; th[1 * OH * SB_W + e] = s1; th[2 * OH * SB_W + e] = s2;
  }
  __syncthreads();
  // ... vertical, then dx = scale (A + 2 x B + y C)
  const float scale = -m.gout[0] * m.inv_count;
  T* D = static_cast<T*>(m.dx) + n * m.ds.n + c * m.ds.c;
  for (int e = tid; e < SB_H * SB_W; e += 256) {
    const int pi = e / SB_W, pj = e % SB_W, r = p0r + pi, col = p0c + pj;
    if (r >= m.H || col >= m.W) continue;
    float A = 0.f, B = 0.f, Cc = 0.f;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const int o = (pi + R - t) * SB_W + pj;
      const float w = m.w.g[t];
      A += w * th[0 * OH * SB_W + o]; B += w * th[1 * OH * SB_W + o]; Cc += w * th[2 * OH * SB_W + o];
    }
    const float xv = lx[(pi + R) * IW + pj + R], yv = ly[(pi + R) * IW + pj + R];
    D[r * m.ds.h + col * m.ds.w] = (T)(scale * (A + 2.f * xv * B + yv * Cc));
  }
}

}  // namespace p2p

// floats of forward workspace: one partial per workgroup + 256 for the two-stage final sum
extern "C" long p2p_ssim_loss_ws(int N, int C, int H, int W, int window) {
  const int K = window == 1 ? 11 : 7;
  if (H < K || W < K) return 0;
  const long th = (H - K + p2p::SF_H) / p2p::SF_H, tw = (W - K + p2p::SF_W) / p2p::SF_W;
  return (long)N * C * th * tw + 256;
}

// dtype: 0 = fp32, 1 = bf16.  strides[8] = (n, c, h, w) of x, then of y.  out[0] = the loss.
extern "C" int p2p_ssim_loss_fwd(const void* x, const void* y, int dtype, const long* strides, int N, int C, int H,
                                 int W, int window, double data_range, float* ws, float* out, hipStream_t st) {
  using namespace p2p;
  SsimArgs m{};
  const int K = ssim_window(window, data_range, m.w);
  if (K == 0 || H < K || W < K) return -1;
  m.x = x; m.y = y;
  m.xs = strides4(strides); m.ys = strides4(strides + 4);
  m.N = N; m.C = C; m.H = H; m.W = W;
  m.tiles_h = (H - K + SF_H) / SF_H;
  m.tiles_w = (W - K + SF_W) / SF_W;
  m.ws = ws;
  if (!ssim_grid_ok(N, C, m.tiles_h)) return -1;
  P2P_SSIM_LAUNCH(ssim_loss_fwd_kernel, K, dtype, m, st, );
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const float scale = (float)(1.0 / ((double)N * C * (H - K + 1) * (W - K + 1)));
  return p2p_sum_fixed(ws, (long)N * C * m.tiles_h * m.tiles_w, scale, out, st);
}

// strides[12] = (n, c, h, w) of x, of y, then of dx.  dx = dL/dx; swap x and y for dL/dy.
extern "C" int p2p_ssim_loss_bwd(const void* x, const void* y, int dtype, const long* strides, int N, int C, int H,
                                 int W, int window, double data_range, const float* gout, void* dx,
                                 hipStream_t st) {
  using namespace p2p;
  SsimArgs m{};
  const int K = ssim_window(window, data_range, m.w);
  if (K == 0 || H < K || W < K) return -1;
  m.x = x; m.y = y; m.dx = dx;
  m.xs = strides4(strides); m.ys = strides4(strides + 4); m.ds = strides4(strides + 8);
  m.N = N; m.C = C; m.H = H; m.W = W;
  m.tiles_h = (H + SB_H - 1) / SB_H;
  m.tiles_w = (W + SB_W - 1) / SB_W;
  m.inv_count = (float)(1.0 / ((double)N * C * (H - K + 1) * (W - K + 1)));
  m.gout = gout;
  if (!ssim_grid_ok(N, C, m.tiles_h)) return -1;
  P2P_SSIM_LAUNCH(ssim_loss_bwd_kernel, K, dtype, m, st, );
  return (int)hipGetLastError();
}
