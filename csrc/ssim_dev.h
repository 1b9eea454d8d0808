// What ssim_loss.hip and ms_ssim_loss.hip share: the window, the per-origin SSIM / cs value and
// its derivatives, the staging of an image rectangle into LDS and the (K, dtype, last) launch
// switch.  The filter passes differ on purpose (profiles/ms_ssim_loss.md) and stay in the files.
#pragma once
#include "common.h"

#define P2P_SSIM_DEV __device__ __forceinline__ P2P_SCALAR_F32

namespace p2p {

constexpr int SSIM_MAXK = 11;

// element strides (n, c, h, w) of one image
struct Strides4 {
  long n, c, h, w;
};
inline Strides4 strides4(const long* s) { return {s[0], s[1], s[2], s[3]}; }

struct SsimWindow {
  float g[SSIM_MAXK];   // 1-D window taps (sum 1)
  float cov, c1, c2;
};

// window: 0 = uniform7, 1 = gauss11.  Returns K, or 0 for an unknown window.
inline int ssim_window(int window, double data_range, SsimWindow& m) {
  int K = 0;
  if (window == 0) {
    K = 7;
    for (int i = 0; i < K; ++i) m.g[i] = (float)(1.0 / 7.0);
    m.cov = (float)(49.0 / 48.0);
  } else if (window == 1) {
    K = 11;
    double g[11], sum = 0.0;
    for (int i = 0; i < K; ++i) sum += g[i] = exp(-(i - 5) * (i - 5) / (2.0 * 1.5 * 1.5));
    for (int i = 0; i < K; ++i) m.g[i] = (float)(g[i] / sum);
    m.cov = 1.f;
  }
  m.c1 = (float)((0.01 * data_range) * (0.01 * data_range));
  m.c2 = (float)((0.03 * data_range) * (0.03 * data_range));
  return K;
}

// window moments (m, n, E[xx], E[yy], E[xy]) -> S (LAST), or cs = A2 / B2
template <bool LAST>
P2P_SSIM_DEV float ssim_point(const float s[5], const SsimWindow& m) {
  const float ux = s[0], uy = s[1];
  const float vx = m.cov * (s[2] - ux * ux), vy = m.cov * (s[3] - uy * uy);
  const float vxy = m.cov * (s[4] - ux * uy);
  const float A2 = 2.f * vxy + m.c2, B2 = vx + vy + m.c2;
  if (!LAST) return A2 / B2;
  const float A1 = 2.f * ux * uy + m.c1, B1 = ux * ux + uy * uy + m.c1;
  return (A1 * A2) / (B1 * B2);
}

// ... -> (a, b, c) = d(S or cs) / d(E[x], E[xx], E[xy]), see the derivations in the two files
template <bool LAST>
P2P_SSIM_DEV void ssim_point_grad(const float s[5], const SsimWindow& m, float& a, float& b, float& c) {
  const float ux = s[0], uy = s[1], f = m.cov;
  const float vx = f * (s[2] - ux * ux), vy = f * (s[3] - uy * uy);
  const float vxy = f * (s[4] - ux * uy);
  const float A2 = 2.f * vxy + m.c2, B2 = vx + vy + m.c2;
  const float r2 = 1.f / B2;
  if (!LAST) {
    const float cs = A2 * r2;
    c = 2.f * f * r2;
    b = -f * cs * r2;
    a = 2.f * f * (ux * cs - uy) * r2;
  } else {
    const float A1 = 2.f * ux * uy + m.c1, B1 = ux * ux + uy * uy + m.c1;
    const float r1 = 1.f / B1, r12 = r1 * r2;
    const float S = A1 * A2 * r12;
    c = 2.f * f * A1 * r12;
    b = -f * S * r2;
    a = 2.f * uy * (A2 - f * A1) * r12 - 2.f * ux * S * (r1 - f * r2);
  }
}

// stage the IH x IW rectangle of x and y whose corner is (r0, c0) as fp32 rows of stride LS,
// zero outside the image.  A: SsimArgs or MsArgs (H, W and the strides xs, ys).
template <typename T, int IH, int IW, int LS, typename A>
P2P_SSIM_DEV void ssim_stage(const A& m, const T* X, const T* Y, int r0, int c0, float* lx, float* ly) {
  for (int e = threadIdx.x; e < IH * IW; e += 256) {
    const int i = e / IW, j = e % IW, r = r0 + i, c = c0 + j;
    float u = 0.f, v = 0.f;
    if (r >= 0 && r < m.H && c >= 0 && c < m.W) {
      u = (float)X[r * m.xs.h + c * m.xs.w];
      v = (float)Y[r * m.ys.h + c * m.ys.w];
    }
    const int o = LS == IW ? e : i * LS + j;   // dense rows: the compiler does not fold this itself
    lx[o] = u;
    ly[o] = v;
  }
}

// the N / C / grid-limit checks of a launch on the grid (tiles_w, C * tiles_h, N)
inline bool ssim_grid_ok(int N, int C, int tiles_h) {
  return N >= 1 && C >= 1 && N <= 65535 && (long)C * tiles_h <= 65535;
}

}  // namespace p2p

// Launch KERNEL<T, K ...> on the grid (tiles_w, C * tiles_h, N) the args m describe, for K in
// {7, 11} and dtype 0 = fp32 / 1 = bf16.  What follows st is appended to the template arguments:
// nothing for ssim_loss.hip's kernels, ", true" or ", false" (LAST) for ms_ssim_loss.hip's.  Only
// launches: the caller has checked the grid and reads hipGetLastError().
#define P2P_SSIM_LAUNCH(KERNEL, K, dtype, m, st, ...)                                                   \
  do {                                                                                                  \
    const dim3 grid_((m).tiles_w, (m).C * (m).tiles_h, (m).N), block_(256);                             \
    if ((K) == 7 && (dtype) == 1) hipLaunchKernelGGL((KERNEL<bf16, 7 __VA_ARGS__>), grid_, block_, 0, st, m);   \
    else if ((K) == 7) hipLaunchKernelGGL((KERNEL<float, 7 __VA_ARGS__>), grid_, block_, 0, st, m);             \
    else if ((dtype) == 1) hipLaunchKernelGGL((KERNEL<bf16, 11 __VA_ARGS__>), grid_, block_, 0, st, m);         \
    else hipLaunchKernelGGL((KERNEL<float, 11 __VA_ARGS__>), grid_, block_, 0, st, m);                          \
  } while (0)
