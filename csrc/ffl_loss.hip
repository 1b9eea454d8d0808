// Focal frequency loss on the device (gfx950), Jiang et al., ICCV 2021:
//   d = x - y,  F = DFT2_ortho(d) per (n, c),  w = |F|^alpha / max_{u,v} |F|^alpha  (a constant),
//   loss = mean_{n,c,u,v} w |F|^2,   dL/dx = gout 2 / (N C H W) Re(IDFT2_ortho(w . F)),  dL/dy = -dL/dx
// (w = 0 on a plane whose spectrum is all zero).  A 2-D DFT of an H x W plane is two dense
// matrix products against twiddle matrices; all four transforms (two forward, two inverse) run
// on v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation.  Plain vector stores, no atomics,
// no host read of anything on the device, so the op can be captured into a graph once the
// twiddle matrices of its sizes exist (the first call of a size builds them on the host).
//
// d is real, so F is Hermitian and only the columns v in [0, W/2] (Wh = W/2 + 1 of them) are
// computed, stored and saved; columns 1 .. W/2 - 1 count twice, mult(v), in the loss sum and
// in the inverse row transform.
//
// Five launches.  "Tile" is the 32 x 32 output of one MFMA accumulator; one WAVE owns one tile
// and a workgroup is as many waves as its strip has tiles (1 .. 16), so H and W only need to
// be multiples of 32 (96 gives 3 waves) and the waves of a workgroup finish together.
//
//  1 row pass     workgroup = 32 rows of one plane.  Stages d = x - y (through the input
//                 strides, fp32) TRANSPOSED in LDS, [w][row], and multiplies by the W x Wh
//                 twiddle columns: wave t makes columns 32 t .. 32 t + 31 of Z = d (C - iS),
//                 two MFMAs per k-step that share the A fragment.  Z: [plane][re, im][H][Wh].
//  2 column pass  workgroup = 32 columns v of one plane.  Stages Z[:, strip] (re and im) in
//                 LDS and wave t makes rows u = 32 t .. 32 t + 31 of F = (C - iS) Z: four MFMAs
//                 per k-step over two A (twiddle) and two B (LDS) fragments.  From the
//                 accumulators: F (saved for the backward, same layout as Z), and per workgroup
//                 one partial sum of mult(v) |F|^(2 + alpha) and one partial max of |F|^2.
//  3 finalize     one thread per plane sums its partials in a fixed order (double):
//                 term = S / max^alpha and inv = 1 / max^alpha (both 0 where max = 0); the
//                 project's fixed-order sum makes the scalar.  One pass gives the sum and the
//                 max because w is |F|^alpha over a per-plane scalar.
//  4 inverse column pass   as 2 with conjugate twiddles; its prologue forms
//                 G = (2 gout / count) inv[plane] |F|^alpha F on the way into LDS.  Writes Y.
//  5 inverse row pass      as 1 with K = the half spectrum: stages mult(v) Y (im negated)
//                 transposed and makes dx[r, w] = sum_v mult(v) (yr cos - yi sin); wave t owns
//                 columns 32 t .. of the FULL width.  Stores dx in x's dtype and layout and,
//                 when asked, dy = -dx in the same loop.
//
// Twiddles: a MATERIALISED n x n matrix pair per length, C[k][j] = cos(2 pi (k j mod n) / n) /
// sqrt(n) and S likewise, built on the host in float64 from one n-entry table with the phase
// reduced as an integer (never sinf of a large product; exact zeros and symmetries), and read
// through L2 like a weight image.  Why not an n-entry LDS table: the MFMA operand of lane l is
// element [k0 + l / 32][j0 + l % 32], which in the matrix is two coalesced 128-byte row
// segments per load, while a table would need (k j) mod n per lane and a bank-conflicted LDS
// gather per operand.  The matrix is symmetric, which is what makes the column passes' A
// operand ([u][h], lanes along u) the same coalesced row read.  512 x 512 x 2 is 2 MB: L2.
//
// Ragged half spectrum: Wh is no tile multiple.  The COMPUTE grid is padded to WP = Wh rounded
// up to 32 (WP <= W, so the padded columns index real twiddles and nothing is read out of
// bounds); the MEMORY layouts of Z, F and Y stay compact at Wh columns: stores of v >= Wh are
// dropped and loads of v >= Wh stage zeros.  The saved F is therefore H x Wh complex, about
// 4 bytes per pixel.  The inverse row pass pads its K (= Wh, odd) to W/2 + 8 with zero rows
// (every K is then a multiple of 8: the k loop is unrolled 4 steps of 2 without a remainder).
//
// LDS (dynamic, checked against 160 KB for n = 512 below): pass 1 W x 33 floats (66 KB at
// 512), passes 2 / 4 2 x H x 32 floats (128 KB at 512, 64 KB at 256), pass 5 2 x (W/2 + 8) x 33
// floats (68 KB at 512, 35 KB at 256).  The transposed strips have the odd stride 33 so the
// staging writes (lanes along w) and the fragment reads (lanes along the row) are both
// conflict-free within each half wave; the column strips are read as 64 consecutive words.
#include "common.h"   // P2P_SCALAR_F32: no packed fp32 arithmetic in these kernels

namespace p2p {

typedef float ffl_f32x16 __attribute__((ext_vector_type(16)));

constexpr int FFL_T = 32;                  // tile side == rows / columns per strip
constexpr int FFL_LS = FFL_T + 1;          // stride of the transposed strips
constexpr int FFL_MIN = 32, FFL_MAX = 512;
constexpr int FFL_LDS_LIMIT = 160 * 1024;

constexpr int ffl_wh(int W) { return W / 2 + 1; }
constexpr int ffl_wp(int W) { return (ffl_wh(W) + FFL_T - 1) / FFL_T * FFL_T; }
constexpr int FFL_KU = 4;                 // k-steps (of 2) per unrolled block: K is a multiple of 8
constexpr int ffl_kp(int W) { return W / 2 + 2 * FFL_KU; }   // pass 5: K = Wh padded with zero rows
constexpr int ffl_lds_row_fwd(int W) { return W * FFL_LS * 4; }
constexpr int ffl_lds_col(int H) { return 2 * H * FFL_T * 4; }
constexpr int ffl_lds_row_inv(int W) { return 2 * ffl_kp(W) * FFL_LS * 4; }
static_assert(ffl_lds_row_fwd(FFL_MAX) <= FFL_LDS_LIMIT && ffl_lds_col(FFL_MAX) + 64 <= FFL_LDS_LIMIT &&
                  ffl_lds_row_inv(FFL_MAX) <= FFL_LDS_LIMIT,
              "LDS budget at n = 512");
static_assert(ffl_wp(FFL_MIN) <= FFL_MIN && ffl_wp(64) <= 64 && ffl_wp(FFL_MAX) <= FFL_MAX &&
                  ffl_kp(FFL_MIN) <= FFL_MIN,
              "padded tiles stay inside the n x n twiddle matrix");

struct FflArgs {
  const void* x;            // pass 1
  const void* y;
  long xn, xc, xh, xw;      // element strides (n, c, h, w) of x
  long yn, yc, yh, yw;      // ... of y
  void* dx;                 // pass 5 (dy may be null)
  void* dy;
  long dn, dc, dh, dw;
  long en, ec, eh, ew;
  int C, H, W, Wh;
  const float* twh;         // [2][H][H]: cos then sin, 1 / sqrt(H) folded in
  const float* tww;         // [2][W][W]
  const float* src;         // half spectrum read by this pass:    [plane][2][H][Wh]
  float* dst;               // ... written
  float* part;              // pass 2: [plane][strips][2] = (sum, max)
  const float* inv;         // pass 4: [plane]
  const float* gout;        // pass 4: dL/dloss on the device
  float alpha, gscale;      // gscale = 2 / (N C H W)
};

// p^(alpha / 2) for p = |F|^2 >= 0: the focal weight up to the per-plane scale.  alpha 0, 1
// and 2 avoid powf (exact, sqrt, exact).
__device__ __forceinline__ P2P_SCALAR_F32 float ffl_weight(float p, float alpha) {
  if (alpha == 0.f) return 1.f;
  if (alpha == 1.f) return sqrtf(p);
  if (alpha == 2.f) return p;
  return p > 0.f ? powf(p, 0.5f * alpha) : 0.f;
}

// row of accumulator register r in the 32 x 32 tile (its column is lane % 32)
__device__ __forceinline__ int ffl_acc_row(int r, int lane) { return (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3); }

#define FFL_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0)

// Passes 1 and 5.  One workgroup = rows r0 .. r0 + 31 of one plane; wave t = output columns
// 32 t ...  A (the strip, k-major in LDS) x B (twiddle rows from global memory).
template <typename T, bool INV>
__global__ void P2P_SCALAR_F32 __launch_bounds__(1024) ffl_row_kernel(FflArgs m) {
  extern __shared__ float ffl_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int strips = m.H / FFL_T;
  const int plane = blockIdx.x / strips, r0 = (blockIdx.x % strips) * FFL_T;
  const int n = plane / m.C, c = plane % m.C;
  const int W = m.W, Wh = m.Wh;
  const long half = (long)m.H * Wh;
  const int K = INV ? W / 2 + 2 * FFL_KU : W;
  float* a0 = ffl_lds;                      // fwd: d;  inv: mult * yr
  float* a1 = ffl_lds + (long)K * FFL_LS;   //          inv: -mult * yi

  if (!INV) {
    const T* X = static_cast<const T*>(m.x) + n * m.xn + c * m.xc;
    const T* Y = static_cast<const T*>(m.y) + n * m.yn + c * m.yc;
    for (int e = tid; e < FFL_T * W; e += blockDim.x) {
      const int i = e / W, w = e % W, r = r0 + i;
      a0[w * FFL_LS + i] = (float)X[r * m.xh + w * m.xw] - (float)Y[r * m.yh + w * m.yw];
    }
  } else {
    const float* S = m.src + (long)plane * 2 * half;
    for (int e = tid; e < FFL_T * K; e += blockDim.x) {
      const int i = e / K, v = e % K;
      float yr = 0.f, yi = 0.f;
      if (v < Wh) {
        const float mult = (v == 0 || v == Wh - 1) ? 1.f : 2.f;
        const long o = (long)(r0 + i) * Wh + v;
        yr = mult * S[o];
        yi = -mult * S[half + o];
      }
      a0[v * FFL_LS + i] = yr;
      a1[v * FFL_LS + i] = yi;
    }
  }
  __syncthreads();

  const int col = wave * FFL_T + (lane & 31);          // < WP <= W (fwd), < W (inv)
  const float* Bc = m.tww + (long)(lane >> 5) * W + col;
  const float* Bs = Bc + (long)W * W;
  const int ao = (lane >> 5) * FFL_LS + (lane & 31);
  ffl_f32x16 acc0 = {0}, acc1 = {0};
  for (int k0 = 0; k0 < K; k0 += 2 * FFL_KU) {
#pragma unroll
    for (int s = 0; s < FFL_KU; ++s) {
      const int k = k0 + 2 * s;
      const float bc = Bc[(long)k * W], bs = Bs[(long)k * W];
      const float u = a0[k * FFL_LS + ao];
      acc0 = FFL_MFMA(u, bc, acc0);
      if (!INV) acc1 = FFL_MFMA(u, bs, acc1);
      else acc0 = FFL_MFMA(a1[k * FFL_LS + ao], bs, acc0);
    }
  }

  if (!INV) {
    if (col >= Wh) return;
    float* Z = m.dst + (long)plane * 2 * half;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long o = (long)(r0 + ffl_acc_row(r, lane)) * Wh + col;
      Z[o] = acc0[r];
      Z[half + o] = -acc1[r];
    }
  } else {
    T* D = static_cast<T*>(m.dx) + n * m.dn + c * m.dc;
    T* E = m.dy ? static_cast<T*>(m.dy) + n * m.en + c * m.ec : nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + ffl_acc_row(r, lane);
      D[row * m.dh + col * m.dw] = (T)acc0[r];
      if (E) E[row * m.eh + col * m.ew] = (T)(-acc0[r]);
    }
  }
}

// Passes 2 and 4.  One workgroup = columns v0 .. v0 + 31 of one plane's half spectrum; wave t
// = output rows 32 t ...  A (twiddle, read as rows of the symmetric matrix) x B (the strip).
// out = (C -+ iS) in:  re = C re +- S im,  im = C im -+ S re  (upper sign: forward).
template <bool INV>
__global__ void P2P_SCALAR_F32 __launch_bounds__(1024) ffl_col_kernel(FflArgs m) {
  extern __shared__ float ffl_lds[];
  __shared__ float red[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = m.H, Wh = m.Wh;
  const int strips = (Wh + FFL_T - 1) / FFL_T;
  const int plane = blockIdx.x / strips, strip = blockIdx.x % strips, v0 = strip * FFL_T;
  const long half = (long)H * Wh;
  const float* S = m.src + (long)plane * 2 * half;
  float* br = ffl_lds;
  float* bi = ffl_lds + H * FFL_T;

  const float coef = INV ? m.gscale * m.gout[0] * m.inv[plane] : 1.f;
  for (int e = tid; e < H * FFL_T; e += blockDim.x) {
    const int h = e >> 5, v = v0 + (e & 31);
    float re = 0.f, im = 0.f;
    if (v < Wh) {
      re = S[(long)h * Wh + v];
      im = S[half + (long)h * Wh + v];
      if (INV) {
        const float g = coef * ffl_weight(re * re + im * im, m.alpha);
        re *= g;
        im *= g;
      }
    }
    br[e] = re;
    bi[e] = im;
  }
  __syncthreads();

  const float* Ac = m.twh + (long)(lane >> 5) * H + wave * FFL_T + (lane & 31);
  const float* As = Ac + (long)H * H;
  ffl_f32x16 accr = {0}, acci = {0};
  for (int k0 = 0; k0 < H; k0 += 2 * FFL_KU) {
#pragma unroll
    for (int s = 0; s < FFL_KU; ++s) {
      const int k = k0 + 2 * s;
      const float ac = Ac[(long)k * H];
      const float as = INV ? -As[(long)k * H] : As[(long)k * H];
      const float zr = br[k * FFL_T + lane], zi = bi[k * FFL_T + lane];
      accr = FFL_MFMA(ac, zr, accr);
      accr = FFL_MFMA(as, zi, accr);
      acci = FFL_MFMA(ac, zi, acci);
      acci = FFL_MFMA(-as, zr, acci);
    }
  }

  const int v = v0 + (lane & 31);
  float* D = m.dst + (long)plane * 2 * half;
  float sum = 0.f, mx = 0.f;
  if (v < Wh) {
    const float mult = (v == 0 || v == Wh - 1) ? 1.f : 2.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long o = (long)(wave * FFL_T + ffl_acc_row(r, lane)) * Wh + v;
      D[o] = accr[r];
      D[half + o] = acci[r];
      if (!INV) {
        const float p = accr[r] * accr[r] + acci[r] * acci[r];
        sum += mult * p * ffl_weight(p, m.alpha);
        mx = fmaxf(mx, p);
      }
    }
  }
  if constexpr (!INV) {
    sum = warp_sum(sum);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) { red[0][wave] = sum; red[1][wave] = mx; }
    __syncthreads();
    if (tid == 0) {
      const int waves = blockDim.x >> 6;
      float s = 0.f, q = 0.f;
      for (int i = 0; i < waves; ++i) { s += red[0][i]; q = fmaxf(q, red[1][i]); }
      m.part[2 * (long)blockIdx.x] = s;
      m.part[2 * (long)blockIdx.x + 1] = q;
    }
  }
}

// one thread per plane: term = S / max^alpha, inv = 1 / max^alpha with max = max |F| (part
// holds max |F|^2), both 0 on an all-zero spectrum
__global__ void __launch_bounds__(256) ffl_finalize_kernel(const float* part, int planes, int strips, double alpha,
                                                           float* term, float* inv) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= planes) return;
  double s = 0.0, mx = 0.0;
  for (int i = 0; i < strips; ++i) {
    s += (double)part[2 * ((long)p * strips + i)];
    mx = fmax(mx, (double)part[2 * ((long)p * strips + i) + 1]);
  }
  const double den = alpha == 0.0 ? 1.0 : pow(mx, 0.5 * alpha);
  term[p] = mx > 0.0 ? (float)(s / den) : 0.f;
  inv[p] = mx > 0.0 ? (float)(1.0 / den) : 0.f;
}

static bool ffl_shape_ok(int N, int C, int H, int W) {
  auto ok = [](int n) { return n >= FFL_MIN && n <= FFL_MAX && n % FFL_T == 0; };
  return N >= 1 && C >= 1 && ok(H) && ok(W) && (long)N * C * (FFL_MAX / FFL_T) < (1L << 31);
}

template <typename K>
static void ffl_go(K kernel, long blocks, int waves, int lds, int lds_max, std::atomic<uint64_t>& mask,
                   const FflArgs& m, hipStream_t st) {
  smem_attr_once(reinterpret_cast<const void*>(kernel), lds_max, mask);   // the kernel's need at n = 512
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * waves), lds, st, m);
}

}  // namespace p2p

// floats of one half spectrum (Z, F or Y): [N * C][2][H][W / 2 + 1]
extern "C" long p2p_ffl_spec(int N, int C, int H, int W) { return 2L * N * C * H * p2p::ffl_wh(W); }

// floats of forward workspace: the (sum, max) partials, the N * C terms and 256 for the
// two-stage final sum
extern "C" long p2p_ffl_ws(int N, int C, int H, int W) {
  return 2L * N * C * (p2p::ffl_wp(W) / p2p::FFL_T) + (long)N * C + 256;
}

// dtype: 0 = fp32, 1 = bf16.  strides[8] = (n, c, h, w) of x, then of y.  twh / tww: the
// [2][n][n] twiddle matrices of H and W.  z: scratch, f: the saved spectrum (p2p_ffl_spec
// floats each).  Writes f, inv[N * C] and loss[0].
extern "C" int p2p_ffl_fwd(const void* x, const void* y, int dtype, const long* strides, int N, int C, int H, int W,
                           double alpha, const float* twh, const float* tww, float* z, float* f, float* ws,
                           float* inv, float* loss, hipStream_t st) {
  using namespace p2p;
  if (!ffl_shape_ok(N, C, H, W)) return -1;
  static std::atomic<uint64_t> mask_rf{0}, mask_rb{0}, mask_c{0};
  const long planes = (long)N * C;
  const int strips = ffl_wp(W) / FFL_T;
  FflArgs m{};
  m.x = x; m.y = y;
  m.xn = strides[0]; m.xc = strides[1]; m.xh = strides[2]; m.xw = strides[3];
  m.yn = strides[4]; m.yc = strides[5]; m.yh = strides[6]; m.yw = strides[7];
  m.C = C; m.H = H; m.W = W; m.Wh = ffl_wh(W);
  m.twh = twh; m.tww = tww; m.alpha = (float)alpha;
  m.dst = z;
  const long rows = planes * (H / FFL_T);
  const int lr = ffl_lds_row_fwd(W), lr_max = ffl_lds_row_fwd(FFL_MAX);
  if (dtype == 1) ffl_go(ffl_row_kernel<bf16, false>, rows, strips, lr, lr_max, mask_rb, m, st);
  else ffl_go(ffl_row_kernel<float, false>, rows, strips, lr, lr_max, mask_rf, m, st);
  m.src = z; m.dst = f; m.part = ws;
  ffl_go(ffl_col_kernel<false>, planes * strips, H / FFL_T, ffl_lds_col(H), ffl_lds_col(FFL_MAX), mask_c, m, st);
  float* term = ws + 2 * planes * strips;
  hipLaunchKernelGGL(ffl_finalize_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, st, ws, (int)planes,
                     strips, alpha, term, inv);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const float scale = (float)(1.0 / ((double)planes * H * W));
  return p2p_sum_fixed(term, planes, scale, loss, st);
}

// strides[8] = (n, c, h, w) of dx, then of dy (dy may be null: only dx is written).
// f, inv: of the forward; ysc: scratch of p2p_ffl_spec floats; gout: dL/dloss on the device.
extern "C" int p2p_ffl_bwd(const float* f, const float* inv, const float* gout, int dtype, const long* strides, int N,
                           int C, int H, int W, double alpha, const float* twh, const float* tww, float* ysc,
                           void* dx, void* dy, hipStream_t st) {
  using namespace p2p;
  if (!ffl_shape_ok(N, C, H, W)) return -1;
  static std::atomic<uint64_t> mask_rf{0}, mask_rb{0}, mask_c{0};
  const long planes = (long)N * C;
  FflArgs m{};
  m.dx = dx; m.dy = dy;
  m.dn = strides[0]; m.dc = strides[1]; m.dh = strides[2]; m.dw = strides[3];
  m.en = strides[4]; m.ec = strides[5]; m.eh = strides[6]; m.ew = strides[7];
  m.C = C; m.H = H; m.W = W; m.Wh = ffl_wh(W);
  m.twh = twh; m.tww = tww; m.alpha = (float)alpha;
  m.gscale = (float)(2.0 / ((double)planes * H * W));
  m.inv = inv; m.gout = gout;
  m.src = f; m.dst = ysc;
  const long cols = planes * (ffl_wp(W) / FFL_T), rows = planes * (H / FFL_T);
  ffl_go(ffl_col_kernel<true>, cols, H / FFL_T, ffl_lds_col(H), ffl_lds_col(FFL_MAX), mask_c, m, st);
  m.src = ysc; m.dst = nullptr;
  const int lr = ffl_lds_row_inv(W), lr_max = ffl_lds_row_inv(FFL_MAX);
  if (dtype == 1) ffl_go(ffl_row_kernel<bf16, true>, rows, W / FFL_T, lr, lr_max, mask_rb, m, st);
  else ffl_go(ffl_row_kernel<float, true>, rows, W / FFL_T, lr, lr_max, mask_rf, m, st);
  return (int)hipGetLastError();
}

// The n x n twiddle pair of one length into out[2][n][n] (host): cos then sin of
// 2 pi (k j mod n) / n, scaled by 1 / sqrt(n).  One n-entry float64 table; the angle is reduced
// to the first quadrant with integers, so zeros and symmetries are exact.
extern "C" void p2p_ffl_twiddles(int n, float* out) {
  const double PI = 3.14159265358979323846, s = 1.0 / sqrt((double)n);
  double* tab = new double[2 * (size_t)n];
  for (int p = 0; p < n; ++p) {
    int q = p <= n - p ? p : n - p;                 // cos(t) = cos(2 pi - t);  q in [0, n / 2]
    double sc = 1.0, ss = p > n / 2 ? -1.0 : 1.0;   // sin(t) = -sin(2 pi - t)
    if (4 * q > n) { q = n / 2 - q; sc = -1.0; }    // cos(t) = -cos(pi - t), sin(t) = sin(pi - t)
    const double t = 2.0 * PI * q / n;              // in [0, pi / 2]
    tab[p] = 4 * q == n ? 0.0 : sc * cos(t) * s;
    tab[n + p] = q == 0 ? 0.0 : ss * sin(t) * s;
  }
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j) {
      const int p = (int)(((long)k * j) % n);
      out[(size_t)k * n + j] = (float)tab[p];
      out[(size_t)n * n + (size_t)k * n + j] = (float)tab[n + p];
    }
  delete[] tab;
}
