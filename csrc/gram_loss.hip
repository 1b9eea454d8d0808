// Gram-matrix style loss on the device (gfx950), Gatys et al. / Johnson et al.:
//   F_b = image b of the features as C x N (N = H W),  G(F)_b = F_b F_b^T / (C N)   (C x C, fp32)
//   L = mean_{b,i,j} (G(fx) - G(fy))^2,   dL/dfx_b = gout 4 / (B C^3 N) D_b fx_b,  D = G(fx) - G(fy)
// fy is a constant.  Features are bf16 NHWC, so image b is X[N][C] row-major and G = X^T X
// reduces over the ROWS: the weight-gradient layout.  C is a multiple of 64 in [64, 512], any
// N >= 1.  Three kernels, plain vector stores, no atomics, no host read of a device value.
//
//  1 gram_fwd      one launch for the 2B images of fx and fy.  A workgroup (4 waves, 2 x 2) owns
//                  one (image, macro pair, pixel split).  The macro tile is PW x PW output
//                  channels, PW = 64 for C = 64 and 128 above; only macro pairs bi <= bj exist
//                  in the grid and inside them only the 32 x 32 tiles gi <= gj are multiplied
//                  (a wave whose tiles all lie below the diagonal only helps loading).
//                  Pixels go through LDS in stages of 64 rows: buffer-load LDS-DMA (16 B per
//                  lane, rows past N and columns past C read as zero, so ragged tails need no
//                  code), 2 slots, the next stage in flight while this one is multiplied.  On a
//                  diagonal macro pair -- every pair for C <= 128, which is where the 16 K and
//                  64 K pixel reductions are -- ONE LDS panel feeds both MFMA operands; an
//                  off-diagonal pair stages its two 128-column panels.  (The issue asked for the
//                  whole Ks x C strip as one image: at C = 512 that needs 136 accumulator tiles
//                  per workgroup, more than 8 waves of registers hold, so the wide taps -- at
//                  most 4 K pixels -- re-read their panels through L2 instead.)  Both operands
//                  are read k-transposed with ds_read_b64_tr_b16 (the reduction index is the
//                  outer dimension), 16-B chunks XOR-swizzled so the 4 rows x 4 chunks of a half
//                  wave hit every bank once, a 2-deep fragment ring with counted waits, into
//                  v_mfma_f32_32x32x16_bf16 with fp32 accumulators.
//                  Split rule: with stages = ceil(N / 64), the grid should reach 1024 workgroups
//                  (4 per CU): sps = max(4, ceil(stages / ceil(1024 / (2B pairs)))) stages per
//                  split, splits = ceil(stages / sps).  Each split writes its fp32 partial to
//                  its own slab ws[image][split][C][C] (upper tiles only).
//  2 gram_finalize one workgroup per (b, 32 x 32 tile pair ti <= tj): sums the slabs of fx and
//                  of fy in split order, D = (Gx - Gy) / (C N) in fp32, through LDS to write the
//                  tile and its mirror (the diagonal tiles take element (min, max), so D is
//                  exactly symmetric), as fp32 D[B][C][C] and as its bf16 image, and one partial
//                  of sum D^2 (mirrored tiles count twice); the project's fixed-order sum makes
//                  the scalar.  Two calls are bitwise equal.
//  3 gram_bwd      dX[N][C] = s X[N][C] D[C][C], s = gout 4 / (B C^3 N) read on the device.
//                  D is symmetric, so the operand "D[k][c] for 8 consecutive k" is 16
//                  contiguous bytes of row c of the bf16 image: no transposed reads here.  A
//                  workgroup owns 64 pixels x BN output channels (BN = 64 for C = 64, else 128)
//                  and loops K = C in chunks of 64: X[64 x 64] and D[BN x 64] by LDS-DMA into 2
//                  slots, rows swizzled by (row / 2) % 8 for conflict-free 16-B fragment reads.
//                  The MFMA computes the tile transposed (rows = channels), so a lane holds 4
//                  consecutive channels of one pixel: scaled, rounded to bf16 and written to LDS
//                  8 bytes at a time, then stored to dX in 16-byte rows.
//                  D goes in as ONE bf16 image: emulated on the CPU (D rounded to bf16, fp32
//                  product, result rounded to bf16) the gradient's max-abs error over max-abs
//                  is 2.4e-3 .. 3.4e-3 at the test shapes against 2.3e-3 .. 3.2e-3 for a hi + lo
//                  pair -- the bf16 rounding of dX itself dominates -- so the second MFMA per
//                  tile would buy nothing.
#include "common.h"

namespace p2p {
namespace {

typedef float gl_f32x16 __attribute__((ext_vector_type(16)));

constexpr int GL_KS = 64;            // pixels per forward stage (4 k16 steps)
constexpr int GL_NT = 256;           // 4 waves, 2 x 2
constexpr int GL_MIN_SPS = 4;        // a split is at least 256 pixels
constexpr int GL_TARGET_WG = 1024;   // 4 workgroups per CU
constexpr uint32_t GL_OOB = 0x80000000u;

struct GramFwdArgs {
  const bf16* fx;
  const bf16* fy;
  float* ws;             // [2B][splits][C][C]
  int B, C, N, nb, splits, sps;
};

struct GramBwdArgs {
  const bf16* x;         // fx
  const bf16* dh;        // [B][C][C] bf16
  const float* gout;
  bf16* dx;
  float gscale;          // 4 / (B C^3 N)
  int B, C, N;
};

template <int N>
__device__ __forceinline__ void gl_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ uint32_t gl_lds(const void* p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const void*)p));
}

// one wave instruction: 64 lanes x 16 B from the buffer into 1 KB of LDS at `lds` (uniform)
__device__ __forceinline__ void gl_bld(__amdgpu_buffer_rsrc_t r, void* lds, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(lds), 16, voff, 0, 0, 0);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t gl_rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}

// a 32x32x16 operand fragment read k-transposed: k rows 8h .. 8h + 3 and 8h + 4 .. 8h + 7 of 32
// columns (RB = bytes per LDS row); afterwards lane l holds column l & 31, k = 8 (l >> 5) + j
template <int OFF, int RB>
__device__ __forceinline__ u32x4 gl_tr_frag(uint32_t addr) {
  static_assert(OFF >= 0 && OFF + 4 * RB < 65536, "ds offset field");
  uint64_t lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(addr), "i"(OFF));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(addr), "i"(OFF + 4 * RB));
  return u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

__device__ __forceinline__ u32x4 gl_frag16(uint32_t addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}

template <int TT>
struct GFrag {
  u32x4 a[TT], b[TT];
};

// wait until at most N LDS reads are outstanding; the fragments are tied in so that no use of
// them moves above the wait
template <int N, int TT>
__device__ __forceinline__ void gl_wait(GFrag<TT>& f) {
  static_assert(N >= 0 && N <= 15, "lgkmcnt range");
  if constexpr (TT == 2) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.b[0]), "+v"(f.b[1]) : "n"(N));
  } else {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(f.a[0]), "+v"(f.b[0]) : "n"(N));
  }
}

// swizzle key of LDS row r of a forward panel (XORed into the 16-B chunk index): rows 128
// columns wide repeat their banks every row, rows 64 wide every second row
template <int PW>
__device__ __forceinline__ int gl_key(int r) {
  return PW == 128 ? 4 * (r & 3) : 4 * ((r >> 1) & 1);
}

template <int S, int TT, int RB>
__device__ __forceinline__ void gl_read_step(GFrag<TT>& f, const uint32_t (&fa)[TT], const uint32_t (&fb)[TT],
                                             uint32_t slot) {
#pragma unroll
  for (int i = 0; i < TT; ++i) f.a[i] = gl_tr_frag<S * 16 * RB, RB>(fa[i] + slot);
#pragma unroll
  for (int j = 0; j < TT; ++j) f.b[j] = gl_tr_frag<S * 16 * RB, RB>(fb[j] + slot);
}

template <int TT>
__device__ __forceinline__ void gl_mma(const GFrag<TT>& f, gl_f32x16 (&acc)[TT][TT], const bool (&on)[TT][TT]) {
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j)
      if (on[i][j])
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.a[i]),
                                                             __builtin_bit_cast(bf16x8, f.b[j]), acc[i][j], 0, 0, 0);
}

// backward fragments of one k16 step: d = rows of D (channels), x = rows of X (pixels)
template <int TN>
struct BFrag {
  u32x4 d[TN], x;
};

template <int N, int TN>
__device__ __forceinline__ void gl_bwait(BFrag<TN>& f) {
  static_assert(N >= 0 && N <= 15, "lgkmcnt range");
  if constexpr (TN == 2) {
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(f.d[0]), "+v"(f.d[1]), "+v"(f.x) : "n"(N));
  } else {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(f.d[0]), "+v"(f.x) : "n"(N));
  }
}

template <int TN>
__device__ __forceinline__ void gl_bmma(const BFrag<TN>& f, gl_f32x16 (&acc)[TN]) {
#pragma unroll
  for (int j = 0; j < TN; ++j)
    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.d[j]),
                                                      __builtin_bit_cast(bf16x8, f.x), acc[j], 0, 0, 0);
}

// the LPW wave loads of one panel of stage `st` (disp = its byte displacement) into `dst`
template <int LPW>
__device__ __forceinline__ void gl_issue(__amdgpu_buffer_rsrc_t r, char* dst, int wid, const uint32_t (&vo)[LPW],
                                         uint32_t disp) {
#pragma unroll
  for (int q = 0; q < LPW; ++q) gl_bld(r, dst + (wid + 4 * q) * 1024, vo[q] == GL_OOB ? GL_OOB : vo[q] + disp);
}

}  // namespace

// PW: macro tile edge and LDS panel width in channels (64: C = 64; 128: C >= 128)
template <int PW>
__global__ void __launch_bounds__(GL_NT) gram_fwd_kernel(GramFwdArgs a) {
  constexpr int TT = PW / 64;             // 32 x 32 tiles per wave, each way
  constexpr int RB = PW * 2;              // bytes per LDS row
  constexpr int CPR = PW / 8;             // 16-B chunks per row
  constexpr int RPB = 1024 / RB;          // rows per wave load
  constexpr int SUB = GL_KS * RB;         // bytes of a panel
  constexpr int LPW = SUB / 1024 / 4;     // loads per wave and panel
  constexpr int NSUB = PW == 64 ? 1 : 2;  // C = 64 has the diagonal pair only
  constexpr int STAGE = NSUB * SUB;
  constexpr int NR = 4 * TT;              // transposed reads per k16 step
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int C = a.C, N = a.N;

  int bid = blockIdx.x;
  const int split = bid % a.splits;
  bid /= a.splits;
  const int pairs = a.nb * (a.nb + 1) / 2;
  const int img = bid / pairs;
  int bi = 0, rem = bid - img * pairs;
  while (rem >= a.nb - bi) {
    rem -= a.nb - bi;
    ++bi;
  }
  const int bj = bi + rem;
  const bool two = NSUB == 2 && bi != bj;

  const int stages = (N + GL_KS - 1) / GL_KS;
  const int s0 = split * a.sps, s1 = min(stages, s0 + a.sps);

  // ---- loader: lane l of wave load (wid + 4 q) fills LDS row RPB (wid + 4 q) + l / CPR, physical
  // chunk l % CPR, with the logical chunk that the swizzle puts there
  const bf16* X = img < a.B ? a.fx + (long)img * N * C : a.fy + (long)(img - a.B) * N * C;
  const __amdgpu_buffer_rsrc_t rs = gl_rsrc(X, (long)N * C * 2);
  uint32_t voa[LPW], vob[LPW];
#pragma unroll
  for (int q = 0; q < LPW; ++q) {
    const int row = RPB * (wid + 4 * q) + lane / CPR;
    const int lc = (lane % CPR) ^ gl_key<PW>(row);
    const int ca = bi * PW + 8 * lc, cb = bj * PW + 8 * lc;
    voa[q] = ca < C ? (uint32_t)((row * C + ca) * 2) : GL_OOB;
    vob[q] = cb < C ? (uint32_t)((row * C + cb) * 2) : GL_OOB;
  }
  const uint32_t stage_bytes = (uint32_t)(GL_KS * C * 2);

  // ---- fragment addresses (slot 0, k16 step 0): group G = lane >> 4 covers columns
  // 16 (G & 1) + 4 p .. + 3 of k rows 8 (G >> 1) + q (+ 4 for the high half)
  uint32_t fa[TT], fb[TT];
  bool on[TT][TT];
  {
    const int G = lane >> 4, qq = (lane & 15) >> 2, p = lane & 3;
    const int krow = 8 * (G >> 1) + qq;
#pragma unroll
    for (int i = 0; i < TT; ++i) {
      const int ca = wm * 32 * TT + i * 32 + 16 * (G & 1) + 4 * p;
      const int cb = wn * 32 * TT + i * 32 + 16 * (G & 1) + 4 * p;
      fa[i] = gl_lds(smem + krow * RB + (((ca >> 3) ^ gl_key<PW>(krow)) * 16) + (ca & 7) * 2);
      fb[i] = gl_lds(smem + (two ? SUB : 0) + krow * RB + (((cb >> 3) ^ gl_key<PW>(krow)) * 16) + (cb & 7) * 2);
    }
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
      for (int j = 0; j < TT; ++j)
        on[i][j] = bi * (PW / 32) + wm * TT + i <= bj * (PW / 32) + wn * TT + j;   // tile gi <= gj (uniform)
  }

  gl_f32x16 acc[TT][TT];
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (s0 < s1) {
    gl_issue<LPW>(rs, smem, wid, voa, (uint32_t)s0 * stage_bytes);
    if (two) gl_issue<LPW>(rs, smem + SUB, wid, vob, (uint32_t)s0 * stage_bytes);
    int cur = 0;
    GFrag<TT> fr[2];
    for (int st = s0; st < s1; ++st) {
      // stage st + 1 into the other slot (its readers passed the barrier that ended stage st - 1)
      if (st + 1 < s1) {
        char* nxt = smem + (cur ^ 1) * STAGE;
        gl_issue<LPW>(rs, nxt, wid, voa, (uint32_t)(st + 1) * stage_bytes);
        if (two) {
          gl_issue<LPW>(rs, nxt + SUB, wid, vob, (uint32_t)(st + 1) * stage_bytes);
          gl_vmcnt<2 * LPW>();
        } else {
          gl_vmcnt<LPW>();
        }
      } else {
        gl_vmcnt<0>();
      }
      __builtin_amdgcn_s_barrier();     // every wave's share of stage st has landed
      __builtin_amdgcn_sched_barrier(0);
      const uint32_t slot = (uint32_t)(cur * STAGE);
      gl_read_step<0, TT, RB>(fr[0], fa, fb, slot);
      gl_read_step<1, TT, RB>(fr[1], fa, fb, slot);
      gl_wait<NR, TT>(fr[0]);
      gl_mma<TT>(fr[0], acc, on);
      __builtin_amdgcn_sched_barrier(0);
      gl_read_step<2, TT, RB>(fr[0], fa, fb, slot);
      gl_wait<NR, TT>(fr[1]);
      gl_mma<TT>(fr[1], acc, on);
      __builtin_amdgcn_sched_barrier(0);
      gl_read_step<3, TT, RB>(fr[1], fa, fb, slot);
      gl_wait<NR, TT>(fr[0]);
      gl_mma<TT>(fr[0], acc, on);
      __builtin_amdgcn_sched_barrier(0);
      gl_wait<0, TT>(fr[1]);
      gl_mma<TT>(fr[1], acc, on);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();     // every read of this slot retired before it is refilled
      cur ^= 1;
    }
  }

  // ---- fp32 partial slab: acc[i][j][reg] = G[row (reg & 3) + 8 (reg >> 2) + 4 h][col l & 31]
  float* slab = a.ws + ((long)img * a.splits + split) * C * C;
  const int h = lane >> 5;
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      const int col = bj * PW + wn * 32 * TT + j * 32 + (lane & 31);
      const int rowb = bi * PW + wm * 32 * TT + i * 32 + 4 * h;
      if (on[i][j] && col < C) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rowb + (r & 3) + 8 * (r >> 2);
          if (row < C) slab[(long)row * C + col] = acc[i][j][r];
        }
      }
    }
}

// One workgroup per (b, tile pair ti <= tj) of 32 x 32; 256 threads, 4 elements each.
__global__ void __launch_bounds__(256) gram_finalize_kernel(const float* ws, int B, int C, int splits, float inv_cn,
                                                            float* d, bf16* dh, float* part) {
  __shared__ float t[32][33];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int nt = C / 32, ntp = nt * (nt + 1) / 2;
  const int b = blockIdx.x / ntp;
  int ti = 0, rem = blockIdx.x - b * ntp;
  while (rem >= nt - ti) {
    rem -= nt - ti;
    ++ti;
  }
  const int tj = ti + rem;
  const long cc = (long)C * C;
  const float* sx = ws + (long)b * splits * cc;
  const float* sy = ws + (long)(B + b) * splits * cc;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + 256 * q, r = e >> 5, c = e & 31;
    const long o = (long)(ti * 32 + r) * C + tj * 32 + c;
    float gx = 0.f, gy = 0.f;
    for (int s = 0; s < splits; ++s) {
      gx += sx[s * cc + o];
      gy += sy[s * cc + o];
    }
    t[r][c] = (gx - gy) * inv_cn;
  }
  __syncthreads();
  float* D = d + (long)b * cc;
  bf16* H = dh + (long)b * cc;
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = tid + 256 * q, r = e >> 5, c = e & 31;
    if (ti == tj) {
      const float v = t[min(r, c)][max(r, c)];
      const long o = (long)(ti * 32 + r) * C + ti * 32 + c;
      D[o] = v;
      H[o] = (bf16)v;
      sum += v * v;
    } else {
      const float v = t[r][c], w = t[c][r];
      const long o = (long)(ti * 32 + r) * C + tj * 32 + c, m = (long)(tj * 32 + r) * C + ti * 32 + c;
      D[o] = v;
      H[o] = (bf16)v;
      D[m] = w;
      H[m] = (bf16)w;
      sum += 2.f * v * v;
    }
  }
  sum = warp_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// TN: 32-channel tiles per wave; the workgroup owns 64 pixels x BN = 64 TN output channels
template <int TN>
__global__ void __launch_bounds__(GL_NT) gram_bwd_kernel(GramBwdArgs a) {
  constexpr int BN = 64 * TN;
  constexpr int XS = 64 * 128;            // X chunk: 64 pixels x 64 k
  constexpr int DS = BN * 128;            // D chunk: BN channels x 64 k
  constexpr int STAGE = XS + DS;
  constexpr int LX = 2, LD = 2 * TN;      // wave loads per wave: X, D
  constexpr int PITCH = BN * 2 + 16;      // output tile row (bytes)
  static_assert(64 * PITCH <= 2 * STAGE, "the output tile reuses the staging LDS");
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wp = wid & 1, wc = wid >> 1;   // pixel half, channel half
  const int C = a.C, N = a.N;
  const int ncn = (C + BN - 1) / BN, nrt = (N + 63) / 64;
  int bid = blockIdx.x;
  const int cn = bid % ncn;
  bid /= ncn;
  const int rt = bid % nrt, b = bid / nrt;
  const int r0 = rt * 64, c0 = cn * BN;

  // ---- loader: a wave load is 8 rows x 128 B; lane l -> row 8 (wid + 4 q) + l / 8, physical
  // chunk l % 8 holding logical chunk (l % 8) ^ ((row / 2) % 8).  Rows past N (X) or past C (D)
  // lie past the end of their buffer and read as zero.
  const __amdgpu_buffer_rsrc_t rx = gl_rsrc(a.x + (long)b * N * C, (long)N * C * 2);
  const __amdgpu_buffer_rsrc_t rd = gl_rsrc(a.dh + (long)b * C * C, (long)C * C * 2);
  uint32_t vx[LX], vd[LD];
#pragma unroll
  for (int q = 0; q < LX; ++q) {
    const int row = 8 * (wid + 4 * q) + (lane >> 3);
    vx[q] = (uint32_t)(((r0 + row) * C + 8 * ((lane & 7) ^ ((row >> 1) & 7))) * 2);
  }
#pragma unroll
  for (int q = 0; q < LD; ++q) {
    const int row = 8 * (wid + 4 * q) + (lane >> 3);
    vd[q] = (uint32_t)(((c0 + row) * C + 8 * ((lane & 7) ^ ((row >> 1) & 7))) * 2);
  }

  // ---- fragment rows: lane l holds row l & 31 of its tile, k = 16 s + 8 (l >> 5) .. + 7
  const int hh = lane >> 5;
  const int xrow = wp * 32 + (lane & 31);
  const uint32_t xbase = gl_lds(smem + xrow * 128), xkey = (uint32_t)((xrow >> 1) & 7);
  uint32_t dbase[TN], dkey[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int drow = wc * 32 * TN + j * 32 + (lane & 31);
    dbase[j] = gl_lds(smem + XS + drow * 128);
    dkey[j] = (uint32_t)((drow >> 1) & 7);
  }

  gl_f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int nk = C / 64;
  gl_issue<LX>(rx, smem, wid, vx, 0u);
  gl_issue<LD>(rd, smem + XS, wid, vd, 0u);
  int cur = 0;
  for (int kc = 0; kc < nk; ++kc) {
    if (kc + 1 < nk) {
      char* nxt = smem + (cur ^ 1) * STAGE;
      gl_issue<LX>(rx, nxt, wid, vx, (uint32_t)(kc + 1) * 128u);
      gl_issue<LD>(rd, nxt + XS, wid, vd, (uint32_t)(kc + 1) * 128u);
      gl_vmcnt<LX + LD>();
    } else {
      gl_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t slot = (uint32_t)(cur * STAGE);
    // the 4 (TN + 1) fragment reads of the chunk go out together (<= 12: the lgkm counter holds
    // 15); step s is multiplied once its own have landed
    BFrag<TN> f[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint32_t kch = (uint32_t)(2 * s + hh);
#pragma unroll
      for (int j = 0; j < TN; ++j) f[s].d[j] = gl_frag16(dbase[j] + slot + ((kch ^ dkey[j]) << 4));
      f[s].x = gl_frag16(xbase + slot + ((kch ^ xkey) << 4));
    }
    gl_bwait<3 * (TN + 1), TN>(f[0]);
    gl_bmma<TN>(f[0], acc);
    gl_bwait<2 * (TN + 1), TN>(f[1]);
    gl_bmma<TN>(f[1], acc);
    gl_bwait<TN + 1, TN>(f[2]);
    gl_bmma<TN>(f[2], acc);
    gl_bwait<0, TN>(f[3]);
    gl_bmma<TN>(f[3], acc);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }

  // ---- epilogue: acc[j][reg] = dX^T[channel (reg & 3) + 8 (reg >> 2) + 4 h][pixel l & 31]: four
  // consecutive channels of one pixel per register group -> LDS tile [pixel][channel], 16-B rows out
  const float s = a.gout[0] * a.gscale;
  char* out = smem;
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (bf16)(s * acc[j][4 * g + r]);
      const int ch = wc * 32 * TN + j * 32 + 8 * g + 4 * hh;
      *reinterpret_cast<bf16x4*>(out + (wp * 32 + (lane & 31)) * PITCH + ch * 2) = v;
    }
  __syncthreads();
  bf16* DX = a.dx + (long)b * N * C;
  for (int e = tid; e < 64 * (BN / 8); e += GL_NT) {
    const int row = e / (BN / 8), ch = e % (BN / 8);
    if (r0 + row < N && c0 + 8 * ch < C)
      *reinterpret_cast<u32x4*>(DX + (long)(r0 + row) * C + c0 + 8 * ch) =
          *reinterpret_cast<const u32x4*>(out + row * PITCH + ch * 16);
  }
}

static bool gram_shape_ok(int B, int C, int N) {
  // 31-bit buffer offsets: one image plus one stage past its end; 2B images of slabs
  return B >= 1 && N >= 1 && C >= 64 && C <= 512 && C % 64 == 0 && ((long)N + GL_KS) * C * 2 < (1L << 31) &&
         (long)B * (C / 32) * (C / 32 + 1) / 2 < (1L << 31);
}

// the split rule of the header: stages per split and the number of splits
static void gram_split(int B, int C, int N, int& nb, int& sps, int& splits) {
  nb = C <= 64 ? 1 : (C + 127) / 128;
  const long wgs = 2L * B * (nb * (nb + 1) / 2);
  const int want = (int)((GL_TARGET_WG + wgs - 1) / wgs);
  const int stages = (N + GL_KS - 1) / GL_KS;
  sps = (stages + want - 1) / want;
  if (sps < GL_MIN_SPS) sps = GL_MIN_SPS;
  splits = (stages + sps - 1) / sps;
}

}  // namespace p2p

extern "C" int p2p_gram_splits(int B, int C, int N) {
  int nb, sps, splits;
  p2p::gram_split(B, C, N, nb, sps, splits);
  return splits;
}

// floats of forward workspace: the slabs, the per-tile partials and 256 for the two-stage sum
extern "C" long p2p_gram_ws(int B, int C, int N) {
  const long nt = C / 32;
  return 2L * B * p2p_gram_splits(B, C, N) * C * C + (long)B * nt * (nt + 1) / 2 + 256;
}

// fx, fy: bf16 [B][N][C] (NHWC, dense).  Writes d (fp32 [B][C][C]), dh (its bf16 image) and loss[0].
extern "C" int p2p_gram_fwd(const void* fx, const void* fy, int B, int C, int N, float* ws, float* d, void* dh,
                            float* loss, hipStream_t st) {
  using namespace p2p;
  if (!gram_shape_ok(B, C, N)) return -1;
  GramFwdArgs a{};
  a.fx = static_cast<const bf16*>(fx);
  a.fy = static_cast<const bf16*>(fy);
  a.ws = ws;
  a.B = B; a.C = C; a.N = N;
  gram_split(B, C, N, a.nb, a.sps, a.splits);
  const long grid = 2L * B * (a.nb * (a.nb + 1) / 2) * a.splits;
  if (grid >= (1L << 31)) return -1;
  if (C == 64) hipLaunchKernelGGL(gram_fwd_kernel<64>, dim3((unsigned)grid), dim3(GL_NT), 0, st, a);
  else hipLaunchKernelGGL(gram_fwd_kernel<128>, dim3((unsigned)grid), dim3(GL_NT), 0, st, a);
  const long nt = C / 32, tiles = (long)B * nt * (nt + 1) / 2;
  float* part = ws + 2L * B * a.splits * C * C;
  hipLaunchKernelGGL(gram_finalize_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ws, B, C, a.splits,
                     (float)(1.0 / ((double)C * N)), d, static_cast<bf16*>(dh), part);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const float scale = (float)(1.0 / ((double)B * C * C));
  return p2p_sum_fixed(part, tiles, scale, loss, st);
}

// dx[B][N][C] = gout 4 / (B C^3 N) fx D, D from dh (the bf16 image of the forward)
extern "C" int p2p_gram_bwd(const void* fx, const void* dh, const float* gout, int B, int C, int N, void* dx,
                            hipStream_t st) {
  using namespace p2p;
  if (!gram_shape_ok(B, C, N)) return -1;
  GramBwdArgs a{};
  a.x = static_cast<const bf16*>(fx);
  a.dh = static_cast<const bf16*>(dh);
  a.gout = gout;
  a.dx = static_cast<bf16*>(dx);
  a.gscale = (float)(4.0 / ((double)B * C * C * C * N));
  a.B = B; a.C = C; a.N = N;
  const long rows = (long)B * ((N + 63) / 64);
  const long grid = C == 64 ? rows : rows * ((C + 127) / 128);
  if (grid >= (1L << 31)) return -1;
  if (C == 64) hipLaunchKernelGGL(gram_bwd_kernel<1>, dim3((unsigned)grid), dim3(GL_NT), 0, st, a);
  else hipLaunchKernelGGL(gram_bwd_kernel<2>, dim3((unsigned)grid), dim3(GL_NT), 0, st, a);
  return (int)hipGetLastError();
}
