// Device kernels for the streaming NCC side-information search (gfx950).
// Torch-free so the file compiles standalone for .s inspection and probing:
//   hipcc --offload-arch=gfx950 -O3 -x hip -c ncc_kernels.h
// Semantics documented in ncc_search.hip (the host wrapper).
#pragma once
#include <hip/hip_runtime.h>
#include "device_common.h"

namespace dsin {

// KITTI stats used inside the SI search (reference src/siFinder.py:62-63;
// the `variances` there are standard deviations)
__constant__ float SIF_MEAN[3] = {93.70454143384742f, 98.28243432206516f,
                                  94.84678088809876f};
__constant__ float SIF_STD[3] = {73.56493292844912f, 75.88547006820752f,
                                 76.74838442810665f};

constexpr float FOURLN2 = 2.772588722239781f;  // 4 ln 2
constexpr float NCC_EPS = 1e-10f;  // guards zero-variance windows (both paths)

constexpr int NCC_TP = 32;   // patches per workgroup (MFMA 32x32 M tile)
constexpr int NCC_TJ = 128;  // cols per workgroup (4 waves x 32)
constexpr int NCC_TI = 8;    // rows looped per workgroup
constexpr int NCC_APAD = 8;  // bf16 pad per A row for the b128 column reads
// v2 only (ncc_main_v2_kernel):
constexpr int NCC_SL = 384;  // taps per A slice (multiple of 16; 2x25KB buffers -> 3 blocks/CU)
constexpr int NCC_TJ2 = 64;  // v2 col tile: 2 j-waves x 32 — the y window
                             // (3 x 27 x 87 bf16 = 14 KB/block) then fits
                             // L1 with two co-resident blocks; the other 2
                             // waves take the other 4-row output group

// Every kernel below except ncc_offsets_kernel runs B images of one geometry
// in one launch. The image index comes from the grid (blockIdx.y, or folded
// into blockIdx.z in the two main kernels), is uniform over the block and is
// used once, at entry, to move the base pointers to this image, in 64-bit
// arithmetic: B*3*H*W can pass 2^31. Per-image strides:
//   tx, ty, y_orig, y_syn          3*H*W
//   psum, psum2, best, rows, cols  P
//   s1, s2                         H*Wc
//   sy, sy2                        Hc*Wc
// Everything after the entry indexes within one image, as for B = 1.

// ---------------------------------------------------------------- stage 0
// Offset tables, computed once per call (geometry only, shared by the images):
//   aoffs[k] = element offset of flat-k within the (3,H,W) image relative to
//              a patch origin (k = (c*ph + a)*pw + b)
//   koffs[k] = element offset of flat-k within the LDS y-window image
//              [3][YR][YCP] relative to (row i=0, col jj=0)
__global__ void ncc_offsets_kernel(unsigned int* __restrict__ aoffs,
                                   unsigned short* __restrict__ koffs,
                                   int H, int W, int ph, int pw, int YR,
                                   int YCP, int K) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  int c = k / (ph * pw), rem = k % (ph * pw);
  int a = rem / pw, b = rem % pw;
  aoffs[k] = (unsigned int)((c * H + a) * W + b);
  koffs[k] = (unsigned short)((c * YR + a) * YCP + b);
}

// ---------------------------------------------------------------- stage 1

__global__ void transform_kernel(const float* __restrict__ img,
                                 bf16* __restrict__ out, long long hw) {
  img += (long long)blockIdx.y * 3 * hw;
  out += (long long)blockIdx.y * 3 * hw;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < hw; i += stride) {
    float r = (img[i] - SIF_MEAN[0]) / SIF_STD[0];
    float g = (img[hw + i] - SIF_MEAN[1]) / SIF_STD[1];
    float b = (img[2 * hw + i] - SIF_MEAN[2]) / SIF_STD[2];
    out[i] = f2b(r + g);
    out[hw + i] = f2b(r - g);
    out[2 * hw + i] = f2b(0.5f * (r + b));
  }
}

// L2+LAB mode (use_L2andLAB): CIELAB of the RAW pixel values, as the
// reference feeds them (0..255 straight into the sRGB gamma, no rescale, no
// fixed-stats normalization). Both piecewise functions take their linear
// branch at and below the threshold, which includes every negative value.
__device__ __forceinline__ float lab_lin(float px) {
  return px <= 0.04045f ? px / 12.92f
                        : powf((px + 0.055f) / 1.055f, 2.4f);
}

__device__ __forceinline__ float lab_f(float t) {
  constexpr float EPS3 = (float)((6.0 / 29.0) * (6.0 / 29.0) * (6.0 / 29.0));
  constexpr float LIN = (float)(3.0 * (6.0 / 29.0) * (6.0 / 29.0));
  return t <= EPS3 ? t / LIN + (float)(4.0 / 29.0) : cbrtf(t);
}

__global__ void lab_transform_kernel(const float* __restrict__ img,
                                     bf16* __restrict__ out, long long hw) {
  img += (long long)blockIdx.y * 3 * hw;
  out += (long long)blockIdx.y * 3 * hw;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < hw; i += stride) {
    const float r = lab_lin(img[i]);
    const float g = lab_lin(img[hw + i]);
    const float b = lab_lin(img[2 * hw + i]);
    // linear RGB -> XYZ over the white point (0.950456, 1, 1.088754)
    const float x = (0.412453f * r + 0.357580f * g + 0.180423f * b) *
                    (float)(1.0 / 0.950456);
    const float y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
    const float z = (0.019334f * r + 0.119193f * g + 0.950227f * b) *
                    (float)(1.0 / 1.088754);
    const float fx = lab_f(x), fy = lab_f(y), fz = lab_f(z);
    out[i] = f2b(116.f * fy - 16.f);
    out[hw + i] = f2b(500.f * (fx - fy));
    out[2 * hw + i] = f2b(200.f * (fy - fz));
  }
}

// ---------------------------------------------------------------- stage 2

__global__ void patch_stats_kernel(const bf16* __restrict__ tx,
                                   const unsigned int* __restrict__ aoffs,
                                   float* __restrict__ psum,
                                   float* __restrict__ psum2,
                                   int H, int W, int ph, int pw, int gw,
                                   int K) {
  const int P = gridDim.x;  // grid (P, B)
  tx += (long long)blockIdx.y * 3 * H * W;
  psum += (long long)blockIdx.y * P;
  psum2 += (long long)blockIdx.y * P;
  int p = blockIdx.x;
  long long base = (long long)((p / gw) * ph) * W + (p % gw) * pw;
  float s = 0.f, s2 = 0.f;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    float v = b2f(tx[base + aoffs[k]]);
    s += v;
    s2 += v * v;
  }
  s = wave_reduce_sum(s);
  s2 = wave_reduce_sum(s2);
  if (threadIdx.x == 0) {
    psum[p] = s;
    psum2[p] = s2;
  }
}

// ---------------------------------------------------------------- stage 3

__global__ void ysum_row_kernel(const bf16* __restrict__ ty,
                                float* __restrict__ s1, float* __restrict__ s2,
                                int H, int W, int pw, int Wc) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)H * Wc;
  ty += (long long)blockIdx.y * 3 * H * W;
  s1 += (long long)blockIdx.y * total;
  s2 += (long long)blockIdx.y * total;
  if (i >= total) return;
  int r = i / Wc, j = i % Wc;
  float a = 0.f, b = 0.f;
  for (int c = 0; c < 3; ++c) {
    const bf16* row = ty + ((long long)c * H + r) * W + j;
    for (int k = 0; k < pw; ++k) {
      float v = b2f(row[k]);
      a += v;
      b += v * v;
    }
  }
  s1[i] = a;
  s2[i] = b;
}

__global__ void ysum_col_kernel(const float* __restrict__ s1,
                                const float* __restrict__ s2,
                                float* __restrict__ sy,
                                float* __restrict__ sy2,
                                int Hc, int Wc, int ph) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)Hc * Wc;
  const long long rows_in = (long long)(Hc + ph - 1) * Wc;  // H*Wc
  s1 += (long long)blockIdx.y * rows_in;
  s2 += (long long)blockIdx.y * rows_in;
  sy += (long long)blockIdx.y * total;
  sy2 += (long long)blockIdx.y * total;
  if (i >= total) return;
  int r = i / Wc, j = i % Wc;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < ph; ++k) {
    a += s1[(long long)(r + k) * Wc + j];
    b += s2[(long long)(r + k) * Wc + j];
  }
  sy[i] = a;
  sy2[i] = b;
}


// ------------------------------------------- stage 4: the shared pieces
// Both main kernels run mfma_f32_32x32x16_bf16 with a patch tile as A:
// A[row = l & 31][k = (l >> 5) * 8 + e], B[k][col = l & 31], and accumulator
// register `reg` of lane l holds C[ncc_prow(reg, l >> 5)][l & 31].

__device__ __forceinline__ int ncc_prow(int reg, int kgrp) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * kgrp;
}

// Dynamic LDS of the two main kernels: byte offsets of the arrays behind As
// (which starts the block) and the launch's byte count. The kernels place
// their arrays by these and the host wrapper sizes the launch by them.
//   v1: As [TP][ASTRIDE] bf16 | Ys [3][YR][YCP] bf16 | Ko [KP] u16 | Pstat
//   v2: As 2 x [TP][ASTRIDE] bf16 | Pstat
// Pstat is [5][TP] float: per patch sum_x, mean_x, den_x (L2: sum_x2 in row
// 0, rows 1 and 2 unused), then the prior's centre row and column.
struct NccLdsV1 {
  int KP, YR, YC, YCP, ASTRIDE;
  int ys, ko, pstat;
  size_t bytes;
};
struct NccLdsV2 {
  int KP, ASTRIDE;
  int pstat;
  size_t bytes;
};

constexpr int NCC_PSTAT_BYTES = 5 * NCC_TP * 4;

__host__ __device__ constexpr NccLdsV1 ncc_lds_v1(int ph, int pw) {
  NccLdsV1 l{};
  l.KP = (3 * ph * pw + 15) & ~15;
  l.YR = NCC_TI + ph - 1;
  l.YC = NCC_TJ + pw - 1;
  l.YCP = (l.YC + 8) & ~7;
  l.ASTRIDE = l.KP + NCC_APAD;
  l.ys = NCC_TP * l.ASTRIDE * 2;
  l.ko = l.ys + 3 * l.YR * l.YCP * 2;
  l.pstat = l.ko + l.KP * 2;
  l.bytes = (size_t)l.pstat + NCC_PSTAT_BYTES;
  return l;
}

__host__ __device__ constexpr NccLdsV2 ncc_lds_v2(int ph, int pw) {
  NccLdsV2 l{};
  l.KP = (3 * ph * pw + 15) & ~15;
  l.ASTRIDE = NCC_SL + NCC_APAD;
  l.pstat = 2 * NCC_TP * l.ASTRIDE * 2;
  l.bytes = (size_t)l.pstat + NCC_PSTAT_BYTES;
  return l;
}

// The first NCC_TP threads of a workgroup fill Pstat for patches p0..p0+TP-1
// (clamped to the last patch; rows beyond P are masked in the epilogue).
template <bool L2>
__device__ __forceinline__ void ncc_stage_pstat(
    float* __restrict__ Pstat, int tid, int p0, int P,
    const float* __restrict__ psum, const float* __restrict__ psum2, int K,
    int ph, int pw, int gw) {
  if (tid < NCC_TP) {
    const float fK = (float)K;
    const float invK = 1.f / fK;
    const int p = min(p0 + tid, P - 1);
    if constexpr (L2) {
      Pstat[tid] = psum2[p];
    } else {
      const float sxv = psum[p];
      const float xm = sxv * invK;
      Pstat[tid] = sxv;
      Pstat[NCC_TP + tid] = xm;
      Pstat[2 * NCC_TP + tid] = psum2[p] - 2.f * xm * sxv + fK * xm * xm;
    }
    Pstat[3 * NCC_TP + tid] = ((float)(p / gw) + 0.5f) * (float)ph;  // cr
    Pstat[4 * NCC_TP + tid] = ((float)(p % gw) + 0.5f) * (float)pw;  // cw
  }
}

// What the epilogue needs besides an accumulator: the call's geometry and
// this lane's place in it (first patch of the workgroup, output column,
// half-wave). Passed by value: by reference ncc_main_v2_kernel<false>
// compiles to 184 registers instead of 180 and the v1 kernels to 16 more
// (profiles/r13_ncc_device.md).
struct NccEpi {
  int H, W, ph, pw, P, Wc, K, use_mask;
  int p0, j, kgrp;
};

// Scores output row iw of one accumulator (16 patches x this lane's column)
// and folds them into the lane's running keys. Fully predicated, no divergent
// branch: fast-rsqrt Pearson (or the L2 distance), the Gaussian prior
// evaluated inline, then the key (flipped float << 32 | ~idx), so that the
// u64 maximum is the best score at the smallest flat index. The L2 winner is
// the MINIMUM, taken by the same maximum on the key of 0 - d: the
// subtraction folds -0 into +0, so equal distances give one key.
template <bool L2>
__device__ __forceinline__ void ncc_epilogue_row(
    const f32x16& acc, int iw, const NccEpi g,
    const float* __restrict__ Pstat, const float* __restrict__ sy,
    const float* __restrict__ sy2, unsigned long long (&bestk)[16]) {
  const float fK = (float)g.K;
  const float invK = 1.f / fK;
  const float ish2 = 4.0f / ((float)g.H * (float)g.H);   // 1/sh^2, sh = H/2
  const float isw2 = 4.0f / ((float)g.W * (float)g.W);
  const bool jvalid = g.j < g.Wc;
  const long long sidx = (long long)iw * g.Wc + (jvalid ? g.j : 0);
  const float di = (float)(iw + g.ph / 2 - 1);
  const float dj0 = (float)(g.j + g.pw / 2 - 1);
  const unsigned int idx = (unsigned int)(iw * g.Wc + g.j);
  const float sy2v = sy2[sidx];
  float syv = 0.f, ym = 0.f, deny = 0.f;
  if constexpr (!L2) {
    syv = sy[sidx];
    ym = syv * invK;
    deny = sy2v - 2.f * ym * syv + fK * ym * ym;
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int prow = ncc_prow(reg, g.kgrp);
    const float av = acc[reg];
    float val;
    if constexpr (L2) {
      val = Pstat[prow] - 2.f * av + sy2v;
    } else {
      const float sxv = Pstat[prow];
      const float xm = Pstat[NCC_TP + prow];
      const float denx = Pstat[2 * NCC_TP + prow];
      const float num = av - ym * sxv - xm * syv + fK * xm * ym;
      val = num * __builtin_amdgcn_rsqf(fmaxf(denx * deny, NCC_EPS));
    }
    if (g.use_mask) {
      const float dd = di - Pstat[3 * NCC_TP + prow];
      const float dj = dj0 - Pstat[4 * NCC_TP + prow];
      val *= __expf(-FOURLN2 * (dd * dd * ish2 + dj * dj * isw2));
    }
    unsigned long long key =
        ((unsigned long long)float_flip(L2 ? 0.f - val : val) << 32) |
        (unsigned long long)(~idx);
    key = (jvalid && (g.p0 + prow) < g.P) ? key : 0ull;
    if (key > bestk[reg]) bestk[reg] = key;
  }
}

// The main kernels' grid is (column tiles, row tiles, B * patch tiles) with
// the image the slowest part of z: the workgroups of one image stay adjacent
// in block order and keep its ty hot in L2/L1, as for one image. Moves the
// per-image pointers to this block's image and returns its first patch.
// zmagic = 2^32 / ptiles + 1 comes from the host: (z * zmagic) >> 32 equals
// z / ptiles for every z, ptiles < 2^16 (the error term z * (zmagic * ptiles
// - 2^32) stays below 2^32), which is all gridDim.z admits. Chosen by
// measurement: with a plain division here the one-image v1 L2 search ran 0.9
// to 1.7 % slower than before the batch, with this form 0.5 to 0.9 %
// (profiles/r15_ncc_batch.md; the mechanism is not established).
__device__ __forceinline__ int ncc_enter_image(
    unsigned long long zmagic, int H, int W, int P, int Hc, int Wc,
    const bf16* __restrict__& tx,
    const bf16* __restrict__& ty, const float* __restrict__& psum,
    const float* __restrict__& psum2, const float* __restrict__& sy,
    const float* __restrict__& sy2, unsigned long long* __restrict__& best) {
  const int ptiles = (P + NCC_TP - 1) / NCC_TP;
  const int b = (int)(((unsigned long long)blockIdx.z * zmagic) >> 32);
  const long long img = (long long)b * 3 * H * W;
  const long long loc = (long long)b * Hc * Wc;
  tx += img;
  ty += img;
  psum += (long long)b * P;
  psum2 += (long long)b * P;
  sy += loc;
  sy2 += loc;
  best += (long long)b * P;
  return (blockIdx.z - b * ptiles) * NCC_TP;
}

// Reduces the running keys across the 32 lanes of each half-wave (distinct
// columns, the same 16 patches) and sends one atomicMax per patch.
__device__ __forceinline__ void ncc_merge_best(
    const unsigned long long (&bestk)[16],
    unsigned long long* __restrict__ best, int p0, int P, int lane) {
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    unsigned long long k = bestk[reg];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      unsigned long long other =
          (unsigned long long)__shfl_xor((long long)k, off, 32);
      if (other > k) k = other;
    }
    const int prow = p0 + ncc_prow(reg, lane >> 5);
    if ((lane & 31) == 0 && prow < P && k != 0ull) atomicMax(&best[prow], k);
  }
}

// ---------------------------------------------------------------- stage 4
// Main correlation kernel, v1 (any pw). MFMA 32x32x16 bf16: 2x the flops per
// B gather of the 16x16 shape, and the gather is the cost here. Per k-chunk
// the B fragment is gathered from the LDS y-window via the koffs table (1
// broadcast b128 read of 8 offsets + 8 u16 value reads per MFMA, no
// per-element index math). Two interleaved i-rows keep two independent
// accumulator chains in flight. Epilogue: ncc_epilogue_row per row, one
// ncc_merge_best at the end.
//
// L2 = true is the L2+LAB mode: same staging, MFMA loop and LDS layout; only
// the epilogue's score and the contents of Pstat differ; psum and sy are not
// read.

template <bool L2>
__global__ __launch_bounds__(256)
void ncc_main_kernel(const bf16* __restrict__ tx, const bf16* __restrict__ ty,
                     const unsigned int* __restrict__ aoffs,
                     const unsigned short* __restrict__ koffs,
                     const float* __restrict__ psum,
                     const float* __restrict__ psum2,
                     const float* __restrict__ sy,
                     const float* __restrict__ sy2,
                     unsigned long long* __restrict__ best,  // (B, P)
                     int H, int W, int ph, int pw, int gw, int P,
                     int Hc, int Wc, int use_mask,
                     unsigned long long zmagic) {
  const int K = 3 * ph * pw;
  const NccLdsV1 lds = ncc_lds_v1(ph, pw);
  const int KP = lds.KP, YR = lds.YR, YC = lds.YC, YCP = lds.YCP;
  const int ASTRIDE = lds.ASTRIDE;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* As = reinterpret_cast<bf16*>(smem);                  // [TP][ASTRIDE]
  bf16* Ys = reinterpret_cast<bf16*>(smem + lds.ys);         // [3][YR][YCP]
  unsigned short* Ko = reinterpret_cast<unsigned short*>(smem + lds.ko);
  float* Pstat = reinterpret_cast<float*>(smem + lds.pstat);  // [5][TP]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int j0 = blockIdx.x * NCC_TJ;
  const int i0 = blockIdx.y * NCC_TI;
  const int p0 = ncc_enter_image(zmagic, H, W, P, Hc, Wc, tx, ty, psum,
                                 psum2, sy, sy2, best);

  // ---- stage A tile (32 patches x K), y window, koffs, patch stats ----
  for (int k = tid; k < KP; k += 256) Ko[k] = (k < K) ? koffs[k] : 0;
  ncc_stage_pstat<L2>(Pstat, tid, p0, P, psum, psum2, K, ph, pw, gw);
#pragma unroll 1
  for (int pi = 0; pi < NCC_TP; ++pi) {
    const int p = p0 + pi;
    const long long pbase =
        (p < P) ? (long long)((p / gw) * ph) * W + (long long)((p % gw) * pw)
                : 0;
    for (int k = tid; k < KP; k += 256) {
      bf16 v = f2b(0.f);
      if (k < K && p < P) v = tx[pbase + aoffs[k]];
      As[pi * ASTRIDE + k] = v;
    }
  }
  {
    const int nY = 3 * YR * YC;
    for (int idx = tid; idx < nY; idx += 256) {
      int c = idx / (YR * YC), rem = idx % (YR * YC);
      int rr = rem / YC, cc = rem % YC;
      int r = i0 + rr, col = j0 + cc;
      float v = (r < H && col < W)
                    ? b2f(ty[((long long)c * H + r) * W + col])
                    : 0.f;
      Ys[(c * YR + rr) * YCP + cc] = f2b(v);
    }
  }
  __syncthreads();

  const int colL = lane & 31;          // col within the wave's 32
  const int kgrp = lane >> 5;          // 0/1 (k-offset 0/8 within 16)
  const int jj = wid * 32 + colL;
  const NccEpi epi = {H, W, ph, pw, P, Wc, K, use_mask, p0, j0 + jj, kgrp};

  unsigned long long bestk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bestk[r] = 0ull;

  const bf16* __restrict__ arow = &As[kgrp * 8];
  const unsigned short* __restrict__ krow = &Ko[kgrp * 8];

  for (int i = 0; i < NCC_TI; i += 2) {
    const int ii = i0 + i;
    if (ii >= Hc) break;
    const bool i1ok = (ii + 1) < Hc;
    f32x16 acc0 = {};
    f32x16 acc1 = {};
    const bf16* __restrict__ yb0 = &Ys[i * YCP + jj];
    const bf16* __restrict__ yb1 = &Ys[(i + 1) * YCP + jj];
    for (int kt = 0; kt < KP / 16; ++kt) {
      const u16x8 ko8 =
          *reinterpret_cast<const u16x8*>(krow + kt * 16);
      bf16x8 bf0, bf1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bf16 v0 = yb0[ko8[e]];
        bf16 v1 = yb1[ko8[e]];
        bf0[e] = *reinterpret_cast<__bf16*>(&v0);
        bf1[e] = *reinterpret_cast<__bf16*>(&v1);
      }
      // A fragment: row = colL (patch), k = kgrp*8 + e
      const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
          &arow[colL * ASTRIDE + kt * 16]);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bf0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bf1, acc1, 0, 0, 0);
    }
    ncc_epilogue_row<L2>(acc0, ii, epi, Pstat, sy, sy2, bestk);
    if (i1ok) ncc_epilogue_row<L2>(acc1, ii + 1, epi, Pstat, sy, sy2, bestk);
  }
  ncc_merge_best(bestk, best, p0, P, lane);
}

// ------------------------------------------------------- stage 4, variant 2
// Requires pw % 8 == 0 (the default (20,24) and every bench fallback patch).
// The v1 kernel keeps the whole (32 x K) A-tile in LDS (93 KB at K=1440 ->
// ONE workgroup per CU, 1 wave/SIMD) and gathers each B fragment with 8
// scalar LDS reads + packing (issue-bound, 105 cyc/MFMA measured). Here:
//   * A is staged in K-SLICES of NCC_SL taps (33 KB -> 3-4 workgroups/CU,
//     the load latency finally has TLP to hide under);
//   * each 8-element k-group of a row lies in ONE patch row, so a B
//     fragment is a single unaligned global u16x8 read of the L1/L2-hot
//     transformed side image (no y-window staging, no offset table, no
//     packing VALU);
//   * the k-loop is OUTER over 4-row output groups, so one LDS A fragment
//     feeds 4 MFMAs (4 independent accumulator chains).

// Same Pstat, epilogue and merge as v1, in both modes.
template <bool L2>
__global__ __launch_bounds__(256)
void ncc_main_v2_kernel(const bf16* __restrict__ tx,
                        const bf16* __restrict__ ty,
                        const unsigned int* __restrict__ aoffs,
                        const float* __restrict__ psum,
                        const float* __restrict__ psum2,
                        const float* __restrict__ sy,
                        const float* __restrict__ sy2,
                        unsigned long long* __restrict__ best,  // (B, P)
                        int H, int W, int ph, int pw, int gw, int P,
                        int Hc, int Wc, int use_mask,
                        unsigned long long zmagic) {
  const int K = 3 * ph * pw;
  const NccLdsV2 lds = ncc_lds_v2(ph, pw);
  const int KP = lds.KP;
  const int ASTRIDE = lds.ASTRIDE;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* As = reinterpret_cast<bf16*>(smem);                   // 2 x [TP][ASTRIDE]
  float* Pstat = reinterpret_cast<float*>(smem + lds.pstat);  // [5][TP]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int j0 = blockIdx.x * NCC_TJ2;
  const int i0 = blockIdx.y * NCC_TI;
  const int p0 = ncc_enter_image(zmagic, H, W, P, Hc, Wc, tx, ty, psum,
                                 psum2, sy, sy2, best);

  ncc_stage_pstat<L2>(Pstat, tid, p0, P, psum, psum2, K, ph, pw, gw);

  // slice staging: 8 threads per patch row, each stages NCC_SL/8 taps (runs
  // of 8 contiguous image elements via aoffs); zero-fills beyond K / beyond
  // P. The 8 threads must cover exactly NCC_SL taps: staging past the slice
  // would spill into the next patch row, the other buffer and Pstat.
  constexpr int S_TAPS = NCC_SL / 8;
  static_assert(NCC_SL % 64 == 0, "slice = 8 threads x whole 8-tap runs");
  const int s_pi = tid & 31;
  const int s_k0 = (tid >> 5) * S_TAPS;
  const int sp = p0 + s_pi;
  const bool s_pok = sp < P;
  const long long s_pbase =
      s_pok ? (long long)((sp / gw) * ph) * W + (long long)((sp % gw) * pw)
            : 0;
  auto stage_slice = [&](int s0, int buf) {
    bf16* dst = As + buf * NCC_TP * ASTRIDE;
#pragma unroll
    for (int r8 = 0; r8 < S_TAPS / 8; ++r8) {
      const int kl = s_k0 + r8 * 8;
      const int kg = s0 + kl;
      u16x8 v = {};
      if (s_pok && kg < K)
        v = *reinterpret_cast<const u16x8*>(&tx[s_pbase + aoffs[kg]]);
      *reinterpret_cast<u16x8*>(&dst[s_pi * ASTRIDE + kl]) = v;
    }
  };

  const int colL = lane & 31;
  const int kgrp = lane >> 5;
  const int jj = (wid & 1) * 32 + colL;   // 2 j-waves cover TJ2 columns
  const int g0 = (wid >> 1) * 4;          // 2 row-group waves cover TI rows
  const NccEpi epi = {H, W, ph, pw, P, Wc, K, use_mask, p0, j0 + jj, kgrp};

  unsigned long long bestk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bestk[r] = 0ull;

  const int nslices = (KP + NCC_SL - 1) / NCC_SL;

  // this wave's 4-row output group (the A slices are shared by all waves)
  const int iig = i0 + g0;
  // clamped row offsets (rows beyond Hc read row Hc-1; discarded below)
  long long rofs[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    rofs[r] = (long long)min(iig + r, Hc - 1) * W + (j0 + jj);
  f32x16 a0 = {}, a1 = {}, a2 = {}, a3 = {};
  // double-buffered slices: slice s+1 stages (scattered global reads + LDS
  // writes into the other buffer) while the MFMA loop consumes slice s; one
  // barrier per slice
  stage_slice(0, 0);
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < nslices; ++s) {
    if (s + 1 < nslices) stage_slice((s + 1) * NCC_SL, (s + 1) & 1);
    bf16* As_cur = As + (s & 1) * NCC_TP * ASTRIDE;
    // incremental (c, a, b) decode of this half-wave's k-group
    int dyc, dya, dyb;
    {
      int k0g = s * NCC_SL + kgrp * 8;
      dyc = k0g / (ph * pw);
      int rem = k0g % (ph * pw);
      dya = rem / pw;
      dyb = rem % pw;
    }
    const int nkt = min(NCC_SL, KP - s * NCC_SL) / 16;
    auto advance = [&]() {
      dyb += 16;
      if (dyb >= pw) {
        dyb -= pw;
        if (++dya >= ph) { dya = 0; ++dyc; }
        if (dyb >= pw) {  // pw == 8: one 16-step crosses two rows
          dyb -= pw;
          if (++dya >= ph) { dya = 0; ++dyc; }
        }
      }
      if (dyc > 2) { dyc = 2; dya = 0; }  // KP padding: A zeros cancel
    };
    // two register SETS ping-pong (no cross-iteration copies): the next
    // chunk's five loads issue before the current chunk's MFMAs
    u16x8 v0a, v1a, v2a, v3a, v0b, v1b, v2b, v3b;
    bf16x8 afa, afb;
    auto load_set = [&](int kt, u16x8& v0, u16x8& v1, u16x8& v2, u16x8& v3,
                        bf16x8& af) {
      const long long offk = ((long long)(dyc * H) + dya) * W + dyb;
      af = *reinterpret_cast<const bf16x8*>(
          &As_cur[colL * ASTRIDE + kt * 16 + kgrp * 8]);
      v0 = *reinterpret_cast<const u16x8*>(&ty[offk + rofs[0]]);
      v1 = *reinterpret_cast<const u16x8*>(&ty[offk + rofs[1]]);
      v2 = *reinterpret_cast<const u16x8*>(&ty[offk + rofs[2]]);
      v3 = *reinterpret_cast<const u16x8*>(&ty[offk + rofs[3]]);
      advance();
    };
    auto mfma_set = [&](const u16x8& v0, const u16x8& v1, const u16x8& v2,
                        const u16x8& v3, const bf16x8& af) {
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          af, *reinterpret_cast<const bf16x8*>(&v0), a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          af, *reinterpret_cast<const bf16x8*>(&v1), a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          af, *reinterpret_cast<const bf16x8*>(&v2), a2, 0, 0, 0);
      a3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          af, *reinterpret_cast<const bf16x8*>(&v3), a3, 0, 0, 0);
    };
    load_set(0, v0a, v1a, v2a, v3a, afa);
    int kt = 0;
    for (; kt + 2 <= nkt; kt += 2) {
      if (kt + 1 < nkt) load_set(kt + 1, v0b, v1b, v2b, v3b, afb);
      mfma_set(v0a, v1a, v2a, v3a, afa);
      if (kt + 2 < nkt) load_set(kt + 2, v0a, v1a, v2a, v3a, afa);
      mfma_set(v0b, v1b, v2b, v3b, afb);
    }
    if (kt < nkt) mfma_set(v0a, v1a, v2a, v3a, afa);  // odd tail
    __syncthreads();  // next slice's buffer fully written AND consumed
  }
  if (iig + 0 < Hc) ncc_epilogue_row<L2>(a0, iig + 0, epi, Pstat, sy, sy2, bestk);
  if (iig + 1 < Hc) ncc_epilogue_row<L2>(a1, iig + 1, epi, Pstat, sy, sy2, bestk);
  if (iig + 2 < Hc) ncc_epilogue_row<L2>(a2, iig + 2, epi, Pstat, sy, sy2, bestk);
  if (iig + 3 < Hc) ncc_epilogue_row<L2>(a3, iig + 3, epi, Pstat, sy, sy2, bestk);

  ncc_merge_best(bestk, best, p0, P, lane);
}

// the four instantiations the host wrapper launches (also what a standalone
// compile of this file emits)
#define NCC_MAIN_ARGS                                                        \
  const bf16*, const bf16*, const unsigned int*, const unsigned short*, \
      const float*, const float*, const float*, const float*,               \
      unsigned long long*, int, int, int, int, int, int, int, int, int, \
      unsigned long long
#define NCC_MAIN_V2_ARGS                                                   \
  const bf16*, const bf16*, const unsigned int*, const float*,        \
      const float*, const float*, const float*, unsigned long long*, int, \
      int, int, int, int, int, int, int, int, unsigned long long
template __global__ void ncc_main_kernel<false>(NCC_MAIN_ARGS);
template __global__ void ncc_main_kernel<true>(NCC_MAIN_ARGS);
template __global__ void ncc_main_v2_kernel<false>(NCC_MAIN_V2_ARGS);
template __global__ void ncc_main_v2_kernel<true>(NCC_MAIN_V2_ARGS);
#undef NCC_MAIN_ARGS
#undef NCC_MAIN_V2_ARGS

// ---------------------------------------------------------------- stage 5

__global__ void scatter_kernel(const unsigned long long* __restrict__ best,
                               const float* __restrict__ y_orig,
                               float* __restrict__ y_syn,
                               long long* __restrict__ rows,
                               long long* __restrict__ cols,
                               int H, int W, int ph, int pw, int gw, int P,
                               int Wc) {
  best += (long long)blockIdx.y * P;
  rows += (long long)blockIdx.y * P;
  cols += (long long)blockIdx.y * P;
  y_orig += (long long)blockIdx.y * 3 * H * W;
  y_syn += (long long)blockIdx.y * 3 * H * W;
  int p = blockIdx.x;
  unsigned int idx = ~(unsigned int)(best[p] & 0xFFFFFFFFull);
  int bi = idx / Wc, bj = idx % Wc;
  if (threadIdx.x == 0) {
    rows[p] = bi;
    cols[p] = bj;
  }
  int pr = (p / gw) * ph, pc = (p % gw) * pw;
  int n = 3 * ph * pw;
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    int c = k / (ph * pw), rem = k % (ph * pw);
    int a = rem / pw, b = rem % pw;
    y_syn[((long long)c * H + pr + a) * W + pc + b] =
        y_orig[((long long)c * H + bi + a) * W + bj + b];
  }
}

}  // namespace dsin
