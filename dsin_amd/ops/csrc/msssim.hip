// Fused fp32 MS-SSIM loss kernels (docs/KERNELS.md K16).
//
// One scale of the differentiable MS-SSIM (losses/msssim.py) is a separable
// VALID Gaussian blur of five maps (a, b, a*a, b*b, a*b) followed by the
// per-pixel ssim / cs expressions and two means. The torch chain launches
// ten convs plus ~20 elementwise kernels per scale; here one kernel per
// scale does all of it out of LDS, and one more computes the analytic
// gradient. Everything accumulates in fp32; inputs are fp32 or bf16, NCHW
// contiguous, planes P = B*C.
//
// * ssim_scale_fwd: one 256-thread workgroup owns a 32x32 tile of the VALID
//   output map, stages the (32+T-1)^2 halo of both images, runs the row pass
//   then the column pass (the order of _blur_sep), evaluates ssim/cs and
//   writes two per-block partial sums with plain stores. The host sums the
//   partials in a fixed order, so the result is bitwise deterministic.
// * ssim_scale_bwd: gather form, one owner per input pixel. The five
//   blurred maps are RECOMPUTED from a halo that is T-1 wider on every side
//   instead of being saved by forward: that keeps ~18 MB of fp32 maps per
//   3x320x960 evaluation out of memory and out of the autograd graph, and
//   costs only LDS-resident FMAs in an op that is launch-bound. (The saved-
//   maps variant was not built, so this is a design choice, not the winner
//   of a measured comparison.)
// * Both images are shifted by -128 before the products are formed and the
//   shift is added back for the luminance terms. Variances are shift
//   invariant, and the smaller magnitudes cut the cancellation in
//   blur(x*x) - blur(x)^2: against an fp64 evaluation the shifted fp32
//   arithmetic is 3-8x closer in the gradient than the unshifted fp32
//   torch path (profiles/r03_msssim.md).
// * down2_fwd / down2_bwd: the dyadic downsample between scales (REFLECT
//   pad 0 front / 1 back, 2-tap box, width then height, ::2) and its exact
//   adjoint, also in gather form.
//
// No atomics, no host synchronisation: every launch goes to the current
// stream, so the whole loss is graph-capturable.

#include "common.h"

namespace dsin {

namespace {

constexpr int MS_TMAX = 11;            // largest supported filter length
constexpr int MS_TILE = 32;            // tile side (fwd: outputs, bwd: inputs)
constexpr int MS_THREADS = 256;
constexpr float MS_SHIFT = 128.f;

// forward LDS: two halos + five row-pass maps  (40 992 B -> 3 blocks / CU)
constexpr int MS_FH = MS_TILE + MS_TMAX - 1;            // 42
constexpr int MS_F_HALO = MS_FH * MS_FH;                // 1764
constexpr int MS_F_ROW = MS_FH * MS_TILE;               // 1344
// backward LDS: region X = two input halos (52x52), reused for the three
// derivative maps (42x42); region Y = five row-pass maps (52x42), reused for
// the vertical pass of the transposed blur (65 312 B -> 2 blocks / CU)
constexpr int MS_BI = MS_TILE + 2 * (MS_TMAX - 1);      // 52
constexpr int MS_BD = MS_TILE + MS_TMAX - 1;            // 42
constexpr int MS_B_X = 2 * MS_BI * MS_BI;               // 5408
constexpr int MS_B_Y = 5 * MS_BI * MS_BD;               // 10920
static_assert(3 * MS_BD * MS_BD <= MS_B_X, "derivative maps must fit in X");
static_assert(3 * MS_TILE * MS_BD <= MS_B_Y, "vertical pass must fit in Y");

// Forward and backward each carry the five-map row pass, the column pass and
// the ssim / cs terms (s11 ... lum), and forward its own block sum, written
// out. They stay so on purpose: hipcc contracts these expressions per
// kernel (forward takes u1*u1 + u2*u2 + c1 as a packed multiply and add,
// backward as an fma; e11 - m1*m1 is an fma in both), and moving any of the
// pieces into a shared function (tried: row pass, column pass, terms, and
// device_common.h's block_wave_sums for the tail) made forward contract
// differently and changed the last bit of its ssim sums
// (profiles/r14_pointwise_device.md).

__device__ __forceinline__ int ms_clamp(int v, int lo, int hi) {
  return min(max(v, lo), hi);
}

// ---------------------------------------------------------------- forward
template <typename TA, typename TB>
__global__ __launch_bounds__(MS_THREADS) void ssim_scale_fwd_kernel(
    const TA* __restrict__ a, const TB* __restrict__ b,
    const float* __restrict__ taps,
    float* __restrict__ parts,  // (2, nblk): row 0 ssim sums, row 1 cs sums
    int H, int W, int T, int tiles_x, int tiles_y, int nblk, float c1,
    float c2) {
  __shared__ float sk[MS_TMAX];
  __shared__ float sA[MS_F_HALO];
  __shared__ float sB[MS_F_HALO];
  __shared__ float sR[5 * MS_F_ROW];
  __shared__ float red[2][MS_THREADS / 64];

  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tx = blk % tiles_x;
  blk /= tiles_x;
  const int ty = blk % tiles_y;
  const int p = blk / tiles_y;
  const int Ho = H - T + 1, Wo = W - T + 1;
  const int y0 = ty * MS_TILE, x0 = tx * MS_TILE;
  const int hh = MS_TILE + T - 1, hw = MS_TILE + T - 1;
  const long long plane = (long long)p * H * W;

  if (tid < T) sk[tid] = taps[tid];
  // halo staging: clamped unconditional loads; positions past the image
  // hold copies of the edge and only feed outputs that are masked below
  for (int i = tid; i < hh * hw; i += MS_THREADS) {
    const int r = i / hw, c = i - r * hw;
    const int gy = min(y0 + r, H - 1), gx = min(x0 + c, W - 1);
    const long long o = plane + (long long)gy * W + gx;
    sA[i] = ld_f32(a, o) - MS_SHIFT;
    sB[i] = ld_f32(b, o) - MS_SHIFT;
  }
  __syncthreads();

  // row pass (along W) of the five maps
  for (int i = tid; i < hh * MS_TILE; i += MS_THREADS) {
    const int r = i / MS_TILE, c = i % MS_TILE;
    const float* pa = sA + r * hw + c;
    const float* pb = sB + r * hw + c;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
    for (int t = 0; t < T; ++t) {
      const float k = sk[t], av = pa[t], bv = pb[t];
      m1 = fmaf(k, av, m1);
      m2 = fmaf(k, bv, m2);
      e11 = fmaf(k, av * av, e11);
      e22 = fmaf(k, bv * bv, e22);
      e12 = fmaf(k, av * bv, e12);
    }
    sR[0 * MS_F_ROW + i] = m1;
    sR[1 * MS_F_ROW + i] = m2;
    sR[2 * MS_F_ROW + i] = e11;
    sR[3 * MS_F_ROW + i] = e22;
    sR[4 * MS_F_ROW + i] = e12;
  }
  __syncthreads();

  // column pass + per-pixel ssim / cs
  float ssum = 0.f, csum = 0.f;
  for (int i = tid; i < MS_TILE * MS_TILE; i += MS_THREADS) {
    const int r = i / MS_TILE, c = i % MS_TILE;
    const float* pr = sR + r * MS_TILE + c;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
    for (int t = 0; t < T; ++t) {
      const float k = sk[t];
      const float* q = pr + t * MS_TILE;
      m1 = fmaf(k, q[0 * MS_F_ROW], m1);
      m2 = fmaf(k, q[1 * MS_F_ROW], m2);
      e11 = fmaf(k, q[2 * MS_F_ROW], e11);
      e22 = fmaf(k, q[3 * MS_F_ROW], e22);
      e12 = fmaf(k, q[4 * MS_F_ROW], e12);
    }
    const float s11 = e11 - m1 * m1;
    const float s22 = e22 - m2 * m2;
    const float s12 = e12 - m1 * m2;
    const float u1 = m1 + MS_SHIFT, u2 = m2 + MS_SHIFT;
    const float v1 = 2.f * s12 + c2;
    const float v2 = s11 + s22 + c2;
    const float cs = v1 / v2;
    const float lum = (2.f * u1 * u2 + c1) / (u1 * u1 + u2 * u2 + c1);
    const bool ok = (y0 + r < Ho) && (x0 + c < Wo);
    ssum += ok ? lum * cs : 0.f;
    csum += ok ? cs : 0.f;
  }
  ssum = wave_reduce_sum(ssum);
  csum = wave_reduce_sum(csum);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = ssum;
    red[1][tid >> 6] = csum;
  }
  __syncthreads();
  if (tid == 0) {
    parts[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    parts[(long long)nblk + blockIdx.x] =
        (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// --------------------------------------------------------------- backward
// Gradient w.r.t. `b` of  g_ssim * mean(ssim) + g_cs * mean(cs); the
// expressions are symmetric in (a, b), so the gradient w.r.t. the first
// image is the same kernel with the two images swapped.
//
// With a' = a - 128, b' = b - 128, primes for the shifted blurred maps and
// u = m' + 128 for the true means:
//   wc = gs * lum + gc,  wl = gs * cs          (gs, gc already / N)
//   D12 = 2 wc / v2                            d/d blur(a'b')
//   DV  = -wc cs / v2                          d/d blur(b'b')
//   DM  = -m1' D12 - 2 m2' DV + 2 wl (u1 - lum u2) / (u1^2 + u2^2 + c1)
//   grad_b = blurT(DM) + 2 b' blurT(DV) + a' blurT(D12)
// blurT is the transposed separable blur (full correlation) and the D maps
// are zero outside the VALID output map.
template <typename TA, typename TB>
__global__ __launch_bounds__(MS_THREADS) void ssim_scale_bwd_kernel(
    const TA* __restrict__ a, const TB* __restrict__ b,
    const float* __restrict__ taps,
    const float* __restrict__ g_ssim,  // scalar, nullable (= 0)
    const float* __restrict__ g_cs,    // scalar, nullable (= 0)
    TB* __restrict__ gb, int H, int W, int T, int tiles_x, int tiles_y,
    float inv_n, float c1, float c2) {
  __shared__ float sk[MS_TMAX];
  __shared__ float sX[MS_B_X];
  __shared__ float sY[MS_B_Y];

  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tx = blk % tiles_x;
  blk /= tiles_x;
  const int ty = blk % tiles_y;
  const int p = blk / tiles_y;
  const int Ho = H - T + 1, Wo = W - T + 1;
  const int y0 = ty * MS_TILE, x0 = tx * MS_TILE;
  const int ih = MS_TILE + 2 * (T - 1), iw = ih;  // input halo
  const int dh = MS_TILE + T - 1, dw = dh;        // derivative-map region
  const int oy0 = y0 - (T - 1), ox0 = x0 - (T - 1);
  const long long plane = (long long)p * H * W;
  const float gs = (g_ssim ? g_ssim[0] : 0.f) * inv_n;
  const float gc = (g_cs ? g_cs[0] : 0.f) * inv_n;

  if (tid < T) sk[tid] = taps[tid];
  float* sA = sX;
  float* sB = sX + ih * iw;
  for (int i = tid; i < ih * iw; i += MS_THREADS) {
    const int r = i / iw, c = i - r * iw;
    const int gy = ms_clamp(oy0 + r, 0, H - 1);
    const int gx = ms_clamp(ox0 + c, 0, W - 1);
    const long long o = plane + (long long)gy * W + gx;
    sA[i] = ld_f32(a, o) - MS_SHIFT;
    sB[i] = ld_f32(b, o) - MS_SHIFT;
  }
  __syncthreads();

  // row pass: ih rows x dw columns of the five maps -> Y
  const int rs = ih * dw;
  for (int i = tid; i < rs; i += MS_THREADS) {
    const int r = i / dw, c = i - r * dw;
    const float* pa = sA + r * iw + c;
    const float* pb = sB + r * iw + c;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
    for (int t = 0; t < T; ++t) {
      const float k = sk[t], av = pa[t], bv = pb[t];
      m1 = fmaf(k, av, m1);
      m2 = fmaf(k, bv, m2);
      e11 = fmaf(k, av * av, e11);
      e22 = fmaf(k, bv * bv, e22);
      e12 = fmaf(k, av * bv, e12);
    }
    sY[0 * rs + i] = m1;
    sY[1 * rs + i] = m2;
    sY[2 * rs + i] = e11;
    sY[3 * rs + i] = e22;
    sY[4 * rs + i] = e12;
  }
  __syncthreads();

  // column pass + derivatives w.r.t. the blurred maps -> X (halos are dead)
  const int ds = dh * dw;
  for (int i = tid; i < ds; i += MS_THREADS) {
    const int r = i / dw, c = i - r * dw;
    const float* pr = sY + r * dw + c;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
    for (int t = 0; t < T; ++t) {
      const float k = sk[t];
      const float* q = pr + t * dw;
      m1 = fmaf(k, q[0 * rs], m1);
      m2 = fmaf(k, q[1 * rs], m2);
      e11 = fmaf(k, q[2 * rs], e11);
      e22 = fmaf(k, q[3 * rs], e22);
      e12 = fmaf(k, q[4 * rs], e12);
    }
    const float s11 = e11 - m1 * m1;
    const float s22 = e22 - m2 * m2;
    const float s12 = e12 - m1 * m2;
    const float u1 = m1 + MS_SHIFT, u2 = m2 + MS_SHIFT;
    const float v1 = 2.f * s12 + c2;
    const float v2 = s11 + s22 + c2;
    const float cs = v1 / v2;
    const float den = u1 * u1 + u2 * u2 + c1;
    const float lum = (2.f * u1 * u2 + c1) / den;
    const float wc = gs * lum + gc;
    const float wl = gs * cs;
    const float d12 = 2.f * wc / v2;
    const float dv = -wc * cs / v2;
    const float dm =
        -m1 * d12 - 2.f * m2 * dv + 2.f * wl * (u1 - lum * u2) / den;
    const int oy = oy0 + r, ox = ox0 + c;
    const bool ok = oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
    sX[0 * ds + i] = ok ? dm : 0.f;
    sX[1 * ds + i] = ok ? dv : 0.f;
    sX[2 * ds + i] = ok ? d12 : 0.f;
  }
  __syncthreads();

  // transposed blur, vertical pass: MS_TILE rows x dw columns -> Y
  const int vs = MS_TILE * dw;
  for (int i = tid; i < vs; i += MS_THREADS) {
    const int r = i / dw, c = i - r * dw;
    const float* pd = sX + (r + T - 1) * dw + c;
    float x0v = 0.f, x1v = 0.f, x2v = 0.f;
    for (int t = 0; t < T; ++t) {
      const float k = sk[t];
      const float* q = pd - t * dw;
      x0v = fmaf(k, q[0 * ds], x0v);
      x1v = fmaf(k, q[1 * ds], x1v);
      x2v = fmaf(k, q[2 * ds], x2v);
    }
    sY[0 * vs + i] = x0v;
    sY[1 * vs + i] = x1v;
    sY[2 * vs + i] = x2v;
  }
  __syncthreads();

  // horizontal pass + combine; one owner per input pixel, plain stores
  for (int i = tid; i < MS_TILE * MS_TILE; i += MS_THREADS) {
    const int r = i / MS_TILE, c = i % MS_TILE;
    const float* pv = sY + r * dw + c + T - 1;
    float gm = 0.f, gv = 0.f, g12 = 0.f;
    for (int t = 0; t < T; ++t) {
      const float k = sk[t];
      gm = fmaf(k, pv[0 * vs - t], gm);
      gv = fmaf(k, pv[1 * vs - t], gv);
      g12 = fmaf(k, pv[2 * vs - t], g12);
    }
    const int y = y0 + r, x = x0 + c;
    const long long o =
        plane + (long long)min(y, H - 1) * W + min(x, W - 1);
    const float av = ld_f32(a, o) - MS_SHIFT;
    const float bv = ld_f32(b, o) - MS_SHIFT;
    const float g = gm + 2.f * bv * gv + av * g12;
    if (y < H && x < W) st_f32(gb, o, g);
  }
}

// ------------------------------------------------------------- downsample
// out[oy][ox] = 0.5 * (0.5 x[y0][x0] + 0.5 x[y0][x1])
//             + 0.5 * (0.5 x[y1][x0] + 0.5 x[y1][x1])
// with y0 = 2 oy, y1 = 2 oy + 1 reflected to H - 2 when it equals H.
template <typename T>
__global__ void down2_fwd_kernel(const T* __restrict__ x,
                                 float* __restrict__ out, int H, int W,
                                 int Ho, int Wo, long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long gstride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += gstride) {
    const int ox = (int)(i % Wo);
    const long long q = i / Wo;
    const int oy = (int)(q % Ho);
    const long long p = q / Ho;
    const int xa = 2 * ox, ya = 2 * oy;
    const int xb = (xa + 1 < W) ? xa + 1 : W - 2;
    const int yb = (ya + 1 < H) ? ya + 1 : H - 2;
    const long long base = p * H * W;
    const float h0 = 0.5f * ld_f32(x, base + (long long)ya * W + xa) +
                     0.5f * ld_f32(x, base + (long long)ya * W + xb);
    const float h1 = 0.5f * ld_f32(x, base + (long long)yb * W + xa) +
                     0.5f * ld_f32(x, base + (long long)yb * W + xb);
    out[i] = 0.5f * h0 + 0.5f * h1;
  }
}

// exact adjoint: input index i feeds output i >> 1 and, when the length is
// odd and i == len - 2, also the last output (the reflected tap)
template <typename T>
__global__ void down2_bwd_kernel(const float* __restrict__ g,
                                 T* __restrict__ gx, int H, int W, int Ho,
                                 int Wo, long long total) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long gstride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += gstride) {
    const int xx = (int)(i % W);
    const long long q = i / W;
    const int yy = (int)(q % H);
    const long long p = q / H;
    const int oxa = xx >> 1, oya = yy >> 1;
    const bool ex = (W & 1) && xx == W - 2;
    const bool ey = (H & 1) && yy == H - 2;
    const int oxb = Wo - 1, oyb = Ho - 1;
    const float* gp = g + p * Ho * Wo;
    const float gaa = gp[(long long)oya * Wo + oxa];
    const float gab = gp[(long long)oya * Wo + oxb];
    const float gba = gp[(long long)oyb * Wo + oxa];
    const float gbb = gp[(long long)oyb * Wo + oxb];
    const float top = gaa + (ex ? gab : 0.f);
    const float bot = gba + (ex ? gbb : 0.f);
    st_f32(gx, i, 0.25f * (top + (ey ? bot : 0.f)));
  }
}

struct MsGeom {
  int P, H, W, T, tiles_x, tiles_y, nblk;
};

MsGeom ms_geom(const torch::Tensor& a, const torch::Tensor& b,
               const torch::Tensor& taps, bool input_tiles) {
  CHECK_CUDA_CONTIG(a);
  CHECK_CUDA_CONTIG(b);
  CHECK_CUDA_CONTIG(taps);
  TORCH_CHECK(a.dim() == 4 && a.sizes() == b.sizes(),
              "ssim_scale: NCHW images of equal shape");
  TORCH_CHECK(taps.dim() == 1 && taps.scalar_type() == torch::kFloat32,
              "ssim_scale: taps must be a 1-D fp32 tensor");
  auto okdt = [](const torch::Tensor& t) {
    return t.scalar_type() == torch::kFloat32 ||
           t.scalar_type() == torch::kBFloat16;
  };
  TORCH_CHECK(okdt(a) && okdt(b), "ssim_scale: images must be fp32 or bf16");
  MsGeom g;
  g.T = (int)taps.numel();
  TORCH_CHECK(a.size(2) < (1 << 30) && a.size(3) < (1 << 30),
              "ssim_scale: image side too large");
  g.H = (int)a.size(2);
  g.W = (int)a.size(3);
  TORCH_CHECK((g.T & 1) && g.T >= 1 && g.T <= MS_TMAX,
              "ssim_scale: taps length must be odd and <= ", MS_TMAX);
  TORCH_CHECK(g.T <= g.H && g.T <= g.W, "ssim_scale: filter of ", g.T,
              " taps does not fit a ", g.H, "x", g.W, " image");
  const long long P = a.size(0) * a.size(1);
  const int eh = input_tiles ? g.H : g.H - g.T + 1;
  const int ew = input_tiles ? g.W : g.W - g.T + 1;
  g.tiles_y = (eh + MS_TILE - 1) / MS_TILE;
  g.tiles_x = (ew + MS_TILE - 1) / MS_TILE;
  const long long nblk = P * g.tiles_y * g.tiles_x;
  TORCH_CHECK(P >= 1 && nblk < (1LL << 31), "ssim_scale: too many tiles");
  g.P = (int)P;
  g.nblk = (int)nblk;
  return g;
}

}  // namespace

// ------------------------------------------------------------------ hosts

torch::Tensor ssim_scale_fwd(torch::Tensor a, torch::Tensor b,
                             torch::Tensor taps, double c1, double c2) {
  const MsGeom g = ms_geom(a, b, taps, false);
  auto parts =
      torch::empty({2, g.nblk}, a.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(a, "ssim_scale_fwd: a", [&](auto ta) {
    dispatch_f32_bf16(b, "ssim_scale_fwd: b", [&](auto tb) {
      using TA = decltype(ta);
      using TB = decltype(tb);
      hipLaunchKernelGGL((ssim_scale_fwd_kernel<TA, TB>), dim3(g.nblk),
                         dim3(MS_THREADS), 0, stream, ptr<const TA>(a),
                         ptr<const TB>(b), taps.data_ptr<float>(),
                         parts.data_ptr<float>(), g.H, g.W, g.T, g.tiles_x,
                         g.tiles_y, g.nblk, (float)c1, (float)c2);
    });
  });
  return parts;
}

std::vector<torch::Tensor> ssim_scale_bwd(
    torch::Tensor a, torch::Tensor b, torch::Tensor taps,
    c10::optional<torch::Tensor> g_ssim, c10::optional<torch::Tensor> g_cs,
    double c1, double c2, bool need_ga, bool need_gb) {
  const MsGeom g = ms_geom(a, b, taps, true);
  auto scalar = [](const c10::optional<torch::Tensor>& t,
                   const char* what) -> const float* {
    if (!t.has_value()) return nullptr;
    check_arg_numel(*t, what, torch::kFloat32, 1);
    return t->data_ptr<float>();
  };
  const float* gs = scalar(g_ssim, "ssim_scale_bwd: g_ssim");
  const float* gc = scalar(g_cs, "ssim_scale_bwd: g_cs");
  const float inv_n = (float)(1.0 / ((double)g.P * (g.H - g.T + 1) *
                                     (g.W - g.T + 1)));
  auto ga = need_ga ? torch::empty_like(a) : torch::Tensor();
  auto gb = need_gb ? torch::empty_like(b) : torch::Tensor();
  auto stream = at::cuda::getCurrentCUDAStream();
  // (other, target): the kernel differentiates w.r.t. its second image
  auto launch = [&](const torch::Tensor& other, const torch::Tensor& target,
                    torch::Tensor& out) {
    dispatch_f32_bf16(other, "ssim_scale_bwd: image", [&](auto to) {
      dispatch_f32_bf16(target, "ssim_scale_bwd: image", [&](auto tt) {
        using TO = decltype(to);
        using TT = decltype(tt);
        hipLaunchKernelGGL((ssim_scale_bwd_kernel<TO, TT>), dim3(g.nblk),
                           dim3(MS_THREADS), 0, stream, ptr<const TO>(other),
                           ptr<const TT>(target), taps.data_ptr<float>(), gs,
                           gc, ptr<TT>(out), g.H, g.W, g.T, g.tiles_x,
                           g.tiles_y, inv_n, (float)c1, (float)c2);
      });
    });
  };
  if (need_gb) launch(a, b, gb);
  // the gradient w.r.t. a swaps the images, and with them the kernel's two
  // element types: the dispatch follows the tensors in the order given here
  if (need_ga) launch(b, a, ga);
  return {ga, gb};
}

torch::Tensor down2_fwd(torch::Tensor x) {
  CHECK_CUDA_CONTIG(x);
  TORCH_CHECK(x.dim() == 4 && x.size(2) >= 2 && x.size(3) >= 2 &&
                  x.size(2) < (1 << 30) && x.size(3) < (1 << 30),
              "downsample2: NCHW with H, W >= 2");
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  auto out = torch::empty({x.size(0), x.size(1), Ho, Wo},
                          x.options().dtype(torch::kFloat32));
  const long long total = out.numel();
  if (total == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(x, "downsample2: x", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((down2_fwd_kernel<T>), dim3(ew_grid(total)),
                       dim3(BLOCK_THREADS), 0, stream, ptr<const T>(x),
                       out.data_ptr<float>(), H, W, Ho, Wo, total);
  });
  return out;
}

torch::Tensor down2_bwd(torch::Tensor g, int64_t H64, int64_t W64,
                        bool bf16_out) {
  CHECK_CUDA_CONTIG(g);
  TORCH_CHECK(g.dim() == 4 && g.scalar_type() == torch::kFloat32,
              "downsample2 backward: fp32 NCHW upstream gradient");
  TORCH_CHECK(H64 >= 2 && W64 >= 2 && H64 < (1 << 30) && W64 < (1 << 30) &&
                  g.size(2) == (H64 + 1) / 2 && g.size(3) == (W64 + 1) / 2,
              "downsample2 backward: gradient shape does not match input");
  const int H = (int)H64, W = (int)W64;
  const int Ho = (int)g.size(2), Wo = (int)g.size(3);
  auto gx = torch::empty(
      {g.size(0), g.size(1), H, W},
      g.options().dtype(bf16_out ? torch::kBFloat16 : torch::kFloat32));
  const long long total = gx.numel();
  if (total == 0) return gx;
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(gx, "downsample2 backward: gx", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((down2_bwd_kernel<T>), dim3(ew_grid(total)),
                       dim3(BLOCK_THREADS), 0, stream, g.data_ptr<float>(),
                       ptr<T>(gx), H, W, Ho, Wo, total);
  });
  return gx;
}

}  // namespace dsin
