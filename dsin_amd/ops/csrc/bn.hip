// Fused batch-norm (+activation) kernel family, v2.
//
// torch.nn.BatchNorm2d semantics: normalize with the BIASED batch variance,
// running_var updated with the UNBIASED variance,
// running = (1-momentum)*running + momentum*batch. bf16 data, fp32 stats.
//
// Layout-aware: NCHW is channel-major, so every kernel runs a 2D grid
// (spatial chunks x B*C) — the channel index is one divide per BLOCK and
// all loads are 16B-vectorized.
//
//  bn_stats_part -> bn_finalize: per-channel mean/rstd (+EMA, scale/shift)
//  bn_apply:       out = act(scale*y + shift)
//  bn_bwd_part:    per-channel sum(dy_eff), sum(dy_eff*xhat), act' inline
//  bn_bwd_apply:   dx = gamma*rstd*(dy_eff - s1/n - xhat*s2/n)
//
// Each kernel walks its row in 8-wide vectors and lets the first block take
// the HW % 8 tail one element per thread; the per-element arithmetic of both
// is one of the four bn_* functions below.

#include "common.h"

namespace dsin {

// statistics: (sum, sum of squares)
__device__ __forceinline__ void bn_stat(float f, float (&acc)[2]) {
  acc[0] += f;
  acc[1] += f * f;
}

// out = act(scale*y + shift (+ res))
__device__ __forceinline__ float bn_apply(float y, float sc, float sh,
                                          bool has_res, float res, int act) {
  float f = y * sc + sh;
  if (has_res) f += res;
  return act_fwd(f, act);
}

// backward sums: (sum dy_eff, sum dy_eff*xhat), dy_eff = dy * act'(out)
__device__ __forceinline__ void bn_bwd_stat(float dy, float y, float out,
                                            float m, float rs, int act,
                                            float (&acc)[2]) {
  const float g = act_grad(dy, out, act);
  acc[0] += g;
  acc[1] += g * (y - m) * rs;
}

// dx; t1, t2 are the two backward sums over n
__device__ __forceinline__ float bn_dx(float dy, float y, float out, float m,
                                       float rs, float gm, float t1, float t2,
                                       int act, int training) {
  const float g = act_grad(dy, out, act);
  if (!training) return gm * rs * g;
  const float xh = (y - m) * rs;
  return gm * rs * (g - t1 - xh * t2);
}

// the 16-byte run at p[i..i+7]
__device__ __forceinline__ u16x8 bn_ld8(const bf16* p, long long i) {
  return *reinterpret_cast<const u16x8*>(&p[i]);
}

__global__ void bn_stats_part_kernel(const bf16* __restrict__ y,
                                     float* __restrict__ psum,   // (S, C)
                                     float* __restrict__ psum2,  // (S, C)
                                     int C, long long HW, int B, int S) {
  const int c = blockIdx.y;
  const int sidx = blockIdx.x;
  float acc[2] = {0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    const bf16* p = y + ((long long)b * C + c) * HW;
    long long i0 = (long long)(sidx * (int)blockDim.x + threadIdx.x) * 8;
    long long stride = (long long)S * blockDim.x * 8;
    for (long long i = i0; i + 7 < HW; i += stride) {
      const u16x8 v = bn_ld8(p, i);
#pragma unroll
      for (int k = 0; k < 8; ++k) bn_stat(b2f(v[k]), acc);
    }
    if (sidx == 0 && threadIdx.x < (HW & 7))  // tail
      bn_stat(b2f(p[(HW & ~7LL) + threadIdx.x]), acc);
  }
  const float* ws = block_wave_sums(acc);
  // per-slice plain stores into (S, C) partials: no atomics, and the
  // buffers need no zero-fill kernel (two fills per BN call was ~0.6 ms
  // per training step); bn_finalize sums the S slices.
  if (threadIdx.x == 0) {
    psum[sidx * C + c] = sum4_serial(ws);
    psum2[sidx * C + c] = sum4_serial(ws + BLOCK_WAVES);
  }
}

// Applies the normalization AND derives scale/shift in-block from the
// (S, C) partial sums (train) or the running stats (eval): the separate
// bn_finalize launch (one tiny kernel per BN call, ~0.6 ms/step across the
// model) is gone. The first block of each channel also publishes
// mean/rstd for the backward and advances the EMA running stats.
__global__ void bn_apply_kernel(const bf16* __restrict__ y,
                                const bf16* __restrict__ res,  // or null
                                bf16* __restrict__ out,
                                const float* __restrict__ psum,  // (S,C)|null
                                const float* __restrict__ psum2,
                                const float* __restrict__ gamma,
                                const float* __restrict__ beta,
                                float* __restrict__ mean_out,
                                float* __restrict__ rstd_out,
                                float* __restrict__ rmean,
                                float* __restrict__ rvar,
                                int C, long long HW, int S, float n,
                                float momentum, float eps, int training,
                                int act) {
  const int bc = blockIdx.y;
  const int c = bc % C;
  float m, rs;
  if (training) {
    float t1 = 0.f, t2 = 0.f;
    for (int sdx = 0; sdx < S; ++sdx) {
      t1 += psum[sdx * C + c];
      t2 += psum2[sdx * C + c];
    }
    m = t1 / n;
    const float var = fmaxf(t2 / n - m * m, 0.f);
    rs = rsqrtf(var + eps);
    if (blockIdx.x == 0 && bc < C && threadIdx.x == 0) {
      mean_out[c] = m;
      rstd_out[c] = rs;
      const float unbias = (n > 1.f) ? var * n / (n - 1.f) : var;
      rmean[c] = (1.f - momentum) * rmean[c] + momentum * m;
      rvar[c] = (1.f - momentum) * rvar[c] + momentum * unbias;
    }
  } else {
    m = rmean[c];
    rs = rsqrtf(rvar[c] + eps);
    if (blockIdx.x == 0 && bc < C && threadIdx.x == 0) {
      mean_out[c] = m;
      rstd_out[c] = rs;
    }
  }
  const float sc = gamma[c] * rs, sh = beta[c] - m * sc;
  const bf16* p = y + (long long)bc * HW;
  const bf16* q = res ? res + (long long)bc * HW : nullptr;
  bf16* o = out + (long long)bc * HW;
  long long i0 = (long long)(blockIdx.x * blockDim.x + threadIdx.x) * 8;
  long long stride = (long long)gridDim.x * blockDim.x * 8;
  for (long long i = i0; i + 7 < HW; i += stride) {
    const u16x8 v = bn_ld8(p, i);
    u16x8 rv;
    if (q) rv = bn_ld8(q, i);
    u16x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      r[k] = f2bits(
          bn_apply(b2f(v[k]), sc, sh, q != nullptr, q ? b2f(rv[k]) : 0.f, act));
    *reinterpret_cast<u16x8*>(&o[i]) = r;
  }
  if (blockIdx.x == 0 && threadIdx.x < (HW & 7)) {
    long long j = (HW & ~7LL) + threadIdx.x;
    o[j] = f2b(
        bn_apply(b2f(p[j]), sc, sh, q != nullptr, q ? b2f(q[j]) : 0.f, act));
  }
}

__global__ void bn_bwd_part_kernel(const bf16* __restrict__ dy,
                                   const bf16* __restrict__ y,
                                   const bf16* __restrict__ out,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   float* __restrict__ s1,
                                   float* __restrict__ s2,
                                   int C, long long HW, int B, int S,
                                   int act) {
  const int c = blockIdx.y;
  const int sidx = blockIdx.x;
  const float m = mean[c], rs = rstd[c];
  float acc[2] = {0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    const long long base = ((long long)b * C + c) * HW;
    long long i0 = (long long)(sidx * (int)blockDim.x + threadIdx.x) * 8;
    long long stride = (long long)S * blockDim.x * 8;
    for (long long i = i0; i + 7 < HW; i += stride) {
      const u16x8 gv = bn_ld8(dy, base + i);
      const u16x8 yv = bn_ld8(y, base + i);
      const u16x8 ov = bn_ld8(out, base + i);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        bn_bwd_stat(b2f(gv[k]), b2f(yv[k]), b2f(ov[k]), m, rs, act, acc);
    }
    if (sidx == 0 && threadIdx.x < (HW & 7)) {
      long long j = base + (HW & ~7LL) + threadIdx.x;
      bn_bwd_stat(b2f(dy[j]), b2f(y[j]), b2f(out[j]), m, rs, act, acc);
    }
  }
  const float* ws = block_wave_sums(acc);
  // plain per-slice stores (deterministic: the host reduces the (S, C)
  // partials with one ordered at::sum — fp32 atomicAdd order varies
  // between runs and was the one nondeterminism in the BN backward)
  if (threadIdx.x == 0) {
    s1[(long long)sidx * C + c] = sum4_serial(ws);
    s2[(long long)sidx * C + c] = sum4_serial(ws + BLOCK_WAVES);
  }
}

__global__ void bn_bwd_apply_kernel(const bf16* __restrict__ dy,
                                    const bf16* __restrict__ y,
                                    const bf16* __restrict__ out,
                                    bf16* __restrict__ dx,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ rstd,
                                    const float* __restrict__ gamma,
                                    const float* __restrict__ s1,
                                    const float* __restrict__ s2,
                                    int C, long long HW, float invn, int act,
                                    int training) {
  const int bc = blockIdx.y;
  const int c = bc % C;
  const float m = mean[c], rs = rstd[c], gm = gamma[c];
  const float t1 = s1[c] * invn, t2 = s2[c] * invn;
  const long long base = (long long)bc * HW;
  long long i0 = (long long)(blockIdx.x * blockDim.x + threadIdx.x) * 8;
  long long stride = (long long)gridDim.x * blockDim.x * 8;
  for (long long i = i0; i + 7 < HW; i += stride) {
    const u16x8 gv = bn_ld8(dy, base + i);
    const u16x8 ov = bn_ld8(out, base + i);
    const u16x8 yv = bn_ld8(y, base + i);
    u16x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      r[k] = f2bits(bn_dx(b2f(gv[k]), b2f(yv[k]), b2f(ov[k]), m, rs, gm, t1,
                          t2, act, training));
    *reinterpret_cast<u16x8*>(&dx[base + i]) = r;
  }
  if (blockIdx.x == 0 && threadIdx.x < (HW & 7)) {
    long long j = base + (HW & ~7LL) + threadIdx.x;
    dx[j] = f2b(bn_dx(b2f(dy[j]), b2f(y[j]), b2f(out[j]), m, rs, gm, t1, t2,
                      act, training));
  }
}

// --------------------------------------------------------------- host

static int _spatial_chunks(long long HW) {
  return (int)std::min<long long>(std::max<long long>(HW / (256 * 8), 1), 32);
}

std::vector<torch::Tensor> bn_fwd(torch::Tensor y, torch::Tensor gamma,
                                  torch::Tensor beta, torch::Tensor rmean,
                                  torch::Tensor rvar, double momentum,
                                  double eps, bool training, int64_t act,
                                  c10::optional<torch::Tensor> residual) {
  check_arg(y, "bn_fwd: y", torch::kBFloat16);
  TORCH_CHECK(y.dim() == 4, "bn_fwd: y must be NCHW");
  const int B = (int)y.size(0), C = (int)y.size(1);
  const long long HW = (long long)y.size(2) * y.size(3);
  check_arg_numel(gamma, "bn_fwd: gamma", torch::kFloat32, C);
  check_arg_numel(beta, "bn_fwd: beta", torch::kFloat32, C);
  check_arg_numel(rmean, "bn_fwd: rmean", torch::kFloat32, C);
  check_arg_numel(rvar, "bn_fwd: rvar", torch::kFloat32, C);
  if (residual.has_value())
    check_arg_shape(*residual, "bn_fwd: residual", torch::kBFloat16,
                    y.sizes());
  auto optsF = y.options().dtype(torch::kFloat32);
  auto mean = torch::empty({C}, optsF);
  auto rstd = torch::empty({C}, optsF);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int S = _spatial_chunks(HW);
  float* psum = nullptr;
  float* psum2 = nullptr;
  torch::Tensor parts;
  if (training) {
    parts = torch::empty({2, S, C}, optsF);  // written fully: no fill
    psum = parts.data_ptr<float>();
    psum2 = psum + (long long)S * C;
    hipLaunchKernelGGL(bn_stats_part_kernel, dim3(S, C), dim3(BLOCK_THREADS),
                       0, stream, ptr<const bf16>(y), psum, psum2, C, HW, B,
                       S);
  }
  auto out = torch::empty_like(y);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(S, B * C), dim3(BLOCK_THREADS), 0,
                     stream, ptr<const bf16>(y),
                     residual.has_value() ? ptr<const bf16>(*residual)
                                          : nullptr,
                     ptr<bf16>(out), psum, psum2, gamma.data_ptr<float>(),
                     beta.data_ptr<float>(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), rmean.data_ptr<float>(),
                     rvar.data_ptr<float>(), C, HW, S,
                     (float)((long long)B * HW), (float)momentum, (float)eps,
                     training ? 1 : 0, (int)act);
  return {out, mean, rstd};
}

std::vector<torch::Tensor> bn_bwd(torch::Tensor dy, torch::Tensor y,
                                  torch::Tensor out, torch::Tensor mean,
                                  torch::Tensor rstd, torch::Tensor gamma,
                                  bool training, int64_t act) {
  check_arg(y, "bn_bwd: y", torch::kBFloat16);
  TORCH_CHECK(y.dim() == 4, "bn_bwd: y must be NCHW");
  const int B = (int)y.size(0), C = (int)y.size(1);
  const long long HW = (long long)y.size(2) * y.size(3);
  check_arg_shape(dy, "bn_bwd: dy", torch::kBFloat16, y.sizes());
  check_arg_shape(out, "bn_bwd: out", torch::kBFloat16, y.sizes());
  check_arg_numel(mean, "bn_bwd: mean", torch::kFloat32, C);
  check_arg_numel(rstd, "bn_bwd: rstd", torch::kFloat32, C);
  check_arg_numel(gamma, "bn_bwd: gamma", torch::kFloat32, C);
  auto optsF = y.options().dtype(torch::kFloat32);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int S = _spatial_chunks(HW);
  // (2, S, C) plain-store partials -> one ordered sum (deterministic)
  auto parts = torch::empty({2, S, C}, optsF);
  hipLaunchKernelGGL(bn_bwd_part_kernel, dim3(S, C), dim3(BLOCK_THREADS), 0,
                     stream, ptr<const bf16>(dy), ptr<const bf16>(y),
                     ptr<const bf16>(out), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), parts[0].data_ptr<float>(),
                     parts[1].data_ptr<float>(), C, HW, B, S, (int)act);
  auto sbuf = parts.sum(1);  // (2, C), contiguous
  auto s1 = sbuf[0];
  auto s2 = sbuf[1];
  auto dx = torch::empty_like(y);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(_spatial_chunks(HW), B * C),
                     dim3(BLOCK_THREADS), 0, stream, ptr<const bf16>(dy),
                     ptr<const bf16>(y), ptr<const bf16>(out), ptr<bf16>(dx),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     gamma.data_ptr<float>(), s1.data_ptr<float>(),
                     s2.data_ptr<float>(), C, HW, 1.f / (float)(B * HW),
                     (int)act, training ? 1 : 0);
  // dgamma = s2, dbeta = s1
  return {dx, s2, s1};
}

}  // namespace dsin
