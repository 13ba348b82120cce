// Fused softmax-cross-entropy bitcost over the L centers dimension.
//
// Mirror of /root/reference/src/probclass_imgcomp.py:100-106:
//   bits[n,c,h,w] = CE(logits[n,:,c,h,w], symbols[n,c,h,w]) * log2(e)
// logits layout (N, L, S) with S = C*H*W flattened spatial+channel sites.
// Backward: dlogits = g * log2e * (softmax(logits) - onehot(sym)).

#include "common.h"

namespace dsin {

constexpr int MAX_LOGITS = 16;
constexpr float LOG2E = 1.4426950408889634f;

__global__ void bitcost_ce_fwd_kernel(const float* __restrict__ logits,
                                      const int64_t* __restrict__ symbols,
                                      float* __restrict__ bits,
                                      int L, int64_t S, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int64_t n = i / S, s = i % S;
    const float* lg = logits + (n * L) * S + s;
    float m = -1e30f;
#pragma unroll 8
    for (int l = 0; l < L; ++l) m = fmaxf(m, lg[l * S]);
    float denom = 0.f;
#pragma unroll 8
    for (int l = 0; l < L; ++l) denom += __expf(lg[l * S] - m);
    int sym = (int)symbols[i];
    // CE = logsumexp - logit[sym]
    bits[i] = (logf(denom) + m - lg[sym * S]) * LOG2E;
  }
}

__global__ void bitcost_ce_bwd_kernel(const float* __restrict__ g,
                                      const float* __restrict__ logits,
                                      const int64_t* __restrict__ symbols,
                                      float* __restrict__ glogits,
                                      int L, int64_t S, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int64_t n = i / S, s = i % S;
    const float* lg = logits + (n * L) * S + s;
    float* gl = glogits + (n * L) * S + s;
    float m = -1e30f;
#pragma unroll 8
    for (int l = 0; l < L; ++l) m = fmaxf(m, lg[l * S]);
    float denom = 0.f;
    float e[MAX_LOGITS];
#pragma unroll 8
    for (int l = 0; l < L; ++l) { e[l] = __expf(lg[l * S] - m); denom += e[l]; }
    float inv = 1.f / denom;
    int sym = (int)symbols[i];
    float gi = g[i] * LOG2E;
#pragma unroll 8
    for (int l = 0; l < L; ++l)
      gl[l * S] = gi * (e[l] * inv - (l == sym ? 1.f : 0.f));
  }
}

// the checks both directions make: fp32 (N, L, C, H, W) logits of at most
// MAX_LOGITS classes and one int64 symbol per site
struct BitcostGeom {
  int L;
  int64_t S, total;  // sites per image, sites
};

static BitcostGeom bitcost_geom(const std::string& op,
                                const torch::Tensor& logits,
                                const torch::Tensor& symbols) {
  check_arg(logits, (op + ": logits").c_str(), torch::kFloat32);
  TORCH_CHECK(logits.dim() == 5, "logits must be (N, L, C, H, W)");
  int64_t N = logits.size(0), L = logits.size(1);
  TORCH_CHECK(L <= MAX_LOGITS, "at most ", MAX_LOGITS, " logit classes");
  int64_t S = logits.numel() / (N * L);
  check_arg(symbols, (op + ": symbols").c_str(), torch::kInt64);
  TORCH_CHECK(symbols.numel() == N * S, "symbols shape mismatch");
  return {(int)L, S, N * S};
}

torch::Tensor bitcost_ce_fwd(torch::Tensor logits, torch::Tensor symbols) {
  const BitcostGeom q = bitcost_geom("bitcost_ce_fwd", logits, symbols);
  auto bits = torch::empty(symbols.sizes(), logits.options());
  hipLaunchKernelGGL(bitcost_ce_fwd_kernel, dim3(ew_grid(q.total)),
                     dim3(BLOCK_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(),
                     logits.data_ptr<float>(), symbols.data_ptr<int64_t>(),
                     bits.data_ptr<float>(), q.L, q.S, q.total);
  return bits;
}

torch::Tensor bitcost_ce_bwd(torch::Tensor g, torch::Tensor logits,
                             torch::Tensor symbols) {
  const BitcostGeom q = bitcost_geom("bitcost_ce_bwd", logits, symbols);
  check_arg_numel(g, "bitcost_ce_bwd: g", torch::kFloat32, q.total);
  auto glogits = torch::empty_like(logits);
  const int L = q.L;
  const int64_t S = q.S, total = q.total;
  hipLaunchKernelGGL(bitcost_ce_bwd_kernel, dim3(ew_grid(total)),
                     dim3(BLOCK_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(),
                     g.data_ptr<float>(), logits.data_ptr<float>(),
                     symbols.data_ptr<int64_t>(), glogits.data_ptr<float>(),
                     (int)L, S, total);
  return glogits;
}

}  // namespace dsin
