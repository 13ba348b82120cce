// Stand-alone check of the portable context model and the range-coder step
// functions on the host, meant to be built with sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined -I dsin_amd/ops/csrc
//       tools/pc_model_check.cpp -o pc_model_check && ./pc_model_check
//
// It includes nothing of the project but pc_model.h and rc_coder.h. It
// checks pexp (end points, cut-off, relative error against double exp),
// the table rule (minimum, total, the non-finite row), then encodes a small
// symbol volume position by position in raster order (which is causal) and
// decodes it back the way the decoder must: tables from the symbols decoded
// so far. Exit status 0 and a last line "ok" on success.

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pc_model.h"
#include "rc_coder.h"

using namespace dsin;

static uint32_t g_seed = 12345u;
static float urand() {  // [-1, 1)
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) / 8388608.0f - 1.0f;
}

static int fail(const char* what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

static int check_pexp() {
  if (pc::pexp(0.f) != 1.0f || pc::pexp(-0.f) != 1.0f) return fail("pexp(0)");
  if (pc::pexp(-87.5f) != 0.f) return fail("pexp below the cut-off");
  if (pc::pexp(-std::numeric_limits<float>::infinity()) != 0.f)
    return fail("pexp(-inf)");
  if (pc::pexp(std::numeric_limits<float>::quiet_NaN()) != 0.f)
    return fail("pexp(NaN)");
  double worst = 0.0;
  for (int i = 0; i <= 2000000; ++i) {
    const float x = -87.0f * (float)i / 2000000.0f;
    const double got = pc::pexp(x), want = std::exp((double)x);
    const double rel = std::fabs(got / want - 1.0);
    if (rel > worst) worst = rel;
  }
  std::printf("pexp: max relative error %.3e over [-87, 0]\n", worst);
  return worst <= 1.2e-7 ? 0 : fail("pexp relative error above 1.2e-7");
}

static int check_tables() {
  for (int L : {2, 6, 16}) {
    for (float scale : {1.f, 8.f, 40.f, 1e30f}) {
      for (int it = 0; it < 20000; ++it) {
        float lg[pc::MAX_L];
        int32_t f[pc::MAX_L];
        for (int l = 0; l < L; ++l) lg[l] = scale * urand();
        pc::table_row(lg, L, f);
        int64_t tot = 0;
        for (int l = 0; l < L; ++l) {
          if (f[l] < 1) return fail("table entry below 1");
          tot += f[l];
        }
        if (tot > 65535) return fail("table total above 65535");
      }
    }
    float lg[pc::MAX_L];
    int32_t f[pc::MAX_L];
    for (int l = 0; l < L; ++l) lg[l] = (float)l;
    lg[L - 1] = std::numeric_limits<float>::infinity();
    pc::table_row(lg, L, f);
    for (int l = 0; l < L; ++l)
      if (f[l] != (65536 - L) / L) return fail("non-finite row not uniform");
  }
  return 0;
}

template <class Fma>
static int roundtrip(int k, int L, int C, int H, int W, float w3_scale) {
  std::vector<float> wts(pc::packed_numel(k, L));
  for (auto& v : wts) v = 0.3f * urand();
  const pc::Weights p = pc::unpack(wts.data(), k, L);
  // padded output channels hold zeros, as ops.pc_pack_weights writes them
  float* wm = wts.data();
  for (int t = 0; t < pc::NT_FIRST + 1; ++t)  // w0 rows and b0
    for (int co = k; co < p.kp; ++co) wm[t * p.kp + co] = 0.f;
  for (const float* base : {p.w1, p.w2}) {
    float* b = wm + (base - wts.data());
    for (int r = 0; r < pc::NT_OTHER * k + 1; ++r)  // rows and the bias
      for (int co = k; co < p.kp; ++co) b[r * p.kp + co] = 0.f;
  }
  for (int i = 0; i < pc::NT_OTHER * k * L; ++i)
    wm[(p.w3 - wts.data()) + i] *= w3_scale;

  std::vector<float> centers(L);
  for (int l = 0; l < L; ++l) centers[l] = -2.f + 4.f * l / (L - 1);
  const int Hp = H + 8, Wp = W + 8, n = C * H * W;
  std::vector<int> syms(n);
  for (auto& s : syms) s = (int)((urand() + 1.f) * 0.5f * L) % L;
  std::vector<float> q((size_t)(C + 4) * Hp * Wp, centers[0]);
  auto at = [&](int c, int h, int w) -> float& {
    return q[((size_t)(c + 4) * Hp + (h + 4)) * Wp + (w + 4)];
  };
  for (int c = 0, i = 0; c < C; ++c)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w, ++i) at(c, h, w) = centers[syms[i]];

  pc::Scratch scratch;
  float lg[pc::MAX_L];
  int32_t f[pc::MAX_L];
  uint32_t cum[rc::MAX_L + 1];
  std::vector<uint8_t> buf(3 * (size_t)n + 16);
  rc::State st;
  rc::init(st);
  const rc::ByteSink sink{buf.data(), buf.size()};
  for (int c = 0, i = 0; c < C; ++c)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w, ++i) {
        pc::eval_position<Fma>(q.data(), Hp, Wp, c, h, w, p, scratch, lg, f);
        rc::cumulate(f, L, cum);
        if (cum[L] > 65535) return fail("total above 65535 in the roundtrip");
        rc::encode(st, sink, cum[syms[i]], (uint32_t)f[syms[i]], cum[L]);
      }
  rc::finish(st, sink);
  if (st.pos > buf.size()) return fail("encoder overran its buffer");
  const uint64_t len = st.pos;

  std::vector<float> q2((size_t)(C + 4) * Hp * Wp, centers[0]);
  const rc::ByteSource src{buf.data(), len};
  rc::decode_start(st, src);
  for (int c = 0, i = 0; c < C; ++c)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w, ++i) {
        pc::eval_position<Fma>(q2.data(), Hp, Wp, c, h, w, p, scratch, lg, f);
        rc::cumulate(f, L, cum);
        const int s = rc::decode_cum(st, src, cum, L);
        if (s != syms[i]) return fail("decoded symbol differs");
        q2[((size_t)(c + 4) * Hp + (h + 4)) * Wp + (w + 4)] = centers[s];
      }
  std::printf("roundtrip k=%d L=%d %dx%dx%d scale %g: %llu bytes\n", k, L, C,
              H, W, (double)w3_scale, (unsigned long long)len);
  return 0;
}

int main() {
  if (check_pexp()) return 1;
  if (check_tables()) return 1;
  if (roundtrip<pc::FmaLibm>(8, 6, 3, 5, 6, 1.f)) return 1;
  if (roundtrip<pc::FmaBuiltin>(20, 16, 2, 3, 4, 1.f)) return 1;
  if (roundtrip<pc::FmaLibm>(32, 2, 1, 2, 7, 40.f)) return 1;
  std::printf("ok\n");
  return 0;
}
