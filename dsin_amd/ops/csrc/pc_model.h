// The portable context model (codec backend id 2): everything a gfx950
// kernel and a plain C++ host function must agree on bit for bit. No torch,
// no HIP runtime; raw pointers only. Specification: docs/KERNELS.md,
// "Portable backend".
//
// Every value here comes from correctly rounded fp32 operations (fmaf, add,
// multiply by a constant, round-to-nearest conversion, exact scaling by a
// power of two) and from integer arithmetic. No multiply feeds an add except
// through an explicit fmaf, and contraction is switched off for the file, so
// the two sides cannot fuse differently. fp32 subnormals are kept on both
// sides (the kernels are built with denormal mode 3; the host must not run
// with flush-to-zero set).
//
// pexp / table_max / table_weight / table_sum / table_entry are the same
// source on both sides. The conv chain exists twice: pc_layer in
// pc_codec.hip (LDS, one thread per group of outputs) and eval_position
// below (host, one position per call), which transcribes pc_layer's
// per-output operation order: bias, then fmaf(v, w, acc) over the packed
// taps and over ci inside a tap, then the skip add, then the ReLU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// Forced inlining on the host too: the hardware-FMA host path is this same
// source inlined into a function compiled for a target with FMA.
#if defined(__HIPCC__)
#define PC_HD __host__ __device__ __forceinline__
#else
#define PC_HD inline __attribute__((always_inline))
#endif

namespace dsin {
namespace pc {

constexpr int MAX_K = 32;
constexpr int MAX_L = 16;
constexpr int NT_FIRST = 13;       // live taps of the first (conv0) mask
constexpr int NT_OTHER = 14;       // live taps of the other masks
constexpr int S0 = 4 * 7 * 7;      // conv0 output sites
constexpr int S1 = 3 * 5 * 5;      // res_conv1 output sites
constexpr int S2 = 2 * 3 * 3;      // res_conv2 output sites
constexpr int SIN = 5 * 9 * 9;     // context sites
constexpr uint32_t FREQ_SCALE = 1u << 16;
constexpr float PEXP_CUTOFF = -87.0f;  // pexp(x) == 0 for x < PEXP_CUTOFF

PC_HD uint32_t float_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, sizeof(u));
  return u;
}

PC_HD float bits_float(uint32_t u) {
  float x;
  __builtin_memcpy(&x, &u, sizeof(x));
  return x;
}

PC_HD bool is_finite(float x) {
  return (float_bits(x) & 0x7f800000u) != 0x7f800000u;
}

PC_HD float relu(float r) { return r > 0.f ? r : 0.f; }  // -0.0, NaN -> +0.0

// exp(x) for x <= 0: exactly 1.0f at 0 (either sign), exactly 0.0f below
// PEXP_CUTOFF, for -inf and for NaN; relative error at most 1.2e-7 between
// (7.7e-8 measured over 2M points of [-87, 0]).
// n = rint(x * log2(e)); r = x - n * ln2 with ln2 split in two constants
// (the high one has 9 significant bits, so n * LN2_HI is exact for
// |n| <= 126); exp(r) on |r| <= 0.35 by a degree-6 Horner form with
// c0 = c1 = 1; the result is scaled by 2^n, which is exact because
// exp(-87) > FLT_MIN keeps it normal.
PC_HD float pexp(float x) {
  if (!(x >= PEXP_CUTOFF)) return 0.f;
  if (x > 0.f) x = 0.f;  // not reached from table_sum: d = lg - max <= 0
  const float LOG2E = 1.44269504088896341f;
  const float LN2_HI = 0.693359375f;
  const float LN2_LO = -2.12194440e-4f;
  const float nf = rintf(x * LOG2E);
  float r = __builtin_fmaf(nf, -LN2_HI, x);
  r = __builtin_fmaf(nf, -LN2_LO, r);
  float p = 0x1.6d1b1cp-10f;
  p = __builtin_fmaf(p, r, 0x1.121582p-7f);
  p = __builtin_fmaf(p, r, 0x1.555514p-5f);
  p = __builtin_fmaf(p, r, 0x1.5554d4p-3f);
  p = __builtin_fmaf(p, r, 0.5f);
  p = __builtin_fmaf(p, r, 1.0f);
  p = __builtin_fmaf(p, r, 1.0f);
  const int n = (int)nf;  // in [-126, 0]
  return p * bits_float((uint32_t)(n + 127) << 23);
}

// u = (uint32)(pexp(lg - m) * 2^24): the product is exact, the conversion
// truncates. u <= 2^24, and u == 2^24 where lg == m.
PC_HD uint32_t table_weight(float lg, float m) {
  return (uint32_t)(pexp(lg - m) * 16777216.0f);
}

// Maximum logit into *m; false when any logit is inf or NaN.
PC_HD bool table_max(const float* lg, int L, float* m) {
  bool finite = true;
  float mx = lg[0];
  for (int l = 0; l < L; ++l) {
    finite = finite && is_finite(lg[l]);
    mx = lg[l] > mx ? lg[l] : mx;
  }
  *m = mx;
  return finite;
}

// S = sum of the weights u[0..L) in 64-bit integers (2^24 <= S <= L * 2^24
// for a finite row; an integer sum, so its order does not matter). S == 0
// marks a row with a non-finite logit.
PC_HD uint64_t table_sum(const uint32_t* u, int L, bool finite) {
  if (!finite) return 0;
  uint64_t S = 0;
  for (int l = 0; l < L; ++l) S += u[l];
  return S;
}

// f_l = max(1, u_l * (65536 - L) / S); the uniform (65536 - L) / L when
// S == 0. The floors sum to at most 65536 - L and the entry of the maximum
// logit (u = 2^24) is never raised, so a row's total is at most 65535.
PC_HD int32_t table_entry(uint32_t u, uint64_t S, int L) {
  const uint64_t scale = (uint64_t)(FREQ_SCALE - (uint32_t)L);
  if (S == 0) return (int32_t)(scale / (uint64_t)L);
  const uint64_t f = (uint64_t)u * scale / S;
  return f < 1 ? 1 : (int32_t)f;
}

// The whole rule on one row. The kernel runs the same four functions with
// one lane per entry (the weights pass through LDS).
PC_HD void table_row(const float* lg, int L, int32_t* f) {
  float m;
  uint32_t u[MAX_L];
  const bool finite = table_max(lg, L, &m);
  for (int l = 0; l < L; ++l) u[l] = finite ? table_weight(lg[l], m) : 0u;
  const uint64_t S = table_sum(u, L, finite);
  for (int l = 0; l < L; ++l) f[l] = table_entry(u[l], S, L);
}

// Packed weights, layout of pc_codec.hip / ops.pc_pack_weights.
struct Weights {
  const float *w0, *b0, *w1, *b1, *w2, *b2, *w3, *b3;
  int k, kp, L;
};

PC_HD Weights unpack(const float* wts, int k, int L) {
  Weights p;
  p.k = k;
  p.kp = (k + 7) / 8 * 8;
  p.L = L;
  p.w0 = wts;
  p.b0 = p.w0 + NT_FIRST * p.kp;
  p.w1 = p.b0 + p.kp;
  p.b1 = p.w1 + (size_t)NT_OTHER * k * p.kp;
  p.w2 = p.b1 + p.kp;
  p.b2 = p.w2 + (size_t)NT_OTHER * k * p.kp;
  p.w3 = p.b2 + p.kp;
  p.b3 = p.w3 + (size_t)NT_OTHER * k * L;
  return p;
}

inline size_t packed_numel(int k, int L) {
  const size_t kp = (size_t)(k + 7) / 8 * 8;
  return NT_FIRST * kp + kp + 2 * ((size_t)NT_OTHER * k * kp + kp) +
         (size_t)NT_OTHER * k * L + L;
}

// Host scratch of one position; activations are [site][kp] so the loop over
// output channels runs over consecutive words.
struct Scratch {
  float in[SIN];
  float a0[S0 * MAX_K];
  float a1[S1 * MAX_K];
  float a2[S2 * MAX_K];
};

// The two ways the host spells fmaf. Both are correctly rounded, so they
// give the same bits: Libm calls the C library, Builtin is left to the
// compiler, which emits the FMA instruction inside a function compiled for
// a target that has one (and the same library call elsewhere).
struct FmaLibm {
  static PC_HD float f(float a, float b, float c) { return ::fmaf(a, b, c); }
};
struct FmaBuiltin {
  static PC_HD float f(float a, float b, float c) {
    return __builtin_fmaf(a, b, c);
  }
};

// One masked VALID conv layer, pc_layer's operation order per output.
// in: [Di*Hi*Wi][cs_in] (cs_in = 1 for the context, kp otherwise),
// out: [(Di-1)*(Hi-2)*(Wi-2)][kp]. kp is a template parameter (8, 16, 24 or
// 32) so the accumulators of a site stay in registers.
template <class Fma, int KP, int NT, int Di, int Hi, int Wi, bool RELU,
          bool SKIP>
PC_HD void host_layer(const float* in, int cs_in, float* out, const float* w,
                      const float* b, int cin, const float* skip) {
  constexpr int Ho = Hi - 2, Wo = Wi - 2, kp = KP;
  for (int d = 0; d < Di - 1; ++d)
    for (int h = 0; h < Ho; ++h)
      for (int x = 0; x < Wo; ++x) {
        const int base = d * Hi * Wi + h * Wi + x;
        float acc[KP];
        for (int co = 0; co < kp; ++co) acc[co] = b[co];
        for (int t = 0; t < NT; ++t) {
          const int off = (t / 9) * Hi * Wi + ((t % 9) / 3) * Wi + (t % 3);
          const float* wt = w + (size_t)t * cin * kp;
          const float* it = in + (size_t)(base + off) * cs_in;
          for (int ci = 0; ci < cin; ++ci) {
            const float v = it[ci];
            const float* wc = wt + (size_t)ci * kp;
            for (int co = 0; co < kp; ++co) acc[co] = Fma::f(v, wc[co], acc[co]);
          }
        }
        float* o = out + (size_t)((d * Ho + h) * Wo + x) * kp;
        const float* s =
            SKIP ? skip + (size_t)((d + 2) * 49 + (h + 2) * 7 + (x + 2)) * kp
                 : nullptr;
        for (int co = 0; co < kp; ++co) {
          float r = acc[co];
          if (SKIP) r += s[co];
          if (RELU) r = relu(r);
          o[co] = r;
        }
      }
}

// Logits and table of position (c, h, w) of the padded value buffer q_pad
// (C+4, H+8, W+8); Hp = H + 8, Wp = W + 8.
template <class Fma, int KP>
PC_HD void eval_position_kp(const float* q_pad, int Hp, int Wp, int c, int h,
                         int w, const Weights& p, Scratch& s, float* logits,
                         int32_t* freqs) {
  for (int i = 0; i < SIN; ++i) {
    const int d = i / 81, r = i - d * 81, y = r / 9, x = r - y * 9;
    s.in[i] = q_pad[((int64_t)(c + d) * Hp + (h + y)) * Wp + (w + x)];
  }
  const int k = p.k, L = p.L;
  constexpr int kp = KP;
  host_layer<Fma, KP, NT_FIRST, 5, 9, 9, true, false>(s.in, 1, s.a0, p.w0,
                                                      p.b0, 1, nullptr);
  host_layer<Fma, KP, NT_OTHER, 4, 7, 7, true, false>(s.a0, kp, s.a1, p.w1,
                                                      p.b1, k, nullptr);
  host_layer<Fma, KP, NT_OTHER, 3, 5, 5, false, true>(s.a1, kp, s.a2, p.w2,
                                                      p.b2, k, s.a0);
  // conv2: tap t of the 2x3x3 input is site t; 14 partials, each a chain
  // over ci from 0.f, added to the bias in tap order.
  float part[NT_OTHER][MAX_L];
  for (int t = 0; t < NT_OTHER; ++t) {
    float acc[MAX_L];
    for (int l = 0; l < L; ++l) acc[l] = 0.f;
    const float* wt = p.w3 + (size_t)t * k * L;
    for (int ci = 0; ci < k; ++ci) {
      const float v = s.a2[(size_t)t * kp + ci];
      for (int l = 0; l < L; ++l) acc[l] = Fma::f(v, wt[ci * L + l], acc[l]);
    }
    for (int l = 0; l < L; ++l) part[t][l] = acc[l];
  }
  for (int l = 0; l < L; ++l) {
    float acc = p.b3[l];
    for (int t = 0; t < NT_OTHER; ++t) acc += part[t][l];
    logits[l] = acc;
  }
  table_row(logits, L, freqs);
}

template <class Fma>
PC_HD void eval_position(const float* q_pad, int Hp, int Wp, int c, int h,
                         int w, const Weights& p, Scratch& s, float* logits,
                         int32_t* freqs) {
  switch (p.kp) {
    case 8:
      eval_position_kp<Fma, 8>(q_pad, Hp, Wp, c, h, w, p, s, logits, freqs);
      break;
    case 16:
      eval_position_kp<Fma, 16>(q_pad, Hp, Wp, c, h, w, p, s, logits, freqs);
      break;
    case 24:
      eval_position_kp<Fma, 24>(q_pad, Hp, Wp, c, h, w, p, s, logits, freqs);
      break;
    default:
      eval_position_kp<Fma, 32>(q_pad, Hp, Wp, c, h, w, p, s, logits, freqs);
      break;
  }
}

}  // namespace pc
}  // namespace dsin
