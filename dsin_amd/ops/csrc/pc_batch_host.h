// Pointer-level host loops of the batched portable codec: B images of one
// symbol-volume shape (C, H, W) share a wave schedule and a position list,
// their payloads lie concatenated in one byte buffer with B+1 offsets. This
// header knows nothing of torch::Tensor, so the extension (pc_codec.hip) and
// a stand-alone sanitizer build (tools/pc_batch_check.cpp) run the same code.
//
// Who evaluates the context model is the caller's business: the functions
// here take tables (B, n, L) or a callable that fills them for one wave.
#pragma once

#include <cstdint>
#include <vector>

#include "rc_coder.h"

namespace dsin {
namespace pcb {

// offs[0..B] must run from 0 to total without decreasing.
inline bool offsets_ok(const int64_t* offs, int64_t B, int64_t total) {
  if (B < 1 || offs[0] != 0 || offs[B] != total) return false;
  for (int64_t b = 0; b < B; ++b)
    if (offs[b + 1] < offs[b]) return false;
  return true;
}

// Range-code n symbols against tables (n, L) into out (cap bytes). Returns
// the stream length; a value above cap reports an overrun (the bytes past
// cap were dropped, nothing was written out of bounds).
inline uint64_t encode_row(const int32_t* syms, const int32_t* freqs,
                           int64_t n, int L, uint8_t* out, uint64_t cap) {
  rc::State st;
  rc::init(st);
  const rc::ByteSink sink{out, cap};
  for (int64_t i = 0; i < n; ++i) {
    const int s = syms[i] < 0 ? 0 : (syms[i] >= L ? L - 1 : syms[i]);
    const int32_t* f = freqs + i * L;
    uint32_t cum = 0, tot = 0;
    for (int l = 0; l < L; ++l) {
      if (l < s) cum += (uint32_t)f[l];
      tot += (uint32_t)f[l];
    }
    rc::encode(st, sink, cum, (uint32_t)f[s], tot);
  }
  rc::finish(st, sink);
  return st.pos;
}

// Splits the flat range [s, e) over images x positions [lo, hi) into one
// piece per image: f(image, first position, one past the last position).
template <class F>
inline void for_image_pieces(int64_t s, int64_t e, int64_t lo, int64_t hi,
                             F&& f) {
  const int64_t nw = hi - lo;
  while (s < e) {
    const int64_t img = s / nw, first = s - img * nw;
    const int64_t last = (e - img * nw) < nw ? (e - img * nw) : nw;
    f(img, lo + first, lo + last);
    s = img * nw + last;
  }
}

struct DecodeArgs {
  int64_t B, n;          // images, positions per image
  int L, C, H, W;
  const int32_t* pos;    // (n, 3), shared by all images
  const int32_t* freqs;  // (B, n, L), filled wave by wave by eval_wave
  const uint8_t* data;   // concatenated payloads
  const int64_t* offs;   // (B + 1): image b owns data[offs[b], offs[b+1])
  const float* centers;  // (L)
  float* q_pad;          // (B, C+4, H+8, W+8), filled in place
  int64_t* out;          // (B, C, H, W)
};

// Wavefront decode of the whole batch: wave i covers positions
// [wave_offsets[i], wave_offsets[i+1]). eval_wave(lo, hi) must fill
// freqs[b, lo..hi) for every image from the current q_pad. Every image has a
// coder state and a byte source of its own, bounded by its own payload: a
// read past the end of image b returns 0, never a byte of image b+1.
template <class EvalWave>
inline void decode_batch(const DecodeArgs& a,
                         const std::vector<int64_t>& wave_offsets,
                         EvalWave&& eval_wave) {
  std::vector<rc::State> st((size_t)a.B);
  std::vector<rc::ByteSource> src((size_t)a.B);
  for (int64_t b = 0; b < a.B; ++b) {
    src[b] = rc::ByteSource{a.data + a.offs[b],
                            (uint64_t)(a.offs[b + 1] - a.offs[b])};
    rc::decode_start(st[b], src[b]);
  }
  const int64_t q_stride = (int64_t)(a.C + 4) * (a.H + 8) * (a.W + 8);
  const int64_t o_stride = (int64_t)a.C * a.H * a.W;
  uint32_t cum[rc::MAX_L + 1];
  for (size_t wv = 1; wv < wave_offsets.size(); ++wv) {
    const int64_t lo = wave_offsets[wv - 1], hi = wave_offsets[wv];
    if (hi == lo) continue;
    eval_wave(lo, hi);
    for (int64_t b = 0; b < a.B; ++b) {
      const int32_t* fp = a.freqs + b * a.n * a.L;
      float* q = a.q_pad + b * q_stride;
      int64_t* o = a.out + b * o_stride;
      for (int64_t i = lo; i < hi; ++i) {
        rc::cumulate(fp + i * a.L, a.L, cum);
        const int s = rc::decode_cum(st[b], src[b], cum, a.L);
        const int c = a.pos[3 * i], h = a.pos[3 * i + 1], w = a.pos[3 * i + 2];
        o[((int64_t)c * a.H + h) * a.W + w] = s;
        q[((int64_t)(c + 4) * (a.H + 8) + (h + 4)) * (a.W + 8) + (w + 4)] =
            a.centers[s];
      }
    }
  }
}

}  // namespace pcb
}  // namespace dsin
