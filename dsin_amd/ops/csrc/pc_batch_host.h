// Pointer-level host loops of the batched portable codec: B images of one
// symbol-volume shape (C, H, W) share a wave schedule and a position list,
// their payloads lie concatenated in one byte buffer with B+1 offsets. This
// header knows nothing of torch::Tensor, so the extension (pc_codec.hip) and
// a stand-alone sanitizer build (tools/pc_batch_check.cpp) run the same code.
// The second half is the ragged form, for images of different shapes
// (tools/pc_ragged_check.cpp).
//
// Who evaluates the context model is the caller's business: the functions
// here take tables (B, n, L) or a callable that fills them for one wave.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
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

// ---------------------------------------------------------------------------
// Ragged form: the images of a batch differ in (C, H, W). Their padded
// volumes lie in one flat fp32 buffer, their symbols in one flat int64
// output, and a descriptor row per image says where:
//   desc[5*b .. 5*b+4] = C_b, H_b, W_b, offset of the (C_b+4, H_b+8, W_b+8)
//   volume in the value buffer, offset of the C_b*H_b*W_b symbols in the
//   output.
// Positions are items (b, c, h, w), int32 (n, 4). A decode takes them sorted
// by (t, b, c, h, w), t = 25c + 5h + w, with a cumulative segment table of
// T*B + 1 entries: wave t is items[seg[t*B], seg[(t+1)*B]) and image b's
// share of it items[seg[t*B+b], seg[t*B+b+1]), which may be empty. An encode
// takes them sorted by (b, t, c, h, w) with B + 1 starts: image b's symbols
// are [starts[b], starts[b+1]) in its own wave order.
// ---------------------------------------------------------------------------

constexpr int DESC = 5;       // int64 words per descriptor row
constexpr int ROW_EXTRA = 24; // bytes of an encoded row beside 3 per symbol

struct Image {
  int C, H, W;
  int64_t q_off, sym_off;
  int64_t q_numel() const { return (int64_t)(C + 4) * (H + 8) * (W + 8); }
  int64_t n() const { return (int64_t)C * H * W; }
};

inline Image image_of(const int64_t* desc, int64_t b) {
  const int64_t* d = desc + DESC * b;
  return Image{(int)d[0], (int)d[1], (int)d[2], d[3], d[4]};
}

// true when the ranges [off[i], off[i] + len[i]) lie in [0, total) and no
// two of them share an element.
inline bool ranges_disjoint(std::vector<std::pair<int64_t, int64_t>> r,
                            int64_t total) {
  std::sort(r.begin(), r.end());
  int64_t end = 0;
  for (const auto& p : r) {
    if (p.first < end || p.second < 0 || p.second > total - p.first)
      return false;
    end = p.first + p.second;
  }
  return true;
}

// A descriptor table is good when every C, H, W is in [1, 65535], the
// volumes lie inside the value buffer of q_total floats without overlap, and
// the symbol ranges lie inside the output of sym_total values without
// overlap. Returns nullptr, or what is wrong.
inline const char* desc_problem(const int64_t* desc, int64_t B,
                                int64_t q_total, int64_t sym_total) {
  if (B < 1) return "a ragged batch needs at least one image";
  std::vector<std::pair<int64_t, int64_t>> q, s;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* d = desc + DESC * b;
    for (int j = 0; j < 3; ++j)
      if (d[j] < 1 || d[j] > 65535) return "C, H, W must be in [1, 65535]";
    if (d[3] < 0 || d[4] < 0) return "negative offset in a descriptor";
    const Image im = image_of(desc, b);
    q.push_back({im.q_off, im.q_numel()});
    s.push_back({im.sym_off, im.n()});
  }
  if (!ranges_disjoint(q, q_total))
    return "padded volumes must lie inside the value buffer without overlap";
  if (!ranges_disjoint(s, sym_total))
    return "symbol ranges must lie inside the output without overlap";
  return nullptr;
}

// Index of the first item that names no image or lies outside its image's
// volume; n when all are good.
inline int64_t first_bad_item(const int32_t* items, int64_t n,
                              const int64_t* desc, int64_t B) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* it = items + 4 * i;
    if (it[0] < 0 || it[0] >= B) return i;
    const Image im = image_of(desc, it[0]);
    if (it[1] < 0 || it[1] >= im.C || it[2] < 0 || it[2] >= im.H ||
        it[3] < 0 || it[3] >= im.W)
      return i;
  }
  return n;
}

// Index of the first item of a decode's segment table that belongs to
// another image than its segment; n when all are good.
inline int64_t first_misfiled_item(const int32_t* items, const int64_t* seg,
                                   int64_t T, int64_t B) {
  for (int64_t j = 0; j < T * B; ++j)
    for (int64_t i = seg[j]; i < seg[j + 1]; ++i)
      if (items[4 * i] != (int32_t)(j % B)) return i;
  return seg[T * B];
}

// Where image b's row starts in the flat output of a ragged encode, given
// the start of its symbols: every row is 8 bytes of length, 3 per symbol and
// 16 more. (RC_HD: the encoder kernel computes the same offset.)
RC_HD int64_t ragged_row_offset(int64_t b, int64_t start) {
  return ROW_EXTRA * b + 3 * start;
}

// Rows [b_lo, b_hi) of a ragged encode: image b codes syms[starts[b],
// starts[b+1]) against the same rows of freqs (n, L) into its row of out:
// the 8-byte little-endian payload length, then the payload.
inline void encode_ragged(const int32_t* syms, const int32_t* freqs,
                          const int64_t* starts, int L, uint8_t* out,
                          int64_t b_lo, int64_t b_hi) {
  for (int64_t b = b_lo; b < b_hi; ++b) {
    const int64_t s = starts[b], n = starts[b + 1] - s;
    uint8_t* row = out + ragged_row_offset(b, s);
    const uint64_t len = encode_row(syms + s, freqs + s * L, n, L, row + 8,
                                    (uint64_t)(3 * n + 16));
    for (int i = 0; i < 8; ++i) row[i] = (uint8_t)((len >> (8 * i)) & 0xFF);
  }
}

struct RaggedDecodeArgs {
  int64_t B, T;            // images, waves of the merged schedule
  int L;
  const int64_t* desc;     // (B, 5)
  const int32_t* items;    // (n, 4), sorted by (t, b, c, h, w)
  const int64_t* seg;      // (T*B + 1)
  const int32_t* freqs;    // (n, L): row i is item i, filled by eval_wave
  const uint8_t* data;     // concatenated payloads
  const int64_t* offs;     // (B + 1)
  const float* centers;    // (L)
  float* q;                // the flat value buffer, filled in place
  int64_t* out;            // the flat symbols
};

// Wavefront decode of a ragged batch. eval_wave(lo, hi) must fill freqs rows
// [lo, hi) from the current value buffer. An image with no item in a wave
// is skipped: its coder state stays untouched and no byte is read. Byte
// sources are bounded per image as in decode_batch.
template <class EvalWave>
inline void decode_ragged(const RaggedDecodeArgs& a, EvalWave&& eval_wave) {
  std::vector<rc::State> st((size_t)a.B);
  std::vector<rc::ByteSource> src((size_t)a.B);
  for (int64_t b = 0; b < a.B; ++b) {
    src[b] = rc::ByteSource{a.data + a.offs[b],
                            (uint64_t)(a.offs[b + 1] - a.offs[b])};
    rc::decode_start(st[b], src[b]);
  }
  uint32_t cum[rc::MAX_L + 1];
  for (int64_t t = 0; t < a.T; ++t) {
    const int64_t* sg = a.seg + t * a.B;
    if (sg[a.B] == sg[0]) continue;
    eval_wave(sg[0], sg[a.B]);
    for (int64_t b = 0; b < a.B; ++b) {
      if (sg[b + 1] == sg[b]) continue;
      const Image im = image_of(a.desc, b);
      float* q = a.q + im.q_off;
      int64_t* o = a.out + im.sym_off;
      for (int64_t i = sg[b]; i < sg[b + 1]; ++i) {
        rc::cumulate(a.freqs + i * a.L, a.L, cum);
        const int s = rc::decode_cum(st[b], src[b], cum, a.L);
        const int c = a.items[4 * i + 1], h = a.items[4 * i + 2],
                  w = a.items[4 * i + 3];
        o[((int64_t)c * im.H + h) * im.W + w] = s;
        q[((int64_t)(c + 4) * (im.H + 8) + (h + 4)) * (im.W + 8) + (w + 4)] =
            a.centers[s];
      }
    }
  }
}

}  // namespace pcb
}  // namespace dsin
