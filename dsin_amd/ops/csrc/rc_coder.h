// Range-coder step functions shared by the device kernels (pc_codec.hip) and
// their host build (used by the CPU tests). Arithmetic mirrors
// dsin_amd/coding/range_coder.py step for step: 64-bit low/range with the
// same masks, Subbotin carry-less renormalisation, a byte read past the end
// of the stream returns 0. The Python `while True` becomes a bounded loop:
// a valid state (range >= 1) renormalises in at most 6 byte shifts (a range
// below 2^16 is realigned to a multiple of 2^8 after one shift and of 2^16
// after two), so RC_MAX_SHIFTS = 8 is never reached on a well-formed table.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RC_HD __host__ __device__ __forceinline__
#else
#define RC_HD inline
#endif

namespace dsin {
namespace rc {

constexpr uint64_t TOP = 1ull << 24;
constexpr uint64_t BOT = 1ull << 16;
constexpr uint64_t M32 = 0xFFFFFFFFull;
constexpr int MAX_SHIFTS = 8;
constexpr int MAX_L = 16;

struct State {
  uint64_t low;
  uint64_t range;
  uint64_t code;  // decoder only
  uint64_t pos;   // bytes written (encoder) / read (decoder)
};

RC_HD void init(State& s) {
  s.low = 0;
  s.range = M32;
  s.code = 0;
  s.pos = 0;
}

// range // tot; both fit 32 bits whenever the state is well formed.
RC_HD uint64_t div_range(uint64_t range, uint32_t tot) {
  if (tot == 0) tot = 1;
  if (range <= M32) return (uint64_t)((uint32_t)range / tot);
  return range / tot;
}

// One renormalisation decision: returns false when the loop ends.
RC_HD bool need_shift(State& s) {
  if ((s.low ^ (s.low + s.range)) < TOP) return true;  // top byte settled
  if (s.range < BOT) {
    s.range = (0 - s.low) & (BOT - 1);
    if (s.range == 0) s.range = BOT;
    return true;
  }
  return false;
}

RC_HD void shift(State& s) {
  s.low = (s.low << 8) & M32;
  s.range = s.range << 8;
  if (s.range > M32) s.range = M32;
}

struct ByteSink {
  uint8_t* buf;
  uint64_t cap;
  RC_HD void put(uint64_t pos, uint8_t b) const {
    if (pos < cap) buf[pos] = b;  // an overrun is reported through the length
  }
};

struct ByteSource {
  const uint8_t* buf;
  uint64_t len;
  RC_HD uint8_t get(uint64_t pos) const { return pos < len ? buf[pos] : 0; }
};

// Encode a symbol occupying [cum, cum+freq) of [0, tot).
template <class Sink>
RC_HD void encode(State& s, const Sink& out, uint32_t cum, uint32_t freq,
                  uint32_t tot) {
  uint64_t r = div_range(s.range, tot);
  s.low = s.low + r * cum;
  s.range = r * freq;
  for (int it = 0; it < MAX_SHIFTS; ++it) {
    if (!need_shift(s)) break;
    out.put(s.pos, (uint8_t)((s.low >> 24) & 0xFF));
    s.pos += 1;
    shift(s);
  }
}

template <class Sink>
RC_HD void finish(State& s, const Sink& out) {
  for (int i = 0; i < 4; ++i) {
    out.put(s.pos, (uint8_t)((s.low >> 24) & 0xFF));
    s.pos += 1;
    s.low = (s.low << 8) & M32;
  }
}

template <class Source>
RC_HD void decode_start(State& s, const Source& in) {
  init(s);
  for (int i = 0; i < 4; ++i) {
    s.code = ((s.code << 8) | in.get(s.pos)) & M32;
    s.pos += 1;
  }
}

// Decode one symbol against a cumulative row cum[0..L] (cum[0] = 0,
// cum[L] = tot). Returns the symbol, which lies in [0, L).
template <class Source>
RC_HD int decode_cum(State& s, const Source& in, const uint32_t* cum, int L) {
  uint32_t tot = cum[L];
  if (tot == 0) tot = 1;
  uint64_t r = div_range(s.range, tot);
  if (r == 0) r = 1;
  uint64_t target;
  if (s.code >= s.low) {
    const uint64_t d = s.code - s.low;  // fits 32 bits on a valid stream
    target = (d <= M32 && r <= M32) ? (uint64_t)((uint32_t)d / (uint32_t)r)
                                    : d / r;
  } else {
    // Python floor division: code - low is negative on a corrupt stream
    const int64_t d = (int64_t)s.code - (int64_t)s.low;
    int64_t q = d / (int64_t)r;
    if (d % (int64_t)r != 0) q -= 1;
    target = (uint64_t)q;
  }
  target &= M32;
  if (target > (uint64_t)tot - 1) target = (uint64_t)tot - 1;
  // cum is non-decreasing: the symbol is the number of l in [1, L) with
  // cum[l] <= target (searchsorted(cum, target, "right") - 1)
  int sym = 0;
  for (int l = 1; l < L; ++l) sym += ((uint64_t)cum[l] <= target) ? 1 : 0;
  const uint32_t lo = cum[sym];
  s.low = s.low + r * lo;
  s.range = r * (uint64_t)(cum[sym + 1] - lo);
  for (int it = 0; it < MAX_SHIFTS; ++it) {
    if (!need_shift(s)) break;
    s.code = ((s.code << 8) | in.get(s.pos)) & M32;
    s.pos += 1;
    shift(s);
  }
  return sym;
}

// Cumulative row of a frequency row f[0..L), L <= MAX_L.
RC_HD void cumulate(const int32_t* f, int L, uint32_t* cum) {
  cum[0] = 0;
  for (int l = 0; l < L; ++l) cum[l + 1] = cum[l] + (uint32_t)f[l];
}

}  // namespace rc
}  // namespace dsin
