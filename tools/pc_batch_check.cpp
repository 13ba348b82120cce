// Stand-alone check of the batched host codec loops (pc_batch_host.h), meant
// to be built with sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined -I dsin_amd/ops/csrc
//       tools/pc_batch_check.cpp -o pc_batch_check && ./pc_batch_check
//
// It includes nothing of the project but pc_batch_host.h, pc_model.h and
// rc_coder.h: the offset arithmetic over concatenated payloads, the per-image
// rows and the split of images x positions are the code the extension runs.
// For several shapes and batch sizes it encodes B symbol volumes row by row,
// packs the payloads exactly (every payload ends where the next begins, and
// the buffer ends with the last one, so a read past an image's end is a read
// the sanitizer sees), decodes the batch, then truncates the middle payload
// and checks that its image decodes as the same bytes decode alone and that
// its neighbours are untouched. Exit status 0 and a last line "ok".

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pc_batch_host.h"
#include "pc_model.h"
#include "rc_coder.h"

using namespace dsin;

static uint32_t g_seed = 2468u;
static float urand() {  // [-1, 1)
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) / 8388608.0f - 1.0f;
}

static int fail(const char* what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

struct Model {
  int k, L;
  std::vector<float> wts, centers;
  pc::Weights p;
};

static Model make_model(int k, int L) {
  Model m;
  m.k = k;
  m.L = L;
  m.wts.resize(pc::packed_numel(k, L));
  for (auto& v : m.wts) v = 0.3f * urand();
  m.p = pc::unpack(m.wts.data(), k, L);
  float* wm = m.wts.data();  // padded output channels hold zeros
  for (int t = 0; t < pc::NT_FIRST + 1; ++t)
    for (int co = k; co < m.p.kp; ++co) wm[t * m.p.kp + co] = 0.f;
  for (const float* base : {m.p.w1, m.p.w2}) {
    float* b = wm + (base - m.wts.data());
    for (int r = 0; r < pc::NT_OTHER * k + 1; ++r)
      for (int co = k; co < m.p.kp; ++co) b[r * m.p.kp + co] = 0.f;
  }
  m.centers.resize(L);
  for (int l = 0; l < L; ++l) m.centers[l] = -2.f + 4.f * l / (L - 1);
  return m;
}

// Wave-ordered positions (t = 25c + 5h + w, then c, h, w) and wave offsets.
static void schedule(int C, int H, int W, std::vector<int32_t>* pos,
                     std::vector<int64_t>* offsets) {
  struct P { int t, c, h, w; };
  std::vector<P> v;
  for (int c = 0; c < C; ++c)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) v.push_back({25 * c + 5 * h + w, c, h, w});
  std::stable_sort(v.begin(), v.end(),
                   [](const P& a, const P& b) { return a.t < b.t; });
  offsets->assign(1, 0);
  for (size_t i = 0; i < v.size(); ++i) {
    if (i && v[i].t != v[i - 1].t) offsets->push_back((int64_t)i);
    pos->insert(pos->end(), {v[i].c, v[i].h, v[i].w});
  }
  offsets->push_back((int64_t)v.size());
}

struct Batch {
  int64_t B, n;
  int C, H, W;
  int64_t q_stride;
  std::vector<int32_t> pos;
  std::vector<int64_t> waves;
};

// Tables of positions [lo, hi) of every image, through the same split of
// images x positions the extension hands to its threads, in uneven chunks.
static void eval_wave(const Model& m, const Batch& bt, const float* q_pad,
                      int32_t* freqs, int64_t lo, int64_t hi) {
  pc::Scratch scratch;
  float lg[pc::MAX_L];
  const int64_t total = bt.B * (hi - lo);
  for (int64_t s = 0; s < total;) {
    const int64_t e = std::min<int64_t>(total, s + 1 + (s % 5));
    pcb::for_image_pieces(s, e, lo, hi, [&](int64_t b, int64_t plo,
                                            int64_t phi) {
      for (int64_t i = plo; i < phi; ++i)
        pc::eval_position<pc::FmaLibm>(
            q_pad + b * bt.q_stride, bt.H + 8, bt.W + 8, bt.pos[3 * i],
            bt.pos[3 * i + 1], bt.pos[3 * i + 2], m.p, scratch, lg,
            freqs + (b * bt.n + i) * m.L);
    });
    s = e;
  }
}

static std::vector<int64_t> decode(const Model& m, const Batch& bt,
                                   const std::vector<uint8_t>& data,
                                   const std::vector<int64_t>& offs,
                                   int64_t B) {
  Batch b1 = bt;
  b1.B = B;
  std::vector<float> q((size_t)(B * bt.q_stride), m.centers[0]);
  std::vector<int32_t> freqs((size_t)(B * bt.n * m.L));
  std::vector<int64_t> out((size_t)(B * bt.n), -1);
  const pcb::DecodeArgs a{B, bt.n, m.L, bt.C, bt.H, bt.W, bt.pos.data(),
                          freqs.data(), data.data(), offs.data(),
                          m.centers.data(), q.data(), out.data()};
  pcb::decode_batch(a, bt.waves, [&](int64_t lo, int64_t hi) {
    eval_wave(m, b1, q.data(), freqs.data(), lo, hi);
  });
  return out;
}

static int check(int k, int L, int C, int H, int W, int64_t B) {
  const Model m = make_model(k, L);
  Batch bt{B, (int64_t)C * H * W, C, H, W,
           (int64_t)(C + 4) * (H + 8) * (W + 8), {}, {}};
  schedule(C, H, W, &bt.pos, &bt.waves);
  const int64_t n = bt.n;

  // symbols: image b is random, 90 % zeros or all zeros in turn
  std::vector<int64_t> sym((size_t)(B * n));
  std::vector<float> q((size_t)(B * bt.q_stride), m.centers[0]);
  for (int64_t b = 0; b < B; ++b)
    for (int c = 0, i = 0; c < C; ++c)
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w, ++i) {
          int s = (int)((urand() + 1.f) * 0.5f * L) % L;
          if (b % 3 == 2 || (b % 3 == 1 && urand() < 0.8f)) s = 0;
          sym[b * n + i] = s;
          q[b * bt.q_stride + ((size_t)(c + 4) * (H + 8) + (h + 4)) * (W + 8) +
            (w + 4)] = m.centers[s];
        }

  // encode: tables of all positions, then one row per image
  std::vector<int32_t> freqs((size_t)(B * n * L));
  eval_wave(m, bt, q.data(), freqs.data(), 0, n);
  const uint64_t cap = 3 * (uint64_t)n + 16;
  std::vector<uint8_t> data;
  std::vector<int64_t> offs(1, 0);
  for (int64_t b = 0; b < B; ++b) {
    std::vector<int32_t> s32((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const int32_t* p = &bt.pos[3 * i];
      s32[i] = (int32_t)sym[b * n + ((int64_t)p[0] * H + p[1]) * W + p[2]];
    }
    std::vector<uint8_t> row(cap);
    const uint64_t len = pcb::encode_row(s32.data(), &freqs[b * n * L], n, L,
                                         row.data(), cap);
    if (len > cap) return fail("encoder overran its row");
    data.insert(data.end(), row.begin(), row.begin() + len);
    offs.push_back((int64_t)data.size());
  }
  if (!pcb::offsets_ok(offs.data(), B, (int64_t)data.size()))
    return fail("offsets_ok refused good offsets");
  if (B > 1) {
    std::vector<int64_t> bad = offs;
    std::swap(bad[1], bad[B]);
    if (bad[1] != bad[B] && pcb::offsets_ok(bad.data(), B, (int64_t)data.size()))
      return fail("offsets_ok took bad offsets");
  }

  if (decode(m, bt, data, offs, B) != sym) return fail("batch roundtrip");

  if (B >= 3) {  // truncate the payload of image 1
    const int64_t full = offs[2] - offs[1];
    for (int64_t cut : {(int64_t)0, std::min<int64_t>(3, full), full / 2}) {
      std::vector<uint8_t> d2(data.begin(), data.begin() + offs[1] + cut);
      d2.insert(d2.end(), data.begin() + offs[2], data.end());
      std::vector<int64_t> o2 = offs;
      for (int64_t b = 2; b <= B; ++b) o2[b] -= full - cut;
      const auto got = decode(m, bt, d2, o2, B);
      const std::vector<uint8_t> alone(data.begin() + offs[1],
                                       data.begin() + offs[1] + cut);
      const auto want = decode(m, bt, alone, {0, cut}, 1);
      for (int64_t i = 0; i < n; ++i) {
        if (got[n + i] != want[i]) return fail("truncated image differs");
        if (got[i] != sym[i] || got[2 * n + i] != sym[2 * n + i])
          return fail("neighbour of a truncated image differs");
      }
    }
  }
  std::printf("batch k=%d L=%d %dx%dx%d B=%lld: %zu bytes\n", k, L, C, H, W,
              (long long)B, data.size());
  return 0;
}

int main() {
  if (check(8, 6, 3, 5, 6, 1)) return 1;
  if (check(8, 6, 3, 5, 6, 3)) return 1;
  if (check(24, 16, 2, 1, 7, 5)) return 1;
  if (check(8, 2, 1, 1, 1, 3)) return 1;
  if (check(20, 6, 3, 10, 12, 4)) return 1;
  std::printf("ok\n");
  return 0;
}
