// Stand-alone check of the ragged host codec loops (pc_batch_host.h), meant
// to be built with sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined -I dsin_amd/ops/csrc
//       tools/pc_ragged_check.cpp -o pc_ragged_check && ./pc_ragged_check
//
// It includes nothing of the project but pc_batch_host.h, pc_model.h and
// rc_coder.h: the descriptor, item and segment arithmetic, the per-image rows
// of the flat encoder output and the wave loop over the merged schedule are
// the code the extension runs. For several mixes of volume shapes it encodes
// the batch with pcb::encode_ragged, compares every stream with the same
// volume coded alone, packs the payloads exactly (every payload ends where
// the next begins, and the buffer ends with the last one, so a read past an
// image's end is a read the sanitizer sees), decodes the batch with
// pcb::decode_ragged, then truncates a middle payload and checks that its
// image decodes as the same bytes decode alone and that the other images
// are untouched. The validators are fed bad tables too. Exit status 0 and a
// last line "ok".

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pc_batch_host.h"
#include "pc_model.h"
#include "rc_coder.h"

using namespace dsin;

static uint32_t g_seed = 97531u;
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

struct Shape { int C, H, W; };
struct Item { int t, b, c, h, w; };

struct Batch {
  int64_t B, n, T, q_total;
  std::vector<int64_t> desc;     // (B, 5)
  std::vector<int32_t> enc;      // items sorted by (b, t, c, h, w)
  std::vector<int64_t> starts;   // (B + 1)
  std::vector<int32_t> dec;      // items sorted by (t, b, c, h, w)
  std::vector<int64_t> seg;      // (T*B + 1)
};

static void push(std::vector<int32_t>* v, const Item& it) {
  v->insert(v->end(), {it.b, it.c, it.h, it.w});
}

static Batch make_batch(const std::vector<Shape>& shapes) {
  Batch bt;
  bt.B = (int64_t)shapes.size();
  std::vector<Item> all;
  int64_t q_off = 0, s_off = 0;
  int tmax = 0;
  bt.starts.assign(1, 0);
  for (int b = 0; b < (int)bt.B; ++b) {
    const Shape s = shapes[b];
    bt.desc.insert(bt.desc.end(), {s.C, s.H, s.W, q_off, s_off});
    q_off += (int64_t)(s.C + 4) * (s.H + 8) * (s.W + 8);
    s_off += (int64_t)s.C * s.H * s.W;
    for (int c = 0; c < s.C; ++c)
      for (int h = 0; h < s.H; ++h)
        for (int w = 0; w < s.W; ++w)
          all.push_back({25 * c + 5 * h + w, b, c, h, w});
    bt.starts.push_back(s_off);
  }
  bt.n = s_off;
  bt.q_total = q_off;
  // all is sorted by (b, c, h, w): stable sorts give the two orders
  std::vector<Item> e = all;
  std::stable_sort(e.begin(), e.end(), [](const Item& x, const Item& y) {
    return x.b != y.b ? x.b < y.b : x.t < y.t;
  });
  for (const Item& it : e) push(&bt.enc, it);
  std::vector<Item> d = all;
  std::stable_sort(d.begin(), d.end(),
                   [](const Item& x, const Item& y) { return x.t < y.t; });
  for (const Item& it : d) {
    push(&bt.dec, it);
    tmax = std::max(tmax, it.t);
  }
  bt.T = tmax + 1;
  std::vector<int64_t> count((size_t)(bt.T * bt.B), 0);
  for (const Item& it : d) count[(size_t)(it.t * bt.B + it.b)] += 1;
  bt.seg.assign(1, 0);
  for (int64_t c : count) bt.seg.push_back(bt.seg.back() + c);
  return bt;
}

// Tables of items [lo, hi), item by item as the extension's threads do.
static void eval_items(const Model& m, const Batch& bt,
                       const std::vector<int32_t>& items, const float* q,
                       int32_t* freqs, int64_t lo, int64_t hi) {
  pc::Scratch scratch;
  float lg[pc::MAX_L];
  for (int64_t i = lo; i < hi; ++i) {
    const int32_t* it = &items[4 * i];
    const pcb::Image im = pcb::image_of(bt.desc.data(), it[0]);
    pc::eval_position<pc::FmaLibm>(q + im.q_off, im.H + 8, im.W + 8, it[1],
                                   it[2], it[3], m.p, scratch, lg,
                                   freqs + i * m.L);
  }
}

static std::vector<int64_t> decode(const Model& m, const Batch& bt,
                                   const std::vector<uint8_t>& data,
                                   const std::vector<int64_t>& offs) {
  std::vector<float> q((size_t)bt.q_total, m.centers[0]);
  std::vector<int32_t> freqs((size_t)(bt.n * m.L));
  std::vector<int64_t> out((size_t)bt.n, -1);
  const pcb::RaggedDecodeArgs a{
      bt.B, bt.T, m.L, bt.desc.data(), bt.dec.data(), bt.seg.data(),
      freqs.data(), data.data(), offs.data(), m.centers.data(), q.data(),
      out.data()};
  pcb::decode_ragged(a, [&](int64_t lo, int64_t hi) {
    eval_items(m, bt, bt.dec, q.data(), freqs.data(), lo, hi);
  });
  return out;
}

// Flat rows of a ragged encode -> exactly packed payloads and their offsets.
static int pack(const Batch& bt, const std::vector<uint8_t>& rows,
                std::vector<uint8_t>* data, std::vector<int64_t>* offs) {
  offs->assign(1, 0);
  for (int64_t b = 0; b < bt.B; ++b) {
    const uint8_t* row =
        rows.data() + pcb::ragged_row_offset(b, bt.starts[b]);
    uint64_t len = 0;
    for (int i = 0; i < 8; ++i) len |= (uint64_t)row[i] << (8 * i);
    if (len > (uint64_t)(3 * (bt.starts[b + 1] - bt.starts[b]) + 16))
      return fail("encoder overran its row");
    data->insert(data->end(), row + 8, row + 8 + len);
    offs->push_back((int64_t)data->size());
  }
  return 0;
}

static int encode(const Model& m, const Batch& bt,
                  const std::vector<int64_t>& sym, std::vector<uint8_t>* data,
                  std::vector<int64_t>* offs) {
  std::vector<float> q((size_t)bt.q_total, m.centers[0]);
  std::vector<int32_t> s32((size_t)bt.n);
  for (int64_t i = 0; i < bt.n; ++i) {
    const int32_t* it = &bt.enc[4 * i];
    const pcb::Image im = pcb::image_of(bt.desc.data(), it[0]);
    const int64_t s =
        sym[im.sym_off + ((int64_t)it[1] * im.H + it[2]) * im.W + it[3]];
    s32[i] = (int32_t)s;
    q[im.q_off + ((int64_t)(it[1] + 4) * (im.H + 8) + (it[2] + 4)) *
                     (im.W + 8) + (it[3] + 4)] = m.centers[s];
  }
  std::vector<int32_t> freqs((size_t)(bt.n * m.L));
  eval_items(m, bt, bt.enc, q.data(), freqs.data(), 0, bt.n);
  // exactly the bytes the rows need: a write past a row's end is seen
  std::vector<uint8_t> rows((size_t)(pcb::ROW_EXTRA * bt.B + 3 * bt.n));
  // rows in two uneven pieces, as the extension's threads split them
  pcb::encode_ragged(s32.data(), freqs.data(), bt.starts.data(), m.L,
                     rows.data(), 0, bt.B / 2);
  pcb::encode_ragged(s32.data(), freqs.data(), bt.starts.data(), m.L,
                     rows.data(), bt.B / 2, bt.B);
  return pack(bt, rows, data, offs);
}

static int check_validators(const Batch& bt) {
  const int64_t B = bt.B;
  if (pcb::desc_problem(bt.desc.data(), B, bt.q_total, bt.n))
    return fail("desc_problem refused a good table");
  if (!pcb::desc_problem(bt.desc.data(), B, bt.q_total - 1, bt.n))
    return fail("desc_problem took a volume past the buffer");
  std::vector<int64_t> d = bt.desc;
  d[0] = 0;
  if (!pcb::desc_problem(d.data(), B, bt.q_total, bt.n))
    return fail("desc_problem took C = 0");
  if (B > 1) {
    d = bt.desc;
    d[pcb::DESC + 3] -= 1;  // volume 1 overlaps volume 0
    if (!pcb::desc_problem(d.data(), B, bt.q_total, bt.n))
      return fail("desc_problem took overlapping volumes");
    d = bt.desc;
    d[pcb::DESC + 4] = 0;  // symbols of image 1 on those of image 0
    if (!pcb::desc_problem(d.data(), B, bt.q_total, bt.n))
      return fail("desc_problem took overlapping symbol ranges");
  }
  if (!pcb::offsets_ok(bt.seg.data(), bt.T * B, bt.n))
    return fail("offsets_ok refused a good segment table");
  if (pcb::first_bad_item(bt.dec.data(), bt.n, bt.desc.data(), B) != bt.n)
    return fail("first_bad_item refused good items");
  if (pcb::first_misfiled_item(bt.dec.data(), bt.seg.data(), bt.T, B) != bt.n)
    return fail("first_misfiled_item refused good items");
  std::vector<int32_t> it = bt.dec;
  it[4 * (bt.n - 1)] = (int32_t)B;
  if (pcb::first_bad_item(it.data(), bt.n, bt.desc.data(), B) != bt.n - 1)
    return fail("first_bad_item took an image index of B");
  it = bt.dec;
  it[4 * (bt.n - 1) + 3] = (int32_t)bt.desc[pcb::DESC * it[4 * (bt.n - 1)] + 2];
  if (pcb::first_bad_item(it.data(), bt.n, bt.desc.data(), B) != bt.n - 1)
    return fail("first_bad_item took w = W");
  return 0;
}

static int check(int k, int L, const std::vector<Shape>& shapes) {
  const Model m = make_model(k, L);
  const Batch bt = make_batch(shapes);
  const int64_t B = bt.B;
  if (check_validators(bt)) return 1;

  // symbols: image b is random, 90 % zeros or all zeros in turn
  std::vector<int64_t> sym((size_t)bt.n);
  for (int64_t b = 0; b < B; ++b)
    for (int64_t i = bt.starts[b]; i < bt.starts[b + 1]; ++i) {
      int s = (int)((urand() + 1.f) * 0.5f * L) % L;
      if (b % 3 == 2 || (b % 3 == 1 && urand() < 0.8f)) s = 0;
      sym[i] = s;
    }

  std::vector<uint8_t> data;
  std::vector<int64_t> offs;
  if (encode(m, bt, sym, &data, &offs)) return 1;
  if (!pcb::offsets_ok(offs.data(), B, (int64_t)data.size()))
    return fail("offsets_ok refused good offsets");

  // every image alone, as a ragged batch of one: same bytes, same symbols
  for (int64_t b = 0; b < B; ++b) {
    const Batch one = make_batch({shapes[b]});
    const std::vector<int64_t> s1(sym.begin() + bt.starts[b],
                                  sym.begin() + bt.starts[b + 1]);
    std::vector<uint8_t> d1;
    std::vector<int64_t> o1;
    if (encode(m, one, s1, &d1, &o1)) return 1;
    if (d1 != std::vector<uint8_t>(data.begin() + offs[b],
                                   data.begin() + offs[b + 1]))
      return fail("stream of an image differs from the image coded alone");
    if (decode(m, one, d1, o1) != s1) return fail("single-image roundtrip");
  }

  if (decode(m, bt, data, offs) != sym) return fail("ragged roundtrip");

  if (B >= 3) {  // truncate the payload of a middle image
    const int64_t mid = B / 2;
    const int64_t full = offs[mid + 1] - offs[mid];
    for (int64_t cut : {(int64_t)0, std::min<int64_t>(3, full), full / 2}) {
      std::vector<uint8_t> d2(data.begin(), data.begin() + offs[mid] + cut);
      d2.insert(d2.end(), data.begin() + offs[mid + 1], data.end());
      std::vector<int64_t> o2 = offs;
      for (int64_t b = mid + 1; b <= B; ++b) o2[b] -= full - cut;
      const auto got = decode(m, bt, d2, o2);
      const std::vector<uint8_t> alone(data.begin() + offs[mid],
                                       data.begin() + offs[mid] + cut);
      const Batch one = make_batch({shapes[mid]});
      const auto want = decode(m, one, alone, {0, cut});
      for (int64_t i = 0; i < bt.n; ++i) {
        const bool in_mid = i >= bt.starts[mid] && i < bt.starts[mid + 1];
        if (in_mid && got[i] != want[i - bt.starts[mid]])
          return fail("truncated image differs");
        if (!in_mid && got[i] != sym[i])
          return fail("another image changed with a truncated one");
      }
    }
  }
  std::printf("ragged k=%d L=%d B=%lld n=%lld T=%lld: %zu bytes\n", k, L,
              (long long)B, (long long)bt.n, (long long)bt.T, data.size());
  return 0;
}

int main() {
  const std::vector<Shape> mix = {
      {3, 5, 6}, {1, 1, 1}, {2, 1, 7}, {3, 10, 12}, {3, 5, 6}};
  std::vector<Shape> rev(mix.rbegin(), mix.rend());
  std::vector<Shape> rot(mix.begin() + 2, mix.end());
  rot.insert(rot.end(), mix.begin(), mix.begin() + 2);
  if (check(8, 6, mix)) return 1;
  if (check(24, 16, rev)) return 1;
  if (check(20, 6, rot)) return 1;
  if (check(8, 2, {{2, 1, 7}})) return 1;
  if (check(8, 2, {{1, 1, 1}, {1, 1, 1}, {1, 1, 1}})) return 1;
  std::vector<Shape> alt;
  for (int b = 0; b < 17; ++b)
    alt.push_back(b % 2 ? Shape{2, 1, 7} : Shape{3, 5, 6});
  if (check(24, 6, alt)) return 1;
  std::printf("ok\n");
  return 0;
}
