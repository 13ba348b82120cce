// Device-resident entropy codec: the probclass context model evaluated per
// position (pc_freqs) and a range coder that never leaves the GPU
// (rc_encode / rc_decode_wave).
//
// Every kernel and every entry point takes a batch of B images of one
// symbol-volume shape: the value buffer is (B, C+4, H+8, W+8), the position
// list is shared, outputs are (B, ...). One image is B = 1, which the Python
// layer decides. The three context-model entry points (pc_freqs, pc_encode,
// pc_decode) dispatch on the device of q_pad: kernels for a GPU tensor, the
// host build of the portable backend for a CPU tensor.
//
// Next to this uniform form stands a ragged one for images of different
// shapes (pc_freqs_ragged, pc_encode_ragged, pc_decode_ragged): one flat
// value buffer, a per-image descriptor table and items (b, c, h, w); the
// layouts are in pc_batch_host.h. Each stage has one __device__ body
// (pc_freqs_body, rc_encode_body, rc_decode_wave_body) holding everything
// after "where is my image, where is my position, where do my rows go", and
// two __global__ kernels that answer those questions and call it.
//
// pc_freqs: one workgroup per (queried position (c, h, w), image); the image
// is blockIdx.y. The position's 5x9x9 causal context is read from the padded
// value buffer q_pad (C+4, H+8, W+8) of its image and pushed through the
// four masked VALID 3-D convs in the order ProbClass.logits uses:
//   conv0 +ReLU  1 -> k   5x9x9 -> 4x7x7
//   res_conv1 +ReLU k -> k 4x7x7 -> 3x5x5
//   res_conv2 + conv0[:, 2:, 2:-2, 2:-2]   3x5x5 -> 2x3x3
//   conv2  k -> L          2x3x3 -> 1
// All activations live in LDS; the packed weights (about 72 KB at k=24, L=6)
// are read from global memory / L2, every workgroup reads the same ones.
// fp32 operands, fp32 FMA accumulation. Every output element is produced by
// exactly one thread looping (tap, ci) in a fixed order, so a position's
// logits and table do not depend on what else is in the launch, other
// images included: the encoder (one launch over all positions) and the
// decoder (one launch per wave) produce bit-identical tables by construction.
//
// Masks are structural. In the flattened (d, kh, kw) order of the 2x3x3
// filter the live taps are exactly the first 13 (first_mask) or 14
// (other_mask) indices; only those are packed and only those are read.
//
// Packed weight layout (fp32, kp = k rounded up to a multiple of 8, padded
// output channels hold zeros and are never read as inputs):
//   w0[13][1][kp] b0[kp] w1[14][k][kp] b1[kp] w2[14][k][kp] b2[kp]
//   w3[14][k][L]  b3[L]
//
// Tables: stabilised fp32 softmax, f = max(1, floor(p * (65536 - L))), so
// tot <= 65535 and the coder's range / tot is never 0.
//
// PORTABLE instantiation (codec backend id 2): the same conv chain with the
// ReLU and the table epilogue of pc_model.h, which a host build reproduces
// bit for bit (the CPU branch of the entry points below).

#include <atomic>
#include <functional>
#include <string>

#include "common.h"
#include "pc_batch_host.h"
#include "pc_model.h"
#include "rc_coder.h"

// No expression in this file lets a multiply feed an add; keep it so.
#pragma clang fp contract(off)

namespace dsin {

// The model's sizes are pc_model.h's (pc::MAX_K, pc::NT_FIRST, pc::S0, ...).
constexpr int PC_MAX_B = 65535;  // images per launch: gridDim.y
constexpr int PC_THREADS = 256;
static_assert(pc::MAX_L == rc::MAX_L, "model and coder disagree on MAX_L");

template <int CG> struct WVec;
template <> struct WVec<8> {
  float v[8];
  __device__ __forceinline__ void load(const float* p) {
    float4 a = *reinterpret_cast<const float4*>(p);
    float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
};
template <> struct WVec<2> {
  float v[2];
  __device__ __forceinline__ void load(const float* p) {
    float2 a = *reinterpret_cast<const float2*>(p);
    v[0] = a.x; v[1] = a.y;
  }
};

// One masked VALID conv layer on LDS activations. in: [cin][Di*Hi*Wi],
// out: [kp][Do*Ho*Wo]. A work item is (group of CG output channels, output
// site); sites are the fast index so a wave reads consecutive LDS words.
template <bool PORTABLE, int CG, int NT, int Di, int Hi, int Wi, bool RELU,
          bool SKIP>
__device__ __forceinline__ void pc_layer(const float* in, float* out,
                                         const float* __restrict__ w,
                                         const float* __restrict__ b, int cin,
                                         int kp, const float* skip) {
  constexpr int Ho = Hi - 2, Wo = Wi - 2;
  constexpr int Si = Di * Hi * Wi, So = (Di - 1) * Ho * Wo;
  const int items = So * (kp / CG);
  for (int item = threadIdx.x; item < items; item += PC_THREADS) {
    const int g = item / So, p = item - g * So;
    const int d = p / (Ho * Wo), rem = p - d * (Ho * Wo);
    const int h = rem / Wo, x = rem - h * Wo;
    const int base = d * Hi * Wi + h * Wi + x;
    const int co0 = g * CG;
    float acc[CG];
#pragma unroll
    for (int j = 0; j < CG; ++j) acc[j] = b[co0 + j];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int off = (t / 9) * Hi * Wi + ((t % 9) / 3) * Wi + (t % 3);
      const float* wt = w + (size_t)t * cin * kp + co0;
      const float* it = in + base + off;
#pragma unroll 4
      for (int ci = 0; ci < cin; ++ci) {
        const float v = it[ci * Si];
        WVec<CG> wv;
        wv.load(wt + ci * kp);
#pragma unroll
        for (int j = 0; j < CG; ++j) acc[j] = fmaf(v, wv.v[j], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < CG; ++j) {
      float r = acc[j];
      if (SKIP)
        r += skip[(co0 + j) * pc::S0 + (d + 2) * 49 + (h + 2) * 7 + (x + 2)];
      if (RELU) r = PORTABLE ? pc::relu(r) : fmaxf(r, 0.f);
      out[(co0 + j) * So + p] = r;
    }
  }
}

// What every pc_freqs workgroup does once it knows its image (q_pad, the
// (C+4, H+8, W+8) volume), its position (c, h, w) and its output rows
// (logits, freqs: L values each): stage the context, run the conv chain,
// write logits and table. A position outside the volume, or live == false
// (the ragged kernel: an item that names no image), writes the table of ones
// and reads nothing.
template <bool PORTABLE>
__device__ __forceinline__ void pc_freqs_body(
    const float* __restrict__ q_pad, int C, int H, int W, bool live, int c,
    int h, int w, const float* __restrict__ wts, int k, int kp, int L,
    float* __restrict__ logits, int* __restrict__ freqs) {
  __shared__ float s_in[pc::SIN + 3];
  __shared__ float s_a0[pc::MAX_K * pc::S0];
  __shared__ float s_a1[pc::MAX_K * pc::S1];
  __shared__ float s_a2[pc::MAX_K * pc::S2];
  __shared__ float s_part[pc::NT_OTHER * pc::MAX_L];
  __shared__ float s_lg[pc::MAX_L];
  __shared__ uint32_t s_u[pc::MAX_L];  // PORTABLE table weights

  const int tid = threadIdx.x;
  if (!live || c < 0 || c >= C || h < 0 || h >= H || w < 0 || w >= W) {
    if (tid < L) {  // never reached through the Python wrappers
      logits[tid] = 0.f;
      freqs[tid] = 1;
    }
    return;
  }
  const int Hp = H + 8, Wp = W + 8;
  for (int i = tid; i < pc::SIN; i += PC_THREADS) {
    const int d = i / 81, r = i - d * 81, y = r / 9, x = r - y * 9;
    s_in[i] = q_pad[((int64_t)(c + d) * Hp + (h + y)) * Wp + (w + x)];
  }
  const float* w0 = wts;
  const float* b0 = w0 + pc::NT_FIRST * kp;
  const float* w1 = b0 + kp;
  const float* b1 = w1 + (size_t)pc::NT_OTHER * k * kp;
  const float* w2 = b1 + kp;
  const float* b2 = w2 + (size_t)pc::NT_OTHER * k * kp;
  const float* w3 = b2 + kp;
  const float* b3 = w3 + (size_t)pc::NT_OTHER * k * L;
  __syncthreads();
  pc_layer<PORTABLE, 8, pc::NT_FIRST, 5, 9, 9, true, false>(
      s_in, s_a0, w0, b0, 1, kp, nullptr);
  __syncthreads();
  pc_layer<PORTABLE, 8, pc::NT_OTHER, 4, 7, 7, true, false>(
      s_a0, s_a1, w1, b1, k, kp, nullptr);
  __syncthreads();
  pc_layer<PORTABLE, 2, pc::NT_OTHER, 3, 5, 5, false, true>(
      s_a1, s_a2, w2, b2, k, kp, s_a0);
  __syncthreads();
  // conv2: one output site; tap t of the 2x3x3 input is site t. Thread
  // (t, l) sums over ci, then thread l adds the 14 partials in tap order.
  if (tid < pc::NT_OTHER * L) {
    const int t = tid / L, l = tid - t * L;
    float acc = 0.f;
    const float* wt = w3 + (size_t)t * k * L + l;
    for (int ci = 0; ci < k; ++ci)
      acc = fmaf(s_a2[ci * pc::S2 + t], wt[ci * L], acc);
    s_part[t * pc::MAX_L + l] = acc;
  }
  __syncthreads();
  if (tid < L) {
    float acc = b3[tid];
    for (int t = 0; t < pc::NT_OTHER; ++t) acc += s_part[t * pc::MAX_L + tid];
    s_lg[tid] = acc;
  }
  __syncthreads();
  if (PORTABLE) {  // pc_model.h: the functions the host build runs
    bool finite = true;
    if (tid < L) {
      float m;
      finite = pc::table_max(s_lg, L, &m);
      s_u[tid] = finite ? pc::table_weight(s_lg[tid], m) : 0u;
    }
    __syncthreads();
    if (tid < L) {
      const uint64_t S = pc::table_sum(s_u, L, finite);
      logits[tid] = s_lg[tid];
      freqs[tid] = pc::table_entry(s_u[tid], S, L);
    }
  } else if (tid < L) {
    float m = s_lg[0];
    for (int l = 1; l < L; ++l) m = fmaxf(m, s_lg[l]);
    float sum = 0.f;
    for (int l = 0; l < L; ++l) sum += expf(s_lg[l] - m);
    const float p = expf(s_lg[tid] - m) / sum;
    int f = (int)floorf(p * (float)(65536 - L));
    logits[tid] = s_lg[tid];
    freqs[tid] = f < 1 ? 1 : f;
  }
}

// Uniform form: position blockIdx.x of image blockIdx.y; outputs (B, n, L).
template <bool PORTABLE>
__global__ void __launch_bounds__(PC_THREADS)
pc_freqs_kernel(const float* __restrict__ q_pad, int64_t q_stride, int C,
                int H, int W, const int* __restrict__ pos,
                const float* __restrict__ wts, int k, int kp, int L,
                float* __restrict__ logits, int* __restrict__ freqs) {
  const int64_t ip = blockIdx.x;
  const int64_t b = (int64_t)blockIdx.y * gridDim.x + ip;
  pc_freqs_body<PORTABLE>(q_pad + (int64_t)blockIdx.y * q_stride, C, H, W,
                          true, pos[3 * ip], pos[3 * ip + 1], pos[3 * ip + 2],
                          wts, k, kp, L, logits + b * L, freqs + b * L);
}

// Per-image descriptor of the ragged form (pcb::DESC int64 words per image,
// layout in pc_batch_host.h): C, H, W, offset of the padded volume in the
// flat value buffer, offset of the symbols in the flat output.
struct PcImage {
  int C, H, W;
  int64_t q_off, sym_off;
};

__device__ __forceinline__ PcImage pc_image(const int64_t* __restrict__ desc,
                                            int64_t b) {
  const int64_t* d = desc + pcb::DESC * b;
  return PcImage{(int)d[0], (int)d[1], (int)d[2], d[3], d[4]};
}

// Ragged form: one workgroup per item (b, c, h, w) of items (n, 4); row
// blockIdx.x of compact (n, L) outputs. The images differ in size and lie
// in one flat value buffer q.
template <bool PORTABLE>
__global__ void __launch_bounds__(PC_THREADS)
pc_freqs_ragged_kernel(const float* __restrict__ q,
                       const int64_t* __restrict__ desc, int B,
                       const int* __restrict__ items,
                       const float* __restrict__ wts, int k, int kp, int L,
                       float* __restrict__ logits, int* __restrict__ freqs) {
  const int64_t row = blockIdx.x;
  const int* it = items + 4 * row;
  const int b = it[0];
  const bool live = b >= 0 && b < B;
  PcImage im{0, 0, 0, 0, 0};
  if (live) im = pc_image(desc, b);
  pc_freqs_body<PORTABLE>(q + im.q_off, im.C, im.H, im.W, live, it[1], it[2],
                          it[3], wts, k, kp, L, logits + row * L,
                          freqs + row * L);
}

// ---------------------------------------------------------------------------
// Range coder kernels. One lane runs the coder; the other lanes of the
// workgroup only stage its operands in LDS (per-symbol cum/freq/tot for the
// encoder; cumulative table rows and a window of the byte stream for the
// decoder) and scatter the decoded symbols.
// ---------------------------------------------------------------------------

constexpr int RC_CHUNK = 256;
constexpr int RC_WIN = RC_CHUNK * rc::MAX_SHIFTS;  // bytes a chunk can read

// What an encoder workgroup does once it knows its image: n symbols syms
// against tables freqs (n, L) into the row out: 8 bytes little-endian
// payload length, then the payload (cap bytes).
__device__ __forceinline__ void rc_encode_body(
    const int* __restrict__ syms, const int* __restrict__ freqs, int64_t n,
    int L, uint8_t* __restrict__ out, uint64_t cap) {
  __shared__ uint32_t s_cum[RC_CHUNK], s_f[RC_CHUNK], s_tot[RC_CHUNK];
  const int tid = threadIdx.x;
  rc::State st;
  rc::init(st);
  const rc::ByteSink sink{out + 8, cap};
  for (int64_t base = 0; base < n; base += RC_CHUNK) {
    const int64_t i = base + tid;
    if (i < n) {
      int s = syms[i];
      s = s < 0 ? 0 : (s >= L ? L - 1 : s);
      const int* f = freqs + i * L;
      uint32_t cum = 0, tot = 0, fs = 0;
      for (int l = 0; l < L; ++l) {
        const uint32_t v = (uint32_t)f[l];
        if (l < s) cum += v;
        if (l == s) fs = v;
        tot += v;
      }
      s_cum[tid] = cum; s_f[tid] = fs; s_tot[tid] = tot;
    }
    __syncthreads();
    if (tid == 0) {
      const int m = (int)((n - base) < RC_CHUNK ? (n - base) : RC_CHUNK);
      for (int j = 0; j < m; ++j)
        rc::encode(st, sink, s_cum[j], s_f[j], s_tot[j]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    rc::finish(st, sink);
    for (int i = 0; i < 8; ++i) out[i] = (uint8_t)((st.pos >> (8 * i)) & 0xFF);
  }
}

// Uniform form, one workgroup per image: syms (B, n), freqs (B, n, L), out
// (B, 8 + cap).
__global__ void __launch_bounds__(RC_CHUNK)
rc_encode_kernel(const int* __restrict__ syms, const int* __restrict__ freqs,
                 int64_t n, int L, uint8_t* __restrict__ out, uint64_t cap) {
  rc_encode_body(syms + (int64_t)blockIdx.x * n,
                 freqs + (int64_t)blockIdx.x * n * L, n, L,
                 out + (int64_t)blockIdx.x * (8 + cap), cap);
}

// Ragged form, one workgroup per image b over symbols [starts[b],
// starts[b+1]) of the flat syms (n) and freqs (n, L); its row starts at
// pcb::ragged_row_offset of the flat out and holds 3 n_b + 16 payload bytes.
__global__ void __launch_bounds__(RC_CHUNK)
rc_encode_ragged_kernel(const int* __restrict__ syms,
                        const int* __restrict__ freqs,
                        const int64_t* __restrict__ starts, int L,
                        uint8_t* __restrict__ out) {
  const int64_t b = blockIdx.x, s = starts[b], n = starts[b + 1] - s;
  rc_encode_body(syms + s, freqs + s * L, n, L,
                 out + pcb::ragged_row_offset(b, s), (uint64_t)(3 * n + 16));
}

// The payload of image b: data[offs[b], offs[b+1]) of the concatenated
// buffer, or all len bytes when offs is null (a single image).
__device__ __forceinline__ rc::ByteSource rc_image_bytes(
    const uint8_t* data, uint64_t len, const int64_t* offs, int64_t b) {
  if (offs == nullptr) return rc::ByteSource{data, len};
  return rc::ByteSource{data + offs[b], (uint64_t)(offs[b + 1] - offs[b])};
}

// One thread per image starts that image's decoder state.
__global__ void rc_decode_init_kernel(rc::State* state,
                                      const uint8_t* __restrict__ data,
                                      uint64_t len,
                                      const int64_t* __restrict__ offs,
                                      int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    rc::State st;
    rc::decode_start(st, rc_image_bytes(data, len, offs, b));
    state[b] = st;
  }
}

struct WindowSource {
  const uint8_t* win;   // LDS copy of data[base, base + RC_WIN), zero filled
  uint64_t base;
  const uint8_t* data;
  uint64_t len;
  __device__ __forceinline__ uint8_t get(uint64_t pos) const {
    if (pos >= len) return 0;
    if (pos >= base && pos - base < (uint64_t)RC_WIN) return win[pos - base];
    return data[pos];
  }
};

// What a decoder workgroup does once it knows its image: decodes nw symbols
// against the rows of freqs (nw, L), advancing *state. bytes is the image's
// own payload, so the window and every later read are bounded by it: past
// its end the coder reads 0, never the next image's first bytes. With pos
// set, symbol i belongs to (c, h, w) = pos[i * pos_stride + 0..2] of the
// image's (C, H, W) volume: it goes to out[c, h, w] and centers[s] into
// q_pad at that position; with pos == nullptr it goes to out[i].
__device__ __forceinline__ void rc_decode_wave_body(
    rc::State* state, const rc::ByteSource bytes,
    const int* __restrict__ freqs, const int* __restrict__ pos,
    int pos_stride, int64_t nw, int L, const float* __restrict__ centers,
    float* __restrict__ q_pad, int C, int H, int W,
    int64_t* __restrict__ out) {
  __shared__ uint32_t s_cum[RC_CHUNK * (rc::MAX_L + 1)];
  __shared__ uint8_t s_win[RC_WIN];
  __shared__ int s_sym[RC_CHUNK];
  __shared__ rc::State s_state;
  const int tid = threadIdx.x;
  const uint8_t* data = bytes.buf;
  const uint64_t len = bytes.len;
  if (tid == 0) s_state = *state;
  __syncthreads();
  for (int64_t base = 0; base < nw; base += RC_CHUNK) {
    const int m = (int)((nw - base) < RC_CHUNK ? (nw - base) : RC_CHUNK);
    const uint64_t wbase = s_state.pos;
    for (int i = tid; i < RC_WIN; i += RC_CHUNK)
      s_win[i] = (wbase + i < len) ? data[wbase + i] : (uint8_t)0;
    if (tid < m)  // every lane builds the cumulative row of its symbol
      rc::cumulate(freqs + (base + tid) * L, L, s_cum + tid * (rc::MAX_L + 1));
    __syncthreads();
    if (tid == 0) {
      rc::State st = s_state;
      const WindowSource src{s_win, wbase, data, len};
      for (int j = 0; j < m; ++j)
        s_sym[j] = rc::decode_cum(st, src, s_cum + j * (rc::MAX_L + 1), L);
      s_state = st;
    }
    __syncthreads();
    if (tid < m) {
      const int s = s_sym[tid];
      const int64_t i = base + tid;
      if (pos == nullptr) {
        out[i] = s;
      } else {
        const int* p = pos + i * pos_stride;
        const int c = p[0], h = p[1], w = p[2];
        if (c >= 0 && c < C && h >= 0 && h < H && w >= 0 && w < W) {
          out[((int64_t)c * H + h) * W + w] = s;
          q_pad[((int64_t)(c + 4) * (H + 8) + (h + 4)) * (W + 8) + (w + 4)] =
              centers[s];
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) *state = s_state;
}

// Uniform form, one workgroup per image b = blockIdx.x: freqs (B, nw, L),
// pos (nw, 3) shared by the images, q_pad (B, C+4, H+8, W+8), out row b of
// out_stride values (C*H*W, or nw when pos == nullptr).
__global__ void __launch_bounds__(RC_CHUNK)
rc_decode_wave_kernel(rc::State* state, const uint8_t* __restrict__ data_all,
                      uint64_t len_all, const int64_t* __restrict__ offs,
                      const int* __restrict__ freqs,
                      const int* __restrict__ pos, int64_t nw, int L,
                      const float* __restrict__ centers,
                      float* __restrict__ q_pad, int64_t q_stride, int C,
                      int H, int W, int64_t* __restrict__ out,
                      int64_t out_stride) {
  const int64_t img = blockIdx.x;
  if (pos != nullptr) q_pad += img * q_stride;
  rc_decode_wave_body(state + img,
                      rc_image_bytes(data_all, len_all, offs, img),
                      freqs + img * nw * L, pos, 3, nw, L, centers, q_pad, C,
                      H, W, out + img * out_stride);
}

// Ragged form, one workgroup per image b = blockIdx.x, for wave t of the
// merged schedule: seg is the (T*B + 1) segment table over items (n, 4)
// sorted by (t, b, c, h, w), freqs the compact tables of the wave (row 0 is
// item seg[t*B]). The workgroup decodes items [seg[t*B+b], seg[t*B+b+1]) into
// its image's volume of the flat value buffer q and its range of the flat
// out. An empty segment returns at once: the state stays untouched and no
// byte is read.
__global__ void __launch_bounds__(RC_CHUNK)
rc_decode_wave_ragged_kernel(rc::State* state,
                             const uint8_t* __restrict__ data_all,
                             uint64_t len_all,
                             const int64_t* __restrict__ offs,
                             const int* __restrict__ freqs,
                             const int* __restrict__ items,
                             const int64_t* __restrict__ seg, int64_t t,
                             const int64_t* __restrict__ desc, int L,
                             const float* __restrict__ centers,
                             float* __restrict__ q,
                             int64_t* __restrict__ out) {
  const int64_t b = blockIdx.x, B = gridDim.x;
  const int64_t w0 = seg[t * B], lo = seg[t * B + b], hi = seg[t * B + b + 1];
  if (hi <= lo) return;
  const PcImage im = pc_image(desc, b);
  rc_decode_wave_body(state + b, rc_image_bytes(data_all, len_all, offs, b),
                      freqs + (lo - w0) * L, items + 4 * lo + 1, 4, hi - lo, L,
                      centers, q + im.q_off, im.C, im.H, im.W,
                      out + im.sym_off);
}

// ---------------------------------------------------------------------------
// Host build of the portable backend (CPU tensors): pc_model.h per position,
// positions of a wave spread over at::parallel_for, the coder step functions
// of rc_coder.h. A position's logits and table depend on nothing but q_pad
// and the weights, so the thread count does not change them.
// ---------------------------------------------------------------------------

// at::parallel_for, compiled with OpenMP in host_parallel.cpp.
void host_parallel_for(int64_t begin, int64_t end, int64_t grain,
                       const std::function<void(int64_t, int64_t)>& f);

struct PcHostArgs {
  const float* q_pad;
  int Hp, Wp;
  const int* pos;
  pc::Weights wts;
  float* logits;  // (n, L), may be nullptr
  int* freqs;     // (n, L)
};

template <class Fma>
static __forceinline__ void pc_host_range_impl(const PcHostArgs& a, int64_t lo,
                                               int64_t hi) {
  pc::Scratch scratch;
  float lg[pc::MAX_L];
  const int L = a.wts.L;
  for (int64_t i = lo; i < hi; ++i) {
    pc::eval_position<Fma>(a.q_pad, a.Hp, a.Wp, a.pos[3 * i], a.pos[3 * i + 1],
                           a.pos[3 * i + 2], a.wts, scratch, lg,
                           a.freqs + i * L);
    if (a.logits)
      for (int l = 0; l < L; ++l) a.logits[i * L + l] = lg[l];
  }
}

static void pc_host_range_libm(const PcHostArgs& a, int64_t lo, int64_t hi) {
  pc_host_range_impl<pc::FmaLibm>(a, lo, hi);
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define PC_HOST_HAS_HW_PATH 1
// The same source compiled for AVX2 + FMA: every fmaf becomes one (vector)
// FMA instruction, which rounds once as the library call does.
__attribute__((target("avx2,fma"))) static void pc_host_range_hw(
    const PcHostArgs& a, int64_t lo, int64_t hi) {
  pc_host_range_impl<pc::FmaBuiltin>(a, lo, hi);
}
static bool pc_host_cpu_has_fma() {
  return __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
}
#else
#define PC_HOST_HAS_HW_PATH 0
static void pc_host_range_hw(const PcHostArgs& a, int64_t lo, int64_t hi) {
  pc_host_range_libm(a, lo, hi);
}
static bool pc_host_cpu_has_fma() { return false; }
#endif

static std::atomic<bool> g_pc_host_force_libm{false};

// Force the library-fmaf path (true) or return to the run-time choice
// (false). Returns the previous setting.
bool pc_host_force_libm(bool on) { return g_pc_host_force_libm.exchange(on); }

// "fma" when the hardware-FMA path would run now, "libm" otherwise.
std::string pc_host_path() {
  return (pc_host_cpu_has_fma() && !g_pc_host_force_libm.load()) ? "fma"
                                                                 : "libm";
}

bool pc_host_has_fma() { return pc_host_cpu_has_fma(); }

// Tables (and logits) of positions [lo, hi) of a.pos in each of B images:
// a describes image 0, image b lies q_stride floats further in q_pad and
// n rows further in logits and freqs, which are (B, n, L). Images x
// positions are spread over the threads together, so a narrow wave of a
// large batch still fills them.
static void pc_host_eval(const PcHostArgs& a, int64_t B, int64_t q_stride,
                         int64_t n, int64_t lo, int64_t hi) {
  if (hi <= lo) return;
  const bool hw = pc_host_cpu_has_fma() && !g_pc_host_force_libm.load();
  const int L = a.wts.L;
  host_parallel_for(0, B * (hi - lo), 1, [&](int64_t s, int64_t e) {
    pcb::for_image_pieces(s, e, lo, hi, [&](int64_t b, int64_t plo,
                                            int64_t phi) {
      PcHostArgs ab = a;
      ab.q_pad += b * q_stride;
      if (ab.logits) ab.logits += b * n * L;
      ab.freqs += b * n * L;
      if (hw)
        pc_host_range_hw(ab, plo, phi);
      else
        pc_host_range_libm(ab, plo, phi);
    });
  });
}

// Ragged form: items (b, c, h, w) of images that differ in size. a.pos is
// the (n, 4) item list, a.q_pad the flat value buffer; Hp and Wp come from
// the item's descriptor. Rows of logits and freqs are compact (n, L).
template <class Fma>
static __forceinline__ void pc_host_items_impl(const PcHostArgs& a,
                                               const int64_t* desc,
                                               int64_t lo, int64_t hi) {
  pc::Scratch scratch;
  float lg[pc::MAX_L];
  const int L = a.wts.L;
  for (int64_t i = lo; i < hi; ++i) {
    const int* it = a.pos + 4 * i;
    const pcb::Image im = pcb::image_of(desc, it[0]);
    pc::eval_position<Fma>(a.q_pad + im.q_off, im.H + 8, im.W + 8, it[1],
                           it[2], it[3], a.wts, scratch, lg, a.freqs + i * L);
    if (a.logits)
      for (int l = 0; l < L; ++l) a.logits[i * L + l] = lg[l];
  }
}

static void pc_host_items_libm(const PcHostArgs& a, const int64_t* desc,
                               int64_t lo, int64_t hi) {
  pc_host_items_impl<pc::FmaLibm>(a, desc, lo, hi);
}

#if PC_HOST_HAS_HW_PATH
__attribute__((target("avx2,fma"))) static void pc_host_items_hw(
    const PcHostArgs& a, const int64_t* desc, int64_t lo, int64_t hi) {
  pc_host_items_impl<pc::FmaBuiltin>(a, desc, lo, hi);
}
#else
static void pc_host_items_hw(const PcHostArgs& a, const int64_t* desc,
                             int64_t lo, int64_t hi) {
  pc_host_items_libm(a, desc, lo, hi);
}
#endif

// Tables (and logits) of items [lo, hi), spread over the threads item by
// item, so a wave fills them whichever images it comes from.
static void pc_host_eval_ragged(const PcHostArgs& a, const int64_t* desc,
                                int64_t lo, int64_t hi) {
  if (hi <= lo) return;
  const bool hw = pc_host_cpu_has_fma() && !g_pc_host_force_libm.load();
  host_parallel_for(lo, hi, 1, [&](int64_t s, int64_t e) {
    if (hw)
      pc_host_items_hw(a, desc, s, e);
    else
      pc_host_items_libm(a, desc, s, e);
  });
}

static PcHostArgs pc_host_args(const torch::Tensor& q_pad,
                               const torch::Tensor& pos,
                               const torch::Tensor& wts, int64_t k, int64_t L,
                               float* logits, int* freqs) {
  return PcHostArgs{q_pad.data_ptr<float>(), (int)q_pad.size(2),
                    (int)q_pad.size(3),      pos.data_ptr<int>(),
                    pc::unpack(wts.data_ptr<float>(), (int)k, (int)L),
                    logits,                  freqs};
}

// ---------------------------------------------------------------------------
// Entry points. q_pad is (B, C+4, H+8, W+8) and decides the device: the
// kernels above for a GPU tensor, the host build for a CPU tensor (portable
// only). Every other tensor lives where q_pad does.
// ---------------------------------------------------------------------------

static void pc_check_tensor(const torch::Tensor& t, const char* what,
                            bool on_gpu) {
  TORCH_CHECK(t.is_cuda() == on_gpu && t.is_contiguous(), "pc_codec: ", what,
              " must be contiguous on the ", on_gpu ? "GPU" : "CPU",
              ", where q_pad is");
}

static void pc_check(const torch::Tensor& q_pad, const torch::Tensor& pos,
                     const torch::Tensor& wts, int64_t k, int64_t L,
                     bool on_gpu, bool portable) {
  TORCH_CHECK(on_gpu || portable,
              "pc_codec: CPU tensors are served by the portable backend only");
  pc_check_tensor(q_pad, "q_pad", on_gpu);
  pc_check_tensor(pos, "positions", on_gpu);
  pc_check_tensor(wts, "packed weights", on_gpu);
  TORCH_CHECK(k >= 1 && k <= pc::MAX_K, "pc_codec: k must be in [1, ",
              pc::MAX_K, "]");
  TORCH_CHECK(L >= 1 && L <= pc::MAX_L, "pc_codec: L must be in [1, ",
              pc::MAX_L, "]");
  TORCH_CHECK(q_pad.scalar_type() == torch::kFloat32 && q_pad.dim() == 4 &&
                  q_pad.size(1) > 4 && q_pad.size(2) > 8 && q_pad.size(3) > 8,
              "pc_codec: q_pad must be fp32 (B, C+4, H+8, W+8)");
  TORCH_CHECK(q_pad.size(0) >= 1 && q_pad.size(0) <= PC_MAX_B,
              "pc_codec: batch size must be in [1, ", PC_MAX_B, "]");
  TORCH_CHECK(pos.scalar_type() == torch::kInt32 && pos.dim() == 2 &&
                  pos.size(1) == 3,
              "pc_codec: positions must be int32 (n, 3)");
  TORCH_CHECK(wts.scalar_type() == torch::kFloat32 &&
                  wts.numel() == (int64_t)pc::packed_numel((int)k, (int)L),
              "pc_codec: packed weights have the wrong size");
  if (on_gpu) return;  // the kernels test every position themselves
  const int C = (int)q_pad.size(1) - 4, H = (int)q_pad.size(2) - 8,
            W = (int)q_pad.size(3) - 8;
  const int* p = pos.data_ptr<int>();
  for (int64_t i = 0; i < pos.size(0); ++i)
    TORCH_CHECK(p[3 * i] >= 0 && p[3 * i] < C && p[3 * i + 1] >= 0 &&
                    p[3 * i + 1] < H && p[3 * i + 2] >= 0 && p[3 * i + 2] < W,
                "pc_codec host: position ", i, " outside the volume");
}

// logits and freqs are (B, n, L).
static void launch_pc_freqs(const torch::Tensor& q_pad, const int* pos,
                            int64_t n, const torch::Tensor& wts, int64_t k,
                            int64_t L, float* logits, int* freqs,
                            bool portable) {
  if (n == 0) return;
  const int64_t B = q_pad.size(0);
  const int C = (int)q_pad.size(1) - 4, H = (int)q_pad.size(2) - 8,
            W = (int)q_pad.size(3) - 8;
  const int kp = (int)((k + 7) / 8 * 8);
  auto kernel = portable ? pc_freqs_kernel<true> : pc_freqs_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n, (unsigned)B), dim3(PC_THREADS),
                     0, at::cuda::getCurrentCUDAStream(),
                     q_pad.data_ptr<float>(), q_pad.stride(0), C, H, W, pos,
                     wts.data_ptr<float>(), (int)k, kp, (int)L, logits, freqs);
}

// (logits, tables) of every position, both (B, n, L), after pc_check. The
// host build skips the logits unless they are asked for (the kernel always
// writes them) and returns an undefined tensor in their place.
static std::tuple<torch::Tensor, torch::Tensor> pc_tables(
    const torch::Tensor& q_pad, const torch::Tensor& pos,
    const torch::Tensor& wts, int64_t k, int64_t L, bool portable,
    bool want_logits) {
  const bool on_gpu = q_pad.is_cuda();
  const int64_t B = q_pad.size(0), n = pos.size(0);
  torch::Tensor logits;
  if (on_gpu || want_logits) logits = torch::empty({B, n, L}, q_pad.options());
  auto freqs = torch::empty({B, n, L}, pos.options());
  if (on_gpu)
    launch_pc_freqs(q_pad, pos.data_ptr<int>(), n, wts, k, L,
                    logits.data_ptr<float>(), freqs.data_ptr<int>(), portable);
  else
    pc_host_eval(pc_host_args(q_pad, pos, wts, k, L,
                              want_logits ? logits.data_ptr<float>() : nullptr,
                              freqs.data_ptr<int>()),
                 B, q_pad.stride(0), n, 0, n);
  return {logits, freqs};
}

std::tuple<torch::Tensor, torch::Tensor> pc_freqs(torch::Tensor q_pad,
                                                  torch::Tensor pos,
                                                  torch::Tensor wts, int64_t k,
                                                  int64_t L, bool portable) {
  pc_check(q_pad, pos, wts, k, L, q_pad.is_cuda(), portable);
  return pc_tables(q_pad, pos, wts, k, L, portable, true);
}

// Device range encoder: syms (B, n), freqs (B, n, L) -> (B, 8 + 3n + 16)
// bytes: row b holds the little-endian payload length of image b, then its
// payload.
torch::Tensor rc_encode(torch::Tensor syms, torch::Tensor freqs) {
  CHECK_CUDA_CONTIG(syms);
  CHECK_CUDA_CONTIG(freqs);
  TORCH_CHECK(syms.scalar_type() == torch::kInt32 && syms.dim() == 2 &&
                  syms.size(0) >= 1 && syms.size(0) <= PC_MAX_B,
              "rc_encode: symbols must be int32 (B, n), B in [1, ", PC_MAX_B,
              "]");
  TORCH_CHECK(freqs.scalar_type() == torch::kInt32 && freqs.dim() == 3 &&
                  freqs.size(0) == syms.size(0) &&
                  freqs.size(1) == syms.size(1) && freqs.size(2) >= 1 &&
                  freqs.size(2) <= rc::MAX_L,
              "rc_encode: tables must be int32 (B, n, L<=16)");
  const int64_t B = syms.size(0), n = syms.size(1), L = freqs.size(2);
  const int64_t cap = 3 * n + 16;
  auto out = torch::empty({B, 8 + cap}, syms.options().dtype(torch::kUInt8));
  hipLaunchKernelGGL(rc_encode_kernel, dim3((unsigned)B), dim3(RC_CHUNK), 0,
                     at::cuda::getCurrentCUDAStream(), syms.data_ptr<int>(),
                     freqs.data_ptr<int>(), n, (int)L,
                     out.data_ptr<uint8_t>(), (uint64_t)cap);
  return out;
}

// Context model + range encoder: syms (B, n) -> the rows of rc_encode, on
// either device.
torch::Tensor pc_encode(torch::Tensor q_pad, torch::Tensor pos,
                        torch::Tensor syms, torch::Tensor wts, int64_t k,
                        int64_t L, bool portable) {
  const bool on_gpu = q_pad.is_cuda();
  pc_check(q_pad, pos, wts, k, L, on_gpu, portable);
  pc_check_tensor(syms, "symbols", on_gpu);
  const int64_t B = q_pad.size(0), n = pos.size(0);
  TORCH_CHECK(syms.scalar_type() == torch::kInt32 && syms.dim() == 2 &&
                  syms.size(0) == B && syms.size(1) == n,
              "pc_encode: symbols must be int32 (B, n), one per position and "
              "image");
  auto freqs = std::get<1>(pc_tables(q_pad, pos, wts, k, L, portable, false));
  if (on_gpu) return rc_encode(syms, freqs);
  const int64_t cap = 3 * n + 16;
  auto out = torch::zeros({B, 8 + cap}, torch::kUInt8);
  const int* sp = syms.data_ptr<int>();
  const int* fp = freqs.data_ptr<int>();
  uint8_t* op = out.data_ptr<uint8_t>();
  host_parallel_for(0, B, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t b = lo; b < hi; ++b) {
      uint8_t* row = op + b * (8 + cap);
      const uint64_t len = pcb::encode_row(sp + b * n, fp + b * n * L, n,
                                           (int)L, row + 8, (uint64_t)cap);
      for (int i = 0; i < 8; ++i) row[i] = (uint8_t)((len >> (8 * i)) & 0xFF);
    }
  });
  return out;
}

// B decoder states, started by one launch. offs is null for a single image
// (B = 1, the whole of data) and (B + 1) int64 on the device otherwise.
static torch::Tensor decode_state(const torch::Tensor& data,
                                  const int64_t* offs, int64_t B) {
  auto state = torch::empty({B, (int64_t)(sizeof(rc::State) / 8)},
                            data.options().dtype(torch::kInt64));
  hipLaunchKernelGGL(rc_decode_init_kernel, dim3((unsigned)((B + 63) / 64)),
                     dim3(64), 0, at::cuda::getCurrentCUDAStream(),
                     reinterpret_cast<rc::State*>(state.data_ptr<int64_t>()),
                     data.data_ptr<uint8_t>(), (uint64_t)data.numel(), offs,
                     B);
  return state;
}

// Decode n symbols against given tables (n, L) in one launch.
torch::Tensor rc_decode(torch::Tensor data, torch::Tensor freqs) {
  CHECK_CUDA_CONTIG(data);
  CHECK_CUDA_CONTIG(freqs);
  TORCH_CHECK(data.scalar_type() == torch::kUInt8 && data.dim() == 1,
              "rc_decode: data must be uint8 (len,)");
  TORCH_CHECK(freqs.scalar_type() == torch::kInt32 && freqs.dim() == 2 &&
                  freqs.size(1) >= 1 && freqs.size(1) <= rc::MAX_L,
              "rc_decode: tables must be int32 (n, L<=16)");
  const int64_t n = freqs.size(0), L = freqs.size(1);
  auto out = torch::zeros({n}, freqs.options().dtype(torch::kInt64));
  if (n == 0) return out;
  auto state = decode_state(data, nullptr, 1);
  hipLaunchKernelGGL(rc_decode_wave_kernel, dim3(1), dim3(RC_CHUNK), 0,
                     at::cuda::getCurrentCUDAStream(),
                     reinterpret_cast<rc::State*>(state.data_ptr<int64_t>()),
                     data.data_ptr<uint8_t>(), (uint64_t)data.numel(),
                     (const int64_t*)nullptr, freqs.data_ptr<int>(),
                     (const int*)nullptr, n, (int)L, (const float*)nullptr,
                     (float*)nullptr, (int64_t)0, 0, 0, 0,
                     out.data_ptr<int64_t>(), n);
  return out;
}

// What a decode takes beside pc_check's arguments: wave i covers
// pos[offsets[i], offsets[i+1]) in every image, image b's payload is
// data[data_offs[b], data_offs[b+1]). Returns the widest wave.
static int64_t pc_decode_check(const std::vector<int64_t>& offsets, int64_t n,
                               const torch::Tensor& data,
                               const std::vector<int64_t>& data_offs,
                               int64_t B, const torch::Tensor& centers,
                               int64_t L, bool on_gpu) {
  pc_check_tensor(data, "data", on_gpu);
  pc_check_tensor(centers, "centers", on_gpu);
  TORCH_CHECK(data.scalar_type() == torch::kUInt8 && data.dim() == 1,
              "pc_decode: data must be uint8 (len,)");
  TORCH_CHECK(centers.scalar_type() == torch::kFloat32 &&
                  centers.numel() == L,
              "pc_decode: centers must be fp32 (L,)");
  TORCH_CHECK((int64_t)data_offs.size() == B + 1 &&
                  pcb::offsets_ok(data_offs.data(), B, data.numel()),
              "pc_decode: payload offsets must be B+1 values running from 0 "
              "to len(data) without decreasing");
  TORCH_CHECK(offsets.size() >= 1 && offsets.front() == 0 &&
                  offsets.back() == n,
              "pc_decode: wave offsets must run from 0 to n");
  int64_t maxw = 0;
  for (size_t i = 1; i < offsets.size(); ++i) {
    TORCH_CHECK(offsets[i] >= offsets[i - 1],
                "pc_decode: wave offsets must not decrease");
    maxw = std::max(maxw, offsets[i] - offsets[i - 1]);
  }
  return maxw;
}

// Wavefront decode of B images; q_pad is filled in place; returns the
// (B, C, H, W) int64 symbols. GPU: one state init, then two launches per
// wave on the current stream whatever B is, with no host synchronisation:
// pc_freqs over (positions of the wave, images), rc_decode_wave with one
// workgroup per image. B = 1 passes no offsets to the kernels and copies
// none. CPU: pcb::decode_batch over the host build of the model.
torch::Tensor pc_decode(torch::Tensor q_pad, torch::Tensor pos,
                        std::vector<int64_t> offsets, torch::Tensor wts,
                        int64_t k, int64_t L, torch::Tensor data,
                        std::vector<int64_t> data_offs, torch::Tensor centers,
                        bool portable) {
  const bool on_gpu = q_pad.is_cuda();
  pc_check(q_pad, pos, wts, k, L, on_gpu, portable);
  const int64_t B = q_pad.size(0), n = pos.size(0);
  const int64_t maxw =
      pc_decode_check(offsets, n, data, data_offs, B, centers, L, on_gpu);
  const int C = (int)q_pad.size(1) - 4, H = (int)q_pad.size(2) - 8,
            W = (int)q_pad.size(3) - 8;
  auto out = torch::zeros({B, C, H, W}, pos.options().dtype(torch::kInt64));
  if (n == 0) return out;
  if (!on_gpu) {
    auto freqs = torch::empty({B, n, L}, pos.options());
    const PcHostArgs a = pc_host_args(q_pad, pos, wts, k, L, nullptr,
                                      freqs.data_ptr<int>());
    const int64_t q_stride = q_pad.stride(0);
    const pcb::DecodeArgs d{B, n, (int)L, C, H, W, pos.data_ptr<int>(),
                            freqs.data_ptr<int>(), data.data_ptr<uint8_t>(),
                            data_offs.data(), centers.data_ptr<float>(),
                            q_pad.data_ptr<float>(), out.data_ptr<int64_t>()};
    pcb::decode_batch(d, offsets, [&](int64_t lo, int64_t hi) {
      pc_host_eval(a, B, q_stride, n, lo, hi);
    });
    return out;
  }
  auto logits = torch::empty({B, maxw, L}, q_pad.options());
  auto freqs = torch::empty({B, maxw, L}, pos.options());
  torch::Tensor offs_dev;
  const int64_t* offs = nullptr;
  if (B > 1) {
    offs_dev = torch::tensor(data_offs, torch::kInt64).to(data.device());
    offs = offs_dev.data_ptr<int64_t>();
  }
  auto state = decode_state(data, offs, B);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int* p = pos.data_ptr<int>();
  for (size_t i = 1; i < offsets.size(); ++i) {
    const int64_t o = offsets[i - 1], nw = offsets[i] - o;
    if (nw == 0) continue;
    // the wave's tables are compact: (B, nw, L) at the head of the buffers
    launch_pc_freqs(q_pad, p + 3 * o, nw, wts, k, L, logits.data_ptr<float>(),
                    freqs.data_ptr<int>(), portable);
    hipLaunchKernelGGL(rc_decode_wave_kernel, dim3((unsigned)B),
                       dim3(RC_CHUNK), 0, stream,
                       reinterpret_cast<rc::State*>(state.data_ptr<int64_t>()),
                       data.data_ptr<uint8_t>(), (uint64_t)data.numel(), offs,
                       freqs.data_ptr<int>(), p + 3 * o, nw, (int)L,
                       centers.data_ptr<float>(), q_pad.data_ptr<float>(),
                       q_pad.stride(0), C, H, W, out.data_ptr<int64_t>(),
                       (int64_t)C * H * W);
  }
  return out;
}

// ---------------------------------------------------------------------------
// Ragged entry points: the images of a batch differ in (C, H, W). q is the
// flat fp32 value buffer and decides the device; desc is the descriptor
// table (B rows of pcb::DESC values, layout in pc_batch_host.h) and items
// the int32 (n, 4) list of (b, c, h, w). Everything is validated on the
// host before the first launch.
// ---------------------------------------------------------------------------

// -> B. The symbol ranges of desc must tile an output of sum(C_b*H_b*W_b)
// values.
static int64_t pc_ragged_check(const torch::Tensor& q,
                               const std::vector<int64_t>& desc,
                               const torch::Tensor& items,
                               const torch::Tensor& wts, int64_t k, int64_t L,
                               bool on_gpu, bool portable,
                               int64_t* sym_total) {
  TORCH_CHECK(on_gpu || portable,
              "pc_codec: CPU tensors are served by the portable backend only");
  pc_check_tensor(q, "the value buffer", on_gpu);
  pc_check_tensor(items, "items", on_gpu);
  pc_check_tensor(wts, "packed weights", on_gpu);
  TORCH_CHECK(k >= 1 && k <= pc::MAX_K, "pc_codec: k must be in [1, ",
              pc::MAX_K, "]");
  TORCH_CHECK(L >= 1 && L <= pc::MAX_L, "pc_codec: L must be in [1, ",
              pc::MAX_L, "]");
  TORCH_CHECK(q.scalar_type() == torch::kFloat32 && q.dim() == 1,
              "pc_codec: the ragged value buffer must be fp32 (numel,)");
  TORCH_CHECK(items.scalar_type() == torch::kInt32 && items.dim() == 2 &&
                  items.size(1) == 4,
              "pc_codec: items must be int32 (n, 4)");
  TORCH_CHECK(wts.scalar_type() == torch::kFloat32 &&
                  wts.numel() == (int64_t)pc::packed_numel((int)k, (int)L),
              "pc_codec: packed weights have the wrong size");
  TORCH_CHECK(!desc.empty() && desc.size() % pcb::DESC == 0,
              "pc_codec: the descriptor table must hold 5 values per image");
  const int64_t B = (int64_t)desc.size() / pcb::DESC;
  TORCH_CHECK(B <= PC_MAX_B, "pc_codec: batch size must be in [1, ", PC_MAX_B,
              "]");
  int64_t total = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* d = desc.data() + pcb::DESC * b;
    TORCH_CHECK(d[0] >= 1 && d[0] <= 65535 && d[1] >= 1 && d[1] <= 65535 &&
                    d[2] >= 1 && d[2] <= 65535,
                "pc_codec: image ", b, ": C, H, W must be in [1, 65535]");
    total += d[0] * d[1] * d[2];
    TORCH_CHECK(total <= ((int64_t)1 << 40), "pc_codec: the batch holds more "
                "than 2^40 symbols");
  }
  const char* bad = pcb::desc_problem(desc.data(), B, q.numel(), total);
  TORCH_CHECK(bad == nullptr, "pc_codec: descriptor table: ", bad);
  *sym_total = total;
  if (on_gpu) return B;  // the kernels test every item themselves
  const int64_t i = pcb::first_bad_item(items.data_ptr<int>(), items.size(0),
                                        desc.data(), B);
  TORCH_CHECK(i == items.size(0), "pc_codec host: item ", i,
              " names no image or lies outside its image's volume");
  return B;
}

static torch::Tensor pc_desc_tensor(const std::vector<int64_t>& v,
                                    const torch::Tensor& like) {
  return torch::tensor(v, torch::kInt64).to(like.device());
}

static void launch_pc_freqs_ragged(const torch::Tensor& q,
                                   const int64_t* desc_dev, int64_t B,
                                   const int* items, int64_t n,
                                   const torch::Tensor& wts, int64_t k,
                                   int64_t L, float* logits, int* freqs,
                                   bool portable) {
  if (n == 0) return;
  const int kp = (int)((k + 7) / 8 * 8);
  auto kernel =
      portable ? pc_freqs_ragged_kernel<true> : pc_freqs_ragged_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(PC_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(), q.data_ptr<float>(),
                     desc_dev, (int)B, items, wts.data_ptr<float>(), (int)k,
                     kp, (int)L, logits, freqs);
}

// (logits, tables) of every item, both (n, L), after pc_ragged_check.
static std::tuple<torch::Tensor, torch::Tensor> pc_tables_ragged(
    const torch::Tensor& q, const std::vector<int64_t>& desc, int64_t B,
    const torch::Tensor& items, const torch::Tensor& wts, int64_t k,
    int64_t L, bool portable, bool want_logits) {
  const bool on_gpu = q.is_cuda();
  const int64_t n = items.size(0);
  TORCH_CHECK(n <= 0x7fffffff, "pc_codec: ", n, " items are above the 2^31-1 "
              "one launch takes; split the batch");
  torch::Tensor logits;
  if (on_gpu || want_logits) logits = torch::empty({n, L}, q.options());
  auto freqs = torch::empty({n, L}, items.options());
  if (on_gpu) {
    auto desc_dev = pc_desc_tensor(desc, q);
    launch_pc_freqs_ragged(q, desc_dev.data_ptr<int64_t>(), B,
                           items.data_ptr<int>(), n, wts, k, L,
                           logits.data_ptr<float>(), freqs.data_ptr<int>(),
                           portable);
  } else {
    const PcHostArgs a{q.data_ptr<float>(), 0, 0, items.data_ptr<int>(),
                       pc::unpack(wts.data_ptr<float>(), (int)k, (int)L),
                       want_logits ? logits.data_ptr<float>() : nullptr,
                       freqs.data_ptr<int>()};
    pc_host_eval_ragged(a, desc.data(), 0, n);
  }
  return {logits, freqs};
}

std::tuple<torch::Tensor, torch::Tensor> pc_freqs_ragged(
    torch::Tensor q, std::vector<int64_t> desc, torch::Tensor items,
    torch::Tensor wts, int64_t k, int64_t L, bool portable) {
  int64_t total;
  const int64_t B = pc_ragged_check(q, desc, items, wts, k, L, q.is_cuda(),
                                    portable, &total);
  return pc_tables_ragged(q, desc, B, items, wts, k, L, portable, true);
}

// Context model + range encoder of a ragged batch. items are sorted by
// (b, t, c, h, w); image b owns items and syms [starts[b], starts[b+1]).
// Returns the flat rows: image b's starts at pcb::ragged_row_offset(b,
// starts[b]) and holds its 8-byte payload length, then 3 n_b + 16 bytes.
// Two launches on the GPU.
torch::Tensor pc_encode_ragged(torch::Tensor q, std::vector<int64_t> desc,
                               torch::Tensor items,
                               std::vector<int64_t> starts, torch::Tensor syms,
                               torch::Tensor wts, int64_t k, int64_t L,
                               bool portable) {
  const bool on_gpu = q.is_cuda();
  int64_t total;
  const int64_t B =
      pc_ragged_check(q, desc, items, wts, k, L, on_gpu, portable, &total);
  pc_check_tensor(syms, "symbols", on_gpu);
  const int64_t n = items.size(0);
  TORCH_CHECK(syms.scalar_type() == torch::kInt32 && syms.dim() == 1 &&
                  syms.size(0) == n,
              "pc_encode_ragged: symbols must be int32 (n,), one per item");
  TORCH_CHECK((int64_t)starts.size() == B + 1 &&
                  pcb::offsets_ok(starts.data(), B, n),
              "pc_encode_ragged: starts must be B+1 values running from 0 to "
              "n without decreasing");
  if (!on_gpu) {
    const int* it = items.data_ptr<int>();
    for (int64_t b = 0; b < B; ++b)
      for (int64_t i = starts[b]; i < starts[b + 1]; ++i)
        TORCH_CHECK(it[4 * i] == b, "pc_encode_ragged host: item ", i,
                    " lies in the range of image ", b, " but names image ",
                    it[4 * i]);
  }
  auto freqs = std::get<1>(
      pc_tables_ragged(q, desc, B, items, wts, k, L, portable, false));
  auto out = torch::zeros({pcb::ROW_EXTRA * B + 3 * n},
                          syms.options().dtype(torch::kUInt8));
  if (on_gpu) {
    auto starts_dev = pc_desc_tensor(starts, q);
    hipLaunchKernelGGL(rc_encode_ragged_kernel, dim3((unsigned)B),
                       dim3(RC_CHUNK), 0, at::cuda::getCurrentCUDAStream(),
                       syms.data_ptr<int>(), freqs.data_ptr<int>(),
                       starts_dev.data_ptr<int64_t>(), (int)L,
                       out.data_ptr<uint8_t>());
    return out;
  }
  const int* sp = syms.data_ptr<int>();
  const int* fp = freqs.data_ptr<int>();
  uint8_t* op = out.data_ptr<uint8_t>();
  host_parallel_for(0, B, 1, [&](int64_t lo, int64_t hi) {
    pcb::encode_ragged(sp, fp, starts.data(), (int)L, op, lo, hi);
  });
  return out;
}

// Wavefront decode of a ragged batch; q is filled in place; returns the flat
// int64 symbols, image b's at its descriptor's offset. items are sorted by
// (t, b, c, h, w) and seg is the (T*B + 1) segment table. GPU: one state
// init, then two launches per non-empty wave of the merged schedule on the
// current stream, whatever B and whatever the mix, with no host
// synchronisation: pc_freqs_ragged over the wave's items, rc_decode_wave
// ragged with one workgroup per image. CPU: pcb::decode_ragged over the host
// build of the model.
torch::Tensor pc_decode_ragged(torch::Tensor q, std::vector<int64_t> desc,
                               torch::Tensor items, std::vector<int64_t> seg,
                               torch::Tensor wts, int64_t k, int64_t L,
                               torch::Tensor data,
                               std::vector<int64_t> data_offs,
                               torch::Tensor centers, bool portable) {
  const bool on_gpu = q.is_cuda();
  int64_t total;
  const int64_t B =
      pc_ragged_check(q, desc, items, wts, k, L, on_gpu, portable, &total);
  const int64_t n = items.size(0);
  TORCH_CHECK(n <= 0x7fffffff, "pc_codec: ", n, " items are above the 2^31-1 "
              "one launch takes; split the batch");
  TORCH_CHECK(seg.size() >= 1 && (int64_t)(seg.size() - 1) % B == 0,
              "pc_decode_ragged: the segment table must hold T*B + 1 values");
  const int64_t T = (int64_t)(seg.size() - 1) / B;
  TORCH_CHECK(T >= 1 && pcb::offsets_ok(seg.data(), T * B, n),
              "pc_decode_ragged: the segment table must run from 0 to n "
              "without decreasing");
  // the uniform checks of data, centers and the payload offsets
  pc_decode_check({0, n}, n, data, data_offs, B, centers, L, on_gpu);
  auto out = torch::zeros({total}, items.options().dtype(torch::kInt64));
  if (n == 0) return out;
  if (!on_gpu) {
    const int64_t i = pcb::first_misfiled_item(items.data_ptr<int>(),
                                               seg.data(), T, B);
    TORCH_CHECK(i == n, "pc_decode_ragged host: item ", i,
                " lies in the segment of another image");
    auto freqs = torch::empty({n, L}, items.options());
    const PcHostArgs a{q.data_ptr<float>(), 0, 0, items.data_ptr<int>(),
                       pc::unpack(wts.data_ptr<float>(), (int)k, (int)L),
                       nullptr, freqs.data_ptr<int>()};
    const pcb::RaggedDecodeArgs d{
        B, T, (int)L, desc.data(), items.data_ptr<int>(), seg.data(),
        freqs.data_ptr<int>(), data.data_ptr<uint8_t>(), data_offs.data(),
        centers.data_ptr<float>(), q.data_ptr<float>(),
        out.data_ptr<int64_t>()};
    pcb::decode_ragged(d, [&](int64_t lo, int64_t hi) {
      pc_host_eval_ragged(a, desc.data(), lo, hi);
    });
    return out;
  }
  int64_t maxw = 0;
  for (int64_t t = 0; t < T; ++t)
    maxw = std::max(maxw, seg[(t + 1) * B] - seg[t * B]);
  auto logits = torch::empty({maxw, L}, q.options());
  auto freqs = torch::empty({maxw, L}, items.options());
  auto desc_dev = pc_desc_tensor(desc, q);
  auto seg_dev = pc_desc_tensor(seg, q);
  auto offs_dev = pc_desc_tensor(data_offs, q);
  const int64_t* offs = offs_dev.data_ptr<int64_t>();
  auto state = decode_state(data, offs, B);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int* it = items.data_ptr<int>();
  for (int64_t t = 0; t < T; ++t) {
    const int64_t o = seg[t * B], nw = seg[(t + 1) * B] - o;
    if (nw == 0) continue;
    launch_pc_freqs_ragged(q, desc_dev.data_ptr<int64_t>(), B, it + 4 * o, nw,
                           wts, k, L, logits.data_ptr<float>(),
                           freqs.data_ptr<int>(), portable);
    hipLaunchKernelGGL(rc_decode_wave_ragged_kernel, dim3((unsigned)B),
                       dim3(RC_CHUNK), 0, stream,
                       reinterpret_cast<rc::State*>(state.data_ptr<int64_t>()),
                       data.data_ptr<uint8_t>(), (uint64_t)data.numel(), offs,
                       freqs.data_ptr<int>(), it, seg_dev.data_ptr<int64_t>(),
                       t, desc_dev.data_ptr<int64_t>(), (int)L,
                       centers.data_ptr<float>(), q.data_ptr<float>(),
                       out.data_ptr<int64_t>());
  }
  return out;
}

// Host build of the coder step functions alone (CPU tensors, given tables),
// for the tests: (n,) symbols -> the payload bytes, no length prefix.
torch::Tensor rc_encode_host(torch::Tensor syms, torch::Tensor freqs) {
  TORCH_CHECK(!syms.is_cuda() && !freqs.is_cuda() && syms.is_contiguous() &&
                  freqs.is_contiguous(),
              "rc_encode_host: CPU contiguous tensors");
  TORCH_CHECK(syms.scalar_type() == torch::kInt32 && syms.dim() == 1 &&
                  freqs.scalar_type() == torch::kInt32 && freqs.dim() == 2 &&
                  freqs.size(0) == syms.size(0) && freqs.size(1) >= 1 &&
                  freqs.size(1) <= rc::MAX_L,
              "rc_encode_host: int32 (n,) symbols and (n, L<=16) tables");
  const int64_t n = syms.size(0), L = freqs.size(1);
  const int64_t cap = 3 * n + 16;
  auto out = torch::zeros({cap}, torch::kUInt8);
  const int64_t len = (int64_t)pcb::encode_row(
      syms.data_ptr<int>(), freqs.data_ptr<int>(), n, (int)L,
      out.data_ptr<uint8_t>(), (uint64_t)cap);
  TORCH_CHECK(len <= cap, "rc_encode_host: stream overran ", cap, " bytes");
  return out.slice(0, 0, len).clone();
}

torch::Tensor rc_decode_host(torch::Tensor data, torch::Tensor freqs) {
  TORCH_CHECK(!data.is_cuda() && !freqs.is_cuda() && data.is_contiguous() &&
                  freqs.is_contiguous(),
              "rc_decode_host: CPU contiguous tensors");
  TORCH_CHECK(data.scalar_type() == torch::kUInt8 && data.dim() == 1 &&
                  freqs.scalar_type() == torch::kInt32 && freqs.dim() == 2 &&
                  freqs.size(1) >= 1 && freqs.size(1) <= rc::MAX_L,
              "rc_decode_host: uint8 data and int32 (n, L<=16) tables");
  const int64_t n = freqs.size(0), L = freqs.size(1);
  auto out = torch::zeros({n}, torch::kInt32);
  const rc::ByteSource src{data.data_ptr<uint8_t>(), (uint64_t)data.numel()};
  rc::State st;
  rc::decode_start(st, src);
  const int* fp = freqs.data_ptr<int>();
  int* op = out.data_ptr<int>();
  uint32_t cum[rc::MAX_L + 1];
  for (int64_t i = 0; i < n; ++i) {
    rc::cumulate(fp + i * L, (int)L, cum);
    op[i] = rc::decode_cum(st, src, cum, (int)L);
  }
  return out;
}

}  // namespace dsin

