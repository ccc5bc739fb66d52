// Augmenting batch gather (augment.h): one workgroup per sample, so the sample's index, its Philox
// draw and with them dx, dy and flip are workgroup-uniform - the generator runs once per wave on
// scalar values and the pixel loop sees three scalars.
//
// NCHW fp32 destination: a thread produces 4 consecutive x of every channel - one 16-byte store
// per channel (W % 4 == 0; scalar stores otherwise), and a u8 pixel is one dword load that serves
// all its channels. A flipped row reads the same 4-pixel span in reverse. C8 bf16 destination: a
// thread produces one pixel's 8-channel group, one 16-byte store. The u8 normalisation table
// (C x 256 floats) sits in LDS, filled once per workgroup; an out-of-range pixel reads byte 0 of
// it, which is the fill (the reference pads the raw image with 0 before it normalises).
//
// NHWC bf16 destination (augment_nhwc_k, exactly C channels): a thread produces 8 consecutive bf16 of
// the sample's flat [H*W*C] output, one 16-byte store (H*W*C % 8 == 0; for C = 3 that spans 3-4
// pixels): the tap coordinates of the span's pixels are computed and, for u8, their tap dwords loaded
// once per pixel, up front and without a branch between them, and serve all channels; the elements
// then consume the pixels in order. Otherwise a thread takes one pixel and stores its channels one
// by one. In translation mode tx, ty and flip are uniform, and so are the
// fractions fx, fy (256 x drops out of u & 255) and the four bilinear weights: a pixel costs two
// row and two column reflections, four taps and seven fp32 operations per channel.
#include "augment.h"
#include "philox.h"

namespace katib_hip {
namespace aug {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16;

constexpr int kThreads = 256;

__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }

template <int SRC, int DST>
__global__ __launch_bounds__(kThreads) void augment_k(Args a) {
  __shared__ float slut[kLutChannels * 256];  // referenced by the u8 forms only
  const int b = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, H = a.H, W = a.W;
  const int64_t i = a.idx[b];
  const bool ok = i >= 0 && i < a.n_src;
  const int64_t is = ok ? i : 0;
  const uint32_t epoch = a.epoch_ptr ? (uint32_t)*a.epoch_ptr : a.epoch_imm;
  const tfm::philox_u32x4 w = tfm::philox4x32_10(
      tfm::philox_u32x4{(uint32_t)i, (uint32_t)((uint64_t)i >> 32), a.stream, epoch}, a.seed_lo, a.seed_hi);
  const uint32_t k = 2u * (uint32_t)a.pad + 1u;
  // offsets with the padding already taken off: source = destination + (dx, dy)
  const int dx = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[0] * k) >> 32) - a.pad);
  const int dy = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[1] * k) >> 32) - a.pad);
  const bool flip = __builtin_amdgcn_readfirstlane((int)(a.flip != 0 && (w[2] >> 31) != 0)) != 0;

  if constexpr (SRC == kSrcU8) {
    for (int j = tid; j < C * 256; j += kThreads) slut[j] = a.lut[j];
    __syncthreads();
  }

  if constexpr (DST == kDstNCHW) {
    const int W4 = (W + 3) >> 2;
    const bool vec = (W & 3) == 0;
    float* out = reinterpret_cast<float*>(a.out) + (int64_t)b * C * H * W;
    for (int t = tid; t < H * W4; t += kThreads) {
      const int y = t / W4, x0 = (t - y * W4) * 4;
      const int sy = y + dy;
      const bool rowok = ok && sy >= 0 && sy < H;
      int sx[4];
      bool in[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int x = x0 + q;
        sx[q] = (flip ? W - 1 - x : x) + dx;
        in[q] = rowok && x < W && sx[q] >= 0 && sx[q] < W;
      }
      if constexpr (SRC == kSrcU8) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(a.src) + (is * H + (rowok ? sy : 0)) * W;
        uint32_t px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = in[q] ? row[sx[q]] : 0u;
#pragma unroll
        for (int c = 0; c < kLutChannels; ++c) {
          if (c < C) {
            f32x4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = slut[c * 256 + ((px[q] >> (8 * c)) & 255u)];
            float* o = out + ((int64_t)c * H + y) * W + x0;
            if (vec) {
              *reinterpret_cast<f32x4*>(o) = v;
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (x0 + q < W) o[q] = v[q];
            }
          }
        }
      } else {
        for (int c = 0; c < C; ++c) {
          const float* row = reinterpret_cast<const float*>(a.src) + ((is * C + c) * H + (rowok ? sy : 0)) * W;
          f32x4 v;
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = in[q] ? row[sx[q]] : 0.f;
          float* o = out + ((int64_t)c * H + y) * W + x0;
          if (vec) {
            *reinterpret_cast<f32x4*>(o) = v;
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (x0 + q < W) o[q] = v[q];
          }
        }
      }
    }
  } else {
    const int C8 = a.C8, G = C8 >> 3;
    u16* out = reinterpret_cast<u16*>(a.out) + (int64_t)b * H * W * C8;
    for (int t = tid; t < H * W * G; t += kThreads) {
      const int p = t / G, g = t - p * G;
      const int y = p / W, x = p - y * W;
      const int sy = y + dy, sx = (flip ? W - 1 - x : x) + dx;
      const bool in = ok && sy >= 0 && sy < H && sx >= 0 && sx < W;
      const int64_t sp = in ? (is * H + sy) * W + sx : 0;  // source pixel
      u16 v[8];
      if constexpr (SRC == kSrcU8) {
        const uint32_t px = in ? reinterpret_cast<const uint32_t*>(a.src)[sp] : 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = g * 8 + q;
          v[q] = c < C ? f2bf(slut[(c & 3) * 256 + ((px >> (8 * (c & 3))) & 255u)]) : (u16)0;
        }
      } else {
        const u16* s = reinterpret_cast<const u16*>(a.src) + sp * C;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = g * 8 + q;
          v[q] = (in && c < C) ? s[c] : (u16)0;
        }
      }
      *reinterpret_cast<u32x4*>(out + (int64_t)t * 8) =
          u32x4{v[0] | ((uint32_t)v[1] << 16), v[2] | ((uint32_t)v[3] << 16), v[4] | ((uint32_t)v[5] << 16),
                v[6] | ((uint32_t)v[7] << 16)};
    }
  }
}

__device__ __forceinline__ float bf2f(u16 v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }

// Keras 'reflect' (d c b a | a b c d | d c b a). One reflection covers every tap of the contract
// (translate <= 0.5); the clamp changes nothing there and keeps any other k inside the image.
__device__ __forceinline__ int reflect(int k, int n) {
  k = k < 0 ? -1 - k : (k >= n ? 2 * n - 1 - k : k);
  return min(max(k, 0), n - 1);
}

// The last line of the translation contract. Every * and + is ONE IEEE fp32 operation, rounded on
// its own, in the order written: contraction is off for this expression so that no multiply is
// fused with an add into an FMA. The torch oracle computes it with one op per operation; that is
// what makes kernel == oracle hold bit for bit (torch.equal) although this is floating point.
__device__ __forceinline__ float bilerp(float waa, float wab, float wae, float wad, float a, float b, float e,
                                        float d) {
#pragma clang fp contract(off)
  const float top = waa * a + wab * b;
  const float bot = wae * e + wad * d;
  return (top + bot) * 0x1p-16f;
}

// One pixel's taps: offsets (in pixels) into the sample, the u8 dwords, and whether the single tap
// of plain / crop mode lies inside the image. Translation mode uses all four, a b / e d.
template <int SRC, bool TR>
struct Taps {
  int o[TR ? 4 : 1];
  uint32_t px[TR ? 4 : 1];
  bool in;
};

// NP: pixel slots of a thread's 8-element span, at least (C + 6) / C + 1 (8 for C < 3, else 4).
template <int SRC, bool TR, int NP>
__global__ __launch_bounds__(kThreads) void augment_nhwc_k(Args a) {
  static_assert(SRC == kSrcU8 || SRC == kSrcBf16, "NHWC is built for u8 and bf16 sources");
  __shared__ float slut[kLutChannels * 256];  // referenced by the u8 forms only
  const int b = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, H = a.H, W = a.W;
  const int total = H * W * C;
  const int64_t i = a.idx[b];
  const bool ok = i >= 0 && i < a.n_src;
  u16* out = reinterpret_cast<u16*>(a.out) + (int64_t)b * total;
  if (!ok) {  // the fill image, exactly, with nothing read from the source
    for (int e = tid; e < total; e += kThreads) out[e] = SRC == kSrcU8 ? f2bf(a.lut[(e % C) * 256]) : (u16)0;
    return;
  }
  const uint32_t epoch = a.epoch_ptr ? (uint32_t)*a.epoch_ptr : a.epoch_imm;
  const tfm::philox_u32x4 w = tfm::philox4x32_10(
      tfm::philox_u32x4{(uint32_t)i, (uint32_t)((uint64_t)i >> 32), a.stream, epoch}, a.seed_lo, a.seed_hi);
  const bool flip = __builtin_amdgcn_readfirstlane((int)(a.flip != 0 && (w[2] >> 31) != 0)) != 0;
  // plain / crop: source = destination + (ox, oy), the padding taken off. Translation: u = 256 x - tx,
  // so x0 = u >> 8 = x + ((-tx) >> 8) and fx = u & 255 = (-tx) & 255 for every x; likewise y.
  int ox, oy;
  float waa = 0.f, wab = 0.f, wae = 0.f, wad = 0.f;
  if constexpr (TR) {
    const int tx = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[0] * (2u * (uint32_t)a.rx + 1u)) >> 32) - a.rx);
    const int ty = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[1] * (2u * (uint32_t)a.ry + 1u)) >> 32) - a.ry);
    ox = (-tx) >> 8, oy = (-ty) >> 8;
    const int fx = (-tx) & 255, fy = (-ty) & 255;
    waa = (float)((256 - fy) * (256 - fx)), wab = (float)((256 - fy) * fx);  // exact: at most 65536
    wae = (float)(fy * (256 - fx)), wad = (float)(fy * fx);
  } else {
    const uint32_t k = 2u * (uint32_t)a.pad + 1u;
    ox = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[0] * k) >> 32) - a.pad);
    oy = __builtin_amdgcn_readfirstlane((int)(((uint64_t)w[1] * k) >> 32) - a.pad);
  }
  if constexpr (SRC == kSrcU8) {
    for (int j = tid; j < C * 256; j += kThreads) slut[j] = a.lut[j];
    __syncthreads();
  }
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(a.src) + i * H * W;  // u8: one dword per pixel
  const u16* s16 = reinterpret_cast<const u16*>(a.src) + i * H * W * C;        // bf16: C values per pixel

  auto locate = [&](int y, int x, Taps<SRC, TR>& t) {
    if constexpr (TR) {
      const int r0 = reflect(y + oy, H) * W, r1 = reflect(y + oy + 1, H) * W;
      int c0 = reflect(x + ox, W), c1 = reflect(x + ox + 1, W);
      if (flip) c0 = W - 1 - c0, c1 = W - 1 - c1;
      t.o[0] = r0 + c0, t.o[1] = r0 + c1, t.o[2] = r1 + c0, t.o[3] = r1 + c1;
      t.in = true;
      if constexpr (SRC == kSrcU8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t.px[j] = s32[t.o[j]];
      }
    } else {
      const int sy = y + oy, sx = (flip ? W - 1 - x : x) + ox;
      t.in = sy >= 0 && sy < H && sx >= 0 && sx < W;
      t.o[0] = t.in ? sy * W + sx : 0;
      if constexpr (SRC == kSrcU8) t.px[0] = t.in ? s32[t.o[0]] : 0u;  // byte 0 of the table is the fill
    }
  };
  auto value = [&](const Taps<SRC, TR>& t, int j, int c) -> float {
    if constexpr (SRC == kSrcU8) return slut[c * 256 + ((t.px[j] >> (8 * c)) & 255u)];
    return bf2f(s16[t.o[j] * C + c]);
  };
  auto element = [&](const Taps<SRC, TR>& t, int c) -> u16 {
    if constexpr (TR) {
      return f2bf(bilerp(waa, wab, wae, wad, value(t, 0, c), value(t, 1, c), value(t, 2, c), value(t, 3, c)));
    } else if constexpr (SRC == kSrcU8) {
      return f2bf(value(t, 0, c));
    } else {
      return t.in ? s16[t.o[0] * C + c] : (u16)0;
    }
  };

  if ((total & 7) == 0) {
    for (int g = tid; g < (total >> 3); g += kThreads) {
      const int p0 = (g * 8) / C;
      int c = g * 8 - p0 * C;
      int y = p0 / W, x = p0 - y * W;
      // The span's pixels first, all NP slots without a branch between them, so that their loads
      // are in flight together; a slot past the last pixel repeats the last pixel and is never used.
      Taps<SRC, TR> t[NP];
#pragma unroll
      for (int s = 0; s < NP; ++s) {
        locate(y, x, t[s]);
        if (++x == W) x = 0, ++y;
        if (y == H) y = H - 1, x = W - 1;
      }
      // Then the 8 elements from slot 0; when a pixel's channels are done the slots move down by
      // one (selects on registers: no indexing by a lane's own value, no branch).
      u16 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        v[q] = element(t[0], c);
        const bool next = ++c == C;
        c = next ? 0 : c;
#pragma unroll
        for (int s = 0; s + 1 < NP; ++s) {
#pragma unroll
          for (int j = 0; j < (TR ? 4 : 1); ++j) {
            t[s].o[j] = next ? t[s + 1].o[j] : t[s].o[j];
            t[s].px[j] = next ? t[s + 1].px[j] : t[s].px[j];
          }
          t[s].in = next ? t[s + 1].in : t[s].in;
        }
      }
      *reinterpret_cast<u32x4*>(out + (int64_t)g * 8) =
          u32x4{v[0] | ((uint32_t)v[1] << 16), v[2] | ((uint32_t)v[3] << 16), v[4] | ((uint32_t)v[5] << 16),
                v[6] | ((uint32_t)v[7] << 16)};
    }
  } else {
    Taps<SRC, TR> t;
    for (int p = tid; p < H * W; p += kThreads) {
      const int y = p / W;
      locate(y, p - y * W, t);
      for (int c = 0; c < C; ++c) out[p * C + c] = element(t, c);
    }
  }
}

template <int SRC, int DST>
hipError_t run(const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((augment_k<SRC, DST>), dim3((unsigned)a.B), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

template <int SRC, bool TR>
hipError_t run_nhwc(const Args& a, hipStream_t st) {
  if (a.C < 3)
    hipLaunchKernelGGL((augment_nhwc_k<SRC, TR, 8>), dim3((unsigned)a.B), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL((augment_nhwc_k<SRC, TR, 4>), dim3((unsigned)a.B), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch(int src_kind, int dst_kind, const Args& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.pad < 0 || a.pad > kMaxPad || a.C < 1 || a.H < 1 || a.W < 1) return hipErrorInvalidValue;
  if (src_kind == kSrcU8 && (a.C > kLutChannels || a.lut == nullptr)) return hipErrorInvalidValue;
  if (dst_kind == kDstC8 && (a.C8 % 8 != 0 || a.C8 < a.C)) return hipErrorInvalidValue;
  if (a.rx < 0 || a.ry < 0 || a.rx > 128 * a.W || a.ry > 128 * a.H) return hipErrorInvalidValue;
  const bool tr = a.rx > 0 || a.ry > 0;  // rx = ry = 0 draws tx = ty = 0: the flip-only plain gather
  if (tr && (a.pad != 0 || dst_kind != kDstNHWC)) return hipErrorInvalidValue;
  if (dst_kind == kDstNHWC) {
    if ((int64_t)a.H * a.W * a.C >= (1ll << 31)) return hipErrorInvalidValue;
    if (src_kind == kSrcU8) return tr ? run_nhwc<kSrcU8, true>(a, st) : run_nhwc<kSrcU8, false>(a, st);
    if (src_kind == kSrcBf16) return tr ? run_nhwc<kSrcBf16, true>(a, st) : run_nhwc<kSrcBf16, false>(a, st);
    return hipErrorInvalidValue;
  }
  if (src_kind == kSrcU8 && dst_kind == kDstNCHW) return run<kSrcU8, kDstNCHW>(a, st);
  if (src_kind == kSrcF32 && dst_kind == kDstNCHW) return run<kSrcF32, kDstNCHW>(a, st);
  if (src_kind == kSrcU8 && dst_kind == kDstC8) return run<kSrcU8, kDstC8>(a, st);
  if (src_kind == kSrcBf16 && dst_kind == kDstC8) return run<kSrcBf16, kDstC8>(a, st);
  return hipErrorInvalidValue;
}

}  // namespace aug
}  // namespace katib_hip
