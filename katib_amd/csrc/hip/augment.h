// Batch gather with random crop + horizontal flip (+ table normalisation) in one launch
// (ops/augment.py holds the contract and the torch oracle). One draw per (sample, stream, epoch):
//   w = Philox4x32-10((i lo, i hi, stream, epoch), (seed lo, seed hi)), i = idx[b] the DATA-SET index;
//   k = 2 pad + 1; dx = (w[0] k) >> 32; dy = (w[1] k) >> 32; flip = flip_enabled && (w[2] >> 31);
//   out[b][c][y][x] = value(i, c, y + dy - pad, (flip ? W - 1 - x : x) + dx - pad), fill[c] outside.
//
// Translation mode (rx | ry > 0, pad == 0, NHWC destination): the same draw w, and
//   tx = ((w[0] (2 rx + 1)) >> 32) - rx, ty likewise from w[1], ry: the translation in 1/256 pixel;
//   flip first, then translate; u = 256 x - tx, x0 = u >> 8 (arithmetic), fx = u & 255; v, y0, fy from y, ty;
//   R_n(k) = k < 0 ? -1 - k : (k >= n ? 2 n - 1 - k : k)  (Keras 'reflect');  col(k) = flip ? W - 1 - R_W(k) : R_W(k);
//   a = value(i, c, R_H(y0), col(x0)), b = value(.., R_H(y0), col(x0 + 1)), e = value(.., R_H(y0 + 1), col(x0)),
//   d = value(.., R_H(y0 + 1), col(x0 + 1));
//   out[b][y][x][c] = ((f((256-fy)(256-fx)) a + f((256-fy) fx) b) + (f(fy (256-fx)) e + f(fy fx) d)) 2^-16,
//   f the exact int -> fp32 conversion, every * and + one fp32 operation rounded on its own in this order (no
//   FMA), the result rounded to bf16 last (nearest-even). rx <= 128 W, ry <= 128 H (translate <= 0.5): one
//   reflection reaches every tap. An index outside [0, n_src) gives the fill image exactly, in both modes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace katib_hip {
namespace aug {

enum SrcKind { kSrcU8 = 0, kSrcF32 = 1, kSrcBf16 = 2 };  // [N][H][W][4] u8 + lut | [N][C][H][W] f32 | [N][H][W][C] bf16
// [B][C][H][W] f32 | [B][H][W][C8] bf16, channels C.. zero | [B][H][W][C] bf16, exactly C channels
enum DstKind { kDstNCHW = 0, kDstC8 = 1, kDstNHWC = 2 };

constexpr int kMaxPad = 16;
constexpr int kLutChannels = 4;  // a u8 pixel is one dword

struct Args {
  const void* src;
  const float* lut;          // [C][256], u8 sources only: value = lut[c][byte], fill = lut[c][0]
  const int64_t* idx;        // [B] data-set indices; outside [0, n_src) -> the fill image, nothing read
  void* out;                 // 16-byte aligned
  const int32_t* epoch_ptr;  // device epoch (read by the kernel: a captured graph replays with a new one) or nullptr
  uint32_t epoch_imm;        // the epoch when epoch_ptr == nullptr
  int64_t n_src;
  int B, C, H, W, C8;
  int pad, flip;
  int rx, ry;                // translation mode: largest |tx|, |ty| in 1/256 pixel; both 0 = plain / crop mode
  uint32_t seed_lo, seed_hi, stream;
};

// Forms built: (u8, NCHW), (f32, NCHW), (u8, C8), (bf16, C8) in plain / crop mode, (u8, NHWC) and
// (bf16, NHWC) in plain / crop and in translation mode; anything else is hipErrorInvalidValue.
hipError_t launch(int src_kind, int dst_kind, const Args& a, hipStream_t st);

}  // namespace aug
}  // namespace katib_hip
