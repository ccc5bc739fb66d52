// Batch gather with random crop + horizontal flip (+ table normalisation) in one launch
// (ops/augment.py holds the contract and the torch oracle). One draw per (sample, stream, epoch):
//   w = Philox4x32-10((i lo, i hi, stream, epoch), (seed lo, seed hi)), i = idx[b] the DATA-SET index;
//   k = 2 pad + 1; dx = (w[0] k) >> 32; dy = (w[1] k) >> 32; flip = flip_enabled && (w[2] >> 31);
//   out[b][c][y][x] = value(i, c, y + dy - pad, (flip ? W - 1 - x : x) + dx - pad), fill[c] outside.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace katib_hip {
namespace aug {

enum SrcKind { kSrcU8 = 0, kSrcF32 = 1, kSrcBf16 = 2 };  // [N][H][W][4] u8 + lut | [N][C][H][W] f32 | [N][H][W][C] bf16
enum DstKind { kDstNCHW = 0, kDstC8 = 1 };               // [B][C][H][W] f32 | [B][H][W][C8] bf16, channels C.. zero

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
  uint32_t seed_lo, seed_hi, stream;
};

// Forms built: (u8, NCHW), (f32, NCHW), (u8, C8), (bf16, C8); any other pair is hipErrorInvalidValue.
hipError_t launch(int src_kind, int dst_kind, const Args& a, hipStream_t st);

}  // namespace aug
}  // namespace katib_hip
