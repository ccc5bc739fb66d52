// Input builder of an ENAS child layer (enas_concat.hip): ReLU + zero-pad + channel concat of up
// to kMaxSrc bf16 NHWC sources with square maps, forward and backward, one launch per direction.
// With pad8 the output pixel holds Cs = 8 ceil(Ct / 8) channels, the last Cs - Ct of them zero.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace katib_hip {
namespace enasconcat {

constexpr int kMaxSrc = 16;

struct Src {
  const void* x;   // [B][H][H][C] bf16 (backward: read only with relu)
  void* gx;        // backward: [B][H][H][C] bf16, or null (no gradient wanted)
  int H, C;        // map size, channels
  int off, t;      // first output channel; rows / columns of zeros above / left of the map
  int row0;        // backward: first (b, y) row of this source among the rows that get a gradient
  uint32_t magic;  // backward: ceil(2^32 / (C / 8)), chunk -> pixel without a division
};

// Entries n..kMaxSrc-1 carry off = row0 = INT_MAX, so the scans need no count.
struct Table {
  Src s[kMaxSrc];
  int n, B, m, Ct;  // sources, batch, output map size (max H), output channels (sum C)
  int Cs;           // channels of an output pixel: Ct, or 8 ceil(Ct / 8) with pad8
  int nar;          // pad8: the one source with C < 8 among sources with C % 8 == 0, else -1
};

// The narrow source of the shifted path, taken out of the table: the table the shifted kernels get
// holds the other sources only (D', every offset a multiple of 8). Its width is a template parameter.
struct Narrow {
  const void* x;  // [B][H][H][c] bf16, 2-byte aligned
  int H, t;       // map size; rows / columns of zeros above / left of the map
  int o8;         // its channel offset in D', in chunks of 8
};

// Fills off, t, row0, magic and m, Ct, Cs, nar from x, gx, H, C, n, B. Returns false when a size is
// out of range: n, an empty source, B * m * m * max(gs, Cs) >= 2^31, or a row too long for the chunk
// arithmetic.
bool finish(Table& tb, int64_t gs, bool pad8);

// 16-byte path: every C % 8 == 0 and every base 16-byte aligned (and gs % 8 == 0, backward).
bool vector_ok(const Table& tb, const void* dense, int64_t gs, bool backward);
// Shifted 16-byte path (pad8): one narrow source (tb.nar) that wants no gradient and needs 2-byte
// alignment only, every other base 16-byte aligned (and gs % 8 == 0, backward).
bool shift_ok(const Table& tb, const void* dense, int64_t gs, bool backward);

// out [B][m][m][Cs] bf16, every element written once (the pad channels with zeros).
hipError_t launch_fwd(const Table& tb, bool relu, void* out, hipStream_t st);
// gout [B][m][m][Cs] bf16 with pixel stride gs >= Cs; every gx of the table written in full, from
// channels < Ct only.
hipError_t launch_bwd(const Table& tb, bool relu, const void* gout, int gs, hipStream_t st);

}  // namespace enasconcat
}  // namespace katib_hip
