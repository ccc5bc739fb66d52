// Head of an ENAS child (enas_head.hip): global average pooling, dropout, the dense classifier and
// softmax cross-entropy with the accuracy bookkeeping, two launches forward and one backward.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace katib_hip {
namespace enashead {

constexpr int kMaxK = 64;    // classes: one lane each in the softmax wave
constexpr int kMaxC = 4096;  // channels: two fp32 rows of a sample in LDS (32 KB) plus the keep bytes

struct Fwd {
  const void* x;       // [B][HW][C] bf16
  const float* w;      // [K][C]
  const float* bias;   // [K]
  const int64_t* y;    // [B]; a label outside [0, K) is clamped for addressing and never a hit
  const int32_t* step; // device step counter, read with dropout only
  float* feat;         // [B][C] keep ? pooled * scale : 0
  uint8_t* keep;       // [B][C] 1 = kept (all 1 without dropout)
  float* logits;       // [B][K]
  float* dl;           // [B][K] (softmax - onehot) / B
  float* loss_b;       // [B]
  float* hit_b;        // [B] 0 / 1
  int B, HW, C, K;
  uint64_t seed;       // dropout: key, site, round(p 2^32), 1 / (1 - p)
  uint32_t site, thr;
  float scale;
};

// loss_b, hit_b [B] -> out[0] = sum loss_b (/ B with mean), out[1] = sum hit_b, both in a fixed
// order; stats (2 floats, or null) += out; *step (or null) += 1.
struct Sum {
  const float* loss_b;
  const float* hit_b;
  float* out;
  float* stats;
  int32_t* step;
  int B, mean;
};

struct Bwd {
  const float* g;       // upstream gradient of the loss, one float in device memory
  const float* dl;      // [B][K]
  const float* w;       // [K][C]
  const float* feat;    // [B][C]
  const uint8_t* keep;  // [B][C]
  void* dx;             // [B][HW][C] bf16, or null
  float* dw;            // [K][C], or null
  float* db;            // [K], or null
  int B, HW, C, K;
  float mscale;         // scale / HW: dx = bf16(g * keep * mscale * sum_k dl W)
  int S;                // pixel segments per sample (data role), 1 <= S <= HW; segments() by default
};

// 16-byte path: C % 8 == 0 and a 16-byte aligned activation.
bool vector_ok(const void* x, int C);
// Pixel segments per sample of the backward's data role (the rule behind kSegBytes).
int segments(int B, int HW, int C);

hipError_t launch_fwd(const Fwd& a, bool drop, hipStream_t st);
hipError_t launch_sum(const Sum& a, hipStream_t st);
hipError_t launch_bwd(const Bwd& a, hipStream_t st);

}  // namespace enashead
}  // namespace katib_hip
