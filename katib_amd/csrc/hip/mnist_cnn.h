// Fused MNIST CNN training kernels (mnist_cnn.hip): conv + bias + ReLU + 2x2 max-pool forward with
// the winner's window position kept, the conv2 data gradient, and the two convolution weight
// gradients with momentum SGD in their epilogue. The geometry is the trial's and is fixed:
// 28x28x1 -> 24x24x20 -> 12x12x20 -> 8x8x50 -> 4x4x50; the batch B is the only runtime size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace katib_hip {
namespace cnn {

typedef uint16_t u16;  // bf16 bits

constexpr int IMG = 28 * 28;          // input pixels
constexpr int C1 = 24;                // conv1 channels, 20 padded to 24
constexpr int P1 = 12 * 12;           // pooled conv1 pixels
constexpr int CO = 50;                // conv2 channels
constexpr int N2 = 64;                // ... padded to 64 in the two bf16 shadows
constexpr int K2 = 25 * C1;           // conv2 reduction: 25 taps x 24 channels
constexpr int K2P = 608;              // ... padded to 19 MFMA steps of 32
constexpr int P2 = 16;                // pooled conv2 pixels
constexpr int F2 = P2 * CO;           // fc1 inputs, order (pooled pixel, channel)
constexpr int KD = 25 * N2;           // conv2 dgrad reduction: 25 taps x 64 channels
constexpr int WG2_IMGS = 8;           // images per conv2 weight-gradient partial
constexpr int WG1_IMGS = 4;           // images per conv1 weight-gradient partial
constexpr int PART2_LD = 608;         // row pitch of a conv2 partial: 600 weights, 1 bias, pad
constexpr int PART1_LD = 640;         // pitch of a conv1 partial: 24 x (25 weights + 1 bias), pad

inline int wg2_slices(int B) { return (B + WG2_IMGS - 1) / WG2_IMGS; }
inline int wg1_slices(int B) { return (B + WG1_IMGS - 1) / WG1_IMGS; }

// p1 [B][12][12][24] bf16 = pool(relu(conv5x5(x[idx?]) + b1)), a1 (may be null) the winner 0..3 per element.
// x [rows][784] bf16; w1s [25][24] bf16 shadow (tap, channel); b1 [24] fp32.
hipError_t conv1_pool_fwd(const u16* x, const int64_t* idx, const u16* w1s, const float* b1, u16* p1, uint8_t* a1,
                          int B, hipStream_t st);
// p2 [B][16][50] bf16 = pool(relu(conv5x5(p1) + b2)), a2 (may be null) likewise.
// w2f [64][608] bf16 shadow, k = (r, s, ci); b2 [50] fp32.
hipError_t conv2_pool_fwd(const u16* p1, const u16* w2f, const float* b2, u16* p2, uint8_t* a2, int B,
                          hipStream_t st);
// dp1 [B][12][12][24] bf16 = (dz2 * w2) [p1 > 0], dz2 = dp2 at each window's winner. w2d [24][25][64] bf16.
hipError_t conv2_dgrad(const u16* dp2, const uint8_t* a2, const u16* w2d, const u16* p1, u16* dp1, int B,
                       hipStream_t st);
// conv2 weight / bias gradient reduced over the batch (partials part [slices][50][608] fp32, summed in
// slice order) and momentum SGD on w2 / w2m [50][600] (co, r, s, ci) and b2 / b2m [50]; re-emits w2f, w2d.
hipError_t conv2_wgrad_sgd(const u16* dp2, const uint8_t* a2, const u16* p1, float* part, float* w2, float* w2m,
                           float* b2, float* b2m, u16* w2f, u16* w2d, const float* lr, float momentum, int B,
                           hipStream_t st);
// conv1 weight / bias gradient (partials part [slices][640] fp32) and momentum SGD on w1 / w1m [24][25],
// b1 / b1m [24]; re-emits w1s. x rows through idx as in the forward.
hipError_t conv1_wgrad_sgd(const u16* dp1, const uint8_t* a1, const u16* x, const int64_t* idx, float* part,
                           float* w1, float* w1m, float* b1, float* b1m, u16* w1s, const float* lr, float momentum,
                           int B, hipStream_t st);

}  // namespace cnn
}  // namespace katib_hip
