// Fused kernels of the Keras MNIST CNN trial (mnist_tfcnn.hip): the 3x3 convolution + bias + ReLU forward
// and its weight gradient with SGD or Adam in the epilogue. The two linear layers and the cross-entropy
// run on mlp.hip. The geometry is the trial's and is fixed: 28x28x1 -> 26x26x32 -> 21,632 -> 128 -> 10;
// the batch B is the only runtime size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace katib_hip {
namespace tfcnn {

typedef uint16_t u16;  // bf16 bits

constexpr int IMG = 28 * 28;        // input pixels
constexpr int OW = 26;              // output width = height (3x3, valid)
constexpr int PIX = OW * OW;        // output pixels
constexpr int C = 32;               // output channels
constexpr int F = PIX * C;          // fc1 inputs, order (pixel, channel): Keras' Flatten of NHWC
constexpr int SPLIT = 4;            // workgroups per image, forward and weight gradient
constexpr int CHUNK = PIX / SPLIT;  // 169 output pixels per workgroup
constexpr int NPART = C * 10;       // one weight-gradient partial: 32 x (9 taps + 1 bias)

inline int64_t part_size(int B) { return (int64_t)B * SPLIT * NPART; }

// z [B][676][32] bf16 = relu(conv3x3_valid(x[idx?]) + b). x [rows][784] bf16; ws [9][32] bf16 shadow
// (tap, channel); b [32] fp32.
hipError_t conv_fwd(const u16* x, const int64_t* idx, const u16* ws, const float* b, u16* z, int B, hipStream_t st);
// dW[c][tap] = sum_{b,p} dz[b][p][c] x[idx[b]][p + tap], db[c] = sum dz, reduced over the batch (partials
// part [4 B][320] fp32, summed in slice order), then momentum SGD on w / wm [32][9] and b / bm [32];
// re-emits ws.
hipError_t conv_wgrad_sgd(const u16* dz, const u16* x, const int64_t* idx, float* part, float* w, float* wm, float* b,
                          float* bm, u16* ws, const float* lr, float momentum, int B, hipStream_t st);
// ... and with torch.optim.Adam (mlp_optim.h AdamUpd): m / v [32][9], bm / bv [32], t = step_t[0].
hipError_t conv_wgrad_adam(const u16* dz, const u16* x, const int64_t* idx, float* part, float* w, float* m, float* v,
                           float* b, float* bm, float* bv, u16* ws, const float* lr, const int* step_t, float beta1,
                           float beta2, float eps, int B, hipStream_t st);

}  // namespace tfcnn
}  // namespace katib_hip
