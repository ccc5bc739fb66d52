// Optimizer of an ENAS child (enas_optim.hip): torch.optim.Adam (default flags) over every parameter
// of the child in one launch, which also zeroes the gradient buffers, sums the depthwise partial
// gradients and re-emits the weight images the convolution kernels read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace katib_hip {
namespace enasoptim {

enum Kind : int { kFlat = 0, kConv = 1, kDepthwise = 2 };

// One parameter tensor. p / m / v are the fp32 master and the two Adam states, all in one layout.
//  kFlat       n elements; g is the parameter's .grad (same layout), zeroed after the update.
//  kConv       p / m / v [K][RS][C]; g the fp32 accumulator [K][RS][C8] conv_wgrad adds into (zeroed, pad
//              columns included); img = bf16 [K][RS][C8] with zero pad columns, wt = bf16 [C8][RS][K] or null.
//  kDepthwise  p / m / v [K][RS] (K output channels, RS taps); g the partials [rows][K][RS] dw_wgrad
//              writes in full (not zeroed); img = fp32 tap-major [RS][K].
struct Seg {
  float* p;
  float* g;
  float* m;
  float* v;
  void* img;
  void* wt;
  int kind;
  int K, C, C8, RS;
  int rows;
  int n;      // elements of p
  int tile0;  // first workgroup of this segment in the launch
};

constexpr int kMaxRows = 1024;

// Workgroups a segment needs.
int tiles(const Seg& s);

// counters[0] = t, the number of completed updates (the launch computes with t + 1 and the workgroup that
// draws the last ticket stores t + 1); counters[1] = the ticket word, 0 between launches.
// update = 0: only (re)write the images from p; p, m, v, g and the counters are left alone.
hipError_t launch(const Seg* segs_dev, int nseg, int total_tiles, int32_t* counters, float lr, float beta1,
                  float beta2, float eps, int update, hipStream_t st);

}  // namespace enasoptim
}  // namespace katib_hip
