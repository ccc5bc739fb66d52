// Gradient fan-in of an ENAS child layer (enas_fanin.hip): the gradient of one layer output x,
// bf16 NHWC [B][H][H][C], summed over up to kMaxTerms readers in one launch. Term k reads its
// gradient g_k [B][m_k][m_k][*] in place, the producer's C channels from channel off_k on, the map
// t_k = (m_k - H) / 2 pixels in from the top-left corner (the pad of enas_concat.h), through the
// reader's ReLU or not:
//
//   gx[b][y][x][c] = bf16( (x[b][y][x][c] > 0 ? sum_{relu k} g_k[b][y + t_k][x + t_k][off_k + c] : 0)
//                          + sum_{other k} g_k[b][y + t_k][x + t_k][off_k + c] )
//
// fp32 sums in table order, one round-to-nearest-even at the end, every element written once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace katib_hip {
namespace enasfanin {

constexpr int kMaxTerms = 16;

struct Term {
  const void* g;  // bf16, 16-byte aligned
  int gs8;        // pixel stride in chunks of 8 channels
  int m, t;       // map size of g; rows / columns of g above / left of the producer's map
  int off8;       // off / 8: the chunk of a pixel of g that holds the producer's first channel
};

struct Table {
  Term k[kMaxTerms];
  const void* x;   // [B][H][H][C] bf16; read only when relu != 0
  int n, B, H, C8;  // terms, batch, the producer's map size and chunks per pixel
  uint32_t relu;   // bit k: term k comes through a ReLU of x
  uint32_t shift;  // bit k: off_k % 8 == sh != 0, the term is read as two chunks and funnel-shifted
  int sh;          // the one non-zero off % 8 of the launch (0: no shifted term)
  uint32_t magic;  // ceil(2^32 / C8), chunk -> pixel without a division
};

// Fills magic and checks the sizes the kernel's 32-bit indices and chunk arithmetic need (n, B, H, C8,
// m_k >= H, B m_k m_k gs_k < 2^31, a pixel of g_k that holds every chunk read, 16-byte bases).
// Returns a message, or null when the table can be launched.
const char* finish(Table& tb, const void* gx);

// gx [B][H][H][C] bf16, 16-byte aligned
hipError_t launch(const Table& tb, void* gx, hipStream_t st);

}  // namespace enasfanin
}  // namespace katib_hip
