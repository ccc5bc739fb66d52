// Internal: LDS layout of the stride-1 plane kernels (dw_bwd_plane_body, dwpw_plane_body): the
// row pitch of the staged planes, the lane -> (row, 16-byte quad) map of a wave tile, the
// weight-gradient job map, and a constexpr model of the ds_read_b128 lane groups that proves at
// build time (static_asserts at the end) that every 16-byte LDS read of those kernels is free of
// bank conflicts for the geometries the DARTS configurations run.
//
// ds_read_b128 on gfx950 is serviced in four fixed groups of 16 lanes, one LDS cycle per group
// when its sixteen 16-byte slots are distinct mod 16 (bank = (byte address / 4) mod 64):
//   {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, and the same two sets + 32.
// In units of 4-lane chunks k = lane / 4 the first set is chunks {0, 3, 5, 6} of a half wave and
// the second {1, 2, 4, 7}: the set is the parity of k's three bits and k >> 1 counts the chunks
// inside a set. The tile map below gives every such group one CELL of 8 rows x 2 adjacent quads
// (of one channel); with a row pitch of 2 (mod 4) quads the 8 rows start on the 8 even slots
// mod 16 and the two quads fill the odd ones, whatever the cell's first row, first quad or tap
// offset (all of them shift the 16 slots together).
#pragma once
#include <hip/hip_runtime.h>

namespace katib_hip {

// Row pitch (floats) of an LDS plane the stride-2 paths stage: a multiple of 4 floats, so the
// 4-pixel paths read every tap row as whole 16-byte ds_read_b128 quads from an aligned base, and
// an odd number of quads. (The odd quad count spreads lanes that sit on CONSECUTIVE ROWS over
// the 16-byte slots; the lanes of one ds_read_b128 lane group sit on consecutive rows only under
// the tile map below, not under a row-major pixel order, where a group holds half rows of 4
// different rows. The stride-1 paths therefore use plane_pitch and the tile map.)
__host__ __device__ constexpr int lds_pitch(int w) {
  return (((w + 3) & ~3) >> 2) & 1 ? ((w + 3) & ~3) : ((w + 3) & ~3) + 4;
}
// Row pitch (floats) of an LDS plane read through the tile map (stride 1): the smallest quad
// count >= w / 4 that is 2 (mod 4)
__host__ __device__ constexpr int tile_pitch(int w) {
  const int q = (w + 3) >> 2;
  return 4 * (q + ((2 - q) & 3));
}
// the staged-plane pitch of a plane kernel of stride S
__host__ __device__ constexpr int plane_pitch(int w, int S) { return S == 1 ? tile_pitch(w) : lds_pitch(w); }

// ---- wave tile: lane -> (cell of the wave, row of the cell, quad of the cell's pair) ----------
constexpr int kCellRows = 8, kCellLanes = 16, kWaveCells = 4, kBlockCells = 16;  // 256 threads
__host__ __device__ constexpr int tile_qlo(int lane) { return lane & 1; }
__host__ __device__ constexpr int tile_row(int lane) { return ((lane >> 1) & 1) | (((lane >> 3) & 3) << 1); }
__host__ __device__ constexpr int tile_cell(int lane) {
  return (((lane >> 2) ^ (lane >> 3) ^ (lane >> 4)) & 1) | (((lane >> 5) & 1) << 1);
}
// The four cells of a wave are consecutive work units u = 4 * (wave + 4 * pass) + tile_cell(lane).
// Input-gradient / forward units: u = (c * nrb + rb) * npair + pair, nrb = ceil(rows / 8) row
// blocks, npair = W / 8 quad pairs: at W = 32 a wave covers 8 rows x 8 quads (whole 128-byte
// rows of one channel), at W = 16 16 rows x 4 quads (or 8 rows of two channels in a short band).
struct TileItem {
  int c, row, quad;
};
__host__ __device__ constexpr TileItem tile_item(int u, int lane, int nrb, int npair) {
  const int t = u / npair, pair = u - t * npair, c = t / nrb, rb = t - c * nrb;
  return TileItem{c, rb * kCellRows + tile_row(lane), 2 * pair + tile_qlo(lane)};
}
// Weight-gradient units: u = ((c * K + ky) * nrb + rb) * xp + part. The 16 lanes of a cell are 8
// input rows x 2 interleaved column parts: lane (row, qlo) of part `part` walks the quads
// 2 * (part + i * xp) + qlo, i < npair / xp, so at every step a cell reads 8 rows x 2 adjacent
// quads like the other phases. xp (a power of two dividing npair) splits the row between cells
// when the (c, ky, rb) cells alone would leave a 16-cell pass partly empty.
struct WgradJob {
  int c, ky, row, q0;  // q0: first quad; the walk advances by 2 * xp quads
};
__host__ __device__ constexpr WgradJob wgrad_job(int u, int lane, int K, int nrb, int xp) {
  const int t = u / xp, part = u - t * xp, t2 = t / nrb, rb = t - t2 * nrb, c = t2 / K, ky = t2 - c * K;
  return WgradJob{c, ky, rb * kCellRows + tile_row(lane), 2 * part + tile_qlo(lane)};
}
// column split of the weight-gradient walk: the xp that needs the fewest (pass, step) rounds
__host__ __device__ constexpr int wgrad_parts(int cells, int npair) {
  int best = 1, cost = ((cells + kBlockCells - 1) / kBlockCells) * npair;
  for (int xp = 2; xp <= npair && npair % xp == 0; xp *= 2) {
    const int c = ((cells * xp + kBlockCells - 1) / kBlockCells) * (npair / xp);
    if (c < cost) best = xp, cost = c;
  }
  return best;
}

// ---- build-time model of ds_read_b128 banking ---------------------------------------------------
// hardware lane group of a lane (the table above, NOT derived from tile_cell)
__host__ __device__ constexpr int b128_group(int lane) {
  constexpr int set[8] = {0, 1, 1, 0, 1, 0, 0, 1};
  return 2 * (lane >> 5) + set[(lane >> 2) & 7];
}
// the 16 lanes of each hardware lane group
struct B128Groups {
  int lane[4][16];
};
__host__ __device__ constexpr B128Groups b128_groups() {
  B128Groups t{};
  int n[4] = {0, 0, 0, 0};
  for (int lane = 0; lane < 64; ++lane) t.lane[b128_group(lane)][n[b128_group(lane)]++] = lane;
  return t;
}
// Worst multiplicity over the 4 lane groups of one wave-wide 16-byte read: the largest number
// of distinct addresses that share a 16-byte slot mod 16 inside a group (1 = conflict-free).
// addr[lane] is a float index (a multiple of 4), < 0 for a lane that does not read.
__host__ __device__ constexpr int b128_multiplicity(const int (&addr)[64], const B128Groups& grp) {
  int worst = 0;
  for (int g = 0; g < 4; ++g) {
    int first[16] = {}, cnt[16] = {};
    for (int i = 0; i < 16; ++i) {
      const int a = addr[grp.lane[g][i]];
      if (a < 0) continue;
      const int s = (a >> 2) & 15;
      if (cnt[s] == 0) {
        first[s] = a;
        cnt[s] = 1;
      } else if (a != first[s]) {
        bool dup = false;
        for (int j = 0; j < i; ++j) dup = dup || addr[grp.lane[g][j]] == a;
        if (!dup) ++cnt[s];
      }
      worst = cnt[s] > worst ? cnt[s] : worst;
    }
  }
  return worst;
}
// Worst multiplicity over every 16-byte LDS read a stride-1 (K, DIL) plane kernel issues on a
// W-wide plane with `rows`-row bands: the tap-row quads of the input-gradient / forward gather
// (plane of pitch tile_pitch(W + 2 PAD), NQ quads from the lane's own quad, every tap row), the
// act(in) read (pitch tile_pitch(W)) and both reads of every step of the weight-gradient walk.
__host__ __device__ constexpr int plane_worst_multiplicity(int K, int DIL, int W, int rows) {
  const int PAD = (K - 1) / 2 * DIL, NQ = (4 + 2 * PAD + 3) / 4;
  const int pd = tile_pitch(W + 2 * PAD), pi = tile_pitch(W), odr = rows + 2 * PAD;
  const int nrb = (rows + kCellRows - 1) / kCellRows, npair = W / 8, C = 4;
  const B128Groups grp = b128_groups();
  int worst = 0;
  for (int wave = 0; wave < 4; ++wave) {
    // gather phase: first pass of every wave
    for (int ky = 0; ky < K; ++ky)
      for (int q = 0; q <= NQ; ++q) {  // q == NQ: the act(in) read
        int addr[64] = {};
        for (int lane = 0; lane < 64; ++lane) {
          const int u = 4 * wave + tile_cell(lane);
          const TileItem it = tile_item(u, lane, nrb, npair);
          const bool on = u < C * nrb * npair && it.row < rows;
          addr[lane] = !on ? -1
                       : q < NQ ? (it.c * odr + it.row + 2 * PAD - ky * DIL) * pd + 4 * it.quad + 4 * q
                                : (it.c * rows + it.row) * pi + 4 * it.quad;
        }
        const int m = b128_multiplicity(addr, grp);
        worst = m > worst ? m : worst;
      }
    // weight-gradient walk
    const int xp = wgrad_parts(C * K * nrb, npair);
    for (int step = 0; step < npair / xp; ++step)
      for (int q = 0; q <= NQ; ++q) {
        int addr[64] = {};
        for (int lane = 0; lane < 64; ++lane) {
          const int u = 4 * wave + tile_cell(lane);
          const WgradJob j = wgrad_job(u, lane, K, nrb, xp);
          const bool on = u < C * K * nrb * xp && j.row < rows;
          const int quad = j.q0 + 2 * xp * step;
          addr[lane] = !on ? -1
                       : q < NQ ? (j.c * odr + j.row + 2 * PAD - j.ky * DIL) * pd + 4 * quad + 4 * q
                                : (j.c * rows + j.row) * pi + 4 * quad;
        }
        const int m = b128_multiplicity(addr, grp);
        worst = m > worst ? m : worst;
      }
  }
  return worst;
}

// every lane group is exactly one cell: 16 distinct (row, quad-of-pair) positions of one cell
__host__ __device__ constexpr bool tile_groups_are_cells() {
  for (int g = 0; g < 4; ++g) {
    int cell = -1, mask = 0;
    for (int lane = 0; lane < 64; ++lane) {
      if (b128_group(lane) != g) continue;
      if (cell >= 0 && cell != tile_cell(lane)) return false;
      cell = tile_cell(lane);
      mask |= 1 << (2 * tile_row(lane) + tile_qlo(lane));
    }
    if (mask != 0xffff) return false;
  }
  return true;
}
static_assert(tile_groups_are_cells(), "a ds_read_b128 lane group must be one 8-row x 2-quad cell");
static_assert(tile_pitch(34) == 40 && tile_pitch(36) == 40 && tile_pitch(40) == 40 && tile_pitch(32) == 40 &&
                  tile_pitch(18) == 24 && tile_pitch(20) == 24 && tile_pitch(24) == 24 && tile_pitch(16) == 24,
              "stride-1 plane pitches of the 32- and 16-wide DARTS layers");
// the B5 and darts-gpu.yaml stride-1 geometries: (K, dil) in {3, 5} x {1, 2}, W in {16, 32},
// whole-plane, half-plane and shorter-than-a-cell bands
#define PLANE_CONFLICT_FREE_AT(K, D, W, R) \
  static_assert(plane_worst_multiplicity(K, D, W, R) == 1, \
                "ds_read_b128 bank conflicts in a stride-1 plane kernel: (K, dil, W, band rows) = (" #K ", " #D ", " #W ", " #R ")")
#define PLANE_CONFLICT_FREE(K, D)     \
  PLANE_CONFLICT_FREE_AT(K, D, 32, 32); \
  PLANE_CONFLICT_FREE_AT(K, D, 32, 16); \
  PLANE_CONFLICT_FREE_AT(K, D, 32, 4);  \
  PLANE_CONFLICT_FREE_AT(K, D, 16, 16); \
  PLANE_CONFLICT_FREE_AT(K, D, 16, 8);  \
  PLANE_CONFLICT_FREE_AT(K, D, 16, 2)
PLANE_CONFLICT_FREE(3, 1);
PLANE_CONFLICT_FREE(5, 1);
PLANE_CONFLICT_FREE(3, 2);
PLANE_CONFLICT_FREE(5, 2);
#undef PLANE_CONFLICT_FREE_AT
#undef PLANE_CONFLICT_FREE

}  // namespace katib_hip
