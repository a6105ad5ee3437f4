// tile.hpp -- the 64 x 8 x 8 classification tile with its one-voxel halo that the plateau search (extrema.hip) and the
// watershed (watershed.hip) read their neighbourhoods from, and the limit its launch puts on the image.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vh {

constexpr unsigned NAN_BITS = 0x7fc00000u;    // every NaN of the source enters LDS as this one (all of them compare alike)
constexpr unsigned GONE_BITS = 0x7fc00001u;   // a voxel outside the image or with mask == 0

constexpr int TX = 64, TY = 8, TZ = 8;        // outputs of a workgroup (256 threads: one x, two y, eight z each)
constexpr int LX = TX + 2, LY = TY + 2, LZ = TZ + 2;

// workgroups of the classification launch: one per tile
inline int64_t tile_count(int64_t nx, int64_t ny, int64_t nz) {
  return ((nx + TX - 1) / TX) * ((ny + TY - 1) / TY) * ((nz + TZ - 1) / TZ);
}

// Fills tile[LZ * LY * LX] with the bit patterns of the workgroup's voxels and their halo, the sign bit flipped where
// `flip` is 0x80000000 (values seen from the maxima: exact), and ends with the barrier.  Returns whether this thread met
// a NaN on a voxel with mask != 0.  Called by all 256 threads (64 x 4) of the workgroup.
__device__ __forceinline__ bool load_tile(const float* __restrict__ src, const float* __restrict__ mask, unsigned flip,
                                          unsigned* tile, int nx, int ny, int nz) {
  const int tid = threadIdx.y * TX + threadIdx.x;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, z0 = blockIdx.z * TZ;
  const int64_t plane = (int64_t)nx * ny;
  bool saw_nan = false;
  for (int k = tid; k < LZ * LY * LX; k += 256) {
    const int lx = k % LX, ly = (k / LX) % LY, lz = k / (LX * LY);
    const int X = x0 - 1 + lx, Y = y0 - 1 + ly, Z = z0 - 1 + lz;
    unsigned b = GONE_BITS;
    if ((unsigned)X < (unsigned)nx && (unsigned)Y < (unsigned)ny && (unsigned)Z < (unsigned)nz) {
      const int64_t i = (int64_t)Z * plane + (int64_t)Y * nx + X;
      if (!mask || mask[i] != 0.0f) {
        const float v = src[i];
        b = (v == v) ? (__float_as_uint(v) ^ flip) : NAN_BITS;
        saw_nan |= v != v;
      }
    }
    tile[k] = b;
  }
  __syncthreads();
  return saw_nan;
}

}  // namespace vh
