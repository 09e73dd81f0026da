// The apron tile of the windowed kernels (despeckle_clamp_kernel, rectify_clamp_kernel; infill_fill_kernel keeps the
// same loop as its own text, for the timing in DESIGN.md 4.20): a workgroup of frame_lib.h's launch shape stages its
// 64 x 4 pixels with an apron of R pixels in LDS, so a pixel's (2R + 1)^2 taps are LDS reads and every cell is fetched
// once per workgroup, not once per tap.  Internal, like frame_lib.h, which a unit includes first.  The kernel declares
// its own __shared__ arrays of tile_cells<R> and says what one cell loads and stores; the shape of the tile, the walk
// over it and the barrier are here.
#pragma once

namespace vimg_frames {
namespace {

template <int R>
constexpr int tile_width = WAVE_X + 2 * R;      // the tile is row-major: the cell one row down is tile_width<R> on
template <int R>
constexpr int tile_cells = tile_width<R> * (ROWS + 2 * R);

// Calls cell(i, gx, gy) for every cell i of the workgroup's tile, the lanes striding over them (consecutive lanes take
// consecutive cells of a row: contiguous requests), with the image coordinates of the cell - which may lie outside the
// image: the callback tests that and stores what "nothing there" is to its window.  Then the barrier; returns the cell
// of the lane's own pixel.  Every lane of the workgroup calls it, inside the image or not.
template <int R, class Cell>
__device__ inline int stage_tile(Cell cell) {
  const int ox = int(blockIdx.x * WAVE_X) - R, oy = int(blockIdx.y * ROWS) - R;
  for (int i = int(threadIdx.y) * WAVE_X + int(threadIdx.x); i < tile_cells<R>; i += WAVE_X * ROWS)
    cell(i, ox + i % tile_width<R>, oy + i / tile_width<R>);
  __syncthreads();
  return (int(threadIdx.y) + R) * tile_width<R> + int(threadIdx.x) + R;
}

}  // namespace
}  // namespace vimg_frames
