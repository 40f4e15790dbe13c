// The argument check that three stages of the exa_raster ABI share (defined once, in ssim.hip).
#pragma once
#include <stdint.h>

namespace exa_raster_impl {

// B x C x H x W images with a window crop = {x0, y0, w, h} (host memory) inside them; reports through the ABI's status
int check_crop(int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* crop);

}  // namespace exa_raster_impl
