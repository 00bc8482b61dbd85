// The display transfer of the 8-bit outputs, shared by mesh_view.hip (the shaded views) and mesh_bake.hip (the base-colour
// texture): one copy of the sRGB encode.  fp64, as written.
#pragma once
#include <math.h>

namespace mesh_raster {

__device__ __forceinline__ double encode(double x, int srgb) {
    if (!srgb) return x;
    return x <= 0.0031308 ? 12.92 * x : 1.055 * pow(x, 1.0 / 2.4) - 0.055;
}

// its inverse, for the textures the viewer reads back: the linear branch up to encode's own value at the knee
__device__ __forceinline__ double decode(double e, int srgb) {
    if (!srgb) return e;
    return e <= 12.92 * 0.0031308 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4);
}

}  // namespace mesh_raster
