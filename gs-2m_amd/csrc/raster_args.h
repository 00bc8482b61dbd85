// Internal to api.hip (the production calls) and debug_hooks.hip (the test hooks): the argument rules of a frame, each stated ONCE,
// and the few host helpers both files use.
#pragma once
#include "common.h"

#define HIP_TRY(expr)                          \
    do {                                       \
        hipError_t e_ = (expr);                \
        if (e_ != hipSuccess) return GS2M_ERR_HIP; \
    } while (0)

// getHigherMsb (rasterizer_impl.cu:31-44): number of key bits that cover the tile ids
static inline uint32_t higher_msb(uint32_t n) {
    uint32_t msb = sizeof(n) * 4, step = msb;
    while (step > 1) {
        step /= 2;
        if (n >> msb) msb += step; else msb -= step;
    }
    if (n >> msb) msb++;
    return msb;
}

// The SET of rules a frame (frame_faults) and the gradient tensors of its backward (grad_faults) break.  The caller decides which
// bind it and what to answer: the production calls GS2M_ERR_UNSUPPORTED where the library could do it but does not (split SH, sizes),
// the hooks GS2M_ERR_INVALID_ARG throughout; the backward does not ask again what only its forward can have accepted.  Each caller
// adds the checks of what is its own: allocators, buffers, outputs, and in a hook the alignment a frame gets from its carved buffers.
enum : unsigned {
    FRAME_BAD_SHAPE = 1u << 0,     // P < 0, an empty image, a feature count outside 0 .. GS2M_NUM_FEATURES
    FRAME_BAD_INPUTS = 1u << 1,    // P > 0 and: no positions or camera matrices; not exactly one colour or covariance source; bad SH
    FRAME_BAD_SPLIT_SH = 1u << 2,  // split SH: M = 16 only, `rest` (and its gradient) 16-byte aligned, both gradients or neither
    FRAME_IMAGE_SIDE = 1u << 3,    // a side beyond 16 * 65535 pixels (tile coordinates are 16-bit)
    FRAME_TILE_COUNT = 1u << 4,    // more than 2^28 tiles
    FRAME_GAUSSIAN_IDS = 1u << 5,  // P >= 2^28: the sorted values carry a 4-bit quadrant mask above the Gaussian id (binning.hip)
    FRAME_NO_GRADS = 1u << 6,      // a gradient tensor that is always written, or that of a precomputed input, is missing
};
static inline unsigned frame_faults(const RasterFrame& f) {
    unsigned bad = 0;
    if (f.P < 0 || f.W <= 0 || f.H <= 0 || f.fc < 0 || f.fc > GS2M_NUM_FEATURES) bad |= FRAME_BAD_SHAPE;
    if (f.P > 0) {
        if (!f.means3D || !f.viewmatrix || !f.projmatrix) bad |= FRAME_BAD_INPUTS;
        if ((f.shs == nullptr) == (f.colors_precomp == nullptr) || (!f.scales || !f.rotations) == (f.cov3D_precomp == nullptr)) bad |= FRAME_BAD_INPUTS;
        if (f.shs && (f.D < 0 || f.D > 3 || f.M < (f.D + 1) * (f.D + 1) || !f.cam_pos)) bad |= FRAME_BAD_INPUTS;
    }
    if (f.shs_rest && (!f.shs || f.M != 16 || (((uintptr_t)f.shs_rest) & 15))) bad |= FRAME_BAD_SPLIT_SH;
    if (f.W > 16 * 65535 || f.H > 16 * 65535) bad |= FRAME_IMAGE_SIDE;
    if ((size_t)f.tiles_x * (size_t)f.tiles_y > ((size_t)1 << 28)) bad |= FRAME_TILE_COUNT;
    if (f.P >= (1 << GS2M_GID_BITS)) bad |= FRAME_GAUSSIAN_IDS;
    return bad;
}
static inline unsigned grad_faults(const RasterFrame& f, const RasterGrads& d) {
    unsigned bad = 0;
    if (!d.means2D || !d.opacities || !d.means3D || !d.scales || !d.rots || !d.features) bad |= FRAME_NO_GRADS;
    // colors / cov3D may be NULL when the input was not given; shs (and shs_rest) with SH input too: dL/dSH is then not computed
    if ((f.colors_precomp && !d.colors) || (f.cov3D_precomp && !d.cov3D)) bad |= FRAME_NO_GRADS;
    if (f.shs_rest && (((d.shs == nullptr) != (d.shs_rest == nullptr)) || (((uintptr_t)d.shs_rest) & 15))) bad |= FRAME_BAD_SPLIT_SH;
    return bad;
}
