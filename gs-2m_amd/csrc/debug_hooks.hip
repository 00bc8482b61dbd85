// Test hooks of libgs2m_raster.so (include/gs2m_raster.h: gs2m_debug_*): single stages of the rasterizer through the launchers of a
// frame, on caller-made inputs and caller-owned buffers.  Nothing here is on the path of a production call (api.hip).
#include "raster_args.h"

extern "C" {

// Test hook: tile_sort.hip on caller-made spans (no rasterization): per tile {~first, last + 1} as the tile sort records them, the
// emission slots of every span in index order, {id | mask, relative row, depth key, -} per slot and a per-wave row base
// table -> ranges, sorted values, the four quadrant lists and their rows and counts.
int gs2m_debug_tile_sort(int tiles, const unsigned* ranges_raw, unsigned* ranges, const unsigned* slot_sorted, const unsigned* e_rec,
                         const unsigned* wave_rowbase, unsigned* point_list, unsigned* row_tmp, unsigned* qlist,
                         unsigned* qrow, unsigned* qcount, void* stream_) {
    if (tiles < 0 || !ranges_raw || !ranges || !slot_sorted || !e_rec || !wave_rowbase || !point_list || !row_tmp || !qlist || !qrow || !qcount) return GS2M_ERR_INVALID_ARG;
    BinningState b = {};
    b.slot_sorted = const_cast<uint32_t*>(slot_sorted); b.e_rec = reinterpret_cast<uint4*>(const_cast<unsigned*>(e_rec));
    b.point_list = point_list; b.sort_valA = row_tmp; b.qlist = reinterpret_cast<uint2*>(qlist); b.qrow = qrow;
    ImageState im = {};
    im.ranges_raw = const_cast<uint32_t*>(ranges_raw);
    im.ranges = reinterpret_cast<uint2*>(ranges);
    im.qcount = qcount;
    GeomState g = {};
    g.wave_rowbase = const_cast<uint32_t*>(wave_rowbase);
    // the span-class words the sort's kernels pass on to each other (common.h: GS2M_CNT_SPAN_*): zeroed per call, as blockscan_kernel does
    static uint32_t* dbg_counters[64] = {nullptr};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return GS2M_ERR_UNSUPPORTED;
    if (dbg_counters[dev] == nullptr) HIP_TRY(hipMalloc(&dbg_counters[dev], 64 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(dbg_counters[dev], 0, 64 * sizeof(uint32_t), (hipStream_t)stream_));
    g.counters = dbg_counters[dev];
    gs2m_launch_tile_sort((size_t)tiles, tiles, 1, SIZE_MAX, b, im, g, (hipStream_t)stream_);  // (a one-row tile grid; the number of entries is not known here)
    HIP_TRY(hipGetLastError());
    return GS2M_OK;
}

// Test hooks (tests/test_radix_sort_gpu.py): radix_sort.hip on caller-made pairs.  Nothing is allocated here: the caller owns every
// buffer (and can put guard words around each).
int gs2m_debug_radix_temp_bytes(long long n, int total_bits, unsigned long long* bytes) {
    if (n < 0 || !bytes) return GS2M_ERR_INVALID_ARG;
    *bytes = (unsigned long long)gs2m_radix_temp_bytes((size_t)n, total_bits);
    return GS2M_OK;
}

int gs2m_debug_radix_plan(int total_bits, int* npass, int* bits4, int* shift4) {
    if (!npass || !bits4 || !shift4) return GS2M_ERR_INVALID_ARG;
    gs2m_radix_plan(total_bits, npass, bits4, shift4);
    return GS2M_OK;
}

int gs2m_debug_radix_sort(long long n, int total_bits, const unsigned* kin, const unsigned* vin, unsigned* kA, unsigned* vA, unsigned* kB,
                          unsigned* vB, void* temp, unsigned long long temp_bytes, int prezeroed, unsigned* range_raw, const unsigned* ext_hist,
                          void* stream_) {
    if (n < 0 || (n > 0 && (!kin || !kA || !vA || !kB || !vB || !temp))) return GS2M_ERR_INVALID_ARG;
    const hipError_t e = gs2m_radix_sort_pairs(temp, (size_t)temp_bytes, kin, vin, kA, vA, kB, vB, (size_t)n, total_bits, prezeroed != 0,
                                               (hipStream_t)stream_, range_raw, ext_hist);
    return e == hipErrorInvalidValue ? GS2M_ERR_INVALID_ARG : gs2m_status(e);
}

// Test hook (tests/test_block_scans_gpu.py): blockscan_kernel, then rowscan_kernel, through the launchers of a frame on caller-made
// count arrays of n_blocks / n_waves words (a frame has ceil(P / 256) and ceil(P / 64)).  `counters`: 64 words; `landing_out`: the
// GS2M_LAND_* words, here in device memory (8-byte aligned: {num_rendered, heavy units} leave in one store).
int gs2m_debug_block_scans(long long n_blocks, const unsigned* block_tt, const unsigned* block_hu, unsigned* block_pref, unsigned* block_hupref,
                           long long n_waves, const unsigned* wave_rows, unsigned* wave_rowbase, unsigned* counters, unsigned* landing_out,
                           void* stream_) {
    if (n_blocks < 1 || n_blocks > 0x7FFFFFFF / 256 || n_waves < 1 || n_waves > 0x7FFFFFFF / 64) return GS2M_ERR_INVALID_ARG;
    if (!block_tt || !block_hu || !block_pref || !block_hupref || !wave_rows || !wave_rowbase || !counters || !landing_out) return GS2M_ERR_INVALID_ARG;
    if ((uintptr_t)landing_out & 7) return GS2M_ERR_INVALID_ARG;
    GeomState g = {};
    g.block_tt = const_cast<uint32_t*>(block_tt); g.block_hu = const_cast<uint32_t*>(block_hu);
    g.block_pref = block_pref; g.block_hupref = block_hupref;
    g.wave_rows = const_cast<uint32_t*>(wave_rows); g.wave_rowbase = wave_rowbase;
    g.counters = counters;
    gs2m_launch_blockscan((int)(n_blocks * 256), g, landing_out, (hipStream_t)stream_);  // (the launchers count in Gaussians)
    gs2m_launch_rowscan((int)(n_waves * 64), g, landing_out, (hipStream_t)stream_);
    HIP_TRY(hipGetLastError());
    return GS2M_OK;
}

// Test hook (tests/test_emit_gpu.py): the emission stage of binning.hip through the launchers of a frame, in a frame's order, on
// caller-made per-Gaussian arrays: the heavy units counted again (only with the crowded-wave rule off, as the forward does),
// blockscan_kernel, emit_kernel + emit_heavy_kernel + rowscan_kernel.  Nothing is allocated here and nothing is zeroed on the side
// (ZeroJobs is empty: the caller zeroes tile_hist, which the preprocess kernel zeroes in a frame).  `heavy_units` sizes the grid
// of emit_heavy_kernel, as the count the forward reads back does.
int gs2m_debug_emit(int P, int W, int H, int tiles_x, int tile_bits, unsigned int crowded, unsigned int heavy_units, const unsigned* rect,
                    const float* rec, const unsigned* depth_key, const unsigned* block_tt, unsigned* block_hu, unsigned* block_pref,
                    unsigned* block_hupref, unsigned* keys_unsorted, unsigned* e_rec, void* hrec, unsigned* gauss_rows, unsigned* wave_rows,
                    unsigned* wave_rowbase, unsigned* counters, unsigned* tile_hist, unsigned* landing_out, void* stream_) {
    if (P < 1 || W < 1 || H < 1 || tiles_x < 1 || tile_bits < 0 || tile_bits > 32 || heavy_units >= (1u << 22)) return GS2M_ERR_INVALID_ARG;
    if (!rect || !rec || !depth_key || !block_tt || !block_hu || !block_pref || !block_hupref || !keys_unsorted || !e_rec || !hrec || !gauss_rows ||
        !wave_rows || !wave_rowbase || !counters || !tile_hist || !landing_out)
        return GS2M_ERR_INVALID_ARG;
    if (((uintptr_t)landing_out & 7) || ((uintptr_t)rect & 7) || ((uintptr_t)rec & 15) || ((uintptr_t)e_rec & 15) || ((uintptr_t)hrec & 3)) return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream_;
    GeomState g = {};
    g.rect = reinterpret_cast<uint2*>(const_cast<unsigned*>(rect));
    g.rec = reinterpret_cast<float4*>(const_cast<float*>(rec));
    g.depth_key = const_cast<uint32_t*>(depth_key);
    g.block_tt = const_cast<uint32_t*>(block_tt); g.block_hu = block_hu;
    g.block_pref = block_pref; g.block_hupref = block_hupref;
    g.gauss_rows = gauss_rows; g.wave_rows = wave_rows; g.wave_rowbase = wave_rowbase;
    g.counters = counters; g.tile_hist = tile_hist;
    BinningState b = {};
    b.keys_unsorted = keys_unsorted;
    b.e_rec = reinterpret_cast<uint4*>(e_rec);
    b.hrec = reinterpret_cast<HeavyUnit*>(hrec);
    if (crowded == GS2M_CROWDED_OFF) gs2m_launch_recount_heavy(P, g, s);
    gs2m_launch_blockscan(P, g, landing_out, s);
    const ZeroJobs zj = {{nullptr, nullptr, nullptr}, {0, 0, 0}};
    gs2m_launch_emit(P, W, H, tiles_x, tile_bits, g, b, heavy_units, crowded, landing_out, zj, s);
    HIP_TRY(hipGetLastError());
    return GS2M_OK;
}

// Test hook (tests/test_preprocess_gpu.py): preprocess_kernel through the launcher of a frame on caller-made inputs and caller-owned
// outputs.  Nothing is allocated here.  The frame is described as the forward describes it (common.h: gs2m_raster_frame) and held to
// the same rules (raster_args.h: what the forward refuses is refused here), and so is every pointer whose alignment a frame gets from its carved buffers
// (rec, sh_dir: float4 stores; rect: uint2 stores) or from the tensor allocator (rotations: float4 loads).  One side zero-fill
// (ZeroJobs), as the frame's digit histograms are.
int gs2m_debug_preprocess(int P, int D, int M, const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                          const float* opacities, const float* shs, const float* shs_rest, const float* cov3D_precomp,
                          const float* colors_precomp, const float* features, const float* viewmatrix, const float* projmatrix,
                          const float* cam_pos, int W, int H, float tan_fovx, float tan_fovy, int shrink, int* radii, int* observe_zero,
                          float* rec, unsigned* tiles_touched, unsigned* rect, unsigned* block_tt, unsigned* block_hu, unsigned* depth_key,
                          unsigned char* clamped, float* sh_dir, unsigned* zero_words, unsigned long long zero_count, void* stream_) {
    RasterFrame f = gs2m_raster_frame(W, H, tan_fovx, tan_fovy);
    f.P = P; f.D = D; f.M = M; f.scale_modifier = scale_modifier;
    f.means3D = means3D; f.shs = shs; f.shs_rest = shs_rest; f.colors_precomp = colors_precomp; f.opacities = opacities; f.scales = scales;
    f.rotations = rotations; f.cov3D_precomp = cov3D_precomp; f.features = features; f.viewmatrix = viewmatrix; f.projmatrix = projmatrix; f.cam_pos = cam_pos;
    if (P < 1 || (frame_faults(f) & ~FRAME_TILE_COUNT) || !opacities || (shs && !sh_dir)) return GS2M_ERR_INVALID_ARG;
    if (!radii || !rec || !tiles_touched || !rect || !block_tt || !block_hu || !depth_key || !clamped) return GS2M_ERR_INVALID_ARG;
    if (((uintptr_t)rec & 15) || ((uintptr_t)sh_dir & 15) || ((uintptr_t)rect & 7) || ((uintptr_t)rotations & 15)) return GS2M_ERR_INVALID_ARG;
    if (zero_count > 0 && !zero_words) return GS2M_ERR_INVALID_ARG;
    GeomState g = {};
    g.rec = reinterpret_cast<float4*>(rec);
    g.tiles_touched = tiles_touched;
    g.rect = reinterpret_cast<uint2*>(rect);
    g.block_tt = block_tt; g.block_hu = block_hu;
    g.depth_key = depth_key;
    g.clamped = clamped;
    g.sh_dir = sh_dir;
    const ZeroJobs zj = {{zero_words, nullptr, nullptr}, {(size_t)zero_count, 0, 0}};
    gs2m_launch_preprocess(f, radii, observe_zero, g, shrink ? 1 : 0, zj, (hipStream_t)stream_);
    HIP_TRY(hipGetLastError());
    return GS2M_OK;
}

// Test hooks (tests/test_blend_gpu.py): blend_fwd_q.hip / blend_bwd_q.hip through the launchers of a frame on caller-made quadrant
// lists (layout: common.h, BinningState::qlist / qrow).  Nothing is allocated here: the caller owns every buffer.
int gs2m_debug_blend_forward(int W, int H, int fc, const float* bg, const unsigned* ranges, const unsigned* qlist, const unsigned* qcount,
                             const float* rec, float* out_color, float* out_buffer, float* final_T, unsigned* n_contrib, int* observe,
                             unsigned* qlast, void* stream_) {
    if (W < 1 || H < 1 || fc < 0 || fc > GS2M_NUM_FEATURES) return GS2M_ERR_INVALID_ARG;
    if (!bg || !ranges || !qlist || !qcount || !rec || !out_color || !out_buffer || !final_T || !n_contrib || !observe || !qlast) return GS2M_ERR_INVALID_ARG;
    GeomState g = {};
    g.rec = reinterpret_cast<float4*>(const_cast<float*>(rec));
    BinningState b = {};
    b.qlist = reinterpret_cast<uint2*>(const_cast<unsigned*>(qlist));
    ImageState im = {};
    im.ranges = reinterpret_cast<uint2*>(const_cast<unsigned*>(ranges));
    im.qcount = const_cast<uint32_t*>(qcount);
    im.final_T = final_T; im.n_contrib = n_contrib; im.qlast = qlast;
    gs2m_launch_blend_fwd_q(W, H, (W + GS2M_TILE - 1) / GS2M_TILE, (H + GS2M_TILE - 1) / GS2M_TILE, fc, bg, g, b, im, out_color, out_buffer, observe,
                            (hipStream_t)stream_);
    HIP_TRY(hipGetLastError());
    return GS2M_OK;
}

int gs2m_debug_blend_backward(int W, int H, int fc, const float* bg, const unsigned* ranges, const unsigned* qlist, const unsigned* qcount,
                              const unsigned* qrow, const unsigned* qlast, const float* rec, const float* final_T, const unsigned* n_contrib,
                              const float* grad_color, const float* grad_buffer, float* rows, void* stream_) {
    if (W < 1 || H < 1 || fc < 0 || fc > GS2M_NUM_FEATURES) return GS2M_ERR_INVALID_ARG;
    if (!bg || !ranges || !qlist || !qcount || !qrow || !qlast || !rec || !final_T || !n_contrib || !grad_color || !grad_buffer || !rows) return GS2M_ERR_INVALID_ARG;
    GeomState g = {};
    g.rec = reinterpret_cast<float4*>(const_cast<float*>(rec));
    BinningState b = {};
    b.qlist = reinterpret_cast<uint2*>(const_cast<unsigned*>(qlist));
    b.qrow = const_cast<uint32_t*>(qrow);
    ImageState im = {};
    im.ranges = reinterpret_cast<uint2*>(const_cast<unsigned*>(ranges));
    im.qcount = const_cast<uint32_t*>(qcount);
    im.qlast = const_cast<uint32_t*>(qlast);
    im.final_T = const_cast<float*>(final_T); im.n_contrib = const_cast<uint32_t*>(n_contrib);
    gs2m_launch_blend_bwd_q(W, H, (W + GS2M_TILE - 1) / GS2M_TILE, (H + GS2M_TILE - 1) / GS2M_TILE, fc, bg, g, b, im, grad_color, grad_buffer, rows,
                            (hipStream_t)stream_);
    HIP_TRY(hipGetLastError());
    return GS2M_OK;
}

// Test hook (tests/test_gaussian_bwd_gpu.py): gaussian_bwd.hip through the two launchers of a frame, in backward_impl's order, on
// caller-made row layouts and caller-owned outputs.  Nothing is allocated here.  The frame and its gradients are held to the rules of
// raster_args.h (what backward_impl refuses is refused here, and the rules of the inputs that the backward leaves to its forward), and so
// is every pointer whose alignment a frame gets from its carved buffers (sh_dir, hrec), from the aligned scratch block (rows) or
// from the tensor allocator (rotations, the float4 outputs, the split SH tensors), and a null among the arrays the kernels of this
// call read.  heavy_units: >= 0 known on the host, -1 read from counters[GS2M_CNT_HUNITS] on the device; windows: 0 = the
// launcher's own rule, 2 or 3 forced.
int gs2m_debug_gaussian_bwd(int P, int D, int M, const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp,
                            const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                            const float* viewmatrix, const float* projmatrix, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                            const int* radii, int fc, const float* rec, const unsigned* gauss_rows, const unsigned* tiles_touched,
                            const unsigned* wave_rowbase, const unsigned char* clamped, const float* sh_dir, const void* hrec,
                            const unsigned* counters, float* rows, int have_rows, long long heavy_units, int windows, float* dL_dmeans2D,
                            float* dL_dconics, float* dL_dopacities, float* dL_dcolors, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dshs,
                            float* dL_dshs_rest, float* dL_dscales, float* dL_drots, float* dL_dfeatures, void* stream_) {
    auto off16 = [](const void* q) { return (((uintptr_t)q) & 15) != 0; };
    RasterFrame f = gs2m_raster_frame(W, H, tan_fovx, tan_fovy);
    f.P = P; f.D = D; f.M = M; f.fc = fc; f.scale_modifier = scale_modifier;
    f.means3D = means3D; f.shs = shs; f.shs_rest = shs_rest; f.colors_precomp = colors_precomp; f.scales = scales;
    f.rotations = rotations; f.cov3D_precomp = cov3D_precomp; f.viewmatrix = viewmatrix; f.projmatrix = projmatrix; f.cam_pos = campos;
    const RasterGrads d = {dL_dmeans2D, dL_dconics, dL_dopacities, dL_dcolors, dL_dmeans3D, dL_dcov3D, dL_dshs, dL_dshs_rest, dL_dscales, dL_drots, dL_dfeatures};
    if (P < 1 || ((frame_faults(f) | grad_faults(f, d)) & ~(FRAME_IMAGE_SIDE | FRAME_TILE_COUNT))) return GS2M_ERR_INVALID_ARG;
    if (windows != 0 && windows != 2 && windows != 3) return GS2M_ERR_INVALID_ARG;
    if (heavy_units < -1 || heavy_units >= (1ll << 22)) return GS2M_ERR_INVALID_ARG;
    if (!radii || (shs && (!clamped || (D > 0 && !sh_dir))) || (!shs_rest && dL_dshs_rest)) return GS2M_ERR_INVALID_ARG;
    if (have_rows && (!rows || !gauss_rows || !tiles_touched || !wave_rowbase)) return GS2M_ERR_INVALID_ARG;
    if (have_rows && heavy_units != 0 && (!hrec || !counters)) return GS2M_ERR_INVALID_ARG;
    if ((have_rows && off16(rows)) || off16(rotations) || off16(dL_dmeans2D) || off16(dL_dconics) || off16(dL_drots) || off16(sh_dir) || (((uintptr_t)hrec) & 3))
        return GS2M_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream_;
    GeomState g = {};
    g.rec = reinterpret_cast<float4*>(const_cast<float*>(rec));
    g.gauss_rows = const_cast<uint32_t*>(gauss_rows);
    g.tiles_touched = const_cast<uint32_t*>(tiles_touched);
    g.wave_rowbase = const_cast<uint32_t*>(wave_rowbase);
    g.clamped = const_cast<uint8_t*>(clamped);
    g.sh_dir = const_cast<float*>(sh_dir);
    g.counters = const_cast<uint32_t*>(counters);
    BinningState b = {};
    b.hrec = reinterpret_cast<HeavyUnit*>(const_cast<void*>(hrec));
    const int rowf = gs2m_row_floats(fc);
    if (have_rows) gs2m_launch_heavy_reduce(rows, rowf, b, g, heavy_units, s);
    gs2m_launch_gaussian_bwd(f, radii, g, rows, rowf, have_rows != 0, d, s, windows);
    HIP_TRY(hipGetLastError());
    return GS2M_OK;
}

int gs2m_debug_row_floats(int fc) {
    if (fc < 0 || fc > GS2M_NUM_FEATURES) return GS2M_ERR_INVALID_ARG;
    return gs2m_row_floats(fc);
}

int gs2m_debug_layout(int P, int R, int width, int height, gs2m_layout* out) {
    if (!out || P < 0 || R < 0 || width <= 0 || height <= 0) return GS2M_ERR_INVALID_ARG;
    const RasterFrame f = gs2m_raster_frame(width, height, 1.f, 1.f);
    const size_t tiles = (size_t)f.tiles_x * f.tiles_y, N = (size_t)width * height;
    const size_t Pn = P > 0 ? (size_t)P : 1, Rn = R > 0 ? (size_t)R : 1;
    GeomState g = gs2m_carve_geom(nullptr, Pn);
    BinningState b = gs2m_carve_binning(nullptr, Rn, gs2m_binning_temp_bytes(Rn, (int)higher_msb((uint32_t)tiles)), 0);
    ImageState im = gs2m_carve_image(nullptr, N, tiles);
    out->geom_bytes = g.total_bytes;
    out->rec = (uint64_t)(uintptr_t)g.rec;
    out->tiles_touched = (uint64_t)(uintptr_t)g.tiles_touched;
    out->depth_key = (uint64_t)(uintptr_t)g.depth_key;
    out->rect = (uint64_t)(uintptr_t)g.rect;
    out->gauss_rows = (uint64_t)(uintptr_t)g.gauss_rows;
    out->clamped = (uint64_t)(uintptr_t)g.clamped;
    out->wave_rowbase = (uint64_t)(uintptr_t)g.wave_rowbase;
    out->counters = (uint64_t)(uintptr_t)g.counters;
    out->binning_bytes = b.total_bytes;
    out->point_list = (uint64_t)(uintptr_t)b.point_list;
    out->tile_keys = (uint64_t)(uintptr_t)b.tile_keys;
    out->qlist = (uint64_t)(uintptr_t)b.qlist;
    out->qrow = (uint64_t)(uintptr_t)b.qrow;
    out->image_bytes = im.total_bytes;
    out->final_T = (uint64_t)(uintptr_t)im.final_T;
    out->n_contrib = (uint64_t)(uintptr_t)im.n_contrib;
    out->ranges = (uint64_t)(uintptr_t)im.ranges;
    out->qcount = (uint64_t)(uintptr_t)im.qcount;
    return GS2M_OK;
}

}  // extern "C"
