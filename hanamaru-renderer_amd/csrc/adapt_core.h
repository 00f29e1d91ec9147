// Adaptive sampling, per lane, host-compilable like noise_core.h: the step from a launch's work item to the tile it renders,
// and the rule that decides whether a tile is rendered on.
//   * A launch under a tile mask (hr_set_tile_mask / hr_select_tiles) covers the ACTIVE 4x4 tiles of the region only.  Its work items are the
//     dense indices 0 .. active - 1: hand-off records, the trace kernel's work units and finer tail, the fix-up lists — everything that is
//     addressed by "tile" — stay on the dense index.  Only where a lane asks for its PIXEL does the index go through the list once
//     (launch_tile), so a path's seed and camera ray are those of its frame pixel (the contract of §4.6) whatever else the launch covers.
//   * LIST is a template parameter of the kernels, not a run-time branch: the forms without a list compile to what they were (the trace
//     kernel pays four VGPR spills for two more SGPRs across its loop, §4.6), the list forms are rows of their own in kernel_variants.h.
//   * The rule: a tile stays active iff at least one of its in-region pixels has e > threshold, e = noise_pixel_error (noise_core.h) of the
//     pixel's moments with the PIXEL's own sampling count — the value hr_read_noise_image returns for it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "device_scene.h"
#include "noise_core.h"

namespace hr {

// tiles a launch covers
template <bool LIST>
HD uint32_t launch_tiles(const RenderParams &rp) { return LIST ? rp.tile_count : rp.tiles_x * rp.tiles_y; }
// dense work-item tile -> the region's tile (what tile_lane_pixel is fed)
template <bool LIST>
HD uint32_t launch_tile(const RenderParams &rp, uint32_t dense) { return LIST ? rp.tile_list[dense] : dense; }

// Pixel pix = 0 .. 15 of the region's tile `tile`: does it keep the tile active?  Pixels of an edge tile that overhang the region hold nothing
// and never do.  moments[reg_h][reg_w][6], counts[reg_h][reg_w] (every in-region count >= 2: the caller has checked).
HD bool adapt_pixel_active(const RenderParams &rp, uint32_t tile, uint32_t pix, const double *moments, const uint32_t *counts, double floor, double threshold) {
    uint32_t px, py, sub;
    tile_lane_pixel(rp, tile, pix * 4u, px, py, sub);
    if (!rp_in_region(rp, px, py)) return false;
    const size_t p = (size_t)py * rp_reg_w(rp) + px;
    return noise_pixel_error(moments + p * 6, (uint64_t)counts[p], floor) > threshold;
}
// The same question asked of an error image e_img[reg_h][reg_w] that is already there (hr_select_tiles_robust: e_R of the sample buckets)
HD bool adapt_pixel_above(const RenderParams &rp, uint32_t tile, uint32_t pix, const double *e_img, double threshold) {
    uint32_t px, py, sub;
    tile_lane_pixel(rp, tile, pix * 4u, px, py, sub);
    if (!rp_in_region(rp, px, py)) return false;
    return e_img[(size_t)py * rp_reg_w(rp) + px] > threshold;
}
// the rule for a whole tile (the device asks one lane per pixel and takes the ballot: select_tiles_kernel, post_kernels.h)
HD bool adapt_tile_active(const RenderParams &rp, uint32_t tile, const double *moments, const uint32_t *counts, double floor, double threshold) {
    bool any = false;
    for (uint32_t pix = 0; pix < 16u; pix++) any = adapt_pixel_active(rp, tile, pix, moments, counts, floor, threshold) || any;
    return any;
}

}  // namespace hr
