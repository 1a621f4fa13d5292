// Error channel of the C ABI: sk_last_error() returns the text of the last failure on
// the calling thread (the Python host raises ValueError / RuntimeError with it).
#include <stdarg.h>
#include <stdio.h>

#include "common.h"

namespace sk {
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
static long long* g_timing = nullptr;
long long* timing_buffer() { return g_timing; }
}  // namespace sk

extern "C" {
int sk_debug_set_timing_buffer(void* device_ptr, size_t bytes) {
    const size_t need = (size_t)sk::kTimingBlocks * 4 * sk::kTimingSlots * sizeof(long long);
    if (device_ptr != nullptr && bytes < need) {
        sk::set_error("sk_debug_set_timing_buffer: %zu bytes, need %zu ([4096][4][16] int64)", bytes, need);
        return SK_ERR_ARG;
    }
    sk::g_timing = (long long*)device_ptr;
    return SK_OK;
}
const char* sk_last_error(void) { return sk::g_err; }
int sk_abi_version(void) { return 34; }  // 34: tile histograms and look-up-table transforms, what equalize() is made of (sk_tile_histograms, sk_apply_tile_luts, sk_equalize_path); 33: exact rank and tap filters with zero / edge / mirror borders (sk_filter_rank, sk_filter_taps, sk_filter_path, sk_filter_tile); 32: exact change of grid by any ratio per axis, nearest / linear / area (sk_resample_volume + workspace query, sk_resample_path); 31: one pooling pass per pyramid level, mode / mean / max by factors of 1 or 2 (sk_pool_volume); 30: dynamic Huffman codes in the deflate encoder (sk_deflate_streams_coded; host: sk_deflate_code_host, sk_deflate_header_host); 29: which instances lie within a distance of each other, the pair table at reach D behind proximity() (sk_instance_proximity + workspace query, sk_instance_proximity_row_values, sk_instance_proximity_reach, sk_instance_proximity_resident); 28: the sparse overlap table of two masks, what relate(), sparse_mask_iou() and compare(sparse=True) read (sk_instance_overlaps + workspace query, sk_instance_overlaps_row_values); 27: geodesic assignment, what split() cuts a fused instance with (sk_geodesic_init, sk_geodesic_rounds, sk_geodesic_finish, sk_geodesic_tiles, sk_geodesic_max_rounds); 26: every skeleton branch traced: node and branch tables of every object, and a given skeleton packed without thinning (sk_skeleton_pack, sk_skeleton_branches_count, sk_skeleton_branches_emit + scratch query, sk_skeleton_nodes_row_values, sk_skeleton_branches_row_values); 25: the image under every instance: intensity moments, extrema and a 256-bin histogram per instance (sk_instance_intensity + sk_instance_intensity_row_values); 24: which kernel a conv or weight-gradient launch runs, as a host query (sk_conv3d_route, sk_conv3d_route_name, sk_train_conv_wgrad_route, sk_train_conv_wgrad_route_name); 23: contacts between instances, the pair table behind contacts() and merge() (sk_instance_contacts + workspace query, sk_instance_contacts_row_values); 22: local thickness, the sphere-painting transform on the distance transform (sk_local_thickness_paint); 21: nearest-instance transform, what grow() is made of (sk_nearest_label, sk_nearest_label_pass); 20: connected pieces of every value of a label volume and their table (sk_label_components + workspace query, sk_component_table + sk_component_table_row_values, sk_apply_piece_lut); 19: compare(): surface voxels of every instance and exact distances between surface voxel sets (sk_instance_surface_count, sk_instance_surface_emit, sk_surface_distances, sk_surface_distance_tile); 18: the marching-cubes mesh of every instance (sk_instance_mesh_count, sk_instance_mesh_emit); 17: exact labelled Euclidean distance transform (sk_label_edt, sk_label_edt_pass); 16: skeleton graph of every object (sk_skeleton_graph + sk_skeleton_graph_row_values); 15: marching-cubes cell classes of every instance (sk_instance_mesh_cells); 14: flood_and_stitch (sk_label_planes + workspace query, sk_plane_overlaps + workspace query, sk_stitch_walk_host); 13: Blosc / LZ4 reader of the reference's stores (sk_lz4_streams, sk_blosc_unshuffle, sk_blosc_plan_host, sk_blosc_decode_host); 12: instance measurements (sk_instance_stats + sk_instance_stats_row_values); 11: --convert (sk_convert_pages_u8); 10: inflate decoder for reading zarr chunks and TIFF strips back (sk_inflate_streams, sk_tiff_undo_predictor); 9: deflate encoder of eval()'s outputs (sk_deflate_streams + bound / workspace queries); 8: dataset statistics of the training command (sk_u8_histogram); 7: Lee thinning of training masks (sk_skeletonize + workspace query, sk_skeletonize_emit); 6: validation matrices (sk_label_soft_skeleton2d, sk_mask_metrics + workspace query); 5: training-crop augmentation (sk_aug_resample, sk_aug_intensity, sk_aug_workspace_bytes, sk_skeleton_to_mask); 4: soft clDice (sk_train_soft_skeleton, sk_train_soft_dice_cldice + workspace queries, sk_train_cldice_term_field / sk_train_cldice_chain); 3: round 3 (sk_debug_set_timing_buffer, sk_mfma_probe, sk_conv3d_box, the 16-bit gradient hand-offs sk_train_interleave2_h / sumpool2_hh / heads_dgrad_f16); 2: round 2 (split mode, fused down conv, bf16 twins)
}
