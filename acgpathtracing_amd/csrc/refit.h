// refit.h — in-place vertex updates of a built scene (pt_update_vertices, include/acgpt.h): the tree keeps its topology and node
// order, every box is recomputed from the new vertices.  Kernels in refit.hip; they include the build's headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "lbvh_build.h"

namespace ptd {

// Sum of the inner nodes' surface areas over the root's: the tree-quality measure of pt_update_info.area_ratio (taken against the
// same quantity at the last build).  Summed from per-block partials in a fixed order: the same vertices give the same bits.
// Computed from the tree as it stands (its records and topology); no array of the scene changes.  Synchronous on return.
bool refit_tree_area(const LbvhResult& r, hipStream_t stream, double& area, std::string& err);

// Rewrites r over new vertices (host, n_verts * 4 floats, the pt_set_scene layout) through d_idx (device, the scene's index buffer,
// n_tris * 3): triangle records and the shade records' normals (material words kept), scene box, pad_abs, fp16 space, fp32 node
// boxes, half_area_ratio / half_box_inflation, the quantisation grid.  What the build returns for the same vertices, bit for bit,
// except the two fp16 ratios (summed in a fixed order here, with float atomics in the build).  Afterwards r holds the fp32 nodes
// and no other node array: every derived array (fp16 nodes, experiment formats, top nodes, four-wide and shared-plane records) is
// released and comes back on first use.  area_out: refit_tree_area of the new tree.  Synchronous on return.
bool refit_lbvh(LbvhResult& r, const float* h_verts_xyzw, size_t n_verts, const uint32_t* d_idx, hipStream_t stream, double& area_out,
                std::string& err);

}  // namespace ptd
