// materials.h — material edits of a built scene (pt_update_materials, include/acgpt.h): a new material table and assignment, the
// tree untouched.  Kernels in materials.hip; they include the build's headers and change nothing in them.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "lbvh_build.h"

namespace ptd {

// Rewrites every leaf slot's material id — h_ids[prim] (host, n_tris ids in the caller's triangle order), or the slot's own when
// h_ids is null — in its triangle record (r2.z) and, tagged against d_mats as tag_shade_records tags it, in its shade record's .w.
// Then copies v0, e1 and e2 of the records of the triangles light_prims names (caller's indices) to edges, 9 floats each, in
// light_prims' order: the record's single fp32 subtractions, what pt_set_scene's light list computes from the vertices.
// Releases the arrays that copy the records (four-wide and shared-plane records); they come back on first use.  The caller has
// checked every id against the table.  Synchronous on return.
bool update_materials(LbvhResult& r, const DevMaterial* d_mats, const uint32_t* h_ids, const std::vector<uint32_t>& light_prims,
                      std::vector<float>& edges, hipStream_t stream, std::string& err);

}  // namespace ptd
