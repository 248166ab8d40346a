// lds_layout.h — dynamic LDS of the one-sided lane machine on an LDS-resident scene (gdpt_render_phases<.., LDS_SCENE = true, ..>), no
// HIP dependency: render_kernels.hip lays a launch out with it, tests/lds_layout_check.cpp sweeps it on the host.
//
// A block's dynamic LDS holds the traversal stack (one column of `stack_levels` slots per lane) and, behind it, the scene copy:
//   [0, scene_off)                stack_levels x kLdsBlockLanes ints, at the (16-byte aligned) base of the dynamic segment, where the
//                                 kernels that walk the scene from HBM have theirs: a lane's column pointer stays tid * 4 + a constant
//   [scene_off, total)            nodes | primitive records | shading table | materials | (pad to 8) light table, in the order and at
//                                 the offsets (from scene_off) setup_trace (render_device.h) copies them to, rounded up to 16
// Both sizes follow the scene: the bytes its tables take, and the host-verified stack bound of the tree the route walks. The caps the
// routes test (scene_fits_lds*: kLdsSceneBytes, kLdsSceneLevels) stay, and the test knob lds_fixed_layout asks for exactly them — the
// amounts every scene was given before — from the same kernel.
#pragma once
#include "device_scene.h"
#include "../../include/gdpt.h"

namespace gd {

constexpr int kLdsSceneBytes = 20 * 1024;     // nodes + prims + shading table + materials of a "small" scene
constexpr int kLdsSceneLevels = 12;           // stack slots per lane when the scene is LDS-resident: the cap
constexpr int kLdsBlockLanes = 256;           // lanes of a block (render_device.h: kBlock)
constexpr int kLdsPerCu = 160 * 1024;         // gfx950
constexpr int kLdsGranule = 1280;             // ... allocated in units of 320 dwords

struct LdsSceneCounts { int num_nodes, num_prims, num_tris, num_materials, num_lights; };   // num_nodes: of the form that is walked

struct LdsLayout {
    int stack_off, stack_levels;   // stack_off = 0
    int scene_off;                 // = the stack's bytes, a multiple of 1 KB
    int nodes_off, prims_off, tris_off, materials_off, lights_off;     // bytes from scene_off
    int scene_end;                 // end of the light table, from scene_off
    int total;                     // dynamic LDS bytes of the launch
    bool ok;                       // the scene is within the caps
};

// wide: the BVH4 form is walked (else the BVH2). stack_need: wide_stack_need / bvh_depth of the scene (the bound on the number of
// entries a lane's stack ever holds). A walk pushes before it pops and never touches a slot at or above the bound (trav_push / trav_pop;
// the leaf cursor lives in the leaf reference, not on the stack), so `stack_need` slots are enough; one is kept for a tree without any.
inline LdsLayout lds_scene_layout(bool wide, const LdsSceneCounts &c, int stack_need, bool fixed) {
    LdsLayout l{};
    const long long node_bytes = wide ? (long long)sizeof(DevBvh4Node) : (long long)sizeof(DevBvhNode);
    const long long nb = (long long)c.num_nodes * node_bytes, pb = (long long)c.num_prims * (long long)sizeof(DevPrim);
    const long long tb = (long long)c.num_tris * (long long)sizeof(DevTriShade), mb = (long long)c.num_materials * (long long)sizeof(GdptMaterial);
    const long long l0 = (nb + pb + tb + mb + 7) & ~7LL;              // (setup_trace: the light table starts on an even word)
    const long long end = l0 + (long long)c.num_lights * 24;
    l.ok = c.num_nodes > 0 && c.num_prims >= 0 && c.num_tris >= 0 && c.num_materials >= 0 && c.num_lights >= 0 &&
           end <= kLdsSceneBytes && stack_need >= 0 && stack_need <= kLdsSceneLevels;
    if (!l.ok) return l;
    l.nodes_off = 0; l.prims_off = (int)nb; l.tris_off = (int)(nb + pb); l.materials_off = (int)(nb + pb + tb); l.lights_off = (int)l0;
    l.scene_end = (int)end;
    l.stack_off = 0;
    l.stack_levels = fixed ? kLdsSceneLevels : (stack_need < 1 ? 1 : stack_need);
    l.scene_off = l.stack_levels * kLdsBlockLanes * (int)sizeof(int);
    l.total = l.scene_off + (fixed ? kLdsSceneBytes : (int)((end + 15) & ~15LL));
    return l;
}

// LDS a CU allocates for a block that asks for `bytes`.
inline int lds_allocated(int bytes) { return (bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule; }

} // namespace gd
