// Stand-alone check of csrc/lds_layout.h (no GPU): the dynamic LDS of the one-sided lane machine on an LDS-resident scene, swept over
// node, primitive, triangle, material and light counts and stack bounds up to the caps, for both tree forms:
//   * the regions (stack, nodes, primitive records, shading table, materials, light table) do not overlap and lie in [0, total);
//   * every region is aligned as setup_trace (render_device.h) reads it: 16 bytes for the stack and the scene copy's base, 8 for the
//     light table (doubles), 4 for every table (the copy moves words), and the table offsets are the ones setup_trace derives;
//   * the fitted total never exceeds the fixed layout's, and at the caps it equals it;
//   * what scene_fits_lds* admits, the layout admits.
// With seven arguments — nodes4 prims tris materials lights stack_need solve_block_bytes — it also checks the point of the exercise for
// that scene: two fitted render blocks and one solve block of that size fit a CU's LDS, allocation granule counted, and two blocks of
// the fixed layout do not leave that room. Built with -fsanitize=address,undefined by tests/test_lds_layout_host.py.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../gradient-based-path-tracing_amd/csrc/lds_layout.h"

namespace {
int fail(const char *what, bool wide, const gd::LdsSceneCounts &c, int need) {
    std::printf("FAIL %s: wide %d nodes %d prims %d tris %d materials %d lights %d stack_need %d\n", what, (int)wide, c.num_nodes, c.num_prims, c.num_tris,
                c.num_materials, c.num_lights, need);
    return 1;
}
// the static LDS of gdpt_render_phases (render_device.h: kPhasesStaticLds): 15 + 8 doubles per lane and the chunk table
constexpr int kStaticLds = (15 + 8) * 256 * 8 + 66 * 4;
}

int main(int argc, char **argv) {
    const int fixed_total = gd::kLdsSceneBytes + gd::kLdsSceneLevels * gd::kLdsBlockLanes * 4;
    unsigned long long checked = 0, at_cap = 0, refused = 0;
    for (int wide = 0; wide < 2; wide++) {
        const int node_bytes = wide ? (int)sizeof(DevBvh4Node) : (int)sizeof(DevBvhNode);
        for (int nodes = 1; nodes * node_bytes <= gd::kLdsSceneBytes + node_bytes; nodes += (nodes < 8 ? 1 : 13))
        for (int prims = 0; prims <= 440; prims += (prims < 4 ? 1 : 37))
        for (int tris = 0; tris <= 90; tris += (tris < 3 ? 1 : 11))
        for (int mats = 0; mats <= 20; mats += (mats < 2 ? 1 : 3))
        for (int lights = 0; lights <= 40; lights += (lights < 3 ? 1 : 9))
        for (int need = 0; need <= gd::kLdsSceneLevels + 1; need++) {
            const gd::LdsSceneCounts c{nodes, prims, tris, mats, lights};
            const gd::LdsLayout l = gd::lds_scene_layout(wide != 0, c, need, false), f = gd::lds_scene_layout(wide != 0, c, need, true);
            const long long bytes = (long long)nodes * node_bytes + (long long)prims * (long long)sizeof(DevPrim) + (long long)tris * (long long)sizeof(DevTriShade) +
                                    (long long)mats * (long long)sizeof(GdptMaterial);
            const bool fits = bytes + 8 + (long long)lights * 24 <= gd::kLdsSceneBytes && need <= gd::kLdsSceneLevels;     // scene_fits_lds*
            if (fits && !l.ok) return fail("a scene the routes admit is refused", wide, c, need);
            if (l.ok != f.ok) return fail("the fixed and the fitted layout disagree on the caps", wide, c, need);
            if (!l.ok) { refused++; continue; }
            checked++;
            // the table offsets setup_trace derives from the counts (words: nw, nw + pw, nw + pw + tw, then the next even word)
            const int nw = nodes * node_bytes / 4, pw = prims * (int)sizeof(DevPrim) / 4, tw = tris * (int)sizeof(DevTriShade) / 4, mw = mats * (int)sizeof(GdptMaterial) / 4;
            const int l0 = (nw + pw + tw + mw + 1) & ~1;
            for (const gd::LdsLayout *p : {&l, &f}) {
                if (p->nodes_off != 0 || p->prims_off != nw * 4 || p->tris_off != (nw + pw) * 4 || p->materials_off != (nw + pw + tw) * 4 || p->lights_off != l0 * 4)
                    return fail("table offsets differ from setup_trace's", wide, c, need);
                if (p->scene_end != (l0 + lights * 6) * 4) return fail("end of the copy", wide, c, need);
                if (p->stack_off != 0 || p->scene_off % 16 || (p->scene_off + p->lights_off) % 8 || (p->scene_off + p->nodes_off) % 16 || p->prims_off % 4 ||
                    p->tris_off % 4 || p->materials_off % 4)
                    return fail("alignment", wide, c, need);
                // in order, without overlap: stack | nodes | prims | tris | materials | lights
                if (!(p->stack_off + p->stack_levels * gd::kLdsBlockLanes * 4 == p->scene_off && p->nodes_off <= p->prims_off && p->prims_off <= p->tris_off &&
                      p->tris_off <= p->materials_off && p->materials_off + mw * 4 <= p->lights_off && p->lights_off + lights * 24 == p->scene_end &&
                      p->scene_off + p->scene_end <= p->total))
                    return fail("regions overlap", wide, c, need);
                if (p->stack_levels < need || p->stack_levels < 1 || p->stack_levels > gd::kLdsSceneLevels) return fail("stack levels", wide, c, need);
                if (p->total % 16 || p->total - (p->scene_off + p->scene_end) >= (p == &l ? 16 : gd::kLdsSceneBytes)) return fail("total", wide, c, need);
            }
            if (f.total != fixed_total || f.scene_off != gd::kLdsSceneLevels * gd::kLdsBlockLanes * 4 || f.stack_levels != gd::kLdsSceneLevels)
                return fail("the fixed layout is not the caps", wide, c, need);
            if (l.total > f.total) return fail("the fitted layout exceeds the fixed one", wide, c, need);
            if (l.scene_end > gd::kLdsSceneBytes - 16 && need == gd::kLdsSceneLevels) {
                at_cap++;
                if (l.total != f.total) return fail("at the caps the fitted layout is not the fixed one", wide, c, need);
            }
        }
    }
    {   // a scene that sits on both caps: 159 BVH4 nodes, one primitive record, three lights = 20472 bytes of copy (16 more would not fit), 12 levels
        const int lights = (gd::kLdsSceneBytes - 159 * (int)sizeof(DevBvh4Node) - (int)sizeof(DevPrim)) / 24;
        const gd::LdsSceneCounts c{159, 1, 0, 0, lights};
        const gd::LdsLayout l = gd::lds_scene_layout(true, c, gd::kLdsSceneLevels, false), f = gd::lds_scene_layout(true, c, gd::kLdsSceneLevels, true);
        if (!l.ok || !f.ok || l.total != f.total || l.total != fixed_total) return fail("the scene on both caps", true, c, gd::kLdsSceneLevels);
        at_cap++;
    }
    if (!checked || !at_cap || !refused) { std::printf("a case never occurred: checked %llu at the caps %llu refused %llu\n", checked, at_cap, refused); return 1; }
    if (gd::lds_allocated(1) != gd::kLdsGranule || gd::lds_allocated(gd::kLdsGranule) != gd::kLdsGranule || gd::lds_allocated(gd::kLdsGranule + 1) != 2 * gd::kLdsGranule) {
        std::printf("lds_allocated\n");
        return 1;
    }
    if (argc == 8) {
        const gd::LdsSceneCounts c{std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])};
        const int need = std::atoi(argv[6]), solve = std::atoi(argv[7]);
        const gd::LdsLayout l = gd::lds_scene_layout(true, c, need, false), f = gd::lds_scene_layout(true, c, need, true);
        if (!l.ok) return fail("the scene given does not fit", true, c, need);
        const int fitted = 2 * gd::lds_allocated(kStaticLds + l.total), fixed = 2 * gd::lds_allocated(kStaticLds + f.total);
        std::printf("scene copy %d B, %d stack levels: block %d B (fixed layout %d B); per CU two blocks %d B + solve block %d B = %d B of %d (fixed layout: %d B)\n",
                    l.scene_end, l.stack_levels, kStaticLds + l.total, kStaticLds + f.total, fitted, gd::lds_allocated(solve), fitted + gd::lds_allocated(solve), gd::kLdsPerCu,
                    fixed + gd::lds_allocated(solve));
        if (fitted + gd::lds_allocated(solve) > gd::kLdsPerCu) { std::printf("FAIL two fitted render blocks and the solve block exceed the CU's LDS\n"); return 1; }
        if (fixed + gd::lds_allocated(solve) <= gd::kLdsPerCu) { std::printf("FAIL the fixed layout leaves the same room: the case is vacuous\n"); return 1; }
    } else if (argc != 1) { std::printf("usage: lds_layout_check [nodes4 prims tris materials lights stack_need solve_block_bytes]\n"); return 2; }
    std::printf("lds_layout_check ok: %llu layouts checked, %llu at the caps, %llu refused\n", checked, at_cap, refused);
    return 0;
}
