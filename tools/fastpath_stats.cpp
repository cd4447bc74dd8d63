// Host build of the test emulator (tests/emu/emu.cpp) that also prints, after each bounce level's line of BMO_EMU_STATS, how many
// union evaluations that level made, how many of them the one `others_lb` compare decided (sdf_any's early return), and how many
// of those ran in tracing_step's specialised union loop; then the level's outside-march trips on shapes that are no union: those of
// the generic trip and those committed in the same loop (BMO_LEAF_MARCH).  At the end: the totals, how the SDF marches ended, and how
// the marches ended that the box cull takes (BMO_BOX_CULL; built with BMO_EMU_BOX_SHADOW those marches run all the same, to be tallied).
// Driven by tools/fastpath_stats.py; the emulator itself is unchanged.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../beamletoptics.jl_amd/csrc/bmo_lane.hpp"

static int fastpath_fprintf(FILE* f, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int r = vfprintf(f, fmt, ap);
    va_end(ap);
    if (strncmp(fmt, "step ", 5) == 0) {
        static long u0 = 0, f0 = 0, l0 = 0, g0 = 0, s0 = 0;
        const long u = bmo::g_emu_union - u0, q = bmo::g_emu_union_fast - f0, l = bmo::g_emu_union_loop - l0;
        fprintf(f, "         union evals %ld  decided by one compare %ld (%.1f %%)  of them in the fast loop %ld (%.1f %%)\n", u, q,
                100.0 * q / std::max(1L, u), l, 100.0 * l / std::max(1L, u));
        const long g = bmo::g_emu_leaf_outside - g0, s = bmo::g_emu_leaf_loop - s0;
        fprintf(f, "         single-shape outside trips: generic %ld  in the loop %ld (%.1f %%)\n", g, s, 100.0 * s / std::max(1L, g + s));
        u0 = bmo::g_emu_union, f0 = bmo::g_emu_union_fast, l0 = bmo::g_emu_union_loop;
        g0 = bmo::g_emu_leaf_outside, s0 = bmo::g_emu_leaf_loop;
    }
    return r;
}
#define fprintf fastpath_fprintf
#include "../tests/emu/emu.cpp"

extern "C" void bmo_fastpath_totals() {
    printf("total    sdf_any %ld  union loop %ld  single-shape outside trips: generic %ld  in the loop %ld\n", bmo::g_emu_sdf_any,
           bmo::g_emu_union_loop, bmo::g_emu_leaf_outside, bmo::g_emu_leaf_loop);
    const long* m = bmo::g_emu_march;
    const long* b = bmo::g_emu_box;
    printf("marches  started %ld  hit offered %ld  on surface, leaving %ld  t0 > lim at CLASSIFY %ld  receded %ld  t0 > lim later %ld  iteration limit %ld  (on surface, entering %ld)\n",
           m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]);
    printf("box cull marches culled %ld (%.1f %%)  receded %ld  lim at CLASSIFY %ld  lim later %ld  iteration limit %ld  hit / entering / leaving %ld / %ld / %ld\n",
           b[0], 100.0 * b[0] / std::max(1L, m[0]), b[4], b[3], b[5], b[6], b[1], b[7], b[2]);
}
