// TEST-ONLY host build for tests/test_box_cull.py: the emulator (emu.cpp, unchanged) in one library with the scene builder, plus two
// entries of its own — the box-cull counters of a BMO_EMU_STATS build, and the box table the scene builder puts into the blob.
// The test compiles this file twice, with -DBMO_BOX_CULL=1 and =0.
#include "../../beamletoptics.jl_amd/csrc/bmo_scene_blob.hpp"

#include "emu.cpp"

extern "C" {
// out[0..7] = g_emu_march (marches started, then how they ended), out[8..15] = g_emu_box (out[8]: candidates the box cull took);
// reset != 0 zeroes them afterwards
void bmo_emu_box_counts(long* out, int reset) {
#if defined(BMO_EMU_STATS)
    for (int q = 0; q < 8; ++q) out[q] = bmo::g_emu_march[q], out[8 + q] = bmo::g_emu_box[q];
    if (reset)
        for (int q = 0; q < 8; ++q) bmo::g_emu_march[q] = bmo::g_emu_box[q] = 0;
#else
    for (int q = 0; q < 16; ++q) out[q] = -1;
#endif
}
int bmo_emu_box_switch() { return BMO_BOX_CULL; }
// The blob's box table of a description: table[6 * s ..] = lo[3], hi[3] of shape s as the kernels read it (inflated), raw[6 * s ..] the
// same box before the margin (shape_box_raw).  Returns the builder's code.
int bmo_emu_box_table(const bmo_scene_desc* d, double* table, double* raw) {
    SceneImage img;
    std::string err;
    if (const int rc = build_scene_image(d, img, err)) return rc;
    const SceneView S = view_of(img.blob.data(), &img.hdr);
    for (int s = 0; s < d->n_shapes; ++s) {
        const ShapeBox b = shape_box_raw(d->shapes, d->children, s);
        for (int a = 0; a < 3; ++a) raw[6 * s + a] = b.lo[a], raw[6 * s + 3 + a] = b.hi[a];
        for (int a = 0; a < 6; ++a) table[6 * s + a] = S.boxes[6 * s + a];
    }
    return BMO_OK;
}
}
