// strip_masks_main.cpp — ptss_probe_strip_masks (host/host_capi.cpp over csrc/ptstrip.h) as a stand-alone program, for
// tests/test_strip_masks_cpu.py to build with -fsanitize=address,undefined and run: the preset scenes at frame shapes that take
// every path of ptstrip::stripMask (one row, a wrap, more than two rows, a ragged last strip, plane padding, several ranks), a few
// cameras in and out of the domain, and exact-size output buffers so that a write past the last word is caught.
// Prints one line per case: name, enabled, words, xor of the words.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptss_host.h"

static int run(const char* name, const ptss_scene_desc& desc, const ptss_camera& cam, int w, int h, int bandRows, int rank, int world) {
    size_t n = 0;
    int on = 0;
    unsigned long long none = 0;
    if (ptss_probe_strip_masks(&desc, &cam, w, h, bandRows, rank, world, &none, 0, &n, &on, nullptr) == PTSS_HOST_OK) return 1;   // capacity 0: refused, n set
    std::vector<unsigned long long> masks(n);
    std::vector<int> triPos(desc.numTriangles ? desc.numTriangles : 1);
    if (ptss_probe_strip_masks(&desc, &cam, w, h, bandRows, rank, world, masks.data(), masks.size(), &n, &on, triPos.data()) != PTSS_HOST_OK) return 2;
    unsigned long long x = 0;
    for (unsigned long long m : masks) x ^= m;
    std::printf("%s %d %zu %016llx\n", name, on, n, x);
    return 0;
}

int main() {
    int rc = 0;
    for (const char* preset : {"mixed", "lambert", "default"}) {
        ptss_scene* s = nullptr;
        if (ptss_scene_create(preset, &s) != PTSS_HOST_OK) return 3;
        ptss_scene_desc desc;
        if (ptss_scene_describe(s, &desc) != PTSS_HOST_OK) return 4;
        ptss_camera cam;
        ptss_camera_default(&cam);
        char name[64];
        const int shapes[][5] = {{130, 9, 8, 0, 1}, {33, 17, 8, 0, 1}, {20, 40, 8, 0, 1}, {64, 9, 8, 1, 2}, {65, 24, 4, 2, 3}, {1920, 16, 8, 0, 1}, {1, 130, 8, 0, 1}, {70, 8, 8, 2, 3}};
        for (const auto& sh : shapes) {
            std::snprintf(name, sizeof name, "%s-%dx%d", preset, sh[0], sh[1]);
            rc |= run(name, desc, cam, sh[0], sh[1], sh[2], sh[3], sh[4]);
        }
        int moved = 0;
        for (unsigned char key : {'h', 'g', 'w', 'q'}) ptss_camera_move(&cam, key, &moved);
        rc |= run("turned", desc, cam, 256, 64, 8, 0, 1);
        cam.position.x = 3e7f;
        rc |= run("far", desc, cam, 256, 64, 8, 0, 1);
        cam.position.x = 1e30f;
        cam.rotation.w = 0.0f / 1.0f;
        cam.zNear = 0.0f;
        rc |= run("degenerate", desc, cam, 256, 64, 8, 0, 1);
        ptss_scene_destroy(s);
    }
    return rc;
}
