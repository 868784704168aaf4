// Prints what psn::ctx_layout lays out, one JSON line per case
// (tests/test_ctx_layout.py checks the lines against the layout's rules). Links
// psn_lk_layout.cpp and nothing else of the library: no GPU, no libpsn_lk.so.
//
//   ctx_layout_dump CASE...            CASE = SCALE/CAP[/WxH,SLOTS]...  (a class per WxH,SLOTS)
//   ctx_layout_dump --plan SRC DST X   psn_lk_resize_plan(SRC, DST, .., X): {"ofs": [..], "coef": [..]}
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "psn_lk_layout.h"

static void print_ints(const char *key, const int *v, size_t n) {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < n; i++) printf("%s%d", i ? ", " : "", v[i]);
    printf("]");
}

// FNV-1a over the table's ints, each as four little-endian bytes
static uint64_t fnv1a(const std::vector<int> &v) {
    uint64_t h = 1469598103934665603ull;
    for (int x : v)
        for (int b = 0; b < 4; b++) h = (h ^ (((uint32_t)x >> (8 * b)) & 0xffu)) * 1099511628211ull;
    return h;
}

static void run_case(const char *text) {
    double scale = 0;
    int cap = 0, used = 0;
    if (sscanf(text, "%lf/%d%n", &scale, &cap, &used) != 2) {
        fprintf(stderr, "bad case %s\n", text);
        exit(2);
    }
    std::vector<psn_lk_frame_class> cls;
    for (const char *p = text + used; *p == '/';) {
        psn_lk_frame_class k{};
        int n = 0;
        if (sscanf(p, "/%dx%d,%d%n", &k.width, &k.height, &k.ring_slots, &n) != 3) {
            fprintf(stderr, "bad class in %s\n", text);
            exit(2);
        }
        cls.push_back(k);
        p += n;
    }
    // every output starts from a mark: a refused input must leave them as they are
    constexpr int kMark = -12345;
    psn::PlanCfg cfg;
    cfg.width = cfg.height = cfg.user_slots = cfg.nslots = cfg.nlevels = cfg.ncls = kMark;
    std::vector<psn::FrameClass> fcls;
    std::vector<int> slot_fcls;
    size_t pyr_bytes = (size_t)kMark;
    const int rc = psn::ctx_layout(cls.empty() ? nullptr : cls.data(), (int)cls.size(), scale, cap, cfg, fcls, slot_fcls, pyr_bytes);
    const bool touched = !fcls.empty() || !slot_fcls.empty() || pyr_bytes != (size_t)kMark || cfg.width != kMark ||
                         cfg.height != kMark || cfg.user_slots != kMark || cfg.nslots != kMark || cfg.nlevels != kMark ||
                         cfg.ncls != kMark;
    printf("{\"case\": \"%s\", \"rc\": %d, \"touched\": %s", text, rc, touched ? "true" : "false");
    if (rc) {
        printf("}\n");
        return;
    }
    printf(", \"pyr_bytes\": %zu, ", pyr_bytes);
    print_ints("slot_fcls", slot_fcls.data(), slot_fcls.size());
    printf(", \"cfg\": {\"width\": %d, \"height\": %d, \"user_slots\": %d, \"nslots\": %d, \"nlevels\": %d, \"ncls\": %d, \"cls\": [",
           cfg.width, cfg.height, cfg.user_slots, cfg.nslots, cfg.nlevels, cfg.ncls);
    for (int k = 0; k < cfg.ncls; k++)
        printf("%s[%d, %d, %d, %d]", k ? ", " : "", cfg.cls[k].width, cfg.cls[k].height, cfg.cls[k].first_slot, cfg.cls[k].nslots);
    printf("]}, \"classes\": [");
    const int nl = cfg.nlevels;
    for (size_t k = 0; k < fcls.size(); k++) {
        const psn::FrameClass &f = fcls[k];
        printf("%s{\"src_w\": %d, \"src_h\": %d, \"w\": %d, \"h\": %d, \"rz\": %s, \"first_slot\": %d, \"nslots\": %d, ", k ? ", " : "",
               f.src_w, f.src_h, f.w, f.h, f.rz ? "true" : "false", f.first_slot, f.nslots);
        print_ints("lw", f.ring.w, (size_t)nl);
        printf(", ");
        print_ints("lh", f.ring.h, (size_t)nl);
        printf(", ");
        print_ints("pitch", f.ring.pitch, (size_t)nl);
        printf(", \"off\": [");
        for (int l = 0; l < nl; l++) printf("%s%lld", l ? ", " : "", f.ring.off[l]);
        printf("], \"slot_bytes\": %lld, \"place\": %zu, \"gray_pitch\": %d, \"gray_bytes\": %zu, \"rz_n\": %zu, \"rz_sum\": \"%016" PRIx64
               "\", \"rz_first\": %d, \"rz_last\": %d}",
               f.ring.slot_bytes, f.place, f.gray_pitch, f.gray_bytes, f.rz_tab.size(), fnv1a(f.rz_tab),
               f.rz_tab.empty() ? 0 : f.rz_tab.front(), f.rz_tab.empty() ? 0 : f.rz_tab.back());
    }
    printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "--plan")) {
        const int src = atoi(argv[2]), dst = atoi(argv[3]);
        std::vector<int> ofs((size_t)(dst > 0 ? dst : 0));
        std::vector<int16_t> coef(2 * ofs.size());
        const int rc = psn_lk_resize_plan(src, dst, ofs.data(), coef.data(), atoi(argv[4]));
        if (rc) return 1;
        const std::vector<int> c32(coef.begin(), coef.end());
        printf("{");
        print_ints("ofs", ofs.data(), ofs.size());
        printf(", ");
        print_ints("coef", c32.data(), c32.size());
        printf("}\n");
        return 0;
    }
    for (int i = 1; i < argc; i++) run_case(argv[i]);
    return 0;
}
