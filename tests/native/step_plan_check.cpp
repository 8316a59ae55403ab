// plan_step (csrc/mev_plan.h) against the choices recorded from the policy functions and
// launch ladders it replaced: a grid of shapes that straddles every threshold, one digest per
// (step_kernel, step_pack, step_split) slice, and named shapes with their whole plan.
//
//   step_plan_check                 check everything, print STEP PLAN OK
//   step_plan_check dump K P S      the rows of slice (step_kernel K, step_pack P, step_split S)
//   step_plan_check dump named      the named shapes' rows
//   step_plan_check digest          the digest of the rows on stdin (a dump from elsewhere)
//   step_plan_check rows            the rows of the shapes on stdin: a line holds a row's first ten
//                                   numbers, then optionally `world` (StepShape::world) and `plain`
//                                   (the call's rows are plain, step_row in mev_plan.h; default 1);
//                                   each row is followed by " | wc step_row serve_row": the key's wc
//                                   as launched and the rows of kStepKeys / kServeKeys (-1: none)
//   step_plan_check keys            both key tables: "step|serve ROW TRAFFIC NM KM PK SPLIT ESPLIT P1 NC WC"
//
// A row: E N R K lidar_slots traffic dims step_kernel step_pack step_split | path pack split
// (as the getters report them) | the k_step key TRAFFIC NM KM PK SPLIT ESPLIT P1 NC, grid,
// block, dynamic LDS bytes (- unless path 2) | the same of the k_serve row that runs (- if
// k_serve does not apply).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "mev_plan.h"

using namespace mev;

static std::string launch_text(const StepKey& k, const StepLaunch& l) {
    char b[160];
    snprintf(b, sizeof b, " %d %d %d %d %d %d %d %d %u %u %u", (int)k.traffic, k.nm, k.km, k.pk, (int)k.split,
             (int)k.esplit, k.p1, k.nc, l.grid, l.block, l.lds);
    return b;
}

static int missing_rows = 0;  // plans whose key has no kernel

static std::string row_text(const StepShape& s) {
    const StepPlan pl = plan_step(s);
    char b[200];
    snprintf(b, sizeof b, "%d %d %d %d %d %d %d %d %d %d | %d %d %d |", s.E, s.N, s.R, s.K, s.lidar_slots, s.traffic,
             s.dims, s.step_kernel, s.step_pack, s.step_split, pl.path, pl.pack, pl.split);
    std::string r = b;
    if (pl.path == 2) {
        if (key_row(kStepKeys, pl.step.key) < 0) ++missing_rows;
        r += launch_text(pl.step.key, pl.step) + " |";
    } else {
        r += " - |";
    }
    if (pl.serve_fits) {
        const int row = serve_row(pl.serve.key);
        if (row < 0) ++missing_rows;
        r += launch_text(row < 0 ? pl.serve.key : kServeKeys[row], pl.serve);
    } else {
        r += " -";
    }
    return r + "\n";
}

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const char* s, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ (unsigned char)s[i]) * 1099511628211ull;
    }
};

// the grid: every threshold of the policy from both sides
static const int kE[] = {1, 16, 48, 63, 64, 65, 100, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192,
                         8193, 16384, 16385};
static const int kN[] = {1, 2, 3, 4, 5, 8, 9, 16, 64};
static const int kR[] = {16, 63, 64, 65, 96, 127, 128, 129, 256, 512, 2048, 4096};
static const int kTraffic[][2] = {{0, 0}, {0, 64}, {1, 16}, {1, 32}, {1, 33}, {1, 64}};  // traffic, max_npcs
static const int kKernel[] = {0, 1, 2}, kPack[] = {0, 1, 2, 4, 8}, kSplit[] = {0, 1, 2, 3};

template <class F>
static void walk_slice(int kernel, int pack, int split, F f) {
    for (const auto& t : kTraffic)
        for (int dims = 0; dims < 2; ++dims)
            for (int E : kE)
                for (int N : kN)
                    for (int R : kR)
                        for (int slots : {R, R - 1}) f(StepShape{E, N, R, t[1], slots, t[0], dims, kernel, pack, split});
}

// ---- recorded from the parent of the commit that introduced plan_step ----
struct Slice { int kernel, pack, split; uint64_t digest; };
static const Slice kSlices[] = {
    {0, 0, 0, 0xb1e15568b4083aa9ull},
    {0, 0, 1, 0x8f4e269c71e9ca0bull},
    {0, 0, 2, 0x08e6e37d8b6c5925ull},
    {0, 0, 3, 0x12459e6ebd289787ull},
    {0, 1, 0, 0xf7083a8b71e8d793ull},
    {0, 1, 1, 0x49650de39ab4dcb9ull},
    {0, 1, 2, 0x996aee86fc6f4921ull},
    {0, 1, 3, 0xf93a40ce4ae49f39ull},
    {0, 2, 0, 0xc32656c796f899fbull},
    {0, 2, 1, 0xa6f7e8a21b5b364full},
    {0, 2, 2, 0xf8f651d3c245b37full},
    {0, 2, 3, 0x9eecdff2f20c7489ull},
    {0, 4, 0, 0xf83d4f8fdb77642bull},
    {0, 4, 1, 0xf91d02492d0a6a63ull},
    {0, 4, 2, 0xaef918455a37fd8bull},
    {0, 4, 3, 0x342154f37c2e9139ull},
    {0, 8, 0, 0xfba808026205094full},
    {0, 8, 1, 0x4de5c607356905dbull},
    {0, 8, 2, 0xc25c0c32671c9c03ull},
    {0, 8, 3, 0x2fd099cfa99681a7ull},
    {1, 0, 0, 0xbddda26a7342cdd7ull},
    {1, 0, 1, 0x27fc23d1c91dd6dfull},
    {1, 0, 2, 0x36a0eee6da332d6full},
    {1, 0, 3, 0x20ebb59f8df1b527ull},
    {1, 1, 0, 0xad5ddcb735a3ed7full},
    {1, 1, 1, 0xf956e9e83a433277ull},
    {1, 1, 2, 0x0eee00d0fa9f0527ull},
    {1, 1, 3, 0x008a698032a52c4full},
    {1, 2, 0, 0x001c5181252a082full},
    {1, 2, 1, 0xe6350da1984d62a7ull},
    {1, 2, 2, 0x63452058046ad697ull},
    {1, 2, 3, 0xe0f2fd1da00fe65full},
    {1, 4, 0, 0x5393f9133c57d867ull},
    {1, 4, 1, 0x1062a23628a8d23full},
    {1, 4, 2, 0x1b172173bba2a58full},
    {1, 4, 3, 0xef9af95a39469647ull},
    {1, 8, 0, 0x2045ec9eb9196c27ull},
    {1, 8, 1, 0x32ca26013cfca63full},
    {1, 8, 2, 0x3d3355ca775e87ffull},
    {1, 8, 3, 0xf267a33343339757ull},
    {2, 0, 0, 0x49f36bb1613e20f3ull},
    {2, 0, 1, 0xbad4790a68ce8f0dull},
    {2, 0, 2, 0xdc3911ee5a9f7227ull},
    {2, 0, 3, 0xa42794d8158ef7cdull},
    {2, 1, 0, 0x960e3bebca999c59ull},
    {2, 1, 1, 0xf8352a194c7c035bull},
    {2, 1, 2, 0xe1aea7bec2d7c7ffull},
    {2, 1, 3, 0xccd617e51317f633ull},
    {2, 2, 0, 0xf610547da3b1a4ddull},
    {2, 2, 1, 0x4ba6aec6e655d56dull},
    {2, 2, 2, 0x7cc39643be4c95e9ull},
    {2, 2, 3, 0x1570fc40c6fff9e7ull},
    {2, 4, 0, 0x3f6d68ce7162c05dull},
    {2, 4, 1, 0x4f4829ae67f64dfdull},
    {2, 4, 2, 0x8d3d4b0a1e8c81b1ull},
    {2, 4, 3, 0xf274559cb28e3d1full},
    {2, 8, 0, 0xf16e45d755602c4dull},
    {2, 8, 1, 0x94090d50a31c7995ull},
    {2, 8, 2, 0x4b0edba40d298865ull},
    {2, 8, 3, 0xd6e70c002e717731ull},
};
static const char* const kNamed[][2] = {
    {"config 1: 1 env x 1 agent x 16 beams",
     "1 1 16 64 16 0 0 0 0 0 | 2 1 1 | 0 8 64 1 1 0 0 1 1 128 9728 | 0 8 64 1 1 0 0 1 1 128 9728"},
    {"config 2: 4096 envs x 1 agent x 64 beams",
     "4096 1 64 64 64 0 0 0 0 0 | 2 4 2 | 0 8 64 4 1 1 64 1 1024 128 9728 | -"},
    {"config 3: 4096 envs x 8 agents x 64 beams",
     "4096 8 64 64 64 0 0 0 0 0 | 2 1 0 | 0 8 64 1 0 0 64 8 4096 64 9728 | -"},
    {"config 4: 4096 envs x 1 ego x 64 beams, traffic, 32 NPC slots",
     "4096 1 64 32 64 1 0 0 0 0 | 2 1 2 | 1 1 32 2 1 1 64 0 2048 192 8704 | -"},
    {"config 5, one GPU's shard: 4096 envs x 8 agents x 128 beams",
     "4096 8 128 64 128 0 0 0 0 0 | 2 1 0 | 0 8 64 1 0 0 128 8 4096 64 9728 | -"},
    {"env.py's default: 1 env x 1 agent x 96 beams",
     "1 1 96 64 96 0 0 0 0 0 | 2 1 1 | 0 8 64 1 1 0 0 1 1 128 9728 | 0 8 64 1 1 0 0 1 1 128 9728"},
    {"env.py's default with traffic, max_npcs 32",
     "1 1 96 32 96 1 0 0 0 0 | 2 1 0 | 1 1 32 1 0 0 0 0 1 64 4480 | 1 1 32 1 0 0 0 0 1 64 4480"},
    {"env.py's default with traffic, max_npcs 64",
     "1 1 96 64 96 1 0 0 0 0 | 1 1 0 | - | 1 0 64 1 0 0 0 0 1 64 5536"},
    {"test_dims_gpu: 6 envs x 4 agents x 32 beams, max_npcs 8",
     "6 4 32 8 32 0 0 0 0 0 | 2 1 1 | 0 8 64 1 1 0 0 0 6 128 9728 | 0 8 64 1 1 0 0 0 6 128 9728"},
    {"test_dims_gpu: the same with per-car sizes",
     "6 4 32 8 32 0 1 0 0 0 | 2 1 0 | 0 0 64 1 0 0 0 0 6 64 3104 | -"},
    {"test_dims_gpu: 6 envs x 1 ego, traffic, max_npcs 8",
     "6 1 32 8 32 1 0 0 0 0 | 2 1 0 | 1 1 32 1 0 0 0 0 6 64 4480 | 1 1 32 1 0 0 0 0 6 64 4480"},
    {"test_properties_gpu: config 3, two kernels",
     "4096 8 64 64 64 0 0 1 1 0 | 1 1 0 | - | -"},
    {"test_properties_gpu: config 3, fused, one wave per env",
     "4096 8 64 64 64 0 0 2 1 1 | 2 1 0 | 0 8 64 1 0 0 64 8 4096 64 9728 | -"},
    {"test_properties_gpu: config 3, early split",
     "4096 8 64 64 64 0 0 2 1 3 | 2 1 2 | 0 8 64 1 1 1 0 0 4096 128 9728 | -"},
    {"test_properties_gpu: 4 agents x 128 beams, early split",
     "4096 4 128 64 128 0 0 2 1 3 | 2 1 2 | 0 8 64 1 1 1 0 0 4096 128 9728 | -"},
    {"test_properties_gpu: 2 agents x 64 beams, early split",
     "4096 2 64 64 64 0 0 2 1 3 | 2 1 2 | 0 8 64 1 1 1 0 0 4096 128 9728 | -"},
    {"test_properties_gpu: 1 agent, early split, 2 envs per workgroup",
     "4096 1 64 64 64 0 0 2 2 3 | 2 2 2 | 0 8 64 2 1 1 0 1 2048 128 9728 | -"},
    {"test_properties_gpu: 2 agents, early split, 4 envs per workgroup",
     "4096 2 64 64 64 0 0 2 4 3 | 2 4 2 | 0 8 64 4 1 1 0 0 1024 128 9728 | -"},
    {"test_properties_gpu: 1 agent, early split, 8 envs per workgroup",
     "4096 1 64 64 64 0 0 2 8 3 | 2 8 2 | 0 8 64 8 1 1 0 0 512 128 9728 | -"},
    {"test_properties_gpu: 1 agent, 2 envs per wave",
     "4096 1 64 64 64 0 0 2 2 1 | 2 2 0 | 0 8 64 2 0 0 0 0 2048 64 9728 | -"},
    {"test_properties_gpu: 1 agent, 4 envs per wave",
     "4096 1 64 64 64 0 0 2 4 1 | 2 4 0 | 0 8 64 4 0 0 0 0 1024 64 9728 | -"},
    {"test_properties_gpu: 1 agent, 8 envs per wave",
     "4096 1 64 64 64 0 0 2 8 1 | 2 8 0 | 0 8 64 8 0 0 0 0 512 64 9728 | -"},
    {"test_properties_gpu: 2 agents, 8 envs per wave asked (4 fit)",
     "4096 2 64 64 64 0 0 2 8 1 | 2 4 0 | 0 8 64 4 0 0 0 0 1024 64 9728 | -"},
    {"test_properties_gpu: 1 agent, 2 envs per workgroup, two waves",
     "4096 1 64 64 64 0 0 2 2 2 | 2 2 1 | 0 8 64 2 1 0 0 0 2048 128 9728 | -"},
    {"test_properties_gpu: 1 agent, 4 envs per workgroup, two waves",
     "4096 1 64 64 64 0 0 2 4 2 | 2 4 1 | 0 8 64 4 1 0 0 0 1024 128 9728 | -"},
    {"test_properties_gpu: 1 agent, 8 envs per workgroup, two waves",
     "4096 1 64 64 64 0 0 2 8 2 | 2 8 1 | 0 8 64 8 1 0 0 0 512 128 9728 | -"},
    {"test_properties_gpu: config 4, fused, one wave per env",
     "4096 1 64 32 64 1 0 2 0 1 | 2 1 0 | 1 1 32 1 0 0 0 0 4096 64 4480 | -"},
    {"test_properties_gpu: config 4, fused, automatic split",
     "4096 1 64 32 64 1 0 2 0 0 | 2 1 2 | 1 1 32 2 1 1 64 0 2048 192 8704 | -"},
    {"test_properties_gpu: 16384 envs, traffic, early split",
     "16384 1 64 32 64 1 0 0 0 3 | 2 1 2 | 1 1 32 2 1 1 64 0 8192 192 8704 | -"},
    {"test_properties_gpu: 16384 envs, traffic, one wave per env",
     "16384 1 64 32 64 1 0 0 0 1 | 2 1 0 | 1 1 32 1 0 0 0 0 16384 64 4480 | -"},
    {"test_properties_gpu: 8 egos + 64 NPC slots, fused asked",
     "4096 8 64 64 64 1 0 2 0 0 | 2 1 0 | 1 0 64 1 0 0 0 0 4096 64 21568 | -"},
    {"test_properties_gpu: 8 egos + 64 NPC slots, automatic",
     "4096 8 64 64 64 1 0 0 0 0 | 1 1 0 | - | -"},
    {"test_properties_gpu: 64 envs x 8 agents x 64 beams",
     "64 8 64 64 64 0 0 0 0 0 | 2 1 1 | 0 8 64 1 1 0 64 8 64 128 9728 | 0 8 64 1 1 0 64 8 64 128 9728"},
    {"test_properties_gpu: 64 envs x 12 agents x 64 beams",
     "64 12 64 64 64 0 0 0 0 0 | 1 1 0 | - | -"},
    {"test_properties_gpu: 4088 envs, traffic (no multiple of 16)",
     "4088 1 64 32 64 1 0 0 0 0 | 2 1 0 | 1 1 32 1 0 0 0 0 4088 64 4480 | -"},
    {"test_properties_gpu: 1000 envs, traffic (no multiple of 16)",
     "1000 1 64 32 64 1 0 0 0 0 | 2 1 0 | 1 1 32 1 0 0 0 0 1000 64 4480 | -"},
};

static bool parse_shape(const char* row, StepShape* s) {
    return sscanf(row, "%d %d %d %d %d %d %d %d %d %d", &s->E, &s->N, &s->R, &s->K, &s->lidar_slots, &s->traffic,
                  &s->dims, &s->step_kernel, &s->step_pack, &s->step_split) == 10;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "digest")) {
        Fnv h;
        char line[512];
        while (fgets(line, sizeof line, stdin)) h.add(line, strlen(line));
        printf("0x%016llxull\n", (unsigned long long)h.h);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "rows")) {
        char line[512];
        while (fgets(line, sizeof line, stdin)) {
            StepShape s;
            int world = 0, plain = 1;
            if (!parse_shape(line, &s)) return 2;
            sscanf(line, "%*d %*d %*d %*d %*d %*d %*d %*d %*d %*d %d %d", &world, &plain);
            s.world = world;
            std::string r = row_text(s);
            r.pop_back();
            const StepPlan pl = plan_step(s);
            const int row = step_row(pl, plain != 0);
            printf("%s | %d %d %d\n", r.c_str(), row >= 0 ? kStepKeys[row].wc : 0, row, serve_row(pl));
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "keys")) {
        auto put = [](const char* tab, int row, const StepKey& k) {
            printf("%s %d %d %d %d %d %d %d %d %d %d\n", tab, row, (int)k.traffic, k.nm, k.km, k.pk, (int)k.split,
                   (int)k.esplit, k.p1, k.nc, k.wc);
        };
        int i = 0;
        for (const StepKey& k : kStepKeys) put("step", i++, k);
        i = 0;
        for (const StepKey& k : kServeKeys) put("serve", i++, k);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "dump") && !strcmp(argv[2], "named")) {
        for (const auto& n : kNamed) {
            StepShape s;
            if (!parse_shape(n[1], &s)) return 2;
            fputs(row_text(s).c_str(), stdout);
        }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "dump")) {
        walk_slice(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), [](const StepShape& s) { fputs(row_text(s).c_str(), stdout); });
        return 0;
    }
    if (argc != 1) return 2;
    int bad = 0, slices = 0;
    for (int kernel : kKernel)
        for (int pack : kPack)
            for (int split : kSplit) {
                Fnv h;
                walk_slice(kernel, pack, split, [&](const StepShape& s) {
                    const std::string r = row_text(s);
                    h.add(r.data(), r.size());
                });
                const Slice* want = nullptr;
                for (const Slice& c : kSlices)
                    if (c.kernel == kernel && c.pack == pack && c.split == split) want = &c;
                ++slices;
                if (!want || want->digest != h.h) {
                    ++bad;
                    printf("slice step_kernel %d step_pack %d step_split %d: digest 0x%016llx, recorded 0x%016llx "
                           "(compare `dump %d %d %d`)\n", kernel, pack, split, (unsigned long long)h.h,
                           (unsigned long long)(want ? want->digest : 0), kernel, pack, split);
                }
            }
    if (slices != (int)(sizeof kSlices / sizeof kSlices[0])) { ++bad; printf("slices: %d walked\n", slices); }
    for (const auto& n : kNamed) {
        StepShape s;
        std::string r = parse_shape(n[1], &s) ? row_text(s) : "?\n";
        r.pop_back();
        if (r != n[1]) {
            ++bad;
            printf("%s:\n  plan     %s\n  recorded %s\n", n[0], r.c_str(), n[1]);
        }
    }
    if (missing_rows) { ++bad; printf("%d plans have no kernel row\n", missing_rows); }
    if (bad) return 1;
    printf("STEP PLAN OK\n");
    return 0;
}
