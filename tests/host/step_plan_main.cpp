// Host sanitizer driver of the denoise loop's step plan (candle-video_amd/host/step_plan.h, header only, built with ASan + UBSan).
// argv: plan B guidance_batch const N g s r LIST                      the unscheduled call
//       plan B guidance_batch sched cfg_star rescale_form N (g s r LIST) x N      a schedule resolved to one guide per step
//       rows L rows row0 B LIST                                       step_skip_rows
// LIST: "-" no list (null), "e" an empty list, else block indices joined by commas.
// stdout: one JSON line - per step [cfg, stg, nbr, batched, slot0, rows, [blocks of the perturbed branch]], the per-call flags, the mix
// (0 classic, 1 _ex) with its cfg_star and rescale_form, and what becomes of the handle's permanent list: "handle" null = left alone,
// else the list set, "handle_null" = it is set through a null pointer.  rows: the mask [L][rows] as integers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../candle-video_amd/host/step_plan.h"

struct List { bool null = true; std::vector<int> v; const int* p() const { return null ? nullptr : v.data(); } };
static List parse_list(const char* a) {
    List l;
    if (!strcmp(a, "-")) return l;
    l.null = false;
    l.v.reserve(8);         // (data() of a reserved empty vector is non-null: the empty list that is not "no list")
    if (!strcmp(a, "e")) return l;
    for (const char* c = a; *c;) { l.v.push_back((int)strtol(c, const_cast<char**>(&c), 10)); if (*c == ',') ++c; }
    return l;
}
static void print_list(const int* p, int n) {
    printf("[");
    for (int k = 0; k < n; ++k) printf("%s%d", k ? ", " : "", p[k]);
    printf("]");
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "rows")) {
        const int L = atoi(argv[2]), rows = atoi(argv[3]), row0 = atoi(argv[4]), B = atoi(argv[5]);
        const List l = parse_list(argv[6]);
        std::vector<float> m(3, 7.0f);      // (whatever it held is overwritten)
        step_skip_rows(L, rows, row0, B, l.p(), (int)l.v.size(), &m);
        if (m.size() != (size_t)L * rows) return 3;
        printf("[");
        for (int i = 0; i < L; ++i) {
            printf("%s[", i ? ", " : "");
            for (int r = 0; r < rows; ++r) printf("%s%d", r ? ", " : "", (int)m[(size_t)i * rows + r]);
            printf("]");
        }
        printf("]\n");
        return 0;
    }
    if (argc < 5 || strcmp(argv[1], "plan")) { fprintf(stderr, "usage: plan B guidance_batch const|sched ... | rows L rows row0 B LIST\n"); return 2; }
    const int B = atoi(argv[2]); const bool gb = atoi(argv[3]) != 0;
    StepPlan plan;
    std::vector<List> lists;
    std::vector<StepGuide> guides;
    auto guide = [&](char** a) { StepGuide g; g.g = strtof(a[0], nullptr); g.s = strtof(a[1], nullptr); g.r = strtof(a[2], nullptr); lists.push_back(parse_list(a[3])); return g; };
    if (!strcmp(argv[4], "const") && argc == 10) {
        StepGuide g = guide(argv + 6);
        g.skip = lists[0].p(); g.n_skip = (int)lists[0].v.size();
        step_plan_constant(atoi(argv[5]), B, g, gb, &plan);
    } else if (!strcmp(argv[4], "sched") && argc >= 8 && argc == 8 + 4 * atoi(argv[7])) {
        const int N = atoi(argv[7]);
        lists.reserve((size_t)N);
        for (int i = 0; i < N; ++i) guides.push_back(guide(argv + 8 + 4 * i));
        for (int i = 0; i < N; ++i) { guides[(size_t)i].n_skip = (int)lists[(size_t)i].v.size(); guides[(size_t)i].skip = guides[(size_t)i].n_skip ? lists[(size_t)i].p() : nullptr; }
        step_plan_scheduled(guides.data(), N, B, atoi(argv[5]), atoi(argv[6]), gb, &plan);
    } else { fprintf(stderr, "bad arguments\n"); return 2; }
    printf("{\"steps\": [");
    for (size_t i = 0; i < plan.steps.size(); ++i) {
        const StepEntry& e = plan.steps[i];
        printf("%s[%d, %d, %d, %d, %d, %d, ", i ? ", " : "", e.cfg ? 1 : 0, e.stg ? 1 : 0, e.nbr, e.batched ? 1 : 0, e.slot0, e.rows);
        print_list(e.guide.skip, e.guide.n_skip);
        printf("]");
    }
    printf("], \"any_cfg\": %d, \"any_stg\": %d, \"any_batched\": %d, \"mix\": %d, \"cfg_star\": %d, \"rescale_form\": %d, \"handle\": ",
           plan.any_cfg ? 1 : 0, plan.any_stg ? 1 : 0, plan.any_batched ? 1 : 0, (int)plan.mix, plan.cfg_star, plan.rescale_form);
    if (plan.set_skip) print_list(plan.perm_skip, plan.n_perm_skip); else printf("null");
    printf(", \"handle_null\": %d}\n", plan.set_skip && !plan.perm_skip ? 1 : 0);
    return 0;
}
