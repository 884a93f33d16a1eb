// Host-only harness of csrc/residency_rule.hpp (tests/test_residency_rule.py builds it with -fsanitize=address,undefined and runs
// it): the candidate rule of the persistent form's capacity query against STAGED self-test outcomes -- the fallback path no GPU
// test can reach without making a self-test fail on purpose.  One line per case: name, capacity, self-test grids, blocks, validated.
#include <cstdio>
#include <initializer_list>
#include <set>
#include <vector>

#include "../../mbrl-lib_amd/csrc/residency_rule.hpp"

using hipets::Occ;

static void run(const char* name, Occ& oc, int want, int wg_cap, std::initializer_list<int> passing) {
    const std::set<int> pass(passing);
    std::vector<int> calls;
    const int cap = hipets::resident_capacity_rule(oc, want, wg_cap, [&](int g) {
        calls.push_back(g);
        return pass.count(g) != 0;
    });
    std::printf("%s capacity=%d calls=", name, cap);
    for (size_t i = 0; i < calls.size(); ++i) std::printf("%s%d", i ? "," : "", calls[i]);
    std::printf(" blocks=%d validated=%d\n", oc.blocks, oc.validated);
}

static Occ fresh() {
    Occ oc;
    oc.blocks = 2, oc.api = 1, oc.n_cu = 256;
    return oc;
}

int main() {
    Occ a = fresh(), b = fresh(), c = fresh(), d = fresh(), e = fresh(), f = fresh();
    run("pass_450", a, 450, 0, {450});
    run("want_300_after_450", a, 300, 0, {});
    run("fail_450_pass_256", b, 450, 0, {256});
    run("fail_always_450", c, 450, 0, {});
    run("fail_200", d, 200, 0, {});
    run("cap100_pass", e, 450, 100, {100});
    run("cap100_fail", f, 450, 100, {});
    std::printf("pays one_per_cu_fits=%d turns=%d two_per_cu=%d beyond_two_per_cu=%d\n", hipets::persistent_pays(200, 512, 256),
                hipets::persistent_pays(450, 256, 256), hipets::persistent_pays(450, 512, 256), hipets::persistent_pays(750, 512, 256));
    return 0;
}
