// Host-only harness of the resident-heads selection rule (csrc/residency_rule.hpp resident_heads_wanted / resident_heads_kept;
// tests/test_resident_heads_rule.py builds it with -fsanitize=address,undefined and runs it): one line per case,
//   <case> wanted=<0|1> kept=<0|1>
// for a DEVICE rollout of `logical` workgroups of R row tiles on 256 CUs whose capacity query answered (persistent, capacity).
#include <cstdio>

#include "../../mbrl-lib_amd/csrc/residency_rule.hpp"

using namespace hipets;

static void run(const char* name, int R, int n_layers, int logical, int horizon, bool persistent, int capacity) {
    const bool wanted = resident_heads_wanted(R, n_layers, logical, 256, horizon);
    const bool kept = wanted && resident_heads_kept(persistent, capacity, logical);
    std::printf("%s wanted=%d kept=%d\n", name, wanted ? 1 : 0, kept ? 1 : 0);
}

int main() {
    run("smallest_R3_pop12", 3, 5, 5, 4, true, 256);            // 5 workgroups, one per member
    run("one_per_cu_R3_pop480", 3, 5, 200, 4, true, 256);
    run("headline_R3_pop500", 3, 5, 210, 30, true, 256);
    run("R4_one_per_cu", 4, 5, 160, 4, true, 256);
    run("turns_R3_pop1080", 3, 5, 450, 4, true, 256);           // more logical workgroups than CUs: the turn-based form
    run("R1_pop360", 1, 5, 450, 4, true, 512);
    run("R1_small", 1, 5, 5, 4, true, 512);
    run("R2_small", 2, 5, 10, 4, true, 512);
    run("three_layer_model", 3, 3, 5, 4, true, 256);
    run("six_layer_model", 3, 6, 5, 4, true, 256);
    run("horizon_1", 3, 5, 5, 1, true, 256);                    // H = 1 never runs the persistent form
    run("exactly_256", 3, 5, 256, 4, true, 256);
    run("257", 3, 5, 257, 4, true, 256);
    run("capped_below_logical", 3, 5, 200, 4, true, 100);       // HIPETS_MAX_WORKGROUPS = 100: turns, so the plain instance
    run("self_test_failed", 3, 5, 200, 4, false, 0);            // capacity 0: per-step launches
    return 0;
}
