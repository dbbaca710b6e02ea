// plan_probe.cpp — prints make_plan's answer (csrc/lbsim_plan.h) for each row of stdin, one JSON
// object per line; tests/test_step_plan.py compiles it as plain C++ and compares the output with
// tests/golden/step_plan.jsonl.  A row is a line of 20 integers: the PlanInput fields in
// declaration order (B S Q policy trace fail leak split res_vpp dur_plane next_reset dyn_mapping
// step_kernel simds), then the Overrides (group_lanes_set group_lanes dyn_wave dyn_epw step_kernel
// step_wave_occ); a 21st, if there, is PlanInput::flow_stats (tests/test_flow_stats.py).
#include <cstdio>

#include "../marllb_amd/csrc/lbsim_plan.h"

namespace {

void print_dyn(const char* name, const lbk::DynPlan& d) {
  std::printf("\"%s\": {\"kernel\": %d, \"width\": %d, \"full\": %d, \"waves\": %d, \"epw\": %d, "
              "\"grid\": %u, \"block\": %u}, ",
              name, d.kernel, d.width, (int)d.full, d.waves, d.epw, d.grid, d.block);
}

void print_obs(const char* name, const lbk::ObsPlan& o, const char* end) {
  std::printf("\"%s\": {\"form\": %d, \"maxs\": %d, \"nchunks\": %d, \"chunk_grid\": %u, "
              "\"grid\": %u, \"block\": %u, \"lds\": %u}%s",
              name, o.form, o.maxs, o.nchunks, o.chunk_grid, o.grid, o.block, o.lds, end);
}

}  // namespace

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    int v[21] = {}, n = 0, used = 0;  // no 21st integer: flow_stats = 0
    for (const char* p = line; n < 21 && std::sscanf(p, "%d%n", &v[n], &used) == 1; p += used) ++n;
    if (n < 20) return 1;  // a short row is an error
    lbk::PlanInput in{};
    in.B = v[0], in.S = v[1], in.Q = v[2], in.policy = v[3];
    in.trace = v[4], in.fail = v[5], in.leak = v[6], in.split = v[7], in.res_vpp = v[8];
    in.dur_plane = v[9], in.next_reset = v[10];
    in.dyn_mapping = v[11], in.step_kernel = v[12], in.simds = v[13];
    in.flow_stats = v[20] != 0;
    lbk::Overrides ov;
    ov.group_lanes_set = v[14], ov.group_lanes = v[15], ov.dyn_wave = v[16], ov.dyn_epw = v[17];
    ov.step_kernel = v[18], ov.step_wave_occ = v[19];
    const lbk::StepPlan p = lbk::make_plan(in, ov);
    std::printf("{\"form\": %d, \"width\": %d, \"occ\": %d, \"obs_maxs\": %d, \"grid\": %u, "
                "\"nr\": %d, \"dynamics_kernel\": %d, ",
                p.form, p.width, p.occ, p.obs_maxs, p.grid, (int)p.nr, p.dyn.kernel);
    print_dyn("dyn", p.dyn);
    print_dyn("reset_dyn", p.reset_dyn);
    print_obs("obs", p.obs, ", ");
    print_obs("reset_obs", p.reset_obs, "}\n");
  }
}
