// Prints the weight-gradient plans of spp-rl_amd/csrc/dw_plan.h (plan_dw: what finalize_dw uploads) for
// tests/test_cpu_dw_plan.py (plain g++, no HIP).
//   dw_plan_dump FILE        FILE holds whitespace-separated commands:
//     set NAME                                    a new job set (phase 0 begins)
//     phase                                       the set's second phase begins
//     job N K0 K1 BF16 A_BF X_BF FUSED            appends a job to the current phase
//     run BP NUM_CU FUSED_NSPLIT                  plans the set (its fused jobs with FUSED_NSPLIT slabs) and prints:
// plan NAME BP NUM_CU need NEED nph NPH
// job INDEX PHASE N K0 K1 BF16 A_BF X_BF FUSED wsplit W split_len L nsplit S slab_off OFF slab_stride STRIDE   (per job)
// phase PH nitems N nlds N max_elems M
// items PH J S0 COUNT ...     runs of the item table: COUNT consecutive items (J, S0), (J, S0 + 1), ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../spp-rl_amd/csrc/dw_plan.h"

using spp::DwJob;

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: dw_plan_dump FILE\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "dw_plan_dump: cannot read %s\n", argv[1]);
    return 2;
  }
  std::string cmd, name;
  std::vector<DwJob> proto;
  std::vector<int> phase_of;
  int ph = 0;
  while (in >> cmd) {
    if (cmd == "set") {
      in >> name;
      proto.clear();
      phase_of.clear();
      ph = 0;
    } else if (cmd == "phase") {
      ph = 1;
    } else if (cmd == "job") {
      DwJob j{};
      in >> j.N >> j.K0 >> j.K1 >> j.bf16 >> j.a_bf >> j.x_bf >> j.fused;
      j.nrow2 = j.N;
      j.slab_stride = spp::round_up((int64_t)j.N * (j.K0 + j.K1) + j.N, 4);  // as dw_job sets it
      proto.push_back(j);
      phase_of.push_back(ph);
    } else if (cmd == "run") {
      int Bp = 0, num_cu = 0, fns = 0;
      in >> Bp >> num_cu >> fns;
      if (!in || proto.empty() || Bp <= 0 || Bp % 32 || num_cu <= 0) {
        std::fprintf(stderr, "dw_plan_dump: bad run\n");
        return 2;
      }
      std::vector<DwJob> jobs = proto;
      for (DwJob& j : jobs) {
        j.Bp = Bp;
        if (j.fused) {
          j.nsplit = fns;
          j.wsplit = 1;
        }
      }
      const int nph = phase_of.back() + 1;
      int j0[2] = {0, 0}, nj[2] = {0, 0};
      for (size_t i = 0; i < jobs.size(); ++i) ++nj[phase_of[i]];
      j0[1] = nj[0];
      const spp::DwPlan P = spp::plan_dw(jobs, j0, nj, nph, Bp, num_cu);
      std::printf("plan %s %d %d need %zu nph %d\n", name.c_str(), Bp, num_cu, P.need, nph);
      for (size_t i = 0; i < jobs.size(); ++i) {
        const DwJob& j = jobs[i];
        std::printf("job %zu %d %d %d %d %d %d %d %d wsplit %d split_len %d nsplit %d slab_off %lld slab_stride %lld\n", i,
                    phase_of[i], j.N, j.K0, j.K1, j.bf16, j.a_bf, j.x_bf, j.fused, j.wsplit, j.split_len, j.nsplit,
                    (long long)P.slab_off[i], (long long)j.slab_stride);
      }
      for (int p = 0; p < nph; ++p) {
        std::printf("phase %d nitems %d nlds %d max_elems %lld\n", p, P.nitems[p], P.nlds[p], (long long)P.max_elems[p]);
        std::printf("items %d", p);
        const int* ij = P.items.data() + P.ioff[p];
        const int* is = ij + P.nitems[p];
        for (int i = 0; i < P.nitems[p];) {
          int n = 1;
          while (i + n < P.nitems[p] && ij[i + n] == ij[i] && is[i + n] == is[i] + n) ++n;
          std::printf(" %d %d %d", ij[i], is[i], n);
          i += n;
        }
        std::printf("\n");
      }
    } else {
      std::fprintf(stderr, "dw_plan_dump: no command '%s'\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
