// cf_os_sides_main.cpp — the one-sided assembly's pair list as the layout plan counts it (csrc/esl_cf_plan.hpp: twins merged, the
// shorter side per block and segment), on the host, for tests/test_cf_os_sides.py and tests/test_gpu_cf_os_sides.py.  Reads the input
// file of tests/cf_plan_main.cpp (tests/cf_plan_ref.py writes it):
//   N nf EU chain_ok comm total_mem
//   sparse tperm_off no_nd nd_min stride os_kernel        (sparse: -1 unset, else the digit of ESL_CF_SPARSE)
//   ue_start[N + 1]   cu_start[nf + 1]   cu_obj[n_list]   cu_id[n_list]
// and a second argument, ESL_CF_OS_LIST (0 or 1, default 1); prints one "name value ..." line per number and array.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_cf_plan.hpp"

static long long next(FILE* f) {
  long long v;
  if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "cf_os_sides_main: the input ends early\n"); exit(2); }
  return v;
}
static std::vector<int> next_ints(FILE* f, size_t n) {
  std::vector<int> v(n);
  for (int& x : v) x = (int)next(f);
  return v;
}
template <class V>
static void print(const char* name, const V& v) {
  printf("%s", name);
  for (auto x : v) printf(" %lld", (long long)x);
  printf("\n");
}

int main(int argc, char** argv) {
  FILE* f = argc >= 2 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: cf_os_sides_main <graph file> [os_list]\n"); return 2; }
  const int N = (int)next(f), nf = (int)next(f);
  const size_t EU = (size_t)next(f);
  const bool chain_ok = next(f) != 0, comm = next(f) != 0;
  const size_t total_mem = (size_t)next(f);
  esl::CfSwitches sw;
  const int sparse = (int)next(f);
  sw.sparse = sparse < 0 ? -1 : '0' + sparse;
  sw.tperm_off = next(f) != 0; sw.no_nd = next(f) != 0; sw.nd_min = (int)next(f); sw.stride = (int)next(f); sw.os_kernel = (int)next(f);
  sw.os_list = argc >= 3 ? atoi(argv[2]) : 1;
  const std::vector<int> ue_start = next_ints(f, (size_t)N + 1), cu_start = next_ints(f, (size_t)nf + 1);
  const std::vector<int> cu_obj = next_ints(f, (size_t)ue_start[(size_t)N]), cu_id = next_ints(f, (size_t)ue_start[(size_t)N]);
  fclose(f);
  esl::CfPlan pl;
  if (!esl::cf_plan_build(N, nf, EU, ue_start, cu_start.data(), cu_obj.data(), cu_id.data(), chain_ok, comm, total_mem, sw, pl)) {
    printf("too_large 1\n");
    return 0;
  }
  const long long scalars[] = {pl.sparse, pl.form, pl.S, pl.nseg, pl.n_list, (long long)pl.os_npairs, pl.os_offsets, pl.os_list,
                               (long long)pl.osm_npairs, (long long)pl.osm_row_npairs, (long long)pl.os_list_npairs};
  const char* names[] = {"sparse", "form", "S", "nseg", "n_list", "os_npairs", "os_offsets", "os_list", "osm_npairs", "osm_row_npairs", "os_list_npairs"};
  for (size_t i = 0; i < sizeof(scalars) / sizeof(scalars[0]); ++i) printf("%s %lld\n", names[i], scalars[i]);
  printf("os_flops %.17g\nosm_flops %.17g\n", pl.os_flops, pl.osm_flops);
  print("seg_start", pl.seg_start); print("inc_p", pl.p); print("inc_o", pl.o);
  print("os", pl.os); print("rank", pl.rank);
  print("os_run", pl.os_run); print("os_heads", pl.os_heads);
  return 0;
}
