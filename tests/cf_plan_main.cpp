// cf_plan_main.cpp — the layout plan of the camera-first elimination (csrc/esl_cf_plan.hpp) on the host, for tests/test_cf_plan.py
// and tests/test_gpu_cf_stride.py.  Reads a graph's lists and the switches from a text file of integers:
//   N nf EU chain_ok comm total_mem
//   sparse tperm_off no_nd nd_min stride os_kernel        (sparse: -1 unset, else the digit of ESL_CF_SPARSE)
//   ue_start[N + 1]   cu_start[nf + 1]   cu_obj[n_list]   cu_id[n_list]
// and prints one "name value ..." line per scalar and array of the plan; flops as %.17g, so that they read back as the same doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_cf_plan.hpp"

static long long next(FILE* f) {
  long long v;
  if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "cf_plan_main: the input ends early\n"); exit(2); }
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
  FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: cf_plan_main <graph file>\n"); return 2; }
  const int N = (int)next(f), nf = (int)next(f);
  const size_t EU = (size_t)next(f);
  const bool chain_ok = next(f) != 0, comm = next(f) != 0;
  const size_t total_mem = (size_t)next(f);
  esl::CfSwitches sw;
  const int sparse = (int)next(f);
  sw.sparse = sparse < 0 ? -1 : '0' + sparse;
  sw.tperm_off = next(f) != 0; sw.no_nd = next(f) != 0; sw.nd_min = (int)next(f); sw.stride = (int)next(f); sw.os_kernel = (int)next(f);
  const std::vector<int> ue_start = next_ints(f, (size_t)N + 1), cu_start = next_ints(f, (size_t)nf + 1);
  const std::vector<int> cu_obj = next_ints(f, (size_t)ue_start[(size_t)N]), cu_id = next_ints(f, (size_t)ue_start[(size_t)N]);
  fclose(f);
  esl::CfPlan pl;
  if (!esl::cf_plan_build(N, nf, EU, ue_start, cu_start.data(), cu_obj.data(), cu_id.data(), chain_ok, comm, total_mem, sw, pl)) {
    printf("too_large 1\n");
    return 0;
  }
  const long long scalars[] = {pl.sparse, pl.form, pl.tperm, pl.nd, pl.stride, pl.n_sep, pl.n_seg, pl.S, pl.nseg, pl.nw, pl.n_chunks, pl.n_list,
                               pl.ldx, pl.ldt, pl.kpad, pl.kpad_s, pl.n_fwork, pl.n_twork, (long long)pl.xc_len, (long long)pl.p_blocks,
                               (long long)pl.prhs_len, (long long)pl.y_len, (long long)pl.os_npairs, pl.os_offsets};
  const char* names[] = {"sparse", "form", "tperm", "nd", "stride", "n_sep", "n_seg", "S", "nseg", "nw", "n_chunks", "n_list", "ldx", "ldt", "kpad", "kpad_s",
                         "n_fwork", "n_twork", "xc_len", "p_blocks", "prhs_len", "y_len", "os_npairs", "os_offsets"};
  for (size_t i = 0; i < sizeof(scalars) / sizeof(scalars[0]); ++i) printf("%s %lld\n", names[i], scalars[i]);
  printf("sp_flops %.17g\nupd_flops %.17g\nos_flops %.17g\n", pl.sp_flops, pl.upd_flops, pl.os_flops);
  print("seg_start", pl.seg_start); print("xld", pl.xld); print("xoff", pl.xoff); print("boff", pl.boff); print("roff", pl.roff);
  print("fw_off", pl.fw_off); print("tw_off", pl.tw_off);
  print("inc_p", pl.p); print("inc_o", pl.o); print("inc_first", pl.first);
  print("os", pl.os); print("ou", pl.ou);
  print("rank", pl.rank); print("unrank", pl.unrank); print("kfirst", pl.kfirst);
  return 0;
}
