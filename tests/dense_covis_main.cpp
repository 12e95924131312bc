// dense_covis_main.cpp — csrc/esl_dense_covis.hpp on the host, without HIP: tests/test_dense_covis_ref.py compiles it with the host
// compiler (plain and with -fsanitize=address,undefined) and holds it to the numpy statement tests/dense_covis_ref.py value by value.
//   dense_covis_main             self-checks of the predicate, the order and the pair count; prints "dense_covis ok"
//   dense_covis_main pred        stdin per line "seen covered cover_num cover_den"; stdout per line dco_redundant as 0 / 1
//   dense_covis_main order       stdin per line "unc_a f_a unc_b f_b"; stdout per line dco_before as 0 / 1
//   dense_covis_main pairs FILE  FILE: "F W", then F rows of W hexadecimal 64-bit words; stdout F lines of F pair counts
//   dense_covis_main check       csrc/esl_dense_check.hpp.  stdin per line: "depth_scale depth_min depth_max depth_tol window min_others
//                                cover_num cover_den max_cull reserved"; stdout per line dco_params_check's refusal text, or "ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_dense_covis.hpp"
#include "../object-oriented-slam_amd/csrc/esl_dense_check.hpp"

using namespace esl;

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED line %d: %s\n", __LINE__, #x);               \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int self_check() {
  CHECK(!dco_redundant(0, 0, 0, 1) && dco_redundant(1, 0, 0, 1) && dco_redundant(10, 9, 9, 10) && !dco_redundant(10, 8, 9, 10));
  CHECK(dco_redundant(2147483647, 2147483647, 1 << 20, 1 << 20) && !dco_redundant(2147483647, 2147483646, 1 << 20, 1 << 20));   // no wrap
  CHECK(dco_before(0, 5, 1, 0) && dco_before(3, 1, 3, 2) && !dco_before(3, 2, 3, 1) && !dco_before(4, 0, 3, 9));
  const unsigned long long a[3] = {~0ull, 0x8000000000000001ull, 0ull}, b[3] = {0xF0ull, 0x8000000000000000ull, ~0ull};
  CHECK(dco_pair_count(a, b, 3) == 5 && dco_pair_count(a, a, 3) == 66 && dco_pair_count(a, b, 0) == 0 && dco_popc(~0ull) == 64);
  CHECK(kDcoMaxFrames == 4096 && kDcoTile >= 2 && kDcoSlab >= 1 && kDcoChunk >= 1);
  std::printf("dense_covis ok\n");
  return 0;
}

static int pred() {
  int s, c, n, d;
  while (std::scanf("%d %d %d %d", &s, &c, &n, &d) == 4) std::printf("%d\n", dco_redundant(s, c, n, d) ? 1 : 0);
  return 0;
}

static int order() {
  int ua, fa, ub, fb;
  while (std::scanf("%d %d %d %d", &ua, &fa, &ub, &fb) == 4) std::printf("%d\n", dco_before(ua, fa, ub, fb) ? 1 : 0);
  return 0;
}

static int pairs(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return 2;
  long F, W;
  if (std::fscanf(f, "%ld %ld", &F, &W) != 2 || F < 0 || F > kDcoMaxFrames || W < 0 || W > (1l << 24)) return 2;
  std::vector<unsigned long long> bits((size_t)F * (size_t)W);
  for (unsigned long long& v : bits)
    if (std::fscanf(f, "%llx", &v) != 1) return 2;
  std::fclose(f);
  for (long a = 0; a < F; ++a) {
    for (long b = 0; b < F; ++b)
      std::printf(b + 1 < F ? "%lld " : "%lld", dco_pair_count(bits.data() + (size_t)a * W, bits.data() + (size_t)b * W, W));
    std::printf("\n");
  }
  return 0;
}

static int check() {
  esl_dense_covis_params p;
  while (std::scanf("%lf %lf %lf %lf %d %d %d %d %d %d", &p.depth_scale, &p.depth_min, &p.depth_max, &p.depth_tol, &p.window, &p.min_others,
                    &p.cover_num, &p.cover_den, &p.max_cull, &p.reserved) == 10) {
    const char* m = dco_params_check(p);
    std::printf("%s\n", m ? m : "ok");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "check") == 0) return check();
  if (argc > 1 && std::strcmp(argv[1], "pred") == 0) return pred();
  if (argc > 1 && std::strcmp(argv[1], "order") == 0) return order();
  if (argc > 2 && std::strcmp(argv[1], "pairs") == 0) return pairs(argv[2]);
  return self_check();
}
