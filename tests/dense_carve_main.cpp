// dense_carve_main.cpp — csrc/esl_dense_carve.hpp on the host, without HIP: tests/test_dense_carve_ref.py compiles it with the host
// compiler (plain and with -fsanitize=address,undefined) and holds it to the numpy statement tests/dense_carve_ref.py value by value.
//   dense_carve_main             self-checks of the verdict, the packed counts and a one-pixel observation; prints "dense_carve ok"
//   dense_carve_main FILE        FILE: "rows cols window depth_scale depth_min depth_max depth_tol min_through through_per_agree fx fy cx
//                                cy n F", then n lines "x y z", then per frame a pose line "tx ty tz qx qy qz qw" and rows cols raw
//                                values.  stdout: per frame one line of n classes (0 agree, 1 nearer, 2 through, 3 no data, 4 depth
//                                out, 5 outside), then per voxel "agree nearer through nodata carved" from the packed accumulator
//   dense_carve_main check       csrc/esl_dense_check.hpp.  stdin per line: "depth_scale depth_min depth_max depth_tol window min_through
//                                through_per_agree apply"; stdout per line dcv_params_check's refusal text, or "ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_dense_carve.hpp"
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
  CHECK(dcv_verdict(0, 2, 2, 1) && !dcv_verdict(0, 1, 2, 1) && dcv_verdict(2, 2, 2, 1) && !dcv_verdict(3, 2, 2, 1));
  CHECK(dcv_verdict(1000, 2, 2, 0) && !dcv_verdict(0, 0, 1, 0));
  CHECK(!dcv_verdict(65535, 65535, 1, 2147483647));          // the product does not wrap
  unsigned long long w = 0;
  for (int k = 0; k < 4; ++k)
    for (int r = 0; r < 16383 + k; ++r) w += dcv_pack_one(k);          // the fields sum to 65535 - 3 + 6: below 2^16 each, no carry
  for (int k = 0; k < 4; ++k) CHECK(dcv_unpack(w, k) == 16383 + k);
  const double P[kDensePose] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, K[4] = {1, 1, 0, 0}, p[3] = {0, 0, 1};
  const unsigned short agree = 1088, through = 1089, nearer = 959, none = 0;
  CHECK(dcv_observe(P, K, p, &agree, 1, 1, 4, 1024.0, 0.1, 6.0, 0.0625) == DCV_AGREE);
  CHECK(dcv_observe(P, K, p, &through, 1, 1, 4, 1024.0, 0.1, 6.0, 0.0625) == DCV_THROUGH);
  CHECK(dcv_observe(P, K, p, &nearer, 1, 1, 0, 1024.0, 0.1, 6.0, 0.0625) == DCV_NEARER);
  CHECK(dcv_observe(P, K, p, &none, 1, 1, 1, 1024.0, 0.1, 6.0, 0.0625) == DCV_NODATA);
  CHECK(dcv_observe(P, K, p, &agree, 1, 1, 1, 1024.0, 1.5, 6.0, 0.0625) == DCV_DEPTH_OUT);
  const double q[3] = {1, 0, 1}, o[3] = {0, 0, 0};
  CHECK(dcv_observe(P, K, q, &agree, 1, 1, 1, 1024.0, 0.1, 6.0, 0.0625) == DCV_OUTSIDE);
  CHECK(dcv_observe(P, K, o, &agree, 1, 1, 1, 1024.0, 0.0, 6.0, 0.0625) == DCV_OUTSIDE);          // 0 / 0 is no coordinate
  std::printf("dense_carve ok\n");
  return 0;
}

static int run(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return 2;
  int rows, cols, window, min_through, tpa;
  long n, F;
  double scale, dmin, dmax, tol, K[4];
  if (std::fscanf(f, "%d %d %d %lf %lf %lf %lf %d %d %lf %lf %lf %lf %ld %ld", &rows, &cols, &window, &scale, &dmin, &dmax, &tol, &min_through,
                  &tpa, &K[0], &K[1], &K[2], &K[3], &n, &F) != 15) return 2;
  if (rows < 1 || cols < 1 || n < 0 || F < 0 || F > kDcvMaxObs || window < 0 || window > kDcvMaxWindow) return 2;
  std::vector<double> xyz((size_t)n * 3);
  for (double& v : xyz)
    if (std::fscanf(f, "%lf", &v) != 1) return 2;
  std::vector<unsigned long long> acc((size_t)n, 0ull);
  std::vector<unsigned short> img((size_t)rows * cols);
  for (long fr = 0; fr < F; ++fr) {
    double cam[7], P[kDensePose];
    for (double& v : cam)
      if (std::fscanf(f, "%lf", &v) != 1) return 2;
    if (!dense_pose(cam, P)) return 2;
    for (unsigned short& v : img) {
      unsigned raw;
      if (std::fscanf(f, "%u", &raw) != 1 || raw > 65535u) return 2;
      v = (unsigned short)raw;
    }
    for (long i = 0; i < n; ++i) {
      const int cls = dcv_observe(P, K, xyz.data() + (size_t)i * 3, img.data(), rows, cols, window, scale, dmin, dmax, tol);
      if (cls <= DCV_NODATA) acc[(size_t)i] += dcv_pack_one(cls);
      std::printf(i + 1 < n ? "%d " : "%d", cls);
    }
    std::printf("\n");
  }
  for (long i = 0; i < n; ++i) {
    const unsigned long long w = acc[(size_t)i];
    std::printf("%d %d %d %d %d\n", dcv_unpack(w, DCV_AGREE), dcv_unpack(w, DCV_NEARER), dcv_unpack(w, DCV_THROUGH), dcv_unpack(w, DCV_NODATA),
                dcv_verdict(dcv_unpack(w, DCV_AGREE), dcv_unpack(w, DCV_THROUGH), min_through, tpa) ? 1 : 0);
  }
  std::fclose(f);
  return 0;
}

static int check() {
  esl_dense_carve_params p;
  while (std::scanf("%lf %lf %lf %lf %d %d %d %d", &p.depth_scale, &p.depth_min, &p.depth_max, &p.depth_tol, &p.window, &p.min_through,
                    &p.through_per_agree, &p.apply) == 8) {
    const char* m = dcv_params_check(p);
    std::printf("%s\n", m ? m : "ok");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "check") == 0) return check();
  if (argc > 1) return run(argv[1]);
  return self_check();
}
