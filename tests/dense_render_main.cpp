// dense_render_main.cpp — csrc/esl_dense_proj.hpp on the host, without HIP: tests/test_dense_render_ref.py compiles it with the host
// compiler (plain and with -fsanitize=address,undefined) and holds it to the numpy statement tests/dense_render_ref.py voxel by voxel.
//   dense_render_main            self-checks of the packing, the depth gate and the comparison classes; prints "dense_proj ok"
//   dense_render_main project    stdin: "e max_radius rows cols depth_min depth_max fx fy cx cy n", a pose line "tx ty tz qx qy qz qw",
//                                then n lines "x y z".  stdout per voxel: "class zbits zq c0 c1 r0 r1" (zbits = the double's 64 bits;
//                                zq and the bounds 0 unless the class is 0 = drawn)
//   dense_render_main check      csrc/esl_dense_check.hpp.  stdin per line: "depth_scale depth_min depth_max depth_tol footprint max_radius
//                                min_count zbuf_bytes npix"; stdout per line drn_params_check's refusal text, or "ok"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_dense_check.hpp"
#include "../object-oriented-slam_amd/csrc/esl_dense_proj.hpp"

using namespace esl;

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED line %d: %s\n", __LINE__, #x);               \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int self_check() {
  CHECK(drn_word(1.0, 7) == ((1ull << 20) << 32 | 7ull));
  CHECK(drn_word_index(drn_word(4095.0, 0xFFFFFFFEu)) == 0xFFFFFFFEu);
  CHECK(drn_word(4095.0, 0xFFFFFFFFu) < kDrnEmpty);
  CHECK(drn_zq(1.0 + 1.0 / 33554432.0) == drn_zq(1.0));                       // 2^-25 m apart: a tie
  CHECK(drn_zq(1.5 / 1048576.0) == 2 && drn_zq(2.5 / 1048576.0) == 2);        // ties to even, as np.rint
  CHECK(drn_depth_in(1.0, 1.0, 6.0) && drn_depth_in(6.0, 1.0, 6.0) && !drn_depth_in(std::nan(""), 0.0, 6.0) && !drn_depth_in(-1.0, 0.0, 6.0));
  CHECK(drn_coord_ok(1073741824.0) && !drn_coord_ok(1073741825.0) && !drn_coord_ok(std::nan("")) && !drn_coord_ok(HUGE_VAL));
  // |z_meas - z| == depth_tol agrees; one raw unit beyond does not
  CHECK(drn_compare(1088, 1.0, 1024.0, 0.1, 6.0, 0.0625) == 0 && drn_compare(1089, 1.0, 1024.0, 0.1, 6.0, 0.0625) == 2);
  CHECK(drn_compare(960, 1.0, 1024.0, 0.1, 6.0, 0.0625) == 0 && drn_compare(959, 1.0, 1024.0, 0.1, 6.0, 0.0625) == 1);
  CHECK(drn_compare(0, 1.0, 1024.0, 0.1, 6.0, 0.0625) == 3 && drn_compare(60000, 1.0, 1024.0, 0.1, 6.0, 0.0625) == 3);
  int lo = 0, hi = 0;
  CHECK(drn_axis(256.0, 32.0, 0.0, 1.0, 1.0 / 128, 8, 64, &lo, &hi) && lo == 30 && hi == 34);
  CHECK(drn_axis(256.0, 31.5, 0.0, 1.0, 0.0, 8, 64, &lo, &hi) && lo == 32 && hi == 32);          // u + 0.5 an integer: the upper pixel
  CHECK(drn_axis(256.0, 32.0, 0.125, 1.0, 1.0 / 128, 8, 64, &lo, &hi) && lo == 62 && hi == 63);  // clipped
  CHECK(!drn_axis(256.0, 32.0, -9.0 / 64, 1.0, 1.0 / 128, 8, 64, &lo, &hi));                     // no pixel
  CHECK(!drn_axis(256.0, 32.0, 0.0, 0.0, 1.0 / 128, 8, 64, &lo, &hi));                           // 0 / 0
  std::printf("dense_proj ok\n");
  return 0;
}

static int project() {
  double e, dmin, dmax, K[4], cam[7], P[kDensePose];
  int max_radius, rows, cols;
  long n;
  if (std::scanf("%lf %d %d %d %lf %lf %lf %lf %lf %lf %ld", &e, &max_radius, &rows, &cols, &dmin, &dmax, &K[0], &K[1], &K[2], &K[3], &n) != 11) return 2;
  for (double& v : cam)
    if (std::scanf("%lf", &v) != 1) return 2;
  if (n < 0 || !dense_pose(cam, P)) return 2;
  std::vector<double> xyz((size_t)n * 3);
  for (double& v : xyz)
    if (std::scanf("%lf", &v) != 1) return 2;
  for (long i = 0; i < n; ++i) {
    double z = 0;
    int box[4] = {0, 0, 0, 0};
    const int cat = drn_project(P, K, xyz.data() + (size_t)i * 3, e, max_radius, rows, cols, dmin, dmax, &z, box);
    uint64_t bits;
    std::memcpy(&bits, &z, 8);
    if (cat != DRN_DRAWN) { std::printf("%d %" PRIu64 " 0 0 0 0 0\n", cat, bits); continue; }
    if (drn_cam_z(P, xyz.data() + (size_t)i * 3) != z) return 3;          // the resolve pass's z is the splat's
    std::printf("%d %" PRIu64 " %llu %d %d %d %d\n", cat, bits, drn_zq(z), box[0], box[1], box[2], box[3]);
  }
  return 0;
}

static int check() {
  esl_dense_render_params p;
  long long zbuf, npix;
  while (std::scanf("%lf %lf %lf %lf %lf %d %d %lld %lld", &p.depth_scale, &p.depth_min, &p.depth_max, &p.depth_tol, &p.footprint, &p.max_radius,
                    &p.min_count, &zbuf, &npix) == 9) {
    p.zbuf_bytes = zbuf;
    const char* m = drn_params_check(p, (size_t)npix);
    std::printf("%s\n", m ? m : "ok");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "check") == 0) return check();
  if (argc > 1 && std::strcmp(argv[1], "project") == 0) return project();
  return self_check();
}
