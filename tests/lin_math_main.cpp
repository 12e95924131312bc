// Host build of esl_math.hpp's per-edge residuals and analytic Jacobians, for tests/test_lin_ref.py: reads edge cases on stdin, one per
// line, and prints the residual and the Jacobians with %.17g.  Test infrastructure; no device code runs.
//   bbox MODE cam[7] obj[10] K[4] meas[4]     MODE 0 reprojection, 1 tangency        -> r 4, Jo 4 x 9, Jc 4 x 6
//   e3d cam[7] obj[10] meas[10]               e3d_half_turn = 1 (the minimum as written) -> r 9, Jo 9 x 9, Jc 9 x 6
//   grav obj[10] normal[3]                                                           -> r 1, Jo 1 x 9
//   odom cam_i[7] cam_j[7] Z[7]                                                      -> r 6, Ji 6 x 6, Jj 6 x 6
// Output per case: three lines "r ...", "Ja ..." (camera / first camera; empty for grav), "Jb ..." (ellipsoid / second camera).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "esl_math.hpp"

using namespace esl;

static bool read_n(double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (std::scanf("%lf", v + i) != 1) return false;
  return true;
}
static void put(const char* tag, const double* v, int n) {
  std::printf("%s", tag);
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

int main() {
  YawTable yt;
  {  // as esl_graph_upload fills it: yaw = k pi / 2, k = -1, 0, 1, 2
    const double ang[4] = {-1, 0, 1, 2};
    double hs[4], hc[4];
    for (int k = 0; k < 4; ++k) { const double yaw = ang[k] * M_PI / 2.0; hs[k] = std::sin(yaw * 0.5); hc[k] = std::cos(yaw * 0.5); }
    yaw_table_fill(yt, hs, hc);
    yt.as_written = 1;
  }
  char cls[16];
  while (std::scanf("%15s", cls) == 1) {
    if (!std::strcmp(cls, "bbox")) {
      int mode;
      double cam[7], obj[10], K[4], meas[4], r[4], Jo[36], Jc[24];
      if (std::scanf("%d", &mode) != 1 || !read_n(cam, 7) || !read_n(obj, 10) || !read_n(K, 4) || !read_n(meas, 4)) return 2;
      jac_box_edge_both(mode, se3_load(cam), ell_load(obj), K, meas, r, Jo, Jc);
      put("r", r, 4); put("Ja", Jc, 24); put("Jb", Jo, 36);
    } else if (!std::strcmp(cls, "e3d")) {
      double cam[7], obj[10], meas[10], r[9], Jo[81], Jc[54];
      if (!read_n(cam, 7) || !read_n(obj, 10) || !read_n(meas, 10)) return 2;
      jac_e3d(se3_load(cam), ell_load(obj), ell_load(meas), yt, r, Jo, Jc);
      put("r", r, 9); put("Ja", Jc, 54); put("Jb", Jo, 81);
    } else if (!std::strcmp(cls, "grav")) {
      double obj[10], n[3], r[1], Jo[9];
      if (!read_n(obj, 10) || !read_n(n, 3)) return 2;
      r[0] = jac_grav(ell_load(obj), n, Jo);
      put("r", r, 1); put("Ja", nullptr, 0); put("Jb", Jo, 9);
    } else if (!std::strcmp(cls, "odom")) {
      double ci[7], cj[7], Z[7], r[6], Ji[36], Jj[36];
      if (!read_n(ci, 7) || !read_n(cj, 7) || !read_n(Z, 7)) return 2;
      jac_odom(se3_load(ci), se3_load(cj), se3_load(Z), r, Ji, Jj);
      put("r", r, 6); put("Ja", Ji, 36); put("Jb", Jj, 36);
    } else {
      std::fprintf(stderr, "unknown edge class %s\n", cls);
      return 2;
    }
  }
  return 0;
}
