// Stand-alone driver of csrc/esl_render_ray.hpp (the per-ray arithmetic of esl_render_map) for tests/test_render_ref.py, which compiles
// it with and without -fsanitize=address,undefined and compares its output with the numpy statement.
//   stdin:  count, then per record 33 numbers: the map row v (10), the columns of [Rco | tco] (4 x 3), the outline's box (4, "nan" when
//           there is none), C22, K (4), rows, cols; then pairs and `pairs` lines "raw z scale min max tol"
//   stdout: per record "valid 0|1 q(4) s(3)"; for a valid one "body b(10)", "bounds flags x0 x1 y0 y1" and one line "hit col row z" per
//           hit pixel, rows outermost; after the records "behind n"; then per pair "cmp category".  Numbers as %.17g.
// The bounds are walked through an image of exactly rows x cols bytes, so bounds that leave the image are an out-of-bounds write; a hit
// pixel outside its body's bounds ends the program with status 5.  Every hit is also put to render_behind with running minima from
// 0.05 to 2 times its depth: a "cannot win" for a hit that would win or tie ends the program with status 7; n counts the times it said
// so rightly.
#include <cstdio>
#include <vector>

#include "../object-oriented-slam_amd/csrc/esl_render_ray.hpp"

int main() {
  int count;
  if (std::scanf("%d", &count) != 1 || count < 0) return 2;
  long long behind = 0;
  for (int c = 0; c < count; ++c) {
    double v[10], n[4][3], bb[4], C22, K[4];
    int rows, cols;
    for (double& x : v) if (std::scanf("%lf", &x) != 1) return 2;
    for (auto& col : n) for (double& x : col) if (std::scanf("%lf", &x) != 1) return 2;
    for (double& x : bb) if (std::scanf("%lf", &x) != 1) return 2;
    if (std::scanf("%lf", &C22) != 1) return 2;
    for (double& x : K) if (std::scanf("%lf", &x) != 1) return 2;
    if (std::scanf("%d %d", &rows, &cols) != 2 || rows < 1 || cols < 1 || rows > esl::kRenderMaxDim || cols > esl::kRenderMaxDim) return 2;
    double q[4] = {0, 0, 0, 0}, s[3];
    const bool ok = esl::render_valid(v, q, s);
    std::printf("valid %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", ok ? 1 : 0, q[0], q[1], q[2], q[3], s[0], s[1], s[2]);
    if (!ok) continue;
    esl::RenderRec r;
    esl::render_body(n, s, r.b);
    std::printf("body");
    for (double x : r.b) std::printf(" %.17g", x);
    std::printf("\n");
    const int flags = esl::render_bounds(bb, C22, n[3][2], r.b[9], rows, cols, r.x0, r.x1, r.y0, r.y1);
    std::printf("bounds %d %d %d %d %d\n", flags, r.x0, r.x1, r.y0, r.y1);
    std::vector<unsigned char> inside((size_t)rows * cols, 0);   // exactly the image
    for (int y = r.y0; y <= r.y1; ++y)
      for (int x = r.x0; x <= r.x1; ++x) inside[(size_t)y * cols + x] = 1;
    if (!(flags & esl::RENDER_DRAWN)) continue;
    for (int row = 0; row < rows; ++row)
      for (int col = 0; col < cols; ++col) {
        double z;
        const esl::RenderRay d = esl::render_ray(K, col, row);
        if (!esl::render_hit(r.b, d, z)) continue;
        if (!inside[(size_t)row * cols + col]) return 5;
        std::printf("hit %d %d %.17g\n", col, row, z);
        double beta, delta;
        if (!esl::render_hit_terms(r.b, d, beta, delta) || esl::render_depth(r.b[9], beta, delta) != z) return 6;
        for (double k : {0.05, 0.3, 0.45, 0.49, 0.4999999, 0.5, 0.5000001, 0.51, 0.75, 0.9999999, 1.0, 1.0000001, 2.0}) {
          const double best = z * k;   // a running minimum at every distance around and in front of this hit
          if (esl::render_behind(r.b[9], beta, delta, best)) {
            if (!(z > best)) return 7;   // it claimed that a hit which would win or tie cannot win
            ++behind;
          }
        }
        if (esl::render_behind(r.b[9], beta, delta, HUGE_VAL)) return 7;
      }
  }
  std::printf("behind %lld\n", behind);
  int pairs;
  if (std::scanf("%d", &pairs) != 1 || pairs < 0) return 2;
  for (int k = 0; k < pairs; ++k) {
    unsigned raw;
    double z, scale, lo, hi, tol;
    if (std::scanf("%u %lf %lf %lf %lf %lf", &raw, &z, &scale, &lo, &hi, &tol) != 6 || raw > 65535u) return 2;
    std::printf("cmp %d\n", esl::render_compare(raw, z, scale, lo, hi, tol));
  }
  return 0;
}
