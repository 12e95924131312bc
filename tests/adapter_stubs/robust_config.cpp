// robust_config.cpp — linked beside tracking_calls.cpp by tests/test_adapter_robust.py: sets the robust-kernel config keys
// (Optimizer.Edges.2D.RobustKernel = 1 = Huber, RobustDelta = 1) before main() runs, as a yaml carrying them would.
#include "esl_ref_surface.hpp"

namespace {
struct RobustKeys {
  RobustKeys() {
    EllipsoidSLAM::Config::values()["Optimizer.Edges.2D.RobustKernel"] = 1;
    EllipsoidSLAM::Config::values()["Optimizer.Edges.2D.RobustDelta"] = 1.0;
  }
} robust_keys;
}  // namespace
