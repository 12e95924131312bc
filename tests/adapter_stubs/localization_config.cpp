// localization_config.cpp — linked beside tracking_calls.cpp by tests/test_adapter_localization.py: sets the config key
// Optimizer.Localization = 1 (every ellipsoid fixed) before main() runs, as a yaml carrying it would.
#include "esl_ref_surface.hpp"

namespace {
struct LocalizationKey {
  LocalizationKey() { EllipsoidSLAM::Config::values()["Optimizer.Localization"] = 1; }
} localization_key;
}  // namespace
