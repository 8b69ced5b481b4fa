// Correctly rounded fp32 transcendentals (fp64 evaluation, one rounding).
// The oracle does the same (oracle/helper.py: cr): feasible candidates'
// res_norm is rounding noise, so reproducible transcendentals are what makes
// the projection-elite order reproducible (DESIGN.md Numerics).  The host
// restatements (carla_host.cpp: crf) round the host libm's fp64 values the
// same way.
#pragma once
#include "common.hpp"

namespace mpcmmd {

DEVI float cr_atan2(float y, float x) { return float(atan2(double(y), double(x))); }
DEVI float cr_sin(float a) { return float(sin(double(a))); }
DEVI float cr_tan(float a) { return float(tan(double(a))); }
// cos and sin from one fp64 sincos (OCML: one argument reduction, the values
// of cos and sin), each rounded once
DEVI void cr_sincos(float a, float& s, float& c) {
  double sd, cd;
  sincos(double(a), &sd, &cd);
  s = float(sd);
  c = float(cd);
}

}  // namespace mpcmmd
