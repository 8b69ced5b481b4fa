// What the fp64 Monte-Carlo validators (k_validate.hip, k_validate_risk.hip)
// share per plan and per rollout step: the controls of a saved trajectory,
// the noise draw, the Beta sampler and the bicycle step (S/validation.py
// compute_controls :122-132, compute_rollout_complete :42-101,
// compute_rollout_one_step :21-40).  One definition each, so both kernels
// roll the same (keys, seed) to the same points.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "rng.hpp"

namespace mpcmmd {

constexpr int kValThreads = 1024;
constexpr int kValMaxObs = 32;
constexpr int kValMaxH = 100;

// uniform-free Beta(a, b) straight from the Philox attempt streams
// (rng.hpp: gamma_attempt), log-space ratio as beta_draw_tab.  The values
// are log of gamma_direct's g (rng.hpp); the loop stays here with a log at
// each exit, the form k_validate's instruction stream was measured in.
// Host-callable too: the surrogate world's host twin draws with it (world_draw.hpp).
HDI void log_gamma_direct(double alpha, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t elem, double& lg,
                           double& lub) {
  const MtConst mc = mt_const(alpha);
  lg = log(mc.d);
  lub = 0.0;
  for (int k = 0; k < kGammaMaxAttempts; ++k) {
    const GammaAttempt g = gamma_attempt(k0, k1, stream, elem, k);
    const double v = 1.0 + mc.c * g.x;
    if (v > 0.0) {
      const double v3 = v * v * v;
      if (mt_accept(g.x, g.u, g.lu, mc.d, v3)) {
        lg = log(mc.d * v3);
        lub = g.lw;
        return;
      }
    }
  }
}

HDI double beta_direct(double a, double b, uint32_t k0, uint32_t k1, uint32_t sa, uint32_t sb, uint32_t elem) {
  double ga, ua, gb, ub;
  log_gamma_direct(a, k0, k1, sa, elem, ga, ua);
  log_gamma_direct(b, k0, k1, sb, elem, gb, ub);
  if (a == 0.0 && b == 0.0) return (ua * 5.0 > ub * 2.0) ? 1.0 : 0.0;
  const double la = a < 1.0 ? ga + ua / a : ga;
  const double lb = b < 1.0 ? gb + ub / b : gb;
  if (la > lb) return 1.0 / (1.0 + exp(lb - la));
  const double ea = exp(la - lb);
  return ea / (ea + 1.0);
}

// The plan's controls into LDS (sv [100], sacc / ssteer [H]); every thread of
// the workgroup calls it (two barriers); the caller's own LDS writes before
// the call are visible after it.
DEVI void val_controls(const float* Pdot, const float* Pddot, const double* cx, const double* cy, int H, int tid,
                       double* sv, double* sacc, double* ssteer) {
  const double dt = 0.15, wb = 2.5;  // prob.t, prob.wheel_base (cem.py:26,40)
  double xd = 0.0, yd = 0.0, xdd = 0.0, ydd = 0.0;
  if (tid < 100) {  // np.dot(prob.Pdot_jax, cx) etc. (validation.py:140-141)
    for (int j = 0; j < 11; ++j) {
      xd += double(Pdot[tid * 11 + j]) * cx[j];
      yd += double(Pdot[tid * 11 + j]) * cy[j];
      xdd += double(Pddot[tid * 11 + j]) * cx[j];
      ydd += double(Pddot[tid * 11 + j]) * cy[j];
    }
    sv[tid] = sqrt(xd * xd + yd * yd);
  }
  __syncthreads();
  if (tid < H) {  // compute_controls (:122-132): acc = diff([v, v_end]) / t, steer = atan(2.5 kappa)
    const double vn = tid < 99 ? sv[tid + 1] : sv[99];
    sacc[tid] = (vn - sv[tid]) / dt;
    const double curv = (ydd * xd - yd * xdd) / pow(xd * xd + yd * yd, 1.5);
    ssteer[tid] = atan(curv * wb);
  }
  __syncthreads();
}

// the noise scalars of a validation call
struct ValNoise {
  int32_t noise;
  double noise_level, acc_const, steer_const, K_steer;
};

// Noisy controls (an, sn) of rollout r at step h (:73-92): draws dr
// [3][R][H] of the configuration, or null for the Philox streams keyed
// (k0, k1), element r H + h.
DEVI void val_noisy_controls(const ValNoise& v, const double* dr, int R, int H, int r, int h, uint32_t k0,
                             uint32_t k1, double acc_h, double steer_h, double& an, double& sn) {
  const uint32_t e = uint32_t(r) * uint32_t(H) + uint32_t(h);
  double na, ns, nc;
  if (dr) {
    na = dr[(0 * size_t(R) + r) * H + h];
    ns = dr[(1 * size_t(R) + r) * H + h];
    nc = dr[(2 * size_t(R) + r) * H + h];
  } else if (v.noise == 0) {
    na = philox_normal(k0, k1, kStreamValAcc, e);
    ns = philox_normal(k0, k1, kStreamValSteer, e);
    nc = philox_normal(k0, k1, kStreamValConst, e);
  } else {
    const double fa = fabs(acc_h), fs = fabs(steer_h);
    na = beta_direct(2.0 * fa, 5.0 * fa, k0, k1, kStreamValGammaAccA, kStreamValGammaAccB, e);
    ns = beta_direct(2.0 * fs + 1e-5, 5.0 * fs + 1e-5, k0, k1, kStreamValGammaSteerA, kStreamValGammaSteerB, e);
    nc = philox_normal(k0, k1, kStreamValConst, e);
  }
  double ap, sp;
  if (v.noise == 0) {
    ap = v.noise_level * fabs(acc_h) * na;
    sp = v.noise_level * fabs(steer_h) * ns;
  } else {  // na, ns are the Beta draws
    ap = v.noise_level * (2.0 * na - 1.0);
    sp = v.K_steer * v.noise_level * (2.0 * ns - 1.0);
  }
  an = acc_h + ap + v.acc_const * nc;
  sn = steer_h + sp + v.steer_const * nc;
}

// compute_rollout_one_step (:21-40)
DEVI void val_bicycle_step(double an, double sn, double& x, double& y, double& vx, double& vy, double& psi) {
  const double dt = 0.15, wb = 2.5;
  double sp_ = sqrt(vx * vx + vy * vy);
  sp_ = sp_ + an * dt;
  const double psidot = sp_ * tan(sn) / wb;
  psi = psi + psidot * dt;
  vx = sp_ * cos(psi);
  vy = sp_ * sin(psi);
  x = x + vx * dt;
  y = y + vy * dt;
}

}  // namespace mpcmmd
