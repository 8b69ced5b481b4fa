#include "mpc_host.hpp"

#include <cmath>
#include <cstring>
#include <limits>

#include "host_api.hpp"

namespace mpcmmd {

namespace {

// the host libm's fp64 values (OCML's on the device)
struct HostMath {
  static double atan64(double a) { return std::atan(a); }
  static double tan64(double a) { return std::tan(a); }
  static void sincos64(double a, double& s, double& c) {
    s = std::sin(a);
    c = std::cos(a);
  }
};

}  // namespace

MpcScalars mpc_scalars(const mpcmmd_mpc_model& m) {
  MpcScalars w;
  w.O = m.num_obs, w.B = m.num_batch, w.noise = m.noise;
  w.dt = m.dt, w.sigma_acc = m.sigma_acc, w.sigma_steer = m.sigma_steer;
  w.acc_const = m.acc_const, w.steer_const = m.steer_const, w.K_steer = m.K_steer;
  w.a_obs = m.a_obs, w.b_obs = m.b_obs, w.y_lb = m.y_lb, w.y_ub = m.y_ub, w.goal_x = m.goal_x;
  return w;
}

int check_mpc_model(const mpcmmd_mpc_model* m) {
  if (!m) return fail(MPCMMD_E_INVALID, "null argument");
  if (m->num_obs < 0 || m->num_obs > kMpcMaxObs) return fail(MPCMMD_E_INVALID, "mpc: 0 <= num_obs <= 64");
  if (m->num_batch < 1) return fail(MPCMMD_E_INVALID, "mpc: num_batch >= 1");
  if (m->noise != 0 && m->noise != 1) return fail(MPCMMD_E_INVALID, "mpc: noise must be 0 (gaussian) or 1 (beta)");
  if (!(m->dt > 0.0f) || !std::isfinite(m->dt)) return fail(MPCMMD_E_INVALID, "mpc: dt must be finite and > 0");
  if (!(m->a_obs > 0.0f) || !(m->b_obs > 0.0f)) return fail(MPCMMD_E_INVALID, "mpc: a_obs, b_obs > 0");
  if (!m->pdot2 || !m->pddot1 || !m->chol || !m->pop0) return fail(MPCMMD_E_INVALID, "mpc model: null array");
  return MPCMMD_OK;
}

int check_mpc(const mpcmmd_mpc_model* m, const mpcmmd_mpc_step_io* io) {
  if (!m || !io) return fail(MPCMMD_E_INVALID, "null argument");
  if (int rc = check_mpc_model(m)) return rc;
  if (!io->cx || !io->cy || (!io->u && !io->key) || !io->mean || !io->pos || !io->vel || !io->done_tick ||
      !io->init_state || !io->st0 || !io->pop || !io->log_d || !io->log_f || !io->log_i ||
      (m->num_obs > 0 && (!io->vehicles || !io->x_obs || !io->y_obs)))
    return fail(MPCMMD_E_INVALID, "mpc step: null array");
  return MPCMMD_OK;
}

void mpc_step_host(const mpcmmd_mpc_model& m, int tick, const mpcmmd_mpc_step_io& io, MpcDraw draw) {
  const MpcScalars w = mpc_scalars(m);
  MpcEgo e{io.pos[0], io.pos[1], io.vel[0], io.vel[1], io.vel[2]};
  MpcControl c = mpc_controller<HostMath>(m.pdot2, m.pddot1, io.cx, io.cy);
  float u[3];
  if (io.u) std::memcpy(u, io.u, sizeof u);
  else draw(w.noise, io.key[0], m.seed, tick, c.a_c, c.s_c, u);
  mpc_perturb(w, u, c);
  const bool frozen = io.done_tick[0] >= 0;
  float ax = 0.0f, ay = 0.0f;  // a frozen state has no acceleration
  if (!frozen) {
    e = mpc_ego_step<HostMath>(e, c.a, c.s, w.dt, &ax, &ay);
    for (int o = 0; o < w.O; ++o) {
      float* v = io.vehicles + size_t(o) * 4;
      v[0] = v[0] + v[2] * w.dt;
      v[1] = v[1] + v[3] * w.dt;
    }
    io.pos[0] = e.x, io.pos[1] = e.y;
    io.vel[0] = e.vx, io.vel[1] = e.vy, io.vel[2] = e.psi;
  }
  // flags
  float clear = -std::numeric_limits<float>::infinity();
  bool clear_nan = false;
  for (int o = 0; o < w.O; ++o) {
    const float t = mpc_clear_term(w, e, io.vehicles + size_t(o) * 4);
    if (t != t) clear_nan = true;
    clear = fmaxf(clear, t);  // a NaN term is ignored here and reported below
  }
  if (clear_nan) clear = canon_nan(NAN);
  const bool lane_out = mpc_lane_out(w, e), collided = !(clear <= 0.0f), goal = mpc_goal(w, e);
  if (!frozen && (collided || goal)) io.done_tick[0] = tick;
  io.log_d[0] = e.x, io.log_d[1] = e.y;
  const float lf[MPCMMD_MPC_LOG_F] = {e.vx, e.vy, e.psi, c.a_c, c.s_c, c.a, c.s, u[0], u[1], u[2], clear, c.curv};
  std::memcpy(io.log_f, lf, sizeof lf);
  io.log_i[0] = lane_out, io.log_i[1] = collided, io.log_i[2] = goal, io.log_i[3] = frozen;
  // the next solve's inputs
  mpc_init_state(e, ax, ay, io.init_state);
  mpc_st0(io.init_state, io.st0);
  for (int o = 0; o < w.O; ++o) {
    const float* v = io.vehicles + size_t(o) * 4;
    for (int k = 0; k < kMpcTrack; ++k) {
      io.x_obs[size_t(o) * kMpcTrack + k] = mpc_track(v[0], v[2], k);
      io.y_obs[size_t(o) * kMpcTrack + k] = mpc_track(v[1], v[3], k);
    }
  }
  for (int b = 0; b < w.B; ++b)
    for (int a = 0; a < 8; ++a) io.pop[size_t(b) * 8 + a] = world_pop(io.mean, m.chol, m.pop0 + size_t(b) * 8, a);
}

}  // namespace mpcmmd
