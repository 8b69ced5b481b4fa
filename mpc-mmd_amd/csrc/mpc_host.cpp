#include "mpc_host.hpp"

#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

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

MpcVehConsts MpcVehTables::view() const {
  return MpcVehConsts{qp->kinv_x.data(), qp->kinv_y.data(), qp->colsum_x.data(), qp->colsum_y.data(),
                      qp->P.data(),      adv.data()};
}

MpcVehTables mpc_vehicle_tables(float dt) {
  std::vector<double> adv = build_vehicle_advance(dt);  // throws before the QP is built
  static const DynObsConsts qp = build_dyn_obs_consts();
  return MpcVehTables{&qp, std::move(adv)};
}

int check_mpc_planned(const mpcmmd_mpc_model* m, const mpcmmd_mpc_planned* pl) {
  if (!m || !pl) return fail(MPCMMD_E_INVALID, "null argument");
  if (!(m->dt > 0.0f && m->dt < 15.0f)) return fail(MPCMMD_E_INVALID, "mpc vehicles: 0 < dt < 15");
  if (m->num_obs > 0 && (!pl->veh_acc || !pl->veh_target)) return fail(MPCMMD_E_INVALID, "mpc vehicles: null array");
  return MPCMMD_OK;
}

void mpc_step_host(const mpcmmd_mpc_model& m, int tick, const mpcmmd_mpc_step_io& io, MpcDraw draw,
                   const mpcmmd_mpc_planned* pl, const MpcVehConsts* vc) {
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
      if (pl) {  // S <- advance(plan(S, target))
        float* a = pl->veh_acc + size_t(o) * 2;
        const float S[6] = {v[0], v[1], v[2], v[3], a[0], a[1]};
        float coef[kVehCoef];
        for (int j = 0; j < kVehCoef; ++j) coef[j] = mpc_veh_coef(*vc, S, pl->veh_target + size_t(o) * 2, j);
        for (int k = 0; k < 4; ++k) v[k] = mpc_veh_advance(vc->adv, coef, k);
        for (int k = 0; k < 2; ++k) a[k] = mpc_veh_advance(vc->adv, coef, 4 + k);
        continue;
      }
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
    if (pl) {  // the tracks of the plan of the state the step leaves
      const float* a = pl->veh_acc + size_t(o) * 2;
      const float S[6] = {v[0], v[1], v[2], v[3], a[0], a[1]};
      if (pl->veh_log) std::memcpy(pl->veh_log + size_t(o) * 6, S, sizeof S);
      float coef[kVehCoef];
      for (int j = 0; j < kVehCoef; ++j) coef[j] = mpc_veh_coef(*vc, S, pl->veh_target + size_t(o) * 2, j);
      for (int k = 0; k < kMpcTrack; ++k) {
        io.x_obs[size_t(o) * kMpcTrack + k] = mpc_veh_track(vc->P, coef, k);
        io.y_obs[size_t(o) * kMpcTrack + k] = mpc_veh_track(vc->P, coef + 11, k);
      }
      continue;
    }
    for (int k = 0; k < kMpcTrack; ++k) {
      io.x_obs[size_t(o) * kMpcTrack + k] = mpc_track(v[0], v[2], k);
      io.y_obs[size_t(o) * kMpcTrack + k] = mpc_track(v[1], v[3], k);
    }
  }
  for (int b = 0; b < w.B; ++b)
    for (int a = 0; a < 8; ++a) io.pop[size_t(b) * 8 + a] = world_pop(io.mean, m.chol, m.pop0 + size_t(b) * 8, a);
}

}  // namespace mpcmmd

extern "C" int mpcmmd_mpc_vehicle_constant(float dt, const char* name, double* dst, size_t count) {
  using namespace mpcmmd;
  if (!name) return fail(MPCMMD_E_INVALID, "null argument");
  if (!(dt > 0.0f && dt < 15.0f)) return fail(MPCMMD_E_INVALID, "mpc vehicles: 0 < dt < 15");
  try {
    const MpcVehTables t = mpc_vehicle_tables(dt);
    const std::string n(name);
    const std::vector<double>* v = n == "kinv_x"     ? &t.qp->kinv_x
                                   : n == "kinv_y"   ? &t.qp->kinv_y
                                   : n == "colsum_x" ? &t.qp->colsum_x
                                   : n == "colsum_y" ? &t.qp->colsum_y
                                   : n == "P"        ? &t.qp->P
                                   : n == "adv"      ? &t.adv
                                                     : nullptr;
    if (!v) return fail(MPCMMD_E_INVALID, "unknown constant " + n);
    if (dst) {
      if (count < v->size()) return fail(MPCMMD_E_INVALID, "dst too small");
      std::memcpy(dst, v->data(), v->size() * 8);
    }
    return int(v->size());
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}
