#include "world_host.hpp"

#include <cmath>
#include <cstring>
#include <limits>

#include "host_api.hpp"

namespace mpcmmd {

namespace {

// the host libm's fp64 values, rounded once (cr_math.hpp on the device)
struct HostMath {
  static float tan(float a) { return float(std::tan(double(a))); }
  static float atan2(float y, float x) { return float(std::atan2(double(y), double(x))); }
  static void sincos(float a, float& s, float& c) {
    s = float(std::sin(double(a)));
    c = float(std::cos(double(a)));
  }
  static void sincos64(double a, double& s, double& c) {
    s = std::sin(a);
    c = std::cos(a);
  }
  static double acos64(double a) { return std::acos(a); }
};

}  // namespace

WorldScalars world_scalars(const mpcmmd_world_model& m) {
  WorldScalars w;
  w.P = m.num_path, w.O = m.num_obs, w.total = m.total_obs, w.n_route = m.num_route;
  w.goal_index = m.goal_index, w.B = m.num_batch, w.noise = m.noise;
  w.dt = m.dt, w.sigma_acc = m.sigma_acc, w.sigma_steer = m.sigma_steer;
  w.acc_const = m.acc_const, w.steer_const = m.steer_const, w.steer_max = m.steer_max;
  w.a_obs = m.a_obs, w.b_obs = m.b_obs, w.y_lb = m.y_lb, w.y_ub = m.y_ub;
  return w;
}

int check_world(const mpcmmd_world_model* m, const mpcmmd_world_step_io* io) {
  if (!m || !io) return fail(MPCMMD_E_INVALID, "null argument");
  if (m->num_path < 2 || m->num_path > 2048) return fail(MPCMMD_E_INVALID, "world: 2 <= num_path <= 2048");
  if (m->num_obs < 1 || m->num_obs > kWorldMaxObs) return fail(MPCMMD_E_INVALID, "world: 1 <= num_obs <= 64");
  if (m->total_obs < 0 || m->total_obs > kWorldMaxObs) return fail(MPCMMD_E_INVALID, "world: 0 <= total_obs <= 64");
  if (m->num_route < 2) return fail(MPCMMD_E_INVALID, "world: num_route >= 2");
  if (m->goal_index < 0 || m->goal_index >= m->num_route)
    return fail(MPCMMD_E_INVALID, "world: goal_index outside the route");
  if (m->num_batch < 1) return fail(MPCMMD_E_INVALID, "world: num_batch >= 1");
  if (m->noise != 0 && m->noise != 1) return fail(MPCMMD_E_INVALID, "world: noise must be 0 (gaussian) or 1 (beta)");
  if (!m->route_x || !m->route_y || !m->route_arc || !m->spline_x || !m->spline_y || !m->pdot4 || !m->chol ||
      !m->pop0)
    return fail(MPCMMD_E_INVALID, "world model: null array");
  if (!io->cx || !io->cy || !io->steer || (!io->u && !io->key) || !io->mean || !io->pos || !io->ego || !io->done_tick ||
      !io->init_state || !io->x_wp || !io->y_wp || !io->obstacles || !io->pop || !io->log_d || !io->log_f ||
      !io->log_i || (m->total_obs > 0 && !io->vehicles))
    return fail(MPCMMD_E_INVALID, "world step: null array");
  return MPCMMD_OK;
}

VehScalars veh_scalars(const mpcmmd_world_routed& r) {
  return VehScalars{r.acc_max, r.brake, r.gap0, r.headway, r.length, r.lane_tol, r.gap_min, r.acc_min};
}

int check_world_routed(const mpcmmd_world_model* m, const mpcmmd_world_routed* rt) {
  if (!m || !rt) return fail(MPCMMD_E_INVALID, "null argument");
  if (m->total_obs > 0 && (!rt->veh_s || !rt->veh_v || !rt->veh_param))
    return fail(MPCMMD_E_INVALID, "routed vehicles: null array");
  if (!(rt->acc_max > 0.0f) || !(rt->brake > 0.0f) || !(rt->gap_min > 0.0f) || !(rt->acc_min < 0.0f) ||
      !(rt->lane_tol >= 0.0f))
    return fail(MPCMMD_E_INVALID,
                "routed vehicles: acc_max > 0, brake > 0, gap_min > 0, acc_min < 0, lane_tol >= 0 must hold");
  return MPCMMD_OK;
}

void world_step_host(const mpcmmd_world_model& m, int tick, const mpcmmd_world_step_io& io, WorldDraw draw,
                     const mpcmmd_world_routed* rt) {
  const WorldScalars w = world_scalars(m);
  const bool reset = rt && tick < 0;  // the chained route's reset-mode step: no plan, nothing moves, no log
  WorldEgo e{io.pos[0], io.pos[1], io.ego[0], io.ego[1], io.ego[2]};
  WorldControl c{};
  float u[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!reset) {
    c = world_controller(w, m.pdot4, io.cx, io.cy, io.steer, e.v);
    if (io.u) std::memcpy(u, io.u, sizeof u);
    else draw(w.noise, io.key[0], m.seed, tick, c.a_c, c.s_c, u);
    world_perturb(w, u, c);
  }
  const bool frozen = reset || io.done_tick[0] >= 0;
  if (!frozen) {
    e = world_ego_step<HostMath>(e, c.a, c.s, w.dt);
    if (!rt)
      for (int o = 0; o < w.total; ++o) {
        float* v = io.vehicles + size_t(o) * 5;
        v[0] = v[0] + v[2] * w.dt;
        v[1] = v[1] + v[3] * w.dt;
      }
    io.pos[0] = e.x, io.pos[1] = e.y;
    io.ego[0] = e.v, io.ego[1] = e.psi, io.ego[2] = e.psidot;
  }
  // the ego on the route
  uint64_t best = ~uint64_t(0);
  int idx = 0;
  for (int j = 0; j < w.n_route; ++j) {
    const uint64_t k = route_key(e.x, e.y, m.route_x[j], m.route_y[j]);
    if (k < best) best = k, idx = j;
  }
  const double s0 = m.route_arc[idx];
  const float d = world_lateral(w, m.route_x, m.route_y, m.route_arc, m.spline_x, m.spline_y, idx, e);
  if (rt) {  // the routed vehicles: every leader from the states before the step, then the rows
    const VehScalars p = veh_scalars(*rt);
    VehLeader lead[kWorldMaxObs];
    if (!frozen)
      for (int o = 0; o < w.total; ++o)
        lead[o] = vehicle_leader(p, o, w.total, rt->veh_s, rt->veh_param, 2, rt->veh_v, s0, d, e.v);
    for (int o = 0; o < w.total; ++o) {
      float a = 0.0f;
      if (!frozen) vehicle_advance(p, w.dt, rt->veh_param[o * 2 + 1], lead[o], rt->veh_s + o, rt->veh_v + o, &a);
      if (rt->veh_log && !reset) rt->veh_log[o * 2] = rt->veh_v[o], rt->veh_log[o * 2 + 1] = a;
      vehicle_pose<HostMath>(m.route_arc, m.spline_x, m.spline_y, w.n_route, rt->veh_s[o], rt->veh_param[o * 2],
                             rt->veh_v[o], io.vehicles + size_t(o) * 5);
    }
  }
  // flags
  float clear = -std::numeric_limits<float>::infinity();
  bool clear_nan = false;
  for (int o = 0; o < w.total; ++o) {
    const float t = clear_term<HostMath>(w, e, io.vehicles + size_t(o) * 5);
    if (t != t) clear_nan = true;
    clear = fmaxf(clear, t);  // a NaN term is ignored here and reported below
  }
  if (clear_nan) clear = canon_nan(NAN);
  const bool lane_out = d < w.y_lb || d > w.y_ub;
  const bool collided = !(clear <= 0.0f);
  const bool goal = world_goal(w, m.route_x, m.route_y, e);
  if (!frozen && (collided || goal)) io.done_tick[0] = tick;
  if (!reset) {
    io.log_d[0] = e.x, io.log_d[1] = e.y, io.log_d[2] = s0;
    const float lf[MPCMMD_WORLD_LOG_F] = {e.v, e.psi, e.psidot, c.a_c, c.s_c, c.a, c.s, u[0], u[1], u[2],
                                          u[3], clear, d};
    std::memcpy(io.log_f, lf, sizeof lf);
    io.log_i[0] = idx, io.log_i[1] = lane_out, io.log_i[2] = collided, io.log_i[3] = goal;
  }
  // the next tick's raw inputs
  const float init[6] = {0.0f, 0.0f, e.v, 0.0f, e.psi, e.psidot};
  std::memcpy(io.init_state, init, sizeof init);
  for (int i = 0; i < w.P; ++i)
    world_waypoint(w, m.route_arc, m.spline_x, m.spline_y, s0, e, i, io.x_wp + i, io.y_wp + i);
  int src[kWorldMaxObs], K = 0;
  for (int o = 0; o < w.total; ++o)
    if (obstacle_kept<HostMath>(e, io.vehicles + size_t(o) * 5)) src[K++] = o;
  const int Lp = K > w.O ? K : w.O;  // padded by the last kept vehicle; none kept: all 300 m away
  const float far[5] = {300.0f, 300.0f, 0.0f, 0.0f, 0.0f};
  double key[kWorldMaxObs];
  const float* row[kWorldMaxObs];
  for (int j = 0; j < Lp; ++j) {
    row[j] = K == 0 ? far : io.vehicles + size_t(src[j < K ? j : K - 1]) * 5;
    key[j] = obstacle_dist2(e, row[j][0], row[j][1]);
  }
  for (int j = 0; j < Lp; ++j) {
    int rank = 0;
    for (int i = 0; i < Lp; ++i) rank += dist_before(key[i], i, key[j], j) ? 1 : 0;
    if (rank >= w.O) continue;
    float* out = io.obstacles + size_t(rank) * 5;
    out[0] = obstacle_shift(row[j][0], e.x), out[1] = obstacle_shift(row[j][1], e.y);
    out[2] = row[j][2], out[3] = row[j][3], out[4] = row[j][4];
  }
  for (int b = 0; b < w.B; ++b)
    for (int a = 0; a < 8; ++a) io.pop[size_t(b) * 8 + a] = world_pop(io.mean, m.chol, m.pop0 + size_t(b) * 8, a);
}

}  // namespace mpcmmd
