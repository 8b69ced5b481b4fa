// Host arithmetic of libmpcmmd's create / begin / finish paths: what the
// handle code (handle.hip, begin.hip, sequence.hip, validate_api.hip) uploads as raw bytes or unpacks
// from a result.  No HIP: compiled by g++, built a second time under
// ASan/UBSan (tests/native/asan_host.cpp) and tested on the CPU.
#pragma once
#include <cstdint>
#include <vector>

#include "carla_host.hpp"
#include "host_constants.hpp"

namespace mpcmmd {

// Cholesky factor L (row-major, lower) of the 8 x 8 matrix a; false if a is
// not positive definite.
bool chol8(const double* a, double* L);

// Handle constants.  fp32 basis [3][100][11]: P, Pdot, Pddot.
std::vector<float> pack_basis(const ProblemConsts& pc);
// guess: c_bar = G v + h with G[k][j] = sum_i Kinv[k][i] (-k_p colsum_j[i]); [2][11][4]
std::vector<double> pack_guess_g(const ProblemConsts& pc);
// the [:11,:11] blocks of a pair of KKT inverses (kx [14][14], ky [15][15]): [2][11][11]
std::vector<double> pack_proj_m(const std::vector<double>& kx, const std::vector<double>& ky);

// Per-solve KKT columns of one configuration, [4][11]: guess x, guess y,
// projection x, projection y, from the boundary vectors (cem_helper.py:
// 152-167).  proj_kx / proj_ky: the projection's KKT inverses (compute_cem_det
// has its own).
void solve_columns(const ProblemConsts& pc, const double* proj_kx, const double* proj_ky, const double bx[3],
                   const double by[4], double* sc);

// st0 [8] of one configuration from init_state (x, y, vx, vy, ., .): heading from the velocity
void initial_state(const float* init_state, float* st0);

// obstacle tracks x_obs / y_obs [O][100] -> [2][O][H]
void obstacle_transpose(const float* x_obs, const float* y_obs, int O, int H, float* out);

// sampling_param (cem_helper.py:122-150): pop [B][8] = mean + L z with
// L L^T = cov and z [B][8] standard normals, the four speeds clipped to
// [0.1, 30].  Throws std::invalid_argument if cov is not positive definite.
void initial_population(const float* mean, const float* cov, const float* z, int B, float* pop);

// external noise rows [T][3][S][H] -> device [T][3][H][S]
std::vector<float> roll_transpose(const float* roll, int T, int S, int H);

PathView path_view(int num_path, const float* x, const float* y, const float* arc, const float* Fxd,
                   const float* Fyd, const float* kappa);

// The initial-state prefix of a CARLA row: (vx, vy, psi) from speed and heading.
void carla_velocity_heading(float v0, float psi0, float* vx, float* vy, float* psi);

// CARLA per-solve setup (carla/optimizer/cem.py:248-264 mmd, 476-492 cvar):
// R noisy initial states (compute_noisy_init_state(_baseline),
// cem_helper.py:660-715; R = n^2 for mmd_opt, n for cvar, 1 for det) as
// rollout rows [R0][8] (R0 >= R, the rest zero), and the boundary vectors from
// the mean of their Frenet states (global_to_frenet_vmap_1, cem_helper.py:
// 348-388).  init_state is init_state_global = (x, y, v, vdot, psi, psidot)
// (C/main_carla.py:352); eps [R][4] standard normals.
void carla_rows(const ProblemConsts& pc, int R, int R0, const float* init_state, const PathView& path,
                const float* eps, std::vector<float>& rows, double* bx, double* by);

// The CARLA setup of a batch of G configurations (mpcmmd_carla_begin_batch):
// whole host images of the three per-configuration CARLA buffers, each
// uploaded as ONE staged piece whatever G is (buffers.hpp declares 1, 6 and 2
// pieces for them), and the boundary vectors of every configuration.
struct CarlaBatch {
  std::vector<float> rows;     // st0r [G][R0][8]
  std::vector<float> path;     // path [G][6][kMaxPath]: array k of path g at (g 6 + k) kMaxPath, zero padded
  std::vector<float> tracks;   // obs_full [G][2][O][100]; empty unless det
  std::vector<double> bx, by;  // [G][3], [G][4]
  struct Piece {
    const char* buffer;  // the device buffer's name (buffers.hpp)
    const std::vector<float>* image;
  };
  std::vector<Piece> staged() const;  // the staged copies of a begin, in upload order
};

// carla_rows of every configuration into its slice: init_state [G][6], paths
// [G], eps[g] -> [R][4]; rows [G][R0][8], bx [G][3], by [G][4].  Slice g is
// bit for bit what carla_rows gives for configuration g alone.
void carla_rows_batch(const ProblemConsts& pc, int G, int R, int R0, const float* init_state, const PathView* paths,
                      const float* const* eps, std::vector<float>& rows, double* bx, double* by);

// the path image [G][6][kMaxPath] of G paths of one length (x, y, arc_vec, Fx_dot, Fy_dot, kappa)
std::vector<float> path_image(int G, const PathView* paths);

// compute_cem_det's tracks, all 100 plan points: x_obs / y_obs [G][O][100] -> [G][2][O][100]
std::vector<float> det_track_image(int G, int O, const float* x_obs, const float* y_obs);

// The whole CARLA setup: rows and boundary vectors (R noisy rows of R0), the
// path image, and with det the track image.
CarlaBatch carla_batch(const ProblemConsts& pc, int G, int R, int R0, int O, bool det, const float* init_state,
                       const PathView* paths, const float* const* eps, const float* x_obs, const float* y_obs);

// The controls of K plans for the CARLA validator (compute_controls,
// cem_helper.py: acc = diff([v, v_end]) / t): v, steer [K][100] -> acc, steer_out [K][H]
void plan_controls(const float* v, const float* steer, int K, int H, std::vector<float>& acc,
                   std::vector<float>& steer_out);

// Tables of the first beta-iteration's selection sel [100 n] (mother rows in
// [0, M)) with sigmas sig [100], indexed by mother row for k_bmoment: rp
// [M + 1] row pointers, pairs (i, sigma bits) grouped by row, and rperm, the
// rows in descending number of distinct sigmas among a row's pairs (stable).
// Throws std::runtime_error on a row out of range.
struct Sel0Tables {
  std::vector<int32_t> rp, pairs, rperm;
};
Sel0Tables first_selection_tables(const int32_t* sel, const float* sig, int n, int M);

// beta_z of one iteration: [89][M+1] (draw order) -> device bz_index layout
// (the sampler's lane image per 16-position block, zero padded), so the
// generation kernel reads whole blocks without bounds in coalesced float4 loads
std::vector<float> beta_z_image(const float* z, int M);

// v_best [100] of a CARLA result: v = sqrt((Pdot cx)^2 + (Pdot cy)^2), fp64 sums rounded once
void plan_speed(const ProblemConsts& pc, const float* cx, const float* cy, float* v_best);

}  // namespace mpcmmd
