// libmpcmmd: the launch sequence of one outer iteration (the stages of
// mpcmmd_run_stage), mpcmmd_iterate and its graph capture.
#include <algorithm>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "draws.hpp"
#include "handle.hpp"
#include "solve_host.hpp"

using namespace mpcmmd;

namespace {

// The first beta-iteration's selection (samples sqrt(20) beta_z0, shared by
// every candidate): k_bselect on one candidate, read back, and its pairs
// indexed by mother row for k_bmoment.  Once per beta_z0 table.
void ensure_sel0(mpcmmd_handle* h) {
  if (h->sel0_valid) return;
  const int n = h->n, M = h->M, np = kBetaSamples * n;
  Params q = h->p;
  q.b0 = 0;
  q.nb = 1;
  launch_bselect(q, 0, h->stream);
  HIPC(hipGetLastError());
  std::vector<int32_t> sel(np);
  std::vector<float> sig(kBetaSamples);
  HIPC(hipMemcpyAsync(sel.data(), h->p.bsel, np * 4, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipMemcpyAsync(sig.data(), h->p.bsig, kBetaSamples * 4, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  const Sel0Tables tab = first_selection_tables(sel.data(), sig.data(), n, M);
  upload(h, h->p.sel0, sel.data(), np * 4);
  upload(h, h->p.sig0, sig.data(), kBetaSamples * 4);
  upload(h, h->p.rp0, tab.rp.data(), (M + 1) * 4);
  upload(h, h->p.rpair0, tab.pairs.data(), size_t(np) * 8);
  upload(h, h->p.rperm, tab.rperm.data(), size_t(M) * 4);
  HIPC(hipStreamSynchronize(h->stream));  // host temporaries
  h->sel0_valid = true;
  ++h->sel0_gen;
}

// k_bmoment wrote the first beta-iteration's direct row sums for the sel0
// table current at its launch; stages 5/6 at t = 0 rely on them
void check_bmoment_gen(mpcmmd_handle* h) {
  if (h->bmoment_gen != h->sel0_gen)
    throw std::invalid_argument(
        "beta_z0 changed (or stage 4 not run) since k_bmoment: rerun stage 4 before beta-iteration 0");
}

// The three thirds of one beta-CEM iteration (compute_beta.py:112-147) of
// candidates [p.b0, p.b0 + p.nb), also stages 5, 6 and 7 of the stage API:
// the samples and their top-n rows,
void run_beta_select(mpcmmd_handle* h, const Params& p, int tb, hipStream_t st) {
  if (tb > 0) h->launch(kKBSample, [&] { launch_bsample(p, tb, st); });
  h->launch(kKBSelect, [&] { tb == 0 ? launch_bsel0(p, st) : launch_bselect(p, tb, st); });
}

// the kernel sums and the QPs,
void run_beta_qp(mpcmmd_handle* h, const Params& p, int tb, hipStream_t st) {
  h->launch(kKBKernel, [&] { launch_bkernel(p, tb, st); });
  if (tb > 0) h->launch(kKBDirect, [&] { launch_bdirect(p, tb, st); });  // first iteration: in k_bmoment
  h->launch(kKBQp, [&] { launch_bqp(p, tb, st); });
}

// the elites and the next iteration's generators
void run_beta_elite(mpcmmd_handle* h, const Params& p, int tb, hipStream_t st) {
  h->launch(kKBElite, [&] { launch_belite(p, tb, st); });
  h->launch(kKBGen, [&] { launch_bgen(p, tb, st); });
}

// one beta-CEM iteration: the three thirds in order
void run_beta_iteration(mpcmmd_handle* h, const Params& p, int tb, hipStream_t st) {
  run_beta_select(h, p, tb, st);
  run_beta_qp(h, p, tb, st);
  run_beta_elite(h, p, tb, st);
}

// the 20 beta-CEM iterations of every candidate: one chain per candidate
// group, each group on its own stream between two events of the handle's
// stream (profiling runs them on the handle's stream, one after another,
// so the HIP-event timings are per kernel)
void run_beta_cem(mpcmmd_handle* h) {
  const int B = h->p.Bt;  // every candidate of every configuration
  if (h->fused_small && bcem_small_ok(h->p)) {
    h->launch(kKBcemSmall, [&] { launch_bcem_small(h->p, h->stream); });
    return;
  }
  // the default split applies to launches of >= 1024 candidates (a batch
  // handle may run fewer configurations than it holds); MPCMMD_GROUPS forces it
  const bool small = B >= 64 && B <= 256;
  const int Gw = h->prof ? 1 : (B >= 1024 || h->groups_forced ? h->groups : (small ? std::min(h->groups, h->small_groups) : 1));
  const int G = std::min(Gw, int(mpcmmd_handle::kMaxGroups));  // gstream[] / gev_done[] hold kMaxGroups
  if (G <= 1) {
    for (int tb = 0; tb < kBetaIters; ++tb) run_beta_iteration(h, h->p, tb, h->stream);
    return;
  }
  std::vector<Params> pg(G, h->p);
  const int per = (B + G - 1) / G;
  for (int g = 0; g < G; ++g) {
    pg[g].b0 = g * per;
    pg[g].nb = std::max(0, std::min(per, B - g * per));
  }
  HIPC(hipEventRecord(h->gev_start, h->stream));
  for (int g = 0; g < G; ++g) HIPC(hipStreamWaitEvent(h->gstream[g], h->gev_start, 0));
  for (int tb = 0; tb < kBetaIters; ++tb)
    for (int g = 0; g < G; ++g)
      if (pg[g].nb > 0) run_beta_iteration(h, pg[g], tb, h->gstream[g]);
  for (int g = 0; g < G; ++g) {
    HIPC(hipEventRecord(h->gev_done[g], h->gstream[g]));
    HIPC(hipStreamWaitEvent(h->stream, h->gev_done[g], 0));
  }
}

// CARLA risk (k_carla.hip): rollouts of the rows from their noisy initial
// states (mode 0: cvar's n baseline rows; mode 1: mmd_opt's reduced set),
// their Frenet transforms, the reducers
void run_carla_risk(mpcmmd_handle* h, int t, int mode) {
  const Params& p = h->p;
  h->launch(kKRollCarla, [&] { launch_roll_carla(p, t, mode, h->stream); });
  h->launch(kKFrenet, [&] { launch_frenet(p, h->stream); });
  h->launch(kKRiskCarla, [&] { launch_risk_carla(p, t, mode, h->stream); });
}

// the draws k_select produces ahead for this solve (mpcmmd_handle::ahead_t)
int ahead_kind(const mpcmmd_handle* h) {
  if (!h->ahead_on) return 0;
  const bool beta = h->p.noise == MPCMMD_NOISE_BETA && h->p.cost != MPCMMD_COST_DET;  // det: no rollouts
  return (h->ext_roll && h->ext_res ? 0 : kAheadNoise) | (beta ? kAheadGamma : 0);
}

// the Beta attempt table of iteration t, unless k_select of t - 1 drew it
// (k_gamma_tab also zeroes the Beta fix-up count).  A table drawn ahead is
// used once: ahead_t is cleared here, so a rerun of stage 2 / 4 for the same t
// (stage API) draws the table again and restarts the fix-up list instead of
// appending to it.
void ensure_gamma_tab(mpcmmd_handle* h, int t) {
  if (h->p.noise != MPCMMD_NOISE_BETA) return;
  if (h->ahead_t == t) {
    h->ahead_t = -1;  // consumed (this iteration's noise was drawn ahead too: stage 0 ran before)
    return;
  }
  h->launch(kKGammaTab, [&] { launch_gamma_tab(h->p, t, h->stream); });
  h->ahead_t = -1;  // the table's one slot now holds t
}

// mmd_opt's preparation (stage 4): mother rollouts, features, their distance
// matrix and its series records
void run_mmd_prep(mpcmmd_handle* h, int t) {
  const Params& p = h->p;
  ensure_gamma_tab(h, t);
  ensure_sel0(h);
  h->launch(kKMother, [&] { launch_mother(p, t, h->stream); });
  h->launch(kKBDist, [&] { launch_bdist(p, h->stream); });
  h->launch(kKBMoment, [&] { launch_bmoment(p, h->stream); });
  h->bmoment_gen = h->sel0_gen;
}

// mmd_opt's final reducer (stage 8) over the reduced set the beta-CEM chose
void run_mmd_final(mpcmmd_handle* h, int t) {
  if (h->carla) run_carla_risk(h, t, 1);
  else h->launch(kKMmdFinal, [&] { launch_mmdfinal(h->p, t, h->stream); });
}

void run_stage(mpcmmd_handle* h, int stage, int t) {
  const Params& p = h->p;
  switch (stage) {
    case 0:
      if (!(h->ahead_t == t && (ahead_kind(h) & kAheadNoise))) h->launch(kKNoise, [&] { launch_noise(p, t, h->stream); });
      break;
    case 1:
      h->launch(kKFront, [&] { launch_front(p, t, h->stream); });
      h->prep_t = -1;  // new residuals; with select_prep no cost norms until stage 2
      break;
    case 2:
      if (p.cost == MPCMMD_COST_DET) break;  // compute_cem_det: no rollouts, zero risks (carla/optimizer/cem.py:717-722)
      if (p.cost == MPCMMD_COST_MMD_OPT) {
        if (!h->mmd_ok) throw std::invalid_argument("mmd_opt unsupported for this configuration: " + h->mmd_why);
        run_mmd_prep(h, t);
        run_beta_cem(h);
        run_mmd_final(h, t);
        break;
      }
      ensure_gamma_tab(h, t);
      if (p.noise == MPCMMD_NOISE_BETA) h->launch(kKBetaPlanes, [&] { launch_beta_planes(p, t, h->stream); });
      if (h->carla) {
        run_carla_risk(h, t, 0);
      } else {
        h->launch(kKRiskBaseline, [&] { launch_risk_baseline(p, t, h->stream); });
        if (p.select_prep) h->prep_t = t;
      }
      break;
    case 3: {
      if (p.select_prep && h->prep_t != t)
        throw std::invalid_argument(
            "stage 3 needs stage 2 of the same iteration after stage 1 (the risk launch sorts the residuals and "
            "forms the cost norms: select_prep; MPCMMD_SELECT_PREP=0 moves them back to stages 1 and 3)");
      const int kind = ahead_kind(h), nxt = kind && t + 1 < h->T ? t + 1 : -1;
      h->launch(kKSelect, [&] { launch_select(p, t, h->stream, nxt, kind); });
      h->ahead_t = nxt;
      break;
    }
    case 4:
    case 5:
    case 6:
    case 7:
    case 8:
      if (p.cost != MPCMMD_COST_MMD_OPT || !h->mmd_ok) throw std::invalid_argument("stages 4-8 need cost mmd_opt");
      if (stage >= 5 && stage <= 7 && t >= kBetaIters) throw std::invalid_argument("beta-CEM iteration out of range");
      if (stage == 4) run_mmd_prep(h, t);
      if (stage == 5) {
        if (t == 0) {
          ensure_sel0(h);
          check_bmoment_gen(h);
        }
        run_beta_select(h, p, t, h->stream);
      }
      if (stage == 6) {
        if (t == 0) check_bmoment_gen(h);
        run_beta_qp(h, p, t, h->stream);
      }
      if (stage == 7) run_beta_elite(h, p, t, h->stream);
      if (stage == 8) run_mmd_final(h, t);
      break;
    default:
      throw std::invalid_argument("stage must be 0..8");
  }
}

}  // namespace

extern "C" {

int mpcmmd_iterate(mpcmmd_handle* h, int32_t t_begin, int32_t count) {
  if (!h) return fail(MPCMMD_E_INVALID, "null handle");
  if (!h->begun) return fail(MPCMMD_E_STATE, "mpcmmd_iterate before mpcmmd_begin");
  if (t_begin < 0 || count < 0 || t_begin + count > h->T) return fail(MPCMMD_E_INVALID, "iteration range");
  return guarded([&] {
    check_device(h);
    auto body = [&](int t_lo, int cnt) {
      for (int t = t_lo; t < t_lo + cnt; ++t) {
        if (!h->ext_roll || !h->ext_res) {
          if (h->ext_roll != h->ext_res) throw std::invalid_argument("roll and resample draws go together");
          run_stage(h, 0, t);
        }
        run_stage(h, 1, t);
        run_stage(h, 2, t);
        run_stage(h, 3, t);
      }
    };
    // graphs of a whole solve (count == T) or of single iterations (count ==
    // 1: all T captured at the first use, so no capture lands in a timed
    // loop), captured from the handle's stream.  mmd_opt launches of 64..256
    // candidates run their beta-CEM candidate groups on the group streams
    // inside the capture: run_beta_cem's event fork / join makes them parallel
    // branches of the graph.  Launches of >= 1024 candidates, and any split
    // forced by MPCMMD_GROUPS, are not captured: they are launched directly
    const bool capturable = h->cost != MPCMMD_COST_MMD_OPT || (h->p.Bt < 1024 && !h->groups_forced);
    const bool whole = t_begin == 0 && count == h->T;
    if (h->graphs && !h->prof && capturable && (whole || count == 1)) {
      if (h->cost == MPCMMD_COST_MMD_OPT) ensure_sel0(h);  // host read-back: never inside a capture
      // key: ... and whether the first iteration's draws were drawn ahead (ai)
      auto key_of = [&](int tb, int cnt, int ai) {
        return std::make_tuple(h->cost, h->p.P, int(h->ext_roll), h->G, whole ? 0 : tb, cnt, ai);
      };
      auto capture = [&](int tb, int cnt, int ai) {
        const int saved = h->ahead_t;
        h->ahead_t = ai ? tb : -1;
        hipGraph_t g = nullptr;
        HIPC(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        try {
          body(tb, cnt);
        } catch (...) {
          (void)hipStreamEndCapture(h->stream, &g);
          if (g) (void)hipGraphDestroy(g);
          h->ahead_t = saved;
          throw;
        }
        HIPC(hipStreamEndCapture(h->stream, &g));
        hipGraphExec_t e = nullptr;
        HIPC(hipGraphInstantiate(&e, g, nullptr, nullptr, 0));
        h->gexec.emplace(key_of(tb, cnt, ai), std::make_pair(g, e));
        h->gahead[key_of(tb, cnt, ai)] = h->ahead_t;
        h->ahead_t = saved;
      };
      const int ai_now = h->ahead_t == t_begin && ahead_kind(h) ? 1 : 0;
      if (h->gexec.find(key_of(t_begin, count, ai_now)) == h->gexec.end()) {
        if (whole) {
          capture(0, h->T, ai_now);
        } else {  // the in-order pattern (iteration tb's draws drawn by tb - 1), then the one asked for
          for (int tb = 0; tb < h->T; ++tb) {
            const int ai = tb > 0 && ahead_kind(h) ? 1 : 0;
            if (h->gexec.find(key_of(tb, 1, ai)) == h->gexec.end()) capture(tb, 1, ai);
          }
          if (h->gexec.find(key_of(t_begin, 1, ai_now)) == h->gexec.end()) capture(t_begin, 1, ai_now);
        }
      }
      HIPC(hipGraphLaunch(h->gexec.find(key_of(t_begin, count, ai_now))->second.second, h->stream));
      h->ahead_t = h->gahead[key_of(t_begin, count, ai_now)];
    } else {
      body(t_begin, count);
    }
    if (count > 0) h->last_t = t_begin + count - 1;  // a zero-count call runs nothing
    return MPCMMD_OK;
  });
}

int mpcmmd_set_graphs(mpcmmd_handle* h, int32_t enable) {
  if (!h) return fail(MPCMMD_E_INVALID, "null handle");
  return guarded([&] {
    check_device(h);
    h->graphs = enable != 0;
    return MPCMMD_OK;
  });
}

int mpcmmd_sync(mpcmmd_handle* h) {
  if (!h) return fail(MPCMMD_E_INVALID, "null handle");
  return guarded([&] {
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));
    if (h->prof) h->collect();
    return MPCMMD_OK;
  });
}

int mpcmmd_run_stage(mpcmmd_handle* h, int32_t stage, int32_t t) {
  if (!h) return fail(MPCMMD_E_INVALID, "null handle");
  if (!h->begun) return fail(MPCMMD_E_STATE, "run_stage before mpcmmd_begin");
  const bool beta_stage = stage >= 5 && stage <= 7;
  if (t < 0 || (!beta_stage && t >= h->T)) return fail(MPCMMD_E_INVALID, "iteration out of range");
  return guarded([&] {
    check_device(h);
    run_stage(h, stage, t);
    if (stage == 3) h->last_t = t;
    HIPC(hipStreamSynchronize(h->stream));
    return MPCMMD_OK;
  });
}

}  // extern "C"
