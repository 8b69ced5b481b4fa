"""The scene queue of the synthetic closed loop on the GPU (CEM.run_campaign):
N scenes through E slots of the chained loop, a slot refilled by k_mpc_queue as soon as its episode
ends.  The reference of every comparison is the existing chained route: scene i alone,
run_episodes(cost, vehicles[i:i+1], starts[i:i+1], T_EP, chained=True, keys=[key_i]) on a handle of
the same max_configs.  Every scene's rows of a campaign, up to and including its end tick, equal
the lone run's first rows bit for bit -- the drawn variates included, which is what the per-slot
tick is for.  Small shapes: n = 4, 2 obstacles, num_prime 8, num_batch 20, maxiter_cem 3; 7 scenes,
3 slots, 5 ticks per episode."""
import ctypes as C

import numpy as np
import pytest

import mpc_queue_model as qm

pytestmark = pytest.mark.gpu

F32 = np.float32
ROWS = ("log_d", "log_f", "log_i", "cx", "cy", "mean")
N, E, T_EP = 7, 3, 5
GOAL_X = 200.0
KEYS = 17 + 100003 * np.arange(N)
# scene 1 collides, scene 3 reaches the goal, both at their local tick 0; the others run 5 ticks
ENDS = [None, (0, qm.COLLISION), None, (0, qm.GOAL), None, None, None]
CASES = {"static-cvar": ("static", "cvar", "gaussian", False), "static-saa": ("static", "saa", "beta", False),
         "dynamic-mmd_opt": ("dynamic", "mmd_opt", "gaussian", True)}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def scenes(variant):
    """7 scenes: two obstacles ahead, starts a few metres apart; scene 1 has a vehicle on the ego's
    start, scene 3 starts 1 cm short of the goal at 5 m/s."""
    y = -1.75 if variant == "dynamic" else 1.75
    v = 3.0 if variant == "dynamic" else 0.0
    vehicles = np.empty((N, 2, 4), F32)
    starts = np.empty((N, 4))
    for i in range(N):
        vehicles[i] = [[35 + 2 * i, y, v, 0], [50 + 3 * i, -y if i % 2 else y, v, 0]]
        starts[i] = [i, y + 0.1 * (i % 3 - 1), 4.0 + 0.5 * (i % 4), 0.05 * (i % 3 - 1)]
    vehicles[1, 0, :2] = starts[1, :2]
    starts[3] = [GOAL_X - 0.01, y, 5.0, 0.0]
    target = np.empty((N, 2, 2), F32)
    target[:, :, 0] = 6.0 + 0.05 * np.arange(N)[:, None] - 0.1 * np.arange(2)[None, :]
    target[:, :, 1] = -1.75
    return vehicles, starts, target


class Campaigns:
    """One handle per case, the lone runs made once and shared, never modified."""

    def __init__(self):
        self.made = {}

    def get(self, case):
        if case not in self.made:
            from optimizer.cem import CEM
            variant, cost, noise, planned = CASES[case]
            prob = CEM(4, 2, 0.1, 8, noise, 0.05, 0.01, num_batch=20, variant=variant, maxiter_cem=3, max_configs=E)
            vehicles, starts, target = scenes(variant)
            kw = lambda sl: dict(planned=dict(target=target[sl], acc=None)) if planned else {}
            alone = [prob.run_episodes(cost, vehicles[i:i + 1], starts[i:i + 1], T_EP, chained=True, keys=[KEYS[i]],
                                       goal_x=GOAL_X, **kw(slice(i, i + 1))) for i in range(N)]
            self.made[case] = dict(prob=prob, cost=cost, vehicles=vehicles, starts=starts, kw=kw, alone=alone,
                                   rows=ROWS + (("veh",) if planned else ()))
        return self.made[case]

    def close(self):
        for c in self.made.values():
            c["prob"].handle.close()


@pytest.fixture(scope="module")
def campaigns(native):
    """MPCMMD_GENWAVE is read when a handle is created: every handle of this module gets the same
    beta-CEM generators whatever its capacity (as tests/test_gpu_mpc_loop.py pins it)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("MPCMMD_GENWAVE", "1")
    c = Campaigns()
    yield c
    c.close()
    mp.undo()


def check_lone_ends(alone):
    """The lone runs end where the scenes were built to end."""
    for i, a in enumerate(alone):
        want = -1 if ENDS[i] is None else ENDS[i][0]
        assert a["done_tick"][0] == want, (i, a["done_tick"])
        if ENDS[i] is not None:
            col = 1 if ENDS[i][1] == qm.COLLISION else 2
            assert a["log_i"][0, 0, col] == 1 and (col == 1 or a["log_i"][0, 0, 1] == 0), (i, a["log_i"][0, 0])


def check_scene(c, got, i, rows_n, what):
    for k in c["rows"]:
        assert same(got[k][:rows_n, i], c["alone"][i][k][:rows_n, 0]), (what, "scene", i, k)
    assert same(got["log_f"][:rows_n, i, 7:10], c["alone"][i]["log_f"][:rows_n, 0, 7:10]), (what, i, "variates")


@pytest.mark.parametrize("case", list(CASES))
def test_campaign_equals_lone_runs(campaigns, case):
    c = campaigns.get(case)
    check_lone_ends(c["alone"])
    got = c["prob"].run_campaign(c["cost"], c["vehicles"], c["starts"], T_EP, slots=E, keys=KEYS, goal_x=GOAL_X,
                                 **c["kw"](slice(None)))
    sched, ticks, finished = qm.schedule(E, T_EP, ENDS)
    assert ticks == 10 and -(-N // E) * T_EP == 15, "10 lockstep ticks where batches of 3 need 15"
    for i in range(N):
        assert got["sched"][i].tolist() == sched[i].tolist(), (i, got["sched"][i], sched[i])
    assert got["lockstep_ticks"] == 10 and got["started"] == N and got["finished"] == N
    assert sched[5].tolist() == [0, 5, 5, 3] and sched[6].tolist() == [2, 5, 5, 3], "slots 0 and 2 refill in slot order"
    assert sorted(np.flatnonzero(sched[:, 0] == 1)) == [1, 3, 4], "slot 1 is refilled twice"
    for i in range(N):
        check_scene(c, got, i, int(sched[i, 2]), case)
        assert got["end_tick"][i] == sched[i, 2] - 1 and got["end_reason"][i] == sched[i, 3]
        assert got["done_tick"][i] == c["alone"][i]["done_tick"][0]
    uu = got["log_f"][:, [0, 2, 4, 5, 6], 9]
    assert np.unique(uu).size == uu.size, "every (scene, tick) its own variates"


def test_budget_then_two_more_ticks(campaigns):
    """8 lockstep ticks: 5 scenes finished, scenes 5 and 6 unfinished with 3 rows each; two more
    queue_run calls of one tick finish them with the full campaign's bits."""
    c = campaigns.get("static-cvar")
    prob = c["prob"]
    ctx, cov = prob.open_campaign(c["vehicles"], c["starts"], T_EP, 10, slots=E, keys=KEYS, goal_x=GOAL_X)
    try:
        ctx.queue_run(c["cost"], 0, 8, cov)
        assert ctx.queue_status() == (7, 5)
        part = prob.campaign_result(ctx, 8, T_EP)
        want, ticks, finished = qm.schedule(E, T_EP, ENDS, budget=8)
        assert finished == 5 and part["sched"].tolist() == want.tolist()
        assert part["end_reason"][5:].tolist() == [qm.UNFINISHED] * 2 and part["end_tick"][5:].tolist() == [2, 2]
        for i in range(N):
            check_scene(c, part, i, int(want[i, 2]), "budget 8")
        ctx.queue_run(c["cost"], 8, 1, cov)
        assert ctx.queue_status() == (7, 5)
        ctx.queue_run(c["cost"], 9, 1, cov)
        assert ctx.queue_status() == (7, 7)
        full = prob.campaign_result(ctx, 10, T_EP)
    finally:
        ctx.close()
    assert full["sched"].tolist() == qm.schedule(E, T_EP, ENDS)[0].tolist()
    for i in range(N):
        check_scene(c, full, i, int(full["sched"][i, 2]), "8 + 1 + 1")


@pytest.mark.parametrize("n", [2, 3])
def test_idle_slots(campaigns, n):
    """N = 2 through 3 slots: slot 2 is idle from the start, owned by no scene, and changes no other
    slot's bits; N = E = 3: every slot idles once its scene has ended."""
    c = campaigns.get("static-cvar")
    got = c["prob"].run_campaign(c["cost"], c["vehicles"][:n], c["starts"][:n], T_EP, slots=E, keys=KEYS[:n],
                                 goal_x=GOAL_X)
    sched, ticks, _ = qm.schedule(E, T_EP, ENDS[:n])
    assert got["sched"].tolist() == sched.tolist() and got["lockstep_ticks"] == 5 and got["finished"] == n
    assert set(got["sched"][:, 0]) == set(range(n)), "no scene owns a slot beyond the table"
    for i in range(n):
        check_scene(c, got, i, int(sched[i, 2]), f"N = {n}")


@pytest.mark.parametrize("slots", [1, 3, 64, 65, 200])
def test_queue_kernel_equals_host_rule(native, slots):
    """k_mpc_queue through its one-launch harness against mpcmmd_mpc_queue_host on every output
    word: one wave, two waves' worth of slots with one slot in the second chunk, four chunks."""
    rng = np.random.default_rng(slots)
    for n_scenes in (max(slots - 2, 1), slots, 2 * slots + 3):
        for pattern in ("mixed", "all", "none", "exhaust"):
            st = qm.random_state(rng, slots, n_scenes, 5, pattern)
            host = native.mpc_queue(4, 5, device=None, **st)
            dev = native.mpc_queue(4, 5, device=0, **st)
            for k in qm.WORDS:
                assert same(dev[k], host[k]), (slots, n_scenes, pattern, k, np.flatnonzero(dev[k] != host[k])[:8])


def test_existing_routes_unchanged_around_a_campaign(campaigns):
    """run_episodes(chained=True) and mpcmmd_solve_batch on the same handle before and after a
    campaign return the same bits."""
    c = campaigns.get("static-cvar")
    prob, h = c["prob"], c["prob"].handle
    veh, st = c["vehicles"][:E], c["starts"][:E]
    init = np.array([0.0, 1.75, 5.0, 0.0, 0.0, 0.0], F32)
    mean = np.array([15.0] * 4 + [0.0] * 4, F32)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    tt = np.linspace(0, 15, 100).astype(F32)
    xo, yo = (veh[:, :, 0:1] + 0 * tt).astype(F32), (veh[:, :, 1:2] + 0 * tt).astype(F32)
    solve = lambda: h.solve_batch("cvar", [11, 12, 13], init, mean, cov, xo, yo, 15.0)
    loop = lambda: prob.run_episodes("cvar", veh, st, T_EP, chained=True, keys=KEYS[:E], goal_x=GOAL_X)
    before, loop_before = solve(), loop()
    prob.run_campaign("cvar", c["vehicles"], c["starts"], T_EP, slots=E, keys=KEYS, goal_x=GOAL_X)
    after, loop_after = solve(), loop()
    for a, b in zip(before, after):
        for k in ("cx", "cy", "cost_lane", "cost_obs"):
            assert same(np.asarray(a[k]), np.asarray(b[k])), k
    for k in ROWS + ("done_tick",):
        assert same(loop_before[k], loop_after[k]), k


def test_state_and_argument_errors(campaigns, native):
    """The queue's limits are errors with a message: MPCMMD_E_STATE (-4) with the validation stage
    on, for a queue run before a queue reset or after an ordinary one, and for mpcmmd_mpc_run after a
    queue reset; MPCMMD_E_INVALID (-1) for the arguments out of range."""
    c = campaigns.get("static-cvar")
    prob, L, fp = c["prob"], native.lib(), native._fptr
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    model = native.MpcModel(prob._cfg, cov, native.pop0_normals(prob._cfg), goal_x=GOAL_X)
    ctx = native.Mpc(prob.handle, model, 6)
    covp, vd = fp(cov.reshape(64)), fp(np.full(E, 15.0, F32))
    st = c["starts"]
    vel = np.concatenate([st[:, 2:4], np.zeros((N, 1))], 1).astype(F32)
    mean = np.tile(np.array([15.0] * 4 + [0.0] * 4, F32), (N, 1))
    table = dict(pos=st[:, :2], vel=vel, vehicles=c["vehicles"], mean=mean, cov=cov, v_des=15.0, keys=KEYS)
    ia, ib = C.c_int32(), C.c_int32()
    sched = np.zeros((N, 4), np.int32)
    sp = sched.ctypes.data_as(C.POINTER(C.c_int32))
    try:
        assert L.mpcmmd_mpc_queue_run(ctx._c, 2, 0, 1, covp) == -4 and b"before mpcmmd_mpc_queue_reset" in L.mpcmmd_last_error()
        assert L.mpcmmd_mpc_queue_status(ctx._c, C.byref(ia), C.byref(ib)) == -4
        assert L.mpcmmd_mpc_queue_log(ctx._c, sp) == -4
        for bad in (dict(slots=0), dict(slots=E + 1), dict(ticks_per_episode=0)):
            with pytest.raises(native.NativeError):
                ctx.queue_reset(**dict(dict(slots=E, ticks_per_episode=T_EP, **table), **bad))
        with pytest.raises(native.NativeError, match="planned policy"):
            ctx.queue_reset(E, T_EP, planned=dict(target=np.zeros((N, 2, 2)), acc=np.zeros((N, 2, 2))), **table)
        with pytest.raises(native.NativeError, match="positive definite"):
            ctx.queue_reset(E, T_EP, **dict(table, cov=-cov))
        empty = native.MpcScenes(0)
        assert L.mpcmmd_mpc_queue_reset(ctx._c, E, T_EP, C.byref(empty), covp) == -1
        assert L.mpcmmd_mpc_queue_run(ctx._c, 2, 0, 1, covp) == -4, "failed resets do not count"
        # an ordinary reset: the ordinary run works, the queue's does not
        ctx.reset(st[:E, :2], vel[:E], c["vehicles"][:E], mean[:E], cov, None, KEYS[:E])
        assert L.mpcmmd_mpc_queue_run(ctx._c, 2, 0, 1, covp) == -4 and b"after mpcmmd_mpc_reset" in L.mpcmmd_last_error()
        ctx.run("cvar", 0, 1, cov, 15.0)
        # a queue reset: the other way round
        ctx.queue_reset(E, T_EP, **table)
        assert L.mpcmmd_mpc_run(ctx._c, 2, 0, 1, covp, vd) == -4 and b"mpcmmd_mpc_queue_reset" in L.mpcmmd_last_error()
        for begin, count in ((0, 7), (-1, 1), (6, 1), (0, -1)):
            assert L.mpcmmd_mpc_queue_run(ctx._c, 2, begin, count, covp) == -1, (begin, count)
        assert L.mpcmmd_mpc_queue_run(ctx._c, 2, 0, 1, None) == -1
        assert L.mpcmmd_mpc_queue_run(ctx._c, 4, 0, 1, covp) == -1, "det is the CARLA optimizer's"
        ctx.queue_run("cvar", 0, 2, cov)
        assert ctx.queue_status() == (5, 2)
        # the policy on: the table must bring its arrays
        ctx.plan_vehicles(np.zeros((1, 2, 2), F32))
        assert L.mpcmmd_mpc_queue_run(ctx._c, 2, 2, 1, covp) == -4, "a stage change needs a new reset"
        with pytest.raises(native.NativeError, match="veh_target"):
            ctx.queue_reset(E, T_EP, **table)
        ctx.plan_vehicles(None)
        # the validation stage on: every queue call is a state error
        ctx.validate(16)
        with pytest.raises(native.NativeError, match="validation stage"):
            ctx.queue_reset(E, T_EP, **table)
        assert L.mpcmmd_mpc_queue_run(ctx._c, 2, 0, 1, covp) == -4
        assert L.mpcmmd_mpc_queue_status(ctx._c, C.byref(ia), C.byref(ib)) == -4
        assert L.mpcmmd_mpc_queue_log(ctx._c, sp) == -4
        ctx.validate(None)
        ctx.queue_reset(E, T_EP, **table)
        ctx.queue_run("cvar", 0, 1, cov)
        assert ctx.queue_status() == (4, 1)
    finally:
        ctx.close()
