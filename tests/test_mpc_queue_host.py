"""The scene queue of the synthetic closed loop without a GPU:
mpcmmd_mpc_queue_host against the NumPy restatement of the rule (tests/mpc_queue_model.py) on every
word of a few hundred random states, the rule's invariants over whole campaigns, the round trip of
cutting a lockstep log by a schedule (optimizer/campaign.py), the argument errors, and the
sanitizer run of the host code (tests/native/asan_mpc_queue.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mpc_queue_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
SLOTS = (1, 3, 64, 65, 200)


def native_mod():
    from optimizer import _native
    return _native


random_state = qm.random_state


def states():
    rng = np.random.default_rng(25)
    for E in SLOTS:
        for N in sorted({max(E - 2, 1), E, E + 1, 2 * E + 3}):
            for pattern in ("mixed", "all", "none", "exhaust"):
                for tpe in (1, 5):
                    for _ in range(2):
                        yield E, N, tpe, pattern, random_state(rng, E, N, tpe, pattern)


def test_symbols():
    n = native_mod()
    for s in ("mpcmmd_mpc_queue_host", "mpcmmd_mpc_queue_device", "mpcmmd_mpc_queue_reset", "mpcmmd_mpc_queue_run",
              "mpcmmd_mpc_queue_status", "mpcmmd_mpc_queue_log"):
        assert s in n.SYMBOLS and hasattr(n.lib(), s), s
    assert n.QUEUE_REASONS == ("unfinished", "collision", "goal", "tick_limit")


def test_host_rule_equals_model():
    """Every word, a few hundred random states: E at the edges of the wave scan, N below, equal to
    and above E, every end pattern, several slots ending on one tick, the table running out in the
    middle of a tick."""
    n = native_mod()
    count = several = ran_out = 0
    for E, N, tpe, pattern, st in states():
        tick = 3 + count % 7
        got = n.mpc_queue(tick, tpe, device=None, **st)
        want = qm.step(tick, tpe, **st)
        for k in qm.WORDS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (E, N, tpe, pattern, k)
        ended = int(want["count"][1] - st["count"][1])
        took = int((want["fresh"] >= 0).sum())
        several += ended > 1
        ran_out += 0 < took < ended
        count += 1
    assert count >= 300 and several > 50 and ran_out > 10, (count, several, ran_out)


@pytest.mark.parametrize("E,N", [(1, 4), (3, 7), (3, 2), (3, 3), (64, 130), (65, 200), (200, 150)])
def test_campaign_invariants(E, N):
    """Whole campaigns through the host rule with random ends: every scene started at most once and
    in index order, slot order kept within a tick, started - finished = live slots, idx_mpc wraps
    like tick_indices, and the schedule's rows tile the (tick, slot) grid without overlap."""
    n = native_mod()
    rng = np.random.default_rng(E * 1000 + N)
    tpe = 4
    keys = rng.integers(-2 ** 31, 2 ** 31, N)
    keys[:2] = (2 ** 31 - 1, -1)
    v_des = rng.uniform(5, 20, N).astype(np.float32)
    w = qm.start(E, keys, v_des)
    order = list(range(min(E, N)))
    t = 0
    while w["count"][1] < N:
        assert t < (N // E + 2) * tpe, "a campaign ends within (ceil(N / E) + 1) ticks_per_episode"
        live = w["scene"] >= 0
        done = np.where(live & (rng.random(E) < 0.25), w["ltick"], w["done"]).astype(np.int32)
        flags = rng.integers(0, 2, (E, 4)).astype(np.int32)
        st = {k: (done if k == "done" else w[k]) for k in qm.STATE}
        w = n.mpc_queue(t, tpe, flags, keys, v_des, device=None, **st)
        took = w["fresh"][w["fresh"] >= 0]
        assert np.array_equal(took, np.arange(len(order), len(order) + took.size)), "index order, slot order"
        order += list(took)
        assert w["count"][0] == len(order) and w["count"][0] - w["count"][1] == int((w["scene"] >= 0).sum())
        want_idx = ((w["ltick"].astype(np.int64) + w["key"].astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(w["idx_mpc"].view(np.uint32), want_idx)
        assert (w["done"][w["scene"] < 0] >= 0).all(), "idle slots are frozen"
        t += 1
    assert order == list(range(N))
    sched = w["sched"]
    grid = np.zeros((t, E), np.int32)
    for slot, first, ticks, reason in sched:
        assert 1 <= ticks <= tpe and reason in (qm.COLLISION, qm.GOAL, qm.TICK_LIMIT)
        grid[first:first + ticks, slot] += 1
    assert grid.max() == 1
    from optimizer.campaign import lockstep_ticks
    assert lockstep_ticks(sched) == t


def test_cut_round_trip():
    """Synthetic lockstep logs whose every row names its (tick, slot): cutting by a schedule
    returns every scene's rows, pads with the last row, and reports the ends."""
    from optimizer import campaign
    E, tpe = 3, 5
    ends = [None, (0, qm.COLLISION), None, (0, qm.GOAL), None, (2, qm.GOAL), None]
    sched, T, finished = qm.schedule(E, tpe, ends)
    assert finished == 7
    tt, ss = np.meshgrid(np.arange(T), np.arange(E), indexing="ij")
    log = dict(log_d=np.stack([tt, ss], -1).astype(np.float64), log_i=(100 * tt + ss)[..., None].astype(np.int32),
               veh=np.stack([tt, ss], -1).astype(np.float32)[:, :, None, :].repeat(2, 2))
    out = campaign.cut(log, sched, tpe)
    for i, (slot, first, ticks, reason) in enumerate(sched):
        for k in log:
            assert out[k].shape == (tpe, 7) + log[k].shape[2:] and out[k].dtype == log[k].dtype
            assert np.array_equal(out[k][:ticks, i], log[k][first:first + ticks, slot]), (i, k)
            assert (out[k][ticks:, i] == log[k][first + ticks - 1, slot]).all(), "padded with the last row"
        assert out["end_tick"][i] == ticks - 1 and out["end_reason"][i] == reason
        assert out["done_tick"][i] == (ticks - 1 if ends[i] is not None else -1)
    # a budget that leaves scenes unfinished or unstarted
    sched, T, finished = qm.schedule(E, tpe, [None] * 7, budget=7)
    assert finished == 3 and T == 7
    out = campaign.cut({k: v[:7] for k, v in log.items()}, sched, tpe)
    assert list(out["end_reason"]) == [3, 3, 3, 0, 0, 0, 0] and list(out["end_tick"]) == [4, 4, 4, 1, 1, 1, -1]
    assert (out["log_d"][:, 6] == 0).all() and campaign.lockstep_ticks(sched) == 7
    with pytest.raises(ValueError):
        campaign.cut({k: v[:6] for k, v in log.items()}, sched, tpe)


def test_main_test_schedule():
    """The schedule tests/test_gpu_mpc_queue.py expects, from the rule: 7 scenes, 3 slots, 5 ticks."""
    ends = [None, (0, qm.COLLISION), None, (0, qm.GOAL), None, None, None]
    sched, T, finished = qm.schedule(3, 5, ends)
    assert T == 10 and finished == 7
    assert sched.tolist() == [[0, 0, 5, 3], [1, 0, 1, 1], [2, 0, 5, 3], [1, 1, 1, 2], [1, 2, 5, 3], [0, 5, 5, 3],
                              [2, 5, 5, 3]]


def test_argument_errors():
    n = native_mod()
    L = n.lib()
    rng = np.random.default_rng(0)
    st = random_state(rng, 3, 4, 5, "mixed")
    n.mpc_queue(0, 5, device=None, **st)
    for bad in (dict(scene=np.array([0, 4, -1])), dict(scene=np.array([-2, 0, 1])), dict(count=np.array([5, 0])),
                dict(count=np.array([-1, 0]))):
        with pytest.raises(n.NativeError):
            n.mpc_queue(0, 5, device=None, **dict(st, **bad))
    with pytest.raises(n.NativeError):
        n.mpc_queue(0, 0, device=None, **st)
    assert L.mpcmmd_mpc_queue_host(None) == -1
    io = n.MpcQueueIO(3, 4, 5, 0)   # every array NULL
    assert L.mpcmmd_mpc_queue_host(C.byref(io)) == -1 and b"null" in L.mpcmmd_last_error()
    # the context's calls check their pointers before anything else
    assert L.mpcmmd_mpc_queue_reset(None, 1, 1, None, None) == -1
    assert L.mpcmmd_mpc_queue_run(None, 2, 0, 1, None) == -1
    assert L.mpcmmd_mpc_queue_status(None, None, None) == -1
    assert L.mpcmmd_mpc_queue_log(None, None) == -1


def test_queue_program_under_sanitizers():
    """`make asan_mpc_queue` builds tests/native/asan_mpc_queue.cpp with the host-only sources under
    ASan / UBSan (-fno-sanitize-recover); its run, a child process with nothing preloaded, must exit
    0 with no sanitizer report, and the schedule it prints must be the NumPy rule's."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", PKG, "asan_mpc_queue"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "asan_mpc_queue")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    ends = [None, (0, qm.COLLISION), None, (0, qm.GOAL), None, None, None]
    sched, T, _ = qm.schedule(3, 5, ends)
    assert lines[0] == f"ticks {T}"
    for i, row in enumerate(sched):
        assert lines[1 + i] == "scene %d %d %d %d %d" % (i, *row), lines[1 + i]


def test_cli_campaign_runner_accounts_every_scene(tmp_path):
    """``closed_loop(run=campaign_runner(E))`` with a stand-in for the GPU: the unchanged accounting
    takes the campaign's per-scene arrays, prints its four figures over N scenes and writes the npz
    with the same keys."""
    from optimizer import campaign, closed_loop as CL
    E, tpe = 3, 5
    ends = [None, (0, qm.COLLISION), None, (0, qm.GOAL), None, None, None]
    sched, T, _ = qm.schedule(E, tpe, ends)

    class Fake:
        def run_campaign(self, cost, vehicles, starts, ticks, slots, **kw):
            assert slots == E and ticks == tpe and kw == dict(keys=None)
            rng = np.random.default_rng(1)
            log = dict(log_d=np.cumsum(rng.random((T, E, 2)), 0), log_f=rng.random((T, E, 12)).astype(np.float32),
                       log_i=np.zeros((T, E, 4), np.int32), cx=np.zeros((T, E, 11), np.float32),
                       cy=np.zeros((T, E, 11), np.float32), mean=np.zeros((T, E, 8), np.float32))
            log["log_i"][0, 1, 1] = 1   # scene 1's collision: slot 1, lockstep tick 0
            return dict(campaign.cut(log, sched, tpe), sched=sched, lockstep_ticks=T, started=7, finished=7)

    lines = []
    res = CL.closed_loop(Fake(), ["cvar"], np.zeros((7, 3, 4)), np.zeros((7, 4)), tpe, str(tmp_path),
                         run=CL.campaign_runner(E, log=lines.append), log=lines.append, keys=None, chained=True,
                         device_step=None)
    out, s = res["cvar"]
    assert "campaign of 7 scenes through 3 slots, 10 lockstep ticks (7 finished; 15 in batches of 3)" in lines[0]
    assert "cvar: 7 episodes x 5 ticks, collision share = 0.1429" in lines[1]
    assert out["done_tick"].tolist() == [-1, 0, -1, 0, -1, -1, -1]
    z = np.load(tmp_path / "closed_loop_cvar.npz")
    assert set(z.files) == set(CL.KEYS) and z["log_d"].shape == (tpe, 7, 2)
    with pytest.raises(ValueError):
        CL.campaign_runner(E)(Fake(), "cvar", None, None, tpe, chained=False)
