"""NumPy restatement of the scene queue's rule (csrc/mpc_queue.hpp), written
from the rule's text: the reference of mpcmmd_mpc_queue_host and, through it, of k_mpc_queue.

Slot e carries scene[e] (-1: idle) and ltick[e].  After the step of a lockstep tick its episode
has ended if done[e] >= 0 or ltick[e] == ticks_per_episode - 1.  Ended slots are served in
ascending slot order; each takes the next unstarted scene or becomes idle."""
import numpy as np

UNFINISHED, COLLISION, GOAL, TICK_LIMIT = range(4)
STATE = ("scene", "ltick", "done", "key", "slot_v_des", "sched", "count")
WORDS = STATE + ("fresh", "idx_mpc")


def step(tick, ticks_per_episode, flags, keys, v_des, scene, ltick, done, key, slot_v_des, sched, count):
    """One lockstep tick.  Returns the dict of WORDS after it; nothing given is modified."""
    flags = np.asarray(flags).reshape(-1, 4)
    E, N = flags.shape[0], len(keys)
    o = dict(scene=np.array(scene, np.int32), ltick=np.array(ltick, np.int32), done=np.array(done, np.int32),
             key=np.array(key, np.uint32), slot_v_des=np.array(slot_v_des, np.float32),
             sched=np.array(sched, np.int32).reshape(N, 4), count=np.array(count, np.int32),
             fresh=np.full(E, -1, np.int32), idx_mpc=np.zeros(E, np.int32))
    nxt = int(o["count"][0])
    ended = 0
    for e in range(E):
        sc, lt, dn = int(o["scene"][e]), int(o["ltick"][e]), int(o["done"][e])
        if sc >= 0 and (dn >= 0 or lt >= ticks_per_episode - 1):
            ended += 1
            o["sched"][sc, 2] = lt + 1
            o["sched"][sc, 3] = TICK_LIMIT if dn < 0 else (COLLISION if flags[e, 1] else GOAL)
            if nxt < N:
                o["sched"][nxt] = (e, tick + 1, 0, UNFINISHED)
                o["scene"][e], o["ltick"][e], o["done"][e], o["fresh"][e] = nxt, 0, -1, nxt
                o["key"][e] = np.uint32(int(keys[nxt]) & 0xFFFFFFFF)
                o["slot_v_des"][e] = np.float32(v_des[nxt])
                nxt += 1
            else:
                o["scene"][e] = -1
                if dn < 0:
                    o["done"][e] = lt   # idle slots are frozen
        elif sc >= 0:
            o["ltick"][e] = lt + 1
            o["sched"][sc, 2] = lt + 1
        o["idx_mpc"][e] = np.array([(int(o["ltick"][e]) + int(o["key"][e])) & 0xFFFFFFFF], np.uint32).view(np.int32)[0]
    o["count"][:] = (nxt, int(o["count"][1]) + ended)
    return o


def start(E, keys, v_des):
    """The words after a queue reset: scenes 0..min(N, E)-1 in their slots, the other slots idle and
    frozen on scene 0's key."""
    N = len(keys)
    k = min(E, N)
    sched = np.zeros((N, 4), np.int32)
    sched[:, :2] = -1
    sched[:k, 0], sched[:k, 1] = np.arange(k), 0
    src = np.where(np.arange(E) < k, np.arange(E), 0)
    return dict(scene=np.where(np.arange(E) < k, np.arange(E), -1).astype(np.int32), ltick=np.zeros(E, np.int32),
                done=np.where(np.arange(E) < k, -1, 0).astype(np.int32),
                key=(np.asarray(keys, np.int64)[src] & 0xFFFFFFFF).astype(np.uint32),
                slot_v_des=np.asarray(v_des, np.float32)[src], sched=sched, count=np.array([k, 0], np.int32))


def schedule(E, ticks_per_episode, ends, budget=None):
    """The schedule of a campaign whose scene i, run alone, ends at local tick ends[i][0] for reason
    ends[i][1] (COLLISION or GOAL), or runs all its ticks (ends[i] None).  Returns (sched, lockstep
    ticks used, finished) after ``budget`` lockstep ticks (None: until every scene has finished)."""
    N = len(ends)
    w = start(E, np.zeros(N, np.int64), np.zeros(N, np.float32))
    t = 0
    while w["count"][1] < N and (budget is None or t < budget):
        flags = np.zeros((E, 4), np.int32)
        done = w["done"].copy()
        for e in range(E):
            sc = int(w["scene"][e])
            if sc >= 0 and ends[sc] is not None and ends[sc][0] == w["ltick"][e] and done[e] < 0:
                done[e] = w["ltick"][e]
                flags[e, 1 if ends[sc][1] == COLLISION else 2] = 1
        w = step(t, ticks_per_episode, flags, np.zeros(N, np.int64), np.zeros(N, np.float32),
                 **{k: (done if k == "done" else w[k]) for k in STATE})
        t += 1
    return w["sched"], t, int(w["count"][1])


def random_state(rng, E, N, tpe, pattern):
    """A state the queue can be in before a tick: distinct started scenes in some slots, the others
    idle.  pattern: "mixed", "all" (every live slot ends), "none", "exhaust" (several slots end with
    fewer scenes left than ended slots)."""
    live_max = min(E, N)
    n_live = live_max if pattern in ("all", "exhaust") else int(rng.integers(0, live_max + 1))
    started = int(rng.integers(n_live, N + 1))
    if pattern == "exhaust":
        started = max(n_live, N - int(rng.integers(0, max(n_live, 1))))   # fewer left than will end
    scene = np.full(E, -1, np.int32)
    slots = rng.permutation(E)[:n_live]
    scene[slots] = rng.permutation(started)[:n_live]
    ltick = rng.integers(0, tpe, E).astype(np.int32)
    done = np.full(E, -1, np.int32)
    if pattern in ("all", "exhaust"):
        how = rng.integers(0, 2, E).astype(bool)
        done[how] = ltick[how]
        ltick[~how] = tpe - 1
    elif pattern == "none":
        ltick = np.minimum(ltick, max(tpe - 2, 0)).astype(np.int32)
        if tpe == 1:
            scene[:] = -1
    else:
        hit = rng.random(E) < 0.3
        done[hit] = ltick[hit]
    done[scene < 0] = rng.integers(0, tpe, int((scene < 0).sum()))   # idle slots are frozen
    flags = rng.integers(0, 2, (E, 4)).astype(np.int32)
    keys = rng.integers(-2 ** 31, 2 ** 31, N)
    keys[rng.random(N) < 0.2] = 2 ** 31 - 1 - rng.integers(0, 3)   # idx_mpc wraps
    return dict(flags=flags, keys=keys, v_des=rng.uniform(5, 20, N).astype(np.float32), scene=scene, ltick=ltick,
                done=done, key=rng.integers(0, 2 ** 32, E).astype(np.uint32),
                slot_v_des=rng.uniform(5, 20, E).astype(np.float32),
                sched=rng.integers(-1, 50, (N, 4)).astype(np.int32),
                count=np.array([started, int(rng.integers(0, started + 1))], np.int32))
