"""k_world_step on the GPU (mpcmmd_world_step_device: one launch, a workgroup
per episode) against mpcmmd_world_step_host: every word the step writes -- the
state, the next tick's init_state, waypoints and obstacles, the first
population and the log row -- is bit-equal.  Shapes: num_batch 20, num_obs 2,
total_obs 0 / 1 / 5 / 64, num_path 37 / 64 (ragged against the 256 threads), a
hairpin route of 130 points whose legs are equidistant from the ego (argmin
ties inside one reduction round) and the 21 k-point synthetic route (82 rounds
per thread, then the waves).  The host step itself is held against the NumPy
restatement in test_world_host.py."""
import numpy as np
import pytest

import world_model as wm

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("pos", "ego", "vehicles", "done_tick", "init_state", "x_wp", "y_wp", "obstacles", "pop", "log_d", "log_f",
        "log_i")
CASES = [("hairpin", 0, 37, "gaussian"), ("hairpin", 1, 64, "beta"), ("hairpin", 5, 37, "beta"),
         ("hairpin", 64, 64, "gaussian"), ("synthetic", 5, 37, "gaussian"), ("synthetic", 64, 64, "beta")]
E_RANDOM = 10


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def routes():
    syn, len_path = wm.synthetic_route()
    hp, _ = wm.hairpin_route()
    return dict(synthetic=(syn, len_path - 1), hairpin=(hp, 129))


@pytest.fixture(scope="module")
def pdot4(native):
    cfg = native.make_config(4, 2, 0.1, 8, "gaussian", 0.0, 0.0, num_batch=20, variant="carla_town05", maxiter_cem=3)
    return native.host_constant(cfg, "Pdot").reshape(-1, 11)[:4]


def episodes(w, route_name):
    """E_RANDOM random episodes, then by index from E_RANDOM:
    0  tie      the ego stands still on the hairpin's centre line (elsewhere: on route point 40)
    1  frozen   a random episode that ended at tick 2
    2  nan_veh  vehicle 0 has a NaN x
    3  nan_ego  the ego's x is NaN: every distance is NaN (first-NaN argmin, NaN keys sort by position)
    4  behind   every vehicle 30 m behind the ego: the placeholders 300 m away
    5  one      only vehicle 0 ahead, the rest behind: padded by the last kept vehicle"""
    rng = np.random.default_rng(17)
    E = E_RANDOM + 6
    ins = wm.random_inputs(rng, w, E)
    T = w["total_obs"]
    t = E_RANDOM
    ins["pos"][t] = (11.5, 0.0) if route_name == "hairpin" else (w["route_x"][40], w["route_y"][40])
    ins["ego"][t] = (0.0, 0.0, 0.0)
    for k in ("cx", "cy", "steer", "u"):
        ins[k][t] = 0.0
    ins["done_tick"][t + 1] = 2
    ins["pos"][t + 3, 0] = np.nan
    for e in (t + 4, t + 5):
        v, psi = 5.0, float(ins["ego"][e, 1])
        ins["ego"][e, 0] = v
        back = ins["pos"][e] - 30.0 * np.array([np.cos(psi), np.sin(psi)])
        ins["vehicles"][e, :, 0] = back[0] + 0.01 * np.arange(T)
        ins["vehicles"][e, :, 1] = back[1]
        ins["vehicles"][e, :, 2:4] = 0.0
    if T:
        ins["vehicles"][t + 2, 0, 0] = np.nan
        psi = float(ins["ego"][t + 5, 1])
        ins["vehicles"][t + 5, 0, :2] = ins["pos"][t + 5] + 20.0 * np.array([np.cos(psi), np.sin(psi)])
    return ins


@pytest.mark.parametrize("route,total,P,noise", CASES)
def test_device_step_equals_host_step(native, routes, pdot4, route, total, P, noise):
    r, goal = routes[route]
    w = wm.small_world(r, goal, num_path=P, num_obs=2, total_obs=total, noise=noise, B=20, seed=total + P)
    model = wm.native_model(native, w, pdot4)
    ins = episodes(w, route)
    want = native.world_step(model, 5, device=None, **ins)
    got = native.world_step(model, 5, device=0, **ins)
    for k in KEYS:
        for e in range(got[k].shape[0]):
            assert same(got[k][e], want[k][e]), (k, e, got[k][e], want[k][e])
    t = E_RANDOM
    li = want["log_i"]
    # the cases are what they claim, on the host's answers
    if route == "hairpin":
        assert li[t, 0] == 23, "the first of the two equidistant points"
        x, y, rx, ry = 11.5, 0.0, w["route_x"], w["route_y"]
        d2 = (x - rx) ** 2 + (y - ry) ** 2
        assert np.sum(d2 == d2.min()) == 2
    assert same(want["pos"][t + 1], ins["pos"][t + 1]) and want["done_tick"][t + 1] == 2
    assert li[t + 3, 0] == 0 and np.isnan(want["x_wp"][t + 3]).all()
    far = want["obstacles"][t + 4, :, :2] + want["pos"][t + 4]
    assert np.allclose(far, 300.0, atol=1e-3)
    if total:
        assert np.isnan(want["log_f"][t + 2, 11]) and li[t + 2, 2] == 1, "a NaN clear counts as collided"
        assert not np.isnan(want["obstacles"][t + 2]).any(), "the NaN vehicle is never kept"
        assert same(want["obstacles"][t + 5, 0], want["obstacles"][t + 5, 1]), "padded by the one kept vehicle"
        assert np.hypot(*want["obstacles"][t + 5, 0, :2]) < 25
    assert len({int(i) for i in li[:E_RANDOM, 0]}) >= E_RANDOM // 2
    assert not same(want["pop"][0], want["pop"][1]) and (want["pop"][..., :4] >= 0.1).all()


@pytest.mark.parametrize("noise,total,P", [("gaussian", 5, 37), ("beta", 64, 64)])
def test_drawn_variates_device_equals_host(native, routes, pdot4, noise, total, P):
    """u = None: thread 0 draws the variates from (key, seed, tick) once a_c and s_c are known, as
    the host twin does (world_draw.hpp, one definition).  Every word bit-equal, the logged variates
    included; the zero-control episode takes the Beta sampler's limit rule on both sides."""
    r, goal = routes["hairpin"]
    w = wm.small_world(r, goal, num_path=P, num_obs=2, total_obs=total, noise=noise, B=20, seed=9)
    model = wm.native_model(native, w, pdot4, seed=21)
    ins = episodes(w, "hairpin")
    del ins["u"]
    E = ins["pos"].shape[0]
    keys = 100000 * np.arange(E) + 17
    want = native.world_step(model, 5, u=None, keys=keys, device=None, **ins)
    got = native.world_step(model, 5, u=None, keys=keys, device=0, **ins)
    for k in KEYS:
        for e in range(E):
            assert same(got[k][e], want[k][e]), (k, e, got[k][e], want[k][e])
    u = want["log_f"][:, 7:11]
    assert len({float(x) for x in u[:, 2]}) == E
    if noise == "beta":
        assert ((u[:, :2] >= 0) & (u[:, :2] <= 1)).all() and set(u[E_RANDOM, :2]) <= {0.0, 1.0}
        assert 0 < u[0, 0] < 1


def test_device_argument_errors(native):
    """The checks come before any HIP call; n_episodes 0 and a device that does not exist."""
    import ctypes as C
    hp, _ = wm.hairpin_route()
    cfg = native.make_config(4, 2, 0.1, 8, "gaussian", 0.0, 0.0, num_batch=20, variant="carla_town05", maxiter_cem=3)
    w = wm.small_world(hp, 129)
    model = wm.native_model(native, w, native.host_constant(cfg, "Pdot").reshape(-1, 11)[:4])
    ins = wm.random_inputs(np.random.default_rng(0), w, 1)
    with pytest.raises(native.NativeError):
        native.world_step(model, 0, device=4096, **ins)
    L = native.lib()
    assert L.mpcmmd_world_step_device(C.byref(model.c), 0, 0, 0, C.byref(native.WorldStepIO())) == -1
