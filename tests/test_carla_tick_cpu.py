"""The CARLA tick route without a GPU: mpcmmd_carla_tick_host (the host route
of one tick in one call) against the Helper chain of ``replay.tick_inputs`` bit
for bit, ``replay.tick_raw_inputs``, the argument errors of the tick entry
points that need no device, and the sanitizer run of the host code
(tests/native/carla_tick_host.cpp).  Floats are compared by their bit
patterns, so NaNs compare too."""
import ctypes as C
import importlib
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
CARLA = os.path.join(PKG, "carla")
F32 = np.float32
O = 3
TICK_SYMBOLS = ("mpcmmd_tick_create", "mpcmmd_tick_destroy", "mpcmmd_carla_tick_begin_batch",
                "mpcmmd_carla_tick_solve_batch", "mpcmmd_carla_tick_host")
# (town, tick) of the synthetic recordings, at each num_path
TICKS = (("Town05", 0), ("Town05", 60), ("Town05", 90), ("Town10HD", 30))
NUM_PATH = (4, 5, 37, 600, 1025)


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(CARLA, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def carla_package():
    """The CARLA drop-in package under an alias (the static package is named ``optimizer`` too)."""
    name = "mpcmmd_carla_optimizer"
    if name not in sys.modules:
        d = os.path.join(CARLA, "optimizer")
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"),
                                                      submodule_search_locations=[d])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return name


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


class World:
    def __init__(self):
        self.R = _load("mpcmmd_carla_replay_tick_cpu", "replay.py")
        self.helper = importlib.import_module(carla_package() + ".cem_helper").Helper(num_prime=60)
        self._rec = {}

    def rec(self, town, num_path):
        if (town, num_path) not in self._rec:
            self._rec[(town, num_path)] = self.R.record_synthetic(ticks=91 if town == "Town05" else 31, town=town,
                                                                  num_path=num_path)
        return self._rec[(town, num_path)]


@pytest.fixture(scope="module")
def world():
    return World()


def test_symbols_and_abi():
    from optimizer import _native
    L = _native.lib()
    assert _native.ABI_VERSION == 5 and L.mpcmmd_abi_version() == 5
    for s in TICK_SYMBOLS:
        assert s in _native.SYMBOLS and hasattr(L, s), s


def _check_tick(world, rec, k):
    """tick_host of tick k's raw inputs equals the Helper chain of tick_inputs; returns the tracks."""
    from optimizer import _native
    init, xo, yo, path = world.R.tick_inputs(rec, k, world.helper, O)
    init2, xw, yw, ob = world.R.tick_raw_inputs(rec, k, O)
    assert same_bits(init, init2) and ob.shape == (O, 5) and xw.shape == yw.shape == (int(rec["num_path"]),)
    got_path, gxo, gyo = _native.carla_tick_host(init2, xw, yw, ob, 0.1)
    for key in _native.PATH_KEYS:
        assert same_bits(got_path[key], path[key]), (k, key)
        assert np.isfinite(path[key]).all(), (k, key)
    assert same_bits(gxo, xo) and same_bits(gyo, yo), k
    return gxo, gyo, got_path


@pytest.mark.parametrize("num_path", NUM_PATH)
def test_tick_host_equals_helper_chain(world, num_path):
    """Path and tracks of Town05 ticks 0, 60, 90 and Town10HD tick 30, bit for bit."""
    paths = []
    for town, k in TICKS:
        gxo, gyo, path = _check_tick(world, world.rec(town, num_path), k)
        assert np.isfinite(gxo).all() and np.isfinite(gyo).all()
        paths.append(path)
    assert not same_bits(paths[1]["y_path"], paths[2]["y_path"]), "ticks with equal paths show nothing"


def test_tracks_are_compute_obs_trajectories(world):
    """The track formula pinned against Helper.compute_obs_trajectories on moving obstacles with
    headings: x[o][k] = x_o + vx_o tt[k] in fp32, tt = linspace(0, 15, 100).astype(float32); and psi
    reaches the Frenet velocities (global_to_frenet_obs scales the speed by cos / sin of the heading
    relative to the path)."""
    from optimizer import _native
    rec = world.rec("Town05", 600)
    init, xw, yw, ob = world.R.tick_raw_inputs(rec, 60, O)
    ob = ob.copy()
    ob[:, 2] = F32([3.0, -1.5, 0.25])
    ob[:, 3] = F32([0.5, 2.0, -4.0])
    ob[:, 4] = F32([0.3, -2.0, 1.1])
    path, xo, yo = _native.carla_tick_host(init, xw, yw, ob, 0.1)
    h = world.helper
    xi, yi, vxi, vyi, pi = h.global_to_frenet_obs_vmap(ob[:, 0], ob[:, 1], ob[:, 2], ob[:, 3], ob[:, 4],
                                                       *(path[k] for k in _native.PATH_KEYS))
    wx, wy, _ = h.compute_obs_trajectories(xi, yi, vxi, vyi, pi)
    assert same_bits(xo, wx) and same_bits(yo, wy)
    tt = np.linspace(0, 15, 100).astype(F32)
    assert same_bits(xo[0], (xi[0] + vxi[0] * tt).astype(F32))
    ob0 = ob.copy()
    ob0[:, 4] = 0.0
    _, xo0, _ = _native.carla_tick_host(init, xw, yw, ob0, 0.1)
    assert not same_bits(xo0, xo), "psi reaches vx of a moving obstacle"


def helper_chain(world, xw, yw, ob, threshold=0.1):
    """The host helpers on raw tick inputs, as replay.tick_inputs chains them: (xo, yo, path dict)."""
    h = world.helper
    x_path, y_path = h.custom_path_smoothing(xw, yw, threshold)
    Fxd, Fyd, _, _, arc, kap, _ = h.compute_path_parameters(x_path, y_path)
    xi, yi, vxi, vyi, pi = h.global_to_frenet_obs_vmap(ob[:, 0], ob[:, 1], ob[:, 2], ob[:, 3], ob[:, 4], x_path, y_path,
                                                       arc, Fxd, Fyd, kap)
    xo, yo, _ = h.compute_obs_trajectories(xi, yi, vxi, vyi, pi)
    return xo, yo, dict(x_path=x_path, y_path=y_path, arc_vec=arc, Fx_dot=Fxd, Fy_dot=Fyd, kappa=kap)


def edge_inputs(world):
    """(name, (init, x_wp, y_wp, obstacles)) of Town05 tick 60 with no obstacle kept (every vehicle
    behind the ego, so all three are the placeholders 300 m away) and with a NaN obstacle x (the
    first-NaN closest index)."""
    rec = world.rec("Town05", 600)
    behind = dict(rec)
    ego = rec["ego"][60]
    back = np.array([np.cos(ego[4]), np.sin(ego[4])], np.float64) * -30.0
    behind["obstacles"] = rec["obstacles"].copy()
    behind["obstacles"][60, :, 0] = F32(ego[0] + back[0])
    behind["obstacles"][60, :, 1] = F32(ego[1] + back[1])
    none_kept = world.R.tick_raw_inputs(behind, 60, O)
    assert np.allclose(none_kept[3][:, :2] + ego[:2], 300.0, atol=1e-3), "no vehicle kept: the 300 m placeholders"
    init, xw, yw, ob = world.R.tick_raw_inputs(rec, 60, O)
    ob = ob.copy()
    ob[1, 0] = np.nan
    return (("none_kept", none_kept), ("nan_x", (init, xw, yw, ob)))


def test_edge_ticks(world):
    from optimizer import _native
    for name, (init, xw, yw, ob) in edge_inputs(world):
        xo, yo, path = helper_chain(world, xw, yw, ob)
        got_path, gxo, gyo = _native.carla_tick_host(init, xw, yw, ob, 0.1)
        assert same_bits(gxo, xo) and same_bits(gyo, yo), name
        for key in _native.PATH_KEYS:
            assert same_bits(got_path[key], path[key]), (name, key)
        if name == "nan_x":
            # first NaN: the distance to path point 0 is already NaN, so s = arc_vec[0] and the lateral
            # offset is NaN: y = d + vy tt is NaN at every point
            assert np.isnan(gyo[1]).all() and np.isfinite(gyo[0]).all() and np.isfinite(gyo[2]).all()


def test_argument_errors_need_no_gpu():
    """NULL handle or tick context, num_path 3 and 2049: MPCMMD_E_INVALID before any HIP call."""
    from optimizer import _native
    L = _native.lib()
    E_INVALID = -1
    out = C.c_void_p()
    assert L.mpcmmd_tick_create(None, 600, C.byref(out)) == E_INVALID and L.mpcmmd_last_error()
    assert L.mpcmmd_tick_create(None, 600, None) == E_INVALID
    assert L.mpcmmd_carla_tick_begin_batch(None, 1, 2, None, None, None, None, None) == E_INVALID
    assert L.mpcmmd_carla_tick_solve_batch(None, 1, 2, None, None, None, None, None, None) == E_INVALID
    L.mpcmmd_tick_destroy(None)
    f = lambda n: np.zeros(n, F32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for bad in (3, 2049):
        xw, yw, ob, p6, xo, yo = f(2049), f(2049), f(5), f(6 * 2049), f(100), f(100)
        rc = L.mpcmmd_carla_tick_host(bad, 1, fp(f(6)), fp(xw), fp(yw), fp(ob), 0.1, fp(p6), fp(xo), fp(yo))
        assert rc == E_INVALID and b"num_path" in L.mpcmmd_last_error(), bad
    xw = np.linspace(0, 30, 8).astype(F32)
    rc = L.mpcmmd_carla_tick_host(8, 1, fp(f(6)), fp(xw), fp(f(8)), fp(f(5)), float("nan"), fp(f(48)), fp(f(100)),
                                  fp(f(100)))
    assert rc == E_INVALID and b"threshold" in L.mpcmmd_last_error()
    rc = L.mpcmmd_carla_tick_host(8, 1, fp(f(6)), None, fp(f(8)), fp(f(5)), 0.1, fp(f(48)), fp(f(100)), fp(f(100)))
    assert rc == E_INVALID


def test_tick_host_program_under_sanitizers():
    """`make asan_tick` builds tests/native/carla_tick_host.cpp with the host-only sources under ASan /
    UBSan (-fno-sanitize-recover); its run at num_path 4 and 37, a child process with nothing
    preloaded, must exit 0 with no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", PKG, "asan_tick"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "carla_tick_host")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok"
