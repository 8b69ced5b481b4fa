"""The device buffers of a handle: which exist for a configuration and how
many bytes each holds (mpcmmd_buffer_info).  The expected sizes restate the
layouts documented beside `struct Params` (csrc/kernels.hpp) and the padding
functions of csrc/layout.hpp; nothing here is copied from a run.  Every name
is listed, so the "*" total is exact: a buffer the library forgets, adds or
resizes fails the test."""
import pytest

pytestmark = pytest.mark.gpu

# csrc/layout.hpp, csrc/host_constants.hpp
K_NUM, K_NVAR, K_LANE = 100, 11, 198
K_BETA_SAMPLES, K_BETA_ITERS, K_BETA_ELITE = 100, 20, 11
K_ELITE, K_ELITE_COST, K_CNORM_STRIDE = 5, 20, 12
K_RESULT_STRIDE = 11 + 11 + 2 + 1 + 20 + 64
K_GEN_STRIDE, K_BZ_COLS, K_FEAT_STRIDE, K_MOM_STRIDE, K_MAX_SPLIT, K_MAX_PATH = 24, 96, 24, 16, 8, 2048


def pos_pad(M):
    return ((M + 1) + 31) & ~31


def ygen_stride(M):
    return ((M + 1) + 31) & ~31


def dist_stride(M):
    return (M + 255) & ~255


def tri_stride(n):
    return ((n * (n - 1) // 2) + 3) & ~3


def gamma_tab_size(S, H):  # gtab_stride (layout.hpp)
    return 4 * 4 * 4 * S * H


def expected(n, O, H, B, T, G=1, beta=False, carla=False, mmd_ok=True):
    """name -> bytes of every device buffer of such a handle."""
    S, M = n, n * n
    M1, BT, Pp = M + 1, G * B, pos_pad(M)
    e = {}
    # constants
    e["basis"] = 3 * K_NUM * K_NVAR * 4
    e["guess_g"] = 2 * K_NVAR * 4 * 8
    e["proj_m"] = 2 * K_NVAR * K_NVAR * 8
    e["fit"] = K_NVAR * H * 8
    # per configuration
    e["solve_c"] = G * 4 * K_NVAR * 8
    e["obs"] = G * 2 * O * H * 4
    e["st0"] = G * 8 * 4
    e["idx_mpc"] = G * 4
    e["v_des"] = G * 4
    e["roll"] = G * T * 3 * H * S * 4
    e["resample"] = G * T * (B - K_ELITE) * 8 * 4
    # Beta noise (16-byte placeholders without it; no attempt table at all)
    e["bplane"] = BT * 2 * H * S * 4 if beta else 16
    e["bfix"] = BT * H * S * 4 if beta else 16
    e["bfix_n"] = 16
    if beta:
        e["gtab"] = G * gamma_tab_size(S, H) * 8
    if mmd_ok:
        e["beta_z0"] = K_BETA_SAMPLES * M1 * 4
        e["beta_z"] = K_BETA_ITERS * Pp * K_BZ_COLS * 4
        e["feat"] = BT * 22 * M * 4
        e["featr"] = BT * M * K_FEAT_STRIDE * 4
        e["bmom"] = BT * M * K_MOM_STRIDE * 4
        e["bdflag"] = BT * K_BETA_SAMPLES * n
        e["bdcount"] = BT * K_MAX_SPLIT * 4
        e["bdlist"] = BT * K_BETA_SAMPLES * n * 4
        e["bdlcount"] = BT * K_BETA_ITERS * 4
        e["sel0"] = K_BETA_SAMPLES * n * 4
        e["sig0"] = K_BETA_SAMPLES * 4
        e["rp0"] = M1 * 4
        e["rpair0"] = K_BETA_SAMPLES * n * 8
        e["rperm"] = M * 4
        e["bdist"] = BT * M * dist_stride(M) * 4
        e["ctrl_n"] = BT * 2 * n * H * 4
        e["bsel"] = BT * K_BETA_SAMPLES * n * 4
        e["bsig"] = BT * K_BETA_SAMPLES * 4
        e["btop"] = BT * K_BETA_SAMPLES * n * 4
        e["bcost"] = BT * K_BETA_SAMPLES * 4
        e["belite"] = 2 * BT * K_BETA_ELITE * M1 * 4
        e["gen"] = BT * Pp * K_GEN_STRIDE * 8
        e["genm"] = BT * Pp * 8
        e["phib"] = BT * ((M1 + 15) // 16) * 66 * 8
        e["bimin"] = BT * 4
        e["bestsel"] = BT * n * 4
        e["brow"] = BT * K_BETA_SAMPLES * n * 4
        e["bkred"] = BT * K_BETA_SAMPLES * tri_stride(n) * 4
        e["ygen"] = BT * K_BZ_COLS * ygen_stride(M) * 4
    if carla:
        R0 = max(M, S) if mmd_ok else S
        e["proj_m_det"] = 2 * K_NVAR * K_NVAR * 8
        e["obs_full"] = G * 2 * O * K_NUM * 4
        e["path"] = G * 6 * K_MAX_PATH * 4
        e["st0r"] = G * R0 * 8 * 4
        e["kappa_i"] = BT * K_NUM * 4
        e["lane_des"] = BT * 4
        e["rxy"] = BT * S * 2 * H * 4
        e["res_steer"] = G * T * K_NUM * 4
    # carry / state and per-iteration intermediates
    e["pop"] = 2 * BT * 8 * 4
    e["mean"] = G * 8 * 4
    e["cov"] = G * 64 * 4
    e["lam_x"] = BT * K_NVAR * 4
    e["lam_y"] = BT * K_NVAR * 4
    e["s_lane"] = BT * K_LANE * 4
    e["cx"] = BT * K_NVAR * 4
    e["cy"] = BT * K_NVAR * 4
    e["traj"] = 6 * BT * K_NUM * 4
    e["cnorm"] = BT * K_CNORM_STRIDE * 8
    e["res_norm"] = BT * 4
    e["acc"] = BT * K_NUM * 4
    e["steer"] = BT * K_NUM * 4
    e["obs_cost"] = BT * 4
    e["lane_cost"] = BT * 4
    e["beta"] = BT * n * 4
    e["sigma"] = BT * 4
    e["res_beta"] = BT * K_BETA_ITERS * 4
    e["btrace"] = BT * K_BETA_ITERS * 4
    e["dbg"] = 64 * 8
    e["stats"] = 8 * 8
    # outputs
    e["results"] = G * T * K_RESULT_STRIDE * 4
    e["tr_proj"] = G * T * B * 4
    e["tr_obs"] = G * T * K_ELITE_COST * 4
    e["tr_cem"] = G * T * K_ELITE * 4
    return e


MMD_ONLY = ("beta_z0", "beta_z", "feat", "featr", "bmom", "bdflag", "bdcount", "bdlist", "bdlcount", "sel0", "sig0",
            "rp0", "rpair0", "rperm", "bdist", "ctrl_n", "bsel", "bsig", "btop", "bcost", "belite", "gen", "genm",
            "phib", "bimin", "bestsel", "brow", "bkred", "ygen")
CARLA_ONLY = ("proj_m_det", "obs_full", "path", "st0r", "kappa_i", "lane_des", "rxy", "res_steer")
# sized for the G B candidates / the G configurations of a batch handle; one table per handle
PER_CANDIDATE = ("pop", "lam_x", "lam_y", "s_lane", "traj", "acc", "steer", "cnorm", "feat", "featr", "bmom", "bdflag",
                 "bdcount", "ctrl_n", "bsel", "bsig", "ygen", "belite", "gen", "genm", "phib", "bdist", "brow", "bkred",
                 "btop", "bcost")
PER_CONFIG = ("solve_c", "obs", "st0", "idx_mpc", "v_des", "roll", "resample", "mean", "cov", "results", "tr_proj",
              "tr_obs", "tr_cem")
PER_HANDLE = ("basis", "guess_g", "proj_m", "fit", "beta_z0", "beta_z", "sel0", "sig0", "rp0", "rpair0", "rperm")


def _open(native, n, O, H, B, T, G=1, noise="gaussian", variant="static"):
    cfg = native.make_config(n, O, 0.1, H, noise, 0.0, 0.0, num_batch=B, maxiter_cem=T, variant=variant)
    return native.Handle(cfg, max_configs=G)


def _check(native, h, exp, absent):
    try:
        got = {k: h.buffer_bytes(k) for k in exp}
        assert got == exp, {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]}
        for k in absent:
            assert k not in exp
            with pytest.raises(native.NativeError, match="no buffer"):
                h.buffer_bytes(k)
        assert h.buffer_bytes("*") == sum(exp.values())
    finally:
        h.close()


def test_static_gaussian_buffers(native):
    """n=4, O=3, H=10, B=32, T=2: every buffer's bytes; no Beta table, no CARLA buffer, no stamp buffer."""
    exp = expected(4, 3, 10, 32, 2)
    assert exp["bplane"] == exp["bfix"] == exp["bfix_n"] == 16
    _check(native, _open(native, 4, 3, 10, 32, 2), exp, ("gtab", "path", "st0r", "obs_full", "proj_m_det", "dbgw"))


def test_beta_noise_buffers(native):
    """Beta noise: the attempt table, the planes and the fix-up list at their full sizes."""
    exp = expected(4, 3, 10, 32, 2, beta=True)
    assert exp["gtab"] == 64 * 4 * 10 * 8 and exp["bplane"] == 32 * 2 * 10 * 4 * 4 and exp["bfix"] == 32 * 10 * 4 * 4
    _check(native, _open(native, 4, 3, 10, 32, 2, noise="beta"), exp, CARLA_ONLY + ("dbgw",))


def test_batch_handle_buffers(native):
    """max_configs = 3: candidate and per-configuration buffers scale by 3, the per-handle tables do not."""
    one, exp = expected(4, 3, 10, 32, 2), expected(4, 3, 10, 32, 2, G=3)
    for k in PER_CANDIDATE + PER_CONFIG:
        assert exp[k] == 3 * one[k], k
    for k in PER_HANDLE:
        assert exp[k] == one[k], k
    _check(native, _open(native, 4, 3, 10, 32, 2, G=3), exp, ("gtab",) + CARLA_ONLY + ("dbgw",))


def test_carla_buffers(native):
    """A CARLA handle (tests/test_gpu_carla.py's smallest shape): its own buffers, R0 = max(M, S) rows in st0r."""
    n, B, H, O, T = 4, 24, 60, 3, 20
    exp = expected(n, O, H, B, T, carla=True)
    assert exp["st0r"] == max(n * n, n) * 8 * 4
    for k in CARLA_ONLY:
        assert k in exp
    _check(native, _open(native, n, O, H, B, T, variant="carla_town05"), exp, ("gtab", "dbgw"))


def test_no_mmd_opt_buffers(native):
    """n = 65 > 64: mmd_opt is unsupported and none of its buffers exists."""
    exp = expected(65, 3, 10, 32, 2, mmd_ok=False)
    _check(native, _open(native, 65, 3, 10, 32, 2), exp, MMD_ONLY + ("gtab",) + CARLA_ONLY + ("dbgw",))
