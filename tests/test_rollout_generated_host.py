"""The generated robots of the rollout tests (generated_robots.ROLLOUT_ROBOTS) and their inputs, judged by the two C oracles alone, without
a GPU: that they are what the table says they are (joint mix, size, fan-out, the kernel instantiation they take), that every env loads
its contacts and joints, that no env takes or nearly takes a discrete decision the fp32 arithmetic could take the other way -- the
condition under which tests/test_gpu_rollout_generated.py compares EVERY env with float64 -- and that the fp32 oracle's own error against
float64, the yardstick of that comparison, is where a CPU trial found it."""
import numpy as np
import pytest

from generated_robots import ROLLOUT_LIMITS, ROLLOUT_ROBOTS, TENSORS, joint_class, oracle_pair, robot, rollout_case, yardstick
from helpers import first_branch_difference

BS, SEEDS, HORIZONS = 3, (0, 1, 2), (1, 8)
# name -> (joint types of sim.JOINT_* present, nb, largest child count, kernel instantiation)
EXPECT = {
    "mixed25": ({1, 3, 4, 5}, 25, 8, "generic"),
    "cmp31": ({4, 5}, 31, 4, "generic"),          # compound joints alone: generic through the turned child frames
    "rev64": ({1, 4}, 64, 1, "revolute"),
    "free1": ({4}, 1, 0, "generic"),              # no joint at all is no single joint type
    "rev12": ({1, 4}, 12, 3, "revolute"),
    "mixed48": ({1, 3, 4, 5}, 48, 5, "generic"),
    "cmp20": ({4, 5}, 20, 4, "compound"),
    "worldmix9": ({1, 3, 5}, 9, 3, "generic"),    # no FREE joint: the base hangs on the world by a FIXED joint
    "cmp20-limits": ({4, 5}, 20, 4, "compound"),
}
# The fp32 oracle's error against float64 over these robots in a CPU trial (rollout_inputs(bs=3, seed=0), T = 8 and 20), per tensor (low, high).
# The yardstick must stay below 4 x high at every horizon, and above low / 4 at T = 8 (a one-step rollout of the one-body robot is below
# the trial's range: 1.6e-7 in wp_vel): an fp32 oracle that has become more exact than fp32 arithmetic is as wrong as one that got worse.
TRIAL = {"wp_pos": (4e-8, 8e-6), "wp_vel": (2e-6, 4e-4), "grf": (1e-6, 3e-4), "jaf": (0.0, 8e-4)}
Y = {}   # [T][robot][tensor], printed by the last test


def test_the_table_is_complete():
    assert set(EXPECT) == set(ROLLOUT_ROBOTS) and set(ROLLOUT_LIMITS) <= set(ROLLOUT_ROBOTS)


@pytest.mark.parametrize("name", list(ROLLOUT_ROBOTS))
def test_robot_is_what_the_table_says(name):
    types, nb, kids, cls = EXPECT[name]
    tpl = robot(name)
    ty, par = np.asarray(tpl["joint_type"]).reshape(-1), np.asarray(tpl["joint_parent"]).reshape(-1)
    assert set(int(t) for t in ty) == types and int(tpl["nb"]) == nb <= 64
    assert (np.bincount(par[par >= 0], minlength=nb).max() if nb > 1 else 0) == kids <= 8
    assert joint_class(tpl) == cls
    if name == "worldmix9":
        assert 4 not in types and par[0] == -1 and (par[1:] >= 0).all()
    dofs = slice(6 if 4 in types else 0, None)   # (a FREE root's six dofs carry the builder's default limit gains, which nothing reads)
    lim_ke, lim_kd = np.asarray(tpl["joint_limit_ke"])[dofs], np.asarray(tpl["joint_limit_kd"])[dofs]
    if name in ROLLOUT_LIMITS:
        assert (lim_ke == 40.0).all() and (lim_kd == 1.0).all() and lim_ke.size > 0
        for env, body, angle in ROLLOUT_LIMITS[name]:
            lo, hi = float(np.asarray(tpl["joint_limit_lower"])[tpl["joint_qd_start"][body]]), float(np.asarray(tpl["joint_limit_upper"])[tpl["joint_qd_start"][body]])
            assert (lo, hi) == (-1.5, 1.5) and angle > 1.5
    else:
        assert (lim_ke == 0.0).all() and (lim_kd == 0.0).all()


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name", list(ROLLOUT_ROBOTS))
def test_inputs_are_fit_to_judge_a_kernel(name, T, oracle_libs):
    """Seeds 0 .. 2, every state a frame.  |grf| > 5 N in every env and |jaf| > 0 in every env of a robot with a joint; no env has a
    decision difference or a near-tie between the fp32 and the float64 oracle before step T (helpers.first_branch_difference, its own
    tolerances); the yardstick -- the largest fp32 error over the three seeds -- is within the trial's range (TRIAL)."""
    from oracle.ref_c import RefC

    y = {k: 0.0 for k in TENSORS}
    for seed in SEEDS:
        tpl, inp = rollout_case(name, T, seed, bs=BS, every_state=True)
        nb = int(tpl["nb"])
        st32, st64 = oracle_pair(tpl, inp)
        per_env = lambda a: np.abs(np.asarray(a).reshape(T + 1, BS, -1)).max((0, 2))
        assert (per_env(st64["grf"]) > 5.0).all(), (name, seed, per_env(st64["grf"]))
        if nb > 1:
            assert (per_env(st64["jaf"]) > 0.0).all(), (name, seed, per_env(st64["jaf"]))
        assert all(np.isfinite(st32[k]).all() and np.isfinite(st64[k]).all() for k in TENSORS)
        rc32, rc64 = RefC(tpl, np.float32), RefC(tpl, np.float64)
        traj = dict(states_q=st32["states_q"], states_qd=st32["states_qd"], states_f=st32["states_f"], clamp=rc32.branch_log(st32)["clamp"])
        first = first_branch_difference(rc64, st64, traj, inp, BS)
        assert (first == T).all(), "%s seed %d T %d: a decision differs or nearly ties at step %s" % (name, seed, T, first)
        for k, v in yardstick(st32, st64).items():
            y[k] = max(y[k], v)
    Y.setdefault(T, {})[name] = y
    for k, (low, high) in TRIAL.items():
        assert y[k] <= 4 * high, (name, T, k, y[k])
        if T == 8 and (k != "jaf" or nb > 1):
            assert y[k] >= low / 4, (name, T, k, y[k])


def test_the_limit_case_has_a_limit_force(oracle_libs):
    """cmp20-limits against the same robot without limit gains, float64, one step: the env that starts beyond its limit gets another
    joint wrench and another twist, the two envs inside their limits the same bits."""
    from oracle.ref_c import RefC

    tpl, inp = rollout_case("cmp20-limits", 1, 0, bs=BS, every_state=True)
    (env, body, angle), = ROLLOUT_LIMITS["cmp20-limits"]
    nq = int(tpl["nq"])
    assert abs(float(inp["q_init"].reshape(BS, nq)[env, tpl["joint_q_start"][body]]) - angle) < 1e-6
    assert (np.abs(np.delete(inp["q_init"].reshape(BS, nq)[:, 7:], [env], axis=0)).max() <= 0.3 + 1e-6)
    off = dict(tpl)
    off["joint_limit_ke"], off["joint_limit_kd"] = np.zeros_like(tpl["joint_limit_ke"]), np.zeros_like(tpl["joint_limit_kd"])
    a, b = (RefC(t, np.float64).rollout_forward(inp, 1, inp["frame2step"], inp["dt"]) for t in (tpl, off))
    e = lambda x: np.asarray(x).reshape(2, BS, int(tpl["nb"]), -1)
    d_jaf, d_vel = np.abs(e(a["jaf"]) - e(b["jaf"])).max((0, 2, 3)), np.abs(e(a["wp_vel"]) - e(b["wp_vel"])).max((0, 2, 3))
    others = [i for i in range(BS) if i != env]
    # 40 N m / rad on 0.12 rad past the limit: ~5 N m
    assert d_jaf[env] > 1.0 and d_vel[env] > 0.0 and (d_jaf[others] == 0).all() and (d_vel[others] == 0).all(), (d_jaf, d_vel)


def test_print_the_yardsticks():
    for T in sorted(Y):
        for name, y in Y[T].items():
            print("yardstick T=%d %-13s %s" % (T, name, "  ".join("%s %.1e" % (k, y[k]) for k in TENSORS)))
