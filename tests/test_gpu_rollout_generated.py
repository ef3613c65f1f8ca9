"""The rollout kernels on GENERATED robots (generated_robots.ROLLOUT_ROBOTS: random trees with general axes, rotated joint origins, turned
child frames, FIXED joints mixed in, a body with 8 children, a base jointed to the world, compound joints past their limits), through
hip_backend.DeviceModel and the C ABI alone, 3 envs unless stated, dt = 0.5 ms.  The recipe of scripts/gpu_stress_robots.py on fixed
robots, tightened: tests/test_rollout_generated_host.py shows that no env of these inputs takes or nearly takes a discrete decision
that fp32 arithmetic could take the other way, so EVERY env is compared, and every state of the rollout.

a. forward, step by step, against the float64 C oracle: per tensor relmax <= max(4 y, floor), y the fp32 C oracle's error on the same inputs
   and the floors those of test_gpu_tight.test_short_horizon_tight (FLOOR);
b. gradients against the float64 adjoint of the kernel's own trajectory (helpers.own_trajectory_check), every env;
c. the newer entries -- forward-only, resumed, chained adjoint, absent controls, selective gradients, zero steps -- give the bits of the
   plain launch (torch.equal: these are contracts, no tolerance);
d. launch geometry: full workgroups of four env groups with a partial last group, two env groups per workgroup, run-to-run bits.

Every test prints what it measured; the figures of (a) are recorded in DESIGN.md section 6."""
import functools
import itertools

import numpy as np
import pytest
import torch

from generated_robots import ROLLOUT_ROBOTS, TENSORS, joint_class, oracle_pair, robot, rollout_case, yardstick
from gpu_harness import FWD, dev, dev_inputs, device_model  # noqa: F401
from helpers import INPUT_NAMES, own_trajectory_check, relmax

pytestmark = pytest.mark.gpu

PARAMS = ("target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia")
STEPWISE = ("torques", "res_f", "refs")
BS = 3
# tests/test_gpu_tight.py test_short_horizon_tight: what a kernel whose arithmetic differs from the oracle's (atan2 twist, bare v_rcp / v_sqrt)
# is allowed where the fp32 oracle itself is more exact than that
FLOOR = dict(wp_pos=1e-6, wp_vel=1e-6, grf=1e-5, jaf=1e-5)
# (robot, kernel family, segment width or None for the model's own): every robot; rev12 in the lane-per-body and in the quad-lane family;
# mixed25 and rev12 also at 64 lanes per env
CASES = [(n, 0, None) for n in ROLLOUT_ROBOTS if n != "rev12"] + [("rev12", 1, None), ("rev12", 2, None), ("mixed25", 0, 64), ("rev12", 1, 64)]
ENTRY_CASES = [("mixed25", 0), ("cmp20", 0), ("worldmix9", 0), ("rev12", 1), ("rev12", 2)]
case_id = lambda c: "-".join(str(x) for x in c if x is not None)


def _model(name, family=0, segw=None):
    dm = device_model(robot(name), family, segw)
    assert dm.kernel_family()[1] == (name == "rev12"), "quad-lane eligible: the revolute-only robot of at most 16 bodies"
    return dm


@functools.lru_cache(maxsize=None)
def _forward_reference(name, T):
    """(template, inputs, fp32 oracle, float64 oracle), every state a frame: computed once per (robot, horizon), shared, never written"""
    tpl, inp = rollout_case(name, T, 0, bs=BS, every_state=True)
    return (tpl, inp) + oracle_pair(tpl, inp)


def _bar_a(tag, out, st32, st64):
    """bar (a) on the four output tensors -> list of violations; prints the kernel's error next to the yardstick"""
    y = yardstick(st32, st64)
    bad = []
    for k in TENSORS:
        e = relmax(out[k], st64[k])
        bar = max(4 * y[k], FLOOR[k])
        print("%-22s %-6s kernel %.1e  fp32 oracle %.1e  bar %.1e" % (tag, k, e, y[k], bar))
        if not (np.isfinite(e) and e <= bar):
            bad.append("%s %s: kernel %.2e above max(4 x %.2e, %.0e)" % (tag, k, e, y[k], FLOOR[k]))
    return bad


# ---- a. forward, step by step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_every_state_against_float64(dev, oracle_libs, case, T):
    name, family, segw = case
    tpl, inp, st32, st64 = _forward_reference(name, T)
    dm = _model(name, family, segw)
    t = dev_inputs(inp, dev)
    f2s = inp["frame2step"]
    assert f2s == list(range(T + 1))
    pos, vel, grf, jaf, _ = dm.rollout_forward(BS, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    out = dict(wp_pos=pos.cpu().numpy(), wp_vel=vel.cpu().numpy(), grf=grf.cpu().numpy(), jaf=jaf.cpu().numpy())
    per_env = np.abs(st64["grf"].reshape(T + 1, BS, -1)).max((0, 2))
    assert (per_env > 5.0).all(), "every env touches the ground"
    bad = _bar_a("%s T=%d" % (case_id(case), T), out, st32, st64)
    assert not bad, "\n".join(bad)
    assert np.abs(out["grf"][T]).max() == 0 and np.abs(out["jaf"][T]).max() == 0   # the frame at state T: no force snapshot


# ---- b. gradients ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [8, 20])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradients_on_the_kernels_own_trajectory(dev, oracle_libs, case, T):
    """Every env: worst tensor <= max(1e-3, 4 x the fp32 oracle's adjoint of the same trajectory) -- the bar scripts/gpu_stress_robots.py has
    held random robots to; all gradients finite.  Robots with at most 31 touching candidates per env-step: every candidate the float64
    restatement says touches is in the forward kernel's hit log."""
    name, family, segw = case
    tpl, inp = rollout_case(name, T, 0, bs=BS)
    assert inp["frame2step"] == sorted({0, T // 2, T})
    dm = _model(name, family, segw)
    r = own_trajectory_check(dm, tpl, inp, dev, hitlog_check=False, abs_floor=1e-7)
    lim = np.maximum(1e-3, 4.0 * r["fp32_atan2"])
    print("%-14s T=%-2d own trajectory: worst per env %s  fp32 oracle %s  touching candidates per env-step <= %d" % (
        case_id(case), T, np.array2string(r["worst"], precision=1), np.array2string(r["fp32_atan2"], precision=1), r["touch_counts"].max()))
    assert all(np.isfinite(v).all() for v in r["grads"].values())
    assert r["worst"].shape == (BS,) and (r["worst"] <= lim).all(), (r["worst"], r["fp32_atan2"], {k: v.max() for k, v in r["errs"].items()})
    assert (r["touch_counts"].max(0) > 0).all(), "every env touches the ground"
    if name == "cmp20-limits":
        assert np.abs(r["grads"]["target_ke"]).max() > 0 and np.abs(r["grads"]["refs"]).max() > 0
    if r["touch_counts"].max() <= 31:
        h = own_trajectory_check(dm, tpl, inp, dev, hitlog_check=True, abs_floor=1e-7)
        print("%-14s T=%-2d hit log: %d touches, %d log entries, %d missing, %d overflowed env-steps" % (
            case_id(case), T, h["touches"], h["log_entries"], h["hitlog_missing"], h["hitlog_overflow"]))
        assert h["touches"] > 0 and h["hitlog_missing"] == 0 and h["hitlog_overflow"] == 0
        assert np.array_equal(h["worst"], r["worst"])


# ---- c. every newer entry gives the established bits ----------------------------------------------------------------------------------
T12, SPLIT = 12, 5
F2S = [0, SPLIT, 6, T12]


class _Ctx:
    pass


@functools.lru_cache(maxsize=None)
def _entries(name, family):
    """The plain launch of one entry case -- 12 steps, frames at {0, 5, 6, 12}, forward saving its trajectory, all gradients -- kept on the
    device (clones: nothing a later launch writes) for the tests that compare an entry with it."""
    dev = torch.device("cuda:0")
    c = _Ctx()
    c.tpl, c.inp = rollout_case(name, T12, 0, bs=BS)
    c.dm = _model(name, family)
    c.dt = c.inp["dt"]
    c.t = dev_inputs(c.inp, dev)
    rng = np.random.RandomState(5)
    N = BS * c.dm.nb
    c.ap = torch.from_numpy((rng.randn(len(F2S), N, 7) * 1e-3).astype(np.float32)).to(dev)
    c.av = torch.from_numpy((rng.randn(len(F2S), N, 6) * 1e-3).astype(np.float32)).to(dev)
    c.par = [c.t[k] for k in PARAMS]
    pos, vel, grf, jaf, ws = c.dm.rollout_forward(BS, T12, c.dt, *[c.t[k] for k in FWD], frame2step=F2S)
    g = c.dm.rollout_backward(BS, T12, c.dt, c.t["q_init"], c.t["qd_init"], c.t["torques"], c.t["refs"], *c.par, F2S, ws, c.ap, c.av)
    c.out = [x.clone() for x in (pos, vel, grf, jaf)]
    c.traj = [x.clone() for x in c.dm.saved_trajectory(ws, BS, T12)]
    c.g = {k: v.clone() for k, v in g.items()}
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in c.g.values()) and all(float(c.g[k].abs().max()) > 0 for k in STEPWISE + ("q_init", "qd_init"))
    per_env = c.out[2].view(len(F2S), BS, -1).abs().amax((0, 2))
    assert bool((per_env > 5.0).all()), "every env touches the ground"
    return c


def _backward(c, ws, want=STEPWISE, torques="given"):
    tq = c.t["torques"] if torques == "given" else torques
    return c.dm.rollout_backward(BS, T12, c.dt, c.t["q_init"], c.t["qd_init"], tq, c.t["refs"], *c.par, F2S, ws, c.ap, c.av, want=want)


@pytest.mark.parametrize("name,family", ENTRY_CASES)
def test_forward_only_launch_gives_the_saving_launchs_bits(dev, name, family):
    c = _entries(name, family)
    o = c.dm.rollout_forward(BS, T12, c.dt, *[c.t[k] for k in FWD], frame2step=F2S, save_trajectory=False)
    assert o[4] is None
    for what, a, b in zip(TENSORS, o[:4], c.out):
        assert torch.equal(a, b), (name, family, what)


@pytest.mark.parametrize("name,family", ENTRY_CASES)
def test_resumed_launch_continues_bit_for_bit(dev, name, family):
    """Resumed at state 5 from the rows of that frame (body states: the world-jointed robot takes the same path), saving and forward-only:
    every common frame and the saved trajectory from step 5 on."""
    c = _entries(name, family)
    fs = F2S.index(SPLIT)
    pos, vel = c.out[0], c.out[1]
    f2s_r = [x - SPLIT for x in F2S if x >= SPLIT]
    ctl = [c.t[k][SPLIT:].contiguous() for k in ("torques", "res_f", "refs")]
    for save, st0 in ((True, torch.cat([pos[fs], vel[fs]], dim=1).contiguous()), (False, (pos[fs], vel[fs]))):
        o = c.dm.rollout_forward(BS, T12 - SPLIT, c.dt, None, None, *ctl, *c.par, frame2step=f2s_r, save_trajectory=save, state0=st0)
        assert (o[4] is None) == (not save)
        for what, a, b in zip(TENSORS, o[:4], c.out):
            assert torch.equal(a, b[fs:]), (name, family, save, what)
        if save:
            for what, a, b in zip(("body_q", "body_qd", "body_f", "clamp mask"), c.dm.saved_trajectory(o[4], BS, T12 - SPLIT), c.traj):
                assert torch.equal(a, b[SPLIT:]), (name, family, "saved " + what)


@pytest.mark.parametrize("name,family", ENTRY_CASES)
def test_chained_adjoint_equals_the_single_adjoint(dev, name, family):
    """Frames at {0, 6, 12}, split at state 5 (no frame, as in tests/test_gpu_resume.py): the later segment's adjoint first, its raw state0
    gradient as the seed of the earlier segment's frame at its last state, then the earlier segment.  torques / refs / res_f gradients of
    all 12 steps and the q_init / qd_init gradients equal the single launch's."""
    c = _entries(name, family)
    s, t = SPLIT, c.t
    keep = [0, 2, 3]                              # F2S without the frame at the split
    f1 = [F2S[i] for i in keep]
    ap, av = c.ap[keep].contiguous(), c.av[keep].contiguous()
    _, _, _, _, ws1 = c.dm.rollout_forward(BS, T12, c.dt, *[t[k] for k in FWD], frame2step=f1)
    g1 = c.dm.rollout_backward(BS, T12, c.dt, t["q_init"], t["qd_init"], t["torques"], t["refs"], *c.par, f1, ws1, ap, av)
    g1 = {k: v.clone() for k, v in g1.items()}
    fa = [0, s]                                   # earlier segment: steps [0, 5), frame 0 and the boundary state
    fb = [x - s for x in f1 if x > s]             # later segment: frames 6 and 12
    ctl_a = [t[k][:s].contiguous() for k in ("torques", "res_f", "refs")]
    ctl_b = [t[k][s:].contiguous() for k in ("torques", "res_f", "refs")]
    pa, va, _, _, ws_a = c.dm.rollout_forward(BS, s, c.dt, t["q_init"], t["qd_init"], *ctl_a, *c.par, frame2step=fa)
    ws_a = ws_a.clone()
    assert torch.equal(pa[1], c.out[0][1]) and torch.equal(va[1], c.out[1][1])
    st = (pa[1], va[1])
    _, _, _, _, ws_b = c.dm.rollout_forward(BS, T12 - s, c.dt, None, None, *ctl_b, *c.par, frame2step=fb, state0=st)
    gb = c.dm.rollout_backward(BS, T12 - s, c.dt, None, None, ctl_b[0], ctl_b[2], *c.par, fb, ws_b, ap[1:].contiguous(), av[1:].contiguous(), state0=st)
    assert "q_init" not in gb and gb["state0"].shape == (BS * c.dm.nb, 13)
    carry = gb["state0"]
    ap_a = torch.cat([ap[:1], carry[None, :, :7]]).contiguous()
    av_a = torch.cat([av[:1], carry[None, :, 7:]]).contiguous()
    ga = c.dm.rollout_backward(BS, s, c.dt, t["q_init"], t["qd_init"], ctl_a[0], ctl_a[2], *c.par, fa, ws_a, ap_a, av_a)
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    for k in STEPWISE:
        assert float(g1[k].abs().max()) > 0.0
        assert torch.equal(torch.cat([ga[k], gb[k]]), g1[k]), (name, family, k)
    for k in ("q_init", "qd_init"):
        assert float(g1[k].abs().max()) > 0.0 and torch.equal(ga[k], g1[k]), (name, family, k)


@pytest.mark.parametrize("name,family", ENTRY_CASES)
def test_absent_controls_equal_zero_tensors(dev, name, family):
    """torques=None / res_f=None, one at a time and both, against launches given zero tensors: every output and every gradient."""
    c = _entries(name, family)
    t = c.t
    z = dict(torques=torch.zeros_like(t["torques"]), res_f=torch.zeros_like(t["res_f"]))
    for absent in (("torques",), ("res_f",), ("torques", "res_f")):
        runs = []
        for null in (False, True):
            a = dict(t)
            for k in absent:
                a[k] = None if null else z[k]
            o = c.dm.rollout_forward(BS, T12, c.dt, *[a[k] for k in FWD], frame2step=F2S)
            g = c.dm.rollout_backward(BS, T12, c.dt, a["q_init"], a["qd_init"], a["torques"], a["refs"], *c.par, F2S, o[4], c.ap, c.av)
            runs.append(([x.clone() for x in o[:4]], {k: v.clone() for k, v in g.items()}))
        (o0, g0), (o1, g1) = runs
        assert float(o0[2].abs().max()) > 5.0
        for what, x, y in zip(TENSORS, o0, o1):
            assert torch.equal(x, y), (name, family, absent, what)
        assert sorted(g0) == sorted(g1) == sorted(c.g)
        for k in g0:
            assert bool(torch.isfinite(g0[k]).all()) and torch.equal(g0[k], g1[k]), (name, family, absent, k)


@pytest.mark.parametrize("name,family", ENTRY_CASES)
def test_every_subset_of_want_leaves_the_other_gradients_bits(dev, name, family):
    c = _entries(name, family)
    _, _, _, _, ws = c.dm.rollout_forward(BS, T12, c.dt, *[c.t[k] for k in FWD], frame2step=F2S)
    for n in (1, 2, 3):
        for want in itertools.combinations(STEPWISE, n):
            g = _backward(c, ws, want=want)
            assert sorted(g) == sorted(k for k in c.g if k not in STEPWISE or k in want), (want, sorted(g))
            for k in g:
                assert torch.equal(g[k], c.g[k]), (name, family, want, k)


def _zero_steps(c):
    t = c.t
    none = [t[k][:0] for k in ("torques", "res_f", "refs")]
    p0, v0, _, _, ws0 = c.dm.rollout_forward(BS, 0, c.dt, t["q_init"], t["qd_init"], *none, *c.par, frame2step=[0])
    g = c.dm.rollout_backward(BS, 0, c.dt, t["q_init"], t["qd_init"], none[0], none[2], *c.par, [0], ws0, c.ap[:1].contiguous(), c.av[:1].contiguous())
    return p0, v0, g


@pytest.mark.parametrize("name,family", ENTRY_CASES)
def test_zero_step_rollout_is_state_0_and_its_adjoint_is_finite(dev, name, family):
    """No steps: the frame at state 0 is state 0 of the 12-step launch, bit for bit; the adjoint of the zero-step rollout is finite."""
    c = _entries(name, family)
    p0, v0, g = _zero_steps(c)
    assert torch.equal(p0[0], c.out[0][0]) and torch.equal(v0[0], c.out[1][0])
    assert all(bool(torch.isfinite(v).all()) for v in g.values())
    assert float(g["q_init"].abs().max()) > 0


@pytest.mark.parametrize("name,family", ENTRY_CASES)
def test_zero_step_rollout_equals_pd_fk_forward(dev, name, family):
    """No steps: the frame at state 0 against pd_fk_forward of (q_init, qd_init), torch.equal.  k_fk and the rollout kernels' eval_fk are
    instantiations of one source, fk_joint; left to the compiler they fused other multiply-add pairs and were one ulp apart on every case
    (pose 6.0e-8 .. 1.2e-7, twist 7.5e-8 .. 1.4e-7 of the tensor's max).  fk_joint's arithmetic is pinned (csrc/pd_device.h)."""
    c = _entries(name, family)
    p0, v0, _ = _zero_steps(c)
    bq, bqd = c.dm.fk_forward(c.t["q_init"].view(BS, -1), c.t["qd_init"].view(BS, -1))
    print("%s family %d zero steps against pd_fk_forward: pose relmax %.1e, twist relmax %.1e" % (
        name, family, relmax(p0[0].cpu().numpy(), bq.view(-1, 7).cpu().numpy()), relmax(v0[0].cpu().numpy(), bqd.view(-1, 6).cpu().numpy())))
    assert torch.equal(p0[0], bq.view(-1, 7)) and torch.equal(v0[0], bqd.view(-1, 6))


def test_resumed_launch_of_one_body_whose_com_is_off_every_axis(dev):
    """The smallest case of what the generated robots found: ONE free body whose centre of mass has a non-zero x (a box off the body's
    origin; the shipped robots' coms all have x = 0), tumbling above the ground, 64 envs, 6 steps.  The rollout carries R com from step to step
    and a launch forms it anew for its state 0; the two sites used to fuse the three products in different orders, so a launch resumed
    from a frame's rows left the single launch by an ulp in the first step (pd_math.h rot_com pins the order).  Resumed at every state."""
    from diffphys_amd import hip_backend, sim
    from helpers import build_template

    b = sim.ModelBuilder()
    b.add_articulation()
    body = b.add_body(origin=sim.transform_identity(), parent=-1, joint_type=sim.JOINT_FREE, joint_armature=0.01)
    b.add_shape_box(body, pos=(0.03, -0.02, 0.017), hx=0.05, hy=0.04, hz=0.03, density=1000.0, ke=1e4, kd=0.0, kf=1e2, mu=1.0)
    tpl = build_template(b)
    assert abs(float(np.asarray(tpl["body_com"]).reshape(3)[0])) > 0.01
    bs, T = 64, 6
    rng = np.random.RandomState(0)
    quat = rng.randn(bs, 4)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    q = np.concatenate([rng.uniform(-0.1, 0.1, (bs, 1)), np.full((bs, 1), 0.5), rng.uniform(-0.1, 0.1, (bs, 1)), quat], 1)
    mass = np.tile(np.asarray(tpl["body_mass"], np.float64), bs)
    inertia = np.tile(np.asarray(tpl["body_inertia"], np.float64), (bs, 1, 1))
    inp = dict(q_init=q.reshape(-1), qd_init=rng.randn(bs * 6), torques=np.zeros((T, bs * 6)), res_f=rng.randn(T, bs, 6) * 0.05, refs=np.zeros((T, bs * 6)),
               target_ke=np.zeros(bs * 6), target_kd=np.zeros(bs * 6), body_mass=mass, body_inv_mass=1 / mass, body_inertia=inertia,
               body_inv_inertia=np.linalg.inv(inertia))
    t = dev_inputs(inp, dev)
    dm = hip_backend.DeviceModel(tpl)
    par = [t[k] for k in PARAMS]
    full = list(range(T + 1))
    pos, vel, grf, jaf, _ = dm.rollout_forward(bs, T, 5e-4, *[t[k] for k in FWD], frame2step=full)
    assert float((pos[T] - pos[0]).abs().max()) > 1e-4   # it moves
    for s in range(1, T):
        ctl = [t[k][s:].contiguous() for k in ("torques", "res_f", "refs")]
        o = dm.rollout_forward(bs, T - s, 5e-4, None, None, *ctl, *par, frame2step=full[: T - s + 1], state0=(pos[s], vel[s]))
        for what, a, ref in zip(TENSORS, o[:4], (pos, vel, grf, jaf)):
            assert torch.equal(a, ref[s:]), (s, what)


def test_the_world_jointed_robot_has_no_free_root():
    tpl = robot("worldmix9")
    assert 4 not in set(int(x) for x in tpl["joint_type"]) and int(tpl["joint_parent"][0]) == -1 and joint_class(tpl) == "generic"
    assert int(tpl["nq"]) == int(tpl["nqd"])   # no pose coordinates: q_init holds joint angles alone


# ---- d. launch geometry ---------------------------------------------------------------------------------------------------------------
T8 = 8


def _tile(inp, bs, dev):
    """the inputs of BS envs tiled to bs envs (env i is a copy of env i % BS) on the device, adjoint seeds included"""
    idx = np.arange(bs) % BS
    t = {}
    for k in INPUT_NAMES + ("adj_pos", "adj_vel"):
        a = np.asarray(inp[k], np.float32)
        lead = a.shape[:1] if k in ("torques", "res_f", "refs", "adj_pos", "adj_vel") else ()
        a = a.reshape(lead + (BS, -1))[..., idx, :]
        t[k] = torch.from_numpy(np.ascontiguousarray(a.reshape(lead + (-1,)))).to(dev)
    return t


def _launch(dm, t, bs, inp):
    f2s, dt = inp["frame2step"], inp["dt"]
    o = dm.rollout_forward(bs, T8, dt, *[t[k] for k in FWD], frame2step=f2s)
    g = dm.rollout_backward(bs, T8, dt, t["q_init"], t["qd_init"], t["torques"], t["refs"], *[t[k] for k in PARAMS], f2s, o[4], t["adj_pos"], t["adj_vel"])
    info = (dm.last_launch_info(0), dm.last_launch_info(1))
    res = dict(zip(TENSORS, (x.clone() for x in o[:4])))
    res.update({"g_" + k: v.clone() for k, v in g.items()})
    return res, info


def _by_env(x, bs, key):
    """[..., bs*n, ...] -> [lead, bs, -1]"""
    lead = x.shape[0] if key in TENSORS or key in ("g_torques", "g_res_f", "g_refs") else 1
    return x.reshape(lead, bs, -1)


def _roles(info, epw):
    """waves per env group of a launch: what tells its kernel variant (split forward 2, or 3 with the cull wave; unsplit forward 1)"""
    groups = info["envs_per_wg"] // epw
    return info["threads_per_wg"] // (64 * groups)


@pytest.mark.parametrize("name,family", [("mixed25", 0), ("cmp20", 0), ("rev12", 1)])
def test_launch_geometry_keeps_every_envs_bits(dev, oracle_libs, name, family):
    """The 3 envs tiled into 4 x CUs x (64 / segw) + 5 envs (full workgroups of four env groups and a partial last group) and into a batch
    that gives two env groups per workgroup: all copies of an env agree bit for bit, outputs and gradients; two runs of every launch are
    the same bits; where a launch ran the kernel variant of the 3-env launch its bits are that launch's, where it did not (the
    compound-only robot: split forward up to 4 x CUs env groups, unsplit beyond) it meets bar (a) against the float64 oracle."""
    tpl, inp = rollout_case(name, T8, 0, bs=BS)
    dm = _model(name, family)
    cus = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    epw = 64 // dm.segment_width()
    small, info_s = _launch(dm, _tile(inp, BS, dev), BS, inp)
    again, _ = _launch(dm, _tile(inp, BS, dev), BS, inp)
    assert all(torch.equal(small[k], again[k]) for k in small)
    assert all(bool(torch.isfinite(v).all()) for v in small.values())
    st32 = st64 = None
    for tag, bs, groups in (("four groups", 4 * cus * epw + 5, 4), ("two groups", (2 * cus - 1) * epw - (epw > 1), 2)):
        t = _tile(inp, bs, dev)
        big, info = _launch(dm, t, bs, inp)
        rerun, _ = _launch(dm, t, bs, inp)
        n_groups = -(-bs // epw)
        assert bs % epw != 0 or epw == 1, "a partial last env group"
        for kind in (0, 1):
            assert info[kind]["envs_per_wg"] == groups * epw and info[kind]["workgroups"] == -(-n_groups // groups), (tag, kind, info[kind])
        print("%s %s: %d envs, forward %s, adjoint %s" % (name, tag, bs, info[0], info[1]))
        idx = torch.arange(bs, device=dev) % BS
        for k, v in big.items():
            assert torch.equal(v, rerun[k]), (name, tag, k, "run to run")
            e = _by_env(v, bs, k)
            assert torch.equal(e, e[:, idx]), (name, tag, k, "copies of an env")
        same = [_roles(info[kind], epw) == _roles(info_s[kind], epw) for kind in (0, 1)]
        assert same[1], "one adjoint variant per joint class"
        if name == "cmp20":
            assert same[0] == (groups == 2) and _roles(info[0], epw) == (2 if groups == 2 else 1), "the unsplit forward beyond 4 x CUs env groups"
        else:
            assert same[0]
        agree = [k for k, v in big.items() if torch.equal(_by_env(v, bs, k)[:, :BS], _by_env(small[k], BS, k))]
        print("%s %s: %d of %d tensors are the bits of the 3-env launch" % (name, tag, len(agree), len(big)))
        if same[0]:
            assert len(agree) == len(big), (name, tag, sorted(set(big) - set(agree)), "against the 3-env launch")
        else:
            if st64 is None:
                st32, st64 = oracle_pair(tpl, inp)
            out = {k: _by_env(big[k], bs, k)[:, :BS].reshape(len(inp["frame2step"]), -1).cpu().numpy().reshape(st64[k].shape) for k in TENSORS}
            bad = _bar_a("%s %s" % (name, tag), out, st32, st64)
            assert not bad, "\n".join(bad)
            assert all(bool(torch.isfinite(v).all()) for v in big.values())
