"""The generalised joint forces of body wrenches (``pd_pose_op`` PD_POSE_GENERALIZED_FORCE, k_generalized_force_fwd / _vjp of
csrc/pd_pose.hip, dp_model.GeneralizedForce, dp_utils.generalized_force / inverse_dynamics) on a real MI355X (run with -m gpu).

Reference: tests/generalized_force_ref.py, the float64 torch restatement (held to its identities by
tests/test_generalized_force_host.py), given the SAME fp32 rows as the GPU.  Bar (the project's, as tests/test_gpu_joint_wrench.py): the
GPU's error over max |reference| per tensor <= max(4 x the error of the fp32 torch evaluation of the same restatement, 1e-5); the round
trip with the GPU's joint wrench twice that (two fp32 ops chained); the one-step inverse dynamics 4 x the error of the float64 oracle
step rounded to fp32.  Both numbers are printed.

Measured on one MI355X (error over max |reference|; GPU / fp32 torch): see DESIGN.md section 8."""
import functools

import numpy as np
import pytest
import torch

from generalized_force_ref import CASES, EFFORTS, TENSORS, case, force_of, g_out_of, generalized_force, rows13
from gpu_harness import dev, dev_inputs  # noqa: F401
from helpers import INPUT_NAMES, relmax, tight_inputs
from joint_coords_ref import joint_coords, oracle_template
from joint_wrench_ref import joint_wrench, template

pytestmark = pytest.mark.gpu
F64 = torch.float64


def bar(what, gpu, f32, ref, floor=1e-5, factor=1.0):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert np.isfinite(e_gpu) and e_gpu <= factor * max(4 * e_32, floor), "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)


@functools.lru_cache(maxsize=None)
def restated(name, S, shift, efforts, dtype):
    """value and gradients of the restatement on a case, with the standard-normal g_out every test uses: computed once, never written"""
    C = case(name, S, shift)
    return force_of(C, dtype, efforts, g_out_of(C))


@functools.lru_cache(maxsize=None)
def gpu_table(name, efforts):
    from diffphys_amd import hip_backend

    return hip_backend.joint_table(template(name), hip_backend.efforts_mode(efforts), torch.device("cuda:0"))


def launch(C, name, efforts, dev, g_out=None, rows=None):
    """-> (out [S, nqd], g_rows [S, nb, 13] or None) as numpy"""
    from diffphys_amd import hip_backend

    nb, nqd = C["nb"], C["nqd"]
    r = torch.from_numpy(rows13(C) if rows is None else rows).to(dev)
    S = r.shape[0] // nb
    out = hip_backend.generalized_force(gpu_table(name, efforts), nb, r)
    assert out.shape == (S, nqd)
    g = None
    if g_out is not None:
        g = hip_backend.generalized_force_vjp(gpu_table(name, efforts), nb, r, torch.from_numpy(np.ascontiguousarray(g_out, np.float32)).to(dev))
        assert g.shape == (S * nb, 13)
        g = g.cpu().numpy().reshape(S, nb, 13)
    return out.cpu().numpy(), g


@pytest.mark.parametrize("efforts", EFFORTS)
@pytest.mark.parametrize("name,S,shift", CASES)
def test_op_and_vjp_match_the_float64_restatement(name, S, shift, efforts, dev):
    """Value and g_rows of a standard-normal g_out against the float64 restatement and its autograd on the same fp32 rows."""
    C = case(name, S, shift)
    g_out = g_out_of(C)
    out, g = launch(C, name, efforts, dev, g_out)
    r64, r32 = restated(name, S, shift, efforts, F64), restated(name, S, shift, efforts, torch.float32)
    tag = "%s x %d%s %s " % (name, S, " far" if shift else "", efforts)
    mine = dict(out=out, g_body_q=g[..., :7], g_body_f=g[..., 7:])
    for k in TENSORS:
        if name == "free1" and k == "g_body_q":   # one FREE body with its com at its origin: no pose enters, the gradient is 0
            assert np.abs(r64[k]).max() == 0 and np.abs(mine[k]).max() <= 1e-6   # (terms of size 1 that cancel: a few fp32 ulps)
            continue
        assert np.abs(r64[k]).max() > 0, k
        bar(tag + k, mine[k], r32[k], r64[k])
    if name == "mixed25":   # the body that gathers 8 children is in the comparison
        assert (np.asarray(C["tpl"]["joint_parent"]).reshape(-1) == 0).sum() == 8


@pytest.mark.parametrize("efforts", EFFORTS)
def test_a_sets_bits_depend_on_nothing_but_the_set(efforts, dev):
    """The last set of the 41-set launch evaluated alone, and everything a second time: equal bits, value and VJP."""
    name = "laikago"
    C = case(name, 41)
    nb = C["nb"]
    g_out = g_out_of(C)
    out, g = launch(C, name, efforts, dev, g_out)
    again = launch(C, name, efforts, dev, g_out)
    assert np.array_equal(out, again[0]) and np.array_equal(g, again[1])
    for s in (0, 40):
        alone = launch(C, name, efforts, dev, g_out[s: s + 1], rows=rows13(C)[s * nb: (s + 1) * nb])
        assert np.array_equal(alone[0][0], out[s]) and np.array_equal(alone[1][0], g[s]), s


def test_a_table_of_another_nb_gives_zeros(dev):
    """The library cannot validate a device buffer: the kernels check the table's nb against the call's and write zeros -- out in the
    width of THAT table's header, which is the only nqd the call states (no row of the table is read)."""
    from diffphys_amd import hip_backend

    C = case("cmp31", 3)
    wrong = gpu_table("mixed25", "actuator").clone()   # 4 + 32 * 25 floats: shorter than the table of 31 bodies
    _, (nb25, nq25, nqd25) = hip_backend._table_tag(gpu_table("mixed25", "actuator"))
    assert nb25 == 25
    wrong._pd_table = ("joint", (31, nq25, nqd25))   # ... passed off as one
    rows = torch.from_numpy(rows13(C)).to(dev)
    out = hip_backend.generalized_force(wrong, 31, rows)
    g = hip_backend.generalized_force_vjp(wrong, 31, rows, torch.ones(3, nqd25, device=dev))
    assert out.shape == (3, nqd25) and g.shape == (93, 13)
    assert (out == 0).all() and (g == 0).all()


def test_empty_and_graph_capture(dev):
    """n = 0; forward and VJP captured in a HIP graph replay eager's bits on new inputs."""
    from diffphys_amd import hip_backend

    name = "human"
    C = case(name, 3)
    nb, nqd = C["nb"], C["nqd"]
    table = gpu_table(name, "actuator")
    empty = torch.zeros(0, 13, device=dev)
    assert hip_backend.generalized_force(table, nb, empty).shape == (0, nqd)
    assert hip_backend.generalized_force_vjp(table, nb, empty, torch.zeros(0, nqd, device=dev)).shape == (0, 13)
    rows = torch.from_numpy(rows13(C)).to(dev)
    g_out = torch.from_numpy(g_out_of(C)).to(dev)
    run = lambda r, g: (hip_backend.generalized_force(table, nb, r), hip_backend.generalized_force_vjp(table, nb, r, g))
    rbuf, gbuf = rows.clone(), g_out.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(rbuf, gbuf)   # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = run(rbuf, gbuf)
    torch.cuda.current_stream().wait_stream(side)
    fresh = rows * 1.01
    g2 = torch.randn(g_out.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    rbuf.copy_(fresh); gbuf.copy_(g2)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(cap, run(fresh, g2)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("efforts", EFFORTS)
def test_autograd_through_the_public_function(efforts, dev):
    """dp_utils.generalized_force on [2, 2, nb, .] tensors: the value is the op's, .grad of both tensors the VJP call's, bit for bit."""
    from diffphys_amd import dp_utils, sim

    name = "human"
    C = case(name, 4)
    nb, nqd = C["nb"], C["nqd"]
    env = sim.Model.from_template(C["tpl"], 4, dev)
    g_out = g_out_of(C)
    out, g = launch(C, name, efforts, dev, g_out)
    bq = torch.from_numpy(C["bq"].copy()).to(dev).view(2, 2, nb, 7).requires_grad_(True)
    bf = torch.from_numpy(C["bf"].copy()).to(dev).view(2, 2, nb, 6).requires_grad_(True)
    mine = dp_utils.generalized_force(bq, bf, env, efforts=efforts)
    assert mine.shape == (2, 2, nqd)
    (mine * torch.from_numpy(g_out).to(dev).view(2, 2, nqd)).sum().backward()
    assert np.array_equal(mine.detach().cpu().numpy().reshape(4, nqd), out)
    assert np.array_equal(bq.grad.cpu().numpy().reshape(4, nb, 7), g[..., :7]) and np.array_equal(bf.grad.cpu().numpy().reshape(4, nb, 6), g[..., 7:])
    key = ("joint", str(dev), "measured" if efforts == "actuator" else "generalized")
    assert key in env._contact_table   # env_joint_table's cache, reused
    with torch.no_grad():   # nothing to differentiate: forward only
        assert torch.equal(dp_utils.generalized_force(bq, bf, env, efforts=efforts), mine.detach())


def _joint_forces(T, bq, bqd, c):
    """float64 -> [S, nqd]: jf of every REVOLUTE / COMPOUND dof on the measured coordinates (0 in the FREE dofs)"""
    from oracle import ref_torch as rt

    S = bq.shape[0]
    jq, jqd = joint_coords(T, bq, bqd, "measured")
    one = torch.ones(S, 1, dtype=T.dtype)
    jf = torch.zeros(S, T.nqd, dtype=T.dtype)
    for i in range(T.nb):
        qs, qds = T.q_start[i], T.qd_start[i]
        for k in range({rt.JOINT_REVOLUTE: 1, rt.JOINT_COMPOUND: 3}.get(T.joint_type[i], 0)):
            j = qds + k
            jf[:, j] = rt.eval_joint_force(jq[:, qs + k], jqd[:, j], c["target"][:, j], c["ke"][:, j], c["kd"][:, j], c["act"][:, j],
                                           T.limit_lower[j], T.limit_upper[j], T.limit_ke[j], T.limit_kd[j], one)[:, 0]
    return jf


@pytest.mark.parametrize("name,S", [("laikago", 5), ("human", 3)])
def test_round_trip_with_the_gpus_joint_wrench(name, S, dev):
    """Exact FK states: generalized_force(joint_wrench(state, controls)) in actuator mode is -jf on every REVOLUTE / COMPOUND dof, jf
    from the float64 joint_coords restatement of the same fp32 rows, and zero on the root, relative to max |jaf|.  Bar: twice the op's
    (two fp32 ops chained), with the fp32 torch chain as the yardstick."""
    from diffphys_amd import dp_utils, sim
    from joint_wrench_ref import case as jw_case

    C = jw_case(name, S, "exact")
    tpl = C["tpl"]
    env = sim.Model.from_template(tpl, S, dev)
    up = lambda k: torch.from_numpy(np.array(C[k])).to(dev)
    jaf = dp_utils.joint_wrench(up("bq"), up("bqd"), env, up("target"), up("ke"), up("kd"), up("act"))
    out = dp_utils.generalized_force(up("bq"), jaf, env, efforts="actuator").cpu().numpy()

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        t = {k: torch.tensor(np.array(C[k]), dtype=dtype) for k in ("bq", "bqd", "target", "act", "ke", "kd")}
        j = joint_wrench(T, t["bq"], t["bqd"], t["target"], t["act"], t["ke"], t["kd"])
        return j.numpy(), generalized_force(T, t["bq"], j, "actuator").numpy()

    (jaf64, _), (_, out32) = chain(F64), chain(torch.float32)
    T64 = oracle_template(tpl)
    t64 = {k: torch.tensor(np.array(C[k]), dtype=F64) for k in ("bq", "bqd", "target", "act", "ke", "kd")}
    want = -_joint_forces(T64, t64["bq"], t64["bqd"], t64).numpy()
    scale = np.abs(jaf64).max()
    e_gpu, e_32 = np.abs(out - want).max() / scale, np.abs(out32 - want).max() / scale
    print("%s x %d round trip with joint_wrench: GPU %.2e, fp32 torch %.2e of max |jaf| = %.3g" % (name, S, e_gpu, e_32, scale))
    assert np.abs(want).max() > 0 and np.isfinite(out).all()
    assert e_gpu <= 2 * max(4 * e_32, 1e-5)


class _Host:
    """the attributes the ForwardWarp family reads from ``self``"""

    def __init__(self, env, bs, nsteps, frame2step, dt):
        self.env, self.num_envs, self.steps_idx, self.frame2step, self.dt = env, bs, range(nsteps), list(frame2step), dt


class _CpuEnv:
    """what dp_utils.inertial_wrench reads of an env, for its float64 evaluation on the CPU"""

    def __init__(self, tpl):
        self.nb, self._tpl = int(tpl["nb"]), tpl

    def template(self):
        return self._tpl


@pytest.mark.parametrize("name", ["laikago", "cmp20"])
def test_one_step_inverse_dynamics_recovers_the_torques(name, dev):
    """3 envs, ONE resumed step (ForwardWarpState, target_ke = target_kd = 0, random torques and res_f) from FK states:
    inverse_dynamics(state, next state, external = res_f + ground_wrench(state)) gives back -(torques - limit force) on every REVOLUTE /
    COMPOUND dof and ~0 on the root.  Yardstick: the float64 oracle's step, its next twists rounded to fp32, then inverse dynamics in
    float64; margin 4 x (the quotient (v' - v) / dt amplifies the fp32 rounding of the twists).  No clamp was active (asserted)."""
    from diffphys_amd import dp_model, dp_utils, sim
    from generated_robots import rollout_inputs
    from oracle import ref_torch as rt

    tpl = template(name)
    bs, nb, nq, nqd = 3, int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
    inp = tight_inputs(tpl, name, bs, 1, seed=5) if name == "laikago" else rollout_inputs(tpl, bs=bs, T=1, seed=3)
    dt = float(inp["dt"])
    inp["target_ke"], inp["target_kd"] = np.zeros(bs * nqd, np.float32), np.zeros(bs * nqd, np.float32)
    rng = np.random.RandomState(17)
    inp["torques"] = (0.5 * rng.randn(1, bs * nqd)).astype(np.float32)
    inp["res_f"] = (0.5 * rng.randn(1, bs * nb, 6)).astype(np.float32)
    T64 = oracle_template(tpl)
    as64 = lambda k, *shape: torch.tensor(np.asarray(inp[k], np.float64).reshape(*shape))
    bq, bqd = rt.eval_fk(T64, as64("q_init", bs, nq), as64("qd_init", bs, nqd))
    bq32, bqd32 = bq.numpy().astype(np.float32), bqd.numpy().astype(np.float32)   # the FK state every side starts from
    bq, bqd = torch.tensor(bq32, dtype=F64), torch.tensor(bqd32, dtype=F64)
    mass, inertia = as64("body_mass", bs, nb), as64("body_inertia", bs, nb, 3, 3)
    c = dict(target=as64("refs", bs, nqd), act=as64("torques", bs, nqd), ke=torch.zeros(bs, nqd, dtype=F64), kd=torch.zeros(bs, nqd, dtype=F64))
    want = -_joint_forces(T64, bq, bqd, c).numpy()   # -(torques - limit force); 0 on the root
    # the yardstick: the float64 oracle's step, rounded to fp32, float64 inverse dynamics
    _, nxt, grf, _ = rt.simulate_step(T64, bq, bqd, as64("res_f", bs, nb, 6), c["target"], c["act"], c["ke"], c["kd"],
                                      as64("body_inv_mass", bs, nb), inertia, as64("body_inv_inertia", bs, nb, 3, 3), dt)
    assert float(nxt.abs().max()) < 10.0
    nxt32 = torch.tensor(nxt.numpy().astype(np.float32), dtype=F64)
    need = dp_utils.inertial_wrench(bq, bqd, nxt32, dt, mass, inertia, _CpuEnv(tpl)) - grf
    yard = generalized_force(T64, bq, need, "actuator").numpy()
    # the GPU: one resumed step, then the public function
    env = sim.Model.from_template(tpl, bs, dev)
    t = dev_inputs(inp, dev)
    s0q, s0qd = torch.from_numpy(bq32.reshape(bs * nb, 7)).to(dev), torch.from_numpy(bqd32.reshape(bs * nb, 6)).to(dev)
    pos, vel = dp_model.ForwardWarpState.apply(s0q, s0qd, *[t[k] for k in INPUT_NAMES[2:]], _Host(env, bs, 1, [0, 1], dt))
    assert torch.equal(pos[0], s0q) and float(vel[1].abs().max()) < 10.0   # state 0 as given; no +-10 clamp in the step
    q0, qd0, qd1 = pos[0].view(bs, nb, 7), vel[0].view(bs, nb, 6), vel[1].view(bs, nb, 6)
    external = t["res_f"].view(bs, nb, 6) + dp_utils.ground_wrench(q0, qd0, env)
    m, I = t["body_mass"].view(bs, nb), t["body_inertia"].view(bs, nb, 3, 3)
    out = dp_utils.inverse_dynamics(q0, qd0, qd1, dt, m, I, env, external=external, efforts="actuator")
    same = dp_utils.generalized_force(q0, (dp_utils.inertial_wrench(q0, qd0, qd1, dt, m, I, env) - external).contiguous(), env)
    assert torch.equal(out, same)   # inverse_dynamics is that composition
    out = out.cpu().numpy()
    e_gpu, e_yard = relmax(out, want), relmax(yard, want)
    print("%s one-step inverse dynamics: GPU %.2e, float64 oracle step rounded to fp32 %.2e (max |torque| %.3g)" % (
        name, e_gpu, e_yard, np.abs(want).max()))
    assert np.abs(want).max() > 0 and np.isfinite(out).all()
    assert e_gpu <= 4 * e_yard


def test_query_reports_the_joint_efforts(dev):
    """phys_model.query(efforts=True) is generalized_force(sim_poses, env 0's jaf) in actuator mode; off by default."""
    from diffphys_amd import dp_utils
    from test_gpu_workload import _model

    model, _ = _model("mi-pace", "cs")
    model.reinit_envs(4, frames_per_wdw=3)
    noise = (torch.randn(4 * 19, generator=torch.Generator().manual_seed(3)) * 0.01).to(dev)
    model.forward(frame_start=torch.arange(4, device=dev), q_init_noise=noise)
    torch.cuda.synchronize()
    assert "sim_joint_efforts" not in model.query()
    data = model.query(efforts=True)
    nb, nqd = int(model.env.nb), int(model.template["nqd"])
    F = data["sim_poses"].shape[0]
    eff = data["sim_joint_efforts"]
    assert eff.shape == (F, nqd) and np.isfinite(eff).all() and np.abs(eff).max() > 0
    poses = torch.from_numpy(np.ascontiguousarray(data["sim_poses"], dtype=np.float32)).to(dev)
    jaf0 = torch.from_numpy(np.ascontiguousarray(data["jaf"][:, :nb], dtype=np.float32)).to(dev)
    assert np.array_equal(dp_utils.generalized_force(poses, jaf0, model.env, efforts="actuator").cpu().numpy(), eff)
