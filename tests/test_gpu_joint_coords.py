"""Joint coordinates from body states (``pd_pose_op`` PD_POSE_JOINT_COORDS, dp_model.InverseKinematics, dp_utils.joint_coords): the
inverse of ForwardKinematics, on a real MI355X (run with -m gpu).

Reference: tests/joint_coords_ref.py, the float64 torch restatement built from oracle/ref_torch.py's quaternion functions (held to eval_fk
and to eval_body_joints' own numbers by tests/test_joint_coords_host.py), given the SAME fp32 states as the GPU.  Bar (the project's, as
tests/test_gpu_ground_wrench.py): the GPU's error over max |reference| per tensor <= max(4 x the error of the fp32 torch evaluation of
the same restatement, 1e-5); the rollout-through gradients additionally stay under that file's caps.  Both numbers are printed.

Measured on one MI355X (error over max |reference|; GPU / fp32 torch): see DESIGN.md section 8."""
import functools

import numpy as np
import pytest
import torch

from gpu_harness import dev, dev_inputs  # noqa: F401
from helpers import INPUT_NAMES, relmax, tight_inputs
from joint_coords_ref import coords_of, fk_states, joint_coords, load_tpl, oracle_template, random_coords, tangent

pytestmark = pytest.mark.gpu

RATES = ["generalized", "measured"]
# (template, state sets): 41 Laikago sets are 533 elements -- sets straddle the forward kernel's workgroups and fill three of the VJP's
VALUE_CASES = [("laikago", 5), ("human", 3), ("laikago_toes", 2), ("laikago", 41), ("laikago", 1)]
VJP_CASES = [("laikago", 5), ("laikago", 41), ("human", 3), ("laikago_toes", 2)]


def bar(what, gpu, f32, ref, floor=1e-5):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert np.isfinite(e_gpu) and e_gpu <= max(4 * e_32, floor), "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)
    return max(4 * e_32, floor)


@functools.lru_cache(maxsize=None)
def fk_case(name, S, lo=0.0):
    """eval_fk (float64, rounded to fp32) of random coordinates: root quaternions random unit, angles uniform with lo <= |q| <= 1; with
    lo = 0 and more than two sets, set 0 sits at the reference pose (all joint angles exactly 0).  Shared by the tests, never written."""
    tpl = load_tpl(name)
    q, qd = random_coords(tpl, S, seed=100 + S, lo=lo, hi=1.0, zero_sets=1 if (lo == 0.0 and S > 2) else 0)
    bq, bqd = fk_states(tpl, q, qd)
    for a in (q, qd, bq, bqd):
        a.setflags(write=False)
    return dict(tpl=tpl, nb=int(tpl["nb"]), q=q, qd=qd, bq=bq, bqd=bqd)


@functools.lru_cache(maxsize=None)
def restated(name, S, lo, rates, dtype):
    C = fk_case(name, S, lo)
    return coords_of(C["tpl"], dtype, C["bq"], C["bqd"], rates)


def gpu_state(C, dev):
    return torch.from_numpy(np.concatenate([C["bq"], C["bqd"]], -1).reshape(-1, 13)).to(dev)


@functools.lru_cache(maxsize=None)
def gpu_table(name, rates):
    from diffphys_amd import hip_backend

    return hip_backend.joint_table(load_tpl(name), rates, torch.device("cuda:0"))


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S", VALUE_CASES)
def test_values_match_the_float64_restatement(name, S, rates, dev):
    from diffphys_amd import hip_backend

    C = fk_case(name, S)
    jq, jqd = hip_backend.joint_coords(gpu_table(name, rates), C["nb"], gpu_state(C, dev))
    assert jq.shape == (S, int(C["tpl"]["nq"])) and jqd.shape == (S, int(C["tpl"]["nqd"]))
    r64, r32 = restated(name, S, 0.0, rates, torch.float64), restated(name, S, 0.0, rates, torch.float32)
    tag = "%s x %d %s " % (name, S, rates)
    b_q = bar(tag + "joint_q", jq.cpu().numpy(), r32[0], r64[0])
    bar(tag + "joint_qd", jqd.cpu().numpy(), r32[1], r64[1])
    if rates == "generalized":   # printed, not asserted: the inverse property is the round-trip test's business
        print(tag + "against the coordinates eval_fk was given: q %.2e, qd %.2e" % (relmax(jq.cpu().numpy(), C["q"]),
                                                                                  relmax(jqd.cpu().numpy(), C["qd"])))
    if S > 2:   # set 0: the reference pose -- every joint angle exactly 0
        ang = jq[0, 7:].cpu().numpy()
        assert (C["q"][0, 7:] == 0).all() and np.isfinite(ang).all() and np.isfinite(jqd[0].cpu().numpy()).all()
        print(tag + "reference pose: max |angle| %.2e" % np.abs(ang).max())
        assert np.abs(ang).max() <= b_q * np.abs(r64[0]).max()


class _Host:
    """the attributes the ForwardWarp family reads from ``self``"""

    def __init__(self, env, bs, nsteps, frame2step, dt):
        self.env, self.num_envs, self.steps_idx, self.frame2step, self.dt = env, bs, range(nsteps), list(frame2step), dt


@pytest.mark.parametrize("name", ["laikago", "human"])
def test_simulated_states(name, dev):
    """Frames of a rollout that starts 4 mm in the ground: the joints are slightly violated there (x_err != 0, swing != 0), which
    eval_fk-made states never are."""
    from diffphys_amd import dp_model, sim, synth

    tpl = load_tpl(name)
    bs, T, f2s = 8, 24, [0, 8, 16, 24]
    nb = int(tpl["nb"])
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=2, penetration=0.004)
    env = sim.Model.from_template(tpl, bs, dev)
    t = list(dev_inputs(inp, dev).values())
    with torch.no_grad():
        pos, vel = dp_model.ForwardWarp.apply(*t, _Host(env, bs, T, f2s, inp["dt"]))
    F = len(f2s)
    bq, bqd = pos.view(F, bs, nb, 7).permute(1, 0, 2, 3), vel.view(F, bs, nb, 6).permute(1, 0, 2, 3)
    q_np, qd_np = pos.view(F * bs, nb, 7).cpu().numpy(), vel.view(F * bs, nb, 6).cpu().numpy()
    frames = q_np.reshape(F, bs, nb, 7)
    assert np.abs(frames[1:] - frames[:1]).max() > 1e-4   # it moved
    for rates in RATES:
        rj_q, rj_qd = dp_model.InverseKinematics.apply(bq, bqd, env, rates)
        assert rj_q.shape == (F, bs, int(tpl["nq"])) and rj_qd.shape == (F, bs, int(tpl["nqd"]))
        r64, r32 = coords_of(tpl, torch.float64, q_np, qd_np, rates), coords_of(tpl, torch.float32, q_np, qd_np, rates)
        bar("%s simulated %s joint_q" % (name, rates), rj_q.reshape(F * bs, -1).cpu().numpy(), r32[0], r64[0])
        bar("%s simulated %s joint_qd" % (name, rates), rj_qd.reshape(F * bs, -1).cpu().numpy(), r32[1], r64[1])
        assert np.abs(r64[1]).max() > 1e-2   # the robot is moving


@pytest.mark.parametrize("name,S", VALUE_CASES)
def test_round_trip_through_the_products_own_kernels(name, S, dev):
    """ForwardKinematics(InverseKinematics(state)) against the state, under 4 x the round-trip error of the fp32 torch restatement
    (fp32 IK restatement, then ref_torch.eval_fk in fp32)."""
    from diffphys_amd import dp_model, sim
    from oracle import ref_torch as rt

    C = fk_case(name, S)
    env = sim.Model.from_template(C["tpl"], S, dev)
    bq = torch.tensor(C["bq"]).to(dev).view(S, 1, C["nb"], 7)
    bqd = torch.tensor(C["bqd"]).to(dev).view(S, 1, C["nb"], 6)
    back_q, back_qd = dp_model.ForwardKinematics.apply(*dp_model.InverseKinematics.apply(bq, bqd, env), env)[:2]
    assert back_q.shape == bq.shape and back_qd.shape == bqd.shape
    T32 = oracle_template(C["tpl"], torch.float32)
    j32 = joint_coords(T32, torch.tensor(C["bq"]), torch.tensor(C["bqd"]), "generalized")
    f32 = rt.eval_fk(T32, *j32)
    bar("%s x %d round trip body_q" % (name, S), back_q.view(S, -1, 7).cpu().numpy(), f32[0].numpy(), C["bq"])
    bar("%s x %d round trip body_qd" % (name, S), back_qd.view(S, -1, 6).cpu().numpy(), f32[1].numpy(), C["bqd"])


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S", VJP_CASES)
def test_vjp_matches_float64_autograd(name, S, rates, dev):
    """g_state of random g_q, g_qd -- the parent-side gather included -- against float64 autograd of the restatement; angles with
    0.05 <= |q| <= 1 (no guarded arc at its kink); the quaternion part of both gradients projected onto the tangent space of the unit
    sphere, so that the comparison does not depend on how either side extends off it."""
    from diffphys_amd import hip_backend

    C = fk_case(name, S, 0.05)
    nb, nq, nqd = C["nb"], int(C["tpl"]["nq"]), int(C["tpl"]["nqd"])
    rng = np.random.RandomState(17)
    g_q, g_qd = rng.randn(S, nq).astype(np.float32), rng.randn(S, nqd).astype(np.float32)
    state, table = gpu_state(C, dev), gpu_table(name, rates)
    args = (table, nb, state, torch.from_numpy(g_q).to(dev), torch.from_numpy(g_qd).to(dev))
    g_s = hip_backend.joint_coords_vjp(*args)
    assert g_s.shape == (S * nb, 13)
    assert torch.equal(g_s, hip_backend.joint_coords_vjp(*args))   # fixed summation order: the same bits
    g_s = g_s.cpu().numpy().reshape(S, nb, 13)
    r64 = coords_of(C["tpl"], torch.float64, C["bq"], C["bqd"], rates, g_q, g_qd)
    r32 = coords_of(C["tpl"], torch.float32, C["bq"], C["bqd"], rates, g_q, g_qd)
    tag = "%s x %d %s " % (name, S, rates)
    bar(tag + "g_body_q", tangent(g_s[..., :7], C["bq"]), tangent(r32[2], C["bq"]), tangent(r64[2], C["bq"]))
    bar(tag + "g_body_qd", g_s[..., 7:], r32[3], r64[3])
    par = np.asarray(C["tpl"]["joint_parent"]).reshape(nb)
    inner = [b for b in range(nb) if (par == b).sum() >= 2]
    assert inner and np.abs(r64[3][:, inner]).max() > 0   # bodies that gather several children are in the comparison


def test_gradients_through_the_rollout(dev):
    """loss = <w_q, IK(wp_pos, wp_vel).q> behind ForwardWarp.apply (Laikago, 8 envs x 3 steps, frames at states 0, 2, 3) against the oracle's
    autograd of ref_torch.rollout followed by the restatement, under the bars of tests/test_gpu_ground_wrench.py's rollout-through
    gradients (its check() with CAPS[robot][3])."""
    from diffphys_amd import dp_model, sim
    from ground_wrench_common import oracle_rollout_grads
    from test_gpu_ground_wrench import CAPS, check

    name, bs, T, f2s = "laikago", 8, 3, [0, 2, 3]
    tpl = load_tpl(name)
    nb, nq = int(tpl["nb"]), int(tpl["nq"])
    inp = tight_inputs(tpl, name, bs, T, seed=5)
    inp["frame2step"] = f2s
    F = len(f2s)
    w_q = np.random.RandomState(23).randn(F, bs, nq)
    env = sim.Model.from_template(tpl, bs, dev)
    t = dev_inputs(inp, dev)
    wrt = ("q_init", "qd_init", "refs")
    for k in wrt:
        t[k].requires_grad_(True)
    pos, vel = dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], _Host(env, bs, T, f2s, inp["dt"]))
    rj_q, _ = dp_model.InverseKinematics.apply(pos.view(F, bs, nb, 7).permute(1, 0, 2, 3), vel.view(F, bs, nb, 6).permute(1, 0, 2, 3), env)
    (rj_q * torch.from_numpy(w_q.astype(np.float32)).to(dev)).sum().backward()

    def loss(dtype):
        T_ = oracle_template(tpl, dtype)

        def fn(p, v, g):
            jq, _ = joint_coords(T_, p.reshape(F * bs, nb, 7), v.reshape(F * bs, nb, 6), "generalized")
            return (jq * torch.as_tensor(w_q.reshape(F * bs, nq), dtype=dtype)).sum()
        return fn

    r64 = oracle_rollout_grads(tpl, torch.float64, inp, loss(torch.float64), wrt)
    r32 = oracle_rollout_grads(tpl, torch.float32, inp, loss(torch.float32), wrt)
    for k in wrt:
        assert np.abs(r64[k]).max() > 0, k
        check("d joint-angle loss / d " + k, t[k].grad.cpu().numpy(), r32[k], r64[k], CAPS[name][3])


QUERY_KEYS = {"sim_traj", "target_traj", "control_ref", "vertex_body", "sim_poses", "target_poses", "control_ref_poses", "com", "com_k",
              "body_mass", "grf", "jaf", "max_w"}   # what query() returned before the flag existed


def test_query_returns_the_simulated_joint_coordinates(dev):
    import importlib.util
    import os

    from diffphys_amd.dataloader import DataLoader
    from diffphys_amd.phys_model import phys_model
    from helpers import ROOT

    spec = importlib.util.spec_from_file_location("pd_main_jc", os.path.join(ROOT, "ppr-diffphys_amd", "main.py"))
    pd_main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pd_main)
    opts = pd_main.get_opts(["--seqname", "mi-pace", "--urdf_template", "laikago", "--logroot", "/tmp/pprdp_test_log/", "--logname", "jc",
                             "--num_envs", "8", "--frames_per_wdw", "4"])
    torch.manual_seed(0)
    np.random.seed(0)
    model = phys_model(opts, DataLoader(opts)).cuda()
    model.train()
    model.reinit_envs(opts["num_envs"], frames_per_wdw=opts["frames_per_wdw"])
    model.set_progress(0)
    model.forward(frame_start=torch.arange(8, device=model.device) * 3)
    plain = model.query()
    assert set(plain) == QUERY_KEYS
    q = model.query(joint_coords=True)
    assert set(q) == QUERY_KEYS | {"sim_joint_q", "sim_joint_qd"}
    assert q["sim_joint_q"].shape == (4, 19) and q["sim_joint_qd"].shape == (4, 18)
    for k in QUERY_KEYS - {"com_k", "max_w"}:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(q[k])), k
    vels = np.stack(list(model.sim_vels), 0)
    assert vels.shape == (4, 13, 6)
    tpl = load_tpl("laikago")
    r64 = coords_of(tpl, torch.float64, q["sim_poses"].astype(np.float32), vels, "generalized")
    r32 = coords_of(tpl, torch.float32, q["sim_poses"].astype(np.float32), vels, "generalized")
    bar("query sim_joint_q", q["sim_joint_q"], r32[0], r64[0])
    bar("query sim_joint_qd", q["sim_joint_qd"], r32[1], r64[1])


def test_the_op_inside_a_captured_graph(dev):
    """Neither entry allocates through HIP or synchronises: forward and VJP captured once, replayed on new inputs: eager's bits."""
    from diffphys_amd import hip_backend

    C = fk_case("human", 3)
    nb, nq, nqd = C["nb"], int(C["tpl"]["nq"]), int(C["tpl"]["nqd"])
    table = gpu_table("human", "generalized")
    state = gpu_state(C, dev)
    gen = torch.Generator().manual_seed(5)
    g_q, g_qd = torch.randn(3, nq, generator=gen).to(dev), torch.randn(3, nqd, generator=gen).to(dev)

    def run(s, a, b):
        jq, jqd = hip_backend.joint_coords(table, nb, s)
        return jq, jqd, hip_backend.joint_coords_vjp(table, nb, s, a, b)

    sbuf, abuf, bbuf = state.clone(), g_q.clone(), g_qd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sbuf, abuf, bbuf)   # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = run(sbuf, abuf, bbuf)
    torch.cuda.current_stream().wait_stream(side)
    for trial in range(2):
        fresh = state * (1.0 + 0.01 * (trial + 1))   # other states (quaternions off the unit sphere: all the same to the arithmetic)
        a2, b2 = torch.randn(3, nq, generator=gen).to(dev), torch.randn(3, nqd, generator=gen).to(dev)
        sbuf.copy_(fresh); abuf.copy_(a2); bbuf.copy_(b2)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(cap, run(fresh, a2, b2)):
            assert torch.equal(got, want), trial
    assert not torch.equal(cap[0], run(state, g_q, g_qd)[0])
