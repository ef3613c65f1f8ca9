"""Robots whose ground-contact tables do not fit in LDS at any segment width (tables in global memory; csrc/pd_host.hip build_device).

Models: laikago_toes (the reference's laikago_toes.urdf compiled into tests/golden/template_laikago_toes.npz: full lower-leg collision
mesh + toe spheres, 11 018 candidates, fixed toe joints -> the generic joint mix: split forward + k_rollout_bwd3), Laikago with its
candidates replicated to ~12 000 / ~40 000 / exactly 65 535 (revolute-only: cull wave, RUNSUM, both kernel families) and human replicated
past 10 000 (compound-only).  Bars are the suite's existing ones: the fp32 C oracle as in test_gpu_parity.py's 5 757-point test, the
own-trajectory check with the short-horizon bars of test_gpu_tight.py, the hit log complete, two runs bit-identical, the fused trajectory
loss equal to the torch composition."""
import os

import numpy as np
import pytest
import torch

from gpu_harness import c_oracles, dev, gpu_rollout, same_bits  # noqa: F401
from helpers import GOLDEN, GRAD_LEAD, per_env, relmax

pytestmark = pytest.mark.gpu



def toes_template():
    with np.load(os.path.join(GOLDEN, "template_laikago_toes.npz")) as z:
        return {k: z[k] for k in z.files}


def replicated(name, nc_total, seed=3):
    """The robot's template with its candidates replicated (jittered by 0.2 mm, as test_more_contact_candidates_than_fit_at_the_default_width
    does) up to nc_total."""
    from diffphys_amd import robots

    tpl = dict(robots.load_template(name))
    nc = len(tpl["contact_body"])
    rng = np.random.RandomState(seed)
    extra = rng.randint(0, nc, nc_total - nc)
    for k in ("contact_body", "contact_dist", "contact_material"):
        tpl[k] = np.concatenate([tpl[k], tpl[k][extra]])
    jitter = (rng.randn(len(extra), 3) * 2e-4).astype(np.float32)
    tpl["contact_point"] = np.concatenate([tpl["contact_point"], tpl["contact_point"][extra] + jitter]).astype(np.float32)
    return tpl


MODELS = {"laikago_toes": (toes_template, "laikago"), "laikago12k": (lambda: replicated("laikago", 12000), "laikago"),
          "laikago40k": (lambda: replicated("laikago", 40000), "laikago"), "human10k": (lambda: replicated("human", 10336), "human")}


def model(key):
    make, robot = MODELS[key]
    return make(), robot


def table_bytes(tpl):
    return 16 * len(tpl["contact_body"])   # the points alone; the tables copied into LDS are larger still


def inputs(tpl, robot, bs, T, seed, kicked=False):
    from diffphys_amd import synth

    inp = synth.make_inputs(tpl, robot, bs=bs, nsteps=T, seed=seed, steps_per_frame=5, penetration=0.003)
    if kicked:   # as test_gpu_tight.py's short kicked horizons: feet leave and hit the ground inside the horizon
        rng = np.random.RandomState(5)
        nb = int(tpl["nb"])
        inp["qd_init"] = (rng.randn(*inp["qd_init"].shape) * 0.3).astype(np.float32)
        inp["frame2step"] = [0, T]
        inp["adj_pos"] = (rng.randn(2, bs * nb, 7) * 1e-3).astype(np.float32)
        inp["adj_vel"] = (rng.randn(2, bs * nb, 6) * 1e-3).astype(np.float32)
    return inp


def oracle(tpl, inp, dtype=np.float32):
    """C oracle forward + adjoint.  A model with FIXED joints (laikago_toes) is evaluated with the kernels' scale-invariant fixed-joint
    angle (set_twist_eval(True)), as test_gpu_parity.py::test_generic_joint_kernel_on_toy_robot does: the literal form turns the fp32 norm
    error of the quaternions into spurious angles for any evaluator."""
    return c_oracles(tpl, inp, dtype, twist_eval=has_fixed(tpl))


def has_fixed(tpl):
    return 3 in set(int(j) for j in np.asarray(tpl["joint_type"]))


def check_grad(tpl, inp, k, mine, gr, as_oracle=lambda g: g):
    """Gradient bar: within 2e-2 of the fp32 oracle (test_gpu_parity.py's 5 757-point test) -- or, where the fp32 oracle itself is further
    from float64 than that, test_gpu_parity.py::test_vs_c_oracle_fresh_seed's: within max(2e-2, 2 x the fp32 oracle's error) of float64.
    A model with fixed joints (the generic kernels) is held to the suite's bar for those, as test_gpu_parity.py::
    test_generic_joint_kernel_on_toy_robot holds its toy robot: the own-trajectory check (test_gradients_vs_float64_adjoint_of_own_trajectory
    below, laikago_toes included); here its gradients must be finite and the difference is printed."""
    e = relmax(mine, as_oracle(gr[k]))
    if has_fixed(tpl):
        print("%s (fixed joints): kernel vs fp32 oracle %.1e" % (k, e))
        assert np.isfinite(mine).all(), k
        return
    if e < 2e-2:
        return
    g64 = as_oracle(oracle(tpl, inp, np.float64)[1][k])
    e64, e32 = relmax(mine, g64), relmax(as_oracle(gr[k]), g64)
    print("%s: kernel vs fp32 oracle %.1e, vs float64 %.1e; fp32 oracle vs float64 %.1e" % (k, e, e64, e32))
    assert e64 < max(2e-2, 2 * e32), (k, e, e64, e32)


def check_vs_oracle(tpl, inp, out):
    """The bars of test_gpu_parity.py::test_more_contact_candidates_than_fit_at_the_default_width (fp32 C oracle)."""
    st, gr = oracle(tpl, inp)
    assert np.abs(st["grf"]).max() > 1.0, "contacts must be active"
    assert relmax(out["wp_pos"], st["wp_pos"]) < 5e-5 and relmax(out["grf"], st["grf"]) < 5e-3, (relmax(out["wp_pos"], st["wp_pos"]), relmax(out["grf"], st["grf"]))
    for k in ("q_init", "qd_init", "refs", "body_inv_mass"):
        check_grad(tpl, inp, k, out["grads"][k].reshape(gr[k].shape), gr)


def assert_global_tables(dm, tpl):
    """Both launches of the last rollout ran with less dynamic LDS than the contact points alone take: the tables stayed in global memory."""
    for kind in (0, 1):
        info = dm.last_launch_info(kind)
        assert 0 < info["lds_bytes_per_wg"] < table_bytes(tpl), (kind, info, table_bytes(tpl))


def sub_batch(inp, bs, pick):
    """The inputs of envs `pick` alone (envs are independent: their outputs and gradients are those of the full batch)."""
    T, F = inp["nsteps"], len(inp["frame2step"])
    sub = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    for k in ("q_init", "qd_init", "target_ke", "target_kd", "body_mass", "body_inv_mass", "body_inertia", "body_inv_inertia"):
        sub[k] = np.ascontiguousarray(inp[k].reshape(bs, -1)[pick].reshape(-1))
    for k in ("torques", "refs", "res_f"):
        sub[k] = np.ascontiguousarray(inp[k].reshape(T, bs, -1)[:, pick].reshape(T, -1))
    for k in ("adj_pos", "adj_vel"):
        sub[k] = np.ascontiguousarray(inp[k].reshape(F, bs, -1)[:, pick].reshape(F, -1))
    return sub


def test_only_models_that_fit_nowhere_take_global_tables(dev):
    """A model that fits keeps its width (Laikago: 16 lanes); every large model builds at a width >= its bodies, accepts a forced width its
    envs' scratch fits, and the revolute-only one stays quad-lane eligible."""
    from diffphys_amd import hip_backend, robots

    dm = hip_backend.DeviceModel(robots.load_template("laikago"))
    assert dm.segment_width() == 16
    for key in MODELS:
        tpl, robot = model(key)
        dm = hip_backend.DeviceModel(tpl)
        nb = int(tpl["nb"])
        w = dm.segment_width()
        print("%s: %d candidates, %d bodies, segment width %d, quad-lane eligible %s" % (key, len(tpl["contact_body"]), nb, w, dm.kernel_family()[1]))
        assert w >= nb
        dm.set_segment_width(64)
        assert dm.segment_width() == 64
    tpl, _ = model("laikago12k")
    assert hip_backend.DeviceModel(tpl).kernel_family()[1], "a revolute-only robot with <= 16 bodies stays quad-lane eligible"


@pytest.mark.parametrize("key,bs,family", [("laikago_toes", 9, 0), ("laikago_toes", 37, 0), ("laikago12k", 9, 1), ("laikago12k", 37, 2),
                                           ("laikago40k", 9, 1), ("laikago40k", 9, 2), ("human10k", 9, 0), ("human10k", 37, 0)])
def test_one_workgroup_against_the_fp32_oracle(key, bs, family, dev, oracle_libs):
    from diffphys_amd import hip_backend

    tpl, robot = model(key)
    dm = hip_backend.DeviceModel(tpl)
    if family:
        dm.set_kernel_family(family)
    inp = inputs(tpl, robot, bs, 12, seed=4)
    out = gpu_rollout(dm, inp, dev)
    assert_global_tables(dm, tpl)
    if family == 2:
        assert dm.last_launch_info(0)["envs_per_wg"] <= 4, dm.last_launch_info(0)   # the quad-lane kernels ran
    check_vs_oracle(tpl, inp, out)
    assert same_bits(out, gpu_rollout(dm, inp, dev)), "two runs must give the same bits"


@pytest.mark.parametrize("key,family", [("laikago_toes", 0), ("laikago12k", 1), ("laikago12k", 2), ("human10k", 0)])
def test_gradients_vs_float64_adjoint_of_own_trajectory(key, family, dev, oracle_libs):
    """helpers.own_trajectory_check, kicked 8-step horizon, with test_gpu_tight.py's bars (Laikago 8 steps; human every env)."""
    from helpers import own_trajectory_check
    from diffphys_amd import hip_backend

    tpl, robot = model(key)
    dm = hip_backend.DeviceModel(tpl)
    if family:
        dm.set_kernel_family(family)
    bs, T = 48, 8
    inp = inputs(tpl, robot, bs, T, seed=9, kicked=True)
    r = own_trajectory_check(dm, tpl, inp, dev)
    w = r["worst"]
    q = lambda a, p: float(np.percentile(a, p))
    print("%s family %d: worst-tensor error per env median %.1e p99.5 %.1e max %.1e; touches %d, missing from the hit log %d" % (
        key, family, np.median(w), q(w, 99.5), w.max(), r["touches"], r["hitlog_missing"]))
    assert all(np.isfinite(v).all() for v in r["grads"].values())
    assert r["touches"] > bs and r["hitlog_missing"] == 0, (r["touches"], r["hitlog_missing"])
    if robot != "laikago":
        assert w.max() < 1e-4 and q(w, 99) < 2e-5, (float(w.max()), q(w, 99))
    else:
        assert w.max() < 5e-4 and q(w, 99.5) < 2e-4 and np.median(w) < 2e-5, (float(w.max()), q(w, 99.5), float(np.median(w)))


@pytest.mark.parametrize("key,bs", [("laikago_toes", 4096), ("laikago12k", 4096), ("human10k", 1024)])
def test_full_chip(key, bs, dev, oracle_libs):
    """A full chip (RUNSUM forward for the revolute model): tables in global memory, two runs bit-identical, and eight envs picked across
    the batch against the fp32 oracle on those envs alone."""
    from diffphys_amd import hip_backend

    tpl, robot = model(key)
    dm = hip_backend.DeviceModel(tpl)
    dm.set_kernel_family(1)
    T = 10
    inp = inputs(tpl, robot, bs, T, seed=7)
    out = gpu_rollout(dm, inp, dev)
    assert_global_tables(dm, tpl)
    if robot == "laikago" and key == "laikago12k":
        assert dm.last_launch_info(0)["threads_per_wg"] % 192 == 0   # body, contact and cull wave per env group
    assert all(np.isfinite(v).all() for v in (out["wp_pos"], out["wp_vel"])) and all(np.isfinite(v).all() for v in out["grads"].values())
    assert same_bits(out, gpu_rollout(dm, inp, dev))
    pick = np.linspace(0, bs - 1, 8).astype(np.int64)
    sub = sub_batch(inp, bs, pick)
    F = len(inp["frame2step"])
    st, gr = oracle(tpl, sub)
    for k, bar in (("wp_pos", 5e-5), ("wp_vel", 5e-3)):
        mine = out[k].reshape(F, bs, -1)[:, pick]
        assert relmax(mine, st[k].reshape(mine.shape)) < bar, (k, relmax(mine, st[k].reshape(mine.shape)))
    for k in ("q_init", "qd_init", "refs", "body_inv_mass"):
        check_grad(tpl, sub, k, per_env(out["grads"][k], bs, GRAD_LEAD[k])[pick], gr, lambda g, k=k: per_env(g, len(pick), GRAD_LEAD[k]))


def test_65535_candidates_build_and_run_65536_are_refused(dev, oracle_libs):
    from diffphys_amd import hip_backend

    tpl = replicated("laikago", 65535)
    dm = hip_backend.DeviceModel(tpl)
    inp = inputs(tpl, "laikago", 9, 6, seed=2)
    out = gpu_rollout(dm, inp, dev)
    assert_global_tables(dm, tpl)
    check_vs_oracle(tpl, inp, out)
    with pytest.raises(RuntimeError, match="more than 65535 contact candidates"):
        hip_backend.DeviceModel(replicated("laikago", 65536))


def test_fused_traj_loss_and_the_drop_in_boundary(dev):
    """laikago_toes through the reference-shaped boundary: ForwardWarp.apply + autograd runs and is finite, ForwardKinematics runs, and
    pd_rollout_*_traj_loss_fk (ForwardWarpTrajLossFK) equals ForwardWarp + se3_loss + reduce_loss and a separate ForwardKinematics, as in
    test_gpu_parity.py: the loss to 1e-6, the poses bit-identical, every gradient to 1e-4 of its tensor's max."""
    from diffphys_amd import dp_model, dp_utils, sim, synth

    tpl = toes_template()
    bs, T = 37, 46
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T, seed=5, steps_per_frame=23, penetration=0.002)
    f2s = [0, 23, T]
    F, nb, nq, nqd = len(f2s), int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])

    class Host:
        pass

    h = Host()
    h.env = sim.Model.from_template(tpl, bs, device=dev)
    h.num_envs, h.steps_idx, h.frame2step, h.dt = bs, range(T), f2s, inp["dt"]
    t = {k: torch.from_numpy(inp[k]).to(dev).requires_grad_(True) for k in synth.INPUT_NAMES}
    args = [t[k] for k in synth.INPUT_NAMES]
    pos, vel = dp_model.ForwardWarp.apply(*args, h)
    assert pos.shape == (F, bs * nb, 7)
    g = torch.Generator().manual_seed(11)
    tgt = (pos.detach().reshape(F, bs, nb, 7).permute(1, 0, 2, 3) + (torch.randn(bs, F, nb, 7, generator=g) * 0.02).to(dev)).contiguous()
    outseq = torch.zeros(bs, F, dtype=torch.bool, device=dev)
    qq = (torch.from_numpy(inp["q_init"]).to(dev).view(1, bs, nq).repeat(F, 1, 1) + 0.01).requires_grad_(True)
    qqd = torch.zeros(F, bs, nqd, device=dev, requires_grad=True)
    w_q = torch.randn(bs, F, nb, 7, generator=g).to(dev)

    def grads():
        out = [t[k].grad.detach().clone() for k in synth.INPUT_NAMES] + [qq.grad.detach().clone()]
        for k in synth.INPUT_NAMES:
            t[k].grad = None
        qq.grad = None
        return out

    sim_pos = pos.reshape(F, bs, nb, 7).permute(1, 0, 2, 3)
    loss_ref = dp_utils.reduce_loss(dp_utils.se3_loss(sim_pos, tgt).mean(-1), clip=True)
    qp, qv, _ = dp_model.ForwardKinematics.apply(qq, qqd, h.env)
    assert qp.shape == (bs, F, nb, 7)
    (loss_ref * 0.37 + (qp * w_q).sum()).backward()
    ref = grads()
    assert all(torch.isfinite(x).all() for x in ref)
    loss, pos2, vel2, qp2, qv2, _ = dp_model.ForwardWarpTrajLossFK.apply(*args, tgt, outseq, qq, qqd, h)
    assert torch.equal(pos2, pos.detach()) and torch.equal(vel2, vel.detach()) and torch.equal(qp2, qp.detach())
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-6 * abs(float(loss_ref.detach())), (float(loss.detach()), float(loss_ref.detach()))
    (loss * 0.37 + (qp2 * w_q).sum()).backward()
    got = grads()
    for a, b in zip(got, ref):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-30
