"""The whole-body (centroidal) op -- PD_POSE_CENTROIDAL, k_centroidal_fwd / k_centroidal_vjp of ppr-diffphys_amd/csrc/pd_pose.hip -- on a
real MI355X (run with -m gpu): total mass, centre of mass and its velocity, linear momentum, angular momentum about the centre of mass,
kinetic and potential energy per state set, and their gradients in the states, the masses and the inertias.

Reference: tests/centroidal_ref.py (the definition over oracle/ref_torch.py's q_rot / q_rot_inv / cross) in float64 on the SAME fp32
inputs.  Bar (the project's, test_gpu_state_ops_generated.bar), per tensor: relmax(GPU, f64) <= max(4 x relmax(fp32 torch, f64), 1e-5),
everything finite, no element excluded, and the input-quality condition relmax(fp32 torch, f64) <= 1e-4 asserted.  Every comparison
prints GPU / fp32 / bar.  Shapes: the set counts of the state-op tests (SETS), the smallest that cross every boundary of the mapping
(256 // nb whole sets per 256-lane workgroup, a lane per body)."""
import functools

import numpy as np
import pytest
import torch

from gpu_harness import FWD, dev, dev_inputs  # noqa: F401
from centroidal_ref import SLICES, centroidal, centroidal_of, template_constants
from generated_robots import robot, rollout_inputs
from helpers import INPUT_NAMES, tight_inputs
from joint_coords_ref import load_tpl
from test_gpu_state_ops_generated import SETS, bar, fk_case, frozen

pytestmark = pytest.mark.gpu

KINDS = ["fk", "tumbled", "scaled"]
NAMES = ("mass", "com", "com_vel", "momentum", "angular_momentum", "kinetic", "potential")


def test_the_launch_shapes_are_the_ones_meant():
    """What SETS promises, checked against the two kernels' mapping: 256 // nb whole sets per workgroup."""
    seen = []
    for name, S in SETS.items():
        nb = int(robot(name)["nb"])
        per_wg = 256 // nb
        assert S * nb > 256 and S * nb <= 600
        assert S % per_wg != 0 or per_wg == 1             # the last workgroup is partly filled
        assert nb > 128 or -(-S // per_wg) >= 2           # at least two workgroups
        seen.append(256 - per_wg * nb)
    assert list(SETS) == ["mixed25", "rev64", "cmp31", "mixed129", "rev256", "world5", "free1"]
    assert seen == [6, 0, 8, 127, 0, 1, 0]                # idle lanes per workgroup
    # the tree's width: nb below, at and above a power of two, and the trivial tree of one body
    assert sorted(int(robot(n)["nb"]) for n in SETS) == [1, 5, 25, 31, 64, 129, 256]


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """fp32 operands [S, nb, .] of a generated robot.
    fk:      the eval_fk states of the state-op tests
    tumbled: those, every set moved by up to +-50 m in x and z and given a common velocity of up to +-2 m/s (the one-pass form of L
             loses 250 ulps here)
    scaled:  the fk states with every quaternion scaled by 0.7 .. 1.4 (rows are taken as they are)
    Masses and inertias: the template's, scaled per (set, body) by 0.8 .. 1.25; g_out standard normal."""
    C = fk_case(name)
    tpl, S, nb = C["tpl"], C["S"], C["nb"]
    rng = np.random.RandomState(900 + nb + KINDS.index(kind))
    bq, bqd = np.array(C["bq"], np.float32), np.array(C["bqd"], np.float32)
    if kind == "tumbled":
        shift = np.zeros((S, 1, 3))
        shift[:, 0, 0], shift[:, 0, 2] = rng.uniform(-50, 50, S), rng.uniform(-50, 50, S)
        bq[..., :3] = (bq[..., :3].astype(np.float64) + shift).astype(np.float32)
        bqd[..., 3:] = (bqd[..., 3:].astype(np.float64) + rng.uniform(-2, 2, (S, 1, 3))).astype(np.float32)
    elif kind == "scaled":
        bq[..., 3:] *= rng.uniform(0.7, 1.4, (S, nb, 1)).astype(np.float32)
    scale = rng.uniform(0.8, 1.25, (S, nb))
    mass = (np.asarray(tpl["body_mass"], np.float64).reshape(1, nb) * scale).astype(np.float32)
    inertia = (np.asarray(tpl["body_inertia"], np.float64).reshape(1, nb, 3, 3) * scale[..., None, None]).astype(np.float32)
    g_out = rng.randn(S, 16).astype(np.float32)
    frozen(bq, bqd, mass, inertia, g_out)
    return dict(tpl=tpl, S=S, nb=nb, bq=bq, bqd=bqd, mass=mass, inertia=inertia, g_out=g_out)


@functools.lru_cache(maxsize=None)
def restated(name, kind, dtype):
    """(out, g_body_q, g_body_qd, g_mass, g_inertia) of the restatement and its autograd in ``dtype``: once, shared."""
    C = case(name, kind)
    out = centroidal_of(C["tpl"], dtype, C["bq"], C["bqd"], C["mass"], C["inertia"], C["g_out"])
    frozen(*out)
    return out


def rows23(bq, bqd, mass, inertia, dev):
    S, nb = bq.shape[:2]
    r = np.concatenate([bq, bqd, np.broadcast_to(mass, (S, nb))[..., None], np.broadcast_to(inertia, (S, nb, 3, 3)).reshape(S, nb, 9)], -1)
    return torch.from_numpy(np.ascontiguousarray(r.reshape(-1, 23), dtype=np.float32)).to(dev)


@functools.lru_cache(maxsize=None)
def gpu_mass_table(name):
    from diffphys_amd import hip_backend

    return hip_backend.mass_table(robot(name), torch.device("cuda:0"))


def compare_outputs(tag, got, r32, r64):
    for k in NAMES:
        bar("%s %s" % (tag, k), got[..., SLICES[k]], r32[..., SLICES[k]], r64[..., SLICES[k]])
    assert (got[..., 15] == 0).all()


def compare_grads(tag, g_rows, r32, r64):
    """g_rows [S, nb, 23] against (g_body_q, g_body_qd, g_mass, g_inertia) of the two restatements: raw partials on both sides."""
    bar(tag + " g_body_q", g_rows[..., :7], r32[0], r64[0])
    bar(tag + " g_body_qd", g_rows[..., 7:13], r32[1], r64[1])
    bar(tag + " g_mass", g_rows[..., 13], r32[2], r64[2])
    bar(tag + " g_inertia", g_rows[..., 14:].reshape(r64[3].shape), r32[3], r64[3])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SETS))
def test_values_and_vjp(name, kind, dev):
    from diffphys_amd import hip_backend

    C = case(name, kind)
    S, nb = C["S"], C["nb"]
    rows, table = rows23(C["bq"], C["bqd"], C["mass"], C["inertia"], dev), gpu_mass_table(name)
    out = hip_backend.centroidal(table, nb, rows)
    g_rows = hip_backend.centroidal_vjp(table, nb, rows, torch.tensor(C["g_out"], device=dev))
    assert out.shape == (S, 16) and g_rows.shape == (S * nb, 23)
    r64, r32 = restated(name, kind, torch.float64), restated(name, kind, torch.float32)
    tag = "%s x %d %s" % (name, S, kind)
    compare_outputs(tag, out.cpu().numpy(), r32[0], r64[0])
    compare_grads(tag, g_rows.cpu().numpy().reshape(S, nb, 23), r32[1:], r64[1:])
    assert all(np.abs(g).max() > 0 for g in r64[1:])
    if kind == "tumbled":
        assert np.abs(C["bq"][..., [0, 2]]).max() > 25.0
    if kind == "scaled":
        qn = np.linalg.norm(C["bq"][..., 3:].astype(np.float64), axis=-1)
        assert qn.min() < 0.8 and qn.max() > 1.25


@pytest.mark.parametrize("name", list(SETS))
def test_a_sets_bits_do_not_depend_on_its_place(name, dev):
    """The outputs and g_b rows of set k computed ALONE equal, bit for bit, those of the full launch -- the first set, the last one (in
    a partly filled workgroup) and, where nb does not divide 256, a set whose elements straddle a 256-element boundary; two runs of the
    full launch: the same bits."""
    from diffphys_amd import hip_backend

    C = case(name, "tumbled")
    S, nb = C["S"], C["nb"]
    rows, table = rows23(C["bq"], C["bqd"], C["mass"], C["inertia"], dev), gpu_mass_table(name)
    g_out = torch.tensor(C["g_out"], device=dev)
    out, g_rows = hip_backend.centroidal(table, nb, rows), hip_backend.centroidal_vjp(table, nb, rows, g_out)
    assert torch.equal(out, hip_backend.centroidal(table, nb, rows)) and torch.equal(g_rows, hip_backend.centroidal_vjp(table, nb, rows, g_out))
    picks = [0, S - 1] + [k for k in range(S) if (k * nb) // 256 != ((k + 1) * nb - 1) // 256][:1]
    assert len(picks) == 3 or 256 % nb == 0
    for k in picks:
        alone = rows[k * nb: (k + 1) * nb].contiguous()
        assert torch.equal(hip_backend.centroidal(table, nb, alone)[0], out[k]), k
        assert torch.equal(hip_backend.centroidal_vjp(table, nb, alone, g_out[k: k + 1].contiguous()), g_rows[k * nb: (k + 1) * nb]), k
    assert torch.isfinite(out).all() and torch.isfinite(g_rows).all()


def test_a_table_of_another_nb_gives_zeros(dev):
    """The library cannot validate a device buffer: the kernels check the table's nb against the call's and write zeros (no row of the
    table is read)."""
    from diffphys_amd import hip_backend

    C = case("cmp31", "fk")
    rows = rows23(C["bq"], C["bqd"], C["mass"], C["inertia"], dev)
    wrong = gpu_mass_table("mixed25").clone()   # 8 + 4 * 25 floats: shorter than the table of 31 bodies
    wrong._pd_table = ("mass", (31,))           # ... passed off as one
    out = hip_backend.centroidal(wrong, 31, rows)
    g = hip_backend.centroidal_vjp(wrong, 31, rows, torch.tensor(C["g_out"], device=dev))
    assert (out == 0).all() and (g == 0).all()


class _Host:
    """the attributes the ForwardWarp family reads from ``self``"""

    def __init__(self, env, bs, nsteps, frame2step, dt):
        self.env, self.num_envs, self.steps_idx, self.frame2step, self.dt = env, bs, range(nsteps), list(frame2step), dt


@pytest.mark.parametrize("name", ["laikago", "human", "quad"])
def test_shipped_templates_on_rollout_frames(name, dev):
    """Frame states of a real rollout (ForwardWarp, 8 envs x 6 steps, tight_inputs: frames at states 0 and 6) with that rollout's per-env
    masses and inertias, through dp_utils.centroidal and its backward."""
    from diffphys_amd import dp_model, dp_utils, sim

    bs, T = 8, 6
    tpl = load_tpl(name)
    nb = int(tpl["nb"])
    inp = tight_inputs(tpl, name, bs, T, seed=5)
    f2s = inp["frame2step"]
    F = len(f2s)
    env = sim.Model.from_template(tpl, bs, dev)
    t = dev_inputs(inp, dev)
    with torch.no_grad():
        pos, vel = dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], _Host(env, bs, T, f2s, inp["dt"]))
    bq, bqd = pos.view(F, bs, nb, 7).clone().requires_grad_(True), vel.view(F, bs, nb, 6).clone().requires_grad_(True)
    mass, inertia = t["body_mass"].view(bs, nb).clone().requires_grad_(True), t["body_inertia"].view(bs, nb, 3, 3).clone().requires_grad_(True)
    cs = dp_utils.centroidal(bq, bqd, mass, inertia, env)
    assert cs.mass.shape == (F, bs) and cs.com.shape == (F, bs, 3) and cs.angular_momentum.shape == (F, bs, 3) and cs.potential.shape == (F, bs)
    out = torch.cat([v.reshape(F, bs, -1) for v in cs], -1)   # [F, bs, 15]
    g_out = np.random.RandomState(3).randn(F, bs, 16).astype(np.float32)
    (out * torch.from_numpy(g_out[..., :15]).to(dev)).sum().backward()
    args = (bq.detach().cpu().numpy().reshape(F * bs, nb, 7), bqd.detach().cpu().numpy().reshape(F * bs, nb, 6),
            np.tile(inp["body_mass"].reshape(bs, nb), (F, 1)), np.tile(inp["body_inertia"].reshape(bs, nb, 3, 3), (F, 1, 1, 1)))
    r64 = centroidal_of(tpl, torch.float64, *args, g_out.reshape(F * bs, 16))
    r32 = centroidal_of(tpl, torch.float32, *args, g_out.reshape(F * bs, 16))
    assert np.abs(bq.detach().cpu().numpy()[1] - bq.detach().cpu().numpy()[0]).max() > 1e-4   # it moved
    compare_outputs(name + " frames", np.concatenate([out.detach().cpu().numpy().reshape(F * bs, 15), np.zeros((F * bs, 1))], -1), r32[0], r64[0])
    tag = name + " frames"
    bar(tag + " g_body_q", bq.grad.cpu().numpy().reshape(F * bs, nb, 7), r32[1], r64[1])
    bar(tag + " g_body_qd", bqd.grad.cpu().numpy().reshape(F * bs, nb, 6), r32[2], r64[2])
    # shared masses: broadcast outside the Function, so autograd sums their gradient over the frames
    fsum = lambda a: a.reshape((F, bs) + a.shape[1:]).sum(0)
    bar(tag + " g_mass (summed over frames)", mass.grad.cpu().numpy(), fsum(r32[3]), fsum(r64[3]))
    bar(tag + " g_inertia (summed over frames)", inertia.grad.cpu().numpy(), fsum(r32[4]), fsum(r64[4]))


@functools.lru_cache(maxsize=None)
def momentum_rollout(name):
    """One GPU rollout of a generated robot, bs 3, 8 steps, 3 mm in the ground, frames at states 3 and 4 (the grf of step 3 with them)."""
    from diffphys_amd import hip_backend, sim

    dev = torch.device("cuda:0")
    tpl = robot(name)
    inp = rollout_inputs(tpl, bs=3, T=8)
    env = sim.Model.from_template(tpl, 3, dev)
    dm = hip_backend.device_model(env)
    t = dev_inputs(inp, dev)
    pos, vel, grf, jaf, ws = dm.rollout_forward(3, 8, inp["dt"], *[t[k] for k in FWD], frame2step=[3, 4])
    return dict(tpl=tpl, inp=inp, env=env, nb=dm.nb, t=t, pos=pos, vel=vel, grf=grf)


@pytest.mark.parametrize("name", ["mixed25", "cmp31", "rev64"])
def test_momentum_identity_through_the_rollout_kernels(name, dev):
    """P(4) - P(3) = dt (sum_bodies grf[3].force + M g) on the states and the grf ONE rollout launch wrote (mixed25, cmp31: the
    generic-joint kernels; rev64: the revolute-only family): joints never change the total linear momentum.  The residual r = max |lhs -
    rhs| / max |rhs| with P, M from the op against the same residual with P, M from the fp32 torch restatement on the same kernel states:
    r_gpu <= max(4 r_fp32, 1e-5).  (The all-fp32 oracle rollout gives r_fp32 = 4.4e-6 .. 6.5e-6 on the CPU: the residual is the fp32
    rounding of v in the integrator, |v| eps against |g| dt.)"""
    from diffphys_amd import dp_utils

    C = momentum_rollout(name)
    tpl, nb, dt, bs = C["tpl"], C["nb"], C["inp"]["dt"], 3
    bq, bqd = C["pos"].view(2, bs, nb, 7), C["vel"].view(2, bs, nb, 6)
    mass, inertia = C["t"]["body_mass"].view(bs, nb), C["t"]["body_inertia"].view(bs, nb, 3, 3)
    cs = dp_utils.centroidal(bq, bqd, mass, inertia, C["env"])
    grav = np.asarray(tpl["gravity"], np.float64).reshape(3)
    force = C["grf"].view(-1, bs, nb, 6)[0, :, :, 3:].double().sum(1).cpu().numpy()   # [bs, 3]
    assert float(C["vel"][..., 3:].abs().max()) < 10.0   # the integrator's velocity clamp is not in play
    contact = (C["grf"].view(-1, bs, nb, 6)[0] - C["t"]["res_f"][3].view(bs, nb, 6)).abs().amax(-1) > 0
    assert int(contact.sum()) >= 1, "no body touches the ground at step 3"

    def residual(P, M):
        rhs = dt * (force + M[0][:, None] * grav)
        return float(np.abs((P[1] - P[0]) - rhs).max() / np.abs(rhs).max())

    r_gpu = residual(cs.momentum.double().cpu().numpy(), cs.mass.double().cpu().numpy())
    args = (bq.cpu().numpy().reshape(2 * bs, nb, 7), bqd.cpu().numpy().reshape(2 * bs, nb, 6),
            np.tile(C["inp"]["body_mass"].reshape(bs, nb), (2, 1)), np.tile(C["inp"]["body_inertia"].reshape(bs, nb, 3, 3), (2, 1, 1, 1)))
    o32 = centroidal_of(tpl, torch.float32, *args)[0].astype(np.float64).reshape(2, bs, 16)
    o64 = centroidal_of(tpl, torch.float64, *args)[0].reshape(2, bs, 16)
    r_32 = residual(o32[..., SLICES["momentum"]], o32[..., 0])
    r_64 = residual(o64[..., SLICES["momentum"]], o64[..., 0])
    lim = max(4 * r_32, 1e-5)
    print("%s momentum identity on the kernels' states: GPU %.2e / fp32 torch %.2e / bar %.2e (float64 P on the same states: %.2e), "
          "%d bodies touching" % (name, r_gpu, r_32, lim, r_64, int(contact.sum())))
    assert np.isfinite(r_gpu) and r_gpu <= lim


def test_gradients_through_the_rollout(dev):
    """loss = sum of squared com, momentum and angular_momentum of centroidal(wp_pos, wp_vel, body_mass, body_inertia) behind
    ForwardWarp.apply (Laikago, 8 envs x 3 steps, frames at states 0, 2, 3) with a phys_model-style parametrisation -- body_inv_mass =
    1 / m, body_inertia = N m, body_inv_inertia = N^-1 / m of ONE leaf m -- so that d loss / d m is the sum of the direct path through
    the op and of the rollout's paths; against the float64 oracle rollout plus the restatement under autograd, under the bars of
    tests/test_gpu_ground_wrench.py's through-the-rollout gradients (its check() with CAPS[robot][3])."""
    from diffphys_amd import dp_model, dp_utils, sim
    from ground_wrench_common import oracle_template
    from oracle import ref_torch as rt
    from test_gpu_ground_wrench import CAPS, check

    name, bs, T, f2s = "laikago", 8, 3, [0, 2, 3]
    tpl = load_tpl(name)
    nb = int(tpl["nb"])
    inp = tight_inputs(tpl, name, bs, T, seed=5)
    F = len(f2s)
    norm_I = (inp["body_inertia"].astype(np.float64) / inp["body_mass"].astype(np.float64)[:, None, None]).astype(np.float32)
    inv_norm_I = np.linalg.inv(norm_I.astype(np.float64)).astype(np.float32)
    wrt = ("q_init", "qd_init", "body_mass")

    def run(as_tensor, rollout, cent):
        t = {k: as_tensor(inp[k]) for k in INPUT_NAMES}
        for k in wrt:
            t[k].requires_grad_(True)
        m, N, iN = t["body_mass"], as_tensor(norm_I), as_tensor(inv_norm_I)
        t["body_inv_mass"], t["body_inertia"], t["body_inv_inertia"] = 1.0 / m, N * m[:, None, None], iN / m[:, None, None]
        pos, vel = rollout(t)
        out = cent(pos.reshape(F, bs, nb, 7), vel.reshape(F, bs, nb, 6), m.view(bs, nb), t["body_inertia"].view(bs, nb, 3, 3))
        loss = (out[..., SLICES["com"]] ** 2).sum() + (out[..., SLICES["momentum"]] ** 2).sum() + (out[..., SLICES["angular_momentum"]] ** 2).sum()
        loss.backward()
        return {k: t[k].grad.detach().cpu().numpy() for k in wrt}

    env = sim.Model.from_template(tpl, bs, dev)
    host = _Host(env, bs, T, f2s, inp["dt"])
    got = run(lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev),
              lambda t: dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], host),
              lambda q, qd, m, I: torch.cat([v.reshape(F, bs, -1) for v in dp_utils.centroidal(q, qd, m, I, env)], -1))

    def oracle(dtype):
        T_ = oracle_template(tpl, dtype)
        com, grav = template_constants(tpl, dtype)

        def rollout(t):
            allq, allqd = rt.rollout(T_, *[t[k] for k in INPUT_NAMES], T, f2s, inp["dt"], return_all=True)
            return allq[f2s], allqd[f2s]
        return run(lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).clone(), rollout,
                   lambda q, qd, m, I: centroidal(q, qd, m.expand(F, bs, nb), I.expand(F, bs, nb, 3, 3), com, grav))

    r64, r32 = oracle(torch.float64), oracle(torch.float32)
    for k in wrt:
        assert np.abs(r64[k]).max() > 0, k
        check("d centroidal loss / d " + k, got[k], r32[k], r64[k], CAPS[name][3])


QUERY_KEYS = {"sim_traj", "target_traj", "control_ref", "vertex_body", "sim_poses", "target_poses", "control_ref_poses", "com", "com_k",
              "body_mass", "grf", "jaf", "max_w"}   # what query() returns without a flag


def test_query_returns_the_simulated_centroidal_quantities(dev):
    import importlib.util
    import os

    from diffphys_amd import dp_utils
    from diffphys_amd.dataloader import DataLoader
    from diffphys_amd.phys_model import phys_model
    from helpers import ROOT

    spec = importlib.util.spec_from_file_location("pd_main_ct", os.path.join(ROOT, "ppr-diffphys_amd", "main.py"))
    pd_main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pd_main)
    opts = pd_main.get_opts(["--seqname", "mi-pace", "--urdf_template", "laikago", "--logroot", "/tmp/pprdp_test_log/", "--logname", "ct",
                             "--num_envs", "8", "--frames_per_wdw", "4"])
    torch.manual_seed(0)
    np.random.seed(0)
    model = phys_model(opts, DataLoader(opts)).cuda()
    model.train()
    model.reinit_envs(opts["num_envs"], frames_per_wdw=opts["frames_per_wdw"])
    model.set_progress(0)
    with torch.no_grad():
        model.body_mass.mul_(torch.linspace(0.8, 1.25, model.body_mass.numel(), device=model.body_mass.device))   # "learned" masses
    model.forward(frame_start=torch.arange(8, device=model.device) * 3)
    plain = model.query()
    assert set(plain) == QUERY_KEYS
    q = model.query(centroidal=True)
    assert set(q) == QUERY_KEYS | {"sim_centroidal"}
    for k in QUERY_KEYS - {"com_k", "max_w"}:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(q[k])), k
    sc = q["sim_centroidal"]
    assert tuple(sc) == NAMES
    for k in NAMES:
        assert isinstance(sc[k], np.ndarray) and sc[k].shape == ((4,) if k in ("mass", "kinetic", "potential") else (4, 3)), k
    up = lambda frames: torch.from_numpy(np.ascontiguousarray(np.stack(list(frames), 0), dtype=np.float32)).to(dev)
    mass = model.body_mass.detach().float()
    direct = dp_utils.centroidal(up(model.sim_trajs), up(model.sim_vels), mass, model.norm_body_inertia.detach().float() * mass[:, None, None],
                                 model.env)
    for k, v in zip(NAMES, direct):
        assert np.array_equal(sc[k], v.cpu().numpy()), k
    np.testing.assert_allclose(sc["mass"], float(mass.double().sum()), rtol=1e-6)   # the learned masses, not the template's
    assert abs(float(mass.double().sum()) - float(np.asarray(model.template["body_mass"], np.float64).sum())) > 1e-3
    model.sim_vels = None
    with pytest.raises(RuntimeError, match="sim_vels"):
        model.query(centroidal=True)


def test_the_op_inside_a_captured_graph(dev):
    """Neither entry allocates through HIP or synchronises: forward and VJP captured once on ONE stream (a single chain, no parallel
    branches), replayed twice on new inputs: eager's bits."""
    from diffphys_amd import hip_backend

    C = case("mixed25", "fk")
    nb, S = C["nb"], C["S"]
    table = gpu_mass_table("mixed25")
    rows = rows23(C["bq"], C["bqd"], C["mass"], C["inertia"], dev)
    gen = torch.Generator().manual_seed(5)
    g_out = torch.randn(S, 16, generator=gen).to(dev)

    def run(r, g):
        return hip_backend.centroidal(table, nb, r), hip_backend.centroidal_vjp(table, nb, r, g)

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
    for trial in range(2):
        fresh = rows * (1.0 + 0.01 * (trial + 1))
        g2 = torch.randn(S, 16, generator=gen).to(dev)
        rbuf.copy_(fresh); gbuf.copy_(g2)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(cap, run(fresh, g2)):
            assert torch.equal(got, want), trial
    assert not torch.equal(cap[0], run(rows, g_out)[0])
