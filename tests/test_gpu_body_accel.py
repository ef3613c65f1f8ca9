"""The accelerations of the bodies of a state (``pd_pose_op`` PD_POSE_BODY_ACCEL, k_body_accel_fwd / _vjp of csrc/pd_pose.hip,
dp_model.BodyAccelerations, dp_utils.body_accelerations / newton_euler_wrench / rnea / bias_forces / forward_dynamics) on a real
MI355X (run with -m gpu).

Reference: tests/body_accel_ref.py, the float64 torch restatement (held to finite differences and identities by
tests/test_body_accel_host.py), given the SAME fp32 rows as the GPU.  Bar (the project's, as tests/test_gpu_body_twists.py): the GPU's
error over max |reference| per tensor <= max(4 x the error of the fp32 torch evaluation of the same restatement, 1e-5); for a chain of
ops the fp32 torch chain is the yardstick.  Both numbers are printed.

Measured on one MI355X (error over max |reference|; GPU / fp32 torch): see DESIGN.md section 8."""
import functools

import numpy as np
import pytest
import torch

from body_accel_ref import (CASES, RATES, TENSORS, accel_case, accel_of, body_accelerations, body_twists, g_out_of, generalized_force,
                            inertia_of, mass_matrix, rnea, robot_template, rows19, slot_index, slots_of)
from gpu_harness import dev  # noqa: F401
from helpers import relmax
from joint_coords_ref import oracle_template

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
ALL_CASES = CASES + [("freeleaf5", 4, None)]   # + the one robot whose FREE joint has a parent


def bar(what, gpu, f32, ref, floor=1e-5):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert np.isfinite(e_gpu) and e_gpu <= max(4 * e_32, floor), "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)


@functools.lru_cache(maxsize=None)
def restated(name, S, shift, rates, dtype):
    """value and gradients of the restatement on a case, with the standard-normal g_out every test uses: computed once, never written"""
    C = accel_case(name, S, shift)
    return accel_of(C, dtype, rates, g_out_of(C))


@functools.lru_cache(maxsize=None)
def gpu_table(name, rates):
    from diffphys_amd import hip_backend

    return hip_backend.joint_table(robot_template(name), rates, torch.device("cuda:0"))


def launch(C, name, rates, dev, g_out=None, rows=None):
    """-> (out [S, nb, 6], g_rows [S, nb, 19] or None) as numpy"""
    from diffphys_amd import hip_backend

    nb = C["nb"]
    r = torch.from_numpy(rows19(C) if rows is None else rows).to(dev)
    S = r.shape[0] // nb
    out = hip_backend.body_accelerations(gpu_table(name, rates), nb, r)
    assert out.shape == (S * nb, 6)
    g = None
    if g_out is not None:
        go = torch.from_numpy(np.ascontiguousarray(g_out, np.float32).reshape(-1, 6)).to(dev)
        g = hip_backend.body_accelerations_vjp(gpu_table(name, rates), nb, r, go)
        assert g.shape == (S * nb, 19)
        g = g.cpu().numpy().reshape(S, nb, 19)
    return out.cpu().numpy().reshape(S, nb, 6), g


# ------------------------------------------------------------------------------------------------------------ 1. values and VJP
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S,shift", ALL_CASES)
def test_op_and_vjp_match_the_float64_restatement(name, S, shift, rates, dev):
    """Value and g_rows of a standard-normal g_out against the float64 restatement and its autograd on the same fp32 rows (jittered
    poses, standard-normal twists and slot derivatives).  mixed25 (a body with 8 children), rev64 (depth 64), rev256 (the cap), the
    far-shifted Laikago and freeleaf5 (a FREE joint below a body) catch a wrong sweep, cap, reference point or parent-side hand-over."""
    C = accel_case(name, S, shift)
    g_out = g_out_of(C)
    out, g = launch(C, name, rates, dev, g_out)
    r64, r32 = restated(name, S, shift, rates, F64), restated(name, S, shift, rates, F32)
    tag = "%s x %d%s %s " % (name, S, " far" if shift else "", rates)
    mine = dict(out=out, g_body_q=g[..., :7], g_body_qd=g[..., 7:13], g_acc=g[..., 13:])
    for k in TENSORS:
        if np.abs(r64[k]).max() == 0:
            # free1: one FREE body of the world with its com at its origin -- a = R_wj s_3..5 (w x v leaves through e_i), no pose and no
            # twist enters and both gradients are 0; the op adds and subtracts terms up to |v| |g| ~ 16: 8 fp32 ulps of that
            assert name == "free1" and k in ("g_body_q", "g_body_qd") and np.abs(mine[k]).max() <= 8 * 1.2e-7 * 16
            continue
        bar(tag + k, mine[k], r32[k], r64[k])
    unused = slot_index(C["tpl"]) == C["nqd"]   # a slot no dof uses: ignored by the value (the rows fill it), zero in the gradient
    assert (mine["g_acc"][:, unused] == 0).all()
    if name == "mixed25":   # the body that gathers 8 children is in the comparison
        assert (np.asarray(C["tpl"]["joint_parent"]).reshape(-1) == 0).sum() == 8


# ------------------------------------------------------------------------------------------------------------ 2. a set's bits
@pytest.mark.parametrize("rates", RATES)
def test_a_sets_bits_depend_on_nothing_but_the_set(rates, dev):
    """Sets 0 and 40 of the 41-set launch evaluated alone, and everything a second time: equal bits, value and VJP."""
    name = "laikago"
    C = accel_case(name, 41)
    nb = C["nb"]
    g_out = g_out_of(C)
    out, g = launch(C, name, rates, dev, g_out)
    again = launch(C, name, rates, dev, g_out)
    assert np.array_equal(out, again[0]) and np.array_equal(g, again[1])
    for s in (0, 40):
        alone = launch(C, name, rates, dev, g_out[s: s + 1], rows=rows19(C)[s * nb: (s + 1) * nb])
        assert np.array_equal(alone[0][0], out[s]) and np.array_equal(alone[1][0], g[s]), s


# ------------------------------------------------------------------------------------------------------------ 3. edges
def test_a_table_of_another_nb_gives_zeros(dev):
    """The library cannot validate a device buffer: the kernels check the table's nb against the call's and write zeros (no row of
    the table is read)."""
    from diffphys_amd import hip_backend

    C = accel_case("cmp31", 3)
    wrong = gpu_table("mixed25", "measured").clone()   # 4 + 32 * 25 floats: shorter than the table of 31 bodies
    _, (nb25, nq25, nqd25) = hip_backend._table_tag(gpu_table("mixed25", "measured"))
    assert nb25 == 25
    wrong._pd_table = ("joint", (31, nq25, nqd25))   # ... passed off as one
    rows = torch.from_numpy(rows19(C)).to(dev)
    out = hip_backend.body_accelerations(wrong, 31, rows)
    g = hip_backend.body_accelerations_vjp(wrong, 31, rows, torch.ones(93, 6, device=dev))
    assert out.shape == (93, 6) and g.shape == (93, 19)
    assert (out == 0).all() and (g == 0).all()


def test_empty_and_graph_capture(dev):
    """n = 0; forward and VJP captured in a HIP graph replay eager's bits on new inputs."""
    from diffphys_amd import hip_backend

    name = "human"
    C = accel_case(name, 3)
    nb = C["nb"]
    table = gpu_table(name, "measured")
    empty = torch.zeros(0, 19, device=dev)
    assert hip_backend.body_accelerations(table, nb, empty).shape == (0, 6)
    assert hip_backend.body_accelerations_vjp(table, nb, empty, torch.zeros(0, 6, device=dev)).shape == (0, 19)
    rows = torch.from_numpy(rows19(C)).to(dev)
    g_out = torch.from_numpy(g_out_of(C).reshape(-1, 6)).to(dev)
    run = lambda r, g: (hip_backend.body_accelerations(table, nb, r), hip_backend.body_accelerations_vjp(table, nb, r, g))
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


# ------------------------------------------------------------------------------------------------------------ 4. autograd
def _draw(C, seed):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nqd"]).astype(np.float32)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name", ["laikago", "human"])
def test_through_autograd_with_body_twists(name, rates, dev):
    """dp_utils.body_accelerations(bq, dp_utils.body_twists(bq, qd), qdd) differentiated in bq, qd and qdd against the float64 chain of
    the two restatements; yardstick: the fp32 torch chain."""
    from diffphys_amd import dp_utils, sim

    S = 3
    C = accel_case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    qd, qdd, g = _draw(C, 61), _draw(C, 63), g_out_of(C)
    t = [torch.from_numpy(np.array(x)).to(dev).requires_grad_(True) for x in (C["bq"], qd, qdd)]
    out = dp_utils.body_accelerations(t[0], dp_utils.body_twists(t[0], t[1], env, rates=rates), t[2], env, rates=rates)
    assert out.shape == (S, nb, 6)
    (out * torch.from_numpy(g).to(dev)).sum().backward()
    assert t[1].grad.shape == (S, nqd) and t[2].grad.shape == (S, nqd)

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        x = [torch.tensor(np.array(v), dtype=dtype).requires_grad_(True) for v in (C["bq"], qd, qdd)]
        o = body_accelerations(T, x[0], body_twists(T, x[0], slots_of(tpl, x[1]), rates), slots_of(tpl, x[2]), rates)
        (o * torch.tensor(g, dtype=dtype)).sum().backward()
        return [o.detach().numpy()] + [v.grad.numpy() for v in x]

    c64, c32 = chain(F64), chain(F32)
    mine = [out.detach().cpu().numpy()] + [v.grad.cpu().numpy() for v in t]
    for k, what in enumerate(("out", "g_body_q", "g_joint_qd", "g_joint_qdd")):
        bar("%s x %d %s chain %s" % (name, S, rates, what), mine[k], c32[k], c64[k])


# ------------------------------------------------------------------------------------------------------------ 5. composition
@pytest.mark.parametrize("name", ["laikago", "human"])
def test_rnea_bias_forces_and_forward_dynamics(name, dev):
    """rnea(qdd) - bias_forces against mass_matrix @ qdd; forward_dynamics(rnea(qdd)) against qdd; rnea at rest against generalized_force
    of the gravity wrench.  Each against float64, the bar 4 x the same chain evaluated with the fp32 torch restatements."""
    from diffphys_amd import dp_utils, sim

    S = 3
    C = accel_case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    qd, qdd = _draw(C, 61), _draw(C, 63)
    bq, jqd, jqdd = (torch.from_numpy(np.array(x)).to(dev) for x in (C["bq"], qd, qdd))
    m = torch.from_numpy(np.asarray(tpl["body_mass"], np.float32).reshape(nb)).to(dev)
    I = torch.from_numpy(np.asarray(tpl["body_inertia"], np.float32).reshape(nb, 3, 3)).to(dev)
    tau = dp_utils.rnea(bq, jqd, jqdd, m, I, env)
    bias = dp_utils.bias_forces(bq, jqd, m, I, env)
    assert tau.shape == (S, nqd) and bias.shape == (S, nqd)
    Hq = (dp_utils.mass_matrix(bq, m, I, env) @ jqdd[..., None])[..., 0]
    back = dp_utils.forward_dynamics(bq, jqd, tau, m, I, env)
    rest = dp_utils.rnea(bq, torch.zeros_like(jqd), None, m, I, env)
    gravity_f = torch.cat([torch.zeros(S, nb, 3, device=dev),
                           -m[None, :, None] * torch.tensor([float(x) for x in tpl["gravity"]], device=dev).expand(S, nb, 3)], -1)
    rest_gf = dp_utils.generalized_force(bq, gravity_f.contiguous(), env, efforts="generalized")

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        q, v, a = (torch.tensor(np.array(x), dtype=dtype) for x in (C["bq"], qd, qdd))
        mass, _, gravity = inertia_of(tpl, dtype)
        t, b = rnea(T, tpl, q, v, a), rnea(T, tpl, q, v, None)
        H = mass_matrix(T, tpl, q)
        gf = torch.cat([torch.zeros(S, nb, 3, dtype=dtype), (-mass[:, None] * gravity).expand(S, nb, 3)], -1)
        return dict(diff=(t - b).numpy(), Hq=(H @ a[..., None])[..., 0].numpy(), back=torch.linalg.solve(H, (t - b)[..., None])[..., 0].numpy(),
                    rest=rnea(T, tpl, q, torch.zeros_like(v), None).numpy(), rest_gf=generalized_force(T, q, gf, "generalized").numpy())

    c64, c32 = chain(F64), chain(F32)
    bar(name + " rnea(qdd) - bias_forces against H qdd", (tau - bias).cpu().numpy(), c32["diff"], c64["Hq"])
    bar(name + " mass_matrix @ qdd", Hq.cpu().numpy(), c32["Hq"], c64["Hq"])
    bar(name + " forward_dynamics(rnea(qdd)) against qdd", back.cpu().numpy(), c32["back"], qdd.astype(np.float64))
    bar(name + " rnea at rest against generalized_force of gravity", rest.cpu().numpy(), c32["rest"], c64["rest_gf"])
    bar(name + " generalized_force of gravity", rest_gf.cpu().numpy(), c32["rest_gf"], c64["rest_gf"])
    tq = jqdd.clone().requires_grad_(True)   # ... and the chain back-propagates
    dp_utils.rnea(bq, jqd, tq, m, I, env).sum().backward()
    assert tq.grad is not None and torch.isfinite(tq.grad).all() and float(tq.grad.abs().max()) > 0
