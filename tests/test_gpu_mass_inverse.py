"""The mass-matrix inverse of a state applied to a joint-space vector (``pd_pose_op`` PD_POSE_MASS_INVERSE, k_mass_inverse of
csrc/pd_pose.hip, dp_model.MassInverse, dp_utils.mass_inverse / mass_matrix_inverse / forward_dynamics(method="articulated")) on a real
MI355X (run with -m gpu).

Reference: tests/mass_inverse_ref.py, the float64 torch restatement of the articulated-body recursion (held to the dense solve by
tests/test_mass_inverse_host.py), given the SAME fp32 rows as the GPU.  Bar (the project's, as tests/test_gpu_body_accel.py): the GPU's
error over max |reference| per tensor <= max(4 x the error of the fp32 torch evaluation of the same restatement, 1e-5); for a chain of
ops the fp32 torch chain is the yardstick.  Both numbers are printed.

Measured on one MI355X (error over max |reference|; GPU / fp32 torch): see DESIGN.md section 8.

The kernel evaluates the recursion in double on fp32 rows, frames and hand-overs (csrc/pd_pose.hip), so on the ill-conditioned robots
(human, rev64, freeleaf5) it is several times closer to float64 than the fp32 restatement, whose error there is the recursion's own
rounding."""
import functools

import numpy as np
import pytest
import torch

from body_accel_ref import rnea
from gpu_harness import dev  # noqa: F401
from helpers import relmax
from joint_coords_ref import oracle_template
from mass_inverse_ref import (ALL_CASES, RATES, accel_case, body_weights, g_out_of, inverse_of, mass_inverse, r_of, robot_template, rows23,
                              slot_index, slots_of, unslot)

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


def bar(what, gpu, f32, ref, floor=1e-5):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert np.isfinite(e_gpu) and e_gpu <= max(4 * e_32, floor), "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)


@functools.lru_cache(maxsize=None)
def restated(name, S, shift, rates, dtype, swapped=False):
    """the restatement's value on a case (swapped: on g_out_of in place of r_of): computed once, never written"""
    C = accel_case(name, S, shift)
    return inverse_of(C, dtype, rates, r6=g_out_of(C) if swapped else None)["out"]


@functools.lru_cache(maxsize=None)
def gpu_table(name, rates):
    from diffphys_amd import hip_backend

    return hip_backend.joint_table(robot_template(name), rates, torch.device("cuda:0"))


def launch(C, name, rates, dev, r6=None, rows=None):
    """-> out [S, nb, 6] as numpy"""
    from diffphys_amd import hip_backend

    nb = C["nb"]
    r = torch.from_numpy(rows23(C, r6) if rows is None else rows).to(dev)
    out = hip_backend.mass_inverse(gpu_table(name, rates), nb, r)
    assert out.shape == (r.shape[0], 6)
    return out.cpu().numpy().reshape(-1, nb, 6)


# ------------------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S,shift", ALL_CASES)
def test_op_matches_the_float64_restatement(name, S, shift, rates, dev):
    """H^-1 r of standard-normal force slots (every slot filled) against the float64 recursion on the same fp32 rows.  mixed25 (a body
    with 8 children), rev64 (depth 64), rev256 (the cap), freeleaf5 (a FREE joint below a body: it hands up zero inertia), worldmix9 /
    world5 (massless FIXED bases) and the far-shifted Laikago (the reference point) catch a wrong sweep, cap, hand-over or lever."""
    C = accel_case(name, S, shift)
    out = launch(C, name, rates, dev)
    bar("%s x %d%s %s out" % (name, S, " far" if shift else "", rates), out, restated(name, S, shift, rates, F32),
        restated(name, S, shift, rates, F64))
    unused = slot_index(C["tpl"]) == C["nqd"]   # a slot no dof uses: ignored on the way in (the rows fill it), exactly 0 on the way out
    assert (out[:, unused] == 0).all()
    if name == "mixed25":   # the body that gathers 8 children is in the comparison
        assert (np.asarray(C["tpl"]["joint_parent"]).reshape(-1) == 0).sum() == 8


# ------------------------------------------------------------------------------------------------------------ 2. symmetry
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S", [("laikago", 41), ("human", 3), ("mixed25", 11), ("rev64", 5), ("freeleaf5", 4)])
def test_op_is_self_adjoint(name, S, rates, dev):
    """<g, op(r)> = <r, op(g)> per state set (H is symmetric; the sums run over the slots in use): both against the float64 value of the
    pairing over sum |g op(r)|, the same pairings of the fp32 restatement as the yardstick."""
    C = accel_case(name, S)
    used = slot_index(C["tpl"]) != C["nqd"]
    r, g = r_of(C) * used, g_out_of(C) * used
    pair = lambda a, b: (np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum((1, 2))
    x64, y64 = restated(name, S, None, rates, F64), restated(name, S, None, rates, F64, True)
    want = pair(g, x64)
    scale = np.abs(np.asarray(g, np.float64) * x64).sum((1, 2))
    assert np.abs(want - pair(r, y64)).max() <= 1e-9 * scale.max()   # the restatement itself is symmetric
    x32, y32 = restated(name, S, None, rates, F32), restated(name, S, None, rates, F32, True)
    x, y = launch(C, name, rates, dev), launch(C, name, rates, dev, r6=g_out_of(C))
    err = lambda a, b: float(max((np.abs(pair(g, a) - want) / scale).max(), (np.abs(pair(r, b) - want) / scale).max()))
    e_gpu, e_32 = err(x, y), err(x32, y32)
    asym = float((np.abs(pair(g, x) - pair(r, y)) / scale).max())
    print("%s x %d %s pairing: GPU %.2e (asymmetry %.2e), fp32 torch %.2e" % (name, S, rates, e_gpu, asym, e_32))
    assert np.isfinite(e_gpu) and e_gpu <= max(4 * e_32, 1e-5) and asym <= max(4 * e_32, 1e-5)


# ------------------------------------------------------------------------------------------------------------ 3. autograd
def _draw(C, seed):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nqd"]).astype(np.float32)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name", ["laikago", "human", "cmp31"])
def test_gradients_through_dp_utils(name, rates, dev):
    """dp_utils.mass_inverse differentiated in body_q, tau, body_mass and body_inertia (the composed gradient: op 21 once more, op 17
    and its VJP) against float64 autograd of the restatement; masses and inertias are shared over the sets, so their gradients are the
    sums over the sets.  Yardstick: fp32 autograd of the restatement."""
    from diffphys_amd import dp_utils, sim

    S = 3
    C = accel_case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    tau, g = _draw(C, 61), _draw(C, 63)
    m32, I32 = body_weights(tpl, 1, F32)
    t = [torch.from_numpy(np.array(x)).to(dev).requires_grad_(True) for x in (C["bq"], tau, m32[0].numpy(), I32[0].numpy())]
    out = dp_utils.mass_inverse(t[0], t[1], t[2], t[3], env, rates=rates)
    assert out.shape == (S, nqd)
    (out * torch.from_numpy(g).to(dev)).sum().backward()
    assert t[1].grad.shape == (S, nqd) and t[2].grad.shape == (nb,) and t[3].grad.shape == (nb, 3, 3)

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        bq, r = (torch.tensor(np.array(v), dtype=dtype).requires_grad_(True) for v in (C["bq"], tau))
        m, I = (v.requires_grad_(True) for v in body_weights(tpl, S, dtype))
        o = unslot(tpl, mass_inverse(T, bq, m, I, slots_of(tpl, r), rates))
        (o * torch.tensor(g, dtype=dtype)).sum().backward()
        return [o.detach().numpy(), bq.grad.numpy(), r.grad.numpy(), m.grad.sum(0).numpy(), I.grad.sum(0).numpy()]

    c64, c32 = chain(F64), chain(F32)
    mine = [out.detach().cpu().numpy()] + [v.grad.cpu().numpy() for v in t]
    missed = []
    for k, what in enumerate(("out", "g_body_q", "g_tau", "g_body_mass", "g_body_inertia")):
        try:   # every figure is printed before the first miss ends the test
            bar("%s x %d %s %s" % (name, S, rates, what), mine[k], c32[k], c64[k])
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, "; ".join(missed)
    # tau alone: one launch in backward, the same slot gradient
    t2 = torch.from_numpy(tau).to(dev).requires_grad_(True)
    (dp_utils.mass_inverse(t[0].detach(), t2, t[2].detach(), t[3].detach(), env, rates=rates) * torch.from_numpy(g).to(dev)).sum().backward()
    assert torch.equal(t2.grad, t[1].grad)


# ------------------------------------------------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("name", ["laikago", "human"])
def test_forward_dynamics_and_the_rnea_round_trip(name, dev):
    """mass_inverse(rnea(qdd) - bias_forces) against qdd; forward_dynamics(method="articulated") and mass_matrix_inverse against the
    float64 chain of the restatements, the fp32 torch chain as the yardstick; method="dense" keeps the bits of the call without the
    keyword."""
    from diffphys_amd import dp_utils, sim

    S = 3
    C = accel_case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    qd, qdd, tau = _draw(C, 61), _draw(C, 63), _draw(C, 65)
    bq, jqd, jqdd, jtau = (torch.from_numpy(np.array(x)).to(dev) for x in (C["bq"], qd, qdd, tau))
    m32, I32 = body_weights(tpl, 1, F32)
    m, I = m32[0].to(dev), I32[0].to(dev)
    back = dp_utils.mass_inverse(bq, dp_utils.rnea(bq, jqd, jqdd, m, I, env) - dp_utils.bias_forces(bq, jqd, m, I, env), m, I, env)
    fd = dp_utils.forward_dynamics(bq, jqd, jtau, m, I, env, method="articulated")
    assert back.shape == (S, nqd) and fd.shape == (S, nqd)
    Hinv = dp_utils.mass_matrix_inverse(bq, m, I, env)
    assert Hinv.shape == (S, nqd, nqd)

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        q, v, a, f = (torch.tensor(np.array(x), dtype=dtype) for x in (C["bq"], qd, qdd, tau))
        mm, II = body_weights(tpl, S, dtype)
        solve = lambda r: unslot(tpl, mass_inverse(T, q, mm, II, slots_of(tpl, r), "generalized"))
        bias = rnea(T, tpl, q, v, None)
        eye = torch.eye(nqd, dtype=dtype)
        Hi = torch.stack([solve(eye[j].expand(S, nqd)) for j in range(nqd)], -1)
        return dict(back=solve(rnea(T, tpl, q, v, a) - bias).numpy(), fd=solve(f - bias).numpy(), Hinv=Hi.numpy())

    c64, c32 = chain(F64), chain(F32)
    bar(name + " mass_inverse(rnea(qdd) - bias_forces) against qdd", back.cpu().numpy(), c32["back"], qdd.astype(np.float64))
    bar(name + " forward_dynamics(articulated)", fd.cpu().numpy(), c32["fd"], c64["fd"])
    bar(name + " mass_matrix_inverse", Hinv.cpu().numpy(), c32["Hinv"], c64["Hinv"])
    dense = dp_utils.forward_dynamics(bq, jqd, jtau, m, I, env)
    assert torch.equal(dense, dp_utils.forward_dynamics(bq, jqd, jtau, m, I, env, method="dense"))
    print("%s forward_dynamics dense: %.2e of max" % (name, relmax(dense.cpu().numpy(), c64["fd"])))
    tq = jtau.clone().requires_grad_(True)   # ... and the articulated chain back-propagates
    dp_utils.forward_dynamics(bq, jqd, tq, m, I, env, method="articulated").sum().backward()
    assert tq.grad is not None and torch.isfinite(tq.grad).all() and float(tq.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 5. bits and edges
@pytest.mark.parametrize("rates", RATES)
def test_a_sets_bits_depend_on_nothing_but_the_set(rates, dev):
    """Sets 0 and 40 of the 41-set launch evaluated alone, and everything a second time: equal bits."""
    name = "laikago"
    C = accel_case(name, 41)
    nb = C["nb"]
    out = launch(C, name, rates, dev)
    assert np.array_equal(out, launch(C, name, rates, dev))
    for s in (0, 40):
        alone = launch(C, name, rates, dev, rows=rows23(C)[s * nb: (s + 1) * nb])
        assert np.array_equal(alone[0], out[s]), s


def test_a_table_of_another_nb_gives_zeros(dev):
    """The library cannot validate a device buffer: the kernel checks the table's nb against the call's and writes zeros (no row of
    the table is read)."""
    from diffphys_amd import hip_backend

    C = accel_case("cmp31", 3)
    wrong = gpu_table("mixed25", "measured").clone()   # 4 + 32 * 25 floats: shorter than the table of 31 bodies
    _, (nb25, nq25, nqd25) = hip_backend._table_tag(gpu_table("mixed25", "measured"))
    assert nb25 == 25
    wrong._pd_table = ("joint", (31, nq25, nqd25))   # ... passed off as one
    out = hip_backend.mass_inverse(wrong, 31, torch.from_numpy(rows23(C)).to(dev))
    assert out.shape == (93, 6) and (out == 0).all()


def test_empty_and_graph_capture(dev):
    """n = 0; the op captured in a HIP graph replays eager's bits on new inputs."""
    from diffphys_amd import hip_backend

    name = "human"
    C = accel_case(name, 3)
    nb = C["nb"]
    table = gpu_table(name, "measured")
    assert hip_backend.mass_inverse(table, nb, torch.zeros(0, 23, device=dev)).shape == (0, 6)
    rows = torch.from_numpy(rows23(C)).to(dev)
    rbuf = rows.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_backend.mass_inverse(table, nb, rbuf)   # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = hip_backend.mass_inverse(table, nb, rbuf)
    torch.cuda.current_stream().wait_stream(side)
    fresh = rows.clone()
    fresh[:, 17:] = torch.randn(rows.shape[0], 6, generator=torch.Generator().manual_seed(7)).to(dev)
    rbuf.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, hip_backend.mass_inverse(table, nb, fresh))
