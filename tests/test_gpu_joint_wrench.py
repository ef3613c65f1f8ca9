"""The joint wrench of body states (``pd_pose_op`` PD_POSE_JOINT_WRENCH, k_joint_wrench_fwd / k_joint_wrench_vjp of csrc/pd_pose.hip,
dp_model.JointWrench, dp_utils.joint_wrench) on a real MI355X (run with -m gpu).

Reference: tests/joint_wrench_ref.py, the float64 torch restatement of the oracle's eval_body_joints in the stable forms (held to the
oracle by tests/test_joint_wrench_host.py, which also asserts the input conditions of every case), given the SAME fp32 rows as the GPU.
Bar (the project's, as tests/test_gpu_joint_coords.py): the GPU's error over max |reference| per tensor <= max(4 x the error of the fp32
torch evaluation of the same restatement, 1e-5); against the rollout's own jaf twice that bar (both are fp32 evaluations of one function
on identical fp32 inputs).  Both numbers are printed.

Measured on one MI355X (error over max |reference|; GPU / fp32 torch): see DESIGN.md section 8."""
import functools

import numpy as np
import pytest
import torch

from gpu_harness import dev, dev_inputs  # noqa: F401
from helpers import INPUT_NAMES, relmax, tight_inputs
from joint_coords_ref import oracle_template
from joint_wrench_ref import CASES, TENSORS, case, dof_grads, joint_wrench, rows25, slot_index, template, unused_slots, wrench_of

pytestmark = pytest.mark.gpu
F64 = torch.float64


def bar(what, gpu, f32, ref, floor=1e-5, factor=1.0):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert np.isfinite(e_gpu) and e_gpu <= factor * max(4 * e_32, floor), "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)
    return factor * max(4 * e_32, floor)


def g_out_of(C, seed=31):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


@functools.lru_cache(maxsize=None)
def restated(name, S, kind, dtype):
    """value and gradients of the restatement on a case, with the standard-normal g_out every test uses: computed once, never written"""
    C = case(name, S, kind)
    return wrench_of(C, dtype, g_out_of(C))


@functools.lru_cache(maxsize=None)
def gpu_table(name):
    from diffphys_amd import hip_backend

    return hip_backend.joint_force_table(template(name), torch.device("cuda:0"))


def launch(C, name, dev, g_out=None, rows=None):
    """-> (out [S, nb, 6], g_rows [S, nb, 25] or None) as numpy"""
    from diffphys_amd import hip_backend

    S, nb = C["bq"].shape[0], C["nb"]
    r = torch.from_numpy(rows25(C) if rows is None else rows).to(dev)
    out = hip_backend.joint_wrench(gpu_table(name), nb, r)
    assert out.shape == (S * nb, 6)
    g = None
    if g_out is not None:
        g = hip_backend.joint_wrench_vjp(gpu_table(name), nb, r, torch.from_numpy(np.ascontiguousarray(g_out, np.float32).reshape(-1, 6)).to(dev))
        assert g.shape == (S * nb, 25)
        g = g.cpu().numpy().reshape(S, nb, 25)
    return out.cpu().numpy().reshape(S, nb, 6), g


@pytest.mark.parametrize("name,S,kind", CASES)
def test_values_match_the_float64_restatement(name, S, kind, dev):
    C = case(name, S, kind)
    out, _ = launch(C, name, dev)
    r64, r32 = restated(name, S, kind, F64), restated(name, S, kind, torch.float32)
    if name == "free1":
        assert (out == 0).all() and (r64["out"] == 0).all()
        return
    bar("%s x %d %s out" % (name, S, kind), out, r32["out"], r64["out"])
    par = np.asarray(C["tpl"]["joint_parent"]).reshape(-1)
    if name == "mixed25":   # the body that gathers 8 children is in the comparison
        assert (par == 0).sum() == 8 and np.abs(r64["out"][:, 0]).max() > 0


@pytest.mark.parametrize("name,S,kind", CASES)
def test_vjp_matches_float64_autograd(name, S, kind, dev):
    """g_rows of a standard-normal g_out -- the parent-side gather included -- against float64 autograd of the restatement: the state's
    raw partials and the four control gradients (scattered back to their dofs); the slots no dof uses are written as 0."""
    C = case(name, S, kind)
    g_out = g_out_of(C)
    _, g = launch(C, name, dev, g_out)
    _, again = launch(C, name, dev, g_out)
    assert np.array_equal(g, again)   # fixed summation order: the same bits
    assert (g[..., 13:][:, unused_slots(C["tpl"])] == 0).all()
    r64, r32 = restated(name, S, kind, F64), restated(name, S, kind, torch.float32)
    if name == "free1":
        assert (g == 0).all()
        return
    tag = "%s x %d %s " % (name, S, kind)
    mine = dict(g_body_q=g[..., :7], g_body_qd=g[..., 7:13], **dof_grads(C["tpl"], g))
    for k in TENSORS[1:]:
        assert np.abs(r64[k]).max() > 0, k
        bar(tag + k, mine[k], r32[k], r64[k])


class _Host:
    """the attributes the ForwardWarp family reads from ``self``"""

    def __init__(self, env, bs, nsteps, frame2step, dt):
        self.env, self.num_envs, self.steps_idx, self.frame2step, self.dt = env, bs, range(nsteps), list(frame2step), dt


def _rollout_inputs(name, tpl, bs, T, f2s):
    from generated_robots import rollout_inputs

    inp = tight_inputs(tpl, name, bs, T, seed=5) if name in ("laikago", "human") else rollout_inputs(tpl, bs=bs, T=T, seed=3)
    inp["frame2step"] = list(f2s)
    return inp


@pytest.mark.parametrize("name", ["laikago", "human", "mixed25"])
def test_the_op_reproduces_the_rollouts_jaf(name, dev):
    """A rollout of T = 8 with frames at states 0, T / 2 and T - 1: the op on (wp_pos[f], wp_vel[f]) and the step's controls against the
    jaf the rollout reports for that frame, under TWICE the op's own bar against float64."""
    from diffphys_amd import hip_backend

    tpl = template(name)
    bs, T, f2s = 4, 8, [0, 4, 7]
    nb, nqd, F = int(tpl["nb"]), int(tpl["nqd"]), 3
    inp = _rollout_inputs(name, tpl, bs, T, f2s)
    t = dev_inputs(inp, dev)
    dm = hip_backend.DeviceModel(tpl)
    pos, vel, grf, jaf, _ = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in hip_backend.ROLLOUT_INPUTS], frame2step=f2s)
    bq, bqd = pos.cpu().numpy().reshape(F * bs, nb, 7), vel.cpu().numpy().reshape(F * bs, nb, 6)
    step = lambda k: np.concatenate([np.asarray(inp[k], np.float32).reshape(T, bs, nqd)[s] for s in f2s], 0)
    gain = lambda k: np.tile(np.asarray(inp[k], np.float32).reshape(bs, nqd), (F, 1))
    C = dict(tpl=tpl, nb=nb, nqd=nqd, bq=bq, bqd=bqd, target=step("refs"), act=step("torques"), ke=gain("target_ke"), kd=gain("target_kd"))
    out, _ = launch(C, name, dev)
    r64, r32 = wrench_of(C, F64)["out"], wrench_of(C, torch.float32)["out"]
    own = bar("%s op on the rollout's frames" % name, out, r32, r64)
    jaf = jaf.cpu().numpy().reshape(F * bs, nb, 6)
    assert np.abs(jaf).max() > 0
    d = relmax(out, jaf)
    print("%s op against the rollout's jaf: %.2e (bar %.2e)" % (name, d, 2 * own))
    assert d <= 2 * own


def test_a_fixed_joint_at_the_exact_identity(dev):
    """laikago_toes with a toe and its shank both at the identity quaternion (the toes' joint frames are unrotated): r_err = (0, 0, 0, 1)
    exactly.  Forward finite and equal to the linear and damping parts alone, VJP finite and on the bar."""
    name = "laikago_toes"
    C = dict(case(name, 2))
    tpl = C["tpl"]
    ty, par = np.asarray(tpl["joint_type"]).reshape(-1), np.asarray(tpl["joint_parent"]).reshape(-1)
    toe = int(np.flatnonzero(ty == 3)[0])
    assert np.array_equal(np.asarray(tpl["joint_X_p"], np.float32).reshape(-1, 7)[toe, 3:], [0, 0, 0, 1])
    bq = C["bq"].copy()
    bq[:, [toe, par[toe]], 3:] = np.asarray([0, 0, 0, 1], np.float32)
    C["bq"] = bq
    g_out = g_out_of(C)
    out, g = launch(C, name, dev, g_out)
    assert np.isfinite(out).all() and np.isfinite(g).all()
    r64, r32 = wrench_of(C, F64, g_out), wrench_of(C, torch.float32, g_out)
    without = wrench_of(C, F64, drop_fixed_angle=True)["out"]
    assert np.array_equal(r64["out"][:, toe], without[:, toe])   # the angular spring of that toe is exactly 0
    b = bar("identity toe out", out, r32["out"], r64["out"])
    assert np.abs(out[:, toe] - without[:, toe]).max() <= b * np.abs(r64["out"]).max()
    mine = dict(g_body_q=g[..., :7], g_body_qd=g[..., 7:13], **dof_grads(tpl, g))
    for k in TENSORS[1:]:
        bar("identity toe " + k, mine[k], r32[k], r64[k])


def test_a_compound_joint_on_its_clamp(dev):
    """cmp31 with a gain of 4e5 on the joints of bodies 1 .. 3: all three torque components of those joints sit on the +-1e4 clamp (asserted
    in float64, none within 1e-3 relative of it) -- their control gradients are EXACTLY 0; everything else meets the bar."""
    from joint_wrench_ref import joint_pairs_raw

    name = "cmp31"
    C = dict(case(name, 3))
    tpl, nqd = C["tpl"], C["nqd"]
    idx = slot_index(tpl)
    hot = idx[1:4].reshape(-1)
    assert (hot < nqd).all()
    ke = C["ke"].copy()
    ke[:, hot] = 4.0e5
    C["ke"] = ke
    T = oracle_template(tpl)
    c64 = {k: torch.tensor(np.array(C[k]), dtype=F64) for k in ("target", "act", "ke", "kd")}
    raw = joint_pairs_raw(T, torch.tensor(np.array(C["bq"]), dtype=F64), torch.tensor(np.array(C["bqd"]), dtype=F64), c64)   # bodies 1 .. nb - 1
    assert np.abs(np.abs(raw) / 1.0e4 - 1.0).min() >= 1e-3
    full = (np.abs(raw[:3, :, :3]) > 1.0e4).all(-1)   # [joint, set]: all three torque components clamped
    assert full.any() and not (np.abs(raw[3:, :, :3]) > 1.0e4).any()
    g_out = g_out_of(C)
    out, g = launch(C, name, dev, g_out)
    for j in range(3):
        for s in range(3):
            if full[j, s]:
                assert (g[s, 1 + j, 13:] == 0).all(), (j, s)
    r64, r32 = wrench_of(C, F64, g_out), wrench_of(C, torch.float32, g_out)
    bar("clamped out", out, r32["out"], r64["out"])
    mine = dict(g_body_q=g[..., :7], g_body_qd=g[..., 7:13], **dof_grads(tpl, g))
    for k in TENSORS[1:]:
        bar("clamped " + k, mine[k], r32[k], r64[k])


def test_unused_slots_and_nan_rows(dev):
    """mixed25: NaN in every control slot no dof uses changes no output bit and no gradient bit, and those slots' gradients are 0; a NaN
    state row disturbs its own set only."""
    name = "mixed25"
    C = case(name, 11)
    g_out = g_out_of(C)
    out, g = launch(C, name, dev, g_out)
    out_n, g_n = launch(C, name, dev, g_out, rows=rows25(C, fill=np.nan))
    assert np.array_equal(out, out_n) and np.array_equal(g, g_n)
    un = unused_slots(C["tpl"])
    assert un.any() and (g_n[..., 13:][:, un] == 0).all()
    rows = rows25(C).reshape(11, C["nb"], 25).copy()
    rows[4, 7, :13] = np.nan
    out_s, g_s = launch(C, name, dev, g_out, rows=rows.reshape(-1, 25))
    keep = [s for s in range(11) if s != 4]
    assert np.array_equal(out_s[keep], out[keep]) and np.array_equal(g_s[keep], g[keep])
    assert np.isnan(out_s[4]).any()


def test_empty_single_set_graph_and_repeat(dev):
    """n = 0; one set; forward and VJP captured in a HIP graph replay eager's bits on new inputs; two runs give equal bits."""
    from diffphys_amd import hip_backend

    name = "human"
    C = case(name, 3)
    nb = C["nb"]
    table = gpu_table(name)
    empty = torch.zeros(0, 25, device=dev)
    assert hip_backend.joint_wrench(table, nb, empty).shape == (0, 6)
    assert hip_backend.joint_wrench_vjp(table, nb, empty, torch.zeros(0, 6, device=dev)).shape == (0, 25)
    rows = torch.from_numpy(rows25(C)).to(dev)
    g_out = torch.from_numpy(g_out_of(C).reshape(-1, 6)).to(dev)
    run = lambda r, g: (hip_backend.joint_wrench(table, nb, r), hip_backend.joint_wrench_vjp(table, nb, r, g))
    all3, first = run(rows, g_out), run(rows[:nb].contiguous(), g_out[:nb].contiguous())
    assert torch.equal(all3[0][:nb], first[0]) and torch.equal(all3[1][:nb], first[1])   # a set's bits do not depend on n
    for a, b in zip(all3, run(rows, g_out)):
        assert torch.equal(a, b)
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
    gen = torch.Generator().manual_seed(7)
    for trial in range(2):
        fresh = rows * (1.0 + 0.01 * (trial + 1))
        g2 = torch.randn(g_out.shape, generator=gen).to(dev)
        rbuf.copy_(fresh); gbuf.copy_(g2)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(cap, run(fresh, g2)):
            assert torch.equal(got, want), trial
    assert not torch.equal(cap[0], all3[0])


def test_gradients_through_the_rollout(dev):
    """loss = <w, joint_wrench(wp_pos, wp_vel, env, refs[s], target_ke, target_kd, torques[s])> behind ForwardWarp.apply (Laikago, 8 envs x
    3 steps, frames at states 0, 2, 3 -- the inputs and caps of tests/test_gpu_joint_coords.py::test_gradients_through_the_rollout)
    against float64 autograd of ref_torch.rollout composed with the restatement: q_init, refs and target_ke.  The last frame is state T:
    it takes the controls of step T - 1."""
    from diffphys_amd import dp_model, dp_utils, sim
    from oracle import ref_torch
    from test_gpu_ground_wrench import CAPS, check

    name, bs, T, f2s = "laikago", 8, 3, [0, 2, 3]
    tpl = template(name)
    nb, nqd, F = int(tpl["nb"]), int(tpl["nqd"]), 3
    inp = tight_inputs(tpl, name, bs, T, seed=5)
    inp["frame2step"] = f2s
    steps = [min(s, T - 1) for s in f2s]
    w = np.random.RandomState(41).randn(F, bs, nb, 6)
    env = sim.Model.from_template(tpl, bs, dev)
    t = dev_inputs(inp, dev)
    wrt = ("q_init", "refs", "target_ke")
    for k in wrt:
        t[k].requires_grad_(True)
    pos, vel = dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], _Host(env, bs, T, f2s, inp["dt"]))
    jw = dp_utils.joint_wrench(pos.view(F, bs, nb, 7), vel.view(F, bs, nb, 6), env, t["refs"].view(T, bs, nqd)[steps],
                               t["target_ke"].view(bs, nqd), t["target_kd"].view(bs, nqd), t["torques"].view(T, bs, nqd)[steps])
    assert jw.shape == (F, bs, nb, 6)
    (jw * torch.from_numpy(w.astype(np.float32)).to(dev)).sum().backward()

    def oracle(dtype):
        T_ = oracle_template(tpl, dtype)
        x = {k: torch.as_tensor(np.asarray(inp[k]), dtype=dtype).clone() for k in INPUT_NAMES}
        for k in wrt:
            x[k].requires_grad_(True)
        allq, allqd = ref_torch.rollout(T_, *[x[k] for k in INPUT_NAMES], T, f2s, inp["dt"], return_all=True)
        bq, bqd = allq[f2s].reshape(F * bs, nb, 7), allqd[f2s].reshape(F * bs, nb, 6)
        per_step = lambda k: x[k].view(T, bs, nqd)[steps].reshape(F * bs, nqd)
        gain = lambda k: x[k].view(1, bs, nqd).expand(F, bs, nqd).reshape(F * bs, nqd)
        out = joint_wrench(T_, bq, bqd, per_step("refs"), per_step("torques"), gain("target_ke"), gain("target_kd"))
        (out * torch.as_tensor(w.reshape(F * bs, nb, 6), dtype=dtype)).sum().backward()
        return {k: x[k].grad.numpy() for k in wrt}

    r64, r32 = oracle(F64), oracle(torch.float32)
    for k in wrt:
        assert np.abs(r64[k]).max() > 0, k
        check("d joint-wrench loss / d " + k, t[k].grad.cpu().numpy().reshape(r64[k].shape), r32[k], r64[k], CAPS[name][3])


def test_shared_gains_sum_their_gradient_over_the_sets(dev):
    """dp_utils.joint_wrench with target_ke [nqd] and target_kd [1] shared by 5 state sets, refs per set, no torques: the value is the
    restatement's on expanded gains, the gradient of a shared gain the SUM over the sets of the per-set gradient."""
    from diffphys_amd import dp_utils, sim

    name, S = "laikago", 5
    C = case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    g_out = g_out_of(C)
    ke1 = C["ke"][0].copy()
    shared = dict(C, ke=np.tile(ke1, (S, 1)), kd=np.full((S, nqd), np.float32(0.25)), act=np.zeros((S, nqd), np.float32))
    bq, bqd = torch.from_numpy(C["bq"].copy()).to(dev).requires_grad_(True), torch.from_numpy(C["bqd"].copy()).to(dev).requires_grad_(True)
    refs = torch.from_numpy(C["target"].copy()).to(dev).requires_grad_(True)
    ke = torch.from_numpy(ke1).to(dev).requires_grad_(True)
    kd = torch.full((1,), 0.25, device=dev).requires_grad_(True)
    out = dp_utils.joint_wrench(bq, bqd, env, refs, ke, kd)
    assert out.shape == (S, nb, 6)
    (out * torch.from_numpy(g_out).to(dev)).sum().backward()
    r64, r32 = wrench_of(shared, F64, g_out), wrench_of(shared, torch.float32, g_out)
    bar("shared gains out", out.detach().cpu().numpy(), r32["out"], r64["out"])
    bar("shared gains g_body_q", bq.grad.cpu().numpy(), r32["g_body_q"], r64["g_body_q"])
    bar("shared gains g_refs", refs.grad.cpu().numpy(), r32["g_target"], r64["g_target"])
    bar("shared gains g_target_ke", ke.grad.cpu().numpy(), r32["g_ke"].sum(0), r64["g_ke"].sum(0))
    bar("shared gains g_target_kd", kd.grad.cpu().numpy(), r32["g_kd"].sum(), r64["g_kd"].sum())
    assert ke.grad.shape == (nqd,) and kd.grad.shape == (1,)
    # the slot index is cached on the env, the table too
    assert ("jointslots", str(dev)) in env._contact_table and ("jointforce", str(dev)) in env._contact_table
