"""The per-body ground-contact state op -- PD_POSE_CONTACT_STATE, k_contact_state_fwd / k_contact_state_vjp of
ppr-diffphys_amd/csrc/pd_pose.hip -- on a real MI355X (run with -m gpu): per body the height, world (x, z) and velocity of its lowest
contact candidate, the summed depth and the number of its touching candidates, and the gradient in the states.

Reference: tests/contact_state_ref.py (the definition over oracle/ref_torch.py's q_rot / cross) in float64 on the SAME fp32 inputs.
Bar (the project's, test_gpu_state_ops_generated.bar), per tensor: relmax(GPU, f64) <= max(4 x relmax(fp32 torch, f64), 1e-5), everything
finite, and the input-quality condition relmax(fp32 torch, f64) <= 1e-4 asserted; every comparison prints GPU / fp32 / bar.  The count
is compared EXACTLY.  Inputs: tests/contact_state_cases.py, whose conditions (no candidate within 1e-6 m of the ground, no two lowest
heights within 1e-5 m of each other -- shipped Laikago excepted, for point_xz, velocity and the VJP of at most 5 % of its elements) every
test asserts in float64 before it launches anything.  Shapes: the set counts of the ground-wrench tests (GW_SETS: element counts that
are no multiple of the four elements of a workgroup, many workgroups), 6 sets of the shipped robots."""
import functools

import numpy as np
import pytest
import torch

from gpu_harness import dev  # noqa: F401
from contact_state_cases import CASES, GENERATED_CASES, STRIDE_COUNTS, TIED, case, conditions, tie_case
from contact_state_ref import contact_state_of, field, input_conditions
from test_gpu_state_ops_generated import GW_SETS, bar, frozen, rows13

pytestmark = pytest.mark.gpu

TENSORS = ("height", "point_xz", "velocity", "depth")


@functools.lru_cache(maxsize=None)
def seed_of(name, kind):
    bq = case(name, kind)[1]
    g = np.random.RandomState(3).randn(bq.shape[0], bq.shape[1], 8).astype(np.float32)
    frozen(g)
    return g


@functools.lru_cache(maxsize=None)
def restated(name, kind, dtype):
    """(out, g_body_q, g_body_qd) of the restatement and its autograd in ``dtype`` with the g_out of seed_of: once, shared."""
    tpl, bq, bqd = case(name, kind)
    out = contact_state_of(tpl, dtype, bq.astype(np.float64), bqd.astype(np.float64), seed_of(name, kind).copy())
    frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def gpu_table(name, kind):
    from diffphys_amd import hip_backend

    return hip_backend.contact_table(case(name, kind)[0], device=torch.device("cuda:0"))


def run(name, kind, dev):
    """-> (out [S, nb, 8], g_state [S, nb, 13]) of the product, numpy; two calls of each must give the same bits."""
    from diffphys_amd import hip_backend

    tpl, bq, bqd = case(name, kind)
    S, nb = bq.shape[:2]
    table, state = gpu_table(name, kind), rows13(bq, bqd, dev)
    g_out = torch.tensor(seed_of(name, kind), device=dev).reshape(-1, 8)
    out, g_s = hip_backend.contact_state(table, nb, state), hip_backend.contact_state_vjp(table, nb, state, g_out)
    assert out.shape == (S * nb, 8) and g_s.shape == (S * nb, 13)
    assert torch.equal(out, hip_backend.contact_state(table, nb, state)) and torch.equal(g_s, hip_backend.contact_state_vjp(table, nb, state, g_out))
    return out.cpu().numpy().reshape(S, nb, 8), g_s.cpu().numpy().reshape(S, nb, 13)


def compare(tag, out, g_s, r32, r64, compared):
    """The bar per tensor.  height, depth and count on every element; point_xz, velocity and the VJP rows on ``compared`` (all elements,
    but for shipped Laikago's near-tied ones).  Bodies without candidates: (+inf, 0 ...) and a zero VJP row, exactly."""
    has = np.isfinite(r64[0][..., 0])
    assert has.any() and np.array_equal(np.isposinf(out[..., 0]), ~has)
    assert (out[~has][:, 1:] == 0).all() and (g_s[~has] == 0).all()
    assert np.array_equal(field(out, "count"), field(r64[0], "count")), tag + "count"
    assert np.array_equal(field(r32[0], "count"), field(r64[0], "count")), tag + "count: the fp32 yardstick disagrees: change the seed"
    for name in TENSORS:
        m = has if name in ("height", "depth") else has & compared
        bar(tag + name, field(out, name)[m], field(r32[0], name)[m], field(r64[0], name)[m])
    m = has & compared
    bar(tag + "g_body_q", g_s[..., :7][m], r32[1][m], r64[1][m])
    bar(tag + "g_body_qd", g_s[..., 7:][m], r32[2][m], r64[2][m])
    assert np.abs(r64[1]).max() > 0 and np.abs(r64[2]).max() > 0


def test_the_launch_shapes_are_the_ones_meant():
    """One wavefront per element, four per workgroup: the generated cases' element counts cross that boundary (some are no multiple
    of 4) and fill many workgroups."""
    n = {name: GW_SETS[name] * case(name, "tumbled")[1].shape[1] for name, _ in GENERATED_CASES}
    assert any(v % 4 for v in n.values()) and any(v % 4 == 0 for v in n.values()) and min(n.values()) >= 200
    assert case("laikago", "shipped")[1].shape[:2] == (6, 13) and case("human", "shipped")[1].shape[0] == 6


# ------------------------------------------------------------------------------------------------------------ 1. values and VJP
@pytest.mark.parametrize("name,kind", CASES)
def test_values_and_vjp(name, kind, dev):
    _, compared = conditions(name, kind)
    out, g_s = run(name, kind, dev)
    compare("%s %s " % (name, kind), out, g_s, restated(name, kind, torch.float32), restated(name, kind, torch.float64), compared)
    if kind == "tumbled":   # bodies in the air and bodies deep in the ground (free1 has one candidate)
        assert (field(out, "height") > 0).any() and (field(out, "count") > (1 if name != "free1" else 0)).any()


# -------------------------------------------------------------------------------------------------------------- 2. lane stride
@pytest.mark.parametrize("k", STRIDE_COUNTS)
def test_lane_stride_edges(k, dev):
    """One body of k candidates (k below, at and above one and two trips of the 64 lanes), one of three with contact_dist 0.02."""
    name = str(k)
    C, compared = conditions(name, "stride")
    out, g_s = run(name, "stride", dev)
    compare("k = %d " % k, out, g_s, restated(name, "stride", torch.float32), restated(name, "stride", torch.float64), compared)
    tpl, bq, _ = case(name, "stride")
    pts = np.asarray(tpl["contact_point"], np.float64)[:k]
    # the reported (x, z) is the float64 winner's and nobody else's: nearer to it than to any other candidate's
    q = torch.as_tensor(bq[:, 0, 3:].astype(np.float64))
    from oracle import ref_torch as rt

    for s in range(bq.shape[0]):
        world = rt.q_rot(q[s].expand(k, 4), torch.as_tensor(pts)).numpy()[:, [0, 2]] + bq[s, 0, [0, 2]].astype(np.float64)
        assert int(np.abs(world - field(out, "point_xz")[s, 0]).sum(1).argmin()) == C["winner"][s, 0]


def test_lane_stride_winners_on_both_sides_of_64():
    w = np.concatenate([input_conditions(*case(str(k), "stride"))["winner"][:, 0] for k in STRIDE_COUNTS])
    assert (w < 64).any() and (w >= 64).any()


# --------------------------------------------------------------------------------------------------------------- 3. exact ties
def test_exact_ties_go_to_the_lowest_index(dev):
    """Candidates 3, 67 and 70 of a 130-candidate body share the lowest height exactly (identity quaternions): lane 3 holds two of them
    (3 and 67: strict < keeps the first), lane 6 the third, and the butterfly must prefer the lower INDEX on equal heights.  The op
    reports candidate 3's (x, z) and velocity, and the VJP is candidate 3's: d / d w = rr_3 x g_u."""
    from diffphys_amd import hip_backend

    tpl, bq, bqd = tie_case()
    S = bq.shape[0]
    table, state = hip_backend.contact_table(tpl, device=dev), rows13(bq, bqd, dev)
    g_out = np.random.RandomState(5).randn(S, 2, 8).astype(np.float32)
    out = hip_backend.contact_state(table, 2, state).cpu().numpy().reshape(S, 2, 8)
    g_s = hip_backend.contact_state_vjp(table, 2, state, torch.from_numpy(g_out).to(dev).reshape(-1, 8)).cpu().numpy().reshape(S, 2, 13)
    r64 = contact_state_of(tpl, torch.float64, bq, bqd, g_out)
    r32 = contact_state_of(tpl, torch.float32, bq, bqd, g_out)
    compare("ties ", out, g_s, r32, r64, np.ones((S, 2), bool))
    pts = np.asarray(tpl["contact_point"], np.float64)
    com = np.asarray(tpl["body_com"], np.float64).reshape(-1, 3)[0]
    p, w, v = bq[:, 0, :3].astype(np.float64), bqd[:, 0, :3].astype(np.float64), bqd[:, 0, 3:].astype(np.float64)
    assert (field(out, "count")[:, 0] == 3).all()
    np.testing.assert_allclose(field(out, "depth")[:, 0], 3 * 0.003, rtol=1e-4)
    g_u = g_out[:, 0, 3:6].astype(np.float64)
    far = np.inf
    for c in TIED:
        rr = np.broadcast_to(pts[c] - com, (S, 3))   # identity quaternion, dist 0: rr = P - com
        e_xz = np.abs(field(out, "point_xz")[:, 0] - (p[:, [0, 2]] + pts[c, [0, 2]])).max()
        e_u = np.abs(field(out, "velocity")[:, 0] - (v + np.cross(w, rr))).max()
        e_w = np.abs(g_s[:, 0, 7:10] - np.cross(rr, g_u)).max()
        print("candidate %d: |xz| %.2e |u| %.2e |g_w| %.2e" % (c, e_xz, e_u, e_w))
        if c == TIED[0]:
            assert e_xz <= 1e-6 and e_u <= 1e-6 and e_w <= 1e-6
        else:
            far = min(far, e_xz, e_u, e_w)
    assert far > 1e-3
    # the p.x and p.z partials: (x, z) = (p.x + rp.x, p.z + rp.z) and nothing else depends on them
    assert np.array_equal(g_s[:, 0, 0], g_out[:, 0, 1]) and np.array_equal(g_s[:, 0, 2], g_out[:, 0, 2])
    assert np.abs(g_s[:, 0, [0, 2]] - r64[1][:, 0, [0, 2]]).max() <= 1e-6


# --------------------------------------------------------------------------------------------- 4. consistency with the ground wrench
@pytest.mark.parametrize("name", sorted(GW_SETS))
def test_count_is_the_ground_wrenchs_touch_decision(name, dev):
    from diffphys_amd import hip_backend

    conditions(name, "shallow")
    tpl, bq, bqd = case(name, "shallow")
    nb = bq.shape[1]
    table, state = gpu_table(name, "shallow"), rows13(bq, bqd, dev)
    count = hip_backend.contact_state(table, nb, state)[:, 7]
    wrench = hip_backend.ground_wrench(table, nb, state)
    touching = count > 0
    assert torch.equal(touching, wrench.abs().amax(1) > 0) and touching.any() and (nb == 1 or (~touching).any())


# --------------------------------------------------------------------------------------------------------------------- 5. edges
def test_edges(dev):
    """A body without candidates; a NaN row among good ones; n = 0; one element; n no multiple of 4."""
    from diffphys_amd import hip_backend

    conditions("mixed25", "tumbled")
    tpl, bq, bqd = case("mixed25", "tumbled")
    tpl = dict(tpl)
    nb = bq.shape[1]
    keep = np.asarray(tpl["contact_body"]).reshape(-1) != 2   # body 2 loses its candidates
    for k in ("contact_body", "contact_point", "contact_dist", "contact_material"):
        tpl[k] = np.asarray(tpl[k])[keep]
    table = hip_backend.contact_table(tpl, device=dev)
    state = rows13(bq, bqd, dev)
    n = state.shape[0]
    g_out = torch.randn(n, 8, generator=torch.Generator().manual_seed(1)).to(dev)
    out, g_s = hip_backend.contact_state(table, nb, state), hip_backend.contact_state_vjp(table, nb, state, g_out)
    none = torch.arange(n, device=dev) % nb == 2
    assert torch.isposinf(out[none, 0]).all() and (out[none, 1:] == 0).all() and (g_s[none] == 0).all()
    assert torch.isfinite(out[~none]).all() and torch.isfinite(g_s[~none]).all() and (g_s[~none].abs().amax(1) > 0).all()
    r64 = contact_state_of(tpl, torch.float64, bq, bqd)[0].reshape(n, 8)
    assert np.array_equal(out[:, 7].cpu().numpy(), r64[:, 7])
    # a NaN (an inf) in a row: every OTHER element keeps the bits of the launch without it
    for bad_value in (float("nan"), float("inf")):
        bad = state.clone()
        bad[5, 4], bad[n - 3, 1], bad[40, 9] = bad_value, bad_value, bad_value
        hit = torch.zeros(n, dtype=torch.bool, device=dev)
        hit[[5, n - 3, 40]] = True
        assert not none[hit].any()
        o2, g2 = hip_backend.contact_state(table, nb, bad), hip_backend.contact_state_vjp(table, nb, bad, g_out)
        assert torch.equal(o2[~hit], out[~hit]) and torch.equal(g2[~hit], g_s[~hit])
    # n = 0, one element, n no multiple of four: an element's bits do not depend on n or on its place in the launch
    empty = hip_backend.contact_state(table, nb, state[:0])
    assert empty.shape == (0, 8) and hip_backend.contact_state_vjp(table, nb, state[:0], g_out[:0]).shape == (0, 13)
    one = hip_backend.contact_table(case("free1", "shallow")[0], device=dev)
    s1 = rows13(*case("free1", "shallow")[1:], dev)
    all1 = hip_backend.contact_state(one, 1, s1)
    for lo, hi in ((0, 1), (7, 8), (3, 10), (1, 6)):
        assert torch.equal(hip_backend.contact_state(one, 1, s1[lo:hi].contiguous()), all1[lo:hi])
    assert n % 4 == 0 and (n - nb) % 4 != 0
    assert torch.equal(hip_backend.contact_state(table, nb, state[nb:].contiguous()), out[nb:])
    assert torch.equal(hip_backend.contact_state_vjp(table, nb, state[nb:].contiguous(), g_out[nb:].contiguous()), g_s[nb:])


# --------------------------------------------------------------------------------------------------------------- 6. capturable
def test_capturable_in_a_graph(dev):
    """no allocation, no synchronisation inside the entries: a captured forward + VJP replays the eager bits"""
    from diffphys_amd import hip_backend as hb

    conditions("cmp31", "shallow")
    tpl, bq, bqd = case("cmp31", "shallow")
    nb = bq.shape[1]
    table, state = gpu_table("cmp31", "shallow"), rows13(bq, bqd, dev)
    g_out = torch.tensor(seed_of("cmp31", "shallow"), device=dev).reshape(-1, 8)
    want = hb.contact_state(table, nb, state), hb.contact_state_vjp(table, nb, state, g_out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hb.contact_state(table, nb, state)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = hb.contact_state(table, nb, state), hb.contact_state_vjp(table, nb, state, g_out)
    torch.cuda.current_stream().wait_stream(side)
    got[0].zero_(); got[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ----------------------------------------------------------------------------------------- 7. dp_utils.contact_state, the two losses
class _Env:
    """what dp_utils.contact_state reads of a sim.Model, for a generated robot"""

    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


def _losses(cs, dp_utils, pair):
    return (dp_utils.penetration_loss(cs), dp_utils.skate_loss(cs, h0=0.02), dp_utils.penetration_loss(cs, bodies=pair),
            dp_utils.skate_loss(cs, h0=0.05, bodies=pair[::-1]))


@pytest.mark.parametrize("name,kind", [("human", "shipped"), ("mixed25", "tumbled")])
def test_dp_utils_contact_state_and_the_losses(name, kind, dev):
    """dp_utils.contact_state on (2, S / 2, nb, .) states of an env, the two losses on it (all bodies; the two bodies deepest in the
    ground) and their gradients in body_q and body_qd, against float64 autograd of the restatement through the SAME two loss
    functions, under the bar.  States lifted 1 m: the penetration term is 0 and so is its gradient."""
    from contact_state_ref import contact_state
    from diffphys_amd import dp_utils, robots
    from oracle import ref_torch

    conditions(name, kind)
    tpl, bq, bqd = case(name, kind)
    S, nb = bq.shape[:2]
    lead = (2, S // 2)
    env = robots.env_from_template(name, 1, device=dev) if kind == "shipped" else _Env(tpl)
    pair = [int(b) for b in np.argsort(field(restated(name, kind, torch.float64)[0], "depth").sum(0))[-2:]]
    q = torch.tensor(bq, device=dev).view(lead + (nb, 7)).requires_grad_(True)
    qd = torch.tensor(bqd, device=dev).view(lead + (nb, 6)).requires_grad_(True)
    cs = dp_utils.contact_state(q, qd, env)
    assert cs.height.shape == lead + (nb,) and cs.point_xz.shape == lead + (nb, 2) and cs.velocity.shape == lead + (nb, 3)
    assert cs.depth.shape == lead + (nb,) and cs.count.shape == lead + (nb,) and not cs.count.requires_grad and cs.depth.requires_grad
    wts = (10.0, 1.0, 3.0, 0.5)
    got = _losses(cs, dp_utils, pair)
    sum(w * l for w, l in zip(wts, got)).backward()

    def reference(dtype):
        T = ref_torch.Template(tpl, dtype)
        a = torch.tensor(bq.astype(np.float64), dtype=dtype).requires_grad_(True)
        b = torch.tensor(bqd.astype(np.float64), dtype=dtype).requires_grad_(True)
        o = contact_state(T, a, b).view(lead + (nb, 8))
        ls = _losses(dp_utils.ContactState(o[..., 0], o[..., 1:3], o[..., 3:6], o[..., 6], o[..., 7].detach()), dp_utils, pair)
        sum(w * l for w, l in zip(wts, ls)).backward()
        return [float(l.detach()) for l in ls], a.grad.numpy(), b.grad.numpy()

    r64, r32 = reference(torch.float64), reference(torch.float32)
    tag = "%s " % name
    assert all(v > 0 for v in r64[0]), r64[0]
    for k, what in enumerate(("penetration", "skate", "penetration of two bodies", "skate of two bodies, h0 = 0.05")):
        bar(tag + what, float(got[k].detach()), r32[0][k], r64[0][k])
    bar(tag + "d losses / d body_q", q.grad.cpu().numpy().reshape(S, nb, 7), r32[1], r64[1])
    bar(tag + "d losses / d body_qd", qd.grad.cpu().numpy().reshape(S, nb, 6), r32[2], r64[2])
    # lifted: nothing touches -- the penetration term is 0 and so is its gradient
    up = torch.tensor(bq, device=dev)
    up[..., 1] += 1.0 if kind == "shipped" else 100.0
    up.requires_grad_(True)
    qd2 = torch.tensor(bqd, device=dev).requires_grad_(True)
    lifted = dp_utils.contact_state(up, qd2, env)
    pen = dp_utils.penetration_loss(lifted)
    pen.backward()
    assert float(pen.detach()) == 0 and float(lifted.count.max()) == 0 and float(up.grad.abs().max()) == 0 and float(qd2.grad.abs().max()) == 0
    assert float(dp_utils.skate_loss(lifted).detach()) == 0


# ---------------------------------------------------------------------------------------------------------------- 8. phys_model
def _iterate(model, fs, noise):
    model.optimizer.zero_grad(set_to_none=True)
    out = model.forward(frame_start=fs, q_init_noise=noise.clone())
    model.backward(out["total_loss"])
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in out.items()}, grads


def test_phys_model_weights_zero_are_the_model_without_the_options(dev):
    from test_gpu_workload import _model

    fs = torch.arange(4, device=dev)
    noise = (torch.randn(4 * 19, generator=torch.Generator().manual_seed(3)) * 0.01).to(dev)
    runs = []
    for with_options in (False, True):
        model, opts = _model("mi-pace", "cs0")
        if with_options:
            assert opts["reg_pen_wt"] == 0.0 and opts["reg_skate_wt"] == 0.0
        else:
            del opts["reg_pen_wt"], opts["reg_skate_wt"]        # a model constructed without the options
        model.reinit_envs(4, frames_per_wdw=3)
        steps = []
        for _ in range(2):
            steps.append(_iterate(model, fs, noise))
            model.update()
        runs.append(steps)
    for (la, ga), (lb, gb) in zip(*runs):
        assert set(la) == set(lb) and "loss_reg_pen" not in lb and "loss_reg_skate" not in lb and set(ga) == set(gb)
        for k in la:
            assert torch.equal(la[k], lb[k]), k
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k


def test_phys_model_with_the_two_regularisers(dev):
    from test_gpu_workload import _model

    model, opts = _model("mi-pace", "cs")
    model.reinit_envs(4, frames_per_wdw=3)
    fs = torch.arange(4, device=dev)
    noise = (torch.randn(4 * 19, generator=torch.Generator().manual_seed(3)) * 0.01).to(dev)
    out0, g0 = _iterate(model, fs, noise)
    assert "loss_reg_pen" not in out0 and "loss_reg_skate" not in out0
    opts["reg_pen_wt"], opts["reg_skate_wt"] = 50.0, 0.5
    out, g = _iterate(model, fs, noise)
    pen, skate = float(out["loss_reg_pen"]), float(out["loss_reg_skate"])
    print("loss_reg_pen %.4e, loss_reg_skate %.4e, loss_traj %.4e" % (pen, skate, float(out["loss_traj"])))
    assert np.isfinite(pen) and pen > 0 and np.isfinite(skate) and skate > 0
    base = {k: float(v) for k, v in out.items()}
    assert abs(base["total_loss"] - sum(opts[k[5:] + "_wt"] * v for k, v in base.items() if k != "total_loss")) <= 1e-6 * abs(base["total_loss"])
    for k in out0:   # the other terms are what they were
        assert k == "total_loss" or torch.equal(out[k], out0[k]), k
    # the regularisers sit on the KINEMATIC states: their gradient reaches the kinematics networks
    assert set(g) == set(g0)
    moved = [k for k in g if not torch.equal(g[k], g0[k])]
    print("gradients that differ from the weight-0 run: %d of %d" % (len(moved), len(g)))
    assert moved and all(torch.isfinite(v).all() for v in g.values())
    assert any(k.startswith("root_pose_mlp") for k in moved) and any(k.startswith("vel_mlp") for k in moved), moved
    # one alone: only its key enters
    opts["reg_pen_wt"] = 0.0
    only, _ = _iterate(model, fs, noise)
    assert "loss_reg_pen" not in only and torch.equal(only["loss_reg_skate"], out["loss_reg_skate"])
    # query(contacts=True)
    nb = int(model.env.nb)
    data = model.query(contacts=True)
    sc = data["sim_contacts"]
    F = data["sim_poses"].shape[0]
    assert set(sc) == {"height", "point_xz", "velocity", "depth", "count"}
    assert sc["height"].shape == (F, nb) and sc["point_xz"].shape == (F, nb, 2) and sc["velocity"].shape == (F, nb, 3)
    assert sc["depth"].shape == (F, nb) and sc["count"].shape == (F, nb) and np.isfinite(sc["height"]).all()
    assert "sim_contacts" not in model.query()
    del model.sim_vels
    with pytest.raises(RuntimeError, match="contacts=True"):
        model.query(contacts=True)
