"""The 2D keypoint reprojection term on the GPU (run with -m gpu on an MI355X).

  1. project_bodies against the reference's OWN fp32 output (tests/golden/ref_host_small.npz, rtk/proj).
  2. Values and vector-Jacobian products of PD_POSE_PROJECT / PD_POSE_PROJECT_POINT through the C ABI against a float64 torch-autograd
     restatement written here (`_project`), element counts that straddle a wavefront, group sizes off the wave boundaries.
     Bars.  Values: max |d| / max(1, |x|) <= 1e-6 (the golden itself is 1.4e-7 from a float64 evaluation).  Gradients: error scaled by
     max |g| of the tensor; the yardstick is a PLAIN fp32 torch evaluation (CPU, autograd) of the same formula on the same inputs against
     float64, taken per op and tensor as the worst over the case set; the bar is 4 x that -- a one-lane kernel has no reason to be worse
     than any fp32 evaluation, the 4 leaves room for another order of the operations.  The yardstick is the worst over the SET and not
     each case's own figure: the error of one fp32 evaluation of a handful of elements is anywhere between 0 and a few ulp (the n = 1
     cases: 1e-8 .. 1.2e-7 for the same formula), so a per-case figure measures the draw, not the formula; over the set it settles at
     9e-8 .. 2.3e-7 (printed by the fixture), and every case, n = 1 included, is held to 4 x that.
  3. Bit-for-bit: a grouped camera = the expanded camera tensor; PROJECT_POINT with c = 0 = PROJECT.
  4. Refusals and edges of the C entries.
  5. differentiable_states of ForwardWarpTrajLoss / ForwardWarpTrajLossFK.
  6. ForwardWarp -> project_bodies -> reproj_loss against float64 (oracle.ref_torch.rollout, autograd), short horizon.
  7. phys_model with traj_2d_wt.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from gpu_harness import BWD, FWD, dev  # noqa: F401
from helpers import GOLDEN, INPUT_NAMES, relmax, tight_inputs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the restatement (any dtype, any device)
def _quat_to_mat(q):
    """q (..., 4) real-LAST, not normalised -> R (..., 3, 3), divided by |q|^2 (geom_utils.quaternion_to_matrix)"""
    i, j, k, r = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    return torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                        s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                        s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], -1).reshape(q.shape[:-1] + (3, 3))


def _project(cam, b):
    """cam [n, 16] (one row per element: expand a grouped camera first), b [n, 7] or [n, 10] -> [n, 2]:
    ((fx x + cx z) / z, (fy y + cy z) / z), (x, y, z) = R p + t, p the body origin or origin + R(q) c."""
    C = cam.reshape(-1, 4, 4)
    p = b[:, :3]
    if b.shape[1] == 10:
        p = p + (_quat_to_mat(b[:, 3:7]) @ b[:, 7:, None])[..., 0]
    v = (C[:, :3, :3] @ p[..., None])[..., 0] + C[:, :3, 3]
    return torch.stack([(C[:, 3, 0] * v[:, 0] + C[:, 3, 2] * v[:, 2]) / v[:, 2], (C[:, 3, 1] * v[:, 1] + C[:, 3, 3] * v[:, 2]) / v[:, 2]], -1)


def _expand(cam_rows, n, g):
    return cam_rows if g == 0 else cam_rows.repeat_interleave(g, 0)


def _cameras(rows, gen, z_lo, z_hi, reach):
    """rows x 16: a random rotation, a translation that keeps every point within `reach` of the origin at a depth in [z_lo, z_hi],
    intrinsics in normalised image units (focal 1 .. 2.5, principal point within +-0.3: pixels only scale both sides of a comparison)."""
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    q = torch.randn(rows, 4, generator=gen, dtype=torch.float64)
    cam = torch.zeros(rows, 4, 4, dtype=torch.float64)
    cam[:, :3, :3] = _quat_to_mat(q)
    cam[:, :2, 3] = u(rows, 2) - 0.5
    cam[:, 2, 3] = z_lo + reach + (z_hi - z_lo - 2 * reach) * u(rows)
    cam[:, 3, :2] = 1.0 + 1.5 * u(rows, 2)
    cam[:, 3, 2:] = 0.6 * u(rows, 2) - 0.3
    return cam.reshape(rows, 16).float()


CASES = [(op, n, g) for op in (3, 4) for n in (1, 63, 64, 65, 130) for g in sorted({0, 1, 5, 13, n}) if g == 0 or n % g == 0]


def _case_inputs(op, n, g):
    gen = torch.Generator().manual_seed(1000 * op + 10 * n + g)
    rows = n if g == 0 else n // g
    cam = _cameras(rows, gen, 1.0, 6.0, 0.9)     # camera z in [1, 6]: |p (+ R c)| <= 0.9
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    b = torch.zeros(n, 7 if op == 3 else 10, dtype=torch.float64)
    reach = 0.9 if op == 3 else 0.55
    b[:, :3] = (2 * u(n, 3) - 1) * reach / 3 ** 0.5
    q = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    b[:, 3:7] = q / q.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * u(n, 1))   # NOT unit: the conversion divides by |q|^2
    if op == 4:
        b[:, 7:] = (2 * u(n, 3) - 1) * 0.35 / 3 ** 0.5
    g_out = torch.randn(n, 2, generator=gen, dtype=torch.float64).float()
    return cam, b.float(), g_out


def _autograd(cam_rows, b, g_out, n, g, dtype):
    """values, d / d camera PER ELEMENT [n, 16], d / d b -- torch autograd in `dtype` on the CPU"""
    cam = _expand(cam_rows, n, g).to(dtype).requires_grad_(True)
    bb = b.to(dtype).requires_grad_(True)
    out = _project(cam, bb)
    out.backward(g_out.to(dtype))
    return out.detach(), cam.grad, bb.grad


def _val_err(a, ref):
    return float(((a.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


def _grad_err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope="module")
def references():
    """float64 references of every case, made once, and the fp32-torch yardstick of the gradient bars: worst over the case set, per op and tensor"""
    refs, yard = {}, {}
    for op, n, g in CASES:
        cam, b, g_out = _case_inputs(op, n, g)
        v64, ga64, gb64 = _autograd(cam, b, g_out, n, g, torch.float64)
        v32, ga32, gb32 = _autograd(cam, b, g_out, n, g, torch.float32)
        C = _expand(cam, n, g).double().reshape(-1, 4, 4)
        p = b.double()[:, :3] if op == 3 else b.double()[:, :3] + (_quat_to_mat(b.double()[:, 3:7]) @ b.double()[:, 7:, None])[..., 0]
        z = (C[:, 2, :3] * p).sum(-1) + C[:, 2, 3]
        assert 1.0 <= float(z.min()) and float(z.max()) <= 6.0, "camera z in [1, 6]"
        refs[op, n, g] = (cam, b, g_out, v64, ga64, gb64)
        for key, e in (("g_a", _grad_err(ga32, ga64)), ("g_b", _grad_err(gb32, gb64)), ("val", _val_err(v32, v64))):
            yard[op, key] = max(yard.get((op, key), 0.0), e)
    print("fp32 torch (CPU) vs float64 over the case set: " + ", ".join("op %d %s %.2e" % (k[0], k[1], v) for k, v in sorted(yard.items())))
    return refs, yard


def _raw(dev):
    from diffphys_amd import hip_backend as hb

    L = hb.lib()
    L.pd_last_error.restype = ctypes.c_char_p
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    stream = lambda: torch.cuda.current_stream().cuda_stream
    return L, ptr, stream


# ------------------------------------------------------------------------------------------------ 1. the reference's own output
def test_project_bodies_equals_the_references_output(dev):
    from diffphys_amd import dp_utils

    with np.load(os.path.join(GOLDEN, "ref_host_small.npz")) as z:
        bodies, rtk, proj = z["rtk/bodies"], z["rtk/rtk"], z["rtk/proj"]
    got = dp_utils.project_bodies(torch.from_numpy(bodies).to(dev), torch.from_numpy(rtk).to(dev))
    assert got.shape == proj.shape == bodies.shape[:-1] + (2,)
    err = _val_err(got.cpu(), torch.from_numpy(proj).double())
    print("project_bodies vs the reference's fp32 output: %.2e" % err)
    assert err <= 1e-6


# ------------------------------------------------------------------------------------------------ 2. values and VJP against float64
@pytest.mark.parametrize("op,n,g", CASES)
def test_values_and_vjp_against_float64(op, n, g, dev, references):
    from diffphys_amd import hip_backend as hb

    refs, yard = references
    cam, b, g_out, v64, ga64, gb64 = refs[op, n, g]
    assert float(v64.abs().max()) < 50 and bool(torch.isfinite(v64).all())
    L, ptr, stream = _raw(dev)
    nb = b.shape[1]
    cam_d, b_d, go_d = cam.to(dev), b.to(dev), g_out.to(dev)
    out = torch.full((n, 2), float("nan"), device=dev)
    g_a = torch.full((n, 16), float("nan"), device=dev)
    g_b = torch.full((n, nb), float("nan"), device=dev)
    assert L.pd_pose_op(op, n, ptr(cam_d), g, ptr(b_d), ptr(out), stream()) == 0, L.pd_last_error()
    assert L.pd_pose_op_vjp(op, n, ptr(cam_d), g, ptr(b_d), ptr(go_d), ptr(g_a), ptr(g_b), stream()) == 0, L.pd_last_error()
    e_v, e_a, e_b = _val_err(out.cpu(), v64), _grad_err(g_a.cpu(), ga64), _grad_err(g_b.cpu(), gb64)
    print("op %d n %3d g %3d: values %.2e (bar 1e-6), g_a %.2e (bar %.2e), g_b %.2e (bar %.2e)" % (
        op, n, g, e_v, e_a, 4 * yard[op, "g_a"], e_b, 4 * yard[op, "g_b"]))
    assert e_v <= 1e-6
    assert e_a <= 4 * yard[op, "g_a"] and e_b <= 4 * yard[op, "g_b"]
    if op == 3:
        assert float(g_b[:, 3:].abs().max()) == 0, "only p is read: the quaternion entries of g_b are 0"
    # either gradient alone: the same bits, the other pointer NULL
    only_a, only_b = torch.empty_like(g_a), torch.empty_like(g_b)
    assert L.pd_pose_op_vjp(op, n, ptr(cam_d), g, ptr(b_d), ptr(go_d), ptr(only_a), None, stream()) == 0
    assert L.pd_pose_op_vjp(op, n, ptr(cam_d), g, ptr(b_d), ptr(go_d), None, ptr(only_b), stream()) == 0
    assert torch.equal(only_a, g_a) and torch.equal(only_b, g_b)
    # the binding: shapes in, the camera gradient summed over each group
    shaped = b_d if g == 0 else b_d.view(n // g, g, nb)
    assert torch.equal(hb.pose_op(op, cam_d, shaped).reshape(n, 2), out)
    s_a, s_b = hb.pose_op_vjp(op, cam_d, shaped, go_d.view(shaped.shape[:-1] + (2,)))
    assert torch.equal(s_b.reshape(n, nb), g_b) and s_a.shape == cam_d.shape
    if g > 1:   # the per-element rows added up in fp32: within the bound of a k-term fp32 sum in any order, (k - 1) 2^-24 sum |x|
        rows = g_a.double().view(n // g, g, 16)
        assert bool(((s_a.double() - rows.sum(1)).abs() <= (g - 1) * 2.0 ** -24 * rows.abs().sum(1) + 1e-30).all())
    else:
        assert torch.equal(s_a, g_a)


# ------------------------------------------------------------------------------------------------ 3. bit for bit
@pytest.mark.parametrize("op", [3, 4])
def test_group_broadcast_equals_the_expanded_camera(op, dev):
    from diffphys_amd import hip_backend as hb

    n, g = 130, 13
    cam, b, g_out = (t.to(dev) for t in _case_inputs(op, n, g))
    full = cam.repeat_interleave(g, 0).contiguous()
    grouped = b.view(n // g, g, -1)
    assert torch.equal(hb.pose_op(op, cam, grouped).reshape(n, 2), hb.pose_op(op, full, b))
    ga1, gb1 = hb.pose_op_vjp(op, cam, grouped, g_out.view(n // g, g, 2))
    ga2, gb2 = hb.pose_op_vjp(op, full, b, g_out)
    assert torch.equal(gb1.reshape(n, -1), gb2)
    assert ga1.shape == cam.shape and ga2.shape == full.shape
    # one camera for all (g = n) as (16,) and as (4, 4)
    one = cam[:1]
    o1, o2 = hb.pose_op(op, one.reshape(16), b), hb.pose_op(op, one.reshape(4, 4), b)
    assert torch.equal(o1, o2) and torch.equal(o1, hb.pose_op(op, one.expand(n, 16).contiguous(), b))


def test_project_point_at_the_origin_equals_project(dev):
    from diffphys_amd import hip_backend as hb

    n, g = 65, 5
    cam, b, g_out = (t.to(dev) for t in _case_inputs(3, n, g))
    b10 = torch.cat([b, torch.zeros(n, 3, device=dev)], 1).contiguous()
    b3, b4 = b.view(n // g, g, 7), b10.view(n // g, g, 10)
    assert torch.equal(hb.pose_op(4, cam, b4), hb.pose_op(3, cam, b3))
    ga3, gb3 = hb.pose_op_vjp(3, cam, b3, g_out.view(n // g, g, 2))
    ga4, gb4 = hb.pose_op_vjp(4, cam, b4, g_out.view(n // g, g, 2))
    assert torch.equal(gb4[..., :3], gb3[..., :3]) and torch.equal(ga4, ga3)


def test_project_points_picks_bodies_and_differentiates_every_operand(dev):
    from diffphys_amd import dp_utils

    gen = torch.Generator().manual_seed(5)
    cam = _cameras(6, gen, 2.0, 5.0, 0.9).view(2, 3, 4, 4)
    bodies = torch.zeros(2, 3, 5, 7, dtype=torch.float64)
    bodies[..., :3] = (torch.rand(2, 3, 5, 3, generator=gen, dtype=torch.float64) - 0.5) * 0.6
    bodies[..., 3:] = torch.randn(2, 3, 5, 4, generator=gen, dtype=torch.float64)
    idx = torch.tensor([4, 0, 4, 2])
    pts = (torch.rand(4, 3, generator=gen, dtype=torch.float64) - 0.5) * 0.4
    w = torch.randn(2, 3, 4, 2, generator=gen, dtype=torch.float64)

    def run(dtype, device, fn):
        leaves = [t.detach().clone().to(dtype).to(device).requires_grad_(True) for t in (bodies, cam, pts)]
        out = fn(*leaves)
        (out * w.to(dtype).to(device)).sum().backward()
        return out.detach().cpu(), [t.grad.cpu() for t in leaves]

    def restated(bod, rtk, p):
        sel = bod[..., idx, :]
        b10 = torch.cat([sel, p.expand(2, 3, 4, 3)], -1).reshape(-1, 10)
        return _project(rtk.reshape(6, 16).repeat_interleave(4, 0), b10).view(2, 3, 4, 2)

    v64, g64 = run(torch.float64, "cpu", restated)
    v32, g32 = run(torch.float32, "cpu", restated)
    v, g = run(torch.float32, dev, lambda bod, rtk, p: dp_utils.project_points(bod, rtk, idx.to(dev), p))
    assert _val_err(v, v64) <= 1e-6
    for a, r32, r64 in zip(g, g32, g64):
        assert a.shape == r64.shape and _grad_err(a, r64) <= max(4 * _grad_err(r32, r64), 1e-6)


# ------------------------------------------------------------------------------------------------ 4. refusals and edges
def test_refusals_and_edges(dev):
    from diffphys_amd import hip_backend as hb

    L, ptr, stream = _raw(dev)
    cam, b, g_out = (t.to(dev) for t in _case_inputs(4, 65, 5))
    for op in (3, 4):
        nb = 7 if op == 3 else 10
        bb = b[:, :nb].contiguous()
        # n = 0 is legal, with or without pointers
        assert L.pd_pose_op(op, 0, None, 0, None, None, stream()) == 0
        assert L.pd_pose_op_vjp(op, 0, None, 5, None, None, None, None, stream()) == 0
        assert hb.pose_op(op, cam[:0].view(0, 4, 4), bb[:0].view(0, 5, nb)).shape == (0, 5, 2)
        # ... and through the binding whichever dimension is the empty one: cameras that serve no element get a zero gradient
        for c, e in ((cam[0].view(4, 4), bb[:0]), (cam[:3].view(3, 4, 4), bb[:0].view(3, 0, nb)), (cam[:0], bb[:0])):
            assert hb.pose_op(op, c, e).shape == e.shape[:-1] + (2,)
            e_a, e_b = hb.pose_op_vjp(op, c, e, torch.empty(e.shape[:-1] + (2,), device=dev))
            assert e_a.shape == c.shape and float(e_a.abs().sum()) == 0 and e_b.shape == e.shape
        # n % g != 0: refused with a message, nothing written
        out = torch.full((65, 2), 7.5, device=dev)
        g_a, g_b = torch.full((65, 16), 7.5, device=dev), torch.full((65, nb), 7.5, device=dev)
        for bad_g in (4, 64, 66, -1):
            assert L.pd_pose_op(op, 65, ptr(cam), bad_g, ptr(bb), ptr(out), stream()) != 0
            assert b"n % g" in L.pd_last_error()
            assert L.pd_pose_op_vjp(op, 65, ptr(cam), bad_g, ptr(bb), ptr(g_out), ptr(g_a), ptr(g_b), stream()) != 0
            assert b"n % g" in L.pd_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.5).all()) and bool((g_a == 7.5).all()) and bool((g_b == 7.5).all())
        assert L.pd_pose_op_vjp(op, 65, ptr(cam), 5, ptr(bb), ptr(g_out), None, None, stream()) != 0   # nothing asked for
    out = torch.full((65, 2), 7.5, device=dev)
    for op in (5, 6, -1):
        assert L.pd_pose_op(op, 65, ptr(cam), 0, ptr(b), ptr(out), stream()) != 0
        assert L.pd_pose_op_vjp(op, 65, ptr(cam), 0, ptr(b), ptr(g_out), ptr(out), None, stream()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())
    # a point in the camera plane: inf / NaN as in the reference, no clamp
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 2, 2, 0.5, 0.5], device=dev)
    p = torch.tensor([[1.0, 0, 0, 0, 0, 0, 1], [0.0, 0, 0, 0, 0, 0, 1]], device=dev)
    o = hb.pose_op(3, eye, p)
    assert bool(torch.isinf(o[0, 0])) and bool(torch.isnan(o[1]).all())


def test_capturable_in_a_graph(dev):
    """no allocation, no synchronisation inside the entries: a captured forward + VJP replays the eager bits"""
    from diffphys_amd import hip_backend as hb

    cam, b, g_out = (t.to(dev) for t in _case_inputs(4, 130, 13))
    grouped, go = b.view(10, 13, 10), g_out.view(10, 13, 2)
    want = hb.pose_op(4, cam, grouped), hb.pose_op_vjp(4, cam, grouped, go, need_a=False)[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hb.pose_op(4, cam, grouped)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = hb.pose_op(4, cam, grouped), hb.pose_op_vjp(4, cam, grouped, go, need_a=False)[1]
    torch.cuda.current_stream().wait_stream(side)
    got[0].zero_(); got[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 5. the fused Functions
@pytest.fixture(scope="module")
def fused_setup(dev):
    from diffphys_amd import dp_model, robots, synth

    name, bs, T, f2s = "laikago", 6, 12, [0, 6, 12]
    tpl = robots.load_template(name)
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=7, steps_per_frame=6, penetration=0.002)
    F, nb, nq, nqd = len(f2s), int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])

    class Host:
        pass

    def host(**kw):
        h = Host()
        h.env = robots.env_from_template(name, bs, device=dev)
        h.num_envs, h.steps_idx, h.frame2step, h.dt = bs, range(T), f2s, inp["dt"]
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    t = {k: torch.from_numpy(inp[k]).to(dev).requires_grad_(True) for k in INPUT_NAMES}
    with torch.no_grad():
        pos0, _ = dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], host())
    g = torch.Generator().manual_seed(21)
    rn = lambda *s: torch.randn(*s, generator=g)
    tgt = (pos0.reshape(F, bs, nb, 7).permute(1, 0, 2, 3) + (rn(bs, F, nb, 7) * 0.02).to(dev)).contiguous()
    outseq = torch.zeros(bs, F, dtype=torch.bool, device=dev)
    outseq[4, 2:] = True
    q0 = torch.from_numpy(inp["q_init"]).view(bs, nq)
    qq = (q0[None] + 0.1 * rn(F, bs, nq)).to(dev).requires_grad_(True)
    qqd = (0.5 * rn(F, bs, nqd)).to(dev).requires_grad_(True)
    c1, c2 = (rn(F, bs * nb, 7) * 0.3).to(dev), (rn(F, bs * nb, 6) * 0.1).to(dev)
    w_q, w_qd = rn(bs, F, nb, 7).to(dev), rn(bs, F, nb, 6).to(dev)
    return dict(name=name, bs=bs, T=T, f2s=f2s, inp=inp, host=host, t=t, tgt=tgt, outseq=outseq, qq=qq, qqd=qqd, c1=c1, c2=c2, w_q=w_q, w_qd=w_qd,
                F=F, nb=nb)


WT = 0.37


def _run_fused(S, fk, h, terms):
    """loss * WT (+ the FK consumers) + terms(pos, vel) through the fused Function -> (loss, pos, vel, gradients by name)"""
    from diffphys_amd import dp_model

    t = S["t"]
    args = [t[k] for k in INPUT_NAMES]
    leaves = dict(t)
    if fk:
        leaves.update(queried_q=S["qq"], queried_qd=S["qqd"])
        loss, pos, vel, qp, qv, _ = dp_model.ForwardWarpTrajLossFK.apply(*args, S["tgt"], S["outseq"], S["qq"], S["qqd"], h)
        total = loss * WT + (qp * S["w_q"]).sum() + (qv * S["w_qd"]).sum()
    else:
        loss, pos, vel = dp_model.ForwardWarpTrajLoss.apply(*args, S["tgt"], S["outseq"], h)
        total = loss * WT
    extra = terms(pos, vel)
    if extra is not None:
        total = total + extra
    for x in leaves.values():
        x.grad = None
    total.backward()
    grads = {k: (None if x.grad is None else x.grad.detach().clone()) for k, x in leaves.items()}
    for x in leaves.values():
        x.grad = None
    return loss.detach().clone(), pos, vel, grads


def _direct(S, fk, adj_pos, adj_vel):
    """the library call the Function's backward must be: dm.rollout_backward_traj_loss(..., adj_pos=, adj_vel=) on a forward of the same inputs"""
    from diffphys_amd import hip_backend

    h = S["host"]()
    dm = hip_backend.device_model(h.env)
    c = lambda x: x.detach().to(torch.float32).contiguous()
    t = S["t"]
    fkin = (c(S["qq"]), c(S["qqd"])) if fk else None
    out = dm.rollout_forward_traj_loss(S["bs"], S["T"], S["inp"]["dt"], *[c(t[k]) for k in FWD], frame2step=S["f2s"], target_pos=c(S["tgt"]),
                                       outseq=S["outseq"], fk=fkin)
    gl = torch.full((1,), WT, device=S["tgt"].device)
    fkb = (fkin[0], fkin[1], S["w_q"].contiguous(), S["w_qd"].contiguous()) if fk else None
    return dm.rollout_backward_traj_loss(S["bs"], S["T"], S["inp"]["dt"], *[c(t[k]) for k in BWD], S["f2s"], out[4], out[5], gl,
                                         adj_pos=adj_pos, adj_vel=adj_vel, fk=fkb)


def _same(grads, g):
    n = 0
    for k, v in g.items():
        k = {"fk_joint_q": "queried_q", "fk_joint_qd": "queried_qd"}.get(k, k)
        if k in grads:
            assert grads[k] is not None and torch.equal(grads[k].reshape(v.shape), v), (k, float((grads[k].reshape(v.shape) - v).abs().max()))
            n += 1
    return n


@pytest.mark.parametrize("fk", [False, True], ids=["ForwardWarpTrajLoss", "ForwardWarpTrajLossFK"])
def test_differentiable_states_of_the_fused_functions(fk, dev, fused_setup):
    from diffphys_amd import dp_model, dp_utils

    S = fused_setup
    c1, c2 = S["c1"], S["c2"]
    both = lambda pos, vel: (pos * c1).sum() + (vel * c2).sum()
    # (a) without the attribute (and with it False): detached outputs, a term on them changes nothing
    loss0, pos0, vel0, base = _run_fused(S, fk, S["host"](), lambda pos, vel: None)
    for h in (S["host"](), S["host"](differentiable_states=False)):
        loss, pos, vel, grads = _run_fused(S, fk, h, both)
        assert not pos.requires_grad and not vel.requires_grad
        assert torch.equal(loss, loss0) and torch.equal(pos, pos0) and torch.equal(vel, vel0)
        assert set(grads) == set(base)
        for k in base:
            assert (grads[k] is None) == (base[k] is None) and (base[k] is None or torch.equal(grads[k], base[k])), k
    # (b) with it: the gradients of the library call with adj_pos / adj_vel, bit for bit
    on = lambda: S["host"](differentiable_states=True)
    loss, pos, vel, grads = _run_fused(S, fk, on(), both)
    assert pos.requires_grad and vel.requires_grad and torch.equal(loss, loss0) and torch.equal(pos, pos0) and torch.equal(vel, vel0)
    assert _same(grads, _direct(S, fk, c1, c2)) >= (12 if fk else 10)
    assert any(not torch.equal(grads[k], base[k]) for k in ("q_init", "qd_init", "refs")), "the term must reach the rollout's inputs"
    _, _, _, only1 = _run_fused(S, fk, on(), lambda pos, vel: (pos * c1).sum())
    assert _same(only1, _direct(S, fk, c1, torch.zeros_like(c2))) >= 10
    _, _, _, only2 = _run_fused(S, fk, on(), lambda pos, vel: (vel * c2).sum())
    assert _same(only2, _direct(S, fk, torch.zeros_like(c1), c2)) >= 10
    # ... and with no term on them it is the call it was
    _, _, _, none = _run_fused(S, fk, on(), lambda pos, vel: None)
    for k in base:
        assert base[k] is None or torch.equal(none[k], base[k]), k
    # (c) against the unfused composition: ForwardWarp -> se3_loss -> reduce_loss(clip=True), plus the same terms
    t = S["t"]
    F, bs, nb = S["F"], S["bs"], S["nb"]
    pos_u, vel_u = dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], S["host"]())
    lt = dp_utils.se3_loss(pos_u.reshape(F, bs, nb, 7).permute(1, 0, 2, 3), S["tgt"]).mean(-1)
    lt = torch.where(S["outseq"], torch.zeros_like(lt), lt)
    loss_u = dp_utils.reduce_loss(lt, clip=True)
    (loss_u * WT + both(pos_u, vel_u)).backward()
    assert abs(float(loss) - float(loss_u)) <= 1e-6 * abs(float(loss_u))
    for k in INPUT_NAMES:
        if t[k].grad is None:
            assert grads[k] is None or float(grads[k].abs().max()) == 0, k
            continue
        a, b = grads[k], t[k].grad
        sc = float(b.abs().max())
        print("   %-18s fused + states vs unfused: %.1e of the tensor's max" % (k, float((a - b).abs().max()) / (sc + 1e-30)))
        assert float((a - b).abs().max()) <= 7e-5 * sc + 1e-30, (k, float((a - b).abs().max()), sc)
        t[k].grad = None


# ------------------------------------------------------------------------------------------------ 6. end to end against float64
@pytest.mark.parametrize("T", [1, 3])
def test_rollout_projection_loss_against_float64(T, dev):
    """ForwardWarp -> project_bodies -> reproj_loss -> backward against oracle.ref_torch.rollout (float64, autograd) -> `_project` in
    float64 -> reproj_loss -> backward: q_init, qd_init, refs, target_ke.  Input recipe (tight_inputs: frames at states 0 and T), error
    measure (relmax) and the gradient cap (CAPS) are those of tests/test_gpu_tight.py::test_short_horizon_tight."""
    from diffphys_amd import dp_model, dp_utils, robots
    from oracle import ref_torch as rt
    from test_gpu_tight import CAPS

    name, bs = "laikago", 48
    tpl = robots.load_template(name)
    inp = tight_inputs(tpl, name, bs, T, seed=11 + T)
    f2s, F, nb = inp["frame2step"], 2, int(tpl["nb"])
    gen = torch.Generator().manual_seed(40 + T)
    rtk = _cameras(bs * F, gen, 2.0, 5.0, 1.2).view(bs, F, 4, 4)
    noise = torch.randn(bs, F, nb, 3, generator=gen, dtype=torch.float64) * 0.05

    def loss_of(pos, rtk_, project):  # pos [bs, F, nb, 7]
        tgt = pos.detach().clone()
        tgt[..., :3] += noise.to(tgt)
        return dp_utils.reproj_loss(project(pos, rtk_), project(tgt, rtk_), rtk_).mean()

    # float64
    T64 = rt.Template(tpl, torch.float64)
    t64 = {k: torch.tensor(inp[k], dtype=torch.float64, requires_grad=True) for k in INPUT_NAMES}
    allq, _ = rt.rollout(T64, *[t64[k] for k in INPUT_NAMES], nsteps=T, frame2step=f2s, dt=inp["dt"], return_all=True)
    pos64 = allq.reshape(T + 1, bs, nb, 7)[f2s].permute(1, 0, 2, 3)
    p64 = lambda pos, r: _project(r.reshape(-1, 16).repeat_interleave(nb, 0), pos.reshape(-1, 7)).view(bs, F, nb, 2)
    z = (rtk.double()[:, :, None, 2, :3] * pos64.detach()[..., :3]).sum(-1) + rtk.double()[:, :, None, 2, 3]
    assert float(z.min()) > 1.0, "every body in front of its camera"
    l64 = loss_of(pos64, rtk.double(), p64)
    l64.backward()
    # product
    class Host:
        pass

    h = Host()
    h.env = robots.env_from_template(name, bs, device=dev)
    h.num_envs, h.steps_idx, h.frame2step, h.dt = bs, range(T), f2s, inp["dt"]
    t = {k: torch.from_numpy(inp[k]).to(dev).requires_grad_(True) for k in INPUT_NAMES}
    pos, _ = dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], h)
    l32 = loss_of(pos.reshape(F, bs, nb, 7).permute(1, 0, 2, 3), rtk.to(dev), dp_utils.project_bodies)
    l32.backward()
    cap_p, _, _, cap_g = CAPS[name]
    l32, l64 = l32.detach(), l64.detach()
    print("T %d: loss %.6e (float64 %.6e)" % (T, float(l32), float(l64)))
    assert relmax(pos.detach().cpu().numpy().reshape(F, bs, nb, 7).transpose(1, 0, 2, 3), pos64.detach().numpy()) <= cap_p
    assert abs(float(l32) - float(l64)) <= cap_g * abs(float(l64))
    for k in ("q_init", "qd_init", "refs", "target_ke"):
        ref = t64[k].grad.numpy()
        e = relmax(t[k].grad.cpu().numpy().reshape(ref.shape), ref)
        print("   grad %-10s %.2e of the tensor's max (cap %.1e), max |g| %.2e" % (k, e, cap_g, np.abs(ref).max()))
        assert np.isfinite(e) and e <= cap_g, k
    assert np.abs(t64["q_init"].grad.numpy()).max() > 0 and np.abs(t64["qd_init"].grad.numpy()).max() > 0


# ------------------------------------------------------------------------------------------------ 7. phys_model
def _synthetic_cameras(model, seed=3):
    gen = torch.Generator().manual_seed(seed)
    n = model.total_frames
    cam = _cameras(n, gen, 2.0, 5.0, 1.4).view(n, 4, 4)
    cam[:, :3, :3] = torch.eye(3)     # looking down the world's -z ... +z axis at the robot, which walks within ~1.4 m of the origin
    cam[:, 2, 3] = torch.linspace(3.3, 3.7, n)
    return cam


def _iterate(model, fs, noise, weight_alone=None):
    model.optimizer.zero_grad(set_to_none=True)
    out = model.forward(frame_start=fs, q_init_noise=noise.clone())
    model.backward(out["total_loss"] if weight_alone is None else weight_alone * out["loss_traj_2d"])
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in out.items()}, grads


def test_phys_model_weight_zero_is_the_model_without_the_option(dev):
    from test_gpu_workload import _model

    fs = torch.arange(4, device=dev)
    noise = (torch.randn(4 * 19, generator=torch.Generator().manual_seed(3)) * 0.01).to(dev)
    runs = []
    for with_option in (False, True):
        model, opts = _model("mi-pace", "r2d0")
        if with_option:
            assert opts["traj_2d_wt"] == 0.0
            model.set_cameras(_synthetic_cameras(model))
        else:
            del opts["traj_2d_wt"]        # a model constructed without the option
        model.reinit_envs(4, frames_per_wdw=3)
        steps = []
        for _ in range(2):
            steps.append(_iterate(model, fs, noise))
            model.update()
        assert not hasattr(model, "differentiable_states")
        runs.append(steps)
    for (la, ga), (lb, gb) in zip(*runs):
        assert set(la) == set(lb) and "loss_traj_2d" not in lb and set(ga) == set(gb)
        for k in la:
            assert torch.equal(la[k], lb[k]), k
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k


def test_phys_model_with_the_2d_term(dev, monkeypatch):
    from diffphys_amd import phys_model as pm
    from test_gpu_workload import _model

    model, opts = _model("mi-pace", "r2d")
    model.reinit_envs(4, frames_per_wdw=3)
    fs = torch.arange(4, device=dev)
    noise = (torch.randn(4 * 19, generator=torch.Generator().manual_seed(3)) * 0.01).to(dev)
    opts["traj_2d_wt"] = 0.5
    with pytest.raises(RuntimeError, match="set_cameras"):
        model.forward(frame_start=fs, q_init_noise=noise.clone())
    with pytest.raises(ValueError):
        model.set_cameras(torch.zeros(model.total_frames + 1, 4, 4))
    model.set_cameras(_synthetic_cameras(model))
    out, _ = _iterate(model, fs, noise)
    assert model.differentiable_states is True
    l2d = float(out["loss_traj_2d"])
    print("loss_traj_2d %.4e, loss_traj %.4e" % (l2d, float(out["loss_traj"])))
    assert np.isfinite(l2d) and l2d > 0
    base = {k: float(v) for k, v in out.items()}
    assert abs(base["total_loss"] - sum(opts[k[5:] + "_wt"] * v for k, v in base.items() if k != "total_loss")) <= 1e-6 * abs(base["total_loss"])
    # the gradient of the weighted term alone: fused Function with differentiable states against the unfused ForwardWarp
    _, g_fused = _iterate(model, fs, noise, weight_alone=0.5)
    model.fuse_traj_loss = False
    out_u, g_unfused = _iterate(model, fs, noise, weight_alone=0.5)
    model.fuse_traj_loss = True
    assert abs(float(out_u["loss_traj_2d"]) - l2d) <= 1e-6 * l2d
    assert set(g_fused) == set(g_unfused) and any(float(g.abs().max()) > 0 for g in g_unfused.values())
    for k, b in g_unfused.items():
        sc = float(b.abs().max())
        assert float((g_fused[k] - b).abs().max()) <= 7e-5 * sc + 1e-30, (k, float((g_fused[k] - b).abs().max()), sc)
    # the simulated poses replaced by the targets: the term is 0
    real = pm.ForwardWarpTrajLossFK

    class Stub:
        @staticmethod
        def apply(*a):
            o = list(real.apply(*a))
            tgt = a[11]                                    # [n, F, nb, 7] -> the rollout's [F, n * nb, 7]
            o[1] = tgt.detach().permute(1, 0, 2, 3).reshape(o[1].shape).contiguous()
            return tuple(o)

    monkeypatch.setattr(pm, "ForwardWarpTrajLossFK", Stub)
    with torch.no_grad():
        z = model.forward(frame_start=fs, q_init_noise=noise.clone())
    monkeypatch.undo()
    assert abs(float(z["loss_traj_2d"])) <= 1e-6
    # observed keypoints given explicitly take the place of the projected targets
    model.set_cameras(_synthetic_cameras(model), torch.zeros(model.total_frames, model.n_links, 2))
    with torch.no_grad():
        given = model.forward(frame_start=fs, q_init_noise=noise.clone())
    assert np.isfinite(float(given["loss_traj_2d"])) and float(given["loss_traj_2d"]) > 10 * l2d
    # weight back to 0: the opt-in goes with it
    opts["traj_2d_wt"] = 0.0
    out0, _ = _iterate(model, fs, noise)
    assert "loss_traj_2d" not in out0 and not hasattr(model, "differentiable_states")
    # ... but an opt-in of the user's own (a term of theirs on the states) outlives the 2D term's coming and going
    model.differentiable_states = True
    for wt in (0.5, 0.0):
        opts["traj_2d_wt"] = wt
        with torch.no_grad():
            model.forward(frame_start=fs, q_init_noise=noise.clone())
        assert model.differentiable_states is True
    del model.differentiable_states
