"""The scaffolding the GPU tests share: the device fixture, rollout inputs on the device, one forward + adjoint launch brought back as numpy,
device models and C oracles of a template, the stand-in host of ForwardWarp.apply.  Kept apart from helpers.py so that the CPU-only tests
import no GPU piece.  A test module shares the fixture by importing it: ``from gpu_harness import dev  # noqa: F401``."""
import numpy as np
import pytest
import torch

from diffphys_amd.hip_backend import ADJOINT_INPUTS as BWD, ROLLOUT_INPUTS as FWD  # noqa: F401
from diffphys_amd.synth import INPUT_NAMES

SEEDED = INPUT_NAMES + ("adj_pos", "adj_vel")   # the rollout inputs and the upstream gradients of the frames
_UNSET = object()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on a GPU box"
    return torch.device("cuda:0")


def dev_inputs(inp, dev, names=INPUT_NAMES):
    """numpy rollout inputs -> dict of contiguous float32 tensors on the device"""
    return {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.float32)).to(dev) for k in names}


def gpu_rollout(dm, inp, dev, backward=True, keep_traj=False):
    """rollout_forward and (backward=True) rollout_backward of the inputs, everything brought back as numpy"""
    bs = inp["q_init"].size // dm.nq
    T, f2s = inp["nsteps"], list(inp["frame2step"])
    t = dev_inputs(inp, dev, SEEDED)
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    out = dict(wp_pos=pos.cpu().numpy(), wp_vel=vel.cpu().numpy(), grf=grf.cpu().numpy(), jaf=jaf.cpu().numpy())
    if backward:
        g = dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, t["adj_pos"], t["adj_vel"])
        out["grads"] = {k: v.cpu().numpy() for k, v in g.items()}
    if keep_traj:  # the states, total wrenches and clamp masks the kernel saved for its adjoint, and the workspace they were read from
        bq, bqd, bf, mask = dm.saved_trajectory(ws, bs, T)
        out["traj"] = dict(states_q=bq.cpu().numpy(), states_qd=bqd.cpu().numpy(), states_f=bf.cpu().numpy(), clamp=mask.cpu().numpy())
        out["ws"] = ws
    return out


def same_bits(a, b, nan_equal=False):
    """Two tensors, or two results of gpu_rollout (frame outputs and every gradient), bit for bit.  nan_equal: a NaN equals a NaN."""
    if isinstance(a, dict):
        pairs = [(a[k], b[k]) for k in ("wp_pos", "wp_vel", "grf", "jaf")] + [(a["grads"][k], b["grads"][k]) for k in a["grads"]]
        return all(same_bits(x, y, nan_equal) for x, y in pairs)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=nan_equal)
    return torch.equal(a, b) or (nan_equal and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()))


def device_model(tpl, family=0, segw=None, literal=False):
    """A DeviceModel of the template at this segment width, kernel family and numeric policy"""
    from diffphys_amd import hip_backend

    dm = hip_backend.DeviceModel(tpl)
    if segw:
        dm.set_segment_width(segw)
    dm.set_kernel_family(family)
    if literal:
        dm.set_numeric_policy(hip_backend.NUM_LITERAL)
    return dm


def c_oracles(tpl, inp, dtype, twist_eval=False):
    """C oracle forward + adjoint of the inputs -> (states, gradients).  twist_eval: the kernels' scale-invariant evaluation of the twist
    and FIXED-joint angles (oracle/ref_c/diffphys_ref.c ref_set_twist_eval) in place of the literal one, the oracle's default."""
    from oracle.ref_c import RefC

    rc = RefC(tpl, dtype)
    rc.set_twist_eval(twist_eval)
    try:
        st = rc.rollout_forward(inp, inp["nsteps"], inp["frame2step"], inp["dt"])
        gr = rc.rollout_backward(st, inp["adj_pos"], inp["adj_vel"])
    finally:
        rc.set_twist_eval(False)
    return st, gr


class _Host:  # the attributes ForwardWarp reads from `self`
    pass


def warp_host(robot, bs, T, f2s, dt, dev, K=_UNSET):
    """The stand-in for the object ForwardWarp.apply is handed.  K: its ``checkpoint_steps``; not given, it has no such attribute."""
    from diffphys_amd import robots

    h = _Host()
    h.env = robots.env_from_template(robot, bs, device=dev)
    h.num_envs, h.steps_idx, h.frame2step, h.dt = bs, range(T), f2s, dt
    if K is not _UNSET:
        h.checkpoint_steps = K
    return h


def warp_grads(cls, names, t_in, h, ap, av, needs=None, absent=()):
    """cls.apply(*inputs, h) and backward of sum(pos * ap) + sum(vel * av) -> (pos, vel, .grad by input name).  The inputs are fresh
    leaves of t_in; those in ``needs`` (default: all) require a gradient, those in ``absent`` are passed as None."""
    x = {k: (None if k in absent else t_in[k].detach().clone().requires_grad_(needs is None or k in needs)) for k in names}
    pos, vel = cls.apply(*[x[k] for k in names], h)
    ((pos * ap).sum() + (vel * av).sum()).backward()
    torch.cuda.synchronize()
    return pos.detach(), vel.detach(), {k: (None if v is None else v.grad) for k, v in x.items()}
